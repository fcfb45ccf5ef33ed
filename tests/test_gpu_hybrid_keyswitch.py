"""GPU tests of the hybrid key switch (include/moai_hip.h, "hybrid key switching": moai_hybrid_digits, moai_hybrid_keygen,
moai_switch_key_hybrid, moai_relinearize_hybrid, moai_apply_galois_hybrid).

1. alpha = 1 is the existing path: bit for bit moai_switch_key / moai_relinearize / moai_apply_galois / moai_kswitch_keygen, on
   the small transform (logn 10) and the tiled one with mixed arithmetic modes (logn 12).
2. alpha > 1 is bit for bit the integer restatement tests/hybrid_ref.py (itself pinned to the oracle at alpha = 1 by
   tests/test_hybrid_ref_cpu.py): full digits, a one-prime last digit, one digit of one prime; random operands, rows of m - 1, zero.
   Digits of 6 and 12 primes once each: the conversion kernel's wider instantiations.
3. It is a key switch: with keys from moai_hybrid_keygen, d0 + d1 s - c s' holds the same small integer in every row, within the
   header's bound B; once at N = 2^16 with MOAI's 35 data primes and 12 special primes.
4. Chunking under a scratch budget of two ciphertexts does not change the result.
5. Every refusal is MOAI_EINVAL and leaves the outputs alone.

Shapes are the smallest at which each branch can go wrong; the restatement is computed once per shape."""
import numpy as np
import pytest

import hybrid_ref as HR
import oracle as O
from hybrid_kit import EINVAL, FILL, MOAI_DATA_BITS, Env, traced, tuned
from hybrid_kit import env_small1, env_small2, env_tiled1, env_tiled3  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

KEY = bytes(range(1, 33))


# ---- 1. alpha = 1 is the existing path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small", "tiled"])
@pytest.mark.parametrize("level", ["top", "one"])
def test_alpha_1_equals_the_existing_entry_points(moai, env_small1, env_tiled1, which, level):
    e = env_small1 if which == "small" else env_tiled1
    L, B, n = (e.lmax if level == "top" else 1), 3, e.n
    rng = np.random.default_rng(e.logn * 10 + L)
    dkey = e.up(e.random_key(rng))
    ct = O.uniform_rns(rng, e.primes[:L], (B, 2), n)
    target = O.uniform_rns(rng, e.primes[:L], (B,), n)
    target[1], target[2] = e.edge_targets(L)
    ct3 = O.uniform_rns(rng, e.primes[:L], (B, 3), n)
    elt = e.ctx.galois_elt_from_step(1)
    dt = e.up(target)
    with traced(moai) as trace:
        # switch_key
        a, b = e.up(ct), e.up(ct)
        e.ctx.switch_key(a, dt, dkey, L, B)
        e.ctx.switch_key_hybrid(b, dt, dkey, L, 1, B)
        assert (a.to_numpy() == b.to_numpy()).all()
        # relinearize
        d3, a, b = e.up(ct3), moai.DeviceBuffer(B * 2 * L * n), moai.DeviceBuffer(B * 2 * L * n)
        e.ctx.relinearize(d3, dkey, a, L, B)
        e.ctx.relinearize_hybrid(d3, dkey, b, L, 1, B)
        assert (a.to_numpy() == b.to_numpy()).all()
        # apply_galois
        a, b = e.up(ct), e.up(ct)
        e.ctx.apply_galois(a, L, elt, dkey, B)
        e.ctx.apply_galois_hybrid(b, L, 1, elt, dkey, B)
        assert (a.to_numpy() == b.to_numpy()).all()
    counts = trace()
    for name in ("switch_key_hybrid", "relinearize_hybrid", "apply_galois_hybrid"):
        assert counts.get((name, L)) == B, name


@pytest.mark.parametrize("which", ["small", "tiled"])
def test_alpha_1_keygen_equals_kswitch_keygen(env_small1, env_tiled1, which):
    e = env_small1 if which == "small" else env_tiled1
    sk = e.ctx.sample_ternary(KEY, 1 << 40, 1, e.k)
    new = e.ctx.sample_ternary(KEY, 2 << 40, 1, e.k)
    e.ctx.ntt_forward(sk, 1, e.k)
    e.ctx.ntt_forward(new, 1, e.k)
    want = e.ctx.kswitch_keygen(KEY, 900, sk, new).to_numpy()
    got = e.ctx.hybrid_keygen(KEY, 900, sk, new, 1).to_numpy()
    assert e.ctx.hybrid_digits(1, e.lmax) == e.k - 1
    assert (got == want).all()


# ---- 2. alpha > 1 against the restatement ------------------------------------------------------------------------------------
def against_restatement(e, L):
    rng = np.random.default_rng(e.logn * 100 + L)
    key = e.random_key(rng)
    B, n = 4, e.n  # two random ciphertexts, one target with every row m - 1, one zero
    ct = O.uniform_rns(rng, e.primes[:L], (B, 2), n)
    target = O.uniform_rns(rng, e.primes[:L], (B,), n)
    target[2], target[3] = e.edge_targets(L)
    dct = e.up(ct)
    e.ctx.switch_key_hybrid(dct, e.up(target), e.up(key), L, e.alpha, B)
    got = dct.to_numpy((B, 2, L, n))
    assert e.ctx.hybrid_digits(e.alpha, L) == HR.beta(L, e.alpha)
    for b in range(B):
        assert (got[b] == HR.switch_key(e.octx, ct[b], target[b], key, L, e.alpha)).all(), b


@pytest.mark.parametrize("L", [5, 3, 1])
def test_alpha_2_small_transform_against_the_restatement(env_small2, L):
    against_restatement(env_small2, L)


@pytest.mark.parametrize("L", [7, 4])
def test_alpha_3_tiled_transform_against_the_restatement(env_tiled3, L):
    against_restatement(env_tiled3, L)


@pytest.mark.parametrize("alpha", [6, 12])
def test_wide_digits_against_the_restatement(moai, alpha):
    """digits of 6 and 12 primes take the conversion kernel's instantiations for up to 8 and up to 16 source rows; alpha + 1 data
    primes leave a last digit of one prime"""
    e = Env(moai, 10, [40] * (alpha + 1), [50] * alpha)
    against_restatement(e, alpha + 1)
    against_restatement(e, alpha)
    e.close()


def test_relinearize_and_galois_against_the_restatement(moai, env_small2):
    e, L, n = env_small2, 3, env_small2.n
    rng = np.random.default_rng(33)
    key = e.random_key(rng)
    dkey = e.up(key)
    ct3 = O.uniform_rns(rng, e.primes[:L], (2, 3), n)
    out = moai.DeviceBuffer(2 * 2 * L * n)
    e.ctx.relinearize_hybrid(e.up(ct3), dkey, out, L, e.alpha, 2)
    got = out.to_numpy((2, 2, L, n))
    for b in range(2):
        assert (got[b] == HR.relinearize(e.octx, ct3[b], key, L, e.alpha)).all(), b
    elt = e.ctx.galois_elt_from_step(3)
    dct = e.up(ct3[:, :2])
    e.ctx.apply_galois_hybrid(dct, L, e.alpha, elt, dkey, 2)
    got = dct.to_numpy((2, 2, L, n))
    for b in range(2):
        assert (got[b] == HR.apply_galois(e.octx, ct3[b, :2], L, elt, key, e.alpha)).all(), b


@pytest.mark.parametrize("which", ["small", "tiled"])
def test_keygen_against_the_restatement(env_small2, env_tiled3, which):
    e = env_small2 if which == "small" else env_tiled3
    rng = np.random.default_rng(7)
    sk = O.uniform_rns(rng, e.primes, (), e.n)  # any residues: the digit formula does not care that a key is small
    new = O.uniform_rns(rng, e.primes, (), e.n)
    got = e.ctx.hybrid_keygen(KEY, 41, e.up(sk), e.up(new), e.alpha).to_numpy((e.digits, 2, e.k, e.n))
    assert (got == HR.keygen(e.octx, KEY, 41, sk, new, e.alpha)).all()


# ---- 3. it is a key switch ---------------------------------------------------------------------------------------------------
def switch_errors(moai, e, levels, B=2):
    """for every level: (the centred rows [B][L][N] of d0 + d1 s - c s' in coefficient form, the bound B)"""
    ctx, n, k = e.ctx, e.n, e.k
    sk = ctx.sample_ternary(KEY, 3 << 40, 1, k)
    s_l1 = int(np.count_nonzero(sk.to_numpy((k, n))[0]))
    ctx.ntt_forward(sk, 1, k)
    new = moai.DeviceBuffer(k * n)
    ctx.galois_permute(sk, new, 1, k, ctx.galois_elt_from_step(1))  # the secret a rotation switches from
    key = ctx.hybrid_keygen(KEY, 1000, sk, new, e.alpha)
    out = []
    for L in levels:
        rng = np.random.default_rng(L)
        c = e.up(O.uniform_rns(rng, e.primes[:L], (B,), n))
        d = moai.DeviceBuffer(B * 2 * L * n)
        moai.hip._check(moai.hip.lib().moai_memset_zero(d.ptr, d.n_words * 8, None))
        ctx.switch_key_hybrid(d, c, key, L, e.alpha, B)
        # v = d0 + d1 s - c s', per ciphertext (the keys' first L rows are their rows at this level)
        v, t = moai.DeviceBuffer(B * L * n), moai.DeviceBuffer(L * n)
        for b in range(B):
            d0, d1 = d.ptr + (2 * b) * L * n * 8, d.ptr + (2 * b + 1) * L * n * 8
            vb = v.ptr + b * L * n * 8
            ctx.dyadic_mul(d1, sk, t, 1, 1, L)
            ctx.add(d0, t, vb, 1, L)
            ctx.dyadic_mul(c.ptr + b * L * n * 8, new, t, 1, 1, L)
            ctx.sub(vb, t, vb, 1, L)
        ctx.ntt_inverse(v, B, L)
        rows = v.to_numpy((B, L, n)).astype(np.int64)
        q = np.array(e.primes[:L], dtype=np.int64).reshape(1, L, 1)
        out.append((np.where(rows > q // 2, rows - q, rows), HR.noise_bound(e.octx, L, e.alpha, s_l1)))
    return out


def check_errors(results):
    for rows, bound in results:
        assert (rows == rows[:, :1]).all()  # every row holds the same integer
        worst = int(np.abs(rows).max())
        print("max |E| = %d, B = %.1f" % (worst, bound))
        assert worst <= bound, (worst, bound)


def test_it_is_a_key_switch_alpha_3(moai, env_tiled3):
    check_errors(switch_errors(moai, env_tiled3, (7, 4)))


def test_it_is_a_key_switch_at_moais_parameters(moai):
    """N = 2^16, MOAI's 35 data primes plus 12 60-bit special primes (a key of 0.15 GB), L = 35 and 15"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12)
    check_errors(switch_errors(moai, e, (35, 15)))
    e.close()


# ---- 4. chunking -------------------------------------------------------------------------------------------------------------
def test_chunks_of_two_give_the_unchunked_result(moai, env_tiled3):
    """L = 7, alpha = 3, beta = 3: 70 rows of 32 KiB of scratch per ciphertext, 84 with the permuted input of apply_galois: 5000 KiB
    hold two switches (chunks of 2, 2, 1) and one rotation (five chunks), 6000 KiB two of either"""
    e, L, B, n = env_tiled3, 7, 5, env_tiled3.n
    rng = np.random.default_rng(4)
    dkey = e.up(e.random_key(rng))
    ct = O.uniform_rns(rng, e.primes[:L], (B, 2), n)
    dt = e.up(O.uniform_rns(rng, e.primes[:L], (B,), n))
    elt = e.ctx.galois_elt_from_step(2)
    got = {}
    with tuned(moai):
        for kb in (None, 5000, 6000):
            moai.hip.reset_tuning()
            if kb:
                moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", kb)
            a, b = e.up(ct), e.up(ct)
            e.ctx.switch_key_hybrid(a, dt, dkey, L, e.alpha, B)
            e.ctx.apply_galois_hybrid(b, L, e.alpha, elt, dkey, B)
            got[kb] = (a.to_numpy(), b.to_numpy())
    for kb in (5000, 6000):
        assert (got[kb][0] == got[None][0]).all() and (got[kb][1] == got[None][1]).all(), kb


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_and_leaves_the_outputs_alone(moai, env_small2):
    e, n, k, alpha = env_small2, env_small2.n, env_small2.k, env_small2.alpha
    L = e.lmax
    lib = moai.hip.lib()
    fill = np.full(2 * 2 * L * n, FILL, dtype=np.uint64)
    out, src = e.up(fill), e.filled(2 * 3 * L * n, 5)
    dkey = moai.DeviceBuffer(e.digits * 2 * k * n)
    odd = 3
    h, o, s, ky = e.ctx.h, out.ptr, src.ptr, dkey.ptr
    calls = [
        # null context or pointer
        lambda: lib.moai_switch_key_hybrid(None, o, s, ky, L, alpha, 2, None),
        lambda: lib.moai_switch_key_hybrid(h, None, s, ky, L, alpha, 2, None),
        lambda: lib.moai_switch_key_hybrid(h, o, None, ky, L, alpha, 2, None),
        lambda: lib.moai_switch_key_hybrid(h, o, s, None, L, alpha, 2, None),
        lambda: lib.moai_relinearize_hybrid(h, None, ky, o, L, alpha, 2, None),
        lambda: lib.moai_relinearize_hybrid(h, s, None, o, L, alpha, 2, None),
        lambda: lib.moai_relinearize_hybrid(h, s, ky, None, L, alpha, 2, None),
        lambda: lib.moai_apply_galois_hybrid(h, None, L, alpha, odd, ky, 2, None),
        lambda: lib.moai_apply_galois_hybrid(h, o, L, alpha, odd, None, 2, None),
        lambda: lib.moai_hybrid_keygen(h, None, 0, s, s, alpha, o, None),
        lambda: lib.moai_hybrid_keygen(h, KEY, 0, None, s, alpha, o, None),
        lambda: lib.moai_hybrid_keygen(h, KEY, 0, s, None, alpha, o, None),
        lambda: lib.moai_hybrid_keygen(h, KEY, 0, s, s, alpha, None, None),
        # alpha = 0, alpha >= k
        lambda: lib.moai_switch_key_hybrid(h, o, s, ky, L, 0, 2, None),
        lambda: lib.moai_switch_key_hybrid(h, o, s, ky, 1, k, 2, None),
        lambda: lib.moai_relinearize_hybrid(h, s, ky, o, 1, k, 2, None),
        lambda: lib.moai_apply_galois_hybrid(h, o, 1, k + 1, odd, ky, 2, None),
        lambda: lib.moai_hybrid_keygen(h, KEY, 0, s, s, 0, o, None),
        lambda: lib.moai_hybrid_keygen(h, KEY, 0, s, s, k, o, None),
        # L = 0, L > k - alpha
        lambda: lib.moai_switch_key_hybrid(h, o, s, ky, 0, alpha, 2, None),
        lambda: lib.moai_switch_key_hybrid(h, o, s, ky, L + 1, alpha, 2, None),
        lambda: lib.moai_relinearize_hybrid(h, s, ky, o, L + 1, alpha, 2, None),
        lambda: lib.moai_apply_galois_hybrid(h, o, L + 1, alpha, odd, ky, 2, None),
        # an even or out-of-range Galois element
        lambda: lib.moai_apply_galois_hybrid(h, o, L, alpha, 4, ky, 2, None),
        lambda: lib.moai_apply_galois_hybrid(h, o, L, alpha, 2 * n + 1, ky, 2, None),
        # a sequence range beyond 2^56: the key has three digits
        lambda: lib.moai_hybrid_keygen(h, KEY, (1 << 56) - 2, s, s, alpha, o, None),
        lambda: lib.moai_hybrid_keygen(h, KEY, 1 << 56, s, s, alpha, o, None),
    ]
    for i, call in enumerate(calls):
        assert call() == EINVAL, i
        assert lib.moai_last_error(), i
    for bad in ((0, L), (k, 1), (alpha, 0), (alpha, L + 1)):
        assert lib.moai_hybrid_digits(h, *bad) == 0 and lib.moai_last_error()
    assert lib.moai_hybrid_digits(None, alpha, L) == 0
    # batch = 0 is MOAI_OK and enqueues nothing
    assert lib.moai_switch_key_hybrid(h, o, s, ky, L, alpha, 0, None) == 0
    assert lib.moai_relinearize_hybrid(h, s, ky, o, L, alpha, 0, None) == 0
    assert lib.moai_apply_galois_hybrid(h, o, L, alpha, odd, ky, 0, None) == 0
    assert (out.to_numpy() == fill).all()
