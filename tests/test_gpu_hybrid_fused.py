"""The fused hybrid key switch (MOAI_HYBRID_FUSED = 1; csrc/hybrid_kernels.hip.h hy_scale_digits_kernel, hy_fwd_strided, hy_contig_mac8):
mod-up, forward transform and key product as two passes, bit for bit the unfused path.

1. moai_switch_key_hybrid against the integer restatement tests/hybrid_ref.py on a chain with FP64, no-guard and guarded rows: one
   strided tile per row (logn 12) and two (13); digits of 3+3+1, 3+1 and 1 primes; MOAI_NTT_FP 0 and 1.
2. the limit primes of every arithmetic mode, key rows all m - 1 and scaled residues all q_r - 1.    3. digits of sixteen 61-bit primes.
4. every other entry point that runs steps 1-4 on one target: fused = unfused, the rescale forms in both rounding modes.
5. scratch budgets that cut the output rows into one group per mode, into several groups, into one row per group.
6. N = 2^16 at MOAI's parameters once.    7. the knob is a switch: off by default, without effect below N = 2^12.

Where a case only needs "same as unfused" the comparator is the knob-off call, which the existing files pin to the restatement.  The
restatement is computed once per shape and shared across the knob and FP parameters."""
import numpy as np
import pytest

import hybrid_ref as HR
import mode_limits as ML
import oracle as O
from hybrid_kit import ENVS, MOAI_DATA_BITS, Env, tuned

pytestmark = pytest.mark.gpu

_envs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for e in _envs.values():
        e.close()
    _envs.clear()


def env(moai, key, make):
    if key not in _envs:
        _envs[key] = make()
    return _envs[key]


def tiled3(moai, logn=12):
    _, data, special = ENVS["tiled3"]
    return env(moai, ("tiled3", logn), lambda: Env(moai, logn, data, special))


def restated(e, L):
    """the against_restatement inputs of one shape -- two random targets, one with every row m - 1, one zero -- and HR.switch_key"""
    if ("fused", L) not in e.cache:
        rng = np.random.default_rng(e.logn * 100 + L)
        key = e.random_key(rng)
        ct = O.uniform_rns(rng, e.primes[:L], (4, 2), e.n)
        target = O.uniform_rns(rng, e.primes[:L], (4,), e.n)
        target[2], target[3] = e.edge_targets(L)
        want = np.stack([HR.switch_key(e.octx, ct[b], target[b], key, L, e.alpha) for b in range(4)])
        e.cache[("fused", L)] = (e.up(key), ct, e.up(target), want)
    return e.cache[("fused", L)]


def switched(e, L, dkey, ct, dtarget):
    d = e.up(ct)
    e.ctx.switch_key_hybrid(d, dtarget, dkey, L, e.alpha, len(ct))
    got = d.to_numpy(ct.shape)
    d.free()
    return got


# ---- 1. the switch against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp", [1, 0])
@pytest.mark.parametrize("L", [7, 4, 1])
@pytest.mark.parametrize("logn", [12, 13])
def test_fused_switch_against_the_restatement(moai, logn, L, fp):
    e = tiled3(moai, logn)
    dkey, ct, dtarget, want = restated(e, L)
    with tuned(moai, MOAI_HYBRID_FUSED=1, MOAI_NTT_FP=fp):
        assert e.ctx.hybrid_fused_groups(L, e.alpha, 4) > 0
        got = switched(e, L, dkey, ct, dtarget)
    assert (got == want).all()


# ---- 2., 3. limit primes and wide digits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,alpha,L", [(w, None, 7) for w in ML.HYBRID_CHAINS] + [("wide", 16, 17), ("wide", 16, 16)])
def test_fused_switch_at_the_limit_primes(moai, which, alpha, L):
    """key rows all m - 1; target = NTT of worst_coeff, so every scaled residue is q_r - 1: the largest sums both passes can form"""
    primes, _, alpha = ML.hybrid_chain(12, which, alpha)
    e = env(moai, (which, alpha), lambda: Env(moai, 12, primes=primes, alpha=alpha))
    key = np.empty((e.digits, 2, e.k, e.n), dtype=np.uint64)
    for i, m in enumerate(e.primes):
        key[:, :, i, :] = m - 1
    target = e.octx.ntt(ML.worst_coeff(e.primes, L, alpha, e.n), L)
    ct = O.uniform_rns(np.random.default_rng(L), e.primes[:L], (1, 2), e.n)
    with tuned(moai, MOAI_HYBRID_FUSED=1):
        assert e.ctx.hybrid_fused_groups(L, alpha, 1) > 0
        dkey, dtarget = e.up(key), e.up(target[None])
        got = switched(e, L, dkey, ct, dtarget)
    dkey.free()
    dtarget.free()
    assert (got[0] == HR.switch_key(e.octx, ct[0], target, key, L, alpha)).all()


# ---- 4. the other entry points: fused = unfused ----------------------------------------------------------------------------------------
def run_form(moai, e, form, L, rng):
    """one call of `form` on two ciphertexts (two members with their own keys where the form takes them); the outputs as arrays"""
    ctx, n, a = e.ctx, e.n, e.alpha
    made = []

    def up(x):
        made.append(e.up(x))
        return made[-1]

    keys = [up(e.random_key(rng)) for _ in range(2)]
    ct3 = O.uniform_rns(rng, e.primes[:L], (2, 3), n)
    ct, ct2 = ct3[:, :2].copy(), O.uniform_rns(rng, e.primes[:L], (2, 2), n)
    Lo = L - 1 if "rescale" in form else L
    out = moai.DeviceBuffer(2 * 2 * Lo * n)
    outs = [moai.DeviceBuffer(2 * Lo * n) for _ in range(2)]
    elt = {"galois_conj": 2 * n - 1}.get(form, ctx.galois_elt_from_step(3))
    if form == "relinearize":
        ctx.relinearize_hybrid(up(ct3), keys[0], out, L, a, 2)
    elif form in ("galois_step", "galois_conj"):
        out.free()
        out = up(ct)
        ctx.apply_galois_hybrid(out, L, a, elt, keys[0], 2)
    elif form == "galois_to":
        ctx.apply_galois_hybrid_to(up(ct), out, L, a, elt, keys[0], 2)
    elif form == "galois_acc":
        out.free()
        out = up(ct2)
        ctx.apply_galois_hybrid_acc(up(ct), out, L, a, elt, keys[0], 2)
    elif form == "relinearize_rescale":
        ctx.relinearize_rescale_hybrid(up(ct3), keys[0], out, L, a, 2)
    elif form == "multiply_relin_rescale":
        ctx.multiply_relin_rescale_hybrid(up(ct), up(ct2), keys[0], out, L, a, 2)
    elif form == "galois_ptrs":
        ctx.apply_galois_hybrid_ptrs([up(ct[0]), up(ct[1])], outs, L, a, [elt, 2 * n - 1], keys, [up(ct2[0]), None])
    elif form == "relinearize_ptrs":
        ctx.relinearize_hybrid_ptrs([up(ct3[0]), up(ct3[1])], outs, keys[1], L, a)
    else:
        ctx.relinearize_rescale_hybrid_ptrs([up(ct3[0]), up(ct3[1])], outs, keys[1], L, a)
    got = [b.to_numpy() for b in (outs if "ptrs" in form else [out])]
    for b in {id(b): b for b in made + outs + [out]}.values():
        b.free()
    return got


FORMS = ["relinearize", "galois_step", "galois_conj", "galois_to", "galois_acc", "galois_ptrs", "relinearize_ptrs"]
RESCALE_FORMS = ["relinearize_rescale", "multiply_relin_rescale", "relinearize_rescale_ptrs"]


@pytest.mark.parametrize("form,exact", [(f, 0) for f in FORMS + RESCALE_FORMS] + [(f, 1) for f in RESCALE_FORMS])
def test_every_entry_point_fused_equals_unfused(moai, form, exact):
    e, L = tiled3(moai), 7
    e.ctx.hybrid_set_rounding(exact)
    try:
        got = {}
        for knob in (0, 1):
            with tuned(moai, MOAI_HYBRID_FUSED=knob):
                got[knob] = run_form(moai, e, form, L, np.random.default_rng(40))
    finally:
        e.ctx.hybrid_set_rounding(0)
    assert len(got[0]) == len(got[1])
    for a, b in zip(got[0], got[1]):
        assert (a == b).all()


# ---- 5. budgets ------------------------------------------------------------------------------------------------------------------------
def test_budgets_that_cut_the_output_rows_into_groups(moai):
    """L = 7, alpha = 3, beta = 3, rows of 32 KiB: 47 rows per ciphertext and 3 per output row in flight.  Every budget holds one
    ciphertext (7 digit rows: the integer modes, eight no-guard rows and two guarded ones): 77 rows take all ten output rows, so one
    group per mode; 59 rows take four (4 + 4 + 2); 50 rows take one row per group, and so does a budget below one ciphertext"""
    e, L = tiled3(moai), 7
    dkey, ct, dtarget, want = restated(e, L)
    groups = {}
    for rows in (77, 59, 50, 3):
        with tuned(moai, MOAI_HYBRID_FUSED=1, MOAI_HYBRID_TMP_KB=rows * 32):
            groups[rows] = e.ctx.hybrid_fused_groups(L, e.alpha, 4)
            assert (switched(e, L, dkey, ct, dtarget) == want).all(), rows
    assert groups == {77: 2, 59: 3, 50: 10, 3: 10}


# ---- 6. N = 2^16 once ------------------------------------------------------------------------------------------------------------------
def test_fused_equals_unfused_at_moais_parameters(moai):
    """MOAI's 35 data primes with 12 special primes: digits of 12 + 12 + 11 primes at L = 35, of 12 + 3 at L = 15; sixteen tiles a row"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12, oracle=False)
    rng = np.random.default_rng(16)
    dkey = e.up(e.random_key(rng))
    for L in (35, 15):
        ct = O.uniform_rns(rng, e.primes[:L], (2, 2), e.n)
        dtarget = e.up(O.uniform_rns(rng, e.primes[:L], (2,), e.n))
        got = {}
        for knob in (0, 1):
            with tuned(moai, MOAI_HYBRID_FUSED=knob):
                assert (e.ctx.hybrid_fused_groups(L, e.alpha, 2) > 0) == bool(knob)
                got[knob] = switched(e, L, dkey, ct, dtarget)
        dtarget.free()
        assert (got[0] == got[1]).all(), L
    dkey.free()
    e.close()


# ---- 7. the switch is a switch ---------------------------------------------------------------------------------------------------------
def test_the_knob_is_off_by_default_and_without_effect_below_4096(moai):
    e = tiled3(moai)
    small = env(moai, "small2", lambda: Env(moai, *ENVS["small2"]))
    assert e.ctx.hybrid_fused_groups(7, e.alpha, 4) == 0
    with tuned(moai, MOAI_HYBRID_FUSED=1):
        assert e.ctx.hybrid_fused_groups(7, e.alpha, 4) > 0
        assert small.ctx.hybrid_fused_groups(5, small.alpha, 4) == 0
        dkey, ct, dtarget, want = restated(small, 5)
        assert (switched(small, 5, dkey, ct, dtarget) == want).all()
    assert e.ctx.hybrid_fused_groups(7, e.alpha, 4) == 0
    with pytest.raises(moai.MoaiError):
        e.ctx.hybrid_fused_groups(e.lmax + 1, e.alpha, 4)
