"""moai_ct_dot_galois (csrc/ctdot_galois.hip.h) and moai_galois_fold (csrc/keyswitch.hip): Q.K^T with the key switches after the sum.
1. The four sums of every output against Python integers on the oracle's permutation table, at the kernel's seams: 12 (staged) and
   8 (gather) outputs per group (13 = a second group), a fold every 32 terms (33), sixteen workgroups per row (N = 4096) and one with
   idle threads (N = 16, always the gather form), a 61-bit prime beside one below 2^51.  At N = 4096 the elements 1, 5^256 and
   5^512 keep aligned blocks of 256 coefficients and read w through LDS; 5 and 2N - 1 gather; "mixed" runs both forms in one call.
2. The fold against two moai_switch_key per output into zero ciphertexts and moai_add.  3. Both orders decrypted under (1, s, s^2) as
   exact integers: E (1 + |s|_1) for the fold, sum_j |m_X[j]|_1 E for moai_apply_galois on every w[j] followed by moai_ct_dot
   (each rotation's error is multiplied by m_X[j]); E = hybrid_ref.noise_bound at alpha = 1, the bound of one moai_switch_key."""
import numpy as np
import pytest

import client_sampling as CS
import hybrid_kit as HK
import hybrid_ref as HR
import mode_limits as ML
import oracle as O
from test_gpu_keyswitch_ptrs import Env  # a 60-bit integer row, the two FP64 classes, a 60-bit special prime; four keys

G, FOLD, MAX_TERMS, SENTINEL = 12, 32, 65536, 0xDEADBEEF  # csrc/ctdot_galois.hip.h CDG_G, CDG_FOLD, CDG_MAX_TERMS
ROWS = ("fpr_hi", "g61")  # the largest prime below 2^51 and the largest below 2^61
_ctxs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


def draw(logn, which, n_out):
    m = 2 << logn
    # "seam": 5^8 = 1 mod 2^5 keeps blocks of N / 16 (256 at N = 4096: the largest staged block, all of it permuted), 5^4 blocks of N / 8
    pool = {"mixed": (pow(5, 256, m), 5, 1, m - 1, pow(5, 512, m)), "staged": (pow(5, 256, m), pow(5, 512, m), 1), "gather": (5, m - 1),
            "seam": (pow(5, 8, m), pow(5, 4, m))}[which]
    return [pool[i % len(pool)] for i in range(n_out)]


def exact(x, w, elts, primes, logn):
    """[n_out][4][L][N] = (x0 pw0, x1 pw0, x0 pw1, x1 pw1) summed over the terms, pw = w permuted by the oracle's table"""
    xo, wo, per_elt = x.astype(object), w.astype(object), {}
    for e in set(elts):
        pw = wo[..., O.galois_table_ntt(logn, e)]
        per_elt[e] = np.stack([np.stack([(xo[:, c & 1, r] * pw[:, c >> 1, r]).sum(axis=0) % q for r, q in enumerate(primes)]) for c in range(4)])
    return np.stack([per_elt[e] for e in elts]).astype(np.uint64)


def run(moai, logn, x, w, elts, terms=None, dout=None):
    primes = [ML.chain(logn)[name] for name in ROWS]
    ctx = HK.cached(_ctxs, logn, lambda: moai.Context(logn, primes))
    shape = (len(elts), 4) + x.shape[2:]
    dout = moai.DeviceBuffer.from_numpy(np.full(shape, SENTINEL, dtype=np.uint64)) if dout is None else dout
    ctx.ct_dot_galois(moai.DeviceBuffer.from_numpy(x), moai.DeviceBuffer.from_numpy(w), dout, elts, x.shape[0] if terms is None else terms, len(primes))
    return dout.to_numpy(shape)


CASES = [(logn, terms, n_out, "mixed") for logn in (12, 4) for terms in (1, 3, FOLD + 1) for n_out in (1, G + 1)] + [
    (12, FOLD + 1, G + 1, "staged"), (12, FOLD + 1, G + 1, "gather"), (12, 1, 1, "gather"), (4, FOLD + 1, G + 1, "gather"),
    (12, 3, G + 1, "seam"), (12, FOLD + 1, G + 1, "mixed, every residue q - 1")]  # 32 terms of (q - 1)^2 reach the accumulator's limit before the fold


@pytest.mark.gpu
@pytest.mark.parametrize("logn,terms,n_out,which", CASES)
def test_sums_match_exact_integers(moai, logn, terms, n_out, which):
    rng = np.random.default_rng(1000 * terms + 10 * n_out + logn)
    primes = [ML.chain(logn)[name] for name in ROWS]
    x, w = (O.uniform_rns(rng, primes, (terms, 2), 1 << logn) for _ in range(2))
    if "q - 1" in which:
        x[:], w[:] = (np.array(primes, dtype=np.uint64)[:, None] - np.uint64(1),) * 2
    elts = draw(logn, which.split(",")[0], n_out)
    got = run(moai, logn, x, w, elts)
    bad = np.argwhere(got != exact(x, w, elts, primes, logn))
    assert not len(bad), ("first of %d at [output, component, prime, coeff]" % len(bad), bad[0].tolist())


@pytest.mark.gpu
def test_refusals_enqueue_nothing(moai):
    logn, m = 12, 2 << 12
    x = np.zeros((3, 2, len(ROWS), 1 << logn), dtype=np.uint64)
    dout = moai.DeviceBuffer.from_numpy(np.full(2 * 4 * x[0, 0].size, SENTINEL, dtype=np.uint64))
    # a valid element before the refused one (gather and staged): a launch of the first group would show in the output
    for elts, terms in (([5, 4], 3), ([pow(5, 256, m), m + 1], 3), ([5, m - 1], 0), ([5, m - 1], MAX_TERMS + 1)):
        with pytest.raises(moai.hip.MoaiError) as err:
            run(moai, logn, x, x, elts, terms, dout)
        assert err.value.code == moai.hip.MOAI_EINVAL, (elts, terms)
        assert (dout.to_numpy((dout.n_words,)) == SENTINEL).all(), (elts, terms)
    with pytest.raises(moai.hip.MoaiError):
        _ctxs[logn].ct_dot_galois(None, moai.DeviceBuffer.from_numpy(x), dout, [5, m - 1], 3, len(ROWS))
    assert (dout.to_numpy((dout.n_words,)) == SENTINEL).all()
    _ctxs[logn].ct_dot_galois(None, None, None, [], 3, len(ROWS))  # no outputs: MOAI_OK


@pytest.mark.gpu
@pytest.mark.parametrize("logn,n_out", [(12, 3), (11, 3), (11, 33)])  # 33 outputs: 66 switches, two passes of the list
def test_fold_is_two_switch_keys_and_the_additions(moai, logn, n_out):
    e, L, up = Env(moai, logn), 3, moai.DeviceBuffer.from_numpy
    rng, rn = np.random.default_rng(logn), 3 * e.n * 8  # bytes of a polynomial
    acc = O.uniform_rns(rng, e.primes[:L], (n_out, 4), e.n)
    keys = [e.dkeys[i % 4] for i in range(n_out)]
    out = up(np.full((n_out, 3, L, e.n), SENTINEL, dtype=np.uint64))
    e.ctx.galois_fold(up(acc), keys, out, L)
    got = out.to_numpy((n_out, 3, L, e.n))
    for i in range(n_out):
        d, u, v = up(acc[i]), up(np.zeros((2, L, e.n), dtype=np.uint64)), up(np.zeros((2, L, e.n), dtype=np.uint64))
        e.ctx.switch_key(u, d.ptr + 2 * rn, keys[i], L, 1)
        e.ctx.switch_key(v, d.ptr + 3 * rn, keys[i], L, 1)
        e.ctx.add(d, u, u, 2, L)                     # (A0 + u0, A1 + u1)
        e.ctx.add(u.ptr + rn, v, u.ptr + rn, 1, L)   # ... + v0
        want = np.concatenate([u.to_numpy((2, L, e.n)), v.to_numpy((2, L, e.n))[1:]])
        assert (got[i] == want).all(), i


@pytest.mark.gpu
def test_deferred_and_conventional_order_decrypt_within_their_bounds(moai):
    e, L, terms, up = Env(moai, 12), 3, 3, moai.DeviceBuffer.from_numpy
    n, primes, rng = e.n, e.primes[:3], np.random.default_rng(3)
    elts = [pow(5, 256, 2 * n), 5]  # the staged and the gather form
    s, s_ntt = HK.secret(e.octx, HK.KEY, 77)
    s_l1, so = int(np.count_nonzero(s)), HR._obj(s_ntt[:L])
    q = np.array(primes, dtype=object).reshape(L, 1)
    m = rng.integers(-1024, 1025, (2, terms, n))
    m_ntt = np.stack([[HR._obj(e.octx.ntt(CS.to_rns(v, primes), L)) for v in side] for side in m])  # [2][terms][L][N]
    c1 = HR._obj(O.uniform_rns(rng, primes, (2, terms), n))
    cts = HR._u64(np.stack([(m_ntt - c1 * so) % q, c1], axis=2))  # [2][terms][2][L][N]: c0 + c1 s = m exactly
    dx, dw = up(cts[0]), up(cts[1])
    tables = [O.galois_table_ntt(e.logn, elt) for elt in elts]
    keys = [e.ctx.kswitch_keygen(HK.KEY, 1000 + 100 * i, up(s_ntt), up(np.ascontiguousarray(s_ntt[:, t]))) for i, t in enumerate(tables)]

    def error(ct3, i):  # the centred integers of c0 + c1 s + c2 s^2 - sum_j m_X[j] pi_i(m_W[j])
        c = HR._obj(ct3)
        want = (m_ntt[0] * m_ntt[1][..., tables[i]]).sum(axis=0) % q
        d = HR._u64((c[0] + c[1] * so + c[2] * so * so) % q)
        return HR.switch_error(e.octx, [d, np.zeros_like(d)], HR._u64(want), s_ntt[:L], np.ones_like(d), L)

    E = HR.noise_bound(e.octx, L, 1, s_l1)
    acc, out = moai.DeviceBuffer(len(elts) * 4 * L * n), moai.DeviceBuffer(len(elts) * 3 * L * n)
    e.ctx.ct_dot_galois(dx, dw, acc, elts, terms, L)
    e.ctx.galois_fold(acc, keys, out, L)
    deferred = max(int(np.abs(error(ct3, i)).max()) for i, ct3 in enumerate(out.to_numpy((len(elts), 3, L, n))))
    conventional, d3 = 0, moai.DeviceBuffer(3 * L * n)
    for i, elt in enumerate(elts):
        rot = up(cts[1])
        e.ctx.apply_galois(rot, L, elt, keys[i], terms)
        e.ctx.ct_dot(dx, rot, d3, terms, L)
        conventional = max(conventional, int(np.abs(error(d3.to_numpy((3, L, n)), i)).max()))
    bounds = E * (1 + s_l1), E * int(np.abs(m[0]).sum())
    print("max |error|: deferred %d (bound %.0f), conventional %d (bound %.0f)" % (deferred, bounds[0], conventional, bounds[1]))
    assert 0 < deferred <= bounds[0] and 0 < conventional <= bounds[1]


def test_declared_cited_exported_and_bound(moai):
    for name in ("moai_ct_dot_galois", "moai_galois_fold"):
        comment = HK.header_comment(name)
        assert "Ct_ct_matrix_mul.hpp:6-56" in comment and "SEAL/evaluator.cpp:" in comment, name
    assert "SEAL/evaluator.cpp:2724-3020" in HK.header_comment("moai_galois_fold")
    assert "terms <= %d" % MAX_TERMS in HK.header_comment("moai_ct_dot_galois")
    HK.exported(moai, ["moai_ct_dot_galois", "moai_galois_fold"], ["ct_dot_galois", "galois_fold"])
