"""The small-degree family (N <= 2048) at the limit primes of tests/mode_limits.py, bit for bit against the CPU oracle.

Below 2^12 none of the tiled or fused kernels run: the transforms are ntt_small (one workgroup per row, the row in LDS), the key
switch is reduce_rows_kernel, ntt_small, keyswitch_mac_kernel (a 128-bit sum over all L digits, no fold: L q^2 < 2^128 is all it
has), sum_rows_kernel, the mod-down is expand_last_kernel, ntt_small, moddown_finalize_kernel, mul_scalar_rescale takes two steps
and the hoisted call makes the separate rotations.  This family has no arithmetic modes, so nothing here asks moai_arith_mode; the
primes are the same ones because the bounds that bind are the same numbers: 61 bits in the lazy butterflies and the 128-bit
sum, and a special prime on either side of the data primes in the mod-down.

Degrees: N = 8 (almost every lane idle, one row is four 16-byte chunks), N = 256 (half the butterfly lanes idle, 128 chunks per
row), N = 2048 (LDS full, eight butterflies per thread); the transforms also at N = 2 and N = 4.  The inputs are those of
tests/test_gpu_mode_limits.py (tests/mode_limit_cases.py)."""
import numpy as np
import pytest

import mode_limits as ML
import oracle as O
from mode_limit_cases import (HOIST_STEPS, K, KS_INPUTS, L8, MIXED_ROWS, ORDER_NAMES, contexts, hoist_case, ks_case, long_case, long_refs,
                              ntt_case, release, rescale_case, up)

pytestmark = pytest.mark.gpu

SMALL_LOGNS = [3, 8, 11]
_own = []  # device contexts of this module's own chains


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    """the cached device contexts live as long as this module's tests, whichever ran"""
    yield
    release()
    for ctx in _own:
        ctx.close()
    _own.clear()


def qcol(primes):
    return np.array(primes, dtype=np.uint64)[:, None]


# ---- 1. the transforms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [1, 2] + SMALL_LOGNS)
def test_ntt_small_at_the_limits(moai, logn):
    """every pattern under all nine primes: forward, round trip, inverse of arbitrary data, and both from the top of the input range
    include/moai_hip.h promises for every row: [0, 4q) forward, [0, 2q) inverse"""
    c = ntt_case(logn)
    primes, names, _, ctx = contexts(moai, logn, "g61_last")
    q = qcol(primes)[None]
    for p, pname in enumerate(ML.PATTERNS):
        x = c["x"][p]
        d = up(moai, x)
        ctx.ntt_forward(d, 2, K)
        assert (d.to_numpy(x.shape) == c["fwd"][p]).all(), "forward, " + pname
        ctx.ntt_inverse(d, 2, K)
        assert (d.to_numpy(x.shape) == x).all(), "round trip, " + pname
        ctx.ntt_inverse(d, 2, K)
        assert (d.to_numpy(x.shape) == c["inv"][p]).all(), "inverse, " + pname
        d.upload(x + np.uint64(3) * q)
        ctx.ntt_forward(d, 2, K)
        assert (d.to_numpy(x.shape) == c["fwd"][p]).all(), "forward from the top of [0, 4q), " + pname
        d.upload(x + q)
        ctx.ntt_inverse(d, 2, K)
        assert (d.to_numpy(x.shape) == c["inv"][p]).all(), "inverse from the top of [0, 2q), " + pname
        d.free()


@pytest.mark.parametrize("logn", [1, 2] + SMALL_LOGNS)
def test_ntt_small_permuted_primes(moai, logn):
    """row r is not prime r (MIXED_ROWS through prime_index), three polynomials: which prime's tables and constants a row gets"""
    n, npoly = 1 << logn, 3
    primes, names, octx, ctx = contexts(moai, logn, "g61_last")
    pidx = [ML.ORDERS["g61_last"].index(name) for name in MIXED_ROWS]
    assert sorted(pidx) == list(range(K)) and pidx != list(range(K))
    pat = ML.pattern_rows([primes[i] for i in pidx], n, np.random.default_rng(6250 + logn))
    x = np.stack([np.roll(pat, j, axis=-1) for j in range(npoly)], axis=1)  # [pattern][3][9][N]
    fwd = octx.ntt(x.reshape(-1, K, n), K, prime_index=pidx).reshape(x.shape)
    inv = octx.ntt(x.reshape(-1, K, n), K, prime_index=pidx, inverse=True).reshape(x.shape)
    for p, pname in enumerate(ML.PATTERNS):
        d = up(moai, x[p])
        ctx.ntt_forward(d, npoly, K, prime_index=pidx)
        assert (d.to_numpy(x[p].shape) == fwd[p]).all(), "forward, " + pname
        ctx.ntt_inverse(d, npoly, K, prime_index=pidx)
        assert (d.to_numpy(x[p].shape) == x[p]).all(), "round trip, " + pname
        ctx.ntt_inverse(d, npoly, K, prime_index=pidx)
        assert (d.to_numpy(x[p].shape) == inv[p]).all(), "inverse, " + pname
        d.free()


# ---- 2. the key switch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,order", [(l, o) for l in SMALL_LOGNS for o in ORDER_NAMES])
def test_key_switch_small_at_the_limits(moai, logn, order):
    """switch_key, apply_galois and relinearize on two ciphertexts per input of KS_INPUTS: keys and digits all q-1 under 59- to
    61-bit primes in the unfolded 128-bit sum, and (fpr_hi_last) a special prime below the data primes in the mod-down"""
    n = 1 << logn
    primes, names, _, ctx = contexts(moai, logn, order)
    elt, cases = ks_case(moai, logn, order)
    assert [c["name"] for c in cases] == list(KS_INPUTS)
    dkeys = {}
    for c in cases:
        if id(c["key"]) not in dkeys:
            dkeys[id(c["key"])] = up(moai, c["key"])
        dkey = dkeys[id(c["key"])]
        d, dt = up(moai, c["ct"]), up(moai, c["tgt"])
        ctx.switch_key(d, dt, dkey, L8, 2)
        assert (d.to_numpy(c["ct"].shape) == c["sk"]).all(), "switch_key, " + c["name"]
        d.upload(c["ctg"])
        ctx.apply_galois(d, L8, elt, dkey, 2)
        assert (d.to_numpy(c["ct"].shape) == c["ag"]).all(), "apply_galois, " + c["name"]
        d3 = up(moai, c["ct3"])
        ctx.relinearize(d3, dkey, d, L8, 2)
        assert (d.to_numpy(c["ct"].shape) == c["rl"]).all(), "relinearize, " + c["name"]
        for b in (d, dt, d3):
            b.free()
    for b in dkeys.values():
        b.free()


@pytest.mark.parametrize("logn,order", [(l, o) for l in SMALL_LOGNS for o in ORDER_NAMES])
def test_key_switch_small_to_acc_and_lists(moai, logn, order):
    """the other entry points of the same kernels with two ciphertexts: moai_apply_galois_to (the permuted c0 as the addend of the
    even polynomials), moai_apply_galois_acc (the accumulator as the addend of all), moai_apply_galois_ptrs (two keys, two
    elements, one member with a sum buffer) and moai_relinearize_ptrs -- the LIST forms of keyswitch_mac_kernel and
    moddown_finalize_kernel; each against the oracle's result for the single ciphertext"""
    n = 1 << logn
    primes, names, octx, ctx = contexts(moai, logn, order)
    elt, cases = ks_case(moai, logn, order)
    shape = (2, 2, L8, n)
    top = np.broadcast_to(qcol(primes[:L8]) - np.uint64(1), shape)  # an addend of all q-1
    for c in cases:
        dkey = up(moai, c["key"])
        src, dst = up(moai, c["ctg"]), moai.DeviceBuffer(c["ctg"].size)
        ctx.apply_galois_to(src, dst, L8, elt, dkey, 2)
        assert (dst.to_numpy(shape) == c["ag"]).all(), "apply_galois_to, " + c["name"]
        assert (src.to_numpy(shape) == c["ctg"]).all(), "apply_galois_to left its source, " + c["name"]
        acc = up(moai, top)
        ctx.apply_galois_acc(src, acc, L8, elt, dkey, 2)
        want = np.stack([octx.add(top[b], c["ag"][b], 2, L8) for b in range(2)])
        assert (acc.to_numpy(shape) == want).all(), "apply_galois_acc, " + c["name"]
        d3 = [up(moai, c["ct3"][b]) for b in range(2)]
        outs = [moai.DeviceBuffer(2 * L8 * n) for _ in range(2)]
        ctx.relinearize_ptrs(d3, outs, dkey, L8)
        for b in range(2):
            assert (outs[b].to_numpy((2, L8, n)) == c["rl"][b]).all(), ("relinearize_ptrs", c["name"], b)
        for buf in [dkey, src, dst, acc] + d3 + outs:
            buf.free()
    # a list of two: the all q-1 key with the rotation, the random key with the conjugation and a sum buffer of all q-1
    conj = 2 * n - 1
    first, last = cases[0], cases[2]
    assert first["key"] is not last["key"]
    want1 = octx.add(top[0], octx.apply_galois(last["ct"][1], L8, conj, last["key"]).reshape(2, L8, n), 2, L8)
    keys = [up(moai, first["key"]), up(moai, last["key"])]
    ins = [up(moai, first["ctg"][0]), up(moai, last["ct"][1])]
    outs = [moai.DeviceBuffer(2 * L8 * n) for _ in range(2)]
    dsum = up(moai, top[0])
    ctx.apply_galois_ptrs(ins, outs, L8, [elt, conj], keys, [None, dsum])
    assert (outs[0].to_numpy((2, L8, n)) == first["ag"][0]).all(), "apply_galois_ptrs, member 0"
    assert (outs[1].to_numpy((2, L8, n)) == want1).all(), "apply_galois_ptrs, member 1 (sum)"
    for buf in keys + ins + outs + [dsum]:
        buf.free()


# ---- 3. rescale and mod-down --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", SMALL_LOGNS)
def test_rescale_small_at_the_limits(moai, logn):
    """every level of both orders: the dropped row's coefficients on the rounding boundary (expand_last_kernel's [x + q_last / 2]
    mod q_last), kept rows all q-1; the two-step mul_scalar_rescale with scalars q-1; and both with an addend of all q-1"""
    n = 1 << logn
    c = rescale_case(moai, logn)
    dropped = set()
    for order in ORDER_NAMES:
        primes, names, octx, ctx = contexts(moai, logn, order)
        for L in range(K, 1, -1):
            dropped.add(names[L - 1])
            x, ref = c[(order, L)]
            top = np.ascontiguousarray(np.broadcast_to(qcol(primes[:L - 1]) - np.uint64(1), ref.shape))
            dx = up(moai, x)
            do = moai.DeviceBuffer(ref.size)
            ctx.rescale(dx, do, 2, L, 2)
            assert (do.to_numpy(ref.shape) == ref).all(), (order, L, "dropped " + names[L - 1])
            dadd = up(moai, top)
            ctx.rescale_add(dx, dadd, do, 2, L, 2)
            want = np.stack([octx.add(ref[b], top[b], 2, L - 1) for b in range(2)])
            assert (do.to_numpy(ref.shape) == want).all(), (order, L, "rescale_add")
            ctx.rescale_add(dx, dadd, dadd, 2, L, 2)  # accumulating in place
            assert (dadd.to_numpy(ref.shape) == want).all(), (order, L, "rescale_add in place")
            if order == "g61_last" and L == K:
                scal = [q - 1 for q in primes]
                ctx.mul_scalar_rescale(dx, scal, do, 2, L, 2)
                assert (do.to_numpy(ref.shape) == c["scalar"]).all(), "mul_scalar_rescale"
                dadd.upload(top)
                ctx.mul_scalar_rescale_add(dx, scal, dadd, do, 2, L, 2)
                want = np.stack([octx.add(c["scalar"][b], top[b], 2, L - 1) for b in range(2)])
                assert (do.to_numpy(ref.shape) == want).all(), "mul_scalar_rescale_add"
                assert (dx.to_numpy(x.shape) == x).all(), "the source of the two-step product"
            for buf in (dx, do, dadd):
                buf.free()
    assert dropped == set(ML.NAMES)  # every prime was the dropped one


# ---- 4. hoisted rotations -----------------------------------------------------------------------------------------------------
def test_hoisted_rotations_small_take_the_separate_calls(moai):
    """below N = 4096 moai_apply_galois_hoisted makes the R separate calls and says so (*used_fallback = 1, include/moai_hip.h);
    the bits are those of the four rotations"""
    logn = 11
    n = 1 << logn
    primes, names, _, ctx = contexts(moai, logn, "g61_last")
    elts, keys, ct, ref = hoist_case(moai, logn)
    R = len(elts)
    assert R == len(HOIST_STEPS) == 4
    dkeys = [up(moai, kk) for kk in keys]
    corrs = [ctx.hoist_correction(dk, e, L8) for dk, e in zip(dkeys, elts)]
    dct = up(moai, ct)
    dout = moai.DeviceBuffer(R * 2 * 2 * L8 * n)
    assert ctx.apply_galois_hoisted(dct, dout, L8, elts, dkeys, corrs, 2) is True
    got = dout.to_numpy(ref.shape)
    for r in range(R):
        assert (got[r] == ref[r]).all(), HOIST_STEPS[r]
    assert (dct.to_numpy(ct.shape) == ct).all()
    for b in corrs + dkeys + [dct, dout]:
        b.free()


# ---- 5. a long chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [17, 63])
def test_long_chain_key_switch_2_11(moai, L):
    """64 primes (MOAI_MAX_RNS): keyswitch_mac_kernel adds L products of canonical residues in 128 bits and never folds, so L = 63
    digits of all q-1 against key rows of all q-1 is its largest sum (63 q^2 < 2^128 for q < 2^61).  The key rows under the 61-bit
    special prime are capped by ML.reference_key_cap, as in long_refs: beyond it the reference's own sum (4 q v L < 2^128) wraps.
    An uncapped 61-bit key has no independent reference in this repository and is out of scope here."""
    logn, k = 11, 64
    n = 1 << logn
    c = long_case(moai, logn, k)
    ctx, primes = c["ctx"], c["primes"]
    assert L < k and all(L * (q - 1) ** 2 < 1 << 128 for q in primes)
    for key, (ct, tgt, ref) in zip(c["keys"], long_refs(c, L)):
        dkey, d, dt = up(moai, key), up(moai, ct[None]), up(moai, tgt[None])
        ctx.switch_key(d, dt, dkey, L, 1)
        got = d.to_numpy((2, L, n))
        for b in (d, dt, dkey):
            b.free()
        assert (got == ref).all(), L


# ---- 6. mod-raise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["g61", "small"])
def test_modraise_small_from_the_largest_and_the_smallest_prime(moai, first):
    """q0 = g61: every target prime is smaller (the coefficient is reduced, and so is q0 in the correction of the upper half);
    q0 = small: every target is larger.  Source COEFFICIENTS 0, q0/2, q0/2 + 1 (where the centred lift changes sign), q0 - 1 and
    random ones; the call gets their forward transform"""
    logn, Lout, B = 8, K, 2
    n = 1 << logn
    c = ML.chain(logn)
    primes = [c[first]] + [c[name] for name in ML.NAMES if name != first]
    assert (primes[0] == max(primes)) if first == "g61" else (primes[0] == min(primes))
    octx, ctx = O.Context(logn, primes), moai.Context(logn, primes)
    _own.append(ctx)
    q0 = primes[0]
    rng = np.random.default_rng(6600 + len(first))
    coeff = O.uniform_rns(rng, primes[:1], (B, 2), n)
    edge = np.array([0, q0 // 2, q0 // 2 + 1, q0 - 1], dtype=np.uint64)
    coeff[0, 0, 0, :] = np.resize(edge, n)   # a whole polynomial on the edges
    coeff[0, 1, 0, :8] = np.resize(edge, 8)  # and the first chunks of a random one
    coeff[1, 0, 0, -4:] = edge
    x = octx.ntt(coeff, 1, prime_index=[0]).reshape(coeff.shape)  # the call takes NTT form: its INTT is `coeff`
    assert (octx.ntt(x, 1, prime_index=[0], inverse=True).reshape(coeff.shape) == coeff).all()
    dx = up(moai, x)
    do = moai.DeviceBuffer(B * 2 * Lout * n)
    ctx.modraise(dx, do, Lout, B)
    got = do.to_numpy((B, 2, Lout, n))
    for b in range(B):
        assert (got[b] == octx.modraise(x[b], Lout)).all(), b
    dx.free()
    do.free()
