"""The transforms, the key switch, mod-down / rescale and the hoisted rotations at the size limit of every arithmetic mode
(tests/mode_limits.py), at every tiled degree, bit for bit against the CPU oracle.  moai_arith_mode tells each test that the
rows it means to exercise are in the intended mode, so a knob default cannot quietly move them to another one.

Inputs carry the magnitudes the bounds are stated for: all q-1, all 0, alternating 0 / q-1, the balanced-digit boundary
q/2, q/2+1, and random.  Key-switch targets are built from coefficient patterns through the oracle's forward transform, so
that the digits carry the pattern.

Batches of the long-chain tests: the key-switch MAC splits its digit range over up to eight workgroups when few ciphertexts
leave the chip empty (csrc/keyswitch.hip ks_splits), and the FP64 folds count digits per split.  The folds at the 16th and
32nd digit therefore only run when batch * (L + 1) * N / 4096 reaches eight workgroups per compute unit; those tests repeat
two ciphertexts up to that batch (the oracle computes each once)."""
import numpy as np
import pytest

import mode_limits as ML
import oracle as O
from mode_limit_cases import (HOIST_STEPS, K, L8, MIXED_ROWS, ORDER_NAMES, contexts, hoist_case, ks_case, long_case, long_refs,
                              ntt_case, release, rescale_case, up)  # the case builders, shared with the small degrees
from mode_limits import FWD_CLASS, INV_CLASS  # the plain forward and inverse transforms

pytestmark = pytest.mark.gpu

LOGNS = [12, 13, 14, 15, 16]
ARITH = ["fp64", "int64"]

# ---- the written contract: the arithmetic class of every chain prime -------------------------------------------------------
# key switch and mod-down: (FP64 allowed, integer only); ng_hi subject to the rule on L
KS_CLASS = {
    "fpn_hi": ("FPN", "NOGUARD"), "fpr_lo": ("FPR", "NOGUARD"), "fpr_hi": ("FPR", "NOGUARD"), "int_lo": ("NOGUARD", "NOGUARD"),
    "ng_hi": ("NOGUARD", "NOGUARD"), "g_lo": ("GUARD", "GUARD"), "g60": ("GUARD", "GUARD"), "g61": ("GUARD", "GUARD"),
    "small": ("FPN", "NOGUARD"),
}


def code(moai, name):
    return getattr(moai.hip, "MODE_" + name)


def set_arith(moai, arith):
    """fp64: the FP64 modes from the first row on; int64: never (tests/test_gpu_parity.py ks_arith)"""
    moai.hip.set_tuning("MOAI_KS_FP_MIN_ROWS", 0 if arith == "fp64" else 1 << 40)
    moai.hip.set_tuning("MOAI_MD_FP_MIN_ROWS", 0 if arith == "fp64" else 1 << 40)


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    """the cached device contexts (nine-prime chains and the long chain) live as long as this module's tests, whichever ran"""
    yield
    release()
    _mixed.clear()


def assert_ks_modes(moai, ctx, names, L, batch, arith, expect=None):
    """every output modulus of a key switch at L data primes (the special prime included) is in its table class; returns the set"""
    col = 0 if arith == "fp64" else 1
    seen = set()
    for i in list(range(L)) + [len(names) - 1]:
        want = (expect or {}).get(names[i]) or KS_CLASS[names[i].rstrip("-")][col]
        got = ctx.arith_mode(i, moai.hip.MODE_OF_KEY_SWITCH, L, batch)
        assert got == code(moai, want), (names[i], want, got)
        seen.add(want)
    return seen


# ---- a. the mode query ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", LOGNS)
def test_mode_query_returns_the_table(moai, logn):
    H = moai.hip
    try:
        for order in ORDER_NAMES:
            primes, names, _, ctx = contexts(moai, logn, order)
            for col, arith in enumerate(ARITH):
                set_arith(moai, arith)
                for i, name in enumerate(names):
                    assert ctx.arith_mode(i, H.MODE_OF_KEY_SWITCH, L8, 2) == code(moai, KS_CLASS[name][col]), (order, arith, name)
                    assert ctx.arith_mode(i, H.MODE_OF_MOD_DOWN, 0, 4 * L8) == code(moai, KS_CLASS[name][col]), (order, arith, name)
            H.reset_tuning()
            # the thresholds count rows: key switch batch * L, mod-down polynomials * kept primes
            i = names.index("fpr_hi")
            H.set_tuning("MOAI_KS_FP_MIN_ROWS", 16)
            H.set_tuning("MOAI_MD_FP_MIN_ROWS", 256)
            assert ctx.arith_mode(i, H.MODE_OF_KEY_SWITCH, L8, 2) == H.MODE_FPR and ctx.arith_mode(i, H.MODE_OF_KEY_SWITCH, L8, 1) == H.MODE_NOGUARD
            assert ctx.arith_mode(i, H.MODE_OF_MOD_DOWN, 0, 256) == H.MODE_FPR and ctx.arith_mode(i, H.MODE_OF_MOD_DOWN, 0, 255) == H.MODE_NOGUARD
            for col, fp in enumerate((1, 0)):
                H.set_tuning("MOAI_NTT_FP", fp)
                H.set_tuning("MOAI_KS_FP_MIN_ROWS", 0)
                for i, name in enumerate(names):
                    assert ctx.arith_mode(i, H.MODE_OF_NTT_FORWARD) == code(moai, FWD_CLASS[name][col]), (order, fp, name)
                    assert ctx.arith_mode(i, H.MODE_OF_NTT_INVERSE) == code(moai, INV_CLASS[name][col]), (order, fp, name)
                    # MOAI_NTT_FP=0 takes the FP64 modes out of the key switch too
                    assert ctx.arith_mode(i, H.MODE_OF_KEY_SWITCH, L8, 2) == code(moai, KS_CLASS[name][col]), (order, fp, name)
            H.reset_tuning()
            # the knobs of the 60-bit transform
            i = names.index("g60")
            H.set_tuning("MOAI_NTT_LAZY16", 0)
            assert ctx.arith_mode(i, H.MODE_OF_NTT_FORWARD) == H.MODE_LAZY8 and ctx.arith_mode(i, H.MODE_OF_NTT_INVERSE) == H.MODE_LAZY8
            H.set_tuning("MOAI_NTT_LAZY8", 0)
            assert ctx.arith_mode(i, H.MODE_OF_NTT_FORWARD) == H.MODE_GUARD2 and ctx.arith_mode(i, H.MODE_OF_NTT_INVERSE) == H.MODE_GUARD
            H.reset_tuning()
        with pytest.raises(moai.MoaiError):
            ctx.arith_mode(K, H.MODE_OF_NTT_FORWARD)
        with pytest.raises(moai.MoaiError):
            ctx.arith_mode(0, 4)
    finally:
        H.reset_tuning()


@pytest.mark.parametrize("logn", [12, 16])
def test_noguard_key_switch_ends_at_36_digits(moai, logn):
    """36 q^2 L < 2^128: the prime just below 2^64 / 36 keeps the 128-bit lazy MAC up to L* = 36 and takes the guards at L* + 1"""
    H = moai.hip
    q = ML.chain(logn)["ng_hi"]
    Ls = ML.largest_noguard_L(q)
    assert 36 * q * q * Ls < 1 << 128 <= 36 * q * q * (Ls + 1) and Ls == 36
    primes, names = ML.long_chain(logn, Ls + 2)
    ctx = moai.Context(logn, primes)
    i = names.index("ng_hi")
    try:
        for arith in ARITH:
            set_arith(moai, arith)
            assert ctx.arith_mode(i, H.MODE_OF_KEY_SWITCH, Ls, 1) == H.MODE_NOGUARD
            assert ctx.arith_mode(i, H.MODE_OF_KEY_SWITCH, Ls + 1, 1) == H.MODE_GUARD
            assert ctx.arith_mode(i, H.MODE_OF_MOD_DOWN, 0, 1 << 20) == H.MODE_NOGUARD  # no MAC, no rule on L
    finally:
        H.reset_tuning()
        ctx.close()


# ---- b. the plain transforms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,fp", [(l, f) for l in LOGNS for f in (1, 0)])
def test_ntt_at_the_limits(moai, logn, fp):
    H = moai.hip
    c = ntt_case(logn)
    primes, names, _, ctx = contexts(moai, logn, "g61_last")
    qcol = np.array(primes, dtype=np.uint64)[None, :, None]
    H.set_tuning("MOAI_NTT_FP", fp)
    try:
        col = 0 if fp else 1
        inv_cls = []
        for i, name in enumerate(names):
            assert ctx.arith_mode(i, H.MODE_OF_NTT_FORWARD) == code(moai, FWD_CLASS[name][col]), name
            inv_cls.append(ctx.arith_mode(i, H.MODE_OF_NTT_INVERSE))
            assert inv_cls[-1] == code(moai, INV_CLASS[name][col]), name
        for p, pname in enumerate(ML.PATTERNS):
            x = c["x"][p]
            d = up(moai, x)
            ctx.ntt_forward(d, 2, K)
            assert (d.to_numpy(x.shape) == c["fwd"][p]).all(), "forward, " + pname
            ctx.ntt_inverse(d, 2, K)
            assert (d.to_numpy(x.shape) == x).all(), "round trip, " + pname
            ctx.ntt_inverse(d, 2, K)
            assert (d.to_numpy(x.shape) == c["inv"][p]).all(), "inverse, " + pname
            # forward: every row at the top of [0, 4q), as include/moai_hip.h promises
            d.upload(x + np.uint64(3) * qcol)
            ctx.ntt_forward(d, 2, K)
            assert (d.to_numpy(x.shape) == c["fwd"][p]).all(), "forward from the top of [0, 4q), " + pname
            # inverse: every row at the top of the range its class accepts (include/moai_hip.h, moai_ntt_inverse)
            lazy = x.copy()
            for i, q in enumerate(primes):
                if inv_cls[i] in (H.MODE_FPN, H.MODE_FPR):
                    lazy[:, i] += ((np.uint64((1 << 52) - 1) - x[:, i]) // np.uint64(q)) * np.uint64(q)
                    assert (lazy[:, i] < np.uint64(1 << 52)).all() and (lazy[:, i] + np.uint64(q) >= np.uint64(1 << 52)).all()
                else:
                    lazy[:, i] += np.uint64((3 if inv_cls[i] in (H.MODE_LAZY16, H.MODE_LAZY8) else 1) * q)
            d.upload(lazy)
            ctx.ntt_inverse(d, 2, K)
            assert (d.to_numpy(x.shape) == c["inv"][p]).all(), "inverse from the top of its input range, " + pname
            d.free()
    finally:
        H.reset_tuning()


# (2^12: a grid of n_poly * rows of a class workgroups, with 3 polynomials no multiple of 8 and with 8 polynomials one -- the two
# arms of the kernels' work-id map; 2^16: the degree with the twiddle copies in LDS and the larger inverse LDS array)
MIXED_SHAPES = [(12, 3), (12, 8), (16, 1)]
MIXED_KNOBS = {"fp": {"MOAI_NTT_FP": 1}, "int": {"MOAI_NTT_FP": 0}, "lazy8": {"MOAI_NTT_LAZY16": 0}}
_mixed = {}


def mixed_case(logn):
    """prime index per row, inputs [pattern][8 or 1][9][N] (polynomial j: the patterns j coefficients on) and the oracle's forward
    transform under that row selection; once per degree, the 3-polynomial case takes the first three"""
    if logn not in _mixed:
        n, npoly = 1 << logn, max(p for l, p in MIXED_SHAPES if l == logn)
        primes = ML.ordered(logn, "g61_last")
        pidx = [ML.ORDERS["g61_last"].index(name) for name in MIXED_ROWS]
        assert sorted(pidx) == list(range(K)) and pidx != list(range(K))
        pat = ML.pattern_rows([primes[i] for i in pidx], n, np.random.default_rng(5250 + logn))
        x = np.stack([np.roll(pat, j, axis=-1) for j in range(npoly)], axis=1)
        fwd = O.Context(logn, primes).ntt(x.reshape(-1, K, n), K, prime_index=pidx).reshape(x.shape)
        for v in (x, fwd):
            v.setflags(write=False)
        _mixed[logn] = (pidx, x, fwd)
    return _mixed[logn]


@pytest.mark.parametrize("logn,npoly,knobs", [(l, p, k) for l, p in MIXED_SHAPES for k in MIXED_KNOBS])
def test_ntt_interleaved_classes_and_permuted_primes(moai, logn, npoly, knobs):
    H = moai.hip
    pidx, x, fwd = mixed_case(logn)
    _, names, _, ctx = contexts(moai, logn, "g61_last")
    for knob, v in MIXED_KNOBS[knobs].items():
        H.set_tuning(knob, v)
    try:
        col = 1 if knobs == "int" else 0
        want = [[H.MODE_LAZY8 if knobs == "lazy8" and table[name][col] == "LAZY16" else code(moai, table[name][col]) for name in MIXED_ROWS]
                for table in (FWD_CLASS, INV_CLASS)]
        got = [[ctx.arith_mode(i, of) for i in pidx] for of in (H.MODE_OF_NTT_FORWARD, H.MODE_OF_NTT_INVERSE)]
        assert got == want
        if knobs == "fp":
            assert all((got[0][r], got[1][r]) != (got[0][r + 1], got[1][r + 1]) for r in range(K - 1)), "neighbours of one class pair"
            assert len(set(got[0])) == 5 and len(set(got[1])) == 4  # every class but the one MOAI_NTT_LAZY16=0 brings
        for p, pname in enumerate(ML.PATTERNS):
            xp = x[p, :npoly]
            d = up(moai, xp)
            ctx.ntt_forward(d, npoly, K, prime_index=pidx)
            assert (d.to_numpy(xp.shape) == fwd[p, :npoly]).all(), "forward, " + pname
            ctx.ntt_inverse(d, npoly, K, prime_index=pidx)
            assert (d.to_numpy(xp.shape) == xp).all(), "round trip, " + pname
            d.free()
    finally:
        H.reset_tuning()


# ---- c. the key switch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,order,arith", [(l, o, a) for l in LOGNS for o in ORDER_NAMES for a in ARITH])
def test_key_switch_at_the_limits(moai, logn, order, arith):
    n = 1 << logn
    primes, names, _, ctx = contexts(moai, logn, order)
    elt, cases = ks_case(moai, logn, order)
    set_arith(moai, arith)
    try:
        seen = assert_ks_modes(moai, ctx, names, L8, 2, arith)
        assert seen == ({"FPN", "FPR", "NOGUARD", "GUARD"} if arith == "fp64" else {"NOGUARD", "GUARD"})
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
    finally:
        moai.hip.reset_tuning()


# N = 2^16: the launch variants of the fused kernels.  The strided pass of an FP64 group runs eight tiles per workgroup,
# software-pipelined, from batch * members * L * 16 >= 16384 tiles on (csrc/keyswitch.hip ks_fused_group), where `members` counts
# the output moduli of that mode in one launch: two per FP64 mode on this chain, so 64 ciphertexts.  "default" is that kernel,
# MOAI_KS_P1_ITEMS=1 the one tile per workgroup that few ciphertexts take anyway, and a scratch budget of one modulus per launch
# (G = 1) leaves too few tiles by design.
# variant: (knobs, moduli of one mode per launch at most -- None: all of them --, pipelined strided pass expected)
KS_VARIANTS = {
    "default": ({}, None, True),
    "p1_items_1": ({"MOAI_KS_P1_ITEMS": 1}, None, False),
    "tmp_mb_g1": ({"MOAI_KS_TMP_MB": 1}, 1, False),
}
KS_VARIANT_BATCH = 64


@pytest.mark.parametrize("variant", list(KS_VARIANTS))
def test_key_switch_launch_variants_at_2_16(moai, variant):
    H = moai.hip
    logn, order, B = 16, "g61_last", KS_VARIANT_BATCH
    n = 1 << logn
    knobs, group_cap, pipelined = KS_VARIANTS[variant]
    primes, names, _, ctx = contexts(moai, logn, order)
    _, cases = ks_case(moai, logn, order)
    set_arith(moai, "fp64")
    for knob, v in knobs.items():
        H.set_tuning(knob, v)
    try:
        assert assert_ks_modes(moai, ctx, names, L8, B, "fp64") == {"FPN", "FPR", "NOGUARD", "GUARD"}
        # the launcher's own condition, per FP64 mode, with the members the query counts
        for mode in (H.MODE_FPN, H.MODE_FPR):
            members = sum(ctx.arith_mode(i, H.MODE_OF_KEY_SWITCH, L8, B) == mode for i in list(range(L8)) + [K - 1])
            assert members == 2
            members = min(members, group_cap or members)
            takes_it = B * members * L8 * (n >> 12) >= 8 * 2048 and knobs.get("MOAI_KS_P1_ITEMS", 8) > 1
            assert takes_it == pipelined, (variant, mode, members)
        # the all q-1 key with its two ciphertexts, then the random key with the four of the other two inputs, repeated up to B
        for group in (cases[:1], cases[1:]):
            assert all(c["key"] is group[0]["key"] for c in group)
            dkey = up(moai, group[0]["key"])
            ct = np.concatenate([c["ct"] for c in group])
            tgt = np.concatenate([c["tgt"] for c in group])
            ref = np.concatenate([c["sk"] for c in group])
            reps = B // len(ct)
            d, dt = up(moai, np.tile(ct, (reps, 1, 1, 1))), up(moai, np.tile(tgt, (reps, 1, 1)))
            ctx.switch_key(d, dt, dkey, L8, B)
            got = d.to_numpy((reps,) + ref.shape)
            for b in (d, dt, dkey):
                b.free()
            assert (got == ref[None]).all(), [c["name"] for c in group]
    finally:
        H.reset_tuning()


# ---- d. rescale and mod-down --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,arith", [(l, a) for l in LOGNS for a in ARITH])
def test_rescale_at_the_limits(moai, logn, arith):
    H = moai.hip
    n = 1 << logn
    c = rescale_case(moai, logn)
    set_arith(moai, arith)
    col = 0 if arith == "fp64" else 1
    try:
        dropped = set()
        for order in ORDER_NAMES:
            primes, names, _, ctx = contexts(moai, logn, order)
            for L in range(K, 1, -1):
                for i in range(L - 1):
                    assert ctx.arith_mode(i, H.MODE_OF_MOD_DOWN, 0, 4 * (L - 1)) == code(moai, KS_CLASS[names[i]][col]), (order, L, names[i])
                assert ctx.arith_mode(L - 1, H.MODE_OF_NTT_INVERSE) == code(moai, INV_CLASS[names[L - 1]][0])  # the row mod-down inverts
                dropped.add(names[L - 1])
                x, ref = c[(order, L)]
                dx = up(moai, x)
                do = moai.DeviceBuffer(2 * 2 * (L - 1) * n)
                ctx.rescale(dx, do, 2, L, 2)
                assert (do.to_numpy(ref.shape) == ref).all(), (order, L, "dropped " + names[L - 1])
                if order == "g61_last" and L == K:
                    ctx.mul_scalar_rescale(dx, [q - 1 for q in primes], do, 2, L, 2)
                    assert (do.to_numpy(ref.shape) == c["scalar"]).all(), "mul_scalar_rescale"
                dx.free()
                do.free()
        assert dropped == set(ML.NAMES)  # every prime was the dropped one
    finally:
        H.reset_tuning()


# ---- e. hoisted rotations -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,arith", [(l, a) for l in [13, 14, 15, 16] for a in ARITH])
def test_hoisted_rotations_at_the_limits(moai, logn, arith):
    n = 1 << logn
    primes, names, _, ctx = contexts(moai, logn, "g61_last")
    elts, keys, ct, ref = hoist_case(moai, logn)
    R = len(elts)
    dkeys = [up(moai, kk) for kk in keys]
    try:
        set_arith(moai, arith)
        assert_ks_modes(moai, ctx, names, L8, 2, arith)
        corrs = [ctx.hoist_correction(dk, e, L8) for dk, e in zip(dkeys, elts)]
        dct = up(moai, ct)
        dout = moai.DeviceBuffer(R * 2 * 2 * L8 * n)
        for per_pass in (4, 2, 0):
            moai.hip.set_tuning("MOAI_KS_HOIST_PAIR", per_pass)
            assert not ctx.apply_galois_hoisted(dct, dout, L8, elts, dkeys, corrs, 2), "fallback taken"
            got = dout.to_numpy(ref.shape)
            for r in range(R):
                assert (got[r] == ref[r]).all(), (per_pass, HOIST_STEPS[r])
        for b in corrs + [dct, dout]:
            b.free()
    finally:
        moai.hip.reset_tuning()
        for b in dkeys:
            b.free()


# ---- f. long chains: where the accumulation bounds bind ----------------------------------------------------------------------


def fold_batch(moai, logn, L):
    """the smallest batch that leaves the MAC's digit range in one piece (csrc/keyswitch.hip ks_splits: eight workgroups per CU)"""
    cus = moai.hip.device_info()[1]
    per_ct = (L + 1) << (logn - 12)
    return max(1, -(-8 * cus // per_ct))


def run_long(moai, logn, k, L, arith, expect):
    c = long_case(moai, logn, k)
    ctx, names, n = c["ctx"], c["names"], 1 << logn
    B = fold_batch(moai, logn, L)
    set_arith(moai, arith)
    try:
        seen = assert_ks_modes(moai, ctx, names, L, B, arith, expect)
        assert seen >= ({"FPN", "FPR", "NOGUARD", "GUARD"} if arith == "fp64" else {"NOGUARD", "GUARD"})
        for key, (ct, tgt, ref) in zip(c["keys"], long_refs(c, L)):
            dkey = up(moai, key)
            d, dt = up(moai, np.tile(ct, (B, 1, 1, 1))), up(moai, np.tile(tgt, (B, 1, 1)))
            ctx.switch_key(d, dt, dkey, L, B)
            got = d.to_numpy((B, 2, L, n))
            for b in (d, dt, dkey):
                b.free()
            assert (got == ref[None]).all(), (L, B)
    finally:
        moai.hip.reset_tuning()


@pytest.mark.parametrize("L,arith", [(L, a) for L in (17, 36, 37) for a in ARITH])
def test_long_chain_key_switch_2_12(moai, L, arith):
    """L = 17: the M_FPN fold at the 16th digit; L* = 36: its second fold at the 32nd, M_FPR folds throughout, and the last L at
    which the 128-bit lazy MAC of the primes just below 2^64 / 36 is admissible; L* + 1: their first guarded L"""
    Ls = ML.largest_noguard_L(ML.chain(12)["ng_hi"])
    assert Ls == 36
    near = {"ng_hi": "GUARD", "ng_hi-": "GUARD"} if L > Ls else None
    run_long(moai, 12, Ls + 2, L, arith, near)


@pytest.mark.parametrize("arith", ARITH)
def test_long_chain_key_switch_2_16(moai, arith):
    """sixteen-stage digits -- the values "below 33 q" that M_FPN leaves unreduced -- enter the FP64 MAC and meet its first fold"""
    run_long(moai, 16, 18, 17, arith, None)
