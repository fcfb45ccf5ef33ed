"""GPU tests of the exact rounding mode of the hybrid mod-downs (include/moai_hip.h, "hybrid rounding mode": moai_hybrid_set_rounding,
moai_hybrid_rounding).  Unless said otherwise the device is compared bit for bit with tests/hybrid_exact_ref.py (pinned by
tests/test_hybrid_exact_cpu.py), and every test leaves its context in MOAI_HYBRID_ROUND_FAST.

1. The mode API: the default, set and query, the refusals, the exports.
2. Switch, relinearize, rotation: alpha = 2 (N = 1024) at L = 5, 4, 1, alpha = 3 (N = 4096) at L = 7, 4; at alpha = 1 exact = fast = the
   existing restatement.
3. The merged rescale and its product form, the same environments, L >= 2.
4. The hoisted rotations, the plaintext-weighted sums and the BSGS sum against the patched restatements.
5. Every instantiation of the conversion kernel: 1, 2, 3 (4), 6 and 7 (8), and 16 sources on 61-bit primes for the switch (alpha = 16)
   and the rescale (alpha = 15), with the key all m - 1 and the input all q - 1, and one random case, at N = 1024 and N = 4096.
6. Directed boundaries: the accumulator is built so that X' hits 0, 1, 2, W-2, W-1, H-1, H, H+1.
7. The default is isolated: exact, then fast on the same context and cached tables is hybrid_ref again.
8. A scratch budget of one ciphertext gives the same bits.
9. The list forms in exact mode are the single calls in exact mode.
10. At MOAI's parameters (N = 2^16, 35 + 12 primes, l = 35) fast - exact is one integer per coefficient in [-(alpha - 1), 0] ([-alpha, 0]
    for the merged rescale), the same in every row, and not zero everywhere."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import hybrid_bsgs_ref as HB
import hybrid_dot_ref as HD
import hybrid_exact_ref as HX
import hybrid_hoist_ref as HH
import hybrid_ref as HR
import hybrid_rescale_ref as RR
import mode_limits as ML
import oracle as O
from hybrid_kit import EINVAL, IDENT, MOAI_DATA_BITS, OK, PATTERN, Env, cached, exported, tuned
from hybrid_kit import env_small1, env_small2, env_tiled1, env_tiled3  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

FAST, EXACT = 0, 1
KEY = bytes(range(1, 33))


@contextlib.contextmanager
def exact(e):
    """the block runs in MOAI_HYBRID_ROUND_EXACT; the context is back in the default afterwards, whatever happened"""
    try:
        e.ctx.hybrid_set_rounding(EXACT)
        yield
    finally:
        e.ctx.hybrid_set_rounding(FAST)


def key_of(e):
    def make():
        k = O.uniform_rns(np.random.default_rng(e.logn * 100 + e.alpha + 7), e.primes, (e.digits, 2), e.n)
        return k, e.up(k)
    return cached(e.cache, "exact key", make)


def run_switch(e, ct, target, dkey, L):
    B = len(ct)
    d = e.up(ct)
    e.ctx.switch_key_hybrid(d, e.up(target), dkey, L, e.alpha, B)
    return d.to_numpy((B, 2, L, e.n))


def run_rescale(e, ct3, dkey, L):
    B = len(ct3)
    out = e.filled((B, 2, L - 1, e.n), PATTERN)
    e.ctx.relinearize_rescale_hybrid(e.up(ct3), dkey, out, L, e.alpha, B)
    return out.to_numpy((B, 2, L - 1, e.n))


# ---- 1. the mode API ------------------------------------------------------------------------------------------------------------------
def test_mode_api(moai, env_small2):
    e, lib = env_small2, moai.hip.lib()
    exported(moai, ["moai_hybrid_set_rounding", "moai_hybrid_rounding"], ["hybrid_set_rounding", "hybrid_rounding"])
    try:
        assert e.ctx.hybrid_rounding() == FAST  # the default
        fresh = moai.Context(e.logn, e.primes)
        assert fresh.hybrid_rounding() == FAST
        fresh.close()
        e.ctx.hybrid_set_rounding(EXACT)
        assert e.ctx.hybrid_rounding() == EXACT
        moai.hip.reset_tuning()  # not a tuning knob
        assert e.ctx.hybrid_rounding() == EXACT
        mode = C.c_int(7)
        for call, text in ((lambda: lib.moai_hybrid_set_rounding(None, EXACT), b"null context"),
                           (lambda: lib.moai_hybrid_rounding(None, C.byref(mode)), b"null context"),
                           (lambda: lib.moai_hybrid_rounding(e.ctx.h, None), b"null mode"),
                           (lambda: lib.moai_hybrid_set_rounding(e.ctx.h, 2), b"rounding mode 2"),
                           (lambda: lib.moai_hybrid_set_rounding(e.ctx.h, -1), b"rounding mode -1")):
            assert call() == EINVAL and text in lib.moai_last_error(), text
        assert mode.value == 7 and e.ctx.hybrid_rounding() == EXACT  # a refusal changes nothing
        with pytest.raises(moai.MoaiError):
            e.ctx.hybrid_set_rounding(5)
        e.ctx.hybrid_set_rounding(FAST)
        assert e.ctx.hybrid_rounding() == FAST and OK == 0
    finally:
        e.ctx.hybrid_set_rounding(FAST)


# ---- 2. switch, relinearize, rotation ---------------------------------------------------------------------------------------------
def check_switches(e, L, B):
    """switch (with a target of m - 1 and one of zero from B = 3 on), relinearize and rotation of the same operands"""
    n = e.n
    rng = np.random.default_rng(e.logn * 100 + e.alpha * 10 + L)
    key, dkey = key_of(e)
    ct3 = O.uniform_rns(rng, e.primes[:L], (B, 3), n)
    if B >= 3:
        ct3[1, 2], ct3[2, 2] = e.edge_targets(L)
    elt = e.elts([3])[0]
    with exact(e):
        got = run_switch(e, ct3[:, :2], ct3[:, 2], dkey, L)
        out = e.filled((B, 2, L, n), PATTERN)
        e.ctx.relinearize_hybrid(e.up(ct3), dkey, out, L, e.alpha, B)
        rot = e.up(ct3[:, :2])
        e.ctx.apply_galois_hybrid(rot, L, e.alpha, elt, dkey, B)
    relin, rot = out.to_numpy((B, 2, L, n)), rot.to_numpy((B, 2, L, n))
    differs = False
    for b in range(B):
        want = HX.switch_key(e.octx, ct3[b, :2], ct3[b, 2], key, L, e.alpha)
        assert (got[b] == want).all(), b
        assert (relin[b] == want).all(), b  # relinearize is that switch
        assert (rot[b] == HX.apply_galois(e.octx, ct3[b, :2], L, elt, key, e.alpha)).all(), b
        fast = HR.switch_key(e.octx, ct3[b, :2], ct3[b, 2], key, L, e.alpha)
        differs = differs or (want != fast).any()
        if e.alpha == 1:
            assert (want == fast).all()  # exact = fast = the existing restatement
    assert differs == (e.alpha > 1)  # an implementation that leaves u in gives the fast bits


@pytest.mark.parametrize("L", [5, 4, 1])
def test_switches_alpha_2_small_transform(env_small2, L):
    check_switches(env_small2, L, 3)


@pytest.mark.parametrize("L", [7, 4])
def test_switches_alpha_3_tiled_transform(env_tiled3, L):
    check_switches(env_tiled3, L, 2)


@pytest.mark.parametrize("which", ["small", "tiled"])
def test_switches_alpha_1_are_the_fast_ones(env_small1, env_tiled1, which):
    e = env_small1 if which == "small" else env_tiled1
    check_switches(e, e.lmax, 3)


# ---- 3. the merged rescale --------------------------------------------------------------------------------------------------------
def check_rescale(e, L, B):
    rng = np.random.default_rng(e.logn * 100 + e.alpha * 10 + L + 1)
    key, dkey = key_of(e)
    ct3 = O.uniform_rns(rng, e.primes[:L], (B, 3), e.n)
    x, y = O.uniform_rns(rng, e.primes[:L], (B, 2), e.n), O.uniform_rns(rng, e.primes[:L], (B, 2), e.n)
    with exact(e):
        got = run_rescale(e, ct3, dkey, L)
        out = e.filled((B, 2, L - 1, e.n), PATTERN)
        e.ctx.multiply_relin_rescale_hybrid(e.up(x), e.up(y), dkey, out, L, e.alpha, B)
    prod = out.to_numpy((B, 2, L - 1, e.n))
    for b in range(B):
        want = HX.relinearize_rescale(e.octx, ct3[b], key, L, e.alpha)
        assert (got[b] == want).all(), b
        assert (want != RR.relinearize_rescale(e.octx, ct3[b], key, L, e.alpha)).any()  # two sources already at alpha = 1
        assert (prod[b] == HX.multiply_relin_rescale(e.octx, x[b], y[b], key, L, e.alpha)).all(), b


@pytest.mark.parametrize("L", [5, 4, 2])
def test_rescale_alpha_2_small_transform(env_small2, L):
    check_rescale(env_small2, L, 3)


@pytest.mark.parametrize("L", [7, 4])
def test_rescale_alpha_3_tiled_transform(env_tiled3, L):
    check_rescale(env_tiled3, L, 2)


@pytest.mark.parametrize("which", ["small", "tiled"])
def test_rescale_alpha_1(env_small1, env_tiled1, which):
    e = env_small1 if which == "small" else env_tiled1
    check_rescale(e, e.lmax, 2)


# ---- 4. the hoisted and BSGS forms against the patched restatements -----------------------------------------------------------------
STEPS = [1, 0, IDENT]  # a rotation, the conjugation, the identity


def check_hoisted_forms(e, L, B):
    n = e.n
    rng = np.random.default_rng(e.logn * 100 + e.alpha * 10 + L + 2)
    elts = e.elts(STEPS)
    keys = [None if elt == 1 else e.random_key(rng) for elt in elts]
    dkeys = [None if k is None else e.up(k) for k in keys]
    corrs = [None if k is None else e.ctx.hybrid_hoist_correction(k, elt, L, e.alpha) for k, elt in zip(dkeys, elts)]
    ct = e.random_input(rng, L, B)
    dct = e.up(ct)
    plains = [[O.uniform_rns(rng, e.rows(L), (), n) for _ in elts] for _ in range(2)]
    plains[1][0] = None
    dplains = [[None if p is None else e.up(p) for p in row] for row in plains]
    giant = e.elts([IDENT, 4])
    gkeys = [None, e.random_key(rng)]
    dgkeys = [None, e.up(gkeys[1])]
    with exact(e):
        hoisted = e.filled((2, B, 2, L, n), PATTERN)
        assert not e.ctx.apply_galois_hybrid_hoisted(dct, hoisted, L, e.alpha, elts[:2], dkeys[:2], corrs[:2], B)
        dots = e.filled((2, B, 2, L, n), PATTERN)
        assert not e.ctx.hybrid_rotate_pt_dot(dct, dots, L, e.alpha, elts, dkeys, corrs, dplains, B)
        bsgs = e.filled((B, 2, L, n), PATTERN)
        assert not e.ctx.hybrid_bsgs_dot(dct, bsgs, L, e.alpha, elts, dkeys, corrs, giant, dgkeys, dplains, B)
    hoisted, dots, bsgs = hoisted.to_numpy((2, B, 2, L, n)), dots.to_numpy((2, B, 2, L, n)), bsgs.to_numpy((B, 2, L, n))
    assert (dct.to_numpy(ct.shape) == ct).all()
    with HX.patched():
        for b in range(B):
            assert (hoisted[:, b] == HH.apply_galois_hoisted(e.octx, ct[b], L, elts[:2], keys[:2], e.alpha)).all(), b
            assert (dots[:, b] == HD.rotate_pt_dot(e.octx, ct[b], L, e.alpha, elts, keys, plains)).all(), b
            assert (bsgs[b] == HB.bsgs_dot(e.octx, ct[b], L, e.alpha, elts, keys, giant, gkeys, plains)).all(), b
    assert (bsgs[0] != HB.bsgs_dot(e.octx, ct[0], L, e.alpha, elts, keys, giant, gkeys, plains)).any()  # not the fast bits


def test_hoisted_forms_alpha_2_small_transform(env_small2):
    check_hoisted_forms(env_small2, 5, 2)


def test_hoisted_forms_alpha_3_tiled_transform(env_tiled3):
    check_hoisted_forms(env_tiled3, 4, 1)


# ---- 5. every instantiation of the conversion ---------------------------------------------------------------------------------------
def test_six_and_seven_sources(moai):
    """alpha = 6: six sources in step 5 and seven in the merged mod-down, the instantiation for up to eight"""
    e = Env(moai, 10, [40] * 7, [50] * 6)
    try:
        check_switches(e, 7, 1)
        check_rescale(e, 7, 1)
    finally:
        e.close()


def limit_operands(e, L):
    """the key all m - 1 and the input all q - 1"""
    key = np.empty((e.digits, 2, e.k, e.n), dtype=np.uint64)
    for r, m in enumerate(e.primes):
        key[:, :, r, :] = m - 1
    ct3 = np.empty((1, 3, L, e.n), dtype=np.uint64)
    for i in range(L):
        ct3[:, :, i, :] = e.primes[i] - 1
    return key, ct3


@pytest.mark.parametrize("logn", [10, 12])
@pytest.mark.parametrize("form", ["switch", "rescale"])
def test_sixteen_sources_on_61_bit_primes(moai, form, logn):
    """L = 2: the switch at alpha = 16 converts sixteen special primes, the rescale at alpha = 15 q_1 and fifteen"""
    alpha = 16 if form == "switch" else 15
    g61 = ML.chain(logn)["g61"]
    primes = [g61] + ML.primes_below(logn, g61, alpha + 1)
    assert all(p >> 60 == 1 for p in primes)
    e = Env(moai, logn, primes=primes, alpha=alpha)
    L = 2
    assert len(HX.bases(e.octx, L, alpha, form == "rescale")[0]) == 16
    try:
        rng = np.random.default_rng(logn + alpha)
        cases = [limit_operands(e, L), (e.random_key(rng), O.uniform_rns(rng, e.primes[:L], (1, 3), e.n))]
        for i, (key, ct3) in enumerate(cases):
            with exact(e):
                if form == "switch":
                    got = run_switch(e, ct3[:, :2], ct3[:, 2], e.up(key), L)[0]
                    want, fast = (f(e.octx, ct3[0, :2], ct3[0, 2], key, L, alpha) for f in (HX.switch_key, HR.switch_key))
                else:
                    got = run_rescale(e, ct3, e.up(key), L)[0]
                    want, fast = (f(e.octx, ct3[0], key, L, alpha) for f in (HX.relinearize_rescale, RR.relinearize_rescale))
            assert (got == want).all(), i
            assert (want != fast).any(), i
    finally:
        e.close()


# ---- 6. directed boundaries ---------------------------------------------------------------------------------------------------------
def check_boundaries(e, rescale):
    """The accumulator of a single-digit switch of the constant 1 is g (*) key digit 0, g the digit's converted constant under each row
    (1 where the digit has one prime: it converts exactly).  So the key is built row by row as g^-1 times the residues of integers Z
    whose X' are the targets, with c_0 = c_1 = 0; the restatement says what Z really was."""
    L = 2 if rescale else 1
    octx, n, alpha = e.octx, e.n, e.alpha
    assert alpha >= 2 and HR.beta(L, alpha) == 1
    rows = HH.rows_of(octx, L, alpha)
    src, ntgt = HX.bases(octx, L, alpha, rescale)
    W = HR._prod(e.primes[r] for r in src)
    H, Qlo = W // 2, HR._prod(e.primes[:ntgt])
    targets = [0, 1, 2, W - 2, W - 1, H - 1, H, H + 1]
    ct3 = np.zeros((1, 3, L, n), dtype=np.uint64)
    ct3[0, 2] = 1  # the constant 1 in NTT form
    ones = np.ones((e.digits, 2, e.k, n), dtype=np.uint64)
    g = RR.lifted(octx, ct3[0], ones, L, alpha)[0, :, 0]  # with the all-ones key the accumulator is g itself
    rng = np.random.default_rng(600 + rescale)
    key = np.zeros((e.digits, 2, e.k, n), dtype=np.uint64)
    want = [targets[c % 8] for c in range(n)]
    for p in range(2):
        z = [int(rng.integers(0, 1 << 62)) % Qlo * W + (x - H) % W for x in want]
        coef = np.stack([HR._u64(np.array([v % e.primes[r] for v in z], dtype=object)) for r in rows])
        Zrows = octx.ntt(coef, len(rows), prime_index=rows)
        for t, r in enumerate(rows):
            m = e.primes[r]
            key[0, p, r] = HR._u64(HR._obj(Zrows[t]) * pow(int(g[t]), -1, m) % m)
    Z = RR.lifted(octx, ct3[0], key, L, alpha)
    for p in range(2):
        diag = {}
        HX.mod_down_rows(octx, Z[p], L, alpha, rescale=rescale, diag=diag)
        assert list(diag["X"]) == want, p  # the accumulator hit its targets
        print("%s p %d: v - v* over the eight targets: %s" % ("rescale" if rescale else "switch", p,
                                                               [int(diag["v"][c]) - int(diag["vstar"][c]) for c in range(8)]))
    with exact(e):
        if rescale:
            got = run_rescale(e, ct3, e.up(key), L)[0]
            assert (got == HX.relinearize_rescale(octx, ct3[0], key, L, alpha, Z=Z)).all()
        else:
            got = run_switch(e, ct3[:, :2], ct3[:, 2], e.up(key), L)[0]
            assert (got == HX.switch_key(octx, ct3[0, :2], ct3[0, 2], key, L, alpha)).all()
    for p in range(2):
        err, _ = HX.quotient_error(octx, Z[p], got[p], L, alpha, rescale)
        assert HX.within_half(err, W).all(), p


@pytest.mark.parametrize("rescale", [False, True])
def test_boundaries_alpha_2(env_small2, rescale):
    check_boundaries(env_small2, rescale)


@pytest.mark.parametrize("rescale", [False, True])
def test_boundaries_alpha_3(env_tiled3, rescale):
    check_boundaries(env_tiled3, rescale)


# ---- 7. the default is isolated -------------------------------------------------------------------------------------------------------
def test_fast_after_exact_is_the_default_restatement(env_small2):
    e, L, B = env_small2, 5, 2
    rng = np.random.default_rng(70)
    key, dkey = key_of(e)
    ct3 = O.uniform_rns(rng, e.primes[:L], (B, 3), e.n)
    with exact(e):
        first = run_switch(e, ct3[:, :2], ct3[:, 2], dkey, L), run_rescale(e, ct3, dkey, L)
    second = run_switch(e, ct3[:, :2], ct3[:, 2], dkey, L), run_rescale(e, ct3, dkey, L)  # the same context and cached tables
    for b in range(B):
        assert (first[0][b] == HX.switch_key(e.octx, ct3[b, :2], ct3[b, 2], key, L, e.alpha)).all()
        assert (second[0][b] == HR.switch_key(e.octx, ct3[b, :2], ct3[b, 2], key, L, e.alpha)).all()
        assert (first[1][b] == HX.relinearize_rescale(e.octx, ct3[b], key, L, e.alpha)).all()
        assert (second[1][b] == RR.relinearize_rescale(e.octx, ct3[b], key, L, e.alpha)).all()


# ---- 8. the scratch budget ------------------------------------------------------------------------------------------------------------
def test_a_budget_of_one_ciphertext_gives_the_same_bits(moai, env_small2):
    """L = 5, alpha = 2, beta = 3: 49 rows of 8 KiB per switch and 37 per merged rescale; 400 KiB hold one of either, not two"""
    e, L, B = env_small2, 5, 3
    rng = np.random.default_rng(80)
    _, dkey = key_of(e)
    ct3 = O.uniform_rns(rng, e.primes[:L], (B, 3), e.n)
    with exact(e):
        whole = run_switch(e, ct3[:, :2], ct3[:, 2], dkey, L), run_rescale(e, ct3, dkey, L)
        with tuned(moai, MOAI_HYBRID_TMP_KB=400):
            parts = run_switch(e, ct3[:, :2], ct3[:, 2], dkey, L), run_rescale(e, ct3, dkey, L)
    assert (parts[0] == whole[0]).all() and (parts[1] == whole[1]).all()
    assert (whole[0][2] == HX.switch_key(e.octx, ct3[2, :2], ct3[2, 2], key_of(e)[0], L, e.alpha)).all()


# ---- 9. the list forms ------------------------------------------------------------------------------------------------------------------
def test_list_forms_are_the_single_calls(moai, env_small2):
    e, L, n = env_small2, 4, env_small2.n
    rng = np.random.default_rng(90)
    key, dkey = key_of(e)
    ct3 = O.uniform_rns(rng, e.primes[:L], (3, 3), n)
    elts = e.elts([1, 3, 0])
    with exact(e):
        single_rot, single_relin, single_resc = [], [], []
        for i in range(3):
            d = e.up(ct3[i, :2])
            e.ctx.apply_galois_hybrid(d, L, e.alpha, elts[i], dkey, 1)
            single_rot.append(d.to_numpy((2, L, n)))
            out = e.filled((2, L, n), PATTERN)
            e.ctx.relinearize_hybrid(e.up(ct3[i]), dkey, out, L, e.alpha, 1)
            single_relin.append(out.to_numpy((2, L, n)))
            single_resc.append(run_rescale(e, ct3[i:i + 1], dkey, L)[0])
        ins, ins3 = [e.up(ct3[i, :2]) for i in range(3)], [e.up(ct3[i]) for i in range(3)]
        outs = [e.filled((2, L, n), PATTERN) for _ in range(3)]
        e.ctx.apply_galois_hybrid_ptrs(ins, outs, L, e.alpha, elts, [dkey] * 3)
        list_rot = [o.to_numpy((2, L, n)) for o in outs]
        e.ctx.relinearize_hybrid_ptrs(ins3, outs, dkey, L, e.alpha)
        list_relin = [o.to_numpy((2, L, n)) for o in outs]
        outs = [e.filled((2, L - 1, n), PATTERN) for _ in range(3)]
        e.ctx.relinearize_rescale_hybrid_ptrs(ins3, outs, dkey, L, e.alpha)
        list_resc = [o.to_numpy((2, L - 1, n)) for o in outs]
        to, acc = e.filled((2, L, n), PATTERN), e.up(ct3[1, :2])
        e.ctx.apply_galois_hybrid_to(ins[0], to, L, e.alpha, elts[0], dkey, 1)
        e.ctx.apply_galois_hybrid_acc(ins[0], acc, L, e.alpha, elts[0], dkey, 1)
    for i in range(3):
        assert (list_rot[i] == single_rot[i]).all() and (list_relin[i] == single_relin[i]).all() and (list_resc[i] == single_resc[i]).all(), i
    assert (single_rot[0] == HX.apply_galois(e.octx, ct3[0, :2], L, elts[0], key, e.alpha)).all()  # and they are exact ones
    assert (to.to_numpy((2, L, n)) == single_rot[0]).all()
    q = np.array(e.primes[:L], dtype=np.uint64).reshape(1, L, 1)
    assert (acc.to_numpy((2, L, n)) == (single_rot[0] + ct3[1, :2]) % q).all()


# ---- 10. the device against itself at MOAI's parameters -----------------------------------------------------------------------------------
def centred_rows(e, diff, polys, rows):
    """a difference of two results [polys][rows][N] (NTT form, on the device) as centred integers in coefficient form"""
    e.ctx.ntt_inverse(diff, polys, rows)
    r = diff.to_numpy((polys, rows, e.n)).astype(np.int64)
    q = np.array(e.primes[:rows], dtype=np.int64).reshape(1, rows, 1)
    return np.where(r > q // 2, r - q, r)


def test_fast_minus_exact_at_moais_parameters(moai):
    """no restatement at this size: fast = exact - u with the fast conversion's overflow u in [0, alpha) ([0, alpha] with alpha + 1 sources)"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12, oracle=False)
    try:
        ctx, n, k, L, alpha = e.ctx, e.n, e.k, 35, 12
        sk = ctx.sample_ternary(KEY, 3 << 40, 1, k)
        ctx.ntt_forward(sk, 1, k)
        new = moai.DeviceBuffer(k * n)
        ctx.dyadic_mul(sk, sk, new, 1, 1, k)
        key = ctx.hybrid_keygen(KEY, 1000, sk, new, alpha)
        ct3 = e.up(O.uniform_rns(np.random.default_rng(35), e.primes[:L], (1, 3), n))
        res = {}
        for mode in (FAST, EXACT):
            try:
                ctx.hybrid_set_rounding(mode)
                sw, rs = moai.DeviceBuffer(2 * L * n), moai.DeviceBuffer(2 * (L - 1) * n)
                ctx.relinearize_hybrid(ct3, key, sw, L, alpha, 1)
                ctx.relinearize_rescale_hybrid(ct3, key, rs, L, alpha, 1)
                res[mode] = sw, rs
            finally:
                ctx.hybrid_set_rounding(FAST)
        for which, rows, low in ((0, L, -(alpha - 1)), (1, L - 1, -alpha)):
            diff = moai.DeviceBuffer(2 * rows * n)
            ctx.sub(res[FAST][which], res[EXACT][which], diff, 2, rows)
            d = centred_rows(e, diff, 2, rows)
            print("%s: fast - exact in [%d, %d], nonzero in %d of %d coefficients"
                  % (("switch", "rescale")[which], d.min(), d.max(), np.count_nonzero(d[:, 0]), d[:, 0].size))
            assert (d == d[:, :1]).all()  # one integer per coefficient, the same in every row
            assert d.min() >= low and d.max() <= 0
            assert d.any()
    finally:
        e.close()
