"""The hybrid key switch, its hoisted rotations and the shared mod-down (csrc/hybrid.hip, csrc/rowlaunch.h) at the size limit of every
arithmetic mode, bit for bit against the integer restatements tests/hybrid_ref.py and tests/hybrid_hoist_ref.py (pinned at these
primes by tests/test_hybrid_limits_cpu.py).  Chains and inputs come from tests/mode_limits.py (hybrid_chain, worst_coeff).

The bounds the kernels' comments state, and the case that reaches each:
    hy_convert_kernel<16>: 16 products below 2^122 per sum     test_wide_digits_at_61_bits[16-*]: sixteen 61-bit sources with scaled
                                                               residues q_r - 1 (worst_coeff) into 61-bit targets
    hy_mac_kernel: 63 products below 2^122                     test_63_digits_switch: alpha = 1, L = 63, 61-bit primes, key all m - 1;
                                                               the NTT-form target of all q - 1 makes every product of the first
                                                               row (q_j - 1) (m - 1), the largest sum there is
    hy_hoisted_mac_kernel, hy_hoist_correction_kernel: 63      test_63_digits_correction_and_hoisted
    hy_mod128 for ANY 128-bit value                            sources above the target: special_small's mod-up (61-bit sources into
                                                               the prime above 2^40) and special_large's mod-down; sources below
                                                               the target: special_small's mod-down (P far below every 61-bit q)
a. every test on a tiled degree asserts the transform class of every row of its chain under the knobs in force
b. switch_key_hybrid on special_large / special_small at every degree (2^10: the small transform, which copies the mod-down's source
   slice first; 2^12..2^16: the tiled kernels, one instantiation per degree), full and partial digits
c. relinearize_hybrid (source slice of stride 3L, offset 2L), apply_galois_hybrid, hybrid_keygen
d. digits of 2, 4, 8, 16 61-bit primes     e. 63 digits     f. hoisted rotations against the restatement itself     g. schedules

Targets are built from coefficient patterns through the oracle's forward transform, so that the digits carry the pattern.  The CPU
oracle is not consulted: above L = 16 at 61 bits its own sum wraps (mode_limits.reference_key_cap).  The restatements are computed
once per (chain, degree, level, key) and shared."""
import numpy as np
import pytest

import hybrid_hoist_ref as HH
import hybrid_kit
import hybrid_ref as HR
import mode_limits as ML
import oracle as O
from hybrid_kit import PATTERN, tuned

pytestmark = pytest.mark.gpu

CHAINS = list(ML.HYBRID_CHAINS)
KEYS = ["max", "rnd"]  # every row all m - 1; uniform
STEPS = [1, 3, -2, 64, 0]  # 0 = conjugation (Galois element 2N - 1)
SEAL_KEY = bytes(range(1, 33))
Q_HALVES = ML.PATTERNS[3]


class Env(hybrid_kit.Env):
    """one chain at one degree: the oracle's and the device's context, the two keys on host and device"""

    def __init__(self, moai, logn, which, alpha):
        primes, self.names, alpha = ML.hybrid_chain(logn, which, alpha)
        super().__init__(moai, logn, primes=primes, alpha=alpha)
        self.which = which
        self._keys, self._dkeys = {}, {}

    def key(self, kind):
        if kind not in self._keys:
            if kind == "max":
                key = np.empty((self.digits, 2, self.k, self.n), dtype=np.uint64)
                for i, m in enumerate(self.primes):
                    key[:, :, i, :] = m - 1
            else:
                key = O.uniform_rns(np.random.default_rng(7100 + self.logn), self.primes, (self.digits, 2), self.n)
            key.setflags(write=False)
            self._keys[kind] = key
        return self._keys[kind]

    def dkey(self, kind):
        if kind not in self._dkeys:
            self._dkeys[kind] = self.up(self.key(kind))
        return self._dkeys[kind]

    def close(self):
        for b in self._dkeys.values():
            b.free()
        super().close()


_envs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    """the cached contexts and keys live as long as this module's tests, whichever ran"""
    yield
    for e in _envs.values():
        e.close()
    _envs.clear()


def env(moai, logn, which, alpha=None):
    if (logn, which, alpha) not in _envs:
        _envs[(logn, which, alpha)] = Env(moai, logn, which, alpha)
    return _envs[(logn, which, alpha)]


def code(moai, name):
    return getattr(moai.hip, "MODE_" + name)


# ---- a. modes ------------------------------------------------------------------------------------------------------------------
def assert_modes(moai, e, fp=1, lazy16=1):
    """every row of the chain is in its table class (tiled degrees; MOAI_NTT_LAZY16=0 moves the LAZY16 rows to LAZY8); returns the
    (forward, inverse) class names of the special rows"""
    if e.logn < 12:
        return None
    H = moai.hip
    out = []
    for i, name in enumerate(e.names):
        want = [table[name.rstrip("-")][0 if fp else 1] for table in (ML.FWD_CLASS, ML.INV_CLASS)]
        want = ["LAZY8" if w == "LAZY16" and not lazy16 else w for w in want]
        got = [e.ctx.arith_mode(i, of) for of in (H.MODE_OF_NTT_FORWARD, H.MODE_OF_NTT_INVERSE)]
        assert got == [code(moai, w) for w in want], (e.which, name, want, got)
        out.append(tuple(want))
    return out[e.lmax:]


@pytest.mark.parametrize("which", CHAINS)
def test_special_rows_take_the_intended_inverse_class(moai, which):
    """the mod-down inverts the special rows: exact integer and lazy butterflies on special_large, FP64 ones on special_small"""
    with tuned(moai):
        inv = [c[1] for c in assert_modes(moai, env(moai, 12, which))]
    assert inv == (["LAZY16", "GUARD", "LAZY16"] if which == "special_large" else ["FPR", "FPN", "FPN"])


# ---- the inputs and the restatement of a switch, computed once --------------------------------------------------------------------
def switch_inputs(e, L):
    """names, ct [B][2][L][N] (random addends) and tgt [B][L][N] (NTT form of the coefficient patterns).  2^10 and 2^12: worst_coeff
    and every pattern of ML.PATTERNS; above: worst_coeff, q/2 and q/2+1, random."""
    if ("in", L) not in e.cache:
        rng = np.random.default_rng(7200 + 100 * e.logn + L)
        pat = ML.pattern_rows(e.primes[:L], e.n, rng)
        worst = ML.worst_coeff(e.primes, L, e.alpha, e.n)
        if e.logn <= 12:
            names, coeff = ("worst_coeff",) + ML.PATTERNS, [worst] + list(pat)
        else:
            names, coeff = ("worst_coeff", Q_HALVES, "random"), [worst, pat[3], pat[4]]
        tgt = np.stack([e.octx.ntt(cf, L) for cf in coeff])
        ct = O.uniform_rns(rng, e.primes[:L], (len(names), 2), e.n)
        for a in (tgt, ct):
            a.setflags(write=False)
        e.cache[("in", L)] = (names, ct, tgt)
    return e.cache[("in", L)]


def switch_ref(e, L, kind, b):
    """HR.switch_key of ciphertext b of switch_inputs with key `kind`"""
    if ("sk", L, kind, b) not in e.cache:
        _, ct, tgt = switch_inputs(e, L)
        ref = HR.switch_key(e.octx, ct[b], tgt[b], e.key(kind), L, e.alpha)
        ref.setflags(write=False)
        e.cache[("sk", L, kind, b)] = ref
    return e.cache[("sk", L, kind, b)]


def galois_case(e, L, kind, step, B):
    """the first B ciphertexts of switch_inputs with c1 placed so that the rotation's permutation brings the target back, and
    HR.apply_galois"""
    names, ct, tgt = switch_inputs(e, L)
    if ("ag", L, kind, step, B) not in e.cache:
        elt = e.elts([step])[0]
        table = O.galois_table_ntt(e.logn, elt)
        ctg = ct[:B].copy()
        ctg[:, 1][..., table] = tgt[:B]
        ref = np.stack([HR.apply_galois(e.octx, ctg[b], L, elt, e.key(kind), e.alpha) for b in range(B)])
        e.cache[("ag", L, kind, step, B)] = (elt, ctg, ref)
    return (names[:B],) + e.cache[("ag", L, kind, step, B)]


def check_switch(e, L, kind, picks=None):
    """switch_key_hybrid on the ciphertexts `picks` of switch_inputs (all of them by default) in one batch"""
    names, ct, tgt = switch_inputs(e, L)
    picks = list(range(len(names))) if picks is None else list(picks)
    d, dt = e.up(ct[picks]), e.up(tgt[picks])
    e.ctx.switch_key_hybrid(d, dt, e.dkey(kind), L, e.alpha, len(picks))
    got = d.to_numpy((len(picks), 2, L, e.n))
    d.free()
    dt.free()
    for i, b in enumerate(picks):
        assert (got[i] == switch_ref(e, L, kind, b)).all(), (e.which, e.logn, L, kind, names[b])


# ---- b. the switch at the limits ------------------------------------------------------------------------------------------------
SWITCH_SHAPES = [(logn, 7) for logn in (10, 12, 13, 14, 15, 16)] + [(logn, L) for logn in (10, 12) for L in (4, 3, 1)]


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("logn,L", SWITCH_SHAPES)
@pytest.mark.parametrize("which", CHAINS)
def test_switch_at_the_limits(moai, which, logn, L, kind):
    """L = 7: digits of 3, 3, 1 primes; 4: a partial last digit; 3: one full digit and no other data row; 1: one digit of one prime"""
    e = env(moai, logn, which)
    with tuned(moai):
        assert_modes(moai, e)
        assert e.ctx.hybrid_digits(e.alpha, L) == HR.beta(L, e.alpha)
        check_switch(e, L, kind)


# ---- c. the other entry points --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", [7, 4])
@pytest.mark.parametrize("which", CHAINS)
def test_relinearize_at_the_limits(moai, which, L, kind):
    """(c0, c1) + switch(c2): the inverse transform and the MAC read the slice of stride 3L at offset 2L"""
    e = env(moai, 12, which)
    names, ct, tgt = switch_inputs(e, L)
    B = len(names)
    d3, out = e.up(np.concatenate([ct, tgt[:, None]], axis=1)), moai.DeviceBuffer(B * 2 * L * e.n)
    try:
        assert_modes(moai, e)
        e.ctx.relinearize_hybrid(d3, e.dkey(kind), out, L, e.alpha, B)
        got = out.to_numpy((B, 2, L, e.n))
    finally:
        moai.hip.reset_tuning()
        d3.free()
        out.free()
    for b in range(B):
        assert (got[b] == switch_ref(e, L, kind, b)).all(), names[b]  # HR.relinearize is HR.switch_key of (c0, c1) and c2


@pytest.mark.parametrize("step", [1, 0])
@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", [7, 4])
@pytest.mark.parametrize("which", CHAINS)
def test_apply_galois_at_the_limits(moai, which, L, kind, step):
    e = env(moai, 12, which)
    names, elt, ctg, ref = galois_case(e, L, kind, step, 3)  # worst_coeff, all q-1, all 0
    d = e.up(ctg)
    try:
        assert_modes(moai, e)
        e.ctx.apply_galois_hybrid(d, L, e.alpha, elt, e.dkey(kind), len(names))
        got = d.to_numpy(ref.shape)
    finally:
        moai.hip.reset_tuning()
        d.free()
    for b in range(len(names)):
        assert (got[b] == ref[b]).all(), names[b]


@pytest.mark.parametrize("which", CHAINS)
def test_keygen_at_the_limits(moai, which):
    """any residues for the two secrets (the digit formula does not care that a key is small); the new key all m - 1, so that
    (P mod q_r) s'[r] is as large as it gets"""
    e = env(moai, 12, which)
    sk = O.uniform_rns(np.random.default_rng(7300), e.primes, (), e.n)
    new = np.stack([np.full(e.n, m - 1, dtype=np.uint64) for m in e.primes])
    dsk, dnew = e.up(sk), e.up(new)
    got = e.ctx.hybrid_keygen(SEAL_KEY, 41, dsk, dnew, e.alpha)
    try:
        assert (got.to_numpy((e.digits, 2, e.k, e.n)) == HR.keygen(e.octx, SEAL_KEY, 41, sk, new, e.alpha)).all()
    finally:
        for b in (dsk, dnew, got):
            b.free()


# ---- d. wide digits at 61 bits ----------------------------------------------------------------------------------------------------
def short_case(e, L):
    """two ciphertexts per key: targets worst_coeff and random; HR.switch_key per key"""
    if ("short", L) not in e.cache:
        rng = np.random.default_rng(7400 + 100 * e.logn + L)
        coeff = [ML.worst_coeff(e.primes, L, e.alpha, e.n), O.uniform_rns(rng, e.primes[:L], (), e.n)]
        tgt = np.stack([e.octx.ntt(cf, L) for cf in coeff])
        ct = O.uniform_rns(rng, e.primes[:L], (2, 2), e.n)
        refs = {kind: np.stack([HR.switch_key(e.octx, ct[b], tgt[b], e.key(kind), L, e.alpha) for b in range(2)]) for kind in KEYS}
        e.cache[("short", L)] = (ct, tgt, refs)
    return e.cache[("short", L)]


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("alpha,logn", [(a, 10) for a in ML.WIDE_ALPHAS] + [(16, 12)])
def test_wide_digits_at_61_bits(moai, alpha, logn, full):
    """digit 0: alpha 61-bit primes whose scaled residues are all q_r - 1, converted to 61-bit special primes: alpha products of
    q_r - 1 and a weight (D_0 / q_r) mod m under a 61-bit m in one sum, the full hy_convert_kernel<alpha>; the mod-down converts alpha 61-bit sources in the same way.
    L = alpha + 1 adds a last digit of the one prime above 2^40, L = alpha leaves the one full digit."""
    e = env(moai, logn, "wide", alpha)
    L = alpha if full else alpha + 1
    ct, tgt, refs = short_case(e, L)
    with tuned(moai):
        assert_modes(moai, e)
        for kind in KEYS:
            d, dt = e.up(ct), e.up(tgt)
            e.ctx.switch_key_hybrid(d, dt, e.dkey(kind), L, alpha, 2)
            got = d.to_numpy(ct.shape)
            d.free()
            dt.free()
            assert (got == refs[kind]).all(), kind


# ---- e. 63 digits -----------------------------------------------------------------------------------------------------------------
L63 = 63


def long_inputs(e):
    """c1 in NTT form [3][63][N]: worst_coeff, random (both free of zero coefficients), and every row all q - 1, whose digits make
    every product of the MAC's first row (q_j - 1) (m - 1)"""
    if "long" not in e.cache:
        rng = np.random.default_rng(7500)
        coeff = [ML.worst_coeff(e.primes, L63, 1, e.n), O.uniform_rns(rng, e.primes[:L63], (), e.n)]
        assert coeff[1].all()
        top = np.stack([np.full(e.n, q - 1, dtype=np.uint64) for q in e.primes[:L63]])
        tgt = np.stack([e.octx.ntt(cf, L63) for cf in coeff] + [top])
        e.cache["long"] = (tgt, O.uniform_rns(rng, e.primes[:L63], (3, 2), e.n))
    return e.cache["long"]


@pytest.mark.parametrize("kind,b", [("max", 0), ("rnd", 1), ("max", 2)])
def test_63_digits_switch(moai, kind, b):
    """alpha = 1 with 64 primes is hy_mac_kernel, not the one-special-prime path: 63 products per sum, no fold"""
    e = env(moai, 10, "long63")
    assert e.k == 64 and e.ctx.hybrid_digits(1, L63) == 63
    tgt, ct = long_inputs(e)
    d, dt = e.up(ct[b]), e.up(tgt[b])
    e.ctx.switch_key_hybrid(d, dt, e.dkey(kind), L63, 1, 1)
    got = d.to_numpy((2, L63, e.n))
    d.free()
    dt.free()
    assert (got == HR.switch_key(e.octx, ct[b], tgt[b], e.key(kind), L63, 1)).all()


def test_63_digits_correction_and_hoisted(moai):
    """hybrid_hoist_correction and apply_galois_hybrid_hoisted with R = 2: a step with the all m - 1 key and the conjugation with the
    random key, on worst_coeff and random"""
    e = env(moai, 10, "long63")
    tgt, ct = long_inputs(e)
    ct = ct[:2].copy()
    ct[:, 1] = tgt[:2]
    check_hoisted(moai, e, L63, ct, e.elts([1, 0]), KEYS, per_pass=(2,))


# ---- f. hoisted rotations against the restatement ---------------------------------------------------------------------------------
def check_hoisted(moai, e, L, ct, elts, kinds, per_pass):
    """the device's corrections against HH.hoist_correction, its hoisted outputs under every MOAI_HYBRID_HOIST_NR of per_pass against
    HH.apply_galois_hoisted, and no fallback: the hoisted MAC is what ran"""
    B, R = len(ct), len(elts)
    for b in range(B):
        assert e.octx.ntt(ct[b, 1], L, inverse=True).all(), b  # zero-free by construction
    keys = [e.key(kind) for kind in kinds]
    dkeys = [e.dkey(kind) for kind in kinds]
    want = np.stack([HH.apply_galois_hoisted(e.octx, ct[b], L, elts, keys, e.alpha) for b in range(B)], axis=1)  # [R][B][2][L][N]
    corrs = [e.ctx.hybrid_hoist_correction(dk, elt, L, e.alpha) for dk, elt in zip(dkeys, elts)]
    dct, dout = e.up(ct), moai.DeviceBuffer(R * B * 2 * L * e.n)
    try:
        seen = {}
        for r in range(R):
            if (kinds[r], elts[r]) not in seen:
                seen[(kinds[r], elts[r])] = HH.hoist_correction(e.octx, keys[r], elts[r], L, e.alpha)
            ref = seen[(kinds[r], elts[r])]
            assert (corrs[r].to_numpy(ref.shape) == ref).all(), ("correction", r)
        for nr in per_pass:
            moai.hip.set_tuning("MOAI_HYBRID_HOIST_NR", nr)
            dout.upload(np.full(R * B * 2 * L * e.n, PATTERN, dtype=np.uint64))
            assert not e.ctx.apply_galois_hybrid_hoisted(dct, dout, L, e.alpha, elts, dkeys, corrs, B), "fallback taken"
            got = dout.to_numpy(want.shape)
            for r in range(R):
                for b in range(B):
                    assert (got[r, b] == want[r, b]).all(), (nr, r, b)
        assert (dct.to_numpy(ct.shape) == ct).all()  # the input is left alone
    finally:
        moai.hip.reset_tuning()
        for b in corrs + [dct, dout]:
            b.free()


def hoist_inputs(e, L, which=("worst_coeff", "all q-1", Q_HALVES, "random")):
    """[B][2][L][N]: c1 = the NTT form of zero-free coefficient rows"""
    rng = np.random.default_rng(7600 + 100 * e.logn + L)
    pat = ML.pattern_rows(e.primes[:L], e.n, rng)
    coeff = {"worst_coeff": ML.worst_coeff(e.primes, L, e.alpha, e.n), "all q-1": pat[0], Q_HALVES: pat[3], "random": pat[4]}
    ct = O.uniform_rns(rng, e.primes[:L], (len(which), 2), e.n)
    for b, name in enumerate(which):
        assert coeff[name].all(), name
        ct[b, 1] = e.octx.ntt(coeff[name], L)
    return ct


# rotation r takes the all m - 1 key where r is even and the random key where it is odd
HOIST_KINDS = ["max", "rnd", "max", "rnd", "max"]


@pytest.mark.parametrize("L", [7, 4])
@pytest.mark.parametrize("which", CHAINS)
def test_hoisted_rotations_against_the_restatement(moai, which, L):
    e = env(moai, 12, which)
    assert_modes(moai, e)
    check_hoisted(moai, e, L, hoist_inputs(e, L), e.elts(STEPS), HOIST_KINDS, per_pass=(4, 2, 1))


def test_hoisted_rotations_against_the_restatement_2_16(moai):
    """the largest ring once, with one ciphertext (worst_coeff): the hoisted restatement of five rotations takes several seconds per
    ciphertext at 2^16"""
    e = env(moai, 16, "special_small")
    assert_modes(moai, e)
    check_hoisted(moai, e, 7, hoist_inputs(e, 7, ("worst_coeff",)), e.elts(STEPS), HOIST_KINDS, per_pass=(4, 2, 1))


# ---- g. schedules -------------------------------------------------------------------------------------------------------------------
# 2^12, special_small, L = 7, five ciphertexts.  A row is 32 KiB: chunks of 96 KiB are one polynomial of the mod-down's three special
# rows (and one of any longer polynomial), so every internal transform -- the source-slice inverse of the mod-down among them -- runs
# chunk by chunk: on the caller's stream under MOAI_NTT_PIPE=0, on two side streams under MOAI_NTT_PIPE_INNER=1 (MOAI_NTT_PIPE_MIN=1:
# ten chunks would otherwise stay on the caller's stream in one piece).  A switch at L = 7, alpha = 3 takes 70 rows of scratch and a
# rotation 84 (tests/test_gpu_hybrid_keyswitch.py): 6000 KiB hold two ciphertexts of either.
CHUNKS = {"MOAI_NTT_CHUNK_MB": 0, "MOAI_NTT_CHUNK_KB": 96}
SCHEDULES = {
    "defaults": {},
    "ntt_fp_0": {"MOAI_NTT_FP": 0},
    "lazy16_0": {"MOAI_NTT_LAZY16": 0},
    "chunks_one_stream": dict(CHUNKS, MOAI_NTT_PIPE=0),
    "chunks_side_streams": dict(CHUNKS, MOAI_NTT_PIPE=2, MOAI_NTT_PIPE_INNER=1, MOAI_NTT_PIPE_MIN=1),
    "tmp_two_ciphertexts": {"MOAI_HYBRID_TMP_KB": 6000},
}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_schedules_give_the_restatements_bits(moai, schedule):
    e, L, B, kind = env(moai, 12, "special_small"), 7, 5, "rnd"
    names, elt, ctg, ref = galois_case(e, L, kind, 2, B)
    knobs = SCHEDULES[schedule]
    with tuned(moai, **knobs):
        assert_modes(moai, e, fp=knobs.get("MOAI_NTT_FP", 1), lazy16=knobs.get("MOAI_NTT_LAZY16", 1))
        check_switch(e, L, kind, picks=range(B))
        d = e.up(ctg)
        e.ctx.apply_galois_hybrid(d, L, e.alpha, elt, e.dkey(kind), B)
        got = d.to_numpy(ref.shape)
        d.free()
        for b in range(B):
            assert (got[b] == ref[b]).all(), ("apply_galois_hybrid", names[b])
