"""The cases that several test files of the hybrid key switch share (tests/test_gpu_hybrid_limits.py, test_gpu_hybrid_pt_dot.py,
test_gpu_hybrid_bsgs.py, test_gpu_hybrid_exact.py, test_gpu_hybrid_sums_limits.py, test_gpu_hybrid_forms_limits.py), on top of
tests/hybrid_kit.py:
    LimitEnv, assert_modes, switch_inputs    a chain of tests/mode_limits.py by name with its two keys, the check that every row of it is
                                             in the arithmetic class its name promises, and the coefficient patterns of a switch
    DotCase, BsgsCase                        one call of moai_hybrid_rotate_pt_dot / moai_hybrid_bsgs_dot with its restatement
    exact, run_switch, run_rescale           the exact rounding mode for a block; the two calls most of its tests make
    boundary_case                            the key that puts the mod-down's X' on 0, 1, 2, W-2, W-1, H-1, H, H+1
Not collected."""
import contextlib

import numpy as np

import hybrid_bsgs_ref as HB
import hybrid_dot_ref as HD
import hybrid_exact_ref as HX
import hybrid_hoist_ref as HH
import hybrid_kit
import hybrid_ref as HR
import hybrid_rescale_ref as RR
import mode_limits as ML
import oracle as O
from hybrid_kit import IDENT, PATTERN, cached

Q_HALVES = ML.PATTERNS[3]
FAST, EXACT = 0, 1
STEPS = [1, 3, -2, 64, 0, IDENT]  # rotate_pt_dot's default terms; 0 = conjugation (Galois element 2N - 1)
BABY = [IDENT, 1, 3, -2, 64, 0]   # bsgs_dot's default baby steps
GIANT = [IDENT, 4, -8]            # and giant steps


# ---- a chain of mode_limits by name ------------------------------------------------------------------------------------------------
class LimitEnv(hybrid_kit.Env):
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


def code(moai, name):
    return getattr(moai.hip, "MODE_" + name)


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


# ---- one call of the two sums ------------------------------------------------------------------------------------------------------
def dot_absent(steps, n_out):
    """output 1 lacks terms 1 and 3; the last output holds only the identity term"""
    if n_out < 3 or IDENT not in steps:
        return set()
    return {(1, 1), (1, 3)} | {(n_out - 1, r) for r, s in enumerate(steps) if s != IDENT}


def bsgs_absent(baby, giant):
    """giant step 1 lacks baby terms 1 and 3; the last giant step holds only the identity baby term"""
    if len(giant) < 3 or IDENT not in baby:
        return set()
    return {(1, 1), (1, 3)} | {(len(giant) - 1, r) for r, s in enumerate(baby) if s != IDENT}


def _keys_of(e, elts, rng, shared_key, kinds):
    """(host, device) keys of the rotations `elts`: none for the element 1; one random key each, or one for all (shared_key), or the
    keys of a LimitEnv by kind (kinds[r])"""
    if kinds is not None:
        return ([None if elt == 1 else e.key(kinds[r]) for r, elt in enumerate(elts)],
                [None if elt == 1 else e.dkey(kinds[r]) for r, elt in enumerate(elts)])
    one_key = e.random_key(rng) if shared_key else None
    return [None if elt == 1 else (one_key if shared_key else e.random_key(rng)) for elt in elts], None


class DotCase:
    """one call of rotate_pt_dot: the operands on the device, and the restatement's outputs computed once (want=False: not at all)"""

    def __init__(self, e, L, steps=STEPS, B=3, n_out=3, seed=0, ct=None, plain=None, shared_key=False, want=True, kinds=None):
        self.e, self.L, self.B, self.R, self.n_out = e, L, B, len(steps), n_out
        rng = np.random.default_rng(e.logn * 1000 + e.alpha * 100 + L * 10 + seed)
        self.elts = e.elts(steps)
        self.keys, self.dkeys = _keys_of(e, self.elts, rng, shared_key, kinds)
        if self.dkeys is None:
            dk = {}
            self.dkeys = [None if k is None else cached(dk, id(k), lambda: e.up(k)) for k in self.keys]
        self.ct = e.random_input(rng, L, B) if ct is None else ct(rng)
        self.dct = e.up(self.ct)
        dc = {}
        self.corrs = [None if k is None else cached(dc, (id(k), elt), lambda: e.ctx.hybrid_hoist_correction(k, elt, L, e.alpha))
                      for k, elt in zip(self.dkeys, self.elts)]
        absent = dot_absent(steps, n_out)
        new_plain = plain or (lambda: O.uniform_rns(rng, e.rows(L), (), e.n))
        self.plains = [[None if (g, r) in absent else new_plain() for r in range(self.R)] for g in range(n_out)]
        dp = {}
        self.dplains = [[None if p is None else cached(dp, id(p), lambda: e.up(p)) for p in row] for row in self.plains]
        self.shape = (n_out, B, 2, L, e.n)
        if want:
            self.want = np.empty(self.shape, dtype=np.uint64)
            with HB._memo_accumulators():  # rotations that share a key and an element share their accumulators
                for b in range(B):
                    self.want[:, b] = HD.rotate_pt_dot(e.octx, self.ct[b], L, e.alpha, self.elts, self.keys, self.plains)

    def run(self):
        """(fallback flag, outputs [n_out][B][2][L][N]) from output buffers filled with a pattern"""
        out = self.e.filled(self.shape, PATTERN)
        fb = self.e.ctx.hybrid_rotate_pt_dot(self.dct, out, self.L, self.e.alpha, self.elts, self.dkeys, self.corrs, self.dplains, self.B)
        got = out.to_numpy(self.shape)
        assert (self.dct.to_numpy(self.ct.shape) == self.ct).all()  # the input is left alone
        return fb, got

    def check(self):
        fb, got = self.run()
        assert not fb
        for g in range(self.n_out):
            assert (got[g] == self.want[g]).all(), g


class BsgsCase:
    """one call of bsgs_dot: the operands on the device, and the restatement's output computed once (want=False: not at all)"""

    def __init__(self, e, L, baby=BABY, giant=GIANT, B=None, seed=0, ct=None, plain=None, shared_key=False, want=True, kinds=None,
                 giant_kinds=None):
        B = (3 if e.logn == 10 else 2) if B is None else B
        self.e, self.L, self.B, self.R, self.ng = e, L, B, len(baby), len(giant)
        rng = np.random.default_rng(e.logn * 1000 + e.alpha * 100 + L * 10 + seed + 5)
        self.baby, self.giant = e.elts(baby), e.elts(giant)
        if kinds is not None:
            (self.bkeys, self.dbkeys), (self.gkeys, self.dgkeys) = (_keys_of(e, self.baby, rng, False, kinds),
                                                                    _keys_of(e, self.giant, rng, False, giant_kinds))
        else:
            one_key = e.random_key(rng) if shared_key else None
            self.bkeys = [None if elt == 1 else (one_key if shared_key else e.random_key(rng)) for elt in self.baby]
            self.gkeys = [None if elt == 1 else (one_key if shared_key else e.random_key(rng)) for elt in self.giant]
            dk = {}
            self.dbkeys = [None if k is None else cached(dk, id(k), lambda: e.up(k)) for k in self.bkeys]
            self.dgkeys = [None if k is None else cached(dk, id(k), lambda: e.up(k)) for k in self.gkeys]
        self.ct = e.random_input(rng, L, B) if ct is None else ct(rng)
        self.dct = e.up(self.ct)
        dc = {}
        self.corrs = [None if k is None else cached(dc, (id(k), elt), lambda: e.ctx.hybrid_hoist_correction(k, elt, L, e.alpha))
                      for k, elt in zip(self.dbkeys, self.baby)]
        absent = bsgs_absent(baby, giant)
        new_plain = plain or (lambda: O.uniform_rns(rng, e.rows(L), (), e.n))
        self.plains = [[None if (g, r) in absent else new_plain() for r in range(self.R)] for g in range(self.ng)]
        dp = {}
        self.dplains = [[None if p is None else cached(dp, id(p), lambda: e.up(p)) for p in row] for row in self.plains]
        self.shape = (B, 2, L, e.n)
        if want:
            self.want = np.stack([HB.bsgs_dot(e.octx, self.ct[b], L, e.alpha, self.baby, self.bkeys, self.giant, self.gkeys, self.plains)
                                  for b in range(B)])

    def run(self):
        """(fallback flag, output [B][2][L][N]) from an output buffer filled with a pattern"""
        out = self.e.filled(self.shape, PATTERN)
        fb = self.e.ctx.hybrid_bsgs_dot(self.dct, out, self.L, self.e.alpha, self.baby, self.dbkeys, self.corrs, self.giant, self.dgkeys,
                                        self.dplains, self.B)
        got = out.to_numpy(self.shape)
        assert (self.dct.to_numpy(self.ct.shape) == self.ct).all()  # the input is left alone
        return fb, got

    def check(self):
        fb, got = self.run()
        assert not fb
        assert (got == self.want).all()


# ---- the exact rounding mode -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def exact(e):
    """the block runs in MOAI_HYBRID_ROUND_EXACT; the context is back in the default afterwards, whatever happened"""
    try:
        e.ctx.hybrid_set_rounding(EXACT)
        yield
    finally:
        e.ctx.hybrid_set_rounding(FAST)


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


def boundary_case(e, rescale):
    """(L, ct3 [1][3][L][N], key, Z): the accumulator of a single-digit switch of the constant 1 is g (*) key digit 0, g the digit's
    converted constant under each row (1 where the digit has one prime: it converts exactly).  So the key is built row by row as g^-1
    times the residues of integers Z whose X' are the targets 0, 1, 2, W-2, W-1, H-1, H, H+1, with c_0 = c_1 = 0; the restatement says
    what Z really was, and that is asserted here."""
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
    return L, ct3, key, Z


def check_boundaries(e, rescale):
    """the device in exact mode on boundary_case: the restatement's bits, and within 1/2 + 2^-40 of the exact quotient"""
    L, ct3, key, Z = boundary_case(e, rescale)
    octx, alpha = e.octx, e.alpha
    W = HR._prod(e.primes[r] for r in HX.bases(octx, L, alpha, rescale)[0])
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
