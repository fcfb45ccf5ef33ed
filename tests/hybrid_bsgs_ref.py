"""moai_hybrid_bsgs_dot (include/moai_hip.h, "giant steps summed in the extended basis") restated in Python integers over
tests/hybrid_ref.py, tests/hybrid_hoist_ref.py and tests/hybrid_dot_ref.py.  The definition goes through the SEPARATE accumulators:
per giant step the inner sum S_g and its addend a_g as hybrid_dot_ref forms them, lifted into Q P without rounding; c1'_g is
hybrid_dot_ref.rotate_pt_dot's own out_g[1]; a giant step with E_g != 1 adds the accumulators of steps 1-4 on the PERMUTED c1'_g
and the permuted lifted polynomial 0; one step 5 (hybrid_hoist_ref.mod_down) without an addend ends it.  Nothing of the device's
fusion is used.  tests/test_hybrid_bsgs_cpu.py holds it to the two identities and to the header's noise bound;
tests/test_gpu_hybrid_bsgs.py compares the device with it bit for bit.  CPU only."""
import numpy as np

import hybrid_dot_ref as HD
import hybrid_hoist_ref as HH
import hybrid_ref as HR
import oracle as O


def inner_sums(octx, ct, L, alpha, elts, keys, plains):
    """per output g: (S_g dict (p, context prime) -> [N] objects, a_g [2][L] lists of [N] objects), as rotate_pt_dot forms them"""
    n, primes = octx.n, octx.primes
    rows = HH.rows_of(octx, L, alpha)
    perm, A = {}, {}
    for r, elt in enumerate(elts):
        if elt != 1 and any(pl[r] is not None for pl in plains):
            perm[r] = ct[:, :, O.galois_table_ntt(octx.logn, elt)]
            A[r] = HD.accumulators(octx, perm[r][1], keys[r], L, alpha)
    res = []
    for pl in plains:
        assert any(p is not None for p in pl), "a giant step with no present term is refused"
        S = {(p, row): np.zeros(n, dtype=object) for p in range(2) for row in rows}
        a = [[np.zeros(n, dtype=object) for _ in range(L)] for _ in range(2)]
        for r, elt in enumerate(elts):
            if pl[r] is None:
                continue
            pt = np.asarray(pl[r], dtype=np.uint64).reshape(L + alpha, n)
            if elt == 1:
                for p in range(2):
                    for i in range(L):
                        a[p][i] = (a[p][i] + HR._obj(pt[i]) * HR._obj(ct[p, i])) % primes[i]
                continue
            for t, row in enumerate(rows):
                for p in range(2):
                    S[p, row] = (S[p, row] + HR._obj(pt[t]) * A[r][p, row]) % primes[row]
            for i in range(L):
                a[0][i] = (a[0][i] + HR._obj(pt[i]) * HR._obj(perm[r][0, i])) % primes[i]
        res.append((S, a))
    return res


class _memo_accumulators:
    """inside the block hybrid_dot_ref.accumulators remembers its results by (key, target): rotate_pt_dot and inner_sums ask for
    the same ones, and giant steps may share a key and a target"""

    def __enter__(self):
        self.plain, memo = HD.accumulators, {}

        def cached(octx, target, key, L, alpha):
            at = (id(key), np.asarray(target).tobytes(), L, alpha)
            if at not in memo:
                memo[at] = self.plain(octx, target, key, L, alpha)
            return memo[at]

        HD.accumulators = cached

    def __exit__(self, *exc):
        HD.accumulators = self.plain


def bsgs_dot(octx, ct, L, alpha, baby_elts, baby_keys, giant_elts, giant_keys, plains):
    """[2][L][N] for ct [2][L][N]: plains[g][r] is p_{g,r} [L + alpha][N] or None; a key is not read where its element is 1"""
    with _memo_accumulators():
        return _bsgs_dot(octx, ct, L, alpha, baby_elts, baby_keys, giant_elts, giant_keys, plains)


def _bsgs_dot(octx, ct, L, alpha, baby_elts, baby_keys, giant_elts, giant_keys, plains):
    k, n, primes = octx.k, octx.n, octx.primes
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, n)
    rows = HH.rows_of(octx, L, alpha)
    P = HR._prod(primes[k - alpha:])
    inner = inner_sums(octx, ct, L, alpha, baby_elts, baby_keys, plains)
    c1p = HD.rotate_pt_dot(octx, ct, L, alpha, baby_elts, baby_keys, plains)[:, 1]  # c1'_g = out_g[1], bit for bit
    Z = {(p, row): np.zeros(n, dtype=object) for p in range(2) for row in rows}
    for g, E in enumerate(giant_elts):
        S, a = inner[g]
        # T_g: the inner sum lifted into Q P, nothing rounded
        T = {}
        for p in range(2):
            for row in rows:
                T[p, row] = (S[p, row] + (P % primes[row]) * a[p][row]) % primes[row] if row < L else S[p, row]
        if E == 1:
            for key in Z:
                Z[key] = (Z[key] + T[key]) % primes[key[1]]
            continue
        table = O.galois_table_ntt(octx.logn, E)
        Bg = HD.accumulators(octx, c1p[g][:, table], giant_keys[g], L, alpha)
        for row in rows:
            Z[0, row] = (Z[0, row] + Bg[0, row] + T[0, row][table]) % primes[row]
            Z[1, row] = (Z[1, row] + Bg[1, row]) % primes[row]
    return HH.mod_down(octx, Z, np.zeros((2, L, n), dtype=np.uint64), L, alpha)


def noise_bound(octx, L, alpha, s_l1, giant_elts, plain_l1_sums):
    """the header's bound: (alpha - 1/2)(1 + |s|_1) + sum_g [ l_g u + [E_g != 1](u + (alpha - 1/2)|s|_1) ] with u = beta N alpha 21
    D_max / P and l_g = plain_l1_sums[g], the sum of |p_{g,r}|_1 over the present terms with e_r != 1"""
    u = HR.approx_u(octx, L, alpha)
    bound = (alpha - 0.5) * (1 + s_l1)
    for E, l1 in zip(giant_elts, plain_l1_sums):
        bound += l1 * u + ((u + (alpha - 0.5) * s_l1) if E != 1 else 0)
    return bound


def bsgs_error(octx, out, ct, s_ntt, L, baby_elts, giant_elts, plains):
    """the centred integer coefficients [N] of out[0] + out[1] s - sum_g sigma_{E_g}(sum_r p_{g,r} sigma_{e_r}(c0 + c1 s)) mod Q_L
    (exact CRT); out, ct [2][L][N], s in NTT form"""
    primes, n = octx.primes[:L], octx.n
    v = np.empty((L, n), dtype=np.uint64)
    for i, q in enumerate(primes):
        m = (HR._obj(ct[0][i]) + HR._obj(ct[1][i]) * HR._obj(s_ntt[i])) % q  # the message under s, NTT form
        x = HR._obj(out[0][i]) + HR._obj(out[1][i]) * HR._obj(s_ntt[i])
        for E, pl in zip(giant_elts, plains):
            inner = np.zeros(n, dtype=object)
            for elt, pt in zip(baby_elts, pl):
                if pt is not None:
                    inner = inner + HR._obj(pt[i]) * m[O.galois_table_ntt(octx.logn, elt)]
            x = x - (inner % q)[O.galois_table_ntt(octx.logn, E)]
        v[i] = HR._u64(x % q)
    v = octx.ntt(v, L, inverse=True)
    Q = HR._prod(primes)
    x = np.zeros(n, dtype=object)
    for i, q in enumerate(primes):
        Qi = Q // q
        x = (x + HR._obj(v[i]) * (Qi * pow(Qi % q, -1, q))) % Q
    return np.where(x > Q // 2, x - Q, x)
