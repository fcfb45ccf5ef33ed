"""moai_hybrid_rotate_pt_dot (include/moai_hip.h, "plaintext-weighted sums of hoisted rotations") restated in Python integers over
tests/hybrid_ref.py and tests/hybrid_hoist_ref.py.  The definition goes through the SEPARATE accumulators A_r of steps 1-4 on the
PERMUTED target, not through the hoisting identity: per output the plaintext-weighted sum of the A_r in the extended basis, ONE
step 5 (hybrid_hoist_ref.mod_down), and the exact products with the permuted c0 and, for the element 1, with the ciphertext
itself.  tests/test_hybrid_pt_dot_cpu.py holds it to hybrid_ref.apply_galois and to the header's noise bound;
tests/test_gpu_hybrid_pt_dot.py compares the device with it bit for bit.  CPU only."""
import numpy as np

import hybrid_hoist_ref as HH
import hybrid_ref as HR
import oracle as O


def accumulators(octx, target, key, L, alpha):
    """steps 1-4 of the hybrid switch of target [L][N] (NTT form): dict (p, context prime) -> [N] canonical, over the L + alpha rows"""
    k, n, primes = octx.k, octx.n, octx.primes
    target = np.asarray(target, dtype=np.uint64).reshape(L, n)
    key = np.asarray(key, dtype=np.uint64).reshape(HR.beta(k - alpha, alpha), 2, k, n)
    rows = HH.rows_of(octx, L, alpha)
    c_coef = octx.ntt(target, L, inverse=True)
    acc = {(p, row): np.zeros(n, dtype=object) for p in range(2) for row in rows}
    for j in range(HR.beta(L, alpha)):
        ext = HR.mod_up(octx, c_coef, j, L, alpha)
        for row in rows:
            d = HR._obj(ext[row] if row in ext else target[row])
            for p in range(2):
                acc[p, row] = (acc[p, row] + d * HR._obj(key[j, p, row])) % primes[row]
    return acc


def rotate_pt_dot(octx, ct, L, alpha, elts, keys, plains):
    """[n_out][2][L][N] for ct [2][L][N]: plains[g][r] is p_{g,r} [L + alpha][N] (rows in the order of rows_of) or None; keys[r] is not
    read where elts[r] == 1"""
    n, primes = octx.n, octx.primes
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, n)
    rows = HH.rows_of(octx, L, alpha)
    # per rotation with a key switch: the permuted ciphertext and its accumulators, computed once for every output
    perm, A = {}, {}
    for r, elt in enumerate(elts):
        if elt != 1 and any(pl[r] is not None for pl in plains):
            perm[r] = ct[:, :, O.galois_table_ntt(octx.logn, elt)]
            A[r] = accumulators(octx, perm[r][1], keys[r], L, alpha)
    outs = []
    for pl in plains:
        assert any(p is not None for p in pl), "an output with no present term is refused"
        S = {(p, row): np.zeros(n, dtype=object) for p in range(2) for row in rows}
        addend = [[np.zeros(n, dtype=object) for _ in range(L)] for _ in range(2)]
        switched = False
        for r, elt in enumerate(elts):
            if pl[r] is None:
                continue
            pt = np.asarray(pl[r], dtype=np.uint64).reshape(L + alpha, n)
            if elt == 1:
                for p in range(2):
                    for i in range(L):
                        addend[p][i] = (addend[p][i] + HR._obj(pt[i]) * HR._obj(ct[p, i])) % primes[i]
                continue
            switched = True
            for t, row in enumerate(rows):
                for p in range(2):
                    S[p, row] = (S[p, row] + HR._obj(pt[t]) * A[r][p, row]) % primes[row]
            for i in range(L):
                addend[0][i] = (addend[0][i] + HR._obj(pt[i]) * HR._obj(perm[r][0, i])) % primes[i]
        addend = np.stack([np.stack([HR._u64(a) for a in addend[p]]) for p in range(2)])
        outs.append(HH.mod_down(octx, S, addend, L, alpha) if switched else addend)
    return np.stack(outs)


def ones_plain(octx, L, alpha):
    """p = 1: all ones in every row of the NTT form"""
    return np.ones((L + alpha, octx.n), dtype=np.uint64)


def encode_plain(octx, coeffs, L, alpha):
    """the integer polynomial `coeffs` [N] (signed) as a plaintext [L + alpha][N] in NTT form"""
    rows = HH.rows_of(octx, L, alpha)
    res = np.stack([HR._u64(np.asarray([int(c) % octx.primes[row] for c in coeffs], dtype=object)) for row in rows])
    return octx.ntt(res, len(rows), prime_index=rows)


def noise_bound(octx, L, alpha, s_l1, plain_l1_sum):
    """the header's bound: (sum_r |p_{g,r}|_1) beta N alpha 21 D_max / P + (alpha - 1/2)(1 + |s|_1), the sum over the terms with
    e_r != 1"""
    return HR.approx_u(octx, L, alpha, times=plain_l1_sum) + (alpha - 0.5) * (1 + s_l1)


def dot_error(octx, out, ct, s_ntt, L, elts, plains_g):
    """the centred integer coefficients [N] of out[0] + out[1] s - sum_r p_r sigma_r(c0 + c1 s) mod Q_L (exact CRT); out, ct
    [2][L][N], s in NTT form, plains_g[r] [L + alpha][N] or None"""
    primes, n = octx.primes[:L], octx.n
    v = np.empty((L, n), dtype=np.uint64)
    for i, q in enumerate(primes):
        m = (HR._obj(ct[0][i]) + HR._obj(ct[1][i]) * HR._obj(s_ntt[i])) % q  # the message under s, NTT form
        x = HR._obj(out[0][i]) + HR._obj(out[1][i]) * HR._obj(s_ntt[i])
        for elt, pt in zip(elts, plains_g):
            if pt is not None:
                x = x - HR._obj(pt[i]) * m[O.galois_table_ntt(octx.logn, elt)]
        v[i] = HR._u64(x % q)
    v = octx.ntt(v, L, inverse=True)
    Q = HR._prod(primes)
    x = np.zeros(n, dtype=object)
    for i, q in enumerate(primes):
        Qi = Q // q
        x = (x + HR._obj(v[i]) * (Qi * pow(Qi % q, -1, q))) % Q
    return np.where(x > Q // 2, x - Q, x)
