"""The hoisted rotations over the hybrid key switch (include/moai_hip.h, "hoisted rotations over the hybrid key switch") restated
in Python integers over tests/hybrid_ref.py: the digits of the UNPERMUTED c1 are built once, every rotation reads them through its
index permutation and adds its correction
    corr[p][row] = NTT_row(mask) (*) sum_j (|R_j| D_j mod m_row) key[j][p][row]      (mod m_row).
tests/test_hybrid_hoist_cpu.py holds this module to hybrid_ref.apply_galois bit for bit; tests/test_gpu_hybrid_hoisted.py compares
the device's correction with hoist_correction.  CPU only."""
import numpy as np

import hybrid_ref as HR
import oracle as O


def sign_mask(logn, elt):
    """[N]: 1 where x -> x^elt negates the coefficient that lands there (GaloisTool::apply_galois, SEAL/util/galois.cpp:133-190)"""
    n = 1 << logn
    raw = (np.arange(n, dtype=np.uint64) * np.uint64(elt)) & np.uint64(2 * n - 1)
    mask = np.zeros(n, dtype=np.uint64)
    mask[(raw & np.uint64(n - 1)).astype(np.int64)] = raw >> np.uint64(logn)
    return mask


def rows_of(octx, L, alpha):
    """the context primes of the L + alpha rows of a switch at L"""
    return list(range(L)) + HR.special_rows(octx.k, alpha)


def hoist_correction(octx, key, elt, L, alpha):
    """[2][L + alpha][N] for key [beta(k - alpha)][2][k][N]"""
    k, n, primes = octx.k, octx.n, octx.primes
    key = np.asarray(key, dtype=np.uint64).reshape(HR.beta(k - alpha, alpha), 2, k, n)
    rows = rows_of(octx, L, alpha)
    mask = octx.ntt(np.stack([sign_mask(octx.logn, elt)] * len(rows)), len(rows), prime_index=rows)
    out = np.empty((2, len(rows), n), dtype=np.uint64)
    for t, row in enumerate(rows):
        m = primes[row]
        for p in range(2):
            s = 0
            for j in range(HR.beta(L, alpha)):
                R = HR.digit_rows(j, L, alpha)
                s = s + HR._obj(key[j, p, row]) * ((len(R) * HR._prod(primes[r] for r in R)) % m)
            out[p, t] = HR._u64((HR._obj(mask[t]) * (s % m)) % m)
    return out


def mod_down(octx, acc, addend, L, alpha):
    """step 5 of the switch: acc dict (p, context prime) -> [N] canonical, addend [2][L][N]; [2][L][N]"""
    k, n, primes = octx.k, octx.n, octx.primes
    sp = HR.special_rows(k, alpha)
    P = HR._prod(primes[r] for r in sp)
    h = P // 2
    out = np.empty((2, L, n), dtype=np.uint64)
    for p in range(2):
        x = octx.ntt(np.stack([HR._u64(acc[p, row]) for row in sp]), alpha, prime_index=sp, inverse=True)
        y = []
        for t, row in enumerate(sp):
            pt = primes[row]
            y.append((((HR._obj(x[t]) + h % pt) % pt) * pow((P // pt) % pt, -1, pt)) % pt)
        conv = np.empty((L, n), dtype=np.uint64)
        for i in range(L):
            q = primes[i]
            conv[i] = HR._u64((sum(y[t] * ((P // primes[row]) % q) for t, row in enumerate(sp)) - h % q) % q)
        conv = octx.ntt(conv, L)
        for i in range(L):
            q = primes[i]
            out[p, i] = HR._u64((HR._obj(addend[p, i]) + (acc[p, i] - HR._obj(conv[i])) * pow(P % q, -1, q)) % q)
    return out


def apply_galois_hoisted(octx, ct, L, elts, keys, alpha):
    """[R][2][L][N]: rotation r of ct [2][L][N] by elts[r] with keys[r], from ONE digit decomposition"""
    k, n, primes = octx.k, octx.n, octx.primes
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, n)
    rows = rows_of(octx, L, alpha)
    c_coef = octx.ntt(ct[1], L, inverse=True)
    digits = []
    for j in range(HR.beta(L, alpha)):
        ext = HR.mod_up(octx, c_coef, j, L, alpha)
        digits.append({row: (ext[row] if row in ext else ct[1][row]) for row in rows})
    outs = []
    for elt, key in zip(elts, keys):
        key = np.asarray(key, dtype=np.uint64).reshape(HR.beta(k - alpha, alpha), 2, k, n)
        table = O.galois_table_ntt(octx.logn, elt)
        corr = hoist_correction(octx, key, elt, L, alpha)
        acc = {}
        for t, row in enumerate(rows):
            m = primes[row]
            for p in range(2):
                s = HR._obj(corr[p, t])
                for j, d in enumerate(digits):
                    s = s + HR._obj(d[row][table]) * HR._obj(key[j, p, row])
                acc[p, row] = s % m
        addend = np.stack([ct[0][:, table], np.zeros_like(ct[0])])
        outs.append(mod_down(octx, acc, addend, L, alpha))
    return np.stack(outs)
