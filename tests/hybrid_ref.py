"""The hybrid key switch of include/moai_hip.h ("hybrid key switching") restated in Python integers: alpha special primes,
digits of alpha data primes.  Conversions are numpy object arrays (exact), transforms are the KAT-pinned oracle's
(tests/oracle.py Context.ntt), the key digits are tests/client_sampling.py's symmetric encryptions.  At alpha = 1 every formula
collapses to SEAL's switch_key_inplace and generate_one_kswitch_key, which tests/test_hybrid_ref_cpu.py checks against the
oracle bit for bit; tests/test_gpu_hybrid_keyswitch.py compares the device with this module.  CPU only."""
import numpy as np

import client_sampling as CS


def beta(L, alpha):
    return -(-L // alpha)


def digit_rows(j, L, alpha):
    """R_j at L data primes"""
    return list(range(j * alpha, min((j + 1) * alpha, L)))


def special_rows(k, alpha):
    return list(range(k - alpha, k))


def _prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def _u64(a):
    return np.asarray(a, dtype=object).astype(np.uint64)


def keygen(octx, key, seq, sk_ntt, new_key_ntt, alpha):
    """[beta(k - alpha)][2][k][N]: digit j = Enc_s(0) over all k rows with sequence seq + j, plus (P mod q_r) s'[r] in row r of c0
    for every r of the top-level digit j"""
    k, primes = octx.k, octx.primes
    Lmax = k - alpha
    P = _prod(primes[k - alpha:])
    out = np.empty((beta(Lmax, alpha), 2, k, octx.n), dtype=np.uint64)
    for j in range(beta(Lmax, alpha)):
        c0, c1 = CS._sym_one(octx, key, seq + j, sk_ntt, k)
        c0 = np.array(c0, dtype=np.uint64)
        for r in digit_rows(j, Lmax, alpha):
            q = primes[r]
            c0[r] = _u64((_obj(c0[r]) + _obj(new_key_ntt[r]) * (P % q)) % q)
        out[j, 0], out[j, 1] = c0, c1
    return out


def mod_up(octx, c_coef, j, L, alpha):
    """digit j extended to every row of {q_i : i < L} + {p_t}, NTT form: dict row index (context prime) -> [N]; the rows of R_j
    are absent (the switch uses the target's own NTT-form rows there)"""
    k, primes = octx.k, octx.primes
    R = digit_rows(j, L, alpha)
    D = _prod(primes[r] for r in R)
    y = {}
    for r in R:
        q = primes[r]
        y[r] = (_obj(c_coef[r]) * pow((D // q) % q, -1, q)) % q
    rows = [i for i in range(L) if i not in R] + special_rows(k, alpha)
    conv = np.empty((len(rows), octx.n), dtype=np.uint64)
    for t, row in enumerate(rows):
        m = primes[row]
        conv[t] = _u64(sum(y[r] * ((D // primes[r]) % m) for r in R) % m)
    conv = octx.ntt(conv, len(rows), prime_index=rows)
    return {row: conv[t] for t, row in enumerate(rows)}


def switch_key(octx, ct, target, key, L, alpha):
    """ct [2][L][N] + the hybrid switch of target [L][N] (NTT form) with key [beta(k - alpha)][2][k][N]"""
    k, n, primes = octx.k, octx.n, octx.primes
    assert 1 <= alpha < k and 1 <= L <= k - alpha
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, n)
    target = np.asarray(target, dtype=np.uint64).reshape(L, n)
    key = np.asarray(key, dtype=np.uint64).reshape(beta(k - alpha, alpha), 2, k, n)
    sp = special_rows(k, alpha)
    rows = list(range(L)) + sp
    P = _prod(primes[r] for r in sp)
    h = P // 2
    # 1. coefficient form
    c_coef = octx.ntt(target, L, inverse=True)
    # 2.-4. digits and inner products
    acc = {(p, row): 0 for p in range(2) for row in rows}
    for j in range(beta(L, alpha)):
        ext = mod_up(octx, c_coef, j, L, alpha)
        for row in rows:
            d = _obj(ext[row] if row in ext else target[row])
            for p in range(2):
                acc[p, row] = (acc[p, row] + d * _obj(key[j, p, row])) % primes[row]
    # 5. mod-down with rounding
    out = np.empty((2, L, n), dtype=np.uint64)
    for p in range(2):
        x = octx.ntt(np.stack([_u64(acc[p, row]) for row in sp]), alpha, prime_index=sp, inverse=True)
        y = []
        for t, row in enumerate(sp):
            pt = primes[row]
            y.append((((_obj(x[t]) + h % pt) % pt) * pow((P // pt) % pt, -1, pt)) % pt)
        conv = np.empty((L, n), dtype=np.uint64)
        for i in range(L):
            q = primes[i]
            conv[i] = _u64((sum(y[t] * ((P // primes[row]) % q) for t, row in enumerate(sp)) - h % q) % q)
        conv = octx.ntt(conv, L)
        for i in range(L):
            q = primes[i]
            out[p, i] = _u64((_obj(ct[p, i]) + (acc[p, i] - _obj(conv[i])) * pow(P % q, -1, q)) % q)
    return out


def relinearize(octx, ct3, key, L, alpha):
    ct3 = np.asarray(ct3, dtype=np.uint64).reshape(3, L, octx.n)
    return switch_key(octx, ct3[:2], ct3[2], key, L, alpha)


def apply_galois(octx, ct, L, elt, key, alpha):
    import oracle as O

    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, octx.n)
    table = O.galois_table_ntt(octx.logn, elt)
    perm = ct[:, :, table]
    base = np.stack([perm[0], np.zeros_like(perm[0])])
    return switch_key(octx, base, perm[1], key, L, alpha)


def approx_u(octx, L, alpha, times=1):
    """the approximation term of every hybrid noise bound, u = beta N alpha 21 D_max / P; `times` u for an integer `times`, with the
    one division last, so that it is rounded once"""
    primes, k = octx.primes, octx.k
    P = _prod(primes[k - alpha:])
    d_max = max(_prod(primes[r] for r in digit_rows(j, L, alpha)) for j in range(beta(L, alpha)))
    return times * beta(L, alpha) * octx.n * alpha * 21 * d_max / P


def noise_bound(octx, L, alpha, s_l1):
    """B of the header: |d0 + d1 s - c s'| <= beta N alpha 21 D_max / P + (alpha - 1/2)(1 + |s|_1)"""
    return approx_u(octx, L, alpha) + (alpha - 0.5) * (1 + s_l1)


def switch_error(octx, d, c, s_ntt, s_new_ntt, L):
    """the centred integer coefficients [N] of d0 + d1 s - c s' mod Q_L (exact CRT), d [2][L][N], c [L][N], keys in NTT form"""
    primes, n = octx.primes[:L], octx.n
    v = np.empty((L, n), dtype=np.uint64)
    for i, q in enumerate(primes):
        v[i] = _u64((_obj(d[0][i]) + _obj(d[1][i]) * _obj(s_ntt[i]) - _obj(c[i]) * _obj(s_new_ntt[i])) % q)
    v = octx.ntt(v, L, inverse=True)
    Q = _prod(primes)
    x = np.zeros(n, dtype=object)
    for i, q in enumerate(primes):
        Qi = Q // q
        x = (x + _obj(v[i]) * (Qi * pow(Qi % q, -1, q))) % Q
    return np.where(x > Q // 2, x - Q, x)
