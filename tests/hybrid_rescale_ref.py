"""moai_relinearize_rescale_hybrid and moai_multiply_relin_rescale_hybrid (include/moai_hip.h, "hybrid relinearize + rescale")
restated in Python integers: steps 1-4 of tests/hybrid_ref.py on c2, then ONE mod-down by W = P q_{L-1} from Q_L P to Q_{L-1}.
Conversions are numpy object arrays (exact), transforms are the KAT-pinned oracle's.  tests/test_hybrid_rescale_cpu.py pins this
module (exact CRT, the oracle's rescale, the noise inequality); tests/test_gpu_hybrid_rescale.py compares the device with it.
CPU only."""
import numpy as np

from hybrid_ref import _obj, _prod, _u64, approx_u, beta, mod_up, special_rows


def accumulate(octx, target, key, L, alpha):
    """steps 1-4: {(p, row): [N] object residues} over the rows 0 .. L-1 and the special rows (context prime indices)"""
    k, n, primes = octx.k, octx.n, octx.primes
    target = np.asarray(target, dtype=np.uint64).reshape(L, n)
    key = np.asarray(key, dtype=np.uint64).reshape(beta(k - alpha, alpha), 2, k, n)
    rows = list(range(L)) + special_rows(k, alpha)
    c_coef = octx.ntt(target, L, inverse=True)
    acc = {(p, row): 0 for p in range(2) for row in rows}
    for j in range(beta(L, alpha)):
        ext = mod_up(octx, c_coef, j, L, alpha)
        for row in rows:
            d = _obj(ext[row] if row in ext else target[row])
            for p in range(2):
                acc[p, row] = (acc[p, row] + d * _obj(key[j, p, row])) % primes[row]
    return acc


def lifted(octx, ct3, key, L, alpha):
    """Z [2][L + alpha][N] (uint64, NTT form, rows 0 .. L-1 then the special rows): Z_p[i] = acc[p][i] + (P mod q_i) c_p[i] on the data
    rows, acc[p][p_t] on the special rows"""
    k, n, primes = octx.k, octx.n, octx.primes
    assert 1 <= alpha < k and 1 <= L <= k - alpha
    ct3 = np.asarray(ct3, dtype=np.uint64).reshape(3, L, n)
    sp = special_rows(k, alpha)
    P = _prod(primes[r] for r in sp)
    acc = accumulate(octx, ct3[2], key, L, alpha)
    Z = np.empty((2, L + alpha, n), dtype=np.uint64)
    for p in range(2):
        for i in range(L):
            q = primes[i]
            Z[p, i] = _u64((acc[p, i] + (P % q) * _obj(ct3[p, i])) % q)
        for t, row in enumerate(sp):
            Z[p, L + t] = _u64(acc[p, row] % primes[row])
    return Z


def relinearize_rescale(octx, ct3, key, L, alpha):
    """ct3 [3][L][N] -> [2][L-1][N], the definition of the header word for word"""
    k, n, primes = octx.k, octx.n, octx.primes
    assert L >= 2 and alpha + 1 <= 16
    sp = special_rows(k, alpha)
    src = [L - 1] + sp                       # S as context prime indices
    src_rows = [L - 1] + [L + t for t in range(alpha)]  # and as rows of Z
    W = _prod(primes[r] for r in src)
    H = W // 2
    Z = lifted(octx, ct3, key, L, alpha)
    out = np.empty((2, L - 1, n), dtype=np.uint64)
    for p in range(2):
        x = octx.ntt(np.stack([Z[p, r] for r in src_rows]), alpha + 1, prime_index=src, inverse=True)
        y = []
        for t, row in enumerate(src):
            m = primes[row]
            y.append((((_obj(x[t]) + H % m) % m) * pow((W // m) % m, -1, m)) % m)
        conv = np.empty((L - 1, n), dtype=np.uint64)
        for i in range(L - 1):
            q = primes[i]
            conv[i] = _u64((sum(y[t] * ((W // primes[row]) % q) for t, row in enumerate(src)) - H % q) % q)
        conv = octx.ntt(conv, L - 1)
        for i in range(L - 1):
            q = primes[i]
            out[p, i] = _u64(((_obj(Z[p, i]) - _obj(conv[i])) * pow(W % q, -1, q)) % q)
    return out


def ct_product(octx, x, y, L):
    """(x0 y0, x0 y1 + x1 y0, x1 y1) [3][L][N], canonical: moai_ct_multiply's residues, and moai_ct_square's where y is x"""
    n = octx.n
    x = np.asarray(x, dtype=np.uint64).reshape(2, L, n)
    y = np.asarray(y, dtype=np.uint64).reshape(2, L, n)
    out = np.empty((3, L, n), dtype=np.uint64)
    for i in range(L):
        q = octx.primes[i]
        x0, x1, y0, y1 = _obj(x[0, i]), _obj(x[1, i]), _obj(y[0, i]), _obj(y[1, i])
        out[0, i], out[1, i], out[2, i] = _u64(x0 * y0 % q), _u64((x0 * y1 + x1 * y0) % q), _u64(x1 * y1 % q)
    return out


def multiply_relin_rescale(octx, x, y, key, L, alpha):
    return relinearize_rescale(octx, ct_product(octx, x, y, L), key, L, alpha)


def crt(octx, rows_ntt, prime_index):
    """the integer coefficients [N] in [0, M) of a polynomial given by its NTT-form rows under the context primes prime_index, M their
    product (exact CRT)"""
    prime_index = list(prime_index)
    v = octx.ntt(np.stack([np.asarray(r, dtype=np.uint64) for r in rows_ntt]), len(prime_index), prime_index=prime_index, inverse=True)
    M = _prod(octx.primes[r] for r in prime_index)
    x = np.zeros(octx.n, dtype=object)
    for t, r in enumerate(prime_index):
        m = octx.primes[r]
        Mi = M // m
        x = (x + _obj(v[t]) * (Mi * pow(Mi % m, -1, m))) % M
    return x


def centred(x, M):
    return np.where(x > M // 2, x - M, x)


def noise_bound(octx, L, alpha, s_l1):
    """the header's bound on |q_{L-1} (out0 + out1 s) - (c0 + c1 s + c2 s^2)|: beta N alpha 21 D_max / P + q_{L-1} (alpha + 1/2)(1 + |s|_1)"""
    return approx_u(octx, L, alpha) + octx.primes[L - 1] * (alpha + 0.5) * (1 + s_l1)


def rescale_error(octx, out, ct3, s_ntt, L):
    """the centred integer coefficients [N] of q_{L-1} (out0 + out1 s) - (c0 + c1 s + c2 s^2) mod Q_L; out [2][L-1][N], ct3 [3][L][N],
    s in NTT form over (at least) the first L primes"""
    primes, n = octx.primes, octx.n
    out = np.asarray(out, dtype=np.uint64).reshape(2, L - 1, n)
    ct3 = np.asarray(ct3, dtype=np.uint64).reshape(3, L, n)
    lo = [_u64((_obj(out[0, i]) + _obj(out[1, i]) * _obj(s_ntt[i])) % primes[i]) for i in range(L - 1)]
    hi = [_u64((_obj(ct3[0, i]) + _obj(ct3[1, i]) * _obj(s_ntt[i]) + _obj(ct3[2, i]) * _obj(s_ntt[i]) * _obj(s_ntt[i])) % primes[i])
          for i in range(L)]
    Q = _prod(primes[:L])
    y = crt(octx, lo, range(L - 1))
    m = crt(octx, hi, range(L))
    return centred((primes[L - 1] * y - m) % Q, Q)
