"""CKKSEncoder::decode_internal (SEAL/ckks.h:644-761) restated from pieces the reference's KATs already pin, as the
comparator of the device decoder (tests/test_oracle_decoder.py pins the comparator itself):

1. the oracle's inverse NTT (inverse_ntt_negacyclic_harvey, ckks.h:692-697);
2. an exact CRT in Python integers (RNSBase::compose_array, util/rns.cpp:354);
3. the reference's word-by-word conversion to double (ckks.h:713-753) in IEEE doubles, every operation rounded on its
   own (numpy float64 element-wise; float(int) is correctly rounded like x86-64's u64 -> double);
4. the oracle's forward DWT with its root_powers_ (mo_fft_transform_to_rev, oracle/moai_oracle.c:1468);
5. the gather through matrix_reps_index_map_ (ckks.h:757-760).
CPU only; N = 2^16 at 36 primes takes a few seconds per plaintext."""
import numpy as np

TWO_POW_64 = float(2**64)


def product(primes):
    Q = 1
    for q in primes:
        Q *= int(q)
    return Q


def compose(coeff_rows, primes):
    """exact x in [0, Q) of every coefficient: coeff_rows [L][N] uint64 -> object array [N] of Python ints."""
    Q = product(primes)
    x = np.zeros(coeff_rows.shape[1], dtype=object)
    for r, q in enumerate(primes):
        q = int(q)
        Qi = Q // q
        w = (Qi * pow(Qi % q, -1, q)) % Q
        x = x + coeff_rows[r].astype(object) * w
    return x % Q


def words_of(x, count):
    """little-endian 64-bit words of every x: object array [count][N] of Python ints."""
    mask = (1 << 64) - 1
    return [(x >> (64 * j)) & mask for j in range(count)]


_to_float = np.frompyfunc(float, 1, 1)


def to_double(v):
    return _to_float(v).astype(np.float64)


def convert(x, primes, scale):
    """ckks.h:713-753 on the composed integers x (object array), in float64: the real parts res[i]."""
    L = len(primes)
    Q = product(primes)
    threshold = (Q + 1) >> 1  # upper_half_threshold (SEAL/context.cpp:376-382)
    neg = np.array([int(v) >= threshold for v in x], dtype=bool)
    xw = words_of(x, L)
    qw = [(Q >> (64 * j)) & ((1 << 64) - 1) for j in range(L)]
    res = np.zeros(x.shape[0], dtype=np.float64)
    scaled = 1.0 / float(scale)
    with np.errstate(all="ignore"):
        for j in range(L):
            w = xw[j]
            # negative branch: x_j > Q_j ? +(x_j - Q_j) : -(Q_j - x_j), no borrow between words
            diff = w - qw[j]
            up = np.array([int(d) > 0 for d in diff], dtype=bool)
            mag = np.where(up, diff, -diff)
            zero_n = np.array([int(m) == 0 for m in mag], dtype=bool)
            term_n = np.where(zero_n, 0.0, to_double(mag) * scaled)
            # non-negative branch
            zero_p = np.array([int(v) == 0 for v in w], dtype=bool)
            term_p = np.where(zero_p, 0.0, to_double(w) * scaled)
            res = np.where(neg, np.where(up, res + term_n, res - term_n), res + term_p)
            scaled = scaled * TWO_POW_64
    return res


def decode_coeffs(enc, res_real, is_complex=False):
    """steps 4 and 5 on the converted real parts (imaginary parts +0.0, ckks.h:712)."""
    n = res_real.shape[0]
    z = np.zeros(n, dtype=np.complex128)
    z.real = res_real
    out = enc.fft_to_rev(z)[enc.index_map[: n // 2]]
    return out if is_complex else np.ascontiguousarray(out.real)


def decode(octx, enc, plain_ntt, L, scale, prime_index=None, is_complex=False):
    """plain_ntt [L][N] NTT form under primes prime_index (None = 0..L-1) -> the reference's decoded slots."""
    idx = list(range(L)) if prime_index is None else [int(i) for i in prime_index]
    primes = [octx.primes[i] for i in idx]
    coeff = octx.ntt(np.asarray(plain_ntt, dtype=np.uint64).reshape(1, L, -1), L, prime_index=prime_index,
                     inverse=True).reshape(L, -1)
    x = compose(coeff, primes)
    return decode_coeffs(enc, convert(x, primes, scale), is_complex)
