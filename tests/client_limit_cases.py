"""The directed inputs of the client-side limit tests (tests/test_gpu_encoder_limits.py, test_gpu_decoder_limits.py,
test_gpu_client_limits.py): coefficients on the exponent boundaries of the encoder's integer split, constants on the boundaries
of std::round, slot vectors whose coefficients straddle 2^53 and 2^64 inside one thread of ckks_fft_finish, a chain of 64 primes of
61 bits whose row sets reach every instantiation of dec_compose, and the composed integers on the edges of the decoder's
comparison, sign mix and carries.  tests/test_client_limits_cpu.py pins every constructor, so that a GPU test cannot pass on inputs
that miss their target.  No GPU, exact Python integers and the CPU oracle only."""
import numpy as np

import mode_limits as ML

ORDER_NAMES = ["fpr_hi_last", "g61_last"]
MASK64 = (1 << 64) - 1

# ---- encoder ----------------------------------------------------------------------------------------------------------------
# 2^sh is the scale: sh = 0 leaves the 53-bit mantissa (split_rounded's sh <= 0 arm), 1 .. 11 shift it into 64 bits, 12 and up keep
# the exponent; residue_shifted folds it 63 bits at a time (63 | 64, 126 | 127), and with the 53 bits of the mantissa 11 | 12 is the
# reference's 64-bit branch boundary, 75 | 76 its 128-bit one
ENC_SHIFTS = (0, 1, 11, 12, 13, 63, 64, 75, 76, 126, 127, 200)
ENC_FINISH_TILE_LOG = 12  # ckks_fft_finish: thread p holds the coefficients p + k 4096


def small_prime(primes):
    """the chain's prime just above 2^40"""
    (q,) = [q for q in primes if 1 << 40 < q < 1 << 41]
    return q


def encoder_magnitudes(primes):
    """[(mantissa, sh, sign)]: the constant slot vector sign * mantissa at scale 2^sh encodes to coefficient 0 = sign * mantissa * 2^sh
    exactly and every other coefficient 0.  Mantissas: 2^52 (one bit), 2^52 + 1 and 2^53 - 1 (53 significant bits) and small * 2^12,
    a multiple of the chain's 41-bit prime that fits 53 bits: its residue under that prime is 0 whatever the sign."""
    small = small_prime(primes)
    mantissas = (1 << 52, (1 << 52) + 1, (1 << 53) - 1, small << 12)
    assert all(m < 1 << 53 for m in mantissas)
    return [(m, sh, sign) for sh in ENC_SHIFTS for m in mantissas for sign in (1, -1)]


def constant_slots(value, logn):
    """the real slot vector that holds `value` in every slot"""
    return np.full((1 << logn) // 2, float(value))


def rounding_constants():
    """[(constant, expected integer)] at scale 1: std::round rounds halfway cases away from zero, and 0.49999999999999994 (the largest
    double below 0.5) to 0, where floor(x + 0.5) gives 1"""
    below_half = float(np.nextafter(0.5, 0.0))
    assert repr(below_half) == "0.49999999999999994"
    pos = [(2.0**52 - 0.5, 1 << 52), (2.0**51 + 0.5, (1 << 51) + 1), (below_half, 0), (0.5, 1), (2.0**53 - 1.0, (1 << 53) - 1)]
    return [(s * c, s * v) for c, v in pos for s in (1, -1)]


def conj_values(enc, values):
    """the encoder's input of its inverse transform (SEAL/ckks.h:505-510): values (zero padded to N/2 slots) through the index map,
    their conjugates through its upper half"""
    n = enc.ctx.n
    slots = n // 2
    v = np.zeros(slots, dtype=np.complex128)
    vals = np.asarray(values)
    v[: vals.size] = vals
    z = np.zeros(n, dtype=np.complex128)
    z[enc.index_map[:slots]] = v
    z[enc.index_map[slots:]] = np.conj(v)
    return z


def restated_coefficients(enc, values, scale):
    """the real coefficients before rounding: the oracle's inverse transform with the scalar scale / N folded into its last stage"""
    return np.ascontiguousarray(enc.fft_from_rev(conj_values(enc, values), scalar=float(scale) / enc.ctx.n).real)


def coefficient_classes(c):
    """0: |c| < 2^53 (split_rounded's sh <= 0), 1: 2^53 <= |c| < 2^64 (1 <= sh <= 11), 2: |c| >= 2^64 (sh >= 12)"""
    a = np.abs(c)
    return (a >= 2.0**53).astype(int) + (a >= 2.0**64).astype(int)


def straddling_threads(c, logn):
    """(all three, low with high, middle with high): how many threads of ckks_fft_finish (coefficients p + k 4096) hold coefficients
    of all three classes, of classes 0 and 2, of classes 1 and 2"""
    cls = coefficient_classes(c).reshape(-1, 1 << ENC_FINISH_TILE_LOG)
    has = [(cls == k).any(axis=0) for k in range(3)]
    return int((has[0] & has[1] & has[2]).sum()), int((has[0] & has[2]).sum()), int((has[1] & has[2]).sum())


STRADDLE_SCALES = (2.0**58, 2.0**62, 2.0**66)


def straddling_vectors(enc, logn, rng):
    """[(values, scale)], three standard normal real slot vectors.  A coefficient of such a vector is about scale / sqrt(N), so at
    the scales of STRADDLE_SCALES none reaches 2^64 at N = 2^13 or 2^16; a power-of-two scale multiplies every restated coefficient
    exactly, so each vector gets the power of two that puts the larger coefficient of its widest thread (the thread with the largest
    ratio max |c| / min |c| among those whose smallest coefficient is not 0) into [2^64, 2^65): that thread then holds a coefficient
    below 2^53 as soon as the ratio exceeds 2^12, and most other threads one in [2^53, 2^64) beside one above 2^64."""
    assert logn > ENC_FINISH_TILE_LOG
    out = []
    for scale in STRADDLE_SCALES:
        v = rng.normal(size=(1 << logn) // 2)
        c = restated_coefficients(enc, v, scale)
        if straddling_threads(c, logn)[0] == 0:
            a = np.abs(c).reshape(-1, 1 << ENC_FINISH_TILE_LOG)
            lo, hi = a.min(axis=0), a.max(axis=0)
            ratio = np.where(lo > 0, hi / np.where(lo > 0, lo, 1.0), 0.0)
            p = int(ratio.argmax())
            # hi[p] = f 2^e with 0.5 <= f < 1: times 2^(65 - e) it lies in [2^64, 2^65)
            scale = scale * 2.0 ** (65 - int(np.frexp(hi[p])[1]))
        out.append((v, scale))
    return out


# ---- decoder ----------------------------------------------------------------------------------------------------------------
DEC_LOGN = 3
# row sets: the first L primes of decoder_chain(); the words of Q and the instantiation NW of dec_compose they run (the next power
# of two): both ends of NW = 2, 4, 8, 16, 32 (W = NW and W = NW / 2 + 1), NW = 64 at its smallest W and at the largest 64 primes of
# 61 bits allow.  L = 3 is there for the lower end of NW = 4 (W = 3).
DEC_WORDS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 8: 8, 9: 9, 16: 16, 17: 17, 32: 31, 33: 32, 34: 33, 64: 61}
DEC_LEVELS = tuple(DEC_WORDS)
DEC_SCALE_SHORT = 2.0**40    # L <= 17: every directed value converts to a finite double
DEC_SCALE_LONG = 2.0**1000   # L >= 32: finite below 2^1984 and where only low words differ from Q's

_dec_chain = []


def decoder_chain():
    """64 primes of 61 bits at N = 8: g61 and the next 63 primes = 1 (mod 16) below it"""
    if not _dec_chain:
        g61 = ML.chain(DEC_LOGN)["g61"]
        _dec_chain.extend([g61] + ML.primes_below(DEC_LOGN, g61, 63))
    return list(_dec_chain)


def words_of_product(primes):
    Q = 1
    for q in primes:
        Q *= int(q)
    return (Q.bit_length() + 63) // 64


def instantiation(words):
    nw = 1
    while nw < words:
        nw <<= 1
    return nw


def decoder_scale(L):
    return DEC_SCALE_SHORT if L <= 17 else DEC_SCALE_LONG


def composed_values(primes):
    """(names, xs, residues): the directed x in [0, Q) of the row set `primes` (names are unique; a value reached twice keeps its
    first name), and their residues as uint64 [len(xs)][L].
        0, 1, 2^64 - 1, 2^64
        2^(64 j) - 1, 2^(64 j) for j < W       all-ones words below an empty one; a lone 1 above zero words (skipped, never times inf)
        P_i - 1, P_i, P_i + 1 for i < L        mixed-radix digits (q - 1, .., q - 1, 0, ..), (0, .., 1, 0, ..): the carry into an empty word
        T - 1, T, T + 1                        on either side of upper_half_threshold
        Q - 1                                  every digit q_i - 1 (sum (q_i - 1) P_i telescopes to it); every word but the lowest equals Q's
        Q - 2^(64 k), +- 1 for 1 <= k < W      the words below k equal Q's (diff 0), word k is one below Q's; + 1: the low word above Q's
        low above, high below                  >= T, low word all ones (above Q's), the words above it those of (Q >> 64) - 1"""
    L = len(primes)
    P = [1]
    for q in primes:
        P.append(P[-1] * int(q))
    Q = P[L]
    W = (Q.bit_length() + 63) // 64
    T = (Q + 1) >> 1
    cand = [("0", 0), ("1", 1), ("2^64-1", MASK64), ("2^64", 1 << 64)]
    for j in range(W):
        cand += [("2^(64*%d)-1" % j, (1 << (64 * j)) - 1), ("2^(64*%d)" % j, 1 << (64 * j))]
    for i in range(L):
        cand += [("P_%d-1" % i, P[i] - 1), ("P_%d" % i, P[i]), ("P_%d+1" % i, P[i] + 1)]
    cand += [("T-1", T - 1), ("T", T), ("T+1", T + 1), ("Q-1", Q - 1)]
    for k in range(1, W):
        cand += [("Q-2^(64*%d)-1" % k, Q - (1 << (64 * k)) - 1), ("Q-2^(64*%d)" % k, Q - (1 << (64 * k))),
                 ("Q-2^(64*%d)+1" % k, Q - (1 << (64 * k)) + 1)]
    cand.append(("sum (q_i-1) P_i", sum((int(q) - 1) * P[i] for i, q in enumerate(primes))))
    if W >= 2:
        cand.append(("low above, high below", ((((Q >> 64) - 1) << 64) | MASK64)))
    names, xs, seen = [], [], set()
    for name, x in cand:
        if 0 <= x < Q and x not in seen:
            seen.add(x)
            names.append(name)
            xs.append(x)
    res = np.array([[x % int(q) for q in primes] for x in xs], dtype=np.uint64).reshape(len(xs), L)
    return names, xs, res


def overflow_names(L):
    """the names of composed_values(decoder_chain()[:L]) whose conversion at decoder_scale(L) overflows in the reference itself (inf,
    or NaN where +inf meets -inf): from word 32 on the factor 2^(64 w) / 2^1000 is inf, and 2^984 times word 31 is when that word
    reaches 2^40.  None up to L = 33 (Q < 2^2013 there: word 31 stays below 2^29)."""
    if L <= 33:
        return frozenset()
    if L == 34:  # W = 33, Q about 2^2074 (P_33 < 2^2013 is still finite): word 32 of x, or its difference from Q's
        return frozenset(["2^(64*32)-1", "2^(64*32)", "T-1", "T", "T+1", "Q-2^(64*32)-1", "Q-2^(64*32)", "Q-2^(64*32)+1"])
    assert L == 64
    out = ["T-1", "T", "T+1"]
    out += ["2^(64*%d)%s" % (j, s) for j in range(32, 61) for s in ("-1", "")]
    out += ["P_%d%s" % (i, s) for i in range(34, 64) for s in ("-1", "", "+1")]
    out += ["Q-2^(64*%d)%s" % (k, s) for k in range(32, 61) for s in ("-1", "", "+1")]
    return frozenset(out)


def coefficient_rows(res, n, fill=False):
    """uint64 [plaintexts][L][n] in coefficient form from residues [count][L].  fill = False: value i in coefficient 0 of plaintext i,
    the other coefficients 0; fill = True: the values fill the n coefficients of a plaintext, n at a time (the last one cycles)."""
    count, L = res.shape
    if not fill:
        out = np.zeros((count, L, n), dtype=np.uint64)
        out[:, :, 0] = res
        return out
    plains = (count + n - 1) // n
    idx = np.arange(plains * n) % count
    return np.ascontiguousarray(res[idx].reshape(plains, n, L).transpose(0, 2, 1))
