"""The directed inputs of the exchange-path edge tests (tests/test_gpu_wire_edges.py for csrc/wire.hip,
tests/test_gpu_sealprng_edges.py for csrc/sealprng.hip): primes that reject a known share of the generator's words, seeds whose
rejected words (the kernels' "marks") lie where the fill and fix-up kernels branch, and wire-form inputs with bits where the
format says they are ignored.  tests/test_exchange_edges_cpu.py pins every constructor against the restatements
(tests/seal_format.py, tests/wire_format.py), so that a GPU test cannot pass on inputs that miss their branch.  No GPU and no
library: the restatements and exact integers only.

Nothing random enters: a seed is SHA-512 of a fixed text and a tag, and where a case needs a seed with a property the tags
0, 1, 2, ... are tried in order and the first hit is kept (at most SEARCH_CAP tags; the expected number is 1 / p, about 20 for the
rarest property).  The searches and the restatement's samples are computed on first use and kept, so that collecting the GPU
files costs nothing; whoever receives a kept array must not write to it."""
import functools
import hashlib

import numpy as np

import mode_limits as ML
import seal_format as SF
import wire_format as WF
from test_gpu_ntt_lazy16 import ntt_prime
from test_gpu_seal_format import _primes_above
from test_gpu_wire import _ntt_prime

SEARCH_CAP = 200
BUF_WORDS = SF.BUFFER_BYTES // 8  # 512: one generator buffer, and the size of seal_fixup's tail buffer
DIVISORS = (17, 40, 33, 20)       # a prime just above 2^64 / d rejects about 1 / d of all words


def seed(name, tag):
    return hashlib.sha512(b"exchange edge seed %s %d" % (name.encode(), tag)).digest()


def stream_words(s, first_buffer, count):
    """uint64 [512 count]: buffers first_buffer .. of Blake2xbPRNG(s) as the words sample_poly_uniform reads"""
    return np.frombuffer(SF.prng_buffers(s, first_buffer, count), dtype="<u8").astype(np.uint64)


def is_mark(word, q):
    return int(word) >= SF.max_multiple(int(q))


def bulk_marks(s, primes, n):
    """bool [L][n]: which of the first L n words sample_poly_uniform rejects (what seal_fill stores as marks)"""
    L = len(primes)
    words = stream_words(s, 0, -(-L * n // BUF_WORDS))[: L * n].reshape(L, n)
    mm = np.array([SF.max_multiple(int(q)) for q in primes], dtype=np.uint64)
    return words >= mm[:, None]


def first_tag(name, has):
    """the first tag whose seed has the property"""
    for tag in range(SEARCH_CAP):
        if has(seed(name, tag)):
            return tag
    raise AssertionError("no seed of %s within %d tags" % (name, SEARCH_CAP))


@functools.lru_cache(maxsize=None)
def sample(s, primes, n):
    """SF.sample_poly_uniform, kept: (residues [L][n], rejections per row)"""
    return SF.sample_poly_uniform(s, list(primes), n)


def samples(seeds, primes, n):
    return [sample(s, tuple(int(q) for q in primes), n) for s in seeds]


# ---- the sampler: wide fill (N >= 512) --------------------------------------------------------------------------------------
W_LOGN, W_N = 12, 1 << 12


@functools.lru_cache(maxsize=None)
def w_primes():
    """the first prime = 1 mod 2N above 2^64 / d for d = 17, 40, 33, 20"""
    return [_primes_above(W_N, d, 1)[0] for d in DIVISORS]


def w1():
    """(primes, seeds): L N = 32 buffers, so the tail starts at word 0 of buffer 32; every seed rejects more than 512 words and
    more than 64 in every row"""
    return w_primes(), [seed("W1", t) for t in range(2)]


def _has_edge_lanes(m):
    g = m.reshape(-1, 64)
    return bool((g[:, 0] & g[:, 63]).any())


def _has_run_of_three(m):
    return bool((m[:-2] & m[1:-1] & m[2:]).any())


@functools.lru_cache(maxsize=None)
def w2_tags():
    """{property: tag} under w_primes(): a mark at coefficient 0 of row 0, one at coefficient N - 1 of row 3 (the first and the last
    word of the bulk), a 64-aligned group of row 0 whose lanes 0 and 63 are both marks, and three adjacent marks in row 0.  The
    first two look at one word, so only its buffer is generated."""
    primes = w_primes()
    last = 4 * W_N - 1
    return {
        "first": first_tag("W2", lambda s: is_mark(stream_words(s, 0, 1)[0], primes[0])),
        "last": first_tag("W2", lambda s: is_mark(stream_words(s, last // BUF_WORDS, 1)[last % BUF_WORDS], primes[3])),
        "lanes": first_tag("W2", lambda s: _has_edge_lanes(bulk_marks(s, primes[:1], W_N)[0])),
        "run": first_tag("W2", lambda s: _has_run_of_three(bulk_marks(s, primes[:1], W_N)[0])),
    }


def w2():
    """(primes, seeds): the distinct seeds of w2_tags(), in the order of their tags"""
    return w_primes(), [seed("W2", t) for t in sorted(set(w2_tags().values()))]


@functools.lru_cache(maxsize=None)
def w3_primes():
    """rejecting (d = 17), just below 2^60 (rejects less than 2^-28), rejecting 61 bits (d = 9), 46 bits, rejecting (d = 20)"""
    return [w_primes()[0], ntt_prime(W_LOGN, (1 << 60) - 1, -1), _primes_above(W_N, 9, 1)[0], _ntt_prime(W_N, 46), w_primes()[3]]


def w3():
    """(primes, seeds): rows 1 and 3 without marks between rows 0, 2 and 4 with more than 100 each"""
    return w3_primes(), [seed("W3", t) for t in range(2)]


# ---- the sampler: narrow fill (N < 512) -------------------------------------------------------------------------------------
def n1():
    """(logn, primes, seeds): N = 256, L = 63; L N = 31.5 buffers, so the tail starts at word 256 of buffer 31, and more than
    256 + 512 rejections carry it through two refills"""
    return 8, _primes_above(256, 17, 63), [seed("N1", t) for t in range(2)]


def n2(logn):
    """(primes, seeds): N = 2 or 8 with the full 64 rows, 40 seeds"""
    return _primes_above(1 << logn, 17, 64), [seed("N2 logn %d" % logn, t) for t in range(40)]


# ---- the sampler: more seeds than one launch holds ----------------------------------------------------------------------------
B1_LOGN, B1_N, B1_COUNT, B1_CHUNK = 6, 64, 65, 32
B1_CLEAN_AT = (5, 32 + 17)  # where the seeds without a mark stand: one in each full chunk, neither first nor last in it


@functools.lru_cache(maxsize=None)
def b1_tags():
    """(tags of the 65 seeds in call order, number of tags looked at): tags in ascending order, 63 whose single row has a mark
    and, at the places of B1_CLEAN_AT, the first two that have none"""
    (q,) = b1_primes()
    marked, clean, tag = [], [], 0
    while len(marked) < B1_COUNT - len(B1_CLEAN_AT) or len(clean) < len(B1_CLEAN_AT):
        assert tag < SEARCH_CAP
        words = stream_words(seed("B1", tag), 0, 1)[:B1_N]
        (marked if any(is_mark(w, q) for w in words) else clean).append(tag)
        tag += 1
    order = marked[: B1_COUNT - len(B1_CLEAN_AT)]
    for at, t in zip(B1_CLEAN_AT, clean):
        order.insert(at, t)
    return tuple(order), tag


def b1_primes():
    return _primes_above(B1_N, 40, 1)


def b1():
    """(primes, seeds): launches of seeds 0 - 31, 32 - 63 and 64"""
    return b1_primes(), [seed("B1", t) for t in b1_tags()[0]]


# ---- the sampler: the arithmetic modes' limit chain ---------------------------------------------------------------------------
def l1():
    """(logn, primes, seeds): full 64-bit words into barrett64 under the nine limit primes"""
    return 12, ML.ordered(12, "g61_last"), [seed("L1", t) for t in range(3)]


# ---- the generator alone ------------------------------------------------------------------------------------------------------
# (first_block, n_blocks): a wavefront owns 16 buffers and a workgroup 64; the last case ends at counter 2^64 - 1 without wrapping
PRNG_RANGES = [(7, nb) for nb in (1, 15, 16, 17, 63, 64, 65)] + [((1 << 64) - 17, 17)]


# ---- the residue check --------------------------------------------------------------------------------------------------------
def check_plants(n, L, n_poly):
    """[(polynomial, row, coefficient)]: both ends of a row and both sides of a workgroup's edge (256 coefficients), in the first
    and the last row of the first and the last polynomial"""
    return [(p, r, i) for p in (0, n_poly - 1) for r in (0, L - 1) for i in (0, 255, 256, n - 1)]


# ---- the wire form ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def width_primes(logn):
    """one NTT prime for every bit length that has one at this degree, ascending"""
    return [q for q in (_ntt_prime(1 << logn, b) for b in range(3, 62)) if q]


def canonical(primes, n, n_poly, rng):
    """uint64 [n_poly][L][n] below the row's prime, with coefficient 0 = 0 and coefficients n - 2 and n - 1 = q - 1 (n - 1 alone at
    n = 2): the first field of a row empty, its last fields as full as a residue gets"""
    out = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in primes]) for _ in range(n_poly)])
    out[:, :, 0] = 0
    for r, q in enumerate(primes):
        out[:, r, max(n - 2, 1):] = q - 1
    return out


def with_high_bits(polys, primes, garbage):
    """polys | (garbage << b_r): the low b_r bits of every word stay, the bits above them are garbage's"""
    out = polys.copy()
    for r, q in enumerate(primes):
        out[:, r] |= np.asarray(garbage[:, r], dtype=np.uint64) << np.uint64(WF.bit_length(q))
    return out


def padded_rows(n, primes):
    """rows whose n b_r bits end inside a word"""
    return [r for r, q in enumerate(primes) if n * WF.bit_length(q) % 64]


def with_padding_ones(words, n, primes, n_poly):
    """the packed polynomials with every padding bit (beyond bit n b_r of a row's last word) set"""
    out = np.array(words, dtype=np.uint64).reshape(n_poly, -1)
    pos = 0
    for q in primes:
        b = WF.bit_length(q)
        pos += WF.row_words(n, b)
        used = n * b % 64
        if used:
            out[:, pos - 1] |= np.uint64(((1 << 64) - 1) >> used << used)
    assert pos == out.shape[1]
    return out.reshape(-1)


VALIDITY_SHAPES = [(4, [30, 31]), (12, [51, 46, 46, 58])]


def validity_plants(logn, L, n_poly):
    """[(polynomial, row, coefficient, kind)], kind 'q' for q_r and 'ones' for 2^b - 1: one bad value per call.  N = 16: the even
    and odd slots at both ends of the second row of the middle polynomial.  N = 4096: the same four slots in the first and the
    last row of the first and the last polynomial; the two kinds alternate over the slots and swap between rows, so that each
    slot sees each kind without taking the full product."""
    n = 1 << logn
    slots = (0, 1, n - 2, n - 1)
    if logn == 4:
        return [(1, 1, i, kind) for i in slots for kind in ("q", "ones")]
    return [(p, r, i, ("q", "ones")[(j + (r != 0)) % 2]) for p in (0, n_poly - 1) for r in (0, L - 1) for j, i in enumerate(slots)]


def bad_value(q, kind):
    return int(q) if kind == "q" else (1 << WF.bit_length(q)) - 1
