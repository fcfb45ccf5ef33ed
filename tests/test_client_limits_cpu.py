"""The constructors of tests/client_limit_cases.py that the client-side GPU limit tests stand on, pinned against the CPU oracle,
the decode comparator and exact Python integers.  No GPU."""
import numpy as np
import pytest

import client_limit_cases as CL
import mode_limits as ML
import oracle as O
import seal_decode as SD

K = 9


def _chain(logn):
    primes = ML.ordered(logn, "g61_last")
    octx = O.Context(logn, primes)
    return primes, octx, O.CkksEncoder(octx)


# ---- encoder ----------------------------------------------------------------------------------------------------------------
def test_encoder_magnitudes_list():
    primes = ML.ordered(12, "g61_last")
    small = CL.small_prime(primes)
    assert small == ML.chain(12)["small"] and (small << 12).bit_length() == 53
    cases = CL.encoder_magnitudes(primes)
    assert len(cases) == len(set(cases)) == 12 * 4 * 2
    assert {sh for _, sh, _ in cases} == {0, 1, 11, 12, 13, 63, 64, 75, 76, 126, 127, 200}
    assert {m for m, _, _ in cases} == {1 << 52, (1 << 52) + 1, (1 << 53) - 1, small << 12}
    assert {s for _, _, s in cases} == {1, -1}
    # the bit counts of the coefficients cover the reference's three branches (<= 64, <= 128, more) on both sides of each boundary
    bits = {int(np.ceil(np.log2(float(m << sh)))) + 1 for m, sh, _ in cases}  # what the reference branches on, in its doubles
    assert {53, 54, 64, 65, 128, 129, 254} <= bits and min(bits) == 53 and max(bits) == 254


@pytest.mark.parametrize("logn", [3, 12, 13, 16])
def test_encoder_magnitudes_encode_to_one_exact_coefficient(logn):
    """the oracle's encoding of the constant sign * mantissa at scale 2^sh, inverse-transformed: coefficient 0 is sign * mantissa * 2^sh
    mod q in Python integers, every other coefficient 0; the multiples of the 41-bit prime have residue 0 under it and no other"""
    primes, octx, enc = _chain(logn)
    small = CL.small_prime(primes)
    seen = set()
    for m, sh, sign in CL.encoder_magnitudes(primes):
        got, nb = enc.encode(CL.constant_slots(sign * m, logn), K, 2.0**sh, return_bits=True)
        coeff = octx.ntt(got[None], K, inverse=True)[0]
        assert not coeff[:, 1:].any(), (m, sh, sign)
        want = [sign * (m << sh) % q for q in primes]
        assert coeff[:, 0].tolist() == want, (m, sh, sign)
        assert nb == int(np.ceil(np.log2(float(m << sh)))) + 1
        seen.add(0 if nb <= 64 else 1 if nb <= 128 else 2)
        if m == small << 12:
            assert [w == 0 for w in want] == [q == small for q in primes]
        else:
            assert all(want)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("logn", [3, 13])
def test_rounding_constants(logn):
    primes, octx, enc = _chain(logn)
    consts = CL.rounding_constants()
    assert [c for c, _ in consts] == [2.0**52 - 0.5, -(2.0**52 - 0.5), 2.0**51 + 0.5, -(2.0**51 + 0.5), 0.49999999999999994,
                                      -0.49999999999999994, 0.5, -0.5, 2.0**53 - 1, -(2.0**53 - 1)]
    assert [v for _, v in consts] == [1 << 52, -(1 << 52), (1 << 51) + 1, -(1 << 51) - 1, 0, 0, 1, -1, (1 << 53) - 1, 1 - (1 << 53)]
    assert np.floor(0.49999999999999994 + 0.5) == 1.0  # what the constant is there for
    for c, v in consts:
        coeff = octx.ntt(enc.encode(CL.constant_slots(c, logn), K, 1.0)[None], K, inverse=True)[0]
        assert not coeff[:, 1:].any(), c
        assert coeff[:, 0].tolist() == [v % q for q in primes], c
        # the restated coefficient is the constant itself: the rounding is the encoder's, not the transform's
        r = CL.restated_coefficients(enc, CL.constant_slots(c, logn), 1.0)
        assert r[0] == c and not r[1:].any()


@pytest.mark.parametrize("logn", [13, 16])
def test_straddling_vectors_straddle_inside_a_thread(logn):
    """some thread of ckks_fft_finish (the coefficients p + k 4096) holds a coefficient below 2^53, one in [2^53, 2^64) and one at or
    above 2^64.  At N = 2^13 a thread holds two coefficients, so there the three classes cannot meet in one: a thread with the first
    and the last, and a thread with the second and the last, take its place (both send an element with no shift through the shifted
    path)."""
    primes, octx, enc = _chain(logn)
    vecs = CL.straddling_vectors(enc, logn, np.random.default_rng(6300 + logn))
    assert len(vecs) == 3
    total = np.zeros(3, dtype=int)
    for v, scale in vecs:
        assert v.shape == ((1 << logn) // 2,) and np.log2(scale) == int(np.log2(scale))
        c = CL.restated_coefficients(enc, v, scale)
        t = np.array(CL.straddling_threads(c, logn))
        assert t[1] > 0 and t[2] > 0
        if logn > 13:
            assert t[0] > 0
        total += t
        enc.encode(v, K, scale)  # fits the chain
    # straddling_threads against a plain restatement of the three classes
    a = np.abs(c)
    n = 1 << logn
    count = 0
    for p in range(4096):
        col = a[p::4096]
        assert col.size == n // 4096
        count += bool((col < 2.0**53).any() and ((col >= 2.0**53) & (col < 2.0**64)).any() and (col >= 2.0**64).any())
    assert count == t[0]


def test_restated_coefficients_round_to_the_encoding():
    """the restatement is what the encoder rounds: round half away from zero of it, reduced, is the oracle's encoding"""
    logn = 8
    primes, octx, enc = _chain(logn)
    rng = np.random.default_rng(3)
    for v in (rng.normal(size=128) + 1j * rng.normal(size=128), rng.normal(size=128), rng.normal(size=42) + 1j * rng.normal(size=42)):
        c = CL.restated_coefficients(enc, v, 2.0**40)
        ints = [int(np.sign(x) * np.floor(abs(x) + 0.5)) for x in c]
        coeff = octx.ntt(enc.encode(v, K, 2.0**40)[None], K, inverse=True)[0]
        for r, q in enumerate(primes):
            assert coeff[r].tolist() == [x % q for x in ints]


# ---- decoder ----------------------------------------------------------------------------------------------------------------
def test_decoder_chain_and_its_word_table():
    primes = CL.decoder_chain()
    assert len(set(primes)) == 64 and primes[0] == ML.chain(3)["g61"] and primes == sorted(primes, reverse=True)
    assert all(ML.is_prime(q) and q % 16 == 1 and q.bit_length() == 61 for q in primes)
    assert CL.DEC_LEVELS == (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 34, 64)
    words = {L: CL.words_of_product(primes[:L]) for L in CL.DEC_LEVELS}
    assert words == CL.DEC_WORDS == {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 8: 8, 9: 9, 16: 16, 17: 17, 32: 31, 33: 32, 34: 33, 64: 61}
    by_nw = {}
    for L, w in words.items():
        by_nw.setdefault(CL.instantiation(w), []).append(w)
    assert sorted(by_nw) == [1, 2, 4, 8, 16, 32, 64]
    for nw in (2, 4, 8, 16, 32):
        assert nw in by_nw[nw] and nw // 2 + 1 in by_nw[nw]
    assert by_nw[64] == [33, 61]
    O.Context(3, primes)


@pytest.mark.parametrize("L", CL.DEC_LEVELS)
def test_composed_values(L):
    primes = CL.decoder_chain()[:L]
    names, xs, res = CL.composed_values(primes)
    Q = SD.product(primes)
    W = CL.DEC_WORDS[L]
    T = (Q + 1) >> 1
    assert len(names) == len(set(names)) == len(xs) == len(set(xs)) and res.shape == (len(xs), L)
    assert all(0 <= x < Q for x in xs)
    # the comparator's composition gives each x back
    back = SD.compose(np.ascontiguousarray(res.T), primes)
    assert [int(v) for v in back] == xs
    have = set(xs)
    P = [1]
    for q in primes:
        P.append(P[-1] * q)
    expect = {0, 1, T - 1, T, T + 1, Q - 1}
    expect |= {v for j in range(W) for v in ((1 << 64 * j) - 1, 1 << 64 * j)}
    expect |= {v for i in range(L) for v in (P[i] - 1, P[i], P[i] + 1)}
    expect |= {Q - (1 << 64 * k) + d for k in range(1, W) for d in (-1, 0, 1)}
    if W > 1:
        expect |= {(1 << 64) - 1, 1 << 64}
    expect = {v for v in expect if 0 <= v < Q}
    assert expect <= have and len(have - expect) <= 1
    # mixed-radix digits: all q_i - 1 is Q - 1, and P_i has the single digit 1
    assert sum((q - 1) * P[i] for i, q in enumerate(primes)) == Q - 1
    qw = [(Q >> 64 * j) & CL.MASK64 for j in range(W)]
    for k in range(1, W):
        x = Q - (1 << 64 * k)
        assert [(x >> 64 * j) & CL.MASK64 for j in range(k)] == qw[:k] and (x >> 64 * k) & CL.MASK64 == qw[k] - 1 and x >= T
        assert (x + 1) & CL.MASK64 == qw[0] + 1
    if W > 1:
        x = xs[names.index("low above, high below")]
        assert x >= T and x & CL.MASK64 > qw[0] and any((x >> 64 * j) & CL.MASK64 < qw[j] for j in range(1, W))
    # the conversion at the test's scale: finite throughout up to L = 17; beyond, finite below 2^1984 and exactly the listed names
    # overflow in the comparator itself
    scale = CL.decoder_scale(L)
    conv = SD.convert(np.array(xs, dtype=object), primes, scale)
    bad = {nm for nm, v in zip(names, conv) if not np.isfinite(v)}
    assert bad == CL.overflow_names(L)
    if L <= 17:
        assert scale == 2.0**40 and not bad
    else:
        assert scale == 2.0**1000
        assert all(np.isfinite(v) for x, v in zip(xs, conv) if x < 1 << 1984)
    if L == 64:
        assert conv[names.index("Q-1")] == -(2.0**-1000)
        assert np.isnan(conv[names.index("T")])
        # above 2^1984 and finite: only low words differ from Q's
        assert all(np.isfinite(conv[names.index(nm)]) for nm in ("Q-2^(64*1)", "Q-2^(64*31)+1", "Q-2^(64*31)-1"))


def test_coefficient_rows_layouts():
    res = np.arange(1, 31, dtype=np.uint64).reshape(10, 3)
    one = CL.coefficient_rows(res, 8)
    assert one.shape == (10, 3, 8) and (one[:, :, 0] == res).all() and not one[:, :, 1:].any()
    full = CL.coefficient_rows(res, 8, fill=True)
    assert full.shape == (2, 3, 8)
    assert (full[0].T == res[:8]).all() and (full[1].T[:2] == res[8:]).all() and (full[1].T[2:] == res[:6]).all()


@pytest.mark.parametrize("L", [2, 64])
def test_single_coefficient_decodes_to_its_conversion_in_every_slot(L):
    """the identity the GPU test uses to see one coefficient on its own: x in coefficient 0 and zeros elsewhere decode to (res, +0.0) in
    every slot, res = the conversion of x, wherever that is finite"""
    primes = CL.decoder_chain()
    octx = O.Context(CL.DEC_LOGN, primes)
    enc = O.CkksEncoder(octx)
    names, xs, res = CL.composed_values(primes[:L])
    scale = CL.decoder_scale(L)
    conv = SD.convert(np.array(xs, dtype=object), primes[:L], scale)
    plain = octx.ntt(CL.coefficient_rows(res, 8), L)
    for i in range(0, len(xs), 7):
        got = SD.decode(octx, enc, plain[i], L, scale, is_complex=True)
        if np.isfinite(conv[i]):
            assert (got.real.view(np.uint64) == conv[i : i + 1].view(np.uint64)).all(), names[i]
            assert (np.ascontiguousarray(got.imag).view(np.uint64) == 0).all(), names[i]
        else:
            assert not np.isfinite(got).any()
