"""Pins tests/exchange_edge_cases.py: every constructor has the property its GPU test (tests/test_gpu_sealprng_edges.py,
tests/test_gpu_wire_edges.py) rests on, shown from the restatements tests/seal_format.py and tests/wire_format.py alone.  CPU
only, and the library is never loaded."""
import numpy as np

import exchange_edge_cases as X
import mode_limits as ML
import seal_format as SF
import wire_format as WF


def _tail_start(L, n):
    """(buffer, word in it) of the first word after the bulk"""
    return divmod(L * n, X.BUF_WORDS)


def _rejection_share(q):
    return ((1 << 64) - 1 - SF.max_multiple(q)) / 2.0**64


# ---- primes -------------------------------------------------------------------------------------------------------------------
def test_rejecting_primes():
    for q, d in zip(X.w_primes(), X.DIVISORS):
        assert q % (2 * X.W_N) == 1 and q < 1 << 60
        assert 1 / (d + 1) < _rejection_share(q) < 1 / (d - 1)
    p = X.w3_primes()
    assert p[2] == 2049638230412492801 and p[2].bit_length() == 61 and 0.111 < _rejection_share(p[2]) < 0.1112
    assert p[1] < 1 << 60 and p[1].bit_length() == 60 and _rejection_share(p[1]) < 2.0**-28
    assert p[3].bit_length() == 46 and _rejection_share(p[3]) < 2.0**-17
    assert all(q % (2 * X.W_N) == 1 and ML.is_prime(q) for q in p) and len(set(p)) == 5
    _, primes, _ = X.n1()
    assert len(set(primes)) == 63 and all(q.bit_length() == 60 and q % 512 == 1 and ML.is_prime(q) for q in primes)
    for logn in (1, 3):
        primes, seeds = X.n2(logn)
        assert len(set(primes)) == 64 and all(q % (2 << logn) == 1 and ML.is_prime(q) for q in primes) and len(set(seeds)) == 40
    (q,) = X.b1_primes()
    assert q % 128 == 1 and 1 / 41 < _rejection_share(q) < 1 / 39


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def test_w1_refills_the_tail_from_a_buffer_boundary():
    primes, seeds = X.w1()
    assert len(seeds) == 2 and _tail_start(len(primes), X.W_N) == (32, 0)
    for s, (res, rejected) in zip(seeds, X.samples(seeds, primes, X.W_N)):
        print("W1 rejections", rejected)
        assert sum(rejected) > X.BUF_WORDS                      # every rejection takes one tail word: buffer 33 is generated
        marks = X.bulk_marks(s, primes, X.W_N)
        assert (marks.sum(axis=1) > 64).all()                   # every row, more marks than a ballot holds
        assert all(c >= m for c, m in zip(rejected, marks.sum(axis=1)))
        assert all((res[r] < np.uint64(q)).all() for r, q in enumerate(primes))


def test_w2_marks_at_the_edges():
    primes = X.w_primes()
    tags = X.w2_tags()
    print("W2 tags", tags)
    assert all(0 <= t < X.SEARCH_CAP for t in tags.values())
    n = X.W_N
    assert X.bulk_marks(X.seed("W2", tags["first"]), primes, n)[0, 0]
    assert X.bulk_marks(X.seed("W2", tags["last"]), primes, n)[3, n - 1]
    groups = X.bulk_marks(X.seed("W2", tags["lanes"]), primes, n)[0].reshape(-1, 64)
    assert (groups[:, 0] & groups[:, 63]).any()
    assert (groups.sum(axis=1) >= 2).any()
    row = X.bulk_marks(X.seed("W2", tags["run"]), primes, n)[0]
    assert (row[:-2] & row[1:-1] & row[2:]).any()
    _, seeds = X.w2()
    assert len(seeds) == len(set(tags.values())) and set(seeds) == {X.seed("W2", t) for t in tags.values()}
    # the restatement serves these marks like any other: the sample at a marked place is a residue
    for s, (res, _) in zip(seeds, X.samples(seeds, primes, n)):
        assert all((res[r] < np.uint64(q)).all() for r, q in enumerate(primes))


def test_w3_rows_without_marks_between_rejecting_rows():
    primes, seeds = X.w3()
    assert len(seeds) == 2 and primes[2].bit_length() == 61
    for order in (primes, primes[::-1]):
        for s, (_, rejected) in zip(seeds, X.samples(seeds, order, X.W_N)):
            marks = X.bulk_marks(s, order, X.W_N).sum(axis=1)
            print("W3 marks per row", marks.tolist(), "rejections", rejected)
            assert marks[1] == marks[3] == rejected[1] == rejected[3] == 0
            assert all(marks[r] > 100 for r in (0, 2, 4))


def test_n1_refills_the_tail_twice_from_mid_buffer():
    logn, primes, seeds = X.n1()
    n = 1 << logn
    assert n < X.BUF_WORDS and len(primes) == 63 and len(seeds) == 2
    assert _tail_start(63, n) == (31, 256)
    for s, (_, rejected) in zip(seeds, X.samples(seeds, primes, n)):
        print("N1 rejections", sum(rejected))
        assert sum(rejected) > 256 + X.BUF_WORDS               # past the end of buffer 31 and past all of buffer 32
        assert min(rejected) >= 1 and X.bulk_marks(s, primes, n).any(axis=1).all()


def test_n2_tiny_degrees_with_64_rows():
    for logn in (1, 3):
        primes, seeds = X.n2(logn)
        got = X.samples(seeds, primes, 1 << logn)
        total = sum(sum(rej) for _, rej in got)
        print("N2 logn %d rejections %d" % (logn, total))
        assert total > 0 and all(res.shape == (64, 1 << logn) for res, _ in got)
        if logn == 1:
            assert any(rej[63] for _, rej in got)
    assert _tail_start(64, 2) == (0, 128) and _tail_start(64, 8) == (1, 0)


def test_b1_seeds_without_marks_in_both_full_launches():
    (q,), seeds = X.b1()
    tags, looked_at = X.b1_tags()
    print("B1: %d tags looked at" % looked_at)
    assert looked_at <= X.SEARCH_CAP and len(seeds) == len(set(seeds)) == X.B1_COUNT == 2 * X.B1_CHUNK + 1
    clean = [i for i, s in enumerate(seeds) if not X.bulk_marks(s, [q], X.B1_N).any()]
    assert clean == list(X.B1_CLEAN_AT)
    assert [i // X.B1_CHUNK for i in clean] == [0, 1]           # one in each launch of 32; the launch of one seed has marks
    for i, (res, rejected) in enumerate(X.samples(seeds, [q], X.B1_N)):
        assert (rejected[0] == 0) == (i in clean)
    # no two seeds give the same residues: a polynomial written from another seed's state cannot pass
    rows = {X.sample(s, (q,), X.B1_N)[0].tobytes() for s in seeds}
    assert len(rows) == X.B1_COUNT


def test_l1_limit_chain():
    logn, primes, seeds = X.l1()
    assert primes == ML.ordered(12, "g61_last") and len(primes) == 9 and len(seeds) == 3
    assert sorted(q.bit_length() for q in primes) == sorted([47, 47, 51, 52, 59, 59, 60, 61, 41])
    for res, _ in X.samples(seeds, primes, 1 << logn):
        assert all((res[r] < np.uint64(q)).all() for r, q in enumerate(primes))


def test_prng_ranges():
    assert sorted(nb for first, nb in X.PRNG_RANGES if first == 7) == [1, 15, 16, 17, 63, 64, 65]
    first, nb = X.PRNG_RANGES[-1]
    assert first + nb - 1 == (1 << 64) - 1                      # the last counter there is: no wrap, so not the error case
    s = X.seed("PRNG", 0)
    top = SF.prng_buffers(s, (1 << 64) - 1, 1)
    assert len(top) == 4096 and top != SF.prng_buffers(s, (1 << 32) - 1, 1) and top != SF.prng_buffers(s, 0, 1)


def test_check_plants():
    plants = X.check_plants(1024, 3, 3)
    assert len(plants) == len(set(plants)) == 16
    assert {p for p, _, _ in plants} == {0, 2} and {r for _, r, _ in plants} == {0, 2}
    assert {i for _, _, i in plants} == {0, 255, 256, 1023}


# ---- the wire form ------------------------------------------------------------------------------------------------------------
def test_width_primes():
    for logn, count, lowest in ((12, 46, 16), (16, 42, 20)):
        primes = X.width_primes(logn)
        bits = [WF.bit_length(q) for q in primes]
        assert bits == list(range(lowest, 62)) and len(primes) == count <= 64
        assert all(q % (2 << logn) == 1 and ML.is_prime(q) for q in primes)
        assert max(bits) << logn <= 61 << 16                    # the largest bit offset of the reciprocal's claim
    for logn in (1, 2, 3, 4, 5, 6):
        bits = [WF.bit_length(q) for q in X.width_primes(logn)]
        assert len(bits) >= 45 and min(bits) < 32 <= max(bits) == 61  # both of wire_pack's paths


def test_canonical_rows():
    for logn in (1, 6, 12):
        n, primes = 1 << logn, X.width_primes(logn)
        polys = X.canonical(primes, n, 2, np.random.default_rng(logn))
        for r, q in enumerate(primes):
            assert (polys[:, r] < np.uint64(q)).all() and (polys[:, r, 0] == 0).all() and (polys[:, r, n - 1] == q - 1).all()
            assert n == 2 or (polys[:, r, n - 2] == q - 1).all()
        words = WF.pack_rows(polys, primes)
        back, invalid = WF.unpack_rows(words, 2, n, primes)
        assert not invalid and (back == polys).all()


def test_high_bits_are_outside_the_field():
    for logn in (6, 12):
        n, primes = 1 << logn, X.width_primes(logn)
        rng = np.random.default_rng(60 + logn)
        polys = X.canonical(primes, n, 1, rng)
        for garbage in (rng.integers(0, 1 << 63, size=polys.shape, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                        np.full(polys.shape, (1 << 64) - 1, dtype=np.uint64)):
            dirty = X.with_high_bits(polys, primes, garbage)
            for r, q in enumerate(primes):
                b = WF.bit_length(q)
                assert (dirty[0, r] & np.uint64((1 << b) - 1) == polys[0, r]).all()
                assert (dirty[0, r] >> np.uint64(b) != 0).all()  # bit b of every word is set: the garbage is odd
        assert (dirty[0] >> np.array([[WF.bit_length(q)] for q in primes], dtype=np.uint64)
                == np.array([[(1 << (64 - WF.bit_length(q))) - 1] for q in primes], dtype=np.uint64)).all()


def test_padding_ones():
    for logn in (1, 2, 3, 4, 5):
        n, primes = 1 << logn, X.width_primes(logn)
        rows = X.padded_rows(n, primes)
        assert rows and rows == [r for r, q in enumerate(primes) if WF.bit_length(q) % (64 >> logn)]
        polys = X.canonical(primes, n, 2, np.random.default_rng(70 + logn))
        clean = WF.pack_rows(polys, primes)
        dirty = X.with_padding_ones(clean, n, primes, 2)
        pw = WF.packed_words(n, primes)
        differ = (dirty != clean).reshape(2, pw)
        ends = np.cumsum([WF.row_words(n, WF.bit_length(q)) for q in primes]) - 1
        assert (differ.sum(axis=1) == len(rows)).all() and differ[:, ends[rows]].all()
        for r in rows:  # every bit from n b on is set, none below is touched
            used = n * WF.bit_length(primes[r]) % 64
            assert (dirty.reshape(2, pw)[:, ends[r]] >> np.uint64(used) == np.uint64((1 << (64 - used)) - 1)).all()
            assert ((dirty ^ clean).reshape(2, pw)[:, ends[r]] & np.uint64((1 << used) - 1) == 0).all()
        back, invalid = WF.unpack_rows(dirty, 2, n, primes)
        assert not invalid and (back == polys).all()


def test_validity_plants():
    for logn, bits in X.VALIDITY_SHAPES:
        n, L = 1 << logn, len(bits)
        plants = X.validity_plants(logn, L, 3)
        assert len(plants) == len(set(plants)) == (8 if logn == 4 else 16)
        assert {i for _, _, i, _ in plants} == {0, 1, n - 2, n - 1}
        for i in (0, 1, n - 2, n - 1):  # every slot sees both kinds
            assert {kind for _, _, j, kind in plants if j == i} == {"q", "ones"}
        if logn == 12:
            assert {(p, r) for p, r, _, _ in plants} == {(0, 0), (0, L - 1), (2, 0), (2, L - 1)}
    assert X.bad_value(1073479681, "q") == 1073479681 and X.bad_value(1073479681, "ones") == (1 << 30) - 1
