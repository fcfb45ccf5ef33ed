"""csrc/sealprng.hip on its directed edges, bit for bit against tests/seal_format.py: the branches of seal_fill and seal_fixup
that tests/test_gpu_seal_format.py's seeds never take.  The inputs come from tests/exchange_edge_cases.py, and
tests/test_exchange_edges_cpu.py shows from the restatement alone that each of them reaches its branch: a tail that is refilled
(from a buffer boundary after a wide fill, from the middle of a buffer after a narrow one), marks in the first and last
coefficient of a polynomial, in lanes 0 and 63 of one ballot and side by side, rows without marks between rejecting rows (a
61-bit one among them), N = 2 and 8 with 64 rows, a second and third launch of seeds with polynomials that need no fix-up beside
ones that do, rows under the arithmetic modes' limit primes, the generator at the wavefront's edges and at the top of its
counter, and the residue check at every corner of its grid.

Not exercised: the overflow word (rejected[1]).  A tail must consume 2 L N + 512 words before it is set, and no prime below
2^61 rejects more than 1 / 8 of them."""
import numpy as np
import pytest

import exchange_edge_cases as X
import oracle as O
import seal_format as SF

pytestmark = pytest.mark.gpu


def _check(moai, logn, primes, seeds, prime_index=None):
    """the three comparisons every sampler test makes; returns the restatement's total of rejected words"""
    n = 1 << logn
    ctx = moai.Context(logn, primes)
    sel = [primes[i] for i in prime_index] if prime_index is not None else list(primes)
    L = len(sel)
    want = X.samples(seeds, sel, n)
    out, rejected, overflow = ctx.seal_sample_uniform(seeds, L, prime_index=prime_index)
    got = out.to_numpy((len(seeds), L, n))
    for b in range(len(seeds)):
        assert np.array_equal(got[b], want[b][0]), (b, np.argwhere(got[b] != want[b][0])[:4].tolist())
    total = sum(sum(rej) for _, rej in want)
    print("logn %d L %d count %d: rejected %d (restatement %d)" % (logn, L, len(seeds), rejected, total))
    assert rejected == total
    assert overflow is False
    assert ctx.check_residues(out, len(seeds), L, prime_index) is False
    return total


def test_tail_refills_wide(moai):
    primes, seeds = X.w1()
    assert _check(moai, X.W_LOGN, primes, seeds) > 2 * X.BUF_WORDS


def test_tail_refills_narrow_from_mid_buffer(moai):
    logn, primes, seeds = X.n1()
    assert _check(moai, logn, primes, seeds) > 2 * (256 + X.BUF_WORDS)


def test_marks_at_the_edges_of_rows_and_ballots(moai):
    primes, seeds = X.w2()
    _check(moai, X.W_LOGN, primes, seeds)


def test_rows_without_marks_between_rejecting_rows(moai):
    primes, seeds = X.w3()
    _check(moai, X.W_LOGN, primes, seeds)
    # the rows follow prime_index: the same context, rows in the reverse order
    _check(moai, X.W_LOGN, primes, seeds, prime_index=list(range(len(primes)))[::-1])


@pytest.mark.parametrize("logn", [1, 3])
def test_tiny_degrees_full_row_count(moai, logn):
    primes, seeds = X.n2(logn)
    assert _check(moai, logn, primes, seeds) > 0


def test_second_and_third_seed_chunk(moai):
    """65 seeds are three launches (32, 32, 1) with the output pointer, the mark counts and the generator states advanced per
    launch; in each full launch one polynomial has no mark.  Written to polynomial 1 of every [2][L][N] pair.  A wrong seed or
    output offset in a later launch fails here.  A wrong offset of the mark counts inside their scratch cannot show in any
    result: fill and fix-up of a launch share the pointer, the counts only grow, and the fix-up reads a count as "not zero" and as
    an early-out bound"""
    primes, seeds = X.b1()
    n, L, count = X.B1_N, 1, len(seeds)
    ctx = moai.Context(X.B1_LOGN, primes)
    want = X.samples(seeds, primes, n)
    total = sum(sum(rej) for _, rej in want)
    sentinel = np.uint64(0xA5A5A5A5DEADBEEF)
    for count_rejected in (True, False):
        d = moai.DeviceBuffer.from_numpy(np.full((count, 2, L, n), sentinel, dtype=np.uint64))
        none, rejected, overflow = ctx.seal_sample_uniform(seeds, L, out=d.ptr + 8 * L * n, stride_words=2 * L * n,
                                                           count_rejected=count_rejected)
        got = d.to_numpy((count, 2, L, n))
        assert none is None
        assert (got[:, 0] == sentinel).all()
        for b in range(count):
            assert np.array_equal(got[b, 1], want[b][0]), b
        if count_rejected:
            print("count %d: rejected %d (restatement %d)" % (count, rejected, total))
            assert rejected == total and overflow is False
        else:
            assert rejected is None and overflow is None
        assert ctx.check_residues(moai.DeviceBuffer.from_numpy(np.ascontiguousarray(got[:, 1])), count, L) is False


def test_limit_chain_rows(moai):
    logn, primes, seeds = X.l1()
    _check(moai, logn, primes, seeds)  # check_residues in it: every residue is below its row's prime


def test_prng_bytes_wavefront_edges(moai):
    ctx = moai.Context(10, O.coeff_modulus_create(1 << 10, [51, 46, 58]))
    seed = X.seed("PRNG", 0)
    for first, n_blocks in X.PRNG_RANGES:
        got = ctx.seal_prng_bytes(seed, first, n_blocks)
        assert len(got) == 4096 * n_blocks
        assert got == SF.prng_buffers(seed, first, n_blocks), (first, n_blocks)


def test_check_residues_positions(moai):
    logn, n = 10, 1 << 10
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    polys = O.uniform_rns(np.random.default_rng(31), primes, (3,), n)
    assert ctx.check_residues(moai.DeviceBuffer.from_numpy(polys), 3, 3) is False
    top = np.empty_like(polys)
    top[:] = np.array([q - 1 for q in primes], dtype=np.uint64)[None, :, None]
    assert ctx.check_residues(moai.DeviceBuffer.from_numpy(top), 3, 3) is False
    for p, r, i in X.check_plants(n, 3, 3):
        bad = polys.copy()
        bad[p, r, i] = primes[r]
        assert ctx.check_residues(moai.DeviceBuffer.from_numpy(bad), 3, 3) is True, (p, r, i)
