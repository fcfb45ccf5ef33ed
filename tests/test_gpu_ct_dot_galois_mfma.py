"""The Gram form of moai_ct_dot_galois (csrc/ctdot_galois_mfma.hip.h, MOAI_CTDOT_GALOIS_MFMA): the four sums against Python integers
on the oracle's permutation table, the form of every output asserted by moai_ct_dot_galois_forms before the call (the integer forms
give the same bits).  Seams: one block of 128 coefficients and sixteen strips (N = 128, where every element is served, 2N - 1 too),
two blocks with every entry of G written once (N = 256, the 128 elements = 1 mod 4), 32 blocks beside the staged and gather forms
in one call (N = 4096); 1, 8, 9 terms (a K-step) and 17 (an LDS stage of 16); 13 and 15 diagonals (a prime below 2^51, one below
2^61); CDGM_MAX_TERMS terms of the largest byte limbs, where a diagonal's int32 sum is at its bound, and one term more, which
stays on the integer forms."""
import numpy as np
import pytest

import hybrid_kit as HK
import mode_limits as ML
import oracle as O
from test_gpu_ct_dot_galois import MAX_TERMS, ROWS, SENTINEL, _ctxs, exact, release_device_contexts, run  # noqa: F401 (the fixture closes _ctxs)

KNOB, LIMIT, STAGE, L = "MOAI_CTDOT_GALOIS_MFMA", 16383, 16, len(ROWS)  # CDGM_MAX_TERMS, CDGM_STAGE


@pytest.fixture(autouse=True)
def reset_tuning(moai):
    yield
    moai.hip.reset_tuning()


def context(moai, logn):
    return HK.cached(_ctxs, logn, lambda: moai.Context(logn, [ML.chain(logn)[name] for name in ROWS]))


def outputs(logn):
    """the elements of a call and its [gather, staged, Gram] counts with the knob at 1 and at 0"""
    m = 2 << logn
    if logn == 7:
        return [1, 3, 5, m - 1, 5], [0, 0, 5], [5, 0, 0]
    if logn == 8:
        return list(range(1, m, 4)), [0, 0, 128], [0, 128, 0]
    # N = 4096: 5^16 keeps blocks of 128 coefficients, 5^32 of 64, 5^8 of 256 (staged); 5 and 2N - 1 gather
    pool = (1, pow(5, 16, m), pow(5, 32, m), pow(5, 8, m), 5, m - 1)
    return [pool[i % 6] for i in range(14)], [4, 2, 8], [4, 10, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("logn,terms", [(7, 1), (7, 8), (7, 9), (7, STAGE + 1), (8, 9), (12, 3), (12, 2 * STAGE + 1)])
def test_gram_form_matches_exact_integers(moai, logn, terms):
    elts, counts, counts_off = outputs(logn)
    ctx = context(moai, logn)
    assert ctx.ct_dot_galois_forms(elts, terms, L) == counts_off
    moai.hip.set_tuning(KNOB, 1)
    assert ctx.ct_dot_galois_forms(elts, terms, L) == counts
    rng = np.random.default_rng(100 * terms + logn)
    primes = [ML.chain(logn)[name] for name in ROWS]
    x, w = (O.uniform_rns(rng, primes, (terms, 2), 1 << logn) for _ in range(2))
    got = run(moai, logn, x, w, elts)
    bad = np.argwhere(got != exact(x, w, elts, primes, logn))
    assert not len(bad), ("first of %d at [output, component, prime, coeff]" % len(bad), bad[0].tolist())


def largest_limbs(q):
    """the canonical value below q whose signed byte limbs are -128 in every place but the top one, which is as large as q allows"""
    top = 256 ** (6 if q <= 1 << 54 else 7)  # MM_DIGITS7_MAX: seven limbs, else eight
    low = 128 * ((top - 1) // 255)
    return min(127, (q - 1 + low) // top) * top - low


@pytest.mark.gpu
@pytest.mark.parametrize("terms,value", [(LIMIT, "q - 1"), (LIMIT, "largest limbs"), (LIMIT + 1, "q - 1")])
def test_accumulator_at_its_bound_and_one_term_past_it(moai, terms, value):
    moai.hip.set_tuning(KNOB, 1)
    primes = [ML.chain(7)[name] for name in ROWS]
    assert context(moai, 7).ct_dot_galois_forms([3], terms, L) == ([0, 0, 1] if terms <= LIMIT else [1, 0, 0])
    v = [q - 1 if value == "q - 1" else largest_limbs(q) for q in primes]
    assert all(0 < a < q for a, q in zip(v, primes))
    x = np.ascontiguousarray(np.broadcast_to(np.array(v, dtype=np.uint64)[:, None], (terms, 2, L, 128)))
    got = run(moai, 7, x, x, [3])
    want = np.array([terms * a * a % q for a, q in zip(v, primes)], dtype=np.uint64)
    assert (got == want[None, None, :, None]).all()


@pytest.mark.gpu
def test_knob_is_the_least_number_of_eligible_outputs(moai):
    ctx, eligible = context(moai, 8), list(range(1, 512, 4))
    moai.hip.set_tuning(KNOB, 64)
    assert ctx.ct_dot_galois_forms(eligible[:63] + [3], 9, L) == [0, 64, 0]  # 3 keeps blocks of 256: staged in either case
    assert ctx.ct_dot_galois_forms(eligible[:64] + [3], 9, L) == [0, 1, 64]
    assert ctx.ct_dot_galois_forms([], 9, L) == [0, 0, 0]


@pytest.mark.gpu
def test_refusals_enqueue_nothing_in_any_form(moai):
    logn, m = 12, 2 << 12
    moai.hip.set_tuning(KNOB, 1)
    ctx, gram = context(moai, logn), pow(5, 16, m)
    x = np.zeros((3, 2, L, 1 << logn), dtype=np.uint64)
    dout = moai.DeviceBuffer.from_numpy(np.full(4 * 4 * x[0, 0].size, SENTINEL, dtype=np.uint64))
    # valid elements of every form before the refused one: a launch of theirs would show in the output
    for elts, terms in (([gram, 4], 3), ([gram, pow(5, 8, m), 5, m + 1], 3), ([gram, 1], 0), ([gram, 1], MAX_TERMS + 1)):
        for call in (lambda: run(moai, logn, x, x, elts, terms, dout), lambda: ctx.ct_dot_galois_forms(elts, terms, L)):
            with pytest.raises(moai.hip.MoaiError) as err:
                call()
            assert err.value.code == moai.hip.MOAI_EINVAL, (elts, terms)
        assert (dout.to_numpy((dout.n_words,)) == SENTINEL).all(), (elts, terms)
    with pytest.raises(moai.hip.MoaiError):
        ctx.ct_dot_galois(None, moai.DeviceBuffer.from_numpy(x), dout, [gram, 1], 3, L)
    assert (dout.to_numpy((dout.n_words,)) == SENTINEL).all()
    assert moai.hip.lib().moai_ct_dot_galois_forms(ctx.h, None, 2, 3, L, None) == moai.hip.MOAI_EINVAL


def test_knob_and_query_are_declared_exported_and_bound(moai):
    moai.hip.set_tuning(KNOB, 1)
    HK.exported(moai, ["moai_ct_dot_galois_forms"], ["ct_dot_galois_forms"])
    assert "galois.cpp:18-51" in HK.header()[HK.header().index("How many outputs that call would send NOW"):][:900]
