"""The fused hybrid mod-down (MOAI_HYBRID_FUSED_DOWN = 1; csrc/hybrid_kernels.hip.h hy_down_scale_kernel, hy_down_strided, hy_down_contig,
hy_rescale_contig): step 5's base conversion on the strided pass's loads and its division on the contiguous pass's stores, bit for bit
the unfused stages in both rounding modes.

1. moai_switch_key_hybrid against the restatements (tests/hybrid_ref.py, tests/hybrid_exact_ref.py): one strided tile per row and two,
   three / three / one sources' worth of targets, FP64 and integer instantiations (MOAI_MD_FP_MIN_ROWS = 1), MOAI_HYBRID_FUSED 0 and 1.
2. the limit primes of every arithmetic mode and sixteen 61-bit sources (seventeen products in exact mode); the directed boundaries of X'.
3. every family that ends in a mod-down: knob 1 = knob 0, which the existing files pin to the restatements.
4. N = 2^16 at MOAI's parameters once.    5. the knob is a switch: off by default, without effect below N = 2^12.

Every comparison asserts hybrid_fused_down_launches(...) > 0 inside its tuned block, so none passes on the unfused stages."""
import contextlib

import numpy as np
import pytest

import hybrid_exact_ref as HX
import hybrid_ref as HR
import mode_limits as ML
import oracle as O
from hybrid_cases import BsgsCase, DotCase, check_boundaries, exact, run_rescale, run_switch
from hybrid_kit import ENVS, MOAI_DATA_BITS, PATTERN, Env, tuned
from test_gpu_hybrid_fused import FORMS, RESCALE_FORMS, run_form

pytestmark = pytest.mark.gpu

_envs, _cases = {}, {}
RESTATED = {0: HR.switch_key, 1: HX.switch_key}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for e in _envs.values():
        e.close()
    _envs.clear()
    _cases.clear()


def env(key, make):
    if key not in _envs:
        _envs[key] = make()
    return _envs[key]


def tiled3(moai, logn=12):
    _, data, special = ENVS["tiled3"]
    return env(("tiled3", logn), lambda: Env(moai, logn, data, special))


def rounding(e, mode):
    """the block's rounding mode: hybrid_cases.exact, or the default"""
    return exact(e) if mode else contextlib.nullcontext()


def restated(e, L, mode):
    """four switches of one shape -- two random targets, one with every row m - 1, one zero -- and their restatement in `mode`"""
    if ("in", L) not in e.cache:
        rng = np.random.default_rng(e.logn * 100 + L)
        key = e.random_key(rng)
        ct = O.uniform_rns(rng, e.primes[:L], (4, 2), e.n)
        target = O.uniform_rns(rng, e.primes[:L], (4,), e.n)
        target[2], target[3] = e.edge_targets(L)
        e.cache[("in", L)] = (key, e.up(key), ct, target)
    key, dkey, ct, target = e.cache[("in", L)]
    if ("want", L, mode) not in e.cache:
        e.cache[("want", L, mode)] = np.stack([RESTATED[mode](e.octx, ct[b], target[b], key, L, e.alpha) for b in range(4)])
    return dkey, ct, target, e.cache[("want", L, mode)]


# ---- 1. the switch against the restatements ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fp", [1, 0])
@pytest.mark.parametrize("L", [7, 4, 1])
@pytest.mark.parametrize("logn", [12, 13])
def test_switch_against_the_restatement(moai, logn, L, fp, mode, fused):
    e = tiled3(moai, logn)
    dkey, ct, target, want = restated(e, L, mode)
    with tuned(moai, MOAI_HYBRID_FUSED_DOWN=1, MOAI_HYBRID_FUSED=fused, MOAI_NTT_FP=fp, MOAI_MD_FP_MIN_ROWS=1), rounding(e, mode):
        assert e.ctx.hybrid_fused_down_launches(L, e.alpha, 8) > 0
        got = run_switch(e, ct, target, dkey, L)
    assert (got == want).all()


# ---- 2. limit primes, wide digits, directed boundaries -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which,alpha,L", [(w, None, 7) for w in ML.HYBRID_CHAINS] + [("wide", 16, 17)])
def test_switch_at_the_limit_primes(moai, which, alpha, L, mode):
    """key rows all m - 1, target = NTT of worst_coeff: the accumulators the mod-down divides are what the largest sums leave; at
    ("wide", 16) sixteen 61-bit sources, with the overflow row seventeen products in exact mode"""
    primes, _, alpha = ML.hybrid_chain(12, which, alpha)
    e = env((which, alpha), lambda: Env(moai, 12, primes=primes, alpha=alpha))
    key = np.empty((e.digits, 2, e.k, e.n), dtype=np.uint64)
    for i, m in enumerate(e.primes):
        key[:, :, i, :] = m - 1
    target = e.octx.ntt(ML.worst_coeff(e.primes, L, alpha, e.n), L)
    ct = O.uniform_rns(np.random.default_rng(L), e.primes[:L], (1, 2), e.n)
    dkey = e.up(key)
    with tuned(moai, MOAI_HYBRID_FUSED_DOWN=1), rounding(e, mode):
        assert e.ctx.hybrid_fused_down_launches(L, alpha, 2) > 0
        got = run_switch(e, ct, target[None], dkey, L)
    dkey.free()
    assert (got[0] == RESTATED[mode](e.octx, ct[0], target, key, L, alpha)).all()


@pytest.mark.parametrize("rescale", [False, True])
def test_boundaries_of_the_exact_mode(moai, rescale):
    """X' on 0, 1, 2, W-2, W-1, H-1, H, H+1 (hybrid_cases.boundary_case): the overflow row decides every one of them"""
    e = tiled3(moai)
    with tuned(moai, MOAI_HYBRID_FUSED_DOWN=1):
        assert e.ctx.hybrid_fused_down_launches(2 if rescale else 1, e.alpha, 2) > 0
        check_boundaries(e, rescale)


# ---- 3. every family: knob 1 = knob 0 --------------------------------------------------------------------------------------------------
def run_family(moai, e, form, L):
    """one call of `form`; the outputs as a list of arrays"""
    ctx, n, a = e.ctx, e.n, e.alpha
    rng = np.random.default_rng(41)
    if form in FORMS + RESCALE_FORMS:
        return run_form(moai, e, form, L, rng)
    if form in ("pt_dot", "bsgs"):  # pt_dot: outputs 0 and 1 have switched terms, output 2 only the identity term
        if form not in _cases:
            _cases[form] = DotCase(e, L, B=2, want=False) if form == "pt_dot" else BsgsCase(e, L, want=False)
        fb, got = _cases[form].run()
    else:
        keys = [e.up(e.random_key(rng)) for _ in range(3)]
        elts = e.elts([1, 3, 0])
        ct = e.random_input(rng, L, 2)
        if form == "hoisted":
            corrs = [ctx.hybrid_hoist_correction(k, elt, L, a) for k, elt in zip(keys, elts)]
            out = e.filled((3, 2, 2, L, n), PATTERN)
            fb = ctx.apply_galois_hybrid_hoisted(e.up(ct), out, L, a, elts, keys, corrs, 2)
            got = out.to_numpy((3, 2, 2, L, n))
        else:  # galois_ptrs_inplace: member 0's output block is its sum block, member 1's is its input block
            sums = O.uniform_rns(rng, e.primes[:L], (2, 2), n)
            blocks = [e.up(sums[0]), e.up(ct[1])]
            ctx.apply_galois_hybrid_ptrs([e.up(ct[0]), blocks[1]], blocks, L, a, elts[:2], keys[:2], [blocks[0], None])
            fb, got = False, np.stack([b.to_numpy((2, L, n)) for b in blocks])
        for k in keys:
            k.free()
    assert not fb
    return [got]


FAMILIES = FORMS + RESCALE_FORMS + ["hoisted", "pt_dot", "bsgs", "galois_ptrs_inplace"]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("form", FAMILIES)
def test_every_family_fused_down_equals_unfused(moai, form, mode):
    e, L = tiled3(moai), 7
    got = {}
    for knob in (0, 1):
        with tuned(moai, MOAI_HYBRID_FUSED_DOWN=knob), rounding(e, mode):
            assert (e.ctx.hybrid_fused_down_launches(L, e.alpha, 4) > 0) == bool(knob)
            got[knob] = run_family(moai, e, form, L)
    assert len(got[0]) == len(got[1])
    for a, b in zip(got[0], got[1]):
        assert (a == b).all()


# ---- 4. N = 2^16 once --------------------------------------------------------------------------------------------------------------------
def test_fused_down_equals_unfused_at_moais_parameters(moai):
    """MOAI's 35 data primes with 12 special primes, sixteen tiles a row: 12 sources to 35 and 15 targets in the switch, 13 to 34 and
    14 in the merged relinearize + rescale"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12, oracle=False)
    rng = np.random.default_rng(16)
    dkey = e.up(e.random_key(rng))
    for L in (35, 15):
        ct3 = O.uniform_rns(rng, e.primes[:L], (2, 3), e.n)
        got = {}
        for knob in (0, 1):
            with tuned(moai, MOAI_HYBRID_FUSED_DOWN=knob):
                assert (e.ctx.hybrid_fused_down_launches(L, e.alpha, 4) > 0) == bool(knob)
                got[knob] = (run_switch(e, ct3[:, :2], ct3[:, 2], dkey, L), run_rescale(e, ct3, dkey, L))
        for a, b in zip(got[0], got[1]):
            assert (a == b).all(), L
    dkey.free()
    e.close()


# ---- 5. the switch is a switch -------------------------------------------------------------------------------------------------------------
def test_the_knob_is_off_by_default_and_without_effect_below_4096(moai):
    e = tiled3(moai)
    small = env("small2", lambda: Env(moai, *ENVS["small2"]))
    assert e.ctx.hybrid_fused_down_launches(7, e.alpha, 8) == 0
    with tuned(moai, MOAI_HYBRID_FUSED_DOWN=1):
        assert e.ctx.hybrid_fused_down_launches(7, e.alpha, 8) > 0
        assert e.ctx.hybrid_fused_down_launches(7, e.alpha, 0) == 0
        assert small.ctx.hybrid_fused_down_launches(5, small.alpha, 8) == 0
        dkey, ct, target, want = restated(small, 5, 0)
        assert (run_switch(small, ct, target, dkey, 5) == want).all()
    assert e.ctx.hybrid_fused_down_launches(7, e.alpha, 8) == 0
    with pytest.raises(moai.MoaiError):
        e.ctx.hybrid_fused_down_launches(e.lmax + 1, e.alpha, 8)
