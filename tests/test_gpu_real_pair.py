"""Multiplication by the monomial X^(N/2) (the slot-wise constant i) in NTT form: moai_mul_i_add and moai_real_split.

CPU: the header declares and cites both entry points, the library exports them, hip.py types them, and the +-I_q pattern the
kernels rely on is what the oracle's transform of the monomial looks like.
GPU (-m gpu): bit-exact against the oracle's add / multiply_plain with the TRANSFORM of the monomial as the plaintext (the
expected values never use the +- pattern), and the operation census names both calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BITS = [20, 46, 51, 58, 61]  # one row under each prime size of the issue's list


def _declaration_with_comment(hdr, name):
    at = hdr.index("int %s(" % name)
    start = hdr.rfind("/*", 0, at)
    # the comment must belong to this declaration: no other declaration in between
    assert ";" not in hdr[hdr.index("*/", start):at], name
    return hdr[start:at]


def test_header_declares_and_cites_both_entry_points(moai):
    hdr = open(os.path.join(ROOT, "include", "moai_hip.h")).read()
    for name in ("moai_mul_i_add", "moai_real_split"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert "SEAL/" in _declaration_with_comment(hdr, name), name
    assert "polyarithsmallmod.h:634-655" in _declaration_with_comment(hdr, "moai_mul_i_add")
    L = C.CDLL(moai.lib_path())
    assert hasattr(L, "moai_mul_i_add") and hasattr(L, "moai_real_split")
    vp, sz = C.c_void_p, C.c_size_t
    assert moai.hip.SYMBOLS["moai_mul_i_add"] == (C.c_int, [vp, vp, vp, vp, sz, sz, C.c_int, vp])
    assert moai.hip.SYMBOLS["moai_real_split"] == (C.c_int, [vp, vp, vp, vp, vp, sz, sz, vp])
    assert callable(moai.Context.mul_i_add) and callable(moai.Context.real_split)
    lib = moai.hip.lib()
    assert lib.moai_mul_i_add.argtypes == moai.hip.SYMBOLS["moai_mul_i_add"][1]


def monomial_ntt(octx, primes, L, negative=False):
    """the oracle's forward transform of +-X^(N/2), [L][N]"""
    mono = np.zeros((L, octx.n), dtype=np.uint64)
    for r in range(L):
        mono[r, octx.n // 2] = primes[r] - 1 if negative else 1
    return octx.ntt(mono, L)


@pytest.mark.parametrize("logn,bits", [(2, [30]), (5, [46, 20]), (9, [61]), (11, [51, 46, 58]), (13, [60, 51, 46]), (16, BITS)])
def test_monomial_transform_is_plus_minus_root_power(logn, bits):
    """In the transform's output order X^(N/2) is +I_q on [0, N/2) and -I_q on [N/2, N), I_q = psi^(N/2), I_q^2 = -1."""
    n = 1 << logn
    primes = O.coeff_modulus_create(n, bits)
    octx = O.Context(logn, primes)
    M = monomial_ntt(octx, primes, len(primes))
    for r, q in enumerate(primes):
        iq = pow(int(O.Tables(logn, q).t.root), n // 2, q)
        assert iq * iq % q == q - 1
        assert (M[r, : n // 2] == np.uint64(iq)).all()
        assert (M[r, n // 2:] == np.uint64(q - iq)).all()


def up(m, a):
    return m.DeviceBuffer.from_numpy(a)


def input_sets(rng, primes, n_poly, n):
    """(name, a, b): uniform residues, then whole arrays of the edge rows 0 and q - 1"""
    L = len(primes)
    zero = np.zeros((n_poly, L, n), dtype=np.uint64)
    top = np.empty((n_poly, L, n), dtype=np.uint64)
    for r, q in enumerate(primes):
        top[:, r, :] = q - 1
    yield "uniform", O.uniform_rns(rng, primes, (n_poly,), n), O.uniform_rns(rng, primes, (n_poly,), n)
    yield "q-1, q-1", top, top
    yield "0, q-1", zero, top
    yield "q-1, 0", top, zero
    yield "0, 0", zero, zero


@pytest.mark.gpu
@pytest.mark.parametrize("n_poly", [1, 2, 96])
@pytest.mark.parametrize("logn", [11, 12, 13, 14, 15, 16])
def test_mul_i_add_and_real_split_match_oracle(moai, logn, n_poly):
    n = 1 << logn
    primes = O.coeff_modulus_create(n, BITS)
    assert [p.bit_length() for p in primes] == BITS
    L = len(primes)
    octx, ctx = O.Context(logn, primes), moai.Context(logn, primes)
    plus, minus = monomial_ntt(octx, primes, L), monomial_ntt(octx, primes, L, negative=True)
    rng = np.random.default_rng(1000 * logn + n_poly)
    shape = (n_poly, L, n)
    for name, a, b in input_sets(rng, primes, n_poly, n):
        da, db = up(moai, a), up(moai, b)
        out = moai.DeviceBuffer(a.size)
        for sign, mono in ((1, plus), (-1, minus)):
            prod = octx.multiply_plain(b, n_poly, L, mono)
            expect = octx.add(a, prod, n_poly, L)
            # separate output
            ctx.mul_i_add(da, db, out, n_poly, L, sign)
            assert (out.to_numpy(shape) == expect).all(), (name, sign, "out")
            # a == NULL: the plain monomial product
            ctx.mul_i_add(None, db, out, n_poly, L, sign)
            assert (out.to_numpy(shape) == prod.reshape(shape)).all(), (name, sign, "a = NULL")
            # out aliases a, out aliases b, product in place
            t = up(moai, a)
            ctx.mul_i_add(t, db, t, n_poly, L, sign)
            assert (t.to_numpy(shape) == expect).all(), (name, sign, "out = a")
            t.upload(b)
            ctx.mul_i_add(da, t, t, n_poly, L, sign)
            assert (t.to_numpy(shape) == expect).all(), (name, sign, "out = b")
            t.upload(b)
            ctx.mul_i_add(None, t, t, n_poly, L, sign)
            assert (t.to_numpy(shape) == prod.reshape(shape)).all(), (name, sign, "in place")
            t.free()
        # real_split: out_re = r + rbar, out_im = -X^(N/2) (r - rbar)
        exp_re = octx.add(a, b, n_poly, L)
        exp_im = octx.multiply_plain(octx.sub(a, b, n_poly, L), n_poly, L, minus)
        out2 = moai.DeviceBuffer(a.size)
        ctx.real_split(da, db, out, out2, n_poly, L)
        assert (out.to_numpy(shape) == exp_re).all(), (name, "re")
        assert (out2.to_numpy(shape) == exp_im.reshape(shape)).all(), (name, "im")
        assert (da.to_numpy(shape) == a).all() and (db.to_numpy(shape) == b).all()  # inputs untouched
        ctx.real_split(da, db, da, db, n_poly, L)  # out_re = r, out_im = rbar
        assert (da.to_numpy(shape) == exp_re).all(), (name, "re aliased")
        assert (db.to_numpy(shape) == exp_im.reshape(shape)).all(), (name, "im aliased")
        for buf in (da, db, out, out2):
            buf.free()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [11, 16])
def test_mul_i_twice_is_negate(moai, logn):
    n, n_poly = 1 << logn, 3
    primes = O.coeff_modulus_create(n, BITS)
    L = len(primes)
    octx, ctx = O.Context(logn, primes), moai.Context(logn, primes)
    x = O.uniform_rns(np.random.default_rng(logn), primes, (n_poly,), n)
    x[0, :, :7] = 0
    d = up(moai, x)
    ctx.mul_i_add(None, d, d, n_poly, L, 1)
    ctx.mul_i_add(None, d, d, n_poly, L, 1)
    assert (d.to_numpy(x.shape) == octx.negate(x, n_poly, L)).all()
    # ... and +i followed by -i is the identity
    ctx.mul_i_add(None, d, d, n_poly, L, 1)
    ctx.mul_i_add(None, d, d, n_poly, L, -1)
    assert (d.to_numpy(x.shape) == octx.negate(x, n_poly, L)).all()


@pytest.mark.gpu
def test_arguments_are_validated(moai):
    logn = 11
    primes = O.coeff_modulus_create(1 << logn, [46, 51])
    ctx = moai.Context(logn, primes)
    d = moai.DeviceBuffer(2 * (1 << logn))
    e = moai.DeviceBuffer(2 * (1 << logn))
    with pytest.raises(moai.hip.MoaiError):
        ctx.mul_i_add(d, e, d, 1, 2, 0)  # sign
    with pytest.raises(moai.hip.MoaiError):
        ctx.mul_i_add(d, None, d, 1, 2, 1)
    with pytest.raises(moai.hip.MoaiError):
        ctx.mul_i_add(d, e, d, 1, 3, 1)  # more rows than primes
    with pytest.raises(moai.hip.MoaiError):
        ctx.real_split(d, e, d, d, 1, 2)  # the two outputs overlap
    with pytest.raises(moai.hip.MoaiError):
        ctx.real_split(d, e, e, d, 1, 2)  # crossed aliasing


@pytest.mark.gpu
def test_census_names_both_calls(moai):
    logn = 12
    primes = O.coeff_modulus_create(1 << logn, [51, 46, 46, 58])
    ctx = moai.Context(logn, primes)
    words = 6 * 3 * (1 << logn)
    a, b, c, d = (moai.DeviceBuffer(words) for _ in range(4))
    for buf in (a, b):
        buf.upload(np.zeros(words, dtype=np.uint64))
    moai.hip.op_trace(True)
    try:
        ctx.mul_i_add(a, b, c, 6, 3, 1)
        ctx.mul_i_add(None, b, c, 4, 2, -1)
        ctx.real_split(a, b, c, d, 6, 3)
        ctx.real_split(a, b, c, d, 2, 3)
    finally:
        moai.hip.op_trace(False)
    counts = moai.hip.op_trace_counts()
    assert counts[("mul_i_add", 3)] == 6 and counts[("mul_i_add", 2)] == 4
    assert counts[("real_split", 3)] == 8
