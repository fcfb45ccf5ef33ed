"""csrc/elementwise.hip at the limit primes of tests/mode_limits.py and at the degrees where its kernels change shape, bit for bit
against the CPU oracle or exact integers.

1. the per-coefficient kernels (ew_kernel, scalar_rows_kernel, ct_mul_kernel, ct_mul_general_kernel, drop_rows_kernel,
   galois_gather_kernel) under all nine limit primes, on operand pairs from {0, 1, q-1, q/2, q/2+1}^2 (ML.pair_patterns), at
   N = 4096 and at N = 256, where a row is 128 sixteen-byte chunks and half of every workgroup idles;
2. mul_i_add_kernel / real_split_kernel on both arms of their sign decision: per lane for N/4 < 256 (logn 2 .. 9), per workgroup
   segment from logn 10 on;
3. every entry point of the file once at N = 2, 4, 8 and 256;
4. ct_pt_matmul_fp_kernel where its bounds bind: primes on either side of 2^52 / 25 (fold every 16 rows / every row), row counts
   around the fold period, and products whose residues all sit at +-q/2 with the quotient estimate at a half-integer
   (ML.matmul_worst); a prime at 2^51 moves the whole level to the integer kernel.

The lazy 128-bit dot sums have their worst-case tests in tests/test_gpu_parity.py (worst61); here they only appear in the degree
sweep."""
import numpy as np
import pytest

import mode_limits as ML
import oracle as O

pytestmark = pytest.mark.gpu

_ctxs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    """the device contexts are built once per (degree, chain) and live as long as this module's tests"""
    yield
    for _, ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


def contexts(moai, logn, primes):
    key = (logn, tuple(primes))
    if key not in _ctxs:
        _ctxs[key] = (O.Context(logn, primes), moai.Context(logn, primes))
    return _ctxs[key]


def up(moai, a):
    return moai.DeviceBuffer.from_numpy(a)


def qcol(primes):
    return np.array(primes, dtype=np.uint64)[:, None]


# ---- 1. the per-coefficient kernels at the limit primes ---------------------------------------------------------------------
@pytest.fixture(scope="module", params=[12, 8])
def env9(request, moai):
    logn = request.param
    n = 1 << logn
    primes = ML.ordered(logn, "g61_last")
    octx, ctx = contexts(moai, logn, primes)
    a, b = ML.pair_rows(primes, 3, n, np.random.default_rng(7100 + logn))
    for v in (a, b):
        v.setflags(write=False)
    return logn, n, primes, octx, ctx, a, b


def test_add_sub_negate_dyadic_at_the_limits(moai, env9):
    logn, n, primes, octx, ctx, a, b = env9
    L, npoly = len(primes), 3
    da, db = up(moai, a), up(moai, b)
    do = moai.DeviceBuffer(a.size)
    want = dict(add=octx.add(a, b, npoly, L), sub=octx.sub(a, b, npoly, L), negate=octx.negate(a, npoly, L))
    ctx.add(da, db, do, npoly, L)
    assert (do.to_numpy(a.shape) == want["add"]).all()
    ctx.sub(da, db, do, npoly, L)
    assert (do.to_numpy(a.shape) == want["sub"]).all()
    ctx.sub(db, da, do, npoly, L)
    assert (do.to_numpy(a.shape) == octx.sub(b, a, npoly, L)).all()
    ctx.negate(da, do, npoly, L)
    assert (do.to_numpy(a.shape) == want["negate"]).all()
    # in place, into the first and into the second operand
    for op in ("add", "sub"):
        t = up(moai, a)
        getattr(ctx, op)(t, db, t, npoly, L)
        assert (t.to_numpy(a.shape) == want[op]).all(), op + " into a"
        t.upload(b)
        getattr(ctx, op)(da, t, t, npoly, L)
        assert (t.to_numpy(a.shape) == want[op]).all(), op + " into b"
        t.free()
    t = up(moai, a)
    ctx.negate(t, t, npoly, L)
    assert (t.to_numpy(a.shape) == want["negate"]).all()
    # the dyadic product, polynomial by polynomial and with one broadcast plaintext
    ctx.dyadic_mul(da, db, do, npoly, npoly, L)
    exp = np.stack([octx.multiply_plain(a[p], 1, L, b[p]).reshape(L, n) for p in range(npoly)])
    assert (do.to_numpy(a.shape) == exp).all()
    ctx.dyadic_mul(da, db, do, npoly, 1, L)
    assert (do.to_numpy(a.shape) == octx.multiply_plain(a, npoly, L, b[0])).all()
    ctx.dyadic_mul(da, db, da, npoly, npoly, L)
    assert (da.to_numpy(a.shape) == exp).all(), "in place"


def test_scalar_rows_at_the_limits(moai, env9):
    """scalars 0, 1, q-1, 2^64-1 (reduced first, polyarithsmallmod.h:209-217) and random ones against every value of the rows:
    multiply_plain / add with the constant-row plaintext"""
    logn, n, primes, octx, ctx, a, b = env9
    L, npoly = len(primes), 3
    rng = np.random.default_rng(7200 + logn)
    da, do = up(moai, a), moai.DeviceBuffer(a.size)
    kinds = {"0": [0] * L, "1": [1] * L, "q-1": [q - 1 for q in primes], "2^64-1": [(1 << 64) - 1] * L,
             "random": [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(L)],
             "q/2+1": [q // 2 + 1 for q in primes]}
    for name, scal in kinds.items():
        pt = np.stack([np.full(n, scal[i] % primes[i], dtype=np.uint64) for i in range(L)])
        ctx.mul_scalar_rows(da, scal, do, npoly, L)
        assert (do.to_numpy(a.shape) == octx.multiply_plain(a, npoly, L, pt)).all(), "mul, scalar " + name
        ctx.add_scalar_rows(da, scal, do, npoly, L)
        ptb = np.ascontiguousarray(np.broadcast_to(pt, a.shape))
        assert (do.to_numpy(a.shape) == octx.add(a, ptb, npoly, L)).all(), "add, scalar " + name
    assert (da.to_numpy(a.shape) == a).all()


def test_ct_products_at_the_limits(moai, env9):
    logn, n, primes, octx, ctx, a, b = env9
    L, B = len(primes), 2
    # two ciphertexts of two polynomials each, from the three pattern polynomials
    x = np.stack([a[:2], np.stack([b[1], a[2]])])
    y = np.stack([b[:2], np.stack([a[1], b[2]])])
    dx, dy = up(moai, x), up(moai, y)
    do = moai.DeviceBuffer(B * 3 * L * n)
    ctx.ct_multiply(dx, dy, do, L, B)
    got = do.to_numpy((B, 3, L, n))
    for i in range(B):
        assert (got[i] == octx.multiply(x[i], y[i], L)).all(), ("multiply", i)
    ctx.ct_square(dx, do, L, B)
    got = do.to_numpy((B, 3, L, n))
    for i in range(B):
        assert (got[i] == octx.square(x[i], L)).all(), ("square", i)
    for sx, sy in ((3, 2), (2, 3)):
        u = np.stack([a[:sx], b[:sx]])
        v = np.stack([b[:sy], a[:sy]])
        dg = moai.DeviceBuffer(B * 4 * L * n)
        ctx.ct_multiply_general(up(moai, u), sx, up(moai, v), sy, dg, L, B)
        got = dg.to_numpy((B, 4, L, n))
        for i in range(B):
            assert (got[i] == octx.multiply_general(u[i], sx, v[i], sy, L)).all(), (sx, sy, i)


def test_mod_drop_and_galois_permute_at_the_limits(moai, env9):
    logn, n, primes, octx, ctx, a, b = env9
    L, B, size = len(primes), 2, 2
    x = np.stack([a[:2], b[:2]])
    dx = up(moai, x)
    for drop in (1, L - 1):
        do = up(moai, np.full(B * size * (L - drop) * n + 2, 7, dtype=np.uint64))
        ctx.mod_drop(dx, do, size, L, drop, B)
        got = do.to_numpy()
        for i in range(B):
            assert (got[:-2].reshape(B, size, L - drop, n)[i] == octx.mod_drop(x[i], size, L, drop)).all(), (drop, i)
        assert (got[-2:] == 7).all(), "wrote past the kept rows"
        do.free()
    do = moai.DeviceBuffer(a.size)
    da = up(moai, a)
    for step in (1, 0):
        elt = ctx.galois_elt_from_step(step)
        assert elt == O.galois_elt_from_step(logn, step) and (step or elt == 2 * n - 1)
        ctx.galois_permute(da, do, 3, L, elt)
        tab = O.galois_table_ntt(logn, elt)
        assert sorted(tab.tolist()) == list(range(n))
        assert (do.to_numpy(a.shape) == a[:, :, tab]).all(), step


# ---- 2. multiplication by X^(N/2): both arms of the sign decision ---------------------------------------------------------
MONO_NAMES = ("g61", "fpr_hi", "small")


def monomial_ntt(octx, primes, negative=False):
    """the oracle's forward transform of +-X^(N/2), [L][N] (tests/test_gpu_real_pair.py)"""
    mono = np.zeros((len(primes), octx.n), dtype=np.uint64)
    for r, q in enumerate(primes):
        mono[r, octx.n // 2] = q - 1 if negative else 1
    return octx.ntt(mono, len(primes))


@pytest.mark.parametrize("n_poly", [1, 3])
@pytest.mark.parametrize("logn", [2, 3, 8, 9, 10, 12])
def test_mul_i_add_and_real_split_on_both_arms(moai, logn, n_poly):
    """N/4 < 256 (logn <= 9): a workgroup's segment spans both halves of the row and every lane decides its sign; logn 10 is the
    first degree at which a segment lies in one half.  Expected from the oracle's multiply_plain by the transform of the monomial."""
    n = 1 << logn
    c = ML.chain(logn)
    primes = [c[name] for name in MONO_NAMES]
    L = len(primes)
    octx, ctx = contexts(moai, logn, primes)
    by_segment = n // 4 >= 256
    assert by_segment == (logn >= 10)
    plus, minus = monomial_ntt(octx, primes), monomial_ntt(octx, primes, negative=True)
    a, b = ML.pair_rows(primes, n_poly, n, np.random.default_rng(7300 + 10 * logn + n_poly))
    shape = a.shape
    da, db = up(moai, a), up(moai, b)
    out, out2 = moai.DeviceBuffer(a.size), moai.DeviceBuffer(a.size)
    for sign, mono in ((1, plus), (-1, minus)):
        prod = octx.multiply_plain(b, n_poly, L, mono).reshape(shape)
        expect = octx.add(a, prod, n_poly, L)
        ctx.mul_i_add(da, db, out, n_poly, L, sign)
        assert (out.to_numpy(shape) == expect).all(), (sign, "with the addend")
        ctx.mul_i_add(None, db, out, n_poly, L, sign)
        assert (out.to_numpy(shape) == prod).all(), (sign, "without")
        t = up(moai, b)
        ctx.mul_i_add(da, t, t, n_poly, L, sign)
        assert (t.to_numpy(shape) == expect).all(), (sign, "out = b")
        t.free()
    exp_re = octx.add(a, b, n_poly, L)
    exp_im = octx.multiply_plain(octx.sub(a, b, n_poly, L), n_poly, L, minus).reshape(shape)
    ctx.real_split(da, db, out, out2, n_poly, L)
    assert (out.to_numpy(shape) == exp_re).all(), "re"
    assert (out2.to_numpy(shape) == exp_im).all(), "im"
    assert (da.to_numpy(shape) == a).all() and (db.to_numpy(shape) == b).all()
    ctx.real_split(da, db, da, db, n_poly, L)  # out_re = r, out_im = rbar: the documented aliasing
    assert (da.to_numpy(shape) == exp_re).all(), "re aliased"
    assert (db.to_numpy(shape) == exp_im).all(), "im aliased"
    # twice is negate; +i then -i is the identity
    d = up(moai, a)
    ctx.mul_i_add(None, d, d, n_poly, L, 1)
    ctx.mul_i_add(None, d, d, n_poly, L, 1)
    assert (d.to_numpy(shape) == octx.negate(a, n_poly, L)).all(), "twice is negate"
    ctx.mul_i_add(None, d, d, n_poly, L, 1)
    ctx.mul_i_add(None, d, d, n_poly, L, -1)
    assert (d.to_numpy(shape) == octx.negate(a, n_poly, L)).all(), "+i then -i"


def test_mul_i_needs_four_coefficients(moai):
    """N = 2: X^(N/2) = X has no two halves of whole chunks; both calls refuse (MOAI_EINVAL) and write nothing"""
    logn = 1
    c = ML.chain(logn)
    primes = [c[name] for name in MONO_NAMES]
    _, ctx = contexts(moai, logn, primes)
    fill = np.full((1, 3, 2), 7, dtype=np.uint64)
    x = O.uniform_rns(np.random.default_rng(1), primes, (1,), 2)
    da, db, out, out2 = up(moai, x), up(moai, x), up(moai, fill), up(moai, fill)
    for call in (lambda: ctx.mul_i_add(da, db, out, 1, 3, 1), lambda: ctx.mul_i_add(None, db, out, 1, 3, -1),
                 lambda: ctx.real_split(da, db, out, out2, 1, 3)):
        with pytest.raises(moai.hip.MoaiError) as err:
            call()
        assert err.value.code == moai.hip.MOAI_EINVAL
    assert (out.to_numpy(fill.shape) == fill).all() and (out2.to_numpy(fill.shape) == fill).all()


# ---- 3. every entry point at the smallest degrees ----------------------------------------------------------------------------
def sweep_data(rng, primes, lead, n):
    """uniform residues with polynomial 0's first row all q-1 and its second row all 0"""
    x = O.uniform_rns(rng, primes, lead, n)
    first = (0,) * len(lead)
    x[first + (0,)] = primes[0] - 1
    x[first + (1,)] = 0
    return x


def chain_sum(octx, terms, size, L):
    """the oracle's add_inplace chain over a list of [size][L][N] products"""
    acc = terms[0]
    for t in terms[1:]:
        acc = octx.add(acc, t, size, L)
    return np.asarray(acc)


@pytest.mark.parametrize("logn", [1, 2, 3, 8])
def test_every_entry_point_at_the_smallest_degrees(moai, logn):
    """N = 2 is one 16-byte chunk per row, N = 4 two, N = 8 four, N = 256 half a workgroup: one call of every entry point of
    csrc/elementwise.hip with the smallest shapes that take each of its kernels, against the oracle's call chains"""
    n = 1 << logn
    c = ML.chain(logn)
    primes = [c[name] for name in MONO_NAMES]
    L = len(primes)
    octx, ctx = contexts(moai, logn, primes)
    rng = np.random.default_rng(7400 + logn)
    a, b = sweep_data(rng, primes, (3,), n), sweep_data(rng, primes, (3,), n)
    da, db = up(moai, a), up(moai, b)
    do = moai.DeviceBuffer(a.size)

    # add / sub / negate / dyadic product / scalar rows
    ctx.add(da, db, do, 3, L)
    assert (do.to_numpy(a.shape) == octx.add(a, b, 3, L)).all()
    ctx.sub(da, db, do, 3, L)
    assert (do.to_numpy(a.shape) == octx.sub(a, b, 3, L)).all()
    ctx.negate(da, do, 3, L)
    assert (do.to_numpy(a.shape) == octx.negate(a, 3, L)).all()
    ctx.dyadic_mul(da, db, do, 3, 1, L)
    assert (do.to_numpy(a.shape) == octx.multiply_plain(a, 3, L, b[0])).all()
    scal = [primes[0] - 1, 0, (1 << 64) - 1]
    pt = np.stack([np.full(n, scal[i] % primes[i], dtype=np.uint64) for i in range(L)])
    ctx.mul_scalar_rows(da, scal, do, 3, L)
    assert (do.to_numpy(a.shape) == octx.multiply_plain(a, 3, L, pt)).all()
    ctx.add_scalar_rows(da, scal, do, 3, L)
    assert (do.to_numpy(a.shape) == octx.add(a, np.ascontiguousarray(np.broadcast_to(pt, a.shape)), 3, L)).all()

    # the monomial product: N >= 4, refused at N = 2 (test_mul_i_needs_four_coefficients)
    if logn >= 2:
        minus = monomial_ntt(octx, primes, negative=True)
        ctx.mul_i_add(da, db, do, 3, L, -1)
        assert (do.to_numpy(a.shape) == octx.add(a, octx.multiply_plain(b, 3, L, minus), 3, L)).all()
        do2 = moai.DeviceBuffer(a.size)
        ctx.real_split(da, db, do, do2, 3, L)
        assert (do.to_numpy(a.shape) == octx.add(a, b, 3, L)).all()
        assert (do2.to_numpy(a.shape) == octx.multiply_plain(octx.sub(a, b, 3, L), 3, L, minus).reshape(a.shape)).all()
    else:
        with pytest.raises(moai.hip.MoaiError):
            ctx.mul_i_add(da, db, do, 3, L, -1)

    # the pointer sums, three terms on a base
    T = 3
    xs = [sweep_data(rng, primes, (2,), n) for _ in range(T)]
    ys = [sweep_data(rng, primes, (2,), n) for _ in range(T)]
    dxs, dys = [up(moai, x) for x in xs], [up(moai, y) for y in ys]
    base2, base3 = sweep_data(rng, primes, (2,), n), sweep_data(rng, primes, (3,), n)
    sc = np.stack([np.array([primes[0] - 1, 0, int(rng.integers(0, primes[2]))], dtype=np.uint64) for _ in range(T)])
    sc[1] = np.array([int(rng.integers(0, q)) for q in primes], dtype=np.uint64)
    d2 = moai.DeviceBuffer(2 * L * n)
    ctx.scalar_dot(dxs, sc, up(moai, base2), d2, 2, L)
    terms = [octx.multiply_plain(xs[t], 2, L, np.ascontiguousarray(np.broadcast_to(sc[t][:, None], (L, n)))) for t in range(T)]
    assert (d2.to_numpy((2, L, n)) == chain_sum(octx, [base2] + terms, 2, L).reshape(2, L, n)).all(), "scalar_dot"
    ps = sweep_data(rng, primes, (T,), n)
    ctx.vector_dot(dxs, up(moai, ps), up(moai, base2), d2, 2, L)
    terms = [octx.multiply_plain(xs[t], 2, L, ps[t]) for t in range(T)]
    assert (d2.to_numpy((2, L, n)) == chain_sum(octx, [base2] + terms, 2, L).reshape(2, L, n)).all(), "vector_dot"
    d3 = moai.DeviceBuffer(3 * L * n)
    ctx.ct_dot_ptrs(dxs, dys, up(moai, base3), d3, L)
    prods = [octx.multiply(xs[t], ys[t], L) for t in range(T)]
    assert (d3.to_numpy((3, L, n)) == chain_sum(octx, [base3] + prods, 3, L).reshape(3, L, n)).all(), "ct_dot_ptrs"
    ctx.ct_dot(up(moai, np.stack(xs)), up(moai, np.stack(ys)), d3, T, L)
    assert (d3.to_numpy((3, L, n)) == chain_sum(octx, prods, 3, L).reshape(3, L, n)).all(), "ct_dot"

    # ciphertext products
    X, Y = np.stack(xs[:2]), np.stack(ys[:2])
    d6 = moai.DeviceBuffer(2 * 3 * L * n)
    ctx.ct_multiply(up(moai, X), up(moai, Y), d6, L, 2)
    assert (d6.to_numpy((2, 3, L, n)) == np.stack([octx.multiply(X[i], Y[i], L) for i in range(2)])).all(), "ct_multiply"
    ctx.ct_square(up(moai, X), d6, L, 2)
    assert (d6.to_numpy((2, 3, L, n)) == np.stack([octx.square(X[i], L) for i in range(2)])).all(), "ct_square"
    d4 = moai.DeviceBuffer(4 * L * n)
    ctx.ct_multiply_general(da, 3, dxs[0], 2, d4, L, 1)
    assert (d4.to_numpy((4, L, n)) == octx.multiply_general(a, 3, xs[0], 2, L)).all(), "ct_multiply_general"

    # sums of ciphertext x plaintext products: 2 polynomials (one per thread) and 5 (four per thread, a short last group)
    n_ops, n_pt, terms_n = 2, 3, 3
    xi, pi, pi2 = [1, 0, 1], [2, 0, 1], [0, 2]
    p = sweep_data(rng, primes, (n_pt,), n)
    dp = up(moai, p)
    for n_poly in (2, 5):
        x = sweep_data(rng, primes, (n_ops, n_poly), n)
        dx = up(moai, x)
        o1, o2 = moai.DeviceBuffer(n_poly * L * n), moai.DeviceBuffer(n_poly * L * n)
        want = chain_sum(octx, [octx.multiply_plain(x[xi[t]], n_poly, L, p[pi[t]]) for t in range(terms_n)], n_poly, L)
        want2 = chain_sum(octx, [octx.multiply_plain(x[xi[t]], n_poly, L, p[pi2[t]]) for t in range(2)], n_poly, L)
        ctx.ct_pt_dot(dx, dp, o1, xi, pi, n_poly, L)
        assert (o1.to_numpy((n_poly, L, n)) == want.reshape(n_poly, L, n)).all(), ("ct_pt_dot", n_poly)
        o1.upload(np.zeros(n_poly * L * n, dtype=np.uint64))
        ctx.ct_pt_dot2(dx, dp, o1, o2, xi, pi, pi2, n_poly, L)
        assert (o1.to_numpy((n_poly, L, n)) == want.reshape(n_poly, L, n)).all(), ("ct_pt_dot2", n_poly)
        assert (o2.to_numpy((n_poly, L, n)) == want2.reshape(n_poly, L, n)).all(), ("ct_pt_dot2, second sum", n_poly)
    rows = 3
    x = sweep_data(rng, primes, (rows, 2), n)
    p1, p2 = sweep_data(rng, primes, (rows,), n), sweep_data(rng, primes, (rows,), n)
    o1, o2 = moai.DeviceBuffer(2 * L * n), moai.DeviceBuffer(2 * L * n)
    ctx.ct_pt_dot_rows(up(moai, x), up(moai, p1), up(moai, p2), o1, o2, rows, 2, L)
    for o, pl in ((o1, p1), (o2, p2)):
        want = chain_sum(octx, [octx.multiply_plain(x[r], 2, L, pl[r]) for r in range(rows)], 2, L)
        assert (o.to_numpy((2, L, n)) == want.reshape(2, L, n)).all(), "ct_pt_dot_rows"

    # the matrix product, 3 x 17: the integer kernel (a 61-bit prime in the level), then the FP64 one on the two rows below 2^51
    cols = 17
    for Lm, pidx in ((L, None), (2, [1, 2])):
        sub = primes if pidx is None else [primes[i] for i in pidx]
        mo, mc = contexts(moai, logn, sub)
        x = sweep_data(rng, sub, (rows, 2), n)
        w = np.stack([rng.integers(0, q, size=(rows, cols), dtype=np.uint64) for q in sub])
        w[:, 0, 0] = qcol(sub)[:, 0] - np.uint64(1)
        dout = moai.DeviceBuffer(cols * 2 * Lm * n)
        mc.ct_pt_matmul(up(moai, x), up(moai, w), dout, rows, cols, 2, Lm)
        got = dout.to_numpy((cols, 2, Lm, n))
        for col in range(cols):
            pts = [np.ascontiguousarray(np.broadcast_to(w[:, j, col][:, None], (Lm, n))) for j in range(rows)]
            want = chain_sum(mo, [mo.multiply_plain(x[j], 2, Lm, pts[j]) for j in range(rows)], 2, Lm)
            assert (got[col] == want.reshape(2, Lm, n)).all(), ("ct_pt_matmul", Lm, col)

    # row moves
    X3 = np.stack([a[:2], b[:2]])
    dd = moai.DeviceBuffer(2 * 2 * 2 * n)
    ctx.mod_drop(up(moai, X3), dd, 2, L, 1, 2)
    assert (dd.to_numpy((2, 2, 2, n)) == np.stack([octx.mod_drop(X3[i], 2, L, 1) for i in range(2)])).all(), "mod_drop"
    elt = ctx.galois_elt_from_step(0)
    assert elt == 2 * n - 1 == O.galois_elt_from_step(logn, 0)
    ctx.galois_permute(da, do, 3, L, elt)
    assert (do.to_numpy(a.shape) == a[:, :, O.galois_table_ntt(logn, elt)]).all(), "galois_permute, conjugation"
    if n // 2 > 1:
        elt = ctx.galois_elt_from_step(1)
        assert elt == O.galois_elt_from_step(logn, 1)
        ctx.galois_permute(da, do, 3, L, elt)
        assert (do.to_numpy(a.shape) == a[:, :, O.galois_table_ntt(logn, elt)]).all(), "galois_permute, step 1"
    else:  # one slot: no rotation to take
        with pytest.raises(moai.MoaiError):
            ctx.galois_elt_from_step(1)
        with pytest.raises(ValueError):
            O.galois_elt_from_step(logn, 1)

    # three separate blocks <-> one packed array
    words = L * n
    blocks = [up(moai, a[i]) for i in range(3)]
    packed = moai.DeviceBuffer(3 * words)
    ctx.gather_blocks(blocks, packed, words)
    assert (packed.to_numpy(a.shape) == a).all(), "gather_blocks"
    ctx.scatter_blocks(db, blocks, words)
    for i in range(3):
        assert (blocks[i].to_numpy((L, n)) == b[i]).all(), "scatter_blocks"


# ---- 4. the FP64 matrix product at its limits ----------------------------------------------------------------------------
# level chain (the data primes of the product), and the unused last prime of the context
MATMUL_CHAINS = {
    "fold16": (("mm_hi", "fpn_hi", "small"), "g60"),       # every prime below 2^52 / 25: a fold every 16 rows
    "fold1": (("mm_lo", "fpr_hi", "fpr_lo"), "g60"),       # the first two at or above it: a fold every row
    "both": (("mm_hi", "mm_lo", "fpr_hi"), "g61"),         # both in one launch
    "integer": (("fpr_hi", "int_lo"), "g60"),              # one prime at 2^51: the level takes the integer kernel
}
MATMUL_ROWS = (15, 16, 17, 32, 33, 49)
MATMUL_INPUTS = ("worst", "worst, w = q - w", "all q-1", "pair patterns x random weights")


def takes_fp64(primes, matmul_fp=1):
    """the written contract of moai_ct_pt_matmul's kernel selection (csrc/elementwise.hip): the exact FP64 kernel when every prime
    of the level is below 2^51 and MOAI_MATMUL_FP is not 0; all or nothing"""
    return matmul_fp != 0 and all(q < 1 << 51 for q in primes)


def matmul_inputs(primes, rows, cols, size, n, rng):
    """per input of MATMUL_INPUTS: x [rows][size][L][N], w [L][rows][cols]"""
    L = len(primes)
    xw = np.empty((rows, size, L, n), dtype=np.uint64)
    w, wn = np.empty((L, rows, cols), dtype=np.uint64), np.empty((L, rows, cols), dtype=np.uint64)
    top_x, top_w = np.empty_like(xw), np.empty_like(w)
    px, pw = np.empty_like(xw), np.empty_like(w)
    for r, q in enumerate(primes):
        x1, w[r], wn[r] = ML.matmul_worst(q, rows, cols, n, rng)
        xw[:, 0, r], xw[:, 1, r] = x1, np.roll(x1, 1, axis=-1)  # the second polynomial: the signs exchanged
        top_x[:, :, r], top_w[r] = q - 1, q - 1
        for j in range(rows):
            for p in range(size):
                u, v = ML.pair_patterns(q, max(n, 32), rng)
                px[j, p, r] = (u if (j + p) % 2 else v)[:n]
        pw[r] = rng.integers(0, q, size=(rows, cols), dtype=np.uint64)
    return list(zip(MATMUL_INPUTS, (xw, xw, top_x, px), (w, wn, top_w, pw)))


def matmul_expected(x, w, level):
    """[cols][size][L][N] = sum_j x[j] w[j][c] mod q in exact integers (ML.matmul_mod), computed once per distinct coefficient: the
    worst-case x repeats with period 2, the all q-1 one with period 1"""
    n = x.shape[-1]
    period = next(p for p in (1, 2, n) if (x == np.tile(x[..., :p], n // p)).all())
    want = np.stack([ML.matmul_mod(x[:, :, r, :period], w[r], q) for r, q in enumerate(level)], axis=2)
    return np.tile(want, n // period)


@pytest.mark.parametrize("which", list(MATMUL_CHAINS))
@pytest.mark.parametrize("logn", [12, 8])
def test_ct_pt_matmul_fp64_kernel_at_its_limits(moai, logn, which):
    """Expected: sum_j x_j w_jc mod q in exact integers (ML.matmul_mod), the same bits from the integer kernel (MOAI_MATMUL_FP=0).
    Which kernel ran cannot be observed; the selection rule is restated (takes_fp64) and asserted on the chain's primes.
    N = 256 leaves the x-grid with one half-filled workgroup; 17 columns are a full group of sixteen and a group of one.
    What binds: a prime of [2^52 / 25, 2^51) that is folded every 16 rows instead of every row fails here (sixteen products at
    +-q/2 reach 8 q = 2^54 under fpr_hi, past the 2^53 up to which doubles hold every integer).  What cannot bind: below 2^52 / 25
    the period of 16 has slack -- every product comes out below 0.9 q (csrc/modarith.hip.h fp_mulmod_q), so even 32 rows on a folded
    sum stay below 29.3 q < 1.18 * 2^52 and a fold at row 31 instead of 15 gives the same bits on every input."""
    n, size, cols = 1 << logn, 2, 17
    names, last = MATMUL_CHAINS[which]
    c = ML.matmul_chain(logn)
    level = [c[x] for x in names]
    L = len(level)
    octx, ctx = contexts(moai, logn, level + [c[last]])
    assert takes_fp64(level) == (which != "integer") and not takes_fp64(level, matmul_fp=0)
    every_row = [not q < ML.MATMUL_FOLD_LIMIT for q in level]
    # (fpr_lo, the third prime of "fold1", is itself below 2^52 / 25 = 2^47.36: 33 q >= 2^52 puts it at 2^46.96)
    assert every_row == {"fold16": [False] * 3, "fold1": [True, True, False], "both": [False, True, True], "integer": [True, True]}[which]
    rng = np.random.default_rng(7500 + logn)
    try:
        for rows in MATMUL_ROWS:
            for name, x, w in matmul_inputs(level, rows, cols, size, n, rng):
                want = matmul_expected(x, w, level)
                if name == "all q-1":
                    assert all((want[:, :, r] == rows * (q - 1) * (q - 1) % q).all() for r, q in enumerate(level))
                dx, dw = up(moai, x), up(moai, w)
                dout = moai.DeviceBuffer(cols * size * L * n)
                for fp in (1, 0):
                    moai.hip.set_tuning("MOAI_MATMUL_FP", fp)
                    dout.upload(np.zeros(cols * size * L * n, dtype=np.uint64))
                    ctx.ct_pt_matmul(dx, dw, dout, rows, cols, size, L)
                    got = dout.to_numpy(want.shape)
                    bad = np.argwhere(got != want)
                    assert not len(bad), (rows, name, "MOAI_MATMUL_FP=%d" % fp, "first of %d at [col, poly, row, coeff]" % len(bad), bad[0].tolist())
                for buf in (dx, dw, dout):
                    buf.free()
    finally:
        moai.hip.reset_tuning()
