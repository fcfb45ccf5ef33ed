"""GPU tests of the hybrid key switches on a list of ciphertexts (include/moai_hip.h, "hybrid key switches on a list of ciphertexts":
moai_apply_galois_hybrid_to, moai_apply_galois_hybrid_acc, moai_apply_galois_hybrid_ptrs, moai_relinearize_hybrid_ptrs,
moai_relinearize_rescale_hybrid_ptrs).  Everything is bit for bit.

1. alpha = 1: the list calls are moai_apply_galois_ptrs / moai_relinearize_ptrs (small transform, logn 10, and the tiled one, logn 12).
2. alpha > 1: the list equals the single calls at batch 1 and the integer restatements tests/hybrid_ref.py and
   tests/hybrid_rescale_ref.py, with a member of rows q - 1, a zero member and a member that repeats another's key and element.
3. Sums and in-place members equal moai_apply_galois_hybrid_acc / _to / the in-place call run singly.
4. _to and _acc at batch 3 equal the in-place call on a copy, and that plus moai_add; out == in works; so under a budget of two.
5. Passes: n = 70 crosses the 64 members of a record; a scratch budget of exactly two members (asserted from the header's formula);
   both give the bits of the default budget.
6. Digits of 6 and 12 primes once each, 7. N = 2^16 at MOAI's parameters once: against the singles.
8. Every refusal of the contract is MOAI_EINVAL with its message, names the member and leaves every output and input alone.
9. moai_op_trace counts the calls they replace.

Outputs are pre-filled with a pattern; after every call the inputs and keys are compared with what was uploaded.  The restatement is
computed once per shape and shared."""
import numpy as np
import pytest

import hybrid_kit
import hybrid_ref as HR
import hybrid_rescale_ref as RR
import oracle as O
from hybrid_kit import EINVAL, ENVS, FILL, MOAI_DATA_BITS, traced, tuned

pytestmark = pytest.mark.gpu


class Env(hybrid_kit.Env):
    """with n_keys uniform keys on host and device, and the elements of two rotations and the conjugation"""

    def __init__(self, moai, logn, data_bits, special_bits, n_keys=3, oracle=True):
        super().__init__(moai, logn, data_bits, special_bits, oracle=oracle)
        rng = np.random.default_rng(1000 + logn + self.k)
        self.keys = [self.random_key(rng) for _ in range(n_keys)]
        self.dkeys = [self.up(key) for key in self.keys]
        self.elements = self.elts([1, 3, 0])

    def out_block(self, L):
        """an output of two polynomials, filled with the pattern"""
        return self.filled((2, L, self.n), FILL)

    def members(self, rng, L, n):
        """n members (ciphertext, element, key index): keys and elements come round, so member 3 repeats member 0's key and element;
        from three members on, member 1 has every row q - 1 and member 2 is zero"""
        cts = O.uniform_rns(rng, self.primes[:L], (n, 2), self.n)
        if n >= 3:
            cts[1], cts[2] = self.edges(L, 2)
        return [(cts[i], self.elements[i % 3], i % len(self.keys)) for i in range(n)]

    def ct3s(self, rng, L, n):
        c = O.uniform_rns(rng, self.primes[:L], (n, 3), self.n)
        if n >= 3:
            c[1], c[2] = self.edges(L, 3)
        return c

    def keys_unchanged(self):
        for i, (d, key) in enumerate(zip(self.dkeys, self.keys)):
            assert (d.to_numpy(key.shape) == key).all(), "key %d was written" % i


_envs = {}


@pytest.fixture
def env(moai):
    def get(name):
        if name not in _envs:
            _envs[name] = Env(moai, *ENVS[name])
        return _envs[name]
    return get


def unchanged(bufs, hosts):
    for i, (d, h) in enumerate(zip(bufs, hosts)):
        assert (d.to_numpy(words=h.size) == h.reshape(-1)).all(), "input %d was written" % i


def run_galois_ptrs(e, L, members, sums=None):
    """the list call on fresh blocks with pattern-filled outputs; the inputs and keys are compared afterwards"""
    d_in = [e.up(ct) for ct, _, _ in members]
    d_out = [e.out_block(L) for _ in members]
    e.ctx.apply_galois_hybrid_ptrs(d_in, d_out, L, e.alpha, [m[1] for m in members], [e.dkeys[m[2]] for m in members], sums)
    got = [d.to_numpy((2, L, e.n)) for d in d_out]
    unchanged(d_in, [m[0] for m in members])
    return got


def single_galois(e, L, members):
    out = []
    for ct, elt, ki in members:
        d = e.up(ct)
        e.ctx.apply_galois_hybrid(d, L, e.alpha, elt, e.dkeys[ki], 1)
        out.append(d.to_numpy((2, L, e.n)))
    return out


def run_relin_ptrs(e, L, ct3, rescale):
    Lout = L - 1 if rescale else L
    d_in = [e.up(c) for c in ct3]
    d_out = [e.out_block(Lout) for _ in ct3]
    call = e.ctx.relinearize_rescale_hybrid_ptrs if rescale else e.ctx.relinearize_hybrid_ptrs
    call(d_in, d_out, e.dkeys[0], L, e.alpha)
    got = [d.to_numpy((2, Lout, e.n)) for d in d_out]
    unchanged(d_in, list(ct3))
    return got


def single_relin(e, L, ct3, rescale):
    Lout = L - 1 if rescale else L
    call = e.ctx.relinearize_rescale_hybrid if rescale else e.ctx.relinearize_hybrid
    out = []
    for c in ct3:
        d = e.out_block(Lout)
        call(e.up(c), e.dkeys[0], d, L, e.alpha, 1)
        out.append(d.to_numpy((2, Lout, e.n)))
    return out


def same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g == np.asarray(w).reshape(g.shape)).all(), (what, i)


# ---- 1. alpha = 1 equals the SEAL-style list calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small1", "tiled1"])
@pytest.mark.parametrize("level", ["top", "one"])
def test_alpha_1_equals_the_seal_style_list_calls(env, which, level):
    e = env(which)
    L, n = (e.lmax if level == "top" else 1), 3
    rng = np.random.default_rng(e.logn * 10 + L)
    members = e.members(rng, L, n)
    elts, keys = [m[1] for m in members], [e.dkeys[m[2]] for m in members]
    assert sorted(elts) == sorted(e.elements) and len(set(m[2] for m in members)) == 3
    addends = O.uniform_rns(rng, e.primes[:L], (n, 2), e.n)
    for with_sums in (False, True):
        d_in = [e.up(m[0]) for m in members]
        sums = [e.up(addends[0]), None, e.up(addends[2])] if with_sums else None
        a, b = [e.out_block(L) for _ in members], [e.out_block(L) for _ in members]
        e.ctx.apply_galois_ptrs(d_in, a, L, elts, keys, sums)
        e.ctx.apply_galois_hybrid_ptrs(d_in, b, L, 1, elts, keys, sums)
        same([d.to_numpy((2, L, e.n)) for d in b], [d.to_numpy((2, L, e.n)) for d in a], "sums %s" % with_sums)
        unchanged(d_in, [m[0] for m in members])
        if with_sums:
            unchanged([sums[0], sums[2]], [addends[0], addends[2]])
    ct3 = e.ct3s(rng, L, n)
    d_in = [e.up(c) for c in ct3]
    a, b = [e.out_block(L) for _ in ct3], [e.out_block(L) for _ in ct3]
    e.ctx.relinearize_ptrs(d_in, a, e.dkeys[1], L)
    e.ctx.relinearize_hybrid_ptrs(d_in, b, e.dkeys[1], L, 1)
    same([d.to_numpy((2, L, e.n)) for d in b], [d.to_numpy((2, L, e.n)) for d in a], "relinearize")
    unchanged(d_in, list(ct3))
    e.keys_unchanged()


# ---- 2. alpha > 1 against the singles and the restatement -------------------------------------------------------------------------------
SHAPES = [("small2", 5), ("small2", 3), ("small2", 1), ("tiled3", 7), ("tiled3", 4)]
_ref = {}


def galois_case(e, which, L):
    """(members, the restatement's outputs) of a shape, computed once"""
    if ("galois", which, L) not in _ref:
        members = e.members(np.random.default_rng(e.logn * 100 + L), L, 5)
        _ref["galois", which, L] = members, [HR.apply_galois(e.octx, ct, L, elt, e.keys[ki], e.alpha) for ct, elt, ki in members]
    return _ref["galois", which, L]


def relin_case(e, which, L, rescale):
    """(four ct3, the restatement's outputs): the list of one member is the first of them"""
    kind = "rescale" if rescale else "relin"
    if (kind, which, L) not in _ref:
        ct3 = e.ct3s(np.random.default_rng(e.logn * 100 + L + 50), L, 4)
        f = RR.relinearize_rescale if rescale else HR.relinearize
        _ref[kind, which, L] = ct3, [f(e.octx, c, e.keys[0], L, e.alpha) for c in ct3]
    return _ref[kind, which, L]


@pytest.mark.parametrize("which,L", SHAPES)
def test_apply_galois_list_against_the_singles_and_the_restatement(env, which, L):
    e = env(which)
    members, want = galois_case(e, which, L)
    assert members[3][1:] == members[0][1:] and len(set(m[2] for m in members)) == 3 and len(set(m[1] for m in members)) == 3
    got = run_galois_ptrs(e, L, members)
    same(got, single_galois(e, L, members), "singles")
    same(got, want, "restatement")
    e.keys_unchanged()


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("which,L", SHAPES)
def test_relinearize_list_against_the_singles_and_the_restatement(env, which, L, n):
    e = env(which)
    ct3, want = relin_case(e, which, L, False)
    got = run_relin_ptrs(e, L, ct3[:n], False)
    same(got, single_relin(e, L, ct3[:n], False), "singles")
    same(got, want[:n], "restatement")
    e.keys_unchanged()


@pytest.mark.parametrize("which,L", [("small2", 5), ("small2", 2), ("tiled3", 7)])
def test_relinearize_rescale_list_against_the_singles_and_the_restatement(env, which, L):
    e = env(which)
    ct3, want = relin_case(e, which, L, True)
    got = run_relin_ptrs(e, L, ct3[:3], True)
    same(got, single_relin(e, L, ct3[:3], True), "singles")
    same(got, want[:3], "restatement")
    e.keys_unchanged()


# ---- 3. sums and in-place members -----------------------------------------------------------------------------------------------------
def test_sums_and_in_place_members(env):
    """member 0 plain, members 1 and 2 with sums, outs[2] is sums[2], outs[3] is ins[3]"""
    e, L, n = env("small2"), 5, 4
    rng = np.random.default_rng(9)
    members = e.members(rng, L, n)
    addends = O.uniform_rns(rng, e.primes[:L], (n, 2), e.n)
    single = []
    for i, (ct, elt, ki) in enumerate(members):
        if i in (1, 2):
            acc = e.up(addends[i])
            e.ctx.apply_galois_hybrid_acc(e.up(ct), acc, L, e.alpha, elt, e.dkeys[ki], 1)
            single.append(acc.to_numpy((2, L, e.n)))
        elif i == 0:
            d = e.out_block(L)
            e.ctx.apply_galois_hybrid_to(e.up(ct), d, L, e.alpha, elt, e.dkeys[ki], 1)
            single.append(d.to_numpy((2, L, e.n)))
        else:
            d = e.up(ct)
            e.ctx.apply_galois_hybrid(d, L, e.alpha, elt, e.dkeys[ki], 1)
            single.append(d.to_numpy((2, L, e.n)))
    plain = single_galois(e, L, members)
    q = np.array(e.primes[:L], dtype=np.uint64).reshape(1, L, 1)
    for i in (1, 2):
        assert (single[i] == (plain[i] + addends[i]) % q).all(), i  # _acc is the switch followed by moai_add's canonical sum
    d_in = [e.up(m[0]) for m in members]
    d_sum = [None, e.up(addends[1]), e.up(addends[2]), None]
    d_out = [e.out_block(L), e.out_block(L), d_sum[2], d_in[3]]
    e.ctx.apply_galois_hybrid_ptrs(d_in, d_out, L, e.alpha, [m[1] for m in members], [e.dkeys[m[2]] for m in members], d_sum)
    same([d.to_numpy((2, L, e.n)) for d in d_out], single, "singles")
    unchanged([d_sum[1]], [addends[1]])  # a sum that is not an output is only read
    unchanged(d_in[:3], [m[0] for m in members[:3]])
    e.keys_unchanged()


# ---- 4. _to and _acc at batch 3 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,L", [("small2", 5), ("tiled3", 4)])
def test_to_and_acc_at_batch_3(moai, env, which, L):
    e, B = env(which), 3
    rng = np.random.default_rng(44 + L)
    ct = O.uniform_rns(rng, e.primes[:L], (B, 2), e.n)
    base = O.uniform_rns(rng, e.primes[:L], (B, 2), e.n)
    elt, dkey = e.elements[1], e.dkeys[2]
    per = (HR.beta(L, e.alpha) * (L + e.alpha) + 4 * L + 4 * e.alpha + 2 * L) * e.n * 8
    two = 2 * per + per // 2 >> 10  # KiB that hold two ciphertexts of the batch, not three
    assert (two << 10) // per == 2
    want = e.up(ct)
    e.ctx.apply_galois_hybrid(want, L, e.alpha, elt, dkey, B)
    want = want.to_numpy((B, 2, L, e.n))
    summed = e.moai.DeviceBuffer(B * 2 * L * e.n)
    e.ctx.add(e.up(want), e.up(base), summed, B * 2, L)
    summed = summed.to_numpy((B, 2, L, e.n))
    with tuned(moai):
        for kb in (None, two):
            moai.hip.reset_tuning()
            if kb:
                moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", kb)
            src, dst = e.up(ct), e.filled((B, 2, L, e.n), FILL)
            e.ctx.apply_galois_hybrid_to(src, dst, L, e.alpha, elt, dkey, B)
            assert (dst.to_numpy((B, 2, L, e.n)) == want).all(), kb
            unchanged([src], [ct])
            e.ctx.apply_galois_hybrid_to(src, src, L, e.alpha, elt, dkey, B)  # out == in
            assert (src.to_numpy((B, 2, L, e.n)) == want).all(), kb
            src, acc = e.up(ct), e.up(base)
            e.ctx.apply_galois_hybrid_acc(src, acc, L, e.alpha, elt, dkey, B)
            assert (acc.to_numpy((B, 2, L, e.n)) == summed).all(), kb
            unchanged([src], [ct])
    e.keys_unchanged()


# ---- 5. passes ------------------------------------------------------------------------------------------------------------------------
def test_seventy_members_take_two_passes(moai, env):
    e, L, n = env("small2"), 1, 70
    members = e.members(np.random.default_rng(70), L, n)
    got = run_galois_ptrs(e, L, members)
    same(got, [HR.apply_galois(e.octx, ct, L, elt, e.keys[ki], e.alpha) for ct, elt, ki in members], "restatement")
    ct3 = e.ct3s(np.random.default_rng(71), L, n)
    relin = run_relin_ptrs(e, L, ct3, False)
    same(relin, [HR.relinearize(e.octx, c, e.keys[0], L, e.alpha) for c in ct3], "restatement")
    with tuned(moai):
        # a budget of 33 members: three passes of 33, 33 and 4
        per = (HR.beta(L, e.alpha) * (L + e.alpha) + 4 * L + 4 * e.alpha + 2 * L) * e.n * 8
        moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", 33 * per + 1023 >> 10)
        assert ((33 * per + 1023 >> 10) << 10) // per == 33
        same(run_galois_ptrs(e, L, members), got, "budget of 33")
    e.keys_unchanged()


def test_a_budget_of_two_members_gives_the_default_budgets_bits(moai, env):
    """n = 5 at L = 5, alpha = 2, beta = 3 on the small ring (rows of 8 KiB).  Rows of scratch per member as the header states them:
    beta (L + alpha) + 4L + 4 alpha + 2L = 59 for the rotation, ... + L = 54 for relinearize, and beta (L + alpha) + 2 (L + alpha) +
    2 (alpha + 1) + 2 (L - 1) + L = 54 for the rescale form: 1000 KiB hold exactly two members of each (passes of 2, 2, 1)"""
    e, L, n, kb = env("small2"), 5, 5, 1000
    a, beta = e.alpha, HR.beta(L, e.alpha)
    rows = {"galois": beta * (L + a) + 4 * L + 4 * a + 2 * L, "relin": beta * (L + a) + 4 * L + 4 * a + L,
            "rescale": beta * (L + a) + 2 * (L + a) + 2 * (a + 1) + 2 * (L - 1) + L}
    assert rows == {"galois": 59, "relin": 54, "rescale": 54}
    for r in rows.values():
        assert (kb << 10) // (r * e.n * 8) == 2
    members = e.members(np.random.default_rng(55), L, n)
    ct3 = e.ct3s(np.random.default_rng(56), L, n)
    got = {}
    with tuned(moai):
        for budget in (None, kb):
            moai.hip.reset_tuning()
            if budget:
                moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", budget)
            got[budget] = (run_galois_ptrs(e, L, members), run_relin_ptrs(e, L, ct3, False), run_relin_ptrs(e, L, ct3, True))
    for x, y in zip(got[kb], got[None]):
        same(x, y, "budget")
    same(got[None][0], single_galois(e, L, members), "singles")
    e.keys_unchanged()


# ---- 6. wide digits, 7. N = 2^16 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [6, 12])
def test_wide_digits_against_the_singles(moai, alpha):
    """digits of 6 and 12 primes: the conversion kernel's instantiations for up to 8 and up to 16 source rows; alpha + 1 data primes
    leave a last digit of one prime"""
    e = Env(moai, 10, [40] * (alpha + 1), [50] * alpha, n_keys=2, oracle=False)
    L = alpha + 1
    members = e.members(np.random.default_rng(alpha), L, 2)
    same(run_galois_ptrs(e, L, members), single_galois(e, L, members), "galois")
    ct3 = e.ct3s(np.random.default_rng(alpha + 1), L, 2)
    for rescale in (False, True):
        same(run_relin_ptrs(e, L, ct3, rescale), single_relin(e, L, ct3, rescale), "relin, rescale %s" % rescale)
    e.keys_unchanged()
    e.close()


def test_n65536_at_moais_parameters_once(moai):
    """N = 2^16, MOAI's 35 data primes plus 12 sixty-bit special primes, L = 15, two members with two keys"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12, n_keys=2, oracle=False)
    L = 15
    rng = np.random.default_rng(16)
    cts = O.uniform_rns(rng, e.primes[:L], (2, 2), e.n)
    members = [(cts[0], e.elements[0], 0), (cts[1], e.elements[2], 1)]
    same(run_galois_ptrs(e, L, members), single_galois(e, L, members), "galois")
    ct3 = e.ct3s(rng, L, 2)
    same(run_relin_ptrs(e, L, ct3, True), single_relin(e, L, ct3, True), "rescale")
    e.keys_unchanged()
    e.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_names_the_member_and_writes_nothing(moai, env):
    e, L, n = env("small2"), 3, 3
    a, N = e.alpha, e.n
    members = e.members(np.random.default_rng(1), L, n)
    ct3 = e.ct3s(np.random.default_rng(2), L, n)
    fill = np.full((2, L, N), FILL, dtype=np.uint64)
    d_in, d_out, d_ct3 = [e.up(m[0]) for m in members], [e.up(fill) for _ in members], [e.up(c) for c in ct3]
    d_sum = e.up(fill)
    elts, keys = [m[1] for m in members], [e.dkeys[m[2]] for m in members]
    words = 2 * L * N
    wide = Env(moai, 10, [40], [50] * 17, n_keys=1, oracle=False)  # 18 primes: alpha = 17 is below k and above 16

    def check(call, text):
        with pytest.raises(moai.hip.MoaiError, match=text) as err:
            call()
        assert err.value.code == EINVAL, text
        for i in range(n):
            assert (d_out[i].to_numpy(words=words) == FILL).all(), (text, i)
        assert (d_sum.to_numpy() == FILL).all(), text
        unchanged(d_in, [m[0] for m in members])
        unchanged(d_ct3, list(ct3))

    def galois(ctx=e.ctx, **change):
        g = dict(ins=d_in, outs=d_out, L=L, alpha=a, elts=elts, keys=keys, sums=None)
        g.update(change)
        return lambda: ctx.apply_galois_hybrid_ptrs(g["ins"], g["outs"], g["L"], g["alpha"], g["elts"], g["keys"], g["sums"])

    def relin(rescale, ctx=e.ctx, **change):
        g = dict(ins=d_ct3, outs=d_out, key=e.dkeys[0], L=L, alpha=a)
        g.update(change)
        f = ctx.relinearize_rescale_hybrid_ptrs if rescale else ctx.relinearize_hybrid_ptrs
        return lambda: f(g["ins"], g["outs"], g["key"], g["L"], g["alpha"])

    hole = lambda xs: [xs[0], None, xs[2]]
    cases = [
        (galois(ins=hole(d_in)), "member 1: null pointer"),
        (galois(outs=hole(d_out)), "member 1: null pointer"),
        (galois(keys=hole(keys)), "member 1: null pointer"),
        (galois(elts=[elts[0], elts[1], 6]), "member 2: Galois element is not valid"),
        (galois(elts=[elts[0], 6, elts[2]], alpha=0), "member 1: Galois element is not valid"),  # before alpha
        (galois(alpha=0, L=0), "alpha = 0"),
        (galois(L=0), "L = 0"),
        (galois(alpha=e.k), "alpha = %d leaves no data prime" % e.k),
        (galois(ctx=wide.ctx, alpha=17, L=1), "alpha = 17: digits of more than 16 primes"),
        (galois(L=e.lmax + 1), "L = %d out of range" % (e.lmax + 1)),
        (galois(L=e.lmax + 1, elts=[elts[0], 2 * N + 1, elts[2]]), "L = %d out of range" % (e.lmax + 1)),  # before the element's range
        (galois(elts=[elts[0], 2 * N + 1, elts[2]]), "member 1: Galois element is not valid"),
        (galois(outs=[d_out[0].ptr, d_in[1].ptr + 8 * N, d_out[2].ptr]), "member 1: the output overlaps the input"),  # a part of its own
        (galois(sums=[None, d_sum.ptr, None], outs=[d_out[0].ptr, d_sum.ptr + 8 * N, d_out[2].ptr]), "member 1: the output overlaps the sum"),
        (galois(sums=[d_in[0], None, None]), "member 0: the sum is the input"),
        (galois(outs=[d_out[0], d_out[0], d_out[2]]), "the output overlaps a block of member"),  # two members, one output
        (galois(outs=[d_out[0], d_in[2], d_out[2]]), "member 1: the output overlaps a block of member 2"),  # another member's input
        (galois(sums=[None, d_out[2], None]), "the output overlaps a block of member"),  # member 1's sum is member 2's output
    ]
    for rescale in (False, True):
        cases += [
            (relin(rescale, ins=hole(d_ct3)), "member 1: null pointer"),
            (relin(rescale, outs=hole(d_out)), "member 1: null pointer"),
            (relin(rescale, alpha=0, L=0), "alpha = 0"),
            (relin(rescale, L=0), "L = 0"),
            (relin(rescale, alpha=e.k), "alpha = %d leaves no data prime" % e.k),
            (relin(rescale, L=e.lmax + 1), "L = %d out of range" % (e.lmax + 1)),
            (relin(rescale, outs=[d_out[0], d_ct3[1], d_out[2]]), "member 1: the output overlaps the input"),  # the output may not be the input
            (relin(rescale, outs=[d_out[0].ptr, d_ct3[1].ptr + 16 * N, d_out[2].ptr]), "member 1: the output overlaps the input"),
            (relin(rescale, outs=[d_out[0], d_out[1], d_ct3[0]]), "member 2: the output overlaps a block of member 0"),
        ]
    cases += [
        (relin(True, L=1), "L = 1: no prime left to rescale to"),
        (relin(True, ctx=wide.ctx, alpha=16, L=1), "L = 1: no prime left to rescale to"),
        (relin(True, ctx=wide.ctx, alpha=16, L=2), "alpha = 16: the merged mod-down converts alpha \\+ 1 residues"),
        # _to / _acc: moai_apply_galois_hybrid's refusals, then the pointers
        (lambda: e.ctx.apply_galois_hybrid_to(d_in[0], d_out[0], L, a, 6, keys[0], 1), "Galois element is not valid"),
        (lambda: e.ctx.apply_galois_hybrid_to(d_in[0], d_out[0], L, 0, elts[0], keys[0], 1), "alpha = 0"),
        (lambda: e.ctx.apply_galois_hybrid_to(d_in[0], d_out[0], e.lmax + 1, a, elts[0], keys[0], 1), "out of range"),
        (lambda: e.ctx.apply_galois_hybrid_to(d_in[0], d_out[0], L, a, 2 * N + 1, keys[0], 1), "Galois element is not valid"),
        (lambda: e.ctx.apply_galois_hybrid_to(None, d_out[0], L, a, elts[0], keys[0], 1), "null argument"),
        (lambda: e.ctx.apply_galois_hybrid_to(d_in[0], None, L, a, elts[0], keys[0], 1), "null argument"),
        (lambda: e.ctx.apply_galois_hybrid_to(d_in[0], d_out[0], L, a, elts[0], None, 1), "null argument"),
        (lambda: e.ctx.apply_galois_hybrid_to(d_in[0].ptr, d_in[0].ptr + 8 * N, L, a, elts[0], keys[0], 1), "the output overlaps an input"),
        (lambda: e.ctx.apply_galois_hybrid_acc(d_in[0], d_in[0], L, a, elts[0], keys[0], 1), "the sum is the input"),
        (lambda: e.ctx.apply_galois_hybrid_acc(None, d_out[0], L, a, elts[0], keys[0], 1), "null argument"),
        (lambda: e.ctx.apply_galois_hybrid_acc(d_in[0].ptr + 8 * N, d_in[0].ptr, L, a, elts[0], keys[0], 1), "the output overlaps an input"),
    ]
    for call, text in cases:
        check(call, text)
    # a null list, and n == 0 whatever else is passed
    lib = moai.hip.lib()
    h = e.ctx.h
    assert lib.moai_apply_galois_hybrid_ptrs(h, None, None, L, a, None, None, None, n, None) == EINVAL and b"null list" in lib.moai_last_error()
    assert lib.moai_relinearize_hybrid_ptrs(h, None, None, keys[0].ptr, L, a, n, None) == EINVAL and b"null list" in lib.moai_last_error()
    assert lib.moai_relinearize_rescale_hybrid_ptrs(h, None, None, None, L, a, n, None) == EINVAL and b"null list" in lib.moai_last_error()
    assert lib.moai_apply_galois_hybrid_ptrs(h, None, None, 0, 0, None, None, None, 0, None) == 0
    assert lib.moai_relinearize_hybrid_ptrs(None, None, None, None, 0, 0, 0, None) == 0
    assert lib.moai_relinearize_rescale_hybrid_ptrs(None, None, None, None, 1, 16, 0, None) == 0
    check(galois(L=0), "L = 0")  # nothing above wrote anything
    # an output block of the rescale form is 2 (L - 1) N words: three outputs packed at that stride are no overlap, one word less is
    packed = e.filled(3 * 2 * (L - 1) * N + 8, FILL)
    step = 2 * (L - 1) * N * 8
    check(relin(True, outs=[packed.ptr, packed.ptr + step - 8, packed.ptr + 2 * step]), "the output overlaps a block of member")
    e.ctx.relinearize_rescale_hybrid_ptrs(d_ct3, [packed.ptr + i * step for i in range(3)], e.dkeys[0], L, a)
    got = packed.to_numpy()
    same(list(got[:3 * 2 * (L - 1) * N].reshape(3, 2, L - 1, N)), single_relin(e, L, ct3, True), "packed outputs")
    assert (got[3 * 2 * (L - 1) * N:] == FILL).all()
    e.keys_unchanged()
    wide.close()


# ---- 9. the census --------------------------------------------------------------------------------------------------------------------
def test_op_trace_counts_the_calls_they_replace(moai, env):
    e, L = env("small2"), 3
    members = e.members(np.random.default_rng(3), L, 5)
    ct3 = e.ct3s(np.random.default_rng(4), L, 4)
    batch = e.up(np.stack([m[0] for m in members[:3]]))
    with traced(moai) as trace:
        run_galois_ptrs(e, L, members)                                                 # 5
        e.ctx.apply_galois_hybrid_to(batch, e.out_block(3 * L), L, e.alpha, e.elements[0], e.dkeys[0], 3)  # 3
        e.ctx.apply_galois_hybrid_acc(batch, e.out_block(3 * L), L, e.alpha, e.elements[0], e.dkeys[0], 3)  # 3
        run_relin_ptrs(e, L, ct3, False)                                               # 4
        run_relin_ptrs(e, L, ct3[:2], True)                                            # 2
    counts = trace()
    assert counts.get(("apply_galois_hybrid", L)) == 11
    assert counts.get(("relinearize_hybrid", L)) == 4
    assert counts.get(("relinearize_rescale_hybrid", L)) == 2
