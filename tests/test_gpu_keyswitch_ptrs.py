"""GPU parity of the key switches on a list of ciphertexts (include/moai_hip.h: moai_apply_galois_ptrs,
moai_relinearize_ptrs): every member bit for bit against the CPU oracle's apply_galois / relinearize, as
tests/test_gpu_parity.py does for the batch forms, and against the single calls they replace.

Shapes: N = 2^12 is the smallest degree on the fused path (ks_contig_mac8 / moddown_contig), N = 2^11 the small path
(keyswitch_mac_kernel / moddown_finalize_kernel), N = 2^16 once for the LOGN = 16 instantiations.  The chain has a prime just
below 2^60 (integer butterflies with guards), one below 2^51 and one below 2^46 (the two FP64 modes) and a 60-bit special
prime, so one list runs integer and FP64 launches; n = 70 crosses the 64 members of a pass."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

BITS = [60, 51, 46, 60]
EINVAL, ERANGE = -1, -3


class Env:
    def __init__(self, moai, logn, bits=BITS, n_keys=4):
        self.logn, self.n = logn, 1 << logn
        self.primes = O.coeff_modulus_create(self.n, bits)
        self.k = len(self.primes)
        self.octx = O.Context(logn, self.primes)
        self.ctx = moai.Context(logn, self.primes)
        rng = np.random.default_rng(logn)
        self.keys = [O.uniform_rns(rng, self.primes, (self.k - 1, 2), self.n) for _ in range(n_keys)]
        self.dkeys = [moai.DeviceBuffer.from_numpy(key) for key in self.keys]
        # two rotations and the conjugation
        self.elts = [self.ctx.galois_elt_from_step(1), self.ctx.galois_elt_from_step(3), 2 * self.n - 1]

    def members(self, rng, L, n):
        """n members (ciphertext, element, key index); from the fourth on, elements and keys come round again: member 3 has
        member 0's element and key"""
        cts = O.uniform_rns(rng, self.primes[:L], (n, 2), self.n)
        return [(cts[i], self.elts[i % 3], (i % 3) if i != 4 else 3) for i in range(n)]

    def want(self, L, members):
        return [self.octx.apply_galois(ct, L, elt, self.keys[ki]).reshape(2, L, self.n) for ct, elt, ki in members]


@pytest.fixture(scope="module")
def env12(moai):
    return Env(moai, 12)


def set_fp(moai, fp):
    """fp: the FP64 modes from the first row on (the default keeps a few ciphertexts at a low level on the integer units)"""
    moai.hip.reset_tuning()
    if fp:
        moai.hip.set_tuning("MOAI_KS_FP_MIN_ROWS", 0)
        moai.hip.set_tuning("MOAI_MD_FP_MIN_ROWS", 0)


def run_ptrs(moai, e, L, members, sums=None, in_place=()):
    """the list call on fresh blocks; returns the downloaded outputs"""
    d_in = [moai.DeviceBuffer.from_numpy(ct) for ct, _, _ in members]
    d_out = [d_in[i] if i in in_place else moai.DeviceBuffer.from_numpy(np.full((2, L, e.n), 7, dtype=np.uint64)) for i in range(len(members))]
    e.ctx.apply_galois_ptrs(d_in, d_out, L, [elt for _, elt, _ in members], [e.dkeys[ki] for _, _, ki in members], sums)
    return [d.to_numpy((2, L, e.n)) for d in d_out]


def test_the_shape_runs_integer_and_fp64_modes(moai, env12):
    H = moai.hip
    try:
        set_fp(moai, True)
        for L, n in ((3, 5), (3, 1), (1, 2)):
            modes = [env12.ctx.arith_mode(p, H.MODE_OF_KEY_SWITCH, L, n) for p in list(range(L)) + [env12.k - 1]]
            assert any(m in (H.MODE_GUARD, H.MODE_NOGUARD) for m in modes), (L, n, modes)
            if L == 3:
                assert H.MODE_FPN in modes and H.MODE_FPR in modes, (L, n, modes)
    finally:
        moai.hip.reset_tuning()


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("L", [3, 1])
def test_apply_galois_ptrs_against_the_oracle(moai, env12, L, n):
    e = env12
    members = e.members(np.random.default_rng(100 * L + n), L, n)
    want = e.want(L, members)
    try:
        for fp in (False, True):
            set_fp(moai, fp)
            moai.hip.op_trace(True)
            got = run_ptrs(moai, e, L, members)
            moai.hip.op_trace(False)
            for i in range(n):
                assert (got[i] == want[i]).all(), (fp, i)
            # traced under the name of the calls it replaces, with batch = n
            assert moai.hip.op_trace_counts().get(("apply_galois_to", L)) == n
    finally:
        moai.hip.op_trace(False)
        moai.hip.reset_tuning()


def test_mixed_key_layouts_in_one_list(moai, env12):
    """a whole key, one trimmed to L levels and one trimmed to more; a member limited below L is MOAI_ERANGE, names the
    member and leaves every output untouched"""
    e, L = env12, 2
    members = e.members(np.random.default_rng(5), L, 3)
    want = e.want(L, members)
    trims = [e.ctx.key_trim(e.dkeys[1], L), e.ctx.key_trim(e.dkeys[2], L + 1), e.ctx.key_trim(e.dkeys[1], L - 1)]
    try:
        d_in = [moai.DeviceBuffer.from_numpy(ct) for ct, _, _ in members]
        fill = np.full((2, L, e.n), 7, dtype=np.uint64)
        d_out = [moai.DeviceBuffer.from_numpy(fill) for _ in members]
        elts = [elt for _, elt, _ in members]
        with pytest.raises(moai.hip.MoaiError, match="member 1: the key was trimmed to 1 levels") as err:
            e.ctx.apply_galois_ptrs(d_in, d_out, L, elts, [e.dkeys[0], trims[2], trims[1]])
        assert err.value.code == ERANGE
        for i in range(3):
            assert (d_out[i].to_numpy((2, L, e.n)) == fill).all(), i
            assert (d_in[i].to_numpy((2, L, e.n)) == members[i][0]).all(), i
        for fp in (False, True):
            set_fp(moai, fp)
            e.ctx.apply_galois_ptrs(d_in, d_out, L, elts, [e.dkeys[0], trims[0], trims[1]])
            for i in range(3):
                assert (d_out[i].to_numpy((2, L, e.n)) == want[i]).all(), (fp, i)
    finally:
        moai.hip.reset_tuning()
        for t in trims:
            e.ctx.key_forget(t)


def test_sums_and_in_place_members(moai, env12):
    """sums[i] null for some members and set for others, one output that is its sum, one that is its input: the results of
    moai_apply_galois_acc / moai_apply_galois_to called singly"""
    e, L, n = env12, 3, 4
    rng = np.random.default_rng(9)
    members = e.members(rng, L, n)
    addends = O.uniform_rns(rng, e.primes[:L], (n, 2), e.n)
    up = moai.DeviceBuffer.from_numpy
    # singly: 0 plain, 1 and 2 accumulated (acc = acc + galois(in)), 3 in place
    single = []
    for i, (ct, elt, ki) in enumerate(members):
        if i in (1, 2):
            acc = up(addends[i])
            e.ctx.apply_galois_acc(up(ct), acc, L, elt, e.dkeys[ki], 1)
            single.append(acc.to_numpy((2, L, e.n)))
        else:
            d = up(ct)
            e.ctx.apply_galois(d, L, elt, e.dkeys[ki], 1)
            single.append(d.to_numpy((2, L, e.n)))
    want = e.want(L, members)
    assert (single[0] == want[0]).all() and (single[3] == want[3]).all()
    assert (single[1] != want[1]).any()
    d_in = [up(ct) for ct, _, _ in members]
    d_sum = [None, up(addends[1]), up(addends[2]), None]
    d_out = [up(np.zeros((2, L, e.n), dtype=np.uint64)), up(np.zeros((2, L, e.n), dtype=np.uint64)), d_sum[2], d_in[3]]
    e.ctx.apply_galois_ptrs(d_in, d_out, L, [m[1] for m in members], [e.dkeys[m[2]] for m in members], d_sum)
    for i in range(n):
        assert (d_out[i].to_numpy((2, L, e.n)) == single[i]).all(), i
    assert (d_sum[1].to_numpy((2, L, e.n)) == addends[1]).all()  # a sum that is not the output is only read
    for i in range(3):
        assert (d_in[i].to_numpy((2, L, e.n)) == members[i][0]).all(), i


def test_seventy_members_take_two_passes(moai, env12):
    e, L, n = env12, 1, 70
    members = e.members(np.random.default_rng(70), L, n)
    want = e.want(L, members)
    got = run_ptrs(moai, e, L, members)
    for i in range(n):
        assert (got[i] == want[i]).all(), i


def test_split_digit_groups(moai, env12):
    """MOAI_KS_TMP_MB so small that the L + 1 output moduli go in more than one group and fewer than L + 1 (ks_group_size)"""
    e, L, n = env12, 3, 5
    per_modulus = n * L * e.n * 8
    mb = 1
    assert 1 < (mb << 20) // per_modulus < L + 1
    members = e.members(np.random.default_rng(33), L, n)
    want = e.want(L, members)
    try:
        for fp in (False, True):
            set_fp(moai, fp)
            moai.hip.set_tuning("MOAI_KS_TMP_MB", mb)
            got = run_ptrs(moai, e, L, members, in_place=(0, 4))
            for i in range(n):
                assert (got[i] == want[i]).all(), (fp, i)
    finally:
        moai.hip.reset_tuning()


def test_small_path_n2048(moai):
    e, L, n = Env(moai, 11), 2, 3
    members = e.members(np.random.default_rng(11), L, n)
    want = e.want(L, members)
    trim = e.ctx.key_trim(e.dkeys[1], L)
    try:
        got = run_ptrs(moai, e, L, members)
        for i in range(n):
            assert (got[i] == want[i]).all(), i
        # a trimmed key and a sum on this path too
        rng = np.random.default_rng(12)
        add = O.uniform_rns(rng, e.primes[:L], (2,), e.n)
        d_in = [moai.DeviceBuffer.from_numpy(ct) for ct, _, _ in members]
        d_sum = moai.DeviceBuffer.from_numpy(add)
        e.ctx.apply_galois_ptrs(d_in, [d_in[0], d_sum, d_in[2]], L, [m[1] for m in members], [e.dkeys[0], trim, e.dkeys[2]], [None, d_sum, None])
        q = np.array(e.primes[:L], dtype=np.uint64).reshape(1, L, 1)
        assert (d_in[0].to_numpy((2, L, e.n)) == want[0]).all() and (d_in[2].to_numpy((2, L, e.n)) == want[2]).all()
        assert (d_sum.to_numpy((2, L, e.n)) == (want[1] + add) % q).all()
    finally:
        e.ctx.key_forget(trim)


def test_n65536_once(moai):
    e, L, n = Env(moai, 16, [60, 51, 60], n_keys=2), 2, 2
    rng = np.random.default_rng(16)
    cts = O.uniform_rns(rng, e.primes[:L], (n, 2), e.n)
    members = [(cts[0], e.elts[0], 0), (cts[1], e.elts[2], 1)]
    want = e.want(L, members)
    try:
        set_fp(moai, True)
        H = moai.hip
        modes = [e.ctx.arith_mode(p, H.MODE_OF_KEY_SWITCH, L, n) for p in (0, 1, e.k - 1)]
        assert H.MODE_GUARD in modes and H.MODE_FPR in modes, modes
        got = run_ptrs(moai, e, L, members)
        for i in range(n):
            assert (got[i] == want[i]).all(), i
    finally:
        moai.hip.reset_tuning()


@pytest.mark.parametrize("n", [1, 4])
def test_relinearize_ptrs(moai, env12, n):
    e, L = env12, 3
    rng = np.random.default_rng(40 + n)
    ct3 = O.uniform_rns(rng, e.primes[:L], (n, 3), e.n)
    up = moai.DeviceBuffer.from_numpy
    want = [e.octx.relinearize(ct3[i], e.keys[0], L).reshape(2, L, e.n) for i in range(n)]
    try:
        for fp in (False, True):
            set_fp(moai, fp)
            single = []
            for i in range(n):
                d = moai.DeviceBuffer(2 * L * e.n)
                e.ctx.relinearize(up(ct3[i]), e.dkeys[0], d, L, 1)
                single.append(d.to_numpy((2, L, e.n)))
            d_in = [up(ct3[i]) for i in range(n)]
            d_out = [moai.DeviceBuffer(2 * L * e.n) for _ in range(n)]
            moai.hip.op_trace(True)
            e.ctx.relinearize_ptrs(d_in, d_out, e.dkeys[0], L)
            moai.hip.op_trace(False)
            assert moai.hip.op_trace_counts().get(("relinearize", L)) == n
            for i in range(n):
                got = d_out[i].to_numpy((2, L, e.n))
                assert (got == single[i]).all() and (got == want[i]).all(), (fp, i)
                assert (d_in[i].to_numpy((3, L, e.n)) == ct3[i]).all(), (fp, i)
    finally:
        moai.hip.op_trace(False)
        moai.hip.reset_tuning()


def test_refused_arguments_leave_the_outputs_untouched(moai, env12):
    e, L, n = env12, 2, 3
    members = e.members(np.random.default_rng(1), L, n)
    up = moai.DeviceBuffer.from_numpy
    fill = np.full((2, L, e.n), 7, dtype=np.uint64)
    d_in = [up(ct) for ct, _, _ in members]
    d_out = [up(fill) for _ in members]
    elts = [m[1] for m in members]
    keys = [e.dkeys[m[2]] for m in members]
    words = 2 * L * e.n
    cases = [
        (dict(elts=[elts[0], 2 * e.n + 1, elts[2]]), "member 1: Galois element is not valid"),
        (dict(outs=[d_out[0], d_out[0], d_out[2]]), "overlaps a block of member"),  # two members, one output
        (dict(outs=[d_out[0], d_in[2], d_out[2]]), "overlaps a block of member"),  # another member's input
        (dict(outs=[d_out[0].ptr, d_in[1].ptr + 8 * e.n, d_out[2].ptr]), "member 1: the output overlaps the input"),  # a part of its own
        (dict(sums=[None, d_out[2], None]), "overlaps a block of member"),  # member 1's sum is member 2's output
        (dict(sums=[d_in[0], None, None]), "member 0: the sum is the input"),
        (dict(L=e.k), "L exceeds"),
    ]
    for change, text in cases:
        a = dict(ins=d_in, outs=d_out, L=L, elts=elts, keys=keys, sums=None)
        a.update(change)
        with pytest.raises(moai.hip.MoaiError, match=text) as err:
            e.ctx.apply_galois_ptrs(a["ins"], a["outs"], a["L"], a["elts"], a["keys"], a["sums"])
        assert err.value.code == EINVAL, text
        for i in range(n):
            assert (d_out[i].to_numpy(words=words) == fill.reshape(-1)).all(), (text, i)
            assert (d_in[i].to_numpy(words=words) == members[i][0].reshape(-1)).all(), (text, i)
    # relinearize: the output may not be the input
    ct3 = up(O.uniform_rns(np.random.default_rng(2), e.primes[:L], (3,), e.n))
    with pytest.raises(moai.hip.MoaiError, match="member 0: the output overlaps the input") as err:
        e.ctx.relinearize_ptrs([ct3], [ct3], e.dkeys[0], L)
    assert err.value.code == EINVAL
