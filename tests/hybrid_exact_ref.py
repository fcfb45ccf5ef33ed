"""MOAI_HYBRID_ROUND_EXACT (include/moai_hip.h, "hybrid rounding mode") restated: the mod-down's base conversion in Python integers
plus numpy float64 for the overflow estimate -- uint64 -> float64 (round to nearest even), one `*` by r_m = 1.0 / float(m) and one `+`
per source, in source order -- and, on top of it and of the other restatements as they are,
    mod_down             hybrid_hoist_ref.mod_down's signature; `patched()` puts it in that module's place, so that
                         hybrid_hoist_ref.apply_galois_hoisted, hybrid_dot_ref.rotate_pt_dot and hybrid_bsgs_ref.bsgs_dot restate the mode
    switch_key / relinearize / apply_galois     hybrid_dot_ref.accumulators + that mod-down
    relinearize_rescale / multiply_relin_rescale     hybrid_rescale_ref.lifted + the conversion with S = {q_{L-1}, p_t}
and what the checks need that contains NO floating point: the lifted accumulator as an integer (lifted_integer), the exact rational
out - Z / W (quotient_error, integers scaled by W), floor((Z + H) / W) (rounded_quotient) and the coefficients inside the 2^-40 band
(guard_band).  tests/test_hybrid_exact_cpu.py pins this module; tests/test_gpu_hybrid_exact.py compares the device with it bit for
bit.  CPU only."""
import contextlib

import numpy as np

import hybrid_dot_ref as HD
import hybrid_hoist_ref as HH
import hybrid_ref as HR
import hybrid_rescale_ref as RR
import oracle as O

EPS_BITS = 40  # the header's promise: |f - sum y_m / m| <= 2^-40


def bases(octx, L, alpha, rescale=False):
    """(source primes S as context prime indices in the order of the accumulator's rows, the number of target primes q_0 ..): step 5
    of a switch, or the merged mod-down of relinearize + rescale"""
    sp = HR.special_rows(octx.k, alpha)
    return ([L - 1] + sp, L - 1) if rescale else (sp, L)


def source_rows(L, alpha, rescale=False):
    """the rows of an accumulator [L + alpha][N] that hold the sources"""
    return list(range(L - 1 if rescale else L, L + alpha))


def convert(octx, x, src, ntgt, exact=True, diag=None):
    """conv [ntgt][N] (coefficient form, canonical) for the source residues x [len(src)][N] (coefficient form, canonical) under the
    context primes src: the contract of the header.  exact=False is the fast form.  diag: a dict that receives y, v (zeros in the
    fast form), v* and X' of this call as object arrays [N]"""
    primes = octx.primes
    n = len(src)
    W = HR._prod(primes[r] for r in src)
    H = W // 2
    y = []
    for t, r in enumerate(src):
        m = primes[r]
        y.append((((HR._obj(x[t]) + H % m) % m) * pow((W // m) % m, -1, m)) % m)
    v = np.zeros(len(y[0]), dtype=object)
    if exact:
        f = np.zeros(len(y[0]), dtype=np.float64)
        for t, r in enumerate(src):
            r_m = np.float64(1.0) / np.float64(float(primes[r]))  # two roundings: the conversion, then the division
            f = f + HR._u64(y[t]).astype(np.float64) * r_m       # one rounded product, one rounded sum
        v = np.minimum(np.maximum(np.floor(f), 0.0), float(n - 1)).astype(np.int64).astype(object)
    if diag is not None:
        total = sum(y[t] * (W // primes[r]) for t, r in enumerate(src))
        diag.update(y=y, v=v, vstar=total // W, X=total % W, W=W)
    conv = np.empty((ntgt, len(y[0])), dtype=np.uint64)
    for i in range(ntgt):
        q = primes[i]
        conv[i] = HR._u64((sum(y[t] * ((W // primes[r]) % q) for t, r in enumerate(src)) - v * (W % q) - H % q) % q)
    return conv


def mod_down_rows(octx, Z, L, alpha, rescale=False, exact=True, diag=None):
    """one polynomial through a mod-down: Z [L + alpha][N] (NTT form, canonical, rows 0 .. L-1 then the special rows) ->
    (Z_i - NTT(conv_i)) [W^-1]_{q_i} mod q_i, [ntgt][N]"""
    primes = octx.primes
    src, ntgt = bases(octx, L, alpha, rescale)
    W = HR._prod(primes[r] for r in src)
    rows = [HR._u64(Z[r]) for r in source_rows(L, alpha, rescale)]
    x = octx.ntt(np.stack(rows), len(src), prime_index=src, inverse=True)
    conv = octx.ntt(convert(octx, x, src, ntgt, exact, diag), ntgt)
    out = np.empty((ntgt, octx.n), dtype=np.uint64)
    for i in range(ntgt):
        q = primes[i]
        out[i] = HR._u64(((HR._obj(Z[i]) - HR._obj(conv[i])) * pow(W % q, -1, q)) % q)
    return out


def acc_rows(octx, acc, p, L, alpha):
    """polynomial p of an accumulator dict (p, context prime) -> [N] as rows [L + alpha][N]"""
    return np.stack([HR._u64(acc[p, row]) for row in HH.rows_of(octx, L, alpha)])


def mod_down(octx, acc, addend, L, alpha, exact=True):
    """hybrid_hoist_ref.mod_down in the exact mode: acc dict (p, context prime) -> [N] canonical, addend [2][L][N]; [2][L][N]"""
    out = np.empty((2, L, octx.n), dtype=np.uint64)
    for p in range(2):
        d = mod_down_rows(octx, acc_rows(octx, acc, p, L, alpha), L, alpha, exact=exact)
        for i in range(L):
            out[p, i] = HR._u64((HR._obj(addend[p][i]) + HR._obj(d[i])) % octx.primes[i])
    return out


@contextlib.contextmanager
def patched():
    """inside the block hybrid_hoist_ref.mod_down is the exact one: apply_galois_hoisted, hybrid_dot_ref.rotate_pt_dot and
    hybrid_bsgs_ref.bsgs_dot, which all take their step 5 from that module, restate the exact mode as they are"""
    plain = HH.mod_down
    HH.mod_down = mod_down
    try:
        yield
    finally:
        HH.mod_down = plain


def switch_key(octx, ct, target, key, L, alpha, exact=True):
    """hybrid_ref.switch_key with the exact step 5"""
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, octx.n)
    return mod_down(octx, HD.accumulators(octx, target, key, L, alpha), ct, L, alpha, exact)


def relinearize(octx, ct3, key, L, alpha):
    ct3 = np.asarray(ct3, dtype=np.uint64).reshape(3, L, octx.n)
    return switch_key(octx, ct3[:2], ct3[2], key, L, alpha)


def apply_galois(octx, ct, L, elt, key, alpha):
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, octx.n)
    perm = ct[:, :, O.galois_table_ntt(octx.logn, elt)]
    return switch_key(octx, np.stack([perm[0], np.zeros_like(perm[0])]), perm[1], key, L, alpha)


def relinearize_rescale(octx, ct3, key, L, alpha, exact=True, Z=None):
    """hybrid_rescale_ref.relinearize_rescale with the exact merged mod-down; Z: hybrid_rescale_ref.lifted's result where the caller
    has it already"""
    assert L >= 2
    Z = RR.lifted(octx, ct3, key, L, alpha) if Z is None else Z
    return np.stack([mod_down_rows(octx, Z[p], L, alpha, rescale=True, exact=exact) for p in range(2)])


def multiply_relin_rescale(octx, x, y, key, L, alpha):
    return relinearize_rescale(octx, RR.ct_product(octx, x, y, L), key, L, alpha)


# ---- the checks' side: integers and rationals only ----------------------------------------------------------------------------------
def lifted_integer(octx, Z, L, alpha):
    """Z [L + alpha][N] (NTT form) as integers [N] in [0, Q_L P): exact CRT"""
    return RR.crt(octx, [HR._u64(r) for r in Z], HH.rows_of(octx, L, alpha))


def _moduli(octx, L, alpha, rescale):
    src, ntgt = bases(octx, L, alpha, rescale)
    return HR._prod(octx.primes[r] for r in src), HR._prod(octx.primes[:ntgt]), ntgt


def quotient_error(octx, Z, out, L, alpha, rescale=False):
    """(e, W): e [N] integers with e / W = out - Z / W exactly, per coefficient; Z [L + alpha][N] the lifted accumulator (NTT form), out
    [ntgt][N] what the mod-down returned for it (NTT form, no addend).  out is an integer modulo Q' = Q_L P / W, so e is the centred
    residue of out W - Z modulo Q' W"""
    W, Qlo, ntgt = _moduli(octx, L, alpha, rescale)
    z = lifted_integer(octx, Z, L, alpha)
    o = RR.crt(octx, list(out), range(ntgt))
    return RR.centred((o * W - z) % (Qlo * W), Qlo * W), W


def within_half(e, W, eps_bits=EPS_BITS):
    """|e / W| <= 1/2 + 2^-eps_bits per coefficient, in integers"""
    return np.array([2 * abs(int(v)) << eps_bits <= W * ((1 << eps_bits) + 2) for v in e])


def rounded_quotient(octx, Z, L, alpha, rescale=False):
    """floor((Z + H) / W) mod Q' as rows [ntgt][N] in NTT form: big integers alone"""
    W, Qlo, ntgt = _moduli(octx, L, alpha, rescale)
    z = lifted_integer(octx, Z, L, alpha)
    r = ((z + W // 2) // W) % Qlo
    rows = np.stack([HR._u64(r % octx.primes[i]) for i in range(ntgt)])
    return octx.ntt(rows, ntgt)


def guard_band(octx, Z, L, alpha, rescale=False, eps_bits=EPS_BITS):
    """the coefficients (indices) whose X' / W, X' = ((Z mod W) + H) mod W, lies in [0, 2^-eps_bits) or (1 - 2^-eps_bits, 1)"""
    W, _, _ = _moduli(octx, L, alpha, rescale)
    z = lifted_integer(octx, Z, L, alpha)
    X = (z % W + W // 2) % W
    return [i for i, x in enumerate(X) if (int(x) << eps_bits) < W or ((W - int(x)) << eps_bits) < W]


def switch_noise_bound(octx, L, alpha, s_l1):
    """hybrid_ref.noise_bound in the exact mode"""
    return HR.approx_u(octx, L, alpha) + (0.5 + 2.0 ** -EPS_BITS) * (1 + s_l1)


def dot_noise_bound(octx, L, alpha, s_l1, plain_l1_sum):
    """hybrid_dot_ref.noise_bound in the exact mode"""
    return HR.approx_u(octx, L, alpha, times=plain_l1_sum) + (0.5 + 2.0 ** -EPS_BITS) * (1 + s_l1)


def bsgs_noise_bound(octx, L, alpha, s_l1, giant_elts, plain_l1_sums):
    """hybrid_bsgs_ref.noise_bound in the exact mode"""
    u, r = HR.approx_u(octx, L, alpha), 0.5 + 2.0 ** -EPS_BITS
    return r * (1 + s_l1) + sum(l1 * u + ((u + r * s_l1) if E != 1 else 0) for E, l1 in zip(giant_elts, plain_l1_sums))


def rescale_noise_bound(octx, L, alpha, s_l1):
    """hybrid_rescale_ref.noise_bound in the exact mode"""
    return HR.approx_u(octx, L, alpha) + octx.primes[L - 1] * (0.5 + 2.0 ** -EPS_BITS) * (1 + s_l1)
