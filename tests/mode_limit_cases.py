"""The inputs and oracle results of the limit-prime tests (tests/mode_limits.py), shared by the tiled degrees
(tests/test_gpu_mode_limits.py) and the small ones (tests/test_gpu_small_degree_limits.py).  Every builder computes its case once
and keeps one degree (or chain) at a time; the test module that used them releases them with release() at its end."""
import numpy as np

import mode_limits as ML
import oracle as O

ORDER_NAMES = ["fpr_hi_last", "g61_last"]
K, L8 = 9, 8

_ctxs = {}
_long = {}
_ntt = {}
_ks = {}
_rs = {}
_hoist = {}


def release():
    """close the cached device contexts (nine-prime chains and the long chain) and drop every cached case"""
    for entry in _ctxs.values():
        entry[3].close()
    for entry in _long.values():
        entry["ctx"].close()
    for cache in (_ctxs, _long, _ntt, _ks, _rs, _hoist):
        cache.clear()


def contexts(moai, logn, order):
    """(primes, names, oracle context, device context) of a nine-prime chain, built once"""
    if (logn, order) not in _ctxs:
        primes = ML.ordered(logn, order)
        _ctxs[(logn, order)] = (primes, ML.ORDERS[order], O.Context(logn, primes), moai.Context(logn, primes))
    return _ctxs[(logn, order)]


def up(moai, a):
    return moai.DeviceBuffer.from_numpy(a)


# ---- the plain transforms ---------------------------------------------------------------------------------------------------
def ntt_case(logn):
    """inputs [pattern][2][9][N] under the chain g61_last and the oracle's transforms, computed once per degree"""
    if logn not in _ntt:
        _ntt.clear()
        n = 1 << logn
        primes = ML.ordered(logn, "g61_last")
        rng = np.random.default_rng(5200 + logn)
        x = np.stack([ML.pattern_rows(primes, n, rng), ML.pattern_rows(primes, n, rng)], axis=1)
        x[:, 1] = np.roll(x[:, 1], 1, axis=-1)  # the second polynomial: the patterns one coefficient on, other random data
        octx = O.Context(logn, primes)
        flat = x.reshape(-1, K, n)
        c = dict(x=x, fwd=octx.ntt(flat, K).reshape(x.shape), inv=octx.ntt(flat, K, inverse=True).reshape(x.shape))
        for v in c.values():
            v.setflags(write=False)
        _ntt[logn] = c
    return _ntt[logn]


# A row selection in which the classes interleave and row r is not prime r: what the launcher's partition of the rows by class
# has to get right (which rows, which primes, which tables per class) and the identity map of the tests above does not force.
# Under the defaults no two neighbouring rows share both their forward and their inverse class.
MIXED_ROWS = ("g60", "fpn_hi", "g61", "fpr_hi", "ng_hi", "small", "g_lo", "fpr_lo", "int_lo")

# ---- the key switch ---------------------------------------------------------------------------------------------------------
KS_INPUTS = ("key and digits all q-1", "digits q/2, q/2+1", "random")


def ks_case(moai, logn, order):
    """Per input of KS_INPUTS: key, targets [2][8][N] in NTT form whose digits carry the pattern, a random ciphertext to add to,
    and the oracle's switch_key, apply_galois and relinearize.  One (degree, order) is kept at a time."""
    if (logn, order) in _ks:
        return _ks[(logn, order)]
    _ks.clear()
    n = 1 << logn
    primes, names, octx, ctx = contexts(moai, logn, order)
    rng = np.random.default_rng(5300 + logn + (7 if order == "g61_last" else 0))
    key_max = np.empty((K - 1, 2, K, n), dtype=np.uint64)
    for i, q in enumerate(primes):
        key_max[:, :, i, :] = q - 1
    key_rnd = O.uniform_rns(rng, primes, (K - 1, 2), n)
    pat = ML.pattern_rows(primes[:L8], n, rng)
    coeff = [np.stack([pat[0], pat[2]]), np.stack([pat[3], np.roll(pat[3], 1, axis=-1)]), O.uniform_rns(rng, primes[:L8], (2,), n)]
    elt = O.galois_elt_from_step(logn, 1)
    table = O.galois_table_ntt(logn, elt)
    cases = []
    for name, key, cf in zip(KS_INPUTS, (key_max, key_rnd, key_rnd), coeff):
        tgt = octx.ntt(cf, L8)  # [2][8][N]
        ct = O.uniform_rns(rng, primes[:L8], (2, 2), n)
        # apply_galois switches the PERMUTED c1: place the target so that the permutation brings it back
        ctg = ct.copy()
        ctg[:, 1][..., table] = tgt
        ct3 = np.concatenate([ct, tgt[:, None]], axis=1)
        cases.append(dict(name=name, key=key, tgt=tgt, ct=ct, ctg=ctg, ct3=ct3,
                          sk=np.stack([octx.switch_key(ct[b], tgt[b], key, L8).reshape(2, L8, n) for b in range(2)]),
                          ag=np.stack([octx.apply_galois(ctg[b], L8, elt, key).reshape(2, L8, n) for b in range(2)]),
                          rl=np.stack([octx.relinearize(ct3[b], key, L8) for b in range(2)])))
    _ks[(logn, order)] = (elt, cases)
    return _ks[(logn, order)]


# ---- rescale and mod-down -----------------------------------------------------------------------------------------------------
def rescale_case(moai, logn):
    """Every level of both chain orders: ciphertext 0 has the dropped row's COEFFICIENTS on the rounding pattern and the kept rows
    all q-1, ciphertext 1 is random; the oracle's rescale of both.  Plus one scalar product + rescale with scalars q-1."""
    if logn not in _rs:
        _rs.clear()
        n = 1 << logn
        out = {}
        for order in ORDER_NAMES:
            primes, names, octx, _ = contexts(moai, logn, order)
            rng = np.random.default_rng(5400 + logn)
            for L in range(K, 1, -1):
                x = O.uniform_rns(rng, primes[:L], (2, 2), n)
                x[0, :, L - 1, :] = octx.ntt(ML.rounding_row(primes[L - 1], n), 1, prime_index=[L - 1]).reshape(n)
                for i in range(L - 1):
                    x[0, :, i, :] = primes[i] - 1
                out[(order, L)] = (x, np.stack([octx.rescale(x[b], 2, L) for b in range(2)]))
        primes, names, octx, _ = contexts(moai, logn, "g61_last")
        x = out[("g61_last", K)][0]
        plain = np.stack([np.full(n, q - 1, dtype=np.uint64) for q in primes])
        out["scalar"] = np.stack([octx.rescale(octx.multiply_plain(x[b], 2, K, plain), 2, K) for b in range(2)])
        _rs[logn] = out
    return _rs[logn]


# ---- hoisted rotations -----------------------------------------------------------------------------------------------------
# steps 1, -2, the conjugation (0) and 3: the pass over four rotations at once (MOAI_KS_HOIST_PAIR=4, ks_hoisted_mac2<4>) runs only
# while four rotations are left, so with four the settings 4, 2 and 0 cover ks_hoisted_mac2<4>, <2> and ks_hoisted_mac
HOIST_STEPS = [1, -2, 0, 3]


def hoist_case(moai, logn):
    if logn not in _hoist:
        _hoist.clear()
        n = 1 << logn
        primes, names, octx, ctx = contexts(moai, logn, "g61_last")
        rng = np.random.default_rng(5500 + logn)
        elts = [O.galois_elt_from_step(logn, s) if s else 2 * n - 1 for s in HOIST_STEPS]
        keys = [O.uniform_rns(rng, primes, (K - 1, 2), n) for _ in HOIST_STEPS]
        for i, q in enumerate(primes):
            keys[0][:, :, i, :] = q - 1
        ct = O.uniform_rns(rng, primes[:L8], (2, 2), n)
        pat = ML.pattern_rows(primes[:L8], n, rng)
        ct[0, 1] = octx.ntt(pat[0], L8)  # INTT(c1) all q-1: no zero coefficient, every digit at its largest
        ref = np.stack([np.stack([octx.apply_galois(ct[b], L8, e, kk).reshape(2, L8, n) for b in range(2)]) for e, kk in zip(elts, keys)])
        _hoist[logn] = (elts, keys, ct, ref)
    return _hoist[logn]


# ---- long chains: where the accumulation bounds bind ----------------------------------------------------------------------
def long_case(moai, logn, k):
    """the chain of k primes, its contexts, an all q-1 and a random key; one chain is kept at a time"""
    if (logn, k) not in _long:
        for v in _long.values():
            v["ctx"].close()
        _long.clear()
        n = 1 << logn
        primes, names = ML.long_chain(logn, k)
        rng = np.random.default_rng(5600 + logn)
        key_max = np.empty((k - 1, 2, k, n), dtype=np.uint64)
        key_rnd = O.uniform_rns(rng, primes, (k - 1, 2), n)
        _long[(logn, k)] = dict(primes=primes, names=names, octx=O.Context(logn, primes), ctx=moai.Context(logn, primes), rng=rng,
                                keys=(key_max, key_rnd), drawn={i: key_rnd[:, :, i, :].copy() for i, q in enumerate(primes) if q >> 60},
                                refs={})
    return _long[(logn, k)]


def long_refs(c, L):
    """per key: ciphertext, target (digits all q-1 for the all q-1 key, random for the random one) and the oracle's switch_key.
    The key rows are all q-1 (or uniform below q) up to what the reference's own 128-bit sum admits at this L
    (ML.reference_key_cap: the 61-bit prime's rows are capped on these chains, nothing else)."""
    primes, octx, rng = c["primes"], c["octx"], c["rng"]
    key_max, key_rnd = c["keys"]
    for i, q in enumerate(primes):
        cap = ML.reference_key_cap(q, L)
        key_max[:, :, i, :] = cap
        if i in c["drawn"]:
            key_rnd[:, :, i, :] = c["drawn"][i] % np.uint64(cap + 1)
    if L not in c["refs"]:
        n = octx.n
        full = np.stack([np.full(n, q - 1, dtype=np.uint64) for q in primes[:L]])
        out = []
        for key, coeff in zip(c["keys"], (full, O.uniform_rns(rng, primes[:L], (), n))):
            tgt = octx.ntt(coeff[None], L)[0]
            ct = O.uniform_rns(rng, primes[:L], (2,), n)
            out.append((ct, tgt, octx.switch_key(ct, tgt, key, L).reshape(2, L, n)))
        c["refs"][L] = out
    return c["refs"][L]
