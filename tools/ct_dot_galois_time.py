#!/usr/bin/env python3
"""Q.K^T of one head two ways in one process, alternating, at MOAI's shape (N = 2^16, 64 operand pairs, 127 outputs with the
elements 5^(256 i), chain index 14: 15 data primes and the special prime):
  conventional  moai_apply_galois_hoisted per operand W[j] (127 rotations, one digit decomposition), then moai_ct_dot per output
  deferred      one moai_ct_dot_galois, then one moai_galois_fold (two key switches per output)
The operands are noise-free encryptions of messages below 2^10 under a ternary secret and the keys are real Galois keys, so
before anything is timed three outputs of either order are decrypted under (1, s, s^2) on the device, the exact product
sum_j m_X[j] pi(m_W[j]) is subtracted, and the centred error (the same integer in every row) is held against its bound: with E
the bound of one moai_switch_key (include/moai_hip.h, the alpha = 1 case of the hybrid formula), E (1 + |s|_1) deferred and
sum_j |m_X[j]|_1 E conventional.
With --sums only moai_ct_dot_galois is timed, on uniform residues and without keys: the integer forms against the Gram form on the
int8 matrix cores (MOAI_CTDOT_GALOIS_MFMA), for 8 to 127 outputs (sums_only below)."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
import bench

m = g.load_package()
LOGN, N, TERMS, N_OUT, L, REPS, CALLS = 16, 65536, 64, 127, 15, 5, 8  # CALLS: per timed window of the short calls
KEY = bytes(range(32))


def primes_of(bits):
    out, seen = [], set()
    for b in bits:
        v = ((1 << b) - 1) // (2 * N) * (2 * N) + 1
        while v in seen or not bench.is_prime(v):
            v -= 2 * N
        seen.add(v)
        out.append(v)
    return out


dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
print("device: %s, %d CUs" % m.hip.device_info()[:2])
primes = primes_of([51] + [46] * (L - 1) + [58])
k, ctx = L + 1, m.Context(LOGN, primes)
elts = [pow(5, 256 * i, 2 * N) for i in range(1, N_OUT + 1)]
gen = torch.Generator(device=dev).manual_seed(11)
q = torch.tensor(primes[:L], dtype=torch.int64, device=dev).view(L, 1)


def sums_only():
    """--sums: moai_ct_dot_galois alone on uniform residues, the integer forms (MOAI_CTDOT_GALOIS_MFMA=0) against the Gram form on
    the int8 matrix cores (=1), alternating in one process after a warm-up call of each whose outputs must be equal words; the
    first n_out of the 127 elements, to find the number of outputs from which the Gram form wins"""
    knob, e0, e1 = "MOAI_CTDOT_GALOIS_MFMA", m.hip.Event(), m.hip.Event()
    x, w = (torch.stack([torch.randint(0, p, (TERMS, 2, N), dtype=torch.int64, device=dev, generator=gen) for p in primes[:L]], dim=2).contiguous()
            for _ in range(2))
    print("\nmoai_ct_dot_galois alone, N = %d, terms = %d, %d data primes (51 + 14 x 46 bits); ms per call, median of %d windows of %d calls "
          "(spread = (max - min) / median)" % (N, TERMS, L, REPS, CALLS))
    print("%6s  %-22s %-22s %s" % ("n_out", "integer forms (knob 0)", "Gram form (knob 1)", "integer / Gram"))
    for n_out in (8, 16, 32, 64, 96, 127):
        out = [torch.empty((n_out, 4, L, N), dtype=torch.int64, device=dev) for _ in range(2)]
        for v in (0, 1):
            m.hip.set_tuning(knob, v)
            assert ctx.ct_dot_galois_forms(elts[:n_out], TERMS, L) == ([0, 0, n_out] if v else [0, n_out, 0])
            ctx.ct_dot_galois(x.data_ptr(), w.data_ptr(), out[v].data_ptr(), elts[:n_out], TERMS, L, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1]), "the two forms differ at n_out = %d" % n_out
        t = ([], [])
        for _ in range(REPS):
            for v in (0, 1):
                m.hip.set_tuning(knob, v)
                e0.record(st)
                for _ in range(CALLS):
                    ctx.ct_dot_galois(x.data_ptr(), w.data_ptr(), out[v].data_ptr(), elts[:n_out], TERMS, L, stream=st)
                e1.record(st)
                torch.cuda.synchronize()
                t[v].append(e1.elapsed_ms_since(e0) / CALLS)
        med = [statistics.median(tv) for tv in t]
        print("%6d  %-22s %-22s %.2f" % ((n_out,) + tuple("%.2f (%.1f %%)" % (md, 100 * (max(tv) - min(tv)) / md) for md, tv in zip(med, t)) + (med[0] / med[1],)))
    m.hip.reset_tuning()
    ctx.close()


if "--sums" in sys.argv[1:]:
    sums_only()
    sys.exit(0)

# the secret, one Galois key and one hoisting correction per element
sk = ctx.sample_ternary(KEY, 3 << 40, 1, k)
s_l1 = int((sk.to_numpy((k, N))[0] != 0).sum())
ctx.ntt_forward(sk, 1, k)
new = m.DeviceBuffer(k * N)
keys, corrs = [], []
for i, e in enumerate(elts):
    ctx.galois_permute(sk, new, 1, k, e)
    keys.append(ctx.kswitch_keygen(KEY, 1000 + 100 * i, sk, new))
    corrs.append(ctx.hoist_correction(keys[-1], e, L))


def encrypt():
    """(messages in NTT form [TERMS][L][N], |m|_1 per message, ciphertexts [TERMS][2][L][N] with c0 + c1 s = m exactly)"""
    msg = torch.randint(0, 1024, (TERMS, 1, N), dtype=torch.int64, device=dev, generator=gen)
    m_ntt = msg.expand(TERMS, L, N).contiguous()
    ctx.ntt_forward(m_ntt.data_ptr(), TERMS, L, stream=st)
    c1 = torch.stack([torch.randint(0, p, (TERMS, N), dtype=torch.int64, device=dev, generator=gen) for p in primes[:L]], dim=1).contiguous()
    c0 = torch.empty_like(c1)
    ctx.dyadic_mul(c1.data_ptr(), sk, c0.data_ptr(), TERMS, 1, L, stream=st)
    ctx.sub(m_ntt.data_ptr(), c0.data_ptr(), c0.data_ptr(), TERMS, L, stream=st)
    return m_ntt, msg.sum(dim=(1, 2)), torch.stack([c0, c1], dim=1).contiguous()


mx_ntt, mx_l1, x = encrypt()
mw_ntt, _, w = encrypt()
rot = torch.empty((N_OUT, TERMS, 2, L, N), dtype=torch.int64, device=dev)  # rot[i][j] = rotate(W[j], step i)
conv = torch.empty((N_OUT, 3, L, N), dtype=torch.int64, device=dev)
acc = torch.empty((N_OUT, 4, L, N), dtype=torch.int64, device=dev)
defer = torch.empty((N_OUT, 3, L, N), dtype=torch.int64, device=dev)


def conventional():
    fell_back = False
    for j in range(TERMS):
        fell_back |= ctx.apply_galois_hoisted(w[j].data_ptr(), [rot[i, j].data_ptr() for i in range(N_OUT)], L, elts, keys, corrs, 1, stream=st)
    for i in range(N_OUT):
        ctx.ct_dot(x.data_ptr(), rot[i].data_ptr(), conv[i].data_ptr(), TERMS, L, stream=st)
    return fell_back


def deferred():
    ctx.ct_dot_galois(x.data_ptr(), w.data_ptr(), acc.data_ptr(), elts, TERMS, L, stream=st)
    ctx.galois_fold(acc.data_ptr(), keys, defer.data_ptr(), L, stream=st)


def error(ct3, i):
    """max |c0 + c1 s + c2 s^2 - sum_j m_X[j] pi_i(m_W[j])| as an integer, from rows that all hold it"""
    t, d, pw = torch.empty((L, N), dtype=torch.int64, device=dev), torch.empty((L, N), dtype=torch.int64, device=dev), torch.empty_like(mw_ntt)
    ctx.dyadic_mul(ct3[2].data_ptr(), sk, t.data_ptr(), 1, 1, L, stream=st)
    ctx.add(ct3[1].data_ptr(), t.data_ptr(), t.data_ptr(), 1, L, stream=st)
    ctx.dyadic_mul(t.data_ptr(), sk, t.data_ptr(), 1, 1, L, stream=st)
    ctx.add(ct3[0].data_ptr(), t.data_ptr(), d.data_ptr(), 1, L, stream=st)
    ctx.galois_permute(mw_ntt.data_ptr(), pw.data_ptr(), TERMS, L, elts[i], stream=st)
    ctx.dyadic_mul(mx_ntt.data_ptr(), pw.data_ptr(), pw.data_ptr(), TERMS, TERMS, L, stream=st)
    torch.cuda.synchronize()
    diff = ((d - pw.sum(dim=0) % q) % q).contiguous()  # 64 residues below 2^51 sum below 2^57
    ctx.ntt_inverse(diff.data_ptr(), 1, L, stream=st)
    torch.cuda.synchronize()
    c = torch.where(diff > q // 2, diff - q, diff)
    assert bool((c == c[:1]).all()), "the rows do not hold one integer"
    return int(c[0].abs().max())


fell_back = conventional()
deferred()
torch.cuda.synchronize()
E = L * N * 21 * max(primes[:L]) / primes[-1] + 0.5 * (1 + s_l1)
bounds = {"conventional": E * int(mx_l1.sum()), "deferred": E * (1 + s_l1)}
worst = {name: max(error(out[i], i) for i in (0, N_OUT // 2, N_OUT - 1)) for name, out in (("conventional", conv), ("deferred", defer))}
print("\nN = %d, terms = %d, n_out = %d, %d data primes (51 + 14 x 46 bits) + a 58-bit special prime; hoisted fell back: %s" % (N, TERMS, N_OUT, L, fell_back))
print("decrypted under (1, s, s^2), outputs 0, %d, %d, |s|_1 = %d, E = %.0f:" % (N_OUT // 2, N_OUT - 1, s_l1, E))
for name in bounds:
    print("  %-13s max |error| %d, bound %.3g" % (name, worst[name], bounds[name]))
    assert 0 < worst[name] <= bounds[name]
parts = {"conventional": conventional, "deferred": deferred, "  moai_ct_dot_galois alone": lambda: ctx.ct_dot_galois(x.data_ptr(), w.data_ptr(), acc.data_ptr(), elts, TERMS, L, stream=st),
         "  moai_galois_fold alone": lambda: ctx.galois_fold(acc.data_ptr(), keys, defer.data_ptr(), L, stream=st)}
times = {name: [] for name in parts}
e0, e1 = m.hip.Event(), m.hip.Event()
for rep in range(REPS):
    for name, call in parts.items():
        calls = 1 if name == "conventional" else CALLS
        e0.record(st)
        for _ in range(calls):
            call()
        e1.record(st)
        torch.cuda.synchronize()
        times[name].append(e1.elapsed_ms_since(e0) / calls)
print("times per call, ms (%d repetitions, alternating, after the warm-up calls above; windows of one conventional or %d other calls):" % (REPS, CALLS))
for name, t in times.items():
    med = statistics.median(t)
    print("  %-27s %s  median %.1f, spread %.1f %%" % (name, " ".join("%.1f" % v for v in t), med, 100 * (max(t) - min(t)) / med))
print("  conventional / deferred: %.2fx;  key switches: %d against %d;  Galois keys: %d x %.0f MiB" % (
    statistics.median(times["conventional"]) / statistics.median(times["deferred"]), N_OUT * TERMS, 2 * N_OUT, N_OUT, (k - 1) * 2 * k * N * 8 / 2 ** 20))
ctx.close()
