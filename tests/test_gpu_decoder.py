"""GPU parity of the client's output path: moai_decrypt against c0 + c1 s (+ c2 s^2) in Python integers, and
moai_ckks_decode against the comparator tests/seal_decode.py (CKKSEncoder::decode_internal, SEAL/ckks.h:644-761, from
pieces pinned by the reference's KATs; tests/test_oracle_decoder.py pins the comparator).  Decoded values are compared
bit for bit (.view(np.uint64)); where the reference's conversion overflows, the non-finite positions must agree (NaN
payload and sign are not compared: x86-64 and gfx950 default NaNs differ).  The last test drives the seal:: shim end to
end (keygen -> encrypt -> Decryptor::decrypt -> CKKSEncoder::decode, and moai_fused::decrypt_decode)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
import seal_decode as SD
from ckks_toy import ToyClient

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")
MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same(got, want):
    """bit-identical where the comparator is finite; non-finite exactly where it is non-finite"""
    got = np.ascontiguousarray(got).view(np.float64).ravel()
    want = np.ascontiguousarray(want).view(np.float64).ravel()
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all(), "non-finite positions differ"
    # infinities carry their sign; only NaNs are compared by position alone
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all()
    mism = np.nonzero(_bits(got[fin]) != _bits(want[fin]))[0]
    assert mism.size == 0, "%d of %d values differ, first at %d: %r vs %r" % (
        mism.size, fin.sum(), mism[0], got[fin][mism[0]], want[fin][mism[0]])


def _setup(logn, bits):
    primes = O.coeff_modulus_create(1 << logn, bits)
    return primes, O.Context(logn, primes), O.CkksEncoder(O.Context(logn, primes))


@pytest.mark.parametrize("logn,bits", [
    (3, [40, 40]), (6, [40, 40, 40, 40]), (7, [60, 60, 60]), (10, [51, 46, 58]), (12, [51, 46, 46, 58]),
    (13, [60, 40, 60]), (14, [46, 51]), (15, [51, 46, 46, 51]), (16, [51, 46, 46, 46, 51, 58]),
])
def test_decode_matches_comparator(moai, logn, bits):
    n = 1 << logn
    primes, octx, enc = _setup(logn, bits)
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(logn)
    L = len(primes)
    slots = n // 2
    vals = np.stack([rng.normal(size=slots) + 1j * rng.normal(size=slots),
                     rng.uniform(-100, 100, size=slots) + 0j])
    scale = 2.0**30
    plain = np.stack([enc.encode(v, L, scale) for v in vals])
    rand = O.uniform_rns(rng, primes, (1,), n)  # uniformly random residues: every conversion branch
    plain = np.concatenate([plain, rand])
    d = moai.DeviceBuffer.from_numpy(plain)
    for is_complex in (False, True):
        got = ctx.ckks_decode(d, L, scale, n_batch=3, is_complex=is_complex)
        for b in range(3):
            assert_same(got[b], SD.decode(octx, enc, plain[b], L, scale, is_complex=is_complex))
    # the input is not modified (the reference decodes a copy)
    assert (d.to_numpy(plain.shape) == plain).all()


@pytest.mark.parametrize("L", [1, 3, 21, 36])
def test_decode_moai_chain(moai, L):
    logn = 16
    n = 1 << logn
    primes, octx, enc = _setup(logn, MOAI_BITS)
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(100 + L)
    slots = n // 2
    # encoded vectors at different scales in one batch, real and complex output
    scales = [2.0**46, 2.0**40 * 1.5]
    vals = [rng.normal(size=slots), rng.uniform(-4, 4, size=slots) + 1j * rng.uniform(-4, 4, size=slots)]
    plain = np.stack([enc.encode(v, L, s) for v, s in zip(vals, scales)])
    d = moai.DeviceBuffer.from_numpy(plain)
    got_r = ctx.ckks_decode(d, L, scales, n_batch=2)
    got_c = ctx.ckks_decode(d, L, scales, n_batch=2, is_complex=True)
    for b in range(2):
        want = SD.decode(octx, enc, plain[b], L, scales[b], is_complex=True)
        assert np.isfinite(want).all()
        assert_same(got_c[b], want)
        assert_same(got_r[b], np.ascontiguousarray(want.real))  # from_complex<double>: the real part of the same value
    # a prime_index subset (rows over other primes than 0..L-1, in another order)
    pidx = list(range(len(primes)))[::-1][:L] if L > 1 else [5]
    sub = enc.encode(vals[0], L, 2.0**40, prime_index=pidx)
    got = ctx.ckks_decode(moai.DeviceBuffer.from_numpy(sub), L, 2.0**40, prime_index=pidx)
    assert_same(got[0], SD.decode(octx, enc, sub, L, 2.0**40, prime_index=pidx))
    # uniformly random residues: every converted value stays finite up to 16 primes; at 36 the reference overflows
    rand = O.uniform_rns(rng, primes[:L], (), n)
    got = ctx.ckks_decode(moai.DeviceBuffer.from_numpy(rand), L, 2.0**46, is_complex=True)
    want = SD.decode(octx, enc, rand, L, 2.0**46, is_complex=True)
    if L <= 16:
        assert np.isfinite(want).all()
    assert_same(got[0], want)


def test_decode_encrypted_then_decrypted(moai):
    logn = 12
    n = 1 << logn
    bits = [51, 46, 46, 46, 58]
    primes, octx, enc = _setup(logn, bits)
    ctx = moai.Context(logn, primes)
    toy = ToyClient(octx, seed=3)
    L = 4
    rng = np.random.default_rng(5)
    z = rng.normal(size=n // 2)
    plain = enc.encode(z, L, 2.0**40)
    ct = toy.encrypt_zero_symmetric(L)
    ct[0] = (ct[0] + plain) % np.array(primes[:L], dtype=np.uint64)[:, None]
    dct = moai.DeviceBuffer.from_numpy(ct)
    dsk = moai.DeviceBuffer.from_numpy(toy.s_ntt)
    dec = ctx.decrypt(dct, 2, dsk, L)
    got = ctx.ckks_decode(dec, L, 2.0**40)
    want = SD.decode(octx, enc, dec.to_numpy((L, n)), L, 2.0**40)
    assert_same(got[0], want)
    assert np.max(np.abs(got[0] - z)) < 1e-6


def _decrypt_ints(ct, s_ntt, primes, idx):
    """c0 + c1 s + c2 s^2 ... mod q in Python integers; ct [size][L][N], s_ntt [k][N] (rows by prime index)"""
    size, L, n = ct.shape
    out = np.empty((L, n), dtype=np.uint64)
    for r, i in enumerate(idx):
        q = int(primes[i])
        s = s_ntt[i].astype(object)
        acc = ct[0, r].astype(object)
        sp = s
        for p in range(1, size):
            acc = (acc + ct[p, r].astype(object) * sp) % q
            sp = (sp * s) % q
        out[r] = acc.astype(np.uint64)
    return out


@pytest.mark.parametrize("size", [2, 3])
def test_decrypt_matches_integers(moai, size):
    logn = 12
    n = 1 << logn
    bits = [51, 46, 46, 46, 58]
    primes, octx, _ = _setup(logn, bits)
    ctx = moai.Context(logn, primes)
    toy = ToyClient(octx, seed=9)
    rng = np.random.default_rng(size)
    dsk_full = moai.DeviceBuffer.from_numpy(toy.s_ntt)
    # batch of 3 at L = 4, rows 0..3
    L, B = 4, 3
    ct = O.uniform_rns(rng, primes[:L], (B, size), n)
    got = ctx.decrypt(moai.DeviceBuffer.from_numpy(ct), size, dsk_full, L, n_batch=B).to_numpy((B, L, n))
    for b in range(B):
        assert (got[b] == _decrypt_ints(ct[b], toy.s_ntt, primes, range(L))).all()
    # a prime_index subset: the key's rows follow prime_index like the ciphertext's
    pidx = [4, 2, 0]
    ct = O.uniform_rns(rng, [primes[i] for i in pidx], (2, size), n)
    sk_sub = moai.DeviceBuffer.from_numpy(np.ascontiguousarray(toy.s_ntt[pidx]))
    got = ctx.decrypt(moai.DeviceBuffer.from_numpy(ct), size, sk_sub, 3, n_batch=2, prime_index=pidx).to_numpy((2, 3, n))
    for b in range(2):
        assert (got[b] == _decrypt_ints(ct[b], toy.s_ntt, primes, pidx)).all()


def test_decode_in_chunks(moai):
    # a scratch budget below one plaintext: every plaintext is its own chunk, same bits
    logn = 16
    n = 1 << logn
    primes, octx, enc = _setup(logn, [51, 46, 46, 58])
    rng = np.random.default_rng(77)
    B, L = 5, 3
    plain = O.uniform_rns(rng, primes[:L], (B,), n)
    d = moai.DeviceBuffer.from_numpy(plain)
    # a fresh context each: a stream arena that already holds the whole batch sets the budget instead
    moai.hip.set_tuning("MOAI_DEC_TMP_MB", 1)
    try:
        chunked = moai.Context(logn, primes).ckks_decode(d, L, 2.0**40, n_batch=B)
    finally:
        moai.hip.reset_tuning()
    full = moai.Context(logn, primes).ckks_decode(d, L, 2.0**40, n_batch=B)
    assert (_bits(full) == _bits(chunked)).all()
    for b in (0, B - 1):
        assert_same(full[b], SD.decode(octx, enc, plain[b], L, 2.0**40))


def test_decode_chunks_and_scale_groups(moai):
    """N = 4096, L = 3: a plaintext needs 4096 * (3 * 8 + 16) = 163840 bytes of scratch.  At MOAI_DEC_TMP_MB = 1 six fit a chunk,
    so 346 plaintexts are 57 chunks of 6 and one of 4; at 24 MiB 153 fit, so they are chunks of 153, 153 and 40, and a chunk of
    153 is two compose launches of 128 (DEC_SCALES, the scales that travel in one launch) and 25.  Every plaintext has its own
    scale, so one that met another's, or another chunk's rows, decodes to other bits."""
    logn = 12
    n = 1 << logn
    primes, octx, enc = _setup(logn, [51, 46, 46, 58])
    rng = np.random.default_rng(346)
    B, L = 2 * 153 + 40, 3
    plain = O.uniform_rns(rng, primes[:L], (B,), n)
    scales = [2.0**30 * (1 + b / 1024) for b in range(B)]
    d = moai.DeviceBuffer.from_numpy(plain)
    # a fresh context each: a stream arena that already holds the whole batch sets the budget instead
    runs = {}
    for mb in (1, 24):
        moai.hip.set_tuning("MOAI_DEC_TMP_MB", mb)
        try:
            runs[mb] = moai.Context(logn, primes).ckks_decode(d, L, scales, n_batch=B)
        finally:
            moai.hip.reset_tuning()
    full = moai.Context(logn, primes).ckks_decode(d, L, scales, n_batch=B)
    assert (_bits(full) == _bits(runs[1])).all() and (_bits(full) == _bits(runs[24])).all()
    # both sides of every chunk and group boundary of the three runs
    for b in (0, 5, 6, 127, 128, 152, 153, 255, 256, 280, 281, 305, 306, 341, 342, B - 1):
        assert_same(full[b], SD.decode(octx, enc, plain[b], L, scales[b]))


def test_argument_errors(moai):
    logn = 10
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    d = moai.DeviceBuffer.from_numpy(np.zeros((3, 3, n), dtype=np.uint64))
    total = ctx.total_coeff_modulus_bit_count(2)
    # ckks.h:672-677: (int)log2(scale) >= total bits, no +1 (encode rejects 2^(total-1), decode does not)
    with pytest.raises(moai.MoaiError, match="scale out of bounds"):
        ctx.ckks_decode(d, 2, 2.0**total)
    ctx.ckks_decode(d, 2, 2.0**total * 0.75)
    ctx.ckks_decode(d, 2, 2.0**(total - 1))
    with pytest.raises(moai.MoaiError, match="scale out of bounds"):
        ctx.ckks_decode(d, 2, [1.0, 0.0], n_batch=2)
    with pytest.raises(moai.MoaiError, match="scale out of bounds"):
        ctx.ckks_decode(d, 2, -1.0)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.ckks_decode(d, 0, 1.0)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.ckks_decode(d, 4, 1.0)
    with pytest.raises(moai.MoaiError):
        ctx.ckks_decode(d, 2, 1.0, prime_index=[0, 3])
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.ckks_decode(None, 2, 1.0)
    with pytest.raises(moai.MoaiError, match="not valid"):
        ctx.decrypt(d, 1, d, 2)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.decrypt(d, 2, d, 4)
    with pytest.raises(moai.MoaiError):
        ctx.decrypt(d, 2, d, 2, prime_index=[7, 0])
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.decrypt(d, 2, None, 2)


SHIM_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "seal/seal.h"
#include "seal/moai_fused.h"
using namespace seal;
static FILE *dump;
static void put_u64(std::uint64_t v) { std::fwrite(&v, 8, 1, dump); }
static void put_f64(double v) { std::fwrite(&v, 8, 1, dump); }
// record: L, scale, is_complex, residues [L][N], decoded values (slots doubles or slots pairs)
template <typename T>
static void record(const SEALContext &context, const Plaintext &pt, const std::vector<T> &dec)
{
    const std::size_t n = context.n(), L = pt.coeff_modulus_size();
    std::vector<std::uint64_t> rows(L * n);
    if (pt.is_scalar())
    {
        for (std::size_t r = 0; r < L; r++)
            for (std::size_t i = 0; i < n; i++)
                rows[r * n + i] = pt.scalar_rows()[r];
    }
    else
    {
        util::hip_check(moai_memcpy_d2h(rows.data(), pt.device_data(), L * n * 8, context.stream()));
        context.sync();
    }
    put_u64(L);
    put_f64(pt.scale());
    put_u64(sizeof(T) == 16 ? 1 : 0);
    std::fwrite(rows.data(), 8, rows.size(), dump);
    std::fwrite(dec.data(), sizeof(T), dec.size(), dump);
}
int main(int argc, char **argv)
{
    dump = std::fopen(argv[1], "wb");
    const std::size_t n = 1 << 16;
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_coeff_modulus(CoeffModulus::Create(n, { 51, 46, 46, 46, 46, 51, 58 }));
    SEALContext context(parms, true, sec_level_type::none);
    KeyGenerator keygen(context);
    PublicKey pk;
    keygen.create_public_key(pk);
    CKKSEncoder encoder(context);
    Encryptor encryptor(context, pk);
    Decryptor decryptor(context, keygen.secret_key());
    Evaluator evaluator(context, encoder);
    const auto &cm = context.key_context_data()->parms().coeff_modulus();
    put_u64(cm.size());
    for (auto &m : cm) put_u64(m.value());
    const std::size_t slots = encoder.slot_count();
    std::vector<double> v(slots);
    for (std::size_t i = 0; i < slots; i++) v[i] = std::sin(0.001 * i) * 3.0 + (i % 7) * 0.25;
    std::vector<Ciphertext> cts;
    int bad = 0;
    for (int drop = 0; drop < 6; drop += 2)  // levels 6, 4, 2
    {
        Plaintext pt, dec_pt;
        encoder.encode(v, std::pow(2.0, 40 + drop), pt);
        Ciphertext ct;
        encryptor.encrypt(pt, ct);
        for (int d = 0; d < drop; d++) evaluator.mod_switch_to_next_inplace(ct);
        decryptor.decrypt(ct, dec_pt);
        std::vector<double> out;
        encoder.decode(dec_pt, out);
        record(context, dec_pt, out);
        std::vector<std::complex<double>> outc;
        encoder.decode(dec_pt, outc);
        record(context, dec_pt, outc);
        for (std::size_t i = 0; i < slots; i++) bad += std::fabs(out[i] - v[i]) > 1e-3;
        cts.push_back(ct);
    }
    // a scalar-row plaintext (constant rows, never materialised)
    {
        Plaintext sp;
        encoder.encode(2.75, std::pow(2.0, 40), sp);
        std::vector<double> out;
        encoder.decode(sp, out);
        record(context, sp, out);
        for (std::size_t i = 0; i < slots; i++) bad += std::fabs(out[i] - 2.75) > 1e-6;
    }
    // moai_fused::decrypt_decode against the per-ciphertext path: mixed levels and a packed ciphertext
    {
        std::vector<Ciphertext> batch = cts;
        batch.push_back(moai_fused::pack({ cts[1], cts[1], cts[1] }, context));
        std::vector<std::vector<double>> got;
        moai_fused::decrypt_decode(batch, decryptor, encoder, got);
        std::vector<Ciphertext> flat = cts;
        for (int i = 0; i < 3; i++) flat.push_back(cts[1]);
        if (got.size() != flat.size()) bad += 1000;
        for (std::size_t c = 0; c < flat.size() && c < got.size(); c++)
        {
            Plaintext p;
            decryptor.decrypt(flat[c], p);
            std::vector<double> one;
            encoder.decode(p, one);
            if (one.size() != got[c].size() || std::memcmp(one.data(), got[c].data(), one.size() * 8) != 0) bad += 1;
        }
    }
    // SEAL's decode scale check (ckks.h:672-677)
    {
        Plaintext p;
        decryptor.decrypt(cts[0], p);
        p.scale() = std::pow(2.0, context.get_context_data(p.parms_id())->total_coeff_modulus_bit_count());
        std::vector<double> out;
        bool thrown = false;
        try { encoder.decode(p, out); } catch (const std::invalid_argument &e) { thrown = std::strstr(e.what(), "scale out of bounds") != nullptr; }
        bad += thrown ? 0 : 1;
    }
    std::fclose(dump);
    unsigned long long checked = 0, violations = 0;
    moai_debug_stream_audit_counts(&checked, &violations);
    std::printf("bad %d violations %llu\n", bad, violations);
    return bad ? 1 : 0;
}
"""


def test_shim_decrypt_decode_bit_exact(tmp_path):
    src = tmp_path / "decode_shim.cpp"
    src.write_text(SHIM_PROGRAM)
    exe = tmp_path / "decode_shim"
    # g++ must be present: a missing compiler fails this test, it does not skip it
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(PKG, "seal_shim"), str(src), "-o", str(exe), "-L" + PKG, "-lmoai_hip",
                        "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    dump = tmp_path / "dump.bin"
    r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "violations 0" in r.stdout, r.stdout
    raw = dump.read_bytes()
    off = 0

    def take(fmt, count=1):
        nonlocal off
        size = struct.calcsize(fmt) * count
        v = np.frombuffer(raw, dtype=np.uint64 if fmt == "Q" else np.float64, count=count, offset=off)
        off += size
        return v

    k = int(take("Q")[0])
    primes = [int(x) for x in take("Q", k)]
    logn = 16
    n = 1 << logn
    octx = O.Context(logn, primes)
    enc = O.CkksEncoder(octx)
    records = 0
    while off < len(raw):
        L = int(take("Q")[0])
        scale = float(take("d")[0])
        is_complex = bool(take("Q")[0])
        rows = take("Q", L * n).reshape(L, n)
        dec = take("d", (n // 2) * (2 if is_complex else 1))
        want = SD.decode(octx, enc, rows, L, scale, is_complex=is_complex)
        assert (dec.view(np.uint64) == np.ascontiguousarray(want).view(np.float64).view(np.uint64)).all()
        records += 1
    assert records == 7
