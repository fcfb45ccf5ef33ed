"""GPU parity of the client's input path (include/moai_hip.h, "client randomness and encryption"): the ChaCha20-driven
samplers, symmetric and public-key encryption and switching-key generation bit for bit against tests/client_sampling.py
(pinned by tests/test_oracle_client.py), deterministic statistics of the samplers with fixed keys, the noise of what the
device encrypts (Python integers, exact CRT), argument errors, and the seal:: shim's device encryption and key generation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import client_sampling as CS
import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")
MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378
KEY = bytes((7 * i + 3) & 0xFF for i in range(32))


def _setup(moai, logn, bits):
    primes = O.coeff_modulus_create(1 << logn, bits)
    return primes, O.Context(logn, primes), moai.Context(logn, primes)


def _rows(buf, first_word, count, moai):
    """count words of a device buffer from word first_word"""
    out = np.empty(count, dtype=np.uint64)
    lib = moai.hip.lib()
    assert lib.moai_stream_sync(None) == 0
    assert lib.moai_memcpy_d2h(out.ctypes.data, buf.ptr + 8 * first_word, count * 8, None) == 0
    assert lib.moai_stream_sync(None) == 0
    return out


def _secret(octx, rng, primes):
    s = rng.integers(-1, 2, size=octx.n)
    return s, octx.ntt(CS.to_rns(s, primes), len(primes))


def _centered_crt(rows, primes):
    """exact signed integers of [L][N] coefficient-form residues"""
    Q = 1
    for q in primes:
        Q *= int(q)
    x = np.zeros(rows.shape[1], dtype=object)
    for r, q in enumerate(primes):
        Qi = Q // int(q)
        x = x + rows[r].astype(object) * (Qi * pow(Qi % int(q), -1, int(q)))
    x = x % Q
    return np.array([int(v) - Q if v > Q // 2 else int(v) for v in x], dtype=object)


@pytest.mark.parametrize("logn,bits", [(4, [30, 31]), (10, [60, 60, 60]), (12, [51, 46, 46, 58]), (16, MOAI_BITS)])
def test_samplers_match_comparator(moai, logn, bits):
    primes, octx, ctx = _setup(moai, logn, bits)
    n, k = 1 << logn, len(primes)
    nonce = (5 << 56) | 1234
    got = ctx.sample_uniform(KEY, nonce, 2, k).to_numpy((2, k, n))
    for p in range(2):
        assert (got[p] == CS.uniform(KEY, nonce + p, primes, n)).all()
    for fn, ref in ((ctx.sample_ternary, CS.ternary), (ctx.sample_cbd, CS.cbd)):
        got = fn(KEY, nonce, 3, k).to_numpy((3, k, n))
        for p in range(3):
            assert (got[p] == CS.to_rns(ref(KEY, nonce + p, n), primes)).all()
    # rows under a prime_index map: row r under primes[pi[r]]
    pi = list(range(k))[::-1][: max(1, k // 2)]
    got = ctx.sample_uniform(KEY, 77, 1, len(pi), prime_index=pi).to_numpy((len(pi), n))
    assert (got == CS.uniform(KEY, 77, [primes[i] for i in pi], n)).all()
    got = ctx.sample_cbd(KEY, 78, 1, len(pi), prime_index=pi).to_numpy((len(pi), n))
    assert (got == CS.to_rns(CS.cbd(KEY, 78, n), [primes[i] for i in pi])).all()


def test_same_stream_whatever_the_split(moai):
    primes, octx, ctx = _setup(moai, 12, [51, 46, 46, 58])
    n, k = octx.n, len(primes)
    for fn in (ctx.sample_uniform, ctx.sample_ternary, ctx.sample_cbd):
        whole = fn(KEY, 40, 5, k).to_numpy((5, k, n))
        parts = np.concatenate([fn(KEY, 40, 2, k).to_numpy((2, k, n)), fn(KEY, 42, 3, k).to_numpy((3, k, n))])
        assert (whole == parts).all()
        # a different key or nonce gives a different stream
        assert (fn(KEY, 41, 1, k).to_numpy((k, n)) != whole[0]).any()
        assert (fn(bytes(32), 40, 1, k).to_numpy((k, n)) != whole[0]).any()


def test_sampler_statistics(moai):
    """fixed keys, so these are deterministic: CBD against Binomial(42, 1/2) - 21 by chi^2, its range, ternary frequencies,
    uniform rows in 16 buckets by chi^2, and every small sample the same integer in every row (CRT)"""
    from math import comb

    primes, octx, ctx = _setup(moai, 16, [60, 60, 50])
    n, k = octx.n, len(primes)
    P = 16
    e = ctx.sample_cbd(KEY, 9, P, k).to_numpy((P, k, n))
    q0 = np.uint64(primes[0])
    v = np.where(e[:, 0] > q0 // np.uint64(2), e[:, 0].astype(np.int64) - np.int64(primes[0]), e[:, 0].astype(np.int64)).ravel()
    assert v.min() >= -21 and v.max() <= 21
    counts = np.bincount(v + 21, minlength=43)
    expect = np.array([comb(42, j) for j in range(43)], dtype=np.float64) / 2.0**42 * v.size
    m = expect >= 5
    chi2 = (((counts[m] - expect[m]) ** 2) / expect[m]).sum()
    assert chi2 < 80, chi2  # ~30 degrees of freedom
    assert abs(v.std() - np.sqrt(10.5)) < 0.02
    for r in range(1, k):
        q = np.int64(primes[r]) if primes[r] < 2**63 else None
        w = e[:, r].astype(np.int64)
        vr = np.where(w > np.int64(primes[r] // 2), w - q, w).ravel()
        assert (vr == v).all(), "a noise sample differs between rows"
    t = ctx.sample_ternary(KEY, 10, P, k).to_numpy((P, k, n))
    tv = np.where(t[:, 0] == np.uint64(primes[0] - 1), -1, t[:, 0].astype(np.int64)).ravel()
    assert set(np.unique(tv)) == {-1, 0, 1}
    tc = np.bincount(tv + 1, minlength=3)
    assert (np.abs(tc - tv.size / 3) < 4 * np.sqrt(tv.size * 2 / 9)).all(), tc
    for r in range(1, k):
        tr = np.where(t[:, r] == np.uint64(primes[r] - 1), -1, t[:, r].astype(np.int64)).ravel()
        assert (tr == tv).all()
    u = ctx.sample_uniform(KEY, 11, 4, k).to_numpy((4, k, n))
    for r in range(k):
        b = (u[:, r].astype(object) * 16 // primes[r]).astype(np.int64).ravel()
        c = np.bincount(b, minlength=16)
        ex = b.size / 16
        assert (((c - ex) ** 2) / ex).sum() < 45  # 15 degrees of freedom
        assert (u[:, r] < np.uint64(primes[r])).all()


@pytest.mark.parametrize("logn,bits", [(10, [51, 46, 46, 58]), (12, [60, 40, 40, 50, 60])])
def test_encrypt_symmetric_matches_comparator(moai, logn, bits):
    primes, octx, ctx = _setup(moai, logn, bits)
    n, k = octx.n, len(primes)
    rng = np.random.default_rng(logn)
    _, s_ntt = _secret(octx, rng, primes)
    d_sk = moai.DeviceBuffer.from_numpy(s_ntt)
    for L in (k, k - 1, 2):
        B = 3
        plain = O.uniform_rns(rng, primes[:L], (B,), n)
        d_plain = moai.DeviceBuffer.from_numpy(plain)
        got = ctx.encrypt_symmetric(KEY, 100 + L, d_sk, L, B, plain=d_plain).to_numpy((B, 2, L, n))
        assert (got == CS.encrypt_symmetric(octx, KEY, 100 + L, s_ntt, L, B, plain)).all()
        got0 = ctx.encrypt_symmetric(KEY, 100 + L, d_sk, L, 1).to_numpy((2, L, n))
        assert (got0 == CS.encrypt_symmetric(octx, KEY, 100 + L, s_ntt, L, 1)[0]).all()


@pytest.mark.parametrize("logn,bits", [(10, [51, 46, 46, 58]), (12, [60, 40, 40, 50, 60])])
def test_encrypt_asymmetric_matches_comparator(moai, logn, bits):
    primes, octx, ctx = _setup(moai, logn, bits)
    n, k = octx.n, len(primes)
    rng = np.random.default_rng(logn + 1)
    _, s_ntt = _secret(octx, rng, primes)
    d_sk = moai.DeviceBuffer.from_numpy(s_ntt)
    d_pk = ctx.encrypt_symmetric(KEY, 0, d_sk, k)  # create_public_key: an encryption of zero at the key level
    pk = d_pk.to_numpy((2, k, n))
    for L in (k, k - 1, 2, 1):
        B = 3
        plain = O.uniform_rns(rng, primes[:L], (B,), n)
        got = ctx.encrypt_asymmetric(KEY, 10 + L, d_pk, L, B, plain=moai.DeviceBuffer.from_numpy(plain)).to_numpy((B, 2, L, n))
        assert (got == CS.encrypt_asymmetric(octx, KEY, 10 + L, pk, L, B, plain)).all(), L
        got0 = ctx.encrypt_asymmetric(KEY, 10 + L, d_pk, L, 2).to_numpy((2, 2, L, n))
        assert (got0 == CS.encrypt_asymmetric(octx, KEY, 10 + L, pk, L, 2)).all(), L


def test_batches_larger_than_one_chunk(moai):
    """N = 2^16 on MOAI's chain: batches that take several scratch chunks (a public-key encryption at L = 35 needs about
    94 MB of scratch per ciphertext, so the 1 GiB budget holds 11 to 13) with a short last chunk; every ciphertext equals the
    comparator, and two calls in a row (the second with the grown arena) agree with it too.  Symmetric encryption (about
    19 MB per ciphertext at L = 36) is checked on both sides of its first chunk boundary."""
    logn = 16
    primes, octx, ctx = _setup(moai, logn, MOAI_BITS)
    n, k = octx.n, len(primes)
    rng = np.random.default_rng(27)
    _, s_ntt = _secret(octx, rng, primes)
    d_sk = moai.DeviceBuffer.from_numpy(s_ntt)
    d_pk = ctx.encrypt_symmetric(KEY, 0, d_sk, k)
    pk = d_pk.to_numpy((2, k, n))
    L, B = k - 1, 27
    plain = O.uniform_rns(rng, primes[:L], (B,), n)
    d_plain = moai.DeviceBuffer.from_numpy(plain)
    for seq in (1000, 2000):
        got = ctx.encrypt_asymmetric(KEY, seq, d_pk, L, B, plain=d_plain)
        for b in range(B):
            one = _rows(got, b * 2 * L * n, 2 * L * n, moai).reshape(2, L, n)
            want = CS.encrypt_asymmetric(octx, KEY, seq + b, pk, L, 1, plain[b:b + 1])[0]
            assert (one == want).all(), (seq, b)
        del got
    B = 60
    got = ctx.encrypt_symmetric(KEY, 3000, d_sk, k, B)
    for b in (0, 55, 56, 57, B - 1):
        one = _rows(got, b * 2 * k * n, 2 * k * n, moai).reshape(2, k, n)
        assert (one == CS.encrypt_symmetric(octx, KEY, 3000 + b, s_ntt, k, 1)[0]).all(), b


def test_encryption_noise(moai):
    """a symmetric zero decrypts to exactly the sampled e, |e| <= 21; an asymmetric zero below the key level decrypts to
    coefficients within ||s||_1 / 2 + 2 (the bound after divide_and_round)"""
    logn = 12
    primes, octx, ctx = _setup(moai, logn, [51, 46, 46, 46, 58])
    n, k = octx.n, len(primes)
    rng = np.random.default_rng(5)
    s, s_ntt = _secret(octx, rng, primes)
    d_sk = moai.DeviceBuffer.from_numpy(s_ntt)
    L, B = 3, 4
    ct = ctx.encrypt_symmetric(KEY, 300, d_sk, L, B)
    dec = ctx.decrypt(ct, 2, d_sk, L, n_batch=B).to_numpy((B, L, n))
    for b in range(B):
        x = _centered_crt(octx.ntt(dec[b], L, inverse=True), primes[:L])
        e = CS.cbd(KEY, CS.nonce(CS.NOISE0, 300 + b), n)
        assert list(x) == list(e) and max(abs(v) for v in x) <= 21
    d_pk = ctx.encrypt_symmetric(KEY, 0, d_sk, k)
    bound = np.abs(s).sum() / 2 + 2
    for L in (k - 1, 2):
        ct = ctx.encrypt_asymmetric(KEY, 400, d_pk, L, B)
        dec = ctx.decrypt(ct, 2, d_sk, L, n_batch=B).to_numpy((B, L, n))
        for b in range(B):
            x = _centered_crt(octx.ntt(dec[b], L, inverse=True), primes[:L])
            assert max(abs(v) for v in x) <= bound


def test_kswitch_keygen_small(moai):
    logn = 12
    for bits in ([51, 46, 46, 58], [60, 50, 40, 50, 46, 60]):
        primes, octx, ctx = _setup(moai, logn, bits)
        n, k = octx.n, len(primes)
        rng = np.random.default_rng(k)
        s, s_ntt = _secret(octx, rng, primes)
        _, s2_ntt = _secret(octx, rng, primes)
        got = ctx.kswitch_keygen(KEY, 500, moai.DeviceBuffer.from_numpy(s_ntt), moai.DeviceBuffer.from_numpy(s2_ntt))
        got = got.to_numpy((k - 1, 2, k, n))
        for J in range(k - 1):
            assert (got[J] == CS.kswitch_digit(octx, KEY, 500, s_ntt, s2_ntt, J)).all(), J
            # c0 + c1 s = (p mod q_J) s' in row J plus CBD noise
            for r in range(k):
                q = primes[r]
                m = (got[J, 0, r].astype(object) + got[J, 1, r].astype(object) * s_ntt[r].astype(object)) % q
                if r == J:
                    m = (m - s2_ntt[r].astype(object) * (primes[k - 1] % q)) % q
                coeff = octx.ntt(m.astype(np.uint64)[None], 1, prime_index=[r], inverse=True)[0].astype(np.int64)
                e = np.where(coeff > np.int64(q // 2), coeff - np.int64(q), coeff)
                assert np.abs(e).max() <= 21


def test_kswitch_keygen_moai_size(moai):
    """N = 2^16 on MOAI's 36 primes: digits 0, 17 and 34 bit-exact on rows {0, J, 35} (only their stream ranges computed)"""
    logn = 16
    primes, octx, ctx = _setup(moai, logn, MOAI_BITS)
    n, k = octx.n, len(primes)
    rng = np.random.default_rng(36)
    _, s_ntt = _secret(octx, rng, primes)
    _, s2_ntt = _secret(octx, rng, primes)
    key = ctx.kswitch_keygen(KEY, 1 << 40, moai.DeviceBuffer.from_numpy(s_ntt), moai.DeviceBuffer.from_numpy(s2_ntt))
    for J in (0, 17, k - 2):
        rows = sorted({0, J, k - 1})
        want = CS.kswitch_digit(octx, KEY, 1 << 40, s_ntt, s2_ntt, J, rows=rows)
        for i in range(2):
            for r in rows:
                got = _rows(key, ((J * 2 + i) * k + r) * n, n, moai)
                assert (got == want[i, r]).all(), (J, i, r)


def test_argument_errors(moai):
    logn = 10
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    d = moai.DeviceBuffer.from_numpy(np.zeros((4, 2, 3, n), dtype=np.uint64))
    with pytest.raises(moai.MoaiError, match="null key"):
        ctx.sample_uniform(None, 0, 1, 3)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.sample_cbd(KEY, 0, 1, 4)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.sample_ternary(KEY, 0, 1, 0)
    with pytest.raises(moai.MoaiError):
        ctx.sample_uniform(KEY, 0, 1, 2, prime_index=[0, 5])
    with pytest.raises(moai.MoaiError, match="wraps"):
        ctx.sample_uniform(KEY, 2**64 - 1, 2, 3)
    with pytest.raises(moai.MoaiError, match="at most 65535"):
        ctx.sample_cbd(KEY, 0, 65536, 1)
    with pytest.raises(moai.MoaiError, match="2\\^56"):
        ctx.encrypt_symmetric(KEY, 2**56 - 1, d, 2, n_batch=2)
    with pytest.raises(moai.MoaiError, match="2\\^56"):
        ctx.encrypt_asymmetric(KEY, 2**56, d, 2)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.encrypt_symmetric(KEY, 0, d, 4)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.encrypt_asymmetric(KEY, 0, d, 0)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.encrypt_symmetric(KEY, 0, None, 2)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.encrypt_asymmetric(KEY, 0, None, 2)
    with pytest.raises(moai.MoaiError, match="null key"):
        ctx.kswitch_keygen(None, 0, d, d)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.kswitch_keygen(KEY, 0, d, None)
    with pytest.raises(moai.MoaiError, match="2\\^56"):
        ctx.kswitch_keygen(KEY, 2**56 - 1, d, d)
    one = moai.Context(logn, primes[:1])
    with pytest.raises(moai.MoaiError, match="keyswitching"):
        one.kswitch_keygen(KEY, 0, d, d)
    # nothing was enqueued: the buffer still holds zeros
    assert not d.to_numpy().any()
    lib = moai.hip.lib()
    assert lib.moai_encrypt_symmetric(None, KEY, 0, d.ptr, None, d.ptr, 1, 1, None, None) == moai.hip.MOAI_EINVAL


SHIM_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "seal/seal.h"
#include "seal/moai_fused.h"
using namespace seal;
static int bad = 0;
static void check(bool ok, const char *what) { if (!ok) { std::printf("FAIL %s\n", what); bad++; } }
static double max_err(const std::vector<double> &a, const std::vector<double> &b)
{
    double m = 0;
    for (std::size_t i = 0; i < a.size(); i++) m = std::max(m, std::fabs(a[i] - b[i]));
    return m;
}
int main()
{
    const std::size_t n = 1 << 13;
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_coeff_modulus(CoeffModulus::Create(n, { 60, 40, 40, 40, 60 }));
    SEALContext context(parms, true, sec_level_type::none);
    KeyGenerator keygen(context);
    unsigned char seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (unsigned char)(3 * i + 1);
    keygen.set_device_rng(std::make_shared<util::DeviceRng>(seed));
    CKKSEncoder encoder(context);
    Evaluator evaluator(context, encoder);
    Decryptor decryptor(context, keygen.secret_key());
    const std::size_t slots = encoder.slot_count();
    const double scale = std::pow(2.0, 40);
    std::vector<double> v(slots);
    for (std::size_t i = 0; i < slots; i++) v[i] = std::sin(0.01 * i) + (i % 5) * 0.125;
    auto decode = [&](const Ciphertext &ct) { Plaintext p; decryptor.decrypt(ct, p); std::vector<double> o; encoder.decode(p, o); return o; };
    Plaintext pt;
    encoder.encode(v, scale, pt);

    // symmetric encryption on the device: Encryptor(context, secret_key)
    Encryptor sym(context, keygen.secret_key());
    Ciphertext cs;
    sym.encrypt_symmetric(pt, cs);
    check(max_err(decode(cs), v) < 1e-6, "encrypt_symmetric round trip");
    Ciphertext z;
    sym.encrypt_zero_symmetric(z);
    z.scale() = scale;
    check(max_err(decode(z), std::vector<double>(slots, 0.0)) < 1e-6, "encrypt_zero_symmetric");
    bool thrown = false;
    try { Ciphertext c; sym.encrypt(pt, c); } catch (const std::logic_error &) { thrown = true; }
    check(thrown, "encrypt without a public key throws");

    // device public key, then the batched SEAL-faithful public-key path
    PublicKey pk;
    moai_fused::create_public_key(keygen, pk);
    Encryptor enc(context, pk, keygen.secret_key());
    Ciphertext ch;
    enc.encrypt(pt, ch); // the host path takes a device-made public key too
    check(max_err(decode(ch), v) < 1e-5, "host encrypt with a device public key");
    std::vector<Plaintext> plains(3);
    for (int i = 0; i < 3; i++) { std::vector<double> w(v); for (auto &x : w) x *= (i + 1); encoder.encode(w, scale, plains[i]); }
    std::vector<Ciphertext> cts;
    moai_fused::encrypt(enc, plains, cts);
    for (int i = 0; i < 3; i++) { std::vector<double> w(v); for (auto &x : w) x *= (i + 1); check(max_err(decode(cts[i]), w) < 1e-6, "moai_fused::encrypt"); }

    // batch_input: MOAI's slot layout, more columns than one group of 64
    {
        const int num_X = 4, num_row = 8, num_col = 70;
        std::vector<std::vector<std::vector<double>>> X(num_X, std::vector<std::vector<double>>(num_row, std::vector<double>(num_col)));
        for (int j = 0; j < num_X; j++) for (int k = 0; k < num_row; k++) for (int i = 0; i < num_col; i++) X[j][k][i] = 0.01 * (j + 3 * k) - 0.001 * i;
        auto in = moai_fused::batch_input(X, num_X, num_row, num_col, scale, context, pk);
        check((int)in.size() == num_col, "batch_input count");
        for (int i = 0; i < num_col; i += 23)
        {
            std::vector<double> want(slots, 0.0);
            for (int j = 0; j < num_X; j++) for (int k = 0; k < num_row; k++) want[num_X * k + j] = X[j][k][i];
            check(in[i].parms_id() == context.first_parms_id(), "batch_input level");
            check(max_err(decode(in[i]), want) < 1e-6, "batch_input values");
        }
    }

    // relinearization and Galois keys from the device drive the evaluator like host-generated ones
    RelinKeys rk_dev, rk_host;
    moai_fused::create_relin_keys(keygen, rk_dev);
    keygen.create_relin_keys(rk_host);
    std::vector<double> v2(slots);
    for (std::size_t i = 0; i < slots; i++) v2[i] = v[i] * v[i];
    Ciphertext m1, m2;
    evaluator.multiply(cs, cs, m1);
    m2 = m1;
    evaluator.relinearize_inplace(m1, rk_dev);
    evaluator.relinearize_inplace(m2, rk_host);
    check(m1.size() == 2, "relinearized size");
    auto d1 = decode(m1), d2 = decode(m2);
    check(max_err(d1, v2) < 1e-4 && max_err(d1, d2) < 1e-4, "relinearize with a device key");
    GaloisKeys gk_dev, gk_host, gk_all;
    moai_fused::create_galois_keys(keygen, std::vector<int>{ 1, 3 }, gk_dev);
    keygen.create_galois_keys(std::vector<int>{ 1, 3 }, gk_host);
    moai_fused::create_galois_keys(keygen, gk_all);
    for (int step : { 1, 3 })
    {
        std::vector<double> want(slots);
        for (std::size_t i = 0; i < slots; i++) want[i] = v[(i + step) % slots];
        Ciphertext r1, r2;
        evaluator.rotate_vector(cs, step, gk_dev, r1);
        evaluator.rotate_vector(cs, step, gk_host, r2);
        auto a = decode(r1), b = decode(r2);
        check(max_err(a, want) < 1e-5 && max_err(a, b) < 1e-5, "rotate_vector with a device key");
    }
    {
        std::vector<double> want(slots);
        for (std::size_t i = 0; i < slots; i++) want[i] = v[(i + 4) % slots];
        Ciphertext r;
        evaluator.rotate_vector(cs, 4, gk_all, r);
        check(max_err(decode(r), want) < 1e-5, "rotate_vector with a device key of all power-of-two steps");
    }
    // a hoisted rotation (one decomposition, two keys) with the device keys
    {
        const std::size_t L = cs.coeff_modulus_size();
        std::vector<std::uint32_t> elts;
        std::vector<const std::uint64_t *> keys, corr;
        std::vector<Ciphertext> outs(2);
        std::vector<std::uint64_t *> optr;
        int steps[2] = { 1, 3 };
        for (int i = 0; i < 2; i++)
        {
            std::uint32_t e = moai_galois_elt_from_step(context.device(), steps[i]);
            std::size_t idx = GaloisKeys::get_index(e);
            elts.push_back(e);
            keys.push_back(gk_dev.device_key(idx, L));
            corr.push_back(gk_dev.hoist_correction(context, idx, e, L));
            outs[i].resize(context, cs.parms_id(), 2);
            outs[i].is_ntt_form() = true;
            outs[i].scale() = cs.scale();
            optr.push_back(outs[i].device_data());
        }
        int fallback = 0;
        util::hip_check(moai_apply_galois_hoisted(context.device(), cs.device_data(), optr.data(), L, elts.data(), keys.data(), corr.data(),
                                                  2, 1, &fallback, context.stream()));
        context.sync();
        for (int i = 0; i < 2; i++)
        {
            std::vector<double> want(slots);
            for (std::size_t j = 0; j < slots; j++) want[j] = v[(j + steps[i]) % slots];
            check(max_err(decode(outs[i]), want) < 1e-5, "hoisted rotation with device keys");
        }
    }
    unsigned long long checked = 0, violations = 0;
    moai_debug_stream_audit_counts(&checked, &violations);
    std::printf("bad %d violations %llu\n", bad, violations);
    return bad ? 1 : 0;
}
"""


def _compile_shim(tmp_path, text, name):
    src = tmp_path / (name + ".cpp")
    src.write_text(text)
    exe = tmp_path / name
    # g++ must be present: a missing compiler fails this test, it does not skip it
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(PKG, "seal_shim"), str(src), "-o", str(exe), "-L" + PKG, "-lmoai_hip",
                        "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_shim_device_encryption_and_keys(tmp_path):
    """Encryptor(context, sk).encrypt_symmetric / encrypt_zero_symmetric, moai_fused::encrypt and batch_input decrypt to
    their inputs within 1e-6 at scale 2^40; device relin / Galois keys (steps and all) drive relinearize, rotate_vector and a
    hoisted rotation with results within 1e-5 (1e-4 for the square) of host-generated keys; the stream audit stays clean"""
    exe = _compile_shim(tmp_path, SHIM_PROGRAM, "client_shim")
    env = dict(os.environ, MOAI_STREAM_AUDIT="1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "bad 0 violations 0" in r.stdout, r.stdout
