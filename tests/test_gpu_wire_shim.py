"""The seal:: surface of the wire form (seal/moai_serialization.h) on the GPU, in one compiled program run as two processes
under MOAI_STREAM_AUDIT=1: save -> load round trips of every type, a seeded ciphertext and seeded keys written by one process
and used by another, the documented exceptions, the seed (and not the noise key) in the saved bytes, and the byte counts at
MOAI's chain computed here from the parameters."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import wire_format as WF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")
MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378
RNG_KEY = bytes((3 * i + 1) & 0xFF for i in range(32))  # the program's DeviceRng key

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
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
static std::vector<seal_byte> read_file(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<seal_byte> b(s.size());
    std::memcpy(b.data(), s.data(), s.size());
    return b;
}
template <class T> static std::vector<seal_byte> to_bytes(const T &x)
{
    std::vector<seal_byte> b(static_cast<std::size_t>(x.save_size()));
    const auto w = x.save(b.data(), b.size());
    check(static_cast<std::size_t>(w) == b.size(), "save(buffer) returns save_size");
    std::stringstream ss;
    const auto w2 = x.save(ss);
    const std::string s = ss.str();
    check(static_cast<std::size_t>(w2) == b.size() && s.size() == b.size() && std::memcmp(s.data(), b.data(), b.size()) == 0,
          "save(stream) writes the bytes of save(buffer), save_size of them");
    return b;
}
template <class T> static void to_file(const T &x, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    const auto w = x.save(f);
    f.close();
    check(static_cast<std::size_t>(w) == read_file(path).size() && w == x.save_size(), "file size equals save_size");
}
static std::vector<std::uint64_t> words(const SEALContext &c, const std::uint64_t *dev, std::size_t n)
{
    std::vector<std::uint64_t> h(n);
    util::hip_check(moai_memcpy_d2h(h.data(), dev, n * 8, c.stream()));
    c.sync();
    return h;
}
static bool same_ct(const Ciphertext &a, const Ciphertext &b)
{
    return a.parms_id() == b.parms_id() && a.scale() == b.scale() && a.is_ntt_form() == b.is_ntt_form() && a.size() == b.size() &&
           a.download() == b.download();
}
static bool same_keys(const SEALContext &c, const KSwitchKeys &a, const KSwitchKeys &b, std::size_t slots)
{
    const std::size_t k = c.key_context_data()->parms().coeff_modulus().size(), w = (k - 1) * 2 * k * c.n();
    bool ok = a.parms_id() == b.parms_id() && a.size() == b.size();
    for (std::size_t i = 0; i < slots; i++)
    {
        if ((a.device_key(i) != nullptr) != (b.device_key(i) != nullptr)) return false;
        if (a.device_key(i)) ok = ok && words(c, a.device_key(i), w) == words(c, b.device_key(i), w);
    }
    return ok;
}
template <class E, class F> static bool throws(F f)
{
    try { f(); } catch (const E &) { return true; } catch (...) { return false; }
    return false;
}
static void input(std::size_t slots, std::vector<double> &v)
{
    v.resize(slots);
    for (std::size_t i = 0; i < slots; i++) v[i] = std::sin(0.01 * i) + (i % 5) * 0.125;
}
// relinearize(cs * cs), rotate_vector(cs, 1), and a hoisted rotation by {1, 3}: the four results
static std::vector<Ciphertext> evaluate(const SEALContext &context, Evaluator &evaluator, const Ciphertext &cs, const RelinKeys &rk, const GaloisKeys &gk)
{
    std::vector<Ciphertext> out(4);
    evaluator.multiply(cs, cs, out[0]);
    evaluator.relinearize_inplace(out[0], rk);
    evaluator.rotate_vector(cs, 1, gk, out[1]);
    const std::size_t L = cs.coeff_modulus_size();
    std::vector<std::uint32_t> elts;
    std::vector<const std::uint64_t *> keys, corr;
    std::vector<std::uint64_t *> optr;
    int steps[2] = { 1, 3 };
    for (int i = 0; i < 2; i++)
    {
        std::uint32_t e = moai_galois_elt_from_step(context.device(), steps[i]);
        std::size_t idx = GaloisKeys::get_index(e);
        elts.push_back(e);
        keys.push_back(gk.device_key(idx, L));
        corr.push_back(gk.hoist_correction(context, idx, e, L));
        out[2 + i].resize(context, cs.parms_id(), 2);
        out[2 + i].is_ntt_form() = true;
        out[2 + i].scale() = cs.scale();
        optr.push_back(out[2 + i].device_data());
    }
    int fallback = 0;
    util::hip_check(moai_apply_galois_hoisted(context.device(), cs.device_data(), optr.data(), L, elts.data(), keys.data(), corr.data(), 2, 1,
                                              &fallback, context.stream()));
    context.sync();
    return out;
}

static int sizes()
{
    // MOAI's parameters (test_full_scheme.hpp:356-378): byte counts only, nothing is written
    const std::size_t n = 1 << 16;
    std::vector<int> bits = { 51 };
    for (int i = 0; i < 20; i++) bits.push_back(46);
    for (int i = 0; i < 14; i++) bits.push_back(51);
    bits.push_back(58);
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_coeff_modulus(CoeffModulus::Create(n, bits));
    SEALContext context(parms, true, sec_level_type::none);
    KeyGenerator keygen(context);
    Encryptor sym(context, keygen.secret_key());
    Ciphertext full;
    sym.encrypt_zero_symmetric(full);
    std::printf("size seeded_ct %lld\n", (long long)sym.encrypt_zero_symmetric().save_size());
    std::printf("size unseeded_ct %lld\n", (long long)full.save_size());
    std::printf("size seeded_galois_1 %lld\n", (long long)keygen.create_galois_keys(std::vector<int>{ 1 }).save_size());
    std::printf("size parms %lld\n", (long long)parms.save_size());
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "", dir = argc > 2 ? argv[2] : ".";
    if (mode == "sizes") return sizes();
    const bool first = mode == "first";
    EncryptionParameters parms(scheme_type::ckks);
    if (first)
    {
        const std::size_t n = 1 << 13;
        parms.set_poly_modulus_degree(n);
        parms.set_coeff_modulus(CoeffModulus::Create(n, { 60, 40, 40, 40, 60 }));
        to_file(parms, dir + "/parms.bin");
        EncryptionParameters again;
        auto b = to_bytes(parms);
        again.load(b.data(), b.size());
        check(again.poly_modulus_degree() == n && again.coeff_modulus().size() == 5 && again.coeff_modulus()[4].value() == parms.coeff_modulus()[4].value() &&
                  again.scheme() == scheme_type::ckks, "EncryptionParameters round trip");
    }
    else
    {
        std::ifstream f(dir + "/parms.bin", std::ios::binary);
        parms.load(f);
    }
    SEALContext context(parms, true, sec_level_type::none);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context, encoder);
    const std::size_t slots = encoder.slot_count(), n = context.n();
    const double scale = std::pow(2.0, 40);
    std::vector<double> v;
    input(slots, v);

    if (!first)
    {
        // everything arrives as bytes: the secret key, a seeded ciphertext, seeded keys, an evaluation input and the first process's results
        SecretKey sk;
        { std::ifstream f(dir + "/sk.bin", std::ios::binary); sk.load(context, f); }
        Decryptor decryptor(context, sk);
        Ciphertext ct;
        { std::ifstream f(dir + "/ct.bin", std::ios::binary); ct.load(context, f); }
        Plaintext p;
        decryptor.decrypt(ct, p);
        std::vector<double> o;
        encoder.decode(p, o);
        std::printf("second: seeded ciphertext decodes with max error %.3e\n", max_err(o, v));
        check(max_err(o, v) < 1e-6, "seeded ciphertext from another process decrypts to its input");
        RelinKeys rk;
        GaloisKeys gk;
        Ciphertext cs;
        { auto b = read_file(dir + "/rk.bin"); rk.load(context, b.data(), b.size()); }
        { auto b = read_file(dir + "/gk.bin"); gk.load(context, b.data(), b.size()); }
        { auto b = read_file(dir + "/in.bin"); cs.load(context, b.data(), b.size()); }
        auto res = evaluate(context, evaluator, cs, rk, gk);
        for (int i = 0; i < 4; i++)
        {
            Ciphertext want;
            auto b = read_file(dir + "/res" + std::to_string(i) + ".bin");
            want.load(context, b.data(), b.size());
            check(same_ct(res[i], want), "result with loaded keys is identical in both processes");
        }
        std::vector<double> want(slots);
        for (std::size_t i = 0; i < slots; i++) want[i] = v[(i + 3) % slots];
        decryptor.decrypt(res[3], p);
        encoder.decode(p, o);
        check(max_err(o, want) < 1e-5, "hoisted rotation with loaded seeded keys");
        unsigned long long checked = 0, violations = 0;
        moai_debug_stream_audit_counts(&checked, &violations);
        std::printf("bad %d violations %llu\n", bad, violations);
        return bad ? 1 : 0;
    }

    KeyGenerator keygen(context);
    unsigned char seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (unsigned char)(3 * i + 1);
    auto rng = std::make_shared<util::DeviceRng>(seed, 1000);
    keygen.set_device_rng(rng);
    Encryptor sym(context, keygen.secret_key());
    sym.set_device_rng(rng);
    Decryptor decryptor(context, keygen.secret_key());
    Plaintext pt;
    encoder.encode(v, scale, pt);
    Ciphertext cs;
    sym.encrypt_symmetric(pt, cs);
    const std::size_t k = 5;

    // ---- save -> load of every type: identical residues, parms_id, scale and form; save_size equals the bytes written ----
    {
        auto b = to_bytes(cs);
        Ciphertext back;
        check(static_cast<std::size_t>(back.load(context, b.data(), b.size())) == b.size() && same_ct(cs, back), "Ciphertext round trip");
        std::stringstream ss;
        cs.save(ss);
        Ciphertext back2;
        back2.unsafe_load(context, ss);
        check(same_ct(cs, back2), "Ciphertext round trip through a stream, unsafe_load");
        // a size-3 ciphertext at a lower level, and one with deferred terms (a product with a scalar plaintext)
        Ciphertext m, low;
        evaluator.multiply(cs, cs, m);
        evaluator.rescale_to_next_inplace(m);
        auto bm = to_bytes(m);
        back.load(context, bm.data(), bm.size());
        check(back.size() == 3 && same_ct(m, back), "size-3 Ciphertext round trip");
        Plaintext two;
        encoder.encode(2.0, cs.parms_id(), scale, two);
        evaluator.multiply_plain(cs, two, low);
        const bool deferred = low.is_deferred();
        auto bl = to_bytes(low);
        back.load(context, bl.data(), bl.size());
        check(same_ct(low, back), "Ciphertext with deferred terms round trip");
        std::printf("first: deferred before save %d\n", (int)deferred);
    }
    {
        auto b = to_bytes(pt);
        Plaintext back;
        back.load(context, b.data(), b.size());
        check(back.parms_id() == pt.parms_id() && back.scale() == pt.scale() && back.is_ntt_form() &&
                  words(context, back.device_data(), 4 * n) == words(context, pt.device_data(), 4 * n), "Plaintext round trip");
        Plaintext sc, sback;
        encoder.encode(-1.5, scale, sc);
        auto bs = to_bytes(sc);
        check(sc.is_scalar(), "saving a scalar plaintext leaves it scalar");
        sback.load(context, bs.data(), bs.size());
        std::vector<double> o;
        encoder.decode(sback, o);
        check(max_err(o, std::vector<double>(slots, -1.5)) < 1e-6 && !sback.is_scalar(), "scalar Plaintext is written out as rows");
        std::vector<double> mv(slots, 0.0);
        for (std::size_t i = 0; i < slots; i += 2) mv[i] = 0.75;
        Plaintext mp, mback;
        encoder.encode(mv, scale, mp);
        auto bmp = to_bytes(mp);
        mback.load(context, bmp.data(), bmp.size());
        encoder.decode(mback, o);
        check(max_err(o, mv) < 1e-6, "masked-constant Plaintext round trip");
    }
    {
        auto b = to_bytes(keygen.secret_key());
        SecretKey back;
        back.load(context, b.data(), b.size());
        Decryptor d2(context, back);
        check(back.parms_id() == context.key_parms_id() &&
                  words(context, d2.secret_key_device(), k * n) == words(context, decryptor.secret_key_device(), k * n), "SecretKey round trip");
        to_file(keygen.secret_key(), dir + "/sk.bin");
    }
    {
        PublicKey pk, back;
        moai_fused::create_public_key(keygen, pk);
        auto b = to_bytes(pk);
        back.load(context, b.data(), b.size());
        check(same_ct(pk.data(), back.data()) && back.parms_id() == context.key_parms_id(), "PublicKey round trip");
        // a seeded public key works like an ordinary one once loaded
        auto sb = to_bytes(keygen.create_public_key());
        check(sb.size() < b.size() * 51 / 100, "seeded PublicKey is half the size");
        PublicKey spk;
        spk.load(context, sb.data(), sb.size());
        Encryptor enc(context, spk);
        Ciphertext c;
        enc.encrypt(pt, c);
        Plaintext p;
        decryptor.decrypt(c, p);
        std::vector<double> o;
        encoder.decode(p, o);
        check(max_err(o, v) < 1e-5, "encrypt with a loaded seeded PublicKey");
    }
    RelinKeys rk_dev;
    GaloisKeys gk_dev;
    moai_fused::create_relin_keys(keygen, rk_dev);
    moai_fused::create_galois_keys(keygen, std::vector<int>{ 1, 3 }, gk_dev);
    {
        auto b = to_bytes(rk_dev);
        RelinKeys back;
        back.load(context, b.data(), b.size());
        check(same_keys(context, rk_dev, back, 1) && back.has_key(2), "RelinKeys round trip");
        auto g = to_bytes(gk_dev);
        GaloisKeys gback;
        const std::uint64_t gen0 = gback.generation();
        gback.load(context, g.data(), g.size());
        check(same_keys(context, gk_dev, gback, n) && gback.size() == 2 && gback.generation() != gen0 && gback.generation() != gk_dev.generation(),
              "GaloisKeys round trip, fresh generation");
        KSwitchKeys base = gk_dev, kback;
        auto kb = to_bytes(base);
        kback.load(context, kb.data(), kb.size());
        check(same_keys(context, base, kback, n), "KSwitchKeys round trip");
        check(throws<std::logic_error>([&] { RelinKeys r; r.load(context, g.data(), g.size()); }), "a Galois key set is not a RelinKeys");
        // a trimmed key set saves its full keys from the parked host copies, and refuses when they were dropped
        GaloisKeys trimmed = gk_dev;
        trimmed.limit_to_chain_index(context, 1);
        auto tb = to_bytes(trimmed);
        check(tb == g, "a trimmed key set saves the bytes of the full one");
        GaloisKeys gone;
        moai_fused::create_galois_keys(keygen, std::vector<int>{ 1 }, gone);
        gone.limit_to_chain_index(context, 1, false);
        check(throws<std::logic_error>([&] { gone.save_size(); std::stringstream s; gone.save(s); }), "a key trimmed without a host copy cannot be saved");
    }

    // ---- seeded objects leave the process ----------------------------------------------------------------------------------
    auto sct = sym.encrypt_symmetric(pt);
    to_file(sct, dir + "/ct.bin");
    {
        Ciphertext here, full;
        auto b = to_bytes(sct);
        here.load(context, b.data(), b.size());
        Plaintext p;
        decryptor.decrypt(here, p);
        std::vector<double> o;
        encoder.decode(p, o);
        check(max_err(o, v) < 1e-6, "seeded ciphertext decrypts to its input");
        check(b.size() < to_bytes(here).size() * 51 / 100, "seeded Ciphertext is half the size of the expanded one");
        auto z = sym.encrypt_zero_symmetric(context.last_parms_id());
        auto zb = to_bytes(z);
        here.load(context, zb.data(), zb.size());
        here.scale() = scale;
        decryptor.decrypt(here, p);
        encoder.decode(p, o);
        check(here.parms_id() == context.last_parms_id() && max_err(o, std::vector<double>(slots, 0.0)) < 1e-6, "seeded encrypt_zero_symmetric");
    }
    {
        // the batch form: three ciphertexts through one seeded encryption, one pack and one copy; each record loads on its own
        std::vector<Plaintext> plains(3);
        for (int i = 0; i < 3; i++) { std::vector<double> w(v); for (auto &x : w) x *= (i + 1); encoder.encode(w, scale, plains[i]); }
        std::stringstream ss;
        const auto written = moai_fused::encrypt_symmetric_save(sym, plains, ss);
        check(static_cast<std::size_t>(written) == ss.str().size() && written == 3 * sct.save_size(), "batch save writes three seeded records");
        for (int i = 0; i < 3; i++)
        {
            Ciphertext c;
            c.load(context, ss);
            Plaintext p;
            decryptor.decrypt(c, p);
            std::vector<double> o, w(v);
            for (auto &x : w) x *= (i + 1);
            encoder.decode(p, o);
            check(max_err(o, w) < 1e-6, "moai_fused::encrypt_symmetric_save");
        }
    }
    to_file(keygen.create_relin_keys(), dir + "/rk.bin");
    to_file(keygen.create_galois_keys(std::vector<int>{ 1, 3 }), dir + "/gk.bin");
    to_file(cs, dir + "/in.bin");
    {
        RelinKeys rk;
        GaloisKeys gk;
        { auto b = read_file(dir + "/rk.bin"); rk.load(context, b.data(), b.size()); }
        { auto b = read_file(dir + "/gk.bin"); gk.load(context, b.data(), b.size()); }
        auto res = evaluate(context, evaluator, cs, rk, gk);
        auto ref = evaluate(context, evaluator, cs, rk_dev, gk_dev);
        std::vector<double> v2(slots), r1(slots), o;
        for (std::size_t i = 0; i < slots; i++) { v2[i] = v[i] * v[i]; r1[i] = v[(i + 1) % slots]; }
        Plaintext p;
        decryptor.decrypt(res[0], p); encoder.decode(p, o);
        check(max_err(o, v2) < 1e-4, "relinearize with a loaded seeded key");
        decryptor.decrypt(res[1], p); encoder.decode(p, o);
        check(max_err(o, r1) < 1e-5, "rotate_vector with a loaded seeded key");
        decryptor.decrypt(ref[1], p); encoder.decode(p, o);
        check(max_err(o, r1) < 1e-5, "rotate_vector with a generated key");
        // the loaded set trims like a generated one
        gk.limit_to_chain_index(context, 1);
        Ciphertext lowc = cs, r;
        evaluator.mod_switch_to_inplace(lowc, context.last_parms_id());
        evaluator.rotate_vector(lowc, 3, gk, r);
        std::vector<double> r3(slots);
        for (std::size_t i = 0; i < slots; i++) r3[i] = v[(i + 3) % slots];
        decryptor.decrypt(r, p); encoder.decode(p, o);
        check(max_err(o, r3) < 1e-5, "a loaded key set trimmed by limit_to_chain_index");
        for (int i = 0; i < 4; i++) to_file(res[i], dir + "/res" + std::to_string(i) + ".bin");
    }

    // ---- the documented exceptions; the destination stays as it was ---------------------------------------------------------
    {
        Ciphertext dest = cs;
        const auto before = dest.download();
        auto intact = [&] { return dest.download() == before && dest.parms_id() == cs.parms_id() && dest.scale() == cs.scale() && dest.size() == 2; };
        auto b = to_bytes(cs);
        check(throws<std::invalid_argument>([&] { dest.load(context, b.data(), b.size() - 8); }) && intact(), "truncated buffer");
        check(throws<std::invalid_argument>([&] { dest.load(context, b.data(), 64); }) && intact(), "buffer shorter than a header");
        check(throws<std::invalid_argument>([&] { dest.load(context, nullptr, 0); }) && intact(), "null buffer");
        check(throws<std::invalid_argument>([&] { cs.save(b.data(), b.size() - 1); }), "save into a buffer that is too small");
        {
            std::stringstream ss(std::string(reinterpret_cast<const char *>(b.data()), b.size() / 2));
            check(throws<std::runtime_error>([&] { dest.load(context, ss); }) && intact(), "stream that ends early");
        }
        auto m = b;
        m[0] = static_cast<seal_byte>(static_cast<unsigned char>(m[0]) ^ 1);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }) && intact(), "flipped magic");
        m = b;
        m[8] = static_cast<seal_byte>(2);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }) && intact(), "incompatible version");
        m = b;
        m[16] = static_cast<seal_byte>(static_cast<unsigned char>(m[16]) | 8);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }) && intact(), "unknown flag");
        m = b;
        m[72] = static_cast<seal_byte>(static_cast<unsigned char>(m[72]) ^ 0x40);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }) && intact(), "wrong parms_id");
        check(throws<std::logic_error>([&] { Plaintext p; p.load(context, b.data(), b.size()); }), "a ciphertext is not a plaintext");
        // field 0 of row 0 (a 60-bit prime) set to 2^60 - 1 >= q
        m = b;
        for (int i = 0; i < 7; i++) m[sizeof(wire::Header) + i] = static_cast<seal_byte>(0xFF);
        m[sizeof(wire::Header) + 7] = static_cast<seal_byte>(static_cast<unsigned char>(m[sizeof(wire::Header) + 7]) | 0x0F);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }) && intact(), "residue >= q");
        Ciphertext lax;
        lax.unsafe_load(context, m.data(), m.size());
        check(lax.size() == 2 && lax.download()[0] == (std::uint64_t(1) << 60) - 1, "unsafe_load skips the residue check");
        check(throws<std::invalid_argument>([&] { cs.save(b.data(), b.size(), compr_mode_type::zstd); }) &&
                  throws<std::invalid_argument>([&] { cs.save_size(compr_mode_type::zlib); }) &&
                  throws<std::invalid_argument>([&] { sct.save_size(compr_mode_type::zstd); }), "unsupported compression mode");
        check(compr_mode_default == compr_mode_type::none, "compr_mode_default");
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


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _compile_shim(tmp_path_factory.mktemp("wire_shim"), PROGRAM, "wire_shim")


def _run(exe, *args):
    env = dict(os.environ, MOAI_STREAM_AUDIT="1")
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    return r.stdout


def test_shim_wire_two_processes(program, tmp_path):
    """every type round-trips bit for bit with save_size == bytes written; a Serializable<Ciphertext> and the secret key
    written by the first process decrypt in the second within the 1e-6 at scale 2^40 of the unseeded path; seeded relin and
    Galois keys give identical results in both processes; the documented exceptions leave the destination unchanged"""
    out = _run(program, "first", tmp_path)
    assert "bad 0 violations 0" in out, out
    out = _run(program, "second", tmp_path)
    assert "bad 0 violations 0" in out, out

    # the saved bytes, read by the Python restatement of the format
    n, bits = 1 << 13, [60, 40, 40, 40, 60]
    primes = O.coeff_modulus_create(n, bits)
    ct = (tmp_path / "ct.bin").read_bytes()
    h = WF.read_header(ct)
    assert h["kind"] == "ciphertext" and h["flags"] == WF.FLAG_SEEDED | WF.FLAG_NTT and h["count"] == 2
    assert (h["n"], h["L"], h["scale"]) == (n, 4, 2.0**40) and h["parms_id"][1:3] == (n, 4)
    assert h["total_bytes"] == len(ct) == WF.record_bytes(n, primes[:4], 2, True)
    # the public seed is the head of the purpose-5 stream of the noise key at the object's sequence; the key itself never leaves
    assert h["seq"] >= 1000 and h["seed"] == WF.public_seed(RNG_KEY, h["seq"])
    assert h["seed"] in ct and RNG_KEY not in ct
    for name, kind, keys in (("rk.bin", "relin_keys", 1), ("gk.bin", "galois_keys", 2)):
        data = (tmp_path / name).read_bytes()
        assert RNG_KEY not in data
        h = WF.read_header(data)
        assert (h["kind"], h["count"], h["L"], h["total_bytes"]) == (kind, keys, 5, len(data))
        pos = WF.HEADER_BYTES + 8 * keys
        index = np.frombuffer(data[WF.HEADER_BYTES:pos], dtype="<u8")
        assert len(set(index)) == keys and (name != "rk.bin" or index[0] == 0)
        for _ in range(keys):
            r = WF.read_header(data[pos:])
            assert (r["kind"], r["count"], r["L"], r["flags"]) == ("kswitch_key", 8, 5, 3)
            assert r["seed"] == WF.public_seed(RNG_KEY, r["seq"]) and r["total_bytes"] == WF.record_bytes(n, primes, 8, True)
            pos += r["total_bytes"]
        assert pos == len(data)
    sk = (tmp_path / "sk.bin").read_bytes()
    h = WF.read_header(sk)
    assert (h["kind"], h["count"], h["L"]) == ("secret_key", 1, 5) and len(sk) == WF.record_bytes(n, primes, 1, False)
    # the secret key's residues are the ternary polynomial's: unpacked by the comparator, every row holds the same signs
    rows, invalid = WF.unpack_rows(np.frombuffer(sk[WF.HEADER_BYTES:], dtype="<u8"), 1, n, primes)
    assert not invalid and rows.shape == (1, 5, n)
    parms = (tmp_path / "parms.bin").read_bytes()
    h = WF.read_header(parms)
    assert (h["kind"], h["n"], h["L"], h["count"]) == ("encryption_parameters", n, 5, 0) and len(parms) == WF.HEADER_BYTES + 8 * 8
    assert [int(x) for x in np.frombuffer(parms[WF.HEADER_BYTES + 24:], dtype="<u8")] == [int(q) for q in primes]


def test_save_size_at_moai_parameters(program):
    """header + sum over rows of ceil(N b_r / 64) * 8 bytes per stored polynomial, exactly: a seeded and an unseeded fresh
    ciphertext (35 data primes) and a seeded Galois key (35 digits of 36 rows) at MOAI's chain.  37.6 % and 37.8 % follow."""
    out = _run(program, "sizes")
    got = {line.split()[1]: int(line.split()[2]) for line in out.splitlines() if line.startswith("size ")}
    n = 1 << 16
    primes = O.coeff_modulus_create(n, MOAI_BITS)
    words_data = sum(-(-n * int(q).bit_length() // 64) for q in primes[:35])
    words_key = sum(-(-n * int(q).bit_length() // 64) for q in primes)
    H = 120
    assert got["seeded_ct"] == H + 8 * words_data == H + 1685 * n // 8
    assert got["unseeded_ct"] == H + 2 * 8 * words_data
    assert got["seeded_galois_1"] == H + 8 + H + 35 * 8 * words_key == 2 * H + 8 + 35 * 1743 * n // 8
    assert got["parms"] == H + 8 * (3 + 36)
    assert round(1000 * got["seeded_ct"] / (2 * 35 * n * 8)) == 376 and round(1000 * got["seeded_galois_1"] / (35 * 2 * 36 * n * 8)) == 378
