"""Switching keys limited to a chain index on the seal:: surface, in one compiled program run as two processes under
MOAI_STREAM_AUDIT=1.  Chain {60, 40, 40, 40, 60} at N = 2^12.  Process one: two KeyGenerators on the same loaded secret key and
the same DeviceRng key and first sequence -- the limited keys of one equal, word for word, the other's full keys after
limit_to_chain_index; the seeded limited keys are written to files.  Process two: the loaded limited keys give the full keys'
bits at chain index <= limit and refuse above it; a mixed set round-trips; SEAL's format refuses; broken kind-10 records are
rejected.  The byte counts are computed here from the parameters (tests/wire_limited.py)."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import wire_format as WF
import wire_limited as WL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")
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
    return b;
}
template <class T> static void to_file(const T &x, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    const auto w = x.save(f);
    f.close();
    check(static_cast<std::size_t>(w) == read_file(path).size() && w == x.save_size(), "file size equals save_size");
}
template <class T> static void from_file(const SEALContext &c, T &x, const std::string &path)
{
    auto b = read_file(path);
    check(static_cast<std::size_t>(x.load(c, b.data(), b.size())) == b.size(), "load consumes the file");
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
// slot `index` of a and of b hold the same words of a key of `levels` data primes
static bool same_slot(const SEALContext &c, const KSwitchKeys &a, const KSwitchKeys &b, std::size_t index, std::size_t levels)
{
    const std::size_t w = moai_key_words(c.device(), levels);
    return a.device_key(index) && b.device_key(index) && words(c, a.device_key(index), w) == words(c, b.device_key(index), w);
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
static std::uint32_t elt_of(const SEALContext &c, int step) { return moai_galois_elt_from_step(c.device(), step); }
static std::size_t slot_of(const SEALContext &c, int step) { return GaloisKeys::get_index(elt_of(c, step)); }
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
        std::uint32_t e = elt_of(context, steps[i]);
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
    for (auto &c : out) c.download(); // deferred results are made now
    return out;
}
static std::shared_ptr<util::DeviceRng> rng_at(std::uint64_t first)
{
    unsigned char seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (unsigned char)(3 * i + 1);
    return std::make_shared<util::DeviceRng>(seed, first);
}
static void put32(std::vector<seal_byte> &b, std::size_t at, std::uint32_t v) { std::memcpy(b.data() + at, &v, 4); }
static void put64(std::vector<seal_byte> &b, std::size_t at, std::uint64_t v) { std::memcpy(b.data() + at, &v, 8); }

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "", dir = argc > 2 ? argv[2] : ".";
    const bool first = mode == "first";
    const std::size_t n = 1 << 12, k = 5;
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_coeff_modulus(CoeffModulus::Create(n, { 60, 40, 40, 40, 60 }));
    SEALContext context(parms, true, sec_level_type::none);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context, encoder);
    const std::size_t slots = encoder.slot_count();
    const double scale = std::pow(2.0, 40);
    std::vector<double> v;
    input(slots, v);
    const std::vector<std::uint32_t> elts = { elt_of(context, 1), elt_of(context, 3) };
    const std::vector<std::size_t> limits = { 1, 2 }; // chain index per element: 2 and 3 data primes
    const std::size_t s1 = slot_of(context, 1), s3 = slot_of(context, 3);

    if (first)
    {
        {
            KeyGenerator fresh(context);
            to_file(fresh.secret_key(), dir + "/sk.bin");
        }
        SecretKey sk;
        from_file(context, sk, dir + "/sk.bin");
        check(throws<std::invalid_argument>([&] { SecretKey none; KeyGenerator g(context, none); }), "KeyGenerator refuses an empty secret key");
        KeyGenerator lim(context, sk), full(context, sk);
        check(words(context, Decryptor(context, lim.secret_key()).secret_key_device(), k * n) ==
                  words(context, Decryptor(context, sk).secret_key_device(), k * n), "KeyGenerator(context, secret_key) keeps the key");
        lim.set_device_rng(rng_at(1000));
        full.set_device_rng(rng_at(1000));
        RelinKeys rk_l, rk_f;
        GaloisKeys gk_l, gk_f;
        moai_fused::create_relin_keys_limited(lim, 1, rk_l);
        moai_fused::create_galois_keys_limited(lim, elts, limits, gk_l);
        moai_fused::create_relin_keys(full, rk_f);
        moai_fused::create_galois_keys(full, elts, gk_f);
        check(lim.device_rng()->take(1) == 1000 + 3 * (k - 1) && full.device_rng()->take(1) == 1000 + 3 * (k - 1),
              "every key reserves k-1 sequences, limited or not");
        check(rk_l.limited_levels(0) == 2 && rk_l.born_limited(0) && gk_l.limited_levels(s1) == 2 && gk_l.limited_levels(s3) == 3 &&
                  gk_l.born_limited(s3) && gk_l.size() == 2 && rk_f.limited_levels(0) == 0 && !gk_f.born_limited(s1) &&
                  gk_l.limited_levels(0) == 0, "the limit of a slot");
        check(gk_l.device_bytes() == (moai_key_words(context.device(), 2) + moai_key_words(context.device(), 3)) * 8 &&
                  moai_key_words(context.device(), 2) == 2 * 2 * 3 * n, "a born-limited set is resident in the trimmed layout");
        RelinKeys rk_t = rk_f;
        GaloisKeys gk_t1 = gk_f, gk_t2 = gk_f;
        rk_t.limit_to_chain_index(context, 1);
        gk_t1.limit_to_chain_index(context, 1);
        gk_t2.limit_to_chain_index(context, 2);
        check(same_slot(context, rk_l, rk_t, 0, 2), "limited relin key == trim of the full one, word for word");
        check(same_slot(context, gk_l, gk_t1, s1, 2), "limited Galois key (chain index 1) == trim of the full one");
        check(same_slot(context, gk_l, gk_t2, s3, 3), "limited Galois key (chain index 2) == trim of the full one");
        // limit_to_chain_index on a born-limited key is a no-op, in either direction
        const std::uint64_t *p1 = gk_l.device_key(s1), *p3 = gk_l.device_key(s3);
        gk_l.limit_to_chain_index(context, 0);
        gk_l.limit_to_chain_index(context, 2);
        check(gk_l.device_key(s1) == p1 && gk_l.device_key(s3) == p3 && gk_l.limited_levels(s1) == 2 && gk_l.limited_levels(s3) == 3 &&
                  same_slot(context, gk_l, gk_t1, s1, 2), "limit_to_chain_index leaves a born-limited key alone");
        check(gk_l.device_key(s1, 2) == p1 && throws<std::logic_error>([&] { gk_l.device_key(s1, 3); }) && gk_l.device_key(s3, 3) == p3 &&
                  throws<std::logic_error>([&] { gk_l.device_key(s3, 4); }), "device_key above the limit throws");
        // chain index >= k-2 gives a full key in the reference's layout
        RelinKeys rk_top;
        KeyGenerator top(context, sk);
        top.set_device_rng(rng_at(1000));
        moai_fused::create_relin_keys_limited(top, k - 2, rk_top);
        check(rk_top.limited_levels(0) == 0 && !rk_top.born_limited(0) &&
                  words(context, rk_top.device_key(0), (k - 1) * 2 * k * n) == words(context, rk_f.device_key(0), (k - 1) * 2 * k * n),
              "chain index k-2 gives the full key");
        check(throws<std::invalid_argument>([&] { GaloisKeys g; moai_fused::create_galois_keys_limited(top, elts, { 1, 2, 3 }, g); }),
              "chain_indices: one entry, or one per element");

        // ---- the seeded forms leave the process: limited and full from the same sequences -------------------------------
        KeyGenerator slim(context, sk), sfull(context, sk);
        slim.set_device_rng(rng_at(5000));
        sfull.set_device_rng(rng_at(5000));
        auto srk = slim.create_relin_keys_limited(1);
        auto sgk = slim.create_galois_keys_limited(elts, limits);
        std::printf("size rk_limited %lld\n", (long long)srk.save_size());
        std::printf("size gk_limited %lld\n", (long long)sgk.save_size());
        to_file(srk, dir + "/rk_l.bin");
        to_file(sgk, dir + "/gk_l.bin");
        to_file(sfull.create_relin_keys(), dir + "/rk_f.bin");
        to_file(sfull.create_galois_keys(elts), dir + "/gk_f.bin");
        check(throws<std::logic_error>([&] { srk.save_size_seal(); }) && throws<std::logic_error>([&] { std::stringstream s; sgk.save_seal(s); }),
              "SEAL's format cannot express a seeded limited key");
        {
            RelinKeys a, b;
            GaloisKeys ga, gb1, gb2;
            from_file(context, a, dir + "/rk_l.bin");
            from_file(context, b, dir + "/rk_f.bin");
            from_file(context, ga, dir + "/gk_l.bin");
            from_file(context, gb1, dir + "/gk_f.bin");
            gb2 = gb1;
            b.limit_to_chain_index(context, 1);
            gb1.limit_to_chain_index(context, 1);
            gb2.limit_to_chain_index(context, 2);
            check(a.born_limited(0) && a.limited_levels(0) == 2 && ga.limited_levels(s1) == 2 && ga.limited_levels(s3) == 3,
                  "a loaded limited key is born limited");
            check(same_slot(context, a, b, 0, 2) && same_slot(context, ga, gb1, s1, 2) && same_slot(context, ga, gb2, s3, 3),
                  "loaded seeded limited keys == trims of the loaded seeded full keys, word for word");
        }
        // inputs of the second process: at chain index 1 (2 data primes) and 2 (3 data primes)
        Encryptor sym(context, sk);
        Plaintext pt;
        encoder.encode(v, scale, pt);
        Ciphertext cs;
        sym.encrypt_symmetric(pt, cs);
        evaluator.mod_switch_to_next_inplace(cs);
        to_file(cs, dir + "/in3.bin");
        evaluator.mod_switch_to_next_inplace(cs);
        to_file(cs, dir + "/in2.bin");
    }
    else
    {
        SecretKey sk;
        from_file(context, sk, dir + "/sk.bin");
        Decryptor decryptor(context, sk);
        RelinKeys rk_l, rk_f;
        GaloisKeys gk_l, gk_f;
        from_file(context, rk_l, dir + "/rk_l.bin");
        from_file(context, rk_f, dir + "/rk_f.bin");
        from_file(context, gk_l, dir + "/gk_l.bin");
        from_file(context, gk_f, dir + "/gk_f.bin");
        Ciphertext c2, c3;
        from_file(context, c2, dir + "/in2.bin");
        from_file(context, c3, dir + "/in3.bin");
        check(c2.coeff_modulus_size() == 2 && c3.coeff_modulus_size() == 3, "inputs at 2 and 3 data primes");
        auto res = evaluate(context, evaluator, c2, rk_l, gk_l);
        auto ref = evaluate(context, evaluator, c2, rk_f, gk_f);
        const char *names[4] = { "relinearize", "rotate_vector", "hoisted rotation by 1", "hoisted rotation by 3" };
        for (int i = 0; i < 4; i++) check(same_ct(res[i], ref[i]), names[i]);
        std::vector<double> want(slots), o;
        for (std::size_t i = 0; i < slots; i++) want[i] = v[(i + 1) % slots];
        Plaintext p;
        decryptor.decrypt(res[1], p);
        encoder.decode(p, o);
        std::printf("second: rotation with a limited key decodes with max error %.3e\n", max_err(o, want));
        check(max_err(o, want) < 1e-5, "rotate_vector with a loaded limited key decrypts to the rotated input");
        // above the limit: the key for step 1 serves 2 data primes, the key for step 3 serves 3
        {
            Ciphertext r, rf, op = c3;
            const auto before = op.download();
            check(throws<std::logic_error>([&] { evaluator.rotate_vector_inplace(op, 1, gk_l); }) && op.download() == before &&
                      op.parms_id() == c3.parms_id() && op.size() == 2, "a rotation above the limit throws and leaves its operand");
            evaluator.rotate_vector(c3, 3, gk_l, r);
            evaluator.rotate_vector(c3, 3, gk_f, rf);
            check(same_ct(r, rf), "a rotation at the limit of the other key");
            Ciphertext m, mop;
            evaluator.multiply(c3, c3, m);
            m.download();
            mop = m;
            const auto mb = mop.download();
            check(throws<std::logic_error>([&] { evaluator.relinearize_inplace(mop, rk_l); }) && mop.download() == mb && mop.size() == 3,
                  "relinearize above the limit throws and leaves its operand");
        }
        // a mixed set (limited to 2, whole, limited to 3) round-trips through save / load; SEAL's format refuses it
        {
            KeyGenerator gen(context, sk);
            GaloisKeys mixed, back;
            const std::vector<std::uint32_t> e3 = { elt_of(context, 1), elt_of(context, 3), elt_of(context, 5) };
            const std::size_t s5 = slot_of(context, 5);
            moai_fused::create_galois_keys_limited(gen, e3, { 1, 3, 2 }, mixed);
            check(mixed.limited_levels(s1) == 2 && mixed.limited_levels(s3) == 0 && mixed.limited_levels(s5) == 3, "a mixed set");
            auto b = to_bytes(mixed);
            back = gk_l;
            check(static_cast<std::size_t>(back.load(context, b.data(), b.size())) == b.size(), "mixed set loads");
            check(back.size() == 3 && back.limited_levels(s1) == 2 && back.born_limited(s1) && back.limited_levels(s3) == 0 &&
                      back.limited_levels(s5) == 3 && same_slot(context, mixed, back, s1, 2) && same_slot(context, mixed, back, s5, 3) &&
                      words(context, mixed.device_key(s3), (k - 1) * 2 * k * n) == words(context, back.device_key(s3), (k - 1) * 2 * k * n),
                  "mixed set round trip");
            check(to_bytes(back) == b, "a loaded mixed set saves the same bytes");
            Ciphertext r, rf;
            evaluator.rotate_vector(c2, 1, back, r);
            evaluator.rotate_vector(c2, 1, mixed, rf);
            check(same_ct(r, rf), "rotation with a reloaded limited key");
            check(throws<std::logic_error>([&] { mixed.save_size_seal(); }) &&
                      throws<std::logic_error>([&] { std::stringstream s; mixed.save_seal(s); }) &&
                      throws<std::logic_error>([&] { std::stringstream s; gk_l.save_seal(s); }), "save_seal refuses a set with a limited key");
            std::stringstream s;
            gk_f.save_seal(s);
            check(static_cast<std::streamoff>(s.str().size()) == gk_f.save_size_seal(), "save_seal of a set of whole keys still works");
        }
        // broken kind-10 records: rejected with "<what> data is invalid", the destination stays as it was
        {
            const auto good = read_file(dir + "/gk_l.bin");
            GaloisKeys dest = gk_l;
            const std::uint64_t *p1 = dest.device_key(s1);
            const std::uint64_t gen = dest.generation();
            auto intact = [&] { return dest.device_key(s1) == p1 && dest.generation() == gen && dest.limited_levels(s1) == 2 && dest.size() == 2; };
            auto rejected = [&](const std::vector<seal_byte> &m) {
                try { dest.load(context, m.data(), m.size()); }
                catch (const std::logic_error &e) { return std::string(e.what()).find("data is invalid") != std::string::npos; }
                catch (...) { return false; }
                return false;
            };
            const std::size_t rec = sizeof(wire::Header) + 8 * 2; // the first key record: behind the set header and two indices
            wire::Header h;
            std::memcpy(&h, good.data() + rec, sizeof(h));
            check(h.kind == wire::kind_kswitch_key_limited && h.count == 4 && h.L == 3 && (h.flags & wire::flag_seeded), "the first record is kind 10");
            auto m = good;
            put32(m, rec + 20, 0); put32(m, rec + 28, 1);
            check(rejected(m) && intact(), "levels = 0");
            m = good;
            put32(m, rec + 20, 2 * k); put32(m, rec + 28, k + 1);
            check(rejected(m) && intact(), "levels = k");
            m = good;
            put32(m, rec + 20, 6);
            check(rejected(m) && intact(), "count and L disagree");
            m = good;
            put64(m, rec + 32, h.total + 8);
            check(rejected(m) && intact(), "a wrong total");
            m = good; // field 0 of row 0 (a 60-bit prime) set to 2^60 - 1 >= q
            for (int i = 0; i < 7; i++) m[rec + sizeof(wire::Header) + i] = static_cast<seal_byte>(0xFF);
            m[rec + sizeof(wire::Header) + 7] = static_cast<seal_byte>(static_cast<unsigned char>(m[rec + sizeof(wire::Header) + 7]) | 0x0F);
            check(rejected(m) && intact(), "residue >= q");
            GaloisKeys lax;
            lax.unsafe_load(context, m.data(), m.size());
            check(lax.limited_levels(s1) == 2, "unsafe_load skips the residue check");
            check(static_cast<std::size_t>(dest.load(context, good.data(), good.size())) == good.size() && dest.generation() != gen, "the honest bytes load");
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


def _run(exe, *args):
    env = dict(os.environ, MOAI_STREAM_AUDIT="1")
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    return r.stdout


def test_shim_limited_keys_two_processes(tmp_path):
    exe = _compile_shim(tmp_path, PROGRAM, "limited_keys_shim")
    out = _run(exe, "first", tmp_path)
    assert "bad 0 violations 0" in out, out
    got = {line.split()[1]: int(line.split()[2]) for line in out.splitlines() if line.startswith("size ")}

    # the saved bytes, read by the Python restatement of the format
    n, bits = 1 << 12, [60, 40, 40, 40, 60]
    primes = O.coeff_modulus_create(n, bits)
    H = WF.HEADER_BYTES
    # chain index 1: 2 stored polynomials of rows {60, 40, 60} bits; chain index 2: 3 of {60, 40, 40, 60}
    k2, k3 = H + 2 * 160 * n // 8, H + 3 * 200 * n // 8
    assert WL.limited_record_bytes(n, primes, 2, True) == k2 and WL.limited_record_bytes(n, primes, 3, True) == k3
    assert got["rk_limited"] == H + 8 + k2 and got["gk_limited"] == H + 16 + k2 + k3
    full_key = WF.record_bytes(n, primes, 8, True)
    for name, kind, levels in (("rk_l.bin", "relin_keys", [2]), ("gk_l.bin", "galois_keys", [2, 3])):
        data = (tmp_path / name).read_bytes()
        assert len(data) == got[name[:2] + "_limited"] and RNG_KEY not in data
        h = WF.read_header(data)
        assert (h["kind"], h["count"], h["L"], h["total_bytes"]) == (kind, len(levels), 5, len(data))  # the set header keeps L = k
        pos = H + 8 * len(levels)
        index = np.frombuffer(data[H:pos], dtype="<u8")
        assert list(index) == sorted(set(index))
        seqs = []
        for lv in levels:
            r = WL.read_header(data[pos:])
            assert WL.check_limited(r, n, primes, h["parms_id"]) == lv
            assert (r["kind"], r["count"], r["L"], r["flags"]) == (WL.KIND_NAME, 2 * lv, lv + 1, WF.FLAG_SEEDED | WF.FLAG_NTT)
            assert r["seed"] == WF.public_seed(RNG_KEY, r["seq"]) and r["seed"] in data
            rows, invalid = WF.unpack_rows(np.frombuffer(data[pos + H:pos + r["total_bytes"]], dtype="<u8"), lv, n, WL.limited_primes(primes, lv))
            assert not invalid and rows.shape == (lv, lv + 1, n)
            seqs.append(r["seq"])
            pos += r["total_bytes"]
        assert pos == len(data)
        # every key reserved k-1 = 4 sequences: the relin key at 5000, the Galois keys at 5004 and 5008
        assert seqs == ([5000] if name == "rk_l.bin" else [5004, 5008])
        assert len(data) < (tmp_path / name.replace("_l", "_f")).stat().st_size
    assert (tmp_path / "rk_f.bin").stat().st_size == H + 8 + full_key

    out = _run(exe, "second", tmp_path)
    assert "bad 0 violations 0" in out, out
