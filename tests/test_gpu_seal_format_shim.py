"""The seal:: surface of SEAL's own format (seal/moai_seal_format.h) on the GPU, in one compiled program over the fixtures
Microsoft SEAL 4.1 wrote (tests/golden/seal_format/, Set A): parameters, secret key, a seeded ciphertext and seeded relinearisation
and Galois keys load from SEAL's bytes; the loaded residues are SEAL's own word for word; decrypt + decode and a rotation with the
loaded keys agree with what SEAL itself decrypted; save_seal reproduces SEAL's files byte for byte; this library's own format
still loads; and the exceptions are SEAL's."""
import json
import os
import subprocess

import numpy as np
import pytest

import seal_format as SF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "seal_format")

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "seal/seal.h"
using namespace seal;
static int bad = 0;
static void check(bool ok, const char *what) { if (!ok) { std::printf("FAIL %s\n", what); bad++; } }
static std::vector<seal_byte> read_file(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<seal_byte> b(s.size());
    std::memcpy(b.data(), s.data(), s.size());
    return b;
}
static void write_words(const std::string &path, const std::vector<std::uint64_t> &w)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(w.data()), static_cast<std::streamsize>(w.size() * 8));
}
static void write_doubles(const std::string &path, const std::vector<double> &v)
{
    std::ofstream f(path);
    for (double x : v) { char buf[40]; std::snprintf(buf, sizeof(buf), "%.17g\n", x); f << buf; }
}
static std::vector<std::uint64_t> words(const SEALContext &c, const std::uint64_t *dev, std::size_t n)
{
    std::vector<std::uint64_t> h(n);
    util::hip_check(moai_memcpy_d2h(h.data(), dev, n * 8, c.stream()));
    c.sync();
    return h;
}
// save_seal in its three spellings writes the same bytes, save_size_seal of them
template <class T> static std::vector<seal_byte> to_seal(const T &x)
{
    std::vector<seal_byte> b(static_cast<std::size_t>(x.save_size_seal()));
    const auto w = x.save_seal(b.data(), b.size());
    std::stringstream ss;
    const auto w2 = x.save_seal(ss);
    const std::string s = ss.str();
    check(static_cast<std::size_t>(w) == b.size() && static_cast<std::size_t>(w2) == b.size() && s.size() == b.size() &&
              std::memcmp(s.data(), b.data(), b.size()) == 0, "save_seal(stream) == save_seal(buffer), save_size_seal bytes");
    return b;
}
template <class E, class F> static bool throws(F f, const char *message)
{
    try { f(); } catch (const E &e) { if (std::strstr(e.what(), message)) return true; std::printf("message: %s\n", e.what()); return false; }
    catch (const std::exception &e) { std::printf("other exception: %s\n", e.what()); return false; }
    return false;
}

int main(int argc, char **argv)
{
    const std::string fx = argv[1], out = argv[2];
    EncryptionParameters parms;
    {
        auto b = read_file(fx + "/a_parms.bin");
        check(static_cast<std::size_t>(parms.load(b.data(), b.size())) == b.size(), "EncryptionParameters::load consumes the file");
        check(parms.poly_modulus_degree() == 64 && parms.coeff_modulus().size() == 4 && parms.scheme() == scheme_type::ckks, "parameters");
        check(to_seal(parms) == b, "save_seal(EncryptionParameters) reproduces SEAL's file");
        std::ifstream f(fx + "/a_parms.bin", std::ios::binary);
        EncryptionParameters again;
        again.load(f);
        check(again.coeff_modulus()[3].value() == parms.coeff_modulus()[3].value(), "EncryptionParameters::load(stream)");
        // this library's own format still loads
        std::stringstream ss;
        parms.save(ss);
        again.load(ss);
        check(again.poly_modulus_degree() == 64, "own-format parameters");
    }
    SEALContext context(parms, true, sec_level_type::none);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context, encoder);
    const std::size_t n = context.n(), k = 4;

    SecretKey sk;
    { std::ifstream f(fx + "/a_sk.bin", std::ios::binary); sk.load(context, f); }
    Decryptor decryptor(context, sk);
    write_words(out + "/sk.words", words(context, decryptor.secret_key_device(), k * n));

    Ciphertext ct;
    auto ct_bytes = read_file(fx + "/a_ct_seeded.bin");
    check(static_cast<std::size_t>(ct.load(context, ct_bytes.data(), ct_bytes.size())) == ct_bytes.size(), "Ciphertext::load consumes the file");
    check(ct.size() == 2 && ct.is_ntt_form() && ct.coeff_modulus_size() == 3 && ct.scale() == std::pow(2.0, 40) &&
              ct.parms_id() == context.first_parms_id(), "seeded ciphertext metadata");
    write_words(out + "/ct.words", ct.download());
    {
        std::ifstream f(fx + "/a_ct_seeded.bin", std::ios::binary);
        Ciphertext c2;
        c2.unsafe_load(context, f);
        check(c2.download() == ct.download(), "unsafe_load from a stream gives the same ciphertext");
    }
    Plaintext p;
    std::vector<double> v;
    decryptor.decrypt(ct, p);
    encoder.decode(p, v);
    write_doubles(out + "/decoded.txt", v);

    RelinKeys rk;
    GaloisKeys gk;
    { auto b = read_file(fx + "/a_rk_seeded.bin"); check(static_cast<std::size_t>(rk.load(context, b.data(), b.size())) == b.size(), "RelinKeys::load"); }
    { std::ifstream f(fx + "/a_gk_seeded.bin", std::ios::binary); gk.load(context, f); }
    const std::size_t kw = (k - 1) * 2 * k * n;
    check(rk.has_key(2) && gk.size() == 2, "key sets hold SEAL's keys");
    write_words(out + "/rk.words", words(context, rk.device_key(0), kw));
    // SEAL/galoiskeys.h: Galois element 5 (step 1) at slot 2, 125 (step 3) at slot 62
    check(gk.device_key(2) && gk.device_key(62), "GaloisKeys keep SEAL's indexing by Galois element");
    if (gk.device_key(2) && gk.device_key(62))
    {
        write_words(out + "/gk0.words", words(context, gk.device_key(2), kw));
        write_words(out + "/gk1.words", words(context, gk.device_key(62), kw));
    }
    Ciphertext rot;
    evaluator.rotate_vector(ct, 1, gk, rot);
    decryptor.decrypt(rot, p);
    encoder.decode(p, v);
    write_doubles(out + "/decoded_rot1.txt", v);
    {
        // relinearisation with the loaded key: (ct * ct) decrypts to the squares
        Ciphertext sq;
        evaluator.multiply(ct, ct, sq);
        evaluator.relinearize_inplace(sq, rk);
        decryptor.decrypt(sq, p);
        encoder.decode(p, v);
        write_doubles(out + "/decoded_sq.txt", v);
    }

    // ---- the return path: save_seal reproduces SEAL's files --------------------------------------------------------------
    {
        auto full = read_file(fx + "/a_ct_full.bin");
        Ciphertext c;
        c.load(context, full.data(), full.size());
        check(c.download() == ct.download(), "the full ciphertext is the expanded seeded one");
        check(to_seal(c) == full, "save_seal(Ciphertext) reproduces SEAL's file");
        check(to_seal(ct) == full, "save_seal of the ciphertext loaded seeded is SEAL's full file");
        auto ptb = read_file(fx + "/a_pt.bin");
        Plaintext pt;
        pt.load(context, ptb.data(), ptb.size());
        check(pt.scale() == std::pow(2.0, 40) && pt.parms_id() == context.first_parms_id(), "Plaintext metadata");
        check(to_seal(pt) == ptb, "save_seal(Plaintext) reproduces SEAL's file");
        auto pkb = read_file(fx + "/a_pk_full.bin");
        PublicKey pk, spk;
        pk.load(context, pkb.data(), pkb.size());
        check(to_seal(pk) == pkb, "save_seal(PublicKey) reproduces SEAL's file");
        auto spkb = read_file(fx + "/a_pk_seeded.bin");
        spk.load(context, spkb.data(), spkb.size());
        check(to_seal(spk) == pkb, "a seeded PublicKey expands to SEAL's full one");
        check(to_seal(sk) == read_file(fx + "/a_sk.bin"), "save_seal(SecretKey) reproduces SEAL's file");
        check(to_seal(rk) == read_file(fx + "/a_rk_full.bin"), "save_seal(RelinKeys) reproduces SEAL's full file");
        check(to_seal(gk) == read_file(fx + "/a_gk_full.bin"), "save_seal(GaloisKeys) reproduces SEAL's full file");
        // a ciphertext computed on the device, out and back
        auto rb = to_seal(rot);
        Ciphertext back;
        back.load(context, rb.data(), rb.size());
        check(back.download() == rot.download() && back.parms_id() == rot.parms_id() && back.scale() == rot.scale() && back.is_ntt_form(),
              "save_seal -> load round trip of a computed ciphertext");
        // this library's own format in the same process
        std::stringstream ss;
        rot.save(ss);
        Ciphertext own;
        own.load(context, ss);
        check(own.download() == rot.download(), "own-format round trip");
        // an object seeded on this side is expanded before it is written: SEAL could not expand a ChaCha20 seed
        Encryptor sym(context, sk);
        auto seeded = sym.encrypt_symmetric(pt);
        std::vector<seal_byte> sb(static_cast<std::size_t>(seeded.save_size_seal()));
        seeded.save_seal(sb.data(), sb.size());
        check(sb.size() == full.size(), "a ciphertext seeded on this side is written out full");
        Ciphertext fresh;
        fresh.load(context, sb.data(), sb.size());
        decryptor.decrypt(fresh, p);
        encoder.decode(p, v);
        write_doubles(out + "/decoded_fresh.txt", v);
    }

    // ---- the exceptions are SEAL's; the destination stays as it was --------------------------------------------------------
    {
        Ciphertext dest = ct;
        const auto before = dest.download();
        auto intact = [&] { return dest.download() == before && dest.scale() == ct.scale() && dest.size() == 2; };
        const auto &b = ct_bytes;
        auto full = read_file(fx + "/a_ct_full.bin");
        {
            std::stringstream ss(std::string(reinterpret_cast<const char *>(b.data()), b.size() - 9));
            check(throws<std::runtime_error>([&] { dest.load(context, ss); }, "I/O error") && intact(), "truncated stream");
        }
        auto m = b;
        m[1] = static_cast<seal_byte>(0xA0);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "loaded SEALHeader is invalid") && intact(), "wrong magic");
        m = b;
        m[0] = static_cast<seal_byte>(0x11);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "invalid") && intact(), "neither format");
        m = b;
        m[5] = static_cast<seal_byte>(1);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "loaded SEALHeader is invalid") && intact(), "zlib mode byte");
        m[5] = static_cast<seal_byte>(2);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "loaded SEALHeader is invalid") && intact(), "zstd mode byte");
        m = b;
        m[3] = static_cast<seal_byte>(5);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "incompatible version") && intact(), "version 5.x");
        m = b;
        m[b.size() - 65] = static_cast<seal_byte>(2);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "unsupported prng_type") && intact(), "shake256 type byte");
        m = b;
        m[16] = static_cast<seal_byte>(static_cast<unsigned char>(m[16]) ^ 0x40);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "ciphertext data is invalid") && intact(), "parms_id not in the chain");
        // residue 0 of row 0 set to q_0: header 16, members 73, DynArray header 16 and size 8
        m = full;
        const std::uint64_t q0 = parms.coeff_modulus()[0].value();
        std::memcpy(m.data() + 113, &q0, 8);
        check(throws<std::logic_error>([&] { dest.load(context, m.data(), m.size()); }, "ciphertext data is invalid") && intact(), "residue == q");
        Ciphertext lax;
        lax.unsafe_load(context, m.data(), m.size());
        check(lax.download()[0] == q0, "unsafe_load skips the residue check");
        m = full;
        m[8] = static_cast<seal_byte>(static_cast<unsigned char>(m[8]) + 8);
        check(throws<std::exception>([&] { dest.load(context, m.data(), m.size()); }, "") && intact(), "a header that lies about its size");
        check(throws<std::logic_error>([&] { Plaintext q; q.load(context, full.data(), full.size()); }, "invalid"), "a ciphertext is not a plaintext");
        auto rkb = read_file(fx + "/a_rk_seeded.bin");
        check(throws<std::logic_error>([&] { dest.load(context, rkb.data(), rkb.size()); }, "invalid") && intact(), "a key set is not a ciphertext");
        check(throws<std::invalid_argument>([&] { ct.save_size_seal(compr_mode_type::zstd); }, "unsupported compression mode"), "save_seal with zstd");
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
"""


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _bytes(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seal_format_shim")
    src = tmp / "seal_format_shim.cpp"
    src.write_text(PROGRAM)
    exe = tmp / "seal_format_shim"
    # g++ must be present: a missing compiler fails this test, it does not skip it
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(PKG, "seal_shim"), str(src), "-o", str(exe), "-L" + PKG, "-lmoai_hip",
                        "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), GOLDEN, str(tmp)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "bad 0" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
    return tmp


def _words(path):
    return np.fromfile(path, dtype="<u8")


def _doubles(path):
    return np.loadtxt(path)


def test_loaded_residues_are_seals(outputs):
    """every word of the seeded ciphertext and of the seeded keys, as loaded and expanded on the device, against the files SEAL
    wrote after its own expansion; the secret key against SEAL's"""
    full = SF.read_ciphertext(_bytes("a_ct_full.bin"))
    assert (_words(outputs / "ct.words") == full["data"].reshape(-1)).all()
    assert (_words(outputs / "sk.words") == SF.read_plaintext(_bytes("a_sk.bin"))["data"]).all()
    rk = SF.read_kswitch_keys(_bytes("a_rk_full.bin"))
    assert (_words(outputs / "rk.words") == np.concatenate([d["data"].reshape(-1) for d in rk["keys"][0]])).all()
    gk = SF.read_kswitch_keys(_bytes("a_gk_full.bin"))
    for name, slot in (("gk0.words", 2), ("gk1.words", 62)):
        assert (_words(outputs / name) == np.concatenate([d["data"].reshape(-1) for d in gk["keys"][slot]])).all()


def test_decrypt_and_rotate_match_seals_own(outputs):
    """the bound is twice the error SEAL's own decrypt + decode had on the same ciphertext (recorded by the fixture generator)"""
    info = _json("a.json")
    values = np.array(info["values"])
    err = np.abs(_doubles(outputs / "decoded.txt") - values).max()
    err_rot = np.abs(_doubles(outputs / "decoded_rot1.txt") - np.roll(values, -1)).max()
    err_fresh = np.abs(_doubles(outputs / "decoded_fresh.txt") - values).max()
    print("decode error %.3e (SEAL %.3e), after rotation %.3e (SEAL %.3e), fresh %.3e" %
          (err, info["max_err"], err_rot, info["max_err_rot1"], err_fresh))
    assert err <= 2 * info["max_err"]
    assert err_rot <= 2 * info["max_err_rot1"]
    # SEAL recorded no product: the bound is the rotation's, which carries the same key-switch noise, scaled by the largest
    # factor a product applies to an input's error, 2 max |v| < 4
    err_sq = np.abs(_doubles(outputs / "decoded_sq.txt") - values * values).max()
    print("square error %.3e" % err_sq)
    assert err_sq <= 4 * 2 * info["max_err_rot1"]
    assert err_fresh <= 1e-6  # a fresh encryption on this side: the bound tests/test_gpu_wire_shim.py uses at this scale
