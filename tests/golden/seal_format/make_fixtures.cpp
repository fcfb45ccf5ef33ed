// make_fixtures.cpp -- writes the fixtures of tests/golden/seal_format/ with Microsoft SEAL 4.1 itself (README.md here has the
// build line).  Everything is CKKS at sec_level_type::none, compression mode none:
//
//   Set A  N = 64,   four primes below 2^60 that reject 1/17 .. 1/40 of all words: parameters, secret key, public key, plaintext,
//          symmetric ciphertext, relinearisation keys, Galois keys for steps {1, 3}; every seeded object also loaded and re-saved
//          full; a.json holds the encoded values and what SEAL's own decrypt + decode returned, also after rotate_vector by 1
//   Set B  N = 1024, three such primes: seeded ciphertext and relinearisation keys; b.json holds the SHA-256 of the full residues
//   Set C  N = 1024, CoeffModulus::Create(1024, {60, 40, 60}): seeded and full ciphertext (the ordinary case: no rejections)
//
// usage: make_fixtures <output directory>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "seal/seal.h"

using namespace seal;

// ---- SHA-256 (FIPS 180-4), for the digests of Set B ---------------------------------------------------------------------------
static std::string sha256(const std::uint8_t *data, std::size_t len)
{
    static const std::uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2
    };
    std::uint32_t h[8] = { 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19 };
    std::vector<std::uint8_t> m(data, data + len);
    m.push_back(0x80);
    while (m.size() % 64 != 56)
    {
        m.push_back(0);
    }
    for (int i = 7; i >= 0; i--)
    {
        m.push_back(static_cast<std::uint8_t>((static_cast<std::uint64_t>(len) * 8) >> (8 * i)));
    }
    auto rotr = [](std::uint32_t x, int r) { return (x >> r) | (x << (32 - r)); };
    for (std::size_t off = 0; off < m.size(); off += 64)
    {
        std::uint32_t w[64];
        for (int i = 0; i < 16; i++)
        {
            w[i] = (std::uint32_t(m[off + 4 * i]) << 24) | (std::uint32_t(m[off + 4 * i + 1]) << 16) | (std::uint32_t(m[off + 4 * i + 2]) << 8) |
                   m[off + 4 * i + 3];
        }
        for (int i = 16; i < 64; i++)
        {
            const std::uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const std::uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        std::uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++)
        {
            const std::uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const std::uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    char out[65];
    for (int i = 0; i < 8; i++)
    {
        std::snprintf(out + 8 * i, 9, "%08x", h[i]);
    }
    return out;
}

static std::string dir;

template <class T>
static void save(const T &x, const std::string &name)
{
    std::ofstream f(dir + "/" + name, std::ios::binary);
    x.save(f, compr_mode_type::none);
}
// what a seeded object looks like after SEAL itself has loaded (expanded) it
template <class T, class S>
static T expand(const SEALContext &context, const S &seeded)
{
    std::stringstream ss;
    seeded.save(ss, compr_mode_type::none);
    T full;
    full.load(context, ss);
    return full;
}
template <class T, class S>
static T save_both(const SEALContext &context, const S &seeded, const std::string &stem)
{
    std::stringstream ss;
    seeded.save(ss, compr_mode_type::none);
    const std::string bytes = ss.str();
    std::ofstream(dir + "/" + stem + "_seeded.bin", std::ios::binary).write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
    T full;
    full.load(context, ss);
    save(full, stem + "_full.bin");
    return full;
}
static SEALContext make_context(std::size_t n, const std::vector<Modulus> &primes)
{
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_coeff_modulus(primes);
    return SEALContext(parms, true, sec_level_type::none);
}
static std::string json_list(const std::vector<double> &v)
{
    std::string s = "[";
    char buf[40];
    for (std::size_t i = 0; i < v.size(); i++)
    {
        std::snprintf(buf, sizeof(buf), "%s%.17g", i ? ", " : "", v[i]);
        s += buf;
    }
    return s + "]";
}
static std::string json_primes(const SEALContext &context)
{
    std::string s = "[";
    const auto &cm = context.key_context_data()->parms().coeff_modulus();
    for (std::size_t i = 0; i < cm.size(); i++)
    {
        s += (i ? ", " : "") + std::to_string(cm[i].value());
    }
    return s + "]";
}
static double max_err(const std::vector<double> &a, const std::vector<double> &b)
{
    double m = 0;
    for (std::size_t i = 0; i < a.size(); i++)
    {
        m = std::max(m, std::fabs(a[i] - b[i]));
    }
    return m;
}
static std::string digest(const Ciphertext &c)
{
    return sha256(reinterpret_cast<const std::uint8_t *>(c.data()), c.dyn_array().size() * 8);
}

static void set_a()
{
    SEALContext context = make_context(64, { Modulus(1085102592571152769ULL), Modulus(461168601842740097ULL), Modulus(558992244657868289ULL),
                                             Modulus(922337203685478017ULL) });
    if (!context.parameters_set())
    {
        throw std::logic_error("Set A: parameters rejected");
    }
    save(context.key_context_data()->parms(), "a_parms.bin");
    KeyGenerator keygen(context);
    save(keygen.secret_key(), "a_sk.bin");
    save_both<PublicKey>(context, keygen.create_public_key(), "a_pk");
    CKKSEncoder encoder(context);
    const std::size_t slots = encoder.slot_count();
    const double scale = std::pow(2.0, 40);
    std::vector<double> v(slots), rot(slots), got, got_rot;
    for (std::size_t i = 0; i < slots; i++)
    {
        v[i] = std::sin(0.3 * static_cast<double>(i)) + static_cast<double>(i % 5) * 0.125;
    }
    for (std::size_t i = 0; i < slots; i++)
    {
        rot[i] = v[(i + 1) % slots];
    }
    Plaintext pt;
    encoder.encode(v, scale, pt);
    save(pt, "a_pt.bin");
    Encryptor sym(context, keygen.secret_key());
    Decryptor decryptor(context, keygen.secret_key());
    Evaluator evaluator(context, encoder); // the reference fork's Evaluator takes the encoder
    Ciphertext ct = save_both<Ciphertext>(context, sym.encrypt_symmetric(pt), "a_ct");
    save_both<RelinKeys>(context, keygen.create_relin_keys(), "a_rk");
    GaloisKeys gk = save_both<GaloisKeys>(context, keygen.create_galois_keys(std::vector<int>{ 1, 3 }), "a_gk");
    Plaintext p;
    decryptor.decrypt(ct, p);
    encoder.decode(p, got);
    Ciphertext r;
    evaluator.rotate_vector(ct, 1, gk, r);
    decryptor.decrypt(r, p);
    encoder.decode(p, got_rot);
    std::ofstream j(dir + "/a.json");
    j << "{\n  \"n\": 64,\n  \"primes\": " << json_primes(context) << ",\n  \"scale_log2\": 40,\n  \"values\": " << json_list(v)
      << ",\n  \"decoded\": " << json_list(got) << ",\n  \"decoded_rot1\": " << json_list(got_rot);
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.17g", max_err(got, v));
    j << ",\n  \"max_err\": " << buf;
    std::snprintf(buf, sizeof(buf), "%.17g", max_err(got_rot, rot));
    j << ",\n  \"max_err_rot1\": " << buf << "\n}\n";
}

static void set_b()
{
    SEALContext context = make_context(1024, { Modulus(1085102592571174913ULL), Modulus(461168601842771969ULL), Modulus(558992244657879041ULL) });
    if (!context.parameters_set())
    {
        throw std::logic_error("Set B: parameters rejected");
    }
    save(context.key_context_data()->parms(), "b_parms.bin");
    KeyGenerator keygen(context);
    CKKSEncoder encoder(context);
    Plaintext pt;
    encoder.encode(1.25, std::pow(2.0, 40), pt);
    Encryptor sym(context, keygen.secret_key());
    auto sct = sym.encrypt_symmetric(pt);
    save(sct, "b_ct_seeded.bin");
    auto srk = keygen.create_relin_keys();
    save(srk, "b_rk_seeded.bin");
    const Ciphertext ct = expand<Ciphertext>(context, sct);
    const RelinKeys rk = expand<RelinKeys>(context, srk);
    // the digits of the key, each [2][k][N], one after the other
    std::vector<std::uint8_t> all;
    for (const auto &digit : rk.data()[0])
    {
        const auto *b = reinterpret_cast<const std::uint8_t *>(digit.data().data());
        all.insert(all.end(), b, b + digit.data().dyn_array().size() * 8);
    }
    std::ofstream j(dir + "/b.json");
    j << "{\n  \"n\": 1024,\n  \"primes\": " << json_primes(context) << ",\n  \"ct_sha256\": \"" << digest(ct) << "\",\n  \"rk_sha256\": \""
      << sha256(all.data(), all.size()) << "\"\n}\n";
}

static void set_c()
{
    SEALContext context = make_context(1024, CoeffModulus::Create(1024, { 60, 40, 60 }));
    save(context.key_context_data()->parms(), "c_parms.bin");
    KeyGenerator keygen(context);
    CKKSEncoder encoder(context);
    Plaintext pt;
    encoder.encode(-0.5, std::pow(2.0, 30), pt);
    Encryptor sym(context, keygen.secret_key());
    save_both<Ciphertext>(context, sym.encrypt_symmetric(pt), "c_ct");
    std::ofstream j(dir + "/c.json");
    j << "{\n  \"n\": 1024,\n  \"primes\": " << json_primes(context) << "\n}\n";
}

int main(int argc, char **argv)
{
    if (argc < 2)
    {
        std::fprintf(stderr, "usage: make_fixtures <output directory>\n");
        return 2;
    }
    dir = argv[1];
    set_a();
    set_b();
    set_c();
    return 0;
}
