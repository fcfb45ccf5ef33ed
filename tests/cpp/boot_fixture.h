// tests/cpp/boot_fixture.h -- what the bootstrapping tests that drive the drop-in Bootstrapper share
// (tests/cpp_sparse/test_bootstrap_sparse.cpp, tests/cpp_real/test_bootstrap_real_pair.cpp): the check counter, a clock, a
// "does it throw" helper, the client side at MOAI's constants with fixed randomness, and the recorded-digest assertion.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>

#include "Bootstrapper.h"
#include "ref_golden.h"

static int g_checks = 0, g_fail = 0;
#define CHECK(cond)                                                \
    do                                                             \
    {                                                              \
        g_checks++;                                                \
        if (!(cond))                                               \
        {                                                          \
            g_fail++;                                              \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                          \
    } while (0)

static double now_s()
{
    return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count();
}

struct Setup
{
    int logN, remaining_level, total_level;
    double scale;
    EncryptionParameters parms{ scheme_type::ckks };
    unique_ptr<SEALContext> context;
    unique_ptr<KeyGenerator> keygen;
    RelinKeys relin_keys;
    GaloisKeys gal_keys;
    unique_ptr<Encryptor> encryptor;
    unique_ptr<Decryptor> decryptor;
    unique_ptr<CKKSEncoder> encoder;
    unique_ptr<Evaluator> evaluator;
    Setup(int logN_, int remaining, size_t sparse_slots = 0) : logN(logN_), remaining_level(remaining)
    {
        // include/test/test_full_scheme.hpp:345-378
        const int logp = 46, logq = 51, log_special_prime = 58, boot_level = 14;
        total_level = remaining_level + boot_level;
        vector<int> bits{ logq };
        for (int i = 0; i < remaining_level; i++) bits.push_back(logp);
        for (int i = 0; i < boot_level; i++) bits.push_back(logq);
        bits.push_back(log_special_prime);
        const size_t N = size_t(1) << logN;
        parms.set_poly_modulus_degree(N);
        parms.set_coeff_modulus(CoeffModulus::Create(N, bits));
        parms.set_secret_key_hamming_weight(192);
        if (sparse_slots)
        {
            parms.set_sparse_slots(sparse_slots);
        }
        scale = pow(2.0, logp);
        context.reset(new SEALContext(parms, true, sec_level_type::none));
        refgolden::FixedRandomness fixed(logN);
        keygen.reset(new KeyGenerator(*context));
        PublicKey pk;
        keygen->create_public_key(pk);
        keygen->create_relin_keys(relin_keys);
        encryptor.reset(new Encryptor(*context, pk));
        decryptor.reset(new Decryptor(*context, keygen->secret_key()));
        encoder.reset(new CKKSEncoder(*context));
        evaluator.reset(new Evaluator(*context, *encoder));
    }
};

static bool throws(const std::function<void()> &f, const char *needle = nullptr)
{
    try
    {
        f();
    }
    catch (const std::exception &e)
    {
        return !needle || strstr(e.what(), needle) != nullptr;
    }
    return false;
}

// the bits this project computed at the commit named in tests/golden/bootstrap_ref_digests.txt ("own." entries)
static void check_recorded(const Setup &s, const std::string &name, const Ciphertext &ct)
{
    CHECK(refgolden::matches_recorded(name, *s.context, ct));
}
