// Full-slot against sparse-slot bootstrapping through the drop-in Bootstrapper, at MOAI's parameters (N = 2^16, the 36-prime
// chain of include/test/test_full_scheme.hpp:345-378, K = 25, degree 59, two double-angle steps).  For logn = 15 (full) and
// each sparse logn given, packs of each size given: one warm-up run (diagonals encoded, scaled third sets built), then `reps`
// timed runs of bootstrap_full_3 / bootstrap_sparse_3 on the pack (device synchronised before and after; the input copy is
// made outside the timed region).  Prints one line per (logn, pack) and a JSON line per row for tools/boot_sparse_time.py.
//
//   bench_bootstrap_sparse [reps=3] [packs=1,16] [sparse logn=12,13,14]
#include <chrono>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <sstream>

#include "Bootstrapper.h"

static double now_s()
{
    return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count();
}

static vector<long> parse_list(const char *s)
{
    vector<long> v;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, ','))
    {
        v.push_back(std::atol(item.c_str()));
    }
    return v;
}

int main(int argc, char **argv)
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const int reps = argc > 1 ? atoi(argv[1]) : 3;
    const vector<long> packs = parse_list(argc > 2 ? argv[2] : "1,16");
    const vector<long> sparse = parse_list(argc > 3 ? argv[3] : "12,13,14");
    const int logN = 16, remaining_level = 20, boot_level = 14;
    const long logNh = logN - 1, boundary_K = 25, deg = 59, scale_factor = 2, inverse_deg = 1, loge = 10;
    vector<int> bits{ 51 };
    for (int i = 0; i < remaining_level; i++) bits.push_back(46);
    for (int i = 0; i < boot_level; i++) bits.push_back(51);
    bits.push_back(58);
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(size_t(1) << logN);
    parms.set_coeff_modulus(CoeffModulus::Create(size_t(1) << logN, bits));
    parms.set_secret_key_hamming_weight(192);
    const double scale = pow(2.0, 46);
    SEALContext context(parms, true, sec_level_type::none);
    KeyGenerator keygen(context);
    PublicKey pk;
    keygen.create_public_key(pk);
    RelinKeys relin_keys;
    keygen.create_relin_keys(relin_keys);
    GaloisKeys gal_keys;
    Encryptor encryptor(context, pk);
    Decryptor decryptor(context, keygen.secret_key());
    CKKSEncoder encoder(context);
    Evaluator evaluator(context, encoder);

    vector<long> logns{ logNh };
    logns.insert(logns.end(), sparse.begin(), sparse.end());
    Bootstrapper boot(loge, logNh, logNh, remaining_level + boot_level, scale, boundary_K, deg, scale_factor, inverse_deg, context, keygen,
                      encoder, encryptor, decryptor, evaluator, relin_keys, gal_keys);
    boot.prepare_mod_polynomial();
    vector<int> steps{ 0 };
    for (int i = 0; i < logNh; i++) steps.push_back(1 << i);
    for (long ln : logns) boot.slot_vec.push_back(ln);
    for (long ln : logns)
    {
        boot.change_logn(ln);
        boot.addLeftRotKeys_Linear_to_vector_3(steps);
    }
    double t0 = now_s();
    keygen.create_galois_keys(steps, gal_keys);
    boot.generate_LT_coefficient_3();
    context.sync();
    printf("# N = 2^%d, %zu primes, %zu rotation keys, keys + diagonals %.1f s\n", logN, bits.size(), steps.size(), now_s() - t0);

    mt19937_64 rng(1);
    uniform_real_distribution<double> ud(-0.02, 0.02);
    for (long ln : logns)
    {
        boot.change_logn(ln);
        const size_t n = size_t(1) << ln;
        for (long pack : packs)
        {
            vector<Ciphertext> members(static_cast<size_t>(pack));
            for (auto &ct : members)
            {
                vector<complex<double>> msg(n), slots(encoder.slot_count());
                for (auto &z : msg) z = { ud(rng), ud(rng) };
                for (size_t i = 0; i < slots.size(); i++) slots[i] = msg[i % n];
                Plaintext p;
                encoder.encode(slots, scale, p);
                encryptor.encrypt(p, ct);
                while (context.get_context_data(ct.parms_id())->chain_index() != 0) evaluator.mod_switch_to_next_inplace(ct);
            }
            const Ciphertext input = pack == 1 ? members[0] : moai_fused::pack(members, context);
            auto once = [&]() {
                Ciphertext in = input, out;
                context.sync();
                const double t = now_s();
                if (ln == logNh)
                {
                    boot.bootstrap_full_3(out, in);
                }
                else
                {
                    boot.bootstrap_sparse_3(out, in);
                }
                context.sync();
                return now_s() - t;
            };
            const double warm = once();
            double best = 1e30, sum = 0;
            for (int r = 0; r < reps; r++)
            {
                const double t = once();
                best = std::min(best, t);
                sum += t;
            }
            const double ms = 1e3 * sum / reps / static_cast<double>(pack);
            printf("logn %2ld %-6s pack %3ld: %8.2f ms per ciphertext (mean of %d; best %.2f; first run %.2f)\n", ln,
                   ln == logNh ? "full" : "sparse", pack, ms, reps, 1e3 * best / pack, 1e3 * warm / pack);
            printf("{\"logn\": %ld, \"kind\": \"%s\", \"pack\": %ld, \"ms_per_ct\": %.3f, \"best_ms_per_ct\": %.3f, \"reps\": %d}\n", ln,
                   ln == logNh ? "full" : "sparse", pack, ms, 1e3 * best / pack, reps);
        }
    }
    return 0;
}
