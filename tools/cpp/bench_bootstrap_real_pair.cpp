// Two real ciphertexts per bootstrap against one, through the drop-in Bootstrapper at MOAI's parameters (N = 2^16, the
// 36-prime chain of include/test/test_full_scheme.hpp:345-378, K = 25, degree 59, two double-angle steps), full slots.
// `total` real ciphertexts (default 96, what one quarter of a bootstrap round holds at packs of 48) go through
//   bootstrap_3            bootstrap_full_3 on packs of `pack`                      (total / pack packed runs)
//   bootstrap_real_3       bootstrap_full_real_3 on packs of `pack`                 (one more key switch per ciphertext)
//   bootstrap_real_many_3  pairs in[2j], in[2j+1], packs of `pack` PAIRS            (total / (2 pack) packed runs)
// each after one warm-up run (diagonals encoded, scaled third sets built), `reps` timed runs, device synchronised before and
// after.  Then the two element-wise kernels behind the pairing next to moai_add at the shape of the split (2 * pack
// polynomials at the bootstrap's output level), timed with events.  One line per leg and a JSON line per row for
// tools/boot_real_pair_time.py.
//
//   bench_bootstrap_real_pair [reps=3] [total=96] [pack=48]
#include <chrono>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "Bootstrapper.h"

static double now_s()
{
    return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv)
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const int reps = argc > 1 ? atoi(argv[1]) : 3;
    const size_t total = argc > 2 ? (size_t)atol(argv[2]) : 96;
    const size_t pack = argc > 3 ? (size_t)atol(argv[3]) : 48;
    if (reps < 1 || pack < 1 || total < 2 * pack || total % (2 * pack) != 0)
    {
        fprintf(stderr, "total must be a multiple of 2 * pack\n");
        return 2;
    }
    setenv("MOAI_BOOT_MAX_PACK", std::to_string(pack).c_str(), 1);
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

    Bootstrapper boot(loge, logNh, logNh, remaining_level + boot_level, scale, boundary_K, deg, scale_factor, inverse_deg, context, keygen,
                      encoder, encryptor, decryptor, evaluator, relin_keys, gal_keys);
    boot.prepare_mod_polynomial();
    vector<int> steps{ 0 };
    for (int i = 0; i < logNh; i++) steps.push_back(1 << i);
    boot.slot_vec.push_back(logNh);
    boot.addLeftRotKeys_Linear_to_vector_3(steps);
    double t0 = now_s();
    keygen.create_galois_keys(steps, gal_keys);
    boot.generate_LT_coefficient_3();
    context.sync();
    printf("# N = 2^%d, %zu primes, %zu rotation keys, keys + diagonals %.1f s\n", logN, bits.size(), steps.size(), now_s() - t0);

    mt19937_64 rng(1);
    uniform_real_distribution<double> ud(-0.02, 0.02);
    vector<Ciphertext> in(total);
    vector<vector<double>> msgs(total);
    for (size_t c = 0; c < total; c++)
    {
        msgs[c].resize(encoder.slot_count());
        for (auto &v : msgs[c]) v = ud(rng);
        Plaintext p;
        encoder.encode(msgs[c], scale, p);
        encryptor.encrypt(p, in[c]);
        while (context.get_context_data(in[c].parms_id())->chain_index() != 0) evaluator.mod_switch_to_next_inplace(in[c]);
    }
    vector<Ciphertext> packs;
    for (size_t at = 0; at < total; at += pack)
    {
        packs.push_back(moai_fused::pack(vector<Ciphertext>(in.begin() + at, in.begin() + at + pack), context));
    }
    vector<Ciphertext> last_out; // what the leg's last run returned, one entry per input
    auto packed_leg = [&](bool real) {
        vector<Ciphertext> outs(packs.size()), copies = packs;
        context.sync();
        const double t = now_s();
        for (size_t k = 0; k < packs.size(); k++)
        {
            real ? boot.bootstrap_full_real_3(outs[k], copies[k]) : boot.bootstrap_full_3(outs[k], copies[k]);
        }
        context.sync();
        const double dt = now_s() - t;
        last_out.clear();
        for (auto &o : outs)
        {
            vector<Ciphertext> m;
            moai_fused::unpack(o, context, m);
            for (auto &c : m) last_out.push_back(std::move(c));
        }
        return dt;
    };
    auto many_leg = [&]() {
        vector<Ciphertext> copies = in, outs;
        context.sync();
        const double t = now_s();
        boot.bootstrap_real_many_3(outs, copies);
        context.sync();
        const double dt = now_s() - t;
        last_out = std::move(outs);
        return dt;
    };
    auto worst_error = [&]() {
        double e = 0;
        for (size_t c : { size_t(0), total - 1 })
        {
            Plaintext p;
            decryptor.decrypt(last_out[c], p);
            vector<complex<double>> dec;
            encoder.decode(p, dec);
            for (size_t i = 0; i < dec.size(); i++) e = max(e, abs(dec[i] - msgs[c][i]));
        }
        return e;
    };
    auto report = [&](const char *leg, size_t per_run, const std::function<double()> &once) {
        const double warm = once();
        double best = 1e30, sum = 0;
        for (int r = 0; r < reps; r++)
        {
            const double t = once();
            best = std::min(best, t);
            sum += t;
        }
        const double ms = 1e3 * sum / reps / (double)total, err = worst_error();
        printf("%-22s %3zu ciphertexts, %2zu per packed run: %8.2f ms per ciphertext (mean of %d; best %.2f; first run %.2f), max |error| of "
               "the first and last %.2e\n",
               leg, total, per_run, ms, reps, 1e3 * best / total, 1e3 * warm / total, err);
        printf("{\"leg\": \"%s\", \"ciphertexts\": %zu, \"per_run\": %zu, \"ms_per_ct\": %.3f, \"best_ms_per_ct\": %.3f, \"reps\": %d, "
               "\"max_error\": %.3e}\n",
               leg, total, per_run, ms, 1e3 * best / total, reps, err);
    };
    report("bootstrap_3", pack, [&] { return packed_leg(false); });
    report("bootstrap_real_3", pack, [&] { return packed_leg(true); });
    report("bootstrap_real_many_3", 2 * pack, many_leg);

    // the element-wise kernels at the shape of the split
    {
        const size_t L = last_out[0].coeff_modulus_size(), n_poly = 2 * pack, N = size_t(1) << logN;
        const size_t words = n_poly * L * N;
        last_out.clear();
        packs.clear();
        void *st = context.stream();
        util::DeviceArray a(words, st), b(words, st), c(words, st), d(words, st);
        util::hip_check(moai_memset_zero(a.get(), words * 8, st));
        util::hip_check(moai_memset_zero(b.get(), words * 8, st));
        void *e0 = nullptr, *e1 = nullptr;
        util::hip_check(moai_event_create(&e0));
        util::hip_check(moai_event_create(&e1));
        auto time_kernel = [&](const char *name, int arrays, const std::function<int()> &launch) {
            for (int w = 0; w < 3; w++) util::hip_check(launch());
            const int iters = 20;
            util::hip_check(moai_event_record(e0, st));
            for (int i = 0; i < iters; i++) util::hip_check(launch());
            util::hip_check(moai_event_record(e1, st));
            util::hip_check(moai_event_synchronize(e1));
            float ms = 0;
            util::hip_check(moai_event_elapsed_ms(e0, e1, &ms));
            const double us = 1e3 * ms / iters, gbs = arrays * words * 8.0 / (us * 1e-6) / 1e9;
            printf("%-12s [%zu][%zu][%zu]: %8.1f us, %7.1f GB/s (%d arrays of %.2f GB)\n", name, n_poly, L, N, us, gbs, arrays,
                   words * 8.0 / 1e9);
            printf("{\"kernel\": \"%s\", \"n_poly\": %zu, \"L\": %zu, \"us\": %.2f, \"gb_per_s\": %.1f}\n", name, n_poly, L, us, gbs);
        };
        moai_ctx *dev = context.device();
        time_kernel("moai_add", 3, [&] { return moai_add(dev, a.get(), b.get(), c.get(), n_poly, L, st); });
        time_kernel("mul_i_add", 3, [&] { return moai_mul_i_add(dev, a.get(), b.get(), c.get(), n_poly, L, 1, st); });
        time_kernel("real_split", 4, [&] { return moai_real_split(dev, a.get(), b.get(), c.get(), d.get(), n_poly, L, st); });
        moai_event_destroy(e0);
        moai_event_destroy(e1);
        context.sync();
    }
    return 0;
}
