// Sparse-slot bootstrapping (logn < logNh) and the sparse decode through the drop-in seal:: shim, driven the way
// tests/cpp/test_bootstrap_real.cpp drives the full-slot case (MOAI's constants: K = 25, degree 59, two double-angle steps,
// Hamming weight 192, 51/46/58-bit primes, boot_level 14), with slot_vec holding logn < logNh.
//
//   decode   N = 2^11: CKKSEncoder reads EncryptionParameters::sparse_slots at construction, set_sparse_slots, decode returns
//            sparse_slots values; moai_fused::decrypt_decode gives the same bits; unset, decode is unchanged
//   (none)   N = 2^11, slot_vec = {7, 9, 10}: bootstrap_3 at the two sparse logn and at full slots
//   --full   N = 2^16, MOAI's 36-prime chain, logn = 12
// Checks per logn: decrypt(bootstrap_3(ct)) decoded with sparse_slots = n is the message (bound next to the assertion); the
// full-slot decode of the output has period n; chain index top - 14 and scale final_scale as in the full case; concurrent
// calls gathered into a pack give the bits of single calls; calls with different logn are never packed together; the
// output of each first call has the recorded bits (tests/golden/bootstrap_ref_digests.txt, "own." entries); regenerated
// sets are not served from transforms cached for the old ones.
#include <omp.h>

#include <chrono>
#include <complex>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>

#include "Bootstrapper.h"
#include "boot_fixture.h"

struct Keys : Setup
{
    using Setup::Setup;
    // n values replicated to N/2 slots, encrypted and moved to the lowest level (test_full_scheme.hpp:642-646)
    void fresh(mt19937_64 &rng, size_t n, double magnitude, vector<complex<double>> &msg, Ciphertext &ct)
    {
        uniform_real_distribution<double> ud(-1.0, 1.0);
        msg.resize(n);
        for (auto &z : msg) z = { ud(rng) * magnitude, ud(rng) * magnitude };
        vector<complex<double>> slots(encoder->slot_count());
        for (size_t i = 0; i < slots.size(); i++) slots[i] = msg[i % n];
        Plaintext p;
        encoder->encode(slots, scale, p);
        encryptor->encrypt(p, ct);
        while (context->get_context_data(ct.parms_id())->chain_index() != 0) evaluator->mod_switch_to_next_inplace(ct);
    }
};

static void run_decode()
{
    const size_t n = 64;
    Keys s(11, 2, n);
    CKKSEncoder &sparse_enc = *s.encoder; // built from parms with sparse_slots = n (ckks.cpp:29-30)
    CHECK(sparse_enc.sparse_slot_count() == n && sparse_enc.slot_count() == 1024);
    Keys f(11, 2);
    CHECK(f.encoder->sparse_slot_count() == 1024);
    mt19937_64 rng(5);
    vector<complex<double>> msg;
    Ciphertext ct;
    s.fresh(rng, n, 1.0, msg, ct);
    Plaintext p;
    s.decryptor->decrypt(ct, p);
    vector<complex<double>> dec;
    vector<double> dec_real;
    sparse_enc.decode(p, dec);
    sparse_enc.decode(p, dec_real);
    CHECK(dec.size() == n && dec_real.size() == n);
    double e = 0;
    for (size_t i = 0; i < n; i++) e = max(e, abs(dec[i] - msg[i]));
    printf("decode: sparse_slots %zu, max |error| %.2e\n", n, e);
    CHECK(e < 1e-6);
    for (size_t i = 0; i < n; i++) CHECK(dec_real[i] == dec[i].real());
    // decrypt_decode follows the encoder's sparse slot count, bit for bit
    vector<vector<complex<double>>> dd;
    moai_fused::decrypt_decode(vector<Ciphertext>{ ct, ct }, *s.decryptor, sparse_enc, dd);
    CHECK(dd.size() == 2 && dd[0].size() == n && memcmp(dd[0].data(), dec.data(), n * sizeof(dec[0])) == 0 &&
          memcmp(dd[1].data(), dec.data(), n * sizeof(dec[0])) == 0);
    // set_sparse_slots: back to all slots is the full decode; another count returns that many values
    CKKSEncoder e2(*s.context);
    e2.set_sparse_slots(1024);
    vector<complex<double>> full;
    e2.decode(p, full);
    CHECK(full.size() == 1024);
    e2.set_sparse_slots(8);
    vector<complex<double>> eight;
    e2.decode(p, eight);
    CHECK(eight.size() == 8);
    e2.set_sparse_slots(3);
    CHECK(throws([&] { e2.decode(p, eight); }, "sparse_slots"));
}

static void run_boot(int logN, int remaining, const vector<long> &logns, int n_threads, double bound)
{
    Keys s(logN, remaining);
    const long logNh = logN - 1;
    const long boundary_K = 25, deg = 59, scale_factor = 2, inverse_deg = 1, loge = 10;
    Bootstrapper boot(loge, logns[0], logNh, s.total_level, s.scale, boundary_K, deg, scale_factor, inverse_deg, *s.context, *s.keygen,
                      *s.encoder, *s.encryptor, *s.decryptor, *s.evaluator, s.relin_keys, s.gal_keys);
    boot.prepare_mod_polynomial();
    vector<int> steps{ 0 };
    for (int i = 0; i < logNh; i++) steps.push_back(1 << i); // covers the sub-sum's steps and the rotation by n
    for (long ln : logns) boot.slot_vec.push_back(ln);
    for (long ln : logns)
    {
        boot.change_logn(ln);
        boot.addLeftRotKeys_Linear_to_vector_3(steps);
    }
    double t0 = now_s();
    {
        refgolden::FixedRandomness fixed(logN);
        s.keygen->create_galois_keys(steps, s.gal_keys);
        s.context->sync();
    }
    boot.generate_LT_coefficient_3();
    printf("N = 2^%d: %zu rotation keys, keys + diagonals %.1f s\n", logN, steps.size(), now_s() - t0);
    const size_t top = s.context->first_context_data()->chain_index();
    mt19937_64 rng(logN * 100 + logns[0]);
    map<long, pair<Ciphertext, Ciphertext>> single; // logn -> (input, output of a call made alone)
    for (long ln : logns)
    {
        const size_t n = size_t(1) << ln;
        boot.change_logn(ln);
        vector<complex<double>> msg;
        Ciphertext ct, out;
        s.fresh(rng, n, 0.02, msg, ct);
        Ciphertext keep = ct;
        t0 = now_s();
        boot.bootstrap_3(out, ct);
        s.context->sync();
        const double dt = now_s() - t0;
        const size_t after = s.context->get_context_data(out.parms_id())->chain_index();
        Plaintext p;
        s.decryptor->decrypt(out, p);
        CKKSEncoder dec_enc(*s.context);
        dec_enc.set_sparse_slots(n);
        vector<complex<double>> dec, full;
        dec_enc.decode(p, dec);
        s.encoder->decode(p, full);
        double err = 0, period = 0;
        for (size_t i = 0; i < n; i++) err = max(err, abs(dec[i] - msg[i]));
        for (size_t i = 0; i < full.size(); i++) period = max(period, abs(full[i] - full[i % n]));
        double full_err = 0;
        for (size_t i = 0; i < full.size(); i++) full_err = max(full_err, abs(full[i] - msg[i % n]));
        printf("  logn %ld: chain index 0 -> %zu of %zu, scale 2^%.1f, max |error| sparse decode %.2e, full decode %.2e, "
               "period-n deviation %.2e (%.2f s)\n",
               ln, after, top, log2(out.scale()), err, full_err, period, dt);
        CHECK(after == top - 14);
        CHECK(out.scale() == s.scale);
        CHECK(out.is_ntt_form() && out.size() == 2);
        CHECK(dec.size() == n);
        CHECK(err < bound);
        CHECK(full_err < bound);
        CHECK(period < bound);
        Ciphertext again = keep, out2;
        if (ln == logNh)
        {
            boot.bootstrap_full_3(out2, again);
        }
        else
        {
            boot.bootstrap_sparse_3(out2, again);
        }
        CHECK(out2.download() == out.download());
        single[ln] = { keep, out };
        check_recorded(s, "own.sparse.logN" + to_string(logN) + ".logn" + to_string(ln) + ".bootstrap_3", out);
    }
    // concurrent calls at one logn are gathered into packs, bit-identical to single calls
    {
        const long ln = logns[0];
        boot.change_logn(ln);
        const int total = n_threads * 2;
        vector<Ciphertext> in(total), alone(total), gathered(total);
        vector<vector<complex<double>>> msgs(total);
        in[0] = single[ln].first;
        for (int i = 1; i < total; i++) s.fresh(rng, size_t(1) << ln, 0.02, msgs[i], in[i]);
        for (int i = 0; i < total; i++)
        {
            Ciphertext c = in[i];
            boot.bootstrap_sparse_3(alone[i], c);
        }
        CHECK(alone[0].download() == single[ln].second.download());
        const auto before = boot.gather_statistics();
#pragma omp parallel num_threads(n_threads)
        {
            const int t = omp_get_thread_num();
#pragma omp barrier
            for (int j = 0; j < 2; j++)
            {
                Ciphertext c = in[t * 2 + j];
                boot.bootstrap_3(gathered[t * 2 + j], c);
            }
        }
        const auto after = boot.gather_statistics();
        const size_t runs = after.first - before.first, members = after.second - before.second;
        printf("  logn %ld: %d concurrent calls in %zu packed runs\n", ln, total, runs);
        CHECK(members == (size_t)total && runs < members);
        for (int i = 0; i < total; i++)
        {
            CHECK(gathered[i].parms_id() == alone[i].parms_id() && gathered[i].scale() == alone[i].scale());
            CHECK(gathered[i].download() == alone[i].download());
        }
    }
    // calls with different logn arriving together -- sparse and sparse, full and sparse -- are run as separate packs, each
    // with the bits of its single call.  The second call is made only once the first is queued (gather_pending), so the
    // change_logn in between never races the first call's read of logn.
    auto together = [&](long la, long lb) {
        boot.change_logn(la);
        const auto before = boot.gather_statistics();
        Ciphertext in_a = single[la].first, in_b = single[lb].first, out_a, out_b;
        std::thread a([&] { boot.bootstrap_3(out_a, in_a); });
        const double t_wait = now_s();
        while (boot.gather_pending() == 0 && now_s() - t_wait < 5.0)
        {
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        boot.change_logn(lb);
        std::thread b([&] { boot.bootstrap_3(out_b, in_b); });
        a.join();
        b.join();
        const auto after = boot.gather_statistics();
        printf("  logn %ld and %ld together: %zu runs for %zu ciphertexts\n", la, lb, after.first - before.first,
               after.second - before.second);
        CHECK(after.second - before.second == 2 && after.first - before.first == 2);
        CHECK(out_a.parms_id() == single[la].second.parms_id() && out_a.download() == single[la].second.download());
        CHECK(out_b.parms_id() == single[lb].second.parms_id() && out_b.download() == single[lb].second.download());
    };
    for (std::size_t i = 0; i + 1 < logns.size(); i++)
    {
        together(logns[i], logns[i + 1]);
    }
    if (single.count(logNh) && logns.size() > 1)
    {
        together(logNh, logns[0]); // the full call first: its pack runs after change_logn made the member logn sparse
    }
    // Regenerating the sets drops the transforms bsgs_linear_transform caches by the ADDRESS of a set: with another
    // boundary_K the first inverse set holds other values at the same address, and the transform must follow them.
    if (single.count(logNh))
    {
        boot.change_logn(logNh);
        const auto v = moai_boot::inverse_split((int)logNh);
        vector<complex<double>> slots(s.encoder->slot_count());
        for (size_t i = 0; i < slots.size(); i++) slots[i] = { 0.01 * (double)(i % 7), -0.02 };
        Plaintext p;
        s.encoder->encode(slots, s.scale, p);
        Ciphertext x, with_k, with_2k, with_k_again;
        s.encryptor->encrypt(p, x);
        auto apply = [&](Ciphertext &out) {
            boot.rotated_bsgs_linear_transform(out, x, v.totlen[0], v.basicstep[0], (int)logNh, boot.invfftcoeff1[boot.slot_index]);
        };
        apply(with_k);
        boot.boundary_K *= 2;
        boot.generate_LT_coefficient_3();
        apply(with_2k);
        boot.boundary_K /= 2;
        boot.generate_LT_coefficient_3();
        apply(with_k_again);
        CHECK(with_2k.download() != with_k.download());
        CHECK(with_k_again.download() == with_k.download());
    }
    // refusals before anything is enqueued
    {
        Bootstrapper other(loge, 2, logNh, s.total_level, s.scale, boundary_K, deg, scale_factor, inverse_deg, *s.context, *s.keygen,
                           *s.encoder, *s.encryptor, *s.decryptor, *s.evaluator, s.relin_keys, s.gal_keys);
        other.slot_vec.push_back(2);
        CHECK(throws([&] { other.generate_LT_coefficient_3(); }, "0 bits"));
        other.slot_vec.assign(1, 0);
        CHECK(throws([&] { other.generate_LT_coefficient_3(); }, "logn == 0"));
        other.slot_vec.assign(1, 1);
        CHECK(throws([&] { other.generate_LT_coefficient_3(); }, "0 bits"));
    }
}

int main(int argc, char **argv)
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    setenv("MOAI_BOOT_COMBINE_US", "400000", 0); // as tests/cpp/test_bootstrap_real.cpp: grouping independent of host load
    const string mode = argc > 1 ? argv[1] : "";
    if (mode == "decode")
    {
        run_decode();
    }
    else if (mode == "--full")
    {
        // the bound the full case meets at N = 2^16 (tests/cpp/test_bootstrap_real.cpp, 1.5e-5 measured there)
        run_boot(16, 20, { 12 }, 4, 2e-5);
    }
    else
    {
        // N = 2^11: key-switch noise at 2^11 is far below that of 2^16; same bound as the full case at 2^11
        run_boot(11, 2, { 7, 9, 10 }, 4, 2e-5); // 10 = logNh: the full-slot call, gathered next to sparse ones
    }
    printf("%d checks, %d failed\n", g_checks, g_fail);
    if (!g_fail)
    {
        printf("ALL OK\n");
    }
    return g_fail ? 1 : 0;
}
