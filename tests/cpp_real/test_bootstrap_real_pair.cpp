// The "real" bootstrap variants (bootstrap_real_3 and what it calls) and two real ciphertexts per bootstrap
// (moai_fused::pair_real / split_real, bootstrap_real_pair_3, bootstrap_real_many_3, Bootstrapper::pair_real) through the
// drop-in seal:: shim, set up as tests/cpp_sparse/test_bootstrap_sparse.cpp is (MOAI's constants: K = 25, degree 59, two
// double-angle steps, Hamming weight 192, 51/46/58-bit primes, boot_level 14).
//
//   (none)   N = 2^11, slot_vec = {7, 9, 10}
//   --full   N = 2^16, MOAI's 36-prime chain, slot_vec = {12, 15}
//
//   1  bootstrap_real_3 on real messages |m| <= 0.02: error below 2e-5 (the bound of the complex case), level, scale, form
//   2  slottocoeff_full_half_3, doubled, against slottocoeff_full_3; bound: twice the error of slottocoeff_full_3 against the
//      clear-text transform of its decrypted input
//   3  pair_real has the bits of encode(i, 1.0) + mod_switch_to + multiply_plain + add; split_real(pair_real(a, b)) is
//      (2a, 2b) within 10 x the error complex_conjugate alone leaves on a
//   4  bootstrap_real_pair_3, |a|, |b| <= 0.02: both outputs within 2e-5, imaginary parts included; at 0.7 the bound of
//      tests/cpp/test_bootstrap_real.cpp for complex messages of that size; table single vs paired at 0.02 .. 1.0 (printed)
//   5  census: bootstrap_real_many_3 on 2B = bootstrap_3 on a pack of B + B conjugations + the two element-wise calls
//   6  determinism: a pair alone = the pair in a pack; gathered real calls = single real calls; real and complex never share
//   7  opt-in pairing of gathered bootstrap_3 calls; off: unchanged bits
//   8  refusals of pair_real
#include <omp.h>

#include <chrono>
#include <complex>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <sstream>
#include <thread>

#include "Bootstrapper.h"
#include "boot_fixture.h"

struct Keys : Setup
{
    using Setup::Setup;
    // n REAL values replicated to N/2 slots, encrypted; moved to the lowest level (test_full_scheme.hpp:642-646) unless `top`
    void fresh(mt19937_64 &rng, size_t n, double magnitude, vector<complex<double>> &msg, Ciphertext &ct, bool top = false,
               double at_scale = 0)
    {
        uniform_real_distribution<double> ud(-1.0, 1.0);
        msg.resize(n);
        for (auto &z : msg) z = { ud(rng) * magnitude, 0.0 };
        encrypt(msg, ct, top, at_scale);
    }
    void encrypt(const vector<complex<double>> &msg, Ciphertext &ct, bool top = false, double at_scale = 0)
    {
        vector<complex<double>> slots(encoder->slot_count());
        for (size_t i = 0; i < slots.size(); i++) slots[i] = msg[i % msg.size()];
        Plaintext p;
        encoder->encode(slots, at_scale > 0 ? at_scale : scale, p);
        encryptor->encrypt(p, ct);
        while (!top && context->get_context_data(ct.parms_id())->chain_index() != 0) evaluator->mod_switch_to_next_inplace(ct);
    }
    // all N/2 slots
    vector<complex<double>> decode(const Ciphertext &ct)
    {
        Plaintext p;
        decryptor->decrypt(ct, p);
        vector<complex<double>> full;
        encoder->decode(p, full);
        return full;
    }
    // max over all N/2 slots of |decoded - factor * msg[i mod n]|, the imaginary part of the decoded value included
    double error(const Ciphertext &ct, const vector<complex<double>> &msg, double factor = 1.0)
    {
        const vector<complex<double>> full = decode(ct);
        double e = 0;
        for (size_t i = 0; i < full.size(); i++) e = max(e, abs(full[i] - factor * msg[i % msg.size()]));
        return e;
    }
    double imag_part(const Ciphertext &ct)
    {
        double e = 0;
        for (auto &z : decode(ct)) e = max(e, fabs(z.imag()));
        return e;
    }
    size_t chain_index(const Ciphertext &ct)
    {
        return context->get_context_data(ct.parms_id())->chain_index();
    }
};

// ---- operation census (moai_op_trace): (entry point, level) -> units
typedef map<pair<string, int>, long> Census;
static Census census_stop()
{
    moai_op_trace(0);
    const size_t need = moai_op_trace_dump(nullptr, 0);
    string buf(need + 16, '\0');
    moai_op_trace_dump(&buf[0], need + 16);
    Census c;
    istringstream in(buf.c_str());
    string name;
    int level;
    long count;
    while (in >> name >> level >> count) c[{ name, level }] += count;
    return c;
}
static long census_total(const Census &c, const string &name)
{
    long t = 0;
    for (auto &kv : c)
        if (kv.first.first == name) t += kv.second;
    return t;
}

// out[t] = sum_k diag[k + first][t mod len] * x[(t + k * step) mod Nh], k = -first .. last: what bsgs_linear_transform
// (first = totlen) and rotated_bsgs_linear_transform (first = 0) compute slot-wise (Bootstrapper.cpp:1997-2129)
static vector<complex<double>> clear_transform(const vector<complex<double>> &x, const vector<vector<complex<double>>> &diag, int first,
                                               int last, long step, double factor)
{
    const long Nh = (long)x.size();
    vector<complex<double>> y(x.size());
    for (long t = 0; t < Nh; t++)
    {
        complex<double> acc = 0;
        for (int k = -first; k <= last; k++)
        {
            const auto &d = diag[(size_t)(k + first)];
            acc += d[(size_t)t % d.size()] * factor * x[(size_t)(((t + k * step) % Nh + Nh) % Nh)];
        }
        y[(size_t)t] = acc;
    }
    return y;
}

static void run(int logN, int remaining, const vector<long> &logns, long pair_sparse_logn, int n_threads)
{
    Keys s(logN, remaining);
    const long logNh = logN - 1;
    const size_t Nh = size_t(1) << logNh;
    const long boundary_K = 25, deg = 59, scale_factor = 2, inverse_deg = 1, loge = 10;
    Bootstrapper boot(loge, logns[0], logNh, s.total_level, s.scale, boundary_K, deg, scale_factor, inverse_deg, *s.context, *s.keygen,
                      *s.encoder, *s.encryptor, *s.decryptor, *s.evaluator, s.relin_keys, s.gal_keys);
    CHECK(boot.pair_real == false); // MOAI_BOOT_PAIR_REAL is not set here: off by default
    boot.prepare_mod_polynomial();
    vector<int> steps{ 0 }; // step 0 is the conjugation key, as in addBootKeys_3
    for (int i = 0; i < logNh; i++) steps.push_back(1 << i);
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
    mt19937_64 rng(logN * 1000 + 7);
    const double bound = 2e-5; // what the complex case meets at both sizes (tests/cpp/test_bootstrap_real.cpp, test_bootstrap_sparse.cpp)
    const string own = "own.real.logN" + to_string(logN); // recorded digests, tests/golden/bootstrap_ref_digests.txt
    auto check_shape = [&](const Ciphertext &out) {
        CHECK(s.chain_index(out) == top - 14);
        CHECK(out.scale() == s.scale);
        CHECK(out.is_ntt_form() && out.size() == 2);
    };

    // ---- 1: bootstrap_real_3 at every logn
    printf("1: bootstrap_real_3\n");
    for (long ln : logns)
    {
        boot.change_logn(ln);
        vector<complex<double>> msg;
        Ciphertext ct, out;
        s.fresh(rng, size_t(1) << ln, 0.02, msg, ct);
        Ciphertext keep = ct;
        t0 = now_s();
        bool threw = false;
        try
        {
            boot.bootstrap_real_3(out, ct);
        }
        catch (const std::exception &e)
        {
            threw = true;
            printf("  logn %ld: bootstrap_real_3 threw: %s\n", ln, e.what());
        }
        CHECK(!threw);
        if (threw)
        {
            continue;
        }
        s.context->sync();
        const double dt = now_s() - t0;
        const double err = s.error(out, msg);
        printf("  logn %ld real: chain index 0 -> %zu of %zu, scale 2^%.1f, max |error| %.2e (%.2f s)\n", ln, s.chain_index(out), top,
               log2(out.scale()), err, dt);
        check_shape(out);
        CHECK(err < bound);
        check_recorded(s, own + ".logn" + to_string(ln) + ".bootstrap_real_3", out);
        // the named variants give the same bits, and bootstrap_inplace_real_3 too
        Ciphertext again = keep, out2;
        if (ln == logNh)
        {
            boot.bootstrap_full_real_3(out2, again);
        }
        else
        {
            boot.bootstrap_sparse_real_3(out2, again);
        }
        CHECK(out2.download() == out.download());
        again = keep;
        boot.bootstrap_inplace_real_3(again);
        CHECK(again.download() == out.download());
    }

    boot.change_logn(logNh);
    const auto &modulus = s.context->first_context_data()->parms().coeff_modulus();

    // ---- 2: the halved slot-to-coefficient transform
    {
        printf("2: slottocoeff_full_half_3 against slottocoeff_full_3\n");
        vector<complex<double>> m1, m2;
        Ciphertext c1, c2;
        // Every stage multiplies by diagonals encoded at the ciphertext's own scale and rescales (scale -> scale^2 / q), so the
        // input sits at the scale of the top prime, as the bootstrap's running scale does.  The third set's constant
        // curr_mod * q_0 * final_scale / (scale^2 * initial_scale) is built for the bootstrap; here initial_scale is chosen so
        // that the constant is about 1.
        const double q_top = (double)modulus[top].value(), q_next = (double)modulus[top - 1].value();
        s.fresh(rng, Nh, 0.02, m1, c1, true, q_top);
        s.fresh(rng, Nh, 0.02, m2, c2, true, q_top);
        const double s1 = q_top * q_top / q_top, s2 = s1 * s1 / q_next;
        const double curr_mod = (double)modulus[top - 2].value(), mod_zero = (double)modulus[0].value();
        boot.initial_scale = curr_mod * mod_zero * boot.final_scale / (s2 * s2);
        const double factor = curr_mod * mod_zero * boot.final_scale / (s2 * s2 * boot.initial_scale);
        Ciphertext full, half;
        boot.slottocoeff_full_3(full, c1, c2);
        boot.slottocoeff_full_half_3(half, c1, c2);
        // the scale bookkeeping `factor` relies on
        CHECK(fabs(full.scale() / (s2 * s2 / curr_mod) - 1) < 1e-9 && half.scale() == full.scale());
        CHECK(s.chain_index(full) == top - 3 && half.parms_id() == full.parms_id());
        check_recorded(s, own + ".slottocoeff_full_half_3", half);
        // clear-text transform of the decrypted input c1 + i c2
        const vector<complex<double>> d1 = s.decode(c1), d2 = s.decode(c2);
        vector<complex<double>> x(Nh);
        for (size_t i = 0; i < Nh; i++) x[i] = d1[i] + complex<double>(0, 1) * d2[i];
        const int p3 = (int)floor(logNh / 3.0), p2 = (int)floor((logNh - p3) / 2.0), p1 = (int)logNh - p3 - p2;
        const int t1 = (1 << p1) - 1, t2 = (1 << p2) - 1, t3 = (1 << p3) - 1;
        const long si = boot.slot_index;
        x = clear_transform(x, boot.fftcoeff1[si], t1, t1, 1, 1.0);
        x = clear_transform(x, boot.fftcoeff2[si], t2, t2, 1L << p1, 1.0);
        x = clear_transform(x, boot.fftcoeff3[si], 0, t3, 1L << (p1 + p2), factor);
        const vector<complex<double>> df = s.decode(full), dh = s.decode(half);
        double err_full = 0, diff = 0, size = 0;
        for (size_t i = 0; i < Nh; i++)
        {
            err_full = max(err_full, abs(df[i] - x[i]));
            diff = max(diff, abs(2.0 * dh[i] - df[i]));
            size = max(size, abs(x[i]));
        }
        printf("  largest value %.3e; slottocoeff_full_3 against the clear-text transform: %.3e; 2 x half - full: %.3e (bound %.3e)\n", size,
               err_full, diff, 2 * err_full);
        CHECK(err_full < 1e-3 * size); // the clear-text transform is the right one
        CHECK(diff <= 2 * err_full);
    }

    // ---- 3: pair_real / split_real
    {
        printf("3: pair_real and split_real\n");
        for (bool at_top : { false, true })
        {
            vector<complex<double>> ma, mb;
            Ciphertext a, b;
            s.fresh(rng, Nh, 1.0, ma, a, at_top);
            s.fresh(rng, Nh, 1.0, mb, b, at_top);
            // the existing route (slottocoeff_full_3's, Bootstrapper.cpp:2760-2777)
            vector<complex<double>> iv(Nh, complex<double>(0.0, 1.0));
            Plaintext ip;
            s.encoder->encode(iv, 1.0, ip);
            s.evaluator->mod_switch_to_inplace(ip, b.parms_id());
            Ciphertext ib, want;
            s.evaluator->multiply_plain(b, ip, ib);
            s.evaluator->add(a, ib, want);
            Ciphertext got;
            moai_fused::pair_real(*s.context, a, b, got);
            CHECK(got.parms_id() == want.parms_id() && got.scale() == want.scale() && got.is_ntt_form() && got.size() == 2);
            CHECK(got.download() == want.download());
            // packed operands
            Ciphertext pa = moai_fused::pack({ a, b, a }, *s.context), pb = moai_fused::pack({ b, a, a }, *s.context), pc;
            moai_fused::pair_real(*s.context, pa, pb, pc);
            vector<Ciphertext> members;
            moai_fused::unpack(pc, *s.context, members);
            CHECK(members.size() == 3 && members[0].download() == want.download());
            // split
            Ciphertext re, im, conj;
            moai_fused::split_real(*s.context, got, s.gal_keys, re, im);
            s.evaluator->complex_conjugate(a, s.gal_keys, conj);
            const double e_conj = s.error(conj, ma), e_re = s.error(re, ma, 2.0), e_im = s.error(im, mb, 2.0);
            printf("  chain index %zu: pair_real bit-identical to multiply_plain + add; complex_conjugate alone %.3e; split: re %.3e, im %.3e "
                   "(bound %.3e)\n",
                   s.chain_index(a), e_conj, e_re, e_im, 10 * e_conj);
            CHECK(re.parms_id() == got.parms_id() && im.parms_id() == got.parms_id() && re.scale() == got.scale() && im.scale() == got.scale());
            CHECK(e_re < 10 * e_conj);
            CHECK(e_im < 10 * e_conj);
        }
    }

    // ---- 4: bootstrap_real_pair_3
    struct PairRun
    {
        double ea, eb, single_a, single_b;
    };
    auto pair_run = [&](long ln, double magnitude, bool with_single, bool recorded = false) {
        boot.change_logn(ln);
        const size_t n = size_t(1) << ln;
        vector<complex<double>> ma, mb;
        Ciphertext a, b, oa, ob;
        s.fresh(rng, n, magnitude, ma, a);
        s.fresh(rng, n, magnitude, mb, b);
        PairRun r{ 0, 0, 0, 0 };
        if (with_single)
        {
            Ciphertext ca = a, cb = b, sa, sb;
            boot.bootstrap_real_3(sa, ca);
            boot.bootstrap_real_3(sb, cb);
            r.single_a = s.error(sa, ma);
            r.single_b = s.error(sb, mb);
        }
        boot.bootstrap_real_pair_3(oa, ob, a, b);
        check_shape(oa);
        check_shape(ob);
        if (recorded)
        {
            check_recorded(s, own + ".logn" + to_string(ln) + ".bootstrap_real_pair_3.a", oa);
            check_recorded(s, own + ".logn" + to_string(ln) + ".bootstrap_real_pair_3.b", ob);
        }
        r.ea = s.error(oa, ma);
        r.eb = s.error(ob, mb);
        return r;
    };
    {
        printf("4: bootstrap_real_pair_3\n");
        for (long ln : { logNh, pair_sparse_logn })
        {
            const PairRun r = pair_run(ln, 0.02, false, true); // the first pair of each logn is pinned
            printf("  logn %ld, |a|, |b| <= 0.02: max |error| a %.2e, b %.2e (imaginary parts of the outputs included)\n", ln, r.ea, r.eb);
            CHECK(r.ea < bound);
            CHECK(r.eb < bound);
        }
        // MOAI's magnitudes: the bound tests/cpp/test_bootstrap_real.cpp:173-182 asserts for complex messages with
        // |Re|, |Im| <= 0.7, which a + i b is
        const PairRun big = pair_run(logNh, 0.7, false);
        printf("  logn %ld, |a|, |b| <= 0.7: max |error| a %.2e, b %.2e (bound %.2e)\n", logNh, big.ea, big.eb, 0.7 * 1.4142 * 0.0065 * 1.2);
        CHECK(big.ea < 0.7 * 1.4142 * 0.0065 * 1.2);
        CHECK(big.eb < 0.7 * 1.4142 * 0.0065 * 1.2);
        // what pairing costs: reported, not asserted
        printf("  magnitude | bootstrap_real_3 alone: a, b | paired: a, b | ratio a, b\n");
        for (double mag : { 0.02, 0.25, 0.7, 1.0 })
        {
            const PairRun r = pair_run(logNh, mag, true);
            printf("  PAIR_TABLE N=2^%d %.2f | %.3e %.3e | %.3e %.3e | %.2f %.2f\n", logN, mag, r.single_a, r.single_b, r.ea, r.eb,
                   r.ea / r.single_a, r.eb / r.single_b);
        }
    }
    boot.change_logn(logNh);

    // ---- 5: the work.  2B real ciphertexts cost one packed bootstrap of B plus B conjugations and two element-wise passes
    {
        printf("5: census\n");
        const size_t B = 4;
        vector<Ciphertext> in(2 * B);
        vector<vector<complex<double>>> msgs(2 * B);
        for (size_t i = 0; i < 2 * B; i++) s.fresh(rng, Nh, 0.02, msgs[i], in[i]);
        Census plain, paired;
        size_t L_out = 0;
        for (int pass = 0; pass < 2; pass++) // the first pass fills the caches of encoded constants
        {
            vector<Ciphertext> half(in.begin(), in.begin() + B);
            Ciphertext packed = moai_fused::pack(half, *s.context), packed_out;
            half.clear();
            s.context->sync();
            moai_op_trace(1);
            boot.bootstrap_full_3(packed_out, packed);
            plain = census_stop();
            L_out = packed_out.coeff_modulus_size();
            vector<Ciphertext> copy = in, out;
            moai_op_trace(1);
            boot.bootstrap_real_many_3(out, copy);
            paired = census_stop();
            if (pass == 1)
            {
                CHECK(out.size() == 2 * B);
                for (size_t i = 0; i < out.size(); i++) CHECK(s.error(out[i], msgs[i]) < bound);
            }
        }
        Census expect = plain;
        // B conjugations at the output level: a key switch each, which permutes both polynomials of its ciphertext first
        expect[{ "apply_galois_to", (int)L_out }] += (long)B;
        expect[{ "galois_permute", (int)L_out }] += (long)(2 * B);
        expect[{ "mul_i_add", 1 }] += (long)(2 * B);           // polynomials: B pairs at the lowest level
        expect[{ "real_split", (int)L_out }] += (long)(2 * B);
        long key_switches = 0;
        for (auto &kv : plain)
            if (kv.first.first == "apply_galois_to" || kv.first.first == "relinearize" || kv.first.first == "switch_key" ||
                kv.first.first == "apply_galois_hoisted")
                key_switches += kv.second;
        printf("  bootstrap_3 on a pack of %zu: %zu census entries, %ld key-switch units (%.1f per ciphertext); bootstrap_real_many_3 on %zu: "
               "%zu entries\n",
               B, plain.size(), key_switches, key_switches / (double)B, 2 * B, paired.size());
        for (auto &kv : expect)
            if (!paired.count(kv.first) || paired[kv.first] != kv.second)
                printf("  differs: %s L=%d expected %ld, got %ld\n", kv.first.first.c_str(), kv.first.second, kv.second,
                       paired.count(kv.first) ? paired[kv.first] : 0L);
        for (auto &kv : paired)
            if (!expect.count(kv.first)) printf("  unexpected: %s L=%d %ld\n", kv.first.first.c_str(), kv.first.second, kv.second);
        CHECK(paired == expect);
        CHECK(census_total(paired, "modraise") == (long)B);
    }

    // ---- 6: determinism where it is promised
    {
        printf("6: determinism\n");
        const int P = 4;
        vector<Ciphertext> in(2 * P);
        vector<vector<complex<double>>> msgs(2 * P);
        for (int i = 0; i < 2 * P; i++) s.fresh(rng, Nh, 0.02, msgs[i], in[i]);
        Ciphertext a = in[0], b = in[1], oa, ob;
        boot.bootstrap_real_pair_3(oa, ob, a, b);
        vector<Ciphertext> copy = in, many;
        boot.bootstrap_real_many_3(many, copy);
        CHECK(many.size() == (size_t)(2 * P) && many[0].download() == oa.download() && many[1].download() == ob.download());
        // an odd count: the last member has the bits of a single real call
        copy.assign(in.begin(), in.begin() + 3);
        boot.bootstrap_real_many_3(many, copy);
        Ciphertext last = in[2], last_out;
        boot.bootstrap_full_real_3(last_out, last);
        CHECK(many.size() == 3 && many[0].download() == oa.download() && many[2].download() == last_out.download());

        // gathered bootstrap_real_3 calls
        const int total = 8;
        vector<Ciphertext> alone(total), gathered(total);
        for (int i = 0; i < total; i++)
        {
            Ciphertext c = in[i];
            boot.bootstrap_full_real_3(alone[i], c);
        }
        const auto before = boot.gather_statistics();
#pragma omp parallel num_threads(total)
        {
            const int t = omp_get_thread_num();
#pragma omp barrier
            Ciphertext c = in[t];
            boot.bootstrap_real_3(gathered[t], c);
        }
        const auto after = boot.gather_statistics();
        const size_t runs = after.first - before.first, members = after.second - before.second;
        printf("  %d concurrent bootstrap_real_3 calls in %zu packed runs\n", total, runs);
        CHECK(members == (size_t)total && runs < members);
        for (int i = 0; i < total; i++) CHECK(gathered[i].download() == alone[i].download());

        // a real and a complex call arriving together: two packs, each with the bits of its single call
        Ciphertext cplx_in = in[1], cplx_alone;
        boot.bootstrap_full_3(cplx_alone, cplx_in);
        const auto b2 = boot.gather_statistics();
        Ciphertext in_r = in[0], in_c = in[1], out_r, out_c;
        std::thread tr([&] { boot.bootstrap_real_3(out_r, in_r); });
        const double t_wait = now_s();
        while (boot.gather_pending() == 0 && now_s() - t_wait < 5.0) std::this_thread::sleep_for(std::chrono::microseconds(200));
        std::thread tc([&] { boot.bootstrap_3(out_c, in_c); });
        tr.join();
        tc.join();
        const auto a2 = boot.gather_statistics();
        printf("  real and complex together: %zu runs for %zu ciphertexts\n", a2.first - b2.first, a2.second - b2.second);
        CHECK(a2.second - b2.second == 2 && a2.first - b2.first == 2);
        CHECK(out_r.download() == alone[0].download());
        CHECK(out_c.download() == cplx_alone.download());
    }

    // ---- 7: opt-in pairing of gathered calls
    {
        printf("7: opt-in pairing\n");
        const int total = 8;
        vector<Ciphertext> in(total), unchanged(total);
        vector<vector<complex<double>>> msgs(total);
        for (int i = 0; i < total; i++) s.fresh(rng, Nh, 0.02, msgs[i], in[i]);
        for (int i = 0; i < total; i++)
        {
            Ciphertext c = in[i];
            boot.bootstrap_full_3(unchanged[i], c);
        }
        auto concurrent = [&](int count, vector<Ciphertext> &out) {
            out.assign((size_t)count, Ciphertext());
#pragma omp parallel num_threads(count)
            {
                const int t = omp_get_thread_num();
#pragma omp barrier
                Ciphertext c = in[t];
                boot.bootstrap_3(out[t], c);
            }
        };
        vector<Ciphertext> out;
        // off (the default): the bits of bootstrap_full_3
        CHECK(!boot.pair_real);
        concurrent(total, out);
        for (int i = 0; i < total; i++) CHECK(out[i].download() == unchanged[i].download());
        // on
        boot.pair_real = true;
        auto before = boot.gather_statistics();
        s.context->sync();
        moai_op_trace(1);
        concurrent(total, out);
        Census c8 = census_stop();
        auto after = boot.gather_statistics();
        double worst = 0;
        for (int i = 0; i < total; i++) worst = max(worst, s.error(out[i], msgs[i]));
        printf("  %d gathered bootstrap_3 calls, pairing on: %zu runs, %zu members, %ld ciphertexts raised, worst error %.2e\n", total,
               after.first - before.first, after.second - before.second, census_total(c8, "modraise"), worst);
        CHECK(after.second - before.second == (size_t)total);
        CHECK(census_total(c8, "modraise") == total / 2); // the bootstrap work of 4
        CHECK(census_total(c8, "real_split") == total);   // polynomials: 4 pairs
        CHECK(worst < bound);
        for (int i = 0; i < total; i++) check_shape(out[i]);
        // an odd count completes; the odd one out goes through the single real sequence
        moai_op_trace(1);
        concurrent(7, out);
        Census c7 = census_stop();
        worst = 0;
        for (int i = 0; i < 7; i++) worst = max(worst, s.error(out[i], msgs[i]));
        printf("  7 calls: %ld ciphertexts raised, worst error %.2e\n", census_total(c7, "modraise"), worst);
        CHECK(census_total(c7, "modraise") >= 4 && census_total(c7, "modraise") < 7);
        CHECK(worst < bound);
        boot.pair_real = false;
        concurrent(2, out);
        CHECK(out[0].download() == unchanged[0].download() && out[1].download() == unchanged[1].download());
    }

    // ---- 8: refusals, before anything is enqueued
    {
        printf("8: refusals\n");
        vector<complex<double>> m;
        Ciphertext low, topct, other_scale, three;
        s.fresh(rng, Nh, 0.02, m, low);
        s.fresh(rng, Nh, 0.02, m, topct, true);
        other_scale = low;
        other_scale.scale() = low.scale() * 2;
        Ciphertext packed = moai_fused::pack({ low, low }, *s.context), out;
        s.context->sync();
        moai_op_trace(1);
        CHECK(throws([&] { moai_fused::pair_real(*s.context, low, topct, out); }, "level"));
        CHECK(throws([&] { moai_fused::pair_real(*s.context, low, other_scale, out); }, "scale"));
        CHECK(throws([&] { moai_fused::pair_real(*s.context, low, packed, out); }, "batch"));
        Ciphertext coeff = low;
        s.evaluator->transform_from_ntt_inplace(coeff);
        Census c = census_stop();
        CHECK(census_total(c, "mul_i_add") == 0);
        CHECK(throws([&] { moai_fused::pair_real(*s.context, low, coeff, out); }, "NTT"));
        Ciphertext oa, ob, ca = low, cb = topct;
        CHECK(throws([&] { boot.bootstrap_real_pair_3(oa, ob, ca, cb); }));
        CHECK(throws([&] { boot.bootstrap(oa, ca); }, "not provided")); // the two-level family still is not
    }
}

int main(int argc, char **argv)
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    setenv("MOAI_BOOT_COMBINE_US", "400000", 0); // as tests/cpp/test_bootstrap_real.cpp: grouping independent of host load
    const string mode = argc > 1 ? argv[1] : "";
    if (mode == "--full")
    {
        run(16, 20, { 12, 15 }, 12, 8);
    }
    else
    {
        run(11, 2, { 7, 9, 10 }, 9, 8);
    }
    printf("%d checks, %d failed\n", g_checks, g_fail);
    if (!g_fail)
    {
        printf("ALL OK\n");
    }
    return g_fail ? 1 : 0;
}
