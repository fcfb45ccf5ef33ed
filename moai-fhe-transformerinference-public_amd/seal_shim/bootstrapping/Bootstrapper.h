// bootstrapping/Bootstrapper.h -- GPU-backed drop-in for MOAI's include/source/bootstrapping/Bootstrapper.h, so that
// softmax.hpp, single_att_block.hpp and the drivers under include/test compile UNCHANGED against seal_shim/
// (add -I<package>/seal_shim/bootstrapping in place of the reference's include/source/bootstrapping).
//
// Interface kept (Bootstrapper.h:14-221, Bootstrapper.cpp): the constructor of :52-69, the public data members, and the
// "level-3" full-slot family MOAI's drivers use --
//   prepare_mod_polynomial (:1973-1977), addLeftRotKeys_Linear_to_vector_3 (:89-184), addBootKeys_3 (:374-392),
//   change_logn (:508-520), genorigcoeff/genfftcoeff_3/geninvfftcoeff_3 through generate_LT_coefficient_3 (:1967-1971),
//   bsgs_linear_transform / rotated_bsgs_linear_transform (:1997-2129), sflinv_full_3 / sfl_full_3 (:2602-2623, :2460-2497),
//   coefftoslot_full_3 / slottocoeff_full_3 (:2742-2777), modraise_inplace (:2938-2992), bootstrap_full_3 (:3231-3251),
//   bootstrap_3 / bootstrap_inplace_3 (:3496-3508), set_final_scale,
//   and the sparse-slot family for 3 <= logn < logNh: the sparse branches of genfftcoeff_3 / geninvfftcoeff_3
//   (:1298-1414, :1694-1817), bootstrap_sparse_3 (:3143-3229; sub-sum, coefftoslot_3, ONE modular reduction,
//   slottocoeff_3).  slot_vec may hold several logn values; change_logn picks one;
//   and the "real" variants of both: sfl_full_half_3 / sfl_half_3 (:2539-2577, :2499-2537), slottocoeff_full_half_3 /
//   slottocoeff_half_3 (:2778-2795, :2735-2740), bootstrap_full_real_3 (:3328-3351), bootstrap_sparse_real_3 (:3253-3326),
//   bootstrap_real_3 / bootstrap_inplace_real_3 (:3510-3522).
// Added (no counterpart in the reference): bootstrap_real_pair_3 / bootstrap_real_many_3 and the opt-in `pair_real`, which
// send TWO real-valued ciphertexts through one bootstrap as a + i b (see `pair_real` below for what the caller promises).
// Not provided: the two-level, one-depth and hoisting variants, which no MOAI driver calls, and the sparse
// logn = 0 (multiply_vector) branch and logn = 1, 2 (the level-3 split leaves a part of 0 bits); they throw.
// Keys of a sparse caller: addBootKeys_3 lists every power of two below Nh, which covers the sub-sum's steps n 2^i and
// slottocoeff_3's rotation by n; addLeftRotKeys_Linear_to_vector_3 (:89-184) lists neither, so a caller that builds
// its own key list from that routine alone must add the steps 2^i, logn <= i < logNh (as the reference's would).
//
// What is different inside:
//  * no NTL: the modular-reduction polynomial comes from bootstrapping/moai_remez.h, the transform diagonals from
//    bootstrapping/moai_fft_diagonals.h (both re-derived; see those files for what pins them);
//  * the evaluation runs on the device through seal/moai_bootstrap_eval.h: ONE engine class, PackedBootstrapper3, for full
//    and sparse slots alike, one instance per logn of slot_vec built on first use (engine_for) and dropped, with the cached
//    transforms of bsgs_linear_transform, whenever the sets or final_scale change (reset_engines).  It issues the evaluator
//    calls of the reference's routines in their order, with the plaintext diagonals encoded once per (level, scale) and
//    cached, and holds no per-call state: the forwards with the reference's names pass the member initial_scale along;
//  * bootstrap_3 is what MOAI calls from its OpenMP loops, one ciphertext per call (include/test/test_full_scheme.hpp:
//    654-660).  Concurrent callers are gathered into ONE packed run (leader / followers, bounded waits): every ciphertext
//    gets exactly the result of its own call -- the packed kernels compute each member independently, bit-identical to
//    a single-ciphertext run (tests/cpp/test_bootstrap_real.cpp) -- but the device sees batches of the caller count.
//    MOAI_BOOT_COMBINE_US sets the gathering window (default 8000 us -- a caller without company waits a quarter of it, 0.1 % of
//    a packed run and 1.5 % of a single bootstrap; 0 = never gather), MOAI_BOOT_MAX_PACK the
//    largest pack (default 48).
#pragma once

#include <chrono>
#include <cmath>
#include <complex>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>
#include <tuple>

#include "ModularReducer.h"
#include "moai_fft_diagonals.h"
#include "seal/moai_bootstrap_eval.h"

// the reference's header opens these namespaces for everything that includes it (Bootstrapper.h:10-12); MOAI's
// headers rely on that
using namespace std;
using namespace seal;
using namespace seal::util;

class Bootstrapper
{
public:
    long loge;
    long logn;
    long n;
    long logNh;
    long Nh;
    long L;

    double initial_scale = 1.0;
    double final_scale;

    long boundary_K;
    long sin_cos_deg;
    long scale_factor;
    long inverse_deg;

    SEALContext &context;
    KeyGenerator &keygen;
    CKKSEncoder &encoder;
    Encryptor &encryptor;
    Decryptor &decryptor;
    Evaluator &evaluator;
    RelinKeys &relin_keys;
    GaloisKeys &gal_keys;

    vector<long> slot_vec;
    long slot_index = 0;
    // [slot index][diagonal][slot], the reference's layout (Bootstrapper.h:43-46)
    vector<vector<vector<complex<double>>>> fftcoeff1, fftcoeff2, fftcoeff3;
    vector<vector<vector<complex<double>>>> invfftcoeff1, invfftcoeff2, invfftcoeff3;

    ModularReducer *mod_reducer;

    // Opt-in (default false; true when MOAI_BOOT_PAIR_REAL=1 is in the environment at construction): the caller promises that
    // EVERY ciphertext handed to bootstrap_3 / bootstrap_real_3 of this object encodes real values.  Gathered calls are then
    // paired in queue order, each pair goes through ONE bootstrap as a + i b (bootstrap_real_pair_3), and an odd one out
    // goes through the single real sequence.  What changes for the caller:
    //  * a result depends on its partner: it is no longer bit-identical to a single call, only equal to it within the
    //    bootstrap's accuracy (tests/cpp_real/test_bootstrap_real_pair.cpp prints single and paired errors side by side);
    //  * the message the modular reduction sees is a + i b, |a + i b| <= sqrt(2) max(|a|, |b|): its sine approximation's
    //    cubic error term grows accordingly and carries a little of b into a's result (DESIGN 5.0d has the table);
    //  * an input that is NOT real leaks its imaginary part into its partner's result.
    // Measured at N = 2^16 on MOAI's chain, full slots, real messages of magnitude 1.0 (tests/cpp_real/test_bootstrap_real_pair
    // --full): max |error| 1.33e-5 and 1.38e-5 for the two members of a pair, against 1.16e-5 and 1.05e-5 for the same two
    // ciphertexts through bootstrap_real_3 alone; at magnitude 0.02: 7.9e-6 / 1.03e-5 paired, 8.6e-6 / 7.7e-6 alone.  That
    // -- an error of up to about 1.4e-5 at magnitude 1, up to 2.2 x the single call's -- is what a caller accepts by setting it.
    // With the flag clear nothing about bootstrap_3 changes.
    bool pair_real = false;

    Bootstrapper(long _loge, long _logn, long _logNh, long _L, double _final_scale, long _boundary_K, long _sin_cos_deg,
                 long _scale_factor, long _inverse_deg, SEALContext &_context, KeyGenerator &_keygen, CKKSEncoder &_encoder,
                 Encryptor &_encryptor, Decryptor &_decryptor, Evaluator &_evaluator, RelinKeys &_relin_keys, GaloisKeys &_gal_keys)
        : loge(_loge), logn(_logn), logNh(_logNh), L(_L), final_scale(_final_scale), boundary_K(_boundary_K),
          sin_cos_deg(_sin_cos_deg), scale_factor(_scale_factor), inverse_deg(_inverse_deg), context(_context), keygen(_keygen),
          encoder(_encoder), encryptor(_encryptor), decryptor(_decryptor), evaluator(_evaluator), relin_keys(_relin_keys),
          gal_keys(_gal_keys)
    {
        n = 1 << logn;
        Nh = 1 << logNh;
        mod_reducer = new ModularReducer(boundary_K, static_cast<double>(loge), sin_cos_deg, scale_factor, inverse_deg, context, encoder,
                                         encryptor, evaluator, relin_keys, decryptor);
        const char *e = std::getenv("MOAI_BOOT_COMBINE_US");
        combine_us_ = e ? std::atol(e) : 8000;
        e = std::getenv("MOAI_BOOT_MAX_PACK");
        max_pack_ = e ? static_cast<std::size_t>(std::atol(e)) : 48;
        if (max_pack_ < 1)
        {
            max_pack_ = 1;
        }
        e = std::getenv("MOAI_BOOT_PAIR_REAL");
        pair_real = e && std::atol(e) == 1;
    }
    Bootstrapper(const Bootstrapper &) = delete;
    Bootstrapper &operator=(const Bootstrapper &) = delete;
    ~Bootstrapper()
    {
        delete mod_reducer;
    }

    inline void set_final_scale(double _final_scale)
    {
        std::lock_guard<std::mutex> run(run_mu_); // not while a bootstrap holds a reference to the engine
        final_scale = _final_scale;
        reset_engines();
    }

    // ---- keys ------------------------------------------------------------------------------------------------------
    void addLeftRotKeys_Linear_to_vector_3(vector<int> &gal_steps_vector)
    {
        moai_fused::boot_rotation_steps_3(static_cast<int>(logn), static_cast<int>(logNh), gal_steps_vector);
    }
    void addBootKeys_3(GaloisKeys &keys)
    {
        vector<int> gal_steps_vector;
        gal_steps_vector.push_back(0);
        for (int i = 0; i < logNh; i++)
        {
            gal_steps_vector.push_back((1 << i));
        }
        addLeftRotKeys_Linear_to_vector_3(gal_steps_vector);
        keygen.create_galois_keys(gal_steps_vector, keys);
        slot_vec.push_back(logn);
        select_slot_index();
    }
    void change_logn(long new_logn)
    {
        std::lock_guard<std::mutex> run(run_mu_); // not while a bootstrap holds a reference to the engine
        logn = new_logn;
        n = (1 << logn);
        select_slot_index(); // the engines are built per logn from slot_vec: none depends on the current one
    }

    // ---- constants -------------------------------------------------------------------------------------------------
    void prepare_mod_polynomial()
    {
        mod_reducer->generate_sin_cos_polynomial();
        mod_reducer->generate_inverse_sine_polynomial();
    }
    // the per-stage matrices live inside moai_fft_diagonals.h; kept as an entry point for callers of the reference's name
    void genorigcoeff()
    {
    }
    void genfftcoeff_3()
    {
        generate_sets(true, false);
    }
    void geninvfftcoeff_3()
    {
        generate_sets(false, true);
    }
    void generate_LT_coefficient_3()
    {
        genorigcoeff();
        generate_sets(true, true);
    }

    // ---- linear transforms (one ciphertext or a pack) ---------------------------------------------------------------
    void bsgs_linear_transform(Ciphertext &rtncipher, Ciphertext &cipher, int totlen, int basicstep, int coeff_logn,
                               const vector<vector<complex<double>>> &fftcoeff)
    {
        transform(false, totlen, basicstep, coeff_logn, fftcoeff).apply(cipher, rtncipher, gal_keys);
    }
    void rotated_bsgs_linear_transform(Ciphertext &rtncipher, Ciphertext &cipher, int totlen, int basicstep, int coeff_logn,
                                       const vector<vector<complex<double>>> &fftcoeff)
    {
        transform(true, totlen, basicstep, coeff_logn, fftcoeff).apply(cipher, rtncipher, gal_keys);
    }
    // the reference's names for the stages, on the current logn; those that rescale the third forward set read the member
    // initial_scale, as the reference's do
    void sflinv_full_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        engine().sflinv(rtncipher, cipher);
    }
    void sfl_full_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        engine().sfl(rtncipher, cipher, false, initial_scale);
    }
    void coefftoslot_full_3(Ciphertext &rtncipher1, Ciphertext &rtncipher2, Ciphertext &cipher)
    {
        engine().coefftoslot_full_3(rtncipher1, rtncipher2, cipher);
    }
    void slottocoeff_full_3(Ciphertext &rtncipher, Ciphertext &cipher1, Ciphertext &cipher2)
    {
        engine().slottocoeff_full_3(rtncipher, cipher1, cipher2, false, initial_scale);
    }
    void sfl_full_half_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        engine().sfl(rtncipher, cipher, true, initial_scale);
    }
    void slottocoeff_full_half_3(Ciphertext &rtncipher, Ciphertext &cipher1, Ciphertext &cipher2)
    {
        engine().slottocoeff_full_3(rtncipher, cipher1, cipher2, true, initial_scale);
    }
    // the sparse counterparts (3 <= logn < logNh)
    void sfl_half_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        sparse_engine().sfl(rtncipher, cipher, true, initial_scale);
    }
    void slottocoeff_half_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        sparse_engine().slottocoeff_3(rtncipher, cipher, true, initial_scale);
    }
    void modraise_inplace(Ciphertext &cipher)
    {
        engine().modraise_inplace(cipher);
    }

    // ---- the bootstrap ----------------------------------------------------------------------------------------------
    // one packed (or single) ciphertext straight through the pipeline; `cipher` is consumed like the reference's
    void bootstrap_full_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        std::lock_guard<std::mutex> run(run_mu_);
        engine().bootstrap_3(rtncipher, cipher);
    }
    // 3 <= logn < logNh; `cipher` is consumed like the reference's
    void bootstrap_sparse_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        std::lock_guard<std::mutex> run(run_mu_);
        sparse_engine().bootstrap_3(rtncipher, cipher);
    }
    void bootstrap_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        const long ln = enter(cipher);
        if (cipher.batch() != 1 || combine_us_ <= 0 || max_pack_ == 1)
        {
            std::lock_guard<std::mutex> run(run_mu_);
            boot_single(ln, KIND_COMPLEX, rtncipher, cipher);
            return;
        }
        gather_and_run(rtncipher, cipher, ln, pair_real ? KIND_PAIR : KIND_COMPLEX);
    }
    void bootstrap_inplace_3(Ciphertext &cipher)
    {
        Ciphertext rtncipher;
        bootstrap_3(rtncipher, cipher);
        cipher = rtncipher;
    }

    // ---- the real variants: the result encodes the real part of the message (:3328-3351, :3253-3326, :3510-3522) -------
    void bootstrap_full_real_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        std::lock_guard<std::mutex> run(run_mu_);
        engine().bootstrap_real_3(rtncipher, cipher);
    }
    void bootstrap_sparse_real_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        std::lock_guard<std::mutex> run(run_mu_);
        sparse_engine().bootstrap_real_3(rtncipher, cipher);
    }
    // concurrent callers are gathered like bootstrap_3's; real and complex requests never share a pack, and a gathered real
    // call has the bits of a single real call (unless `pair_real` is set, see there)
    void bootstrap_real_3(Ciphertext &rtncipher, Ciphertext &cipher)
    {
        const long ln = enter(cipher);
        if (cipher.batch() != 1 || combine_us_ <= 0 || max_pack_ == 1)
        {
            std::lock_guard<std::mutex> run(run_mu_);
            boot_single(ln, KIND_REAL, rtncipher, cipher);
            return;
        }
        gather_and_run(rtncipher, cipher, ln, pair_real ? KIND_PAIR : KIND_REAL);
    }
    void bootstrap_inplace_real_3(Ciphertext &cipher)
    {
        Ciphertext rtncipher;
        bootstrap_real_3(rtncipher, cipher);
        cipher = rtncipher;
    }
    // Two real-valued ciphertexts (single or packed alike, same level and scale) through ONE bootstrap; both inputs are
    // consumed like bootstrap_3's.  Outputs at final_scale, on the level bootstrap_3 leaves.  See `pair_real` above for
    // what pairing means for accuracy.
    void bootstrap_real_pair_3(Ciphertext &rtn_a, Ciphertext &rtn_b, Ciphertext &a, Ciphertext &b)
    {
        const long ln = enter(a);
        std::lock_guard<std::mutex> run(run_mu_);
        engine_for(ln).bootstrap_real_pair_3(rtn_a, rtn_b, a, b);
    }
    // in[2j] is paired with in[2j + 1]; the pairs run in packs of at most MOAI_BOOT_MAX_PACK pairs, an odd last member goes
    // through the single real sequence.  All inputs on one level, with one scale; they are consumed.
    void bootstrap_real_many_3(vector<Ciphertext> &rtn, vector<Ciphertext> &in)
    {
        if (in.empty())
        {
            rtn.clear();
            return;
        }
        const long ln = enter(in[0]);
        for (auto &c : in)
        {
            if (c.batch() != 1 || c.parms_id() != in[0].parms_id() || c.scale() != in[0].scale() || c.size() != in[0].size() ||
                c.is_ntt_form() != in[0].is_ntt_form())
            {
                throw std::invalid_argument("bootstrap_real_many_3: single ciphertexts of one level, size, form and scale");
            }
        }
        std::vector<Ciphertext *> ins, outs;
        std::vector<Ciphertext> result(in.size());
        for (std::size_t i = 0; i < in.size(); i++)
        {
            ins.push_back(&in[i]);
            outs.push_back(&result[i]);
        }
        std::lock_guard<std::mutex> run(run_mu_);
        for (std::size_t at = 0; at < in.size(); at += 2 * max_pack_)
        {
            const std::size_t cnt = std::min(in.size() - at, 2 * max_pack_);
            run_paired(ln, ins.data() + at, outs.data() + at, cnt);
            runs_++;
            members_ += cnt;
        }
        rtn = std::move(result);
    }
    // calls waiting to be gathered into a pack (a caller that must know its call is queued, e.g. before change_logn)
    std::size_t gather_pending() const
    {
        std::lock_guard<std::mutex> g(gather_mu_);
        return pending_.size();
    }
    // how the calls of this object were grouped so far: {packed runs, ciphertexts}
    std::pair<std::size_t, std::size_t> gather_statistics() const
    {
        std::lock_guard<std::mutex> run(run_mu_);
        return { runs_, members_ };
    }

    // the variants no MOAI driver calls
    void bootstrap(Ciphertext &, Ciphertext &)
    {
        unsupported("bootstrap");
    }
    void bootstrap_inplace(Ciphertext &)
    {
        unsupported("bootstrap_inplace");
    }
    void bootstrap_hoisting(Ciphertext &, Ciphertext &)
    {
        unsupported("bootstrap_hoisting");
    }
    void generate_LT_coefficient()
    {
        unsupported("generate_LT_coefficient");
    }
    void addBootKeys(GaloisKeys &)
    {
        unsupported("addBootKeys");
    }

private:
    [[noreturn]] static void unsupported(const char *what)
    {
        throw std::logic_error(std::string("Bootstrapper::") + what + " is not provided: only the level-3 family (bootstrap_3, bootstrap_real_3 and what they call) is");
    }
    void select_slot_index()
    {
        slot_index = -1;
        for (std::size_t i = 0; i < slot_vec.size(); i++)
        {
            if (slot_vec[i] == logn)
            {
                slot_index = static_cast<long>(i);
                break;
            }
        }
        if (slot_index == -1)
        {
            throw std::invalid_argument("LT coefficients were not generated for this logn");
        }
    }
    void check_sparse(long ln) const
    {
        if (const char *why = moai_boot::sparse_unsupported_reason(static_cast<int>(ln), static_cast<int>(logNh)))
        {
            throw std::invalid_argument(std::string("bootstrap_sparse_3: ") + why);
        }
    }
    void generate_sets(bool forward, bool inverse)
    {
        auto size_to = [&](vector<vector<vector<complex<double>>>> &v) { v.resize(slot_vec.size()); };
        size_to(fftcoeff1);
        size_to(fftcoeff2);
        size_to(fftcoeff3);
        size_to(invfftcoeff1);
        size_to(invfftcoeff2);
        size_to(invfftcoeff3);
        for (std::size_t u = 0; u < slot_vec.size(); u++)
        {
            if (slot_vec[u] != logNh)
            {
                check_sparse(slot_vec[u]);
            }
            moai_boot::LevelThreeDiagonals d =
                slot_vec[u] == logNh ? moai_boot::level_three_diagonals(static_cast<int>(slot_vec[u]), boundary_K)
                                     : moai_boot::level_three_sparse_diagonals(static_cast<int>(slot_vec[u]), static_cast<int>(logNh), boundary_K);
            if (forward)
            {
                fftcoeff1[u] = std::move(d.fftcoeff1);
                fftcoeff2[u] = std::move(d.fftcoeff2);
                fftcoeff3[u] = std::move(d.fftcoeff3);
            }
            if (inverse)
            {
                invfftcoeff1[u] = std::move(d.invfftcoeff1);
                invfftcoeff2[u] = std::move(d.invfftcoeff2);
                invfftcoeff3[u] = std::move(d.invfftcoeff3);
            }
        }
        reset_engines();
    }
    // The engines hold copies of the sets and final_scale; the transforms behind bsgs_linear_transform are keyed by the
    // ADDRESS of a set, whose contents generate_sets replaces: both go when either input changes.
    void reset_engines()
    {
        std::lock_guard<std::mutex> g(engine_mu_);
        engines_.clear();
        transforms_.clear();
    }
    // what every bootstrap entry point does first: the reference writes the member initial_scale from every calling thread
    // as well (:3497, :3511), and a sparse logn without a level-3 bootstrapping is refused before anything is enqueued.
    // Returns the logn of this call.
    long enter(const Ciphertext &cipher)
    {
        initial_scale = cipher.scale();
        const long ln = logn;
        if (ln != logNh)
        {
            check_sparse(ln);
        }
        return ln;
    }

    // The pipeline of slot_vec's entry `ln`, full slots (ln == logNh) or sparse, built on first use.  Independent of the
    // current logn, so a gathered call runs on the engine of its own logn whatever change_logn did meanwhile.
    moai_fused::PackedBootstrapper3 &engine_for(long ln)
    {
        if (ln != logNh)
        {
            check_sparse(ln);
        }
        std::lock_guard<std::mutex> g(engine_mu_);
        auto &e = engines_[ln];
        if (!e)
        {
            e.reset(new moai_fused::PackedBootstrapper3(context, encoder, evaluator, relin_keys, gal_keys, static_cast<int>(ln),
                                                        static_cast<int>(logNh), final_scale, diagonals_of(ln), mod_reducer->packed_reducer()));
        }
        return *e;
    }
    // the full-slot pipeline behind the reference's member-logn entry points (sflinv_full_3 ... bootstrap_full_3)
    moai_fused::PackedBootstrapper3 &engine()
    {
        if (logn != logNh)
        {
            throw std::logic_error("only logn == logNh is provided");
        }
        return engine_for(logNh);
    }
    // its counterpart behind the sparse names (bootstrap_sparse_3, sfl_half_3, ...)
    moai_fused::PackedBootstrapper3 &sparse_engine()
    {
        check_sparse(logn);
        return engine_for(logn);
    }
    // the six sets of slot_vec's entry `ln` (caller holds engine_mu_)
    moai_fused::BootDiagonals3 diagonals_of(long ln) const
    {
        std::size_t u = slot_vec.size();
        for (std::size_t i = 0; i < slot_vec.size(); i++)
        {
            if (slot_vec[i] == ln)
            {
                u = i;
                break;
            }
        }
        if (u == slot_vec.size())
        {
            throw std::invalid_argument("LT coefficients were not generated for this logn");
        }
        if (fftcoeff1.size() <= u || invfftcoeff1.size() <= u || fftcoeff1[u].empty() || invfftcoeff1[u].empty())
        {
            throw std::logic_error("generate_LT_coefficient_3() has not run");
        }
        return { fftcoeff1[u], fftcoeff2[u], fftcoeff3[u], invfftcoeff1[u], invfftcoeff2[u], invfftcoeff3[u] };
    }
    moai_fused::BsgsLinearTransform &transform(bool rotated, int totlen, int basicstep, int coeff_logn,
                                               const vector<vector<complex<double>>> &fftcoeff)
    {
        std::lock_guard<std::mutex> g(engine_mu_);
        auto key = std::make_tuple(static_cast<const void *>(&fftcoeff), rotated, totlen, basicstep, coeff_logn);
        auto it = transforms_.find(key);
        if (it == transforms_.end())
        {
            it = transforms_
                     .emplace(key, std::unique_ptr<moai_fused::BsgsLinearTransform>(new moai_fused::BsgsLinearTransform(
                                       context, static_cast<int>(Nh), totlen, basicstep, coeff_logn, fftcoeff, rotated)))
                     .first;
        }
        return *it->second;
    }

    // ---- one run on the engine of `ln` (caller holds run_mu_) ---------------------------------------------------------
    enum Kind
    {
        KIND_COMPLEX, // bootstrap_3
        KIND_REAL,    // bootstrap_real_3
        KIND_PAIR     // either, with `pair_real` set: real by the caller's promise, paired two to a bootstrap
    };
    void boot_single(long ln, Kind kind, Ciphertext &out, Ciphertext &in)
    {
        auto &e = engine_for(ln);
        kind == KIND_COMPLEX ? e.bootstrap_3(out, in) : e.bootstrap_real_3(out, in);
    }
    // in[2j] with in[2j + 1] as one packed paired run, an odd last member through the single real sequence
    void run_paired(long ln, Ciphertext *const *in, Ciphertext *const *out, std::size_t count)
    {
        const std::size_t pairs = count / 2;
        if (pairs == 1)
        {
            Ciphertext oa, ob;
            engine_for(ln).bootstrap_real_pair_3(oa, ob, *in[0], *in[1]);
            *out[0] = std::move(oa);
            *out[1] = std::move(ob);
        }
        else if (pairs > 1)
        {
            std::vector<Ciphertext> first, second;
            first.reserve(pairs);
            second.reserve(pairs);
            for (std::size_t j = 0; j < pairs; j++)
            {
                first.push_back(*in[2 * j]);
                second.push_back(*in[2 * j + 1]);
            }
            Ciphertext pa = moai_fused::pack(first, context), pb = moai_fused::pack(second, context), oa, ob;
            first.clear();
            second.clear();
            engine_for(ln).bootstrap_real_pair_3(oa, ob, pa, pb);
            moai_fused::unpack(oa, context, first);
            moai_fused::unpack(ob, context, second);
            for (std::size_t j = 0; j < pairs; j++)
            {
                *out[2 * j] = std::move(first[j]);
                *out[2 * j + 1] = std::move(second[j]);
            }
        }
        if (count & 1)
        {
            Ciphertext o;
            boot_single(ln, KIND_REAL, o, *in[count - 1]);
            *out[count - 1] = std::move(o);
        }
    }

    // ---- gathering of concurrent bootstrap_3 / bootstrap_real_3 calls ---------------------------------------------------
    struct Request
    {
        Ciphertext *out;
        Ciphertext *in;
        long logn; // the caller's logn: calls with different logn, or sparse and full ones, never share a pack
        Kind kind; // nor do calls of different kinds
        bool done = false;
        std::exception_ptr error;
    };
    // Every caller queues its request; the caller at the head of the queue leads ONE packed run (its own request is part
    // of it), the others sleep until their request is done or they reach the head.  All waits end: a leader's wait for
    // company is bounded by the window, and a finished run always wakes the queue.
    void gather_and_run(Ciphertext &rtncipher, Ciphertext &cipher, long ln, Kind kind)
    {
        Request me{ &rtncipher, &cipher, ln, kind };
        std::unique_lock<std::mutex> lk(gather_mu_);
        pending_.push_back(&me);
        gather_cv_.notify_all();
        while (!me.done)
        {
            if (leader_active_ || pending_.front() != &me)
            {
                gather_cv_.wait(lk);
                continue;
            }
            leader_active_ = true;
            // wait for company: until the pack is full, nobody new arrived for a quarter of the window, or the window ends
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(combine_us_);
            // with pairing a pack holds max_pack_ PAIRS
            const std::size_t max_take = kind == KIND_PAIR ? 2 * max_pack_ : max_pack_;
            while (pending_.size() < max_take)
            {
                const std::size_t seen = pending_.size();
                auto quiet = std::chrono::steady_clock::now() + std::chrono::microseconds(combine_us_ / 4 + 1);
                if (deadline < quiet)
                {
                    quiet = deadline;
                }
                gather_cv_.wait_until(lk, quiet, [&] { return pending_.size() > seen; });
                if (pending_.size() == seen || std::chrono::steady_clock::now() >= deadline)
                {
                    break;
                }
            }
            const std::size_t take = pending_.size() < max_take ? pending_.size() : max_take;
            std::vector<Request *> batch(pending_.begin(), pending_.begin() + static_cast<std::ptrdiff_t>(take));
            pending_.erase(pending_.begin(), pending_.begin() + static_cast<std::ptrdiff_t>(take));
            lk.unlock();
            // whatever happens in the run (an allocation that fails outside the groups' own try blocks included), the batch is
            // marked done and the queue is woken: no caller may sleep for ever behind a leader that left with an exception
            std::exception_ptr run_error;
            try
            {
                run_batch(batch);
            }
            catch (...)
            {
                run_error = std::current_exception();
            }
            lk.lock();
            for (Request *r : batch)
            {
                if (run_error && !r->error)
                {
                    r->error = run_error;
                }
                r->done = true;
            }
            leader_active_ = false;
            gather_cv_.notify_all();
        }
        lk.unlock();
        if (me.error)
        {
            std::rethrow_exception(me.error);
        }
    }
    // members are grouped by (logn, kind, level, scale); each group is one packed run -- a KIND_PAIR group pairs its members in
    // queue order first
    void run_batch(const std::vector<Request *> &batch)
    {
        std::vector<bool> used(batch.size(), false);
        for (std::size_t i = 0; i < batch.size(); i++)
        {
            if (used[i])
            {
                continue;
            }
            std::vector<std::size_t> group;
            for (std::size_t j = i; j < batch.size(); j++)
            {
                if (!used[j] && batch[j]->logn == batch[i]->logn && batch[j]->kind == batch[i]->kind && batch[j]->in->parms_id() == batch[i]->in->parms_id() && batch[j]->in->scale() == batch[i]->in->scale() &&
                    batch[j]->in->size() == batch[i]->in->size() && batch[j]->in->is_ntt_form() == batch[i]->in->is_ntt_form())
                {
                    group.push_back(j);
                    used[j] = true;
                }
            }
            std::exception_ptr err;
            try
            {
                std::lock_guard<std::mutex> run(run_mu_);
                const long ln = batch[i]->logn;
                const Kind kind = batch[i]->kind;
                auto boot = [&](Ciphertext &out, Ciphertext &in) { boot_single(ln, kind == KIND_PAIR ? KIND_REAL : kind, out, in); };
                if (kind == KIND_PAIR && group.size() > 1)
                {
                    // a group may exceed 2 max_pack_ only if a non-pairing leader took it: keep the packs bounded anyway
                    std::vector<Ciphertext *> ins, outs;
                    for (std::size_t j : group)
                    {
                        ins.push_back(batch[j]->in);
                        outs.push_back(batch[j]->out);
                    }
                    for (std::size_t at = 0; at < ins.size(); at += 2 * max_pack_)
                    {
                        run_paired(ln, ins.data() + at, outs.data() + at, std::min(ins.size() - at, 2 * max_pack_));
                    }
                }
                else if (group.size() == 1)
                {
                    boot(*batch[group[0]]->out, *batch[group[0]]->in);
                }
                else
                {
                    std::vector<Ciphertext> members;
                    members.reserve(group.size());
                    for (std::size_t j : group)
                    {
                        members.push_back(*batch[j]->in);
                    }
                    Ciphertext packed = moai_fused::pack(members, context), packed_out;
                    members.clear();
                    boot(packed_out, packed);
                    std::vector<Ciphertext> outs;
                    moai_fused::unpack(packed_out, context, outs);
                    for (std::size_t g = 0; g < group.size(); g++)
                    {
                        *batch[group[g]]->out = std::move(outs[g]);
                    }
                }
                runs_++;
                members_ += group.size();
            }
            catch (...)
            {
                err = std::current_exception();
            }
            for (std::size_t j : group)
            {
                batch[j]->error = err;
            }
        }
    }

    mutable std::mutex engine_mu_, run_mu_, gather_mu_;
    std::condition_variable gather_cv_;
    std::vector<Request *> pending_;
    bool leader_active_ = false;
    long combine_us_ = 2000;
    std::size_t max_pack_ = 48;
    std::size_t runs_ = 0, members_ = 0;
    std::map<long, std::unique_ptr<moai_fused::PackedBootstrapper3>> engines_; // by logn, full (logNh) and sparse alike
    std::map<std::tuple<const void *, bool, int, int, int>, std::unique_ptr<moai_fused::BsgsLinearTransform>> transforms_;
};
