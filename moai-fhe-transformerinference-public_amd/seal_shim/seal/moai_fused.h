// seal/moai_fused.h -- drop-in replacements for MOAI routines that the device can execute as ONE kernel
// instead of rows*cols evaluator calls.  Same signature, same results (bit-identical ciphertexts).
//
// moai_fused::ct_pt_matrix_mul_wo_pre replaces
// include/source/matrix_mul/Ct_pt_matrix_mul.hpp:4-49 (and the "_large" variant :51-101, which differs
// only in its OpenMP blocking): out[i] = rescale( sum_j multiply_plain(enc_X[j], encode(W[j][i])) ).
//
// moai_fused::ct_ct_matrix_mul_colpacking replaces include/source/matrix_mul/Ct_ct_matrix_mul.hpp:6-56
// (Q K^T): out[i] = rescale(relinearize( sum_j multiply(X[j], rotate(W[j], i * num_batch)) )).
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <map>
#include <memory>

#include "seal/seal.h"

namespace moai_fused
{
    // ---- packed ciphertexts -----------------------------------------------------------------------------------
    // pack(): one seal::Ciphertext holding all of `cts` (same size, level, scale, NTT form) back to back.  Every
    // Evaluator method applied to it performs the operation on each member with the device's batched kernels,
    // so a per-ciphertext MOAI routine called on the pack (gelu_v2, exp, invert_sqrt, eval_odd_deg9_poly, ...)
    // does the work of the OpenMP loop MOAI wraps around it, with the same result for every member bit for
    // bit.  unpack() splits it again.
    inline seal::Ciphertext pack(const std::vector<seal::Ciphertext> &cts, const seal::SEALContext &context)
    {
        using namespace seal;
        if (cts.empty())
        {
            throw std::invalid_argument("nothing to pack");
        }
        const Ciphertext &f = cts[0];
        for (auto &c : cts)
        {
            if (c.parms_id() != f.parms_id() || c.size() != f.size() || c.is_ntt_form() != f.is_ntt_form() ||
                c.scale() != f.scale() || c.batch() != 1)
            {
                throw std::invalid_argument("pack: ciphertexts differ in level, size, form or scale");
            }
        }
        Ciphertext out;
        out.resize_batch(context, f.parms_id(), f.size(), cts.size());
        out.is_ntt_form() = f.is_ntt_form();
        out.scale() = f.scale();
        const std::size_t words = f.size() * f.coeff_modulus_size() * f.poly_modulus_degree();
        for (std::size_t b = 0; b < cts.size(); b++)
        {
            util::hip_check(moai_memcpy_d2d(out.device_data() + b * words, cts[b].device_data(), words * 8, context.stream()));
        }
        return out;
    }
    inline void unpack(const seal::Ciphertext &packed, const seal::SEALContext &context, std::vector<seal::Ciphertext> &cts)
    {
        using namespace seal;
        const std::size_t B = packed.batch();
        std::vector<Ciphertext> out(B);
        const std::size_t words = packed.size() * packed.coeff_modulus_size() * packed.poly_modulus_degree();
        for (std::size_t b = 0; b < B; b++)
        {
            out[b].resize(context, packed.parms_id(), packed.size());
            out[b].is_ntt_form() = packed.is_ntt_form();
            out[b].scale() = packed.scale();
            util::hip_check(moai_memcpy_d2d(out[b].device_data(), packed.device_data() + b * words, words * 8, context.stream()));
        }
        cts = std::move(out);
    }

    // ---- two real ciphertexts in one complex one ----------------------------------------------------------------
    // pair_real(): out = a + i b, the slot-wise constant i being the monomial X^(N/2) -- exact, no level and no scale
    // consumed.  The same residues as the reference's way to multiply by i (encode(i, 1.0), mod_switch_to, multiply_plain:
    // include/source/bootstrapping/Bootstrapper.cpp:2760-2777) followed by add, in one pass over a and b (moai_mul_i_add).
    // a, b (single or packed alike): same level, scale and batch, size 2, NTT form; anything else throws before any work
    // is enqueued.  `out` may be `a` or `b`.
    inline void pair_real(const seal::SEALContext &context, const seal::Ciphertext &a, const seal::Ciphertext &b, seal::Ciphertext &out)
    {
        using namespace seal;
        if (a.size() != 2 || b.size() != 2)
        {
            throw std::invalid_argument("pair_real: ciphertexts of size 2 only");
        }
        if (!a.is_ntt_form() || !b.is_ntt_form())
        {
            throw std::invalid_argument("pair_real: ciphertexts must be in NTT form");
        }
        if (a.parms_id() != b.parms_id())
        {
            throw std::invalid_argument("pair_real: ciphertexts differ in level");
        }
        if (a.scale() != b.scale())
        {
            throw std::invalid_argument("pair_real: ciphertexts differ in scale");
        }
        if (a.batch() != b.batch())
        {
            throw std::invalid_argument("pair_real: ciphertexts differ in batch size");
        }
        if (!context.get_context_data(a.parms_id()))
        {
            throw std::invalid_argument("pair_real: ciphertext is not valid for encryption parameters");
        }
        Ciphertext c;
        c.resize_batch(context, a.parms_id(), 2, a.batch());
        c.is_ntt_form() = true;
        c.scale() = a.scale();
        util::hip_check(moai_mul_i_add(context.device(), a.device_data(), b.device_data(), c.device_data(), 2 * a.batch(),
                                       a.coeff_modulus_size(), 1, context.stream()));
        out = std::move(c);
    }
    // split_real(): for r = a + i b with real a, b:  out_re = r + conj(r) = 2a,  out_im = -i (r - conj(r)) = 2b.  One key switch
    // (the conjugation, Galois element 2N - 1 as in Evaluator::complex_conjugate, SEAL/evaluator.h:1428-1450) and one pass
    // over r and its conjugate (moai_real_split).  Level, scale and form of r.  The outputs may be r itself.
    inline void split_real(const seal::SEALContext &context, const seal::Ciphertext &r, const seal::GaloisKeys &gal_keys,
                           seal::Ciphertext &out_re, seal::Ciphertext &out_im)
    {
        using namespace seal;
        if (r.size() != 2 || !r.is_ntt_form())
        {
            throw std::invalid_argument("split_real: a size-2 ciphertext in NTT form only");
        }
        if (!context.get_context_data(r.parms_id()))
        {
            throw std::invalid_argument("split_real: ciphertext is not valid for encryption parameters");
        }
        if (gal_keys.parms_id() != context.key_parms_id())
        {
            throw std::invalid_argument("galois_keys is not valid for encryption parameters");
        }
        const std::uint32_t elt = static_cast<std::uint32_t>(2 * context.n() - 1);
        if (!gal_keys.has_key(elt))
        {
            throw std::invalid_argument("Galois key not present");
        }
        if (&out_re == &out_im)
        {
            throw std::invalid_argument("split_real: two distinct outputs");
        }
        const std::size_t L = r.coeff_modulus_size(), B = r.batch();
        Ciphertext re, im;
        re.resize_batch(context, r.parms_id(), 2, B);
        im.resize_batch(context, r.parms_id(), 2, B);
        re.is_ntt_form() = im.is_ntt_form() = true;
        re.scale() = im.scale() = r.scale();
        const std::uint64_t *src = r.device_data();
        util::hip_check(moai_apply_galois_to(context.device(), src, im.device_data(), L, elt,
                                             gal_keys.device_key(GaloisKeys::get_index(elt), L), B, context.stream()));
        util::hip_check(moai_real_split(context.device(), src, im.device_data(), re.device_data(), im.device_data(), 2 * B, L,
                                        context.stream()));
        out_re = std::move(re);
        out_im = std::move(im);
    }

    // ---- client output path -----------------------------------------------------------------------------------
    // decrypt_decode(): Decryptor::decrypt then CKKSEncoder::decode of every ciphertext, with the same values bit for
    // bit, for callers that own many ciphertexts (MOAI decrypts all 768 outputs of a layer, test_full_scheme.hpp:1047-1065).
    // Packed ciphertexts (pack() above) are accepted and contribute batch() entries to `out`, in order.  Ciphertexts are
    // grouped by level; per group, the members are decrypted (one moai_decrypt per ciphertext, per packed ciphertext
    // one for all of its members) into one plaintext buffer and decoded by one moai_ckks_decode, then one copy to the
    // host.  A group's plaintext buffer is bounded (1 GiB): larger groups go in chunks.  Synchronises once per chunk.
    template <typename T>
    inline void decrypt_decode(const std::vector<seal::Ciphertext> &cts, const seal::Decryptor &decryptor,
                               const seal::CKKSEncoder &encoder, std::vector<std::vector<T>> &out)
    {
        using namespace seal;
        static_assert(std::is_same<T, double>::value || std::is_same<T, std::complex<double>>::value,
                      "decode to double or std::complex<double>");
        constexpr bool cplx = std::is_same<T, std::complex<double>>::value;
        const SEALContext &context = decryptor.context();
        // the encoder's sparse slot count decides what decode returns (CKKSEncoder::decode)
        const std::size_t n = context.n(), slots = encoder.sparse_slot_count(), full_slots = encoder.slot_count();
        void *st = context.stream();
        struct Member
        {
            const std::uint64_t *ct;
            std::size_t size, L, out;
            double scale;
        };
        std::map<std::size_t, std::vector<Member>> groups; // by level
        std::size_t total = 0;
        for (const Ciphertext &c : cts)
        {
            auto cd = context.get_context_data(c.parms_id());
            if (!cd || c.size() < 2)
            {
                throw std::invalid_argument("encrypted is not valid for encryption parameters");
            }
            if (!c.is_ntt_form())
            {
                throw std::invalid_argument("encrypted must be in NTT form");
            }
            if (c.scale() <= 0 || (static_cast<int>(std::log2(c.scale())) >= cd->total_coeff_modulus_bit_count()))
            {
                throw std::invalid_argument("scale out of bounds");
            }
            const std::size_t L = c.coeff_modulus_size(), words = c.size() * L * n;
            const std::uint64_t *base = c.device_data();
            for (std::size_t b = 0; b < c.batch(); b++)
            {
                groups[L].push_back({ base + b * words, c.size(), L, total++, c.scale() });
            }
        }
        out.assign(total, std::vector<T>());
        const std::size_t per_value = cplx ? 2 : 1;
        std::vector<double> host;
        for (auto &kv : groups)
        {
            const std::size_t L = kv.first;
            const std::vector<Member> &m = kv.second;
            std::size_t chunk = (std::size_t(1) << 30) / (L * n * 8);
            chunk = chunk < 1 ? 1 : chunk;
            for (std::size_t m0 = 0; m0 < m.size(); m0 += chunk)
            {
                const std::size_t nb = std::min(chunk, m.size() - m0);
                util::DeviceArray plain(nb * L * n, st), dout(nb * slots * per_value, st);
                std::vector<double> scales(nb);
                // runs of consecutive members of one packed ciphertext share a launch
                for (std::size_t i = 0; i < nb;)
                {
                    std::size_t j = i + 1;
                    while (j < nb && m[m0 + j].size == m[m0 + i].size &&
                           m[m0 + j].ct == m[m0 + j - 1].ct + m[m0 + i].size * L * n)
                    {
                        j++;
                    }
                    util::hip_check(moai_decrypt(context.device(), m[m0 + i].ct, m[m0 + i].size, decryptor.secret_key_device(),
                                                 plain.get() + i * L * n, j - i, L, nullptr, st));
                    i = j;
                }
                for (std::size_t i = 0; i < nb; i++)
                {
                    scales[i] = m[m0 + i].scale;
                }
                if (slots == full_slots)
                {
                    util::hip_check(moai_ckks_decode(context.device(), plain.get(), nb, L, nullptr, scales.data(), cplx ? 1 : 0,
                                                     reinterpret_cast<double *>(dout.get()), st));
                }
                else
                {
                    util::hip_check(moai_ckks_decode_sparse(context.device(), plain.get(), nb, L, nullptr, scales.data(), slots,
                                                            cplx ? 1 : 0, reinterpret_cast<double *>(dout.get()), st));
                }
                host.resize(nb * slots * per_value);
                util::hip_check(moai_memcpy_d2h(host.data(), dout.get(), host.size() * 8, st));
                context.sync();
                for (std::size_t i = 0; i < nb; i++)
                {
                    std::vector<T> &o = out[m[m0 + i].out];
                    o.resize(slots);
                    std::memcpy(static_cast<void *>(o.data()), host.data() + i * slots * per_value, slots * sizeof(T));
                }
            }
        }
    }

    inline std::vector<seal::Ciphertext> ct_pt_matrix_mul_wo_pre(const std::vector<seal::Ciphertext> &enc_X,
                                                                 const std::vector<std::vector<double>> &W, int col_X,
                                                                 int col_W, int row_W, const seal::SEALContext &seal_context,
                                                                 int computed_cols = -1)
    {
        using namespace seal;
        std::vector<Ciphertext> output(static_cast<std::size_t>(col_W));
        // the "_large" variant of the reference fills only the first 128 * (col_W / 128) columns
        col_W = computed_cols >= 0 ? computed_cols : col_W;
        if (col_W == 0)
        {
            return output;
        }
        if (col_X != row_W)
        {
            std::cout << "ERROR: bad dimensions of X or W. " << std::endl;
            return output;
        }
        const double scale = enc_X[0].scale();
        const parms_id_type pid = enc_X[0].parms_id();
        auto cd = seal_context.get_context_data(pid);
        if (!cd || !cd->next_context_data())
        {
            throw std::invalid_argument("end of modulus switching chain reached");
        }
        const auto &cm = cd->parms().coeff_modulus();
        const std::size_t L = cm.size(), n = seal_context.n();
        const std::size_t rows = static_cast<std::size_t>(row_W), cols = static_cast<std::size_t>(col_W);
        for (std::size_t j = 0; j < rows; j++)
        {
            if (enc_X[j].parms_id() != pid || enc_X[j].size() != 2 || !enc_X[j].is_ntt_form())
            {
                throw std::invalid_argument("encrypted_ntt and plain_ntt parameter mismatch");
            }
        }
        // the scalar plaintexts' residues, exactly as CKKSEncoder::encode(double, parms_id, scale) makes them;
        // output columns in chunks, so that the staging buffers stay within a few GiB however wide W is
        CKKSEncoder encoder(seal_context);
        void *st = seal_context.stream();
        const std::size_t ct_words = 2 * L * n;
        const std::size_t chunk = std::max<std::size_t>(16, std::min<std::size_t>(cols, (std::size_t(4) << 30) / (ct_words * 8)));
        util::DeviceArray dx(rows * ct_words, st), dw(L * rows * chunk, st), dout(chunk * ct_words, st),
            dres(chunk * 2 * (L - 1) * n, st);
        for (std::size_t j = 0; j < rows; j++)
        {
            util::hip_check(moai_memcpy_d2d(dx.get() + j * ct_words, enc_X[j].device_data(), ct_words * 8, st));
        }
        const parms_id_type next_id = cd->next_context_data()->parms_id();
        std::vector<std::uint64_t> w;
        for (std::size_t c0 = 0; c0 < cols; c0 += chunk)
        {
            const std::size_t cc = std::min(chunk, cols - c0);
            w.assign(L * rows * cc, 0);
            for (std::size_t j = 0; j < rows; j++)
            {
                for (std::size_t c = 0; c < cc; c++)
                {
                    Plaintext p;
                    encoder.encode(W[j][c0 + c], pid, enc_X[j].scale(), p);
                    for (std::size_t r = 0; r < L; r++)
                    {
                        w[(r * rows + j) * cc + c] = p.scalar_rows()[r];
                    }
                }
            }
            util::hip_check(moai_memcpy_h2d(dw.get(), w.data(), w.size() * 8, st));
            util::hip_check(moai_ct_pt_matmul(seal_context.device(), dx.get(), dw.get(), dout.get(), rows, cc, 2, L, st));
            util::hip_check(moai_rescale(seal_context.device(), dout.get(), dres.get(), 2, L, cc, st));
            for (std::size_t c = 0; c < cc; c++)
            {
                Ciphertext &o = output[c0 + c];
                o.resize(seal_context, next_id, 2);
                util::hip_check(moai_memcpy_d2d(o.device_data(), dres.get() + c * 2 * (L - 1) * n, 2 * (L - 1) * n * 8, st));
                o.is_ntt_form() = true;
                o.scale() = scale; // Ct_pt_matrix_mul.hpp:41
            }
            seal_context.sync(); // w is refilled for the next chunk
        }
        seal_context.sync(); // w and the staging buffers go out of scope
        return output;
    }
    // include/source/matrix_mul/Ct_pt_matrix_mul.hpp:51-101: the same product with another OpenMP blocking; like
    // the reference it fills the first 128 * (col_W / 128) output columns
    inline std::vector<seal::Ciphertext> ct_pt_matrix_mul_wo_pre_large(const std::vector<seal::Ciphertext> &enc_X,
                                                                       const std::vector<std::vector<double>> &W, int col_X,
                                                                       int col_W, int row_W,
                                                                       const seal::SEALContext &seal_context)
    {
        return ct_pt_matrix_mul_wo_pre(enc_X, W, col_X, col_W, row_W, seal_context, 128 * (col_W / 128));
    }

    // moai_fused::ct_pt_matrix_mul_wo_pre_w_mask replaces include/source/matrix_mul/Ct_pt_matrix_mul.hpp:103-170
    // (self-output and final feed-forward products of the 12-layer run, test_full_scheme.hpp:601,928): every
    // weight is encoded as the VECTOR mask * w -- rows*cols FP64 transforms, which cannot be shared because
    // rounding does not commute with the scaling by w.  Here a column's `rows` plaintexts are produced by one
    // moai_ckks_encode_masked call straight from the weights (nothing but `rows` doubles crosses PCIe), the
    // products and sums of the column are moai_ct_pt_dot passes, and all columns are rescaled in one call.
    // Same ciphertexts bit for bit; like the reference only the first 128 * (col_W / 128) columns are computed.
    inline std::vector<seal::Ciphertext> ct_pt_matrix_mul_wo_pre_w_mask(const std::vector<seal::Ciphertext> &enc_X,
                                                                        const std::vector<std::vector<double>> &W,
                                                                        const std::vector<int> &bias_vec, int col_X,
                                                                        int col_W, int row_W,
                                                                        const seal::SEALContext &seal_context)
    {
        using namespace seal;
        std::vector<Ciphertext> output(static_cast<std::size_t>(col_W));
        if (col_X != row_W)
        {
            std::cout << "ERROR: bad dimensions of X or W. " << std::endl;
            return output;
        }
        const double scale = enc_X[0].scale();
        const parms_id_type pid = enc_X[0].parms_id();
        auto cd = seal_context.get_context_data(pid);
        if (!cd || !cd->next_context_data())
        {
            throw std::invalid_argument("end of modulus switching chain reached");
        }
        const auto &cm = cd->parms().coeff_modulus();
        const std::size_t L = cm.size(), n = seal_context.n(), slots = n >> 1;
        const std::size_t rows = static_cast<std::size_t>(row_W);
        const std::size_t cols = static_cast<std::size_t>(128 * (col_W / 128));
        for (std::size_t j = 0; j < rows; j++)
        {
            if (enc_X[j].parms_id() != pid || enc_X[j].size() != 2 || !enc_X[j].is_ntt_form())
            {
                throw std::invalid_argument("encrypted_ntt and plain_ntt parameter mismatch");
            }
            if (enc_X[j].scale() != scale)
            {
                throw std::invalid_argument("scale mismatch");
            }
        }
        // CKKSEncoder::encode and multiply_plain checks (ckks.h:493-497, evaluator.cpp:2351-2357)
        if (scale <= 0 || (static_cast<int>(std::log2(scale)) + 1 >= cd->total_coeff_modulus_bit_count()))
        {
            throw std::invalid_argument("scale out of bounds");
        }
        if (static_cast<int>(std::log2(scale * scale)) >= cd->total_coeff_modulus_bit_count())
        {
            throw std::invalid_argument("scale out of bounds");
        }
        if (bias_vec.size() < slots)
        {
            throw std::invalid_argument("bias_vec is shorter than the slot count");
        }
        if (cols == 0)
        {
            return output;
        }
        void *st = seal_context.stream();
        moai_ctx *dev = seal_context.device();
        const std::size_t ct_words = 2 * L * n;
        static_assert(sizeof(int) == 4, "bias_vec is uploaded as int32");
        // two columns per round: their 2 * rows plaintexts come from one moai_ckks_encode_masked call, and one pass over the
        // input ciphertexts (moai_ct_pt_dot_rows) forms both columns' sums
        const std::size_t group = cols >= 2 ? 2 : 1;
        util::DeviceArray dmask((slots + 1) / 2, st), dconst(2 * group * rows, st); // constants, then max |coeff| per vector
        util::hip_check(moai_memcpy_h2d(dmask.get(), bias_vec.data(), slots * 4, st));
        util::DeviceArray dX(rows * ct_words, st), dP(group * rows * L * n, st), dacc(cols * ct_words, st);
        for (std::size_t j = 0; j < rows; j++)
        {
            util::hip_check(moai_memcpy_d2d(dX.get() + j * ct_words, enc_X[j].device_data(), ct_words * 8, st));
        }
        std::vector<double> wcol(group * rows), mx(group * rows);
        const int total_bits = cd->total_coeff_modulus_bit_count();
        for (std::size_t c = 0; c < cols; c += group)
        {
            const std::size_t g = std::min(group, cols - c);
            for (std::size_t k = 0; k < g; k++)
            {
                for (std::size_t j = 0; j < rows; j++)
                {
                    wcol[k * rows + j] = W[j][c + k];
                }
            }
            util::hip_check(moai_memcpy_h2d(dconst.get(), wcol.data(), g * rows * 8, st));
            double *max_dev = reinterpret_cast<double *>(dconst.get() + group * rows);
            util::hip_check(moai_ckks_encode_masked(dev, reinterpret_cast<const double *>(dconst.get()),
                                                    reinterpret_cast<const std::int32_t *>(dmask.get()), slots, g * rows, dP.get(), L,
                                                    nullptr, scale, max_dev, st));
            std::uint64_t *acc = dacc.get() + c * ct_words;
            util::hip_check(moai_ct_pt_dot_rows(dev, dX.get(), dP.get(), g == 2 ? dP.get() + rows * L * n : nullptr, acc,
                                                g == 2 ? acc + ct_words : nullptr, rows, 2, L, st));
            util::hip_check(moai_memcpy_d2h(mx.data(), max_dev, g * rows * 8, st));
            seal_context.sync(); // wcol / mx are reused by the next round
            for (std::size_t k = 0; k < g * rows; k++)
            {
                int bits = static_cast<int>(std::ceil(std::log2(std::max<>(mx[k], 1.0)))) + 1;
                if (!(bits < total_bits))
                {
                    throw std::invalid_argument("encoded values are too large");
                }
            }
        }
        util::DeviceArray dres(cols * 2 * (L - 1) * n, st);
        util::hip_check(moai_rescale(dev, dacc.get(), dres.get(), 2, L, cols, st));
        const parms_id_type next_id = cd->next_context_data()->parms_id();
        for (std::size_t c = 0; c < cols; c++)
        {
            output[c].resize(seal_context, next_id, 2);
            util::hip_check(moai_memcpy_d2d(output[c].device_data(), dres.get() + c * 2 * (L - 1) * n, 2 * (L - 1) * n * 8, st));
            output[c].is_ntt_form() = true;
            output[c].scale() = scale; // Ct_pt_matrix_mul.hpp:160
        }
        seal_context.sync();
        return output;
    }

    namespace detail
    {
        // The key switches Evaluator::rotate_internal (SEAL/evaluator.cpp:2667-2722) performs for `steps`, as
        // the list of Galois elements in the order it applies them: one element when the key exists,
        // otherwise the non-adjacent form, each term through rotate_internal again, a term of N/2 skipped.
        inline void rotation_sequence(const seal::SEALContext &context, const seal::GaloisKeys &keys, int steps,
                                      std::vector<std::uint32_t> &out)
        {
            if (steps == 0)
            {
                return;
            }
            std::uint32_t elt = moai_galois_elt_from_step(context.device(), steps);
            if (!elt)
            {
                throw std::invalid_argument("step count too large");
            }
            if (keys.has_key(elt))
            {
                out.push_back(elt);
                return;
            }
            std::vector<int> naf_steps = seal::util::naf(steps);
            if (naf_steps.size() == 1)
            {
                throw std::invalid_argument("Galois key not present");
            }
            for (int st : naf_steps)
            {
                if (static_cast<std::size_t>(std::abs(st)) != (context.n() >> 1))
                {
                    rotation_sequence(context, keys, st, out);
                }
            }
        }
    } // namespace detail

    // Same arguments and the same ciphertexts, bit for bit, as MOAI's ct_ct_matrix_mul_colpacking.  What
    // changes is the schedule: (1) the col_X columns travel as one batch, so every rotation is one batched
    // key switch instead of col_X single ones; (2) rows whose rotation sequences share a prefix (3*256 =
    // [-256, +1024] and 7*256 = [-256, +2048] both start with -256) share the prefix's result -- the same
    // operations on the same operands give the same bits, so nothing but the count of key switches changes
    // (355 -> 169 per column for 128 rows); (3) the col_X multiply + add_inplace pairs of a row are one
    // moai_ct_dot pass; (4) relinearize and rescale run once over all rows.
    inline std::vector<seal::Ciphertext> ct_ct_matrix_mul_colpacking(const std::vector<seal::Ciphertext> &enc_X,
                                                                     const std::vector<seal::Ciphertext> &enc_W,
                                                                     const seal::GaloisKeys &RotK,
                                                                     const seal::RelinKeys &relin_keys,
                                                                     const seal::SEALContext &seal_context, int col_X,
                                                                     int row_X, int col_W, int row_W, int num_batch)
    {
        using namespace seal;
        std::vector<Ciphertext> output(static_cast<std::size_t>(row_X));
        if (col_X != col_W || row_X != row_W)
        {
            std::cout << "ERROR: bad dimensions of X or W. " << std::endl;
            return output;
        }
        const double scale = enc_X[0].scale();
        const parms_id_type pid = enc_X[0].parms_id();
        auto cd = seal_context.get_context_data(pid);
        if (!cd)
        {
            throw std::invalid_argument("encrypted1 is not valid for encryption parameters");
        }
        const std::size_t cols = static_cast<std::size_t>(col_X), rows = static_cast<std::size_t>(row_X);
        for (std::size_t j = 0; j < cols; j++)
        {
            // the checks of Evaluator::multiply_inplace / add_inplace (evaluator.cpp:596-640, 155-180)
            if (enc_X[j].parms_id() != pid || enc_W[j].parms_id() != pid)
            {
                throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
            }
            if (enc_X[j].size() != 2 || enc_W[j].size() != 2)
            {
                throw std::logic_error("only size-2 ciphertexts are multiplied on the device");
            }
            if (!enc_X[j].is_ntt_form() || !enc_W[j].is_ntt_form())
            {
                throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
            }
            if (enc_X[j].scale() != enc_X[0].scale() || enc_W[j].scale() != enc_W[0].scale())
            {
                throw std::invalid_argument("scale mismatch");
            }
        }
        if (RotK.parms_id() != seal_context.key_parms_id())
        {
            throw std::invalid_argument("galois_keys is not valid for encryption parameters");
        }
        if (relin_keys.parms_id() != seal_context.key_parms_id())
        {
            throw std::invalid_argument("relin_keys is not valid for encryption parameters");
        }
        if (relin_keys.size() < 1)
        {
            throw std::invalid_argument("not enough relinearization keys");
        }
        if (!cd->next_context_data())
        {
            throw std::invalid_argument("end of modulus switching chain reached");
        }
        // scale of the products (evaluator.cpp:789-795, 904-908)
        const double new_scale = enc_X[0].scale() * enc_W[0].scale();
        if (new_scale <= 0 || (static_cast<int>(std::log2(new_scale)) >= cd->total_coeff_modulus_bit_count()))
        {
            throw std::invalid_argument("scale out of bounds");
        }
        // rotation sequences per row, rows ordered so that shared prefixes are adjacent
        std::vector<std::vector<std::uint32_t>> seq(rows);
        for (std::size_t i = 1; i < rows; i++)
        {
            detail::rotation_sequence(seal_context, RotK, static_cast<int>(i) * num_batch, seq[i]);
        }
        std::vector<std::size_t> order(rows);
        for (std::size_t i = 0; i < rows; i++)
        {
            order[i] = i;
        }
        std::sort(order.begin(), order.end(), [&](std::size_t a, std::size_t b) { return seq[a] < seq[b]; });

        const std::size_t L = cd->parms().coeff_modulus().size(), n = seal_context.n();
        const std::size_t ct_words = 2 * L * n;
        void *st = seal_context.stream();
        moai_ctx *dev = seal_context.device();
        util::DeviceArray dX(cols * ct_words, st), dW(cols * ct_words, st), d3(rows * 3 * L * n, st);
        for (std::size_t j = 0; j < cols; j++)
        {
            util::hip_check(moai_memcpy_d2d(dX.get() + j * ct_words, enc_X[j].device_data(), ct_words * 8, st));
            util::hip_check(moai_memcpy_d2d(dW.get() + j * ct_words, enc_W[j].device_data(), ct_words * 8, st));
        }
        // The rotation sequences form a prefix tree: a node = all columns of W after a prefix of key switches; the rows
        // whose sequence ends at a node take their products there.  The children of a node rotate the SAME ciphertexts by
        // different steps: with two or more of them that is one hoisted call (one digit decomposition for all of them,
        // moai_apply_galois_hoisted; same bits), otherwise one batched key switch.
        struct Node
        {
            std::map<std::uint32_t, std::unique_ptr<Node>> child;
            std::vector<std::size_t> ends;
        };
        Node root;
        for (std::size_t i = 0; i < rows; i++)
        {
            Node *at = &root;
            for (std::uint32_t e : seq[i])
            {
                auto &c = at->child[e];
                if (!c)
                {
                    c.reset(new Node());
                }
                at = c.get();
            }
            at->ends.push_back(i);
        }
        (void)order;
        static const bool hoist = [] {
            const char *e = std::getenv("MOAI_SHIM_HOIST");
            return !(e && e[0] == '0');
        }();
        std::function<void(const Node &, const std::uint64_t *)> walk = [&](const Node &node, const std::uint64_t *buf) {
            for (std::size_t i : node.ends)
            {
                util::hip_check(moai_ct_dot(dev, dX.get(), buf, d3.get() + i * 3 * L * n, cols, L, st));
            }
            if (node.child.empty())
            {
                return;
            }
            std::vector<util::DeviceArray> kids;
            kids.reserve(node.child.size());
            std::vector<std::uint32_t> elts;
            std::vector<const std::uint64_t *> kptr, cptr;
            std::vector<std::uint64_t *> optr;
            for (auto &kv : node.child)
            {
                kids.emplace_back(cols * ct_words, st);
                elts.push_back(kv.first);
                const std::size_t index = GaloisKeys::get_index(kv.first);
                kptr.push_back(RotK.device_key(index, L));
                optr.push_back(kids.back().get());
            }
            if (hoist && elts.size() >= 2 && seal_context.logn() >= 12)
            {
                for (std::uint32_t e : elts)
                {
                    cptr.push_back(RotK.hoist_correction(seal_context, GaloisKeys::get_index(e), e, L));
                }
                int fell_back = 0;
                util::hip_check(moai_apply_galois_hoisted(dev, buf, optr.data(), L, elts.data(), kptr.data(), cptr.data(), elts.size(), cols,
                                                          &fell_back, st));
            }
            else
            {
                for (std::size_t c = 0; c < elts.size(); c++)
                {
                    util::hip_check(moai_apply_galois_to(dev, buf, optr[c], L, elts[c], kptr[c], cols, st));
                }
            }
            std::size_t c = 0;
            for (auto &kv : node.child)
            {
                walk(*kv.second, kids[c].get());
                kids[c] = util::DeviceArray(); // release as soon as the subtree is done
                c++;
            }
        };
        walk(root, dW.get());
        util::DeviceArray d2(rows * ct_words, st), dres(rows * 2 * (L - 1) * n, st);
        util::hip_check(moai_relinearize(dev, d3.get(), relin_keys.device_key(0, L), d2.get(), L, rows, st));
        util::hip_check(moai_rescale(dev, d2.get(), dres.get(), 2, L, rows, st));
        const parms_id_type next_id = cd->next_context_data()->parms_id();
        for (std::size_t i = 0; i < rows; i++)
        {
            output[i].resize(seal_context, next_id, 2);
            util::hip_check(moai_memcpy_d2d(output[i].device_data(), dres.get() + i * 2 * (L - 1) * n, 2 * (L - 1) * n * 8, st));
            output[i].is_ntt_form() = true;
            output[i].scale() = scale; // Ct_ct_matrix_mul.hpp:48
        }
        seal_context.sync(); // the staging buffers go out of scope
        return output;
    }
    // moai_fused::ct_ct_matrix_mul_diagpacking replaces include/source/matrix_mul/Ct_ct_matrix_mul.hpp:58-153
    // (softmax(QK^T) V): same arguments, same ciphertexts bit for bit.  The rotations of X that share a step, the
    // baby-step rotations of all columns of W, the relinearize / rescale of all partial products and the giant-step
    // rotations each run as batched calls; the products of a (column, giant step) pair are one moai_ct_dot.
    inline std::vector<seal::Ciphertext> ct_ct_matrix_mul_diagpacking(const std::vector<seal::Ciphertext> &enc_X,
                                                                      const std::vector<seal::Ciphertext> &enc_W,
                                                                      const seal::GaloisKeys &RotK,
                                                                      const seal::RelinKeys &relin_keys,
                                                                      const seal::SEALContext &seal_context, int col_X,
                                                                      int row_X, int col_W, int row_W, int num_batch)
    {
        using namespace seal;
        (void)row_W;
        const double scale = enc_X[0].scale();
        std::vector<Ciphertext> output(static_cast<std::size_t>(col_W));
        // Ct_ct_matrix_mul.hpp:71-79
        int g = static_cast<int>(std::sqrt(static_cast<double>(col_X)));
        if (g * g < col_X)
        {
            g++;
        }
        int b = col_X / g;
        if (b * g < col_X)
        {
            b++;
        }
        const parms_id_type pid = enc_X[0].parms_id();
        auto cd = seal_context.get_context_data(pid);
        if (!cd)
        {
            throw std::invalid_argument("encrypted1 is not valid for encryption parameters");
        }
        if (row_X < col_X)
        {
            throw std::logic_error("the replacement expects every diagonal of X to be present (row_X >= col_X)");
        }
        for (int i = 0; i < col_X; i++)
        {
            const Ciphertext &c = enc_X[static_cast<std::size_t>(i)];
            if (c.parms_id() != pid || c.size() != 2 || !c.is_ntt_form() || c.scale() != scale)
            {
                throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
            }
        }
        for (int i = 0; i < col_W; i++)
        {
            const Ciphertext &c = enc_W[static_cast<std::size_t>(i)];
            if (c.parms_id() != pid || c.size() != 2 || !c.is_ntt_form() || c.scale() != enc_W[0].scale())
            {
                throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
            }
        }
        if (RotK.parms_id() != seal_context.key_parms_id())
        {
            throw std::invalid_argument("galois_keys is not valid for encryption parameters");
        }
        if (relin_keys.parms_id() != seal_context.key_parms_id() || relin_keys.size() < 1)
        {
            throw std::invalid_argument("relin_keys is not valid for encryption parameters");
        }
        if (!cd->next_context_data())
        {
            throw std::invalid_argument("end of modulus switching chain reached");
        }
        const double new_scale = scale * enc_W[0].scale();
        if (new_scale <= 0 || (static_cast<int>(std::log2(new_scale)) >= cd->total_coeff_modulus_bit_count()))
        {
            throw std::invalid_argument("scale out of bounds");
        }
        const std::size_t L = cd->parms().coeff_modulus().size(), n = seal_context.n();
        const std::size_t ctw = 2 * L * n, G = static_cast<std::size_t>(g), Bg = static_cast<std::size_t>(b);
        const std::size_t cols = static_cast<std::size_t>(col_W), nx = static_cast<std::size_t>(col_X);
        void *st = seal_context.stream();
        moai_ctx *dev = seal_context.device();
        std::vector<std::uint32_t> seq;
        auto rotate = [&](std::uint64_t *data, int step, std::size_t count) {
            // Evaluator::rotate_vector on `count` contiguous ciphertexts
            seq.clear();
            detail::rotation_sequence(seal_context, RotK, step, seq);
            for (std::uint32_t elt : seq)
            {
                util::hip_check(moai_apply_galois(dev, data, L, elt, RotK.device_key(GaloisKeys::get_index(elt), L), count, st));
            }
        };
        // rot_enc_X[index], index = i*g + j: enc_X[index] rotated by (col_X - i*g) * num_batch (:86-101)
        util::DeviceArray rx(Bg * G * ctw, st);
        for (std::size_t idx = 0; idx < nx; idx++)
        {
            util::hip_check(moai_memcpy_d2d(rx.get() + idx * ctw, enc_X[idx].device_data(), ctw * 8, st));
        }
        if (Bg * G > nx)
        {
            util::hip_check(moai_memset_zero(rx.get() + nx * ctw, (Bg * G - nx) * ctw * 8, st));
        }
        for (std::size_t i = 0; i < Bg; i++)
        {
            const int rot_ind = (col_X - static_cast<int>(i * G)) * num_batch;
            const std::size_t first = i * G, count = std::min(G, nx > first ? nx - first : 0);
            if (count && rot_ind != col_X * num_batch)
            {
                rotate(rx.get() + first * ctw, rot_ind, count);
            }
        }
        // baby steps: c_g[i][k] = enc_W[i] rotated by k * num_batch (:107-113), stored [i][k]
        util::DeviceArray cg(cols * G * ctw, st), stage(cols * ctw, st);
        for (std::size_t i = 0; i < cols; i++)
        {
            util::hip_check(moai_memcpy_d2d(stage.get() + i * ctw, enc_W[i].device_data(), ctw * 8, st));
        }
        for (std::size_t k = 0; k < G; k++)
        {
            util::DeviceArray rot(cols * ctw, st);
            util::hip_check(moai_memcpy_d2d(rot.get(), stage.get(), cols * ctw * 8, st));
            if (k)
            {
                rotate(rot.get(), static_cast<int>(k) * num_batch, cols);
            }
            for (std::size_t i = 0; i < cols; i++)
            {
                util::hip_check(moai_memcpy_d2d(cg.get() + (i * G + k) * ctw, rot.get() + i * ctw, ctw * 8, st));
            }
        }
        // giant steps: out[i][j] = sum_k c_g[i][k] * rot_enc_X[j*g + k] (:116-141), all relinearized and rescaled together
        util::DeviceArray d3(cols * Bg * 3 * L * n, st);
        for (std::size_t i = 0; i < cols; i++)
        {
            for (std::size_t j = 0; j < Bg; j++)
            {
                const std::size_t first = j * G, count = std::min(G, nx > first ? nx - first : 0);
                if (!count)
                {
                    throw std::logic_error("empty giant step");
                }
                util::hip_check(moai_ct_dot(dev, cg.get() + i * G * ctw, rx.get() + first * ctw, d3.get() + (j * cols + i) * 3 * L * n,
                                            count, L, st));
            }
        }
        util::DeviceArray d2(cols * Bg * ctw, st), dres(cols * Bg * 2 * (L - 1) * n, st);
        util::hip_check(moai_relinearize(dev, d3.get(), relin_keys.device_key(0, L), d2.get(), L, cols * Bg, st));
        util::hip_check(moai_rescale(dev, d2.get(), dres.get(), 2, L, cols * Bg, st));
        // output[i] = out[i][0] + sum_{j>=1} rotate(out[i][j], j*g*num_batch) (:142-150); layout [j][i]
        const std::size_t Lr = L - 1, rw = 2 * Lr * n;
        for (std::size_t j = 1; j < Bg; j++)
        {
            std::uint64_t *blk = dres.get() + j * cols * rw;
            seq.clear();
            detail::rotation_sequence(seal_context, RotK, static_cast<int>(j * G) * num_batch, seq);
            for (std::uint32_t elt : seq)
            {
                util::hip_check(moai_apply_galois(dev, blk, Lr, elt, RotK.device_key(GaloisKeys::get_index(elt), Lr), cols, st));
            }
            util::hip_check(moai_add(dev, dres.get(), blk, dres.get(), cols * 2, Lr, st));
        }
        const parms_id_type next_id = cd->next_context_data()->parms_id();
        for (std::size_t i = 0; i < cols; i++)
        {
            output[i].resize(seal_context, next_id, 2);
            util::hip_check(moai_memcpy_d2d(output[i].device_data(), dres.get() + i * rw, rw * 8, st));
            output[i].is_ntt_form() = true;
            output[i].scale() = scale; // :139
        }
        seal_context.sync();
        return output;
    }

    // ---- the client's input path on the device (opt-in; include/moai_hip.h "client randomness and encryption") ---------
    // Keys drawn on the device from the key generator's util::DeviceRng: ordinary PublicKey / RelinKeys / GaloisKeys (fresh
    // generation and hoisting cache, as KeyGenerator's own methods give them), so every evaluator path takes them unchanged.
    inline void create_public_key(seal::KeyGenerator &keygen, seal::PublicKey &destination)
    {
        keygen.create_public_key_device(destination);
    }
    inline void create_relin_keys(seal::KeyGenerator &keygen, seal::RelinKeys &destination)
    {
        keygen.create_relin_keys_device(destination);
    }
    inline void create_galois_keys(seal::KeyGenerator &keygen, const std::vector<std::uint32_t> &galois_elts, seal::GaloisKeys &destination)
    {
        keygen.create_galois_keys_device(galois_elts, destination);
    }
    // keys limited to a chain index, drawn on the device in the trimmed layout (KeyGenerator::create_*_keys_limited)
    inline void create_relin_keys_limited(seal::KeyGenerator &keygen, std::size_t chain_index, seal::RelinKeys &destination)
    {
        keygen.create_relin_keys_limited_device(chain_index, destination);
    }
    inline void create_galois_keys_limited(seal::KeyGenerator &keygen, const std::vector<std::uint32_t> &galois_elts,
                                           const std::vector<std::size_t> &chain_indices, seal::GaloisKeys &destination)
    {
        keygen.create_galois_keys_limited_device(galois_elts, chain_indices, destination);
    }
    inline void create_galois_keys(seal::KeyGenerator &keygen, const std::vector<int> &steps, seal::GaloisKeys &destination)
    {
        keygen.create_galois_keys_device(keygen.galois_elts_from_steps(steps), destination);
    }
    inline void create_galois_keys(seal::KeyGenerator &keygen, seal::GaloisKeys &destination)
    {
        keygen.create_galois_keys_device(keygen.galois_elts_all(), destination);
    }

    namespace detail
    {
        // encrypts `count` NTT-form plaintexts [count][L][N] (contiguous, device) at level parms_id into cts[first ..), batched:
        // SEAL-faithful public-key encryption (moai_encrypt_asymmetric), then one scatter per 64 ciphertexts
        inline void encrypt_packed(const seal::Encryptor &encryptor, seal::parms_id_type parms_id, const std::uint64_t *plains,
                                   std::size_t count, double scale, std::vector<seal::Ciphertext> &cts, std::size_t first)
        {
            using namespace seal;
            const SEALContext &context = encryptor.context();
            const std::uint64_t *pk = encryptor.public_key_device();
            if (!pk)
            {
                throw std::logic_error("public key is not set");
            }
            const std::size_t n = context.n();
            const std::size_t L = context.get_context_data(parms_id)->parms().coeff_modulus().size();
            void *st = context.stream();
            util::DeviceArray packed(count * 2 * L * n, st);
            const auto &rng = encryptor.device_rng();
            util::hip_check(moai_encrypt_asymmetric(context.device(), rng->key(), rng->take(count), pk, plains, packed.get(), count, L, st));
            for (std::size_t g = 0; g < count; g += 64)
            {
                const std::size_t m = std::min<std::size_t>(64, count - g);
                std::uint64_t *dst[64];
                for (std::size_t j = 0; j < m; j++)
                {
                    Ciphertext &c = cts[first + g + j];
                    c.resize(context, parms_id, 2);
                    c.is_ntt_form() = true;
                    c.scale() = scale;
                    dst[j] = c.device_data();
                }
                util::hip_check(moai_scatter_blocks(context.device(), packed.get() + g * 2 * L * n, dst, m, 2 * L * n, st));
            }
            context.sync();
        }

        // Cuts `plains` into runs of at most 64 NTT-form vector plaintexts at one level and scale, gathers each run into one
        // device block [count][L][N] and calls f(first, count, L, gathered).  `what` names the caller in the refusal of a
        // scalar-row plaintext.
        template <typename F>
        inline void for_plain_runs(const seal::SEALContext &context, const std::vector<seal::Plaintext> &plains, const char *what, F f)
        {
            using namespace seal;
            for (std::size_t i = 0; i < plains.size();)
            {
                const Plaintext &p0 = plains[i];
                auto cd = context.get_context_data(p0.parms_id());
                if (!cd || !p0.is_ntt_form())
                {
                    throw std::invalid_argument("plain is not valid for encryption parameters");
                }
                if (p0.is_scalar())
                {
                    throw std::invalid_argument(std::string(what) + " takes vector plaintexts");
                }
                std::size_t j = i + 1;
                while (j < plains.size() && j - i < 64 && plains[j].parms_id() == p0.parms_id() && plains[j].scale() == p0.scale() &&
                       !plains[j].is_scalar() && plains[j].is_ntt_form())
                {
                    j++;
                }
                const std::size_t L = cd->parms().coeff_modulus().size();
                util::DeviceArray gathered((j - i) * L * context.n(), context.stream());
                const std::uint64_t *src[64];
                for (std::size_t t = i; t < j; t++)
                {
                    src[t - i] = plains[t].device_data();
                }
                util::hip_check(moai_gather_blocks(context.device(), src, gathered.get(), j - i, L * context.n(), context.stream()));
                f(i, j - i, L, gathered.get());
                i = j;
            }
        }
    } // namespace detail

    // Encryptor::encrypt for many plaintexts (SEAL/encryptor.cpp:88-173 with the public key): batched device launches per run
    // of plaintexts at one level and scale.  Scalar-row plaintexts are refused (std::invalid_argument): encode them as vectors,
    // or encrypt them with Encryptor::encrypt.
    inline void encrypt(const seal::Encryptor &encryptor, const std::vector<seal::Plaintext> &plains, std::vector<seal::Ciphertext> &cts)
    {
        cts.resize(plains.size());
        detail::for_plain_runs(encryptor.context(), plains, "moai_fused::encrypt",
                               [&](std::size_t first, std::size_t count, std::size_t, const std::uint64_t *gathered) {
                                   detail::encrypt_packed(encryptor, plains[first].parms_id(), gathered, count, plains[first].scale(), cts, first);
                               });
    }

    // Encryptor::encrypt_symmetric(plain).save(stream) for many plaintexts (SEAL/encryptor.h:374-404 with save_seed): per run of up
    // to 64 plaintexts at one level and scale ONE moai_encrypt_symmetric_seeded, ONE moai_pack_rows and ONE device-to-host copy
    // into page-locked memory; then one record per ciphertext, in order, each loadable with Ciphertext::load.  The ciphertexts of
    // a run share the run's public seed and take consecutive sequences.  Returns the bytes written (13.8 MB per ciphertext at
    // MOAI's parameters instead of the 36.7 MB a download of the expanded ciphertext moves).
    inline std::streamoff encrypt_symmetric_save(const seal::Encryptor &encryptor, const std::vector<seal::Plaintext> &plains, std::ostream &stream)
    {
        using namespace seal;
        const SEALContext &context = encryptor.context();
        const std::uint64_t *sk = encryptor.secret_key_device();
        if (!sk)
        {
            throw std::logic_error("secret key is not set");
        }
        const std::size_t n = context.n();
        void *st = context.stream();
        wire::StreamSink sink(stream);
        std::streamoff total = 0;
        struct Pinned
        {
            void *p = nullptr;
            ~Pinned()
            {
                if (p)
                {
                    moai_host_free(p);
                }
            }
        } host;
        std::size_t host_bytes = 0;
        detail::for_plain_runs(context, plains, "moai_fused::encrypt_symmetric_save",
                               [&](std::size_t first, std::size_t m, std::size_t L, const std::uint64_t *gathered) {
            const std::size_t pw = wire::packed_words(context.device(), L);
            util::DeviceArray packed(m * pw, st);
            // one record head for the run, its block the m c0 polynomials; always under the run's ChaCha20 seed, the only kind
            // the wire format carries seeded
            wire::Record r = util::seeded_record_head(wire::kind_ciphertext, 2, L, plains[first].parms_id(), m * L * n, context);
            r.scale = plains[first].scale();
            const auto &rng = encryptor.device_rng();
            const std::uint64_t seq0 = rng->take(m);
            util::public_seed(rng->key(), seq0, r.seed);
            util::hip_check(moai_encrypt_symmetric_seeded(context.device(), rng->key(), r.seed, seq0, sk, gathered, r.block->get(), m, L, nullptr, st));
            util::hip_check(moai_pack_rows(context.device(), r.block->get(), packed.get(), m, L, nullptr, st));
            if (host_bytes < m * pw * 8)
            {
                if (host.p)
                {
                    util::hip_check(moai_host_free(host.p));
                    host.p = nullptr;
                }
                host_bytes = m * pw * 8;
                util::hip_check(moai_host_malloc(&host.p, host_bytes));
            }
            util::hip_check(moai_memcpy_d2h(host.p, packed.get(), m * pw * 8, st));
            context.sync();
            for (std::size_t b = 0; b < m; b++)
            {
                r.seq = seq0 + b;
                const wire::Header h = wire::make_header(r, n, sizeof(wire::Header) + pw * 8);
                sink.put(&h, sizeof(h));
                sink.put(static_cast<const std::uint8_t *>(host.p) + b * pw * 8, pw * 8);
                total += static_cast<std::streamoff>(sizeof(h) + pw * 8);
            }
        });
        return total;
    }

    // batch_input of MOAI (include/source/matrix_mul/Batch_encode_encrypt.hpp:8-38): column i of the inputs, slot
    // num_X * k + j = X[j][k][i], encoded at `scale` (moai_ckks_encode, many columns per launch) and encrypted with pk on the
    // device in batched launches.  Same slot layout and level as the reference; fresh randomness (rng: null = OS-keyed).
    inline std::vector<seal::Ciphertext> batch_input(const std::vector<std::vector<std::vector<double>>> &X, int num_X, int num_row,
                                                     int num_col, double scale, const seal::SEALContext &seal_context,
                                                     const seal::PublicKey &pk,
                                                     std::shared_ptr<seal::util::DeviceRng> rng = nullptr)
    {
        using namespace seal;
        Encryptor encryptor(seal_context, pk);
        if (rng)
        {
            encryptor.set_device_rng(rng);
        }
        const std::size_t n = seal_context.n(), slots = n / 2;
        const parms_id_type parms_id = seal_context.first_parms_id();
        auto cd = seal_context.get_context_data(parms_id);
        const std::size_t L = cd->parms().coeff_modulus().size();
        if (scale <= 0 || (static_cast<int>(std::log2(scale)) + 1 >= cd->total_coeff_modulus_bit_count()))
        {
            throw std::invalid_argument("scale out of bounds");
        }
        if (static_cast<std::size_t>(num_X) * static_cast<std::size_t>(num_row) > slots)
        {
            throw std::invalid_argument("values_size is too large");
        }
        void *st = seal_context.stream();
        std::vector<Ciphertext> output(num_col);
        constexpr std::size_t G = 64;
        std::vector<double> vals(G * slots);
        util::DeviceArray dvals(G * slots, st);
        util::DeviceArray dmax(G, st);
        util::DeviceArray plains(G * L * n, st);
        for (int c0 = 0; c0 < num_col; c0 += static_cast<int>(G))
        {
            const std::size_t m = std::min<std::size_t>(G, static_cast<std::size_t>(num_col - c0));
            std::fill(vals.begin(), vals.end(), 0.0);
            for (std::size_t t = 0; t < m; t++)
            {
                double *vec = vals.data() + t * slots;
                for (int j = 0; j < num_X; ++j)
                {
                    for (int k = 0; k < num_row; ++k)
                    {
                        vec[num_X * k + j] = X[j][k][c0 + t];
                    }
                }
            }
            util::hip_check(moai_memcpy_h2d(dvals.get(), vals.data(), m * slots * 8, st));
            util::hip_check(moai_ckks_encode(seal_context.device(), reinterpret_cast<const double *>(dvals.get()), 0, slots, m,
                                             plains.get(), L, nullptr, scale, reinterpret_cast<double *>(dmax.get()), st));
            // ckks.h:527-538 for every column
            std::vector<double> mx(m);
            util::hip_check(moai_memcpy_d2h(mx.data(), dmax.get(), m * 8, st));
            seal_context.sync();
            for (double v : mx)
            {
                const int bits = static_cast<int>(std::ceil(std::log2(std::max<>(v, 1.0)))) + 1;
                if (!(bits < cd->total_coeff_modulus_bit_count()))
                {
                    throw std::invalid_argument("encoded values are too large");
                }
            }
            detail::encrypt_packed(encryptor, parms_id, plains.get(), m, scale, output, static_cast<std::size_t>(c0));
        }
        return output;
    }
} // namespace moai_fused
