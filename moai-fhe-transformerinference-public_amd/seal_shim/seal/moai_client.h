// seal/moai_client.h -- client-side classes of the seal:: surface: CKKSEncoder, KeyGenerator,
// Encryptor, Decryptor.  Host code (randomness, FP64 FFT, CRT); out of the hot-path scope
//  but needed so that MOAI's programs link and run.  Their NTTs are
// executed on the device through moai_ntt_forward / moai_ntt_inverse.
#pragma once
#include <cerrno>
#include <exception>
#include <memory>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include <sys/random.h>
#include <sys/types.h>

namespace seal
{
    namespace util
    {
        // Randomness of the client side: ChaCha20 (RFC 8439 block function, 20 rounds) in counter mode, keyed per thread
        // with 256 bits + a 64-bit nonce drawn from the operating system (getrandom(2), /dev/urandom as a fallback).
        // The reference expands a 512-bit OS seed with Blake2xb / Shake256 (SEAL/randomgen.cpp:18-62, 142-169); the
        // construction differs, the property does not: every secret (ternary key, uniform a, noise, u / e0 / e1) comes
        // from a cryptographic stream whose state cannot be recovered from the public outputs.  Satisfies the C++
        // UniformRandomBitGenerator requirements, so the standard distributions below take it.
        class ChaCha20Rng
        {
        public:
            using result_type = std::uint64_t;
            static constexpr result_type min()
            {
                return 0;
            }
            static constexpr result_type max()
            {
                return ~static_cast<result_type>(0);
            }
            ChaCha20Rng()
            {
                unsigned char seed[40];
                os_random(seed, sizeof(seed));
                init(seed);
            }
            // a fixed stream (known-answer test of the block function): 32-byte key + 8-byte nonce
            explicit ChaCha20Rng(const unsigned char (&seed)[40])
            {
                init(seed);
            }
            result_type operator()()
            {
                if (pos_ == 8)
                {
                    refill();
                }
                return buf_[pos_++];
            }
            static void os_random(unsigned char *out, std::size_t len)
            {
                std::size_t got = 0;
                while (got < len)
                {
                    ssize_t r = ::getrandom(out + got, len - got, 0);
                    if (r > 0)
                    {
                        got += static_cast<std::size_t>(r);
                    }
                    else if (r < 0 && errno == EINTR)
                    {
                        continue;
                    }
                    else
                    {
                        break;
                    }
                }
                if (got < len)
                {
                    std::FILE *f = std::fopen("/dev/urandom", "rb");
                    if (f)
                    {
                        got += std::fread(out + got, 1, len - got, f);
                        std::fclose(f);
                    }
                }
                if (got < len)
                {
                    throw std::runtime_error("no operating-system randomness available");
                }
            }

        private:
            static std::uint32_t rotl(std::uint32_t v, int c)
            {
                return (v << c) | (v >> (32 - c));
            }
            static void quarter(std::uint32_t *x, int a, int b, int c, int d)
            {
                x[a] += x[b];
                x[d] = rotl(x[d] ^ x[a], 16);
                x[c] += x[d];
                x[b] = rotl(x[b] ^ x[c], 12);
                x[a] += x[b];
                x[d] = rotl(x[d] ^ x[a], 8);
                x[c] += x[d];
                x[b] = rotl(x[b] ^ x[c], 7);
            }
            void init(const unsigned char *seed)
            {
                static const std::uint32_t sigma[4] = { 0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u }; // "expand 32-byte k"
                std::memcpy(state_, sigma, 16);
                std::memcpy(state_ + 4, seed, 32);      // key
                state_[12] = state_[13] = 0;            // 64-bit block counter
                std::memcpy(state_ + 14, seed + 32, 8); // nonce
                pos_ = 8;
            }
            void refill()
            {
                std::uint32_t x[16];
                std::memcpy(x, state_, sizeof(x));
                for (int i = 0; i < 10; i++)
                {
                    quarter(x, 0, 4, 8, 12);
                    quarter(x, 1, 5, 9, 13);
                    quarter(x, 2, 6, 10, 14);
                    quarter(x, 3, 7, 11, 15);
                    quarter(x, 0, 5, 10, 15);
                    quarter(x, 1, 6, 11, 12);
                    quarter(x, 2, 7, 8, 13);
                    quarter(x, 3, 4, 9, 14);
                }
                for (int i = 0; i < 16; i++)
                {
                    x[i] += state_[i];
                }
                std::memcpy(buf_, x, sizeof(buf_));
                if (++state_[12] == 0)
                {
                    ++state_[13];
                }
                pos_ = 0;
            }
            std::uint32_t state_[16];
            std::uint64_t buf_[8];
            int pos_ = 8;
        };

        inline ChaCha20Rng &thread_rng()
        {
            static thread_local ChaCha20Rng g;
            return g;
        }

        // Which generator the public half of a seeded object (a Serializable<T>) is the expansion of: this library's ChaCha20
        // stream (the default, and the only kind its own wire format carries seeded), or SEAL's Blake2xbPRNG under a 64-byte seed
        // per ciphertext or key digit, which save_seal then writes seeded as SEAL itself would (SEAL/ciphertext.cpp:190-381)
        enum class seed_kind
        {
            chacha20,
            seal_blake2xb
        };

        // Randomness of the device samplers (include/moai_hip.h, "client randomness and encryption"): a 32-byte ChaCha20 key
        // drawn from the operating system, and an atomic counter that hands out disjoint ranges of nonce sequences, so that
        // every encryption or key digit drawn with this object uses a stream of its own, whichever thread asks.  Tests and
        // tools construct it from a fixed key for reproducible output.
        class DeviceRng
        {
        public:
            DeviceRng()
            {
                ChaCha20Rng::os_random(key_, sizeof(key_));
            }
            explicit DeviceRng(const unsigned char (&key)[32], std::uint64_t first_sequence = 0) : next_(first_sequence)
            {
                std::memcpy(key_, key, sizeof(key_));
            }
            const unsigned char *key() const
            {
                return key_;
            }
            // the first of `count` consecutive sequence numbers nobody else gets
            std::uint64_t take(std::uint64_t count)
            {
                const std::uint64_t first = next_.fetch_add(count);
                if (first >= (std::uint64_t(1) << 56) || count > (std::uint64_t(1) << 56) - first)
                {
                    throw std::logic_error("device randomness exhausted: draw a new key");
                }
                return first;
            }
            // opt-in: the calls without a destination (Encryptor::encrypt_symmetric(plain), KeyGenerator::create_*_keys())
            // return objects seeded for SEAL.  Noise and sequence numbers are what they are under the default.
            void set_seed_kind(seed_kind kind)
            {
                kind_.store(kind);
            }
            seed_kind get_seed_kind() const
            {
                return kind_.load();
            }

        private:
            unsigned char key_[32];
            std::atomic<std::uint64_t> next_{ 0 };
            std::atomic<seed_kind> kind_{ seed_kind::chacha20 };
        };

        // the first `words` 64-bit words, little endian, of the stream (noise key, purpose << 56 | seq)
        inline void stream_head(const unsigned char *noise_key, std::uint64_t purpose, std::uint64_t seq, std::uint8_t *out, int words)
        {
            unsigned char init[40];
            std::memcpy(init, noise_key, 32);
            const std::uint64_t nonce = (purpose << 56) | seq;
            for (int i = 0; i < 8; i++)
            {
                init[32 + i] = static_cast<unsigned char>(nonce >> (8 * i));
            }
            ChaCha20Rng g(init);
            for (int w = 0; w < words; w++)
            {
                const std::uint64_t v = g();
                for (int i = 0; i < 8; i++)
                {
                    out[8 * w + i] = static_cast<std::uint8_t>(v >> (8 * i));
                }
            }
        }

        // The public seed of a seeded object (include/moai_hip.h, purpose 5): the first 32 bytes of the stream
        // (noise key, 5 << 56 | seq).  ChaCha20 output does not reveal its key, so the seed may travel where the key may not
        // (the reference draws its public seed from the secret generator the same way, SEAL/util/rlwe.cpp:353-363).
        inline void public_seed(const unsigned char *noise_key, std::uint64_t seq, std::uint8_t (&seed)[32])
        {
            stream_head(noise_key, 5, seq, seed, 4);
        }
        // The SEAL seeds of `count` consecutive objects (include/moai_hip.h, purpose 6): for the ciphertext or key digit with
        // sequence seq + b the 64 bytes W[0..7] of the stream (noise key, 6 << 56 | seq + b)
        inline std::vector<std::uint8_t> seal_seeds(const unsigned char *noise_key, std::uint64_t seq, std::size_t count)
        {
            std::vector<std::uint8_t> seeds(64 * count);
            for (std::size_t b = 0; b < count; b++)
            {
                stream_head(noise_key, 6, seq + b, seeds.data() + 64 * b, 8);
            }
            return seeds;
        }
        // a zeroed device uint32_t[2] for moai_seal_sample_uniform's `rejected`
        inline std::shared_ptr<DeviceArray> seal_flags(void *stream)
        {
            auto f = std::make_shared<DeviceArray>(1, stream);
            hip_check(moai_memset_zero(f->get(), 8, stream));
            return f;
        }

        // The head of a seeded record: `count` polynomials of L rows, of which the stored half -- `words` 64-bit words, yet to be
        // computed -- lies in a block of the record's own
        inline wire::Record seeded_record_head(std::uint32_t kind, std::size_t count, std::size_t L, const parms_id_type &parms_id,
                                               std::size_t words, const SEALContext &context)
        {
            wire::Record r;
            r.kind = kind;
            r.flags = wire::flag_ntt | wire::flag_seeded;
            r.count = static_cast<std::uint32_t>(count);
            r.L = static_cast<std::uint32_t>(L);
            r.parms_id = parms_id;
            r.block = std::make_shared<DeviceArray>(words, context.stream());
            r.data = r.block->get();
            return r;
        }
        // Takes `sequences` consecutive sequences of `rng` for the record and computes its stored half under the generator's seed
        // kind.  ChaCha20: the record carries its first sequence and the public seed of that sequence, and seeded(seq) runs.
        // SEAL's Blake2xb: the same sequences for the noise, one 64-byte SEAL seed per sequence for the uniform halves, and
        // seal_seeded(seq, rejected) runs, with the device counters the record keeps until it is saved.
        template <typename Seeded, typename SealSeeded>
        inline void fill_seeded_record(wire::Record &r, DeviceRng &rng, std::size_t sequences, void *stream, Seeded seeded, SealSeeded seal_seeded)
        {
            const std::uint64_t seq = rng.take(sequences);
            if (rng.get_seed_kind() == seed_kind::seal_blake2xb)
            {
                r.seal_seeds = seal_seeds(rng.key(), seq, sequences);
                r.seal_flags = seal_flags(stream);
                hip_check(seal_seeded(seq, reinterpret_cast<std::uint32_t *>(r.seal_flags->get())));
                return;
            }
            r.seq = seq;
            public_seed(rng.key(), r.seq, r.seed);
            hip_check(seeded(seq));
        }
        // c0 of one symmetric encryption of `plain` (null: of zero) at L primes, seeded: a ciphertext, or the public key at the
        // key level
        inline wire::Record seeded_encryption(std::uint32_t kind, std::size_t L, const parms_id_type &parms_id, const std::uint64_t *sk_ntt,
                                              const std::uint64_t *plain, DeviceRng &rng, const SEALContext &context)
        {
            wire::Record r = seeded_record_head(kind, 2, L, parms_id, L * context.n(), context);
            std::uint64_t *c0 = r.block->get();
            fill_seeded_record(
                r, rng, 1, context.stream(),
                [&](std::uint64_t seq) {
                    return moai_encrypt_symmetric_seeded(context.device(), rng.key(), r.seed, seq, sk_ntt, plain, c0, 1, L, nullptr, context.stream());
                },
                [&](std::uint64_t seq, std::uint32_t *rejected) {
                    return moai_encrypt_symmetric_seal_seeded(context.device(), rng.key(), r.seal_seeds.data(), seq, sk_ntt, plain, c0, 1, L, nullptr,
                                                              rejected, context.stream());
                });
            return r;
        }

        // data primes of a key limited to chain index c, of k primes with the special one: c + 1, and the full k-1 from c = k-2 on
        inline std::size_t levels_of(std::size_t chain_index, std::size_t k)
        {
            return chain_index >= k - 2 ? k - 1 : chain_index + 1;
        }
        // What a call generates: (slot, levels) per switching key; levels == k-1 is a whole key
        using KeyPlan = std::vector<std::pair<std::uint64_t, std::size_t>>;
        // The plan of a set of Galois keys at degree n: one entry per distinct element, in the order given; the first mention of
        // an element counts.  chain_indices: null for whole keys, otherwise one entry per element or a single entry for all.
        // Host arithmetic only: every element is checked here, before the first key is generated.
        inline KeyPlan galois_key_plan(const std::vector<std::uint32_t> &galois_elts, const std::vector<std::size_t> *chain_indices, std::size_t n,
                                       std::size_t k)
        {
            if (chain_indices && chain_indices->size() != 1 && chain_indices->size() != galois_elts.size())
            {
                throw std::invalid_argument("chain_indices must hold one entry, or one per Galois element");
            }
            KeyPlan plan;
            for (std::size_t i = 0; i < galois_elts.size(); i++)
            {
                const std::uint32_t elt = galois_elts[i];
                if (!(elt & 1) || elt >= 2 * n)
                {
                    throw std::invalid_argument("Galois element is not valid");
                }
                const std::uint64_t slot = (elt - 1) >> 1; // GaloisKeys::get_index
                const bool seen = std::any_of(plan.begin(), plan.end(), [slot](const KeyPlan::value_type &p) { return p.first == slot; });
                if (!seen)
                {
                    plan.emplace_back(slot, chain_indices ? levels_of((*chain_indices)[chain_indices->size() == 1 ? 0 : i], k) : k - 1);
                }
            }
            return plan;
        }

        // uniform residues [rows][N], row r under primes[r]
        inline void sample_uniform(const std::vector<std::uint64_t> &primes, std::size_t n, std::vector<std::uint64_t> &out)
        {
            out.resize(primes.size() * n);
            // rows are independent and every thread owns its generator: a switching key at MOAI's size draws 35 x 36 x
            // 65536 residues, which one host thread takes about a second for
#pragma omp parallel for schedule(dynamic)
            for (std::size_t r = 0; r < primes.size(); r++)
            {
                auto &g = thread_rng();
                std::uniform_int_distribution<std::uint64_t> d(0, primes[r] - 1);
                for (std::size_t i = 0; i < n; i++)
                {
                    out[r * n + i] = d(g);
                }
            }
        }

        // small signed polynomial -> RNS rows
        inline void to_rns(const std::vector<std::int64_t> &poly, const std::vector<std::uint64_t> &primes,
                           std::vector<std::uint64_t> &out)
        {
            const std::size_t n = poly.size();
            out.resize(primes.size() * n);
#pragma omp parallel for schedule(static)
            for (std::size_t r = 0; r < primes.size(); r++)
            {
                const std::uint64_t q = primes[r];
                for (std::size_t i = 0; i < n; i++)
                {
                    std::int64_t v = poly[i];
                    out[r * n + i] = v >= 0 ? static_cast<std::uint64_t>(v) % q
                                            : q - (static_cast<std::uint64_t>(-v) % q == 0 ? q : static_cast<std::uint64_t>(-v) % q);
                }
            }
        }

        // centred binomial / clipped normal noise, sigma = 3.2 (SEAL/util/globals.h noise_standard_deviation)
        inline void sample_noise(std::size_t n, std::vector<std::int64_t> &e)
        {
            e.resize(n);
            std::normal_distribution<double> d(0.0, 3.2);
            auto &g = thread_rng();
            for (auto &x : e)
            {
                double v;
                do
                {
                    v = d(g);
                } while (std::fabs(v) > 19.2); // noise_max_deviation = 6 sigma
                x = static_cast<std::int64_t>(std::llround(v));
            }
        }

        // ternary secret; hamming weight hw > 0 gives the fork's sparse secret (SEAL/util/rlwe.cpp:40-97)
        inline void sample_ternary(std::size_t n, std::size_t hw, std::vector<std::int64_t> &s)
        {
            s.assign(n, 0);
            auto &g = thread_rng();
            if (hw == 0 || hw >= n)
            {
                std::uniform_int_distribution<int> d(-1, 1);
                for (auto &x : s)
                {
                    x = d(g);
                }
                return;
            }
            std::size_t placed = 0;
            std::uniform_int_distribution<std::size_t> pos(0, n - 1);
            std::uniform_int_distribution<int> sign(0, 1);
            while (placed < hw)
            {
                std::size_t p = pos(g);
                if (s[p] == 0)
                {
                    s[p] = sign(g) ? 1 : -1;
                    placed++;
                }
            }
        }
    } // namespace util
    using util::seed_kind;

    // =================================================================================================
    // CKKSEncoder  (SEAL/ckks.{h,cpp})
    // =================================================================================================
    class CKKSEncoder
    {
    public:
        CKKSEncoder(const SEALContext &context) : context_(context)
        {
            slots_ = context_.n() >> 1;
            // ckks.cpp:29-30 (0 = all slots)
            sparse_slots_ = context_.first_context_data()->parms().sparse_slots();
            if (sparse_slots_ == 0)
            {
                sparse_slots_ = slots_;
            }
        }

        std::size_t slot_count() const noexcept
        {
            return slots_;
        }
        // ckks.h:446-450; decode returns this many values.  The device decoder refuses a count that is not a power of two
        // in [1, N/2].
        void set_sparse_slots(std::size_t sparse_slots)
        {
            sparse_slots_ = sparse_slots;
        }
        std::size_t sparse_slot_count() const noexcept
        {
            return sparse_slots_;
        }

        // ---- vector encodes (SEAL/ckks.h:457-637) -------------------------------------------------
        template <typename T>
        void encode(const std::vector<T> &values, parms_id_type parms_id, double scale, Plaintext &destination,
                    MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encode_vector(values.data(), values.size(), parms_id, scale, destination);
        }
        template <typename T>
        void encode(const std::vector<T> &values, double scale, Plaintext &destination,
                    MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encode_vector(values.data(), values.size(), context_.first_parms_id(), scale, destination);
        }
        // ---- scalar encodes (SEAL/ckks.cpp:77-216): constant rows ---------------------------------
        void encode(double value, parms_id_type parms_id, double scale, Plaintext &destination,
                    MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encode_scalar(value, parms_id, scale, destination);
        }
        void encode(double value, double scale, Plaintext &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encode_scalar(value, context_.first_parms_id(), scale, destination);
        }
        void encode(std::complex<double> value, parms_id_type parms_id, double scale, Plaintext &destination,
                    MemoryPoolHandle = MemoryPoolHandle()) const
        {
            std::vector<std::complex<double>> v(slots_, value);
            encode_vector(v.data(), v.size(), parms_id, scale, destination);
        }
        void encode(std::complex<double> value, double scale, Plaintext &destination,
                    MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encode(value, context_.first_parms_id(), scale, destination);
        }
        void encode(std::int64_t value, parms_id_type parms_id, Plaintext &destination) const
        {
            encode_scalar(static_cast<double>(value), parms_id, 1.0, destination);
        }
        void encode(std::int64_t value, Plaintext &destination) const
        {
            encode(value, context_.first_parms_id(), destination);
        }

        // ---- decode (SEAL/ckks.h:644-760): moai_ckks_decode, then N/2 values to the host; with sparse slots set
        // (sparse_slots_ != slots_, ckks.h:703-713) moai_ckks_decode_sparse and sparse_slots_ values -----------------
        template <typename T>
        void decode(const Plaintext &plain, std::vector<T> &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            static_assert(std::is_same<T, double>::value || std::is_same<T, std::complex<double>>::value,
                          "decode to double or std::complex<double>");
            auto cd = context_.get_context_data(plain.parms_id());
            if (!cd || !plain.is_ntt_form())
            {
                throw std::invalid_argument("plain is not in NTT form");
            }
            // ckks.h:672-677
            if (plain.scale() <= 0 ||
                (static_cast<int>(std::log2(plain.scale())) >= cd->total_coeff_modulus_bit_count()))
            {
                throw std::invalid_argument("scale out of bounds");
            }
            const std::size_t n = context_.n();
            const std::size_t L = cd->parms().coeff_modulus().size();
            void *st = context_.stream();
            util::DeviceArray rows;
            const std::uint64_t *src = nullptr;
            if (plain.is_scalar())
            {
                // constant rows are the NTT of a constant polynomial
                rows.resize(L * n, st);
                util::hip_check(moai_memset_zero(rows.get(), L * n * 8, st));
                util::hip_check(moai_add_scalar_rows(context_.device(), rows.get(), plain.scalar_rows().data(), rows.get(), 1,
                                                     L, st));
                src = rows.get();
            }
            else
            {
                src = plain.device_data(); // materialises a masked plaintext
            }
            constexpr bool cplx = std::is_same<T, std::complex<double>>::value;
            const std::size_t count = sparse_slots_;
            util::DeviceArray out((count ? count : 1) * (cplx ? 2 : 1), st);
            const double scale = plain.scale();
            if (count == slots_)
            {
                util::hip_check(moai_ckks_decode(context_.device(), src, 1, L, nullptr, &scale, cplx ? 1 : 0,
                                                 reinterpret_cast<double *>(out.get()), st));
            }
            else
            {
                util::hip_check(moai_ckks_decode_sparse(context_.device(), src, 1, L, nullptr, &scale, count, cplx ? 1 : 0,
                                                        reinterpret_cast<double *>(out.get()), st));
            }
            destination.resize(count);
            util::hip_check(moai_memcpy_d2h(destination.data(), out.get(), count * sizeof(T), st));
            context_.sync();
        }

    private:
        static const double *as_doubles(const double *v)
        {
            return v;
        }
        static const double *as_doubles(const std::complex<double> *v)
        {
            return reinterpret_cast<const double *>(v); // (re, im) pairs, [complex.numbers.general]
        }

        // SEAL/ckks.h:457-637 on the device (moai_ckks_encode): only the values go over PCIe
        template <typename T>
        void encode_vector(const T *values, std::size_t count, parms_id_type parms_id, double scale,
                           Plaintext &destination) const
        {
            auto cd = context_.get_context_data(parms_id);
            if (!cd)
            {
                throw std::invalid_argument("parms_id is not valid for encryption parameters");
            }
            if (!values && count > 0)
            {
                throw std::invalid_argument("values cannot be null");
            }
            if (count > slots_)
            {
                throw std::invalid_argument("values_size is too large");
            }
            const auto &cm = cd->parms().coeff_modulus();
            if (scale <= 0 || (static_cast<int>(std::log2(scale)) + 1 >= cd->total_coeff_modulus_bit_count()))
            {
                throw std::invalid_argument("scale out of bounds");
            }
            const bool is_complex = std::is_same<T, std::complex<double>>::value;
            const std::size_t n = context_.n();
            const std::size_t L = cm.size();
            const std::size_t words = count * (is_complex ? 2 : 1);
            void *stream = context_.stream();
            // Every coefficient is (scale / N) * sum of N unit-modulus multiples of the slot values and their
            // conjugates, so |coefficient| <= scale * max |value|.  When that bound already passes the
            // reference's range check (ckks.h:527-538) the check cannot fail and nothing has to come back from
            // the device; otherwise the exact maximum is fetched and tested like the reference does.
            double max_abs = 0;
            for (std::size_t i = 0; i < count; i++)
            {
                max_abs = std::max<>(max_abs, static_cast<double>(std::abs(values[i])));
            }
            const double bound = scale * max_abs * (1.0 + 1e-9);
            const bool conclusive = std::isfinite(bound) && static_cast<int>(std::ceil(std::log2(std::max<>(bound, 1.0)))) + 1 <
                                                                cd->total_coeff_modulus_bit_count();
            // a full vector with one non-zero value at some slots and zero elsewhere -- MOAI's masked weights and biases
            // (Ct_pt_matrix_mul.hpp:124-146, single_att_block.hpp:33-42): recorded, not transformed (Plaintext::mask_).  Only when
            // the range check above cannot fail, so that every exception of the reference is still raised here and now.
            if (!is_complex && conclusive && count == slots_ && util::lazy_enabled())
            {
                if (record_masked_constant(reinterpret_cast<const double *>(values), count, parms_id, scale, L, n, destination))
                {
                    return;
                }
            }
            util::DeviceArray staging(words + 1, stream); // values, then max |coefficient|
            StagingSlot &slot = staging_slot(words * 8);
            if (words)
            {
                // through page-locked memory, so that the copy is asynchronous and the caller's vector is free
                // again when this function returns
                std::memcpy(slot.host, as_doubles(values), words * 8);
                util::hip_check(moai_memcpy_h2d(staging.get(), slot.host, words * 8, stream));
            }
            destination.scalar_rows_.clear();
            destination.parms_id_ = parms_id_zero;
            destination.n_ = n;
            destination.L_ = L;
            destination.stream_ = stream;
            destination.data_.resize(L * n, stream);
            double *max_dev = reinterpret_cast<double *>(staging.get() + words);
            util::hip_check(moai_ckks_encode(context_.device(), reinterpret_cast<const double *>(staging.get()),
                                             is_complex ? 1 : 0, count, 1, destination.data_.get(), L, nullptr, scale,
                                             conclusive ? nullptr : max_dev, stream));
            util::hip_check(moai_event_record(slot.event, stream));
            slot.pending = true;
            if (!conclusive)
            {
                double max_coeff = 0;
                util::hip_check(moai_memcpy_d2h(&max_coeff, max_dev, 8, stream));
                context_.sync();
                // ckks.h:527-538 (the negated comparison also catches NaN)
                int max_coeff_bit_count = static_cast<int>(std::ceil(std::log2(std::max<>(max_coeff, 1.0)))) + 1;
                if (!(max_coeff_bit_count < cd->total_coeff_modulus_bit_count()))
                {
                    destination.data_.release();
                    throw std::invalid_argument("encoded values are too large");
                }
            }
            destination.parms_id_ = parms_id;
            destination.scale_ = scale;
        }

        // values = c * mask with mask in {0, 1}^slots and c != 0?  Then the plaintext records (mask, c, scale).  The mask's device
        // copy is shared by every plaintext with the same pattern this thread encodes in a row (MOAI encodes thousands per mask).
        bool record_masked_constant(const double *values, std::size_t count, parms_id_type parms_id, double scale, std::size_t L, std::size_t n,
                                    Plaintext &destination) const
        {
            double c = 0;
            std::size_t first = count;
            for (std::size_t i = 0; i < count; i++)
            {
                if (values[i] != 0.0)
                {
                    c = values[i];
                    first = i;
                    break;
                }
            }
            if (first == count || !std::isfinite(c))
            {
                return false; // all zero (the reference encodes that too; rare): the ordinary path
            }
            static thread_local std::shared_ptr<const util::SlotMask> last;
            static thread_local moai_ctx *last_dev = nullptr;
            const bool try_last = last && last_dev == context_.device() && last->host.size() == count;
            bool same = try_last;
            for (std::size_t i = 0; i < count; i++)
            {
                const double v = values[i];
                if (v != 0.0 && v != c)
                {
                    return false; // a general vector
                }
                if (same && (v != 0.0) != (last->host[i] != 0))
                {
                    same = false;
                }
            }
            if (!same)
            {
                auto m = std::make_shared<util::SlotMask>();
                m->host.resize(count);
                for (std::size_t i = 0; i < count; i++)
                {
                    m->host[i] = values[i] != 0.0 ? 1 : 0;
                }
                m->dev = std::make_shared<util::DeviceArray>((count + 1) / 2, context_.stream());
                util::hip_check(moai_memcpy_h2d(m->dev->get(), m->host.data(), count * 4, context_.stream()));
                context_.sync(); // once per new pattern
                last = m;
                last_dev = context_.device();
            }
            destination.scalar_rows_.clear();
            destination.data_.release();
            destination.n_ = n;
            destination.L_ = L;
            destination.stream_ = context_.stream();
            destination.dev_ = context_.device();
            destination.parms_id_ = parms_id;
            destination.scale_ = scale;
            {
                std::lock_guard<std::mutex> g(util::lazy_mutex());
                destination.mask_ = last;
                destination.mask_c_ = c;
                destination.mask_scale_ = scale;
                destination.mask_L_ = L;
                destination.owed_.v.store(true, std::memory_order_release);
            }
            return true;
        }

        // page-locked staging buffers for the values of vector encodes: a small ring per host thread; a slot is
        // reused only after the event recorded behind its last copy has completed
        struct StagingSlot
        {
            void *host = nullptr;
            std::size_t bytes = 0;
            void *event = nullptr;
            bool pending = false;
        };
        static StagingSlot &staging_slot(std::size_t bytes)
        {
            static thread_local StagingSlot ring[4];
            static thread_local unsigned next = 0;
            StagingSlot &s = ring[next++ & 3u];
            if (s.pending)
            {
                util::hip_check(moai_event_synchronize(s.event));
                s.pending = false;
            }
            if (!s.event)
            {
                util::hip_check(moai_event_create(&s.event));
            }
            if (s.bytes < bytes)
            {
                if (s.host)
                {
                    util::hip_check(moai_host_free(s.host));
                }
                s.bytes = std::max<std::size_t>(bytes, std::size_t(1) << 16);
                util::hip_check(moai_host_malloc(&s.host, s.bytes));
            }
            return s;
        }

        void encode_scalar(double value, parms_id_type parms_id, double scale, Plaintext &destination) const
        {
            auto cd = context_.get_context_data(parms_id);
            if (!cd)
            {
                throw std::invalid_argument("parms_id is not valid for encryption parameters");
            }
            const auto &cm = cd->parms().coeff_modulus();
            // SEAL/ckks.cpp:101-115
            if (scale <= 0 || (static_cast<int>(std::log2(scale)) >= cd->total_coeff_modulus_bit_count()))
            {
                throw std::invalid_argument("scale out of bounds");
            }
            value *= scale;
            int coeff_bit_count = value == 0.0 ? 1 : static_cast<int>(std::log2(std::fabs(value))) + 2;
            if (coeff_bit_count >= cd->total_coeff_modulus_bit_count())
            {
                throw std::invalid_argument("encoded value is too large");
            }
            // ckks.cpp:126-211: round, then the exact integer modulo each prime (all three branches of the
            // reference compute that), sign applied by negate_uint_mod; every coefficient of the NTT-form
            // row equals it, so only the L residues are kept
            double c = std::round(value);
            bool neg = std::signbit(c);
            double a = std::fabs(c);
            int e = 0;
            double mant = std::frexp(a, &e); // a = mant * 2^e, mant in [0.5, 1)
            std::uint64_t m53 = a != 0.0 ? static_cast<std::uint64_t>(std::ldexp(mant, 53)) : 0;
            int sh = e - 53;
            destination.scalar_rows_.resize(cm.size());
            for (std::size_t r = 0; r < cm.size(); r++)
            {
                const std::uint64_t q = cm[r].value();
                std::uint64_t v;
                if (sh <= 0)
                {
                    v = (sh > -64 ? (m53 >> (-sh)) : 0) % q;
                }
                else
                {
                    v = m53 % q;
                    for (int left = sh; left > 0;)
                    {
                        int step = left < 63 ? left : 63;
                        v = static_cast<std::uint64_t>((static_cast<util::u128>(v) << step) % q);
                        left -= step;
                    }
                }
                destination.scalar_rows_[r] = (neg && v) ? q - v : v;
            }
            destination.parms_id_ = parms_id;
            destination.scale_ = scale;
            destination.n_ = context_.n();
            destination.L_ = cm.size();
            destination.stream_ = context_.stream();
            destination.data_.release();
        }

    private:
        SEALContext context_;
        std::size_t slots_ = 0;
        std::size_t sparse_slots_ = 0;
    };

    // =================================================================================================
    // KeyGenerator  (SEAL/keygenerator.cpp)
    // =================================================================================================
    class KeyGenerator
    {
    public:
        KeyGenerator(const SEALContext &context) : context_(context)
        {
            const auto &kp = context_.key_context_data()->parms();
            set_parms();
            std::vector<std::int64_t> s;
            util::sample_ternary(n_, kp.secret_key_hamming_weight(), s);
            std::vector<std::uint64_t> rns;
            util::to_rns(s, primes_, rns);
            sk_.ntt_ = std::make_shared<util::DeviceArray>(k_ * n_, context_.stream());
            upload_ntt(rns, *sk_.ntt_, k_);
            sk_.parms_id_ = context_.key_parms_id();
        }
        // a generator for an existing secret key (SEAL/keygenerator.h, the second constructor; SEAL/keygenerator.cpp:31-45)
        KeyGenerator(const SEALContext &context, const SecretKey &secret_key) : context_(context)
        {
            set_parms();
            if (!secret_key.ntt_ || secret_key.parms_id() != context_.key_parms_id() || secret_key.ntt_->size() != k_ * n_)
            {
                throw std::invalid_argument("secret key is not valid for encryption parameters");
            }
            sk_ = secret_key;
        }
        const SecretKey &secret_key() const
        {
            return sk_;
        }
        void create_public_key(PublicKey &destination) const
        {
            destination.ct_.resize(context_, context_.key_parms_id(), 2);
            encrypt_zero_symmetric(destination.ct_.device_data());
            destination.ct_.is_ntt_form() = true;
            destination.ct_.scale() = 1.0;
        }
        // relinearization key for s^2 (SEAL/keygenerator.cpp:129-168)
        void create_relin_keys(RelinKeys &destination)
        {
            generate_into(destination, relin_plan(k_ - 1), New::s_squared, Draw::host);
        }
        // keys for the given Galois elements (SEAL/keygenerator.cpp:170-235), generated in the order given, an element
        // mentioned again skipped.  Every element is checked before the first key is generated (util::galois_key_plan): a call
        // that refuses one leaves the destination as it was and draws no randomness.
        void create_galois_keys(const std::vector<std::uint32_t> &galois_elts, GaloisKeys &destination)
        {
            generate_into(destination, galois_plan(galois_elts, nullptr), New::rotated, Draw::host);
        }

        // ---- device key generation (opt-in, moai_fused::create_*; not part of the reference API) ------------------------
        // The same keys drawn on the device from util::DeviceRng streams: one moai_encrypt_symmetric for the public key and
        // one moai_kswitch_keygen per switching key (all k-1 digits in one chain of launches).
        void create_public_key_device(PublicKey &destination) const
        {
            destination.ct_.resize(context_, context_.key_parms_id(), 2);
            util::hip_check(moai_encrypt_symmetric(context_.device(), rng_->key(), rng_->take(1), sk_.ntt_->get(), nullptr,
                                                   destination.ct_.device_data(), 1, k_, nullptr, context_.stream()));
            destination.ct_.is_ntt_form() = true;
            destination.ct_.scale() = 1.0;
            context_.sync();
        }
        void create_relin_keys_device(RelinKeys &destination)
        {
            generate_into(destination, relin_plan(k_ - 1), New::s_squared, Draw::device);
        }
        void create_galois_keys_device(const std::vector<std::uint32_t> &galois_elts, GaloisKeys &destination)
        {
            generate_into(destination, galois_plan(galois_elts, nullptr), New::rotated, Draw::device);
        }
        // ---- seeded keys for the wire (SEAL/keygenerator.h:92-118, 138-160, 190-300: the overloads without a destination) ----
        // c0 of every key digit from moai_kswitch_keygen_seeded and the public seed of the key; the uniform halves are drawn
        // where the key is loaded (moai_expand_seeded).  The key's digits take the sequences [seq, seq + k - 1) of the device
        // generator for their noise, and the same sequences under the key's own seed for a.
        Serializable<PublicKey> create_public_key() const
        {
            wire::Object o = seeded_object(wire::kind_public_key);
            o.head = util::seeded_encryption(wire::kind_public_key, k_, context_.key_parms_id(), sk_.ntt_->get(), nullptr, *rng_, context_);
            context_.sync();
            return Serializable<PublicKey>(std::move(o));
        }
        Serializable<RelinKeys> create_relin_keys()
        {
            return Serializable<RelinKeys>(generate_seeded(relin_plan(k_ - 1), New::s_squared, Seeds::either));
        }
        // the keys in the order of their slots, as a saved set holds them
        Serializable<GaloisKeys> create_galois_keys(const std::vector<std::uint32_t> &galois_elts)
        {
            return Serializable<GaloisKeys>(generate_seeded(by_slot(galois_plan(galois_elts, nullptr)), New::rotated, Seeds::either));
        }
        Serializable<GaloisKeys> create_galois_keys(const std::vector<int> &steps)
        {
            return create_galois_keys(galois_elts_from_steps(steps));
        }
        Serializable<GaloisKeys> create_galois_keys()
        {
            return create_galois_keys(galois_elts_all());
        }
        // ---- keys limited to a chain index (not part of the reference API; include/moai_hip.h, "keys limited to a chain index") ----
        // A key that is only used at chain index <= c is generated, shipped and loaded as the digits J < c + 1 and the rows
        // {0 .. c, special prime} a switch reads there (SEAL/evaluator.cpp:2818, 2831): (c+1)(c+2) / ((k-1) k) of the key.
        // c >= k-2 gives a full key.  Every key, limited or not, reserves k-1 sequences of the device generator, so a generator
        // with a fixed secret key and a fixed DeviceRng(key, first_sequence) produces, key for key, the trim of what it would
        // have produced in full.  chain_indices: one entry per element, or a single entry for all.
        Serializable<RelinKeys> create_relin_keys_limited(std::size_t chain_index)
        {
            return Serializable<RelinKeys>(generate_seeded(relin_plan(util::levels_of(chain_index, k_)), New::s_squared, Seeds::chacha20_only));
        }
        // the first mention of an element decides its levels; then the keys in the order of their slots, as create_galois_keys writes them
        Serializable<GaloisKeys> create_galois_keys_limited(const std::vector<std::uint32_t> &galois_elts,
                                                            const std::vector<std::size_t> &chain_indices)
        {
            return Serializable<GaloisKeys>(generate_seeded(by_slot(galois_plan(galois_elts, &chain_indices)), New::rotated, Seeds::chacha20_only));
        }
        // the same into a destination, drawn on the device like moai_fused::create_*_keys (a and e from the generator's one key),
        // in the order given
        void create_relin_keys_limited_device(std::size_t chain_index, RelinKeys &destination)
        {
            generate_into(destination, relin_plan(util::levels_of(chain_index, k_)), New::s_squared, Draw::device);
        }
        void create_galois_keys_limited_device(const std::vector<std::uint32_t> &galois_elts, const std::vector<std::size_t> &chain_indices,
                                               GaloisKeys &destination)
        {
            generate_into(destination, galois_plan(galois_elts, &chain_indices), New::rotated, Draw::device);
        }
        // the randomness of the device paths (a fresh OS-keyed one by default)
        void set_device_rng(std::shared_ptr<util::DeviceRng> rng)
        {
            if (!rng)
            {
                throw std::invalid_argument("rng cannot be null");
            }
            rng_ = std::move(rng);
        }
        const std::shared_ptr<util::DeviceRng> &device_rng() const
        {
            return rng_;
        }
        // GaloisTool::get_elts_all (SEAL/util/galois.cpp:106-131): the conjugation and every power-of-two rotation
        std::vector<std::uint32_t> galois_elts_all() const
        {
            std::vector<std::uint32_t> elts;
            const std::uint64_t m = static_cast<std::uint64_t>(n_) << 1;
            elts.push_back(static_cast<std::uint32_t>(m - 1));
            std::uint64_t pos = 5, neg = 0;
            for (std::uint64_t x = 1; x < m; x += 2)
            {
                if (((x * 5) & (m - 1)) == 1)
                {
                    neg = x;
                    break;
                }
            }
            for (int i = 0; i < context_.logn() - 1; i++)
            {
                elts.push_back(static_cast<std::uint32_t>(pos));
                pos = (pos * pos) & (m - 1);
                elts.push_back(static_cast<std::uint32_t>(neg));
                neg = (neg * neg) & (m - 1);
            }
            return elts;
        }
        std::vector<std::uint32_t> galois_elts_from_steps(const std::vector<int> &steps) const
        {
            std::vector<std::uint32_t> elts;
            for (int s : steps)
            {
                std::uint32_t e = moai_galois_elt_from_step(context_.device(), s);
                if (!e)
                {
                    throw std::invalid_argument("step count too large");
                }
                elts.push_back(e);
            }
            return elts;
        }
        void create_galois_keys(const std::vector<int> &steps, GaloisKeys &destination)
        {
            create_galois_keys(galois_elts_from_steps(steps), destination);
        }
        // all power-of-two rotations and the conjugation (GaloisTool::get_elts_all,
        // SEAL/util/galois.cpp:106-131)
        void create_galois_keys(GaloisKeys &destination)
        {
            create_galois_keys(galois_elts_all(), destination);
        }

    private:
        void set_parms()
        {
            for (auto &m : context_.key_context_data()->parms().coeff_modulus())
            {
                primes_.push_back(m.value());
            }
            n_ = context_.n();
            k_ = primes_.size();
        }
        void require_keyswitching() const
        {
            if (!context_.using_keyswitching())
            {
                throw std::logic_error("keyswitching is not supported by the context");
            }
        }
        wire::Object seeded_object(std::uint32_t kind) const
        {
            wire::Object o;
            o.dev = context_.device();
            o.stream = context_.stream();
            o.is_set = kind != wire::kind_public_key;
            o.head.kind = kind;
            o.head.flags = wire::flag_ntt;
            o.head.L = static_cast<std::uint32_t>(k_);
            o.head.parms_id = context_.key_parms_id();
            return o;
        }

        // ---- switching keys: every create_*_keys member is a plan (what to generate, in which order), a new key per slot and
        // a place for the finished key.  The order of a plan is the order in which its keys take their sequences of the device
        // generator: k-1 per key, limited or not. ------------------------------------------------------------------------------
        enum class New
        {
            s_squared, // the relinearization key: slot 0 switches from s^2
            rotated    // Galois keys: slot i switches from s under the element 2 i + 1
        };
        enum class Draw
        {
            host,  // the reference's construction with host randomness (make_kswitch_key)
            device // moai_kswitch_keygen / moai_kswitch_keygen_limited with util::DeviceRng randomness
        };
        enum class Seeds
        {
            either,       // whichever kind the device generator is set to
            chacha20_only // the members that limit keys: SEAL's format has no limited key
        };
        util::KeyPlan relin_plan(std::size_t levels) const
        {
            require_keyswitching();
            return util::KeyPlan{ { 0, levels } };
        }
        util::KeyPlan galois_plan(const std::vector<std::uint32_t> &galois_elts, const std::vector<std::size_t> *chain_indices) const
        {
            require_keyswitching();
            return util::galois_key_plan(galois_elts, chain_indices, n_, k_);
        }
        static util::KeyPlan by_slot(util::KeyPlan plan)
        {
            std::stable_sort(plan.begin(), plan.end(),
                             [](const util::KeyPlan::value_type &a, const util::KeyPlan::value_type &b) { return a.first < b.first; });
            return plan;
        }
        // walks a plan: sink(slot, levels, new_key_ntt) with the new key [k][N] of each slot in turn
        template <typename Sink>
        void generate(const util::KeyPlan &plan, New what, Sink sink) const
        {
            util::DeviceArray new_key(k_ * n_, context_.stream());
            if (what == New::s_squared)
            {
                util::hip_check(moai_dyadic_mul(context_.device(), sk_.ntt_->get(), sk_.ntt_->get(), new_key.get(), 1, 1, k_,
                                                context_.stream()));
            }
            for (const auto &p : plan)
            {
                if (what == New::rotated)
                {
                    util::hip_check(moai_galois_permute(context_.device(), sk_.ntt_->get(), new_key.get(), 1, k_,
                                                        static_cast<std::uint32_t>(2 * p.first + 1), context_.stream()));
                }
                sink(p.first, p.second, new_key.get());
            }
            context_.sync();
        }
        // the plan's keys replace the set in `destination` (KSwitchKeys::reset: with it go the hoisting constants and the
        // residency record of the keys it held)
        void generate_into(KSwitchKeys &destination, const util::KeyPlan &plan, New what, Draw draw) const
        {
            destination.reset(what == New::s_squared ? 1 : n_, context_.key_parms_id());
            generate(plan, what, [&](std::size_t slot, std::size_t levels, const std::uint64_t *new_key_ntt) {
                if (draw == Draw::host)
                {
                    destination.keys_[slot] = make_kswitch_key(new_key_ntt);
                    return;
                }
                // all digits in one chain of launches; a key limited below k-1 levels in the trimmed layout, with no full key behind it
                const bool whole = levels == k_ - 1;
                auto key = whole ? std::make_shared<util::DeviceArray>((k_ - 1) * 2 * k_ * n_, context_.stream()) : wire::limited_key_block(context_, levels);
                const std::uint64_t seq = rng_->take(k_ - 1);
                util::hip_check(whole ? moai_kswitch_keygen(context_.device(), rng_->key(), seq, sk_.ntt_->get(), new_key_ntt, key->get(), context_.stream())
                                      : moai_kswitch_keygen_limited(context_.device(), rng_->key(), seq, sk_.ntt_->get(), new_key_ntt, levels,
                                                                    key->get(), context_.stream()));
                destination.keys_[slot] = key;
                if (!whole)
                {
                    destination.mark_born_limited(context_, slot, levels);
                }
            });
        }
        // the plan's keys as a seeded set for the wire: c0 of every digit, the whole key (record kind 9) at levels == k-1, otherwise
        // the limited one (kind 10)
        wire::Object generate_seeded(const util::KeyPlan &plan, New what, Seeds seeds) const
        {
            wire::Object o = seeded_object(what == New::s_squared ? wire::kind_relin_keys : wire::kind_galois_keys);
            generate(plan, what, [&](std::size_t slot, std::size_t levels, const std::uint64_t *new_key_ntt) {
                if (seeds == Seeds::chacha20_only && rng_->get_seed_kind() == util::seed_kind::seal_blake2xb)
                {
                    throw std::logic_error("a key limited to a chain index has no form in SEAL's format: generate it under seed_kind::chacha20");
                }
                const bool whole = levels == k_ - 1;
                wire::Record r = util::seeded_record_head(whole ? wire::kind_kswitch_key : wire::kind_kswitch_key_limited, 2 * levels, levels + 1,
                                                          context_.key_parms_id(), levels * (levels + 1) * n_, context_);
                std::uint64_t *c0 = r.block->get();
                util::fill_seeded_record(
                    r, *rng_, k_ - 1, context_.stream(),
                    [&](std::uint64_t seq) {
                        return whole ? moai_kswitch_keygen_seeded(context_.device(), rng_->key(), r.seed, seq, sk_.ntt_->get(), new_key_ntt, c0,
                                                                  context_.stream())
                                     : moai_kswitch_keygen_limited_seeded(context_.device(), rng_->key(), r.seed, seq, sk_.ntt_->get(), new_key_ntt,
                                                                          levels, c0, context_.stream());
                    },
                    // whole keys only: a of digit J from the SEAL seed of sequence seq + J
                    [&](std::uint64_t seq, std::uint32_t *rejected) {
                        return moai_kswitch_keygen_seal_seeded(context_.device(), rng_->key(), r.seal_seeds.data(), seq, sk_.ntt_->get(), new_key_ntt,
                                                               c0, rejected, context_.stream());
                    });
                o.indices.push_back(slot);
                o.keys.push_back(std::move(r));
            });
            o.head.count = static_cast<std::uint32_t>(o.keys.size());
            return o;
        }
        void upload_ntt(const std::vector<std::uint64_t> &rns, util::DeviceArray &dst, std::size_t rows) const
        {
            util::hip_check(moai_memcpy_h2d(dst.get(), rns.data(), rows * n_ * 8, context_.stream()));
            context_.sync();
            util::hip_check(moai_ntt_forward(context_.device(), dst.get(), 1, rows, nullptr, context_.stream()));
        }
        // (c0, c1) = (-(a s) + e, a) at the key level, NTT form, written to dst [2][k][N]
        void encrypt_zero_symmetric(std::uint64_t *dst) const
        {
            std::vector<std::uint64_t> a;
            util::sample_uniform(primes_, n_, a);
            std::vector<std::int64_t> e;
            util::sample_noise(n_, e);
            std::vector<std::uint64_t> e_rns;
            util::to_rns(e, primes_, e_rns);
            std::uint64_t *c0 = dst;
            std::uint64_t *c1 = dst + k_ * n_;
            util::hip_check(moai_memcpy_h2d(c1, a.data(), k_ * n_ * 8, context_.stream()));
            util::hip_check(moai_memcpy_h2d(c0, e_rns.data(), k_ * n_ * 8, context_.stream()));
            context_.sync();
            util::hip_check(moai_ntt_forward(context_.device(), c0, 1, k_, nullptr, context_.stream()));
            util::DeviceArray as(k_ * n_, context_.stream());
            util::hip_check(moai_dyadic_mul(context_.device(), c1, sk_.ntt_->get(), as.get(), 1, 1, k_, context_.stream()));
            util::hip_check(moai_sub(context_.device(), c0, as.get(), c0, 1, k_, context_.stream()));
            context_.sync();
        }
        // SEAL/keygenerator.cpp:303-336: key[J] = Enc(0) with c0's row J += (p mod q_J) * new_key[J]
        std::shared_ptr<util::DeviceArray> make_kswitch_key(const std::uint64_t *new_key_ntt) const
        {
            const std::size_t digits = k_ - 1;
            auto key = std::make_shared<util::DeviceArray>(digits * 2 * k_ * n_, context_.stream());
            util::DeviceArray scaled(k_ * n_, context_.stream());
            std::vector<std::uint64_t> factor(k_, 0);
            for (std::size_t j = 0; j < k_; j++)
            {
                factor[j] = primes_[k_ - 1] % primes_[j];
            }
            util::hip_check(moai_mul_scalar_rows(context_.device(), new_key_ntt, factor.data(), scaled.get(), 1, k_,
                                                 context_.stream()));
            // The digits are independent encryptions of zero: host threads draw their randomness side by side (a key at
            // MOAI's size is 35 x 2 x 36 x 65536 samples) and enqueue on the context's one stream, where each digit's own
            // operations keep their order.  Every thread adds through its own addend [k][N], zero except row J =
            // (p mod q_J) * new_key[J].
            std::exception_ptr failure;
#pragma omp parallel
            {
                std::unique_ptr<util::DeviceArray> sparse;
#pragma omp for schedule(dynamic)
                for (std::size_t J = 0; J < digits; J++)
                {
                    try
                    {
                        if (!sparse)
                        {
                            sparse.reset(new util::DeviceArray(k_ * n_, context_.stream()));
                            util::hip_check(moai_memset_zero(sparse->get(), k_ * n_ * 8, context_.stream()));
                        }
                        std::uint64_t *ct = key->get() + J * 2 * k_ * n_;
                        encrypt_zero_symmetric(ct);
                        util::hip_check(moai_memcpy_d2d(sparse->get() + J * n_, scaled.get() + J * n_, n_ * 8, context_.stream()));
                        util::hip_check(moai_add(context_.device(), ct, sparse->get(), ct, 1, k_, context_.stream()));
                        util::hip_check(moai_memset_zero(sparse->get() + J * n_, n_ * 8, context_.stream()));
                    }
                    catch (...)
                    {
#pragma omp critical(moai_keygen_failure)
                        failure = std::current_exception();
                    }
                }
                if (sparse)
                {
                    context_.sync(); // before this thread's addend is released
                }
            }
            if (failure)
            {
                std::rethrow_exception(failure);
            }
            context_.sync();
            return key;
        }

        SEALContext context_;
        std::vector<std::uint64_t> primes_;
        std::size_t n_ = 0, k_ = 0;
        SecretKey sk_;
        std::shared_ptr<util::DeviceRng> rng_ = std::make_shared<util::DeviceRng>();
    };

    // =================================================================================================
    // Encryptor / Decryptor
    // =================================================================================================
    class Encryptor
    {
    public:
        Encryptor(const SEALContext &context, const PublicKey &public_key) : context_(context), pk_(public_key.data())
        {}
        // symmetric encryption runs on the device (moai_encrypt_symmetric) with util::DeviceRng randomness
        Encryptor(const SEALContext &context, const SecretKey &secret_key) : context_(context), sk_(secret_key.ntt_)
        {}
        Encryptor(const SEALContext &context, const PublicKey &public_key, const SecretKey &secret_key)
            : context_(context), pk_(public_key.data()), sk_(secret_key.ntt_)
        {}
        void set_public_key(const PublicKey &public_key)
        {
            pk_ = public_key.data();
        }
        void set_secret_key(const SecretKey &secret_key)
        {
            sk_ = secret_key.ntt_;
        }
        // Encryptor::encrypt_symmetric (SEAL/encryptor.h:337-372, encryptor.cpp:88-120): one moai_encrypt_symmetric launch chain
        void encrypt_symmetric(const Plaintext &plain, Ciphertext &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            const std::size_t L = check_plain(plain);
            // a vector plaintext goes into the encryption call; only constant rows are added afterwards
            encrypt_symmetric_device(plain.parms_id(), plain.is_scalar() ? nullptr : plain.device_data(), destination);
            if (plain.is_scalar())
            {
                add_plain(destination.device_data(), plain, L);
            }
            destination.scale() = plain.scale();
            context_.sync();
        }
        void encrypt_zero_symmetric(parms_id_type parms_id, Ciphertext &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encrypt_symmetric_device(parms_id, nullptr, destination);
            context_.sync();
        }
        void encrypt_zero_symmetric(Ciphertext &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encrypt_zero_symmetric(context_.first_parms_id(), destination);
        }
        // ---- seeded ciphertexts for the wire (SEAL/encryptor.h:374-404, 430-478: the overloads without a destination) -----
        // c0 from moai_encrypt_symmetric_seeded and the public seed; c1 is drawn where the ciphertext is loaded
        Serializable<Ciphertext> encrypt_symmetric(const Plaintext &plain, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            const std::size_t L = check_plain(plain);
            wire::Object o = seeded_ciphertext(plain.parms_id(), plain.is_scalar() ? nullptr : plain.device_data());
            if (plain.is_scalar())
            {
                add_plain(o.head.block->get(), plain, L);
            }
            o.head.scale = plain.scale();
            context_.sync();
            return Serializable<Ciphertext>(std::move(o));
        }
        Serializable<Ciphertext> encrypt_zero_symmetric(parms_id_type parms_id, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            wire::Object o = seeded_ciphertext(parms_id, nullptr);
            context_.sync();
            return Serializable<Ciphertext>(std::move(o));
        }
        Serializable<Ciphertext> encrypt_zero_symmetric(MemoryPoolHandle = MemoryPoolHandle()) const
        {
            return encrypt_zero_symmetric(context_.first_parms_id());
        }
        // ---- for moai_fused (not part of the reference API) ----------------------------------------------------------------
        // the key-level public key [2][k][N] on the device, null when none is set
        const std::uint64_t *public_key_device() const
        {
            return pk_.size() ? pk_.device_data() : nullptr;
        }
        // the secret key in NTT form over all primes, [k][N] on the device, null when none is set
        const std::uint64_t *secret_key_device() const
        {
            return sk_ ? sk_->get() : nullptr;
        }
        const SEALContext &context() const
        {
            return context_;
        }
        void set_device_rng(std::shared_ptr<util::DeviceRng> rng)
        {
            if (!rng)
            {
                throw std::invalid_argument("rng cannot be null");
            }
            rng_ = std::move(rng);
        }
        const std::shared_ptr<util::DeviceRng> &device_rng() const
        {
            return rng_;
        }
        // public-key encryption at the level of `plain` (SEAL/encryptor.cpp encrypt_internal; the
        // reference samples at the key level and divides by the special prime, here the public key is
        // restricted to the plaintext's primes -- a fresh RLWE encryption either way)
        void encrypt(const Plaintext &plain, Ciphertext &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            const std::size_t L = check_plain(plain);
            encrypt_zero(plain.parms_id(), destination);
            add_plain(destination.device_data(), plain, L);
            destination.scale() = plain.scale();
        }
        void encrypt_zero(parms_id_type parms_id, Ciphertext &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            const std::size_t L = level_of(parms_id), n = context_.n();
            if (!pk_.size())
            {
                throw std::logic_error("public key is not set");
            }
            const std::size_t k = context_.key_context_data()->parms().coeff_modulus().size();
            const auto cd = context_.get_context_data(parms_id);
            std::vector<std::uint64_t> primes;
            for (auto &m : cd->parms().coeff_modulus())
            {
                primes.push_back(m.value());
            }
            destination.resize(context_, parms_id, 2);
            destination.is_ntt_form() = true;
            destination.scale() = 1.0;
            // u ternary, e0, e1 noise
            std::vector<std::int64_t> u, e0, e1;
            util::sample_ternary(n, 0, u);
            util::sample_noise(n, e0);
            util::sample_noise(n, e1);
            std::vector<std::uint64_t> u_rns, e_rns(2 * L * n), tmp;
            util::to_rns(u, primes, u_rns);
            util::to_rns(e0, primes, tmp);
            std::copy(tmp.begin(), tmp.end(), e_rns.begin());
            util::to_rns(e1, primes, tmp);
            std::copy(tmp.begin(), tmp.end(), e_rns.begin() + static_cast<std::ptrdiff_t>(L * n));
            util::DeviceArray du(L * n, context_.stream());
            util::hip_check(moai_memcpy_h2d(du.get(), u_rns.data(), L * n * 8, context_.stream()));
            util::hip_check(moai_memcpy_h2d(destination.device_data(), e_rns.data(), 2 * L * n * 8, context_.stream()));
            context_.sync();
            util::hip_check(moai_ntt_forward(context_.device(), du.get(), 1, L, nullptr, context_.stream()));
            util::hip_check(moai_ntt_forward(context_.device(), destination.device_data(), 2, L, nullptr, context_.stream()));
            // c_i = pk_i * u + e_i over the first L primes of the key-level public key
            util::DeviceArray prod(L * n, context_.stream());
            for (int i = 0; i < 2; i++)
            {
                const std::uint64_t *pk_poly = pk_.device_data() + static_cast<std::size_t>(i) * k * n;
                std::uint64_t *c = destination.device_data() + static_cast<std::size_t>(i) * L * n;
                util::hip_check(moai_dyadic_mul(context_.device(), pk_poly, du.get(), prod.get(), 1, 1, L, context_.stream()));
                util::hip_check(moai_add(context_.device(), c, prod.get(), c, 1, L, context_.stream()));
            }
            context_.sync();
        }
        void encrypt_zero(Ciphertext &destination, MemoryPoolHandle = MemoryPoolHandle()) const
        {
            encrypt_zero(context_.first_parms_id(), destination);
        }

    private:
        // the number of primes at parms_id
        std::size_t level_of(const parms_id_type &parms_id) const
        {
            auto cd = context_.get_context_data(parms_id);
            if (!cd)
            {
                throw std::invalid_argument("parms_id is not valid for encryption parameters");
            }
            return cd->parms().coeff_modulus().size();
        }
        const std::uint64_t *require_secret_key() const
        {
            if (!sk_)
            {
                throw std::logic_error("secret key is not set");
            }
            return sk_->get();
        }
        // the number of primes of a plaintext that can be encrypted
        std::size_t check_plain(const Plaintext &plain) const
        {
            auto cd = context_.get_context_data(plain.parms_id());
            if (!cd || !plain.is_ntt_form())
            {
                throw std::invalid_argument("plain is not valid for encryption parameters");
            }
            return cd->parms().coeff_modulus().size();
        }
        // dst [L][N] += plain: its constant rows, or its vector
        void add_plain(std::uint64_t *dst, const Plaintext &plain, std::size_t L) const
        {
            util::hip_check(plain.is_scalar() ? moai_add_scalar_rows(context_.device(), dst, plain.scalar_rows().data(), dst, 1, L, context_.stream())
                                              : moai_add(context_.device(), dst, plain.device_data(), dst, 1, L, context_.stream()));
        }
        wire::Object seeded_ciphertext(parms_id_type parms_id, const std::uint64_t *plain) const
        {
            const std::size_t L = level_of(parms_id);
            wire::Object o;
            o.dev = context_.device();
            o.stream = context_.stream();
            o.head = util::seeded_encryption(wire::kind_ciphertext, L, parms_id, require_secret_key(), plain, *rng_, context_);
            return o;
        }
        void encrypt_symmetric_device(parms_id_type parms_id, const std::uint64_t *plain, Ciphertext &destination) const
        {
            const std::size_t L = level_of(parms_id);
            const std::uint64_t *sk = require_secret_key();
            destination.resize(context_, parms_id, 2);
            destination.is_ntt_form() = true;
            destination.scale() = 1.0;
            util::hip_check(moai_encrypt_symmetric(context_.device(), rng_->key(), rng_->take(1), sk, plain, destination.device_data(), 1, L, nullptr,
                                                   context_.stream()));
        }

        SEALContext context_;
        Ciphertext pk_;
        std::shared_ptr<util::DeviceArray> sk_;
        std::shared_ptr<util::DeviceRng> rng_ = std::make_shared<util::DeviceRng>();
    };

    class Decryptor
    {
    public:
        Decryptor(const SEALContext &context, const SecretKey &secret_key) : context_(context), sk_(secret_key.ntt_)
        {}
        // c0 + c1 s + c2 s^2 ... (SEAL/decryptor.cpp:131-205), one moai_decrypt launch
        void decrypt(const Ciphertext &encrypted, Plaintext &destination)
        {
            auto cd = context_.get_context_data(encrypted.parms_id());
            if (!cd || encrypted.size() < 2)
            {
                throw std::invalid_argument("encrypted is not valid for encryption parameters");
            }
            if (!encrypted.is_ntt_form())
            {
                throw std::invalid_argument("encrypted must be in NTT form");
            }
            if (encrypted.batch() != 1)
            {
                throw std::invalid_argument("packed ciphertext: moai_fused::unpack it before decrypting");
            }
            const std::size_t L = encrypted.coeff_modulus_size(), n = context_.n();
            destination.scalar_rows_.clear();
            destination.parms_id_ = encrypted.parms_id();
            destination.scale_ = encrypted.scale();
            destination.n_ = n;
            destination.L_ = L;
            destination.stream_ = context_.stream();
            destination.data_.resize(L * n, context_.stream());
            util::hip_check(moai_decrypt(context_.device(), encrypted.device_data(), encrypted.size(), sk_->get(),
                                         destination.data_.get(), 1, L, nullptr, context_.stream()));
            context_.sync();
        }

        // the secret key in NTT form over all primes, [k][N] on the device (moai_fused::decrypt_decode)
        const std::uint64_t *secret_key_device() const
        {
            return sk_->get();
        }
        const SEALContext &context() const
        {
            return context_;
        }

    private:
        SEALContext context_;
        std::shared_ptr<util::DeviceArray> sk_;
    };
} // namespace seal
