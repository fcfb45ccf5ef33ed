// seal/moai_seal_format.h -- Microsoft SEAL 4.1's own serialized format on the seal:: surface, compression mode `none`: what a
// stock SEAL client writes and expects back.  Included from seal/seal.h behind seal/moai_serialization.h, whose Object / Record
// describe an object on either side of both formats, so each type's to_wire() / from_wire() serve this one unchanged.
// tests/seal_format.py restates the bytes; DESIGN.md section 5.0f has the facts.
//
//   object  = SEALHeader (16 bytes: u16 magic 0xA15E, u8 16, u8 major, u8 minor, u8 compr_mode, u16 0, u64 total bytes) + members
//             (SEAL/serialization.h:76-91); nested objects (DynArray, Modulus, UniformRandomGeneratorInfo, each PublicKey of a
//             key set) carry their own header
//   Ciphertext, PublicKey     parms_id[4], u8 NTT form, u64 size, u64 N, u64 L, f64 scale, u64 correction factor, DynArray; a
//                             seeded one stores polynomial 0 alone, followed by UniformRandomGeneratorInfo (u8 type, 64-byte
//                             seed), and polynomial 1 is sample_poly_uniform of that seed (SEAL/ciphertext.cpp:190-381)
//   Plaintext, SecretKey      parms_id[4], u64 coefficient count, f64 scale, DynArray (SEAL/plaintext.cpp:205-300)
//   KSwitchKeys and derived   parms_id[4], u64 slots, per slot u64 digits and that many PublicKey (SEAL/kswitchkeys.cpp:45-140);
//                             GaloisKeys has N slots, slot (galois_elt - 1) / 2 (SEAL/galoiskeys.h)
//   EncryptionParameters      u8 scheme, u64 N, u64 L, L + 1 Modulus (the last one plain_modulus) (SEAL/encryptionparams.cpp:15-110)
//
// parms_id in these bytes is SEAL's (SEALContext::ContextData::seal_parms_id), mapped to and from the shim's own on the way.
// Load: the stored residues go to the device in one copy per stored object, straight into the block the object keeps; the
// seeded halves of a ciphertext or of a whole switching key come from ONE moai_seal_sample_uniform (Blake2xb on the device); the
// residue check (moai_check_residues) and the expansion's overflow word come back in one 16-byte copy.  A header that names zlib
// or zstd is rejected as SEAL built without them rejects it, Shake256 seeds with SEAL's "unsupported prng_type".
// Save: an object seeded with SEAL's own generator on this side (util::seed_kind::seal_blake2xb, wire::Record::seal_seeds) is
// written seeded, polynomial 0 and UniformRandomGeneratorInfo with type byte 1 per ciphertext or key digit, as SEAL's save_seed
// route writes it; what is seeded with ChaCha20, which SEAL cannot expand, is expanded first and written in full.
#pragma once

namespace seal
{
    namespace sealfmt
    {
        constexpr std::uint16_t magic = 0xA15E;
        constexpr std::size_t header_bytes = 16, ct_member_bytes = 73, pt_member_bytes = 48, prng_info_bytes = 16 + 1 + 64;

        struct Header
        {
            std::uint16_t magic;
            std::uint8_t header_size, version_major, version_minor, compr_mode;
            std::uint16_t reserved;
            std::uint64_t size;
        };
        static_assert(sizeof(Header) == header_bytes, "SEALHeader is 16 bytes");

        inline Header make_seal_header(std::size_t total)
        {
            return Header{ magic, static_cast<std::uint8_t>(header_bytes), 4, 1, 0, 0, total };
        }
        // Serialization::Load, SEAL/serialization.cpp:361-370: the version first, then the header as a build without zlib and
        // zstd judges it (IsValidHeader, SEAL/serialization.h:172-191)
        inline Header get_header(wire::Source &src)
        {
            Header h;
            std::memcpy(&h, src.view(header_bytes), header_bytes);
            if (h.version_major != 4)
            {
                throw std::logic_error("incompatible version");
            }
            if (h.magic != magic || h.header_size != header_bytes || h.compr_mode != 0)
            {
                throw std::logic_error("loaded SEALHeader is invalid");
            }
            return h;
        }
        // an object's header says how long the object was
        struct Scope
        {
            wire::Source &src;
            std::size_t start, size;
            explicit Scope(wire::Source &s) : src(s), start(s.consumed), size(sealfmt::get_header(s).size)
            {}
            void close() const
            {
                if (src.consumed - start != size)
                {
                    throw std::logic_error("invalid data size"); // SEAL/serialization.cpp:381-384
                }
            }
        };
        template <class T>
        inline T get(wire::Source &src)
        {
            T x;
            std::memcpy(&x, src.view(sizeof(T)), sizeof(T));
            return x;
        }
        inline parms_id_type get_id(wire::Source &src)
        {
            parms_id_type id;
            std::memcpy(id.data(), src.view(32), 32);
            return id;
        }
        inline std::size_t dyn_bytes(std::size_t words)
        {
            return header_bytes + 8 + 8 * words;
        }
        inline parms_id_type id_of(moai_ctx *dev, std::size_t L)
        {
            std::vector<std::uint64_t> primes(L);
            for (std::size_t i = 0; i < L; i++)
            {
                primes[i] = moai_ctx_prime(dev, i);
            }
            return util::seal_parms_id(moai_ctx_coeff_count(dev), primes);
        }
        inline bool is_set(std::uint32_t kind)
        {
            return kind == wire::kind_kswitch_keys || kind == wire::kind_relin_keys || kind == wire::kind_galois_keys;
        }
        inline bool is_plain(std::uint32_t kind)
        {
            return kind == wire::kind_plaintext || kind == wire::kind_secret_key;
        }

        // ---- sizes --------------------------------------------------------------------------------------------------------
        // a seeded Ciphertext / PublicKey: polynomial 0 and the generator's info (SEAL/ciphertext.cpp:190-247)
        inline std::size_t seeded_ct_bytes(std::size_t LN)
        {
            return header_bytes + ct_member_bytes + dyn_bytes(LN) + prng_info_bytes;
        }
        inline std::size_t record_bytes(const wire::Object &o, const wire::Record &r)
        {
            const std::size_t LN = r.L * moai_ctx_coeff_count(o.dev);
            if (r.seal_seeded())
            {
                return r.stored() * seeded_ct_bytes(LN);
            }
            return header_bytes + (is_plain(r.kind) ? pt_member_bytes + dyn_bytes(LN) : ct_member_bytes + dyn_bytes(r.count * LN));
        }
        inline std::size_t slots(const wire::Object &o)
        {
            if (o.head.kind == wire::kind_galois_keys)
            {
                return moai_ctx_coeff_count(o.dev); // KeyGenerator::create_galois_keys resizes to N, SEAL/keygenerator.cpp:208
            }
            return o.indices.empty() ? 0 : static_cast<std::size_t>(o.indices.back()) + 1;
        }
        inline std::size_t object_bytes(const wire::Object &o)
        {
            if (!o.dev)
            {
                throw std::logic_error("object is empty or its context is gone");
            }
            if (!o.is_set)
            {
                return sealfmt::record_bytes(o, o.head);
            }
            for (auto &r : o.keys)
            {
                if (r.kind == wire::kind_kswitch_key_limited)
                {
                    throw std::logic_error("a key limited to a chain index has no form in SEAL's format: save it in this library's own");
                }
            }
            const std::size_t n = moai_ctx_coeff_count(o.dev), k = o.head.L;
            const std::size_t digit = header_bytes + ct_member_bytes + dyn_bytes(2 * k * n);
            std::size_t bytes = header_bytes + 32 + 8 + 8 * slots(o);
            for (auto &r : o.keys)
            {
                bytes += (k - 1) * (r.seal_seeded() ? seeded_ct_bytes(k * n) : digit);
            }
            return bytes;
        }

        // ---- save ---------------------------------------------------------------------------------------------------------
        inline void put_data(const wire::Object &o, const std::uint64_t *dev_words, std::size_t words, wire::Sink &sink)
        {
            const Header h = make_seal_header(dyn_bytes(words));
            const std::uint64_t size64 = words;
            sink.put(&h, sizeof(h));
            sink.put(&size64, 8);
            std::uint8_t *dst = sink.space(words * 8);
            util::hip_check(moai_memcpy_d2h(dst, dev_words, words * 8, o.stream));
            util::hip_check(moai_stream_sync(o.stream));
            sink.commit();
        }
        // one Ciphertext / PublicKey: `polys` polynomials of L rows at dev_words; seal_seed: polynomial 0 alone is there and stored,
        // followed by UniformRandomGeneratorInfo { blake2xb, the 64 bytes }
        inline void put_ct(const wire::Object &o, const std::uint64_t *dev_words, std::size_t polys, std::size_t L, bool ntt, double scale,
                           wire::Sink &sink, const std::uint8_t *seal_seed = nullptr)
        {
            const std::size_t n = moai_ctx_coeff_count(o.dev), stored = seal_seed ? 1 : polys;
            const Header h = make_seal_header(seal_seed ? seeded_ct_bytes(L * n) : header_bytes + ct_member_bytes + dyn_bytes(polys * L * n));
            sink.put(&h, sizeof(h));
            const parms_id_type id = id_of(o.dev, L);
            const std::uint8_t ntt_byte = ntt ? 1 : 0;
            const std::uint64_t f[3] = { polys, n, L }, correction = 1;
            sink.put(id.data(), 32);
            sink.put(&ntt_byte, 1);
            sink.put(f, 24);
            sink.put(&scale, 8);
            sink.put(&correction, 8);
            put_data(o, dev_words, stored * L * n, sink);
            if (seal_seed)
            {
                const Header info = make_seal_header(prng_info_bytes);
                const std::uint8_t type = 1; // prng_type::blake2xb
                sink.put(&info, sizeof(info));
                sink.put(&type, 1);
                sink.put(seal_seed, 64);
            }
        }
        inline void put_record(const wire::Object &o, const wire::Record &r, wire::Sink &sink)
        {
            const std::size_t n = moai_ctx_coeff_count(o.dev), LN = r.L * n;
            if (r.seal_seeded())
            {
                // seeded with SEAL's generator: every ciphertext or key digit goes out as polynomial 0 and its seed
                const wire::SealOverflow overflow(o, r);
                for (std::size_t j = 0; j < r.stored(); j++)
                {
                    const bool key = r.kind == wire::kind_kswitch_key;
                    put_ct(o, r.data + j * LN, 2, r.L, key || (r.flags & wire::flag_ntt) != 0, key ? 1.0 : r.scale, sink,
                           r.seal_seeds.data() + 64 * j);
                    overflow.settle(); // put_ct has synchronised
                }
                return;
            }
            // seeded on this side: ChaCha20, which SEAL cannot expand
            const std::uint64_t *data = r.data;
            util::DeviceArray full;
            if (r.flags & wire::flag_seeded)
            {
                full.resize(r.count * LN, o.stream);
                util::hip_check(moai_expand_seeded(o.dev, r.seed, r.seq, r.data, full.get(), r.stored(), r.L, nullptr, o.stream));
                data = full.get();
            }
            if (is_plain(r.kind))
            {
                const Header h = make_seal_header(sealfmt::record_bytes(o, r));
                const parms_id_type id = id_of(o.dev, r.L);
                const std::uint64_t count = LN;
                const double scale = r.kind == wire::kind_secret_key ? 1.0 : r.scale;
                sink.put(&h, sizeof(h));
                sink.put(id.data(), 32);
                sink.put(&count, 8);
                sink.put(&scale, 8);
                put_data(o, data, LN, sink);
                return;
            }
            if (r.kind == wire::kind_kswitch_key)
            {
                for (std::size_t j = 0; j < r.count / 2; j++)
                {
                    put_ct(o, data + j * 2 * LN, 2, r.L, true, 1.0, sink);
                }
                return;
            }
            put_ct(o, data, r.count, r.L, (r.flags & wire::flag_ntt) != 0, r.scale, sink);
        }
        inline std::streamoff save_object(const wire::Object &o, wire::Sink &sink)
        {
            const std::size_t total = sealfmt::object_bytes(o);
            if (!o.is_set)
            {
                sealfmt::put_record(o, o.head, sink);
                return static_cast<std::streamoff>(total);
            }
            const Header h = make_seal_header(total);
            const parms_id_type id = id_of(o.dev, o.head.L);
            const std::uint64_t dim1 = slots(o);
            sink.put(&h, sizeof(h));
            sink.put(id.data(), 32);
            sink.put(&dim1, 8);
            std::size_t next = 0;
            for (std::uint64_t slot = 0; slot < dim1; slot++)
            {
                const bool here = next < o.indices.size() && o.indices[next] == slot;
                const std::uint64_t dim2 = here ? o.head.L - 1 : 0;
                sink.put(&dim2, 8);
                if (here)
                {
                    sealfmt::put_record(o, o.keys[next++], sink);
                }
            }
            return static_cast<std::streamoff>(total);
        }

        // ---- load ---------------------------------------------------------------------------------------------------------
        struct Loader
        {
            const SEALContext &context;
            wire::Source &src;
            bool check;
            moai_ctx *dev;
            void *st;
            std::size_t n;
            util::DeviceArray flags; // as uint32_t: [0] a residue >= its prime, [2] rejected words, [3] a tail ran over its bound
            bool flagged = false;

            Loader(const SEALContext &c, wire::Source &s, bool chk) : context(c), src(s), check(chk), dev(c.device()), st(c.stream()), n(c.n())
            {
                if (!context.parameters_set())
                {
                    throw std::invalid_argument("encryption parameters are not set correctly");
                }
            }
            std::uint32_t *flag(std::size_t i)
            {
                if (!flagged)
                {
                    flags.resize(2, st);
                    util::hip_check(moai_memset_zero(flags.get(), 16, st));
                    flagged = true;
                }
                return reinterpret_cast<std::uint32_t *>(flags.get()) + i;
            }
            void to_device(std::uint64_t *dst, std::size_t words)
            {
                const std::uint8_t *bytes = src.view(words * 8);
                util::hip_check(moai_memcpy_h2d(dst, bytes, words * 8, st));
                if (!src.stable())
                {
                    context.sync(); // the next view reuses the staging bytes
                }
            }
            void residues(const std::uint64_t *data, std::size_t polys, std::size_t L)
            {
                if (check)
                {
                    util::hip_check(moai_check_residues(dev, data, polys, L, nullptr, flag(0), st));
                }
            }
            // one read-back for the whole object
            void settle(const char *what)
            {
                std::uint32_t f[4] = { 0, 0, 0, 0 };
                if (flagged)
                {
                    util::hip_check(moai_memcpy_d2h(f, flags.get(), 16, st));
                }
                context.sync();
                if (f[3])
                {
                    throw std::logic_error("ciphertext data is invalid"); // a seed whose expansion does not end
                }
                if (f[0])
                {
                    throw std::logic_error(std::string(what) + " data is invalid"); // is_valid_for, SEAL/valcheck.cpp:302-335
                }
            }

            // the members of a Ciphertext or PublicKey up to and including the DynArray's size
            struct CtMeta
            {
                parms_id_type id = parms_id_zero; // the shim's own
                bool ntt = false, seeded = false;
                std::size_t size = 0, L = 0;
                double scale = 1.0;
                Scope whole, dyn;
            };
            CtMeta ct_meta(std::size_t max_size)
            {
                Scope whole(src);
                const parms_id_type seal_id = get_id(src);
                const std::uint8_t ntt = get<std::uint8_t>(src);
                const std::uint64_t size = get<std::uint64_t>(src), N = get<std::uint64_t>(src), L = get<std::uint64_t>(src);
                const double scale = get<double>(src);
                (void)get<std::uint64_t>(src); // correction_factor: BGV only
                auto cd = context.get_context_data_seal(seal_id);
                // is_metadata_valid_for, SEAL/valcheck.cpp:44-80; key levels allowed as in Ciphertext::load_members
                if (!cd || N != n || L != cd->parms().coeff_modulus().size() || size < 2 || size > max_size)
                {
                    throw std::logic_error("ciphertext data is invalid");
                }
                Scope dyn(src);
                const std::uint64_t words = get<std::uint64_t>(src);
                const bool seeded = size == 2 && words == L * n;
                if (!seeded && words != size * L * n)
                {
                    throw std::logic_error("ciphertext data is invalid");
                }
                return CtMeta{ cd->parms_id(), ntt != 0, seeded, static_cast<std::size_t>(size), static_cast<std::size_t>(L), scale, whole, dyn };
            }
            // the residues into dst [size][L][N] (a seeded one: polynomial 0 only) and, seeded, the seed appended to `seeds`
            void ct_data(const CtMeta &m, std::uint64_t *dst, std::vector<std::uint8_t> &seeds)
            {
                to_device(dst, (m.seeded ? 1 : m.size) * m.L * n);
                m.dyn.close();
                if (m.seeded)
                {
                    Scope info(src);
                    const std::uint8_t *p = src.view(65);
                    if (p[0] != 1) // prng_type::blake2xb; make_prng gives none for anything else this build lacks
                    {
                        throw std::logic_error("unsupported prng_type"); // SEAL/ciphertext.cpp:127
                    }
                    seeds.insert(seeds.end(), p + 1, p + 65);
                    info.close();
                }
                m.whole.close();
            }
            void expand(const std::vector<std::uint8_t> &seeds, std::uint64_t *block, std::size_t L)
            {
                if (!seeds.empty())
                {
                    util::hip_check(moai_seal_sample_uniform(dev, seeds.data(), block + L * n, 2 * L * n, seeds.size() / 64, L, nullptr, flag(2), st));
                }
            }

            wire::Record ciphertext(std::uint32_t kind)
            {
                const CtMeta m = ct_meta(kind == wire::kind_public_key ? 2 : 6);
                // a ciphertext lives at a data level (is_valid_for without pure key levels, SEAL/ciphertext.h:520-525)
                if (kind == wire::kind_ciphertext && m.id == context.key_parms_id() && context.using_keyswitching())
                {
                    throw std::logic_error("ciphertext data is invalid");
                }
                wire::Record r;
                r.kind = kind;
                r.flags = m.ntt ? wire::flag_ntt : 0;
                r.count = static_cast<std::uint32_t>(m.size);
                r.L = static_cast<std::uint32_t>(m.L);
                r.scale = m.scale;
                r.parms_id = m.id;
                r.block = std::make_shared<util::DeviceArray>(m.size * m.L * n, st);
                r.data = r.block->get();
                std::vector<std::uint8_t> seeds;
                ct_data(m, r.block->get(), seeds);
                expand(seeds, r.block->get(), m.L);
                residues(r.data, m.size, m.L);
                return r;
            }
            wire::Record plaintext(std::uint32_t kind)
            {
                Scope whole(src);
                const parms_id_type seal_id = get_id(src);
                const std::uint64_t count = get<std::uint64_t>(src);
                const double scale = get<double>(src);
                auto cd = context.get_context_data_seal(seal_id);
                // CKKS plaintexts are in NTT form at a level of the chain (is_metadata_valid_for, SEAL/valcheck.cpp:19-42)
                if (!cd || count != cd->parms().coeff_modulus().size() * n)
                {
                    throw std::logic_error("plaintext data is invalid");
                }
                Scope dyn(src);
                if (get<std::uint64_t>(src) != count)
                {
                    throw std::logic_error("plaintext data is invalid");
                }
                wire::Record r;
                r.kind = kind;
                r.flags = wire::flag_ntt;
                r.count = 1;
                r.L = static_cast<std::uint32_t>(count / n);
                r.scale = scale;
                r.parms_id = cd->parms_id();
                r.block = std::make_shared<util::DeviceArray>(count, st);
                r.data = r.block->get();
                to_device(r.block->get(), count);
                dyn.close();
                whole.close();
                residues(r.data, 1, r.L);
                return r;
            }
            wire::Object key_set(std::uint32_t kind)
            {
                wire::Object o;
                o.dev = dev;
                o.stream = st;
                o.is_set = true;
                Scope whole(src);
                const parms_id_type seal_id = get_id(src);
                const std::uint64_t dim1 = get<std::uint64_t>(src);
                auto cd = context.get_context_data_seal(seal_id);
                const std::size_t k = context.key_context_data()->parms().coeff_modulus().size();
                if (!cd || cd->parms_id() != context.key_parms_id() || k < 2 || dim1 > n)
                {
                    throw std::logic_error("KSwitchKeys data is invalid"); // is_metadata_valid_for, SEAL/valcheck.cpp:150-190
                }
                o.head.kind = kind;
                o.head.flags = wire::flag_ntt;
                o.head.L = static_cast<std::uint32_t>(k);
                o.head.parms_id = cd->parms_id();
                for (std::uint64_t slot = 0; slot < dim1; slot++)
                {
                    const std::uint64_t dim2 = get<std::uint64_t>(src);
                    if (dim2 == 0)
                    {
                        continue;
                    }
                    if (dim2 != k - 1)
                    {
                        throw std::logic_error("KSwitchKeys data is invalid");
                    }
                    // the layout every key-switch entry point takes: [k-1][2][k][N]
                    wire::Record r;
                    r.kind = wire::kind_kswitch_key;
                    r.flags = wire::flag_ntt;
                    r.count = static_cast<std::uint32_t>(2 * (k - 1));
                    r.L = static_cast<std::uint32_t>(k);
                    r.parms_id = cd->parms_id();
                    r.block = std::make_shared<util::DeviceArray>(2 * (k - 1) * k * n, st);
                    r.data = r.block->get();
                    std::vector<std::uint8_t> seeds;
                    for (std::size_t j = 0; j < k - 1; j++)
                    {
                        const CtMeta m = ct_meta(2);
                        if (m.id != context.key_parms_id() || !m.ntt || (j && m.seeded != !seeds.empty()))
                        {
                            throw std::logic_error("KSwitchKeys data is invalid");
                        }
                        ct_data(m, r.block->get() + j * 2 * k * n, seeds);
                    }
                    expand(seeds, r.block->get(), k);
                    residues(r.data, 2 * (k - 1), k);
                    o.indices.push_back(slot);
                    o.keys.push_back(std::move(r));
                }
                whole.close();
                o.head.count = static_cast<std::uint32_t>(o.keys.size());
                return o;
            }
        };

        inline wire::Object load_object(const SEALContext &context, wire::Source &src, std::uint32_t kind, bool check)
        {
            Loader ld(context, src, check);
            if (is_set(kind))
            {
                wire::Object o = ld.key_set(kind);
                ld.settle("KSwitchKeys");
                return o;
            }
            wire::Object o;
            o.dev = ld.dev;
            o.stream = ld.st;
            o.head = is_plain(kind) ? ld.plaintext(kind) : ld.ciphertext(kind);
            ld.settle(kind == wire::kind_plaintext    ? "Plaintext"
                      : kind == wire::kind_secret_key ? "SecretKey"
                      : kind == wire::kind_public_key ? "PublicKey"
                                                      : "ciphertext");
            return o;
        }

        // ---- EncryptionParameters: host only ------------------------------------------------------------------------------
        inline std::size_t parms_bytes(std::size_t L)
        {
            return header_bytes + 1 + 8 + 8 + (L + 1) * (header_bytes + 8);
        }
        inline void put_parms(scheme_type scheme, std::size_t n, const std::vector<Modulus> &cm, wire::Sink &sink)
        {
            const Header h = make_seal_header(parms_bytes(cm.size())), mh = make_seal_header(header_bytes + 8);
            const std::uint8_t s = static_cast<std::uint8_t>(scheme);
            const std::uint64_t f[2] = { n, cm.size() };
            sink.put(&h, sizeof(h));
            sink.put(&s, 1);
            sink.put(f, 16);
            for (std::size_t i = 0; i <= cm.size(); i++)
            {
                const std::uint64_t q = i < cm.size() ? cm[i].value() : 0; // the last one: plain_modulus, zero for CKKS
                sink.put(&mh, sizeof(mh));
                sink.put(&q, 8);
            }
        }
        struct Parms
        {
            std::uint8_t scheme;
            std::uint64_t n;
            std::vector<std::uint64_t> primes;
        };
        inline Parms get_parms(wire::Source &src)
        {
            Scope whole(src);
            Parms p;
            p.scheme = get<std::uint8_t>(src);
            p.n = get<std::uint64_t>(src);
            const std::uint64_t L = get<std::uint64_t>(src);
            if (p.n > 131072) // SEAL_POLY_MOD_DEGREE_MAX
            {
                throw std::logic_error("poly_modulus_degree is invalid");
            }
            if (L > 256) // SEAL_COEFF_MOD_COUNT_MAX
            {
                throw std::logic_error("coeff_modulus is invalid");
            }
            for (std::uint64_t i = 0; i <= L; i++)
            {
                Scope mod(src);
                const std::uint64_t q = get<std::uint64_t>(src);
                mod.close();
                if (i < L)
                {
                    p.primes.push_back(q);
                }
                else if (q)
                {
                    throw std::logic_error("plain_modulus is not supported for this scheme"); // SEAL/encryptionparams.h:265
                }
            }
            whole.close();
            return p;
        }
    } // namespace sealfmt
} // namespace seal
