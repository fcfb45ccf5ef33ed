// seal/moai_serialization.h -- the wire form of the seal:: surface: save / load / save_size with SEAL's signatures
// (SEAL/serialization.h, SEAL/serializable.h) over this library's own format.  Included from seal/seal.h.
//
// save writes this library's own format, which is smaller than SEAL's: seeds are expanded with ChaCha20 (include/moai_hip.h,
// "Stream contract") where SEAL uses Blake2xb / Shake256 (SEAL/randomgen.cpp), the parms_id is the shim's own hash, and rows
// are bit-packed, which SEAL's format cannot express.  SEAL's own byte format is the other one this surface speaks
// (seal/moai_seal_format.h): load recognises either from its first byte, and save_seal / save_size_seal write SEAL's.  DESIGN.md
// section 5.0e specifies this format completely and tests/wire_format.py restates it.  In short, little-endian and 8-byte aligned:
//
//   record  = header (120 bytes) + stored x packed polynomial          (moai_pack_rows: every row at its prime's bit length)
//   header  = magic "MOAIWIRE", u32 version (1), u32 kind, u32 flags (1 seeded, 2 NTT form), u32 polynomial count, u32 N, u32 L,
//             u64 total bytes, f64 scale, u64 parms_id[4], u64 first sequence, u8 seed[32]
//   seeded  : the odd polynomials (c1 of a ciphertext, of every key digit) are not stored; polynomial 2 b + 1 is
//             uniform(seed, 1 << 56 | first sequence + b) (moai_expand_seeded), so stored = count / 2
//   key set = header (kind 5 / 6 / 7, count = number of keys, total = the whole set) + u64 index[count] + one record of kind 9
//             (count = 2 (k - 1) polynomials of k rows) per key, or of kind 10 for a key limited to a chain index
//   kind 10 = a limited switching key (include/moai_hip.h, "keys limited to a chain index"): count = 2 levels polynomials,
//             L = levels + 1 rows packed under the primes {0 .. levels-1, k-1}, parms_id of the key level; seeded: the odd
//             polynomials are moai_expand_seeded_limited of the seed (stream positions of the full k-row draw)
//
//   SEAL seeds : an object made under util::seed_kind::seal_blake2xb (Record::seal_seeds) has no seeded form here.  save expands
//             it first (moai_seal_sample_uniform) and writes the unseeded record; save_seal writes SEAL's seeded layout.
//
// Everything that touches residues runs on the device: pack + one device-to-host copy on save; one host-to-device copy +
// unpack (with the residue check of is_data_valid_for folded in) + expand on load.
#pragma once
#include <cstddef>

namespace seal
{
    namespace wire
    {
        constexpr std::uint32_t version = 1;
        constexpr std::uint32_t kind_ciphertext = 1, kind_plaintext = 2, kind_public_key = 3, kind_secret_key = 4, kind_kswitch_keys = 5,
                                kind_relin_keys = 6, kind_galois_keys = 7, kind_encryption_parameters = 8, kind_kswitch_key = 9,
                                kind_kswitch_key_limited = 10;
        constexpr std::uint32_t flag_seeded = 1, flag_ntt = 2;

        struct Header
        {
            char magic[8];
            std::uint32_t version, kind, flags, count, n, L;
            std::uint64_t total;
            double scale;
            std::uint64_t parms_id[4];
            std::uint64_t seq;
            std::uint8_t seed[32];
        };
        static_assert(sizeof(Header) == 120, "the wire header is 120 bytes without padding");

        // one record in memory: `count` polynomials of L rows, of which stored() are on the device at `data`
        struct Record
        {
            std::uint32_t kind = 0, flags = 0, count = 0, L = 0;
            double scale = 1.0;
            parms_id_type parms_id = parms_id_zero;
            std::uint64_t seq = 0;
            std::uint8_t seed[32] = {};
            // seeded for SEAL instead (util::seed_kind::seal_blake2xb): 64 bytes per stored polynomial b, of which polynomial
            // 2 b + 1 is sample_poly_uniform; seq and seed stay zero.  seal_flags: the device uint32_t[2] the generating call
            // counted its rejections into (moai_seal_sample_uniform's `rejected`), read back when the object is saved
            std::vector<std::uint8_t> seal_seeds;
            std::shared_ptr<util::DeviceArray> seal_flags;
            std::shared_ptr<util::DeviceArray> block; // owner of `data`, where the record has one of its own
            const std::uint64_t *data = nullptr;      // device [stored()][L][N]; after a load: all `count` polynomials
            std::size_t stored() const
            {
                return (flags & flag_seeded) ? count / 2 : count;
            }
            bool seal_seeded() const
            {
                return !seal_seeds.empty();
            }
        };
        // what save writes and load reads: one record, or a key set
        struct Object
        {
            Record head;
            bool is_set = false;
            std::vector<std::uint64_t> indices;
            std::vector<Record> keys;
            moai_ctx *dev = nullptr;
            void *stream = nullptr;
        };

        inline void check_mode(compr_mode_type m)
        {
            if (m != compr_mode_type::none)
            {
                throw std::invalid_argument("unsupported compression mode"); // SEAL/serialization.cpp:89,107
            }
        }

        // ---- where bytes go and come from -------------------------------------------------------------------------------
        struct Sink
        {
            virtual ~Sink() = default;
            virtual void put(const void *p, std::size_t bytes) = 0;
            virtual std::uint8_t *space(std::size_t bytes) = 0; // to be filled by a device-to-host copy, then commit()
            virtual void commit() = 0;
        };
        struct BufferSink : Sink
        {
            std::uint8_t *out;
            std::size_t size, pos = 0;
            BufferSink(seal_byte *o, std::size_t s) : out(reinterpret_cast<std::uint8_t *>(o)), size(s)
            {
                if (!o)
                {
                    throw std::invalid_argument("out cannot be null"); // SEAL/serialization.cpp:189-217
                }
            }
            void put(const void *p, std::size_t bytes) override
            {
                std::memcpy(space(bytes), p, bytes);
            }
            std::uint8_t *space(std::size_t bytes) override
            {
                if (bytes > size - pos)
                {
                    throw std::invalid_argument("buffer is too small");
                }
                pos += bytes;
                return out + pos - bytes;
            }
            void commit() override
            {}
        };
        struct StreamSink : Sink
        {
            std::ostream &s;
            std::vector<std::uint8_t> tmp;
            explicit StreamSink(std::ostream &o) : s(o)
            {}
            void put(const void *p, std::size_t bytes) override
            {
                s.write(static_cast<const char *>(p), static_cast<std::streamsize>(bytes));
                if (!s)
                {
                    throw std::runtime_error("I/O error"); // SEAL/serialization.cpp:55-80
                }
            }
            std::uint8_t *space(std::size_t bytes) override
            {
                tmp.resize(bytes);
                return tmp.data();
            }
            void commit() override
            {
                put(tmp.data(), tmp.size());
                tmp.clear();
            }
        };
        struct Source
        {
            virtual ~Source() = default;
            virtual const std::uint8_t *view(std::size_t bytes) = 0; // valid until the next call
            virtual int peek() = 0;                                   // the next byte without consuming it, -1 at the end
            virtual bool stable() const = 0;                          // a view stays valid after the next call
            std::size_t consumed = 0;
        };
        struct BufferSource : Source
        {
            const std::uint8_t *in;
            std::size_t size;
            BufferSource(const seal_byte *i, std::size_t s) : in(reinterpret_cast<const std::uint8_t *>(i)), size(s)
            {
                if (!i)
                {
                    throw std::invalid_argument("in cannot be null");
                }
            }
            const std::uint8_t *view(std::size_t bytes) override
            {
                if (bytes > size - consumed)
                {
                    throw std::invalid_argument("buffer is too small");
                }
                consumed += bytes;
                return in + consumed - bytes;
            }
            int peek() override
            {
                return consumed < size ? in[consumed] : -1;
            }
            bool stable() const override
            {
                return true;
            }
        };
        struct StreamSource : Source
        {
            std::istream &s;
            std::vector<std::uint8_t> tmp;
            explicit StreamSource(std::istream &i) : s(i)
            {}
            const std::uint8_t *view(std::size_t bytes) override
            {
                // in steps, so that a header that lies about its size cannot make this allocate what the stream never delivers
                tmp.clear();
                while (tmp.size() < bytes)
                {
                    const std::size_t step = std::min<std::size_t>(bytes - tmp.size(), std::size_t(1) << 26);
                    const std::size_t at = tmp.size();
                    tmp.resize(at + step);
                    s.read(reinterpret_cast<char *>(tmp.data() + at), static_cast<std::streamsize>(step));
                    if (static_cast<std::size_t>(s.gcount()) != step)
                    {
                        throw std::runtime_error("I/O error: input stream ended unexpectedly"); // SEAL/serialization.cpp:71-76
                    }
                }
                consumed += bytes;
                return tmp.data();
            }
            int peek() override
            {
                const auto c = s.peek();
                return c == std::istream::traits_type::eof() ? -1 : static_cast<int>(static_cast<unsigned char>(c));
            }
            bool stable() const override
            {
                return false;
            }
        };

        // ---- sizes --------------------------------------------------------------------------------------------------------
        // the primes a record's rows sit under: empty (0 .. L-1), or {0 .. L-2, k-1} for a limited switching key
        inline std::vector<std::uint32_t> record_rows(moai_ctx *dev, std::uint32_t kind, std::size_t L)
        {
            std::vector<std::uint32_t> idx;
            if (kind == kind_kswitch_key_limited && L >= 2)
            {
                for (std::size_t r = 0; r + 1 < L; r++)
                {
                    idx.push_back(static_cast<std::uint32_t>(r));
                }
                idx.push_back(static_cast<std::uint32_t>(moai_ctx_prime_count(dev) - 1));
            }
            return idx;
        }
        inline std::size_t packed_words(moai_ctx *dev, std::size_t L, const std::vector<std::uint32_t> &rows = {})
        {
            const std::size_t w = moai_packed_words(dev, L, rows.empty() ? nullptr : rows.data());
            if (!w)
            {
                throw std::logic_error(moai_last_error());
            }
            return w;
        }
        inline std::size_t record_bytes(moai_ctx *dev, const Record &r)
        {
            const std::size_t polys = r.seal_seeded() ? r.count : r.stored(); // SEAL seeds are expanded on the way out
            return sizeof(Header) + (polys ? polys * packed_words(dev, r.L, record_rows(dev, r.kind, r.L)) * 8 : 0);
        }
        inline std::size_t object_bytes(const Object &o)
        {
            if (!o.is_set)
            {
                return record_bytes(o.dev, o.head);
            }
            std::size_t b = sizeof(Header) + 8 * o.indices.size();
            for (auto &k : o.keys)
            {
                b += record_bytes(o.dev, k);
            }
            return b;
        }

        // ---- save -----------------------------------------------------------------------------------------------------------
        inline Header make_header(const Record &r, std::size_t n, std::size_t total)
        {
            Header h;
            std::memset(&h, 0, sizeof(h));
            std::memcpy(h.magic, "MOAIWIRE", 8);
            h.version = version;
            h.kind = r.kind;
            h.flags = r.flags;
            h.count = r.count;
            h.n = static_cast<std::uint32_t>(n);
            h.L = r.L;
            h.total = total;
            h.scale = r.scale;
            std::copy(r.parms_id.begin(), r.parms_id.end(), h.parms_id);
            h.seq = r.seq;
            std::memcpy(h.seed, r.seed, 32);
            return h;
        }
        // what the generating call left in a SEAL-seeded record's overflow word, enqueued before a synchronisation and judged
        // after it: a seed whose replacements ran over their bound (what the loader's expansion raises for such a seed)
        struct SealOverflow
        {
            std::uint32_t f[2] = { 0, 0 };
            SealOverflow(const Object &o, const Record &r)
            {
                if (r.seal_seeded() && r.seal_flags)
                {
                    util::hip_check(moai_memcpy_d2h(f, r.seal_flags->get(), 8, o.stream));
                }
            }
            void settle() const
            {
                if (f[1])
                {
                    throw std::logic_error("ciphertext data is invalid");
                }
            }
        };
        // all `count` polynomials of a SEAL-seeded record: c0 copied, the uniform halves from moai_seal_sample_uniform
        inline void expand_seal_seeded(const Object &o, const Record &r, util::DeviceArray &full)
        {
            const std::size_t LN = r.L * moai_ctx_coeff_count(o.dev);
            full.resize(r.count * LN, o.stream);
            for (std::size_t b = 0; b < r.stored(); b++)
            {
                util::hip_check(moai_memcpy_d2d(full.get() + 2 * b * LN, r.data + b * LN, LN * 8, o.stream));
            }
            util::hip_check(moai_seal_sample_uniform(o.dev, r.seal_seeds.data(), full.get() + LN, 2 * LN, r.stored(), r.L, nullptr, nullptr,
                                                     o.stream));
        }
        inline void put_record(const Object &o, const Record &r0, Sink &sink)
        {
            const std::size_t n = moai_ctx_coeff_count(o.dev);
            Record r = r0;
            util::DeviceArray full;
            const SealOverflow overflow(o, r0);
            if (r0.seal_seeded())
            {
                expand_seal_seeded(o, r0, full);
                r.flags &= ~flag_seeded;
                r.seal_seeds.clear();
                r.data = full.get();
            }
            const Header h = make_header(r, n, record_bytes(o.dev, r));
            sink.put(&h, sizeof(h));
            if (!r.stored())
            {
                return;
            }
            // the whole record in one moai_pack_rows and one device-to-host copy
            const std::vector<std::uint32_t> rows = record_rows(o.dev, r.kind, r.L);
            const std::size_t words = r.stored() * packed_words(o.dev, r.L, rows);
            util::DeviceArray packed(words, o.stream);
            util::hip_check(moai_pack_rows(o.dev, r.data, packed.get(), r.stored(), r.L, rows.empty() ? nullptr : rows.data(), o.stream));
            std::uint8_t *dst = sink.space(words * 8);
            util::hip_check(moai_memcpy_d2h(dst, packed.get(), words * 8, o.stream));
            util::hip_check(moai_stream_sync(o.stream));
            overflow.settle();
            sink.commit();
        }
        inline std::streamoff save_object(const Object &o, Sink &sink)
        {
            if (!o.dev)
            {
                throw std::logic_error("object is empty or its context is gone");
            }
            const std::size_t total = object_bytes(o);
            if (!o.is_set)
            {
                put_record(o, o.head, sink);
                return static_cast<std::streamoff>(total);
            }
            const Header h = make_header(o.head, moai_ctx_coeff_count(o.dev), total);
            sink.put(&h, sizeof(h));
            sink.put(o.indices.data(), 8 * o.indices.size());
            for (auto &k : o.keys)
            {
                put_record(o, k, sink);
            }
            return static_cast<std::streamoff>(total);
        }

        // ---- load -----------------------------------------------------------------------------------------------------------
        // SEAL/serialization.cpp:365-383: anything unknown is an error, never a guess
        inline Header get_header(Source &src)
        {
            Header h;
            std::memcpy(&h, src.view(sizeof(Header)), sizeof(Header));
            if (std::memcmp(h.magic, "MOAIWIRE", 8) != 0)
            {
                throw std::logic_error("loaded header is invalid: not a moai wire record");
            }
            if (h.version != version)
            {
                throw std::logic_error("incompatible version");
            }
            if (h.kind < 1 || h.kind > kind_kswitch_key_limited || (h.flags & ~(flag_seeded | flag_ntt)) || h.seq >> 56 || h.total < sizeof(Header))
            {
                throw std::logic_error("loaded header is invalid");
            }
            bool any_seed = h.seq != 0;
            for (int i = 0; i < 32; i++)
            {
                any_seed = any_seed || h.seed[i];
            }
            if (!(h.flags & flag_seeded) && any_seed)
            {
                throw std::logic_error("loaded header is invalid");
            }
            return h;
        }
        // the header's claims against the context: N, a parms_id the context knows, the row count of that level
        inline void check_against(const SEALContext &context, const Header &h, std::uint32_t kind, const char *what)
        {
            parms_id_type id = { h.parms_id[0], h.parms_id[1], h.parms_id[2], h.parms_id[3] };
            auto cd = context.get_context_data(id);
            if (h.kind != kind || h.n != context.n() || !cd || cd->parms().coeff_modulus().size() != h.L ||
                ((h.flags & flag_seeded) && (h.count & 1)))
            {
                throw std::logic_error(std::string(what) + " data is invalid"); // SEAL/ciphertext.cpp:302,358
            }
        }
        // a limited switching key inside a key set: N, the key level's parms_id, 1 <= levels <= k-1 with L = levels + 1 rows and
        // 2 levels polynomials
        inline void check_limited(const SEALContext &context, const Header &h, const char *what)
        {
            const std::size_t k = context.key_context_data()->parms().coeff_modulus().size();
            parms_id_type id = { h.parms_id[0], h.parms_id[1], h.parms_id[2], h.parms_id[3] };
            if (h.n != context.n() || id != context.key_parms_id() || k < 2 || h.L < 2 || h.L > k || h.count != 2 * (std::size_t(h.L) - 1))
            {
                throw std::logic_error(std::string(what) + " data is invalid");
            }
        }
        // a block [levels][2][levels+1][N] whose trimmed layout the library keeps by its address (moai_key_register and the entry
        // points that record): the record is dropped before the block goes back to the pool
        inline std::shared_ptr<util::DeviceArray> limited_key_block(const SEALContext &context, std::size_t levels)
        {
            std::shared_ptr<SEALContext> keep(new SEALContext(context));
            return std::shared_ptr<util::DeviceArray>(new util::DeviceArray(moai_key_words(context.device(), levels), context.stream()),
                                                      [keep](util::DeviceArray *p) {
                                                          moai_key_forget(keep->device(), p->get());
                                                          delete p;
                                                      });
        }
        inline Record get_record(const SEALContext &context, Source &src, std::uint32_t kind, const char *what, bool check, std::size_t max_count)
        {
            const Header h = get_header(src);
            // where a whole switching key is expected, one limited to a chain index may stand
            const bool limited = kind == kind_kswitch_key && h.kind == kind_kswitch_key_limited;
            if (limited)
            {
                check_limited(context, h, what);
            }
            else
            {
                check_against(context, h, kind, what);
            }
            Record r;
            r.kind = h.kind;
            r.flags = h.flags;
            r.count = h.count;
            r.L = h.L;
            r.scale = h.scale;
            r.parms_id = { h.parms_id[0], h.parms_id[1], h.parms_id[2], h.parms_id[3] };
            r.seq = h.seq;
            std::memcpy(r.seed, h.seed, 32);
            if (r.count < 1 || r.count > max_count || h.total != record_bytes(context.device(), r))
            {
                throw std::logic_error(std::string(what) + " data is invalid");
            }
            moai_ctx *dev = context.device();
            void *st = context.stream();
            const std::size_t n = context.n(), stored = r.stored(), LN = r.L * n;
            const std::vector<std::uint32_t> rows = record_rows(dev, r.kind, r.L);
            const std::uint32_t *pidx = rows.empty() ? nullptr : rows.data();
            const std::size_t words = stored * packed_words(dev, r.L, rows);
            const std::uint8_t *bytes = src.view(words * 8);
            util::DeviceArray packed(words, st), flag(1, st);
            util::hip_check(moai_memcpy_h2d(packed.get(), bytes, words * 8, st));
            auto out = limited ? limited_key_block(context, r.L - 1) : std::make_shared<util::DeviceArray>(r.count * LN, st);
            std::uint64_t bad = 0;
            if (check)
            {
                util::hip_check(moai_memset_zero(flag.get(), 8, st));
            }
            std::uint32_t *dflag = check ? reinterpret_cast<std::uint32_t *>(flag.get()) : nullptr;
            if (r.flags & flag_seeded)
            {
                util::DeviceArray c0(stored * LN, st);
                util::hip_check(moai_unpack_rows(dev, packed.get(), c0.get(), stored, r.L, pidx, dflag, st));
                if (limited)
                {
                    util::hip_check(moai_expand_seeded_limited(dev, r.seed, r.seq, c0.get(), r.L - 1, out->get(), st));
                }
                else
                {
                    util::hip_check(moai_expand_seeded(dev, r.seed, r.seq, c0.get(), out->get(), stored, r.L, nullptr, st));
                }
            }
            else
            {
                util::hip_check(moai_unpack_rows(dev, packed.get(), out->get(), stored, r.L, pidx, dflag, st));
                if (limited)
                {
                    util::hip_check(moai_key_register(dev, out->get(), r.L - 1));
                }
            }
            if (check)
            {
                util::hip_check(moai_memcpy_d2h(&bad, flag.get(), 8, st));
            }
            context.sync();
            if (bad)
            {
                throw std::logic_error(std::string(what) + " data is invalid"); // a residue >= its prime
            }
            r.block = out;
            r.data = out->get();
            return r;
        }
        inline Object load_object(const SEALContext &context, Source &src, std::uint32_t kind, const char *what, bool check)
        {
            Object o;
            o.dev = context.device();
            o.stream = context.stream();
            const std::size_t k = context.key_context_data()->parms().coeff_modulus().size();
            if (kind != kind_kswitch_keys && kind != kind_relin_keys && kind != kind_galois_keys)
            {
                o.head = get_record(context, src, kind, what, check, kind == kind_ciphertext ? 6 : (kind == kind_public_key ? 2 : 1));
                return o;
            }
            o.is_set = true;
            const Header h = get_header(src);
            check_against(context, h, kind, what);
            parms_id_type id = { h.parms_id[0], h.parms_id[1], h.parms_id[2], h.parms_id[3] };
            if (id != context.key_parms_id() || h.count > context.n() || (h.flags & flag_seeded) || k < 2)
            {
                throw std::logic_error(std::string(what) + " data is invalid");
            }
            o.head.kind = h.kind;
            o.head.flags = h.flags;
            o.head.count = h.count;
            o.head.L = h.L;
            o.head.parms_id = id;
            o.indices.resize(h.count);
            if (h.count)
            {
                std::memcpy(o.indices.data(), src.view(8 * h.count), 8 * h.count);
            }
            for (std::size_t i = 0; i < o.indices.size(); i++)
            {
                if (o.indices[i] >= context.n() || (i && o.indices[i] <= o.indices[i - 1]))
                {
                    throw std::logic_error(std::string(what) + " data is invalid");
                }
            }
            for (std::size_t i = 0; i < o.indices.size(); i++)
            {
                Record r = get_record(context, src, kind_kswitch_key, what, check, 2 * (k - 1));
                if (r.count != 2 * (r.kind == kind_kswitch_key_limited ? std::size_t(r.L) - 1 : k - 1) || r.parms_id != id)
                {
                    throw std::logic_error(std::string(what) + " data is invalid");
                }
                o.keys.push_back(std::move(r));
            }
            if (src.consumed != h.total)
            {
                throw std::logic_error(std::string(what) + " data is invalid");
            }
            return o;
        }
    } // namespace wire

    namespace sealfmt
    {
        // seal/moai_seal_format.h: SEAL 4.1's own byte format, compression mode none
        constexpr int first_byte = 0x5E; // of SEALHeader::magic 0xA15E; this library's own format starts with 'M'
        inline std::size_t object_bytes(const wire::Object &o);
        inline std::streamoff save_object(const wire::Object &o, wire::Sink &sink);
        inline wire::Object load_object(const SEALContext &context, wire::Source &src, std::uint32_t kind, bool check);
    } // namespace sealfmt

    // SEAL/serializable.h: an object that can only be saved -- what the seeded encryptions and key generators return.  It holds
    // c0 of every ciphertext or key digit and the public seed (ChaCha20: one per object; SEAL's Blake2xb: one per ciphertext or
    // digit); the uniform halves are not kept on this side.
    template <class T>
    class Serializable
    {
    public:
        std::streamoff save_size(compr_mode_type compr_mode = compr_mode_default) const
        {
            wire::check_mode(compr_mode);
            return static_cast<std::streamoff>(wire::object_bytes(obj_));
        }
        std::streamoff save(std::ostream &stream, compr_mode_type compr_mode = compr_mode_default) const
        {
            wire::check_mode(compr_mode);
            wire::StreamSink s(stream);
            return wire::save_object(obj_, s);
        }
        std::streamoff save(seal_byte *out, std::size_t size, compr_mode_type compr_mode = compr_mode_default) const
        {
            wire::check_mode(compr_mode);
            wire::BufferSink s(out, size);
            return wire::save_object(obj_, s);
        }
        // SEAL's own format: seeded as SEAL writes it when the object was made under util::seed_kind::seal_blake2xb; otherwise
        // unseeded, because SEAL cannot expand a ChaCha20 seed, so the object is expanded first
        std::streamoff save_size_seal(compr_mode_type compr_mode = compr_mode_default) const
        {
            wire::check_mode(compr_mode);
            return static_cast<std::streamoff>(sealfmt::object_bytes(obj_));
        }
        std::streamoff save_seal(std::ostream &stream, compr_mode_type compr_mode = compr_mode_default) const
        {
            wire::check_mode(compr_mode);
            wire::StreamSink s(stream);
            return sealfmt::save_object(obj_, s);
        }
        std::streamoff save_seal(seal_byte *out, std::size_t size, compr_mode_type compr_mode = compr_mode_default) const
        {
            wire::check_mode(compr_mode);
            wire::BufferSink s(out, size);
            return sealfmt::save_object(obj_, s);
        }

    private:
        friend class Encryptor;
        friend class KeyGenerator;
        explicit Serializable(wire::Object o) : obj_(std::move(o))
        {}
        wire::Object obj_;
    };

// save / load with SEAL's signatures (SEAL/ciphertext.h:560-720 and the same block of every other type) over two hooks each
// type defines in seal/moai_serialization_impl.h: to_wire() settles lazy state and describes the object without changing it,
// from_wire() validates what is specific to the type and only then replaces *this (a failed load leaves it as it was).
// save_seal / save_size_seal write SEAL's own format (seal/moai_seal_format.h), and load takes either format.
#define MOAI_WIRE_METHODS(KIND)                                                                                         \
    std::streamoff save_size_seal(compr_mode_type compr_mode = compr_mode_default) const                                \
    {                                                                                                                   \
        wire::check_mode(compr_mode);                                                                                   \
        return static_cast<std::streamoff>(sealfmt::object_bytes(to_wire()));                                           \
    }                                                                                                                   \
    std::streamoff save_seal(std::ostream &stream, compr_mode_type compr_mode = compr_mode_default) const               \
    {                                                                                                                   \
        wire::check_mode(compr_mode);                                                                                   \
        wire::StreamSink s(stream);                                                                                     \
        return sealfmt::save_object(to_wire(), s);                                                                      \
    }                                                                                                                   \
    std::streamoff save_seal(seal_byte *out, std::size_t size, compr_mode_type compr_mode = compr_mode_default) const   \
    {                                                                                                                   \
        wire::check_mode(compr_mode);                                                                                   \
        wire::BufferSink s(out, size);                                                                                  \
        return sealfmt::save_object(to_wire(), s);                                                                      \
    }                                                                                                                   \
    std::streamoff save_size(compr_mode_type compr_mode = compr_mode_default) const                                     \
    {                                                                                                                   \
        wire::check_mode(compr_mode);                                                                                   \
        return static_cast<std::streamoff>(wire::object_bytes(to_wire()));                                              \
    }                                                                                                                   \
    std::streamoff save(std::ostream &stream, compr_mode_type compr_mode = compr_mode_default) const                    \
    {                                                                                                                   \
        wire::check_mode(compr_mode);                                                                                   \
        wire::StreamSink s(stream);                                                                                     \
        return wire::save_object(to_wire(), s);                                                                         \
    }                                                                                                                   \
    std::streamoff save(seal_byte *out, std::size_t size, compr_mode_type compr_mode = compr_mode_default) const        \
    {                                                                                                                   \
        wire::check_mode(compr_mode);                                                                                   \
        wire::BufferSink s(out, size);                                                                                  \
        return wire::save_object(to_wire(), s);                                                                         \
    }                                                                                                                   \
    std::streamoff load(const SEALContext &context, std::istream &stream)                                               \
    {                                                                                                                   \
        wire::StreamSource s(stream);                                                                                   \
        return load_from(context, s, true);                                                                             \
    }                                                                                                                   \
    std::streamoff load(const SEALContext &context, const seal_byte *in, std::size_t size)                              \
    {                                                                                                                   \
        wire::BufferSource s(in, size);                                                                                 \
        return load_from(context, s, true);                                                                             \
    }                                                                                                                   \
    std::streamoff unsafe_load(const SEALContext &context, std::istream &stream)                                        \
    {                                                                                                                   \
        wire::StreamSource s(stream);                                                                                   \
        return load_from(context, s, false);                                                                            \
    }                                                                                                                   \
    std::streamoff unsafe_load(const SEALContext &context, const seal_byte *in, std::size_t size)                       \
    {                                                                                                                   \
        wire::BufferSource s(in, size);                                                                                 \
        return load_from(context, s, false);                                                                            \
    }                                                                                                                   \
    wire::Object to_wire() const;                                                                                       \
    void from_wire(const SEALContext &context, wire::Object &&o);                                                       \
    std::streamoff load_from(const SEALContext &context, wire::Source &s, bool check)                                   \
    {                                                                                                                   \
        from_wire(context, s.peek() == sealfmt::first_byte ? sealfmt::load_object(context, s, KIND, check)              \
                                                           : wire::load_object(context, s, KIND, "loaded", check));     \
        return static_cast<std::streamoff>(s.consumed);                                                                 \
    }
} // namespace seal
