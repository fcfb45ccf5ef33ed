// seal/moai_serialization_impl.h -- the per-type halves of the wire form (seal/moai_serialization.h): to_wire() settles an
// object's lazy state and describes it without changing it; from_wire() checks what only the type knows and then, and only
// then, replaces the destination.  Included at the end of seal/seal.h.
#pragma once

namespace seal
{
    // ---- Ciphertext (SEAL/ciphertext.cpp:204-372) ------------------------------------------------------------------------
    inline wire::Object Ciphertext::to_wire() const
    {
        if (batch_ != 1)
        {
            throw std::logic_error("packed ciphertext: moai_fused::unpack it before saving");
        }
        if (!size_ || !dev_)
        {
            throw std::logic_error("ciphertext is empty");
        }
        wire::Object o;
        o.dev = dev_;
        o.stream = stream_;
        o.head.data = device_data(); // deferred terms and a pending rotation are made now; the value does not change
        o.head.block = buf_;
        o.head.kind = wire::kind_ciphertext;
        o.head.flags = is_ntt_form_ ? wire::flag_ntt : 0;
        o.head.count = static_cast<std::uint32_t>(size_);
        o.head.L = static_cast<std::uint32_t>(L_);
        o.head.scale = scale_;
        o.head.parms_id = parms_id_;
        return o;
    }
    inline void Ciphertext::from_wire(const SEALContext &context, wire::Object &&o)
    {
        const wire::Record &r = o.head;
        if (r.count < 2)
        {
            throw std::logic_error("ciphertext data is invalid");
        }
        Ciphertext fresh;
        fresh.parms_id_ = r.parms_id;
        fresh.is_ntt_form_ = (r.flags & wire::flag_ntt) != 0;
        fresh.size_ = r.count;
        fresh.n_ = context.n();
        fresh.L_ = r.L;
        fresh.scale_ = r.scale;
        fresh.stream_ = context.stream();
        fresh.dev_ = context.device();
        fresh.buf_ = r.block;
        *this = std::move(fresh);
    }

    // ---- Plaintext (SEAL/plaintext.cpp:150-260) ---------------------------------------------------------------------------
    inline wire::Object Plaintext::to_wire() const
    {
        moai_ctx *dev = dev_ ? dev_ : util::stream_device(stream_);
        if (!is_ntt_form() || !L_ || !dev)
        {
            throw std::logic_error("plaintext is empty");
        }
        wire::Object o;
        o.dev = dev;
        o.stream = stream_;
        if (is_scalar())
        {
            // constant rows are the NTT of a constant polynomial: written out in a block of the record's own
            o.head.block = std::make_shared<util::DeviceArray>(L_ * n_, stream_);
            util::hip_check(moai_memset_zero(o.head.block->get(), L_ * n_ * 8, stream_));
            util::hip_check(moai_add_scalar_rows(dev, o.head.block->get(), scalar_rows_.data(), o.head.block->get(), 1, L_, stream_));
            o.head.data = o.head.block->get();
        }
        else
        {
            o.head.data = device_data(); // a masked constant is transformed now (Plaintext::materialize)
        }
        o.head.kind = wire::kind_plaintext;
        o.head.flags = wire::flag_ntt;
        o.head.count = 1;
        o.head.L = static_cast<std::uint32_t>(L_);
        o.head.scale = scale_;
        o.head.parms_id = parms_id_;
        return o;
    }
    inline void Plaintext::from_wire(const SEALContext &context, wire::Object &&o)
    {
        wire::Record &r = o.head;
        if (!(r.flags & wire::flag_ntt) || (r.flags & wire::flag_seeded))
        {
            throw std::logic_error("plaintext data is invalid");
        }
        Plaintext fresh;
        fresh.parms_id_ = r.parms_id;
        fresh.scale_ = r.scale;
        fresh.n_ = context.n();
        fresh.L_ = r.L;
        fresh.stream_ = context.stream();
        fresh.dev_ = context.device();
        fresh.data_ = std::move(*r.block);
        *this = std::move(fresh);
    }

    // ---- SecretKey (SEAL/secretkey.h:130-230) --------------------------------------------------------------------------------
    inline wire::Object SecretKey::to_wire() const
    {
        moai_ctx *dev = ntt_ ? util::stream_device(ntt_->stream()) : nullptr;
        if (!dev)
        {
            throw std::logic_error("secret key is empty");
        }
        wire::Object o;
        o.dev = dev;
        o.stream = ntt_->stream();
        o.head.block = ntt_;
        o.head.data = ntt_->get();
        o.head.kind = wire::kind_secret_key;
        o.head.flags = wire::flag_ntt;
        o.head.count = 1;
        o.head.L = static_cast<std::uint32_t>(moai_ctx_prime_count(dev));
        o.head.parms_id = parms_id_;
        return o;
    }
    inline void SecretKey::from_wire(const SEALContext &context, wire::Object &&o)
    {
        if (o.head.parms_id != context.key_parms_id() || (o.head.flags & wire::flag_seeded))
        {
            throw std::logic_error("secret key data is invalid");
        }
        parms_id_ = o.head.parms_id;
        ntt_ = o.head.block;
    }

    // ---- PublicKey (SEAL/publickey.h:120-220) --------------------------------------------------------------------------------
    inline wire::Object PublicKey::to_wire() const
    {
        wire::Object o = ct_.to_wire();
        o.head.kind = wire::kind_public_key;
        return o;
    }
    inline void PublicKey::from_wire(const SEALContext &context, wire::Object &&o)
    {
        if (o.head.parms_id != context.key_parms_id() || o.head.count != 2)
        {
            throw std::logic_error("public key data is invalid");
        }
        ct_.from_wire(context, std::move(o));
    }

    // ---- KSwitchKeys, RelinKeys, GaloisKeys (SEAL/kswitchkeys.h:220-330) -----------------------------------------------------
    inline wire::Object KSwitchKeys::set_to_wire(std::uint32_t kind) const
    {
        wire::Object o;
        o.is_set = true;
        for (std::size_t i = 0; i < keys_.size(); i++)
        {
            if (!keys_[i])
            {
                continue;
            }
            // the full key: a key trimmed by limit_to_chain_index is saved from the copy that came back, or from its parked host copy;
            // a key born limited is saved as it is (record kind 10)
            std::shared_ptr<util::DeviceArray> full = keys_[i];
            std::size_t born = 0;
            if (res_)
            {
                std::lock_guard<std::mutex> g(res_->mu);
                if (i < res_->born.size() && res_->born[i])
                {
                    born = res_->levels[i];
                }
                else if (i < res_->levels.size() && res_->levels[i])
                {
                    if (i < res_->regrown.size() && res_->regrown[i])
                    {
                        full = res_->regrown[i];
                    }
                    else if (res_->host[i])
                    {
                        void *st = keys_[i]->stream();
                        full = std::make_shared<util::DeviceArray>(res_->host[i]->size(), st);
                        util::hip_check(moai_memcpy_h2d(full->get(), res_->host[i]->data(), res_->host[i]->size() * 8, st));
                        util::hip_check(moai_stream_sync(st));
                    }
                    else
                    {
                        throw std::logic_error("key was trimmed without a host copy: the full key is gone and cannot be saved");
                    }
                }
            }
            if (!o.dev)
            {
                o.stream = full->stream();
                o.dev = util::stream_device(o.stream);
                if (!o.dev)
                {
                    throw std::logic_error("key set outlived its context");
                }
            }
            const std::size_t k = moai_ctx_prime_count(o.dev);
            wire::Record r;
            r.kind = born ? wire::kind_kswitch_key_limited : wire::kind_kswitch_key;
            r.flags = wire::flag_ntt;
            r.count = static_cast<std::uint32_t>(2 * (born ? born : k - 1));
            r.L = static_cast<std::uint32_t>(born ? born + 1 : k);
            r.parms_id = parms_id_;
            r.block = full;
            r.data = full->get();
            o.indices.push_back(i);
            o.keys.push_back(std::move(r));
        }
        if (!o.dev)
        {
            throw std::logic_error("key set is empty");
        }
        o.head.kind = kind;
        o.head.flags = wire::flag_ntt;
        o.head.count = static_cast<std::uint32_t>(o.keys.size());
        o.head.L = static_cast<std::uint32_t>(moai_ctx_prime_count(o.dev));
        o.head.parms_id = parms_id_;
        return o;
    }
    inline void KSwitchKeys::set_from_wire(const SEALContext &context, wire::Object &&o, std::size_t min_slots)
    {
        // whole keys in the reference's layout and keys born limited (record kind 10: trimmed blocks the library knows),
        // constants of hoisted rotations yet to be derived, and a generation of its own, so that nothing cached with the keys
        // this object held before is mistaken for these
        std::vector<std::shared_ptr<util::DeviceArray>> keys(std::max<std::size_t>(min_slots, o.indices.empty() ? 0 : o.indices.back() + 1));
        for (std::size_t i = 0; i < o.indices.size(); i++)
        {
            keys[o.indices[i]] = o.keys[i].block;
        }
        reset(0, o.head.parms_id);
        keys_ = std::move(keys);
        for (std::size_t i = 0; i < o.indices.size(); i++)
        {
            if (o.keys[i].kind == wire::kind_kswitch_key_limited)
            {
                mark_born_limited(context, o.indices[i], o.keys[i].L - 1);
            }
        }
    }
    inline wire::Object KSwitchKeys::to_wire() const
    {
        return set_to_wire(wire::kind_kswitch_keys);
    }
    inline void KSwitchKeys::from_wire(const SEALContext &context, wire::Object &&o)
    {
        set_from_wire(context, std::move(o), 0);
    }
    inline wire::Object RelinKeys::to_wire() const
    {
        return set_to_wire(wire::kind_relin_keys);
    }
    inline void RelinKeys::from_wire(const SEALContext &context, wire::Object &&o)
    {
        set_from_wire(context, std::move(o), 1);
    }
    inline wire::Object GaloisKeys::to_wire() const
    {
        return set_to_wire(wire::kind_galois_keys);
    }
    inline void GaloisKeys::from_wire(const SEALContext &context, wire::Object &&o)
    {
        set_from_wire(context, std::move(o), context.n());
    }

    // ---- EncryptionParameters (SEAL/encryptionparams.h:383-470): host only ---------------------------------------------------
    // header (kind 8, N, L = k, no polynomials) + u64 scheme, u64 secret_key_hamming_weight, u64 sparse_slots, u64 prime[k]
    inline std::streamoff EncryptionParameters::save_size(compr_mode_type compr_mode) const
    {
        wire::check_mode(compr_mode);
        return static_cast<std::streamoff>(sizeof(wire::Header) + 8 * (3 + coeff_modulus_.size()));
    }
    inline std::streamoff EncryptionParameters::save(seal_byte *out, std::size_t size, compr_mode_type compr_mode) const
    {
        wire::check_mode(compr_mode);
        wire::BufferSink sink(out, size);
        wire::Record r;
        r.kind = wire::kind_encryption_parameters;
        r.L = static_cast<std::uint32_t>(coeff_modulus_.size());
        r.scale = 0;
        const std::size_t total = static_cast<std::size_t>(save_size());
        const wire::Header h = wire::make_header(r, poly_modulus_degree_, total);
        sink.put(&h, sizeof(h));
        std::vector<std::uint64_t> body = { static_cast<std::uint64_t>(scheme_), secret_key_hamming_weight_, sparse_slots_ };
        for (auto &m : coeff_modulus_)
        {
            body.push_back(m.value());
        }
        sink.put(body.data(), 8 * body.size());
        return static_cast<std::streamoff>(total);
    }
    inline std::streamoff EncryptionParameters::save(std::ostream &stream, compr_mode_type compr_mode) const
    {
        std::vector<seal_byte> buf(static_cast<std::size_t>(save_size(compr_mode)));
        save(buf.data(), buf.size(), compr_mode);
        wire::StreamSink sink(stream);
        sink.put(buf.data(), buf.size());
        return static_cast<std::streamoff>(buf.size());
    }
    // SEAL's own format: u8 scheme, u64 N, u64 L, L + 1 Modulus objects (the fork's hamming weight and sparse slots do not travel)
    inline std::streamoff EncryptionParameters::save_size_seal(compr_mode_type compr_mode) const
    {
        wire::check_mode(compr_mode);
        return static_cast<std::streamoff>(sealfmt::parms_bytes(coeff_modulus_.size()));
    }
    inline std::streamoff EncryptionParameters::save_seal(seal_byte *out, std::size_t size, compr_mode_type compr_mode) const
    {
        wire::check_mode(compr_mode);
        wire::BufferSink sink(out, size);
        sealfmt::put_parms(scheme_, poly_modulus_degree_, coeff_modulus_, sink);
        return save_size_seal();
    }
    inline std::streamoff EncryptionParameters::save_seal(std::ostream &stream, compr_mode_type compr_mode) const
    {
        wire::check_mode(compr_mode);
        wire::StreamSink sink(stream);
        sealfmt::put_parms(scheme_, poly_modulus_degree_, coeff_modulus_, sink);
        return save_size_seal();
    }
    inline std::streamoff EncryptionParameters::load_seal(wire::Source &src)
    {
        const sealfmt::Parms p = sealfmt::get_parms(src);
        EncryptionParameters fresh(static_cast<scheme_type>(p.scheme)); // throws for a scheme this build does not provide
        fresh.set_poly_modulus_degree(p.n);
        std::vector<Modulus> cm;
        for (auto q : p.primes)
        {
            cm.emplace_back(q);
        }
        fresh.set_coeff_modulus(cm);
        *this = fresh;
        return static_cast<std::streamoff>(src.consumed);
    }
    inline std::streamoff EncryptionParameters::load(const seal_byte *in, std::size_t size)
    {
        wire::BufferSource src(in, size);
        if (src.peek() == sealfmt::first_byte)
        {
            return load_seal(src);
        }
        const wire::Header h = wire::get_header(src);
        if (h.kind != wire::kind_encryption_parameters || h.count || h.flags || h.L < 1 || h.L > 256 ||
            h.total != sizeof(wire::Header) + 8 * (3 + std::size_t(h.L)))
        {
            throw std::logic_error("encryption parameters data is invalid");
        }
        std::vector<std::uint64_t> body(3 + h.L);
        std::memcpy(body.data(), src.view(8 * body.size()), 8 * body.size());
        EncryptionParameters fresh(static_cast<scheme_type>(body[0])); // throws for a scheme this build does not provide
        fresh.set_poly_modulus_degree(h.n);
        std::vector<Modulus> cm;
        for (std::size_t i = 0; i < h.L; i++)
        {
            cm.emplace_back(body[3 + i]);
        }
        fresh.set_coeff_modulus(cm);
        fresh.set_secret_key_hamming_weight(body[1]);
        fresh.set_sparse_slots(body[2]);
        *this = fresh;
        return static_cast<std::streamoff>(src.consumed);
    }
    inline std::streamoff EncryptionParameters::load(std::istream &stream)
    {
        wire::StreamSource src(stream);
        if (src.peek() == sealfmt::first_byte)
        {
            return load_seal(src);
        }
        std::vector<seal_byte> buf(sizeof(wire::Header));
        std::memcpy(buf.data(), src.view(sizeof(wire::Header)), sizeof(wire::Header));
        wire::Header h;
        std::memcpy(&h, buf.data(), sizeof(h));
        if (h.total < sizeof(h) || h.total > sizeof(h) + 8 * (3 + 256))
        {
            throw std::logic_error("encryption parameters data is invalid");
        }
        buf.resize(h.total);
        std::memcpy(buf.data() + sizeof(h), src.view(h.total - sizeof(h)), h.total - sizeof(h));
        return load(buf.data(), buf.size());
    }
} // namespace seal
