// seal/util/blake2b.h -- a small host BLAKE2b (RFC 7693, sequential mode, unkeyed) for the one hash the seal:: surface needs:
// SEAL's parms_id, BLAKE2b-256 over the parameters as an array of 64-bit words (SEAL/util/hash.h:29-36 under
// EncryptionParameters::compute_parms_id, SEAL/encryptionparams.cpp:124-158).  tests/seal_format.py restates it.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace seal
{
    namespace util
    {
        inline void blake2b_compress(std::uint64_t h[8], const std::uint64_t m[16], std::uint64_t t, bool last)
        {
            static const std::uint64_t iv[8] = { 0x6A09E667F3BCC908ull, 0xBB67AE8584CAA73Bull, 0x3C6EF372FE94F82Bull, 0xA54FF53A5F1D36F1ull,
                                                 0x510E527FADE682D1ull, 0x9B05688C2B3E6C1Full, 0x1F83D9ABFB41BD6Bull, 0x5BE0CD19137E2179ull };
            static const std::uint8_t sigma[10][16] = {
                { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 }, { 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3 },
                { 11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4 }, { 7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8 },
                { 9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13 }, { 2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9 },
                { 12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11 }, { 13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10 },
                { 6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5 }, { 10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0 }
            };
            std::uint64_t v[16];
            for (int i = 0; i < 8; i++)
            {
                v[i] = h[i];
                v[i + 8] = iv[i];
            }
            v[12] ^= t;
            if (last)
            {
                v[14] = ~v[14];
            }
            auto rotr = [](std::uint64_t x, int r) { return (x >> r) | (x << (64 - r)); };
            auto g = [&](int a, int b, int c, int d, std::uint64_t x, std::uint64_t y) {
                v[a] = v[a] + v[b] + x;
                v[d] = rotr(v[d] ^ v[a], 32);
                v[c] = v[c] + v[d];
                v[b] = rotr(v[b] ^ v[c], 24);
                v[a] = v[a] + v[b] + y;
                v[d] = rotr(v[d] ^ v[a], 16);
                v[c] = v[c] + v[d];
                v[b] = rotr(v[b] ^ v[c], 63);
            };
            for (int r = 0; r < 12; r++)
            {
                const std::uint8_t *s = sigma[r % 10];
                g(0, 4, 8, 12, m[s[0]], m[s[1]]);
                g(1, 5, 9, 13, m[s[2]], m[s[3]]);
                g(2, 6, 10, 14, m[s[4]], m[s[5]]);
                g(3, 7, 11, 15, m[s[6]], m[s[7]]);
                g(0, 5, 10, 15, m[s[8]], m[s[9]]);
                g(1, 6, 11, 12, m[s[10]], m[s[11]]);
                g(2, 7, 8, 13, m[s[12]], m[s[13]]);
                g(3, 4, 9, 14, m[s[14]], m[s[15]]);
            }
            for (int i = 0; i < 8; i++)
            {
                h[i] ^= v[i] ^ v[i + 8];
            }
        }

        // BLAKE2b-256 of `count` little-endian 64-bit words, read back as four little-endian words
        inline std::array<std::uint64_t, 4> blake2b_256_words(const std::uint64_t *words, std::size_t count)
        {
            std::uint64_t h[8] = { 0x6A09E667F3BCC908ull ^ 0x01010020ull, 0xBB67AE8584CAA73Bull, 0x3C6EF372FE94F82Bull, 0xA54FF53A5F1D36F1ull,
                                   0x510E527FADE682D1ull, 0x9B05688C2B3E6C1Full, 0x1F83D9ABFB41BD6Bull, 0x5BE0CD19137E2179ull };
            std::size_t done = 0;
            std::uint64_t m[16];
            while (count - done > 16)
            {
                std::memcpy(m, words + done, 128);
                done += 16;
                blake2b_compress(h, m, 8 * done, false);
            }
            std::memset(m, 0, sizeof(m));
            std::memcpy(m, words + done, 8 * (count - done));
            blake2b_compress(h, m, 8 * count, true);
            return { h[0], h[1], h[2], h[3] };
        }

        // SEAL's parms_id of CKKS parameters: the words [scheme = 2, N, q_0 .. q_{L-1}, plain_modulus = 0]
        inline std::array<std::uint64_t, 4> seal_parms_id(std::uint64_t n, const std::vector<std::uint64_t> &primes)
        {
            std::vector<std::uint64_t> w = { 2, n };
            w.insert(w.end(), primes.begin(), primes.end());
            w.push_back(0);
            return blake2b_256_words(w.data(), w.size());
        }
    } // namespace util
} // namespace seal
