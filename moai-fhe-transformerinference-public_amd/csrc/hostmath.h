// hostmath.h -- host-only number theory shared by context.hip, encoder.hip and decoder.hip.
#pragma once
#include "common.h"

namespace moai {

typedef unsigned __int128 u128;

static inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q)
{
    return (uint64_t)(((u128)a * b) % q);
}

static inline uint64_t powmod(uint64_t a, uint64_t e, uint64_t q)
{
    uint64_t r = 1;
    a %= q;
    while (e)
    {
        if (e & 1)
        {
            r = mulmod(r, a, q);
        }
        a = mulmod(a, a, q);
        e >>= 1;
    }
    return r;
}

// w with its Shoup quotient floor(w * 2^64 / q)
static inline Tw make_tw(uint64_t w, uint64_t q)
{
    Tw t;
    t.w = w;
    t.wq = (uint64_t)((((u128)w) << 64) / q);
    return t;
}

// the low `bits` bits of x in reverse order
static inline uint32_t bitrev(uint32_t x, int bits)
{
    return bits ? (__builtin_bitreverse32(x) >> (32 - bits)) : 0;
}

// a *= q for a little-endian multi-word a whose top word is not zero; it gains a word when the product carries out
static inline void mul_word(std::vector<uint64_t> &a, uint64_t q)
{
    u128 carry = 0;
    for (uint64_t &w : a)
    {
        const u128 t = (u128)w * q + carry;
        w = (uint64_t)t;
        carry = t >> 64;
    }
    if (carry)
    {
        a.push_back((uint64_t)carry);
    }
}

// the little-endian words, without leading zero words, of the product of the L context primes idx[0..L) (null: the first L);
// every index is below c->k
static inline std::vector<uint64_t> prime_product(const moai_ctx *c, const uint32_t *idx, size_t L)
{
    std::vector<uint64_t> prod(1, 1);
    for (size_t i = 0; i < L; i++)
    {
        mul_word(prod, c->primes[idx ? idx[i] : i]);
    }
    return prod;
}

// significant bits of such a product
static inline int bit_length(const std::vector<uint64_t> &a)
{
    return 64 * (int)a.size() - __builtin_clzll(a.back());
}

} // namespace moai
