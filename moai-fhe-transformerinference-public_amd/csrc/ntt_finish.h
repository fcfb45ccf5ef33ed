// ntt_finish.h -- the arithmetic of the passes that finish a 60-bit transform (M_LAZY8 / M_LAZY16, modarith.hip.h): N^-1 by shift
// and the one-step final reduction.  Plain C++ for the device and the host alike, so that a CPU program can check it against
// 128-bit arithmetic (tests/cpp/test_ntt_finish_arith.cpp); context.hip computes the per-prime constants with the functions at
// the end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MOAI_HD __host__ __device__ __forceinline__
#else
#define MOAI_HD inline
#endif

namespace moai {

// lo | hi << 32, put together as a pair of words.  Spelled ((uint64_t)hi << 32) | lo, the shift discards the upper half of the
// zero-extended hi, which lets the device compiler evaluate the whole 32-bit sum behind hi in 64 bits instead:
// mul_shoup_approx's four cross products y0 w1 + y1 w0 + t0 n1 + t1 n0 (modarith.hip.h) became 64-bit multiplies of a word by a
// whole operand (y w1, y1 w, ...), each lowered to a v_mad_u64_u32 chain -- one more multiply-add and a register copy per
// butterfly in every lazy kernel, and where the twiddle is wave-uniform (the inverse strided pass's phase A and last stage)
// multiplies by the literal 0 that stands for the low word of  w << 32  on top: 374 v_mad_u64_u32 and 171 copies per thread
// where 216 and none do the work.
MOAI_HD uint64_t pack64(uint32_t lo, uint32_t hi)
{
#if defined(__clang__)
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 r = { lo, hi };
    return __builtin_bit_cast(uint64_t, r);
#else
    return ((uint64_t)hi << 32) | lo;
#endif
}

// x * N^-1 mod q for N = 2^logn and a prime q = 1 (mod 2N), without the Shoup product.  q = qh N + 1 gives N qh = -1, so
// N^-1 = -qh (mod q); with m = (-x) mod N the sum x + m is a multiple of N and
//     x N^-1 = (x + m) N^-1 - m N^-1 = (x + m) / N + m qh   (mod q).
// Bounds, for x < 16q < 2^64: x + m <= 16q - 1 + N - 1 < 2^64 (16q <= 2^64 - 32N + 16); m qh <= (N - 1)(q - 1)/N < q; the
// result is below 16q/N + 1 + q, which is below q (1 + 16/4096) + 1 < 2q for logn >= 12 (q > 2^20).  At logn = 1 it reaches 8.5q:
// the tiled kernels only.  The product m qh is one multiply-add on the low word of qh plus m * hi(qh) into the high word; m and
// hi(qh) are below 2^24 (q < 2^60 and logn >= 12 put qh below 2^48), which the mask tells the device compiler: a 24-bit multiply-add.
MOAI_HD uint64_t ninv_by_shift(uint64_t x, uint64_t qh, int logn)
{
    const uint32_t m = (0u - (uint32_t)x) & ((1u << logn) - 1u);
    const uint64_t r = ((x + m) >> logn) + (uint64_t)m * (uint32_t)qh;
    return pack64((uint32_t)r, (uint32_t)(r >> 32) + m * ((uint32_t)(qh >> 32) & 0xffffffu));
}
constexpr int NINV_SHIFT_IN = 16; // accepts x below 16q ...
constexpr int NINV_SHIFT_OUT = 2; // ... and returns a value below 2q (logn >= 12)

// One quotient step that takes z < 16q to z mod q + {0, q}:  k = floor(floor(z / 2^s) M / 2^32) with M = floor(2^(32+s) / q)
// never exceeds z / q, and falls short of it by less than 1 + 2^s/q + z/2^(32+s).  With s = max(bits(q) - 20, 0) the last two
// terms are below 2^-19 (1/q where s = 0) and 2^-8 (z < 2^(bits+4)), so k is floor(z/q) or one less and  z - k q  is below 2q; z >> s is below
// 2^24 and M below 2^32 (2^s < q).  The difference is formed modulo 2^64 as z + k (2^64 - q): one multiply-add on the low
// words plus k * hi(2^64 - q) into the high word.  The caller subtracts q once more where the value is q or more.
MOAI_HD uint64_t final_quotient_step(uint64_t z, uint32_t s, uint32_t M, uint64_t nq)
{
    const uint32_t k = (uint32_t)(((uint64_t)(uint32_t)(z >> s) * M) >> 32);
    const uint64_t r = z + (uint64_t)k * (uint32_t)nq;
    return pack64((uint32_t)r, (uint32_t)(r >> 32) + k * (uint32_t)(nq >> 32));
}
constexpr int FINAL_STEP_IN = 16; // accepts z below 16q ...
constexpr int FINAL_STEP_OUT = 2; // ... and returns a value below 2q

// ---- the per-prime constants (host) ---------------------------------------------------------------------------------
inline uint64_t ninv_shift_qh(uint64_t q, int logn)
{
    return (q - 1) >> logn;
}
inline uint32_t final_step_shift(uint64_t q)
{
    int bits = 0;
    while (bits < 64 && (q >> bits))
    {
        ++bits;
    }
    return (uint32_t)(bits > 20 ? bits - 20 : 0);
}
inline uint32_t final_step_mult(uint64_t q, uint32_t s)
{
    return (uint32_t)(((unsigned __int128)1 << (32 + s)) / q);
}

} // namespace moai
