// sealprng.hip -- Microsoft SEAL's default generator and its uniform sampler on the device (include/moai_hip.h, "SEAL's own
// format"): what a seeded ciphertext or key written by a SEAL client expands to, bit for bit.  tests/seal_format.py restates it.
//
// Blake2xbPRNG(seed) is counter mode (SEAL/randomgen.cpp:201-211 over SEAL/util/blake2xb.c:32-181): buffer c of 4096 bytes is
//   root_c    = BLAKE2b-512, keyed with the 64-byte seed and xof_length 4096, of the 8 bytes of c: two compressions, of which
//               the first (the padded key block) depends on the seed alone and is done once per seed ON THE HOST (SealArgs::h1)
//   block_c,i = one compression of root_c followed by zeros with node_offset i, for i < 64: bytes [64 i, 64 i + 64) of the buffer
//
//   seal_fill   : a wavefront owns 16 consecutive buffers.  Lanes 0..15 compute the 16 roots (one compression, every lane runs
//                 it, so the roots cost 1/16 on top of the blocks, and no lane recomputes a root); then per buffer the root is
//                 broadcast with v_readlane into scalar registers and lane i computes block i.  The message of that compression is
//                 the root and eight literal zeros.  RAW stores the words; WIDE (N >= 512: a buffer lies in one row) and NARROW
//                 fold in sample_poly_uniform's accept test and Barrett reduction (SEAL/util/rlwe.cpp:137-166): a rejected word is
//                 stored as all ones, which no residue equals, and counted per (polynomial, row).
//   seal_fixup  : one wavefront per polynomial; returns at once when the polynomial has no rejected word.  Otherwise it walks the
//                 rows that have some in SEAL's order (row, then coefficient), finds the marks with a ballot over 64 coefficients
//                 and replaces each by the next accepted word of the stream's tail, which it generates itself buffer by buffer
//                 into LDS.  Serial in the replaced words; bounded: a polynomial may consume 2 L N + 512 tail words, then the
//                 overflow word is set and the remaining marks stay (they fail the residue check).
//   seal_check  : is_data_valid_for's residue check on unpacked rows (SEAL/valcheck.cpp:302-335).
#include <mutex>

#include "launch.h"
#include "modarith.hip.h"

namespace moai {

#define B2_IV0 0x6A09E667F3BCC908ull
#define B2_IV1 0xBB67AE8584CAA73Bull
#define B2_IV2 0x3C6EF372FE94F82Bull
#define B2_IV3 0xA54FF53A5F1D36F1ull
#define B2_IV4 0x510E527FADE682D1ull
#define B2_IV5 0x9B05688C2B3E6C1Full
#define B2_IV6 0x1F83D9ABFB41BD6Bull
#define B2_IV7 0x5BE0CD19137E2179ull

// r is a literal at every call.  On the device a rotation by 32 renames the two halves and every other one is two
// v_alignbit_b32; written as 64-bit shifts the compiler spends five instructions on it.
__host__ __device__ __forceinline__ uint64_t rotr64(uint64_t x, int r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lo = r < 32 ? (uint32_t)x : (uint32_t)(x >> 32), hi = r < 32 ? (uint32_t)(x >> 32) : (uint32_t)x;
    if ((r & 31) == 0)
    {
        return ((uint64_t)hi << 32) | lo;
    }
    return ((uint64_t)__builtin_amdgcn_alignbit(lo, hi, r & 31) << 32) | __builtin_amdgcn_alignbit(hi, lo, r & 31);
#else
    return (x >> r) | (x << (64 - r));
#endif
}

#define B2_G(a, b, c, d, x, y)  \
    do                          \
    {                           \
        a = a + b + (x);        \
        d = rotr64(d ^ a, 32);  \
        c = c + d;              \
        b = rotr64(b ^ c, 24);  \
        a = a + b + (y);        \
        d = rotr64(d ^ a, 16);  \
        c = c + d;              \
        b = rotr64(b ^ c, 63);  \
    } while (0)

// the message indices are literals so that a message word that is a literal zero disappears from the round
#define B2_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    do                                                                                 \
    {                                                                                  \
        B2_G(v0, v4, v8, v12, m[s0], m[s1]);                                           \
        B2_G(v1, v5, v9, v13, m[s2], m[s3]);                                           \
        B2_G(v2, v6, v10, v14, m[s4], m[s5]);                                          \
        B2_G(v3, v7, v11, v15, m[s6], m[s7]);                                          \
        B2_G(v0, v5, v10, v15, m[s8], m[s9]);                                          \
        B2_G(v1, v6, v11, v12, m[s10], m[s11]);                                        \
        B2_G(v2, v7, v8, v13, m[s12], m[s13]);                                         \
        B2_G(v3, v4, v9, v14, m[s14], m[s15]);                                         \
    } while (0)

// RFC 7693's F: h <- F(h, m, t, last) for a byte counter t below 2^64
__host__ __device__ __forceinline__ void b2_compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last)
{
    uint64_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    uint64_t v8 = B2_IV0, v9 = B2_IV1, v10 = B2_IV2, v11 = B2_IV3, v12 = B2_IV4 ^ t, v13 = B2_IV5;
    uint64_t v14 = last ? ~B2_IV6 : B2_IV6, v15 = B2_IV7;
    B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    B2_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    B2_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    B2_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    B2_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    B2_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    B2_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    B2_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    B2_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
    B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    h[0] ^= v0 ^ v8;
    h[1] ^= v1 ^ v9;
    h[2] ^= v2 ^ v10;
    h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12;
    h[5] ^= v5 ^ v13;
    h[6] ^= v6 ^ v14;
    h[7] ^= v7 ^ v15;
}

constexpr uint32_t SEAL_BUF_WORDS = 512;  // one generator buffer: 4096 bytes (SEAL/randomgen.h, buffer_size_)
constexpr uint32_t SEAL_WAVE_BUFS = 16;   // buffers per wavefront
constexpr uint32_t SEAL_SEEDS = 32;       // seeds per launch: their states travel as kernel arguments
constexpr uint64_t SEAL_MARK = ~0ull;     // a rejected word until seal_fixup replaces it

enum
{
    FILL_RAW,
    FILL_WIDE,
    FILL_NARROW
};

struct SealArgs
{
    uint64_t h1[SEAL_SEEDS][8]; // per seed: the state after the key block
    uint64_t *out;              // polynomial (seed) p at out + p * stride
    size_t stride;              // in words
    uint32_t *cnt;              // [polynomials][L]: marks in each row
    uint32_t *rejected;         // NULL, or [0] += rejected stream words, [1] = 1 when a tail ran over its bound
    const PrimeConst *pc;
    RowMap rows;
    uint64_t first;             // counter of buffer 0
    uint64_t nbuf;              // buffers per polynomial
    uint32_t L;
    uint32_t logn;
};

__device__ __forceinline__ uint64_t readlane64(uint64_t x, uint32_t lane)
{
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)x, (int)lane);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)lane);
    return ((uint64_t)hi << 32) | lo;
}

// root of buffer `counter` from the state after the key block: the second and final compression, t = 128 + 8
__device__ __forceinline__ void seal_root(uint64_t h[8], uint64_t counter)
{
    const uint64_t m[16] = { counter, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    b2_compress(h, m, 136, true);
}

// bytes [64 i, 64 i + 64) of a buffer from its root: parameter block { digest_length 64, key_length 0, fanout 0, depth 0,
// leaf_length 64, node_offset i, xof_length 4096, node_depth 0, inner_length 64 }, one compression, t = 64, final
__device__ __forceinline__ void seal_block(uint64_t o[8], const uint64_t root[8], uint32_t i)
{
    const uint64_t m[16] = { root[0], root[1], root[2], root[3], root[4], root[5], root[6], root[7], 0, 0, 0, 0, 0, 0, 0, 0 };
    o[0] = B2_IV0 ^ 0x0000004000000040ull;
    o[1] = B2_IV1 ^ ((uint64_t)4096 << 32 | i);
    o[2] = B2_IV2 ^ 0x4000ull;
    o[3] = B2_IV3;
    o[4] = B2_IV4;
    o[5] = B2_IV5;
    o[6] = B2_IV6;
    o[7] = B2_IV7;
    b2_compress(o, m, 64, true);
}

// SEAL/util/rlwe.cpp:154: a word at or above it is rejected
__device__ __forceinline__ uint64_t max_multiple(uint64_t q, uint64_t cr1)
{
    return ~0ull - barrett64(~0ull, q, cr1) - 1;
}

template <int MODE>
__global__ __launch_bounds__(256) void seal_fill(SealArgs g)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t p = blockIdx.y;
    const uint64_t buf0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * SEAL_WAVE_BUFS;
    if (buf0 >= g.nbuf) // uniform over the wavefront
    {
        return;
    }
    uint64_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++)
    {
        h[i] = g.h1[p][i];
    }
    seal_root(h, g.first + buf0 + (lane & (SEAL_WAVE_BUFS - 1))); // lane b < 16 holds the root of buffer buf0 + b
    const uint32_t nb = (uint32_t)(g.nbuf - buf0 < SEAL_WAVE_BUFS ? g.nbuf - buf0 : SEAL_WAVE_BUFS);
    const uint64_t LN = (uint64_t)g.L << g.logn;
    uint64_t *poly = g.out + (size_t)p * g.stride;
#pragma unroll 1
    for (uint32_t b = 0; b < nb; b++)
    {
        uint64_t root[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
        {
            root[i] = readlane64(h[i], b);
        }
        seal_block(o, root, lane);
        const uint64_t w0 = (buf0 + b) * SEAL_BUF_WORDS + lane * 8; // stream word of o[0]
        if (MODE == FILL_RAW)
        {
#pragma unroll
            for (int j = 0; j < 8; j += 2)
            {
                *reinterpret_cast<ulonglong2 *>(poly + w0 + j) = make_ulonglong2(o[j], o[j + 1]);
            }
        }
        else if (MODE == FILL_WIDE)
        {
            // N >= 512: the buffer lies in one row, and L N is a multiple of 512, so all of it is in range
            const uint32_t row = __builtin_amdgcn_readfirstlane((uint32_t)(w0 >> g.logn));
            const PrimeConst &pc = g.pc[g.rows.idx[row]];
            const uint64_t q = pc.q, cr1 = pc.cr1, mm = max_multiple(q, cr1);
            uint32_t nrej = 0;
#pragma unroll
            for (int j = 0; j < 8; j++)
            {
                const bool rej = o[j] >= mm;
                nrej += rej;
                o[j] = rej ? SEAL_MARK : barrett64(o[j], q, cr1);
            }
#pragma unroll
            for (int j = 0; j < 8; j += 2)
            {
                *reinterpret_cast<ulonglong2 *>(poly + w0 + j) = make_ulonglong2(o[j], o[j + 1]);
            }
            if (nrej)
            {
                atomicAdd(g.cnt + p * g.L + row, nrej);
                if (g.rejected)
                {
                    atomicAdd(g.rejected, nrej);
                }
            }
        }
        else
        {
            // rows shorter than a buffer, and a last buffer that runs into the tail: word by word
#pragma unroll 1
            for (int j = 0; j < 8; j++)
            {
                const uint64_t w = w0 + j;
                if (w < LN)
                {
                    const uint32_t row = (uint32_t)(w >> g.logn);
                    const PrimeConst &pc = g.pc[g.rows.idx[row]];
                    const uint64_t q = pc.q, cr1 = pc.cr1;
                    const bool rej = o[j] >= max_multiple(q, cr1);
                    poly[w] = rej ? SEAL_MARK : barrett64(o[j], q, cr1);
                    if (rej)
                    {
                        atomicAdd(g.cnt + p * g.L + row, 1u);
                        if (g.rejected)
                        {
                            atomicAdd(g.rejected, 1u);
                        }
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void seal_fixup(SealArgs g)
{
    __shared__ uint64_t tail[SEAL_BUF_WORDS];
    const uint32_t lane = threadIdx.x;
    const uint32_t p = blockIdx.x;
    const uint32_t *cnt = g.cnt + p * g.L;
    uint32_t total = 0;
    for (uint32_t j = 0; j < g.L; j++)
    {
        total |= cnt[j];
    }
    if (__builtin_amdgcn_readfirstlane(total) == 0)
    {
        return; // the ordinary case
    }
    const uint32_t n = 1u << g.logn;
    const uint64_t LN = (uint64_t)g.L << g.logn;
    const uint64_t cap = 2 * LN + SEAL_BUF_WORDS;
    uint64_t *poly = g.out + (size_t)p * g.stride;
    // the tail starts at stream word L N: inside buffer L N / 512 when that is not a multiple of 512
    uint64_t next = LN / SEAL_BUF_WORDS, consumed = 0;
    uint32_t tpos = (uint32_t)(LN % SEAL_BUF_WORDS), extra = 0;
    bool have = false; // tail[] holds buffer next - 1
    // the next word of the tail that is below mm; false when the polynomial has used up its bound.  Uniform over the wavefront.
    auto take = [&](uint64_t mm, uint64_t &w) -> bool {
        for (;;)
        {
            if (consumed >= cap)
            {
                return false;
            }
            if (!have || tpos == SEAL_BUF_WORDS)
            {
                uint64_t h[8], o[8];
#pragma unroll
                for (int k = 0; k < 8; k++)
                {
                    h[k] = g.h1[p][k];
                }
                seal_root(h, next);
                seal_block(o, h, lane);
                __syncthreads(); // every lane is done with the previous buffer
#pragma unroll
                for (int k = 0; k < 8; k++)
                {
                    tail[lane * 8 + k] = o[k];
                }
                __syncthreads();
                tpos = have ? 0 : tpos;
                have = true;
                next++;
            }
            w = tail[tpos++];
            consumed++;
            if (w < mm)
            {
                return true;
            }
            extra++;
        }
    };
    auto finish = [&](bool overflow) {
        if (g.rejected && lane == 0)
        {
            if (extra)
            {
                atomicAdd(g.rejected, extra);
            }
            if (overflow)
            {
                g.rejected[1] = 1;
            }
        }
    };
    for (uint32_t j = 0; j < g.L; j++)
    {
        const uint32_t want = __builtin_amdgcn_readfirstlane(cnt[j]);
        if (want == 0)
        {
            continue;
        }
        const PrimeConst &pc = g.pc[g.rows.idx[j]];
        const uint64_t q = pc.q, cr1 = pc.cr1, mm = max_multiple(q, cr1);
        uint64_t *row = poly + ((size_t)j << g.logn);
        uint32_t served = 0;
        for (uint32_t base = 0; base < n && served < want; base += 64)
        {
            const uint32_t i = base + lane;
            const uint64_t v = i < n ? row[i] : 0;
            uint64_t marks = __ballot(v == SEAL_MARK);
            while (marks) // uniform over the wavefront
            {
                const uint32_t bit = (uint32_t)__builtin_ctzll(marks);
                marks &= marks - 1;
                uint64_t w;
                if (!take(mm, w))
                {
                    finish(true);
                    return;
                }
                if (lane == 0)
                {
                    row[base + bit] = barrett64(w, q, cr1);
                }
                served++;
            }
        }
    }
    finish(false);
}

struct CheckArgs
{
    const uint64_t *data;
    uint32_t *invalid;
    const PrimeConst *pc;
    RowMap rows;
    uint32_t L;
    uint32_t logn;
};

__global__ __launch_bounds__(256) void seal_check(CheckArgs g)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 1u << g.logn)
    {
        return;
    }
    const uint64_t q = g.pc[g.rows.idx[blockIdx.y]].q;
    if (g.data[(((size_t)blockIdx.z * g.L + blockIdx.y) << g.logn) + i] >= q)
    {
        *g.invalid = 1; // every lane that finds one stores the same value: no atomic needed
    }
}

// the state after the key block of Blake2xbPRNG(seed): parameter block { digest_length 64, key_length 64, fanout 1, depth 1,
// leaf_length 0, node_offset 0, xof_length 4096, node_depth 0, inner_length 0 }, the seed padded to 128 bytes, t = 128
static void key_state(const uint8_t *seed, uint64_t h[8])
{
    uint64_t m[16] = {};
    for (int i = 0; i < 64; i++)
    {
        m[i / 8] |= (uint64_t)seed[i] << (8 * (i % 8));
    }
    const uint64_t iv[8] = { B2_IV0, B2_IV1, B2_IV2, B2_IV3, B2_IV4, B2_IV5, B2_IV6, B2_IV7 };
    for (int i = 0; i < 8; i++)
    {
        h[i] = iv[i];
    }
    h[0] ^= 0x01014040ull;
    h[1] ^= (uint64_t)4096 << 32;
    b2_compress(h, m, 128, false);
}

// moai_seal_sample_uniform after its checks, for a caller that holds op_mutex and owns the scratch (launch.h)
int seal_uniform_launch(moai_ctx *c, const uint8_t *seeds, uint64_t *out, size_t stride_words, size_t count, size_t L,
                        const RowMap &rows, uint32_t *cnt, uint32_t *rejected, hipStream_t s)
{
    const size_t LN = L * c->n;
    MOAI_HIP_CHECK(hipMemsetAsync(cnt, 0, count * L * sizeof(uint32_t), s));
    SealArgs a = {};
    a.rows = rows;
    a.stride = stride_words;
    a.rejected = rejected;
    a.pc = c->pc;
    a.nbuf = (LN + SEAL_BUF_WORDS - 1) / SEAL_BUF_WORDS;
    a.L = (uint32_t)L;
    a.logn = (uint32_t)c->logn;
    const uint32_t blocks = (uint32_t)((a.nbuf + 4 * SEAL_WAVE_BUFS - 1) / (4 * SEAL_WAVE_BUFS));
    return for_chunks(count, SEAL_SEEDS, [&](size_t p0, size_t np) {
        for (size_t p = 0; p < np; p++)
        {
            key_state(seeds + (p0 + p) * 64, a.h1[p]);
        }
        a.out = out + p0 * stride_words;
        a.cnt = cnt + p0 * L;
        hipLaunchKernelGGL(c->logn >= 9 ? seal_fill<FILL_WIDE> : seal_fill<FILL_NARROW>, dim3(blocks, (uint32_t)np), dim3(256), 0, s, a);
        MOAI_LAUNCH_CHECK();
        hipLaunchKernelGGL(seal_fixup, dim3((uint32_t)np), dim3(64), 0, s, a);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    });
}

} // namespace moai

using namespace moai;

extern "C" int moai_seal_prng_bytes(moai_ctx *c, const uint8_t *seed, uint64_t first_block, uint64_t n_blocks, void *out, void *stream)
{
    MOAI_AUDIT(stream, out);
    trace_op("seal_prng_bytes", 1, n_blocks);
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (!seed)
    {
        return set_error(MOAI_EINVAL, "null seed");
    }
    if (n_blocks == 0)
    {
        return MOAI_OK;
    }
    if (!out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    if ((uintptr_t)out & 15)
    {
        return set_error(MOAI_EINVAL, "out must be 16-byte aligned");
    }
    if (first_block + (n_blocks - 1) < first_block)
    {
        return set_error(MOAI_EINVAL, "block range wraps around 2^64");
    }
    if (n_blocks > ((uint64_t)1 << 36))
    {
        return set_error(MOAI_EINVAL, "too many blocks");
    }
    MOAI_TRY(enter_device(c));
    SealArgs a = {};
    key_state(seed, a.h1[0]);
    a.out = static_cast<uint64_t *>(out);
    a.first = first_block;
    a.nbuf = n_blocks;
    const uint64_t per_block = 4 * SEAL_WAVE_BUFS;
    hipLaunchKernelGGL(seal_fill<FILL_RAW>, dim3((uint32_t)((n_blocks + per_block - 1) / per_block)), dim3(256), 0, (hipStream_t)stream, a);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

extern "C" int moai_seal_sample_uniform(moai_ctx *c, const uint8_t *seeds, uint64_t *out, size_t stride_words, size_t count, size_t L,
                                        const uint32_t *prime_index, uint32_t *rejected, void *stream)
{
    MOAI_AUDIT(stream, out, rejected);
    trace_op("seal_sample_uniform", L, count);
    RowMap rows;
    MOAI_TRY(rows_entry(c, L, prime_index, &rows));
    if (!seeds)
    {
        return set_error(MOAI_EINVAL, "null seed");
    }
    if (!out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    if (count == 0 || count > ((size_t)1 << 24))
    {
        return set_error(MOAI_EINVAL, "count must be between 1 and 2^24");
    }
    const size_t LN = L * c->n;
    if (stride_words < LN)
    {
        return set_error(MOAI_EINVAL, "stride is smaller than a polynomial");
    }
    if (((uintptr_t)out & 15) || ((stride_words & 1) && count > 1))
    {
        return set_error(MOAI_EINVAL, "out must be 16-byte aligned");
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> op(*static_cast<std::mutex *>(c->op_mutex));
    void *ws = nullptr;
    MOAI_TRY(workspace(c, count * L * sizeof(uint32_t), s, &ws));
    return seal_uniform_launch(c, seeds, out, stride_words, count, L, rows, static_cast<uint32_t *>(ws), rejected, s);
}

extern "C" int moai_check_residues(moai_ctx *c, const uint64_t *data, size_t n_poly, size_t L, const uint32_t *prime_index,
                                   uint32_t *invalid, void *stream)
{
    MOAI_AUDIT(stream, data, invalid);
    trace_op("check_residues", L, n_poly);
    CheckArgs a;
    MOAI_TRY(rows_entry(c, L, prime_index, &a.rows));
    if (n_poly == 0)
    {
        return MOAI_OK;
    }
    if (!data || !invalid)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    if (n_poly > ((size_t)1 << 40))
    {
        return set_error(MOAI_EINVAL, "too many polynomials");
    }
    MOAI_TRY(enter_device(c));
    a.invalid = invalid;
    a.pc = c->pc;
    a.L = (uint32_t)L;
    a.logn = (uint32_t)c->logn;
    // gridDim.z holds at most 65535 polynomials
    return for_chunks(n_poly, 65535, [&](size_t p0, size_t np) {
        a.data = data + p0 * L * c->n;
        hipLaunchKernelGGL(seal_check, dim3((uint32_t)((c->n + 255) / 256), (uint32_t)L, (uint32_t)np), dim3(256), 0, (hipStream_t)stream, a);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    });
}
