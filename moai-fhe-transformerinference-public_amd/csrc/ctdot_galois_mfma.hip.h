// ctdot_galois_mfma.hip.h -- moai_ct_dot_galois on the int8 matrix cores (MOAI_CTDOT_GALOIS_MFMA), included by elementwise.hip after
// matmul_mfma.hip.h, whose byte limbs (mm_digits), diagonal operand words (mm_diag), offset-2^31 recombination (mm_recombine) and
// 13 / 15 diagonal split at MM_DIGITS7_MAX it uses as they are, and after ctdot_galois.hip.h, whose sums it forms with the same bits:
//     out[j][p + 2 p'][i] = sum_t x[t][p][i] w[t][p'][table_j[i]] mod q, canonical          (A0, A1, B0, B1 = p + 2 p' = 0, 1, 2, 3).
//
// Gram block.  An element e = 1 mod 2^k permutes inside aligned blocks of N / 2^(k-1) coefficients (ctdot_galois.hip.h).  Where
// that block is at most CDGM_BLOCK = 128 coefficients, every word an output needs at coefficient c of block beta is an entry of
//     G_beta[c, p; c', p'] = sum_t x[t][p][c] w[t][p'][c']                     c, c' < 128 of the block, per prime:
// out[j][p + 2 p'][c] = G_beta[c, p; table_j[c] & 127, p'].  G_beta is a 256 x 256 x terms matrix product whose operands are plain
// contiguous segments of x and w: no operand is permuted on the way in, the permutation only selects entries on the way out.  MOAI's
// 127 elements 5^(256 i) at N = 2^16 act on a block as the cyclic group of order 128, so with the identity they use every entry
// of G once; the kernel does not need that: any elements, repeated or few, read the entries they need and the others are not written.
// Tile.  One v_mfma_i32_16x16x64_i8 tile is M = 2 cl + p (coefficient cl < 8 of a strip of x, polynomial p), N = 2 c'l + p'
// (coefficient c'l < 8 of a tile of w, polynomial p'), K = 8 terms x 8 digit slots; as in ctct_mfma.hip.h the A operand carries the
// diagonal (mm_diag of the byte-reversed digit word of x, formed once for both N tiles of a wave) and the B operand the plain digits
// of w.  The four polynomial products are four separate entries: nothing is joined across lanes.  Tiles are always full.
// Work split.  A workgroup of four waves owns one prime, one block and one strip of 8 coefficients of x: a 16 x 256 slice of G, 16
// N tiles.  A wave keeps two N tiles of accumulators (ND * 8 registers, what cc_block keeps), so the slice is formed in two passes
// over the terms: pass h covers coefficients 64 h .. 64 h + 63 of w, wave v the tiles 2 v and 2 v + 1 of those eight.  The
// accumulators stay in registers over all terms of a pass; the number of terms is limited by int32 alone (below).
// Operands through LDS, CDGM_STAGE = 16 terms (two K-steps) at a time.  Per term the strip of x is 2 x 64 bytes and the pass's half
// block of w 2 x 512 bytes, fetched as 16-byte chunks (five per thread and stage) into registers while the stage before is
// multiplied, and stored after it: two barriers per stage.  Pitches, in 8-byte words; LDS has 64 banks of 4 bytes and serves a
// 64-bit read of 32 lanes (two lane groups kg = lane / 16, whose terms differ by two) per pass:
//   w  [term][p'][64]: a lane group reads, per p', 8 consecutive words = 8 bank pairs; CDGM_WP = 72 = 8 mod 32 puts p' = 1 on the next
//      8 bank pairs, and CDGM_WT = 152 words (2 x 72 + 8) = 304 dwords makes two terms 608 = 32 mod 64 dwords: the other 16 bank pairs.
//   x  [term][p][8]: the group's 16 words are consecutive; CDGM_XT = 24 words makes two terms 96 = 32 mod 64 dwords likewise.
// Zero operands: nothing is fetched from past the end.  A stage slot past the last term fetches the last term again (inside the
// arrays, no branch) and is never read: the lanes of such a term read the stage's last valid term and select zero where the
// operand is formed, as in cc_block.
// Epilogue.  Each pass recombines its accumulators (16 values per lane in all) and puts the canonical residues into the strip's
// G[cl][c'][p + 2 p'] in LDS (8 x 128 x 4 words, 32 KiB; a lane's two polynomials p are one 16-byte store).  After both passes
// thread (j, cl) = (tid / 8, tid % 8) walks the requested outputs j, j + 32, ...: it reads its table entry, the four words
// G[cl][table & 127][0..3] (two 16-byte reads) and stores one word to each of the four sums, so that eight lanes write one 64-byte
// segment.  Tables and output indices come from a device array (CdgmOut) written before the launch: a call may have 128 outputs and more.
// int32.  |x_a w_b| <= 2^14 and a diagonal sums at most 8 digit pairs per term: |T_d| <= terms * 2^17, inside mm_recombine's
// |T_d| < 2^31 for terms <= CDGM_MAX_TERMS = 16383.  A longer sum is not chunked: the entry point leaves it on the integer forms.
// Bounds.  N is a power of two of at least 128, so blocks and strips are whole; a table entry is masked to the block; j < count
// selects the outputs that exist; every global offset is formed in size_t.
#pragma once
#include "ctdot_galois.hip.h"
#include "matmul_mfma.hip.h"

namespace moai {

constexpr uint32_t CDGM_BLOCK = 128;       // coefficients per Gram block: the largest closed block this form serves
constexpr uint32_t CDGM_STAGE = 16;        // terms per LDS stage
constexpr uint32_t CDGM_WP = 72, CDGM_WT = 2 * CDGM_WP + 8, CDGM_XT = 24; // pitches in words: polynomial and term of w, term of x
constexpr uint32_t CDGM_G_WORDS = 8 * CDGM_BLOCK * 4;
constexpr uint32_t CDGM_W_WORDS = CDGM_STAGE * CDGM_WT;
constexpr uint32_t CDGM_LDS_WORDS = CDGM_G_WORDS + CDGM_STAGE * (CDGM_WT + CDGM_XT);
constexpr size_t CDGM_MAX_TERMS = 16383;   // terms per sum in this form
constexpr int CDGM_WRITE = 64;             // CdgmOut records per launch of cdgm_outs_kernel
static_assert(CDGM_MAX_TERMS * 8 * (1u << 14) < (1ull << 31), "a diagonal sum over all terms fits int32 with the 2^31 offset");
static_assert((CDGM_MAX_TERMS + 1) * 8 * (1u << 14) >= (1ull << 31), "and one more term would not");
static_assert(CDGM_WP % 32 == 8 && (2 * 2 * CDGM_WT) % 64 == 32 && (2 * 2 * CDGM_XT) % 64 == 32 && CDGM_WP % 2 == 0 && CDGM_WT % 2 == 0,
              "the 32 lanes of a 64-bit LDS read fall in 32 bank pairs; 16-byte stores stay aligned");
static_assert(CDGM_STAGE % 8 == 0 && CDGM_LDS_WORDS * 8 <= 65536, "whole K-steps; two workgroups per CU");

struct CdgmOut
{
    const uint32_t *table; // galois_table of the output's element
    uint32_t oi, pad;      // out + oi * 4 * L * N
};

struct CdgmArgs
{
    const uint64_t *x;  // [terms][2][L][N]
    const uint64_t *w;  // [terms][2][L][N]
    uint64_t *out;      // [n_out][4][L][N]
    const PrimeConst *pc;
    uint32_t L, n2, terms, count;
    const CdgmOut *outs; // [count], device memory
};

struct CdgmOutsArgs
{
    CdgmOut e[CDGM_WRITE];
};

// the records of up to CDGM_WRITE outputs go to device memory on the call's stream as a kernel argument (as ks_list_write_kernel's do)
__global__ __launch_bounds__(CDGM_WRITE) void cdgm_outs_kernel(CdgmOutsArgs h, CdgmOut *d, uint32_t cnt)
{
    if (threadIdx.x < cnt)
    {
        d[threadIdx.x] = h.e[threadIdx.x];
    }
}

template <int ND>
__device__ __forceinline__ void cdgm_block(const CdgmArgs &g, uint64_t *lds)
{
    const uint32_t r = blockIdx.y;
    const PrimeConst *pc = g.pc + r;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const uint64_t t64 = barrett128(0, 1, q, cr0, cr1);
    const uint32_t tid = threadIdx.x, wv = tid >> 6, lane = tid & 63u, l16 = lane & 15u, kg = lane >> 4;
    const size_t n = 2 * (size_t)g.n2, row = (size_t)g.L * n;
    const size_t b0 = (size_t)(blockIdx.x >> 4) * CDGM_BLOCK; // the block's first coefficient
    const uint32_t c0 = (blockIdx.x & 15u) * 8u;              // the strip's first coefficient inside the block
    uint64_t *gl = lds, *wl = lds + CDGM_G_WORDS, *xl = wl + CDGM_W_WORDS;

    uint32_t bias_u[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
    {
        bias_u[d] = 0x80000000u;
    }
    const uint64_t bias = mm_recombine<ND>(bias_u, q, cr0, cr1, t64);

    // ---- the thread's chunks of a stage: four of w (chunk tid + 256 i: term 4 i + tid / 64, polynomial, 32 chunks of a half block)
    //      and, for the first 128 threads, one of x (term tid / 8, polynomial, 4 chunks of the strip)
    const uint32_t wt = tid >> 6, wp = (tid >> 5) & 1u, wc = 2u * (tid & 31u);
    const uint32_t xt = tid >> 3, xp = (tid >> 2) & 1u, xc = 2u * (tid & 3u);
    const uint64_t *wsrc = g.w + ((size_t)wp * g.L + r) * n + b0 + wc;
    const uint64_t *xsrc = g.x + ((size_t)xp * g.L + r) * n + b0 + c0 + xc;
    // a term past the last one fetches the last one again (inside the arrays, no branch); it is stored and never read
    const uint32_t last = g.terms - 1u;
    ulonglong2 wn0, wn1, wn2, wn3, xn = {};
    auto fetch = [&](uint32_t t0, uint32_t half) {
        const uint64_t *ws = wsrc + 64u * half;
        const uint32_t t = t0 + wt;
        wn0 = *chunks(ws + (size_t)(t < last ? t : last) * 2 * row);
        wn1 = *chunks(ws + (size_t)(t + 4u < last ? t + 4u : last) * 2 * row);
        wn2 = *chunks(ws + (size_t)(t + 8u < last ? t + 8u : last) * 2 * row);
        wn3 = *chunks(ws + (size_t)(t + 12u < last ? t + 12u : last) * 2 * row);
        if (tid < 128u)
        {
            xn = *chunks(xsrc + (size_t)(t0 + xt < last ? t0 + xt : last) * 2 * row);
        }
    };
    auto put = [&]() {
        uint64_t *wd = wl + wt * CDGM_WT + wp * CDGM_WP + wc;
        *chunks(wd) = wn0;
        *chunks(wd + 4u * CDGM_WT) = wn1;
        *chunks(wd + 8u * CDGM_WT) = wn2;
        *chunks(wd + 12u * CDGM_WT) = wn3;
        if (tid < 128u)
        {
            *chunks(xl + xt * CDGM_XT + xp * 8u + xc) = xn;
        }
    };

    // the lane's words of a staged term: x[p = l16 & 1][c0 + l16 / 2] and, per N tile, w[p' = l16 & 1][8 (2 wv + t) + l16 / 2]
    const uint32_t xoff = (l16 & 1u) * 8u + (l16 >> 1);
    const uint32_t woff = (l16 & 1u) * CDGM_WP + 16u * wv + (l16 >> 1);

    fetch(0, 0);
    for (uint32_t half = 0; half < 2u; ++half)
    {
        mm_v4i acc[ND][2];
#pragma unroll
        for (int d = 0; d < ND; ++d)
        {
            acc[d][0] = mm_v4i{ 0, 0, 0, 0 };
            acc[d][1] = mm_v4i{ 0, 0, 0, 0 };
        }
        for (uint32_t t0 = 0; t0 < g.terms; t0 += CDGM_STAGE)
        {
            const uint32_t kcur = g.terms - t0 < CDGM_STAGE ? g.terms - t0 : CDGM_STAGE;
            put();
            __syncthreads();
            // the next stage's chunks travel while this one is multiplied
            if (t0 + CDGM_STAGE < g.terms)
            {
                fetch(t0 + CDGM_STAGE, half);
            }
            else if (half == 0)
            {
                fetch(0, 1);
            }
            const uint32_t steps = (kcur + 7u) >> 3;
            for (uint32_t s = 0; s < steps; ++s)
            {
                const uint32_t tt = 8u * s + 2u * kg;
                uint64_t aw[2], bw[2][2];
#pragma unroll
                for (int e = 0; e < 2; ++e)
                {
                    const uint32_t tc = tt + e < kcur ? tt + e : kcur - 1u;
                    aw[e] = xl[tc * CDGM_XT + xoff];
                    bw[0][e] = wl[tc * CDGM_WT + woff];
                    bw[1][e] = wl[tc * CDGM_WT + woff + 8u];
                }
                // what was read for a term past the end becomes zero here, where it is used
                const uint64_t m0 = tt < kcur ? ~0ull : 0, m1 = tt + 1u < kcur ? ~0ull : 0;
                const uint64_t r0 = __builtin_bswap64(mm_digits(aw[0] & m0)), r1 = __builtin_bswap64(mm_digits(aw[1] & m1));
                const uint32_t rx[4] = { (uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32) };
                mm_v4i bop[2];
#pragma unroll
                for (int t = 0; t < 2; ++t)
                {
                    const uint64_t d0 = mm_digits(bw[t][0] & m0), d1 = mm_digits(bw[t][1] & m1);
                    bop[t] = mm_v4i{ (int)(uint32_t)d0, (int)(uint32_t)(d0 >> 32), (int)(uint32_t)d1, (int)(uint32_t)(d1 >> 32) };
                }
#pragma unroll
                for (int d = 0; d < ND; ++d)
                {
                    int a0, a1, a2, a3;
                    mm_diag(d, rx[0], rx[1], a0, a1);
                    mm_diag(d, rx[2], rx[3], a2, a3);
                    const mm_v4i aop = { a0, a1, a2, a3 };
                    acc[d][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aop, bop[0], acc[d][0], 0, 0, 0);
                    acc[d][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aop, bop[1], acc[d][1], 0, 0, 0);
                }
            }
            __syncthreads(); // every wave has read the stage before the next one is put
        }
        // ---- register v of tile t: M = 4 kg + v, so cl = 2 kg + v / 2 and p = v % 2; N = l16, so c' = 64 half + 8 (2 wv + t) + l16 / 2
        //      and p' = l16 % 2.  G[cl][c'][p + 2 p']: v = 0, 1 and v = 2, 3 are neighbours
#pragma unroll
        for (int t = 0; t < 2; ++t)
        {
            uint64_t res[4];
#pragma unroll
            for (int v = 0; v < 4; ++v)
            {
                uint32_t u[ND];
#pragma unroll
                for (int d = 0; d < ND; ++d)
                {
                    u[d] = (uint32_t)acc[d][t][v] ^ 0x80000000u;
                }
                res[v] = submod(mm_recombine<ND>(u, q, cr0, cr1, t64), bias, q);
            }
            const uint32_t cp = 64u * half + 16u * wv + 8u * t + (l16 >> 1);
            uint64_t *ge = gl + ((2u * kg) * CDGM_BLOCK + cp) * 4u + 2u * (l16 & 1u);
            *chunks(ge) = make_ulonglong2(res[0], res[1]);
            *chunks(ge + CDGM_BLOCK * 4u) = make_ulonglong2(res[2], res[3]);
        }
    }
    __syncthreads();

    // ---- the outputs: thread (j, cl) reads G[cl][table_j & 127][0..3]; eight lanes store one 64-byte segment of each sum
    const uint32_t cl = tid & 7u;
    const size_t at = (size_t)r * n + b0 + c0 + cl;
    for (uint32_t j = tid >> 3; j < g.count; j += 32u)
    {
        const CdgmOut o = g.outs[j];
        const uint32_t src = o.table[b0 + c0 + cl] & (CDGM_BLOCK - 1u);
        const uint64_t *ge = gl + (cl * CDGM_BLOCK + src) * 4u;
        const ulonglong2 a = *chunks(ge), b = *chunks(ge + 2);
        uint64_t *ob = g.out + (size_t)o.oi * 4 * row + at;
        ob[0] = a.x;
        ob[row] = a.y;
        ob[2 * row] = b.x;
        ob[3 * row] = b.y;
    }
}

// blockIdx.y = prime; blockIdx.x = block of CDGM_BLOCK coefficients * 16 + strip: the strips that read the same block of w are
// neighbours in launch order
__global__ __launch_bounds__(256, 2) void ct_dot_galois_mfma_kernel(CdgmArgs g)
{
    __shared__ __attribute__((aligned(16))) uint64_t lds[CDGM_LDS_WORDS];
    if (g.pc[blockIdx.y].q <= MM_DIGITS7_MAX)
    {
        cdgm_block<13>(g, lds);
    }
    else
    {
        cdgm_block<15>(g, lds);
    }
}

} // namespace moai
