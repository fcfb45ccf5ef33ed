// ctct_mfma.hip.h -- moai_ct_ct_matmul on the int8 matrix cores, included by elementwise.hip after matmul_mfma.hip.h, whose byte
// limbs (mm_digits), diagonal operand words (mm_diag), offset-2^31 recombination (mm_recombine) and 13 / 15 diagonal split at
// MM_DIGITS7_MAX it uses as they are.  The same canonical residues as ct_dot_kernel per (i, j):
//     out[j][i] = (sum_t a0 b0, sum_t (a0 b1 + a1 b0), sum_t a1 b1) mod q   with a = a[i][t], b = b[j][t], per prime and coefficient.
//
// Tile.  No operand is shared between coefficients, so one v_mfma_i32_16x16x64_i8 tile belongs to ONE coefficient: its M index is
// 2 il + p (ciphertext il < 8 of a, polynomial p), its N index 2 jl + p' (ciphertext jl < 8 of b, polynomial p'), its K = 64 is
// 8 terms t x 8 digit slots.  The tile of diagonal d holds all four polynomial products of 8 x 8 ciphertext pairs:
//     c0 = tile[2 il][2 jl],  c2 = tile[2 il + 1][2 jl + 1],  c1 = tile[2 il][2 jl + 1] + tile[2 il + 1][2 jl].
// The A operand carries the diagonal: byte slot s of term t holds digit d - s of the a word (mm_diag of the byte-reversed digit
// word), the B operand the plain digits of the b word, so T_d = sum_t sum_s a_(d-s) b_s.  A wave keeps one M tile x CC_NT = 2 N
// tiles of one coefficient (ND * 8 accumulator registers); the A operand of a diagonal is formed once and feeds both N tiles.
// Middle term.  Lane l holds, in register v, M = 4 (l / 16) + v and N = l % 16: ciphertexts ia = 2 (l / 16) (v = 0, 1) and
// ib = ia + 1 (v = 2, 3) of the M tile, and column jl = (l % 16) / 2 with p' = l % 2.  An even lane holds c0(ia), c0(ib) and the
// halves tile[2 ia + 1][2 jl], tile[2 ib + 1][2 jl] of c1; its odd neighbour holds c2(ia), c2(ib) and the other halves.  One DPP
// exchange per diagonal (quad_perm [1, 0, 3, 2]) gives the even lane the missing half of c1(ia) and the odd lane that of c1(ib);
// the halves are added as int32 diagonal sums, so every lane recombines three values per N tile, three per ciphertext pair.
// int32.  A half is at most k * 8 * 2^14 in magnitude, the sum of two 2 * k * 8 * 2^14 <= 2^30 for k <= CC_KMAX = 4096, inside the
// |T_d| < 2^31 that mm_recombine's offset needs.  Larger k is refused by the entry point, not chunked.
// Operands through LDS.  A workgroup (four waves, two workgroups per CU) owns 16 consecutive coefficients of one prime, one M tile
// and one pair of N tiles.  It reads the 128-byte segment of those coefficients from every (ciphertext, polynomial, term) row it
// needs -- eight lanes x 16 bytes per row, 32 rows per pass -- into LDS as stage[term][row][CC_PITCH], rows = the valid rows of
// the A tile followed by the valid rows of the B tiles.  CC_PITCH = 17 words: the 16 rows that the lanes of one lane group read
// for one coefficient are 34 dwords apart and fall in 16 different bank pairs.  Each wave then walks four of the coefficients; for
// each it reads its two A words and two B words per N tile and K-step from LDS, one step ahead of the MFMAs that use them.  A stage
// holds as many terms as 64 KB allow: all of them when k * rows * 17 words fit (k <= 12 at MOAI's 16 + 22 rows, k <= 10 at the
// full 48), else a multiple of eight; a later stage adds its residues onto what the same lane stored for the stage before.
// While one workgroup of a CU waits for its stage the other one computes; within a workgroup the stage is not double-buffered
// (the recombinations, not the loads, set the time).
// Zero operands: terms past the stage's end and ciphertexts past m or nb are never read from memory; their lanes read a valid
// LDS word and select zero where it is used, as in mm_mfma_wave.
#pragma once
#include "matmul_mfma.hip.h"

namespace moai {

constexpr int CC_NT = 2;               // N tiles (of eight ciphertexts of b) per wave
constexpr uint32_t CC_KMAX = 4096;     // terms per sum
constexpr uint32_t CC_PITCH = 17;      // words from one staged row to the next: 16 coefficients and one of padding
constexpr uint32_t CC_LDS_WORDS = 8192;
static_assert(2ull * CC_KMAX * 8 * (1u << 14) <= (1ull << 30), "the summed middle term's diagonals fit int32 with the 2^31 offset");
static_assert((16 + 16 * CC_NT) * CC_PITCH * 8 <= CC_LDS_WORDS, "a stage holds at least one K-step of the full tile");

struct CtCtArgs
{
    const uint64_t *a; // [m][k][2][L][N]
    const uint64_t *b; // [nb][k][2][L][N]
    uint64_t *out;     // [nb][m][3][L][N]
    const PrimeConst *pc;
    uint32_t L, n2, m, nb, k;
    uint32_t mtiles, ngroups; // M tiles of 8 and N groups of 8 * CC_NT ciphertexts
};

// One workgroup: coefficients n0 .. n0 + 15 of prime blockIdx.y, ciphertexts i0 .. of a (ar = 2 * valid ones rows) and j0 .. of b
// (br rows, in NT tiles of 16).
template <int ND, int NT>
__device__ __forceinline__ void cc_block(const CtCtArgs &g, uint64_t *lds, const uint32_t i0, const uint32_t j0, const uint32_t n0,
                                         const uint32_t ar, const uint32_t br)
{
    const uint32_t r = blockIdx.y;
    const PrimeConst *pc = g.pc + r;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const uint64_t t64 = barrett128(0, 1, q, cr0, cr1);
    const uint32_t tid = threadIdx.x, wv = tid >> 6, lane = tid & 63u, l16 = lane & 15u, kg = lane >> 4;
    const bool odd = l16 & 1u;
    const size_t n = 2 * (size_t)g.n2;
    const uint32_t rows = ar + br;
    const uint32_t cap = CC_LDS_WORDS / (rows * CC_PITCH);
    const uint32_t kc = g.k <= cap ? g.k : cap & ~7u;

    // the lane's rows of the stage; a row past the tile's valid ones reads row 0 and selects zero
    const bool av = l16 < ar;
    const uint32_t arow = av ? l16 : 0u;
    bool bv[NT];
    uint32_t brow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
    {
        bv[t] = 16u * t + l16 < br;
        brow[t] = ar + (bv[t] ? 16u * t + l16 : 0u);
    }
    uint32_t bias_u[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
    {
        bias_u[d] = 0x80000000u;
    }
    const uint64_t bias = mm_recombine<ND>(bias_u, q, cr0, cr1, t64);

    // where the lane's three values per N tile go: (ia, ib, the middle term of ia or ib) x (c0 or c2, c0 or c2, c1)
    const uint32_t ia = i0 + 2u * kg;
    const uint32_t oi[3] = { ia, ia + 1u, odd ? ia + 1u : ia };
    const uint32_t oc[3] = { odd ? 2u : 0u, odd ? 2u : 0u, 1u };

    for (uint32_t t0 = 0; t0 < g.k; t0 += kc)
    {
        const uint32_t kcur = g.k - t0 < kc ? g.k - t0 : kc;
        if (t0)
        {
            __syncthreads(); // every wave has read the stage before
        }
        // ---- stage: segment s = term * rows + row, eight lanes x 16 bytes each
        const uint32_t part = 2u * (tid & 7u), total = kcur * rows;
#pragma unroll 4
        for (uint32_t s = tid >> 3; s < total; s += 32u)
        {
            const uint32_t t = s / rows, row = s - t * rows;
            const bool is_a = row < ar;
            const uint32_t ct = is_a ? i0 + (row >> 1) : j0 + ((row - ar) >> 1); // ar is even: row & 1 is the polynomial of either
            const uint64_t *src = (is_a ? g.a : g.b) + ((((size_t)ct * g.k + t0 + t) * 2 + (row & 1u)) * g.L + r) * n + n0 + part;
            const ulonglong2 v = *chunks(src);
            lds[s * CC_PITCH + part] = v.x;
            lds[s * CC_PITCH + part + 1u] = v.y;
        }
        __syncthreads();

        // ---- each wave: four coefficients, one after another; two neighbours leave as one 16-byte store
        const uint32_t steps = (kcur + 7u) >> 3;
        uint64_t prev[NT][3] = {};
#pragma unroll 1
        for (uint32_t cc = 0; cc < 4u; ++cc)
        {
            const uint32_t c = 4u * wv + cc;
            mm_v4i acc[ND][NT];
#pragma unroll
            for (int d = 0; d < ND; ++d)
            {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                {
                    acc[d][t] = mm_v4i{ 0, 0, 0, 0 };
                }
            }
            uint64_t aw[2], bw[NT][2];
            auto load = [&](uint32_t s) {
#pragma unroll
                for (int e = 0; e < 2; ++e)
                {
                    const uint32_t tt = 8u * s + 2u * kg + e;
                    const uint32_t base = (tt < kcur ? tt : kcur - 1u) * rows;
                    aw[e] = lds[(base + arow) * CC_PITCH + c];
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                    {
                        bw[t][e] = lds[(base + brow[t]) * CC_PITCH + c];
                    }
                }
            };
            load(0);
            for (uint32_t s = 0; s < steps; ++s)
            {
                // what was read for a term past the end or a row past the tile becomes zero here, where it is used
                const uint32_t tt = 8u * s + 2u * kg;
                const uint64_t m0 = tt < kcur ? ~0ull : 0, m1 = tt + 1u < kcur ? ~0ull : 0;
                const uint64_t r0 = __builtin_bswap64(mm_digits(aw[0] & (av ? m0 : 0))), r1 = __builtin_bswap64(mm_digits(aw[1] & (av ? m1 : 0)));
                const uint32_t rx[4] = { (uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32) };
                mm_v4i bop[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                {
                    const uint64_t d0 = mm_digits(bw[t][0] & (bv[t] ? m0 : 0)), d1 = mm_digits(bw[t][1] & (bv[t] ? m1 : 0));
                    bop[t] = mm_v4i{ (int)(uint32_t)d0, (int)(uint32_t)(d0 >> 32), (int)(uint32_t)d1, (int)(uint32_t)(d1 >> 32) };
                }
                load(s + 1u); // the next step's words (a step past the end reads the last term again and is not used)
#pragma unroll
                for (int d = 0; d < ND; ++d)
                {
                    int a0, a1, a2, a3;
                    mm_diag(d, rx[0], rx[1], a0, a1);
                    mm_diag(d, rx[2], rx[3], a2, a3);
                    const mm_v4i aop = { a0, a1, a2, a3 };
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                    {
                        acc[d][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aop, bop[t], acc[d][t], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
            {
                uint32_t u[3][ND];
#pragma unroll
                for (int d = 0; d < ND; ++d)
                {
                    const mm_v4i x = acc[d][t];
                    // the neighbour's half of the lane's middle term: an even lane sends v = 3 and receives v = 0, an odd one the reverse
                    const int got = __builtin_amdgcn_update_dpp(0, odd ? x[0] : x[3], 0xB1, 0xF, 0xF, false);
                    u[0][d] = (uint32_t)(odd ? x[1] : x[0]) ^ 0x80000000u;
                    u[1][d] = (uint32_t)(odd ? x[3] : x[2]) ^ 0x80000000u;
                    u[2][d] = (uint32_t)((odd ? x[2] : x[1]) + got) ^ 0x80000000u;
                }
                const uint32_t j = j0 + 8u * t + (l16 >> 1);
#pragma unroll
                for (int e = 0; e < 3; ++e)
                {
                    const uint64_t v = submod(mm_recombine<ND>(u[e], q, cr0, cr1, t64), bias, q);
                    if (!(cc & 1u))
                    {
                        prev[t][e] = v;
                    }
                    else if (j < g.nb && oi[e] < g.m)
                    {
                        ulonglong2 *o = chunks(g.out + ((((size_t)j * g.m + oi[e]) * 3 + oc[e]) * g.L + r) * n + n0 + c - 1u);
                        ulonglong2 w = make_ulonglong2(prev[t][e], v);
                        if (t0)
                        {
                            w = add2(w, *o, q);
                        }
                        *o = w;
                    }
                }
            }
        }
    }
}

// blockIdx.y = prime; blockIdx.x = (block of 16 coefficients * N groups + N group) * M tiles + M tile: the M tiles that read the
// same rows of b are neighbours in launch order.  N is a power of two of at least 16 (the entry point keeps smaller rings on
// ct_dot_kernel), so a block is whole.  An N group that nb cuts down to one tile runs the one-tile form.
__global__ __launch_bounds__(256, 2) void ct_ct_matmul_mfma_kernel(CtCtArgs g)
{
    __shared__ uint64_t lds[CC_LDS_WORDS];
    const uint32_t mt = blockIdx.x % g.mtiles, rest = blockIdx.x / g.mtiles;
    const uint32_t i0 = 8u * mt, j0 = 8u * CC_NT * (rest % g.ngroups), n0 = 16u * (rest / g.ngroups);
    const uint32_t ar = 2u * (g.m - i0 < 8u ? g.m - i0 : 8u), br = 2u * (g.nb - j0 < 8u * CC_NT ? g.nb - j0 : 8u * CC_NT);
    const bool d7 = g.pc[blockIdx.y].q <= MM_DIGITS7_MAX;
    if (br > 16u)
    {
        d7 ? cc_block<13, CC_NT>(g, lds, i0, j0, n0, ar, br) : cc_block<15, CC_NT>(g, lds, i0, j0, n0, ar, br);
    }
    else
    {
        d7 ? cc_block<13, 1>(g, lds, i0, j0, n0, ar, br) : cc_block<15, 1>(g, lds, i0, j0, n0, ar, br);
    }
}

} // namespace moai
