// matmul_mfma.hip.h -- moai_ct_pt_matmul on the int8 matrix cores (MOAI_MATMUL_MFMA=1), included by elementwise.hip after
// MatmulArgs.  The same canonical residues as ct_pt_matmul_kernel and ct_pt_matmul_fp_kernel:
//     out[c][n] = sum_j W[j][c] * X[j][n] mod q          per polynomial, prime and coefficient n.
//
// Limbs.  Every residue v < q < 2^61 has one balanced radix-256 form v = sum_{a<8} v_a 2^(8a), v_a in [-128, 127].  With
// C = 0x8080808080808080 the bytes of v + C are v_a + 128 in [0, 255] (no wrap: v + C < 2^61 + 2^63.01 < 2^64, moai_ctx_create
// refuses primes of 2^61 and above), and flipping bit 7 of a byte b = v_a + 128 makes it the two's-complement int8 v_a.  So the
// bytes of (v + C) ^ C are the digits (mm_digits).  Digit 7 is zero for v < 127 (2^56 - 1) / 255 (the largest value of seven
// digits), which is above 2^54: a prime q <= 2^54 needs 7 digits, any other 8.
// Diagonals.  sum_j w x = sum_d T_d 2^(8d) with T_d = sum_j sum_a w_a[j] x_(d-a)[j], d < ND = 15 (8 digits) or 13 (7 digits).
// One v_mfma_i32_16x16x64_i8 multiplies a 16 x 64 by a 64 x 16 int8 matrix exactly into int32.  Its K = 64 is 8 rows j x 8 digit
// slots a: the M index is the output column c, the N index the coefficient n.  A lane's 16 A bytes are the digit words of W for
// two rows (lane / 16 selects which two), and its 16 B bytes for diagonal d hold x_(d-a) in slot a: with R the byte-reversed
// digit word of x (byte t of R = x_(7-t)) that is R >> 8 (7 - d) for d <= 7 and R << 8 (d - 7) above, zeros shifted in where
// d - a leaves 0..7.  A and B share the lane -> k mapping of the instruction, so which (row, digit) sits at which k does not
// matter; of the C tile, lane l register v holds column 4 (l / 16) + v and coefficient l % 16.
// int32.  |w_a x_b| <= 2^14 and a diagonal sums at most 8 digit pairs per row: |T_d| <= rows * 8 * 2^14.  A K-chunk of
// MM_KC = 8192 rows keeps |T_d| <= 2^30 < 2^31 (16383 rows would still fit, 16384 would not); every chunk is reduced to a
// canonical residue and the chunks are added mod q.
// Recombination, once per output element and chunk (mm_recombine).  u_d = T_d + 2^31 in [0, 2^32) (bit 31 flipped), so
// V' = sum_d u_d 2^(8d) = V + 2^31 sum_d 2^(8d) is non-negative; the same function applied to u_d = 2^31 gives the offset mod q,
// which is subtracted mod q.  Four diagonals at a time: s_i = sum_{e<4} u_(4i+e) 2^(8e) < 2^32 (1 + 2^8 + 2^16 + 2^24) < 2^57;
// Lo = s_0 + s_1 2^32 and Hi = s_2 + s_3 2^32 are below 2^57 + 2^89 < 2^90, V' = Lo + Hi 2^64.  Hi mod q < 2^61 times
// 2^64 mod q < 2^61 is below 2^122, plus Lo below 2^123: inside barrett128's range, whose result is canonical.
#pragma once
#include "modarith.hip.h"

namespace moai {

typedef int mm_v4i __attribute__((ext_vector_type(4)));

constexpr int MM_CT = 2;           // column tiles of 16 per wave: ND * 4 * MM_CT accumulator registers
constexpr uint32_t MM_KC = 8192;   // rows per K-chunk
constexpr uint64_t MM_DIGITS7_MAX = 1ull << 54; // q <= this: 7 digits, 13 diagonals
static_assert(MM_KC % 8 == 0 && (uint64_t)MM_KC * 8 * (1u << 14) < (1ull << 31), "a K-chunk's diagonals fit int32");
static_assert(MM_DIGITS7_MAX <= 127 * ((1ull << 56) - 1) / 255, "seven digits hold every residue of such a prime");

__device__ __forceinline__ uint64_t mm_digits(uint64_t v)
{
    constexpr uint64_t C = 0x8080808080808080ull;
    return (v + C) ^ C;
}

// B operand words of diagonal D from the byte-reversed digit word (hi:lo): the 64-bit shift by whole bytes, written in 32-bit
// operations (v_alignbyte_b32 and 32-bit shifts run at full rate, the 64-bit shifts do not)
__device__ __forceinline__ void mm_diag(const int d, uint32_t lo, uint32_t hi, int &olo, int &ohi)
{
    // d is a constant once the caller's loop is unrolled
    if (d <= 7)
    {
        const int m = 7 - d; // right by m bytes
        olo = (int)(m == 0 ? lo : m < 4 ? __builtin_amdgcn_alignbyte(hi, lo, m) : hi >> (8 * (m - 4)));
        ohi = (int)(m < 4 ? hi >> (8 * m) : 0u);
    }
    else
    {
        const int m = d - 7; // left by m bytes
        ohi = (int)(m < 4 ? __builtin_amdgcn_alignbyte(hi, lo, 4 - m) : lo << (8 * (m - 4)));
        olo = (int)(m < 4 ? lo << (8 * m) : 0u);
    }
}

// sum_d u[d] 2^(8d) mod q, canonical, for u[d] < 2^32; t64 = 2^64 mod q.  Bounds in the head of this file.
template <int ND>
__device__ __forceinline__ uint64_t mm_recombine(const uint32_t (&u)[ND], uint64_t q, uint64_t cr0, uint64_t cr1, uint64_t t64)
{
    uint64_t s[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int d = 0; d < ND; ++d)
    {
        s[d >> 2] += (uint64_t)u[d] << (8 * (d & 3));
    }
    uint64_t l0 = s[0] + (s[1] << 32);
    uint64_t l1 = (s[1] >> 32) + (l0 < s[0] ? 1 : 0);
    const uint64_t h0 = s[2] + (s[3] << 32);
    const uint64_t h1 = (s[3] >> 32) + (h0 < s[2] ? 1 : 0);
    mac128(l0, l1, barrett128(h0, h1, q, cr0, cr1), t64);
    return barrett128(l0, l1, q, cr0, cr1);
}

// One wave: the 16 coefficients from n0 (lane % 16 selects one) times the CT * 16 columns from c0 (the first of them exists), over
// all rows.
// Per K-step of 8 rows a lane loads two words of X (16 lanes x 8 B: one 128-byte segment per row) and two words of W per column
// tile (16 consecutive columns of a row), issued two steps of matrix work before their use.  The B operand of a
// diagonal is formed once and feeds the CT column tiles.  Rows past the chunk's end and columns past cols are zero operands.
template <int ND, int CT>
__device__ __forceinline__ void mm_mfma_wave(const MatmulArgs &g, const uint32_t n0, const uint32_t c0)
{
    const uint32_t pr = blockIdx.y; // p * L + r
    const uint32_t r = pr % g.L;
    const PrimeConst *pc = g.pc + r;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const uint64_t t64 = barrett128(0, 1, q, cr0, cr1);
    const uint32_t lane = threadIdx.x & 63u, l16 = lane & 15u, kg = lane >> 4;
    const size_t n = 2 * (size_t)g.n2;
    const size_t xstride = (size_t)g.size * g.L * n; // words from row j to row j + 1 of X
    const uint64_t *__restrict__ xb = g.x + (size_t)pr * n + n0 + l16;
    const uint64_t *__restrict__ wb = g.w + (size_t)r * g.rows * g.cols;
    // Rows past the chunk's end and columns past cols load the last valid element instead (no branch, always inside the arrays)
    // and select zero.
    bool colv[CT];
    uint32_t wcol[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
    {
        const uint32_t c = c0 + 16u * t + l16;
        colv[t] = c < g.cols;
        wcol[t] = colv[t] ? c : g.cols - 1;
    }
    uint32_t bias_u[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
    {
        bias_u[d] = 0x80000000u;
    }
    const uint64_t bias = mm_recombine<ND>(bias_u, q, cr0, cr1, t64);

    uint64_t res[CT][4] = {};
    for (uint32_t jb = 0; jb < g.rows; jb += MM_KC)
    {
        const uint32_t je = g.rows - jb < MM_KC ? g.rows : jb + MM_KC;
        mm_v4i acc[ND][CT];
#pragma unroll
        for (int d = 0; d < ND; ++d)
        {
#pragma unroll
            for (int t = 0; t < CT; ++t)
            {
                acc[d][t] = mm_v4i{ 0, 0, 0, 0 };
            }
        }
        // Two K-steps (16 rows) per iteration.  What the loop carries is the formed operands (A words and reversed digit words of X),
        // never a loaded register: an iteration issues the loads of the next 16 rows, runs the 2 * ND * CT MFMAs of its own operands
        // and only then turns what arrived into the next operands, so a load has two steps of matrix work to arrive.  A second step
        // past the chunk's end multiplies zeros.
        uint64_t xv[2][2], wv[2][CT][2];
        mm_v4i a[2][CT];
        uint32_t rx[2][4]; // per step: low and high word of R for the lane's two rows
        auto load = [&](uint32_t j0) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
            {
#pragma unroll
                for (int e = 0; e < 2; ++e)
                {
                    const uint32_t j = j0 + 8u * h + 2u * kg + e;
                    const size_t jc = j < je ? j : g.rows - 1;
                    xv[h][e] = xb[jc * xstride];
#pragma unroll
                    for (int t = 0; t < CT; ++t)
                    {
                        wv[h][t][e] = wb[jc * g.cols + wcol[t]];
                    }
                }
            }
        };
        // what was loaded for a row past the end or a column past cols becomes zero here, where it is used
        auto form = [&](uint32_t j0) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
            {
                const uint32_t j = j0 + 8u * h + 2u * kg;
                const uint64_t m0 = j < je ? ~0ull : 0, m1 = j + 1u < je ? ~0ull : 0;
#pragma unroll
                for (int t = 0; t < CT; ++t)
                {
                    const uint64_t d0 = mm_digits(wv[h][t][0] & (colv[t] ? m0 : 0)), d1 = mm_digits(wv[h][t][1] & (colv[t] ? m1 : 0));
                    a[h][t] = mm_v4i{ (int)(uint32_t)d0, (int)(uint32_t)(d0 >> 32), (int)(uint32_t)d1, (int)(uint32_t)(d1 >> 32) };
                }
                const uint64_t r0 = __builtin_bswap64(mm_digits(xv[h][0] & m0)), r1 = __builtin_bswap64(mm_digits(xv[h][1] & m1));
                rx[h][0] = (uint32_t)r0;
                rx[h][1] = (uint32_t)(r0 >> 32);
                rx[h][2] = (uint32_t)r1;
                rx[h][3] = (uint32_t)(r1 >> 32);
            }
        };
        load(jb);
        form(jb);
        for (uint32_t j0 = jb; j0 < je; j0 += 16)
        {
            load(j0 + 16);
            __builtin_amdgcn_sched_barrier(0); // the loads stay ahead of the matrix work
#pragma unroll
            for (int h = 0; h < 2; ++h)
            {
#pragma unroll
                for (int d = 0; d < ND; ++d)
                {
                    int b0, b1, b2, b3;
                    mm_diag(d, rx[h][0], rx[h][1], b0, b1);
                    mm_diag(d, rx[h][2], rx[h][3], b2, b3);
                    const mm_v4i b = { b0, b1, b2, b3 };
#pragma unroll
                    for (int t = 0; t < CT; ++t)
                    {
                        acc[d][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[h][t], b, acc[d][t], 0, 0, 0);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            form(j0 + 16);
        }
#pragma unroll
        for (int t = 0; t < CT; ++t)
        {
#pragma unroll
            for (int v = 0; v < 4; ++v)
            {
                uint32_t u[ND];
#pragma unroll
                for (int d = 0; d < ND; ++d)
                {
                    u[d] = (uint32_t)acc[d][t][v] ^ 0x80000000u;
                }
                res[t][v] = csub(res[t][v] + submod(mm_recombine<ND>(u, q, cr0, cr1, t64), bias, q), q);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < CT; ++t)
    {
#pragma unroll
        for (int v = 0; v < 4; ++v)
        {
            const uint32_t c = c0 + 16u * t + 4u * kg + v;
            if (c < g.cols)
            {
                g.out[((size_t)c * g.size * g.L + pr) * n + n0 + l16] = res[t][v];
            }
        }
    }
}

// blockIdx.y = p * L + r; blockIdx.x = (block of 64 coefficients) * column groups + column group, so that the workgroups that
// read the same rows of X are neighbours in launch order; each of the four waves owns 16 coefficients.  N is a power of two of
// at least 16 (the launcher keeps smaller rings on the other kernels), so a strip is whole or absent.  A group that cols cuts short
// runs tile by tile, so that no MFMA of the full groups sits behind a branch.
template <int ND, int CT>
__device__ __forceinline__ void mm_mfma_group(const MatmulArgs &g, const uint32_t n0, const uint32_t c0)
{
    if (c0 + 16u * CT <= g.cols)
    {
        mm_mfma_wave<ND, CT>(g, n0, c0);
        return;
    }
    for (uint32_t c = c0; c < g.cols; c += 16u)
    {
        mm_mfma_wave<ND, 1>(g, n0, c);
    }
}

template <int CT>
__global__ __launch_bounds__(256, 2) void ct_pt_matmul_mfma_kernel(MatmulArgs g, uint32_t col_groups)
{
    const uint32_t n0 = ((blockIdx.x / col_groups) * 4u + (threadIdx.x >> 6)) * 16u;
    const uint32_t c0 = (blockIdx.x % col_groups) * (16u * CT);
    if (n0 >= 2u * g.n2)
    {
        return;
    }
    if (g.pc[blockIdx.y % g.L].q <= MM_DIGITS7_MAX)
    {
        mm_mfma_group<13, CT>(g, n0, c0);
    }
    else
    {
        mm_mfma_group<15, CT>(g, n0, c0);
    }
}

} // namespace moai
