// ctdot_galois.hip.h -- moai_ct_dot_galois: the sums of ciphertext x ciphertext products over one operand list and its Galois
// images, before any key switch, included by elementwise.hip.  For output j with element e_j and permutation table_j
// (galois_table: what moai_galois_permute reads), per prime and coefficient i:
//     A0 = sum_t x[t][0][i] w[t][0][table_j[i]]     A1 = sum_t x[t][1][i] w[t][0][table_j[i]]
//     B0 = sum_t x[t][0][i] w[t][1][table_j[i]]     B1 = sum_t x[t][1][i] w[t][1][table_j[i]]          mod q, canonical.
// (pi(w0), pi(w1)) encrypts pi(m_W) under pi(s) with no key switch, so (A0, A1) is the part of sum_t X[t] pi(W[t]) that is
// already under s and (B0, B1) the part that still carries a factor pi(s): moai_galois_fold switches those two, twice per
// output instead of once per term (include/moai_hip.h).
//
// Work split.  A thread owns ONE coefficient of one prime row for a group of G outputs: 4 G sums of 128 bits (four registers
// each) that stay in registers over all terms.  Per term it loads its two words of x[t] once for the whole group and, per
// output, the two words of w[t] at that output's permuted index: four 64 x 64 -> 128-bit products per output and term.  An
// x word is read once per group of outputs.  G = 12 staged (192 registers of sums, 234 in all) and G = 8 gather (202: its
// 64-bit addresses cost what four more outputs would): two waves per SIMD, no scratch, profiles/ctdot_galois_isa.txt.
// The outputs of a group need not be neighbours (oi[]), so the host groups by form.
// Permuted index.  It does not depend on the term: src[j] = table_j[i] is loaded once, G registers.
// Where w comes from.
//   STAGED  In bit-reversed order the NTT-form automorphism is i' -> e i' + (e - 1) / 2 mod N (galois_table_kernel:
//           table[i] = brev(e brev(i) + (e - 1) / 2)).  For e = 1 mod 2^k the low k - 1 bits of i' are fixed, so in natural
//           order the permutation stays inside aligned blocks of N / 2^(k-1) coefficients.  MOAI's steps are multiples of a
//           power of two (5^(i num_batch): 5^256 = 1 mod 2^10), and where that block is at most CDG_BLOCK = 256
//           coefficients the workgroup's 256 outputs coefficients read only the same 256 coefficients of w: per term the
//           workgroup stages them for both components with one coalesced 16-byte load per thread (4 KiB) and every output
//           reads its permuted words from LDS.  Two buffers: term t + 1 is loaded into registers before the products of
//           term t and stored after them, one barrier per term (a buffer is written one barrier after its last reader).
//   gather  Any other element (step 1, the conjugation 2N - 1), and any ring smaller than a block: the words come from
//           global memory at src[j], 8 bytes each.  No LDS, no barrier, idle threads return at once.
//   Both forms add the same integers, so they give the same bits.
// Reduction.  A product of canonical residues is below 2^122; the sums are folded (barrett128) every CDG_FOLD = 32 terms:
// 32 products on a canonical residue stay below 2^127 + 2^61.  The fold makes the number of terms free of the
// accumulators' width; CDG_MAX_TERMS is what the 32-bit term counter and the entry point's size checks are written for.
// Bounds.  i < N per thread (STAGED: N is a multiple of 256, every thread is live and reaches every barrier); a table entry
// is below N, its low eight bits below the staged block; j < gcount selects the outputs that exist (uniform branches: the
// tables and indices are kernel arguments); every offset is formed in size_t.
#pragma once
#include "modarith.hip.h"

namespace moai {

constexpr int CDG_G = 12;            // outputs per group, staged form
constexpr int CDG_G_GATHER = 8;      // ... gather form: twelve 64-bit addresses on top of the sums do not fit two waves
constexpr uint32_t CDG_BLOCK = 256;  // coefficients per workgroup, and the block of w a workgroup stages
constexpr uint32_t CDG_FOLD = 32;    // terms between two folds of the 128-bit sums
constexpr size_t CDG_MAX_TERMS = 65536;
static_assert((CDG_FOLD & (CDG_FOLD - 1)) == 0 && CDG_FOLD <= 32, "32 products below 2^122 on a residue below 2^61 fit 128 bits");

struct CtDotGaloisArgs
{
    const uint64_t *x;  // [terms][2][L][N]
    const uint64_t *w;  // [terms][2][L][N]
    uint64_t *out;      // output oi[j] = out + oi[j] * 4 * L * N, [4][L][N]
    const PrimeConst *pc;
    uint32_t L, n2, terms, gcount;
    const uint32_t *table[CDG_G]; // galois_table of the group's elements
    uint32_t oi[CDG_G];
};

template <int G, bool STAGED>
__global__ __launch_bounds__(256, 2) void ct_dot_galois_kernel(CtDotGaloisArgs g)
{
    static_assert(G <= CDG_G, "the tables of a group are CDG_G kernel arguments");
    __shared__ ulonglong2 stage[STAGED ? 2 * CDG_BLOCK : 1]; // [buffer][component][CDG_BLOCK / 2 chunks]
    const uint32_t prime = blockIdx.y;
    const PrimeConst *pc = g.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n = 2 * (size_t)g.n2;
    const size_t i = (size_t)blockIdx.x * CDG_BLOCK + threadIdx.x;
    if (!STAGED && i >= n)
    {
        return;
    }
    const size_t row = (size_t)g.L * n; // a polynomial
    const size_t ct = 2 * row;          // a term
    const uint64_t *__restrict__ xb = g.x + (size_t)prime * n + i;
    const uint64_t *__restrict__ wb = g.w + (size_t)prime * n;
    uint32_t src[G];
#pragma unroll
    for (int j = 0; j < G; ++j)
    {
        src[j] = 0;
        if ((uint32_t)j < g.gcount) // uniform
        {
            src[j] = STAGED ? g.table[j][i] & (CDG_BLOCK - 1u) : g.table[j][i];
        }
    }
    // component c of the staged block: chunk (thread & 127) of w[t][c][prime][block]
    const uint32_t comp = threadIdx.x >> 7, ch = threadIdx.x & 127u;
    const ulonglong2 *__restrict__ ws = nullptr;
    ulonglong2 next = {};
    if constexpr (STAGED)
    {
        ws = reinterpret_cast<const ulonglong2 *>(wb + (size_t)comp * row + (size_t)blockIdx.x * CDG_BLOCK) + ch;
        stage[comp * (CDG_BLOCK / 2) + ch] = ws[0];
        __syncthreads();
    }
    uint64_t lo[G][4] = {}, hi[G][4] = {};
    for (uint32_t t = 0; t < g.terms; ++t)
    {
        const bool more = t + 1 < g.terms; // uniform
        if constexpr (STAGED)
        {
            if (more)
            {
                next = ws[(size_t)(t + 1) * row]; // `ct` words = `row` chunks
            }
        }
        const uint64_t x0 = xb[(size_t)t * ct], x1 = xb[(size_t)t * ct + row];
        const uint64_t *buf = reinterpret_cast<const uint64_t *>(stage) + (t & 1u) * 2u * CDG_BLOCK;
        const uint64_t *wt = wb + (size_t)t * ct;
#pragma unroll
        for (int j = 0; j < G; ++j)
        {
            if ((uint32_t)j < g.gcount)
            {
                const uint64_t w0 = STAGED ? buf[src[j]] : wt[src[j]];
                const uint64_t w1 = STAGED ? buf[CDG_BLOCK + src[j]] : wt[row + src[j]];
                mac128(lo[j][0], hi[j][0], x0, w0);
                mac128(lo[j][1], hi[j][1], x1, w0);
                mac128(lo[j][2], hi[j][2], x0, w1);
                mac128(lo[j][3], hi[j][3], x1, w1);
            }
        }
        if ((t & (CDG_FOLD - 1u)) == CDG_FOLD - 1u)
        {
#pragma unroll
            for (int j = 0; j < G; ++j)
            {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                {
                    lo[j][k] = barrett128(lo[j][k], hi[j][k], q, cr0, cr1);
                    hi[j][k] = 0;
                }
            }
        }
        if constexpr (STAGED)
        {
            if (more)
            {
                stage[((t + 1u) & 1u) * CDG_BLOCK + comp * (CDG_BLOCK / 2) + ch] = next;
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < G; ++j)
    {
        if ((uint32_t)j < g.gcount)
        {
            uint64_t *ob = g.out + (size_t)g.oi[j] * 4 * row + (size_t)prime * n + i;
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                ob[(size_t)k * row] = barrett128(lo[j][k], hi[j][k], q, cr0, cr1);
            }
        }
    }
}

} // namespace moai
