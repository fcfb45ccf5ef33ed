// ctpt_many.hip.h -- moai_ct_pt_dot_many: every giant-step sum of a baby-step / giant-step transform in one pass over the
// baby-step ciphertexts, included by elementwise.hip.  The same canonical residues as one ct_pt_dot_kernel launch per output:
//     out[g][poly] = sum_t x[xi[g][t]][poly] (.) p[pi[g][t]] mod q          per prime and coefficient.
//
// Form.  Per prime and coefficient the call is a dense product of an (outputs x operands) matrix of plaintext values by an
// (operands x polynomials) matrix of ciphertext values.  It runs on the integer units, not on the int8 matrix cores: the
// transforms of the bootstrap have R = 4 or 7 baby steps (moai_bootstrap_lt.h, N = 2^16: 8 giant steps x 4 and 9 x 7), so a
// 16 x 16 x 64 tile would hold ONE K-step (8 terms x 8 digits, half of it zero at R = 4) under 13 or 15 diagonals and pay one
// recombination (about 290 or 315 instructions in ct_ct_matmul_mfma_kernel, profiles/ctct_mfma_isa.txt) per output element
// for at most seven products, where the lazy 128-bit sum pays a 64 x 64 -> 128-bit product and a 128-bit addition per term and
// one barrett128 per output element.  DESIGN 5.0y has the two estimates side by side.
// Columns.  The host turns the index lists of a group of outputs into at most CPM_COLS columns: column c is one operand xi[c],
// a mask of the outputs of the group that have a term with it, and for those outputs the plaintext pi[c][j].  An output that
// lacks an operand another one has skips the column (a zero weight; the branch is uniform, the tables are kernel arguments
// read by scalar loads); an output that names an operand twice takes two columns.  A column adds at most one product to a
// sum, so the sums are folded every 32 columns as ct_pt_dot_kernel folds every 32 terms: 32 products below 2^122 on a
// canonical residue stay below 2^128.
// Work split.  A thread owns ONE coefficient of P polynomials and G outputs: G * P sums of 128 bits (4 registers each),
// <8, 4> = 128 and <12, 3> = 144 registers of sums.  Per column it loads P operand words and up to G plaintext words and
// multiplies each operand word, held in registers, into the sums of the outputs of the mask.  An operand word is read once
// per call (once per group when the call has more than CPM_G outputs), a plaintext word once per group of P polynomials:
// blockIdx.x = block of 256 coefficients * polynomial groups + polynomial group, so the workgroups that read the same
// plaintext words are neighbours in launch order and find them in cache.  No LDS: no value is shared between threads.
// Bounds.  i < N checked per thread; poly0 + k < n_poly selects zero operands and skips the store; output j < gcount (the
// mask never names another).  Indices are below 2^16 (checked by the entry point), every offset is formed in size_t.
#pragma once
#include "modarith.hip.h"

namespace moai {

constexpr int CPM_G = 12;     // outputs per group (the larger kernel)
constexpr int CPM_COLS = 64;  // columns per group: one output of CTPT_MAX_TERMS terms always fits
static_assert(CPM_COLS >= 64 && CPM_G <= 16, "a single output of 64 terms is one group; the mask is 16 bits");

struct CtPtManyArgs
{
    const uint64_t *x;   // operand k = x + k * n_poly * L * N
    const uint64_t *p;   // [n_pt][L][N]
    uint64_t *out;       // output j of the group = out + j * out_stride, [n_poly][L][N]
    size_t out_stride;   // words
    const PrimeConst *pc;
    uint32_t L, n2, n_poly, pgroups, cols, gcount;
    uint32_t xi[CPM_COLS];
    uint16_t mask[CPM_COLS];
    uint16_t pi[CPM_COLS][CPM_G];
};

template <int G, int P>
__global__ __launch_bounds__(256) void ct_pt_dot_many_kernel(CtPtManyArgs g)
{
    static_assert(G <= CPM_G, "the plaintext table has CPM_G entries per column");
    const uint32_t prime = blockIdx.y;
    const uint32_t poly0 = (blockIdx.x % g.pgroups) * P;
    const uint32_t np = g.n_poly - poly0 < (uint32_t)P ? g.n_poly - poly0 : (uint32_t)P; // uniform over the block
    const PrimeConst *pc = g.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n = 2 * (size_t)g.n2;
    const size_t i = (size_t)(blockIdx.x / g.pgroups) * 256u + threadIdx.x;
    if (i >= n)
    {
        return;
    }
    const size_t row = (size_t)g.L * n; // a polynomial of an operand or an output, and a plaintext
    const size_t op_stride = (size_t)g.n_poly * row;
    const size_t at = ((size_t)poly0 * g.L + prime) * n + i;
    const uint64_t *__restrict__ xb = g.x + at;
    const uint64_t *__restrict__ pb = g.p + (size_t)prime * n + i;
    uint64_t lo[G][P] = {}, hi[G][P] = {};
    for (uint32_t c = 0; c < g.cols; ++c)
    {
        const uint32_t m = g.mask[c];
        const uint64_t *xt = xb + (size_t)g.xi[c] * op_stride;
        uint64_t a[P], w[G];
#pragma unroll
        for (int k = 0; k < P; ++k)
        {
            a[k] = (uint32_t)k < np ? xt[(size_t)k * row] : 0;
        }
#pragma unroll
        for (int j = 0; j < G; ++j)
        {
            w[j] = 0;
            if (m >> j & 1u) // uniform
            {
                w[j] = pb[(size_t)g.pi[c][j] * row];
            }
        }
#pragma unroll
        for (int j = 0; j < G; ++j)
        {
            if (m >> j & 1u)
            {
#pragma unroll
                for (int k = 0; k < P; ++k)
                {
                    mac128(lo[j][k], hi[j][k], a[k], w[j]);
                }
            }
        }
        if ((c & 31u) == 31u)
        {
#pragma unroll
            for (int j = 0; j < G; ++j)
            {
#pragma unroll
                for (int k = 0; k < P; ++k)
                {
                    lo[j][k] = barrett128(lo[j][k], hi[j][k], q, cr0, cr1);
                    hi[j][k] = 0;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < G; ++j)
    {
        if ((uint32_t)j < g.gcount)
        {
            uint64_t *ob = g.out + (size_t)j * g.out_stride + at;
#pragma unroll
            for (int k = 0; k < P; ++k)
            {
                if ((uint32_t)k < np)
                {
                    ob[(size_t)k * row] = barrett128(lo[j][k], hi[j][k], q, cr0, cr1);
                }
            }
        }
    }
}

} // namespace moai
