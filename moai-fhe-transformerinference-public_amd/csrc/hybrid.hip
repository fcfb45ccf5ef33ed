// hybrid.hip -- hybrid key switching: alpha special primes, digits of alpha data primes.
//
// Reference: Evaluator::switch_key_inplace (SEAL/evaluator.cpp:2724-3020) and KeyGenerator::generate_one_kswitch_key
// (SEAL/keygenerator.cpp:303-336) are exactly the alpha = 1 case of what is computed here; include/moai_hip.h, section
// "hybrid key switching", states the algorithm for any alpha and tests/hybrid_ref.py restates it in integers.
//
// Context primes m_0 .. m_{k-1}: special p_t = m_{k-alpha+t}, P their product; data q_i = m_i, i < k - alpha.  At L data primes
// digit j < beta = ceil(L / alpha) is the rows R_j = [j alpha, min((j+1) alpha, L)), D_j their product.
//
// Structure on the device, unfused, per chunk of the batch (scratch per ciphertext: hy_rows_per_ct rows of N words):
//   t        = INTT(target)                                                     [B][L][N]
//   ext_j    = hy_convert_kernel: digit j from base R_j to every other row      [B][L - |R_j| + alpha][N], then forward NTT
//              (rows of R_j are not converted: the MAC reads the target's own NTT-form rows)
//   acc      = hy_mac_kernel: sum_j ext_j (*) key[j][p][row], 128-bit sums      [B][2][L + alpha][N]
//   x        = INTT(special rows of acc)                                        [2B][alpha][N]
//   conv     = hy_convert_kernel: base {p_t} -> {q_i} with the rounding terms   [2B][L][N], then forward NTT
//   out      = moddown_finalize (keyswitch.hip, the unfused mod-down's last kernel): addend + (acc - conv) P^-1
// Hoisted rotations (R automorphisms of one ciphertext, each with its own key) run t, ext_j and their forward transforms ONCE on
// the unpermuted c1 and replace the MAC by hy_hoisted_mac_kernel, which reads the digits through each rotation's permutation
// table and adds that rotation's correction (hy_hoist_correction_kernel; the header states the identity).
// Plaintext-weighted sums of hoisted rotations keep S_g and an addend per output in the extended basis (hy_hoisted_dot_kernel) and
// take one step 5 per sum; a whole baby-step / giant-step transform (moai_hybrid_bsgs_dot) stops that inner stage before its step 5,
// takes only c1 of every inner sum down (hy_c1_moddown_permute_kernel), and sums the giant steps' digit-key products and the lifted
// inner sums into one accumulator Z over Q P (hy_bsgs_mac_kernel) that takes the one final step 5.
// Relinearize + rescale (moai_relinearize_rescale_hybrid) replaces step 5 and the rescale behind it by ONE mod-down by W = P q_{L-1}:
// row L - 1 of the accumulator is lifted by (P mod q_{L-1}) c_p (hy_lift_last_row_kernel), rows L-1 .. L+alpha-1 are the conversion's
// alpha + 1 sources, and hy_rescale_finalize_kernel carries the two multipliers W^-1 and q_{L-1}^-1; moai_multiply_relin_rescale_hybrid
// forms the three-polynomial product in the chunk's scratch first (hy_ct_product_kernel).
// The list forms (moai_apply_galois_hybrid_ptrs, moai_relinearize_hybrid_ptrs, moai_relinearize_rescale_hybrid_ptrs) gather a pass of
// single ciphertexts, each in its own block, into that same scratch (galois_gather_list) and run the chain above on it; the kernels
// that read a member's key or touch a caller's block (hy_mac_kernel, moddown_finalize, hy_lift_last_row_kernel,
// hy_rescale_finalize_kernel) have a LIST instantiation that takes those pointers from the pass's KsList record.
// Every transform goes through ntt_launch with a RowMap.  The constants of one (L, alpha) live in one device block (HyTable)
// that the context owns.
#include <algorithm>
#include <mutex>
#include <vector>

#include "hostmath.h"
#include "launch.h"
#include "modarith.hip.h"

namespace moai {

// a digit's source rows are held in registers by the conversion kernel; the constants are products of at most this many residues
constexpr uint32_t HY_MAX_ALPHA = 16;

// One fast base conversion: sources r < nsrc under context primes src_prime[r], targets t < ntgt under tgt_prime[t]:
//   y_r = ((x_r + src_pre[r]) mod s_r) * src_inv[r] mod s_r,   out_t = ((sum_r y_r w[t][r]) - tgt_post[t]) mod m_t
// mod-up of digit j: src_pre = tgt_post = 0, src_inv = (D_j / q_r)^-1, w = (D_j / q_r) mod m_t
// mod-down:          src_pre = floor(P / 2) mod p_t, tgt_post = floor(P / 2) mod q_i, src_inv = (P / p_t)^-1, w = (P / p_t) mod q_i
struct alignas(16) HyConv
{
    uint32_t nsrc, ntgt, pad[2];
    uint32_t src_prime[HY_MAX_ALPHA];
    uint32_t tgt_prime[MOAI_MAX_RNS];
    Tw src_inv[HY_MAX_ALPHA];
    uint64_t src_pre[HY_MAX_ALPHA];
    uint64_t tgt_post[MOAI_MAX_RNS];
    uint64_t w[MOAI_MAX_RNS][HY_MAX_ALPHA];
};

// the constants of a switch at (L, alpha): conv[j], j < beta, are the mod-ups and conv[beta] is the mod-down; behind them lie the
// multipliers of the hoisted rotations' correction, [beta][L + alpha] words: |R_j| D_j mod m_row (hy_hoist_mult)
struct alignas(16) HyTable
{
    Tw pinv[MOAI_MAX_RNS]; // P^-1 mod q_i
    HyConv conv[1];
};

// device address arithmetic only
static inline const uint64_t *hy_hoist_mult(const HyTable *tab, size_t beta)
{
    return reinterpret_cast<const uint64_t *>(tab->conv + beta + 1);
}

// (hi * 2^64 + lo) mod q for ANY 128-bit value: barrett128's quotient is short of the true one by at most 2 there, so one more
// conditional subtraction makes the residue canonical (a source residue is below ITS prime, which may be far above the target's)
__device__ __forceinline__ uint64_t hy_mod128(uint64_t lo, uint64_t hi, uint64_t q, uint64_t cr0, uint64_t cr1)
{
    return csub(barrett128(lo, hi, q, cr0, cr1), q);
}

struct HyConvArgs
{
    const uint64_t *src; // polynomial b's source row r at row b * src_stride + src_off + r, coefficient form, canonical
    uint64_t *dst;       // [B][ntgt][N], canonical
    const HyConv *cv;
    const PrimeConst *pc;
    uint32_t src_stride, src_off;
    uint32_t n2;
};

// blockIdx.y = polynomial.  A thread reads the nsrc <= AMAX source residues of its two coefficients once, scales them, and walks
// the target rows: per target nsrc 128-bit multiply-adds (at most 16 products below 2^122) and one reduction.  The constants are
// indexed by uniform values: scalar loads.
template <int AMAX>
__global__ __launch_bounds__(256) void hy_convert_kernel(HyConvArgs g)
{
    const HyConv &cv = *g.cv;
    const uint32_t ns = cv.nsrc, nt = cv.ntgt;
    const size_t n2 = g.n2;
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(g.src) + ((size_t)blockIdx.y * g.src_stride + g.src_off) * n2;
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(g.dst) + (size_t)blockIdx.y * nt * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.n2; j += gridDim.x * 256u)
    {
        ulonglong2 y[AMAX];
#pragma unroll
        for (int r = 0; r < AMAX; ++r)
        {
            y[r] = make_ulonglong2(0, 0);
            if ((uint32_t)r < ns)
            {
                const uint64_t q = g.pc[cv.src_prime[r]].q, pre = cv.src_pre[r];
                const Tw inv = cv.src_inv[r];
                const ulonglong2 v = s[(size_t)r * n2 + j];
                y[r].x = csub(mul_shoup_lazy(csub(v.x + pre, q), inv.w, inv.wq, q), q);
                y[r].y = csub(mul_shoup_lazy(csub(v.y + pre, q), inv.w, inv.wq, q), q);
            }
        }
        for (uint32_t t = 0; t < nt; ++t)
        {
            const PrimeConst *pc = g.pc + cv.tgt_prime[t];
            const uint64_t m = pc->q, cr0 = pc->cr0, cr1 = pc->cr1, post = cv.tgt_post[t];
            uint64_t lx = 0, hx = 0, ly = 0, hy = 0;
#pragma unroll
            for (int r = 0; r < AMAX; ++r)
            {
                if ((uint32_t)r < ns)
                {
                    mac2(lx, hx, ly, hy, y[r], cv.w[t][r]);
                }
            }
            ulonglong2 o;
            o.x = submod(hy_mod128(lx, hx, m, cr0, cr1), post, m);
            o.y = submod(hy_mod128(ly, hy, m, cr0, cr1), post, m);
            d[(size_t)t * n2 + j] = o;
        }
    }
}

// what every kernel below knows of a switch at (L, alpha); hy_dims fills it
struct HyDims
{
    const PrimeConst *pc;
    uint32_t L, alpha, beta, k;
    uint32_t n2;
};

// The operand of digit j under the prime of `row`, for ciphertext b of B, at L data primes in digits of alpha: `own` where the row is
// one of the digit's own primes (the ciphertext's NTT-form row as it is), else the digit's converted row in ext (HyMacArgs::ext, as
// rows of row_elems elements of T)
template <class T>
__device__ __forceinline__ const T *hy_digit_operand(const T *own, const T *ext, size_t row_elems, uint32_t L, uint32_t alpha, uint32_t B,
                                                     uint32_t b, uint32_t row, uint32_t j)
{
    const uint32_t lo = j * alpha, hi = min(lo + alpha, L), nr = hi - lo;
    if (row >= lo && row < hi)
    {
        return own;
    }
    const uint32_t pos = row < lo ? row : row - nr;
    return ext + ((size_t)j * B * L + (size_t)b * (L - nr + alpha) + pos) * row_elems;
}

struct HyMacArgs
{
    const uint64_t *ext;   // digit j's converted rows at ext + j * B * L * N: [B][L - |R_j| + alpha][N], NTT form
    const uint64_t *tgt;   // ciphertext b's NTT-form target row r at row b * tgt_stride + tgt_off + r
    const uint64_t *key;   // [beta(k - alpha)][2][k][N]
    uint64_t *acc;         // [B][2][L + alpha][N]
    uint32_t tgt_stride, tgt_off;
    HyDims d;
};

struct HyMacListArgs : HyMacArgs
{
    const KsList *lst; // ciphertext b's key is lst->keys[b], in the same whole layout (key unused)
};

// acc[b][p][row] = sum_{j < beta} digit_j[row] (*) key[j][p][row]; blockIdx.x = b (the workgroups that read the same key words
// are dispatched together), blockIdx.z = row.  At most 63 products below 2^122 per sum: no fold before the one reduction.
// LIST: every ciphertext of the batch has its own key (KsList).  The ciphertext index is uniform over the workgroup, so the list
// entry arrives through a scalar load; the digits and the accumulators stay in the pass's contiguous scratch.
template <bool LIST = false>
__global__ __launch_bounds__(256) void hy_mac_kernel(std::conditional_t<LIST, HyMacListArgs, HyMacArgs> g)
{
    const HyDims &d = g.d;
    const uint32_t b = blockIdx.x, B = gridDim.x, row = blockIdx.z;
    const uint32_t prime = hy_row_prime(row, d.L, d.alpha, d.k);
    const PrimeConst *pc = d.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    const ulonglong2 *ext = reinterpret_cast<const ulonglong2 *>(g.ext);
    const ulonglong2 *tgt = reinterpret_cast<const ulonglong2 *>(g.tgt) + ((size_t)b * g.tgt_stride + g.tgt_off) * n2;
    const ulonglong2 *key = reinterpret_cast<const ulonglong2 *>(g.key) + (size_t)prime * n2;
    if constexpr (LIST)
    {
        key = reinterpret_cast<const ulonglong2 *>(g.lst->keys[b]) + (size_t)prime * n2;
    }
    ulonglong2 *acc0 = reinterpret_cast<ulonglong2 *>(g.acc) + ((size_t)(b * 2 + 0) * (d.L + d.alpha) + row) * n2;
    ulonglong2 *acc1 = reinterpret_cast<ulonglong2 *>(g.acc) + ((size_t)(b * 2 + 1) * (d.L + d.alpha) + row) * n2;
    for (uint32_t x = blockIdx.y * 256u + threadIdx.x; x < d.n2; x += gridDim.y * 256u)
    {
        uint64_t l0x = 0, h0x = 0, l0y = 0, h0y = 0, l1x = 0, h1x = 0, l1y = 0, h1y = 0;
        for (uint32_t j = 0; j < d.beta; ++j)
        {
            const ulonglong2 *op = hy_digit_operand(tgt + (size_t)row * n2, ext, n2, d.L, d.alpha, B, b, row, j);
            const ulonglong2 o = op[x];
            const ulonglong2 k0 = key[(size_t)(j * 2 + 0) * d.k * n2 + x];
            const ulonglong2 k1 = key[(size_t)(j * 2 + 1) * d.k * n2 + x];
            mac2(l0x, h0x, l0y, h0y, o, k0);
            mac2(l1x, h1x, l1y, h1y, o, k1);
        }
        acc0[x] = reduce2(l0x, h0x, l0y, h0y, q, cr0, cr1);
        acc1[x] = reduce2(l1x, h1x, l1y, h1y, q, cr0, cr1);
    }
}

struct HyCorrArgs
{
    const uint64_t *key;  // [beta(k - alpha)][2][k][N]
    const uint64_t *mask; // [L + alpha][N]: NTT of the rotation's sign mask under each row's prime
    const uint64_t *mult; // [beta][L + alpha]: |R_j| D_j mod m_row
    uint64_t *out;        // [2][L + alpha][N]
    HyDims d;
};

// out[p][row] = mask[row] (*) sum_{j < beta} mult[j][row] key[j][p][row]; blockIdx.y = p * (L + alpha) + row.  At most 63 products
// below 2^122.  A multiplier of zero (the rows of R_j itself, D_j mod q_r = 0) is skipped: the branch is uniform.
__global__ __launch_bounds__(256) void hy_hoist_correction_kernel(HyCorrArgs g)
{
    const HyDims &d = g.d;
    const uint32_t rows = d.L + d.alpha, p = blockIdx.y / rows, row = blockIdx.y % rows;
    const uint32_t prime = hy_row_prime(row, d.L, d.alpha, d.k);
    const PrimeConst *pc = d.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    const ulonglong2 *key = reinterpret_cast<const ulonglong2 *>(g.key) + ((size_t)p * d.k + prime) * n2;
    const ulonglong2 *mk = reinterpret_cast<const ulonglong2 *>(g.mask) + (size_t)row * n2;
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(g.out) + (size_t)blockIdx.y * n2;
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < d.n2; x += gridDim.x * 256u)
    {
        uint64_t lx = 0, hx = 0, ly = 0, hy = 0;
        for (uint32_t j = 0; j < d.beta; ++j)
        {
            const uint64_t f = g.mult[j * rows + row];
            if (f)
            {
                mac2(lx, hx, ly, hy, key[(size_t)j * 2 * d.k * n2 + x], f);
            }
        }
        o[x] = mulmod2(reduce2(lx, hx, ly, hy, q, cr0, cr1), mk[x], q, cr0, cr1);
    }
}

constexpr int HY_HOIST_MAX_NR = 4;

struct HyHoistMacArgs
{
    const uint64_t *ext; // as HyMacArgs: the digits of the UNPERMUTED c1
    const uint64_t *in;  // the unpermuted input [B][2][L][N]: its c1 row r is the digit under prime r
    const uint32_t *table[HY_HOIST_MAX_NR]; // per rotation: its NTT-form index permutation (galois_table), out[i] = in[table[i]]
    const uint64_t *key[HY_HOIST_MAX_NR];   // its key [beta(k - alpha)][2][k][N]
    const uint64_t *corr[HY_HOIST_MAX_NR];  // its correction [2][L + alpha][N]
    uint64_t *acc[HY_HOIST_MAX_NR];         // its accumulators [B][2][L + alpha][N]
    HyDims d;
};

// acc_r[b][p][row] = sum_{j < beta} digit_j[row][table_r] (*) key_r[j][p][row] + corr_r[p][row] for NR rotations in one pass over
// the digits; grid as hy_mac_kernel (blockIdx.x = b, blockIdx.z = row).  A thread owns two neighbouring OUTPUT positions: the key,
// the correction and the accumulators are read and written in order, two words per lane, and only the digit is gathered (beta of
// the 3 beta + 4 words per output).  Per digit every load of every rotation is issued before the arithmetic.  Sums as in
// hy_mac_kernel: at most 63 products below 2^122, one reduction, then the canonical add of the correction.
template <int NR>
__global__ __launch_bounds__(256) void hy_hoisted_mac_kernel(HyHoistMacArgs g)
{
    const HyDims &d = g.d;
    const uint32_t b = blockIdx.x, B = gridDim.x, row = blockIdx.z;
    const uint32_t prime = hy_row_prime(row, d.L, d.alpha, d.k);
    const PrimeConst *pc = d.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    const uint64_t *own = g.in + ((size_t)(b * 2 + 1) * d.L + row) * 2 * n2; // read only where row < L
    const size_t acc_row = ((size_t)b * 2 * (d.L + d.alpha) + row) * n2, acc_poly = (size_t)(d.L + d.alpha) * n2;
    for (uint32_t x = blockIdx.y * 256u + threadIdx.x; x < d.n2; x += gridDim.y * 256u)
    {
        uint2 src[NR];
        uint64_t l0x[NR], h0x[NR], l0y[NR], h0y[NR], l1x[NR], h1x[NR], l1y[NR], h1y[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r)
        {
            src[r] = reinterpret_cast<const uint2 *>(g.table[r])[x];
            l0x[r] = h0x[r] = l0y[r] = h0y[r] = l1x[r] = h1x[r] = l1y[r] = h1y[r] = 0;
        }
        for (uint32_t j = 0; j < d.beta; ++j)
        {
            // the digit under one of its own primes is the input's c1 row, read through the same permutation
            const uint64_t *op = hy_digit_operand(own, g.ext, 2 * n2, d.L, d.alpha, B, b, row, j);
            const size_t koff = ((size_t)j * 2 * d.k + prime) * n2 + x;
            ulonglong2 o[NR], k0[NR], k1[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r)
            {
                const ulonglong2 *key = reinterpret_cast<const ulonglong2 *>(g.key[r]);
                o[r] = make_ulonglong2(op[src[r].x], op[src[r].y]);
                k0[r] = key[koff];
                k1[r] = key[koff + (size_t)d.k * n2];
            }
#pragma unroll
            for (int r = 0; r < NR; ++r)
            {
                mac2(l0x[r], h0x[r], l0y[r], h0y[r], o[r], k0[r]);
                mac2(l1x[r], h1x[r], l1y[r], h1y[r], o[r], k1[r]);
            }
        }
        ulonglong2 c0[NR], c1[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r)
        {
            const ulonglong2 *corr = reinterpret_cast<const ulonglong2 *>(g.corr[r]) + (size_t)row * n2 + x;
            c0[r] = corr[0];
            c1[r] = corr[acc_poly];
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
        {
            ulonglong2 *acc = reinterpret_cast<ulonglong2 *>(g.acc[r]) + acc_row + x;
            acc[0] = add2(reduce2(l0x[r], h0x[r], l0y[r], h0y[r], q, cr0, cr1), c0[r], q);
            acc[acc_poly] = add2(reduce2(l1x[r], h1x[r], l1y[r], h1y[r], q, cr0, cr1), c1[r], q);
        }
    }
}

// ---- plaintext-weighted sums of rotations (moai_hybrid_rotate_pt_dot) ---------------------------------------------------------
// outputs in flight per launch: their plaintext pointers travel as kernel arguments
constexpr int HY_DOT_MAX_NG = 16;

struct HyDotOutputs
{
    uint64_t *S;     // output h's extended-basis sums at S + h * B * 2 * (L + alpha) * N: [B][2][L + alpha][N], canonical
    uint64_t *add;   // its addend at add + h * B * 2 * L * N: [B][2][L][N], canonical, always read-modified-written
    uint32_t ng;     // outputs of this launch
    uint32_t seeded; // bit h: S of output h already holds a sum; clear: this launch's products start it
    const uint64_t *plain[HY_DOT_MAX_NG][HY_HOIST_MAX_NR]; // p_{g,r} [L + alpha][N] of output h and rotation r of the pass; null: absent
};

// hy_hoisted_mac_kernel's sums for one thread at output chunk x, kept in registers: a0[r], a1[r] = the canonical acc_r[b][0][row] and
// acc_r[b][1][row], correction included, and src[r] = the two source positions of rotation r.  The same loads in the same order and
// the same bound (at most 63 products below 2^122, one reduction, the canonical add of the correction); that kernel keeps its own
// copy of the loop so that its code is what it was.
template <int NR>
__device__ __forceinline__ void hy_hoisted_sums(const HyHoistMacArgs &g, uint32_t b, uint32_t B, uint32_t row, uint32_t prime, uint32_t x,
                                                uint2 (&src)[NR], ulonglong2 (&a0)[NR], ulonglong2 (&a1)[NR])
{
    const HyDims &d = g.d;
    const PrimeConst *pc = d.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    const uint64_t *own = g.in + ((size_t)(b * 2 + 1) * d.L + row) * 2 * n2; // read only where row < L
    const size_t acc_poly = (size_t)(d.L + d.alpha) * n2;
    uint64_t l0x[NR], h0x[NR], l0y[NR], h0y[NR], l1x[NR], h1x[NR], l1y[NR], h1y[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r)
    {
        src[r] = reinterpret_cast<const uint2 *>(g.table[r])[x];
        l0x[r] = h0x[r] = l0y[r] = h0y[r] = l1x[r] = h1x[r] = l1y[r] = h1y[r] = 0;
    }
    for (uint32_t j = 0; j < d.beta; ++j)
    {
        // the digit under one of its own primes is the input's c1 row, read through the same permutation
        const uint64_t *op = hy_digit_operand(own, g.ext, 2 * n2, d.L, d.alpha, B, b, row, j);
        const size_t koff = ((size_t)j * 2 * d.k + prime) * n2 + x;
        ulonglong2 o[NR], k0[NR], k1[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r)
        {
            const ulonglong2 *key = reinterpret_cast<const ulonglong2 *>(g.key[r]);
            o[r] = make_ulonglong2(op[src[r].x], op[src[r].y]);
            k0[r] = key[koff];
            k1[r] = key[koff + (size_t)d.k * n2];
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
        {
            mac2(l0x[r], h0x[r], l0y[r], h0y[r], o[r], k0[r]);
            mac2(l1x[r], h1x[r], l1y[r], h1y[r], o[r], k1[r]);
        }
    }
    ulonglong2 c0[NR], c1[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r)
    {
        const ulonglong2 *corr = reinterpret_cast<const ulonglong2 *>(g.corr[r]) + (size_t)row * n2 + x;
        c0[r] = corr[0];
        c1[r] = corr[acc_poly];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
    {
        a0[r] = add2(reduce2(l0x[r], h0x[r], l0y[r], h0y[r], q, cr0, cr1), c0[r], q);
        a1[r] = add2(reduce2(l1x[r], h1x[r], l1y[r], h1y[r], q, cr0, cr1), c1[r], q);
    }
}

// S_h[b][p][row] += sum_r plain[h][r][row] (*) acc_r[b][p][row] and, on the data rows, add_h[b][0][row] += sum_r plain[h][r][row] (*)
// perm_r(c0)[row], for the NR rotations of one pass of hy_hoisted_sums and every output in flight: the accumulators of a rotation
// never leave the registers.  Grid as hy_hoisted_mac_kernel.  A rotation's sums and its gathered c0 are formed once and reused by
// every output; the plaintext, S and the addend are read and written in order.  Every 128-bit sum here is one canonical residue
// (below 2^61) plus at most NR <= 4 products below 2^122, below 2^125: no fold, one reduction, and the stored value is canonical
// again, so the sum over any number of rotations is carried across passes as residues.  An absent term (a null pointer, uniform)
// multiplies by zero; an output with no term in the pass is skipped, and one whose S no pass has written yet starts from zero.
template <int NR>
__global__ __launch_bounds__(256) void hy_hoisted_dot_kernel(HyHoistMacArgs g, HyDotOutputs o)
{
    const HyDims &d = g.d;
    const uint32_t b = blockIdx.x, B = gridDim.x, row = blockIdx.z;
    const uint32_t prime = hy_row_prime(row, d.L, d.alpha, d.k);
    const PrimeConst *pc = d.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    const size_t s_row = ((size_t)b * 2 * (d.L + d.alpha) + row) * n2, s_poly = (size_t)(d.L + d.alpha) * n2;
    const size_t s_out = (size_t)B * 2 * s_poly, add_out = (size_t)B * 2 * d.L * n2;
    const bool data = row < d.L;
    const uint64_t *c0 = g.in + ((size_t)(b * 2) * d.L + row) * 2 * n2; // read only on the data rows
    const size_t add_row = ((size_t)b * 2 * d.L + row) * n2;
    for (uint32_t x = blockIdx.y * 256u + threadIdx.x; x < d.n2; x += gridDim.y * 256u)
    {
        uint2 src[NR];
        ulonglong2 a0[NR], a1[NR], u[NR];
        hy_hoisted_sums<NR>(g, b, B, row, prime, x, src, a0, a1);
#pragma unroll
        for (int r = 0; r < NR; ++r)
        {
            u[r] = data ? make_ulonglong2(c0[src[r].x], c0[src[r].y]) : make_ulonglong2(0, 0);
        }
        for (uint32_t h = 0; h < o.ng; ++h)
        {
            ulonglong2 p[NR];
            bool any = false;
#pragma unroll
            for (int r = 0; r < NR; ++r)
            {
                p[r] = make_ulonglong2(0, 0);
                if (o.plain[h][r])
                {
                    p[r] = reinterpret_cast<const ulonglong2 *>(o.plain[h][r])[(size_t)row * n2 + x];
                    any = true;
                }
            }
            if (!any)
            {
                continue;
            }
            // every load of this output before its arithmetic; an absent term multiplies by zero
            ulonglong2 *S = reinterpret_cast<ulonglong2 *>(o.S) + h * s_out + s_row + x;
            ulonglong2 *ad = reinterpret_cast<ulonglong2 *>(o.add) + h * add_out + add_row + x; // touched only on the data rows
            const bool seeded = (o.seeded >> h) & 1u;
            const ulonglong2 zero = make_ulonglong2(0, 0);
            const ulonglong2 s0 = seeded ? S[0] : zero, s1 = seeded ? S[s_poly] : zero, ad0 = data ? ad[0] : zero;
            uint64_t l0x, h0x, l0y, h0y, l1x, h1x, l1y, h1y, lux, hux, luy, huy;
            seed2(l0x, h0x, l0y, h0y, s0);
            seed2(l1x, h1x, l1y, h1y, s1);
            seed2(lux, hux, luy, huy, ad0);
#pragma unroll
            for (int r = 0; r < NR; ++r)
            {
                mac2(l0x, h0x, l0y, h0y, a0[r], p[r]);
                mac2(l1x, h1x, l1y, h1y, a1[r], p[r]);
                mac2(lux, hux, luy, huy, u[r], p[r]);
            }
            S[0] = reduce2(l0x, h0x, l0y, h0y, q, cr0, cr1);
            S[s_poly] = reduce2(l1x, h1x, l1y, h1y, q, cr0, cr1);
            if (data)
            {
                ad[0] = reduce2(lux, hux, luy, huy, q, cr0, cr1);
            }
        }
    }
}

struct HyDotTermArgs
{
    const uint64_t *A; // the term's accumulators [B][2][L + alpha][N], canonical; null: an identity term, which has none
    const uint64_t *u; // ciphertext b's rows at u + b * 2 * L * N, [2][L][N]: the permuted input of a rotation, the input itself for
                       // an identity term
    HyDims d;
};

// One term r of the sums, for every output in flight (plain[h][0] = p_{h,r}, null: absent); blockIdx.x = b, .z = row.
//   a rotation (A set, rows of L + alpha):  S_h[b][p][row] += plain (*) A[b][p][row];  add_h[b][0][row] += plain (*) u[b][0][row] on data rows
//   an identity term (A null, rows of L):   add_h[b][p][row] += plain (*) u[b][p][row], p in {0, 1}
// The unhoisted route of a chunk and the identity terms.  addmul2: every product is reduced and added canonically, no 128-bit sum.
__global__ __launch_bounds__(256) void hy_dot_term_kernel(HyDotTermArgs g, HyDotOutputs o)
{
    const HyDims &d = g.d;
    const uint32_t b = blockIdx.x, B = gridDim.x, row = blockIdx.z;
    const uint32_t prime = hy_row_prime(row, d.L, d.alpha, d.k);
    const PrimeConst *pc = d.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    const size_t s_row = ((size_t)b * 2 * (d.L + d.alpha) + row) * n2, s_poly = (size_t)(d.L + d.alpha) * n2;
    const size_t s_out = (size_t)B * 2 * s_poly, add_out = (size_t)B * 2 * d.L * n2;
    const size_t add_row = ((size_t)b * 2 * d.L + row) * n2, add_poly = (size_t)d.L * n2; // the layout of u and of an addend
    const bool data = row < d.L;
    const ulonglong2 *A = reinterpret_cast<const ulonglong2 *>(g.A), *u = reinterpret_cast<const ulonglong2 *>(g.u);
    for (uint32_t x = blockIdx.y * 256u + threadIdx.x; x < d.n2; x += gridDim.y * 256u)
    {
        ulonglong2 a0, a1, u0, u1;
        a0 = a1 = u0 = u1 = make_ulonglong2(0, 0);
        if (A)
        {
            a0 = A[s_row + x];
            a1 = A[s_row + s_poly + x];
        }
        if (data)
        {
            u0 = u[add_row + x];
            if (!A)
            {
                u1 = u[add_row + add_poly + x];
            }
        }
        for (uint32_t h = 0; h < o.ng; ++h)
        {
            if (!o.plain[h][0])
            {
                continue;
            }
            const ulonglong2 p = reinterpret_cast<const ulonglong2 *>(o.plain[h][0])[(size_t)row * n2 + x];
            if (A)
            {
                ulonglong2 *S = reinterpret_cast<ulonglong2 *>(o.S) + h * s_out + s_row + x;
                const bool seeded = (o.seeded >> h) & 1u;
                const ulonglong2 zero = make_ulonglong2(0, 0);
                S[0] = addmul2(seeded ? S[0] : zero, a0, p, q, cr0, cr1);
                S[s_poly] = addmul2(seeded ? S[s_poly] : zero, a1, p, q, cr0, cr1);
            }
            if (data)
            {
                ulonglong2 *ad = reinterpret_cast<ulonglong2 *>(o.add) + h * add_out + add_row + x;
                ad[0] = addmul2(ad[0], u0, p, q, cr0, cr1);
                if (!A)
                {
                    ad[add_poly] = addmul2(ad[add_poly], u1, p, q, cr0, cr1);
                }
            }
        }
    }
}

// ---- giant steps summed in the extended basis (moai_hybrid_bsgs_dot) ------------------------------------------------------------
struct HyC1Args
{
    const uint64_t *S;    // [ng][B][2][L + alpha][N]: polynomial 1 of pair (h, b) is read where h < n_md
    const uint64_t *conv; // [n_md * B][L][N], NTT form: the base conversion of the special rows of S[.][.][1]
    const uint64_t *add;  // [ng][B][2][L][N]: the addends, polynomial 1 read
    uint64_t *tgt;        // [n_rot * B][L][N]
    const uint32_t *table[HY_DOT_MAX_NG]; // giant step h's index permutation, h < n_rot
    const Tw *pinv;       // P^-1 mod q_i
    uint32_t n_md, B;
    HyDims d;
};

// The one-polynomial form of the mod-down's last kernel, with the giant step's permutation applied as it writes: for pair (h, b),
//   c1'[i] = add[h][b][1][i] + (S[h][b][1][i] - conv[h B + b][i]) P^-1 mod q_i   where h < n_md (moddown_finalize_kernel's arithmetic),
//   c1'[i] = add[h][b][1][i]                                                    otherwise (an inner sum without a switched term),
// and tgt[h B + b][i][x] = c1'[i][table_h[x]].  blockIdx.y = (h B + b) L + i.  The target is written in order, two words per lane;
// the two or three sources are gathered.
__global__ __launch_bounds__(256) void hy_c1_moddown_permute_kernel(HyC1Args g)
{
    const HyDims &d = g.d;
    const uint32_t pair = blockIdx.y / d.L, i = blockIdx.y % d.L, h = pair / g.B;
    const uint64_t q = d.pc[i].q;
    const Tw inv = g.pinv[i];
    const size_t n = 2 * (size_t)d.n2;
    const uint64_t *S = g.S + ((size_t)(pair * 2 + 1) * (d.L + d.alpha) + i) * n;
    const uint64_t *u = g.conv + ((size_t)pair * d.L + i) * n;
    const uint64_t *ad = g.add + ((size_t)(pair * 2 + 1) * d.L + i) * n;
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(g.tgt) + (size_t)blockIdx.y * d.n2;
    const uint2 *table = reinterpret_cast<const uint2 *>(g.table[h]);
    const bool md = h < g.n_md;
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < d.n2; x += gridDim.x * 256u)
    {
        const uint2 src = table[x];
        ulonglong2 r = make_ulonglong2(ad[src.x], ad[src.y]);
        if (md)
        {
            ulonglong2 v;
            v.x = csub(mul_shoup_lazy(S[src.x] + q - u[src.x], inv.w, inv.wq, q), q);
            v.y = csub(mul_shoup_lazy(S[src.y] + q - u[src.y], inv.w, inv.wq, q), q);
            r = add2(v, r, q);
        }
        o[x] = r;
    }
}

struct HyBsgsMacArgs
{
    const uint64_t *ext; // as HyMacArgs for the n_rot * B targets: digit j at ext + j * n_rot * B * L * N
    const uint64_t *tgt; // [n_rot * B][L][N]: perm_{E_h}(c1'_h) of pair (h, b) at row block h * B + b
    const uint64_t *S;   // [ng][B][2][L + alpha][N], canonical (zero where the inner sum has no switched term)
    const uint64_t *add; // [ng][B][2][L][N], canonical
    uint64_t *Z;         // [B][2][L + alpha][N]
    const uint32_t *table[HY_DOT_MAX_NG]; // giant step h < n_rot: its index permutation
    const uint64_t *key[HY_DOT_MAX_NG];   // and its key [beta(k - alpha)][2][k][N]
    uint64_t fac[MOAI_MAX_RNS];           // P mod q_i
    uint32_t n_rot, ng;  // giant steps h < n_rot have E_h != 1, n_rot <= h < ng have E_h = 1
    uint32_t zseeded;    // Z holds the sum of the earlier groups; clear: this launch starts it
    HyDims d;
};

// Z[b][p][row] (+)= sum_{h < ng} contribution of giant step h, for the giant steps of one group; grid as hy_mac_kernel (blockIdx.x =
// b, blockIdx.z = row).  With T_h = S_h + (P mod q_row) a_h on the data rows and T_h = S_h on the special rows (the inner sum lifted
// into Q P, nothing rounded):
//   h < n_rot (E_h != 1):  Z[0] += sum_j digit_{h,j}[row] (*) key_h[j][0][row] + T_h[0][row][table_h],   Z[1] += sum_j digit_{h,j}[row]
//                          (*) key_h[j][1][row], the digits those of perm_{E_h}(c1'_h) (steps 1-3 on tgt)
//   h >= n_rot (E_h = 1):  Z[p] += T_h[p][row]
// A thread owns two neighbouring output positions; the digits, the keys and Z are read in order and only T_h[0] of a rotated giant
// step is gathered.  No B_h and no permuted T_h[0] reaches memory, and Z is read (after the first group) and written once.
// 128-bit sums: the running sums z0, z1 are canonical residues (below 2^61).  Per giant step a sum is seeded with one of them and
// takes the beta <= 63 products below 2^122 of the digits: below 2^61 + 63 2^122 < 2^128, one reduction.  The lifted term is then
// one canonical residue (z + S, added canonically) plus ONE product below 2^122, reduced again.  Every giant step leaves canonical
// residues behind, so the sum over any number of giant steps and groups is carried as residues and cannot overflow.
__global__ __launch_bounds__(256) void hy_bsgs_mac_kernel(HyBsgsMacArgs g)
{
    const HyDims &d = g.d;
    const uint32_t b = blockIdx.x, B = gridDim.x, row = blockIdx.z;
    const uint32_t prime = hy_row_prime(row, d.L, d.alpha, d.k);
    const PrimeConst *pc = d.pc + prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    const bool data = row < d.L;
    const uint64_t fac = data ? g.fac[row] : 0;
    const size_t s_row = ((size_t)b * 2 * (d.L + d.alpha) + row) * n2, s_poly = (size_t)(d.L + d.alpha) * n2;
    const size_t s_out = (size_t)B * 2 * s_poly, add_out = (size_t)B * 2 * d.L * n2;
    const size_t add_row = ((size_t)b * 2 * d.L + row) * n2, add_poly = (size_t)d.L * n2; // touched only on the data rows
    const ulonglong2 *ext = reinterpret_cast<const ulonglong2 *>(g.ext);
    const ulonglong2 *S = reinterpret_cast<const ulonglong2 *>(g.S), *ad = reinterpret_cast<const ulonglong2 *>(g.add);
    ulonglong2 *Z = reinterpret_cast<ulonglong2 *>(g.Z) + s_row;
    const ulonglong2 zero = make_ulonglong2(0, 0);
    for (uint32_t x = blockIdx.y * 256u + threadIdx.x; x < d.n2; x += gridDim.y * 256u)
    {
        ulonglong2 z0 = zero, z1 = zero;
        if (g.zseeded)
        {
            z0 = Z[x];
            z1 = Z[s_poly + x];
        }
        for (uint32_t h = 0; h < g.n_rot; ++h)
        {
            const uint32_t pair = h * B + b;
            // the lifted inner sum's polynomial 0, gathered: its loads are issued before the digit loop
            const uint2 src = reinterpret_cast<const uint2 *>(g.table[h])[x];
            const uint64_t *Sh = g.S + 2 * (h * s_out + s_row), *ah = g.add + 2 * (h * add_out + add_row);
            const ulonglong2 t0 = make_ulonglong2(Sh[src.x], Sh[src.y]);
            const ulonglong2 a0 = data ? make_ulonglong2(ah[src.x], ah[src.y]) : zero;
            const ulonglong2 *own = reinterpret_cast<const ulonglong2 *>(g.tgt) + ((size_t)pair * d.L + row) * n2; // read where row < L
            const ulonglong2 *key = reinterpret_cast<const ulonglong2 *>(g.key[h]) + (size_t)prime * n2;
            uint64_t l0x, h0x, l0y, h0y, l1x, h1x, l1y, h1y;
            seed2(l0x, h0x, l0y, h0y, z0);
            seed2(l1x, h1x, l1y, h1y, z1);
            for (uint32_t j = 0; j < d.beta; ++j)
            {
                const ulonglong2 *op = hy_digit_operand(own, ext, n2, d.L, d.alpha, g.n_rot * B, pair, row, j);
                const ulonglong2 o = op[x];
                const ulonglong2 k0 = key[(size_t)(j * 2 + 0) * d.k * n2 + x];
                const ulonglong2 k1 = key[(size_t)(j * 2 + 1) * d.k * n2 + x];
                mac2(l0x, h0x, l0y, h0y, o, k0);
                mac2(l1x, h1x, l1y, h1y, o, k1);
            }
            z1 = reduce2(l1x, h1x, l1y, h1y, q, cr0, cr1);
            seed2(l0x, h0x, l0y, h0y, add2(reduce2(l0x, h0x, l0y, h0y, q, cr0, cr1), t0, q));
            mac2(l0x, h0x, l0y, h0y, a0, fac);
            z0 = reduce2(l0x, h0x, l0y, h0y, q, cr0, cr1);
        }
        for (uint32_t h = g.n_rot; h < g.ng; ++h)
        {
            const ulonglong2 t0 = S[h * s_out + s_row + x], t1 = S[h * s_out + s_row + s_poly + x];
            ulonglong2 a0 = zero, a1 = zero;
            if (data)
            {
                a0 = ad[h * add_out + add_row + x];
                a1 = ad[h * add_out + add_row + add_poly + x];
            }
            uint64_t l0x, h0x, l0y, h0y, l1x, h1x, l1y, h1y;
            seed2(l0x, h0x, l0y, h0y, add2(z0, t0, q));
            seed2(l1x, h1x, l1y, h1y, add2(z1, t1, q));
            mac2(l0x, h0x, l0y, h0y, a0, fac);
            mac2(l1x, h1x, l1y, h1y, a1, fac);
            z0 = reduce2(l0x, h0x, l0y, h0y, q, cr0, cr1);
            z1 = reduce2(l1x, h1x, l1y, h1y, q, cr0, cr1);
        }
        Z[x] = z0;
        Z[s_poly + x] = z1;
    }
}

struct HyKeyAddArgs
{
    uint64_t *key;          // [beta][2][k][N]
    const uint64_t *newkey; // [k][N], rows < k - alpha read
    uint64_t fac[MOAI_MAX_RNS]; // P mod q_r
    HyDims d;                   // at L = k - alpha
};

// row r of c0 of digit r / alpha += (P mod q_r) * newkey[r]      (keygenerator.cpp:315-333 with P for the special prime)
__global__ __launch_bounds__(256) void hy_key_add_kernel(HyKeyAddArgs g)
{
    const uint32_t r = blockIdx.y;
    const PrimeConst *pc = g.d.pc + r;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1, fac = g.fac[r];
    const size_t n2 = g.d.n2;
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(g.key) + ((size_t)(r / g.d.alpha) * 2 * g.d.k + r) * n2;
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(g.newkey) + (size_t)r * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.d.n2; j += gridDim.x * 256u)
    {
        const ulonglong2 v = s[j];
        ulonglong2 c = dst[j];
        c.x = csub(c.x + mulmod_barrett(v.x, fac, q, cr0, cr1), q);
        c.y = csub(c.y + mulmod_barrett(v.y, fac, q, cr0, cr1), q);
        dst[j] = c;
    }
}

// ---- relinearize + rescale: one mod-down by W = P q_{L-1} (moai_relinearize_rescale_hybrid) ---------------------------------------
// the constants of the merged mod-down at (L, alpha), a sibling of HyTable in the context's map of device blocks: sources
// S = {q_{L-1}, p_0 .. p_{alpha-1}}, targets q_i, i < L - 1
struct alignas(16) HyRescaleTable
{
    Tw winv[MOAI_MAX_RNS]; // W^-1 mod q_i
    Tw qinv[MOAI_MAX_RNS]; // q_{L-1}^-1 mod q_i
    HyConv conv;           // src_pre = floor(W / 2) mod m, tgt_post = floor(W / 2) mod q_i, src_inv = (W / m)^-1, w = (W / m) mod q_i
};

struct HyProductArgs
{
    const uint64_t *x, *y; // [B][2][L][N], y may be x
    uint64_t *out;         // [B][3][L][N]
    const PrimeConst *pc;
    uint32_t L, n2;
};

// out[b] = (x0 y0, x0 y1 + x1 y0, x1 y1) under q_i; blockIdx.y = b * L + i.  The canonical residues of moai_ct_multiply, and of
// moai_ct_square where y is x (x0 x1 + x1 x0 = 2 x0 x1).  The middle sum is two products below 2^122: below 2^123, one reduction.
__global__ __launch_bounds__(256) void hy_ct_product_kernel(HyProductArgs g)
{
    const uint32_t b = blockIdx.y / g.L, i = blockIdx.y % g.L;
    const PrimeConst *pc = g.pc + i;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = g.n2;
    const ulonglong2 *x0 = reinterpret_cast<const ulonglong2 *>(g.x) + ((size_t)(b * 2) * g.L + i) * n2, *x1 = x0 + (size_t)g.L * n2;
    const ulonglong2 *y0 = reinterpret_cast<const ulonglong2 *>(g.y) + ((size_t)(b * 2) * g.L + i) * n2, *y1 = y0 + (size_t)g.L * n2;
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(g.out) + ((size_t)(b * 3) * g.L + i) * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.n2; j += gridDim.x * 256u)
    {
        const ulonglong2 a0 = x0[j], a1 = x1[j], b0 = y0[j], b1 = y1[j];
        uint64_t lx = 0, hx = 0, ly = 0, hy = 0;
        mac2(lx, hx, ly, hy, a0, b1);
        mac2(lx, hx, ly, hy, a1, b0);
        o[j] = mulmod2(a0, b0, q, cr0, cr1);
        o[(size_t)g.L * n2 + j] = reduce2(lx, hx, ly, hy, q, cr0, cr1);
        o[2 * (size_t)g.L * n2 + j] = mulmod2(a1, b1, q, cr0, cr1);
    }
}

struct HyLiftArgs
{
    uint64_t *acc;       // [B][2][L + alpha][N]: row L - 1 of both polynomials is lifted in place
    const uint64_t *ct3; // [B][3][L][N]: row L - 1 of c_0 and c_1 read
    uint64_t plast;      // P mod q_{L-1}
    HyDims d;
};

struct HyLiftListArgs : HyLiftArgs
{
    const KsList *lst; // ciphertext b's [3][L][N] block is lst->ins[b] (ct3 unused)
};

// Z_p[L-1] = acc[p][L-1] + (P mod q_{L-1}) c_p[L-1]: the one data row among the merged mod-down's sources; blockIdx.y = b * 2 + p.
// The sum is one canonical residue (below 2^61) plus one product below 2^122: one reduction.
// LIST: c_p is read from the member's own block; b is uniform over the workgroup (a scalar load of the list entry).
template <bool LIST = false>
__global__ __launch_bounds__(256) void hy_lift_last_row_kernel(std::conditional_t<LIST, HyLiftListArgs, HyLiftArgs> g)
{
    const HyDims &d = g.d;
    const uint32_t b = blockIdx.y >> 1, p = blockIdx.y & 1u, last = d.L - 1;
    const PrimeConst *pc = d.pc + last;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t n2 = d.n2;
    ulonglong2 *acc = reinterpret_cast<ulonglong2 *>(g.acc) + ((size_t)blockIdx.y * (d.L + d.alpha) + last) * n2;
    const ulonglong2 *cp = reinterpret_cast<const ulonglong2 *>(g.ct3) + ((size_t)(b * 3 + p) * d.L + last) * n2;
    if constexpr (LIST)
    {
        cp = reinterpret_cast<const ulonglong2 *>(g.lst->ins[b]) + ((size_t)p * d.L + last) * n2;
    }
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < d.n2; x += gridDim.x * 256u)
    {
        uint64_t lx, hx, ly, hy;
        seed2(lx, hx, ly, hy, acc[x]);
        mac2(lx, hx, ly, hy, cp[x], g.plast);
        acc[x] = reduce2(lx, hx, ly, hy, q, cr0, cr1);
    }
}

struct HyRescaleFinalArgs
{
    const uint64_t *acc;  // [B][2][L + alpha][N]
    const uint64_t *conv; // [2B][L - 1][N], NTT form
    const uint64_t *ct3;  // [B][3][L][N]: c_0 and c_1 read
    uint64_t *out;        // [B][2][L - 1][N]
    const Tw *winv, *qinv;
    HyDims d;
};

struct HyRescaleFinalListArgs : HyRescaleFinalArgs
{
    const KsList *lst; // ciphertext b's [3][L][N] block is lst->ins[b] and its [2][L - 1][N] result lst->outs[b] (ct3 and out unused)
};

// out[b][p][i] = c_p[i] [q_{L-1}^-1]_{q_i} + (acc[p][i] - conv_i) [W^-1]_{q_i} mod q_i, i < L - 1: the finish of the merged mod-down
// with the lift (P mod q_i) c_p[i] W^-1 = c_p[i] q_{L-1}^-1 taken on its own multiplier.  blockIdx.y = (b * 2 + p) (L - 1) + i.  No
// 128-bit sum: two Shoup products made canonical and one canonical add.
// LIST: c_p and the output per member, as hy_lift_last_row_kernel.
template <bool LIST = false>
__global__ __launch_bounds__(256) void hy_rescale_finalize_kernel(std::conditional_t<LIST, HyRescaleFinalListArgs, HyRescaleFinalArgs> g)
{
    const HyDims &d = g.d;
    const uint32_t lo = d.L - 1, poly = blockIdx.y / lo, i = blockIdx.y % lo, b = poly >> 1, p = poly & 1u;
    const uint64_t q = d.pc[i].q;
    const Tw wi = g.winv[i], qi = g.qinv[i];
    const size_t n2 = d.n2;
    const ulonglong2 *acc = reinterpret_cast<const ulonglong2 *>(g.acc) + ((size_t)poly * (d.L + d.alpha) + i) * n2;
    const ulonglong2 *u = reinterpret_cast<const ulonglong2 *>(g.conv) + (size_t)blockIdx.y * n2;
    const ulonglong2 *cp = reinterpret_cast<const ulonglong2 *>(g.ct3) + ((size_t)(b * 3 + p) * d.L + i) * n2;
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(g.out) + (size_t)blockIdx.y * n2;
    if constexpr (LIST)
    {
        cp = reinterpret_cast<const ulonglong2 *>(g.lst->ins[b]) + ((size_t)p * d.L + i) * n2;
        o = reinterpret_cast<ulonglong2 *>(g.lst->outs[b]) + ((size_t)p * lo + i) * n2;
    }
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < d.n2; x += gridDim.x * 256u)
    {
        const ulonglong2 a = acc[x], v = u[x], c = cp[x];
        ulonglong2 r, t;
        r.x = csub(mul_shoup_lazy(a.x + q - v.x, wi.w, wi.wq, q), q);
        r.y = csub(mul_shoup_lazy(a.y + q - v.y, wi.w, wi.wq, q), q);
        t.x = csub(mul_shoup_lazy(c.x, qi.w, qi.wq, q), q);
        t.y = csub(mul_shoup_lazy(c.y, qi.w, qi.wq, q), q);
        o[x] = add2(r, t, q);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static inline size_t hy_beta(size_t L, size_t alpha)
{
    return (L + alpha - 1) / alpha;
}

static HyDims hy_dims(const moai_ctx *c, size_t L, size_t alpha)
{
    HyDims d;
    d.alpha = (uint32_t)alpha;
    d.beta = (uint32_t)hy_beta(L, alpha);
    d.k = (uint32_t)c->k;
    fill_rows(d, c, L);
    return d;
}

// product of the context primes idx[0..cnt) except idx[skip], modulo m
static uint64_t hy_prod_mod(const moai_ctx *c, const uint32_t *idx, size_t cnt, size_t skip, uint64_t m)
{
    uint64_t r = 1 % m;
    for (size_t i = 0; i < cnt; ++i)
    {
        if (i != skip)
        {
            r = mulmod(r, c->primes[idx[i]] % m, m);
        }
    }
    return r;
}

static uint64_t hy_invmod(uint64_t a, uint64_t q)
{
    return powmod(a, q - 2, q);
}

// floor(P / 2) mod m from P mod m (P odd)
static uint64_t hy_half_mod(uint64_t p_mod_m, uint64_t m)
{
    return mulmod((p_mod_m + m - 1) % m, hy_invmod(2, m), m);
}

// the device block of constants for (L, alpha); the caller holds op_mutex.  Built on first use with a blocking copy from a host
// buffer that lives until the copy has returned.
static int hy_table(moai_ctx *c, size_t L, size_t alpha, const HyTable **out)
{
    const auto key = std::make_pair(L, alpha);
    auto it = c->hybrid_tables.find(key);
    if (it != c->hybrid_tables.end())
    {
        *out = static_cast<const HyTable *>(it->second);
        return MOAI_OK;
    }
    const size_t k = c->k, beta = hy_beta(L, alpha);
    const size_t conv_bytes = offsetof(HyTable, conv) + (beta + 1) * sizeof(HyConv);
    const size_t bytes = conv_bytes + beta * (L + alpha) * sizeof(uint64_t);
    std::vector<unsigned char> host(bytes, 0);
    HyTable *t = reinterpret_cast<HyTable *>(host.data());
    HyConv *convs = reinterpret_cast<HyConv *>(host.data() + offsetof(HyTable, conv));
    uint32_t special[HY_MAX_ALPHA];
    for (size_t s = 0; s < alpha; ++s)
    {
        special[s] = (uint32_t)(k - alpha + s);
    }
    for (size_t i = 0; i < L; ++i)
    {
        const uint64_t q = c->primes[i];
        t->pinv[i] = make_tw(hy_invmod(hy_prod_mod(c, special, alpha, alpha, q), q), q);
    }
    for (size_t j = 0; j < beta; ++j)
    {
        HyConv &cv = convs[j];
        const size_t lo = j * alpha, hi = std::min(lo + alpha, L);
        cv.nsrc = (uint32_t)(hi - lo);
        for (size_t r = 0; r < cv.nsrc; ++r)
        {
            cv.src_prime[r] = (uint32_t)(lo + r);
        }
        for (size_t r = 0; r < cv.nsrc; ++r)
        {
            const uint64_t q = c->primes[lo + r];
            cv.src_inv[r] = make_tw(hy_invmod(hy_prod_mod(c, cv.src_prime, cv.nsrc, r, q), q), q);
        }
        cv.ntgt = 0;
        for (size_t row = 0; row < L + alpha; ++row)
        {
            if (row >= lo && row < hi)
            {
                continue;
            }
            const uint32_t prime = (uint32_t)hy_row_prime(row, L, alpha, k);
            const uint32_t tg = cv.ntgt++;
            cv.tgt_prime[tg] = prime;
            for (size_t r = 0; r < cv.nsrc; ++r)
            {
                cv.w[tg][r] = hy_prod_mod(c, cv.src_prime, cv.nsrc, r, c->primes[prime]);
            }
        }
    }
    {
        HyConv &cv = convs[beta];
        cv.nsrc = (uint32_t)alpha;
        cv.ntgt = (uint32_t)L;
        for (size_t s = 0; s < alpha; ++s)
        {
            const uint64_t p = c->primes[special[s]];
            cv.src_prime[s] = special[s];
            cv.src_inv[s] = make_tw(hy_invmod(hy_prod_mod(c, special, alpha, s, p), p), p);
            cv.src_pre[s] = hy_half_mod(0, p);
        }
        for (size_t i = 0; i < L; ++i)
        {
            const uint64_t q = c->primes[i];
            cv.tgt_prime[i] = (uint32_t)i;
            cv.tgt_post[i] = hy_half_mod(hy_prod_mod(c, special, alpha, alpha, q), q);
            for (size_t s = 0; s < alpha; ++s)
            {
                cv.w[i][s] = hy_prod_mod(c, special, alpha, s, q);
            }
        }
    }
    // the hoisted rotations' correction: sum_{r in R_j} q_r (D_j / q_r) = |R_j| D_j, modulo every row's prime (0 on the rows of R_j)
    uint64_t *mult = reinterpret_cast<uint64_t *>(host.data() + conv_bytes);
    for (size_t j = 0; j < beta; ++j)
    {
        const HyConv &cv = convs[j];
        for (size_t row = 0; row < L + alpha; ++row)
        {
            const uint64_t m = c->primes[hy_row_prime(row, L, alpha, k)];
            mult[j * (L + alpha) + row] = mulmod(cv.nsrc % m, hy_prod_mod(c, cv.src_prime, cv.nsrc, cv.nsrc, m), m);
        }
    }
    void *dev = nullptr;
    MOAI_HIP_CHECK(hipMalloc(&dev, bytes));
    hipError_t e = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        (void)hipFree(dev);
        return set_error(MOAI_EHIP, "hybrid key-switch constants: %s", hipGetErrorString(e));
    }
    c->hybrid_tables[key] = dev;
    *out = static_cast<const HyTable *>(dev);
    return MOAI_OK;
}

static int hy_convert(moai_ctx *c, const uint64_t *src, size_t src_stride, size_t src_off, uint64_t *dst, const HyConv *cv, size_t nsrc,
                      size_t polys, hipStream_t s)
{
    HyConvArgs a;
    a.src = src;
    a.dst = dst;
    a.cv = cv;
    a.pc = c->pc;
    a.src_stride = (uint32_t)src_stride;
    a.src_off = (uint32_t)src_off;
    a.n2 = (uint32_t)(c->n >> 1);
    // the smallest instantiation that holds the digit: its registers are the unrolled source rows
    const int amax = nsrc <= 1 ? 1 : nsrc <= 2 ? 2 : nsrc <= 4 ? 4 : nsrc <= 8 ? 8 : 16;
    return dispatch<1, 2, 4, 8, 16>("digit size ", amax,
                                    [&](auto A) { return launch_rows(hy_convert_kernel<decltype(A)::value>, c, polys, s, a); });
}

// rows of N words of scratch per ciphertext: t, the converted digits, acc, the special rows, conv, and gal_rows rows of gathered
// input (2 L: the permuted input of apply_galois; L: the third polynomial of a member of the relinearize list; 0 otherwise)
static size_t hy_rows_per_ct(size_t L, size_t alpha, size_t gal_rows)
{
    const size_t beta = hy_beta(L, alpha);
    return gal_rows + L + (beta * (L + alpha) - L) + 2 * (L + alpha) + 2 * alpha + 2 * L;
}

struct HyLayout
{
    size_t gal, t, ext, acc, x, conv, total; // byte offsets
};

static HyLayout hy_layout(const moai_ctx *c, size_t L, size_t alpha, size_t cb, size_t gal_rows)
{
    const size_t row = c->n * sizeof(uint64_t), beta = hy_beta(L, alpha);
    HyLayout w;
    w.gal = 0;
    w.t = w.gal + align256(cb * gal_rows * row);
    w.ext = w.t + align256(cb * L * row);
    w.acc = w.ext + align256(cb * (beta * (L + alpha) - L) * row);
    w.x = w.acc + align256(cb * 2 * (L + alpha) * row);
    w.conv = w.x + align256(cb * 2 * alpha * row);
    w.total = w.conv + align256(cb * 2 * L * row);
    return w;
}

// ciphertexts per chunk: as many as MOAI_HYBRID_TMP_KB holds, at least one
static size_t hy_chunk(const moai_ctx *c, size_t L, size_t alpha, size_t batch, size_t gal_rows)
{
    const size_t budget = (size_t)std::max(1l, tuning(K_HYBRID_TMP_KB)) << 10;
    const size_t per = hy_rows_per_ct(L, alpha, gal_rows) * c->n * sizeof(uint64_t);
    size_t cb = budget / per;
    cb = cb < 1 ? 1 : cb;
    // row-per-workgroup launches: 2 * cb * (L + alpha) rows in gridDim.y
    const size_t cap = 65535 / (2 * (L + alpha));
    cb = cb > cap ? cap : cb;
    return cb < batch ? cb : batch;
}

// steps 1-3 for B ciphertexts: t [B][L][N] = INTT of the target rows tg, ext = the converted rows of every digit in NTT form
// (HyMacArgs::ext)
static int hy_decompose(moai_ctx *c, const HyTable *tab, const KsTarget &tg, size_t L, size_t alpha, size_t B, uint64_t *t, uint64_t *ext,
                        hipStream_t s)
{
    const size_t n = c->n, beta = hy_beta(L, alpha);
    const HyConv *cvs = tab->conv; // device address arithmetic only
    RowMap rm;
    // 1. t = INTT(target)
    MOAI_TRY(make_rowmap(c, L, nullptr, &rm));
    MOAI_TRY(ntt_launch(c, t, B, L, rm, true, s, tg.ptr, tg.stride_rows, tg.off_rows));
    // 2., 3. mod-up of every digit and the forward transform of the converted rows: all rows but the digit's own
    for (size_t j = 0; j < beta; ++j)
    {
        const size_t lo = j * alpha, hi = std::min(lo + alpha, L);
        uint64_t *ext_j = ext + j * B * L * n;
        MOAI_TRY(hy_convert(c, t, L, lo, ext_j, cvs + j, hi - lo, B, s));
        const size_t cr = hy_rowmap(c, L, alpha, lo, hi, &rm);
        MOAI_TRY(ntt_launch(c, ext_j, B, cr, rm, false, s));
    }
    return MOAI_OK;
}

// step 5 up to the last kernel, for the accumulators [B][2][L + alpha][N] of B switches: x [2B][alpha][N] = INTT(special rows),
// conv [2B][L][N] = NTT(base conversion with the rounding terms)
static int hy_mod_down(moai_ctx *c, const HyTable *tab, const uint64_t *acc, uint64_t *x, uint64_t *conv, size_t L, size_t alpha, size_t B,
                       hipStream_t s)
{
    RowMap rm{};
    hy_rowmap(c, L, alpha, 0, L, &rm); // the special rows
    MOAI_TRY(ntt_launch(c, x, 2 * B, alpha, rm, true, s, acc, L + alpha, L));
    MOAI_TRY(hy_convert(c, x, alpha, 0, conv, tab->conv + hy_beta(L, alpha), alpha, 2 * B, s));
    MOAI_TRY(make_rowmap(c, L, nullptr, &rm));
    return ntt_launch(c, conv, 2 * B, L, rm, false, s);
}

// the hy_mac_kernel / hy_hoisted_mac_kernel grid: blockIdx.x = ciphertext, .y covers a row, .z = row of L + alpha
static int hy_mac_grid(const moai_ctx *c, size_t B, size_t rows, dim3 *grid)
{
    MOAI_CHECK_GRID_ROWS(rows);
    *grid = dim3((uint32_t)B, row_grid(c, 1).x, (uint32_t)rows);
    return MOAI_OK;
}

// step 4 for B ciphertexts with the key m.key or, with a list, member b's own
static int hy_mac(moai_ctx *c, const HyMacArgs &m, size_t B, const KsList *lst, hipStream_t s)
{
    dim3 grid;
    MOAI_TRY(hy_mac_grid(c, B, m.d.L + m.d.alpha, &grid));
    return plain_or_list<HyMacListArgs>(m, lst, [&](const auto &args, auto LIST) {
        hipLaunchKernelGGL(hy_mac_kernel<decltype(LIST)::value>, grid, dim3(256), 0, s, args);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    });
}

// one chunk of B ciphertexts: out [B][2][L][N] = add (KsAddend) + the switch of the target rows tg.  With tg.lst (a device record,
// common.h KsList) ciphertext b's key is lst->keys[b] and the last kernel writes lst->outs[b], adds lst->sums[b] and, for add.mode 1,
// reads the addend from lst->ins[b]; key and out are not used
static int hy_switch_chunk(moai_ctx *c, const HyTable *tab, uint64_t *out, const KsTarget &tg, const uint64_t *key, size_t L, size_t alpha,
                           size_t B, void *wsp, const HyLayout &w, const KsAddend &add, hipStream_t s)
{
    uint64_t *t = at_bytes(wsp, w.t), *ext = at_bytes(wsp, w.ext), *acc = at_bytes(wsp, w.acc), *x = at_bytes(wsp, w.x);
    uint64_t *conv = at_bytes(wsp, w.conv);
    // 1. t = INTT(target); 2., 3. mod-up of every digit and the forward transform of the converted rows
    MOAI_TRY(hy_decompose(c, tab, tg, L, alpha, B, t, ext, s));
    // 4. the inner products with the key
    HyMacArgs m;
    m.ext = ext;
    m.tgt = tg.ptr;
    m.key = key;
    m.acc = acc;
    m.tgt_stride = (uint32_t)tg.stride_rows;
    m.tgt_off = (uint32_t)tg.off_rows;
    m.d = hy_dims(c, L, alpha);
    MOAI_TRY(hy_mac(c, m, B, tg.lst, s));
    // 5. mod-down: x = INTT(special rows), conv = NTT(base conversion with the rounding terms), out = addend + (acc - conv) / P
    MOAI_TRY(hy_mod_down(c, tab, acc, x, conv, L, alpha, B, s));
    return moddown_finalize(c, acc, (uint32_t)(L + alpha), conv, out, 2 * B, L, tab->pinv, add, tg.lst, s);
}

// what every hybrid entry point refuses, in the order the header gives: first what needs no context
static int hy_check(const moai_ctx *c, size_t alpha, size_t L, bool level)
{
    if (alpha == 0)
    {
        return set_error(MOAI_EINVAL, "alpha = 0: a digit holds at least one prime");
    }
    if (level && L == 0)
    {
        return set_error(MOAI_EINVAL, "L = 0 out of range");
    }
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (alpha >= c->k)
    {
        return set_error(MOAI_EINVAL, "alpha = %zu leaves no data prime in a context of %zu primes", alpha, c->k);
    }
    if (alpha > HY_MAX_ALPHA)
    {
        return set_error(MOAI_EINVAL, "alpha = %zu: digits of more than %u primes are not supported", alpha, HY_MAX_ALPHA);
    }
    if (level && L > c->k - alpha)
    {
        return set_error(MOAI_EINVAL, "L = %zu out of range: %zu data primes with alpha = %zu", L, c->k - alpha, alpha);
    }
    return MOAI_OK;
}

enum
{
    HY_SWITCH,
    HY_RELIN,
    HY_GALOIS
};

// the three switches: validated, then chunk by chunk on the stream's workspace
//   HY_SWITCH  io = ct [batch][2][L][N] in place, in = target [batch][L][N]
//   HY_RELIN   in = ct3 [batch][3][L][N], io = out [batch][2][L][N]
//   HY_GALOIS  in [batch][2][L][N], io = out [batch][2][L][N], which may be in itself; sum: null, or [batch][2][L][N] added by the last
//              kernel (it may be io, never in)
static int hy_entry(moai_ctx *c, int kind, uint64_t *io, const uint64_t *in, const uint64_t *key, size_t L, size_t alpha, uint32_t elt,
                    size_t batch, void *stream, const uint64_t *sum = nullptr)
{
    // every kind but HY_GALOIS comes with element 1; an even element is refused before the context is looked at
    MOAI_TRY(galois_elt_check(nullptr, elt));
    MOAI_TRY(hy_check(c, alpha, L, true));
    MOAI_TRY(galois_elt_check(c, elt));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (!io || !key || !in || (kind == HY_RELIN && in == io))
    {
        return set_error(MOAI_EINVAL, kind == HY_RELIN ? "bad pointers" : "null argument");
    }
    const size_t n = c->n;
    if (kind == HY_GALOIS)
    {
        const size_t bytes = batch * 2 * L * n * sizeof(uint64_t);
        if (sum && sum == in)
        {
            return set_error(MOAI_EINVAL, "null argument, or the sum is the input"); // as moai_apply_galois_acc
        }
        if ((io != in && overlap(io, bytes, in, bytes)) || (sum && sum != io && overlap(io, bytes, sum, bytes)))
        {
            return set_error(MOAI_EINVAL, "the output overlaps an input");
        }
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *table = nullptr;
    if (kind == HY_GALOIS)
    {
        MOAI_TRY(galois_table(c, elt, &table)); // built before the first launch of the call
    }
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    const size_t gal_rows = kind == HY_GALOIS ? 2 * L : 0;
    const size_t cb = hy_chunk(c, L, alpha, batch, gal_rows);
    const HyLayout w = hy_layout(c, L, alpha, cb, gal_rows);
    void *wsp;
    MOAI_TRY(workspace(c, w.total, s, &wsp));
    return for_chunks(batch, cb, [&](size_t b0, size_t B) {
        switch (kind)
        {
        case HY_SWITCH:
            // ct += switch(target)
            return hy_switch_chunk(c, tab, io + b0 * 2 * L * n, { in + b0 * L * n, L, 0 }, key, L, alpha, B, wsp, w,
                                   { io + b0 * 2 * L * n, 2 * L, 1 }, s);
        case HY_RELIN:
            // out = (c0, c1) + switch(c2)      (evaluator.cpp:1383-1392)
            return hy_switch_chunk(c, tab, io + b0 * 2 * L * n, { in + b0 * 3 * L * n, 3 * L, 2 * L }, key, L, alpha, B, wsp, w,
                                   { in + b0 * 3 * L * n, 3 * L, 1 }, s);
        default:
        {
            // out = (galois(in0), 0) + switch(galois(in1)) [+ sum]      (evaluator.cpp:2631-2654): both summands are added by the last
            // kernel, so a chunk of out is written once, after the chunk of in has been permuted into the scratch
            uint64_t *tmp = at_bytes(wsp, w.gal);
            MOAI_TRY(moai_galois_permute(c, in + b0 * 2 * L * n, tmp, B * 2, L, elt, stream));
            return hy_switch_chunk(c, tab, io + b0 * 2 * L * n, { tmp, 2 * L, L }, key, L, alpha, B, wsp, w,
                                   { tmp, 2 * L, 2, sum ? sum + b0 * 2 * L * n : nullptr }, s);
        }
        }
    });
}

// ---- hoisted rotations ------------------------------------------------------------------------------------------------------
// rows of N words of scratch: per ciphertext t and the converted digits, per (rotation in flight, ciphertext) acc, the special
// rows, conv and the permuted c0
static inline size_t hy_hoist_shared_rows(size_t L, size_t alpha)
{
    return hy_beta(L, alpha) * (L + alpha);
}

static inline size_t hy_hoist_rotation_rows(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * alpha + 2 * L + L;
}

struct HyHoistLayout
{
    size_t flag, t, ext, acc, x, conv, c0, total; // byte offsets
};

static HyHoistLayout hy_hoist_layout(const moai_ctx *c, size_t L, size_t alpha, size_t cb, size_t G)
{
    const size_t row = c->n * sizeof(uint64_t), beta = hy_beta(L, alpha);
    HyHoistLayout w;
    w.flag = 0;
    w.t = 256;
    w.ext = w.t + align256(cb * L * row);
    w.acc = w.ext + align256(cb * (beta * (L + alpha) - L) * row);
    w.x = w.acc + align256(G * cb * 2 * (L + alpha) * row);
    w.conv = w.x + align256(G * cb * 2 * alpha * row);
    w.c0 = w.conv + align256(G * cb * 2 * L * row);
    w.total = w.c0 + align256(G * cb * L * row);
    return w;
}

// ciphertexts per chunk (*cb) and rotations in flight (*G) under MOAI_HYBRID_TMP_KB: as many ciphertexts as fit with one rotation
// in flight, then as many rotations as fit beside them; at least one of each, and no row-per-workgroup grid above 65535 (the
// mod-down runs over 2 * cb * G polynomials of at most L + alpha rows)
static void hy_hoist_chunk(const moai_ctx *c, size_t L, size_t alpha, size_t batch, size_t R, size_t *cb_out, size_t *G_out)
{
    const size_t budget = (size_t)std::max(1l, tuning(K_HYBRID_TMP_KB)) << 10, row = c->n * sizeof(uint64_t);
    const size_t shared = hy_hoist_shared_rows(L, alpha) * row, rot = hy_hoist_rotation_rows(L, alpha) * row;
    const size_t cap = 65535 / (2 * (L + alpha));
    size_t cb = budget / (shared + rot);
    cb = cb < 1 ? 1 : cb;
    cb = cb > cap ? cap : cb;
    cb = cb < batch ? cb : batch;
    size_t G = budget / cb > shared ? (budget / cb - shared) / rot : 0;
    G = G < 1 ? 1 : G;
    G = G > cap / cb ? cap / cb : G;
    *cb_out = cb;
    *G_out = G < R ? G : R;
}

static int hy_hoist_correction(moai_ctx *c, const uint64_t *key, uint32_t elt, size_t L, size_t alpha, uint64_t *correction, hipStream_t s)
{
    const size_t rows = L + alpha, beta = hy_beta(L, alpha);
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    void *wsp;
    MOAI_TRY(workspace(c, align256(rows * c->n * sizeof(uint64_t)), s, &wsp));
    uint64_t *mask = static_cast<uint64_t *>(wsp);
    // the sign mask under every row's prime, then its forward transform
    MOAI_TRY(galois_sign_mask(c, mask, elt, rows, s));
    RowMap rm{};
    hy_rowmap(c, L, alpha, 0, 0, &rm);
    MOAI_TRY(ntt_launch(c, mask, 1, rows, rm, false, s));
    HyCorrArgs g;
    g.key = key;
    g.mask = mask;
    g.mult = hy_hoist_mult(tab, beta);
    g.out = correction;
    g.d = hy_dims(c, L, alpha);
    return launch_rows(hy_hoist_correction_kernel, c, 2 * rows, s, g);
}

struct HyHoistRotations
{
    size_t R;
    const uint32_t *elts;
    const uint32_t *const *tables;
    const uint64_t *const *keys, *const *corrs;
    uint64_t *const *outs;
};

// the hoisted MAC for rotations [r0, r0 + g) of one chunk, MOAI_HYBRID_HOIST_NR of them per pass over the digits; rotation r0 + h
// accumulates at acc + h * B * 2 * (L + alpha) * N
static int hy_hoisted_mac(moai_ctx *c, const uint64_t *ext, const uint64_t *in, const HyHoistRotations &rot, size_t r0, size_t g,
                          uint64_t *acc, size_t L, size_t alpha, size_t B, hipStream_t s)
{
    const long per_pass = tuning(K_HYBRID_HOIST_NR);
    dim3 grid;
    MOAI_TRY(hy_mac_grid(c, B, L + alpha, &grid));
    for (size_t r = 0; r < g;)
    {
        const size_t nr = per_pass >= 4 && r + 3 < g ? 4 : (per_pass >= 2 && r + 1 < g ? 2 : 1);
        HyHoistMacArgs m;
        m.ext = ext;
        m.in = in;
        for (size_t h = 0; h < (size_t)HY_HOIST_MAX_NR; ++h)
        {
            const size_t rr = r + (h < nr ? h : 0);
            m.table[h] = rot.tables[r0 + rr];
            m.key[h] = rot.keys[r0 + rr];
            m.corr[h] = rot.corrs[r0 + rr];
            m.acc[h] = acc + rr * B * 2 * (L + alpha) * c->n;
        }
        m.d = hy_dims(c, L, alpha);
        MOAI_TRY((dispatch<1, 2, 4>("rotations per pass ", (int)nr, [&](auto NR) {
            hipLaunchKernelGGL(hy_hoisted_mac_kernel<decltype(NR)::value>, grid, dim3(256), 0, s, m);
            return MOAI_OK;
        })));
        MOAI_LAUNCH_CHECK();
        r += nr;
    }
    return MOAI_OK;
}

// one chunk of B ciphertexts at `in` [B][2][L][N]; rotation r's result goes to rot.outs[r] + out_off.  *fallback is set when
// INTT(c1) holds a zero coefficient: nothing but the scratch has been written then, and the caller makes the separate calls.
static int hy_hoist_chunk_run(moai_ctx *c, const uint64_t *in, size_t out_off, const HyHoistRotations &rot, size_t L, size_t alpha, size_t B,
                              size_t cb, size_t G, bool *fallback, hipStream_t s)
{
    const size_t n = c->n;
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    const HyHoistLayout w = hy_hoist_layout(c, L, alpha, cb, G);
    void *wsp;
    MOAI_TRY(workspace(c, w.total, s, &wsp));
    uint32_t *flag = reinterpret_cast<uint32_t *>(at_bytes(wsp, w.flag));
    uint64_t *t = at_bytes(wsp, w.t), *ext = at_bytes(wsp, w.ext), *acc = at_bytes(wsp, w.acc), *x = at_bytes(wsp, w.x);
    uint64_t *conv = at_bytes(wsp, w.conv), *pc0 = at_bytes(wsp, w.c0);
    // steps 1-3 on the UNPERMUTED c1, once for all rotations
    MOAI_TRY(hy_decompose(c, tab, { in, 2 * L, L }, L, alpha, B, t, ext, s));
    MOAI_TRY(probe_any_zero(c, t, B * L * n, flag, s, fallback)); // a zero coefficient: the identity does not hold for it
    if (*fallback)
    {
        return MOAI_OK;
    }
    return for_chunks(rot.R, G, [&](size_t r0, size_t g) {
        MOAI_TRY(hy_hoisted_mac(c, ext, in, rot, r0, g, acc, L, alpha, B, s));
        // pc0 [g][B][L][N] = perm_r(c0): the addend of the even polynomials (add_mode 2, ciphertexts L rows apart)
        for (size_t r = 0; r < g; ++r)
        {
            MOAI_TRY(galois_permute_c0(c, in, pc0 + r * B * L * n, B, L, rot.elts[r0 + r], s));
        }
        // steps 5 over (rotation, ciphertext) pairs
        MOAI_TRY(hy_mod_down(c, tab, acc, x, conv, L, alpha, g * B, s));
        for (size_t r = 0; r < g; ++r)
        {
            MOAI_TRY(moddown_finalize(c, acc + r * B * 2 * (L + alpha) * n, (uint32_t)(L + alpha), conv + r * B * 2 * L * n,
                                      rot.outs[r0 + r] + out_off, 2 * B, L, tab->pinv, { pc0 + r * B * L * n, L, 2 }, nullptr, s));
        }
        return MOAI_OK;
    });
}

// ---- plaintext-weighted sums of hoisted rotations -------------------------------------------------------------------------------
// rows of N words of scratch: per ciphertext t, the converted digits and the unhoisted route's permuted input and accumulators; per
// (output in flight, ciphertext) the sums S, the special rows, conv and the addend.  Nothing grows with R.
static inline size_t hy_dot_shared_rows(size_t L, size_t alpha)
{
    return hy_beta(L, alpha) * (L + alpha) + 2 * L + 2 * (L + alpha);
}

static inline size_t hy_dot_output_rows(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * alpha + 2 * L + 2 * L;
}

struct HyDotLayout
{
    size_t flag, t, ext, gal, acc, S, x, conv, add, total; // byte offsets
};

static HyDotLayout hy_dot_layout(const moai_ctx *c, size_t L, size_t alpha, size_t cb, size_t G)
{
    const size_t row = c->n * sizeof(uint64_t), beta = hy_beta(L, alpha);
    HyDotLayout w;
    w.flag = 0;
    w.t = 256;
    w.ext = w.t + align256(cb * L * row);
    w.gal = w.ext + align256(cb * (beta * (L + alpha) - L) * row);
    w.acc = w.gal + align256(cb * 2 * L * row);
    w.S = w.acc + align256(cb * 2 * (L + alpha) * row);
    w.x = w.S + align256(G * cb * 2 * (L + alpha) * row);
    w.conv = w.x + align256(G * cb * 2 * alpha * row);
    w.add = w.conv + align256(G * cb * 2 * L * row);
    w.total = w.add + align256(G * cb * 2 * L * row);
    return w;
}

// ciphertexts per chunk (*cb) and outputs in flight (*G) under MOAI_HYBRID_TMP_KB, as hy_hoist_chunk sizes ciphertexts and rotations:
// at least one of each, G at most HY_DOT_MAX_NG, and no row-per-workgroup grid above 65535 (the mod-down runs over 2 * cb * G
// polynomials of at most L + alpha rows)
static void hy_dot_chunk(const moai_ctx *c, size_t L, size_t alpha, size_t batch, size_t n_out, size_t *cb_out, size_t *G_out)
{
    const size_t budget = (size_t)std::max(1l, tuning(K_HYBRID_TMP_KB)) << 10, row = c->n * sizeof(uint64_t);
    const size_t shared = hy_dot_shared_rows(L, alpha) * row, out = hy_dot_output_rows(L, alpha) * row;
    const size_t cap = 65535 / (2 * (L + alpha));
    size_t cb = budget / (shared + out);
    cb = cb < 1 ? 1 : cb;
    cb = cb > cap ? cap : cb;
    cb = cb < batch ? cb : batch;
    size_t G = budget / cb > shared ? (budget / cb - shared) / out : 0;
    G = G < 1 ? 1 : G;
    G = G > cap / cb ? cap / cb : G;
    G = G > (size_t)HY_DOT_MAX_NG ? (size_t)HY_DOT_MAX_NG : G;
    *cb_out = cb;
    *G_out = G < n_out ? G : n_out;
}

struct HyDotTerms
{
    size_t R, n_out;
    const uint32_t *elts;
    const uint32_t *const *tables; // null where the element is 1
    const uint64_t *const *keys, *const *corrs, *const *plains; // plains[g * R + r]
    uint64_t *const *outs;
};

// whether rotation r carries a term of one of the outputs gs[0 .. ng)
static bool hy_dot_used(const HyDotTerms &tm, const size_t *gs, size_t ng, size_t r)
{
    for (size_t h = 0; h < ng; ++h)
    {
        if (tm.plains[gs[h] * tm.R + r])
        {
            return true;
        }
    }
    return false;
}

// column `slot` of o.plain = the plaintexts of rotation r for the outputs gs[0 .. ng); returns the outputs that have one as bits
static uint32_t hy_dot_column(HyDotOutputs &o, const HyDotTerms &tm, const size_t *gs, size_t ng, size_t r, size_t slot)
{
    uint32_t present = 0;
    for (size_t h = 0; h < ng; ++h)
    {
        o.plain[h][slot] = tm.plains[gs[h] * tm.R + r];
        present |= o.plain[h][slot] ? 1u << h : 0u;
    }
    return present;
}

// one term through hy_dot_term_kernel: rows of L + alpha with accumulators A, rows of L without
static int hy_dot_term(moai_ctx *c, const uint64_t *A, const uint64_t *u, HyDotOutputs &o, const HyDotTerms &tm, const size_t *gs, size_t ng,
                       size_t r, size_t L, size_t alpha, size_t B, hipStream_t s)
{
    const uint32_t present = hy_dot_column(o, tm, gs, ng, r, 0);
    HyDotTermArgs a;
    a.A = A;
    a.u = u;
    a.d = hy_dims(c, L, alpha);
    dim3 grid;
    MOAI_TRY(hy_mac_grid(c, B, A ? L + alpha : L, &grid));
    hipLaunchKernelGGL(hy_dot_term_kernel, grid, dim3(256), 0, s, a, o);
    MOAI_LAUNCH_CHECK();
    o.seeded |= A ? present : 0u;
    return MOAI_OK;
}

// the scratch of the inner stage of a chunk: t and the digits of the unpermuted c1, and the unhoisted route's permuted input and
// accumulators
struct HyDotScratch
{
    uint64_t *t, *ext, *gal, *acc;
};

// The inner stage for the outputs gs[0 .. ng) of one chunk of B ciphertexts at `in`, up to its step 5: o.S and o.add (o.ng = ng)
// receive S_g and the addend a_g of every output, and o.seeded tells which outputs have a switched term (the S of the others is
// not written).  sc.t / sc.ext hold the digits of the unpermuted c1 unless `fallback`, which takes every rotation through the
// unhoisted steps 1-4 on the permuted input, to the same bits.  Shared by moai_hybrid_rotate_pt_dot and moai_hybrid_bsgs_dot.
static int hy_dot_inner(moai_ctx *c, const HyTable *tab, const uint64_t *in, const HyDotTerms &tm, const size_t *gs, size_t ng,
                        HyDotOutputs &o, const HyDotScratch &sc, size_t L, size_t alpha, size_t B, bool fallback, hipStream_t s)
{
    const size_t ct_words = B * 2 * L * c->n;
    const long per_pass = tuning(K_HYBRID_HOIST_NR);
    dim3 grid;
    MOAI_TRY(hy_mac_grid(c, B, L + alpha, &grid));
    MOAI_HIP_CHECK(hipMemsetAsync(o.add, 0, ng * ct_words * sizeof(uint64_t), s));
    std::vector<size_t> rot, ident; // the terms these outputs have
    for (size_t r = 0; r < tm.R; ++r)
    {
        if (hy_dot_used(tm, gs, ng, r))
        {
            (tm.elts[r] == 1 ? ident : rot).push_back(r);
        }
    }
    if (!fallback)
    {
        // the hoisted MAC, MOAI_HYBRID_HOIST_NR rotations per pass over the digits, weighted into S and the addend
        for (size_t i = 0; i < rot.size();)
        {
            const size_t left = rot.size() - i, nr = per_pass >= 4 && left >= 4 ? 4 : (per_pass >= 2 && left >= 2 ? 2 : 1);
            HyHoistMacArgs m{};
            m.ext = sc.ext;
            m.in = in;
            uint32_t present = 0;
            for (size_t h = 0; h < nr; ++h)
            {
                const size_t r = rot[i + h];
                m.table[h] = tm.tables[r];
                m.key[h] = tm.keys[r];
                m.corr[h] = tm.corrs[r];
                present |= hy_dot_column(o, tm, gs, ng, r, h);
            }
            m.d = hy_dims(c, L, alpha);
            MOAI_TRY((dispatch<1, 2, 4>("rotations per pass ", (int)nr, [&](auto NR) {
                hipLaunchKernelGGL(hy_hoisted_dot_kernel<decltype(NR)::value>, grid, dim3(256), 0, s, m, o);
                return MOAI_OK;
            })));
            MOAI_LAUNCH_CHECK();
            o.seeded |= present;
            i += nr;
        }
    }
    else
    {
        // per rotation: permute, steps 1-4 into one scratch accumulator, then its products
        for (size_t r : rot)
        {
            MOAI_TRY(moai_galois_permute(c, in, sc.gal, B * 2, L, tm.elts[r], s));
            MOAI_TRY(hy_decompose(c, tab, { sc.gal, 2 * L, L }, L, alpha, B, sc.t, sc.ext, s));
            HyMacArgs m;
            m.ext = sc.ext;
            m.tgt = sc.gal;
            m.key = tm.keys[r];
            m.acc = sc.acc;
            m.tgt_stride = (uint32_t)(2 * L);
            m.tgt_off = (uint32_t)L;
            m.d = hy_dims(c, L, alpha);
            hipLaunchKernelGGL(hy_mac_kernel<false>, grid, dim3(256), 0, s, m);
            MOAI_LAUNCH_CHECK();
            MOAI_TRY(hy_dot_term(c, sc.acc, sc.gal, o, tm, gs, ng, r, L, alpha, B, s));
        }
    }
    for (size_t r : ident)
    {
        MOAI_TRY(hy_dot_term(c, nullptr, in, o, tm, gs, ng, r, L, alpha, B, s));
    }
    return MOAI_OK;
}

// one chunk of B ciphertexts at `in` [B][2][L][N]; output g's result goes to tm.outs[g] + out_off.  sw: the outputs with a term whose
// element is not 1, G of them in flight; the others (idn) are sums of plain products.  *fallback is set when INTT(c1) holds a zero
// coefficient: the chunk then takes every rotation through the unhoisted steps 1-4 on the permuted input, to the same bits.
static int hy_dot_chunk_run(moai_ctx *c, const uint64_t *in, size_t out_off, const HyDotTerms &tm, const std::vector<size_t> &sw,
                            const std::vector<size_t> &idn, size_t L, size_t alpha, size_t B, size_t cb, size_t G, bool *fallback,
                            hipStream_t s)
{
    const size_t n = c->n, ct_words = B * 2 * L * n;
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    const HyDotLayout w = hy_dot_layout(c, L, alpha, cb, G);
    void *wsp;
    MOAI_TRY(workspace(c, w.total, s, &wsp));
    uint32_t *flag = reinterpret_cast<uint32_t *>(at_bytes(wsp, w.flag));
    const HyDotScratch sc = { at_bytes(wsp, w.t), at_bytes(wsp, w.ext), at_bytes(wsp, w.gal), at_bytes(wsp, w.acc) };
    uint64_t *S = at_bytes(wsp, w.S), *x = at_bytes(wsp, w.x), *conv = at_bytes(wsp, w.conv), *add = at_bytes(wsp, w.add);
    if (!sw.empty())
    {
        // steps 1-3 on the UNPERMUTED c1, once for all rotations and outputs
        MOAI_TRY(hy_decompose(c, tab, { in, 2 * L, L }, L, alpha, B, sc.t, sc.ext, s));
        MOAI_TRY(probe_any_zero(c, sc.t, B * L * n, flag, s, fallback)); // a zero coefficient: the identity does not hold for it
    }
    MOAI_TRY(for_chunks(sw.size(), G, [&](size_t g0, size_t ng) {
        const size_t *gs = sw.data() + g0;
        HyDotOutputs o{};
        o.S = S;
        o.add = add;
        o.ng = (uint32_t)ng;
        MOAI_TRY(hy_dot_inner(c, tab, in, tm, gs, ng, o, sc, L, alpha, B, *fallback, s));
        // step 5 once per output, over (output, ciphertext) pairs
        MOAI_TRY(hy_mod_down(c, tab, S, x, conv, L, alpha, ng * B, s));
        for (size_t h = 0; h < ng; ++h)
        {
            MOAI_TRY(moddown_finalize(c, S + h * B * 2 * (L + alpha) * n, (uint32_t)(L + alpha), conv + h * ct_words, tm.outs[gs[h]] + out_off,
                                      2 * B, L, tab->pinv, { add + h * ct_words, 2 * L, 1 }, nullptr, s));
        }
        return MOAI_OK;
    }));
    // outputs of identity terms only: no step 5, the sum is formed in the output itself
    for (size_t g : idn)
    {
        HyDotOutputs o{};
        o.add = tm.outs[g] + out_off;
        o.ng = 1;
        MOAI_HIP_CHECK(hipMemsetAsync(o.add, 0, ct_words * sizeof(uint64_t), s));
        for (size_t r = 0; r < tm.R; ++r)
        {
            if (tm.plains[g * tm.R + r])
            {
                MOAI_TRY(hy_dot_term(c, nullptr, in, o, tm, &g, 1, r, L, alpha, B, s));
            }
        }
    }
    return MOAI_OK;
}

// ---- giant steps summed in the extended basis --------------------------------------------------------------------------------------
// rows of N words of scratch: per ciphertext the inner stage's shared rows, the sum Z and the special rows and conv of its step 5; per
// (giant step in flight, ciphertext) S and the addend, the special rows and conv of c1', the permuted c1' and its t and digits
static inline size_t hy_bsgs_shared_rows(size_t L, size_t alpha)
{
    return hy_dot_shared_rows(L, alpha) + 2 * (L + alpha) + 2 * alpha + 2 * L;
}

static inline size_t hy_bsgs_giant_rows(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * L + alpha + L + L + hy_beta(L, alpha) * (L + alpha);
}

struct HyBsgsLayout
{
    size_t flag, t, ext, gal, acc, Z, zx, zconv, S, add, x, conv, tgt, t2, ext2, total; // byte offsets
};

static HyBsgsLayout hy_bsgs_layout(const moai_ctx *c, size_t L, size_t alpha, size_t cb, size_t G)
{
    const size_t row = c->n * sizeof(uint64_t), beta = hy_beta(L, alpha);
    HyBsgsLayout w;
    w.flag = 0;
    w.t = 256;
    w.ext = w.t + align256(cb * L * row);
    w.gal = w.ext + align256(cb * (beta * (L + alpha) - L) * row);
    w.acc = w.gal + align256(cb * 2 * L * row);
    w.Z = w.acc + align256(cb * 2 * (L + alpha) * row);
    w.zx = w.Z + align256(cb * 2 * (L + alpha) * row);
    w.zconv = w.zx + align256(cb * 2 * alpha * row);
    w.S = w.zconv + align256(cb * 2 * L * row);
    w.add = w.S + align256(G * cb * 2 * (L + alpha) * row);
    w.x = w.add + align256(G * cb * 2 * L * row);
    w.conv = w.x + align256(G * cb * alpha * row);
    w.tgt = w.conv + align256(G * cb * L * row);
    w.t2 = w.tgt + align256(G * cb * L * row);
    w.ext2 = w.t2 + align256(G * cb * L * row);
    w.total = w.ext2 + align256(G * cb * (beta * (L + alpha) - L) * row);
    return w;
}

// ciphertexts per chunk (*cb) and giant steps in flight (*G) under MOAI_HYBRID_TMP_KB.  A group of giant steps repeats the inner
// stage's MAC over every baby step it uses while a batch chunk repeats nothing, so the giant steps come first: all of them (at most
// HY_DOT_MAX_NG) are in flight when one ciphertext fits beside them, and cb is the largest count that fits with them; else one
// ciphertext per chunk with as many giant steps as fit, at least one.  No row-per-workgroup grid above 65535 (the transforms run over
// cb * G polynomials of at most 2 (L + alpha) rows), and the chunks of a batch are evened out.
static void hy_bsgs_chunk(const moai_ctx *c, size_t L, size_t alpha, size_t batch, size_t n_giant, size_t *cb_out, size_t *G_out)
{
    const size_t budget = (size_t)std::max(1l, tuning(K_HYBRID_TMP_KB)) << 10, row = c->n * sizeof(uint64_t);
    const size_t shared = hy_bsgs_shared_rows(L, alpha) * row, giant = hy_bsgs_giant_rows(L, alpha) * row;
    const size_t cap = 65535 / (2 * (L + alpha));
    size_t G = std::min(std::min(n_giant, (size_t)HY_DOT_MAX_NG), cap);
    size_t cb = budget / (shared + G * giant);
    if (cb < 1)
    {
        cb = 1;
        G = budget > shared ? (budget - shared) / giant : 0;
        G = G < 1 ? 1 : G;
    }
    cb = cb > cap / G ? cap / G : cb;
    cb = cb < batch ? cb : batch;
    const size_t chunks = (batch + cb - 1) / cb;
    *cb_out = (batch + chunks - 1) / chunks;
    *G_out = G;
}

struct HyBsgsGiants
{
    size_t n;
    const uint32_t *elts;
    const uint32_t *const *tables; // null where the element is 1
    const uint64_t *const *keys;
    const std::vector<char> *switched; // giant step g's inner sum has a term whose baby element is not 1
};

// one chunk of B ciphertexts at `in` [B][2][L][N] into out [B][2][L][N]; tm holds the baby terms with one output per giant step
// (tm.outs unused), G giant steps in flight.  *fallback as in hy_dot_chunk_run: the inner stage's zero probe.
static int hy_bsgs_chunk_run(moai_ctx *c, const uint64_t *in, uint64_t *out, const HyDotTerms &tm, const HyBsgsGiants &gi, bool any_switched,
                             size_t L, size_t alpha, size_t B, size_t cb, size_t G, bool *fallback, hipStream_t s)
{
    const size_t n = c->n, s_words = B * 2 * (L + alpha) * n;
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    const HyBsgsLayout w = hy_bsgs_layout(c, L, alpha, cb, G);
    void *wsp;
    MOAI_TRY(workspace(c, w.total, s, &wsp));
    uint32_t *flag = reinterpret_cast<uint32_t *>(at_bytes(wsp, w.flag));
    const HyDotScratch sc = { at_bytes(wsp, w.t), at_bytes(wsp, w.ext), at_bytes(wsp, w.gal), at_bytes(wsp, w.acc) };
    uint64_t *Z = at_bytes(wsp, w.Z), *zx = at_bytes(wsp, w.zx), *zconv = at_bytes(wsp, w.zconv);
    uint64_t *S = at_bytes(wsp, w.S), *add = at_bytes(wsp, w.add), *x = at_bytes(wsp, w.x), *conv = at_bytes(wsp, w.conv);
    uint64_t *tgt = at_bytes(wsp, w.tgt), *t2 = at_bytes(wsp, w.t2), *ext2 = at_bytes(wsp, w.ext2);
    if (any_switched)
    {
        // steps 1-3 on the UNPERMUTED c1, once for all baby steps and giant steps
        MOAI_TRY(hy_decompose(c, tab, { in, 2 * L, L }, L, alpha, B, sc.t, sc.ext, s));
        MOAI_TRY(probe_any_zero(c, sc.t, B * L * n, flag, s, fallback)); // a zero coefficient: the identity does not hold for it
    }
    HyBsgsMacArgs m{};
    m.ext = ext2;
    m.tgt = tgt;
    m.S = S;
    m.add = add;
    m.Z = Z;
    m.d = hy_dims(c, L, alpha);
    uint32_t special[HY_MAX_ALPHA];
    for (size_t t = 0; t < alpha; ++t)
    {
        special[t] = (uint32_t)(c->k - alpha + t);
    }
    for (size_t i = 0; i < L; ++i)
    {
        m.fac[i] = hy_prod_mod(c, special, alpha, alpha, c->primes[i]);
    }
    dim3 grid;
    MOAI_TRY(hy_mac_grid(c, B, L + alpha, &grid));
    MOAI_TRY(for_chunks(gi.n, G, [&](size_t g0, size_t ng) {
        // the group's giant steps in the order the kernels index them: rotated ones whose c1' takes a mod-down, rotated ones whose
        // inner sum has no switched term, then those of element 1 (a sum of canonical residues does not depend on the order)
        std::vector<size_t> gs;
        size_t n_md = 0, n_rot = 0;
        for (int cls = 0; cls < 3; ++cls)
        {
            for (size_t g = g0; g < g0 + ng; ++g)
            {
                const int is = gi.elts[g] == 1 ? 2 : ((*gi.switched)[g] ? 0 : 1);
                if (is == cls)
                {
                    gs.push_back(g);
                }
            }
            n_md = cls == 0 ? gs.size() : n_md;
            n_rot = cls == 1 ? gs.size() : n_rot;
        }
        HyDotOutputs o{};
        o.S = S;
        o.add = add;
        o.ng = (uint32_t)ng;
        MOAI_TRY(hy_dot_inner(c, tab, in, tm, gs.data(), ng, o, sc, L, alpha, B, *fallback, s));
        for (size_t h = 0; h < ng; ++h)
        {
            if (!((o.seeded >> h) & 1u))
            {
                MOAI_HIP_CHECK(hipMemsetAsync(S + h * s_words, 0, s_words * sizeof(uint64_t), s)); // no switched term: S_g = 0
            }
        }
        if (n_rot)
        {
            if (n_md)
            {
                // step 5 of S_g[1] alone: the special rows of polynomial 1 of every (giant step, ciphertext) pair
                RowMap rm{};
                hy_rowmap(c, L, alpha, 0, L, &rm);
                MOAI_TRY(ntt_launch(c, x, n_md * B, alpha, rm, true, s, S, 2 * (L + alpha), (L + alpha) + L));
                MOAI_TRY(hy_convert(c, x, alpha, 0, conv, tab->conv + hy_beta(L, alpha), alpha, n_md * B, s));
                MOAI_TRY(make_rowmap(c, L, nullptr, &rm));
                MOAI_TRY(ntt_launch(c, conv, n_md * B, L, rm, false, s));
            }
            // tgt = perm_{E_g}(c1'_g), then steps 1-3 on all (giant step, ciphertext) pairs at once
            HyC1Args a{};
            a.S = S;
            a.conv = conv;
            a.add = add;
            a.tgt = tgt;
            a.pinv = tab->pinv;
            a.n_md = (uint32_t)n_md;
            a.B = (uint32_t)B;
            a.d = m.d;
            for (size_t h = 0; h < n_rot; ++h)
            {
                a.table[h] = m.table[h] = gi.tables[gs[h]];
                m.key[h] = gi.keys[gs[h]];
            }
            MOAI_TRY(launch_rows(hy_c1_moddown_permute_kernel, c, n_rot * B * L, s, a));
            MOAI_TRY(hy_decompose(c, tab, { tgt, L, 0 }, L, alpha, n_rot * B, t2, ext2, s));
        }
        m.n_rot = (uint32_t)n_rot;
        m.ng = (uint32_t)ng;
        m.zseeded = g0 ? 1u : 0u;
        hipLaunchKernelGGL(hy_bsgs_mac_kernel, grid, dim3(256), 0, s, m);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    }));
    // the one final step 5, both polynomials, no addend
    MOAI_TRY(hy_mod_down(c, tab, Z, zx, zconv, L, alpha, B, s));
    return moddown_finalize(c, Z, (uint32_t)(L + alpha), zconv, out, 2 * B, L, tab->pinv, {}, nullptr, s);
}

// ---- relinearize + rescale --------------------------------------------------------------------------------------------------------
// the merged mod-down's constants share the context's map with hy_table's blocks: the same (L, alpha) with this bit in alpha
constexpr size_t HY_RESCALE_KEY = (size_t)1 << 32;

// the device block of the merged mod-down's constants for (L, alpha), L >= 2 and alpha + 1 <= HY_MAX_ALPHA; the caller holds
// op_mutex.  Built on first use with a blocking copy, as hy_table.
static int hy_rescale_table(moai_ctx *c, size_t L, size_t alpha, const HyRescaleTable **out)
{
    const auto key = std::make_pair(L, alpha | HY_RESCALE_KEY);
    auto it = c->hybrid_tables.find(key);
    if (it != c->hybrid_tables.end())
    {
        *out = static_cast<const HyRescaleTable *>(it->second);
        return MOAI_OK;
    }
    std::vector<unsigned char> host(sizeof(HyRescaleTable), 0);
    HyRescaleTable *t = reinterpret_cast<HyRescaleTable *>(host.data());
    HyConv &cv = t->conv;
    const size_t k = c->k, last = L - 1;
    cv.nsrc = (uint32_t)(alpha + 1);
    cv.ntgt = (uint32_t)last;
    cv.src_prime[0] = (uint32_t)last;
    for (size_t s = 0; s < alpha; ++s)
    {
        cv.src_prime[1 + s] = (uint32_t)(k - alpha + s);
    }
    for (size_t r = 0; r < cv.nsrc; ++r)
    {
        const uint64_t m = c->primes[cv.src_prime[r]];
        cv.src_inv[r] = make_tw(hy_invmod(hy_prod_mod(c, cv.src_prime, cv.nsrc, r, m), m), m);
        cv.src_pre[r] = hy_half_mod(0, m);
    }
    for (size_t i = 0; i < last; ++i)
    {
        const uint64_t q = c->primes[i];
        const uint64_t w_mod_q = hy_prod_mod(c, cv.src_prime, cv.nsrc, cv.nsrc, q);
        cv.tgt_prime[i] = (uint32_t)i;
        cv.tgt_post[i] = hy_half_mod(w_mod_q, q);
        for (size_t r = 0; r < cv.nsrc; ++r)
        {
            cv.w[i][r] = hy_prod_mod(c, cv.src_prime, cv.nsrc, r, q);
        }
        t->winv[i] = make_tw(hy_invmod(w_mod_q, q), q);
        t->qinv[i] = make_tw(hy_invmod(c->primes[last] % q, q), q);
    }
    void *dev = nullptr;
    MOAI_HIP_CHECK(hipMalloc(&dev, host.size()));
    hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        (void)hipFree(dev);
        return set_error(MOAI_EHIP, "hybrid relinearize-rescale constants: %s", hipGetErrorString(e));
    }
    c->hybrid_tables[key] = dev;
    *out = static_cast<const HyRescaleTable *>(dev);
    return MOAI_OK;
}

// rows of N words of scratch per ciphertext: t, the converted digits, acc, the alpha + 1 source rows of the merged mod-down, conv
// over L - 1 rows, and head_rows rows in front of them (3 L: the three-polynomial product of moai_multiply_relin_rescale_hybrid;
// L: the gathered third polynomial of a member of the list form; 0 otherwise)
static size_t hy_rescale_rows_per_ct(size_t L, size_t alpha, size_t head_rows)
{
    const size_t beta = hy_beta(L, alpha);
    return head_rows + L + (beta * (L + alpha) - L) + 2 * (L + alpha) + 2 * (alpha + 1) + 2 * (L - 1);
}

struct HyRescaleLayout
{
    size_t prod, t, ext, acc, x, conv, total; // byte offsets
};

static HyRescaleLayout hy_rescale_layout(const moai_ctx *c, size_t L, size_t alpha, size_t cb, size_t head_rows)
{
    const size_t row = c->n * sizeof(uint64_t), beta = hy_beta(L, alpha);
    HyRescaleLayout w;
    w.prod = 0;
    w.t = w.prod + align256(cb * head_rows * row);
    w.ext = w.t + align256(cb * L * row);
    w.acc = w.ext + align256(cb * (beta * (L + alpha) - L) * row);
    w.x = w.acc + align256(cb * 2 * (L + alpha) * row);
    w.conv = w.x + align256(cb * 2 * (alpha + 1) * row);
    w.total = w.conv + align256(cb * 2 * (L - 1) * row);
    return w;
}

// ciphertexts per chunk: as many as MOAI_HYBRID_TMP_KB holds, at least one; no row-per-workgroup grid above 65535 (the widest runs
// over 3 * cb * L rows with the product, 2 * cb * (L + alpha) without)
static size_t hy_rescale_chunk(const moai_ctx *c, size_t L, size_t alpha, size_t batch, size_t head_rows)
{
    const size_t budget = (size_t)std::max(1l, tuning(K_HYBRID_TMP_KB)) << 10;
    const size_t per = hy_rescale_rows_per_ct(L, alpha, head_rows) * c->n * sizeof(uint64_t);
    size_t cb = budget / per;
    cb = cb < 1 ? 1 : cb;
    const size_t cap = 65535 / std::max(2 * (L + alpha), 3 * L);
    cb = cb > cap ? cap : cb;
    return cb < batch ? cb : batch;
}

// one chunk of B ciphertexts: out [B][2][L - 1][N] = the merged mod-down of (c0, c1) + switch(c2) for ct3 [B][3][L][N].  With lst (a
// device record, common.h KsList) c2 [B][L][N] has been gathered to w.gal, c0 and c1 are read from lst->ins[b], the key is
// lst->keys[b] and the result goes to lst->outs[b]; ct3, key and out are not used
static int hy_rescale_chunk_run(moai_ctx *c, const HyTable *tab, const HyRescaleTable *rt, const uint64_t *ct3, const uint64_t *key,
                                uint64_t *out, size_t L, size_t alpha, size_t B, void *wsp, const HyRescaleLayout &w, hipStream_t s,
                                const KsList *lst = nullptr)
{
    uint64_t *t = at_bytes(wsp, w.t), *ext = at_bytes(wsp, w.ext), *acc = at_bytes(wsp, w.acc), *x = at_bytes(wsp, w.x);
    uint64_t *conv = at_bytes(wsp, w.conv);
    // steps 1-4 on c2, as every switch
    const KsTarget tg = lst ? KsTarget{ at_bytes(wsp, w.prod), L, 0 } : KsTarget{ ct3, 3 * L, 2 * L };
    MOAI_TRY(hy_decompose(c, tab, tg, L, alpha, B, t, ext, s));
    HyMacArgs m;
    m.ext = ext;
    m.tgt = tg.ptr;
    m.key = key;
    m.acc = acc;
    m.tgt_stride = (uint32_t)tg.stride_rows;
    m.tgt_off = (uint32_t)tg.off_rows;
    m.d = hy_dims(c, L, alpha);
    MOAI_TRY(hy_mac(c, m, B, lst, s));
    // the lift of the one data row among the sources (the rows below it take theirs in the last kernel)
    HyLiftArgs lf;
    lf.acc = acc;
    lf.ct3 = ct3;
    lf.d = m.d;
    uint32_t special[HY_MAX_ALPHA];
    for (size_t sp = 0; sp < alpha; ++sp)
    {
        special[sp] = (uint32_t)(c->k - alpha + sp);
    }
    lf.plast = hy_prod_mod(c, special, alpha, alpha, c->primes[L - 1]);
    MOAI_TRY(plain_or_list<HyLiftListArgs>(lf, lst, [&](const auto &args, auto LIST) {
        return launch_rows(hy_lift_last_row_kernel<decltype(LIST)::value>, c, 2 * B, s, args);
    }));
    // the merged mod-down: x = INTT(rows L-1 .. L+alpha-1 of acc, contiguous), conv = NTT(base conversion with W's rounding terms)
    RowMap rm{};
    hy_rowmap(c, L, alpha, 0, L - 1, &rm);
    MOAI_TRY(ntt_launch(c, x, 2 * B, alpha + 1, rm, true, s, acc, L + alpha, L - 1));
    MOAI_TRY(hy_convert(c, x, alpha + 1, 0, conv, &rt->conv, alpha + 1, 2 * B, s));
    MOAI_TRY(make_rowmap(c, L - 1, nullptr, &rm));
    MOAI_TRY(ntt_launch(c, conv, 2 * B, L - 1, rm, false, s));
    HyRescaleFinalArgs f;
    f.acc = acc;
    f.conv = conv;
    f.ct3 = ct3;
    f.out = out;
    f.winv = rt->winv; // device address arithmetic only
    f.qinv = rt->qinv;
    f.d = m.d;
    return plain_or_list<HyRescaleFinalListArgs>(f, lst, [&](const auto &args, auto LIST) {
        return launch_rows(hy_rescale_finalize_kernel<decltype(LIST)::value>, c, 2 * B * (L - 1), s, args);
    });
}

// what the merged forms refuse: what needs no context first, in hy_check's order (alpha = 0 and L = 0 are its own)
static int hy_rescale_check(const moai_ctx *c, size_t alpha, size_t L)
{
    if (alpha != 0 && L == 1)
    {
        return set_error(MOAI_EINVAL, "L = 1: no prime left to rescale to");
    }
    if (alpha == HY_MAX_ALPHA && L != 0)
    {
        return set_error(MOAI_EINVAL, "alpha = %zu: the merged mod-down converts alpha + 1 residues, at most %u", alpha, HY_MAX_ALPHA);
    }
    return hy_check(c, alpha, L, true);
}

// the two entry points: validated, then chunk by chunk on the stream's workspace
//   y null:  x = ct3 [batch][3][L][N]
//   y set:   x, y [batch][2][L][N] (y may be x); their product lives in the chunk's workspace
static int hy_rescale_entry(moai_ctx *c, const uint64_t *x, const uint64_t *y, bool product, const uint64_t *key, uint64_t *out, size_t L,
                            size_t alpha, size_t batch, void *stream)
{
    MOAI_TRY(hy_rescale_check(c, alpha, L));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (!x || (product && !y) || !key || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t n = c->n, row = n * sizeof(uint64_t);
    const size_t out_bytes = batch * 2 * (L - 1) * row, in_bytes = batch * (product ? 2 : 3) * L * row;
    const size_t key_bytes = hy_beta(c->k - alpha, alpha) * 2 * c->k * row;
    if (overlap(out, out_bytes, x, in_bytes) || (product && overlap(out, out_bytes, y, in_bytes)) || overlap(out, out_bytes, key, key_bytes))
    {
        return set_error(MOAI_EINVAL, "the output must not overlap an input");
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    const HyRescaleTable *rt;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    MOAI_TRY(hy_rescale_table(c, L, alpha, &rt));
    const size_t cb = hy_rescale_chunk(c, L, alpha, batch, product ? 3 * L : 0);
    const HyRescaleLayout w = hy_rescale_layout(c, L, alpha, cb, product ? 3 * L : 0);
    void *wsp;
    MOAI_TRY(workspace(c, w.total, s, &wsp));
    return for_chunks(batch, cb, [&](size_t b0, size_t B) {
        const uint64_t *ct3 = x + b0 * 3 * L * n;
        if (product)
        {
            HyProductArgs g;
            g.x = x + b0 * 2 * L * n;
            g.y = y + b0 * 2 * L * n;
            g.out = at_bytes(wsp, w.prod);
            fill_rows(g, c, L);
            MOAI_TRY(launch_rows(hy_ct_product_kernel, c, B * L, s, g));
            ct3 = g.out;
        }
        return hy_rescale_chunk_run(c, tab, rt, ct3, key, out + b0 * 2 * (L - 1) * n, L, alpha, B, wsp, w, s);
    });
}

// ---- the switches on a list of ciphertexts, each in its own block (and, for the rotation, with its own key and element) ------------
enum
{
    HY_LIST_GALOIS,
    HY_LIST_RELIN,
    HY_LIST_RESCALE
};

// What the three list entry points share; the n single calls at batch 1 in one chain of launches per pass.
//   HY_LIST_GALOIS   member i is [2][L][N] and gets apply_galois by elts[i] with keys[i], plus sums[i]; outs[i] [2][L][N]
//   HY_LIST_RELIN    member i is [3][L][N]; outs[i] [2][L][N] = (c0, c1) + switch(c2) with one_key
//   HY_LIST_RESCALE  the same through the merged mod-down; outs[i] [2][L - 1][N]
// Everything is validated before anything is enqueued (the context-free part and the overlaps are keyswitch.hip's own checks).  A
// pass takes min(KS_LIST_MAX, the chunk MOAI_HYBRID_TMP_KB allows) members: its record goes to the device as a kernel argument,
// galois_gather_list permutes the members (or, with the identity table, collects their third polynomials) into the chunk's
// contiguous scratch, steps 1-3 and the mod-down's transforms run on that scratch as they do for a batch, and the MAC and the last
// kernels take the member's key, addends and output from the record.
static int hy_ptrs_impl(moai_ctx *c, int kind, const uint64_t *const *ins, uint64_t *const *outs, size_t L, size_t alpha,
                        const uint32_t *elts, const uint64_t *const *keys, const uint64_t *one_key, const uint64_t *const *sums, size_t n,
                        void *stream)
{
    const bool relin = kind != HY_LIST_GALOIS, rescale = kind == HY_LIST_RESCALE;
    if (n == 0)
    {
        return MOAI_OK;
    }
    MOAI_TRY(ks_list_check_members(ins, outs, elts, keys, one_key, n, relin));
    MOAI_TRY(rescale ? hy_rescale_check(c, alpha, L) : hy_check(c, alpha, L, true));
    const size_t row = c->n * sizeof(uint64_t), Lout = rescale ? L - 1 : L;
    MOAI_TRY(ks_list_check_blocks(c, ins, outs, elts, sums, n, (relin ? 3 : 2) * L * row, 2 * Lout * row, relin));
    MOAI_TRY(enter_device(c));
    std::vector<const uint32_t *> tables(n);
    for (size_t i = 0; i < n; ++i)
    {
        // relinearize: element 1, the identity permutation -- the gather then only collects the third polynomials
        MOAI_TRY(galois_table(c, relin ? 1u : elts[i], &tables[i]));
    }
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    const HyRescaleTable *rt = nullptr;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    if (rescale)
    {
        MOAI_TRY(hy_rescale_table(c, L, alpha, &rt));
    }
    const size_t gal_rows = relin ? L : 2 * L; // rows per member of the gathered target
    const size_t nb = std::min(KS_LIST_MAX, rescale ? hy_rescale_chunk(c, L, alpha, n, gal_rows) : hy_chunk(c, L, alpha, n, gal_rows));
    HyLayout w{};
    HyRescaleLayout wr{};
    if (rescale)
    {
        wr = hy_rescale_layout(c, L, alpha, nb, gal_rows);
    }
    else
    {
        w = hy_layout(c, L, alpha, nb, gal_rows);
    }
    const size_t sz_list = align256(sizeof(KsList));
    void *wsp;
    MOAI_TRY(workspace(c, sz_list + (rescale ? wr.total : w.total), s, &wsp));
    KsList *dlist = static_cast<KsList *>(wsp);
    void *chunk = at_bytes(wsp, sz_list);
    return for_chunks(n, nb, [&](size_t m0, size_t cnt) {
        KsList h;
        for (size_t e = 0; e < KS_LIST_MAX; ++e)
        {
            const size_t i = m0 + (e < cnt ? e : 0); // the unused entries repeat the pass's first member
            h.ins[e] = ins[i];
            h.outs[e] = outs[i];
            h.sums[e] = sums ? sums[i] : nullptr;
            h.keys[e] = relin ? one_key : keys[i];
            h.tables[e] = tables[i];
            h.key_rows[e] = (uint32_t)c->k; // the whole layout
        }
        MOAI_TRY(ks_list_write(h, dlist, s));
        uint64_t *tmp = at_bytes(chunk, rescale ? wr.prod : w.gal);
        switch (kind)
        {
        case HY_LIST_GALOIS:
            // tmp [cnt][2][L][N] = galois(ins); out = (galois(in0), 0) + switch(galois(in1)) [+ sum]   (evaluator.cpp:2631-2654)
            MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, 2 * L, 0, s));
            return hy_switch_chunk(c, tab, nullptr, { tmp, 2 * L, L, dlist }, nullptr, L, alpha, cnt, chunk, w, { tmp, 2 * L, 2 }, s);
        case HY_LIST_RELIN:
            // tmp [cnt][L][N] = the members' third polynomials; out = (c0, c1) + switch(c2)   (evaluator.cpp:1383-1392)
            MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, L, 2 * L, s));
            return hy_switch_chunk(c, tab, nullptr, { tmp, L, 0, dlist }, nullptr, L, alpha, cnt, chunk, w, { nullptr, 0, 1 }, s);
        default:
            MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, L, 2 * L, s));
            return hy_rescale_chunk_run(c, tab, rt, nullptr, nullptr, nullptr, L, alpha, cnt, chunk, wr, s, dlist);
        }
    });
}

} // namespace moai

using namespace moai;

extern "C" size_t moai_hybrid_digits(const moai_ctx *c, size_t alpha, size_t L)
{
    if (hy_check(c, alpha, L, true))
    {
        return 0;
    }
    return hy_beta(L, alpha);
}

extern "C" int moai_hybrid_keygen(moai_ctx *c, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, const uint64_t *new_key_ntt,
                                  size_t alpha, uint64_t *out, void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, new_key_ntt, out);
    MOAI_TRY(hy_check(c, alpha, 0, false));
    const size_t k = c->k, Lmax = k - alpha, digits = hy_beta(Lmax, alpha);
    trace_op("hybrid_keygen", k, digits);
    if (!key)
    {
        return set_error(MOAI_EINVAL, "null key");
    }
    if (!sk_ntt || !new_key_ntt || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    // digit j = Enc_s(0) over all k rows with sequence seq + j (validates the sequence range before it enqueues)
    MOAI_TRY(encrypt_zero_key_level(c, key, seq, sk_ntt, out, digits, (hipStream_t)stream));
    HyKeyAddArgs a;
    a.key = out;
    a.newkey = new_key_ntt;
    a.d = hy_dims(c, Lmax, alpha);
    uint32_t special[HY_MAX_ALPHA];
    for (size_t s = 0; s < alpha; ++s)
    {
        special[s] = (uint32_t)(k - alpha + s);
    }
    for (size_t r = 0; r < MOAI_MAX_RNS; ++r)
    {
        a.fac[r] = r < Lmax ? hy_prod_mod(c, special, alpha, alpha, c->primes[r]) : 0;
    }
    return launch_rows(hy_key_add_kernel, c, Lmax, stream, a);
}

extern "C" int moai_switch_key_hybrid(moai_ctx *c, uint64_t *ct, const uint64_t *target, const uint64_t *key, size_t L, size_t alpha,
                                      size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct, target, key);
    trace_op("switch_key_hybrid", L, batch);
    return hy_entry(c, HY_SWITCH, ct, target, key, L, alpha, 1, batch, stream);
}

extern "C" int moai_relinearize_hybrid(moai_ctx *c, const uint64_t *ct3, const uint64_t *key, uint64_t *out, size_t L, size_t alpha,
                                       size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct3, key, out);
    trace_op("relinearize_hybrid", L, batch);
    return hy_entry(c, HY_RELIN, out, ct3, key, L, alpha, 1, batch, stream);
}

extern "C" int moai_apply_galois_hybrid(moai_ctx *c, uint64_t *ct, size_t L, size_t alpha, uint32_t galois_elt, const uint64_t *key,
                                        size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct, key);
    trace_op("apply_galois_hybrid", L, batch);
    return hy_entry(c, HY_GALOIS, ct, ct, key, L, alpha, galois_elt, batch, stream);
}

extern "C" int moai_apply_galois_hybrid_to(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t L, size_t alpha, uint32_t galois_elt,
                                           const uint64_t *key, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, out, key);
    trace_op("apply_galois_hybrid", L, batch);
    return hy_entry(c, HY_GALOIS, out, in, key, L, alpha, galois_elt, batch, stream);
}

extern "C" int moai_apply_galois_hybrid_acc(moai_ctx *c, const uint64_t *in, uint64_t *acc, size_t L, size_t alpha, uint32_t galois_elt,
                                            const uint64_t *key, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, acc, key);
    trace_op("apply_galois_hybrid", L, batch); // the same switch; the addition that follows it is what is saved
    return hy_entry(c, HY_GALOIS, acc, in, key, L, alpha, galois_elt, batch, stream, acc);
}

extern "C" int moai_apply_galois_hybrid_ptrs(moai_ctx *c, const uint64_t *const *ins, uint64_t *const *outs, size_t L, size_t alpha,
                                             const uint32_t *galois_elts, const uint64_t *const *keys, const uint64_t *const *sums, size_t n,
                                             void *stream)
{
    for (size_t i = 0; ins && outs && keys && i < n; ++i)
    {
        MOAI_AUDIT(stream, ins[i], outs[i], keys[i], sums ? sums[i] : nullptr);
    }
    trace_op("apply_galois_hybrid", L, n); // the calls it replaces
    return hy_ptrs_impl(c, HY_LIST_GALOIS, ins, outs, L, alpha, galois_elts, keys, nullptr, sums, n, stream);
}

extern "C" int moai_relinearize_hybrid_ptrs(moai_ctx *c, const uint64_t *const *ct3s, uint64_t *const *outs, const uint64_t *key, size_t L,
                                            size_t alpha, size_t n, void *stream)
{
    MOAI_AUDIT(stream, key);
    for (size_t i = 0; ct3s && outs && i < n; ++i)
    {
        MOAI_AUDIT(stream, ct3s[i], outs[i]);
    }
    trace_op("relinearize_hybrid", L, n);
    return hy_ptrs_impl(c, HY_LIST_RELIN, ct3s, outs, L, alpha, nullptr, nullptr, key, nullptr, n, stream);
}

extern "C" int moai_hybrid_hoist_correction(moai_ctx *c, const uint64_t *key, uint32_t galois_elt, size_t L, size_t alpha,
                                            uint64_t *correction, void *stream)
{
    MOAI_AUDIT(stream, key, correction);
    trace_op("hybrid_hoist_correction", L, 1);
    MOAI_TRY(galois_elt_check(nullptr, galois_elt)); // oddness first: it needs no context
    MOAI_TRY(hy_check(c, alpha, L, true));
    MOAI_TRY(galois_elt_check(c, galois_elt));
    if (!key || !correction)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    MOAI_TRY(enter_device(c));
    return hy_hoist_correction(c, key, galois_elt, L, alpha, correction, (hipStream_t)stream);
}

extern "C" int moai_apply_galois_hybrid_hoisted(moai_ctx *c, const uint64_t *in, uint64_t *const *outs, size_t L, size_t alpha,
                                                const uint32_t *galois_elts, const uint64_t *const *keys,
                                                const uint64_t *const *corrections, size_t R, size_t batch, int *used_fallback, void *stream)
{
    MOAI_AUDIT(stream, in);
    for (size_t r = 0; outs && keys && corrections && r < R; ++r)
    {
        MOAI_AUDIT(stream, outs[r], keys[r], corrections[r]);
    }
    trace_op("apply_galois_hybrid_hoisted", L, batch * R);
    if (used_fallback)
    {
        *used_fallback = 0;
    }
    MOAI_TRY(hy_check(c, alpha, L, true));
    if (batch == 0 || R == 0)
    {
        return MOAI_OK;
    }
    if (!in || !outs || !galois_elts || !keys || !corrections)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t n = c->n, ct_bytes = batch * 2 * L * n * sizeof(uint64_t);
    for (size_t r = 0; r < R; ++r)
    {
        if (!keys[r] || !corrections[r] || !outs[r])
        {
            return set_error(MOAI_EINVAL, "null key, correction or output");
        }
        MOAI_TRY(galois_elt_check(c, galois_elts[r]));
        if (overlap(outs[r], ct_bytes, in, ct_bytes))
        {
            return set_error(MOAI_EINVAL, "an output must not alias the input");
        }
        for (size_t q = 0; q < r; ++q)
        {
            if (overlap(outs[r], ct_bytes, outs[q], ct_bytes))
            {
                return set_error(MOAI_EINVAL, "an output must not alias another output");
            }
        }
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::vector<const uint32_t *> tables(R);
    for (size_t r = 0; r < R; ++r)
    {
        MOAI_TRY(galois_table(c, galois_elts[r], &tables[r])); // built before the first launch of the call
    }
    const HyHoistRotations rot = { R, galois_elts, tables.data(), keys, corrections, outs };
    size_t cb, G;
    hy_hoist_chunk(c, L, alpha, batch, R, &cb, &G);
    return for_chunks(batch, cb, [&](size_t b0, size_t B) {
        const size_t off = b0 * 2 * L * n;
        bool fallback = false;
        MOAI_TRY(hy_hoist_chunk_run(c, in + off, off, rot, L, alpha, B, cb, G, &fallback, s));
        if (fallback)
        {
            // the separate rotations of this chunk, each on a copy of the input (they take the lock and the workspace themselves)
            if (used_fallback)
            {
                *used_fallback = 1;
            }
            for (size_t r = 0; r < R; ++r)
            {
                MOAI_HIP_CHECK(hipMemcpyAsync(outs[r] + off, in + off, B * 2 * L * n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
                MOAI_TRY(hy_entry(c, HY_GALOIS, outs[r] + off, outs[r] + off, keys[r], L, alpha, galois_elts[r], B, stream));
            }
        }
        return MOAI_OK;
    });
}

extern "C" int moai_hybrid_rotate_pt_dot(moai_ctx *c, const uint64_t *in, uint64_t *const *outs, size_t n_out, size_t L, size_t alpha,
                                         const uint32_t *galois_elts, const uint64_t *const *keys, const uint64_t *const *corrections,
                                         size_t R, const uint64_t *const *plains, size_t batch, int *used_fallback, void *stream)
{
    MOAI_AUDIT(stream, in);
    for (size_t g = 0; outs && g < n_out; ++g)
    {
        MOAI_AUDIT(stream, outs[g]);
    }
    trace_op("hybrid_rotate_pt_dot", L, batch * n_out);
    if (used_fallback)
    {
        *used_fallback = 0;
    }
    for (size_t r = 0; galois_elts && r < R; ++r)
    {
        MOAI_TRY(galois_elt_check(nullptr, galois_elts[r])); // oddness first: it needs no context
    }
    MOAI_TRY(hy_check(c, alpha, L, true));
    if (batch == 0 || n_out == 0)
    {
        return MOAI_OK;
    }
    if (!in || !outs || !plains || (R && (!galois_elts || !keys || !corrections)))
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t n = c->n, ct_bytes = batch * 2 * L * n * sizeof(uint64_t);
    for (size_t r = 0; r < R; ++r)
    {
        MOAI_TRY(galois_elt_check(c, galois_elts[r]));
        if (galois_elts[r] != 1 && (!keys[r] || !corrections[r]))
        {
            return set_error(MOAI_EINVAL, "null key or correction of rotation %zu", r);
        }
    }
    std::vector<size_t> sw, idn; // outputs with and without a term that is switched
    for (size_t g = 0; g < n_out; ++g)
    {
        if (!outs[g])
        {
            return set_error(MOAI_EINVAL, "null output");
        }
        if (overlap(outs[g], ct_bytes, in, ct_bytes))
        {
            return set_error(MOAI_EINVAL, "an output must not alias the input");
        }
        for (size_t q = 0; q < g; ++q)
        {
            if (overlap(outs[g], ct_bytes, outs[q], ct_bytes))
            {
                return set_error(MOAI_EINVAL, "an output must not alias another output");
            }
        }
        bool any = false, switched = false;
        for (size_t r = 0; r < R; ++r)
        {
            if (plains[g * R + r])
            {
                any = true;
                switched = switched || galois_elts[r] != 1;
            }
        }
        if (!any)
        {
            return set_error(MOAI_EINVAL, "output %zu has no term", g);
        }
        (switched ? sw : idn).push_back(g);
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::vector<const uint32_t *> tables(R, nullptr);
    for (size_t r = 0; r < R; ++r)
    {
        if (galois_elts[r] != 1)
        {
            MOAI_TRY(galois_table(c, galois_elts[r], &tables[r])); // built before the first launch of the call
        }
    }
    const HyDotTerms tm = { R, n_out, galois_elts, tables.data(), keys, corrections, plains, outs };
    size_t cb, G;
    hy_dot_chunk(c, L, alpha, batch, std::max<size_t>(sw.size(), 1), &cb, &G);
    return for_chunks(batch, cb, [&](size_t b0, size_t B) {
        const size_t off = b0 * 2 * L * n;
        bool fallback = false;
        MOAI_TRY(hy_dot_chunk_run(c, in + off, off, tm, sw, idn, L, alpha, B, cb, G, &fallback, s));
        if (fallback && used_fallback)
        {
            *used_fallback = 1;
        }
        return MOAI_OK;
    });
}

extern "C" int moai_hybrid_bsgs_dot(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t L, size_t alpha, const uint32_t *baby_elts,
                                    const uint64_t *const *baby_keys, const uint64_t *const *baby_corrections, size_t R,
                                    const uint32_t *giant_elts, const uint64_t *const *giant_keys, size_t n_giant,
                                    const uint64_t *const *plains, size_t batch, int *used_fallback, void *stream)
{
    MOAI_AUDIT(stream, in, out);
    trace_op("hybrid_bsgs_dot", L, batch);
    if (used_fallback)
    {
        *used_fallback = 0;
    }
    for (size_t r = 0; baby_elts && r < R; ++r)
    {
        MOAI_TRY(galois_elt_check(nullptr, baby_elts[r])); // oddness first: it needs no context
    }
    for (size_t g = 0; giant_elts && g < n_giant; ++g)
    {
        MOAI_TRY(galois_elt_check(nullptr, giant_elts[g]));
    }
    MOAI_TRY(hy_check(c, alpha, L, true));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (R == 0 || n_giant == 0)
    {
        return set_error(MOAI_EINVAL, "R = %zu baby steps and %zu giant steps: a sum needs at least one of each", R, n_giant);
    }
    if (!in || !out || !plains || !baby_elts || !baby_keys || !baby_corrections || !giant_elts || !giant_keys)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t n = c->n, ct_bytes = batch * 2 * L * n * sizeof(uint64_t);
    if (overlap(out, ct_bytes, in, ct_bytes))
    {
        return set_error(MOAI_EINVAL, "the output must not alias the input");
    }
    for (size_t r = 0; r < R; ++r)
    {
        MOAI_TRY(galois_elt_check(c, baby_elts[r]));
        if (baby_elts[r] != 1 && (!baby_keys[r] || !baby_corrections[r]))
        {
            return set_error(MOAI_EINVAL, "null key or correction of baby step %zu", r);
        }
    }
    std::vector<char> switched(n_giant, 0); // giant step g's inner sum has a term that is switched
    bool any_switched = false;
    for (size_t g = 0; g < n_giant; ++g)
    {
        MOAI_TRY(galois_elt_check(c, giant_elts[g]));
        if (giant_elts[g] != 1 && !giant_keys[g])
        {
            return set_error(MOAI_EINVAL, "null key of giant step %zu", g);
        }
        bool any = false;
        for (size_t r = 0; r < R; ++r)
        {
            if (plains[g * R + r])
            {
                any = true;
                switched[g] = switched[g] || baby_elts[r] != 1;
            }
        }
        if (!any)
        {
            return set_error(MOAI_EINVAL, "giant step %zu has no term", g);
        }
        any_switched = any_switched || switched[g];
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::vector<const uint32_t *> baby_tables(R, nullptr), giant_tables(n_giant, nullptr);
    for (size_t r = 0; r < R; ++r)
    {
        if (baby_elts[r] != 1)
        {
            MOAI_TRY(galois_table(c, baby_elts[r], &baby_tables[r])); // built before the first launch of the call
        }
    }
    for (size_t g = 0; g < n_giant; ++g)
    {
        if (giant_elts[g] != 1)
        {
            MOAI_TRY(galois_table(c, giant_elts[g], &giant_tables[g]));
        }
    }
    const HyDotTerms tm = { R, n_giant, baby_elts, baby_tables.data(), baby_keys, baby_corrections, plains, nullptr };
    const HyBsgsGiants gi = { n_giant, giant_elts, giant_tables.data(), giant_keys, &switched };
    size_t cb, G;
    hy_bsgs_chunk(c, L, alpha, batch, n_giant, &cb, &G);
    return for_chunks(batch, cb, [&](size_t b0, size_t B) {
        const size_t off = b0 * 2 * L * n;
        bool fallback = false;
        MOAI_TRY(hy_bsgs_chunk_run(c, in + off, out + off, tm, gi, any_switched, L, alpha, B, cb, G, &fallback, s));
        if (fallback && used_fallback)
        {
            *used_fallback = 1;
        }
        return MOAI_OK;
    });
}

extern "C" int moai_relinearize_rescale_hybrid(moai_ctx *c, const uint64_t *ct3, const uint64_t *key, uint64_t *out, size_t L, size_t alpha,
                                               size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct3, key, out);
    trace_op("relinearize_rescale_hybrid", L, batch);
    return hy_rescale_entry(c, ct3, nullptr, false, key, out, L, alpha, batch, stream);
}

extern "C" int moai_relinearize_rescale_hybrid_ptrs(moai_ctx *c, const uint64_t *const *ct3s, uint64_t *const *outs, const uint64_t *key,
                                                    size_t L, size_t alpha, size_t n, void *stream)
{
    MOAI_AUDIT(stream, key);
    for (size_t i = 0; ct3s && outs && i < n; ++i)
    {
        MOAI_AUDIT(stream, ct3s[i], outs[i]);
    }
    trace_op("relinearize_rescale_hybrid", L, n);
    return hy_ptrs_impl(c, HY_LIST_RESCALE, ct3s, outs, L, alpha, nullptr, nullptr, key, nullptr, n, stream);
}

extern "C" int moai_multiply_relin_rescale_hybrid(moai_ctx *c, const uint64_t *x, const uint64_t *y, const uint64_t *key, uint64_t *out,
                                                  size_t L, size_t alpha, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, x, y, key, out);
    trace_op("multiply_relin_rescale_hybrid", L, batch);
    return hy_rescale_entry(c, x, y, true, key, out, L, alpha, batch, stream);
}
