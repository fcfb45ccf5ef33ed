// hybrid_kernels.hip.h -- the argument structs, the constant blocks (HyConv, HyTable, HyRescaleTable) and every kernel of the hybrid
// key switch.  Only hybrid.hip includes it; the chain the kernels form is described at the head of that file.
#pragma once
#include <type_traits>

#include "launch.h"
#include "modarith.hip.h"
#include "ntt_kernels.hip.h"

namespace moai {

// a digit's source rows are held in registers by the conversion kernel; the constants are products of at most this many residues
constexpr uint32_t HY_MAX_ALPHA = 16;

// One fast base conversion: sources r < nsrc under context primes src_prime[r], targets t < ntgt under tgt_prime[t]:
//   y_r = ((x_r + src_pre[r]) mod s_r) * src_inv[r] mod s_r,   out_t = ((sum_r y_r w[t][r]) - tgt_post[t]) mod m_t
// mod-up of digit j: src_pre = tgt_post = 0, src_inv = (D_j / q_r)^-1, w = (D_j / q_r) mod m_t
// mod-down:          src_pre = floor(P / 2) mod p_t, tgt_post = floor(P / 2) mod q_i, src_inv = (P / p_t)^-1, w = (P / p_t) mod q_i
// The exact mod-down (MOAI_HYBRID_ROUND_EXACT) also takes the overflow v of the sum out, out_t = ((sum_r y_r w[t][r]) + v tgt_negw[t]
// - tgt_post[t]) mod m_t: src_rinv[r] = RN(1.0 / (double)s_r), tgt_negw[t] = m_t - (P mod m_t).  Both are filled for every mod-down
// whatever the mode (zero in the mod-ups), so a cached block does not depend on it.
struct alignas(16) HyConv
{
    uint32_t nsrc, ntgt, pad[2];
    uint32_t src_prime[HY_MAX_ALPHA];
    uint32_t tgt_prime[MOAI_MAX_RNS];
    Tw src_inv[HY_MAX_ALPHA];
    uint64_t src_pre[HY_MAX_ALPHA];
    uint64_t tgt_post[MOAI_MAX_RNS];
    uint64_t w[MOAI_MAX_RNS][HY_MAX_ALPHA];
    double src_rinv[HY_MAX_ALPHA];
    uint64_t tgt_negw[MOAI_MAX_RNS];
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
//
// EXACT (a mod-down in MOAI_HYBRID_ROUND_EXACT; the fast instantiation's code is what it was).  As integers sum_r y_r (W / s_r) =
// X' + v* W with X' in [0, W) and v* = floor(sum_r y_r / s_r) in [0, nsrc).  The kernel estimates that sum in binary64 as the header
// states it -- f = 0; f = f (+) ((double)y_r (x) src_rinv[r]) in source order, every step one rounded operation (the file is compiled
// with contraction off, and the pragma below says so again) -- takes v = min(max(floor(f), 0), nsrc - 1) and adds v (m_t - (W mod
// m_t)) to the 128-bit sum: one more product, below 2^4 2^61, so the sum is 17 products below 2^122 < 2^127.
// The bound on |f - sum_r y_r / s_r|, u = 2^-53, n = nsrc <= 17, s_r < 2^61, y_r < s_r:
//   src_rinv[r] = (1 / s_r)(1 + d1), (double)y_r = y_r (1 + d2), the product (1 + d3), |d| <= u: each term t_r = (y_r / s_r)(1 + e_r)
//   with |e_r| <= 3u + 3u^2 + u^3 < 3.01u, and y_r / s_r < 1, so |t_r - y_r / s_r| < 3.01u and t_r < 1 + 3.01u.
//   The first addition (0 + t_0) is exact; every later partial sum is below 17 (1 + 3.01u) < 32, and so is its rounded value (32 is
//   representable), so its rounding error is at most half an ulp of a value below 32, 2^4 u; n - 1 such additions.
//   |f - sum_r y_r / s_r| <= 3.01 n u + 16 (n - 1) u <= (51.2 + 256) u < 323 2^-53 < 2^-44.
// The header promises eps = 2^-40.  Hence floor(f) differs from v* only where X' / W is within eps of 0 or of 1, by one and to the near
// side, and the clamp keeps v in [0, nsrc) where f rounds onto nsrc itself (nsrc = 1, y = s - 1: the product is 1.0).
// Registers: the fast <16> takes 166 VGPRs, three waves per SIMD, and the target loop waits for its constants (behind the stores of
// the previous target the compiler fetches them with vector loads of their uniform addresses, not with the scalar loads the note
// above counts on), so the waves in flight are what hides that wait.  Left alone the exact <16> takes 178 and runs
// two, 24 % slower per launch; asked to fit three it takes 166 with 20 bytes of spill per lane outside the target loop.  The
// attribute's value for the fast instantiations is the default: their code is the same text.
template <int AMAX, bool EXACT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(EXACT ? 3 : 1))) void hy_convert_kernel(HyConvArgs g)
{
#pragma clang fp contract(off)
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
        // the overflow of the two coefficients: below nsrc <= 16, kept in 32 bits (the registers of this kernel are its occupancy)
        [[maybe_unused]] uint32_t vx = 0, vy = 0;
        if constexpr (EXACT)
        {
            double fx = 0.0, fy = 0.0;
#pragma unroll
            for (int r = 0; r < AMAX; ++r)
            {
                if ((uint32_t)r < ns)
                {
                    const double ri = cv.src_rinv[r];
                    const double tx = __ull2double_rn(y[r].x) * ri, ty = __ull2double_rn(y[r].y) * ri;
                    fx = fx + tx;
                    fy = fy + ty;
                }
            }
            // f >= 0 (a sum of non-negative terms), so the lower clamp is the conversion's own; the upper one is the contract's
            const double top = (double)(ns - 1);
            vx = (uint32_t)fmin(floor(fx), top);
            vy = (uint32_t)fmin(floor(fy), top);
        }
        for (uint32_t t = 0; t < nt; ++t)
        {
            const PrimeConst *pc = g.pc + cv.tgt_prime[t];
            const uint64_t m = pc->q, cr0 = pc->cr0, cr1 = pc->cr1, post = cv.tgt_post[t];
            uint64_t lx = 0, hx = 0, ly = 0, hy = 0;
            if constexpr (EXACT)
            {
                mac2(lx, hx, ly, hy, make_ulonglong2(vx, vy), cv.tgt_negw[t]);
            }
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

// ---- the fused switch (MOAI_HYBRID_FUSED): steps 2-4 as two passes around the forward transform ------------------------------------
// Steps 2-4 of the unfused chain move, per converted coefficient, 8 B out of the conversion, 32 B through the two transform passes
// and 8 B back into the MAC.  Here the fast base conversion rides on the strided pass's loads (hy_fwd_strided) and the contiguous
// pass multiplies every finished digit straight into the accumulators (hy_contig_mac8): a converted row exists only as the strided
// pass's output, tmp [B][G][beta][N] for the G output rows of a launch, and a transformed digit never reaches memory.  What the
// two kernels leave in acc [B][2][L + alpha][N] are the canonical residues hy_mac_kernel leaves -- the same sums modulo the same
// primes -- so everything behind step 4 runs unchanged.  ks_fwd_strided / ks_contig_mac8 (keyswitch_kernels.hip.h) are the alpha = 1
// shape of the same pair; these serve digits of up to HY_MAX_ALPHA primes and hybrid.hip's row order.

// the output rows of one launch pair: rows of one arithmetic mode (32-bit entries: scalar loads, see RowMap).  The unused entries
// repeat the first member.
struct HyFusedGroup
{
    uint32_t prime[MOAI_MAX_RNS]; // context prime of member g
    uint32_t row[MOAI_MAX_RNS];   // its row of L + alpha
};

struct HyScaleArgs
{
    uint64_t *t; // [B][L][N], coefficient form, canonical: scaled in place
    const HyConv *cv;
    HyDims d;
};

// step 2's scaled residues, once per ciphertext: y_r = c_r [(D_j / q_r)^-1]_{q_r} over the L rows of t = INTT(c), in place (nothing
// else reads t: a digit's own rows come from the NTT-form target).  blockIdx.y = b * L + r.  The product hy_convert_kernel forms per
// conversion (src_pre = 0 in a mod-up), here outside the loop over the L + alpha - |R_j| target rows.
__global__ __launch_bounds__(256) void hy_scale_digits_kernel(HyScaleArgs g)
{
    const HyDims &d = g.d;
    const uint32_t row = blockIdx.y % d.L, j = row / d.alpha;
    const uint64_t q = d.pc[row].q;
    const Tw inv = g.cv[j].src_inv[row - j * d.alpha];
    ulonglong2 *t = reinterpret_cast<ulonglong2 *>(g.t) + (size_t)blockIdx.y * d.n2;
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < d.n2; x += gridDim.x * 256u)
    {
        ulonglong2 v = t[x];
        v.x = csub(mul_shoup_lazy(v.x, inv.w, inv.wq, q), q);
        v.y = csub(mul_shoup_lazy(v.y, inv.w, inv.wq, q), q);
        t[x] = v;
    }
}

// strided_load_raw's index (ntt_kernels.hip.h: element j * 256 + tid of a tile, as the OR of its three fields) for one j, for a pass
// that does not take all sixteen values at once
template <int LOGN>
__device__ __forceinline__ uint32_t strided_index(int j, uint32_t tid)
{
    constexpr int GB = 12 - (LOGN - 8);
    constexpr uint32_t G = 1u << GB;
    return GB == 8 ? (uint32_t)j * 256u + tid : ((uint32_t)j << (16 - GB)) | ((tid >> GB) << 8) | (tid & (G - 1));
}

struct HyP1Args
{
    const uint64_t *y; // [B][L][N]: the scaled residues (hy_scale_digits_kernel), coefficient form, canonical
    uint64_t *tmp;     // [B][G][beta][N] after the strided pass, in the lazy range ks_fwd_strided leaves
    const Tw *tw;
    const PrimeConst *pc;
    const HyConv *cv;  // [beta]: the mod-ups of HyTable
    HyFusedGroup grp;
    uint32_t L, alpha, beta;
    uint32_t G;
    uint32_t total_work; // B * beta * TPR * G
};

// The strided pass with the fast base conversion on its loads.  Work item = (ciphertext b, digit j, output row of the group, tile);
// an item whose row is one of the digit's own primes has nothing to do (hy_contig_mac8 reads the target's NTT-form row there).
// A thread holds its 16 coefficients as 16 128-bit sums and walks the digit's |R_j| <= 16 source rows in a loop whose trip count is
// uniform over the workgroup: 16 loads with the tile's strided addressing, then 16 multiply-adds with w[row][r], one scalar load from
// the digit's HyConv.  No template parameter on the digit size, so no instantiation that holds a whole digit in registers
// (hy_convert_kernel<16>: 166 VGPRs).  The sixteen loads of a source row are issued as two halves of eight: with all sixteen in flight
// beside the 64 registers of sums the kernel spilled 3-10 registers per lane at four waves per SIMD, one reload of them inside this
// loop; in halves it takes 118-120 VGPRs and no scratch.  N = 2^12 (no exchange, no LDS, the sixteen stores off one address) takes
// 142 and is bounded to three waves instead: at four it spilled 60-68 bytes per lane.
// At most 16 products below 2^122: the sums stay below 2^126.  Then ONE reduction to the
// canonical residue -- hy_mod128, since a source residue may be far above the target prime -- in the FP64 modes its conversion to the
// balanced double (the residue is below q < 2^51: LoadFp52's operation), and strided_core as it is.
// Order of the work ids, under xcd_remap: the group's output rows fastest, then the tile, the digit, the ciphertext.  The G
// workgroups that share one (tile, digit, ciphertext) read the same |R_j| source tiles (alpha * 32 KiB) and are neighbours on one
// XCD, so G - 1 of the G reads come from that XCD's L2.  With ks_fwd_strided's order (tile fastest) the neighbours share a row and
// the re-use distance of a source tile is a whole digit, alpha * 512 KiB at N = 2^16 per output row, against 4 MiB of L2.  The other
// order was not measured.
template <int LOGN, int MODE>
__global__ __launch_bounds__(256, LOGN == 12 ? 3 : 4) void hy_fwd_strided(HyP1Args a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    constexpr uint32_t TG = 1u << (12 - (LOGN - 8)); // columns of a tile
    __shared__ uint64_t lds[4096];
    uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t g = w % a.G;
    w /= a.G;
    const uint32_t tile = w % TPR;
    w /= TPR;
    const uint32_t j = w % a.beta;
    const uint32_t b = w / a.beta;
    const uint32_t prime = __builtin_amdgcn_readfirstlane(a.grp.prime[g]);
    const uint32_t row = __builtin_amdgcn_readfirstlane(a.grp.row[g]);
    const uint32_t lo = j * a.alpha, hi = min(lo + a.alpha, a.L), ns = hi - lo;
    if (row >= lo && row < hi)
    {
        return;
    }
    const uint32_t tg = row < lo ? row : row - ns; // the row's place among the conversion's targets
    const HyConv &cv = a.cv[j];
    const PrimeConst *pc = a.pc + prime;
    const uint64_t *in = a.y + (((size_t)b * a.L + lo) << LOGN) + tile * TG;
    uint64_t *out = a.tmp + ((((size_t)b * a.G + g) * a.beta + j) << LOGN);
    uint64_t x[16], xh[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        x[i] = xh[i] = 0;
    }
    for (uint32_t r = 0; r < ns; ++r)
    {
        const uint64_t *__restrict__ irow = in + ((size_t)r << LOGN);
        const uint64_t wr = cv.w[tg][r];
        // the sixteen loads in two halves of eight: sixteen registers of loads in flight beside the 64 of the sums, not 32
#pragma unroll
        for (int h = 0; h < 2; ++h)
        {
            uint64_t raw[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
            {
                raw[i] = irow[strided_index<LOGN>(h * 8 + i, threadIdx.x)];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
            {
                mac128(x[h * 8 + i], xh[h * 8 + i], raw[i], wr);
            }
        }
    }
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        x[i] = hy_mod128(x[i], xh[i], q, cr0, cr1);
        if (mode_fp(MODE))
        {
            x[i] = d2u(fp_red(fp_from_u52(x[i]), u2d(pc->qd), u2d(pc->qinv)));
        }
    }
    strided_core<LOGN, MODE, false>(x, out + tile * TG, a.tw + ((size_t)prime << LOGN), mode_q<MODE>(*pc), mode_q2<MODE>(*pc), lds,
                                    threadIdx.x);
}

struct HyP2Args
{
    const uint64_t *tmp; // [B][G][beta][N]
    const uint64_t *tgt; // the target in NTT form: ciphertext b's row r at tgt + ((b * tgt_stride + tgt_off + r) << LOGN)
    uint32_t tgt_stride, tgt_off;
    const uint64_t *key; // [beta(k - alpha)][2][k][N]
    uint64_t *acc;       // [B][2][L + alpha][N], hy_mac_kernel's layout
    const Tw *tw;
    const double *tw1;   // FP64 modes: the forward powers as plain doubles
    const PrimeConst *pc;
    HyFusedGroup grp;
    uint32_t L, alpha, beta;
    uint32_t G;
    uint32_t k;
    uint32_t B;
    uint32_t total_work; // B * 2 TPR * G: 2048-coefficient tiles
};

struct HyP2ListArgs : HyP2Args
{
    const KsList *lst; // ciphertext b's key is lst->keys[b], in the same whole layout (key unused)
};

// The contiguous pass plus the key MAC over the beta digits of one output row; ks_contig_mac8's structure (its comment has the
// register layouts P1 / P2 / P3 and the swizzles): a workgroup owns a 2048-coefficient tile of (ciphertext, output row), runs
// radix-8 / radix-8 / radix-4 with two LDS exchanges that stay inside a wave, and multiplies the eight finished coefficients into
// the 2 x 8 accumulators from the registers that finish the transform; the FP64 modes keep the thirteen per-thread twiddles of stages
// 3..7 in registers and the seven of stages 0..2 in LDS across the digit loop.  Where the output row is one of digit j's own primes
// (row < L, row / alpha = j) the operand is the target's NTT-form row as it is, not tmp.  Key word: key[j][p][prime of the row],
// k rows per polynomial.
// Sums, beta <= 63 digits:
//   M_GUARD    the digit is normalised to its canonical residue: at most 63 products below 2^122, one barrett128 (hy_mac_kernel's sum)
//   M_NOGUARD  the unreduced digit (below 33 q) goes straight into the MAC; the host picks the mode only where 36 q^2 beta < 2^128
//              (ks_mode's condition with beta in place of L)
//   M_FPN      33 q < 2^52: products below 2.5 q as the butterflies left the digit, sixteen of them on a folded sum below 40.5 q < 2^53
//   M_FPR      the digit folded to |v| <= q / 2, products below 0.88 q, three of them on a folded sum (2^53 / q > 4)
// (the FP64 bounds are ks_contig_mac8's, which has their derivation: the periods do not depend on the number of digits).
// LIST: member b's key from the pass's KsList record, as hy_mac_kernel<true>: a scalar load at the head of the workgroup.
template <int LOGN, int MODE, bool LIST = false>
__global__ __launch_bounds__(256, 4) void hy_contig_mac8(std::conditional_t<LIST, HyP2ListArgs, HyP2Args> a)
{
    constexpr int R1 = LOGN - 8;
    constexpr uint32_t TPR8 = 1u << (LOGN - 11);
    __shared__ ulonglong2 lds_a2[1024];
    __shared__ ulonglong2 lds_b2[1024];
    constexpr bool TW012 = mode_fp(MODE);
    __shared__ double lds_tw[TW012 ? 64 : 1];
    uint64_t *lds_a = reinterpret_cast<uint64_t *>(lds_a2);
    uint64_t *lds_b = reinterpret_cast<uint64_t *>(lds_b2);

    // ciphertext fastest: the workgroups that read the same key words and twiddles run together
    uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t bq = w % a.B;
    w /= a.B;
    const uint32_t tile = w % TPR8;
    const uint32_t g = w / TPR8;
    const uint32_t prime = a.grp.prime[g];
    const uint32_t row = a.grp.row[g];
    const uint32_t own = row < a.L ? row / a.alpha : a.beta; // the digit this row belongs to; none for a special row
    const PrimeConst *pc = a.pc + prime;
    const uint64_t q = pc->q;
    const uint64_t bq1 = mode_q<MODE>(*pc), bq2 = mode_q2<MODE>(*pc); // the butterflies' (q, q2) under MODE
    const Tw *__restrict__ tw = a.tw + ((size_t)prime << LOGN);
    const double *__restrict__ tw1 = a.tw1 + ((size_t)prime << LOGN);
    const uint32_t tid0 = threadIdx.x;
    const uint64_t *key = a.key;
    if constexpr (LIST)
    {
        key = a.lst->keys[bq];
    }

    uint64_t lo0[8], hi0[8], lo1[8], hi1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
    {
        lo0[e] = hi0[e] = lo1[e] = hi1[e] = 0;
    }
    const uint64_t *__restrict__ dig = a.tmp + ((((size_t)bq * a.G + g) * a.beta) << LOGN) + ((size_t)tile << 11);

    double twr[13];
    if (mode_fp(MODE))
    {
        const uint32_t b = tid0 >> 5, r = tid0 & 31u, hi3 = r >> 2;
        const uint32_t blk = (tile << 3) + b;
        twr[0] = tw1[(1u << (R1 + 3)) + (blk << 3) + hi3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
        {
            twr[1 + i] = tw1[(1u << (R1 + 4)) + (blk << 4) + ((hi3 << 1) | (uint32_t)i)];
            twr[7 + i] = tw1[(1u << (R1 + 6)) + (blk << 6) + ((r << 1) | (uint32_t)i)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            twr[3 + i] = tw1[(1u << (R1 + 5)) + (blk << 5) + ((hi3 << 2) | (uint32_t)i)];
            twr[9 + i] = tw1[(1u << (R1 + 7)) + (blk << 7) + ((r << 2) | (uint32_t)i)];
        }
    }
    if (TW012)
    {
        if (tid0 < 64u && (tid0 & 7u) < 7u)
        {
            const uint32_t b_ = tid0 >> 3, i = tid0 & 7u;
            const uint32_t u = i == 0 ? 0u : (i < 3 ? 1u : 2u);
            lds_tw[tid0] = tw1[(1u << (R1 + u)) + ((((uint32_t)tile << 3) + b_) << u) + (i - ((1u << u) - 1u))];
        }
        lds_barrier(); // written by wave 0, read by all four
    }
    for (uint32_t J = 0; J < a.beta; ++J)
    {
        // opaque copy of the thread index: keeps the per-thread address arithmetic inside the loop instead of hoisted into (and
        // spilled from) registers the accumulators need
        uint32_t tid = tid0;
        asm volatile("" : "+v"(tid));
        const uint32_t b = tid >> 5;
        const uint32_t r = tid & 31u;
        const uint32_t hi3 = r >> 2, lo2 = r & 3u;
        const uint32_t blk = (tile << 3) + b;
        // chunk (16 bytes = 2 coefficients) of this thread's 8 contiguous coefficients inside the tile
        const uint32_t ch0 = (b << 7) | (r << 2);
        const uint64_t *__restrict__ base = dig + ((size_t)J << LOGN);
        uint64_t x[8];
        const bool direct = (own == J); // workgroup-uniform
        const ulonglong2 *__restrict__ k0 =
            reinterpret_cast<const ulonglong2 *>(key + (((size_t)(J * 2 + 0) * a.k + prime) << LOGN)) + ((size_t)tile << 10) + ch0;
        const ulonglong2 *__restrict__ k1 =
            reinterpret_cast<const ulonglong2 *>(key + (((size_t)(J * 2 + 1) * a.k + prime) << LOGN)) + ((size_t)tile << 10) + ch0;
        if (direct)
        {
            // digit under one of its own primes: canonical NTT-form values straight from the target row
            const ulonglong2 *__restrict__ trow =
                reinterpret_cast<const ulonglong2 *>(a.tgt + (((size_t)bq * a.tgt_stride + a.tgt_off + row) << LOGN)) + ((size_t)tile << 10) + ch0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                ulonglong2 v = trow[c];
                // FP64 modes: as doubles, like the values the butterflies leave (canonical below q: nothing to fold)
                x[2 * c] = mode_fp(MODE) ? d2u(fp_from_u52(v.x)) : v.x;
                x[2 * c + 1] = mode_fp(MODE) ? d2u(fp_from_u52(v.y)) : v.y;
            }
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
                x[j] = base[(b << 8) | ((uint32_t)j << 5) | r];
            }
            // stages 0..2: layout P1
#pragma unroll
            for (int u = 0; u < 3; ++u)
            {
                const int half = 4 >> u;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                {
                    if (!(j & half))
                    {
                        if (mode_fp(MODE))
                        {
                            ct_bfly_fp1_sel(x[j], x[j + half], lds_tw[(b << 3) + ((1u << u) - 1u) + (uint32_t)(j >> (3 - u))], u2d(bq1),
                                            u2d(bq2), MODE == M_FPR && !(u & 1));
                        }
                        else
                        {
                            Tw t = tw[(1u << (R1 + u)) + (blk << u) + (uint32_t)(j >> (3 - u))];
                            ct_bfly_t<MODE>(x[j], x[j + half], t.w, t.wq, bq1, bq2);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
                lds_a[phys8_a((b << 8) | ((uint32_t)j << 5) | r)] = x[j];
            }
            lds_wave_sync(); // block b's 32 threads are half a wave: both exchanges stay inside one wave
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
                x[j] = lds_a[phys8_a((b << 8) | (hi3 << 5) | ((uint32_t)j << 2) | lo2)];
            }
            // stages 3..5: layout P2
#pragma unroll
            for (int u = 3; u < 6; ++u)
            {
                const int half = 4 >> (u - 3);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                {
                    if (!(j & half))
                    {
                        uint32_t t_ = (hi3 << 5) | ((uint32_t)j << 2) | lo2;
                        if (mode_fp(MODE))
                        {
                            ct_bfly_fp1_sel(x[j], x[j + half], twr[(u == 3) ? 0 : (u == 4) ? 1 + (j >> 2) : 3 + (j >> 1)], u2d(bq1), u2d(bq2),
                                            MODE == M_FPR && !(u & 1));
                        }
                        else
                        {
                            Tw t = tw[(1u << (R1 + u)) + (blk << u) + (t_ >> (8 - u))];
                            ct_bfly_t<MODE>(x[j], x[j + half], t.w, t.wq, bq1, bq2);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
                lds_b[phys8_b((b << 8) | (hi3 << 5) | ((uint32_t)j << 2) | lo2)] = x[j];
            }
            lds_wave_sync();
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                // coefficients (r << 3) | 2c, 2c+1: chunk c of the row, stored at chunk c ^ ((r >> 2) & 3)
                ulonglong2 v = lds_b2[((b << 8) | (r << 3)) / 2 + ((uint32_t)c ^ ((r >> 2) & 3u))];
                x[2 * c] = v.x;
                x[2 * c + 1] = v.y;
            }
            // stages 6..7: layout P3
#pragma unroll
            for (int u = 6; u < 8; ++u)
            {
                const int half = 2 >> (u - 6);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                {
                    if (!(j & half))
                    {
                        uint32_t t_ = (r << 3) | (uint32_t)j;
                        if (mode_fp(MODE))
                        {
                            ct_bfly_fp1_sel(x[j], x[j + half], twr[(u == 6) ? 7 + (j >> 2) : 9 + (j >> 1)], u2d(bq1), u2d(bq2),
                                            MODE == M_FPR && !(u & 1));
                        }
                        else
                        {
                            Tw t = tw[(1u << (R1 + u)) + (blk << u) + (t_ >> (8 - u))];
                            ct_bfly_t<MODE>(x[j], x[j + half], t.w, t.wq, bq1, bq2);
                        }
                    }
                }
            }
        }
        if (mode_fp(MODE))
        {
            // the MAC on the FP64 pipe (fp_mulmod_q, the key residue canonical below 2^51); the sixteen key residues are all issued at
            // the head, with one wait, and one wave-uniform branch goes around the sixteen periodic reductions (ks_contig_mac8 measured
            // that arrangement)
            const bool fold = MODE == M_FPR ? (J % 3u == 2u) : ((J & 15u) == 15u);
            const double qd = u2d(bq1), qinv = u2d(bq2);
            ulonglong2 kpa[4], kpb[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                kpa[c] = k0[c];
                kpb[c] = k1[c];
            }
            double sm[16];
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                const double vx = MODE == M_FPN ? u2d(x[2 * c]) : fp_red(u2d(x[2 * c]), qd, qinv);
                const double vy = MODE == M_FPN ? u2d(x[2 * c + 1]) : fp_red(u2d(x[2 * c + 1]), qd, qinv);
                sm[4 * c + 0] = u2d(lo0[2 * c]) + fp_mulmod_q(vx, fp_from_u52(kpa[c].x), qd, qinv);
                sm[4 * c + 1] = u2d(lo0[2 * c + 1]) + fp_mulmod_q(vy, fp_from_u52(kpa[c].y), qd, qinv);
                sm[4 * c + 2] = u2d(lo1[2 * c]) + fp_mulmod_q(vx, fp_from_u52(kpb[c].x), qd, qinv);
                sm[4 * c + 3] = u2d(lo1[2 * c + 1]) + fp_mulmod_q(vy, fp_from_u52(kpb[c].y), qd, qinv);
            }
            if (fold)
            {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                {
                    sm[i] = fp_red(sm[i], qd, qinv);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                lo0[2 * c] = d2u(sm[4 * c + 0]);
                lo0[2 * c + 1] = d2u(sm[4 * c + 1]);
                lo1[2 * c] = d2u(sm[4 * c + 2]);
                lo1[2 * c + 1] = d2u(sm[4 * c + 3]);
            }
        }
        else
        {
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                uint64_t vx = x[2 * c], vy = x[2 * c + 1];
                if (MODE == M_GUARD && !direct)
                {
                    vx = csub(csub(vx, bq2), q);
                    vy = csub(csub(vy, bq2), q);
                }
                ulonglong2 ka = k0[c];
                ulonglong2 kb = k1[c];
                mac128(lo0[2 * c], hi0[2 * c], vx, ka.x);
                mac128(lo0[2 * c + 1], hi0[2 * c + 1], vy, ka.y);
                mac128(lo1[2 * c], hi1[2 * c], vx, kb.x);
                mac128(lo1[2 * c + 1], hi1[2 * c + 1], vy, kb.y);
            }
        }
        // no barrier here: the next digit writes buffer A, whose readers of this wave all passed the second wait above, and buffer B
        // is written again only behind the next first wait
    }
    const uint32_t ch0 = ((tid0 >> 5) << 7) | ((tid0 & 31u) << 2);
    const uint64_t cr0 = pc->cr0, cr1 = pc->cr1;
    const size_t rows = a.L + a.alpha;
    ulonglong2 *__restrict__ o0 = reinterpret_cast<ulonglong2 *>(a.acc + ((((size_t)bq * 2 + 0) * rows + row) << LOGN)) + ((size_t)tile << 10) + ch0;
    ulonglong2 *__restrict__ o1 = reinterpret_cast<ulonglong2 *>(a.acc + ((((size_t)bq * 2 + 1) * rows + row) << LOGN)) + ((size_t)tile << 10) + ch0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
        ulonglong2 r0, r1;
        if (mode_fp(MODE))
        {
            const double qd = u2d(bq1), qinv = u2d(bq2);
            r0.x = fp_to_canonical(u2d(lo0[2 * c]), qd, qinv);
            r0.y = fp_to_canonical(u2d(lo0[2 * c + 1]), qd, qinv);
            r1.x = fp_to_canonical(u2d(lo1[2 * c]), qd, qinv);
            r1.y = fp_to_canonical(u2d(lo1[2 * c + 1]), qd, qinv);
        }
        else
        {
            r0.x = barrett128(lo0[2 * c], hi0[2 * c], q, cr0, cr1);
            r0.y = barrett128(lo0[2 * c + 1], hi0[2 * c + 1], q, cr0, cr1);
            r1.x = barrett128(lo1[2 * c], hi1[2 * c], q, cr0, cr1);
            r1.y = barrett128(lo1[2 * c + 1], hi1[2 * c + 1], q, cr0, cr1);
        }
        o0[c] = r0;
        o1[c] = r1;
    }
}

// ---- the fused mod-down (MOAI_HYBRID_FUSED_DOWN): step 5 as a scale kernel and two passes around the forward transform -----------------
// Behind the INTT of its nsrc source rows the unfused step 5 moves, per polynomial and in rows of N words: the conversion nsrc + ntgt
// (hy_convert_kernel reads every source once and writes every target), the transform of the converted rows 4 ntgt (two passes, each a
// read and a write), the last kernel 3 ntgt (accumulator, converted row, output; one or two more with addends).  A converted row
// crosses memory six times, 8 ntgt rows in all.  Here the conversion's per-source work is done once per coefficient
// (hy_down_scale_kernel, 2 nsrc rows, one more written in exact mode), its sums ride on the strided pass's loads (hy_down_strided:
// nsrc source tiles read per output row, ntgt of them per source tile, all but the first from the XCD's L2 under the order below; ntgt
// rows written) and the division on the contiguous pass's stores (hy_down_contig / hy_rescale_contig: the converted row and the
// accumulator read, the output written, 3 ntgt).  A converted row crosses memory twice: 2 nsrc + 4 ntgt rows from HBM plus the re-read
// source tiles, against 5 nsrc + 8 ntgt.  At L = 35, alpha = 12 with the INTT's 4 nsrc on both sides: 212 against 340.  Arithmetic on
// the code; what the re-reads cost is a question for the measurement.
// All three leave the canonical residues the unfused chain leaves -- the conversion's sum is reduced by the same hy_mod128 and
// submod, the transform's output is canonical in every mode, the division is the same Shoup product -- so every output is bit for
// bit what moddown_finalize_kernel / hy_rescale_finalize_kernel write, in both rounding modes.  moddown_strided / moddown_contig
// (keyswitch_kernels.hip.h) are the one-source shape of the same pair.
struct HyDownScaleArgs
{
    uint64_t *x; // [P][nsrc][N], coefficient form, canonical: scaled in place
    uint64_t *v; // EXACT: polynomial p's overflow row, N words, at v + p * v_stride * N
    const HyConv *cv;
    const PrimeConst *pc;
    uint32_t v_stride;
    uint32_t n2;
};

// The mod-down's per-source work, once per coefficient instead of once per target row: in place on x,
//   y_r = ((x_r + src_pre[r]) mod s_r) src_inv[r] mod s_r, canonical
// (hy_convert_kernel's first loop; what hy_scale_digits_kernel does for the mod-ups).  blockIdx.y = polynomial.  A thread streams its
// two coefficients through the nsrc rows in source order, the next row's load issued before this row's arithmetic; no register array.
// EXACT (MOAI_HYBRID_ROUND_EXACT): the overflow estimate of hy_convert_kernel<.., true>, the same operations in the same order --
// f = 0; f = f (+) ((double)y_r (x) src_rinv[r]), contraction off, v = min(floor(f), nsrc - 1); its comment has the error bound --
// written as one more row of 64-bit words per polynomial, which hy_down_strided reads as a seventeenth source of weight tgt_negw[t].
// Where that row lives: the polynomial's FIRST SOURCE ROW inside the accumulator (row `off` of its `stride` rows; the host passes v =
// acc + off N and v_stride = stride).  The out-of-place INTT in front of this kernel was the last reader of the accumulator's source
// rows: the contiguous passes read rows below the first source only (i < L of L + alpha for the plain mod-down, i < L - 1 for the
// merged rescale, whose first source is the lifted row L - 1).  Checked for every caller: the switch, hoisted and rescale
// accumulators (HY_ACC) are rewritten whole by the next chunk's MAC; the pt-dot sums (HY_S) are started from zero by the first pass
// of the next group of outputs (HyDotOutputs::seeded = 0) and every output that takes a step 5 has a switched term; the BSGS sum
// (HY_Z) takes its one final step 5 behind the last group and the next chunk starts it with zseeded = 0.  The inner c1-only mod-down
// of the BSGS sum keeps the unfused stages and its S is read again by hy_bsgs_mac_kernel, special rows included: it is not routed
// here.  No scratch region is added.
template <bool EXACT>
__global__ __launch_bounds__(256) void hy_down_scale_kernel(HyDownScaleArgs g)
{
#pragma clang fp contract(off)
    const HyConv &cv = *g.cv;
    const uint32_t ns = cv.nsrc;
    const size_t n2 = g.n2;
    ulonglong2 *x = reinterpret_cast<ulonglong2 *>(g.x) + (size_t)blockIdx.y * ns * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.n2; j += gridDim.x * 256u)
    {
        [[maybe_unused]] double fx = 0.0, fy = 0.0;
        ulonglong2 next = x[j];
        for (uint32_t r = 0; r < ns; ++r)
        {
            const uint64_t q = g.pc[cv.src_prime[r]].q, pre = cv.src_pre[r];
            const Tw inv = cv.src_inv[r];
            ulonglong2 y = next;
            if (r + 1 < ns)
            {
                next = x[(size_t)(r + 1) * n2 + j];
            }
            y.x = csub(mul_shoup_lazy(csub(y.x + pre, q), inv.w, inv.wq, q), q);
            y.y = csub(mul_shoup_lazy(csub(y.y + pre, q), inv.w, inv.wq, q), q);
            x[(size_t)r * n2 + j] = y;
            if constexpr (EXACT)
            {
                const double ri = cv.src_rinv[r];
                const double tx = __ull2double_rn(y.x) * ri, ty = __ull2double_rn(y.y) * ri;
                fx = fx + tx;
                fy = fy + ty;
            }
        }
        if constexpr (EXACT)
        {
            // f >= 0, so the lower clamp is the conversion's own; the upper one is the contract's (hy_convert_kernel)
            const double top = (double)(ns - 1);
            ulonglong2 *v = reinterpret_cast<ulonglong2 *>(g.v) + (size_t)blockIdx.y * g.v_stride * n2;
            v[j] = make_ulonglong2((uint64_t)(uint32_t)fmin(floor(fx), top), (uint64_t)(uint32_t)fmin(floor(fy), top));
        }
    }
}

struct HyDownP1Args
{
    const uint64_t *x; // [P][nsrc][N]: the scaled residues (hy_down_scale_kernel), coefficient form, canonical
    const uint64_t *v; // exact: the overflow rows, polynomial p's at v + p * v_stride * N (read only then)
    uint64_t *conv;    // [P][ntgt][N] after the strided pass, in the lazy range hy_fwd_strided leaves
    const Tw *tw;
    const PrimeConst *pc;
    const HyConv *cv;  // the mod-down's conversion
    RowMap sel;        // the output rows (= targets = data primes) of this launch: one arithmetic mode per launch
    uint32_t Lsel;
    uint32_t v_stride;
    uint32_t exact;      // 0 or 1: the extra trip over the overflow row
    uint32_t total_work; // P * TPR * Lsel
};

// The strided pass with the mod-down's base conversion on its loads; hy_fwd_strided's structure.  Work item = (polynomial, tile,
// output row of the launch).  A thread holds its 16 coefficients as 16 128-bit sums and walks the nsrc <= 16 source rows in a loop
// whose trip count is uniform over the workgroup: sixteen loads with the tile's strided addressing, in two halves of eight, then
// sixteen multiply-adds with w[t][r], one scalar load from the HyConv.  In exact mode the overflow row is one more trip of the same
// loop -- another row pointer and the weight tgt_negw[t], both selected by a uniform condition -- so 17 products below 2^122 and a
// sum below 2^127 (hy_convert_kernel's comment has the bound); no second instantiation.  Then ONE hy_mod128, the submod of
// tgt_post[t] (the canonical residue hy_convert_kernel stores), in the FP64 modes its conversion to the balanced double (below
// q < 2^51: LoadFp52's operation), and strided_core as it is.
// Order of the work ids, under xcd_remap: output row fastest, then tile, then polynomial.  The Lsel workgroups that share one
// (tile, polynomial) read the same nsrc source tiles (nsrc * 32 KiB) and are neighbours on one XCD; no digit index: all ntgt rows of
// a polynomial share one set of sources.  The other order (tile fastest, moddown_strided's) was not measured.
// Registers, scratch and waves: the table at hy_down_contig.  No scratch, four waves; N = 2^12 is bounded to three as hy_fwd_strided is.
template <int LOGN, int MODE>
__global__ __launch_bounds__(256, LOGN == 12 ? 3 : 4) void hy_down_strided(HyDownP1Args a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    constexpr uint32_t TG = 1u << (12 - (LOGN - 8)); // columns of a tile
    __shared__ uint64_t lds[4096];
    uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t g = w % a.Lsel;
    w /= a.Lsel;
    const uint32_t tile = w % TPR;
    const uint32_t p = w / TPR;
    const uint32_t t = __builtin_amdgcn_readfirstlane(a.sel.idx[g]);
    const HyConv &cv = *a.cv;
    const uint32_t ns = cv.nsrc, nt = cv.ntgt, trips = ns + a.exact;
    const uint32_t prime = cv.tgt_prime[t];
    const PrimeConst *pc = a.pc + prime;
    const uint64_t *in = a.x + (((size_t)p * ns) << LOGN) + tile * TG;
    const uint64_t *vrow = a.v + (((size_t)p * a.v_stride) << LOGN) + tile * TG;
    uint64_t *out = a.conv + (((size_t)p * nt + t) << LOGN);
    uint64_t x[16], xh[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        x[i] = xh[i] = 0;
    }
    for (uint32_t r = 0; r < trips; ++r)
    {
        const bool over = r == ns; // the exact mode's last trip: the overflow row
        const uint64_t *__restrict__ irow = over ? vrow : in + ((size_t)r << LOGN);
        const uint64_t wr = over ? cv.tgt_negw[t] : cv.w[t][r];
        // the sixteen loads in two halves of eight, as in hy_fwd_strided
#pragma unroll
        for (int h = 0; h < 2; ++h)
        {
            uint64_t raw[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
            {
                raw[i] = irow[strided_index<LOGN>(h * 8 + i, threadIdx.x)];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
            {
                mac128(x[h * 8 + i], xh[h * 8 + i], raw[i], wr);
            }
        }
    }
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1, post = cv.tgt_post[t];
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        x[i] = submod(hy_mod128(x[i], xh[i], q, cr0, cr1), post, q);
        if (mode_fp(MODE))
        {
            x[i] = d2u(fp_red(fp_from_u52(x[i]), u2d(pc->qd), u2d(pc->qinv)));
        }
    }
    strided_core<LOGN, MODE, false>(x, out + tile * TG, a.tw + ((size_t)prime << LOGN), mode_q<MODE>(*pc), mode_q2<MODE>(*pc), lds,
                                    threadIdx.x);
}

// what the contiguous pass of the plain mod-down does with a finished chunk u of NTT(conv): out = (acc - u) inv [+ add] [+ add2],
// moddown_finalize_kernel's arithmetic.  StoreModDown's shape (the operands of four chunks fetched together, before the four calls
// that finish them) without its partial sums and scalar product, and under names of its own -- one per LIST -- so that every kernel
// here instantiates its own fwd_contig_tile and the existing kernels' instruction streams stay what they are (the note on
// StoreModDownList).  A thread reads the chunks it adds before it writes the same chunks, so out may be add or add2.
template <bool LIST>
struct StoreHyDown
{
    const ulonglong2 *acc;  // tile base of the row being divided
    ulonglong2 *out;        // tile base of the result row
    const ulonglong2 *add;  // tile base of the row to add, or nullptr
    const ulonglong2 *add2; // tile base of a second row to add, or nullptr
    uint64_t q;
    Tw inv;
    ulonglong2 av[4], cv[4], dv[4];
    __device__ __forceinline__ void fetch(const uint32_t (&chs)[4])
    {
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            av[i] = acc[chs[i]];
        }
        if (add)
        {
#pragma unroll
            for (int i = 0; i < 4; ++i)
            {
                cv[i] = add[chs[i]];
            }
        }
        if (add2)
        {
#pragma unroll
            for (int i = 0; i < 4; ++i)
            {
                dv[i] = add2[chs[i]];
            }
        }
    }
    __device__ __forceinline__ void operator()(int i, uint32_t ch, ulonglong2 u) const
    {
        ulonglong2 r;
        r.x = csub(mul_shoup_lazy(av[i].x + q - u.x, inv.w, inv.wq, q), q);
        r.y = csub(mul_shoup_lazy(av[i].y + q - u.y, inv.w, inv.wq, q), q);
        if (add)
        {
            r = moai::add2(r, cv[i], q);
        }
        if (add2)
        {
            r = moai::add2(r, dv[i], q);
        }
        out[ch] = r;
    }
};

struct HyDownP2Args
{
    uint64_t *conv;      // [P][ntgt][N]: the strided pass's output
    const uint64_t *acc; // row (p, i) at acc + (p * acc_stride + i) * N
    uint64_t *out;       // [P][ntgt][N]
    const Tw *tw;
    const Tw *twb;
    const PrimeConst *pc;
    const Tw *inv;       // the divisor's inverse mod q_i
    const uint64_t *addend; // the addends as in ModDownArgs (KsAddend)
    const uint64_t *addend2;
    uint32_t addend_bstride;
    int add_mode;
    uint32_t acc_stride;
    uint32_t ntgt;
    uint32_t P;
    uint32_t total_work; // P * TPR * Lsel
    RowMap sel;
    uint32_t Lsel;
};

struct HyDownP2ListArgs : HyDownP2Args
{
    const KsList *lst; // as moddown_contig: polynomials 2b and 2b + 1 go to lst->outs[b] plus lst->sums[b]; add_mode 1 reads lst->ins[b]
};

// The contiguous pass of the plain mod-down with the division on its stores: moddown_contig's structure -- polynomial fastest, one
// 4096-coefficient tile per workgroup through fwd_contig_tile, every KsAddend mode and the LIST addressing -- on the hybrid
// accumulator's rows (acc_stride = L + alpha, inv = P^-1).
// Resources as the compiler reports them (gfx950, this file's flags; VGPRs, and the waves per SIMD they allow; no instantiation of
// any of the kernels takes scratch, so nothing spills inside hy_down_strided's source loop; LIST and plain take the same):
//                        M_GUARD    M_NOGUARD   M_FPN      M_FPR
//   hy_down_strided      108, 4     108, 4      108, 4     108, 4     N = 2^13 .. 2^16 (110 at 2^15); 32 KiB of LDS
//                        140, 3     140, 3      140, 3     140, 3     N = 2^12: no exchange, no LDS; bounded to three as hy_fwd_strided
//   hy_down_contig        79, 5      79, 5       93, 5      85, 5     every N; 32 KiB of LDS, which also allow five workgroups a CU
//   hy_rescale_contig    101, 4      99, 4      122, 4     100, 4     every N
//   hy_down_scale_kernel 25 (fast), 33 (exact): eight waves
// The overflow row costs the strided pass no register: kept in the pass's registers instead, the estimate would need the nsrc
// scaled residues of all sixteen coefficients before the first sum, which is hy_convert_kernel<16>'s 166 VGPRs and three waves.
template <int LOGN, int MODE, bool LIST = false>
__global__ __launch_bounds__(256) void hy_down_contig(std::conditional_t<LIST, HyDownP2ListArgs, HyDownP2Args> a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    __shared__ ulonglong2 lds2[2048];
    uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t p = w % a.P;
    w /= a.P;
    const uint32_t tile = w % TPR;
    const uint32_t i = __builtin_amdgcn_readfirstlane(a.sel.idx[w / TPR]);
    const PrimeConst &pc = a.pc[i];
    const size_t orow = ((size_t)p * a.ntgt + i) << LOGN, toff = (size_t)tile << 11;
    StoreHyDown<LIST> st;
    st.acc = reinterpret_cast<const ulonglong2 *>(a.acc + (((size_t)p * a.acc_stride + i) << LOGN)) + toff;
    st.out = reinterpret_cast<ulonglong2 *>(a.out + orow) + toff;
    st.q = pc.q;
    st.inv = a.inv[i];
    st.add = nullptr;
    if (a.add_mode == 1 || (a.add_mode == 2 && !(p & 1u)))
    {
        st.add = reinterpret_cast<const ulonglong2 *>(a.addend + (((size_t)(p >> 1) * a.addend_bstride + (size_t)(p & 1u) * a.ntgt + i) << LOGN)) + toff;
    }
    st.add2 = a.addend2 ? reinterpret_cast<const ulonglong2 *>(a.addend2 + orow) + toff : nullptr;
    if constexpr (LIST)
    {
        const uint32_t b = p >> 1;
        const size_t row = ((size_t)(p & 1u) * a.ntgt + i) << LOGN; // inside the member's [2][ntgt][N]
        st.out = reinterpret_cast<ulonglong2 *>(a.lst->outs[b] + row) + toff;
        const uint64_t *sum = a.lst->sums[b];
        st.add2 = sum ? reinterpret_cast<const ulonglong2 *>(sum + row) + toff : nullptr;
        if (a.add_mode == 1)
        {
            st.add = reinterpret_cast<const ulonglong2 *>(a.lst->ins[b] + row) + toff;
        }
    }
    // the tile hands the store canonical integers in every mode
    fwd_contig_tile<LOGN, MODE, StoreHyDown<LIST>>(a.conv + orow, tile, a.tw + ((size_t)i << LOGN), mode_q<MODE>(pc), mode_q2<MODE>(pc), lds2,
                                                   threadIdx.x, a.twb + (size_t)i * ((size_t)TPR * 15 * 256), pc.cr1, st);
}

// the merged relinearize + rescale's finish on a finished chunk u of NTT(conv): out = c_p [q_{L-1}^-1] + (acc - u) [W^-1],
// hy_rescale_finalize_kernel's two Shoup products made canonical and one canonical add
template <bool LIST>
struct StoreHyRescale
{
    const ulonglong2 *acc; // tile base of the accumulator's row
    const ulonglong2 *cp;  // tile base of c_p's row
    ulonglong2 *out;       // tile base of the result row
    uint64_t q;
    Tw wi, qi;
    ulonglong2 av[4], cv[4];
    __device__ __forceinline__ void fetch(const uint32_t (&chs)[4])
    {
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            av[i] = acc[chs[i]];
            cv[i] = cp[chs[i]];
        }
    }
    __device__ __forceinline__ void operator()(int i, uint32_t ch, ulonglong2 u) const
    {
        ulonglong2 r, t;
        r.x = csub(mul_shoup_lazy(av[i].x + q - u.x, wi.w, wi.wq, q), q);
        r.y = csub(mul_shoup_lazy(av[i].y + q - u.y, wi.w, wi.wq, q), q);
        t.x = csub(mul_shoup_lazy(cv[i].x, qi.w, qi.wq, q), q);
        t.y = csub(mul_shoup_lazy(cv[i].y, qi.w, qi.wq, q), q);
        out[ch] = add2(r, t, q);
    }
};

struct HyRescaleP2Args
{
    uint64_t *conv;      // [2B][L - 1][N]: the strided pass's output
    const uint64_t *acc; // [B][2][L + alpha][N]
    const uint64_t *ct3; // [B][3][L][N]: c_0 and c_1 read
    uint64_t *out;       // [B][2][L - 1][N]
    const Tw *tw;
    const Tw *twb;
    const PrimeConst *pc;
    const Tw *winv, *qinv;
    uint32_t L, alpha;
    uint32_t P;          // 2B
    uint32_t total_work; // P * TPR * Lsel
    RowMap sel;
    uint32_t Lsel;
};

struct HyRescaleP2ListArgs : HyRescaleP2Args
{
    const KsList *lst; // ciphertext b's [3][L][N] block is lst->ins[b] and its [2][L - 1][N] result lst->outs[b] (ct3 and out unused)
};

// The contiguous pass of the merged mod-down with hy_rescale_finalize_kernel's formula on its stores, rows i < L - 1, plain and LIST
// addressing as there; the work order of hy_down_contig.
template <int LOGN, int MODE, bool LIST = false>
__global__ __launch_bounds__(256) void hy_rescale_contig(std::conditional_t<LIST, HyRescaleP2ListArgs, HyRescaleP2Args> a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    __shared__ ulonglong2 lds2[2048];
    uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t poly = w % a.P;
    w /= a.P;
    const uint32_t tile = w % TPR;
    const uint32_t i = __builtin_amdgcn_readfirstlane(a.sel.idx[w / TPR]);
    const uint32_t lo = a.L - 1, b = poly >> 1, p = poly & 1u;
    const PrimeConst &pc = a.pc[i];
    const size_t orow = ((size_t)poly * lo + i) << LOGN, toff = (size_t)tile << 11;
    StoreHyRescale<LIST> st;
    st.acc = reinterpret_cast<const ulonglong2 *>(a.acc + (((size_t)poly * (a.L + a.alpha) + i) << LOGN)) + toff;
    st.cp = reinterpret_cast<const ulonglong2 *>(a.ct3 + (((size_t)(b * 3 + p) * a.L + i) << LOGN)) + toff;
    st.out = reinterpret_cast<ulonglong2 *>(a.out + orow) + toff;
    if constexpr (LIST)
    {
        st.cp = reinterpret_cast<const ulonglong2 *>(a.lst->ins[b] + (((size_t)p * a.L + i) << LOGN)) + toff;
        st.out = reinterpret_cast<ulonglong2 *>(a.lst->outs[b] + (((size_t)p * lo + i) << LOGN)) + toff;
    }
    st.q = pc.q;
    st.wi = a.winv[i];
    st.qi = a.qinv[i];
    fwd_contig_tile<LOGN, MODE, StoreHyRescale<LIST>>(a.conv + orow, tile, a.tw + ((size_t)i << LOGN), mode_q<MODE>(pc), mode_q2<MODE>(pc),
                                                      lds2, threadIdx.x, a.twb + (size_t)i * ((size_t)TPR * 15 * 256), pc.cr1, st);
}

} // namespace moai
