// hybrid_kernels.hip.h -- the argument structs, the constant blocks (HyConv, HyTable, HyRescaleTable) and every kernel of the hybrid
// key switch.  Only hybrid.hip includes it; the chain the kernels form is described at the head of that file.
#pragma once
#include <type_traits>

#include "launch.h"
#include "modarith.hip.h"

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

} // namespace moai
