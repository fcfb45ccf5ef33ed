// modarith.hip.h -- 64-bit modular arithmetic for CDNA4 (no native 64-bit multiplier: everything
// lowers to v_mad_u64_u32 / v_mul_hi_u32 chains).  Any algorithm is admissible as long as the final
// canonical residues equal the reference's (SEAL/util/uintarithsmallmod.h:167-326).
#pragma once
#include "common.h"
#include "ntt_finish.h"

namespace moai {

__device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b)
{
    return __umul64hi(a, b);
}

// Shoup lazy product: y * w mod q in [0, 2q) for ANY 64-bit y, given wq = floor(w * 2^64 / q)
// (multiply_uint_mod_lazy, uintarithsmallmod.h:313-326).  Written as y*w + t*(-q) so that the two
// low products accumulate in one v_mad_u64_u32 chain instead of ending in a 64-bit subtract
// (v_sub_co / v_subb_co plus a VCC wait state on gfx950).
__device__ __forceinline__ uint64_t mul_shoup_lazy(uint64_t y, uint64_t w, uint64_t wq, uint64_t q)
{
    uint64_t t = mulhi64(y, wq);
    return y * w + t * (0 - q);
}

__device__ __forceinline__ uint64_t csub(uint64_t x, uint64_t m)
{
    // x >= m ? x - m : x
    return x >= m ? x - m : x;
}

// Barrett reduction of a 128-bit value (hi:lo) with cr = floor(2^128/q) (barrett_reduce_128,
// uintarithsmallmod.h:167-203).  Exact for q < 2^63.
__device__ __forceinline__ uint64_t barrett128(uint64_t lo, uint64_t hi, uint64_t q, uint64_t cr0, uint64_t cr1)
{
    // floor((hi:lo) * cr / 2^128), low 64 bits
    uint64_t carry = mulhi64(lo, cr0);
    uint64_t t_lo = lo * cr1;
    uint64_t t_hi = mulhi64(lo, cr1);
    uint64_t s = t_lo + carry;
    uint64_t tmp3 = t_hi + (s < t_lo ? 1 : 0);
    uint64_t u_lo = hi * cr0;
    uint64_t u_hi = mulhi64(hi, cr0);
    uint64_t s2 = s + u_lo;
    uint64_t c2 = u_hi + (s2 < s ? 1 : 0);
    uint64_t quot = hi * cr1 + tmp3 + c2;
    uint64_t r = lo - quot * q;
    return csub(r, q);
}

__device__ __forceinline__ uint64_t mulmod_barrett(uint64_t a, uint64_t b, uint64_t q, uint64_t cr0, uint64_t cr1)
{
    return barrett128(a * b, mulhi64(a, b), q, cr0, cr1);
}

// barrett_reduce_64 (uintarithsmallmod.h:211-230)
__device__ __forceinline__ uint64_t barrett64(uint64_t x, uint64_t q, uint64_t cr1)
{
    uint64_t t = mulhi64(x, cr1);
    return csub(x - t * q, q);
}

// x - y mod q for canonical x, y
__device__ __forceinline__ uint64_t submod(uint64_t x, uint64_t y, uint64_t q)
{
    return x >= y ? x - y : x + q - y;
}

// (hi:lo) += a * b, modulo 2^128
__device__ __forceinline__ void mac128(uint64_t &lo, uint64_t &hi, uint64_t a, uint64_t b)
{
    uint64_t pl = a * b;
    uint64_t ph = mulhi64(a, b);
    lo += pl;
    hi += ph + (lo < pl ? 1 : 0);
}

// ---- lane pairs: the two coefficients of one 16-byte access, canonical in and out ------------------------------------
__device__ __forceinline__ ulonglong2 add2(ulonglong2 x, ulonglong2 y, uint64_t q)
{
    return make_ulonglong2(csub(x.x + y.x, q), csub(x.y + y.y, q));
}
__device__ __forceinline__ ulonglong2 sub2(ulonglong2 x, ulonglong2 y, uint64_t q)
{
    return make_ulonglong2(submod(x.x, y.x, q), submod(x.y, y.y, q));
}
__device__ __forceinline__ ulonglong2 neg2(ulonglong2 x, uint64_t q)
{
    return make_ulonglong2(x.x ? q - x.x : 0, x.y ? q - x.y : 0);
}
__device__ __forceinline__ ulonglong2 mulmod2(ulonglong2 x, ulonglong2 y, uint64_t q, uint64_t cr0, uint64_t cr1)
{
    return make_ulonglong2(mulmod_barrett(x.x, y.x, q, cr0, cr1), mulmod_barrett(x.y, y.y, q, cr0, cr1));
}
// acc + x * y, each lane's product added and reduced before the other lane's
__device__ __forceinline__ ulonglong2 addmul2(ulonglong2 acc, ulonglong2 x, ulonglong2 y, uint64_t q, uint64_t cr0, uint64_t cr1)
{
    return make_ulonglong2(csub(acc.x + mulmod_barrett(x.x, y.x, q, cr0, cr1), q), csub(acc.y + mulmod_barrett(x.y, y.y, q, cr0, cr1), q));
}

// ---- the 128-bit sums of a lane pair -----------------------------------------------------------------------------------
// Products of residues are accumulated without reduction (mac2) and brought back below q with one Barrett step (fold2 /
// reduce2); the canonical residues of a sum do not depend on when the reductions happen.  moai_ctx_create accepts primes
// below 2^61 only, so a product of two residues is below 2^122 and 63 of them on top of a folded sum or a base below 2^61
// stay below 2^128 (and far inside barrett128's range).  When to fold is the caller's business: every kernel states its
// own period and why it fits.
// The accumulator is four words (lx, hx: the x lane's low and high word; ly, hy: the y lane's) that the kernel declares,
// zeroed, as plain locals or as elements of plain arrays, and that these functions take by reference.  Not a struct on
// purpose: words that sit in a struct, or whose addresses pass through one, are allocated to registers differently once
// they are indexed in an unrolled loop (ct_pt_matmul_kernel: 150 instead of 166 VGPRs), and this layer is meant to compile
// to exactly what the hand-written sums did.
__device__ __forceinline__ void seed2(uint64_t &lx, uint64_t &hx, uint64_t &ly, uint64_t &hy, ulonglong2 base)
{
    lx = base.x;
    ly = base.y;
    hx = hy = 0;
}
__device__ __forceinline__ void mac2(uint64_t &lx, uint64_t &hx, uint64_t &ly, uint64_t &hy, ulonglong2 a, ulonglong2 b)
{
    mac128(lx, hx, a.x, b.x);
    mac128(ly, hy, a.y, b.y);
}
__device__ __forceinline__ void mac2(uint64_t &lx, uint64_t &hx, uint64_t &ly, uint64_t &hy, ulonglong2 a, uint64_t s)
{
    mac128(lx, hx, a.x, s);
    mac128(ly, hy, a.y, s);
}
__device__ __forceinline__ ulonglong2 reduce2(uint64_t lx, uint64_t hx, uint64_t ly, uint64_t hy, uint64_t q, uint64_t cr0, uint64_t cr1)
{
    return make_ulonglong2(barrett128(lx, hx, q, cr0, cr1), barrett128(ly, hy, q, cr0, cr1));
}
__device__ __forceinline__ void fold2(uint64_t &lx, uint64_t &hx, uint64_t &ly, uint64_t &hy, uint64_t q, uint64_t cr0, uint64_t cr1)
{
    seed2(lx, hx, ly, hy, reduce2(lx, hx, ly, hy, q, cr0, cr1));
}

// Cooley-Tukey butterfly, Harvey lazy form: x, y in [0, 4q) -> [0, 4q)   (SEAL/util/ntt.h:30-61,
// dwthandler.h:110-163)
__device__ __forceinline__ void ct_bfly(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2)
{
    uint64_t u = csub(x, q2);
    uint64_t v = mul_shoup_lazy(y, w, wq, q);
    x = u + v;
    y = u + q2 - v;
}

// Cooley-Tukey butterfly without the guard: values grow by 2q per stage, so 16 stages starting below
// 4q stay below 36q.  Used when 36q < 2^64 (every prime of MOAI's chain, <= 58 bits); the pass that
// finishes the transform reduces with one Barrett step.  Same residues as ct_bfly.
__device__ __forceinline__ void ct_bfly_noguard(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2)
{
    uint64_t v = mul_shoup_lazy(y, w, wq, q);
    uint64_t u = x;
    x = u + v;
    y = u + q2 - v;
}

// ---- FP64 arithmetic for primes below 2^51 ---------------------------------------------------------------
// gfx950 issues v_fma_f64 / v_mul_f64 / v_add_f64 / v_rndne_f64 at the rate of ONE 32-bit integer multiply
// (tools/valu_bench: 59 vs 56 lane-ops/clk/CU), and a 64-bit Shoup product costs ten of those multiplies.  For
// q < 2^51 the same exact integers fit the 53-bit significand: values live in the 64-bit registers as doubles
// holding (signed) integers, and
//     y * w - rint(y * (w/q)) * q      with h = RN(y*w), l = fma(y, w, -h) (the exact rounding error of h)
// is computed without any rounding: |y| < 2^52 makes the quotient estimate off by less than 1.5, so the true
// remainder r has |r| < 1.5 q, h - c*q = r - l is an integer below 2^53 (|l| <= 2^50), the fma returns it
// exactly and adding l gives r.  Eight FP64 operations per butterfly instead of ~26 integer ones (measured
// 4.5e12 against 1.7e12 butterflies/s).  The final canonical residues are those of the same exact integers,
// i.e. the reference's.  Everything here relies on -ffp-contract=off plus the explicit fma calls.
// Twiddles are {double w, double RN(w/q)} in a Tw's two words; the mode's (q, q2) arguments carry the bit
// patterns of (double q, double RN(1/q)).
enum
{
    M_LAZY16 = -3, // integer, q < 2^60: M_LAZY8's product, values below 16q, a guard where the bound needs one (lazy16_fwd / lazy16_inv)
    M_LAZY8 = -2,  // integer, q < 2^60: approximate Shoup quotient, values below 8q, see ct_bfly_lazy8; plain forward NTT
    M_GUARD2 = -1, // integer, any q < 2^61: the guard of every SECOND stage only (values below 8q), plain forward NTT
    M_GUARD = 0,   // integer, reference discipline [0,4q)
    M_NOGUARD = 1, // integer, 36 q < 2^64
    M_FPN = 2,     // FP64, 33 q < 2^52 (context.hip build_prime): sixteen stages need no intermediate reduction
    M_FPR = 3      // FP64, q < 2^51: the untouched operand of every butterfly is reduced first
};
// the modes whose butterflies take (2^64 - q, 2^64 - 4q)
constexpr bool mode_lazy(int mode)
{
    return mode == M_LAZY8 || mode == M_LAZY16;
}
// the modes whose butterflies take the bit patterns of (double q, 1/q) and work on doubles
constexpr bool mode_fp(int mode)
{
    return mode == M_FPN || mode == M_FPR;
}

__device__ __forceinline__ double u2d(uint64_t b)
{
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ uint64_t d2u(double d)
{
    return (uint64_t)__double_as_longlong(d);
}
// exact conversion of an integer below 2^53
__device__ __forceinline__ double fp_from_u64(uint64_t v)
{
    return __builtin_fma((double)(uint32_t)(v >> 32), 4294967296.0, (double)(uint32_t)v);
}
// exact conversion of an integer below 2^52 in two cheap steps: its bits are the mantissa of 2^52 + v (an OR on the high
// dword), and subtracting 2^52 is exact.  The key-switch kernels convert sixteen key residues and eight digits per
// thread and digit this way (canonical residues of primes below 2^51) instead of with two v_cvt + one fma.
__device__ __forceinline__ double fp_from_u52(uint64_t v)
{
    return u2d(v | 0x4330000000000000ull) - 4503599627370496.0;
}
// x - rint(x/q) q, |result| <= q/2 (+1): exact for integer |x| < 2^53
__device__ __forceinline__ double fp_red(double x, double q, double qinv)
{
    double c = __builtin_rint(x * qinv);
    return __builtin_fma(-c, q, x);
}
__device__ __forceinline__ double fp_mulmod(double y, double w, double wq, double q)
{
    double h = y * w;
    double l = __builtin_fma(y, w, -h);
    double c = __builtin_rint(y * wq);
    return __builtin_fma(-c, q, h) + l;
}
// y * k - rint(y k / q) q for two plain integers (no precomputed quotient): with |y| <= q/2 + 1 and
// 0 <= k < q < 2^51 the estimate RN(y k) * RN(1/q) is within 0.4 of the real quotient, |result| < 0.9 q
__device__ __forceinline__ double fp_mulmod_q(double y, double k, double q, double qinv)
{
    double h = y * k;
    double l = __builtin_fma(y, k, -h);
    double c = __builtin_rint(h * qinv);
    return __builtin_fma(-c, q, h) + l;
}
// representative in [0, q) as a 64-bit integer
__device__ __forceinline__ uint64_t fp_to_canonical(double x, double q, double qinv)
{
    double r = fp_red(x, q, qinv);
    r = r < 0.0 ? r + q : r;
    return d2u(r + 4503599627370496.0) & 0x000fffffffffffffull; // 2^52 + r has r in its low 52 bits
}

template <bool RED>
__device__ __forceinline__ void ct_bfly_fp(uint64_t &xb, uint64_t &yb, uint64_t wb, uint64_t wqb, uint64_t qb, uint64_t qinvb)
{
    const double q = u2d(qb);
    double u = u2d(xb);
    if (RED)
    {
        u = fp_red(u, q, u2d(qinvb));
    }
    double v = fp_mulmod(u2d(yb), u2d(wb), u2d(wqb), q);
    xb = d2u(u + v);
    yb = d2u(u - v);
}

// The same butterfly with the twiddle given as w alone (8 bytes instead of 16): the quotient is estimated from
// RN(y w) * RN(1/q) like fp_mulmod_q.  The estimate is off by up to 3 * 2^-53 |y|, so the product comes out with
// |v| < 2q for |y| < 2^52: sixteen stages from q/2 stay below 33 q (M_FPN needs 33 q < 2^52, true for primes
// below 2^46.9); M_FPR (q < 2^51, so 2^53 > 4q) reduces BOTH operands first, which keeps |v| < 0.88 q and the outputs below
// 1.38 q.  One stage without the reductions may follow such a stage: with |u|, |y| <= 1.38 q the estimate is off by at most
// 0.5 + 3 * 2^-53 * 1.38 q < 1.54, so |v| < 1.54 q, h - c q = r - l stays an integer below 2^52 (|l| <= 2^49) and the outputs stay
// below 2.92 q < 2^53: exact.  The key switch's contiguous pass therefore reduces at every SECOND stage (its input, the
// strided pass's output, is below 2q).
template <bool RED>
__device__ __forceinline__ void ct_bfly_fp1(uint64_t &xb, uint64_t &yb, double w, double q, double qinv)
{
    double u = u2d(xb), y = u2d(yb);
    if (RED)
    {
        u = fp_red(u, q, qinv);
        y = fp_red(y, q, qinv);
    }
    double v = fp_mulmod_q(y, w, q, qinv);
    xb = d2u(u + v);
    yb = d2u(u - v);
}
// the same with the choice as an argument: a constant once the caller's stage loop is unrolled
__device__ __forceinline__ void ct_bfly_fp1_sel(uint64_t &xb, uint64_t &yb, double w, double q, double qinv, const bool red)
{
    if (red)
    {
        ct_bfly_fp1<true>(xb, yb, w, q, qinv);
    }
    else
    {
        ct_bfly_fp1<false>(xb, yb, w, q, qinv);
    }
}

// Cooley-Tukey butterfly of M_GUARD2.  The reference subtracts 2q from x when x >= 2q in every butterfly to keep
// values below 4q (dwthandler.h:94-146); the Shoup product accepts any 64-bit y and the sums grow by at most 2q per
// stage, so for q < 2^61 one guard per TWO stages is enough: an unguarded stage takes values below 6q to below 8q,
// the next one subtracts 4q when x >= 4q (u < 4q) and is back below 6q.  Residues are unchanged.
template <bool GUARDED>
__device__ __forceinline__ void ct_bfly_guard2(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2)
{
    uint64_t u = GUARDED ? csub(x, q2 << 1) : x;
    uint64_t v = mul_shoup_lazy(y, w, wq, q);
    x = u + v;
    y = u + q2 - v;
}

// ---- M_LAZY8: the integer butterfly with fewer instructions (q < 2^60) ----------------------------------------------
// Instruction counts on gfx950 decide this kernel (PMC: the integer pipes are busy 85 % of the time), and the exact
// Shoup product costs about 20 of the 31 VALU instructions of a butterfly: four partial products plus three register moves
// and a 64-bit add for hi64(y * wq), two three-multiply low products, and a 64-bit subtract that lowers to a carry pair.
// Here:
//  * the quotient takes the two HIGH cross terms only:  t' = y1 q1 + hi32(y1 q0) + hi32(y0 q1)  (y = y1:y0, wq = q1:q0).
//    The exact t = floor(y wq / 2^64) has  t - 2 <= t' <= t  (the dropped low parts of the two cross terms and hi32(y0 q0)
//    sum to less than 3 * 2^32), so  r = y w - t' q  lies in [0, 4q) instead of [0, 2q): two mul_hi, one mad, one add;
//  * r is ONE multiply-add chain modulo 2^64:  y0 w0 + t0 n0  in a 64-bit accumulator, the four cross products into its
//    high word, with n = 2^64 - q read from the per-prime record (no subtract);
//  * every stage guards  u = x - 4q if x >= 4q  by adding 2^64 - 4q and testing the sign (values stay below 8q < 2^63), so
//    x' = u + r < 8q and y' = u + 4q - r in (0, 8q): the same residues as the reference's [0, 4q) discipline.
// The pass that finishes the transform reduces below q with one quotient step and one such conditional subtraction (ntt_finish.h).
__device__ __forceinline__ uint64_t csub_sign(uint64_t x, uint64_t neg_m)
{
    // x - m if x >= m else x, for x < 2^63 and m <= 2^62, given 2^64 - m
    uint64_t d = x + neg_m;
    return (int64_t)d < 0 ? x : d;
}
// (the result's two words are put together by pack64, ntt_finish.h: as a shift and an OR the high word's sum is widened to 64 bits)
__device__ __forceinline__ uint64_t mul_shoup_approx(uint64_t y, uint64_t w, uint64_t wq, uint64_t nq)
{
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32);
    const uint32_t q0 = (uint32_t)wq, q1 = (uint32_t)(wq >> 32);
    uint64_t t = (uint64_t)y1 * q1 + __umulhi(y1, q0);
    t += __umulhi(y0, q1);
    const uint32_t t0 = (uint32_t)t, t1 = (uint32_t)(t >> 32);
    const uint32_t w0 = (uint32_t)w, w1 = (uint32_t)(w >> 32);
    const uint32_t n0 = (uint32_t)nq, n1 = (uint32_t)(nq >> 32);
    uint64_t p = (uint64_t)y0 * w0;
    p += (uint64_t)t0 * n0;
    const uint32_t hi = (uint32_t)(p >> 32) + y0 * w1 + y1 * w0 + t0 * n1 + t1 * n0;
    return pack64((uint32_t)p, hi);
}
// x, y below 8q -> below 8q; nq = 2^64 - q, n4q = 2^64 - 4q
__device__ __forceinline__ void ct_bfly_lazy8(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t nq, uint64_t n4q)
{
    const uint64_t u = csub_sign(x, n4q);
    const uint64_t v = mul_shoup_approx(y, w, wq, nq);
    x = u + v;
    y = u - (v + n4q);
}

// Gentleman-Sande counterparts: x, y below 4q -> below 4q (the sum is guarded, the difference goes through the product,
// which accepts any 64-bit operand); the last stage folds N^-1 in and needs no guard at all
__device__ __forceinline__ void gs_bfly_lazy8(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t nq, uint64_t n4q)
{
    const uint64_t u = x, v = y;
    x = csub_sign(u + v, n4q);
    y = mul_shoup_approx(u - (v + n4q), w, wq, nq);
}
// (tiled kernels, LOGN >= 12: the sum, below 8q, takes N^-1 by shift and comes out below 2q; qh = (q - 1) / N)
template <int LOGN>
__device__ __forceinline__ void gs_bfly_last_lazy8(uint64_t &x, uint64_t &y, uint64_t qh, const Tw &ninv_w1, uint64_t nq, uint64_t n4q)
{
    static_assert(LOGN >= 12, "N^-1 by shift returns less than 2q from logn = 12 on");
    const uint64_t u = x, v = y;
    x = ninv_by_shift(u + v, qh, LOGN);
    y = mul_shoup_approx(u - (v + n4q), ninv_w1.w, ninv_w1.wq, nq);
}
// ---- M_LAZY16: M_LAZY8 with a guard only where the bound needs one (q < 2^60) ------------------------------------------
// M_LAZY8 keeps values below 8q (4q in the inverse) only so that csub_sign can test bit 63.  The approximate product accepts any
// 64-bit operand and 16q < 2^64, so with a guard that tests the CARRY of x + (2^64 - m) values may grow to 16q, and a stage whose
// input bound allows it runs without a guard.  Which stages those are is decided at compile time by the two bound trackers below;
// the kernels static_assert what the trackers prove (no value of 16q or more, the bound one pass hands to the other, the bound
// the existing final subtractions expect).  Bounds are multiples of q, exclusive.  Same residues as every other mode.
__device__ __forceinline__ uint64_t csub_carry(uint64_t x, uint64_t neg_m)
{
    // x - m if x >= m else x, for any x and 0 < m < 2^64, given 2^64 - m: the sum wraps exactly when x >= m
    const uint64_t d = x + neg_m;
    return d < x ? d : x;
}
// Forward: u + v and u + 4q - v are below bound(u) + 4q.  Stages [first, first + count) of a 2^logn transform from bound b0: a
// stage goes unguarded iff its input bound + 4q <= 16q, else x takes one conditional subtraction of 8q (below 16q -> below 8q);
// the transform's last stage brings x below 8q whatever its input bound, so that its outputs are below 12q: the one-step final
// reduction (ntt_finish.h final_quotient_step) accepts 16q.  Bit s of g8: stage s subtracts 8q conditionally.
struct Lazy16Fwd
{
    uint32_t g8;
    int end;  // bound of the outputs of the last stage run
    int peak; // largest bound met
};
constexpr Lazy16Fwd lazy16_fwd(int logn, int first, int count, int b0)
{
    Lazy16Fwd r{ 0, b0, b0 };
    int b = b0;
    for (int s = first; s < first + count; ++s)
    {
        int u = b;
        if (s == logn - 1)
        {
            if (u > 8)
            {
                r.g8 |= 1u << s;
                u = u - 8 > 8 ? u - 8 : 8;
            }
        }
        else if (b + 4 > 16)
        {
            r.g8 |= 1u << s;
            u = b - 8 > 8 ? b - 8 : 8;
        }
        b = u + 4;
        r.peak = b > r.peak ? b : r.peak;
    }
    r.end = b;
    return r;
}
// what the strided pass (stages 0 .. logn-9, from inputs below 8q like M_LAZY8's) hands to the contiguous pass
constexpr int lazy16_fwd_handover(int logn)
{
    return (logn & 1) ? 12 : 16;
}
// G: x takes a conditional subtraction of 8q; nq = 2^64 - q, n4q = 2^64 - 4q
template <bool G>
__device__ __forceinline__ void ct_bfly_lazy16(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t nq, uint64_t n4q)
{
    uint64_t u = x;
    if (G)
    {
        u = csub_carry(u, n4q << 1);
    }
    const uint64_t v = mul_shoup_approx(y, w, wq, nq);
    x = u + v;
    y = u - (v + n4q);
}
// Inverse: the sum u + v doubles the bound, the difference goes through the product and comes out below 4q.  Two sums of 16q
// would not fit 64 bits, so a sum is brought back below 8q at once; what the range buys is that a butterfly whose two inputs are
// both PRODUCTS (below 4q: sum below 8q) needs no guard.  Inside one radix-16 register block that is known per register: after a
// stage of distance h the registers with bit h set hold products, and the next stage (distance 2h) pairs registers that agree in
// bit h.  One block of `count` stages from inputs below bin q: bit i of xk = the butterflies of stage i that are not known to
// take two products (all of stage 0) have inputs up to 8q -- guard the sum with 8q, form the difference as u - v + 8q; otherwise
// inputs below 4q, no guard, u - v + 4q.  The transform's last stage (`last`) guards nothing: its difference goes through the
// product with N^-1 w_1 (below 4q), its sum -- below 16q, as `peak` proves -- through N^-1 by shift (ntt_finish.h ninv_by_shift:
// below 2q), so the two halves of its outputs end with different bounds, `out` and `xlast`.
struct Lazy16Inv
{
    uint32_t xk;
    int out;   // bound of the block's outputs
    int peak;  // largest bound met, sums before their guard included
    int xlast; // `last`: bound of the sums times N^-1
};
constexpr Lazy16Inv lazy16_inv(int count, int bin, bool last)
{
    Lazy16Inv r{ 0, bin, bin, 0 };
    int bx = bin;
    for (int i = 0; i < count; ++i)
    {
        const bool fin = last && i == count - 1;
        const int sum = 2 * bx;
        if (bx > 4)
        {
            r.xk |= 1u << i;
            r.peak = bx > 8 ? 99 : r.peak; // u - v + 8q needs v below 8q
        }
        r.peak = sum > r.peak ? sum : r.peak;
        if (fin)
        {
            r.peak = sum > NINV_SHIFT_IN ? 99 : r.peak;
            r.xlast = NINV_SHIFT_OUT;
        }
        const int xout = fin ? NINV_SHIFT_OUT : (sum > 8 ? (sum - 8 > 8 ? sum - 8 : 8) : sum);
        const int pout = (i > 0 && !fin) ? 8 : 4; // sums of two products; the products themselves
        bx = xout > pout ? xout : pout;
    }
    r.out = bx;
    return r;
}
// what the contiguous pass (two blocks of four stages, inputs below 4q like M_LAZY8's) hands to the strided pass
constexpr int lazy16_inv_handover()
{
    return 8;
}
// K: 1 = inputs below 8q, sum guarded; 0 = inputs below 4q
template <int K>
__device__ __forceinline__ void gs_bfly_lazy16(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t nq, uint64_t n4q)
{
    const uint64_t u = x, v = y;
    x = K ? csub_carry(u + v, n4q << 1) : u + v;
    y = mul_shoup_approx(u - (v + (K ? n4q << 1 : n4q)), w, wq, nq);
}
template <int K, int LOGN>
__device__ __forceinline__ void gs_bfly_last_lazy16(uint64_t &x, uint64_t &y, uint64_t qh, const Tw &ninv_w1, uint64_t nq, uint64_t n4q)
{
    static_assert(LOGN >= 12, "N^-1 by shift returns less than 2q from logn = 12 on");
    const uint64_t u = x, v = y;
    x = ninv_by_shift(u + v, qh, LOGN); // (lazy16_inv: the sum is below 16q)
    y = mul_shoup_approx(u - (v + (K ? n4q << 1 : n4q)), ninv_w1.w, ninv_w1.wq, nq);
}
// the kind of the butterfly on registers (j, j + half) in stage i of a block with schedule xk; a constant once the caller's loops
// are unrolled
__device__ __forceinline__ int lazy16_inv_kind(uint32_t xk, int i, int j, int half)
{
    return (i > 0 && (j & (half >> 1))) ? 0 : (int)((xk >> i) & 1u);
}

// STAGES_LEFT = number of stages after this one (compile-time in the unrolled tiles): M_GUARD2 guards the stages
// with an even number left, so the last stage of a transform is guarded and hands over values below 6q
template <int MODE, int STAGES_LEFT = 0>
__device__ __forceinline__ void ct_bfly_t(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2)
{
    if (MODE == M_LAZY8)
    {
        ct_bfly_lazy8(x, y, w, wq, q, q2); // (q, q2) carry (2^64 - q, 2^64 - 4q)
    }
    else if (MODE == M_GUARD2)
    {
        ct_bfly_guard2<(STAGES_LEFT % 2) == 0>(x, y, w, wq, q, q2);
    }
    else if (MODE == M_FPN)
    {
        ct_bfly_fp<false>(x, y, w, wq, q, q2);
    }
    else if (MODE == M_FPR)
    {
        ct_bfly_fp<true>(x, y, w, wq, q, q2);
    }
    else if (MODE == M_NOGUARD)
    {
        ct_bfly_noguard(x, y, w, wq, q, q2);
    }
    else
    {
        ct_bfly(x, y, w, wq, q, q2);
    }
}

// Gentleman-Sande butterfly, lazy: x, y in [0, 2q) -> [0, 2q)   (dwthandler.h:226-250)
__device__ __forceinline__ void gs_bfly(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2)
{
    uint64_t u = x;
    uint64_t v = y;
    x = csub(u + v, q2);
    y = mul_shoup_lazy(u + q2 - v, w, wq, q);
}

// last inverse stage with N^-1 folded in (dwthandler.h:273-314)
__device__ __forceinline__ void gs_bfly_last(uint64_t &x, uint64_t &y, const Tw &ninv, const Tw &ninv_w1, uint64_t q,
                                             uint64_t q2)
{
    uint64_t u = x;
    uint64_t v = y;
    x = mul_shoup_lazy(csub(u + v, q2), ninv.w, ninv.wq, q);
    y = mul_shoup_lazy(u + q2 - v, ninv_w1.w, ninv_w1.wq, q);
}

// ---- inverse transform in exact FP64 arithmetic (primes below 2^51; the scheme of the forward M_FPN / M_FPR modes) ----------
// Gentleman-Sande butterfly on doubles holding integers: x' = u + v, y' = (u - v) w mod q with the product reduced at once
// (fp_mulmod: exact for |u - v| < 2^52).  The sums double from stage to stage, the products come out below 1.5 q:
//   FPR  (q < 2^51, 2^53 > 4q): sum and difference are reduced in every butterfly (inputs below q, outputs below 0.75 q);
//   FPN  (33 q < 2^52, context.hip build_prime): `redsum` reduces the sum in every FOURTH stage of a pass, and the last stage of the
//        transform multiplies both outputs by N^-1 (gs_bfly_last_fp).  Worst case, counted stage by stage with B the bound on a
//        butterfly's inputs: sum and difference are below 2B, the product below 1.5 q, so B' = max(2B, 1.5 q), or 1.5 q after a
//        `redsum` stage (the folded sum is at most q/2).  The load folds to B = q/2; a block of four stages from there sees
//        differences of q, 3q, 6q, 12q and ends at 1.5 q, every later block sees 3q, 6q, 12q, 24q: that is the second register block
//        of the contiguous pass and every full block of the strided pass, at every degree (the strided pass of N = 2^(12 + r)
//        counts its r + 4 stages from zero, so its last, unfolded stage multiplies sums and differences of at most 24q by N^-1).
//        No operand of a product exceeds 24 q < 33 q < 2^52, no sum before its fold 24 q < 2^53.
// Same exact integers as the integer butterflies, canonical at the end (fp_to_canonical): the reference's residues.
template <bool FPR>
__device__ __forceinline__ void gs_bfly_fp(uint64_t &xb, uint64_t &yb, uint64_t wb, uint64_t wqb, uint64_t qb, uint64_t qinvb, const bool redsum)
{
    const double q = u2d(qb), qi = u2d(qinvb);
    const double u = u2d(xb), v = u2d(yb);
    double s = u + v, d = u - v;
    if (FPR)
    {
        s = fp_red(s, q, qi);
        d = fp_red(d, q, qi);
    }
    else if (redsum)
    {
        s = fp_red(s, q, qi);
    }
    xb = d2u(s);
    yb = d2u(fp_mulmod(d, u2d(wb), u2d(wqb), q));
}
// last stage: x' = (u + v) N^-1, y' = (u - v) (N^-1 w_1); the constants as plain doubles, quotient from RN(1/q)
template <bool FPR>
__device__ __forceinline__ void gs_bfly_last_fp(uint64_t &xb, uint64_t &yb, double ninv, double ninv_w1, double q, double qi)
{
    const double u = u2d(xb), v = u2d(yb);
    double s = u + v, d = u - v;
    if (FPR)
    {
        s = fp_red(s, q, qi);
        d = fp_red(d, q, qi);
    }
    xb = d2u(fp_mulmod_q(s, ninv, q, qi));
    yb = d2u(fp_mulmod_q(d, ninv_w1, q, qi));
}
// The inverse butterfly of MODE with (q, q2) = the mode's two constants (ntt_kernels.hip.h mode_q / mode_q2); redsum: M_FPN's fold
// of the sum.  M_LAZY16 chooses between its two per butterfly (ntt_kernels.hip.h gs_bfly_tile); M_GUARD2 and M_NOGUARD have none.
template <int MODE>
__device__ __forceinline__ void gs_bfly_t(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2, const bool redsum)
{
    static_assert(MODE == M_GUARD || MODE == M_LAZY8 || mode_fp(MODE), "no inverse butterfly of this mode");
    if (MODE == M_LAZY8)
    {
        gs_bfly_lazy8(x, y, w, wq, q, q2);
    }
    else if (mode_fp(MODE))
    {
        gs_bfly_fp<MODE == M_FPR>(x, y, w, wq, q, q2, redsum);
    }
    else
    {
        gs_bfly(x, y, w, wq, q, q2);
    }
}
// the same for the last stage of the transform, N^-1 folded in (the lazy modes have their own: gs_bfly_last_lazy8 / _lazy16)
template <int MODE>
__device__ __forceinline__ void gs_bfly_last_t(uint64_t &x, uint64_t &y, const Tw &ninv, const Tw &ninv_w1, uint64_t q, uint64_t q2)
{
    static_assert(MODE == M_GUARD || mode_fp(MODE), "no inverse butterfly of this mode");
    if (mode_fp(MODE))
    {
        gs_bfly_last_fp<MODE == M_FPR>(x, y, fp_from_u64(ninv.w), fp_from_u64(ninv_w1.w), u2d(q), u2d(q2));
    }
    else
    {
        gs_bfly_last(x, y, ninv, ninv_w1, q, q2);
    }
}

} // namespace moai
