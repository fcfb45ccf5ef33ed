// The device arithmetic helpers (csrc/modarith.hip.h, csrc/ntt_finish.h, the top of csrc/ntt_kernels.hip.h) one by one, on the
// device, against 128-bit integer arithmetic on the host, at the limit prime of every arithmetic mode.
//
//   test_modarith_device [--host-only] LOGN name=prime ... [LOGN name=prime ...]
//
// The primes are those of tests/mode_limits.py chain(LOGN) under their names there.  The program is one table of cases (`cases()`):
// a case names a helper, the primes it applies to, an input generator with its domain, and the contract of the helper's comment.
// Per case one tiny __global__ wrapper (case_kernel<Op>) applies the helper elementwise to arrays; one launch per (case, prime) of at
// most 2^16 inputs.  The host recomputes every element in (unsigned) __int128 and asserts
//   (a) the residue relation, (b) the output bound the comment states, or, where it states none, the domain of the helper that
//   consumes the value in the kernels, (c) for the FP64 helpers: the result is an integer-valued double with exactly the bits of
//   the value that exact integer arithmetic gives (the quotient c = rint(...) is the host's IEEE one: one multiply and one rint).
// No tolerance anywhere: equalities of integers or bit patterns, and inequalities taken from the header's text (1.38 q is
// 100 |r| < 138 q in 128 bits).
// Inputs of a case: every special operand with every special twiddle; for the butterflies every special y with every special
// twiddle (x cycling through its specials) and every special x with every special y (twiddle cycling); then random (operand,
// twiddle) pairs up to 2^16 inputs in all.  Integer specials: 0, 1, q - 1, q, every kq and kq +- 1 below the bound, the bound - 1;
// for "any 64-bit" also 2^64 - 1, 2^64 - 2, 2^63, 2^63 +- 1 and words whose low or high half is all ones or all zeros (the carries
// of the cross terms mul_shoup_approx drops).  Twiddles: 0, 1, 2, q - 1, q - 2, (q +- 1) / 2 and 64 random.  FP operands: 0, +-1,
// +-q/2, +-(q/2 + 1), +-(bound - k) for k = 0..3, and operands y with y w mod q = (q -+ 1) / 2 -+ d: y w / q is then within
// (2d + 1) / 2q < 2^-40 of a half-integer on either side, the rounding boundary of rint.
// --host-only needs no device: it builds the table, checks that every generated input lies in its case's domain, and prints it.
// On any HIP error the program prints it and exits at once with no further launch.  ALL PASS and status 0 only if every case passed.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ntt_kernels.hip.h"

using namespace moai;
typedef unsigned __int128 u128;
typedef __int128 i128;
typedef uint64_t u64;

namespace {

// ---- device side --------------------------------------------------------------------------------------------------------------
struct KA
{
    PrimeConst pc;
    int logn;
    int aux; // the case's parameter (a stage's guard, a flag)
};

template <class Op>
__global__ void case_kernel(const KA k, const u64 *__restrict__ a, const u64 *__restrict__ b, const u64 *__restrict__ w,
                            const u64 *__restrict__ wq, u64 *__restrict__ o0, u64 *__restrict__ o1, const uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
    {
        u64 r0 = 0, r1 = 0;
        Op::run(k, a[i], b[i], w[i], wq[i], r0, r1);
        o0[i] = r0;
        o1[i] = r1;
    }
}

#define OP(name, ...)                                                                                                         \
    struct name                                                                                                               \
    {                                                                                                                         \
        static __device__ __forceinline__ void run(const KA &k, u64 a, u64 b, u64 w, u64 wq, u64 &o0, u64 &o1)                \
        {                                                                                                                     \
            const PrimeConst &p = k.pc;                                                                                       \
            (void)p;                                                                                                          \
            __VA_ARGS__                                                                                                       \
        }                                                                                                                     \
    }
// a helper that takes LOGN as a template argument, under the chain's logn
#define BY_LOGN(call)                                                                                                         \
    switch (k.logn)                                                                                                           \
    {                                                                                                                         \
    case 12: { constexpr int LN = 12; call; break; }                                                                          \
    case 13: { constexpr int LN = 13; call; break; }                                                                          \
    case 14: { constexpr int LN = 14; call; break; }                                                                          \
    case 15: { constexpr int LN = 15; call; break; }                                                                          \
    default: { constexpr int LN = 16; call; break; }                                                                          \
    }

OP(OpShoupLazy, o0 = mul_shoup_lazy(b, w, wq, p.q););
OP(OpBarrett64, o0 = barrett64(a, p.q, p.cr1););
OP(OpBarrett128, o0 = barrett128(a, b, p.q, p.cr0, p.cr1););
OP(OpMulmodBarrett, o0 = mulmod_barrett(a, b, p.q, p.cr0, p.cr1););
OP(OpMac128, o0 = a; o1 = b; mac128(o0, o1, w, wq););
// 63 products on a base, a fold, 63 products by a scalar on the folded sum, the final reduction
OP(OpMac2, u64 lx; u64 hx; u64 ly; u64 hy; seed2(lx, hx, ly, hy, make_ulonglong2(a, b));
   for (int i = 0; i < 63; ++i) { mac2(lx, hx, ly, hy, make_ulonglong2(w, wq), make_ulonglong2(wq, wq)); }
   fold2(lx, hx, ly, hy, p.q, p.cr0, p.cr1);
   for (int i = 0; i < 63; ++i) { mac2(lx, hx, ly, hy, make_ulonglong2(w, wq), w); }
   const ulonglong2 r = reduce2(lx, hx, ly, hy, p.q, p.cr0, p.cr1); o0 = r.x; o1 = r.y;);
OP(OpCsub, o0 = csub(a, b););
OP(OpSubmod, o0 = submod(a, b, p.q););
OP(OpCsubSign, o0 = csub_sign(a, 0 - b););
OP(OpCsubCarry, o0 = csub_carry(a, 0 - b););
OP(OpAdd2, const ulonglong2 r = add2(make_ulonglong2(a, b), make_ulonglong2(w, wq), p.q); o0 = r.x; o1 = r.y;);
OP(OpSub2, const ulonglong2 r = sub2(make_ulonglong2(a, b), make_ulonglong2(w, wq), p.q); o0 = r.x; o1 = r.y;);
OP(OpNeg2, const ulonglong2 r = neg2(make_ulonglong2(a, b), p.q); o0 = r.x; o1 = r.y;);
OP(OpMulmod2, const ulonglong2 r = mulmod2(make_ulonglong2(a, b), make_ulonglong2(w, wq), p.q, p.cr0, p.cr1); o0 = r.x; o1 = r.y;);
OP(OpAddmul2, const ulonglong2 r = addmul2(make_ulonglong2(a, b), make_ulonglong2(w, wq), make_ulonglong2(wq, w), p.q, p.cr0, p.cr1);
   o0 = r.x; o1 = r.y;);
OP(OpShoupApprox, o0 = mul_shoup_approx(b, w, wq, p.nq););
OP(OpCt, o0 = a; o1 = b; ct_bfly_t<M_GUARD>(o0, o1, w, wq, p.q, p.q2););
OP(OpCtNoguard, o0 = a; o1 = b; ct_bfly_t<M_NOGUARD>(o0, o1, w, wq, p.q, p.q2););
OP(OpCtGuard2Off, o0 = a; o1 = b; ct_bfly_guard2<false>(o0, o1, w, wq, p.q, p.q2););
OP(OpCtGuard2On, o0 = a; o1 = b; ct_bfly_guard2<true>(o0, o1, w, wq, p.q, p.q2););
OP(OpCtLazy8, o0 = a; o1 = b; ct_bfly_t<M_LAZY8>(o0, o1, w, wq, p.nq, p.n4q););
OP(OpGsLazy8, o0 = a; o1 = b; gs_bfly_t<M_LAZY8>(o0, o1, w, wq, p.nq, p.n4q, false););
OP(OpGsLastLazy8, o0 = a; o1 = b; BY_LOGN(gs_bfly_last_lazy8<LN>(o0, o1, p.qh, p.ninv_w1, p.nq, p.n4q)););
OP(OpCtLazy16, o0 = a; o1 = b;
   if ((k.aux >> 8) & 1) { ct_bfly_lazy16<true>(o0, o1, w, wq, p.nq, p.n4q); } else { ct_bfly_lazy16<false>(o0, o1, w, wq, p.nq, p.n4q); });
OP(OpLazyFinal, o0 = lazy_final(a, p.nq, ((u64)p.red_s << 32) | p.red_m););
OP(OpGsLazy16K0, o0 = a; o1 = b; gs_bfly_lazy16<0>(o0, o1, w, wq, p.nq, p.n4q););
OP(OpGsLazy16K1, o0 = a; o1 = b; gs_bfly_lazy16<1>(o0, o1, w, wq, p.nq, p.n4q););
OP(OpGsLastLazy16K0, o0 = a; o1 = b; BY_LOGN((gs_bfly_last_lazy16<0, LN>(o0, o1, p.qh, p.ninv_w1, p.nq, p.n4q))););
OP(OpGsLastLazy16K1, o0 = a; o1 = b; BY_LOGN((gs_bfly_last_lazy16<1, LN>(o0, o1, p.qh, p.ninv_w1, p.nq, p.n4q))););
OP(OpGs, o0 = a; o1 = b; gs_bfly_t<M_GUARD>(o0, o1, w, wq, p.q, p.q2, false););
OP(OpGsLast, o0 = a; o1 = b; gs_bfly_last_t<M_GUARD>(o0, o1, p.ninv, p.ninv_w1, p.q, p.q2););
OP(OpNinvShift, o0 = ninv_by_shift(a, p.qh, k.logn););
OP(OpFinalStep, o0 = final_quotient_step(a, p.red_s, p.red_m, p.nq););
OP(OpLoadBarrett, const LoadBarrett op{ p.q, p.cr1 }; o0 = op(a););
// FP64: values travel as the bit patterns of doubles
OP(OpFpFromU64, o0 = d2u(fp_from_u64(a)););
OP(OpFpFromU52, o0 = d2u(fp_from_u52(a)););
OP(OpFpRed, o0 = d2u(fp_red(u2d(a), u2d(p.qd), u2d(p.qinv))););
OP(OpFpMulmod, o0 = d2u(fp_mulmod(u2d(b), u2d(w), u2d(wq), u2d(p.qd))););
OP(OpFpMulmodQ, o0 = d2u(fp_mulmod_q(u2d(b), u2d(w), u2d(p.qd), u2d(p.qinv))););
OP(OpFpToCanonical, o0 = fp_to_canonical(u2d(a), u2d(p.qd), u2d(p.qinv)););
OP(OpCtFpN, o0 = a; o1 = b; ct_bfly_t<M_FPN>(o0, o1, w, wq, p.qd, p.qinv););
OP(OpCtFpR, o0 = a; o1 = b; ct_bfly_t<M_FPR>(o0, o1, w, wq, p.qd, p.qinv););
OP(OpCtFp1Red, o0 = a; o1 = b; ct_bfly_fp1<true>(o0, o1, u2d(w), u2d(p.qd), u2d(p.qinv)););
OP(OpCtFp1, o0 = a; o1 = b; ct_bfly_fp1<false>(o0, o1, u2d(w), u2d(p.qd), u2d(p.qinv)););
OP(OpCtFp1Sel, o0 = a; o1 = b; ct_bfly_fp1_sel(o0, o1, u2d(w), u2d(p.qd), u2d(p.qinv), k.aux != 0););
OP(OpGsFpR, o0 = a; o1 = b; gs_bfly_t<M_FPR>(o0, o1, w, wq, p.qd, p.qinv, (k.aux >> 8) != 0););
OP(OpGsFpN, o0 = a; o1 = b; gs_bfly_t<M_FPN>(o0, o1, w, wq, p.qd, p.qinv, (k.aux >> 8) != 0););
OP(OpGsLastFpN, o0 = a; o1 = b; gs_bfly_last_t<M_FPN>(o0, o1, p.ninv, p.ninv_w1, p.qd, p.qinv););
OP(OpGsLastFpR, o0 = a; o1 = b; gs_bfly_last_t<M_FPR>(o0, o1, p.ninv, p.ninv_w1, p.qd, p.qinv););
OP(OpLoadFp, const LoadFp op{ p.qd, p.qinv }; o0 = op(a););
OP(OpLoadFp52, const LoadFp52 op{ p.qd, p.qinv }; o0 = op(a););
OP(OpLoadBarrettFp, const LoadBarrettFp op{ p.q, p.cr1, p.qd, p.qinv }; o0 = op(a););

[[noreturn]] void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stdout, fmt, ap);
    va_end(ap);
    std::printf("\n");
    std::fflush(stdout);
    std::exit(2);
}
// any HIP error ends the program at once: nothing more is launched
#define HIPX(expr)                                                                              \
    do                                                                                          \
    {                                                                                           \
        const hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                                   \
        {                                                                                       \
            die("HIP error: %s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                       \
    } while (0)

constexpr uint32_t MAX_INPUTS = 1u << 16;

template <class Op>
void launch(const KA &k, const u64 *a, const u64 *b, const u64 *w, const u64 *wq, u64 *o0, u64 *o1, uint32_t n)
{
    if (n == 0 || n > MAX_INPUTS)
    {
        die("launch of %u inputs", n);
    }
    hipLaunchKernelGGL(case_kernel<Op>, dim3((n + 255u) / 256u), dim3(256), 0, 0, k, a, b, w, wq, o0, o1, n);
    HIPX(hipGetLastError());
}

// ---- host arithmetic ----------------------------------------------------------------------------------------------------------
u64 mulmod(u64 a, u64 b, u64 q)
{
    return (u64)((u128)a * b % q);
}
u64 powmod(u64 a, u64 e, u64 q)
{
    u64 r = 1;
    for (a %= q; e; e >>= 1, a = mulmod(a, a, q))
    {
        if (e & 1)
        {
            r = mulmod(r, a, q);
        }
    }
    return r;
}
// the smallest primitive 2N-th root of unity (context.hip minimal_primitive_root)
u64 minimal_root(u64 two_n, u64 q)
{
    const u64 cof = (q - 1) / two_n;
    u64 root = 0;
    for (u64 c = 2; c < 4096 && !root; ++c)
    {
        const u64 r = powmod(c, cof, q);
        if (powmod(r, two_n >> 1, q) == q - 1)
        {
            root = r;
        }
    }
    if (!root)
    {
        die("no primitive root of order %llu mod %llu", (unsigned long long)two_n, (unsigned long long)q);
    }
    const u64 sq = mulmod(root, root, q);
    u64 cur = root, best = root;
    for (u64 i = 0; i < two_n; i += 2)
    {
        best = cur < best ? cur : best;
        cur = mulmod(cur, sq, q);
    }
    return best;
}
// hostmath.h make_tw
Tw make_tw(u64 w, u64 q)
{
    return Tw{ w, (u64)((((u128)w) << 64) / q) };
}
u64 dbits(double d)
{
    u64 b;
    memcpy(&b, &d, 8);
    return b;
}
double bitsd(u64 b)
{
    double d;
    memcpy(&d, &b, 8);
    return d;
}

struct Prime
{
    std::string name;
    int logn;
    u64 q;
    KA ka;
    double qd, qinv;
};

// context.hip build_prime
Prime make_prime(const std::string &name, int logn, u64 q)
{
    Prime P;
    P.name = name;
    P.logn = logn;
    P.q = q;
    const u64 n = 1ull << logn;
    if (q < 3 || q >= (1ull << 61) || (q - 1) % (2 * n))
    {
        die("%s = %llu is no prime = 1 (mod 2N) below 2^61", name.c_str(), (unsigned long long)q);
    }
    PrimeConst &pc = P.ka.pc;
    memset(&P.ka, 0, sizeof(P.ka));
    P.ka.logn = logn;
    pc.q = q;
    pc.q2 = q << 1;
    pc.nq = 0 - q;
    pc.n4q = 0 - (q << 2);
    pc.qh = ninv_shift_qh(q, logn);
    pc.red_s = final_step_shift(q);
    pc.red_m = final_step_mult(q, pc.red_s);
    const u128 hi = (u128)1 << 64;
    pc.cr1 = (u64)(hi / q);
    pc.cr0 = (u64)(((hi % q) << 64) / q);
    P.qd = (double)q;
    P.qinv = 1.0 / P.qd;
    if (q < (1ull << 51))
    {
        pc.qd = dbits(P.qd);
        pc.qinv = dbits(P.qinv);
        pc.fp_mode = (33 * (u128)q < ((u128)1 << 52)) ? 2 : 3;
    }
    const u64 psi = minimal_root(2 * n, q), psi_inv = powmod(psi, q - 2, q);
    const u64 ninv = powmod(n % q, q - 2, q);
    pc.ninv = make_tw(ninv, q);
    pc.ninv_w1 = make_tw(mulmod(ninv, powmod(psi_inv, n >> 1, q), q), q); // inv_tw[1] = psi^-bitrev(1) = psi^-(N/2)
    return P;
}

bool p_all(const Prime &)
{
    return true;
}
bool p_lt60(const Prime &P)
{
    return P.q < (1ull << 60);
}
bool p_noguard(const Prime &P)
{
    return P.q < 0xffffffffffffffffull / 36; // ntt.hip noguard_ok
}
bool p_fp(const Prime &P)
{
    return P.q < (1ull << 51);
}
bool p_fpn(const Prime &P)
{
    return 33 * (u128)P.q < ((u128)1 << 52);
}

struct Rng
{
    u64 s;
    u64 next()
    {
        u64 z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    // uniform below bound (bound <= 2^64)
    u64 below(u128 bound)
    {
        return (u64)(((u128)next() * bound) >> 64);
    }
    // uniform integer with |v| <= maxv
    int64_t sym(int64_t maxv)
    {
        return (int64_t)below(2 * (u128)maxv + 1) - maxv;
    }
};

struct In
{
    std::vector<u64> a, b, w, wq;
    void clear()
    {
        for (std::vector<u64> *v : { &a, &b, &w, &wq })
        {
            v->clear();
            v->reserve(MAX_INPUTS);
        }
    }
    void push(u64 x, u64 y, u64 t, u64 tq)
    {
        if (a.size() < MAX_INPUTS)
        {
            a.push_back(x);
            b.push_back(y);
            w.push_back(t);
            wq.push_back(tq);
        }
        else
        {
            die("more than 2^16 special inputs in one case");
        }
    }
    size_t n() const
    {
        return a.size();
    }
};

// ---- input lists --------------------------------------------------------------------------------------------------------------
void add_unique(std::vector<u64> &v, u64 x)
{
    for (u64 y : v)
    {
        if (y == x)
        {
            return;
        }
    }
    v.push_back(x);
}
// below k q (k q <= 2^64)
std::vector<u64> sp_below(u64 q, int k)
{
    const u128 bound = (u128)k * q;
    std::vector<u64> v;
    auto add = [&](u128 x) {
        if (x < bound)
        {
            add_unique(v, (u64)x);
        }
    };
    add(0);
    add(1);
    add(q - 1);
    add(q);
    for (int j = 1; j <= k; ++j)
    {
        add((u128)j * q - 1);
        add((u128)j * q);
        add((u128)j * q + 1);
    }
    add(bound - 1);
    return v;
}
std::vector<u64> sp_any(u64 q, Rng &r)
{
    int k = 16;
    while ((u128)k * q > ((u128)1 << 64))
    {
        --k;
    }
    std::vector<u64> v = sp_below(q, k);
    const u64 extra[] = { ~0ull, ~0ull - 1, 1ull << 63, (1ull << 63) + 1, (1ull << 63) - 1, 0xffffffff00000000ull, 0x00000000ffffffffull,
                          0x0000000100000000ull, 0xfffffffeffffffffull, 0xffffffff00000001ull, 0x00000001ffffffffull };
    for (u64 x : extra)
    {
        add_unique(v, x);
    }
    for (int i = 0; i < 4; ++i)
    {
        const u64 x = r.next();
        add_unique(v, x | 0xffffffffull);         // low half all ones
        add_unique(v, x & 0xffffffff00000000ull); // low half all zeros
        add_unique(v, x | 0xffffffff00000000ull); // high half all ones
        add_unique(v, x & 0xffffffffull);         // high half all zeros
    }
    return v;
}
// twiddle residues: the specials, then 64 random
std::vector<u64> sp_tw(u64 q, Rng &r)
{
    std::vector<u64> v = { 0, 1, 2, q - 1, q - 2, (q - 1) / 2, (q + 1) / 2 };
    for (int i = 0; i < 64; ++i)
    {
        v.push_back(r.below(q));
    }
    return v;
}
// integers |v| <= maxv
std::vector<int64_t> sp_fp(u64 q, int64_t maxv)
{
    std::vector<int64_t> v;
    auto add = [&](int64_t x) {
        for (int64_t s : { x, -x })
        {
            bool seen = s > maxv || s < -maxv;
            for (int64_t y : v)
            {
                seen = seen || y == s;
            }
            if (!seen)
            {
                v.push_back(s);
            }
        }
    };
    add(0);
    add(1);
    add((int64_t)(q / 2));
    add((int64_t)(q / 2 + 1));
    for (int k = 0; k < 4; ++k)
    {
        add(maxv - k);
    }
    return v;
}
u64 fpb(int64_t v)
{
    return dbits((double)v); // |v| <= 2^53: exact
}
// operands y, |y| <= maxv, with y w mod q within 2^-40 q of q/2 on either side: the balanced representative and the ones next to +-maxv
void half_integer_operands(u64 q, u64 w, int64_t maxv, std::vector<int64_t> &out)
{
    if (w % q == 0)
    {
        return;
    }
    const u64 winv = powmod(w, q - 2, q);
    int dmax = (int)(((q >> 39) - 1) / 2); // (2d + 1) / 2q < 2^-40
    dmax = dmax > 3 ? 3 : dmax;
    for (int d : { 0, dmax })
    {
        for (u64 h : { (q - 1) / 2 - (u64)d, (q + 1) / 2 + (u64)d })
        {
            const int64_t y0 = (int64_t)mulmod(winv, h, q);
            const int64_t bal = y0 > (int64_t)(q / 2) ? y0 - (int64_t)q : y0;
            if (bal <= maxv && bal >= -maxv)
            {
                out.push_back(bal);
            }
            if (maxv >= (int64_t)q)
            {
                const int64_t top = y0 + (maxv - y0) / (int64_t)q * (int64_t)q;
                const int64_t bot = top - (maxv + top) / (int64_t)q * (int64_t)q;
                out.push_back(top);
                out.push_back(bot);
            }
        }
    }
}

enum TwKind
{
    TW_SHOUP, // {w, floor(w 2^64 / q)}
    TW_FP,    // {double w, double RN(w / q)} (context.hip to_fp)
    TW_FP1,   // {double w, 0}
    TW_RES    // two residues
};
Tw enc_tw(const Prime &P, TwKind kind, u64 w, Rng &r)
{
    switch (kind)
    {
    case TW_SHOUP:
        return make_tw(w, P.q);
    case TW_FP:
        return Tw{ dbits((double)w), dbits((double)w / P.qd) };
    case TW_FP1:
        return Tw{ dbits((double)w), 0 };
    default:
        return Tw{ w, r.below(P.q) };
    }
}
bool tw_ok(const Prime &P, TwKind kind, u64 w, u64 wq)
{
    switch (kind)
    {
    case TW_SHOUP:
        return w < P.q && wq == (u64)((((u128)w) << 64) / P.q);
    case TW_FP:
    case TW_FP1: {
        const double d = bitsd(w);
        if (!(d >= 0.0 && d < P.qd && d == __builtin_rint(d)))
        {
            return false;
        }
        return kind == TW_FP1 ? wq == 0 : wq == dbits(d / P.qd);
    }
    default:
        return w < P.q && wq < P.q;
    }
}

// every y with every twiddle (x cycling), every x with every y (twiddle cycling), then random up to 2^16
template <class RX, class RY>
void fill(const Prime &P, Rng &r, In &in, TwKind kind, const std::vector<u64> &X, const std::vector<u64> &Y, RX rx, RY ry)
{
    const std::vector<u64> T = sp_tw(P.q, r);
    size_t i = 0;
    for (u64 y : Y)
    {
        for (u64 t : T)
        {
            const Tw e = enc_tw(P, kind, t, r);
            in.push(X[i++ % X.size()], y, e.w, e.wq);
        }
    }
    if (X.size() > 1)
    {
        for (u64 x : X)
        {
            for (u64 y : Y)
            {
                const Tw e = enc_tw(P, kind, T[i++ % T.size()], r);
                in.push(x, y, e.w, e.wq);
            }
        }
    }
    while (in.n() < MAX_INPUTS)
    {
        const Tw e = enc_tw(P, kind, r.below(P.q), r);
        in.push(rx(), ry(), e.w, e.wq);
    }
}
// integer operands: kx, ky = the bound as a multiple of q, 0 = any 64-bit word; kx < 0: no x operand
void fill_int(const Prime &P, Rng &r, In &in, int kx, int ky, TwKind kind = TW_SHOUP)
{
    const std::vector<u64> X = kx < 0 ? std::vector<u64>{ 0 } : (kx ? sp_below(P.q, kx) : sp_any(P.q, r));
    const std::vector<u64> Y = ky ? sp_below(P.q, ky) : sp_any(P.q, r);
    fill(P, r, in, kind, X, Y, [&] { return kx < 0 ? 0 : (kx ? r.below((u128)kx * P.q) : r.next()); },
         [&] { return ky ? r.below((u128)ky * P.q) : r.next(); });
}
// FP operands: |x| <= mx, |y| <= my; mx < 0: no x operand.  y also takes the operands at the rounding boundary of its product.
void fill_fp(const Prime &P, Rng &r, In &in, int64_t mx, int64_t my, TwKind kind)
{
    std::vector<u64> X = { 0 }, Y;
    if (mx >= 0)
    {
        X.clear();
        for (int64_t v : sp_fp(P.q, mx))
        {
            X.push_back(fpb(v));
        }
    }
    for (int64_t v : sp_fp(P.q, my))
    {
        Y.push_back(fpb(v));
    }
    const std::vector<u64> T = sp_tw(P.q, r);
    size_t i = 0;
    for (u64 t : T)
    {
        std::vector<int64_t> ys;
        half_integer_operands(P.q, t, my, ys);
        const Tw e = enc_tw(P, kind, t, r);
        for (int64_t y : ys)
        {
            in.push(X[i++ % X.size()], fpb(y), e.w, e.wq);
        }
    }
    fill(P, r, in, kind, X, Y, [&] { return mx < 0 ? 0 : fpb(r.sym(mx)); }, [&] { return fpb(r.sym(my)); });
}

// ---- decoding and checking ----------------------------------------------------------------------------------------------------
// the integer an FP64 value holds; false if it holds none
bool fp_int(u64 bits, i128 &v)
{
    const double d = bitsd(bits);
    if (!(d == d) || !(d > -9.0e18 && d < 9.0e18) || d != __builtin_rint(d))
    {
        return false;
    }
    v = (i128)(long long)d;
    return true;
}
bool fp_in(u64 bits, i128 maxv)
{
    i128 v;
    return fp_int(bits, v) && v <= maxv && v >= -maxv && !(v == 0 && bits != 0); // no negative zero among the inputs
}
i128 iabs(i128 v)
{
    return v < 0 ? -v : v;
}
u64 imod(i128 v, u64 q)
{
    const i128 r = v % (i128)q;
    return (u64)(r < 0 ? r + q : r);
}
// the exact integers of the FP64 helpers: the quotient is the helper's own IEEE estimate, everything else integer arithmetic
i128 h_fp_red(const Prime &P, i128 x)
{
    const double c = __builtin_rint((double)(long long)x * P.qinv);
    return x - (i128)(long long)c * (i128)P.q;
}
i128 h_fp_mulmod(const Prime &P, i128 y, u64 w)
{
    const double wq = (double)w / P.qd;
    const double c = __builtin_rint((double)(long long)y * wq);
    return y * (i128)w - (i128)(long long)c * (i128)P.q;
}
i128 h_fp_mulmod_q(const Prime &P, i128 y, u64 k)
{
    const double h = (double)(long long)y * (double)k;
    const double c = __builtin_rint(h * P.qinv);
    return y * (i128)k - (i128)(long long)c * (i128)P.q;
}
const i128 TWO52 = (i128)1 << 52, TWO53 = (i128)1 << 53;

struct Res
{
    const char *why = nullptr; // what failed
    u128 mag = 0;              // the largest output magnitude, for the table of observed maxima
};
#define REQ(cond, text)  \
    do                   \
    {                    \
        if (!(cond))     \
        {                \
            R.why = text; \
            return R;    \
        }                \
    } while (0)
void see(Res &R, u128 v)
{
    R.mag = v > R.mag ? v : R.mag;
}
// an integer output: the residue, and the bound k q
#define INT_OUT(o, residue, k)                                            \
    REQ((o) % q == (residue), "residue of " #o);                          \
    REQ((u128)(o) < (u128)(k) * q, #o " is not below " #k " q");          \
    see(R, (o))
// an FP64 output: the bits of the exact integer `exp`, the residue, and |value| * den < num * q
#define FP_OUT(o, exp, residue, num, den)                                                                   \
    REQ(iabs(exp) < TWO53 && (o) == dbits((double)(long long)(exp)), #o " differs from the exact integer"); \
    REQ(imod((exp), q) == (residue), "residue of " #o);                                                     \
    REQ(iabs(exp) * (den) < (i128)(num) * (i128)q, #o ": " #den " |value| is not below " #num " q");         \
    see(R, (u128)iabs(exp))
// |value| <= q/2 + 1 (fp_red)
#define FP_OUT_HALF(o, exp, residue)                                                                        \
    REQ(iabs(exp) < TWO53 && (o) == dbits((double)(long long)(exp)), #o " differs from the exact integer"); \
    REQ(imod((exp), q) == (residue), "residue of " #o);                                                     \
    REQ(iabs(exp) <= (i128)(q / 2 + 1), #o ": |value| exceeds q/2 + 1");                                     \
    see(R, (u128)iabs(exp))

typedef void (*GenFn)(const Prime &, int aux, Rng &, In &);
typedef bool (*DomFn)(const Prime &, int aux, u64 a, u64 b, u64 w, u64 wq);
typedef Res (*ChkFn)(const Prime &, int aux, u64 a, u64 b, u64 w, u64 wq, u64 o0, u64 o1);
typedef void (*LaunchFn)(const KA &, const u64 *, const u64 *, const u64 *, const u64 *, u64 *, u64 *, uint32_t);

struct Case
{
    std::string name;  // the helper (and the case's parameter)
    const char *cite;  // where the helper and the comment that is its contract stand
    const char *primes;
    bool (*applies)(const Prime &);
    std::string domain, contract;
    int aux;
    LaunchFn run;
    GenFn gen;
    DomFn dom;
    ChkFn chk;
};

#define GEN [](const Prime &P, int aux, Rng &r, In &in)
#define DOM [](const Prime &P, int aux, u64 a, u64 b, u64 w, u64 wq) -> bool
#define CHK [](const Prime &P, int aux, u64 a, u64 b, u64 w, u64 wq, u64 o0, u64 o1) -> Res
#define PRE                    \
    const u64 q = P.q;         \
    Res R;                     \
    (void)aux; (void)a; (void)b; (void)w; (void)wq; (void)o0; (void)o1; (void)q;
#define DPRE const u64 q = P.q; (void)aux; (void)a; (void)b; (void)w; (void)wq; (void)q;

bool below(u64 v, int k, u64 q)
{
    return (u128)v < (u128)k * q;
}
std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// the bounds of the chained FP64 forward stages: inputs |.| <= B(s), B(0) = q/2 + 1 (what the load leaves), growth g/2 q per stage
int64_t chain_bound(u64 q, int s, int g_half)
{
    return (int64_t)(q / 2 + 1) + (int64_t)(((u128)s * g_half * q) / 2);
}
// gs_bfly_fp<false>: the input bound of a stage in half q: q/2 (+1, what the load leaves), q, 1.5 q, 3 q, 6 q, 12 q
int64_t gs_fp_bound(u64 q, int hb)
{
    return hb == 1 ? (int64_t)(q / 2 + 1) : (int64_t)(((u128)hb * q) / 2);
}

std::vector<Case> cases()
{
    std::vector<Case> t;
    const char *ALL = "all", *LT60 = "q < 2^60 (all but g61)", *NG = "36 q < 2^64 (fpn_hi .. ng_hi, small)", *FP = "q < 2^51 (fpn_hi, fpr_lo, fpr_hi, small)",
               *FPN = "33 q < 2^52 (fpn_hi, small)";

    // ---- integer helpers --------------------------------------------------------------------------------------------------------
    t.push_back({ "mul_shoup_lazy", "modarith.hip.h:19", ALL, p_all, "any 64-bit y; w < q, wq = floor(w 2^64 / q)", "= y w (mod q), below 2q", 0, launch<OpShoupLazy>,
                  GEN { fill_int(P, r, in, -1, 0); }, DOM { DPRE return tw_ok(P, TW_SHOUP, w, wq); },
                  CHK { PRE INT_OUT(o0, mulmod(b % q, w, q), 2); return R; } });
    t.push_back({ "barrett64", "modarith.hip.h:56", ALL, p_all, "any 64-bit x", "x mod q, canonical", 0, launch<OpBarrett64>,
                  GEN { fill_int(P, r, in, 0, 1); }, DOM { return true; }, CHK { PRE INT_OUT(o0, a % q, 1); return R; } });
    t.push_back({ "barrett128", "modarith.hip.h:33", ALL, p_all, "any 128-bit (hi:lo)", "(hi:lo) mod q, canonical", 0, launch<OpBarrett128>,
                  GEN { fill(P, r, in, TW_RES, sp_any(P.q, r), sp_any(P.q, r), [&] { return r.next(); }, [&] { return r.next(); }); }, DOM { return true; },
                  CHK { PRE INT_OUT(o0, (u64)((((u128)b << 64) | a) % q), 1); return R; } });
    t.push_back({ "mulmod_barrett", "modarith.hip.h:50", ALL, p_all, "any 64-bit a, b (any 128-bit product)", "a b mod q, canonical", 0, launch<OpMulmodBarrett>,
                  GEN { fill(P, r, in, TW_RES, sp_any(P.q, r), sp_any(P.q, r), [&] { return r.next(); }, [&] { return r.next(); }); }, DOM { return true; },
                  CHK { PRE INT_OUT(o0, mulmod(a % q, b % q, q), 1); return R; } });
    t.push_back({ "mac128", "modarith.hip.h:69", ALL, p_all, "any (hi:lo), any 64-bit a, b", "(hi:lo) + a b modulo 2^128, exactly", 0, launch<OpMac128>,
                  GEN {
                      const std::vector<u64> S = sp_any(P.q, r);
                      size_t i = 0;
                      for (u64 x : S)
                      {
                          for (u64 y : S)
                          {
                              in.push(S[i % S.size()], S[(i / 3) % S.size()], x, y); // every pair of factors
                              in.push(x, y, S[i % S.size()], S[(i / 3) % S.size()]); // every accumulator
                              ++i;
                          }
                      }
                      while (in.n() < MAX_INPUTS)
                      {
                          in.push(r.next(), r.next(), r.next(), r.next());
                      }
                  },
                  DOM { return true; },
                  CHK {
                      PRE const u128 e = (((u128)b << 64) | a) + (u128)w * wq;
                      REQ(o0 == (u64)e && o1 == (u64)(e >> 64), "128-bit sum");
                      return R;
                  } });
    t.push_back({ "seed2 + mac2 (both forms) + fold2 + reduce2", "modarith.hip.h:117", ALL, p_all,
                  "base lanes below 2^61; 63 products of residues (q - 1 among them), fold, 63 more by a scalar", "the sums mod q, canonical", 0, launch<OpMac2>,
                  GEN {
                      const std::vector<u64> S = { 0, 1, P.q - 1, P.q - 2, (P.q - 1) / 2 }, B = { 0, 1, P.q - 1, P.q, (1ull << 61) - 1, 1ull << 60 };
                      for (u64 x : S)
                      {
                          for (u64 y : S)
                          {
                              for (u64 c : B)
                              {
                                  in.push(c, B[(x + y) % B.size()], x, y);
                              }
                          }
                      }
                      while (in.n() < MAX_INPUTS)
                      {
                          in.push(r.below((u128)1 << 61), r.below((u128)1 << 61), r.below(P.q), r.below(P.q));
                      }
                  },
                  DOM { DPRE return a < (1ull << 61) && b < (1ull << 61) && w < q && wq < q; },
                  CHK {
                      PRE const u128 sx = (u128)a + 63 * ((u128)w * wq), sy = (u128)b + 63 * ((u128)wq * wq); // below 2^128: 63 q^2 + 2^61
                      const u128 fx = sx % q + 63 * ((u128)w * w), fy = sy % q + 63 * ((u128)wq * w);
                      INT_OUT(o0, (u64)(fx % q), 1);
                      INT_OUT(o1, (u64)(fy % q), 1);
                      return R;
                  } });
    t.push_back({ "csub", "modarith.hip.h:25", ALL, p_all, "any 64-bit x, m", "x - m if x >= m, else x", 0, launch<OpCsub>,
                  GEN { fill_int(P, r, in, 0, 0, TW_RES); }, DOM { return true; }, CHK { PRE REQ(o0 == (a >= b ? a - b : a), "value"); return R; } });
    t.push_back({ "submod", "modarith.hip.h:63", ALL, p_all, "canonical x, y", "x - y mod q, canonical", 0, launch<OpSubmod>,
                  GEN { fill_int(P, r, in, 1, 1, TW_RES); }, DOM { DPRE return a < q && b < q; },
                  CHK { PRE INT_OUT(o0, (u64)(((u128)a + q - b) % q), 1); return R; } });
    t.push_back({ "csub_sign", "modarith.hip.h:315", ALL, p_all, "x < 2^63, 0 < m <= 2^62 (m = q, 2q, 4q where they fit, 2^62, 1, random)", "x - m if x >= m, else x", 0,
                  launch<OpCsubSign>,
                  GEN {
                      std::vector<u64> M = { 1, 1ull << 62, (1ull << 62) - 1 };
                      for (int k : { 1, 2, 4 })
                      {
                          if ((u128)k * P.q <= (1ull << 62))
                          {
                              M.push_back((u64)k * P.q);
                          }
                      }
                      std::vector<u64> X = { (1ull << 63) - 1, (1ull << 63) - 2, 0xffffffffull, 0x7fffffff00000000ull };
                      for (u64 x : sp_any(P.q, r))
                      {
                          if (x < (1ull << 63))
                          {
                              X.push_back(x);
                          }
                      }
                      for (u64 m : M)
                      {
                          for (u64 x : X)
                          {
                              in.push(x, m, 0, 0);
                          }
                          for (u64 d : { 0ull, 1ull, 2ull })
                          {
                              for (u64 x : std::initializer_list<u64>{ m - (d < m ? d : 0), m + d, m + (1ull << 62) - 1 + d })
                              {
                                  if (x < (1ull << 63))
                                  {
                                      in.push(x, m, 0, 0);
                                  }
                              }
                          }
                      }
                      while (in.n() < MAX_INPUTS)
                      {
                          in.push(r.next() >> 1, 1 + r.below((u128)1 << 62), 0, 0);
                      }
                  },
                  DOM { return a < (1ull << 63) && b > 0 && b <= (1ull << 62); }, CHK { PRE REQ(o0 == (a >= b ? a - b : a), "value"); return R; } });
    t.push_back({ "csub_carry", "modarith.hip.h:368", ALL, p_all, "any 64-bit x, 0 < m < 2^64", "x - m if x >= m, else x", 0, launch<OpCsubCarry>,
                  GEN {
                      std::vector<u64> M = sp_any(P.q, r), X = M;
                      M.erase(M.begin()); // (0)
                      for (u64 m : M)
                      {
                          for (u64 x : X)
                          {
                              in.push(x, m, 0, 0);
                          }
                          in.push(m - 1, m, 0, 0);
                          in.push(m + 1, m, 0, 0);
                      }
                      while (in.n() < MAX_INPUTS)
                      {
                          const u64 m = r.next() | ((in.n() & 1) ? 0 : 1ull << 63); // half of them above 2^63: the difference's sign says nothing
                          in.push(r.next(), m ? m : 1, 0, 0);
                      }
                  },
                  DOM { return b > 0; }, CHK { PRE REQ(o0 == (a >= b ? a - b : a), "value"); return R; } });
    t.push_back({ "add2", "modarith.hip.h:78", ALL, p_all, "canonical lanes", "x + y mod q, canonical", 0, launch<OpAdd2>,
                  GEN { fill_int(P, r, in, 1, 1, TW_RES); }, DOM { DPRE return a < q && b < q && w < q && wq < q; },
                  CHK { PRE INT_OUT(o0, (u64)(((u128)a + w) % q), 1); INT_OUT(o1, (u64)(((u128)b + wq) % q), 1); return R; } });
    t.push_back({ "sub2", "modarith.hip.h:82", ALL, p_all, "canonical lanes", "x - y mod q, canonical", 0, launch<OpSub2>,
                  GEN { fill_int(P, r, in, 1, 1, TW_RES); }, DOM { DPRE return a < q && b < q && w < q && wq < q; },
                  CHK { PRE INT_OUT(o0, (u64)(((u128)a + q - w) % q), 1); INT_OUT(o1, (u64)(((u128)b + q - wq) % q), 1); return R; } });
    t.push_back({ "neg2", "modarith.hip.h:86", ALL, p_all, "canonical lanes", "-x mod q, canonical", 0, launch<OpNeg2>,
                  GEN { fill_int(P, r, in, 1, 1, TW_RES); }, DOM { DPRE return a < q && b < q; },
                  CHK { PRE INT_OUT(o0, (q - a) % q, 1); INT_OUT(o1, (q - b) % q, 1); return R; } });
    t.push_back({ "mulmod2", "modarith.hip.h:90", ALL, p_all, "canonical lanes", "x y mod q, canonical", 0, launch<OpMulmod2>,
                  GEN { fill_int(P, r, in, 1, 1, TW_RES); }, DOM { DPRE return a < q && b < q && w < q && wq < q; },
                  CHK { PRE INT_OUT(o0, mulmod(a, w, q), 1); INT_OUT(o1, mulmod(b, wq, q), 1); return R; } });
    t.push_back({ "addmul2", "modarith.hip.h:95", ALL, p_all, "canonical lanes", "acc + x y mod q, canonical", 0, launch<OpAddmul2>,
                  GEN { fill_int(P, r, in, 1, 1, TW_RES); }, DOM { DPRE return a < q && b < q && w < q && wq < q; },
                  CHK { PRE INT_OUT(o0, (u64)(((u128)a + mulmod(w, wq, q)) % q), 1); INT_OUT(o1, (u64)(((u128)b + mulmod(wq, w, q)) % q), 1); return R; } });
    t.push_back({ "mul_shoup_approx", "modarith.hip.h:322", LT60, p_lt60, "any 64-bit y; w < q, wq = floor(w 2^64 / q)",
                  "= y w (mod q), below 4q; the quotient used is t - 2 <= t' <= t", 0, launch<OpShoupApprox>, GEN { fill_int(P, r, in, -1, 0); },
                  DOM { DPRE return tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE INT_OUT(o0, mulmod(b % q, w, q), 4);
                      const u128 tp = ((u128)b * w - o0) / q, tt = ((u128)b * wq) >> 64; // y w - t' q = the result
                      REQ(tp <= tt && tp + 2 >= tt, "the quotient estimate is not within [t - 2, t]");
                      return R;
                  } });
    t.push_back({ "ct_bfly (through ct_bfly_t<M_GUARD>)", "modarith.hip.h:138", ALL, p_all, "x, y below 4q", "x + y w, x - y w (mod q), below 4q", 0, launch<OpCt>,
                  GEN { fill_int(P, r, in, 4, 4); }, DOM { DPRE return below(a, 4, q) && below(b, 4, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE const u64 yw = mulmod(b % q, w, q);
                      INT_OUT(o0, (u64)(((u128)a % q + yw) % q), 4);
                      INT_OUT(o1, (u64)(((u128)a % q + q - yw) % q), 4);
                      return R;
                  } });
    for (int B = 4; B <= 34; B += 2)
    {
        t.push_back({ fmt("ct_bfly_noguard (through ct_bfly_t<M_NOGUARD>), B = %d", B), "modarith.hip.h:149", NG, p_noguard, fmt("x, y below %d q", B),
                      fmt("x + y w, x - y w (mod q), below %d q; the two sum to 2x + 2q in 128 bits (no wrap)", B + 2), B, launch<OpCtNoguard>,
                      GEN { fill_int(P, r, in, aux, aux); }, DOM { DPRE return below(a, aux, q) && below(b, aux, q) && tw_ok(P, TW_SHOUP, w, wq); },
                      CHK {
                          PRE const u64 yw = mulmod(b % q, w, q);
                          INT_OUT(o0, (u64)(((u128)a % q + yw) % q), aux + 2);
                          INT_OUT(o1, (u64)(((u128)a % q + q - yw) % q), aux + 2);
                          REQ((u128)o0 + o1 == 2 * (u128)a + 2 * (u128)q, "the outputs do not sum to 2x + 2q");
                          return R;
                      } });
    }
    t.push_back({ "ct_bfly_guard2<false>", "modarith.hip.h:294", ALL, p_all, "x, y below 6q", "x + y w, x - y w (mod q), below 8q", 0, launch<OpCtGuard2Off>,
                  GEN { fill_int(P, r, in, 6, 6); }, DOM { DPRE return below(a, 6, q) && below(b, 6, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE const u64 yw = mulmod(b % q, w, q);
                      INT_OUT(o0, (u64)(((u128)a % q + yw) % q), 8);
                      INT_OUT(o1, (u64)(((u128)a % q + q - yw) % q), 8);
                      return R;
                  } });
    t.push_back({ "ct_bfly_guard2<true>", "modarith.hip.h:294", ALL, p_all, "x, y below 8q", "x + y w, x - y w (mod q), below 6q", 0, launch<OpCtGuard2On>,
                  GEN { fill_int(P, r, in, 8, 8); }, DOM { DPRE return below(a, 8, q) && below(b, 8, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE const u64 yw = mulmod(b % q, w, q);
                      INT_OUT(o0, (u64)(((u128)a % q + yw) % q), 6);
                      INT_OUT(o1, (u64)(((u128)a % q + q - yw) % q), 6);
                      return R;
                  } });
    t.push_back({ "ct_bfly_lazy8 (through ct_bfly_t<M_LAZY8>)", "modarith.hip.h:337", LT60, p_lt60, "x, y below 8q", "x + y w, x - y w (mod q), below 8q", 0,
                  launch<OpCtLazy8>, GEN { fill_int(P, r, in, 8, 8); }, DOM { DPRE return below(a, 8, q) && below(b, 8, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE const u64 yw = mulmod(b % q, w, q);
                      INT_OUT(o0, (u64)(((u128)a % q + yw) % q), 8);
                      INT_OUT(o1, (u64)(((u128)a % q + q - yw) % q), 8);
                      return R;
                  } });
    t.push_back({ "gs_bfly_lazy8 (through gs_bfly_t<M_LAZY8>)", "modarith.hip.h:347", LT60, p_lt60, "x, y below 4q", "x + y, (x - y) w (mod q), below 4q", 0,
                  launch<OpGsLazy8>, GEN { fill_int(P, r, in, 4, 4); }, DOM { DPRE return below(a, 4, q) && below(b, 4, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE INT_OUT(o0, (u64)(((u128)a + b) % q), 4);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 4 * (u128)q - b) % q), w, q), 4);
                      return R;
                  } });
    t.push_back({ "gs_bfly_last_lazy8<LOGN>, LOGN = the chain's (12 and 16)", "modarith.hip.h:355", LT60, p_lt60, "x, y below 4q",
                  "(x + y) N^-1 below 2q, (x - y) N^-1 w_1 below 4q (mod q)", 0, launch<OpGsLastLazy8>, GEN { fill_int(P, r, in, 4, 4); },
                  DOM { DPRE return below(a, 4, q) && below(b, 4, q); },
                  CHK {
                      PRE INT_OUT(o0, mulmod((u64)(((u128)a + b) % q), P.ka.pc.ninv.w, q), 2);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 4 * (u128)q - b) % q), P.ka.pc.ninv_w1.w, q), 4);
                      return R;
                  } });
    // ct_bfly_lazy16<G>: every (input bound, guard, output bound) that lazy16_fwd schedules for the two passes of logn = 12 .. 16
    {
        std::vector<int> seen;
        for (int logn = 12; logn <= 16; ++logn)
        {
            const int R1 = logn - 8;
            const Lazy16Fwd p1 = lazy16_fwd(logn, 0, R1, 8), p2 = lazy16_fwd(logn, R1, 8, lazy16_fwd_handover(logn));
            if (p1.peak > 16 || p2.peak > 16 || p1.end != lazy16_fwd_handover(logn) || p2.end > FINAL_STEP_IN)
            {
                die("lazy16_fwd: the schedule of logn = %d breaks what the kernels assert", logn);
            }
            for (int s = 0; s < logn; ++s)
            {
                const int first = s < R1 ? 0 : R1, b0 = s < R1 ? 8 : lazy16_fwd_handover(logn);
                const int bin = lazy16_fwd(logn, first, s - first, b0).end;
                const Lazy16Fwd r = lazy16_fwd(logn, first, s - first + 1, b0);
                const int g = (int)((r.g8 >> s) & 1u), key = bin | (g << 8) | (r.end << 16);
                bool dup = false;
                for (int k : seen)
                {
                    dup = dup || k == key;
                }
                if (!dup)
                {
                    seen.push_back(key);
                    t.push_back({ fmt("ct_bfly_lazy16<%s>, inputs below %d q", g ? "true" : "false", bin), "modarith.hip.h:417", LT60, p_lt60,
                                  fmt("x, y below %d q, a stage lazy16_fwd runs %s (first met: logn %d, stage %d)", bin, g ? "with the guard" : "unguarded", logn, s),
                                  fmt("x + y w, x - y w (mod q), below %d q, the tracker's next bound", r.end), key, launch<OpCtLazy16>,
                                  GEN { fill_int(P, r, in, aux & 255, aux & 255); },
                                  DOM { DPRE return below(a, aux & 255, q) && below(b, aux & 255, q) && tw_ok(P, TW_SHOUP, w, wq); },
                                  CHK {
                                      PRE const u64 yw = mulmod(b % q, w, q);
                                      const int bout = aux >> 16;
                                      REQ(bout <= 16, "the tracker allows 16 q or more");
                                      INT_OUT(o0, (u64)(((u128)a % q + yw) % q), bout);
                                      INT_OUT(o1, (u64)(((u128)a % q + q - yw) % q), bout);
                                      // the guard is used exactly where g8 says: the outputs sum to 2u + 4q with u = x, or x - 8q where x >= 8q
                                      const u128 u = (((aux >> 8) & 1) && (u128)a >= 8 * (u128)q) ? (u128)a - 8 * (u128)q : (u128)a;
                                      REQ((u128)o0 + o1 == 2 * u + 4 * (u128)q, "the outputs do not sum to 2u + 4q: the guard differs from the schedule's");
                                      return R;
                                  } });
                    t.back().aux = key;
                }
            }
        }
    }
    t.push_back({ "lazy_final", "ntt_kernels.hip.h:115", LT60, p_lt60, "z below 16q", "z mod q, canonical", 0, launch<OpLazyFinal>, GEN { fill_int(P, r, in, 16, 1); },
                  DOM { DPRE return below(a, 16, q); }, CHK { PRE INT_OUT(o0, a % q, 1); return R; } });
    // the inverse schedule: every stage lazy16_inv runs with K = 1 has inputs below 8q, every other one inputs below 4q
    for (int rb = 0; rb <= 4; ++rb)
    {
        const Lazy16Inv z1 = lazy16_inv(4, 4, false), z2 = lazy16_inv(4, z1.out, false), zb = lazy16_inv(rb, lazy16_inv_handover(), false),
                        za = lazy16_inv(4, zb.out, true);
        if (z1.peak > 16 || z2.peak > 16 || zb.peak > 16 || za.peak > 16 || z2.out != lazy16_inv_handover() || za.out > 4 || za.xlast > 2)
        {
            die("lazy16_inv: the schedule of logn = %d breaks what the kernels assert", 12 + rb);
        }
        const struct
        {
            int count, bin;
            bool last;
        } blocks[] = { { 4, 4, false }, { 4, z1.out, false }, { rb, lazy16_inv_handover(), false }, { 4, zb.out, true } };
        for (const auto &bl : blocks)
        {
            const uint32_t xk = lazy16_inv(bl.count, bl.bin, bl.last).xk;
            for (int i = 0; i < bl.count; ++i)
            {
                const int bx = lazy16_inv(i, bl.bin, false).out;
                if (bx > (((xk >> i) & 1u) ? 8 : 4))
                {
                    die("lazy16_inv: stage %d of a block from %d q has inputs below %d q with K = %u", i, bl.bin, bx, (xk >> i) & 1u);
                }
            }
        }
    }
    t.push_back({ "gs_bfly_lazy16<0>", "modarith.hip.h:477", LT60, p_lt60, "x, y below 4q (lazy16_inv: every stage with K = 0)", "x + y below 8q, (x - y) w below 4q (mod q)",
                  0, launch<OpGsLazy16K0>, GEN { fill_int(P, r, in, 4, 4); }, DOM { DPRE return below(a, 4, q) && below(b, 4, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE INT_OUT(o0, (u64)(((u128)a + b) % q), 8);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 8 * (u128)q - b) % q), w, q), 4);
                      return R;
                  } });
    t.push_back({ "gs_bfly_lazy16<1>", "modarith.hip.h:477", LT60, p_lt60, "x, y below 8q (lazy16_inv: every stage with K = 1)", "x + y below 8q, (x - y) w below 4q (mod q)",
                  0, launch<OpGsLazy16K1>, GEN { fill_int(P, r, in, 8, 8); }, DOM { DPRE return below(a, 8, q) && below(b, 8, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE INT_OUT(o0, (u64)(((u128)a + b) % q), 8);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 8 * (u128)q - b) % q), w, q), 4);
                      return R;
                  } });
    t.push_back({ "gs_bfly_last_lazy16<0, LOGN>, LOGN = the chain's (12 and 16)", "modarith.hip.h:484", LT60, p_lt60, "x, y below 4q",
                  "(x + y) N^-1 below 2q (lazy16_inv xlast), (x - y) N^-1 w_1 below 4q (mod q)", 0, launch<OpGsLastLazy16K0>, GEN { fill_int(P, r, in, 4, 4); },
                  DOM { DPRE return below(a, 4, q) && below(b, 4, q); },
                  CHK {
                      PRE INT_OUT(o0, mulmod((u64)(((u128)a + b) % q), P.ka.pc.ninv.w, q), 2);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 8 * (u128)q - b) % q), P.ka.pc.ninv_w1.w, q), 4);
                      return R;
                  } });
    t.push_back({ "gs_bfly_last_lazy16<1, LOGN>, LOGN = the chain's (12 and 16)", "modarith.hip.h:484", LT60, p_lt60, "x, y below 8q (the sum below 16q)",
                  "(x + y) N^-1 below 2q (lazy16_inv xlast), (x - y) N^-1 w_1 below 4q (mod q)", 0, launch<OpGsLastLazy16K1>, GEN { fill_int(P, r, in, 8, 8); },
                  DOM { DPRE return below(a, 8, q) && below(b, 8, q); },
                  CHK {
                      PRE INT_OUT(o0, mulmod((u64)(((u128)a + b) % q), P.ka.pc.ninv.w, q), 2);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 8 * (u128)q - b) % q), P.ka.pc.ninv_w1.w, q), 4);
                      return R;
                  } });
    t.push_back({ "gs_bfly (through gs_bfly_t<M_GUARD>)", "modarith.hip.h:530", ALL, p_all, "x, y below 2q", "x + y, (x - y) w (mod q), below 2q", 0, launch<OpGs>,
                  GEN { fill_int(P, r, in, 2, 2); }, DOM { DPRE return below(a, 2, q) && below(b, 2, q) && tw_ok(P, TW_SHOUP, w, wq); },
                  CHK {
                      PRE INT_OUT(o0, (u64)(((u128)a + b) % q), 2);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 2 * (u128)q - b) % q), w, q), 2);
                      return R;
                  } });
    t.push_back({ "gs_bfly_last (through gs_bfly_last_t<M_GUARD>)", "modarith.hip.h:539", ALL, p_all, "x, y below 2q", "(x + y) N^-1, (x - y) N^-1 w_1 (mod q), below 2q", 0,
                  launch<OpGsLast>, GEN { fill_int(P, r, in, 2, 2); }, DOM { DPRE return below(a, 2, q) && below(b, 2, q); },
                  CHK {
                      PRE INT_OUT(o0, mulmod((u64)(((u128)a + b) % q), P.ka.pc.ninv.w, q), 2);
                      INT_OUT(o1, mulmod((u64)(((u128)a + 2 * (u128)q - b) % q), P.ka.pc.ninv_w1.w, q), 2);
                      return R;
                  } });
    // the input classes of test_ntt_finish_arith.cpp: 0, 1, N - 1, N, q - 1, q, every k q, the bound - 1, - (N - 1), - N, random below 16q
    t.push_back({ "ninv_by_shift, logn = the chain's", "ntt_finish.h:41", LT60, p_lt60, "x below 16q", "x N^-1 (mod q), below 2q", 0, launch<OpNinvShift>,
                  GEN {
                      const u64 n = 1ull << P.logn, bound = 16 * P.q;
                      std::vector<u64> X = sp_below(P.q, 16);
                      for (u64 x : { n - 1, n, n + 1, bound - (n - 1), bound - n, bound - n - 1, P.q - 1 + n, 15 * P.q + n })
                      {
                          add_unique(X, x);
                      }
                      fill(P, r, in, TW_RES, X, { 0 }, [&] { return r.below((u128)16 * P.q); }, [&] { return 0; });
                  },
                  DOM { DPRE return below(a, 16, q); }, CHK { PRE INT_OUT(o0, mulmod(a % q, P.ka.pc.ninv.w, q), 2); return R; } });
    t.push_back({ "final_quotient_step", "ntt_finish.h:55", LT60, p_lt60, "z below 16q", "z mod q or z mod q + q", 0, launch<OpFinalStep>,
                  GEN {
                      const u64 n = 1ull << P.logn, bound = 16 * P.q;
                      std::vector<u64> X = sp_below(P.q, 16);
                      for (u64 x : { n - 1, n, bound - (n - 1), bound - n })
                      {
                          add_unique(X, x);
                      }
                      fill(P, r, in, TW_RES, X, { 0 }, [&] { return r.below((u128)16 * P.q); }, [&] { return 0; });
                  },
                  DOM { DPRE return below(a, 16, q); }, CHK { PRE INT_OUT(o0, a % q, 2); return R; } });
    t.push_back({ "LoadBarrett", "ntt_kernels.hip.h:134", ALL, p_all, "any 64-bit v", "v mod q, canonical", 0, launch<OpLoadBarrett>, GEN { fill_int(P, r, in, 0, 1); },
                  DOM { return true; }, CHK { PRE INT_OUT(o0, a % q, 1); return R; } });

    // ---- FP64 helpers: values are integer-valued doubles ------------------------------------------------------------------------
    t.push_back({ "fp_from_u64", "modarith.hip.h:200", FP, p_fp, "integer v below 2^53", "the double that holds v, exactly", 0, launch<OpFpFromU64>,
                  GEN {
                      std::vector<u64> X = sp_below(P.q, 2);
                      for (u64 x : { (1ull << 53) - 1, (1ull << 53) - 2, 1ull << 52, (1ull << 52) + 1, (1ull << 52) - 1, 0xffffffffull, 1ull << 32, (1ull << 32) + 1,
                                     0x1fffff00000000ull, 0x1fffff00000001ull, 0x100000ffffffffull })
                      {
                          add_unique(X, x);
                      }
                      fill(P, r, in, TW_RES, X, { 0 }, [&] { return r.below((u128)1 << 53); }, [&] { return 0; });
                  },
                  DOM { return a < (1ull << 53); }, CHK { PRE REQ(o0 == dbits((double)a), "value"); return R; } });
    t.push_back({ "fp_from_u52", "modarith.hip.h:207", FP, p_fp, "integer v below 2^52", "the double that holds v, exactly", 0, launch<OpFpFromU52>,
                  GEN {
                      std::vector<u64> X = sp_below(P.q, 1);
                      for (u64 x : { (1ull << 52) - 1, (1ull << 52) - 2, 1ull << 51, (1ull << 51) + 1, 0xffffffffull, 1ull << 32, (1ull << 32) + 1, 0xfffff00000000ull,
                                     0xfffff00000001ull })
                      {
                          add_unique(X, x);
                      }
                      fill(P, r, in, TW_RES, X, { 0 }, [&] { return r.below((u128)1 << 52); }, [&] { return 0; });
                  },
                  DOM { return a < (1ull << 52); }, CHK { PRE REQ(o0 == dbits((double)a), "value"); return R; } });
    t.push_back({ "fp_red", "modarith.hip.h:212", FP, p_fp, "integer |x| < 2^53, among them k q + (q +- 1) / 2", "= x (mod q), |r| <= q/2 + 1, exact", 0, launch<OpFpRed>,
                  GEN {
                      const int64_t maxv = (1ll << 53) - 1, q = (int64_t)P.q, top = maxv / q - 1;
                      for (int64_t k : { (int64_t)0, (int64_t)1, top / 2, top })
                      {
                          for (int64_t h : { (q - 1) / 2, (q + 1) / 2, (q - 3) / 2, (q + 3) / 2 })
                          {
                              in.push(0, fpb(k * q + h), 0, 0);
                              in.push(0, fpb(-(k * q + h)), 0, 0);
                          }
                      }
                      fill_fp(P, r, in, -1, maxv, TW_FP);
                      std::swap(in.a, in.b); // the operand travels in a
                  },
                  DOM { return fp_in(a, TWO53 - 1); },
                  CHK {
                      PRE i128 x;
                      fp_int(a, x);
                      const i128 e = h_fp_red(P, x);
                      FP_OUT_HALF(o0, e, imod(x, q));
                      return R;
                  } });
    t.push_back({ "fp_mulmod", "modarith.hip.h:217", FP, p_fp, "integer |y| < 2^52; {w, RN(w/q)}, w < q", "= y w (mod q), |r| < 1.5 q, exact", 0, launch<OpFpMulmod>,
                  GEN { fill_fp(P, r, in, -1, (1ll << 52) - 1, TW_FP); }, DOM { return fp_in(b, TWO52 - 1) && tw_ok(P, TW_FP, w, wq); },
                  CHK {
                      PRE i128 y;
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w);
                      const i128 e = h_fp_mulmod(P, y, wi);
                      FP_OUT(o0, e, mulmod(imod(y, q), wi, q), 3, 2);
                      return R;
                  } });
    t.push_back({ "fp_mulmod_q, |y| <= q/2 + 1", "modarith.hip.h:226", FP, p_fp, "integer |y| <= q/2 + 1; integer 0 <= k < q", "= y k (mod q), |r| < 0.9 q, exact", 0,
                  launch<OpFpMulmodQ>, GEN { fill_fp(P, r, in, -1, (int64_t)(P.q / 2 + 1), TW_FP1); },
                  DOM { DPRE return fp_in(b, (i128)(q / 2 + 1)) && tw_ok(P, TW_FP1, w, wq); },
                  CHK {
                      PRE i128 y;
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w);
                      const i128 e = h_fp_mulmod_q(P, y, wi);
                      FP_OUT(o0, e, mulmod(imod(y, q), wi, q), 9, 10);
                      return R;
                  } });
    t.push_back({ "fp_mulmod_q, |y| < 2^52", "modarith.hip.h:226", FP, p_fp, "integer |y| < 2^52; integer 0 <= k < q (the comment of ct_bfly_fp1)",
                  "= y k (mod q), |r| < 2 q, exact", 0,
                  launch<OpFpMulmodQ>, GEN { fill_fp(P, r, in, -1, (1ll << 52) - 1, TW_FP1); }, DOM { return fp_in(b, TWO52 - 1) && tw_ok(P, TW_FP1, w, wq); },
                  CHK {
                      PRE i128 y;
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w);
                      const i128 e = h_fp_mulmod_q(P, y, wi);
                      FP_OUT(o0, e, mulmod(imod(y, q), wi, q), 2, 1);
                      return R;
                  } });
    t.push_back({ "fp_mulmod_q, |y| <= 24 q", "modarith.hip.h:226", FPN, p_fpn, "integer |y| <= 24 q (what gs_bfly_last_fp<false> feeds it); integer 0 <= k < q",
                  "= y k (mod q), |r| < 2 q, exact", 0, launch<OpFpMulmodQ>, GEN { fill_fp(P, r, in, -1, (int64_t)(24 * P.q), TW_FP1); },
                  DOM { DPRE return fp_in(b, (i128)24 * q) && tw_ok(P, TW_FP1, w, wq); },
                  CHK {
                      PRE i128 y;
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w);
                      const i128 e = h_fp_mulmod_q(P, y, wi);
                      FP_OUT(o0, e, mulmod(imod(y, q), wi, q), 2, 1);
                      return R;
                  } });
    t.push_back({ "fp_to_canonical", "modarith.hip.h:234", FP, p_fp, "integer |x| < 2^53", "x mod q in [0, q) as a 64-bit integer", 0, launch<OpFpToCanonical>,
                  GEN {
                      fill_fp(P, r, in, -1, (1ll << 53) - 1, TW_FP);
                      std::swap(in.a, in.b);
                  },
                  DOM { return fp_in(a, TWO53 - 1); },
                  CHK {
                      PRE i128 x;
                      fp_int(a, x);
                      INT_OUT(o0, imod(x, q), 1);
                      return R;
                  } });
    for (int s = 0; s < 16; ++s)
    {
        t.push_back({ fmt("ct_bfly_fp<false> (through ct_bfly_t<M_FPN>), stage %d of 16 from q/2", s), "modarith.hip.h:242", FPN, p_fpn,
                      fmt("integer |x|, |y| <= q/2 + 1 + %d * 1.5 q; {w, RN(w/q)}", s), fmt("x + y w, x - y w (mod q), |.| <= q/2 + 1 + %d * 1.5 q, exact", s + 1), s,
                      launch<OpCtFpN>, GEN { fill_fp(P, r, in, chain_bound(P.q, aux, 3), chain_bound(P.q, aux, 3), TW_FP); },
                      DOM { DPRE return fp_in(a, chain_bound(q, aux, 3)) && fp_in(b, chain_bound(q, aux, 3)) && tw_ok(P, TW_FP, w, wq); },
                      CHK {
                          PRE i128 x, y;
                          fp_int(a, x);
                          fp_int(b, y);
                          const u64 wi = (u64)bitsd(w), yw = mulmod(imod(y, q), wi, q);
                          const i128 v = h_fp_mulmod(P, y, wi), e0 = x + v, e1 = x - v, lim = (i128)chain_bound(q, aux + 1, 3) + 1;
                          REQ(lim <= TWO52, "the chain leaves 2^52");
                          REQ(iabs(e0) < lim && iabs(e1) < lim, "an output exceeds the stage's bound");
                          FP_OUT(o0, e0, (imod(x, q) + yw) % q, 33, 1);
                          FP_OUT(o1, e1, (imod(x, q) + q - yw) % q, 33, 1);
                          return R;
                      } });
    }
    t.push_back({ "ct_bfly_fp<true> (through ct_bfly_t<M_FPR>)", "modarith.hip.h:242", FP, p_fp, "integer |x| < 2^53, |y| < 2^52; {w, RN(w/q)}",
                  "x + y w, x - y w (mod q), |.| < 2 q + 1 (q/2 + 1 and 1.5 q) and below 2^52, the next stage's domain; exact", 0, launch<OpCtFpR>,
                  GEN { fill_fp(P, r, in, (1ll << 53) - 1, (1ll << 52) - 1, TW_FP); }, DOM { return fp_in(a, TWO53 - 1) && fp_in(b, TWO52 - 1) && tw_ok(P, TW_FP, w, wq); },
                  CHK {
                      PRE i128 x, y;
                      fp_int(a, x);
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w), yw = mulmod(imod(y, q), wi, q);
                      const i128 u = h_fp_red(P, x), v = h_fp_mulmod(P, y, wi), e0 = u + v, e1 = u - v;
                      REQ(iabs(u) <= (i128)(q / 2 + 1) && 2 * iabs(v) < 3 * (i128)q, "the reduced x or the product leaves its bound");
                      REQ(iabs(e0) < TWO52 && iabs(e1) < TWO52, "an output leaves the next stage's domain");
                      FP_OUT(o0, e0, (imod(x, q) + yw) % q, 2 * (i128)q + 1, (i128)q);
                      FP_OUT(o1, e1, (imod(x, q) + q - yw) % q, 2 * (i128)q + 1, (i128)q);
                      return R;
                  } });
    t.push_back({ "ct_bfly_fp1<true>", "modarith.hip.h:264", FP, p_fp, "integer |x|, |y| < 2^53; integer w < q", "x + y w, x - y w (mod q), |.| < 1.38 q, exact", 0,
                  launch<OpCtFp1Red>, GEN { fill_fp(P, r, in, (1ll << 53) - 1, (1ll << 53) - 1, TW_FP1); },
                  DOM { return fp_in(a, TWO53 - 1) && fp_in(b, TWO53 - 1) && tw_ok(P, TW_FP1, w, wq); },
                  CHK {
                      PRE i128 x, y;
                      fp_int(a, x);
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w), yw = mulmod(imod(y, q), wi, q);
                      const i128 u = h_fp_red(P, x), v = h_fp_mulmod_q(P, h_fp_red(P, y), wi);
                      REQ(100 * iabs(v) < 88 * (i128)q, "the product is not below 0.88 q");
                      FP_OUT(o0, u + v, (imod(x, q) + yw) % q, 138, 100);
                      FP_OUT(o1, u - v, (imod(x, q) + q - yw) % q, 138, 100);
                      return R;
                  } });
    t.push_back({ "ct_bfly_fp1<false> after a <true> stage", "modarith.hip.h:264", FP, p_fp, "integer |x|, |y| < 1.38 q; integer w < q",
                  "x + y w, x - y w (mod q), |.| < 2.92 q, the product below 1.54 q; exact", 0, launch<OpCtFp1>,
                  GEN { fill_fp(P, r, in, (int64_t)((138 * (u128)P.q - 1) / 100), (int64_t)((138 * (u128)P.q - 1) / 100), TW_FP1); },
                  DOM { DPRE const i128 m = (i128)((138 * (u128)q - 1) / 100); return fp_in(a, m) && fp_in(b, m) && tw_ok(P, TW_FP1, w, wq); },
                  CHK {
                      PRE i128 x, y;
                      fp_int(a, x);
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w), yw = mulmod(imod(y, q), wi, q);
                      const i128 v = h_fp_mulmod_q(P, y, wi);
                      REQ(100 * iabs(v) < 154 * (i128)q, "the product is not below 1.54 q");
                      FP_OUT(o0, x + v, (imod(x, q) + yw) % q, 292, 100);
                      FP_OUT(o1, x - v, (imod(x, q) + q - yw) % q, 292, 100);
                      return R;
                  } });
    for (int s = 0; s < 16; ++s)
    {
        t.push_back({ fmt("ct_bfly_fp1<false>, stage %d of 16 from q/2", s), "modarith.hip.h:264", FPN, p_fpn, fmt("integer |x|, |y| <= q/2 + 1 + %d * 2 q; integer w < q", s),
                      fmt("x + y w, x - y w (mod q), |.| <= q/2 + 1 + %d * 2 q and below 33 q, exact", s + 1), s, launch<OpCtFp1>,
                      GEN { fill_fp(P, r, in, chain_bound(P.q, aux, 4), chain_bound(P.q, aux, 4), TW_FP1); },
                      DOM { DPRE return fp_in(a, chain_bound(q, aux, 4)) && fp_in(b, chain_bound(q, aux, 4)) && tw_ok(P, TW_FP1, w, wq); },
                      CHK {
                          PRE i128 x, y;
                          fp_int(a, x);
                          fp_int(b, y);
                          const u64 wi = (u64)bitsd(w), yw = mulmod(imod(y, q), wi, q);
                          const i128 v = h_fp_mulmod_q(P, y, wi), e0 = x + v, e1 = x - v, lim = (i128)chain_bound(q, aux + 1, 4) + 1;
                          REQ(iabs(e0) < lim && iabs(e1) < lim, "an output exceeds the stage's bound");
                          FP_OUT(o0, e0, (imod(x, q) + yw) % q, 33, 1);
                          FP_OUT(o1, e1, (imod(x, q) + q - yw) % q, 33, 1);
                          return R;
                      } });
    }
    t.push_back({ "ct_bfly_fp1_sel, red = true", "modarith.hip.h:277", FP, p_fp, "integer |x|, |y| < 2^53; integer w < q", "as ct_bfly_fp1<true>: |.| < 1.38 q, exact", 1,
                  launch<OpCtFp1Sel>, GEN { fill_fp(P, r, in, (1ll << 53) - 1, (1ll << 53) - 1, TW_FP1); },
                  DOM { return fp_in(a, TWO53 - 1) && fp_in(b, TWO53 - 1) && tw_ok(P, TW_FP1, w, wq); },
                  CHK {
                      PRE i128 x, y;
                      fp_int(a, x);
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w), yw = mulmod(imod(y, q), wi, q);
                      const i128 u = h_fp_red(P, x), v = h_fp_mulmod_q(P, h_fp_red(P, y), wi);
                      FP_OUT(o0, u + v, (imod(x, q) + yw) % q, 138, 100);
                      FP_OUT(o1, u - v, (imod(x, q) + q - yw) % q, 138, 100);
                      return R;
                  } });
    t.push_back({ "ct_bfly_fp1_sel, red = false", "modarith.hip.h:277", FP, p_fp, "integer |x|, |y| < 1.38 q; integer w < q",
                  "as ct_bfly_fp1<false> after a <true> stage: |.| < 2.92 q, exact", 0, launch<OpCtFp1Sel>,
                  GEN { fill_fp(P, r, in, (int64_t)((138 * (u128)P.q - 1) / 100), (int64_t)((138 * (u128)P.q - 1) / 100), TW_FP1); },
                  DOM { DPRE const i128 m = (i128)((138 * (u128)q - 1) / 100); return fp_in(a, m) && fp_in(b, m) && tw_ok(P, TW_FP1, w, wq); },
                  CHK {
                      PRE i128 x, y;
                      fp_int(a, x);
                      fp_int(b, y);
                      const u64 wi = (u64)bitsd(w), yw = mulmod(imod(y, q), wi, q);
                      const i128 v = h_fp_mulmod_q(P, y, wi);
                      FP_OUT(o0, x + v, (imod(x, q) + yw) % q, 292, 100);
                      FP_OUT(o1, x - v, (imod(x, q) + q - yw) % q, 292, 100);
                      return R;
                  } });
    for (int redsum = 0; redsum < 2; ++redsum)
    {
        t.push_back({ fmt("gs_bfly_fp<true> (through gs_bfly_t<M_FPR>), redsum = %d", redsum), "modarith.hip.h:562", FP, p_fp,
                      "integer |x|, |y| < 2^52 (what the load hands over); {w, RN(w/q)}", "x + y, |.| <= q/2 + 1; (x - y) w, |.| < 0.75 q (mod q); exact", redsum << 8,
                      launch<OpGsFpR>, GEN { fill_fp(P, r, in, (1ll << 52) - 1, (1ll << 52) - 1, TW_FP); },
                      DOM { return fp_in(a, TWO52 - 1) && fp_in(b, TWO52 - 1) && tw_ok(P, TW_FP, w, wq); },
                      CHK {
                          PRE i128 x, y;
                          fp_int(a, x);
                          fp_int(b, y);
                          const u64 wi = (u64)bitsd(w);
                          const i128 s = h_fp_red(P, x + y), d = h_fp_red(P, x - y), e1 = h_fp_mulmod(P, d, wi);
                          FP_OUT_HALF(o0, s, imod(x + y, q));
                          FP_OUT(o1, e1, mulmod(imod(x - y, q), wi, q), 3, 4);
                          return R;
                      } });
    }
    // FPN's inverse schedule: input bounds q/2 (the load), q, 1.5 q, 3 q, 6 q, 12 q, with and without the fold of the sum
    for (int hb : { 1, 2, 3, 6, 12, 24 })
    {
        for (int redsum = 0; redsum < 2; ++redsum)
        {
            t.push_back({ fmt("gs_bfly_fp<false> (through gs_bfly_t<M_FPN>), inputs to %s q, redsum = %d", hb == 1 ? "0.5" : fmt("%g", hb / 2.0).c_str(), redsum),
                          "modarith.hip.h:562", FPN, p_fpn,
                          fmt("integer |x|, |y| <= %s (the difference at most %d q <= 24 q); {w, RN(w/q)}", hb == 1 ? "q/2 + 1" : fmt("%g q", hb / 2.0).c_str(), hb),
                          fmt("x + y, %s; (x - y) w, |.| < 1.5 q (mod q); exact", redsum ? "folded to |.| <= q/2 + 1" : "unreduced"), hb | (redsum << 8), launch<OpGsFpN>,
                          GEN { fill_fp(P, r, in, gs_fp_bound(P.q, aux & 255), gs_fp_bound(P.q, aux & 255), TW_FP); },
                          DOM { DPRE const i128 m = gs_fp_bound(q, aux & 255); return 2 * m <= 24 * (i128)q + 2 && fp_in(a, m) && fp_in(b, m) && tw_ok(P, TW_FP, w, wq); },
                          CHK {
                              PRE i128 x, y;
                              fp_int(a, x);
                              fp_int(b, y);
                              const u64 wi = (u64)bitsd(w);
                              const i128 e1 = h_fp_mulmod(P, x - y, wi);
                              if (aux >> 8)
                              {
                                  const i128 s = h_fp_red(P, x + y);
                                  FP_OUT_HALF(o0, s, imod(x + y, q));
                              }
                              else
                              {
                                  FP_OUT(o0, x + y, imod(x + y, q), 24 * (i128)q + 3, (i128)q);
                              }
                              FP_OUT(o1, e1, mulmod(imod(x - y, q), wi, q), 3, 2);
                              return R;
                          } });
        }
    }
    t.push_back({ "gs_bfly_last_fp<false> (through gs_bfly_last_t<M_FPN>)", "modarith.hip.h:581", FPN, p_fpn, "integer |x|, |y| <= 12 q (sum and difference at most 24 q)",
                  "(x + y) N^-1, (x - y) N^-1 w_1 (mod q), |.| < 2 q (fp_to_canonical takes |.| < 2^53); exact", 0, launch<OpGsLastFpN>,
                  GEN { fill_fp(P, r, in, (int64_t)(12 * P.q), (int64_t)(12 * P.q), TW_FP1); }, DOM { DPRE return fp_in(a, (i128)12 * q) && fp_in(b, (i128)12 * q); },
                  CHK {
                      PRE i128 x, y;
                      fp_int(a, x);
                      fp_int(b, y);
                      const u64 n0 = P.ka.pc.ninv.w, n1 = P.ka.pc.ninv_w1.w;
                      FP_OUT(o0, h_fp_mulmod_q(P, x + y, n0), mulmod(imod(x + y, q), n0, q), 2, 1);
                      FP_OUT(o1, h_fp_mulmod_q(P, x - y, n1), mulmod(imod(x - y, q), n1, q), 2, 1);
                      return R;
                  } });
    t.push_back({ "gs_bfly_last_fp<true> (through gs_bfly_last_t<M_FPR>)", "modarith.hip.h:581", FP, p_fp, "integer |x|, |y| < 2^52",
                  "(x + y) N^-1, (x - y) N^-1 w_1 (mod q), |.| < 0.9 q; exact", 0, launch<OpGsLastFpR>,
                  GEN { fill_fp(P, r, in, (1ll << 52) - 1, (1ll << 52) - 1, TW_FP1); }, DOM { return fp_in(a, TWO52 - 1) && fp_in(b, TWO52 - 1); },
                  CHK {
                      PRE i128 x, y;
                      fp_int(a, x);
                      fp_int(b, y);
                      const u64 n0 = P.ka.pc.ninv.w, n1 = P.ka.pc.ninv_w1.w;
                      FP_OUT(o0, h_fp_mulmod_q(P, h_fp_red(P, x + y), n0), mulmod(imod(x + y, q), n0, q), 9, 10);
                      FP_OUT(o1, h_fp_mulmod_q(P, h_fp_red(P, x - y), n1), mulmod(imod(x - y, q), n1, q), 9, 10);
                      return R;
                  } });
    t.push_back({ "LoadFp", "ntt_kernels.hip.h:145", FP, p_fp, "integer v below 2^53", "= v (mod q), |.| <= q/2 + 1, exact", 0, launch<OpLoadFp>,
                  GEN {
                      std::vector<u64> X = sp_below(P.q, (int)std::min<u64>(64, ((1ull << 53) - 1) / P.q));
                      for (u64 x : { (1ull << 53) - 1, (1ull << 53) - 2, 1ull << 52, (1ull << 52) + 1, (1ull << 52) - 1, 0xffffffffull, 1ull << 32 })
                      {
                          add_unique(X, x);
                      }
                      for (u64 k : std::initializer_list<u64>{ 0, 1, ((1ull << 53) - 1) / P.q - 1 })
                      {
                          add_unique(X, k * P.q + (P.q - 1) / 2);
                          add_unique(X, k * P.q + (P.q + 1) / 2);
                      }
                      fill(P, r, in, TW_RES, X, { 0 }, [&] { return r.below((u128)1 << 53); }, [&] { return 0; });
                  },
                  DOM { return a < (1ull << 53); }, CHK { PRE const i128 e = h_fp_red(P, (i128)a); FP_OUT_HALF(o0, e, a % q); return R; } });
    t.push_back({ "LoadFp52", "ntt_kernels.hip.h:155", FP, p_fp, "integer v below 2^52", "= v (mod q), |.| <= q/2 + 1, exact", 0, launch<OpLoadFp52>,
                  GEN {
                      std::vector<u64> X = sp_below(P.q, (int)std::min<u64>(64, ((1ull << 52) - 1) / P.q));
                      for (u64 x : { (1ull << 52) - 1, (1ull << 52) - 2, 1ull << 51, (1ull << 51) + 1, 0xffffffffull, 1ull << 32 })
                      {
                          add_unique(X, x);
                      }
                      for (u64 k : std::initializer_list<u64>{ 0, 1, ((1ull << 52) - 1) / P.q - 1 })
                      {
                          add_unique(X, k * P.q + (P.q - 1) / 2);
                          add_unique(X, k * P.q + (P.q + 1) / 2);
                      }
                      fill(P, r, in, TW_RES, X, { 0 }, [&] { return r.below((u128)1 << 52); }, [&] { return 0; });
                  },
                  DOM { return a < (1ull << 52); }, CHK { PRE const i128 e = h_fp_red(P, (i128)a); FP_OUT_HALF(o0, e, a % q); return R; } });
    t.push_back({ "LoadBarrettFp", "ntt_kernels.hip.h:165", FP, p_fp, "any 64-bit v", "= v (mod q), |.| <= q/2 + 1, exact", 0, launch<OpLoadBarrettFp>,
                  GEN {
                      std::vector<u64> X = sp_any(P.q, r);
                      for (u64 k : { (u64)0, (u64)1, ~(u64)0 / P.q - 1 })
                      {
                          add_unique(X, k * P.q + (P.q - 1) / 2);
                          add_unique(X, k * P.q + (P.q + 1) / 2);
                      }
                      fill(P, r, in, TW_RES, X, { 0 }, [&] { return r.next(); }, [&] { return 0; });
                  },
                  DOM { return true; }, CHK { PRE const i128 e = h_fp_red(P, (i128)(a % q)); FP_OUT_HALF(o0, e, a % q); return R; } });
    return t;
}

std::string prime_names(const Case &c, const std::vector<Prime> &primes)
{
    std::string s;
    for (const Prime &P : primes)
    {
        if (c.applies(P))
        {
            s += (s.empty() ? "" : " ") + P.name + "@" + std::to_string(P.logn);
        }
    }
    return s;
}

} // namespace

int main(int argc, char **argv)
{
    bool host_only = false;
    std::vector<Prime> primes;
    int logn = 0;
    for (int i = 1; i < argc; ++i)
    {
        const std::string arg = argv[i];
        const size_t eq = arg.find('=');
        if (arg == "--host-only")
        {
            host_only = true;
        }
        else if (eq == std::string::npos)
        {
            logn = std::atoi(arg.c_str());
            if (logn < 12 || logn > 16)
            {
                die("logn = %s: 12 .. 16", arg.c_str());
            }
        }
        else
        {
            if (!logn)
            {
                die("a logn comes before the first name=prime");
            }
            primes.push_back(make_prime(arg.substr(0, eq), logn, std::strtoull(arg.c_str() + eq + 1, nullptr, 10)));
        }
    }
    if (primes.empty())
    {
        die("usage: test_modarith_device [--host-only] LOGN name=prime ... [LOGN name=prime ...]");
    }
    const std::vector<Case> table = cases();

    u64 *dev[6] = {};
    std::vector<u64> o0(MAX_INPUTS), o1(MAX_INPUTS);
    if (!host_only)
    {
        int count = 0;
        HIPX(hipGetDeviceCount(&count));
        if (count < 1)
        {
            die("HIP error: no device");
        }
        hipDeviceProp_t prop;
        HIPX(hipGetDeviceProperties(&prop, 0));
        std::printf("device: %s\n", prop.gcnArchName);
        for (u64 *&p : dev)
        {
            HIPX(hipMalloc((void **)&p, MAX_INPUTS * sizeof(u64)));
        }
    }

    In in;
    std::vector<Res> res(MAX_INPUTS);
    int failed_cases = 0;
    size_t launches = 0, inputs_total = 0;
    for (size_t ci = 0; ci < table.size(); ++ci)
    {
        const Case &c = table[ci];
        std::printf("case %zu: %s [%s]\n    primes: %s -- %s\n    domain: %s\n    contract: %s\n", ci, c.name.c_str(), c.cite, c.primes, prime_names(c, primes).c_str(),
                    c.domain.c_str(), c.contract.c_str());
        bool any = false, ok = true;
        int printed = 0;
        for (size_t pi = 0; pi < primes.size(); ++pi)
        {
            const Prime &P = primes[pi];
            if (!c.applies(P))
            {
                continue;
            }
            any = true;
            Rng rng{ 0x243f6a8885a308d3ull ^ (ci * 0x100000001b3ull) ^ (pi << 48) };
            in.clear();
            c.gen(P, c.aux, rng, in);
            const uint32_t n = (uint32_t)in.n();
            size_t outside = 0;
            for (uint32_t i = 0; i < n; ++i)
            {
                outside += c.dom(P, c.aux, in.a[i], in.b[i], in.w[i], in.wq[i]) ? 0 : 1;
            }
            if (outside || n == 0 || n > MAX_INPUTS)
            {
                std::printf("    FAIL %s@%d: %zu of %u generated inputs lie outside the domain\n", P.name.c_str(), P.logn, outside, n);
                ok = false;
                continue;
            }
            inputs_total += n;
            if (host_only)
            {
                std::printf("    %-7s logn %2d q %20llu: %u inputs, all in the domain\n", P.name.c_str(), P.logn, (unsigned long long)P.q, n);
                continue;
            }
            KA ka = P.ka;
            ka.aux = c.aux;
            const u64 *src[4] = { in.a.data(), in.b.data(), in.w.data(), in.wq.data() };
            for (int k = 0; k < 4; ++k)
            {
                HIPX(hipMemcpy(dev[k], src[k], n * sizeof(u64), hipMemcpyHostToDevice));
            }
            HIPX(hipMemset(dev[4], 0xff, n * sizeof(u64)));
            HIPX(hipMemset(dev[5], 0xff, n * sizeof(u64)));
            c.run(ka, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], n);
            ++launches;
            HIPX(hipDeviceSynchronize());
            HIPX(hipMemcpy(o0.data(), dev[4], n * sizeof(u64), hipMemcpyDeviceToHost));
            HIPX(hipMemcpy(o1.data(), dev[5], n * sizeof(u64), hipMemcpyDeviceToHost));
            // the host's 128-bit recomputation, spread over a few threads
            constexpr int T = 8;
            std::fill(res.begin(), res.end(), Res());
            std::thread th[T];
            for (int k = 0; k < T; ++k)
            {
                th[k] = std::thread([&, k] {
                    for (uint32_t i = (uint32_t)k; i < n; i += T)
                    {
                        res[i] = c.chk(P, c.aux, in.a[i], in.b[i], in.w[i], in.wq[i], o0[i], o1[i]);
                    }
                });
            }
            for (std::thread &x : th)
            {
                x.join();
            }
            u128 mag = 0;
            size_t bad = 0;
            for (uint32_t i = 0; i < n; ++i)
            {
                mag = res[i].mag > mag ? res[i].mag : mag;
                if (res[i].why)
                {
                    ++bad;
                    if (printed < 20)
                    {
                        ++printed;
                        std::printf("    MISMATCH %s@%d input %u: %s: a = %016llx b = %016llx w = %016llx wq = %016llx -> %016llx %016llx\n", P.name.c_str(), P.logn, i,
                                    res[i].why, (unsigned long long)in.a[i], (unsigned long long)in.b[i], (unsigned long long)in.w[i], (unsigned long long)in.wq[i],
                                    (unsigned long long)o0[i], (unsigned long long)o1[i]);
                    }
                }
            }
            std::printf("    %-7s logn %2d q %20llu: %u inputs, largest output %.6f q%s\n", P.name.c_str(), P.logn, (unsigned long long)P.q, n,
                        (double)mag / (double)P.q, bad ? fmt(", %zu MISMATCHES", bad).c_str() : "");
            ok = ok && !bad;
        }
        if (!any)
        {
            std::printf("    FAIL: no prime on the command line that this case applies to\n");
            ok = false;
        }
        std::printf("    %s: %s\n", ok ? "ok" : "FAILED", c.name.c_str());
        failed_cases += ok ? 0 : 1;
    }
    if (!host_only)
    {
        for (u64 *p : dev)
        {
            HIPX(hipFree(p));
        }
    }
    std::printf("%zu cases, %zu primes, %zu launches, %zu inputs\n", table.size(), primes.size(), launches, inputs_total);
    if (failed_cases)
    {
        std::printf("%d cases FAILED\n", failed_cases);
        return 1;
    }
    std::printf(host_only ? "HOST ONLY: ALL INPUTS IN THEIR DOMAINS\n" : "ALL PASS\n");
    return 0;
}
