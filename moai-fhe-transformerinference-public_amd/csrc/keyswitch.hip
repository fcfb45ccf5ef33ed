// keyswitch.hip -- rescale, key switching (relinearize / apply_galois) and modraise.
//
// Reference: RNSTool::divide_and_round_q_last_ntt_inplace (SEAL/util/rns.cpp:830-901),
// Evaluator::switch_key_inplace (SEAL/evaluator.cpp:2724-3020), relinearize_internal (:1345-1400),
// apply_galois_inplace (:2563-2665), Bootstrapper::modraise_inplace
// (include/source/bootstrapping/Bootstrapper.cpp:2938-2992).
//
// Structure on the device (all batched over the leading ciphertext index):
//   rescale:     last = INTT(c_last) -> u_i = [last + q_last/2]_{q_last} mod q_i + fix_i -> NTT_{q_i}(u_i)
//                -> out_i = (c_i - u_i) * q_last^-1
//   switch_key:  t = INTT(target); for each output modulus I in {q_0..q_{L-1}, p}:
//                    ops_J = NTT_{q_I}(t_J mod q_I) for every digit J (for I == J this reproduces
//                    target_J exactly, so no special case is needed),
//                    acc_{K,I} = sum_J ops_J (*) key[J][K][I]   (128-bit accumulate, one Barrett);
//                then the same "divide by the last modulus and round" step with p as the last
//                modulus, accumulated into the ciphertext.
// The loop over I is outermost so that the 2*L key rows of modulus I are read once per batch.
#include <mutex>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hostmath.h"
#include "launch.h"
#include <vector>

#include "keyswitch_kernels.hip.h"

namespace moai {

// out row y (group = y / rows_per_group, w = y % rows_per_group) = in row group * in_stride + in_off + w;
// with zero_from >= 0, rows whose w >= zero_from are written as zero instead
__global__ __launch_bounds__(256) void copy_rows_kernel(const uint64_t *in, uint64_t *out, uint32_t rows_per_group,
                                                        uint32_t in_stride, uint32_t in_off, uint32_t zero_from,
                                                        uint32_t n2)
{
    const uint32_t grp = blockIdx.y / rows_per_group;
    const uint32_t w = blockIdx.y % rows_per_group;
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(in) + ((size_t)grp * in_stride + in_off + w) * n2;
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(out) + (size_t)blockIdx.y * n2;
    const bool zero = w >= zero_from;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n2; j += gridDim.x * 256u)
    {
        ulonglong2 v;
        v.x = 0;
        v.y = 0;
        d[j] = zero ? v : s[j];
    }
}

static const uint32_t NO_ZERO = 0xffffffffu;

// out row y = sum over `splits` partial copies of in row (y * in_stride + in_off), mod the one prime
__global__ __launch_bounds__(256) void sum_rows_kernel(const uint64_t *in, uint64_t *out, uint32_t in_stride, uint32_t in_off,
                                                       uint32_t splits, size_t split_stride, const PrimeConst *pc,
                                                       uint32_t prime, uint32_t n2)
{
    const uint64_t q = pc[prime].q;
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(in) + ((size_t)blockIdx.y * in_stride + in_off) * n2;
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(out) + (size_t)blockIdx.y * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n2; j += gridDim.x * 256u)
    {
        ulonglong2 v = s[j];
        for (uint32_t sp = 1; sp < splits; ++sp)
        {
            ulonglong2 y = s[j + sp * (split_stride >> 1)];
            v.x = csub(v.x + y.x, q);
            v.y = csub(v.y + y.y, q);
        }
        d[j] = v;
    }
}

struct ExpandLastArgs
{
    const uint64_t *last;  // [P][N], canonical under prime_last
    uint64_t *u;           // [P][Lout][N]
    const PrimeConst *pc;
    uint32_t prime_last;
    uint32_t Lout;
    uint32_t n2;
};

// u[p][i] = ([last + q_last/2] mod q_last) mod q_i + (q_i - (q_last/2 mod q_i))     in [0, 2 q_i)
// (rns.cpp:858-878 / evaluator.cpp:2964-2992)
__global__ __launch_bounds__(256) void expand_last_kernel(ExpandLastArgs g)
{
    const uint32_t p = blockIdx.y / g.Lout;
    const uint32_t i = blockIdx.y % g.Lout;
    const uint64_t ql = g.pc[g.prime_last].q;
    const uint64_t half = ql >> 1;
    const PrimeConst *pc = g.pc + i;
    const uint64_t q = pc->q, cr1 = pc->cr1;
    const uint64_t fix = q - barrett64(half, q, cr1);
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(g.last) + (size_t)p * g.n2;
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(g.u) + (size_t)blockIdx.y * g.n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.n2; j += gridDim.x * 256u)
    {
        ulonglong2 v = s[j];
        ulonglong2 r;
        r.x = barrett64(csub(v.x + half, ql), q, cr1) + fix;
        r.y = barrett64(csub(v.y + half, ql), q, cr1) + fix;
        d[j] = r;
    }
}

struct FinalizeArgs
{
    const uint64_t *acc;   // row (p, i) at acc + (p * acc_stride + i) * N
    const uint64_t *u;     // [P][Lout][N] canonical
    uint64_t *out;         // [P][Lout][N]
    const PrimeConst *pc;
    const Tw *inv_last;    // inv_qlast + prime_last * k : q_last^-1 mod q_i
    uint32_t acc_stride;
    uint32_t Lout;
    uint32_t n2;
    const uint64_t *addend; // see ModDownArgs
    const uint64_t *addend2;
    uint32_t addend_bstride;
    int add_mode;
};

struct FinalizeListArgs : FinalizeArgs
{
    const KsList *lst; // see moddown_contig
};

// (acc_i - u_i) * q_last^-1 mod q_i      (rns.cpp:892-897 / evaluator.cpp:3012-3017)
// LIST: outputs, second addends and (add_mode 1) first addends per ciphertext p / 2, as in moddown_contig
template <bool LIST = false>
__global__ __launch_bounds__(256) void moddown_finalize_kernel(std::conditional_t<LIST, FinalizeListArgs, FinalizeArgs> g)
{
    const uint32_t p = blockIdx.y / g.Lout, i = blockIdx.y % g.Lout;
    const uint64_t q = g.pc[i].q;
    const Tw inv = g.inv_last[i];
    const size_t n2 = g.n2;
    const ulonglong2 *a = reinterpret_cast<const ulonglong2 *>(g.acc) + ((size_t)p * g.acc_stride + i) * n2;
    const ulonglong2 *u = reinterpret_cast<const ulonglong2 *>(g.u) + (size_t)blockIdx.y * n2;
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(g.out) + (size_t)blockIdx.y * n2;
    const size_t row = ((size_t)(p & 1u) * g.Lout + i) * n2; // inside a ciphertext's [2][Lout][N]
    const ulonglong2 *ad = nullptr, *ad2 = nullptr;          // null: nothing to add (uniform over the workgroup)
    if (g.add_mode == 1 || (g.add_mode == 2 && !(p & 1u)))
    {
        ad = reinterpret_cast<const ulonglong2 *>(g.addend) + (size_t)(p >> 1) * g.addend_bstride * n2 + row;
    }
    if constexpr (LIST)
    {
        o = reinterpret_cast<ulonglong2 *>(g.lst->outs[p >> 1]) + row;
        if (g.lst->sums[p >> 1])
        {
            ad2 = reinterpret_cast<const ulonglong2 *>(g.lst->sums[p >> 1]) + row;
        }
        if (g.add_mode == 1)
        {
            ad = reinterpret_cast<const ulonglong2 *>(g.lst->ins[p >> 1]) + row;
        }
    }
    else if (g.addend2)
    {
        ad2 = reinterpret_cast<const ulonglong2 *>(g.addend2) + (size_t)blockIdx.y * n2;
    }
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.n2; j += gridDim.x * 256u)
    {
        const ulonglong2 x = a[j], y = u[j];
        ulonglong2 r;
        r.x = csub(mul_shoup_lazy(x.x + q - y.x, inv.w, inv.wq, q), q);
        r.y = csub(mul_shoup_lazy(x.y + q - y.y, inv.w, inv.wq, q), q);
        if (ad)
        {
            r = add2(r, ad[j], q);
        }
        if (ad2)
        {
            r = add2(r, ad2[j], q);
        }
        o[j] = r;
    }
}

// ops[b][J] = t[b][J] mod q_I   (evaluator.cpp:2844-2854); all rows under one prime
__global__ __launch_bounds__(256) void reduce_rows_kernel(const uint64_t *t, uint64_t *ops, const PrimeConst *pc,
                                                          uint32_t prime, uint32_t n2)
{
    const uint64_t q = pc[prime].q, cr1 = pc[prime].cr1;
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(t) + (size_t)blockIdx.y * n2;
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(ops) + (size_t)blockIdx.y * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n2; j += gridDim.x * 256u)
    {
        ulonglong2 v = s[j];
        v.x = barrett64(v.x, q, cr1);
        v.y = barrett64(v.y, q, cr1);
        d[j] = v;
    }
}

struct MacArgs
{
    const uint64_t *ops;   // [B][L][N] NTT form under prime I
    const uint64_t *key;   // [k-1][2][k][N]
    uint64_t *acc;         // [B][2][L+1][N]
    const PrimeConst *pc;
    uint32_t L;
    uint32_t k;            // rows per key polynomial in the key's layout
    uint32_t krow;         // the key row of prime I in that layout (the special prime's is the last)
    uint32_t prime;        // I (context prime index)
    uint32_t slot;         // row of acc to write (I, or L for the special prime)
    uint32_t n2;
};

struct MacListArgs : MacArgs
{
    const KsList *lst; // ciphertext b's key is lst->keys[b] with lst->key_rows[b] rows (key, k and krow unused)
};

// acc[b][K][slot] = sum_J ops[b][J] (*) key[J][K][prime]  mod q      (evaluator.cpp:2858-2910)
// blockIdx.y = b
template <bool LIST = false>
__global__ __launch_bounds__(256) void keyswitch_mac_kernel(std::conditional_t<LIST, MacListArgs, MacArgs> g)
{
    const PrimeConst *pc = g.pc + g.prime;
    const uint64_t q = pc->q, cr0 = pc->cr0, cr1 = pc->cr1;
    const uint32_t b = blockIdx.y;
    const size_t n2 = g.n2;
    const ulonglong2 *ops = reinterpret_cast<const ulonglong2 *>(g.ops) + (size_t)b * g.L * n2;
    const ulonglong2 *key = reinterpret_cast<const ulonglong2 *>(g.key);
    uint32_t list_k = 0;
    if constexpr (LIST)
    {
        key = reinterpret_cast<const ulonglong2 *>(g.lst->keys[b]);
        list_k = g.lst->key_rows[b];
    }
    const uint32_t key_k = LIST ? list_k : g.k;
    const uint32_t krow = LIST ? (g.slot == g.L ? list_k - 1 : g.prime) : g.krow;
    ulonglong2 *acc0 = reinterpret_cast<ulonglong2 *>(g.acc) + ((size_t)(b * 2 + 0) * (g.L + 1) + g.slot) * n2;
    ulonglong2 *acc1 = reinterpret_cast<ulonglong2 *>(g.acc) + ((size_t)(b * 2 + 1) * (g.L + 1) + g.slot) * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.n2; j += gridDim.x * 256u)
    {
        uint64_t l0x = 0, h0x = 0, l0y = 0, h0y = 0, l1x = 0, h1x = 0, l1y = 0, h1y = 0;
        for (uint32_t J = 0; J < g.L; ++J)
        {
            ulonglong2 o = ops[(size_t)J * n2 + j];
            ulonglong2 k0 = key[((size_t)(J * 2 + 0) * key_k + krow) * n2 + j];
            ulonglong2 k1 = key[((size_t)(J * 2 + 1) * key_k + krow) * n2 + j];
            mac128(l0x, h0x, o.x, k0.x);
            mac128(l0y, h0y, o.y, k0.y);
            mac128(l1x, h1x, o.x, k1.x);
            mac128(l1y, h1y, o.y, k1.y);
        }
        ulonglong2 r0, r1;
        r0.x = barrett128(l0x, h0x, q, cr0, cr1);
        r0.y = barrett128(l0y, h0y, q, cr0, cr1);
        r1.x = barrett128(l1x, h1x, q, cr0, cr1);
        r1.y = barrett128(l1y, h1y, q, cr0, cr1);
        acc0[j] = r0;
        acc1[j] = r1;
    }
}

struct RaiseArgs
{
    const uint64_t *src;  // [P][N] coefficient form, canonical mod q0
    uint64_t *out;        // [P][Lout][N]
    const PrimeConst *pc;
    uint32_t Lout;
    uint32_t n2;
};

// Bootstrapper.cpp:2964-2988: dest = src mod q_j, plus (q_j - q0 mod q_j) when src > q0/2
__global__ __launch_bounds__(256) void modraise_kernel(RaiseArgs g)
{
    const uint32_t p = blockIdx.y / g.Lout;
    const uint32_t jrow = blockIdx.y % g.Lout;
    const uint64_t q0 = g.pc[0].q;
    const uint64_t q = g.pc[jrow].q, cr1 = g.pc[jrow].cr1;
    const uint64_t minus_q0 = jrow == 0 ? 0 : q - barrett64(q0, q, cr1);
    const uint64_t half = q0 >> 1;
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(g.src) + (size_t)p * g.n2;
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(g.out) + (size_t)blockIdx.y * g.n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < g.n2; j += gridDim.x * 256u)
    {
        ulonglong2 v = s[j], r;
        r.x = barrett64(v.x, q, cr1);
        r.y = barrett64(v.y, q, cr1);
        if (v.x > half)
        {
            r.x = csub(r.x + minus_q0, q);
        }
        if (v.y > half)
        {
            r.y = csub(r.y + minus_q0, q);
        }
        d[j] = r;
    }
}

// f(LOGN, MODE) over the degrees and arithmetic modes that the key-switch and mod-down kernels are compiled for
template <class F>
static int dispatch_ks(int logn, int mode, F &&f)
{
    return dispatch_logn(logn, [&](auto LG) {
        return dispatch<M_GUARD, M_NOGUARD, M_FPN, M_FPR>("key-switch arithmetic mode ", mode, [&](auto MD) { return f(LG, MD); });
    });
}

// whether mod-down and rescale of `rows` = polynomials * kept primes may use the FP64 arithmetic modes: below
// MOAI_MD_FP_MIN_ROWS rows the extra launches cost more than the FP64 butterflies save (a single
// ciphertext at MOAI's top level: 162 vs 147 ms per bootstrap; packs of 16: 66.0 vs 67.1 ms)
static bool md_allow_fp(size_t rows)
{
    return (long)rows >= tuning(K_MD_FP_MIN_ROWS);
}

// Shared tail of rescale and key switch: divide rows [0, Lout) of `acc` by the modulus `prime_last`
// whose NTT-form row is `last_rows` ([P][N], overwritten), rounding to nearest.
//   acc row (p, i) = acc + (p * acc_stride + i) * N ; out [P][Lout][N]
// scratch: u [P][Lout][N]
//   add: what is added to the quotient (KsAddend); nothing for a plain rescale
//   lst (device memory, key switch only): polynomials 2b and 2b + 1 go to lst->outs[b] plus lst->sums[b], and add.mode 1 reads
//   lst->ins[b]; out and add.second are null then (the LIST kernels)
static int moddown(moai_ctx *c, uint64_t *last_rows, const uint64_t *acc, uint32_t acc_stride, uint64_t *u, uint64_t *out, size_t P,
                   size_t Lout, uint32_t prime_last, const KsAddend &add, hipStream_t s, uint32_t acc_splits = 1,
                   size_t acc_split_stride = 0, const Tw *scal = nullptr, const KsList *lst = nullptr)
{
    const Tw *inv_last = c->inv_qlast + (size_t)prime_last * c->k;
    RowMap rm;
    uint32_t pl = prime_last;
    MOAI_TRY(make_rowmap(c, 1, &pl, &rm));
    MOAI_TRY(ntt_launch(c, last_rows, P, 1, rm, true, s));
    if (c->logn >= 12)
    {
        // fused: the expand rides on the strided pass's loads, the division on the contiguous pass's stores
        ModDownArgs a;
        a.last = last_rows;
        a.u = u;
        a.acc = acc;
        a.out = out;
        a.pc = c->pc;
        a.inv_last = inv_last;
        a.prime_last = prime_last;
        a.acc_stride = acc_stride;
        a.Lout = (uint32_t)Lout;
        a.P = (uint32_t)P;
        a.addend = add.ptr;
        a.addend2 = add.second;
        a.addend_bstride = (uint32_t)add.bstride;
        a.add_mode = add.mode;
        a.has_scal = scal ? 1 : 0;
        if (scal)
        {
            for (size_t i = 0; i < Lout; ++i)
            {
                a.scal[i] = scal[i];
            }
        }
        a.acc_splits = acc_splits;
        a.acc_split_stride = acc_split_stride;
        // one pair of launches per arithmetic mode present among the output moduli (ntt_mode, md_allow_fp)
        const bool allow_fp = md_allow_fp(P * Lout);
        for (int mode = M_GUARD; mode <= M_FPR; ++mode)
        {
            a.Lsel = 0;
            for (size_t i = 0; i < Lout; ++i)
            {
                if (ntt_mode(c, (uint32_t)i, allow_fp) == mode)
                {
                    a.sel.idx[a.Lsel++] = (uint32_t)i;
                }
            }
            if (!a.Lsel)
            {
                continue;
            }
            a.total_work = (uint32_t)(P * a.Lsel * (c->n >> 12));
            const TwPair t = twiddles(c, mode, false);
            a.tw = t.tw;
            a.twb = t.twb;
            MOAI_TRY(dispatch_ks(c->logn, mode, [&](auto LG, auto MD) {
                hipLaunchKernelGGL((moddown_strided<decltype(LG)::value, decltype(MD)::value>), dim3(a.total_work), dim3(256), 0, s, a);
                return plain_or_list<ModDownListArgs>(a, lst, [&](const auto &args, auto LIST) {
                    hipLaunchKernelGGL((moddown_contig<decltype(LG)::value, decltype(MD)::value, decltype(LIST)::value>), dim3(a.total_work),
                                       dim3(256), 0, s, args);
                    return MOAI_OK;
                });
            }));
        }
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    }
    if (scal)
    {
        return set_error(MOAI_ELOGIC, "fused scalar product needs the tiled transform");
    }
    ExpandLastArgs e;
    e.last = last_rows;
    e.u = u;
    e.pc = c->pc;
    e.prime_last = prime_last;
    e.Lout = (uint32_t)Lout;
    e.n2 = (uint32_t)(c->n >> 1);
    MOAI_TRY(launch_rows(expand_last_kernel, c, P * Lout, s, e));
    MOAI_TRY(make_rowmap(c, Lout, nullptr, &rm));
    MOAI_TRY(ntt_launch(c, u, P, Lout, rm, false, s));
    return moddown_finalize(c, acc, acc_stride, u, out, P, Lout, inv_last, add, lst, s);
}

// the last kernel of the unfused mod-down (launch.h): the tail above and the hybrid key switch's base conversion (hybrid.hip)
int moddown_finalize(moai_ctx *c, const uint64_t *acc, uint32_t acc_stride, const uint64_t *u, uint64_t *out, size_t P, size_t Lout,
                     const Tw *inv, const KsAddend &add, const KsList *lst, hipStream_t s)
{
    FinalizeArgs f;
    f.acc = acc;
    f.u = u;
    f.out = out;
    f.pc = c->pc;
    f.inv_last = inv;
    f.acc_stride = acc_stride;
    f.Lout = (uint32_t)Lout;
    f.n2 = (uint32_t)(c->n >> 1);
    f.addend = add.ptr;
    f.addend2 = add.second;
    f.addend_bstride = (uint32_t)add.bstride;
    f.add_mode = add.mode;
    return plain_or_list<FinalizeListArgs>(f, lst, [&](const auto &args, auto LIST) {
        return launch_rows(moddown_finalize_kernel<decltype(LIST)::value>, c, P * Lout, s, args);
    });
}

static int check_level(const moai_ctx *c, size_t L, size_t polys)
{
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (L == 0 || L > c->k)
    {
        return set_error(MOAI_EINVAL, "L = %zu out of range for a context of %zu primes", L, c->k);
    }
    if (polys * (L + 1) > 0x7fffffffull)
    {
        return set_error(MOAI_EINVAL, "batch too large for one launch");
    }
    return enter_device(c);
}

// what a key switch at L data primes needs of the context: a special prime, and L of the other k - 1
static int check_switch_level(const moai_ctx *c, size_t L)
{
    if (c->k < 2)
    {
        return set_error(MOAI_ELOGIC, "keyswitching is not supported by the context");
    }
    if (L > c->k - 1)
    {
        return set_error(MOAI_EINVAL, "L exceeds the key's decomposition size");
    }
    return MOAI_OK;
}

// rows per key polynomial of `key` (k for the reference's layout, levels + 1 for a key moai_key_trim produced), after checking
// that the key holds what a switch at L data primes reads: digits J < L and rows {0 .. L-1, special} (SEAL/evaluator.cpp:2818,2831)
// member >= 0: the key is that member's of a list, and the message says so
static int key_rows_for(moai_ctx *c, const uint64_t *key, size_t L, uint32_t *rows, long member = -1)
{
    std::lock_guard<std::mutex> g(*static_cast<std::mutex *>(c->mutex));
    auto it = c->key_layouts.find(key);
    if (it == c->key_layouts.end())
    {
        *rows = (uint32_t)c->k;
        return MOAI_OK;
    }
    if ((L > it->second.digits || L + 1 > it->second.rows) && member >= 0)
    {
        return set_error(MOAI_ERANGE, "member %ld: the key was trimmed to %u levels and cannot switch a ciphertext of %zu data primes", member,
                         it->second.digits, L);
    }
    if (L > it->second.digits || L + 1 > it->second.rows)
    {
        return set_error(MOAI_ERANGE, "the key was trimmed to %u levels and cannot switch a ciphertext of %zu data primes",
                         it->second.digits, L);
    }
    *rows = it->second.rows;
    return MOAI_OK;
}

// number of output moduli whose digits are in flight at once: bounded by the scratch budget
// (MOAI_KS_TMP_MB, default 8192 MiB) so that small batches expose (L+1) x 16 tiles of parallelism in
// one launch while large batches stay within a few GiB of workspace
static size_t ks_group_size(const moai_ctx *c, size_t L, size_t batch)
{
    long budget_mb = tuning(K_KS_TMP_MB);
    if (budget_mb < 1)
    {
        budget_mb = 1;
    }
    const size_t per_modulus = batch * L * c->n * sizeof(uint64_t);
    size_t g = ((size_t)budget_mb << 20) / (per_modulus ? per_modulus : 1);
    if (g < 1)
    {
        g = 1;
    }
    if (g > L + 1)
    {
        g = L + 1;
    }
    return g;
}

// Few ciphertexts leave the MAC kernel with (L+1)*16*batch long-running workgroups, barely more than the
// chip holds at two per CU, so its second round runs almost empty.  Splitting the digit range S ways gives
// S times more, S times shorter workgroups; the partial sums are added where they are consumed.
static uint32_t ks_splits(const moai_ctx *c, size_t L, size_t batch)
{
    if (c->logn < 12)
    {
        return 1;
    }
    const size_t wgs = batch * (L + 1) * (c->n >> 12);
    const size_t want = (size_t)c->num_cu * 8;
    size_t s = (want + wgs - 1) / wgs;
    if (s > 8)
    {
        s = 8;
    }
    if (s > L)
    {
        s = L;
    }
    if (s < 1)
    {
        s = 1;
    }
    // no empty split: with chunks of ceil(L/s) digits, ceil(L/chunk) splits cover the range exactly
    const size_t chunk = (L + s - 1) / s;
    return (uint32_t)((L + chunk - 1) / chunk);
}

static size_t ks_tmp_rows(const moai_ctx *c, size_t L, size_t batch)
{
    size_t fused = c->logn >= 12 ? batch * ks_group_size(c, L, batch) * L : 0;
    size_t plain = 2 * batch * L; // ops [B][L] (unfused path) and u [2B][L] (mod-down)
    return fused > plain ? fused : plain;
}

// workspace of one key switch, byte offsets: t [B][L][N] | ops, the digits in flight and later u [2B][L][N] |
// acc [splits][B][2][L+1][N] | last [2B][N]
struct KsLayout
{
    uint32_t splits;
    size_t split_stride; // words from one partial accumulator to the next
    size_t t, ops, acc, last, total;
};

static KsLayout ks_layout(const moai_ctx *c, size_t L, size_t batch)
{
    const size_t row_bytes = c->n * sizeof(uint64_t);
    KsLayout w;
    w.splits = ks_splits(c, L, batch);
    w.split_stride = batch * 2 * (L + 1) * c->n;
    w.t = 0;
    w.ops = w.t + align256(batch * L * row_bytes);
    w.acc = w.ops + align256(ks_tmp_rows(c, L, batch) * row_bytes);
    w.last = w.acc + align256(w.splits * w.split_stride * sizeof(uint64_t));
    w.total = w.last + align256(batch * 2 * row_bytes);
    return w;
}

static size_t switch_key_ws_bytes(const moai_ctx *c, size_t L, size_t batch)
{
    return ks_layout(c, L, batch).total;
}

// which arithmetic the fused kernels use for output modulus `prime` (keyswitch_kernels.hip.h): the forward
// transform's mode, with the integer no-guard form only when the lazy digit may also enter the MAC unreduced
static int ks_mode(const moai_ctx *c, uint32_t prime, size_t L, bool allow_fp)
{
    const int m = ntt_mode(c, prime, allow_fp);
    if (m != M_NOGUARD)
    {
        return m;
    }
    // 36 q * q * L < 2^128
    const uint64_t q = c->primes[prime];
    unsigned __int128 lim = (unsigned __int128)q * q;
    return lim < ((~(unsigned __int128)0) / (36 * (unsigned __int128)(L ? L : 1))) ? M_NOGUARD : M_GUARD;
}

// a few ciphertexts at a low level are launch-bound and stay on the integer modes (MOAI_KS_FP_MIN_ROWS, ks_plan)
static bool ks_allow_fp(size_t L, size_t batch)
{
    return (long)(batch * L) >= tuning(K_KS_FP_MIN_ROWS);
}

// The launches of a key switch at L data primes: the output moduli (slot I = L stands for the special prime) ordered by
// arithmetic mode, cut into groups of at most ks_group_size() moduli of one mode.  The unused entries of a KsGroup repeat its
// first member.  Every mode is one more pair of launches: a few ciphertexts at a low level are launch-bound and stay on the
// single integer group (measured: FP64 pays from about 16 digit rows per call, MOAI_KS_FP_MIN_ROWS).
struct KsPlanGroup
{
    KsGroup grp;
    size_t g; // members
    int mode;
};

static std::vector<KsPlanGroup> ks_plan(const moai_ctx *c, size_t L, size_t batch)
{
    const size_t G = ks_group_size(c, L, batch);
    const bool allow_fp = ks_allow_fp(L, batch);
    const auto prime_of = [&](size_t Iidx) { return (uint32_t)(Iidx == L ? c->k - 1 : Iidx); };
    std::vector<uint32_t> order;
    std::vector<int> order_mode;
    for (int mode = M_FPR; mode >= M_GUARD; --mode)
    {
        for (size_t Iidx = 0; Iidx <= L; ++Iidx)
        {
            if (ks_mode(c, prime_of(Iidx), L, allow_fp) == mode)
            {
                order.push_back((uint32_t)Iidx);
                order_mode.push_back(mode);
            }
        }
    }
    std::vector<KsPlanGroup> plan;
    for (size_t o0 = 0; o0 < order.size();)
    {
        KsPlanGroup pg;
        pg.mode = order_mode[o0];
        pg.g = 0;
        while (o0 + pg.g < order.size() && pg.g < G && order_mode[o0 + pg.g] == pg.mode)
        {
            ++pg.g;
        }
        for (size_t i = 0; i < MOAI_MAX_RNS; ++i)
        {
            const size_t Iidx = order[o0 + (i < pg.g ? i : 0)];
            pg.grp.prime[i] = prime_of(Iidx);
            pg.grp.slot[i] = (uint32_t)Iidx;
        }
        plan.push_back(pg);
        o0 += pg.g;
    }
    return plan;
}

template <int LOGN, int MODE>
static int ks_fused_group(moai_ctx *c, const uint64_t *t, uint64_t *tmp, const uint64_t *key, uint64_t *acc, size_t L, size_t batch,
                          const KsGroup &grp, size_t G, uint32_t splits, const KsTarget &tg, hipStream_t s)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    KsP1Args p1;
    p1.t = t;
    p1.tmp = tmp;
    p1.tw = twiddles(c, MODE, false).tw;
    p1.pc = c->pc;
    p1.grp = grp;
    p1.L = (uint32_t)L;
    p1.G = (uint32_t)G;
    p1.total_work = (uint32_t)(batch * G * L * TPR);
    // N = 2^16, FP64 modes, enough work to fill the chip that way: eight tiles per workgroup, software-pipelined
    // (fwd_strided_tiles; MOAI_KS_P1_ITEMS=1: one tile per workgroup)
    constexpr int P1_ITEMS = (LOGN == 16 && MODE >= M_FPN) ? 8 : 1;
    if (P1_ITEMS > 1 && p1.total_work >= 8u * 2048u && tuning(K_KS_P1_ITEMS) > 1)
    {
        hipLaunchKernelGGL((ks_fwd_strided<LOGN, MODE, P1_ITEMS>), dim3(p1.total_work / P1_ITEMS), dim3(256), 0, s, p1);
    }
    else
    {
        hipLaunchKernelGGL((ks_fwd_strided<LOGN, MODE>), dim3(p1.total_work), dim3(256), 0, s, p1);
    }
    MOAI_LAUNCH_CHECK();
    KsP2Args p2;
    p2.tmp = tmp;
    p2.tgt = tg.ptr;
    p2.tgt_stride = (uint32_t)tg.stride_rows;
    p2.tgt_off = (uint32_t)tg.off_rows;
    p2.key = key;
    p2.acc = acc;
    p2.tw = p1.tw;
    p2.tw1 = c->fwd_twf1;
    p2.pc = c->pc;
    p2.grp = grp;
    p2.L = (uint32_t)L;
    p2.G = (uint32_t)G;
    p2.k = tg.key_rows;
    p2.B = (uint32_t)batch;
    p2.S = splits;
    p2.jchunk = (uint32_t)((L + splits - 1) / splits);
    p2.split_stride = batch * 2 * (L + 1) * c->n;
    p2.total_work = (uint32_t)(batch * G * TPR * 2 * splits); // 2048-coefficient tiles
    return plain_or_list<KsP2ListArgs>(p2, tg.lst, [&](const auto &args, auto LIST) {
        hipLaunchKernelGGL((ks_contig_mac8<LOGN, MODE, decltype(LIST)::value>), dim3(p2.total_work), dim3(256), 0, s, args);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    });
}

// wsp: switch_key_ws_bytes() bytes of scratch.
// ct [batch][2][L][N] = add (KsAddend) + key switch of the target rows tg; ct may be the addend itself
// tg.lst (device memory; its keys validated by the caller): ciphertext b is switched with lst->keys[b] and its result goes to
// lst->outs[b] (+ lst->sums[b]); ct, key and add.second are null then, and add.mode 1 adds lst->ins[b] (moddown)
static int switch_key_impl(moai_ctx *c, uint64_t *ct, KsTarget tg, const uint64_t *key, size_t L, size_t batch, void *wsp, hipStream_t s,
                           const KsAddend &add)
{
    const size_t n = c->n;
    const size_t k = c->k;
    MOAI_TRY(check_switch_level(c, L));
    if (!tg.lst)
    {
        MOAI_TRY(key_rows_for(c, key, L, &tg.key_rows));
    }
    const KsLayout w = ks_layout(c, L, batch);
    uint64_t *t = at_bytes(wsp, w.t), *ops = at_bytes(wsp, w.ops), *acc = at_bytes(wsp, w.acc), *last = at_bytes(wsp, w.last);
    const uint32_t n2 = (uint32_t)(n >> 1);

    // 1. t = INTT(target)      (evaluator.cpp:2804-2812)
    RowMap rm;
    MOAI_TRY(make_rowmap(c, L, nullptr, &rm));
    MOAI_TRY(ntt_launch(c, t, batch, L, rm, true, s, tg.ptr, tg.stride_rows, tg.off_rows));
    // 2. inner products per output modulus    (evaluator.cpp:2817-2911)
    if (c->logn >= 12)
    {
        // fused: "mod q_I" rides on the strided pass's loads, the key MAC on the contiguous pass
        if (batch * ks_group_size(c, L, batch) * L * (n >> 11) > 0x7fffffffull)
        {
            return set_error(MOAI_EINVAL, "batch too large for one launch");
        }
        for (const KsPlanGroup &pg : ks_plan(c, L, batch))
        {
            MOAI_TRY(dispatch_ks(c->logn, pg.mode, [&](auto LG, auto MD) {
                return ks_fused_group<decltype(LG)::value, decltype(MD)::value>(c, t, ops, key, acc, L, batch, pg.grp, pg.g, w.splits, tg, s);
            }));
        }
    }
    else
    {
        // small transforms (N <= 2048): separate reduce -> NTT -> MAC launches
        for (size_t Iidx = 0; Iidx <= L; ++Iidx)
        {
            const uint32_t prime = (uint32_t)(Iidx == L ? k - 1 : Iidx);
            MOAI_TRY(launch_rows(reduce_rows_kernel, c, batch * L, s, t, ops, c->pc, prime, n2));
            for (size_t r = 0; r < L; ++r)
            {
                rm.idx[r] = (uint32_t)prime;
            }
            MOAI_TRY(ntt_launch(c, ops, batch, L, rm, false, s));
            MacArgs m;
            m.ops = ops;
            m.key = key;
            m.acc = acc;
            m.pc = c->pc;
            m.L = (uint32_t)L;
            m.k = tg.key_rows;
            m.krow = Iidx == L ? tg.key_rows - 1 : prime;
            m.prime = prime;
            m.slot = (uint32_t)Iidx;
            m.n2 = n2;
            MOAI_TRY(plain_or_list<MacListArgs>(m, tg.lst, [&](const auto &args, auto LIST) {
                return launch_rows(keyswitch_mac_kernel<decltype(LIST)::value>, c, batch, s, args);
            }));
        }
    }
    // 3. mod-down by the special prime, accumulated into ct   (evaluator.cpp:2913-3018)
    MOAI_TRY(launch_rows(sum_rows_kernel, c, batch * 2, s, acc, last, (uint32_t)(L + 1), (uint32_t)L, w.splits, w.split_stride, c->pc,
                         (uint32_t)(k - 1), n2));
    return moddown(c, last, acc, (uint32_t)(L + 1), ops, ct, batch * 2, L, (uint32_t)(k - 1), add, s, w.splits, w.split_stride, nullptr,
                   tg.lst);
}

} // namespace moai

using namespace moai;

// the header's codes are the enum of modarith.hip.h
static_assert(MOAI_MODE_LAZY16 == moai::M_LAZY16 && MOAI_MODE_LAZY8 == moai::M_LAZY8 && MOAI_MODE_GUARD2 == moai::M_GUARD2 &&
                  MOAI_MODE_GUARD == moai::M_GUARD && MOAI_MODE_NOGUARD == moai::M_NOGUARD && MOAI_MODE_FPN == moai::M_FPN &&
                  MOAI_MODE_FPR == moai::M_FPR,
              "include/moai_hip.h and modarith.hip.h disagree");

// read-only: the mode the launchers would pick now (ks_plan, moddown, launch_fwd, launch_inv call the same functions)
extern "C" int moai_arith_mode(const moai_ctx *c, size_t prime, int op, size_t L, size_t rows, int *mode)
{
    if (!c || !mode)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    if (prime >= c->k)
    {
        return set_error(MOAI_ERANGE, "prime index %zu out of range (k = %zu)", prime, c->k);
    }
    const uint32_t p = (uint32_t)prime;
    switch (op)
    {
    case MOAI_MODE_OF_KEY_SWITCH:
        *mode = ks_mode(c, p, L, ks_allow_fp(L, rows));
        return MOAI_OK;
    case MOAI_MODE_OF_MOD_DOWN:
        *mode = ntt_mode(c, p, md_allow_fp(rows));
        return MOAI_OK;
    case MOAI_MODE_OF_NTT_FORWARD:
        *mode = fwd_class(c, p);
        return MOAI_OK;
    case MOAI_MODE_OF_NTT_INVERSE:
        *mode = inv_class(c, p);
        return MOAI_OK;
    default:
        return set_error(MOAI_EINVAL, "unknown operation %d", op);
    }
}

namespace moai {
// rows[r][:] = rows[r][:] * s mod q, canonical   (the dropped row of a fused scalar product + rescale)
__global__ __launch_bounds__(256) void scale_rows_kernel(uint64_t *rows, Tw s, uint64_t q, uint32_t n2)
{
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(rows) + (size_t)blockIdx.y * n2;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n2; j += gridDim.x * 256u)
    {
        ulonglong2 x = d[j];
        x.x = csub(mul_shoup_lazy(x.x, s.w, s.wq, q), q);
        x.y = csub(mul_shoup_lazy(x.y, s.w, s.wq, q), q);
        d[j] = x;
    }
}
} // namespace moai

// rescale_to_next (scalars == nullptr) or a scalar plaintext product followed by it, plus an optional addend of the output's
// shape ([batch * size][L - 1][N]; may be `out` itself) that the last kernel adds to the quotient
// (locked: the caller already holds the context's op_mutex, see rescale_nolock)
static int rescale_common(moai_ctx *c, const uint64_t *in, const uint64_t *scalars, const uint64_t *addend, uint64_t *out, size_t size,
                          size_t L, size_t batch, void *stream, bool locked = false)
{
    const size_t P = batch * size;
    int rc = check_level(c, L, P);
    if (rc)
    {
        return rc;
    }
    if (L < 2)
    {
        // SEAL/evaluator.cpp:1693-1696
        return set_error(MOAI_EINVAL, "end of modulus switching chain reached");
    }
    if (P == 0)
    {
        return MOAI_OK;
    }
    if (!in || !out || in == out || in == addend)
    {
        return set_error(MOAI_EINVAL, "bad in/out pointers");
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = c->n * sizeof(uint64_t);
    if (scalars && c->logn < 12)
    {
        // small transforms take the two separate steps
        void *tmp = nullptr;
        MOAI_TRY(moai_malloc(&tmp, P * L * row_bytes));
        rc = moai_mul_scalar_rows(c, in, scalars, static_cast<uint64_t *>(tmp), P, L, stream);
        if (!rc)
        {
            rc = rescale_common(c, static_cast<const uint64_t *>(tmp), nullptr, addend, out, size, L, batch, stream);
        }
        hipError_t e = hipStreamSynchronize(s);
        moai_free(tmp);
        return rc ? rc : (e == hipSuccess ? MOAI_OK : set_error(MOAI_EHIP, "%s", hipGetErrorString(e)));
    }
    Tw sc[MOAI_MAX_RNS];
    if (scalars)
    {
        for (size_t r = 0; r < L; r++)
        {
            sc[r] = make_tw(scalars[r] % c->primes[r], c->primes[r]); // barrett_reduce_64, polyarithsmallmod.h:209-217
        }
    }
    const size_t sz_last = align256(P * row_bytes);
    const size_t sz_u = align256(P * (L - 1) * row_bytes);
    std::unique_lock<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex), std::defer_lock);
    if (!locked)
    {
        op_lock.lock();
    }
    void *wsp;
    MOAI_TRY(workspace(c, sz_last + sz_u, s, &wsp));
    uint64_t *last = static_cast<uint64_t *>(wsp);
    uint64_t *u = at_bytes(wsp, sz_last);
    MOAI_TRY(launch_rows(copy_rows_kernel, c, P, s, in, last, 1u, (uint32_t)L, (uint32_t)(L - 1), NO_ZERO, (uint32_t)(c->n >> 1)));
    if (scalars)
    {
        MOAI_TRY(launch_rows(scale_rows_kernel, c, P, s, last, sc[L - 1], c->primes[L - 1], (uint32_t)(c->n >> 1)));
    }
    // the addend has the output's layout: polynomial p starts (L - 1) rows after polynomial p - 1 (ModDownArgs: pairs of
    // polynomials 2 (L - 1) rows apart)
    return moddown(c, last, in, (uint32_t)L, u, out, P, L - 1, (uint32_t)(L - 1), { addend, 2 * (L - 1), addend ? 1 : 0 }, s, 1, 0,
                   scalars ? sc : nullptr);
}

namespace moai {
size_t rescale_ws_bytes(const moai_ctx *c, size_t L, size_t polys)
{
    const size_t row_bytes = c->n * sizeof(uint64_t);
    return align256(polys * row_bytes) + align256(polys * (L - 1) * row_bytes);
}

int rescale_nolock(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t size, size_t L, size_t batch, hipStream_t s)
{
    return rescale_common(c, in, nullptr, nullptr, out, size, L, batch, (void *)s, true);
}
} // namespace moai

extern "C" int moai_rescale(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t size, size_t L, size_t batch,
                            void *stream)
{
    MOAI_AUDIT(stream, in, out);
    trace_op("rescale", L, batch * size);
    return rescale_common(c, in, nullptr, nullptr, out, size, L, batch, stream);
}

extern "C" int moai_rescale_add(moai_ctx *c, const uint64_t *in, const uint64_t *addend, uint64_t *out, size_t size, size_t L,
                                size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, addend, out);
    trace_op("rescale_add", L, batch * size);
    if (!addend)
    {
        return set_error(MOAI_EINVAL, "null addend");
    }
    return rescale_common(c, in, nullptr, addend, out, size, L, batch, stream);
}

extern "C" int moai_mul_scalar_rescale(moai_ctx *c, const uint64_t *in, const uint64_t *scalars, uint64_t *out, size_t size,
                                       size_t L, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, scalars, out);
    trace_op("mul_scalar_rescale", L, batch * size);
    if (!scalars)
    {
        return set_error(MOAI_EINVAL, "bad pointers");
    }
    return rescale_common(c, in, scalars, nullptr, out, size, L, batch, stream);
}

extern "C" int moai_mul_scalar_rescale_add(moai_ctx *c, const uint64_t *in, const uint64_t *scalars, const uint64_t *addend,
                                           uint64_t *out, size_t size, size_t L, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, scalars, addend, out);
    trace_op("mul_scalar_rescale_add", L, batch * size);
    if (!scalars || !addend)
    {
        return set_error(MOAI_EINVAL, "bad pointers");
    }
    return rescale_common(c, in, scalars, addend, out, size, L, batch, stream);
}

extern "C" int moai_switch_key(moai_ctx *c, uint64_t *ct, const uint64_t *target, const uint64_t *key, size_t L,
                               size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct, target, key);
    trace_op("switch_key", L, batch);
    MOAI_TRY(check_level(c, L, batch * 2));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (!ct || !target || !key)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    void *wsp;
    MOAI_TRY(workspace(c, switch_key_ws_bytes(c, L, batch), (hipStream_t)stream, &wsp));
    return switch_key_impl(c, ct, { target, L, 0 }, key, L, batch, wsp, (hipStream_t)stream, { ct, 2 * L, 1 });
}

extern "C" int moai_relinearize(moai_ctx *c, const uint64_t *ct3, const uint64_t *relin_key, uint64_t *out, size_t L,
                                size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct3, relin_key, out);
    trace_op("relinearize", L, batch);
    MOAI_TRY(check_level(c, L, batch * 3));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (!ct3 || !relin_key || !out || out == ct3)
    {
        return set_error(MOAI_EINVAL, "bad pointers");
    }
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    void *wsp;
    MOAI_TRY(workspace(c, switch_key_ws_bytes(c, L, batch), s, &wsp));
    // out = (c0, c1) + switch_key(c2, relin_keys[0])      (evaluator.cpp:1383-1392): c0 and c1 are read from ct3 by
    // the last kernel of the key switch, no copy first
    return switch_key_impl(c, out, { ct3, 3 * L, 2 * L }, relin_key, L, batch, wsp, s, { ct3, 3 * L, 1 });
}

// out = (galois(in0), 0) + switch_key(galois(in1)) [+ sum]      (evaluator.cpp:2631-2654): both summands are added by the
// last kernel of the key switch, so `out` is written once and may be `in` (or `sum`)
static int apply_galois_impl(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t L, uint32_t galois_elt, const uint64_t *galois_key,
                             size_t batch, void *stream, const uint64_t *sum)
{
    hipStream_t s = (hipStream_t)stream;
    const size_t sz_tmp = align256(batch * 2 * L * c->n * sizeof(uint64_t));
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    void *wsp;
    MOAI_TRY(workspace(c, sz_tmp + switch_key_ws_bytes(c, L, batch), s, &wsp));
    uint64_t *tmp = static_cast<uint64_t *>(wsp); // galois(in), both polynomials
    MOAI_TRY(moai_galois_permute(c, in, tmp, batch * 2, L, galois_elt, stream));
    return switch_key_impl(c, out, { tmp, 2 * L, L }, galois_key, L, batch, at_bytes(wsp, sz_tmp), s, { tmp, 2 * L, 2, sum });
}

extern "C" int moai_apply_galois_to(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t L, uint32_t galois_elt,
                                    const uint64_t *galois_key, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, out, galois_key);
    trace_op("apply_galois_to", L, batch);
    MOAI_TRY(check_level(c, L, batch * 2));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (!in || !out || !galois_key)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    return apply_galois_impl(c, in, out, L, galois_elt, galois_key, batch, stream, nullptr);
}

extern "C" int moai_apply_galois(moai_ctx *c, uint64_t *ct, size_t L, uint32_t galois_elt, const uint64_t *galois_key,
                                 size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct, galois_key);
    return moai_apply_galois_to(c, ct, ct, L, galois_elt, galois_key, batch, stream);
}

extern "C" int moai_apply_galois_acc(moai_ctx *c, const uint64_t *in, uint64_t *acc, size_t L, uint32_t galois_elt,
                                     const uint64_t *galois_key, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, acc, galois_key);
    trace_op("apply_galois_to", L, batch); // the same key switch; the addition that follows it is what is saved
    MOAI_TRY(check_level(c, L, batch * 2));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (!in || !acc || !galois_key || in == acc)
    {
        return set_error(MOAI_EINVAL, "null argument, or the sum is the input");
    }
    return apply_galois_impl(c, in, acc, L, galois_elt, galois_key, batch, stream, acc);
}

// ---- key switches on a list of ciphertexts, each with its own key and element ----------------------------------------------
namespace moai {

// one pass's list goes to device memory on the call's stream: the record travels as a kernel argument and thread i stores
// entry i (no host-to-device copy, which would read pageable memory after the call has returned)
__global__ __launch_bounds__(64) void ks_list_write_kernel(KsList h, KsList *d)
{
    const uint32_t i = threadIdx.x;
    d->ins[i] = h.ins[i];
    d->outs[i] = h.outs[i];
    d->sums[i] = h.sums[i];
    d->keys[i] = h.keys[i];
    d->tables[i] = h.tables[i];
    d->key_rows[i] = h.key_rows[i];
}

// the three steps of a list call that hybrid.hip's list forms share with the two below (launch.h)
int ks_list_write(const KsList &h, KsList *d, hipStream_t s)
{
    hipLaunchKernelGGL(ks_list_write_kernel, dim3(1), dim3((uint32_t)KS_LIST_MAX), 0, s, h, d);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

int ks_list_check_members(const uint64_t *const *ins, uint64_t *const *outs, const uint32_t *elts, const uint64_t *const *keys,
                          const uint64_t *one_key, size_t n, bool relin)
{
    if (!ins || !outs || (relin ? !one_key : (!elts || !keys)))
    {
        return set_error(MOAI_EINVAL, "null list");
    }
    for (size_t i = 0; i < n; ++i)
    {
        if (!ins[i] || !outs[i] || (!relin && !keys[i]))
        {
            return set_error(MOAI_EINVAL, "member %zu: null pointer", i);
        }
        if (!relin && !(elts[i] & 1u))
        {
            return set_error(MOAI_EINVAL, "member %zu: Galois element is not valid", i);
        }
    }
    return MOAI_OK;
}

int ks_list_check_blocks(const moai_ctx *c, const uint64_t *const *ins, uint64_t *const *outs, const uint32_t *elts,
                         const uint64_t *const *sums, size_t n, size_t in_bytes, size_t out_bytes, bool relin)
{
    for (size_t i = 0; i < n; ++i)
    {
        if (!relin && elts[i] >= 2 * c->n)
        {
            return set_error(MOAI_EINVAL, "member %zu: Galois element is not valid", i);
        }
        // a member's own blocks: the output may be the input or the sum exactly (apply_galois), never a part of them
        const uint64_t *sum = sums ? sums[i] : nullptr;
        if (outs[i] != ins[i] ? overlap(outs[i], out_bytes, ins[i], in_bytes) : relin)
        {
            return set_error(MOAI_EINVAL, "member %zu: the output overlaps the input", i);
        }
        if (sum && outs[i] != sum && overlap(outs[i], out_bytes, sum, out_bytes))
        {
            return set_error(MOAI_EINVAL, "member %zu: the output overlaps the sum", i);
        }
        if (sum && sum == ins[i])
        {
            return set_error(MOAI_EINVAL, "member %zu: the sum is the input", i); // as moai_apply_galois_acc
        }
    }
    // another member's blocks: passes and workgroups run in no order that a caller could rely on.  Every block sorted by its
    // start; a block that overlaps an output starts less than the longest block before the output's end, so each output looks at
    // the few blocks in that window: n log n, not n^2, for the lists a caller may pass (any n).
    struct Block
    {
        uintptr_t at;
        size_t bytes, member;
    };
    std::vector<Block> blocks;
    blocks.reserve(3 * n);
    for (size_t i = 0; i < n; ++i)
    {
        blocks.push_back({ (uintptr_t)ins[i], in_bytes, i });
        blocks.push_back({ (uintptr_t)outs[i], out_bytes, i });
        if (sums && sums[i])
        {
            blocks.push_back({ (uintptr_t)sums[i], out_bytes, i });
        }
    }
    std::sort(blocks.begin(), blocks.end(), [](const Block &x, const Block &y) { return x.at < y.at; });
    for (size_t i = 0; i < n; ++i)
    {
        const uintptr_t lo = (uintptr_t)outs[i], hi = lo + out_bytes;
        auto it = std::lower_bound(blocks.begin(), blocks.end(), lo > in_bytes ? lo - in_bytes : 0,
                                   [](const Block &x, uintptr_t v) { return x.at < v; });
        for (; it != blocks.end() && it->at < hi; ++it)
        {
            if (it->member != i && it->at + it->bytes > lo)
            {
                return set_error(MOAI_EINVAL, "member %zu: the output overlaps a block of member %zu", i, it->member);
            }
        }
    }
    return MOAI_OK;
}

// What the two list entry points share.  relin: member i is [3][L][N], its third polynomial is switched with `one_key` and the
// first two are added (moai_relinearize); else member i is [2][L][N] and gets apply_galois by elts[i] with keys[i], plus sums[i].
// Everything is validated before anything is enqueued; then at most KS_LIST_MAX members per pass: the list, one gather that
// also permutes (galois_gather_kernel<true>) into the contiguous scratch, and the key switch with the LIST kernels.
static int ks_ptrs_impl(moai_ctx *c, const uint64_t *const *ins, uint64_t *const *outs, size_t L, const uint32_t *elts,
                        const uint64_t *const *keys, const uint64_t *one_key, const uint64_t *const *sums, size_t n, bool relin, void *stream)
{
    if (n == 0)
    {
        return MOAI_OK;
    }
    MOAI_TRY(ks_list_check_members(ins, outs, elts, keys, one_key, n, relin));
    const size_t nb = n < KS_LIST_MAX ? n : KS_LIST_MAX; // members per pass
    MOAI_TRY(check_level(c, L, nb * (relin ? 3 : 2)));
    MOAI_TRY(check_switch_level(c, L));
    const size_t rn = L * c->n, in_bytes = (relin ? 3 : 2) * rn * sizeof(uint64_t), out_bytes = 2 * rn * sizeof(uint64_t);
    MOAI_TRY(ks_list_check_blocks(c, ins, outs, elts, sums, n, in_bytes, out_bytes, relin));
    std::vector<uint32_t> key_rows(n);
    if (relin)
    {
        MOAI_TRY(key_rows_for(c, one_key, L, &key_rows[0]));
        std::fill(key_rows.begin(), key_rows.end(), key_rows[0]);
    }
    for (size_t i = 0; !relin && i < n; ++i)
    {
        MOAI_TRY(key_rows_for(c, keys[i], L, &key_rows[i], (long)i));
    }
    std::vector<const uint32_t *> tables(n);
    for (size_t i = 0; i < n; ++i)
    {
        // relinearize: element 1, the identity permutation -- the gather then only collects the third polynomials
        MOAI_TRY(galois_table(c, relin ? 1u : elts[i], &tables[i]));
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t rows_tmp = relin ? L : 2 * L; // rows per member of the gathered target
    const size_t sz_list = align256(sizeof(KsList)), sz_tmp = align256(nb * rows_tmp * c->n * sizeof(uint64_t));
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    void *wsp;
    MOAI_TRY(workspace(c, sz_list + sz_tmp + switch_key_ws_bytes(c, L, nb), s, &wsp));
    KsList *dlist = static_cast<KsList *>(wsp);
    uint64_t *tmp = at_bytes(wsp, sz_list);
    return for_chunks(n, KS_LIST_MAX, [&](size_t m0, size_t cnt) {
        KsList h;
        for (size_t e = 0; e < KS_LIST_MAX; ++e)
        {
            const size_t i = m0 + (e < cnt ? e : 0); // the unused entries repeat the pass's first member
            h.ins[e] = ins[i];
            h.outs[e] = outs[i];
            h.sums[e] = sums ? sums[i] : nullptr;
            h.keys[e] = relin ? one_key : keys[i];
            h.tables[e] = tables[i];
            h.key_rows[e] = key_rows[i];
        }
        MOAI_TRY(ks_list_write(h, dlist, s));
        if (relin)
        {
            // tmp [cnt][L][N] = the members' third polynomials; out = (c0, c1) + switch_key(c2)   (evaluator.cpp:1383-1392)
            MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, L, 2 * L, s));
            return switch_key_impl(c, nullptr, { tmp, L, 0, dlist }, nullptr, L, cnt, at_bytes(wsp, sz_list + sz_tmp), s, { nullptr, 0, 1 });
        }
        // tmp [cnt][2][L][N] = galois(ins); out = (galois(in0), 0) + switch_key(galois(in1)) [+ sum]   (evaluator.cpp:2631-2654)
        MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, 2 * L, 0, s));
        return switch_key_impl(c, nullptr, { tmp, 2 * L, L, dlist }, nullptr, L, cnt, at_bytes(wsp, sz_list + sz_tmp), s, { tmp, 2 * L, 2 });
    });
}

} // namespace moai

extern "C" int moai_apply_galois_ptrs(moai_ctx *c, const uint64_t *const *ins, uint64_t *const *outs, size_t L, const uint32_t *galois_elts,
                                      const uint64_t *const *galois_keys, const uint64_t *const *sums, size_t n, void *stream)
{
    for (size_t i = 0; ins && outs && galois_keys && i < n; ++i)
    {
        MOAI_AUDIT(stream, ins[i], outs[i], galois_keys[i], sums ? sums[i] : nullptr);
    }
    trace_op("apply_galois_to", L, n); // the calls it replaces
    return ks_ptrs_impl(c, ins, outs, L, galois_elts, galois_keys, nullptr, sums, n, false, stream);
}

extern "C" int moai_relinearize_ptrs(moai_ctx *c, const uint64_t *const *ct3s, uint64_t *const *outs, const uint64_t *relin_key, size_t L,
                                     size_t n, void *stream)
{
    MOAI_AUDIT(stream, relin_key);
    for (size_t i = 0; ct3s && outs && i < n; ++i)
    {
        MOAI_AUDIT(stream, ct3s[i], outs[i]);
    }
    trace_op("relinearize", L, n);
    return ks_ptrs_impl(c, ct3s, outs, L, nullptr, nullptr, relin_key, nullptr, n, true, stream);
}

extern "C" int moai_modraise(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t L_out, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, out);
    trace_op("modraise", L_out, batch);
    const size_t P = batch * 2;
    MOAI_TRY(check_level(c, L_out, P));
    if (batch == 0)
    {
        return MOAI_OK;
    }
    if (!in || !out || in == out)
    {
        return set_error(MOAI_EINVAL, "bad pointers");
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = c->n * sizeof(uint64_t);
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    void *wsp;
    MOAI_TRY(workspace(c, align256(P * row_bytes), s, &wsp));
    uint64_t *src = static_cast<uint64_t *>(wsp);
    MOAI_HIP_CHECK(hipMemcpyAsync(src, in, P * row_bytes, hipMemcpyDeviceToDevice, s));
    RowMap rm;
    MOAI_TRY(make_rowmap(c, 1, nullptr, &rm));
    MOAI_TRY(ntt_launch(c, src, P, 1, rm, true, s));
    RaiseArgs g;
    g.src = src;
    g.out = out;
    g.pc = c->pc;
    g.Lout = (uint32_t)L_out;
    g.n2 = (uint32_t)(c->n >> 1);
    MOAI_TRY(launch_rows(modraise_kernel, c, P * L_out, s, g));
    MOAI_TRY(make_rowmap(c, L_out, nullptr, &rm));
    return ntt_launch(c, out, P, L_out, rm, false, s);
}

// ---- hoisted rotations (keyswitch_kernels.hip.h explains the identity) --------------------------------------------
namespace moai {

template <int LOGN, int MODE>
static void hoist_contig_finish(moai_ctx *c, uint64_t *tmp, size_t L, size_t batch, const KsGroup &grp, size_t G, hipStream_t s)
{
    // the strided pass left [B][G][L][N] in the mode's lazy form: the plain contiguous pass finishes every row of group
    // member g under that member's prime and leaves canonical residues
    constexpr uint32_t tpr = 1u << (LOGN - 12);
    const TwPair t = twiddles(c, MODE, false);
    for (size_t g = 0; g < G; ++g)
    {
        NttArgs a = ntt_args(c, tmp, batch, G * L, RowMap{}, false);
        a.tw = t.tw;
        a.twb = t.twb;
        a.Lsel = 0;
        for (size_t J = 0; J < L; ++J)
        {
            if (grp.slot[g] == J)
            {
                continue; // the strided pass skipped it: the digit under its own prime is read from the ciphertext
            }
            a.sel.idx[a.Lsel] = (uint32_t)(g * L + J);
            a.selp.idx[a.Lsel++] = grp.prime[g];
        }
        if (a.Lsel == 0)
        {
            continue; // L = 1: the only digit of a data prime's member is the one read from the ciphertext
        }
        a.total_work = a.n_poly * a.Lsel * tpr;
        hipLaunchKernelGGL((ntt_fwd_contig<LOGN, MODE>), dim3(a.total_work), dim3(256), 0, s, a);
    }
}

// what the rotations of one hoisted call share (one entry per rotation)
struct HoistRotations
{
    size_t R;
    const uint32_t *const *tables, *const *itables;
    const uint64_t *const *keys;
    const uint32_t *key_rows;
    const uint64_t *const *corrs;
    uint64_t *acc; // rotation r accumulates at acc + r * acc_stride_words
    size_t acc_stride_words;
};

template <int LOGN, int MODE>
static int hoist_group(moai_ctx *c, const uint64_t *t, uint64_t *tmp, const uint64_t *in, size_t L, size_t batch, const KsGroup &grp,
                       size_t G, const HoistRotations &rot, hipStream_t s)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    constexpr bool FP = MODE >= M_FPN;
    KsP1Args p1;
    p1.t = t;
    p1.tmp = tmp;
    p1.tw = twiddles(c, MODE, false).tw;
    p1.pc = c->pc;
    p1.grp = grp;
    p1.L = (uint32_t)L;
    p1.G = (uint32_t)G;
    p1.total_work = (uint32_t)(batch * G * L * TPR);
    hipLaunchKernelGGL((ks_fwd_strided<LOGN, MODE>), dim3(p1.total_work), dim3(256), 0, s, p1);
    MOAI_LAUNCH_CHECK();
    hoist_contig_finish<LOGN, MODE>(c, tmp, L, batch, grp, G, s);
    MOAI_LAUNCH_CHECK();
    // FP64 modes: four or two rotations per pass over the digits (ks_hoisted_mac2); MOAI_KS_HOIST_PAIR=0 keeps one per pass,
    // 2 at most two
    const long pair = FP ? tuning(K_KS_HOIST_PAIR) : 0;
    for (size_t r = 0; r < rot.R; ++r)
    {
        const size_t nr = pair >= 4 && r + 3 < rot.R ? 4 : (pair >= 1 && r + 1 < rot.R ? 2 : 1);
        if (nr > 1)
        {
            HoistMac2Args m2;
            m2.dig = tmp;
            m2.ct = in;
            for (size_t h = 0; h < 4; ++h)
            {
                const size_t rr = r + (h < nr ? h : 0);
                m2.itable[h] = rot.itables[rr];
                m2.key[h] = rot.keys[rr];
                m2.krows[h] = rot.key_rows[rr];
                m2.corr[h] = rot.corrs[rr];
                m2.acc[h] = rot.acc + rr * rot.acc_stride_words;
            }
            m2.pc = c->pc;
            m2.grp = grp;
            m2.L = (uint32_t)L;
            m2.G = (uint32_t)G;
            m2.k = (uint32_t)c->k;
            m2.B = (uint32_t)batch;
            m2.total_work = (uint32_t)(batch * G * TPR * 2);
            MOAI_TRY((dispatch<2, 4>("rotations per pass ", (int)nr, [&](auto NR) {
                hipLaunchKernelGGL((ks_hoisted_mac2<LOGN, MODE == M_FPR, decltype(NR)::value>), dim3(m2.total_work), dim3(256), 0, s, m2);
                return MOAI_OK;
            })));
            r += nr - 1;
            continue;
        }
        HoistMacArgs m;
        m.dig = tmp;
        m.ct = in;
        m.table = rot.tables[r];
        m.key = rot.keys[r];
        m.corr = rot.corrs[r];
        m.acc = rot.acc + r * rot.acc_stride_words;
        m.pc = c->pc;
        m.grp = grp;
        m.L = (uint32_t)L;
        m.G = (uint32_t)G;
        m.k = rot.key_rows[r];
        m.B = (uint32_t)batch;
        m.total_work = (uint32_t)(batch * G * TPR * 2);
        hipLaunchKernelGGL((ks_hoisted_mac<LOGN, FP, MODE == M_FPR>), dim3(m.total_work), dim3(256), 0, s, m);
    }
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

// workspace of one hoisted call of R rotations, byte offsets: flag | t [B][L][N] | tmp [B][G][L][N] | acc [R][B][2][L+1][N] |
// last [2B][N] | u [2B][L][N] | c0 [B][L][N]
struct HoistLayout
{
    size_t acc_stride_words;
    size_t flag, t, tmp, acc, last, u, c0, total;
};

static HoistLayout hoist_layout(const moai_ctx *c, size_t L, size_t batch, size_t R)
{
    const size_t row_bytes = c->n * sizeof(uint64_t);
    HoistLayout w;
    w.acc_stride_words = batch * 2 * (L + 1) * c->n;
    w.flag = 0;
    w.t = 256;
    w.tmp = w.t + align256(batch * L * row_bytes);
    w.acc = w.tmp + align256(batch * ks_group_size(c, L, batch) * L * row_bytes);
    w.last = w.acc + align256(R * w.acc_stride_words * sizeof(uint64_t));
    w.u = w.last + align256(batch * 2 * row_bytes);
    w.c0 = w.u + align256(2 * batch * L * row_bytes);
    w.total = w.c0 + align256(batch * L * row_bytes);
    return w;
}

int galois_sign_mask(moai_ctx *c, uint64_t *mask, uint32_t galois_elt, size_t copies, hipStream_t s)
{
    hipLaunchKernelGGL(galois_sign_mask_kernel, dim3((uint32_t)((c->n + 255) / 256)), dim3(256), 0, s, mask, (uint32_t)c->logn, galois_elt,
                       (uint32_t)copies);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

int probe_any_zero(moai_ctx *c, const uint64_t *v, size_t words, uint32_t *flag, hipStream_t s, bool *found)
{
    (void)c;
    MOAI_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(any_zero_kernel, dim3(1024), dim3(256), 0, s, v, words / 2, flag);
    MOAI_LAUNCH_CHECK();
    uint32_t host_flag = 0;
    MOAI_HIP_CHECK(hipMemcpyAsync(&host_flag, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MOAI_HIP_CHECK(hipStreamSynchronize(s));
    *found = host_flag != 0;
    return MOAI_OK;
}

} // namespace moai

extern "C" int moai_hoist_correction(moai_ctx *c, const uint64_t *galois_key, uint32_t galois_elt, size_t L, uint64_t *correction,
                                     void *stream)
{
    MOAI_AUDIT(stream, galois_key, correction);
    trace_op("hoist_correction", L, 1);
    MOAI_TRY(check_level(c, L, 2));
    if (!galois_key || !correction)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    if (c->k < 2 || L > c->k - 1)
    {
        return set_error(MOAI_EINVAL, "L exceeds the key's decomposition size");
    }
    MOAI_TRY(galois_elt_check(c, galois_elt));
    uint32_t key_rows = 0;
    MOAI_TRY(key_rows_for(c, galois_key, L, &key_rows));
    hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = c->n * sizeof(uint64_t);
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    void *wsp;
    MOAI_TRY(workspace(c, align256((L + 1) * row_bytes), s, &wsp));
    uint64_t *mask = static_cast<uint64_t *>(wsp);
    MOAI_TRY(galois_sign_mask(c, mask, galois_elt, L + 1, s));
    std::vector<uint32_t> pidx(L + 1);
    for (size_t i = 0; i < L; ++i)
    {
        pidx[i] = (uint32_t)i;
    }
    pidx[L] = (uint32_t)(c->k - 1);
    RowMap rm;
    MOAI_TRY(make_rowmap(c, L + 1, pidx.data(), &rm));
    MOAI_TRY(ntt_launch(c, mask, 1, L + 1, rm, false, s));
    HoistCorrArgs g;
    g.key = galois_key;
    g.mask = mask;
    g.out = correction;
    g.pc = c->pc;
    g.L = (uint32_t)L;
    g.k = (uint32_t)c->k;
    g.krows = key_rows;
    g.n2 = (uint32_t)(c->n >> 1);
    return launch_rows(ks_hoist_correction_kernel, c, 2 * (L + 1), s, g);
}

extern "C" int moai_apply_galois_hoisted(moai_ctx *c, const uint64_t *in, uint64_t *const *outs, size_t L, const uint32_t *galois_elts,
                                         const uint64_t *const *galois_keys, const uint64_t *const *corrections, size_t R, size_t batch,
                                         int *used_fallback, void *stream)
{
    MOAI_AUDIT(stream, in);
    for (size_t r = 0; outs && galois_keys && corrections && r < R; ++r)
    {
        MOAI_AUDIT(stream, outs[r], galois_keys[r], corrections[r]);
    }
    if (R > 64 && outs && galois_elts && galois_keys && corrections)
    {
        // the accumulators of one pass are sized for 64 rotations: more are done 64 at a time, each pass with its own digit
        // decomposition (the results do not depend on the grouping)
        int any_fallback = 0;
        for (size_t r0 = 0; r0 < R; r0 += 64)
        {
            int fb = 0;
            const int rc = moai_apply_galois_hoisted(c, in, outs + r0, L, galois_elts + r0, galois_keys + r0, corrections + r0,
                                                     R - r0 < 64 ? R - r0 : 64, batch, &fb, stream);
            if (rc)
            {
                return rc;
            }
            any_fallback |= fb;
        }
        if (used_fallback)
        {
            *used_fallback = any_fallback;
        }
        return MOAI_OK;
    }
    trace_op("apply_galois_hoisted", L, batch * R);
    if (used_fallback)
    {
        *used_fallback = 0;
    }
    MOAI_TRY(check_level(c, L, batch * 2));
    if (batch == 0 || R == 0)
    {
        return MOAI_OK;
    }
    if (!in || !outs || !galois_elts || !galois_keys || !corrections)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t n = c->n, k = c->k;
    MOAI_TRY(check_switch_level(c, L));
    hipStream_t s = (hipStream_t)stream;
    std::vector<const uint32_t *> tables(R), itables(R);
    for (size_t r = 0; r < R; ++r)
    {
        if (!galois_keys[r] || !corrections[r] || !outs[r] || outs[r] == in)
        {
            return set_error(MOAI_EINVAL, "null key, correction or output (an output must not be the input)");
        }
        MOAI_TRY(galois_table(c, galois_elts[r], &tables[r]));
        // the inverse permutation is the table of the inverse element (mod 2N, by Newton's iteration on an odd number)
        const uint32_t two_n_mask = (uint32_t)(2 * n - 1);
        uint32_t inv = galois_elts[r];
        for (int it = 0; it < 5; ++it)
        {
            inv = (inv * (2u - galois_elts[r] * inv)) & two_n_mask;
        }
        MOAI_TRY(galois_table(c, inv, &itables[r]));
    }
    std::vector<uint32_t> key_rows(R);
    for (size_t r = 0; r < R; ++r)
    {
        MOAI_TRY(key_rows_for(c, galois_keys[r], L, &key_rows[r]));
    }
    bool fallback = c->logn < 12;
    if (!fallback)
    {
        const HoistLayout w = hoist_layout(c, L, batch, R);
        std::unique_lock<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
        void *wsp;
        MOAI_TRY(workspace(c, w.total, s, &wsp));
        uint32_t *flag = reinterpret_cast<uint32_t *>(at_bytes(wsp, w.flag));
        uint64_t *t = at_bytes(wsp, w.t), *tmp = at_bytes(wsp, w.tmp), *acc = at_bytes(wsp, w.acc), *last = at_bytes(wsp, w.last);
        uint64_t *u = at_bytes(wsp, w.u), *pc0 = at_bytes(wsp, w.c0);
        const uint32_t n2 = (uint32_t)(n >> 1);
        // t = INTT(c1), UNPERMUTED: once for all rotations
        RowMap rm;
        MOAI_TRY(make_rowmap(c, L, nullptr, &rm));
        MOAI_TRY(ntt_launch(c, t, batch, L, rm, true, s, in, 2 * L, L));
        MOAI_TRY(probe_any_zero(c, t, batch * L * n, flag, s, &fallback)); // a zero coefficient: the identity above does not hold for it
        if (!fallback)
        {
            const HoistRotations rot = { R, tables.data(), itables.data(), galois_keys, key_rows.data(), corrections, acc, w.acc_stride_words };
            for (const KsPlanGroup &pg : ks_plan(c, L, batch))
            {
                MOAI_TRY(dispatch_ks(c->logn, pg.mode, [&](auto LG, auto MD) {
                    return hoist_group<decltype(LG)::value, decltype(MD)::value>(c, t, tmp, in, L, batch, pg.grp, pg.g, rot, s);
                }));
            }
            // per rotation: the permuted c0 is the addend, then the shared mod-down tail (evaluator.cpp:2913-3018)
            for (size_t r = 0; r < R; ++r)
            {
                uint64_t *acc_r = acc + r * w.acc_stride_words;
                // pc0 [B][L][N] = perm(c0 of in): the addend of the even polynomials (add_mode 2, ciphertexts L rows apart)
                MOAI_TRY(galois_permute_c0(c, in, pc0, batch, L, galois_elts[r], s));
                MOAI_TRY(launch_rows(sum_rows_kernel, c, batch * 2, s, acc_r, last, (uint32_t)(L + 1), (uint32_t)L, 1u, (size_t)0, c->pc,
                                     (uint32_t)(k - 1), n2));
                MOAI_TRY(moddown(c, last, acc_r, (uint32_t)(L + 1), u, outs[r], batch * 2, L, (uint32_t)(k - 1), { pc0, L, 2 }, s));
            }
            return MOAI_OK;
        }
    }
    // fallback: the reference's sequence per rotation
    if (used_fallback)
    {
        *used_fallback = 1;
    }
    for (size_t r = 0; r < R; ++r)
    {
        MOAI_TRY(moai_apply_galois_to(c, in, outs[r], L, galois_elts[r], galois_keys[r], batch, stream));
    }
    return MOAI_OK;
}

// ---- level-trimmed key residency ------------------------------------------------------------------------------------------------
extern "C" size_t moai_key_words(const moai_ctx *c, size_t levels)
{
    if (!c || c->k < 2)
    {
        return 0;
    }
    const size_t lv = levels > c->k - 1 ? c->k - 1 : levels;
    return lv * 2 * (lv + 1) * c->n;
}

extern "C" int moai_key_trim(moai_ctx *c, const uint64_t *full_key, size_t levels, uint64_t *trimmed, void *stream)
{
    MOAI_AUDIT(stream, full_key, trimmed);
    if (!c || !full_key || !trimmed)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    MOAI_TRY(enter_device(c));
    const size_t k = c->k, n = c->n;
    if (k < 2 || levels < 1 || levels > k - 1)
    {
        return set_error(MOAI_EINVAL, "levels must lie in 1 .. %zu", k < 2 ? (size_t)0 : k - 1);
    }
    {
        std::lock_guard<std::mutex> g(*static_cast<std::mutex *>(c->mutex));
        if (c->key_layouts.count(full_key))
        {
            return set_error(MOAI_EINVAL, "the source of moai_key_trim must be a key in the reference's layout");
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = levels + 1;
    for (size_t J = 0; J < levels; ++J)
    {
        for (size_t K = 0; K < 2; ++K)
        {
            const uint64_t *src = full_key + (J * 2 + K) * k * n;
            uint64_t *dst = trimmed + (J * 2 + K) * rows * n;
            MOAI_HIP_CHECK(hipMemcpyAsync(dst, src, levels * n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
            MOAI_HIP_CHECK(hipMemcpyAsync(dst + levels * n, src + (k - 1) * n, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
        }
    }
    std::lock_guard<std::mutex> g(*static_cast<std::mutex *>(c->mutex));
    c->key_layouts[trimmed] = moai_ctx::KeyLayout{ (uint32_t)levels, (uint32_t)rows };
    return MOAI_OK;
}

extern "C" int moai_key_register(moai_ctx *c, const uint64_t *key, size_t levels)
{
    if (!c || !key)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t k = c->k;
    if (k < 2 || levels < 1 || levels > k - 1)
    {
        return set_error(MOAI_EINVAL, "levels must lie in 1 .. %zu", k < 2 ? (size_t)0 : k - 1);
    }
    std::lock_guard<std::mutex> g(*static_cast<std::mutex *>(c->mutex));
    auto it = c->key_layouts.find(key);
    if (it != c->key_layouts.end() && (it->second.digits != levels || it->second.rows != levels + 1))
    {
        return set_error(MOAI_EINVAL, "the address is recorded as a key of %u levels; moai_key_forget it first", it->second.digits);
    }
    c->key_layouts[key] = moai_ctx::KeyLayout{ (uint32_t)levels, (uint32_t)(levels + 1) };
    return MOAI_OK;
}

extern "C" int moai_key_forget(moai_ctx *c, const uint64_t *key)
{
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    std::lock_guard<std::mutex> g(*static_cast<std::mutex *>(c->mutex));
    c->key_layouts.erase(key);
    return MOAI_OK;
}
