// hybrid.hip -- hybrid key switching: alpha special primes, digits of alpha data primes.
//
// Reference: Evaluator::switch_key_inplace (SEAL/evaluator.cpp:2724-3020) and KeyGenerator::generate_one_kswitch_key
// (SEAL/keygenerator.cpp:303-336) are exactly the alpha = 1 case of what is computed here; include/moai_hip.h, section
// "hybrid key switching", states the algorithm for any alpha and tests/hybrid_ref.py restates it in integers.
//
// Context primes m_0 .. m_{k-1}: special p_t = m_{k-alpha+t}, P their product; data q_i = m_i, i < k - alpha.  At L data primes
// digit j < beta = ceil(L / alpha) is the rows R_j = [j alpha, min((j+1) alpha, L)), D_j their product.
//
// Structure on the device, unfused, per chunk of the batch (scratch per ciphertext: the rows of hy_plan_switch, N words each):
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
// Rounding mode (moai_hybrid_set_rounding, an atomic of the context): every mod-down above is hy_mod_down -> hy_convert; in
// MOAI_HYBRID_ROUND_EXACT that one launch takes hy_convert_kernel<.., true>, which removes the fast conversion's overflow with a
// binary64 estimate (the header states the contract, the kernel derives the error bound).  An entry point reads the mode once
// (hy_exact) and hands it down as `exact`; the mod-ups, the constants' cache and every other launch do not depend on it.
// Every transform goes through ntt_launch with a RowMap.  The constants of one (L, alpha) live in one device block (HyTable)
// that the context owns.
//
// Files: the argument structs, the constant blocks and every kernel are in hybrid_kernels.hip.h; this file is the host code.  The
// scratch of a chunk is planned by hybrid_scratch.h (host only, no context, no device): each call family (switch, hoisted, pt-dot,
// bsgs, rescale) states its regions once -- a name, a row count, held per ciphertext or per (group, ciphertext) pair -- and from that
// one statement a HyPlan takes the row totals that size a chunk under MOAI_HYBRID_TMP_KB, the 256-aligned offsets and the total.
// Three sizing policies: ciphertexts only; ciphertexts, then groups beside them; groups first with the chunks evened out.
#include <algorithm>
#include <mutex>
#include <vector>

#include "hostmath.h"
#include "launch.h"
#include "modarith.hip.h"

#include "hybrid_kernels.hip.h"
#include "hybrid_scratch.h"

namespace moai {

// ---- host side ------------------------------------------------------------------------------------------------------------
static HyDims hy_dims(const moai_ctx *c, size_t L, size_t alpha)
{
    HyDims d;
    d.alpha = (uint32_t)alpha;
    d.beta = (uint32_t)hy_beta(L, alpha);
    d.k = (uint32_t)c->k;
    fill_rows(d, c, L);
    return d;
}

// the bytes of scratch a chunk may take (MOAI_HYBRID_TMP_KB), for the plans of hybrid_scratch.h
static size_t hy_budget()
{
    return (size_t)std::max(1l, tuning(K_HYBRID_TMP_KB)) << 10;
}

// the context's rounding mode (moai_hybrid_set_rounding), read ONCE by every entry point before anything else: all the mod-downs of
// a call, and the separate calls of a fallback, round alike whatever another thread sets meanwhile
static bool hy_exact(const moai_ctx *c)
{
    return c && c->hybrid_rounding.load(std::memory_order_relaxed) == MOAI_HYBRID_ROUND_EXACT;
}

static uint64_t *hy_at(void *wsp, const HyPlan &p, HyRegion r)
{
    return at_bytes(wsp, p.off[r]);
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

// P mod m, P the product of the alpha special primes
static uint64_t hy_p_mod(const moai_ctx *c, size_t alpha, uint64_t m)
{
    uint64_t r = 1 % m;
    for (size_t s = 0; s < alpha; ++s)
    {
        r = mulmod(r, c->primes[c->k - alpha + s] % m, m);
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

// cv = the mod-down by W, the product of the context primes src[0 .. nsrc), to the data primes 0 .. ntgt-1, with the rounding terms
// of floor(W / 2) and the constants of the exact mode (HyConv states the formulas)
static void hy_moddown_conv(const moai_ctx *c, HyConv &cv, const uint32_t *src, size_t nsrc, size_t ntgt)
{
    cv.nsrc = (uint32_t)nsrc;
    cv.ntgt = (uint32_t)ntgt;
    for (size_t r = 0; r < nsrc; ++r)
    {
        const uint64_t m = c->primes[src[r]];
        cv.src_prime[r] = src[r];
        cv.src_inv[r] = make_tw(hy_invmod(hy_prod_mod(c, src, nsrc, r, m), m), m);
        cv.src_pre[r] = hy_half_mod(0, m);
        cv.src_rinv[r] = 1.0 / (double)m; // two roundings: the conversion, then the division
    }
    for (size_t i = 0; i < ntgt; ++i)
    {
        const uint64_t q = c->primes[i], w_mod_q = hy_prod_mod(c, src, nsrc, nsrc, q);
        cv.tgt_prime[i] = (uint32_t)i;
        cv.tgt_post[i] = hy_half_mod(w_mod_q, q);
        cv.tgt_negw[i] = q - w_mod_q; // W and q are coprime: in (0, q)
        for (size_t r = 0; r < nsrc; ++r)
        {
            cv.w[i][r] = hy_prod_mod(c, src, nsrc, r, q);
        }
    }
}

// The device block of constants the context caches under `key`; the caller holds op_mutex.  Built on first use: fill(host) writes the
// zeroed block of `bytes`, which goes over with a blocking copy from a host buffer that lives until the copy has returned.
template <class T, class Fill>
static int hy_cached_table(moai_ctx *c, std::pair<size_t, size_t> key, size_t bytes, const char *what, const T **out, Fill &&fill)
{
    auto it = c->hybrid_tables.find(key);
    if (it == c->hybrid_tables.end())
    {
        std::vector<unsigned char> host(bytes, 0);
        fill(host.data());
        void *dev = nullptr;
        MOAI_HIP_CHECK(hipMalloc(&dev, bytes));
        hipError_t e = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess)
        {
            (void)hipFree(dev);
            return set_error(MOAI_EHIP, "hybrid %s constants: %s", what, hipGetErrorString(e));
        }
        it = c->hybrid_tables.emplace(key, dev).first;
    }
    *out = static_cast<const T *>(it->second);
    return MOAI_OK;
}

// the constants for (L, alpha)
static int hy_table(moai_ctx *c, size_t L, size_t alpha, const HyTable **out)
{
    const size_t k = c->k, beta = hy_beta(L, alpha);
    const size_t conv_bytes = offsetof(HyTable, conv) + (beta + 1) * sizeof(HyConv);
    const size_t bytes = conv_bytes + beta * (L + alpha) * sizeof(uint64_t);
    return hy_cached_table(c, std::make_pair(L, alpha), bytes, "key-switch", out, [&](unsigned char *host) {
        HyTable *t = reinterpret_cast<HyTable *>(host);
        HyConv *convs = reinterpret_cast<HyConv *>(host + offsetof(HyTable, conv));
        for (size_t i = 0; i < L; ++i)
        {
            const uint64_t q = c->primes[i];
            t->pinv[i] = make_tw(hy_invmod(hy_p_mod(c, alpha, q), q), q);
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
        RowMap special{};
        hy_rowmap(c, L, alpha, 0, L, &special);
        hy_moddown_conv(c, convs[beta], special.idx, alpha, L);
        // the hoisted rotations' correction: sum_{r in R_j} q_r (D_j / q_r) = |R_j| D_j, modulo every row's prime (0 on the rows of R_j)
        uint64_t *mult = reinterpret_cast<uint64_t *>(host + conv_bytes);
        for (size_t j = 0; j < beta; ++j)
        {
            const HyConv &cv = convs[j];
            for (size_t row = 0; row < L + alpha; ++row)
            {
                const uint64_t m = c->primes[hy_row_prime(row, L, alpha, k)];
                mult[j * (L + alpha) + row] = mulmod(cv.nsrc % m, hy_prod_mod(c, cv.src_prime, cv.nsrc, cv.nsrc, m), m);
            }
        }
    });
}

// exact: the mod-down of MOAI_HYBRID_ROUND_EXACT, a separate instantiation; the mod-ups are always fast
static int hy_convert(moai_ctx *c, const uint64_t *src, size_t src_stride, size_t src_off, uint64_t *dst, const HyConv *cv, size_t nsrc,
                      size_t polys, hipStream_t s, bool exact = false)
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
    if (exact)
    {
        return dispatch<1, 2, 4, 8, 16>("digit size ", amax,
                                        [&](auto A) { return launch_rows(hy_convert_kernel<decltype(A)::value, true>, c, polys, s, a); });
    }
    return dispatch<1, 2, 4, 8, 16>("digit size ", amax,
                                    [&](auto A) { return launch_rows(hy_convert_kernel<decltype(A)::value>, c, polys, s, a); });
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

// A mod-down up to its last kernel, for `polys` polynomials whose nsrc source rows -- the last nsrc of a switch's L + alpha -- are
// rows off .. off + nsrc - 1 of every `stride` rows at src: x [polys][nsrc][N] = INTT(those rows), conv [polys][ntgt][N] = NTT(cv's
// base conversion with the rounding terms, fast or exact as the call's rounding mode says), ntgt = L + alpha - nsrc
static int hy_mod_down(moai_ctx *c, const HyConv *cv, const uint64_t *src, size_t stride, size_t off, size_t nsrc, size_t ntgt, size_t polys,
                       uint64_t *x, uint64_t *conv, size_t L, size_t alpha, bool exact, hipStream_t s)
{
    RowMap rm{};
    hy_rowmap(c, L, alpha, 0, ntgt, &rm);
    MOAI_TRY(ntt_launch(c, x, polys, nsrc, rm, true, s, src, stride, off));
    MOAI_TRY(hy_convert(c, x, nsrc, 0, conv, cv, nsrc, polys, s, exact));
    MOAI_TRY(make_rowmap(c, ntgt, nullptr, &rm));
    return ntt_launch(c, conv, polys, ntgt, rm, false, s);
}

// step 5 up to the last kernel, for the accumulators [B][2][L + alpha][N] of B switches: x [2B][alpha][N] = INTT(special rows),
// conv [2B][L][N]
static int hy_step5(moai_ctx *c, const HyTable *tab, const uint64_t *acc, uint64_t *x, uint64_t *conv, size_t L, size_t alpha, size_t B,
                    bool exact, hipStream_t s)
{
    return hy_mod_down(c, tab->conv + hy_beta(L, alpha), acc, L + alpha, L, alpha, L, 2 * B, x, conv, L, alpha, exact, s);
}

// the hy_mac_kernel / hy_hoisted_mac_kernel grid: blockIdx.x = ciphertext, .y covers a row, .z = row of L + alpha
static int hy_mac_grid(const moai_ctx *c, size_t B, size_t rows, dim3 *grid)
{
    MOAI_CHECK_GRID_ROWS(rows);
    *grid = dim3((uint32_t)B, row_grid(c, 1).x, (uint32_t)rows);
    return MOAI_OK;
}

// step 4 for B ciphertexts: acc = the inner products of the digits of the target rows tg (ext, and the target's own rows) with `key`
// or, with tg.lst, member b's own
static int hy_mac(moai_ctx *c, const KsTarget &tg, const uint64_t *ext, const uint64_t *key, uint64_t *acc, size_t L, size_t alpha, size_t B,
                  hipStream_t s)
{
    HyMacArgs m;
    m.ext = ext;
    m.tgt = tg.ptr;
    m.key = key;
    m.acc = acc;
    m.tgt_stride = (uint32_t)tg.stride_rows;
    m.tgt_off = (uint32_t)tg.off_rows;
    m.d = hy_dims(c, L, alpha);
    dim3 grid;
    MOAI_TRY(hy_mac_grid(c, B, L + alpha, &grid));
    return plain_or_list<HyMacListArgs>(m, tg.lst, [&](const auto &args, auto LIST) {
        hipLaunchKernelGGL(hy_mac_kernel<decltype(LIST)::value>, grid, dim3(256), 0, s, args);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    });
}

// rotations of the next pass of a hoisted MAC over the digits when `left` are left: MOAI_HYBRID_HOIST_NR of them, 4, 2 or 1
static size_t hy_pass_size(size_t left)
{
    const long per_pass = tuning(K_HYBRID_HOIST_NR);
    return per_pass >= 4 && left >= 4 ? 4 : (per_pass >= 2 && left >= 2 ? 2 : 1);
}

// one chunk of B ciphertexts: out [B][2][L][N] = add (KsAddend) + the switch of the target rows tg.  With tg.lst (a device record,
// common.h KsList) ciphertext b's key is lst->keys[b] and the last kernel writes lst->outs[b], adds lst->sums[b] and, for add.mode 1,
// reads the addend from lst->ins[b]; key and out are not used
static int hy_switch_chunk(moai_ctx *c, const HyTable *tab, uint64_t *out, const KsTarget &tg, const uint64_t *key, size_t L, size_t alpha,
                           size_t B, void *wsp, const HyPlan &w, const KsAddend &add, bool exact, hipStream_t s)
{
    uint64_t *ext = hy_at(wsp, w, HY_EXT), *acc = hy_at(wsp, w, HY_ACC), *conv = hy_at(wsp, w, HY_CONV);
    // 1. t = INTT(target); 2., 3. mod-up of every digit and the forward transform of the converted rows
    MOAI_TRY(hy_decompose(c, tab, tg, L, alpha, B, hy_at(wsp, w, HY_T), ext, s));
    // 4. the inner products with the key
    MOAI_TRY(hy_mac(c, tg, ext, key, acc, L, alpha, B, s));
    // 5. mod-down: x = INTT(special rows), conv = NTT(base conversion with the rounding terms), out = addend + (acc - conv) / P
    MOAI_TRY(hy_step5(c, tab, acc, hy_at(wsp, w, HY_X), conv, L, alpha, B, exact, s));
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
// exact: the rounding mode the entry point read (hy_exact)
static int hy_entry(moai_ctx *c, int kind, uint64_t *io, const uint64_t *in, const uint64_t *key, size_t L, size_t alpha, uint32_t elt,
                    size_t batch, bool exact, void *stream, const uint64_t *sum = nullptr)
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
    // 2 L rows in front: the permuted input of apply_galois
    const HyPlan w = hy_plan_switch(n, L, alpha, batch, kind == HY_GALOIS ? 2 * L : 0, hy_budget());
    void *wsp;
    MOAI_TRY(workspace(c, w.total, s, &wsp));
    return for_chunks(batch, w.cb, [&](size_t b0, size_t B) {
        switch (kind)
        {
        case HY_SWITCH:
            // ct += switch(target)
            return hy_switch_chunk(c, tab, io + b0 * 2 * L * n, { in + b0 * L * n, L, 0 }, key, L, alpha, B, wsp, w,
                                   { io + b0 * 2 * L * n, 2 * L, 1 }, exact, s);
        case HY_RELIN:
            // out = (c0, c1) + switch(c2)      (evaluator.cpp:1383-1392)
            return hy_switch_chunk(c, tab, io + b0 * 2 * L * n, { in + b0 * 3 * L * n, 3 * L, 2 * L }, key, L, alpha, B, wsp, w,
                                   { in + b0 * 3 * L * n, 3 * L, 1 }, exact, s);
        default:
        {
            // out = (galois(in0), 0) + switch(galois(in1)) [+ sum]      (evaluator.cpp:2631-2654): both summands are added by the last
            // kernel, so a chunk of out is written once, after the chunk of in has been permuted into the scratch
            uint64_t *tmp = hy_at(wsp, w, HY_HEAD);
            MOAI_TRY(moai_galois_permute(c, in + b0 * 2 * L * n, tmp, B * 2, L, elt, stream));
            return hy_switch_chunk(c, tab, io + b0 * 2 * L * n, { tmp, 2 * L, L }, key, L, alpha, B, wsp, w,
                                   { tmp, 2 * L, 2, sum ? sum + b0 * 2 * L * n : nullptr }, exact, s);
        }
        }
    });
}

// ---- hoisted rotations ------------------------------------------------------------------------------------------------------
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

// What a chunk of the three hoisted families (their plans keep the probe's flag in front) begins with, under the lock it holds to the
// chunk's end -- per chunk, because a fallback re-enters hy_entry, which takes the lock itself: the constants, the workspace of plan p
// and, with `decompose`, steps 1-3 on the UNPERMUTED c1 of the B ciphertexts at `in` [B][2][L][N], once for everything that reads the
// digits, and the zero probe: *fallback is set when INTT(c1) holds a zero coefficient, for which the identity does not hold.  Then
// body(tab, wsp).
template <class F>
static int hy_hoisted_chunk(moai_ctx *c, const HyPlan &p, const uint64_t *in, size_t L, size_t alpha, size_t B, bool decompose,
                            bool *fallback, hipStream_t s, F &&body)
{
    std::lock_guard<std::mutex> op_lock(*static_cast<std::mutex *>(c->op_mutex));
    const HyTable *tab;
    MOAI_TRY(hy_table(c, L, alpha, &tab));
    void *wsp;
    MOAI_TRY(workspace(c, p.total, s, &wsp));
    if (decompose)
    {
        uint64_t *t = hy_at(wsp, p, HY_T);
        MOAI_TRY(hy_decompose(c, tab, { in, 2 * L, L }, L, alpha, B, t, hy_at(wsp, p, HY_EXT), s));
        MOAI_TRY(probe_any_zero(c, t, B * L * c->n, static_cast<uint32_t *>(wsp), s, fallback));
    }
    return body(tab, wsp);
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
    dim3 grid;
    MOAI_TRY(hy_mac_grid(c, B, L + alpha, &grid));
    for (size_t r = 0; r < g;)
    {
        const size_t nr = hy_pass_size(g - r);
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

// one chunk of B ciphertexts at `in` [B][2][L][N] on plan p; rotation r's result goes to rot.outs[r] + out_off.  *fallback is set
// when INTT(c1) holds a zero coefficient: nothing but the scratch has been written then, and the caller makes the separate calls.
static int hy_hoist_chunk_run(moai_ctx *c, const uint64_t *in, size_t out_off, const HyHoistRotations &rot, size_t L, size_t alpha, size_t B,
                              const HyPlan &p, bool *fallback, bool exact, hipStream_t s)
{
    const size_t n = c->n;
    return hy_hoisted_chunk(c, p, in, L, alpha, B, true, fallback, s, [&](const HyTable *tab, void *wsp) -> int {
        if (*fallback)
        {
            return MOAI_OK;
        }
        uint64_t *acc = hy_at(wsp, p, HY_ACC), *conv = hy_at(wsp, p, HY_CONV), *pc0 = hy_at(wsp, p, HY_C0);
        return for_chunks(rot.R, p.G, [&](size_t r0, size_t g) {
            MOAI_TRY(hy_hoisted_mac(c, hy_at(wsp, p, HY_EXT), in, rot, r0, g, acc, L, alpha, B, s));
            // pc0 [g][B][L][N] = perm_r(c0): the addend of the even polynomials (add_mode 2, ciphertexts L rows apart)
            for (size_t r = 0; r < g; ++r)
            {
                MOAI_TRY(galois_permute_c0(c, in, pc0 + r * B * L * n, B, L, rot.elts[r0 + r], s));
            }
            // steps 5 over (rotation, ciphertext) pairs
            MOAI_TRY(hy_step5(c, tab, acc, hy_at(wsp, p, HY_X), conv, L, alpha, g * B, exact, s));
            for (size_t r = 0; r < g; ++r)
            {
                MOAI_TRY(moddown_finalize(c, acc + r * B * 2 * (L + alpha) * n, (uint32_t)(L + alpha), conv + r * B * 2 * L * n,
                                          rot.outs[r0 + r] + out_off, 2 * B, L, tab->pinv, { pc0 + r * B * L * n, L, 2 }, nullptr, s));
            }
            return MOAI_OK;
        });
    });
}

// ---- plaintext-weighted sums of hoisted rotations -------------------------------------------------------------------------------
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

static HyDotScratch hy_dot_scratch(void *wsp, const HyPlan &p)
{
    return { hy_at(wsp, p, HY_T), hy_at(wsp, p, HY_EXT), hy_at(wsp, p, HY_GAL), hy_at(wsp, p, HY_ACC) };
}

// The inner stage for the outputs gs[0 .. ng) of one chunk of B ciphertexts at `in`, up to its step 5: o.S and o.add (o.ng = ng)
// receive S_g and the addend a_g of every output, and o.seeded tells which outputs have a switched term (the S of the others is
// not written).  sc.t / sc.ext hold the digits of the unpermuted c1 unless `fallback`, which takes every rotation through the
// unhoisted steps 1-4 on the permuted input, to the same bits.  Shared by moai_hybrid_rotate_pt_dot and moai_hybrid_bsgs_dot.
static int hy_dot_inner(moai_ctx *c, const HyTable *tab, const uint64_t *in, const HyDotTerms &tm, const size_t *gs, size_t ng,
                        HyDotOutputs &o, const HyDotScratch &sc, size_t L, size_t alpha, size_t B, bool fallback, hipStream_t s)
{
    const size_t ct_words = B * 2 * L * c->n;
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
            const size_t nr = hy_pass_size(rot.size() - i);
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
        const KsTarget tg = { sc.gal, 2 * L, L };
        for (size_t r : rot)
        {
            MOAI_TRY(moai_galois_permute(c, in, sc.gal, B * 2, L, tm.elts[r], s));
            MOAI_TRY(hy_decompose(c, tab, tg, L, alpha, B, sc.t, sc.ext, s));
            MOAI_TRY(hy_mac(c, tg, sc.ext, tm.keys[r], sc.acc, L, alpha, B, s));
            MOAI_TRY(hy_dot_term(c, sc.acc, sc.gal, o, tm, gs, ng, r, L, alpha, B, s));
        }
    }
    for (size_t r : ident)
    {
        MOAI_TRY(hy_dot_term(c, nullptr, in, o, tm, gs, ng, r, L, alpha, B, s));
    }
    return MOAI_OK;
}

// one chunk of B ciphertexts at `in` [B][2][L][N] on plan p; output g's result goes to tm.outs[g] + out_off.  sw: the outputs with a
// term whose element is not 1, p.G of them in flight; the others (idn) are sums of plain products.  *fallback is set when INTT(c1)
// holds a zero coefficient: the chunk then takes every rotation through the unhoisted steps 1-4 on the permuted input, to the same
// bits.
static int hy_dot_chunk_run(moai_ctx *c, const uint64_t *in, size_t out_off, const HyDotTerms &tm, const std::vector<size_t> &sw,
                            const std::vector<size_t> &idn, size_t L, size_t alpha, size_t B, const HyPlan &p, bool *fallback, bool exact,
                            hipStream_t s)
{
    const size_t n = c->n, ct_words = B * 2 * L * n;
    // steps 1-3 and the probe only where an output has a switched term
    return hy_hoisted_chunk(c, p, in, L, alpha, B, !sw.empty(), fallback, s, [&](const HyTable *tab, void *wsp) -> int {
        const HyDotScratch sc = hy_dot_scratch(wsp, p);
        uint64_t *S = hy_at(wsp, p, HY_S), *conv = hy_at(wsp, p, HY_CONV), *add = hy_at(wsp, p, HY_ADD);
        MOAI_TRY(for_chunks(sw.size(), p.G, [&](size_t g0, size_t ng) {
            const size_t *gs = sw.data() + g0;
            HyDotOutputs o{};
            o.S = S;
            o.add = add;
            o.ng = (uint32_t)ng;
            MOAI_TRY(hy_dot_inner(c, tab, in, tm, gs, ng, o, sc, L, alpha, B, *fallback, s));
            // step 5 once per output, over (output, ciphertext) pairs
            MOAI_TRY(hy_step5(c, tab, S, hy_at(wsp, p, HY_X), conv, L, alpha, ng * B, exact, s));
            for (size_t h = 0; h < ng; ++h)
            {
                MOAI_TRY(moddown_finalize(c, S + h * B * 2 * (L + alpha) * n, (uint32_t)(L + alpha), conv + h * ct_words,
                                          tm.outs[gs[h]] + out_off, 2 * B, L, tab->pinv, { add + h * ct_words, 2 * L, 1 }, nullptr, s));
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
    });
}

// ---- giant steps summed in the extended basis --------------------------------------------------------------------------------------
struct HyBsgsGiants
{
    size_t n;
    const uint32_t *elts;
    const uint32_t *const *tables; // null where the element is 1
    const uint64_t *const *keys;
    const std::vector<char> *switched; // giant step g's inner sum has a term whose baby element is not 1
};

// one chunk of B ciphertexts at `in` [B][2][L][N] into out [B][2][L][N] on plan p; tm holds the baby terms with one output per giant
// step (tm.outs unused), p.G giant steps in flight.  *fallback as in hy_dot_chunk_run: the inner stage's zero probe.
static int hy_bsgs_chunk_run(moai_ctx *c, const uint64_t *in, uint64_t *out, const HyDotTerms &tm, const HyBsgsGiants &gi, bool any_switched,
                             size_t L, size_t alpha, size_t B, const HyPlan &p, bool *fallback, bool exact, hipStream_t s)
{
    const size_t n = c->n, s_words = B * 2 * (L + alpha) * n;
    return hy_hoisted_chunk(c, p, in, L, alpha, B, any_switched, fallback, s, [&](const HyTable *tab, void *wsp) -> int {
        const HyDotScratch sc = hy_dot_scratch(wsp, p);
        uint64_t *Z = hy_at(wsp, p, HY_Z), *zconv = hy_at(wsp, p, HY_ZCONV);
        uint64_t *S = hy_at(wsp, p, HY_S), *add = hy_at(wsp, p, HY_ADD), *x = hy_at(wsp, p, HY_X), *conv = hy_at(wsp, p, HY_CONV);
        uint64_t *tgt = hy_at(wsp, p, HY_TGT), *ext2 = hy_at(wsp, p, HY_EXT2);
        HyBsgsMacArgs m{};
        m.ext = ext2;
        m.tgt = tgt;
        m.S = S;
        m.add = add;
        m.Z = Z;
        m.d = hy_dims(c, L, alpha);
        for (size_t i = 0; i < L; ++i)
        {
            m.fac[i] = hy_p_mod(c, alpha, c->primes[i]);
        }
        dim3 grid;
        MOAI_TRY(hy_mac_grid(c, B, L + alpha, &grid));
        MOAI_TRY(for_chunks(gi.n, p.G, [&](size_t g0, size_t ng) {
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
                    MOAI_TRY(hy_mod_down(c, tab->conv + hy_beta(L, alpha), S, 2 * (L + alpha), (L + alpha) + L, alpha, L, n_md * B, x, conv,
                                         L, alpha, exact, s));
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
                MOAI_TRY(hy_decompose(c, tab, { tgt, L, 0 }, L, alpha, n_rot * B, hy_at(wsp, p, HY_T2), ext2, s));
            }
            m.n_rot = (uint32_t)n_rot;
            m.ng = (uint32_t)ng;
            m.zseeded = g0 ? 1u : 0u;
            hipLaunchKernelGGL(hy_bsgs_mac_kernel, grid, dim3(256), 0, s, m);
            MOAI_LAUNCH_CHECK();
            return MOAI_OK;
        }));
        // the one final step 5, both polynomials, no addend
        MOAI_TRY(hy_step5(c, tab, Z, hy_at(wsp, p, HY_ZX), zconv, L, alpha, B, exact, s));
        return moddown_finalize(c, Z, (uint32_t)(L + alpha), zconv, out, 2 * B, L, tab->pinv, {}, nullptr, s);
    });
}

// ---- relinearize + rescale --------------------------------------------------------------------------------------------------------
// the merged mod-down's constants share the context's map with hy_table's blocks: the same (L, alpha) with this bit in alpha
constexpr size_t HY_RESCALE_KEY = (size_t)1 << 32;

// the constants of the merged mod-down for (L, alpha), L >= 2 and alpha + 1 <= HY_MAX_ALPHA
static int hy_rescale_table(moai_ctx *c, size_t L, size_t alpha, const HyRescaleTable **out)
{
    const auto key = std::make_pair(L, alpha | HY_RESCALE_KEY);
    return hy_cached_table(c, key, sizeof(HyRescaleTable), "relinearize-rescale", out, [&](unsigned char *host) {
        HyRescaleTable *t = reinterpret_cast<HyRescaleTable *>(host);
        const size_t last = L - 1;
        RowMap src{}; // q_{L-1}, then the special primes: W is their product
        const size_t nsrc = hy_rowmap(c, L, alpha, 0, last, &src);
        hy_moddown_conv(c, t->conv, src.idx, nsrc, last);
        for (size_t i = 0; i < last; ++i)
        {
            const uint64_t q = c->primes[i];
            t->winv[i] = make_tw(hy_invmod(hy_prod_mod(c, src.idx, nsrc, nsrc, q), q), q);
            t->qinv[i] = make_tw(hy_invmod(c->primes[last] % q, q), q);
        }
    });
}

// one chunk of B ciphertexts: out [B][2][L - 1][N] = the merged mod-down of (c0, c1) + switch(c2) for ct3 [B][3][L][N].  With lst (a
// device record, common.h KsList) c2 [B][L][N] has been gathered to the plan's head, c0 and c1 are read from lst->ins[b], the key is
// lst->keys[b] and the result goes to lst->outs[b]; ct3, key and out are not used
static int hy_rescale_chunk_run(moai_ctx *c, const HyTable *tab, const HyRescaleTable *rt, const uint64_t *ct3, const uint64_t *key,
                                uint64_t *out, size_t L, size_t alpha, size_t B, void *wsp, const HyPlan &w, bool exact, hipStream_t s,
                                const KsList *lst = nullptr)
{
    uint64_t *ext = hy_at(wsp, w, HY_EXT), *acc = hy_at(wsp, w, HY_ACC), *conv = hy_at(wsp, w, HY_CONV);
    // steps 1-4 on c2, as every switch
    const KsTarget tg = lst ? KsTarget{ hy_at(wsp, w, HY_HEAD), L, 0, lst } : KsTarget{ ct3, 3 * L, 2 * L };
    MOAI_TRY(hy_decompose(c, tab, tg, L, alpha, B, hy_at(wsp, w, HY_T), ext, s));
    MOAI_TRY(hy_mac(c, tg, ext, key, acc, L, alpha, B, s));
    // the lift of the one data row among the sources (the rows below it take theirs in the last kernel)
    HyLiftArgs lf;
    lf.acc = acc;
    lf.ct3 = ct3;
    lf.d = hy_dims(c, L, alpha);
    lf.plast = hy_p_mod(c, alpha, c->primes[L - 1]);
    MOAI_TRY(plain_or_list<HyLiftListArgs>(lf, lst, [&](const auto &args, auto LIST) {
        return launch_rows(hy_lift_last_row_kernel<decltype(LIST)::value>, c, 2 * B, s, args);
    }));
    // the merged mod-down: x = INTT(rows L-1 .. L+alpha-1 of acc, contiguous), conv = NTT(base conversion with W's rounding terms)
    MOAI_TRY(hy_mod_down(c, &rt->conv, acc, L + alpha, L - 1, alpha + 1, L - 1, 2 * B, hy_at(wsp, w, HY_X), conv, L, alpha, exact, s));
    HyRescaleFinalArgs f;
    f.acc = acc;
    f.conv = conv;
    f.ct3 = ct3;
    f.out = out;
    f.winv = rt->winv; // device address arithmetic only
    f.qinv = rt->qinv;
    f.d = lf.d;
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
    const bool exact = hy_exact(c);
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
    // 3 L rows in front: the three-polynomial product
    const HyPlan w = hy_plan_rescale(n, L, alpha, batch, product ? 3 * L : 0, hy_budget());
    void *wsp;
    MOAI_TRY(workspace(c, w.total, s, &wsp));
    return for_chunks(batch, w.cb, [&](size_t b0, size_t B) {
        const uint64_t *ct3 = x + b0 * 3 * L * n;
        if (product)
        {
            HyProductArgs g;
            g.x = x + b0 * 2 * L * n;
            g.y = y + b0 * 2 * L * n;
            g.out = hy_at(wsp, w, HY_HEAD);
            fill_rows(g, c, L);
            MOAI_TRY(launch_rows(hy_ct_product_kernel, c, B * L, s, g));
            ct3 = g.out;
        }
        return hy_rescale_chunk_run(c, tab, rt, ct3, key, out + b0 * 2 * (L - 1) * n, L, alpha, B, wsp, w, exact, s);
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
// galois_gather_list permutes the members (or, with the identity table, collects their third polynomials) into the head of the
// chunk's contiguous scratch, steps 1-3 and the mod-down's transforms run on that scratch as they do for a batch, and the MAC and the
// last kernels take the member's key, addends and output from the record.
static int hy_ptrs_impl(moai_ctx *c, int kind, const uint64_t *const *ins, uint64_t *const *outs, size_t L, size_t alpha,
                        const uint32_t *elts, const uint64_t *const *keys, const uint64_t *one_key, const uint64_t *const *sums, size_t n,
                        void *stream)
{
    const bool relin = kind != HY_LIST_GALOIS, rescale = kind == HY_LIST_RESCALE, exact = hy_exact(c);
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
    const HyPlan w = rescale ? hy_plan_rescale(c->n, L, alpha, n, gal_rows, hy_budget(), KS_LIST_MAX)
                             : hy_plan_switch(c->n, L, alpha, n, gal_rows, hy_budget(), KS_LIST_MAX);
    const size_t sz_list = align256(sizeof(KsList));
    void *wsp;
    MOAI_TRY(workspace(c, sz_list + w.total, s, &wsp));
    KsList *dlist = static_cast<KsList *>(wsp);
    void *chunk = at_bytes(wsp, sz_list);
    return for_chunks(n, w.cb, [&](size_t m0, size_t cnt) {
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
        uint64_t *tmp = hy_at(chunk, w, HY_HEAD);
        switch (kind)
        {
        case HY_LIST_GALOIS:
            // tmp [cnt][2][L][N] = galois(ins); out = (galois(in0), 0) + switch(galois(in1)) [+ sum]   (evaluator.cpp:2631-2654)
            MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, 2 * L, 0, s));
            return hy_switch_chunk(c, tab, nullptr, { tmp, 2 * L, L, dlist }, nullptr, L, alpha, cnt, chunk, w, { tmp, 2 * L, 2 }, exact, s);
        case HY_LIST_RELIN:
            // tmp [cnt][L][N] = the members' third polynomials; out = (c0, c1) + switch(c2)   (evaluator.cpp:1383-1392)
            MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, L, 2 * L, s));
            return hy_switch_chunk(c, tab, nullptr, { tmp, L, 0, dlist }, nullptr, L, alpha, cnt, chunk, w, { nullptr, 0, 1 }, exact, s);
        default:
            MOAI_TRY(galois_gather_list(c, dlist, tmp, cnt, L, 2 * L, s));
            return hy_rescale_chunk_run(c, tab, rt, nullptr, nullptr, nullptr, L, alpha, cnt, chunk, w, exact, s, dlist);
        }
    });
}

// ---- what the entry points of the hoisted families share ------------------------------------------------------------------------------
// an even element is refused before the context is looked at: oddness needs none
static int hy_odd_check(const uint32_t *elts, size_t n)
{
    for (size_t r = 0; elts && r < n; ++r)
    {
        MOAI_TRY(galois_elt_check(nullptr, elts[r]));
    }
    return MOAI_OK;
}

// output i of outs, ct_bytes long, against the input and the outputs before it
static int hy_output_alias_check(uint64_t *const *outs, size_t i, const uint64_t *in, size_t ct_bytes)
{
    if (overlap(outs[i], ct_bytes, in, ct_bytes))
    {
        return set_error(MOAI_EINVAL, "an output must not alias the input");
    }
    for (size_t q = 0; q < i; ++q)
    {
        if (overlap(outs[i], ct_bytes, outs[q], ct_bytes))
        {
            return set_error(MOAI_EINVAL, "an output must not alias another output");
        }
    }
    return MOAI_OK;
}

// (*tables)[r] = the permutation table of elts[r], built before the first launch of the call; with skip_identity null where the
// element is 1
static int hy_galois_tables(moai_ctx *c, const uint32_t *elts, size_t n, bool skip_identity, std::vector<const uint32_t *> *tables)
{
    tables->assign(n, nullptr);
    for (size_t r = 0; r < n; ++r)
    {
        if (!skip_identity || elts[r] != 1)
        {
            MOAI_TRY(galois_table(c, elts[r], &(*tables)[r]));
        }
    }
    return MOAI_OK;
}

// the terms plains[g * R + r], r < R, of sum g: whether it has any, and whether one of them is switched (its element is not 1)
static void hy_term_census(const uint64_t *const *plains, size_t g, size_t R, const uint32_t *elts, bool *any, bool *switched)
{
    *any = *switched = false;
    for (size_t r = 0; r < R; ++r)
    {
        if (plains[g * R + r])
        {
            *any = true;
            *switched = *switched || elts[r] != 1;
        }
    }
}

// run(off, B, &fallback) for every chunk of at most cb of the batch's ciphertexts of ct_words words each, off the chunk's word offset;
// a chunk that reports a fallback sets *used_fallback (where given) and then runs on_fallback(off, B)
template <class Run, class OnFallback>
static int hy_batch_chunks(size_t batch, size_t cb, size_t ct_words, int *used_fallback, Run &&run, OnFallback &&on_fallback)
{
    return for_chunks(batch, cb, [&](size_t b0, size_t B) {
        const size_t off = b0 * ct_words;
        bool fallback = false;
        MOAI_TRY(run(off, B, &fallback));
        if (fallback)
        {
            if (used_fallback)
            {
                *used_fallback = 1;
            }
            MOAI_TRY(on_fallback(off, B));
        }
        return MOAI_OK;
    });
}

template <class Run>
static int hy_batch_chunks(size_t batch, size_t cb, size_t ct_words, int *used_fallback, Run &&run)
{
    return hy_batch_chunks(batch, cb, ct_words, used_fallback, run, [](size_t, size_t) { return MOAI_OK; });
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
    for (size_t r = 0; r < MOAI_MAX_RNS; ++r)
    {
        a.fac[r] = r < Lmax ? hy_p_mod(c, alpha, c->primes[r]) : 0;
    }
    return launch_rows(hy_key_add_kernel, c, Lmax, stream, a);
}

extern "C" int moai_switch_key_hybrid(moai_ctx *c, uint64_t *ct, const uint64_t *target, const uint64_t *key, size_t L, size_t alpha,
                                      size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct, target, key);
    trace_op("switch_key_hybrid", L, batch);
    return hy_entry(c, HY_SWITCH, ct, target, key, L, alpha, 1, batch, hy_exact(c), stream);
}

extern "C" int moai_relinearize_hybrid(moai_ctx *c, const uint64_t *ct3, const uint64_t *key, uint64_t *out, size_t L, size_t alpha,
                                       size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct3, key, out);
    trace_op("relinearize_hybrid", L, batch);
    return hy_entry(c, HY_RELIN, out, ct3, key, L, alpha, 1, batch, hy_exact(c), stream);
}

extern "C" int moai_apply_galois_hybrid(moai_ctx *c, uint64_t *ct, size_t L, size_t alpha, uint32_t galois_elt, const uint64_t *key,
                                        size_t batch, void *stream)
{
    MOAI_AUDIT(stream, ct, key);
    trace_op("apply_galois_hybrid", L, batch);
    return hy_entry(c, HY_GALOIS, ct, ct, key, L, alpha, galois_elt, batch, hy_exact(c), stream);
}

extern "C" int moai_apply_galois_hybrid_to(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t L, size_t alpha, uint32_t galois_elt,
                                           const uint64_t *key, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, out, key);
    trace_op("apply_galois_hybrid", L, batch);
    return hy_entry(c, HY_GALOIS, out, in, key, L, alpha, galois_elt, batch, hy_exact(c), stream);
}

extern "C" int moai_apply_galois_hybrid_acc(moai_ctx *c, const uint64_t *in, uint64_t *acc, size_t L, size_t alpha, uint32_t galois_elt,
                                            const uint64_t *key, size_t batch, void *stream)
{
    MOAI_AUDIT(stream, in, acc, key);
    trace_op("apply_galois_hybrid", L, batch); // the same switch; the addition that follows it is what is saved
    return hy_entry(c, HY_GALOIS, acc, in, key, L, alpha, galois_elt, batch, hy_exact(c), stream, acc);
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
    const bool exact = hy_exact(c);
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
        MOAI_TRY(hy_output_alias_check(outs, r, in, ct_bytes));
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::vector<const uint32_t *> tables;
    MOAI_TRY(hy_galois_tables(c, galois_elts, R, false, &tables));
    const HyHoistRotations rot = { R, galois_elts, tables.data(), keys, corrections, outs };
    const HyPlan p = hy_plan_hoisted(n, L, alpha, batch, R, hy_budget());
    return hy_batch_chunks(
        batch, p.cb, 2 * L * n, used_fallback,
        [&](size_t off, size_t B, bool *fallback) { return hy_hoist_chunk_run(c, in + off, off, rot, L, alpha, B, p, fallback, exact, s); },
        [&](size_t off, size_t B) {
            // the separate rotations of this chunk, each on a copy of the input (they take the lock and the workspace themselves)
            for (size_t r = 0; r < R; ++r)
            {
                MOAI_HIP_CHECK(hipMemcpyAsync(outs[r] + off, in + off, B * 2 * L * n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
                MOAI_TRY(hy_entry(c, HY_GALOIS, outs[r] + off, outs[r] + off, keys[r], L, alpha, galois_elts[r], B, exact, stream));
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
    MOAI_TRY(hy_odd_check(galois_elts, R));
    MOAI_TRY(hy_check(c, alpha, L, true));
    const bool exact = hy_exact(c);
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
        MOAI_TRY(hy_output_alias_check(outs, g, in, ct_bytes));
        bool any, switched;
        hy_term_census(plains, g, R, galois_elts, &any, &switched);
        if (!any)
        {
            return set_error(MOAI_EINVAL, "output %zu has no term", g);
        }
        (switched ? sw : idn).push_back(g);
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::vector<const uint32_t *> tables;
    MOAI_TRY(hy_galois_tables(c, galois_elts, R, true, &tables));
    const HyDotTerms tm = { R, n_out, galois_elts, tables.data(), keys, corrections, plains, outs };
    const HyPlan p = hy_plan_dot(n, L, alpha, batch, std::max<size_t>(sw.size(), 1), HY_DOT_MAX_NG, hy_budget());
    return hy_batch_chunks(batch, p.cb, 2 * L * n, used_fallback, [&](size_t off, size_t B, bool *fallback) {
        return hy_dot_chunk_run(c, in + off, off, tm, sw, idn, L, alpha, B, p, fallback, exact, s);
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
    MOAI_TRY(hy_odd_check(baby_elts, R));
    MOAI_TRY(hy_odd_check(giant_elts, n_giant));
    MOAI_TRY(hy_check(c, alpha, L, true));
    const bool exact = hy_exact(c);
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
        bool any, sw;
        hy_term_census(plains, g, R, baby_elts, &any, &sw);
        if (!any)
        {
            return set_error(MOAI_EINVAL, "giant step %zu has no term", g);
        }
        switched[g] = sw;
        any_switched = any_switched || sw;
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    std::vector<const uint32_t *> baby_tables, giant_tables;
    MOAI_TRY(hy_galois_tables(c, baby_elts, R, true, &baby_tables));
    MOAI_TRY(hy_galois_tables(c, giant_elts, n_giant, true, &giant_tables));
    const HyDotTerms tm = { R, n_giant, baby_elts, baby_tables.data(), baby_keys, baby_corrections, plains, nullptr };
    const HyBsgsGiants gi = { n_giant, giant_elts, giant_tables.data(), giant_keys, &switched };
    const HyPlan p = hy_plan_bsgs(n, L, alpha, batch, n_giant, HY_DOT_MAX_NG, hy_budget());
    return hy_batch_chunks(batch, p.cb, 2 * L * n, used_fallback, [&](size_t off, size_t B, bool *fallback) {
        return hy_bsgs_chunk_run(c, in + off, out + off, tm, gi, any_switched, L, alpha, B, p, fallback, exact, s);
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

extern "C" int moai_hybrid_set_rounding(moai_ctx *c, int mode)
{
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (mode != MOAI_HYBRID_ROUND_FAST && mode != MOAI_HYBRID_ROUND_EXACT)
    {
        return set_error(MOAI_EINVAL, "rounding mode %d: MOAI_HYBRID_ROUND_FAST (0) or MOAI_HYBRID_ROUND_EXACT (1)", mode);
    }
    c->hybrid_rounding.store(mode, std::memory_order_relaxed);
    return MOAI_OK;
}

extern "C" int moai_hybrid_rounding(const moai_ctx *c, int *mode)
{
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (!mode)
    {
        return set_error(MOAI_EINVAL, "null mode pointer");
    }
    *mode = c->hybrid_rounding.load(std::memory_order_relaxed);
    return MOAI_OK;
}
