// decoder.hip -- the client's output path on the device: Decryptor::ckks_decrypt (SEAL/decryptor.cpp:154-187, 299-381) and
// CKKSEncoder::decode_internal (SEAL/ckks.h:644-761), bit-identical to the reference's scalar x86-64 build.
//
// Decrypt is exact integer arithmetic: one launch for a batch, out = sum_i c_i * s^i mod q with the powers of s formed in
// registers.
//
// Decode, per chunk of plaintexts (the scratch is bounded, see chunk_items in ckks_decode_impl):
//   moai_ntt_inverse  : on a scratch copy of the rows (the caller's input is never modified; the reference copies too)
//   dec_compose<NW>   : exact CRT composition of every coefficient into the words of x in [0, Q), then the reference's
//                       word-by-word conversion to double (ckks.h:713-753), one coefficient per thread
//   dec_fft_head<R>   : the first logn-12 stages of DWTHandler::transform_to_rev (gaps >= 4096) in registers
//   dec_fft_tail      : the last min(logn, 12) stages in 4096-element LDS tiles, then the matrix_reps_index_map_ gather
//
// Composition.  x is accumulated prime by prime, x_{i+1} = x_i + v_i * P_i with P_i = q_0 ... q_{i-1} and the mixed-radix digit
// v_i = (a_i - x_i mod q_i) * P_i^-1 mod q_i (Garner); x_i mod q_i is  sum_w x_i[w] * (2^64w mod q_i)  with Shoup operands.
// Only the words of x are live (no digit array), so they stay in VGPRs at every level: NW (the next power of two >= the
// words of Q) is a template parameter and every word loop is unrolled with a uniform bound.  x < Q at every step, so no
// final reduction.  At MOAI's 36 primes (1743 bits, 28 words, NW = 32) the kernel holds 64 VGPRs of x; its register count
// and occupancy are recorded in DESIGN.md.  The constants of a set of rows (words of every P_i, Q and (Q+1)/2, the
// Shoup operands) are built on the host on first use of that set and kept in the context.
//
// Conversion.  The reference adds  (double)word * scaled_two_pow_64  with the factor starting at 1/scale and multiplied by
// 2^64 after every word, and skips a zero word (diff ? ... : 0.0) instead of multiplying it: at 36 primes and scale 2^46 the
// factor overflows to +inf from word 17 on, and 0 * inf would be NaN.  Words at and above the words of Q are zero on both
// sides of the comparison, so skipping them adds or subtracts 0.0 to an accumulator that is never -0.0: the same bits.
// (double) of a 64-bit word is correctly rounded on both sides: x86-64's conversion, and gfx950's  cvt(hi) * 2^32 + cvt(lo)
// with one rounding in the final add.
//
// DWT.  Every butterfly is  u + y*r, u - y*r  with the complex product as four separately rounded products and two sums
// (std::complex<double> operator* on finite values; the file is compiled with -ffp-contract=off), so any parallel schedule
// gives the reference's bits.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "hostmath.h"
#include "launch.h"
#include "modarith.hip.h"

namespace moai {

constexpr int DEC_TILE_LOG = 12;
constexpr uint32_t DEC_TILE = 1u << DEC_TILE_LOG;
constexpr uint32_t DEC_SCALES = 128; // plaintexts per compose launch: their 1/scale travel in the kernel arguments

// ---- decrypt ------------------------------------------------------------------------------------------------------------
struct DecryptArgs
{
    const uint64_t *ct; // [n_batch][size][L][N]
    const uint64_t *sk; // [L][N]
    uint64_t *out;      // [n_batch][L][N]
    const PrimeConst *pc;
    RowMap rows;
    uint32_t size;
    uint32_t L;
    uint32_t logn;
};

__global__ __launch_bounds__(256) void dec_decrypt(DecryptArgs g)
{
    const uint32_t n = 1u << g.logn;
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n)
    {
        return;
    }
    const uint32_t r = blockIdx.y;
    const size_t b = blockIdx.z;
    const PrimeConst pc = g.pc[g.rows.idx[r]];
    const size_t row = (size_t)n * g.L;
    const uint64_t *c = g.ct + b * g.size * row + (size_t)r * n + p;
    const uint64_t s = g.sk[(size_t)r * n + p];
    uint64_t acc = c[0];
    uint64_t spow = s;
    for (uint32_t i = 1; i < g.size; i++)
    {
        const uint64_t t = mulmod_barrett(c[i * row], spow, pc.q, pc.cr0, pc.cr1);
        acc = csub(acc + t, pc.q); // both below q < 2^61
        if (i + 1 < g.size)
        {
            spow = mulmod_barrett(spow, s, pc.q, pc.cr0, pc.cr1);
        }
    }
    g.out[(b * g.L + r) * n + p] = acc;
}

// ---- decode: composition and conversion ----------------------------------------------------------------------------------
struct ComposeArgs
{
    const uint64_t *in; // coefficient form [n_batch][L][N]
    double2 *out;       // [n_batch][N]
    const Tw *pw;       // [L][W]: 2^(64 w) mod q_i
    const Tw *invp;     // [L]: P_i^-1 mod q_i
    const uint64_t *P;  // [L][W]: words of P_i
    const uint64_t *nw; // [L]: significant words of P_i
    const uint64_t *q;  // [L]
    const uint64_t *Q;  // [W]
    const uint64_t *T;  // [W]: upper_half_threshold = (Q + 1) / 2
    uint32_t L;
    uint32_t W;
    uint32_t logn;
    uint32_t zero_mask; // sparse decode: coefficients with (p & zero_mask) != 0 are projected away (0 = keep all)
    double inv_scale[DEC_SCALES];
};

template <int NW>
__global__ __launch_bounds__(256) void dec_compose(ComposeArgs g)
{
    const uint32_t n = 1u << g.logn;
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n)
    {
        return;
    }
    const uint32_t b = blockIdx.y;
    if (p & g.zero_mask)
    {
        // ckks.h:704-712 zeroes the composed words; the conversion of an all-zero x is +0.0
        g.out[(size_t)b * n + p] = make_double2(0.0, 0.0);
        return;
    }
    const uint64_t *in = g.in + (size_t)b * g.L * n + p;
    uint64_t x[NW];
#pragma unroll
    for (int w = 0; w < NW; w++)
    {
        x[w] = 0;
    }
    for (uint32_t i = 0; i < g.L; i++)
    {
        const uint64_t q = g.q[i];
        const uint64_t q2 = q << 1;
        const uint32_t nw = (uint32_t)g.nw[i];
        const Tw *pw = g.pw + (size_t)i * g.W;
        const uint64_t *P = g.P + (size_t)i * g.W;
        // x mod q_i; x < P_i has nw words
        uint64_t acc = 0;
#pragma unroll
        for (int w = 0; w < NW; w++)
        {
            if ((uint32_t)w < nw)
            {
                acc = csub(acc + mul_shoup_lazy(x[w], pw[w].w, pw[w].wq, q), q2);
            }
        }
        acc = csub(acc, q);
        const uint64_t a = in[(size_t)i * n];
        const uint64_t d = submod(a, acc, q);
        const Tw ip = g.invp[i];
        const uint64_t v = csub(mul_shoup_lazy(d, ip.w, ip.wq, q), q);
        // x += v * P_i  (the sum is below P_{i+1}: the carry out of word nw - 1 lands in word nw, which is zero)
        uint64_t carry = 0;
#pragma unroll
        for (int w = 0; w < NW; w++)
        {
            if ((uint32_t)w < nw)
            {
                const uint64_t pwd = P[w];
                uint64_t lo = v * pwd;
                uint64_t hi = mulhi64(v, pwd);
                lo += carry;
                hi += lo < carry ? 1 : 0;
                const uint64_t s = x[w] + lo;
                hi += s < lo ? 1 : 0;
                x[w] = s;
                carry = hi;
            }
            else if ((uint32_t)w == nw)
            {
                x[w] += carry;
            }
        }
    }
    // is_greater_than_or_equal_uint(x, upper_half_threshold) (ckks.h:716-717)
    int cmp = 0;
#pragma unroll
    for (int w = NW - 1; w >= 0; w--)
    {
        if ((uint32_t)w < g.W && cmp == 0)
        {
            const uint64_t t = g.T[w];
            cmp = x[w] > t ? 1 : (x[w] < t ? -1 : 0);
        }
    }
    const double two_pow_64 = 18446744073709551616.0;
    double scaled = g.inv_scale[b];
    double res = 0.0;
    if (cmp >= 0)
    {
        // ckks.h:718-733: per word, no borrow between words
#pragma unroll
        for (int w = 0; w < NW; w++)
        {
            if ((uint32_t)w < g.W)
            {
                const uint64_t Qw = g.Q[w];
                if (x[w] > Qw)
                {
                    const uint64_t diff = x[w] - Qw;
                    res += diff ? static_cast<double>(diff) * scaled : 0.0;
                }
                else
                {
                    const uint64_t diff = Qw - x[w];
                    res -= diff ? static_cast<double>(diff) * scaled : 0.0;
                }
                scaled *= two_pow_64;
            }
        }
    }
    else
    {
        // ckks.h:735-741
#pragma unroll
        for (int w = 0; w < NW; w++)
        {
            if ((uint32_t)w < g.W)
            {
                res += x[w] ? static_cast<double>(x[w]) * scaled : 0.0;
                scaled *= two_pow_64;
            }
        }
    }
    g.out[(size_t)b * n + p] = make_double2(res, 0.0);
}

// ---- decode: DWTHandler::transform_to_rev (dwthandler.h:94-191, no scalar) -------------------------------------------------
// (x, y) <- (u + v, u - v) with u = x, v = y * r (Arithmetic<complex<double>, complex<double>, double>, ckks.h:46-81)
__device__ __forceinline__ void ct_cbfly(double &xr, double &xi, double &yr, double &yi, double rr, double ri)
{
    const double ac = yr * rr, bd = yi * ri, ad = yr * ri, bc = yi * rr;
    const double vr = ac - bd, vi = ad + bc;
    const double ur = xr, ui = xi;
    xr = ur + vr;
    xi = ui + vi;
    yr = ur - vr;
    yi = ui - vi;
}

// stages 0..R-1 (gap = n / 2^(s+1) >= 4096): thread p holds elements p + k * 4096, k < 2^R; stage s pairs k with
// k + 2^(R-s-1), group k >> (R-s), root root_powers_[2^s + group]
template <int R>
__global__ __launch_bounds__(256) void dec_fft_head(double2 *data, const double2 *roots, uint32_t logn)
{
    constexpr uint32_t K = 1u << R;
    const uint32_t n = 1u << logn;
    const uint32_t p = blockIdx.x * 256 + threadIdx.x; // < 4096: the grid covers exactly one tile
    double2 *d = data + (size_t)blockIdx.y * n + p;
    double xr[K], xi[K];
#pragma unroll
    for (uint32_t k = 0; k < K; k++)
    {
        const double2 v = d[k * DEC_TILE];
        xr[k] = v.x;
        xi[k] = v.y;
    }
#pragma unroll
    for (int s = 0; s < R; s++)
    {
        const uint32_t half = K >> (s + 1);
#pragma unroll
        for (uint32_t k = 0; k < K; k++)
        {
            if (!(k & half))
            {
                const double2 r = roots[(1u << s) + (k >> (R - s))];
                ct_cbfly(xr[k], xi[k], xr[k + half], xi[k + half], r.x, r.y);
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < K; k++)
    {
        d[k * DEC_TILE] = make_double2(xr[k], xi[k]);
    }
}

struct TailArgs
{
    const double2 *data;   // [n_batch][N]
    const double2 *roots;  // root_powers_ [N]
    const uint32_t *src;   // [N]: slot whose matrix_reps_index_map_ entry is this position
    double *out;           // [n_batch][out_slots] or [n_batch][out_slots][2]
    uint32_t logn;
    uint32_t out_slots;    // N/2, or the sparse slot count
    uint32_t first_stage;  // max(logn - 12, 0)
    uint32_t is_complex;
};

__global__ __launch_bounds__(256) void dec_fft_tail(TailArgs g)
{
    __shared__ double re[DEC_TILE];
    __shared__ double im[DEC_TILE];
    const uint32_t n = 1u << g.logn;
    const uint32_t slots = g.out_slots;
    const uint32_t tile = n < DEC_TILE ? n : DEC_TILE;
    const uint32_t tiles = n / tile;
    const uint32_t b = blockIdx.x / tiles;
    const uint32_t base = (blockIdx.x % tiles) * tile;
    const uint32_t tid = threadIdx.x;
    const double2 *in = g.data + (size_t)b * n + base;
    for (uint32_t k = tid; k < tile; k += 256)
    {
        const double2 v = in[k];
        re[k] = v.x;
        im[k] = v.y;
    }
    __syncthreads();
    for (uint32_t s = g.first_stage; s < g.logn; s++)
    {
        const uint32_t lg = g.logn - s - 1; // log2(gap)
        const uint32_t gap = 1u << lg;
        const double2 *roots = g.roots + (1u << s) + (base >> (lg + 1));
        for (uint32_t t = tid; t < (tile >> 1); t += 256)
        {
            const uint32_t grp = t >> lg;
            const uint32_t x = (grp << (lg + 1)) + (t & (gap - 1));
            const uint32_t y = x + gap;
            const double2 r = roots[grp];
            double xr = re[x], xi = im[x], yr = re[y], yi = im[y];
            ct_cbfly(xr, xi, yr, yi, r.x, r.y);
            re[x] = xr;
            im[x] = xi;
            re[y] = yr;
            im[y] = yi;
        }
        __syncthreads();
    }
    // destination[i] = res[matrix_reps_index_map_[i]] for i < out_slots (ckks.h:757-760), through the inverse map
    for (uint32_t k = tid; k < tile; k += 256)
    {
        const uint32_t slot = g.src[base + k];
        if (slot < slots)
        {
            if (g.is_complex)
            {
                double *o = g.out + ((size_t)b * slots + slot) * 2;
                o[0] = re[k];
                o[1] = im[k];
            }
            else
            {
                g.out[(size_t)b * slots + slot] = re[k];
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// the composition constants of one set of rows, one block of 64-bit words: offsets of the parts in ComposeArgs order
struct DecLayout
{
    size_t pw, invp, P, nw, q, Q, T, words;
    DecLayout(size_t L, size_t W)
        : pw(0), invp(pw + 2 * L * W), P(invp + 2 * L), nw(P + L * W), q(nw + L), Q(q + L), T(Q + W), words(T + W)
    {
    }
};

// fills the table pointers, L and W (the words of Q) of `a`, building the block on first use of the set of rows
static int dec_table(moai_ctx *c, const RowMap &rows, size_t L, ComposeArgs *a)
{
    std::lock_guard<std::mutex> g(*static_cast<std::mutex *>(c->mutex));
    std::vector<uint32_t> key(rows.idx, rows.idx + L);
    // P[i] = q_0 ... q_{i-1}, prod = Q
    std::vector<uint64_t> prod(1, 1);
    std::vector<std::vector<uint64_t>> P(L);
    for (size_t i = 0; i < L; i++)
    {
        P[i] = prod;
        mul_word(prod, c->primes[rows.idx[i]]);
    }
    const size_t W = prod.size();
    const DecLayout lay(L, W);
    auto it = c->dec_tables.find(key);
    const uint64_t *base = it != c->dec_tables.end() ? it->second : nullptr;
    if (!base)
    {
        std::vector<uint64_t> h(lay.words, 0);
        for (size_t i = 0; i < L; i++)
        {
            const uint64_t q = c->primes[rows.idx[i]];
            const uint64_t two64 = (uint64_t)(((u128)1 << 64) % q);
            uint64_t pwr = 1;
            for (size_t w = 0; w < W; w++)
            {
                const Tw t = make_tw(pwr, q);
                h[lay.pw + 2 * (i * W + w)] = t.w;
                h[lay.pw + 2 * (i * W + w) + 1] = t.wq;
                pwr = mulmod(pwr, two64, q);
            }
            // P_i mod q_i, then its inverse (q_i is prime and coprime to the others)
            uint64_t pm = 0;
            for (size_t w = P[i].size(); w-- > 0;)
            {
                pm = (uint64_t)((((u128)pm << 64) | P[i][w]) % q);
            }
            if (pm == 0)
            {
                return set_error(MOAI_EINVAL, "prime_index repeats a prime");
            }
            const Tw ip = make_tw(powmod(pm, q - 2, q), q);
            h[lay.invp + 2 * i] = ip.w;
            h[lay.invp + 2 * i + 1] = ip.wq;
            std::copy(P[i].begin(), P[i].end(), h.begin() + lay.P + i * W);
            h[lay.nw + i] = P[i].size();
            h[lay.q + i] = q;
        }
        // upper_half_threshold = (Q + 1) >> 1 (SEAL/context.cpp:376-382); Q is odd so Q + 1 does not carry out of W words
        std::copy(prod.begin(), prod.end(), h.begin() + lay.Q);
        for (size_t w = 0; w < W; w++)
        {
            if (++prod[w] != 0)
            {
                break;
            }
        }
        for (size_t w = 0; w < W; w++)
        {
            h[lay.T + w] = (prod[w] >> 1) | (w + 1 < W ? prod[w + 1] << 63 : 0);
        }
        uint64_t *d = nullptr;
        MOAI_HIP_CHECK(hipMalloc(&d, h.size() * 8));
        MOAI_HIP_CHECK(hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice));
        c->dec_tables[key] = d;
        base = d;
    }
    a->pw = reinterpret_cast<const Tw *>(base + lay.pw);
    a->invp = reinterpret_cast<const Tw *>(base + lay.invp);
    a->P = base + lay.P;
    a->nw = base + lay.nw;
    a->q = base + lay.q;
    a->Q = base + lay.Q;
    a->T = base + lay.T;
    a->L = (uint32_t)L;
    a->W = (uint32_t)W;
    return MOAI_OK;
}

} // namespace moai

using namespace moai;

extern "C" int moai_decrypt(moai_ctx *c, const uint64_t *ct, size_t size, const uint64_t *sk_ntt, uint64_t *out,
                            size_t n_batch, size_t L, const uint32_t *prime_index, void *stream)
{
    MOAI_AUDIT(stream, ct, sk_ntt, out);
    trace_op("decrypt", L, n_batch);
    DecryptArgs g;
    MOAI_TRY(rows_entry(c, L, prime_index, &g.rows));
    if (size < 2)
    {
        return set_error(MOAI_EINVAL, "encrypted is not valid for encryption parameters");
    }
    if (size > 0xffffu)
    {
        return set_error(MOAI_EINVAL, "ciphertext size too large");
    }
    if (n_batch == 0)
    {
        return MOAI_OK;
    }
    if (n_batch > 65535)
    {
        return set_error(MOAI_EINVAL, "at most 65535 ciphertexts per call");
    }
    if (!ct || !sk_ntt || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    MOAI_TRY(enter_device(c));
    g.ct = ct;
    g.sk = sk_ntt;
    g.out = out;
    g.pc = c->pc;
    g.size = (uint32_t)size;
    g.L = (uint32_t)L;
    g.logn = (uint32_t)c->logn;
    dim3 grid((uint32_t)((c->n + 255) / 256), (uint32_t)L, (uint32_t)n_batch);
    hipLaunchKernelGGL(dec_decrypt, grid, dim3(256), 0, (hipStream_t)stream, g);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

// decode_internal with sparse_slots_ = out_slots (N/2: the full-slot decode); the caller has validated out_slots
static int ckks_decode_impl(moai_ctx *c, const uint64_t *plain_ntt, size_t n_batch, size_t L, const uint32_t *prime_index,
                            const double *scales, size_t out_slots, int is_complex, double *out, void *stream)
{
    RowMap rows;
    MOAI_TRY(rows_entry(c, L, prime_index, &rows));
    if (c->logn < 3 || c->logn > DEC_TILE_LOG + 4)
    {
        return set_error(MOAI_ELOGIC, "decoder supports 8 <= N <= 2^16");
    }
    if (n_batch == 0)
    {
        return MOAI_OK;
    }
    if (!plain_ntt || !scales || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    // ckks.h:672-677 (no +1, unlike encode); a non-finite scale is out of bounds too
    const int total_bits = total_coeff_bits(c, L, prime_index);
    for (size_t b = 0; b < n_batch; b++)
    {
        const double sc = scales[b];
        if (!(sc > 0) || !std::isfinite(sc) || static_cast<int>(std::log2(sc)) >= total_bits)
        {
            return set_error(MOAI_EINVAL, "scale out of bounds");
        }
    }
    MOAI_TRY(enter_device(c));
    MOAI_TRY(ensure_ckks_tables(c));
    ComposeArgs a;
    MOAI_TRY(dec_table(c, rows, L, &a));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> op(*static_cast<std::mutex *>(c->op_mutex));
    // plaintexts per chunk: the scratch of one is its L rows plus N complex doubles; the budget is the stream's arena when that
    // is larger (moai_ctx_reserve), else MOAI_DEC_TMP_MB (default 1024 MiB)
    const size_t n = c->n, per = n * (L * sizeof(uint64_t) + sizeof(double2));
    const size_t cb = chunk_items(c, s, per, n_batch, 65535, (size_t)std::max(1l, tuning(K_DEC_TMP_MB)) << 20);
    void *scratch = nullptr;
    MOAI_TRY(workspace(c, cb * per, s, &scratch));
    uint64_t *rows_tmp = static_cast<uint64_t *>(scratch);
    double2 *vals = reinterpret_cast<double2 *>(rows_tmp + cb * L * n);
    a.logn = (uint32_t)c->logn;
    a.zero_mask = (uint32_t)((n >> 1) / out_slots - 1); // sparsity - 1 (ckks.h:705)
    int NW = 1; // the words of Q rounded up to a power of two
    while (NW < (int)a.W)
    {
        NW <<= 1;
    }
    const uint32_t logn = (uint32_t)c->logn;
    const int R = logn > (uint32_t)DEC_TILE_LOG ? (int)logn - DEC_TILE_LOG : 0;
    const uint32_t tile = n < DEC_TILE ? (uint32_t)n : DEC_TILE;
    const size_t slots = out_slots;
    return for_chunks(n_batch, cb, [&](size_t b0, size_t nb) {
        // SEAL copies the plaintext before inverse_ntt_negacyclic_harvey (ckks.h:689-697)
        MOAI_TRY(ntt_launch(c, rows_tmp, nb, L, rows, true, s, plain_ntt + b0 * L * n, L, 0));
        MOAI_TRY(for_chunks(nb, DEC_SCALES, [&](size_t g0, size_t gn) {
            a.in = rows_tmp + g0 * L * n;
            a.out = vals + g0 * n;
            for (size_t j = 0; j < gn; j++)
            {
                a.inv_scale[j] = double(1.0) / scales[b0 + g0 + j];
            }
            dim3 grid((uint32_t)((n + 255) / 256), (uint32_t)gn);
            return dispatch<1, 2, 4, 8, 16, 32, 64>("composition words ", NW, [&](auto nw) {
                hipLaunchKernelGGL(dec_compose<decltype(nw)::value>, grid, dim3(256), 0, s, a);
                MOAI_LAUNCH_CHECK();
                return MOAI_OK;
            });
        }));
        const double2 *roots = reinterpret_cast<const double2 *>(c->ckks_roots);
        if (R > 0)
        {
            MOAI_TRY((dispatch<1, 2, 3, 4>("decoder head stages ", R, [&](auto r) {
                hipLaunchKernelGGL(dec_fft_head<decltype(r)::value>, dim3(DEC_TILE / 256, (uint32_t)nb), dim3(256), 0, s, vals, roots, logn);
                MOAI_LAUNCH_CHECK();
                return MOAI_OK;
            })));
        }
        TailArgs t;
        t.data = vals;
        t.roots = roots;
        t.src = c->ckks_src_map;
        t.out = out + b0 * slots * (is_complex ? 2 : 1);
        t.logn = logn;
        t.out_slots = (uint32_t)out_slots;
        t.first_stage = (uint32_t)R;
        t.is_complex = is_complex ? 1u : 0u;
        hipLaunchKernelGGL(dec_fft_tail, dim3((uint32_t)(nb * (n / tile))), dim3(256), 0, s, t);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    });
}

extern "C" int moai_ckks_decode(moai_ctx *c, const uint64_t *plain_ntt, size_t n_batch, size_t L,
                                const uint32_t *prime_index, const double *scales, int is_complex, double *out,
                                void *stream)
{
    MOAI_AUDIT(stream, plain_ntt, out);
    trace_op("ckks_decode", L, n_batch);
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    return ckks_decode_impl(c, plain_ntt, n_batch, L, prime_index, scales, c->n >> 1, is_complex, out, stream);
}

extern "C" int moai_ckks_decode_sparse(moai_ctx *c, const uint64_t *plain_ntt, size_t n_batch, size_t L,
                                       const uint32_t *prime_index, const double *scales, size_t sparse_slots,
                                       int is_complex, double *out, void *stream)
{
    MOAI_AUDIT(stream, plain_ntt, out);
    trace_op("ckks_decode_sparse", L, n_batch);
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (sparse_slots == 0 || sparse_slots > (c->n >> 1) || (sparse_slots & (sparse_slots - 1)) != 0)
    {
        return set_error(MOAI_EINVAL, "sparse_slots must be a power of two in [1, N/2]");
    }
    return ckks_decode_impl(c, plain_ntt, n_batch, L, prime_index, scales, sparse_slots, is_complex, out, stream);
}
