// ntt.hip -- launchers of the negacyclic NTT kernels (C ABI: moai_ntt_forward / moai_ntt_inverse).
#include <mutex>

#include "ntt_kernels.hip.h"
#include "launch.h"

namespace moai {

// 36 q < 2^64: forward butterflies may skip the per-stage guard (modarith.hip.h ct_bfly_noguard)
bool noguard_ok(uint64_t q)
{
    return q < (~0ull) / 36;
}

int ntt_mode(const moai_ctx *c, uint32_t prime, bool allow_fp)
{
    const int m = (int)c->pc_host[prime].fp_mode;
    if (allow_fp && m && tuning(K_NTT_FP))
    {
        return m;
    }
    return noguard_ok(c->primes[prime]) ? M_NOGUARD : M_GUARD;
}

TwPair twiddles(const moai_ctx *c, int mode, bool inverse)
{
    if (mode_fp(mode))
    {
        return inverse ? TwPair{ c->inv_twf, c->inv_twfb } : TwPair{ c->fwd_twf, c->fwd_twfb };
    }
    return inverse ? TwPair{ c->inv_tw, c->inv_twb } : TwPair{ c->fwd_tw, c->fwd_twb };
}

// integer primes below 2^60 take the butterflies with the approximate Shoup quotient (M_LAZY8), the others the exact
// ones; same residues either way (modarith.hip.h)
static bool lazy8_ok(const moai_ctx *c, uint32_t prime)
{
    return tuning(K_NTT_LAZY8) && c->primes[prime] < (1ull << 60);
}
// the same rows keep values below 16q and guard only where the bound needs it (M_LAZY16) unless MOAI_NTT_LAZY16=0
static bool lazy16_ok(const moai_ctx *c, uint32_t prime)
{
    return lazy8_ok(c, prime) && tuning(K_NTT_LAZY16);
}

// The plain transform has no M_GUARD kernels: ntt_mode's integer primes with guards take M_LAZY16 (or M_LAZY8) below 2^60, else
// the guard of every second stage (M_GUARD2).
int fwd_class(const moai_ctx *c, uint32_t prime)
{
    const int m = ntt_mode(c, prime);
    if (m != M_GUARD)
    {
        return m;
    }
    return lazy16_ok(c, prime) ? M_LAZY16 : (lazy8_ok(c, prime) ? M_LAZY8 : M_GUARD2);
}

// inverse: FP64 below 2^51 like the forward transform, the approximate Shoup quotient below 2^60 (the inverse has no butterflies
// without guards, so ntt_mode's M_NOGUARD rows take it too), else the exact integer butterflies (M_GUARD)
int inv_class(const moai_ctx *c, uint32_t prime)
{
    const int m = ntt_mode(c, prime);
    if (mode_fp(m))
    {
        return m;
    }
    return lazy16_ok(c, prime) ? M_LAZY16 : (lazy8_ok(c, prime) ? M_LAZY8 : M_GUARD);
}

NttArgs ntt_args(const moai_ctx *c, uint64_t *data, size_t n_poly, size_t L, const RowMap &rows, bool inverse)
{
    NttArgs a;
    const TwPair t = twiddles(c, M_GUARD, inverse);
    a.data = data;
    a.tw = t.tw;
    a.twb = t.twb;
    a.pc = c->pc;
    a.rows = rows;
    for (size_t r = 0; r < MOAI_MAX_RNS; ++r)
    {
        a.sel.idx[r] = (uint32_t)(r < L ? r : 0);
        a.selp.idx[r] = rows.idx[r < L ? r : 0];
    }
    a.Lsel = (uint32_t)L;
    a.L = (uint32_t)L;
    a.n_poly = (uint32_t)n_poly;
    a.total_work = 0;
    a.src = nullptr;
    a.src_stride = a.src_off = 0;
    a.lds_twiddles = tuning(K_NTT_LDSTW) ? 1u : 0u;
    return a;
}

// the single contiguous pass of one class
template <int LOGN, int MODE, bool INV>
static void launch_contig_single(const NttArgs &a, hipStream_t s)
{
    if constexpr (INV)
    {
        hipLaunchKernelGGL((ntt_inv_contig<LOGN, MODE>), dim3(a.total_work), dim3(256), 0, s, a);
    }
    else if constexpr (MODE == M_LAZY16)
    {
        // where the first four stages' twiddles come from is compiled into this mode's contiguous pass
        if (a.lds_twiddles)
        {
            hipLaunchKernelGGL((ntt_fwd_contig<LOGN, MODE, 1>), dim3(a.total_work), dim3(256), 0, s, a);
        }
        else
        {
            hipLaunchKernelGGL((ntt_fwd_contig<LOGN, MODE, 0>), dim3(a.total_work), dim3(256), 0, s, a);
        }
    }
    else
    {
        hipLaunchKernelGGL((ntt_fwd_contig<LOGN, MODE>), dim3(a.total_work), dim3(256), 0, s, a);
    }
}

// The contiguous pass of one class.  pair (MOAI_NTT_PAIR) and a mode that has the paired kernels: one workgroup per tile of two
// polynomials, which fetches the tile's twiddles once (ntt_kernels.hip.h fwd_contig_tile2); the last polynomial of an odd
// count, or the only one, goes to the single kernel in a launch of its own.
template <int LOGN, int MODE, bool INV>
static void launch_contig(const NttArgs &a, bool pair, hipStream_t s)
{
    if constexpr (contig_pair_mode(MODE))
    {
        // (the forward paired kernel takes its first stages' twiddles through LDS: MOAI_NTT_LDSTW=0 keeps the single kernels)
        if (pair && a.n_poly >= 2 && (INV || a.lds_twiddles))
        {
            constexpr uint32_t TPR = 1u << (LOGN - 12);
            NttArgs p = a;
            p.n_poly = a.n_poly & ~1u;
            p.total_work = (p.n_poly >> 1) * a.Lsel * TPR;
            if constexpr (INV)
            {
                hipLaunchKernelGGL((ntt_inv_contig2<LOGN, MODE>), dim3(p.total_work), dim3(256), 0, s, p);
            }
            else
            {
                hipLaunchKernelGGL((ntt_fwd_contig2<LOGN, MODE>), dim3(p.total_work), dim3(256), 0, s, p);
            }
            if (a.n_poly & 1u)
            {
                NttArgs r = a;
                r.data = a.data + (((size_t)p.n_poly * a.L) << LOGN);
                if (a.src)
                {
                    r.src = a.src + (((size_t)p.n_poly * a.src_stride) << LOGN);
                }
                r.n_poly = 1;
                r.total_work = a.Lsel * TPR;
                launch_contig_single<LOGN, MODE, INV>(r, s);
            }
            return;
        }
    }
    launch_contig_single<LOGN, MODE, INV>(a, s);
}

// the forward pair of launches of one class; `a` selects its rows and carries its tables and grid size
template <int LOGN, int MODE>
static void launch_fwd_mode(const NttArgs &a, bool pair, hipStream_t s)
{
    // (the software-pipelined strided pass of the key switch, fwd_strided_tiles, does not pay here: measured in round 3 on 256 x 2
    // polynomials, 11.25 against 11.37 ms with the bench's 60-bit primes and 7.77 against 7.40 ms -- slower -- with MOAI's FP64
    // rows.  An in-place transform reads as much as it writes and has no cached operand; five resident workgroups of one tile
    // each keep more of that traffic in flight than four pipelined ones.)
    hipLaunchKernelGGL((ntt_fwd_strided<LOGN, MODE>), dim3(a.total_work), dim3(256), 0, s, a);
    launch_contig<LOGN, MODE, false>(a, pair, s);
}

// a.sel / a.selp / a.Lsel = the rows of `a` (and their primes) whose class -- fwd_class or inv_class -- is `mode`
static void select_class(const moai_ctx *c, int (*row_class)(const moai_ctx *, uint32_t), int mode, NttArgs &a)
{
    a.Lsel = 0;
    for (uint32_t r = 0; r < a.L; ++r)
    {
        const uint32_t prime = a.rows.idx[r];
        if (row_class(c, prime) == mode)
        {
            a.selp.idx[a.Lsel] = prime;
            a.sel.idx[a.Lsel++] = r;
        }
    }
}

// The rows are split by the arithmetic their prime allows and every class that has rows gets its own pair of launches, in the
// order of MODES, with the tables of its mode.
template <int LOGN, bool INV, int... MODES>
static int launch_classes(const moai_ctx *c, const NttArgs &base, hipStream_t s)
{
    for (int mode : { MODES... })
    {
        NttArgs a = base;
        select_class(c, INV ? inv_class : fwd_class, mode, a);
        if (a.Lsel == 0)
        {
            continue;
        }
        const TwPair t = twiddles(c, mode, INV);
        a.tw = t.tw;
        a.twb = t.twb;
        a.total_work = a.n_poly * a.Lsel * (1u << (LOGN - 12));
        const bool pair = tuning(K_NTT_PAIR) != 0;
        MOAI_TRY((dispatch<MODES...>(INV ? "inverse transform mode " : "forward transform mode ", mode, [&](auto MD) {
            constexpr int MODE = decltype(MD)::value;
            if constexpr (INV)
            {
                launch_contig<LOGN, MODE, true>(a, pair, s);
                hipLaunchKernelGGL((ntt_inv_strided<LOGN, MODE>), dim3(a.total_work), dim3(256), 0, s, a);
            }
            else
            {
                launch_fwd_mode<LOGN, MODE>(a, pair, s);
            }
            return MOAI_OK;
        })));
    }
    return MOAI_OK;
}

// forward transform: the classes of fwd_class
template <int LOGN>
static int launch_fwd(const moai_ctx *c, const NttArgs &base, hipStream_t s)
{
    return launch_classes<LOGN, false, M_LAZY16, M_LAZY8, M_GUARD2, M_NOGUARD, M_FPN, M_FPR>(c, base, s);
}

// inverse transform, the classes of inv_class: rows of primes below 2^51 run in exact FP64 arithmetic like the forward transform
// (M_FPN / M_FPR, modarith.hip.h gs_bfly_fp; MOAI_NTT_FP=0 keeps them on the integer units), rows of primes below 2^60 take the
// integer butterflies with the approximate Shoup quotient (M_LAZY16, or M_LAZY8), the others the exact ones (M_GUARD); same residues
template <int LOGN>
static int launch_inv(const moai_ctx *c, const NttArgs &base, hipStream_t s)
{
    return launch_classes<LOGN, true, M_GUARD, M_LAZY8, M_FPN, M_FPR, M_LAZY16>(c, base, s);
}

size_t ntt_pipe_plan(size_t n_poly, size_t L, size_t n, size_t chunk_bytes, long k, long min_chunks, size_t *chunk_polys, int *streams)
{
    size_t chunk = n_poly, per_stream = 0;
    int nk = 0;
    if (n_poly && L && n && chunk_bytes)
    {
        // (a polynomial too large for size_t is larger than any chunk)
        const size_t poly_bytes = L > (~(size_t)0) / sizeof(uint64_t) / n ? ~(size_t)0 : L * n * sizeof(uint64_t);
        chunk = chunk_bytes / poly_bytes;
        chunk = chunk < 1 ? 1 : (chunk > n_poly ? n_poly : chunk);
    }
    const size_t chunks = chunk ? (n_poly + chunk - 1) / chunk : 0;
    if (k >= 1 && chunks >= 2)
    {
        nk = k > NTT_PIPE_MAX ? NTT_PIPE_MAX : (int)k;
        nk = (size_t)nk > chunks ? (int)chunks : nk;
        per_stream = (chunks + (size_t)nk - 1) / (size_t)nk;
        if (min_chunks > 0 && per_stream < (size_t)min_chunks)
        {
            // the fork and the join cost a small batch more than the overlap gives back (profiles/ntt_pipe_sweep.txt)
            nk = 0;
            per_stream = 0;
        }
    }
    if (chunk_polys)
    {
        *chunk_polys = chunk;
    }
    if (streams)
    {
        *streams = nk;
    }
    return per_stream;
}

// data [n_poly][L][N]; rows maps row -> prime.  Returns a MOAI_* code.
int ntt_launch(moai_ctx *c, uint64_t *data, size_t n_poly, size_t L, const RowMap &rows, bool inverse, hipStream_t s,
               const uint64_t *src, size_t src_stride_rows, size_t src_off_rows, bool entry)
{
    if (n_poly == 0 || L == 0)
    {
        return MOAI_OK;
    }
    if (src && !inverse)
    {
        return set_error(MOAI_ELOGIC, "only the inverse transform reads from another buffer");
    }
    if (src && (src_stride_rows > 0xffffffffull || src_off_rows > 0xffffffffull || src_off_rows + L > src_stride_rows))
    {
        return set_error(MOAI_EINVAL, "source slice outside its layout");
    }
    if (n_poly * L * (c->n >> (c->logn >= 12 ? 12 : 0)) > 0x7fffffffull || n_poly > 0xffffffffull)
    {
        return set_error(MOAI_EINVAL, "batch too large for one launch");
    }
    NttArgs a = ntt_args(c, data, n_poly, L, rows, inverse);
    const int logn = c->logn;
    const bool naive = tuning(K_NTT_NAIVE) != 0;
    if (src)
    {
        if (naive || logn <= 11)
        {
            // the paths that transform in place: bring the slice over first
            const size_t row_bytes = c->n * sizeof(uint64_t);
            MOAI_HIP_CHECK(hipMemcpy2DAsync(data, L * row_bytes, src + src_off_rows * c->n, src_stride_rows * row_bytes, L * row_bytes, n_poly,
                                            hipMemcpyDeviceToDevice, s));
        }
        else
        {
            a.src = src;
            a.src_stride = (uint32_t)src_stride_rows;
            a.src_off = (uint32_t)src_off_rows;
        }
    }
    if (naive && logn >= 1)
    {
        const dim3 grid = row_grid(c, n_poly * L);
        if (!inverse)
        {
            for (int st = 0; st < logn; ++st)
            {
                hipLaunchKernelGGL(ntt_stage_global<false>, grid, dim3(256), 0, s, a, logn, st, st == logn - 1);
            }
        }
        else
        {
            for (int st = logn - 1; st >= 0; --st)
            {
                hipLaunchKernelGGL(ntt_stage_global<true>, grid, dim3(256), 0, s, a, logn, st, st == 0);
            }
        }
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    }
    if (logn <= 11)
    {
        dim3 grid((uint32_t)(n_poly * L));
        if (inverse)
        {
            hipLaunchKernelGGL(ntt_small<true>, grid, dim3(256), 0, s, a, logn);
        }
        else
        {
            hipLaunchKernelGGL(ntt_small<false>, grid, dim3(256), 0, s, a, logn);
        }
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    }
    // The two passes of one transform exchange the whole polynomial through memory.  Launched per chunk of polynomials
    // (MOAI_NTT_CHUNK_MB [+ _KB], 0 = one chunk), the second pass can read from the 256 MiB Infinity Cache what the first one just
    // wrote.  On one stream that gains nothing: every launch of a chunk ends in a tail that leaves the chip part empty, and the
    // round-2 sweep broke even down to 88 MiB and lost below (profiles/r02_g_ntt_subbatch_experiment.txt).  MOAI_NTT_PIPE = K
    // deals the chunks round-robin to K side streams instead: stream order keeps a chunk's second pass behind its first, chunks
    // are independent, so chunk i's second pass runs beside chunk i+1's first and fills its tail (profiles/ntt_pipe_sweep.txt).
    // The caller's stream forks to the side streams through one event and joins them through one event each.
    size_t chunk = n_poly;
    int nk = 0;
    const long chunk_mb = tuning(K_NTT_CHUNK_MB), chunk_kb = tuning(K_NTT_CHUNK_KB);
    const size_t chunk_bytes = ((size_t)(chunk_mb > 0 ? chunk_mb : 0) << 20) + ((size_t)(chunk_kb > 0 ? chunk_kb : 0) << 10);
    const long want = tuning(K_NTT_PIPE);
    ntt_pipe_plan(n_poly, L, c->n, chunk_bytes, want > 0 && (entry || tuning(K_NTT_PIPE_INNER)) ? want : 0, tuning(K_NTT_PIPE_MIN), &chunk,
                  &nk);
    moai_ctx::NttPipe *pipe = nullptr;
    if (nk > 0)
    {
        // a capture must not acquire parallel branches: a capturing stream keeps the single-stream loop
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess)
        {
            (void)hipGetLastError();
        }
        else if (cap == hipStreamCaptureStatusNone)
        {
            pipe = ntt_pipe(c, s);
        }
    }
    std::unique_lock<std::mutex> pipe_lock;
    if (want > 0 && !pipe)
    {
        // the chunks are there for the side streams: a call that takes none (the library's own transforms, a capture, a small
        // batch) is one pair of launches.  MOAI_NTT_PIPE=0 keeps the chunk loop on the caller's stream.
        chunk = n_poly;
    }
    if (pipe)
    {
        pipe_lock = std::unique_lock<std::mutex>(*static_cast<std::mutex *>(pipe->mu));
        MOAI_HIP_CHECK(hipEventRecord(pipe->fork, s));
        for (int i = 0; i < nk; ++i)
        {
            MOAI_HIP_CHECK(hipStreamWaitEvent(pipe->side[i], pipe->fork, 0));
        }
    }
    int rc = MOAI_OK;
    size_t ci = 0;
    for (size_t p0 = 0; p0 < n_poly && rc == MOAI_OK; p0 += chunk, ++ci)
    {
        const hipStream_t cs = pipe ? pipe->side[ci % (size_t)nk] : s;
        a.data = data + p0 * L * c->n;
        if (a.src)
        {
            a.src = src + p0 * src_stride_rows * c->n;
        }
        a.n_poly = (uint32_t)(n_poly - p0 < chunk ? n_poly - p0 : chunk);
        rc = dispatch_logn(logn, [&](auto LG) {
            return inverse ? launch_inv<decltype(LG)::value>(c, a, cs) : launch_fwd<decltype(LG)::value>(c, a, cs);
        });
    }
    if (pipe)
    {
        // (also after an error: the caller's stream never leaves a side stream behind)
        for (int i = 0; i < nk; ++i)
        {
            MOAI_HIP_CHECK(hipEventRecord(pipe->join[i], pipe->side[i]));
            MOAI_HIP_CHECK(hipStreamWaitEvent(s, pipe->join[i], 0));
        }
    }
    MOAI_TRY(rc);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

int make_rowmap(const moai_ctx *c, size_t L, const uint32_t *prime_index, RowMap *out)
{
    if (L > MOAI_MAX_RNS)
    {
        return set_error(MOAI_EINVAL, "L = %zu exceeds MOAI_MAX_RNS", L);
    }
    for (size_t r = 0; r < L; r++)
    {
        uint32_t p = prime_index ? prime_index[r] : (uint32_t)r;
        if (p >= c->k)
        {
            return set_error(MOAI_ERANGE, "prime index %u out of range (k = %zu)", p, c->k);
        }
        out->idx[r] = (uint32_t)p;
    }
    for (size_t r = L; r < MOAI_MAX_RNS; r++)
    {
        out->idx[r] = 0;
    }
    return MOAI_OK;
}

int rows_entry(const moai_ctx *c, size_t L, const uint32_t *prime_index, RowMap *out)
{
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (L == 0 || L > c->k || L > MOAI_MAX_RNS)
    {
        return set_error(MOAI_EINVAL, "invalid level");
    }
    return make_rowmap(c, L, prime_index, out);
}

} // namespace moai

using namespace moai;

static int ntt_entry(moai_ctx *c, uint64_t *data, size_t n_poly, size_t L, const uint32_t *prime_index, void *stream,
                     bool inverse)
{
    if (!c || (!data && n_poly * L))
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    RowMap rows;
    int rc = make_rowmap(c, L, prime_index, &rows);
    if (!rc)
    {
        rc = enter_device(c);
    }
    if (rc)
    {
        return rc;
    }
    return ntt_launch(c, data, n_poly, L, rows, inverse, (hipStream_t)stream, nullptr, 0, 0, true);
}

extern "C" size_t moai_ntt_pipe_plan(size_t n_poly, size_t L, size_t n, size_t chunk_bytes, long k, long min_chunks)
{
    return ntt_pipe_plan(n_poly, L, n, chunk_bytes, k, min_chunks);
}

extern "C" int moai_ntt_forward(moai_ctx *c, uint64_t *data, size_t n_poly, size_t L, const uint32_t *prime_index,
                                void *stream)
{
    MOAI_AUDIT(stream, data);
    trace_op("ntt_forward", L, n_poly);
    return ntt_entry(c, data, n_poly, L, prime_index, stream, false);
}

extern "C" int moai_ntt_inverse(moai_ctx *c, uint64_t *data, size_t n_poly, size_t L, const uint32_t *prime_index,
                                void *stream)
{
    MOAI_AUDIT(stream, data);
    trace_op("ntt_inverse", L, n_poly);
    return ntt_entry(c, data, n_poly, L, prime_index, stream, true);
}
