// ntt_kernels.hip.h -- negacyclic NTT / INTT for gfx950.
//
// What it computes is the reference's ntt_negacyclic_harvey / inverse_ntt_negacyclic_harvey
// (SEAL/util/ntt.cpp:394-475, butterflies SEAL/util/dwthandler.h:94-356): forward = Cooley-Tukey,
// natural order in, bit-reversed order out; inverse = Gentleman-Sande, bit-reversed in, natural
// out, N^-1 folded into the last stage.  How it computes it is CDNA4's: for N = 2^LOGN with
// 12 <= LOGN <= 16 the LOGN stages are split into a STRIDED pass (the first LOGN-8 stages: 256
// interleaved sub-transforms whose elements are 256 apart) and a CONTIGUOUS pass (the last 8
// stages: independent 256-point transforms on consecutive coefficients).  A 256-thread workgroup
// owns a 4096-coefficient tile (32 KiB); every thread keeps 16 coefficients in VGPRs and runs
// radix-16 (4 stages) on them, the tile is transposed once through LDS (XOR-swizzled so both
// sides are bank-conflict free), and the thread runs the remaining <= 4 stages.  Global accesses
// are 128-byte runs (strided pass) or whole-wave 1 KiB rows (contiguous pass, staged through LDS).
// One RNS prime per block column: a workgroup works under a single prime, its twiddles come from
// that prime's table, and the blockIdx -> tile map keeps the workgroups that share twiddles on
// one XCD so the table lines stay in that XCD's L2.
//
// Lazy ranges: forward keeps values in [0,4q) between stages, inverse in [0,2q), like the
// reference; the pass that finishes a transform writes canonical residues.
// (M_LAZY8: below 8q / 4q; M_LAZY16: below 16q with the guards its bound trackers ask for, modarith.hip.h.)
#pragma once
#include "modarith.hip.h"

namespace moai {

// Observed dispatch is round-robin over the 8 XCDs (blocks b and b+8 share an XCD).  Give each XCD
// a contiguous range of work ids so that neighbours in work order share an L2.  Speed only.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t total)
{
    if (total & 7u)
    {
        return b;
    }
    return (b & 7u) * (total >> 3) + (b >> 3);
}

// Workgroup barrier for data exchanged through LDS only: waits for this wave's LDS traffic, not for its
// outstanding global loads (a __syncthreads() would drain vmcnt as well and serialise the prefetch below).
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Exchange between lanes of ONE wave through LDS: a wave's LDS instructions execute in issue order, so data written by
// one lane is there for another lane of the same wave once the wave's LDS counter has drained; no s_barrier, the
// other waves of the workgroup run on.  (The asm also keeps the compiler from moving LDS accesses across it.)
__device__ __forceinline__ void lds_wave_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- LDS tile layouts ------------------------------------------------------------------------------
// contiguous pass: element e of the 4096-tile lives in 16-byte chunk (e>>1); chunks are XOR-swizzled
// within each 128-byte row so that "one row per lane" (ds_*_b128) and "one column per lane"
// (ds_*_b64) accesses are both conflict free.
__device__ __forceinline__ uint32_t phys_contig(uint32_t e)
{
    uint32_t row = e >> 4;
    uint32_t c = (e >> 1) & 7u;
    return (row << 4) | (((c ^ (row & 7u)) << 1) | (e & 1u));
}

template <int GB>
__device__ __forceinline__ uint32_t phys_strided(uint32_t e)
{
    // only the 16-column tile (LOGN = 16) needs it: odd 256-blocks are shifted by half a bank row
    if (GB == 4)
    {
        return e ^ (((e >> 8) & 1u) << 4);
    }
    return e;
}

struct NttArgs
{
    uint64_t *data;            // [n_poly][L][N]
    const Tw *tw;              // fwd or inv table, [k][N]
    const Tw *twb;             // same direction, per-thread order for the contiguous pass's last 4 stages
    const PrimeConst *pc;      // [k]
    RowMap rows;               // row r -> prime
    RowMap sel;                // the rows this launch transforms: sel.idx[0..Lsel) (rows of one arithmetic mode)
    RowMap selp;               // their primes: selp.idx[i] = rows.idx[sel.idx[i]]
    uint32_t L;
    uint32_t Lsel;
    uint32_t n_poly;
    uint32_t total_work;       // grid size
    // inverse transform only: when set, the first pass reads polynomial p's row r from src row p * src_stride + src_off + r
    // instead of from `data` (the transform of a slice of a larger layout, written into `data`, without a copy first)
    const uint64_t *src;
    uint32_t src_stride;
    uint32_t src_off;
    uint32_t lds_twiddles; // forward contiguous pass: the first four stages' twiddles through LDS (MOAI_NTT_LDSTW=0: global loads)
};

// (q, q2) arguments of a tile function under MODE, forward or inverse: the integer pair (q, 2q), its lazy form
// (2^64 - q, 2^64 - 4q), or the bit patterns of (double q, 1/q)
template <int MODE>
__device__ __forceinline__ uint64_t mode_q(const PrimeConst &pc)
{
    return mode_fp(MODE) ? pc.qd : (mode_lazy(MODE) ? pc.nq : pc.q);
}
template <int MODE>
__device__ __forceinline__ uint64_t mode_q2(const PrimeConst &pc)
{
    return mode_fp(MODE) ? pc.qinv : (mode_lazy(MODE) ? pc.n4q : pc.q2);
}
// the `cr1` argument of fwd_contig_tile, the constant of the pass's final reduction: M_NOGUARD's Barrett word, or the lazy modes'
// quotient step (ntt_finish.h), red_m in the low and red_s in the high word
template <int MODE>
__device__ __forceinline__ uint64_t mode_fin(const PrimeConst &pc)
{
    return mode_lazy(MODE) ? ((uint64_t)pc.red_s << 32) | pc.red_m : pc.cr1;
}
// the end of a lazy transform: a value below 16q to its canonical residue; nq = 2^64 - q, fin = mode_fin
__device__ __forceinline__ uint64_t lazy_final(uint64_t z, uint64_t nq, uint64_t fin)
{
    static_assert(FINAL_STEP_OUT == 2, "one conditional subtraction follows the quotient step");
    return csub_sign(final_quotient_step(z, (uint32_t)(fin >> 32), (uint32_t)fin, nq), nq);
}

// =====================================================================================================
// forward, strided pass: stages 0 .. LOGN-9
// =====================================================================================================
struct LoadIdentity
{
    __device__ __forceinline__ uint64_t operator()(uint64_t v) const
    {
        return v;
    }
};

// v mod q on load (modulo_poly_coeffs, SEAL/util/polyarithsmallmod.cpp:18-41): the key switch feeds
// digits that are canonical under another prime (SEAL/evaluator.cpp:2844-2854)
struct LoadBarrett
{
    uint64_t q, cr1;
    __device__ __forceinline__ uint64_t operator()(uint64_t v) const
    {
        return barrett64(v, q, cr1);
    }
};

// FP64 modes: any integer below 2^53 -> the double holding its balanced residue (|.| <= q/2); serves both as
// the plain load and as the "mod q_I" of the key switch
struct LoadFp
{
    uint64_t qd, qinv;
    __device__ __forceinline__ uint64_t operator()(uint64_t v) const
    {
        return d2u(fp_red(fp_from_u64(v), u2d(qd), u2d(qinv)));
    }
};

// the same for an integer known to be below 2^52 (a key-switch digit canonical under a prime below 2^52)
struct LoadFp52
{
    uint64_t qd, qinv;
    __device__ __forceinline__ uint64_t operator()(uint64_t v) const
    {
        return d2u(fp_red(fp_from_u52(v), u2d(qd), u2d(qinv)));
    }
};

// the same for integers of any size (a key-switch digit under a 52..61-bit prime): integer Barrett step first
struct LoadBarrettFp
{
    uint64_t q, cr1, qd, qinv;
    __device__ __forceinline__ uint64_t operator()(uint64_t v) const
    {
        return d2u(fp_red(fp_from_u52(barrett64(v, q, cr1)), u2d(qd), u2d(qinv))); // reduced below q < 2^51
    }
};


// the unrolled stage loops of the tiles carry the stage number in a loop variable; M_GUARD2 needs it as a constant
// (M_LAZY16 also needs LOGN: its schedule counts stages from the head of the transform)
template <int MODE, int LOGN = 0>
__device__ __forceinline__ void ct_bfly_stage(uint64_t &x, uint64_t &y, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2, int stages_left)
{
    if constexpr (MODE == M_LAZY16) // (if constexpr: the other modes pass no LOGN, and LOGN = 0 has no schedule to evaluate)
    {
        constexpr int R1 = LOGN - 8;
        constexpr Lazy16Fwd p1 = lazy16_fwd(LOGN, 0, R1, 8), p2 = lazy16_fwd(LOGN, R1, 8, lazy16_fwd_handover(LOGN));
        static_assert(p1.peak <= 16 && p2.peak <= 16, "a value of 16q or more");
        static_assert(p1.end == lazy16_fwd_handover(LOGN), "the contiguous pass starts from another bound");
        static_assert(p2.end <= FINAL_STEP_IN, "the final reduction expects values below 16q");
        constexpr uint32_t g8 = p1.g8 | p2.g8;
        const int s = LOGN - 1 - stages_left;
        if ((g8 >> s) & 1u)
        {
            ct_bfly_lazy16<true>(x, y, w, wq, q, q2);
        }
        else
        {
            ct_bfly_lazy16<false>(x, y, w, wq, q, q2);
        }
    }
    else if (MODE == M_GUARD2)
    {
        if (stages_left & 1)
        {
            ct_bfly_guard2<false>(x, y, w, wq, q, q2);
        }
        else
        {
            ct_bfly_guard2<true>(x, y, w, wq, q, q2);
        }
    }
    else
    {
        ct_bfly_t<MODE>(x, y, w, wq, q, q2);
    }
}

// the 16 values a thread takes from its tile of the input row (tile base = row + tile * G), not yet converted
// Element e = j * 256 + tid of the tile sits in column e & (G - 1) of sub-transform e >> GB, sub-transforms 256 apart.  Every caller's
// `tid` is a thread of a 256-thread workgroup, so the three fields of the index -- j, tid's sub-transform, tid's column -- share no
// bit, and the index is written as their OR.  Written as the shifts and sums of e, the compiled addresses depended on whether the
// compiler had traced `tid` back to the workgroup size at the point where it simplified this function -- one 32-bit offset off a scalar
// base per access, or a 64-bit sum per access -- and that changed with the set of kernels that shared the function.  (Telling it with
// __builtin_assume(tid < 256) picks the 64-bit sums at N = 2^14 and 2^15: 110-160 bytes more per kernel.)
template <int LOGN>
__device__ __forceinline__ void strided_load_raw(const uint64_t *__restrict__ irow, const uint32_t tid, uint64_t (&raw)[16])
{
    constexpr int GB = 12 - (LOGN - 8);
    constexpr uint32_t G = 1u << GB;
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        // N = 2^12 (GB = 8: the index is j * 256 + tid) keeps the sum: its sixteen loads then share one 64-bit address and differ in
        // their immediate offsets, sixteen offset registers fewer, which is what keeps those kernels at eight waves per SIMD
        raw[j] = irow[GB == 8 ? (uint32_t)j * 256u + tid : ((uint32_t)j << (16 - GB)) | ((tid >> GB) << 8) | (tid & (G - 1))];
    }
}

// everything after the load: the butterflies of both phases, the exchange and the stores of one tile (row = tile base of the
// output row).  SYNC_FIRST: the workgroup has used `lds` for an earlier tile -- wait until everybody has read it.  The barriers
// wait for LDS traffic only (lds_barrier), so global loads and stores of neighbouring tiles stay in flight across them.
// LDSTW: phase B takes its twiddles (entries 16..255 of the table) from the workgroup's copy in LDS, `ldstw`
template <int LOGN, int MODE, bool SYNC_FIRST, bool LDSTW = false>
__device__ __forceinline__ void strided_core(uint64_t (&x)[16], uint64_t *__restrict__ row, const Tw *__restrict__ tw, uint64_t q,
                                             uint64_t q2, uint64_t *lds, const uint32_t tid, const Tw *ldstw = nullptr)
{
    // phase A's fifteen twiddles (entries 1..15 of the table) are the same for every thread: read through the constant address
    // space, so that they stay SCALAR loads also inside a loop over tiles -- behind the stores of an earlier iteration the compiler
    // turns a uniform global load into a vector load (it cannot see that no kernel ever writes the tables), and the wait for a
    // vector load also waits for the prefetch of the next tile issued before it
    typedef const Tw __attribute__((address_space(4))) *TwConst;
    const TwConst twa = (TwConst)(uintptr_t)tw;
    constexpr int R1 = LOGN - 8;
    constexpr int RB = R1 - 4;
    constexpr int GB = 12 - R1;
    constexpr uint32_t G = 1u << GB;
    // phase A: top four bits of t live in the register index
#pragma unroll
    for (int u = 0; u < 4; ++u)
    {
        const int half = 8 >> u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            if (!(j & half))
            {
                const uint32_t ti = (1u << u) + (uint32_t)(j >> (4 - u));
                ct_bfly_stage<MODE, LOGN>(x[j], x[j + half], twa[ti].w, twa[ti].wq, q, q2, LOGN - 1 - u);
            }
        }
    }
    if (RB > 0)
    {
        if (SYNC_FIRST)
        {
            lds_barrier();
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            lds[phys_strided<GB>((uint32_t)j * 256u + tid)] = x[j];
        }
        lds_barrier();
        const uint32_t g = tid & (G - 1);
        const uint32_t th = tid >> GB;
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            x[j] = lds[phys_strided<GB>((th << (GB + 4)) | ((uint32_t)j << GB) | g)];
        }
        // phase B: low RB bits of t
#pragma unroll
        for (int s = 4; s < R1; ++s)
        {
            const int half = 1 << (R1 - 1 - s);
#pragma unroll
            for (int j = 0; j < 16; ++j)
            {
                if (!(j & half))
                {
                    uint32_t t_ = (th << 4) | (uint32_t)j;
                    Tw t = LDSTW ? ldstw[(1u << s) + (t_ >> (R1 - s))] : tw[(1u << s) + (t_ >> (R1 - s))];
                    ct_bfly_stage<MODE, LOGN>(x[j], x[j + half], t.w, t.wq, q, q2, LOGN - 1 - s);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            uint32_t t_ = (th << 4) | (uint32_t)j;
            row[(t_ << 8) | g] = x[j]; // (non-temporal stores measured the same: 2080 against 2092 us in the key switch's pass)
        }
    }
    else
    {
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            uint32_t e = (uint32_t)j * 256u + tid;
            row[((e >> GB) << 8) + (e & (G - 1))] = x[j];
        }
    }
}

// one tile of the strided pass: reads row `inp`, writes row `rowp` (may be the same row)
// LDSTW (N = 2^16, `lds` with 512 more words): phase B's twiddles -- entries 16..255 of the table, the same for every tile -- are
// copied into LDS, one 16-byte load per thread issued with the tile's own loads, and read from there behind the exchange
template <int LOGN, class LoadOp, int MODE, bool LDSTW = false>
__device__ __forceinline__ void fwd_strided_tile(const uint64_t *__restrict__ inp, uint64_t *__restrict__ rowp, uint32_t tile,
                                                 const Tw *__restrict__ tw, uint64_t q, uint64_t q2, uint64_t *lds,
                                                 const uint32_t tid, LoadOp op = LoadOp())
{
    constexpr uint32_t G = 1u << (12 - (LOGN - 8));
    static_assert(!LDSTW || LOGN == 16, "the LDS copy holds the 256 entries phase B of N = 2^16 indexes");
    Tw *ldstw = reinterpret_cast<Tw *>(lds + 4096);
    uint64_t x[16];
    strided_load_raw<LOGN>(inp + tile * G, tid, x);
    if (LDSTW)
    {
        ldstw[tid] = tw[tid]; // visible to the workgroup behind the exchange's barrier
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        x[j] = op(x[j]);
    }
    strided_core<LOGN, MODE, false, LDSTW>(x, rowp + tile * G, tw, q, q2, lds, tid, LDSTW ? ldstw : nullptr);
}

// ITEMS consecutive tiles of one row by one workgroup, software-pipelined: the loads of tile i + 1 are issued before the
// butterflies of tile i, and the stores of tile i drain under the butterflies of tile i + 1.  A workgroup that loads, computes and
// stores ONE tile keeps the memory system busy only through its neighbours on the CU, and 32 KiB of LDS plus ~96 VGPRs allow four
// or five of them: measured on the key switch's strided pass (round 3), 2.37 ms per launch against 1.96 ms for its
// memory traffic alone and 1.62 ms for its arithmetic alone -- the two did not overlap.
template <int LOGN, class LoadOp, int MODE, int ITEMS>
__device__ __forceinline__ void fwd_strided_tiles(const uint64_t *inp, uint64_t *rowp, uint32_t tile0,
                                                  const Tw *__restrict__ tw, uint64_t q, uint64_t q2, uint64_t *lds, const uint32_t tid,
                                                  LoadOp op)
{
    constexpr uint32_t G = 1u << (12 - (LOGN - 8));
    static_assert(LOGN == 16, "the LDS copy holds the 256 entries phase B of N = 2^16 indexes");
    uint64_t raw[16], x[16];
    strided_load_raw<LOGN>(inp + tile0 * G, tid, raw);
    // phase B's twiddles into LDS (`lds` + 4096 words: 256 entries of 16 bytes, one per thread; entries 16..255 are used).
    // Fetched from memory inside the loop, every wait for one of them would also wait for the stores of the previous tile
    // and for the prefetch of the next one: vector memory operations complete in order.
    Tw *ldstw = reinterpret_cast<Tw *>(lds + 4096);
    ldstw[tid] = tw[tid];
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        x[j] = op(raw[j]);
    }
    // one loop body (not unrolled: four copies of it would not fit the instruction cache).  The first tile's values are converted
    // before the loop, so the body starts from arithmetic results and not from pending loads: entered that way, its first wait
    // would also cover the loads it has just issued.
#pragma unroll 1
    for (uint32_t it = 0; it < (uint32_t)ITEMS; ++it)
    {
        // opaque copy of the thread index: the per-thread addresses (16 loads, 16 stores, 32 LDS slots, the twiddles) are
        // recomputed in every iteration instead of hoisted out of the loop into registers the prefetch needs
        uint32_t t = tid;
        asm volatile("" : "+v"(t));
        const bool more = it + 1u < (uint32_t)ITEMS;
        if (more)
        {
            strided_load_raw<LOGN>(inp + (tile0 + it + 1u) * G, t, raw);
        }
        strided_core<LOGN, MODE, true, true>(x, rowp + (tile0 + it) * G, tw, q, q2, lds, t, ldstw);
        if (more)
        {
#pragma unroll
            for (int j = 0; j < 16; ++j)
            {
                x[j] = op(raw[j]);
            }
        }
    }
}

// five waves per SIMD (96 VGPRs) where the body fits; the modes whose body does not (12, 8 and 14 spilled registers
// under that cap) run faster at four: M_GUARD2 12.17 -> 11.90 ms per batch transform, FP64 / unguarded rows 2-3 %
constexpr bool fwd_strided_occ4(int mode)
{
    return mode == M_GUARD2 || mode_lazy(mode) || mode == M_FPR || mode == M_NOGUARD;
}
template <int LOGN, int MODE>
__global__ __launch_bounds__(256, fwd_strided_occ4(MODE) ? 4 : 5) void ntt_fwd_strided(NttArgs a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    // the modes that run four workgroups per CU anyway take phase B's twiddles through LDS at N = 2^16 (4 KiB more)
    constexpr bool LDSTW = LOGN == 16 && fwd_strided_occ4(MODE);
    __shared__ uint64_t lds[4096 + (LDSTW ? 512 : 0)];
    const uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t tile = w % TPR;
    const uint32_t srow = w / TPR;                 // over n_poly * Lsel selected rows
    const uint32_t si = srow % a.Lsel;
    // 16-bit kernarg entries arrive through a vector load: pin them back to scalars, or every address and
    // modulus derived from them lives in VGPRs
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.sel.idx[si]);
    const uint32_t prime = __builtin_amdgcn_readfirstlane(a.selp.idx[si]);
    const PrimeConst &pc = a.pc[prime];
    uint64_t *rowp = a.data + ((size_t)((srow / a.Lsel) * a.L + r) << LOGN);
    const uint64_t q = mode_q<MODE>(pc), q2 = mode_q2<MODE>(pc);
    if (mode_fp(MODE))
    {
        LoadFp op;
        op.qd = pc.qd;
        op.qinv = pc.qinv;
        fwd_strided_tile<LOGN, LoadFp, MODE, LDSTW>(rowp, rowp, tile, a.tw + ((size_t)prime << LOGN), q, q2, lds, threadIdx.x, op);
    }
    else
    {
        fwd_strided_tile<LOGN, LoadIdentity, MODE, LDSTW>(rowp, rowp, tile, a.tw + ((size_t)prime << LOGN), q, q2, lds, threadIdx.x);
    }
}

// =====================================================================================================
// forward, contiguous pass: stages LOGN-8 .. LOGN-1 on 16 consecutive 256-blocks; writes canonical
// =====================================================================================================
// what the contiguous pass does with a finished 16-byte chunk (index ch within the 4096-coefficient tile)
// fetch(chs) is called with four chunk indices before the four calls that finish them: a store operation that needs operands
// from memory issues all its loads there, in one batch, instead of one round trip per chunk and operand
struct StoreTile
{
    ulonglong2 *out; // tile base
    __device__ __forceinline__ void fetch(const uint32_t (&)[4])
    {
    }
    __device__ __forceinline__ void operator()(int, uint32_t ch, ulonglong2 v) const
    {
        out[ch] = v;
    }
};

// M_NOGUARD: input below 20q (strided pass without guards), stages without guards, one Barrett step at
// the end (cr1 = high word of floor(2^128/q)); M_GUARD: the reference's [0,4q) discipline; FP64 modes: doubles
// in, canonical integers out (q, q2 carry the bit patterns of (double q, 1/q))
// ldstw (or null): 240 entries of LDS beside lds2 for the twiddles of the first four stages -- fifteen per 256-block, shared by the
// block's sixteen threads.  Every wave fetches the sixty of its own four blocks with ONE load per lane and reads them back from LDS
// (broadcast reads, no s_barrier: the blocks of a wave are its own), instead of fifteen 16-byte global loads per thread issued one
// or two ahead of the butterflies that use them.
// TWL: -1 = `ldstw` decides at run time (the reads are then generic loads: every wait for one drains LDS and memory alike);
// 0 = memory; 1 = LDS, known at compile time: the reads are ds_read_b128, and the copy's load is issued with the tile's own
// sixteen and waited for only where it is written to LDS, instead of costing one round trip in front of every tile.
template <int LOGN, int MODE, class StoreOp, int TWL = -1>
__device__ __forceinline__ void fwd_contig_tile(uint64_t *__restrict__ rowp, uint32_t tile, const Tw *__restrict__ tw,
                                                uint64_t q, uint64_t q2, ulonglong2 *lds2, const uint32_t tid,
                                                const Tw *__restrict__ twb, uint64_t cr1, StoreOp store, Tw *ldstw = nullptr)
{
    constexpr int R1 = LOGN - 8;
    uint64_t *lds = reinterpret_cast<uint64_t *>(lds2);
    uint64_t *__restrict__ base = rowp + ((size_t)tile << 12);
    const uint32_t b = tid >> 4;
    const uint32_t tl = tid & 15u;
    const uint32_t blk = (tile << 4) + b;
    const Tw *__restrict__ twbt = twb + (size_t)tile * (15 * 256);

    const bool use_lds = TWL < 0 ? ldstw != nullptr : TWL == 1;
    Tw fill;
    uint32_t fill_slot = 0;
    if (use_lds)
    {
        const uint32_t lane = tid & 63u;
        if (TWL == 1)
        {
            // lanes 60..63 repeat lane 59's load, so that it is issued without a branch, and store nothing
            const uint32_t l = lane < 59u ? lane : 59u;
            const uint32_t bb = ((tid >> 6) << 2) + l / 15u, i = l % 15u;
            const uint32_t u = i == 0 ? 0u : (i < 3 ? 1u : (i < 7 ? 2u : 3u)), k = i - ((1u << u) - 1u);
            fill = tw[(1u << (R1 + u)) + (((tile << 4) + bb) << u) + k];
            fill_slot = bb * 15u + i;
        }
        else if (lane < 60u)
        {
            const uint32_t bb = ((tid >> 6) << 2) + lane / 15u, i = lane % 15u;       // block of this wave, slot 2^u - 1 + k
            const uint32_t u = i == 0 ? 0u : (i < 3 ? 1u : (i < 7 ? 2u : 3u)), k = i - ((1u << u) - 1u);
            ldstw[bb * 15u + i] = tw[(1u << (R1 + u)) + (((tile << 4) + bb) << u) + k];
        }
    }
    uint64_t x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        x[j] = base[(b << 8) | ((uint32_t)j << 4) | tl];
    }
    if (use_lds)
    {
        if (TWL == 1 && (tid & 63u) < 60u)
        {
            ldstw[fill_slot] = fill;
        }
        lds_wave_sync();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
    {
        const int half = 8 >> u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            if (!(j & half))
            {
                Tw t = use_lds ? ldstw[b * 15u + ((1u << u) - 1u) + (uint32_t)(j >> (4 - u))]
                               : tw[(1u << (R1 + u)) + (blk << u) + (uint32_t)(j >> (4 - u))];
                ct_bfly_stage<MODE, LOGN>(x[j], x[j + half], t.w, t.wq, q, q2, 7 - u);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        lds[phys_contig((b << 8) | ((uint32_t)j << 4) | tl)] = x[j];
    }
    // a 256-block belongs to 16 consecutive threads, i.e. to one wave: every exchange of this pass is wave-local
    lds_wave_sync();
    const uint32_t myrow = tid; // (b << 4) | th
#pragma unroll
    for (int c = 0; c < 8; ++c)
    {
        ulonglong2 v = lds2[(myrow << 3) | ((uint32_t)c ^ (myrow & 7u))];
        x[2 * c] = v.x;
        x[2 * c + 1] = v.y;
    }
#pragma unroll
    for (int u = 4; u < 8; ++u)
    {
        const int half = 8 >> (u - 4);
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            if (!(j & half))
            {
                // slot = 2^(u-4) - 1 + (j >> (8-u)); consecutive threads read consecutive entries
                Tw t = twbt[(((1u << (u - 4)) - 1u + (uint32_t)(j >> (8 - u))) << 8) + tid];
                ct_bfly_stage<MODE, LOGN>(x[j], x[j + half], t.w, t.wq, q, q2, 7 - u);
            }
        }
    }
    // a thread overwrites the row it alone has read
#pragma unroll
    for (int c = 0; c < 8; ++c)
    {
        ulonglong2 v;
        if (mode_fp(MODE))
        {
            v.x = fp_to_canonical(u2d(x[2 * c]), u2d(q), u2d(q2));
            v.y = fp_to_canonical(u2d(x[2 * c + 1]), u2d(q), u2d(q2));
        }
        else if (MODE == M_NOGUARD)
        {
            v.x = barrett64(x[2 * c], q, cr1);
            v.y = barrett64(x[2 * c + 1], q, cr1);
        }
        else if (mode_lazy(MODE))
        {
            // values below 8q (M_LAZY8) or 12q (M_LAZY16, ct_bfly_stage); `q` carries 2^64 - q, `cr1` mode_fin.  One quotient step and one
            // conditional subtraction, 10 vector instructions, where three conditional subtractions (from 8q) take 12 -- and the
            // last stage of M_LAZY16 keeps the guard that brought its outputs below 8q for them
            v.x = lazy_final(x[2 * c], q, cr1);
            v.y = lazy_final(x[2 * c + 1], q, cr1);
        }
        else if (MODE == M_GUARD2)
        {
            // the last stage is a guarded one: values below 6q
            v.x = csub(csub(csub(x[2 * c], q2 << 1), q2), q);
            v.y = csub(csub(csub(x[2 * c + 1], q2 << 1), q2), q);
        }
        else
        {
            v.x = csub(csub(x[2 * c], q2), q);
            v.y = csub(csub(x[2 * c + 1], q2), q);
        }
        lds2[(myrow << 3) | ((uint32_t)c ^ (myrow & 7u))] = v;
    }
    lds_wave_sync();
    // every wave stores the 64 rows (8 KiB, contiguous in memory) its own lanes finished: 1 KiB per wave instruction
    const uint32_t wbase = (tid >> 6) << 9, lane = tid & 63u;
#pragma unroll
    for (int h = 0; h < 2; ++h)
    {
        uint32_t chs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            chs[i] = wbase + (uint32_t)(4 * h + i) * 64u + lane;
        }
        store.fetch(chs);
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const uint32_t rr = chs[i] >> 3;
            store(i, chs[i], lds2[(rr << 3) | ((chs[i] & 7u) ^ (rr & 7u))]);
        }
    }
}

// TWL (fwd_contig_tile): -1 = NttArgs::lds_twiddles decides at run time, 0 / 1 = compiled in (M_LAZY16)
// (36.6 KiB of LDS admit four workgroups per CU, and every mode's body fits the 128 registers that go with them; said here so that
// the allocator does not settle for 129 and three)
template <int LOGN, int MODE, int TWL = -1>
__global__ __launch_bounds__(256, 4) void ntt_fwd_contig(NttArgs a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    __shared__ ulonglong2 lds2[2048 + 240]; // the tile, and the first four stages' twiddles (fwd_contig_tile, ldstw)
    const uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t pol = w % a.n_poly;
    const uint32_t rest = w / a.n_poly;
    const uint32_t tile = rest % TPR;
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.sel.idx[rest / TPR]);
    const uint32_t prime = __builtin_amdgcn_readfirstlane(a.selp.idx[rest / TPR]);
    const PrimeConst &pc = a.pc[prime];
    uint64_t *rowp = a.data + (((size_t)pol * a.L + r) << LOGN);
    StoreTile st;
    st.out = reinterpret_cast<ulonglong2 *>(rowp + ((size_t)tile << 12));
    fwd_contig_tile<LOGN, MODE, StoreTile, TWL>(rowp, tile, a.tw + ((size_t)prime << LOGN), mode_q<MODE>(pc), mode_q2<MODE>(pc), lds2, threadIdx.x,
                                                a.twb + (size_t)prime * ((size_t)TPR * 15 * 256), mode_fin<MODE>(pc), st,
                                                (TWL < 0 ? a.lds_twiddles != 0 : TWL == 1) ? reinterpret_cast<Tw *>(lds2 + 2048) : nullptr);
}

// Orders the LDS accesses of one wave in the program without waiting for any of them: a wave's LDS instructions execute in issue
// order, so a slot that a lane reads may be overwritten by another lane of the same wave in a later instruction.
__device__ __forceinline__ void lds_wave_order()
{
    asm volatile("" ::: "memory");
}

// The fifteen twiddles of four stages on sixteen registers are slots 2^u - 1 + k, k < 2^u, of stage u.  The paired tiles fetch
// them PAIR_TW_AHEAD slots ahead of the butterflies that use them and close every butterfly pair with pair_fence: left alone the
// compiler moves all fifteen loads (60 registers) to the head of the stages, beside 64 registers of data, and spills.
// (The stage loops of the paired tiles run over the eight butterflies of a stage, not over sixteen registers of which every
// second one is skipped: with twice the body, the skipped half counted, the loops went past the size up to which they are unrolled.)
// Eight: the largest distance at which neither kernel spills (nine: 12 bytes in the inverse one), and on the bench's batch
// 18.31 ms per step against 18.58 with four (profiles/ntt_pair_parent_vs_branch.txt).
constexpr int PAIR_TW_AHEAD = 8;
// No instruction: the four values are what the program holds from here on, and no memory access moves across.
__device__ __forceinline__ void pair_fence(uint64_t &a0, uint64_t &a1, uint64_t &b0, uint64_t &b1)
{
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1)::"memory");
}
// the inverse stages run from the widest slot range down: slots 7..14, 3..6, 1..2, 0
constexpr int inv_slot_of_order(int k)
{
    return k < 8 ? 7 + k : (k < 12 ? k - 5 : (k < 14 ? k - 11 : 0));
}
constexpr int inv_order_of_slot(int s)
{
    return s >= 7 ? s - 7 : (s >= 3 ? s + 5 : (s >= 1 ? s + 11 : 14));
}
constexpr int slot_stage(int s)
{
    return s >= 7 ? 3 : (s >= 3 ? 2 : (s >= 1 ? 1 : 0));
}

// the modes whose contiguous passes exist in the paired form (fwd_contig_tile2, inv_contig_tile2)
constexpr bool contig_pair_mode(int mode)
{
    return mode == M_LAZY16;
}

// The same tile of TWO polynomials (rows rowA and rowB under one prime) by one workgroup.  The fifteen per-thread twiddles of the
// last four stages depend on (prime, tile, thread) only -- 60 KiB per 32 KiB tile of data --, so does the LDS copy of the first
// four stages' and all the index arithmetic: every twiddle is fetched once and applied to A's butterfly and to B's.  Both tiles'
// loads are issued before the first butterfly.  The exchanges are wave-local; the tiles pass through the one 32 KiB buffer one
// after the other, so LDS stays what fwd_contig_tile takes.  Plain stores (StoreTile) only; the first four stages' twiddles come
// through LDS (fwd_contig_tile's TWL = 1).
template <int LOGN, int MODE>
__device__ __forceinline__ void fwd_contig_tile2(uint64_t *__restrict__ rowA, uint64_t *__restrict__ rowB, uint32_t tile,
                                                 const Tw *__restrict__ tw, uint64_t q, uint64_t q2, ulonglong2 *lds2, const uint32_t tid,
                                                 const Tw *__restrict__ twb, uint64_t cr1, Tw *ldstw)
{
    static_assert(contig_pair_mode(MODE) && mode_lazy(MODE), "the paired pass ends in the lazy modes' final reduction");
    constexpr int R1 = LOGN - 8;
    uint64_t *lds = reinterpret_cast<uint64_t *>(lds2);
    uint64_t *__restrict__ baseA = rowA + ((size_t)tile << 12);
    uint64_t *__restrict__ baseB = rowB + ((size_t)tile << 12);
    const uint32_t b = tid >> 4;
    const uint32_t tl = tid & 15u;
    const Tw *__restrict__ twbt = twb + (size_t)tile * (15 * 256);

    Tw fill;
    uint32_t fill_slot = 0;
    {
        // as in fwd_contig_tile: lanes 60..63 repeat lane 59's load and store nothing
        const uint32_t lane = tid & 63u;
        const uint32_t l = lane < 59u ? lane : 59u;
        const uint32_t bb = ((tid >> 6) << 2) + l / 15u, i = l % 15u;
        const uint32_t u = i == 0 ? 0u : (i < 3 ? 1u : (i < 7 ? 2u : 3u)), k = i - ((1u << u) - 1u);
        fill = tw[(1u << (R1 + u)) + (((tile << 4) + bb) << u) + k];
        fill_slot = bb * 15u + i;
    }
    uint64_t xa[16], xb[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        xa[j] = baseA[(b << 8) | ((uint32_t)j << 4) | tl];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        xb[j] = baseB[(b << 8) | ((uint32_t)j << 4) | tl];
    }
    if ((tid & 63u) < 60u)
    {
        ldstw[fill_slot] = fill;
    }
    lds_wave_sync();
#pragma unroll
    for (int u = 0; u < 4; ++u)
    {
        const int half = 8 >> u;
#pragma unroll
        for (int i = 0; i < 8; ++i)
        {
            const int j = ((i & ~(half - 1)) << 1) | (i & (half - 1)); // the i-th register index without the bit `half`
            {
                Tw t = ldstw[b * 15u + ((1u << u) - 1u) + (uint32_t)(j >> (4 - u))];
                ct_bfly_stage<MODE, LOGN>(xa[j], xa[j + half], t.w, t.wq, q, q2, 7 - u);
                ct_bfly_stage<MODE, LOGN>(xb[j], xb[j + half], t.w, t.wq, q, q2, 7 - u);
            }
        }
    }
    // the per-thread twiddles of the last four stages, slot s at twbt[s * 256 + tid]: the first ones arrive under the exchange
    Tw tq[15];
#pragma unroll
    for (int s = 0; s < PAIR_TW_AHEAD; ++s)
    {
        tq[s] = twbt[((uint32_t)s << 8) + tid];
    }
    const uint32_t myrow = tid; // (b << 4) | th
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        lds[phys_contig((b << 8) | ((uint32_t)j << 4) | tl)] = xa[j];
    }
    lds_wave_sync();
#pragma unroll
    for (int c = 0; c < 8; ++c)
    {
        ulonglong2 v = lds2[(myrow << 3) | ((uint32_t)c ^ (myrow & 7u))];
        xa[2 * c] = v.x;
        xa[2 * c + 1] = v.y;
    }
    lds_wave_order(); // B's columns overwrite A's behind the reads of A's rows
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        lds[phys_contig((b << 8) | ((uint32_t)j << 4) | tl)] = xb[j];
    }
    lds_wave_sync();
#pragma unroll
    for (int c = 0; c < 8; ++c)
    {
        ulonglong2 v = lds2[(myrow << 3) | ((uint32_t)c ^ (myrow & 7u))];
        xb[2 * c] = v.x;
        xb[2 * c + 1] = v.y;
    }
#pragma unroll
    for (int u = 4; u < 8; ++u)
    {
        const int half = 8 >> (u - 4);
#pragma unroll
        for (int i = 0; i < 8; ++i)
        {
            const int j = ((i & ~(half - 1)) << 1) | (i & (half - 1)); // the i-th register index without the bit `half`
            {
                const int slot = (1 << (u - 4)) - 1 + (j >> (8 - u)); // used in ascending order
                if ((j & ((1 << (8 - u)) - 1)) == 0)
                {
                    if (slot + PAIR_TW_AHEAD < 15)
                    {
                        tq[slot + PAIR_TW_AHEAD] = twbt[((uint32_t)(slot + PAIR_TW_AHEAD) << 8) + tid];
                    }
                }
                const Tw t = tq[slot];
                ct_bfly_stage<MODE, LOGN>(xa[j], xa[j + half], t.w, t.wq, q, q2, 7 - u);
                ct_bfly_stage<MODE, LOGN>(xb[j], xb[j + half], t.w, t.wq, q, q2, 7 - u);
                pair_fence(xa[j], xa[j + half], xb[j], xb[j + half]);
            }
        }
    }
    // per tile as in fwd_contig_tile: a thread's finished row to LDS, then every wave stores its own 8 KiB, 1 KiB per instruction.
    // (An opaque copy of the thread index: the eight swizzled row slots are computed again here instead of staying in registers
    // that the 64 values and the twiddles in flight need across the four stages above.)
    uint32_t t2 = tid;
    asm volatile("" : "+v"(t2));
    const uint32_t wbase = (t2 >> 6) << 9, lane = t2 & 63u;
#pragma unroll
    for (int p = 0; p < 2; ++p)
    {
        if (p)
        {
            lds_wave_order(); // B's rows overwrite A's behind the reads of A's chunks
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
        {
            ulonglong2 v;
            v.x = lazy_final(p ? xb[2 * c] : xa[2 * c], q, cr1);
            v.y = lazy_final(p ? xb[2 * c + 1] : xa[2 * c + 1], q, cr1);
            lds2[(t2 << 3) | ((uint32_t)c ^ (t2 & 7u))] = v;
        }
        lds_wave_sync();
        ulonglong2 *out = reinterpret_cast<ulonglong2 *>(p ? baseB : baseA);
#pragma unroll
        for (int i = 0; i < 8; ++i)
        {
            const uint32_t ch = wbase + (uint32_t)i * 64u + lane;
            const uint32_t rr = ch >> 3;
            out[ch] = lds2[(rr << 3) | ((ch & 7u) ^ (rr & 7u))];
        }
    }
}

// polynomials 2p and 2p + 1 of the launch per workgroup; a.n_poly is even (the launcher gives an odd last polynomial to
// ntt_fwd_contig), a.total_work = n_poly / 2 * Lsel * TPR.  The pair index runs fastest, as the polynomial does in ntt_fwd_contig.
template <int LOGN, int MODE>
__global__ __launch_bounds__(256, 4) void ntt_fwd_contig2(NttArgs a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    __shared__ ulonglong2 lds2[2048 + 240];
    const uint32_t pairs = a.n_poly >> 1;
    const uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t pol = (w % pairs) << 1;
    const uint32_t rest = w / pairs;
    const uint32_t tile = rest % TPR;
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.sel.idx[rest / TPR]);
    const uint32_t prime = __builtin_amdgcn_readfirstlane(a.selp.idx[rest / TPR]);
    const PrimeConst &pc = a.pc[prime];
    uint64_t *rowA = a.data + (((size_t)pol * a.L + r) << LOGN);
    fwd_contig_tile2<LOGN, MODE>(rowA, rowA + ((size_t)a.L << LOGN), tile, a.tw + ((size_t)prime << LOGN), mode_q<MODE>(pc), mode_q2<MODE>(pc),
                                      lds2, threadIdx.x, a.twb + (size_t)prime * ((size_t)TPR * 15 * 256), mode_fin<MODE>(pc),
                                      reinterpret_cast<Tw *>(lds2 + 2048));
}

// =====================================================================================================
// inverse, contiguous pass: stages LOGN-1 .. LOGN-8 (gap 1 .. 128); lazy [0,2q) out
// =====================================================================================================
// MODE: M_GUARD the exact integer butterflies; M_LAZY8 / M_LAZY16 (modarith.hip.h) with (q, q2) = (2^64 - q, 2^64 - 4q), values below
// 4q instead of 2q; M_FPN / M_FPR exact FP64 (modarith.hip.h gs_bfly_fp: canonical integers in, doubles out to the strided pass;
// tw / twb = the FP64 inverse tables, (q, q2) = the bit patterns of (double q, 1/q)).  M_GUARD2 and M_NOGUARD are forward only.
// one butterfly of an inverse tile on registers (j, j + half): stage i of a register block whose M_LAZY16 schedule is xk
template <int MODE>
__device__ __forceinline__ void gs_bfly_tile(uint64_t (&x)[16], int j, int half, uint64_t w, uint64_t wq, uint64_t q, uint64_t q2, const bool redsum,
                                             uint32_t xk, int i)
{
    if constexpr (MODE == M_LAZY16)
    {
        if (lazy16_inv_kind(xk, i, j, half))
        {
            gs_bfly_lazy16<1>(x[j], x[j + half], w, wq, q, q2);
        }
        else
        {
            gs_bfly_lazy16<0>(x[j], x[j + half], w, wq, q, q2);
        }
    }
    else
    {
        gs_bfly_t<MODE>(x[j], x[j + half], w, wq, q, q2, redsum);
    }
}

template <int LOGN, int MODE>
__device__ __forceinline__ void inv_contig_tile(uint64_t *rowp, uint32_t tile, const Tw *__restrict__ tw,
                                                uint64_t q, uint64_t q2, ulonglong2 *lds2, const uint32_t tid,
                                                const Tw *__restrict__ twb, const uint64_t *srcp = nullptr, Tw *ldstw = nullptr)
{
    static_assert(MODE != M_GUARD2 && MODE != M_NOGUARD, "M_GUARD2 and M_NOGUARD have no inverse butterflies");
    constexpr int R1 = LOGN - 8;
    uint64_t *lds = reinterpret_cast<uint64_t *>(lds2);
    uint64_t *base = rowp + ((size_t)tile << 12);
    const uint32_t b = tid >> 4;
    const uint32_t tl = tid & 15u;
    const uint32_t blk = (tile << 4) + b;
    const Tw *__restrict__ twbt = twb + (size_t)tile * (15 * 256);
    // M_LAZY16: two register blocks of four stages from inputs below 4q
    constexpr Lazy16Inv z1 = lazy16_inv(4, 4, false), z2 = lazy16_inv(4, z1.out, false);
    static_assert(z1.peak <= 16 && z2.peak <= 16, "a value of 16q or more");
    static_assert(z2.out == lazy16_inv_handover(), "the strided pass starts from another bound");

    // the per-thread twiddles of the first four stages do not depend on the data: fetch them while the tile is
    // staged through LDS instead of one by one behind the barrier (-3.7 % on the inverse transform; the same
    // prefetch in the forward passes costs registers they do not have and measured slower)
    Tw tb[15];
#pragma unroll
    for (int i = 0; i < 15; ++i)
    {
        tb[i] = twbt[((uint32_t)i << 8) + tid];
    }
    // ldstw (optional, unused by the kernels): the last four stages' twiddles through LDS like the forward pass's first four
    // (fwd_contig_tile).  Measured on the bench's batch, same box: inverse 11.05 ms with it against 10.99 without -- this pass
    // already has its first four stages' twiddles in registers before the tile arrives, and the extra 4 KiB of LDS buy nothing.
    if (ldstw)
    {
        const uint32_t ln = tid & 63u;
        if (ln < 60u)
        {
            const uint32_t bb = ((tid >> 6) << 2) + ln / 15u, i = ln % 15u;
            const uint32_t u = i == 0 ? 0u : (i < 3 ? 1u : (i < 7 ? 2u : 3u)), k = i - ((1u << u) - 1u);
            ldstw[bb * 15u + i] = tw[(1u << (R1 + u)) + (((tile << 4) + bb) << u) + k];
        }
    }
    // the row read may be another buffer's (NttArgs::src) or the one written: the tile is whole in LDS before any of it is stored
    const ulonglong2 *in2 = reinterpret_cast<const ulonglong2 *>(srcp ? srcp + ((size_t)tile << 12) : base);
    // every wave stages the 64 rows its own lanes transform (8 KiB, contiguous): the exchanges of this pass are wave-local
    const uint32_t wbase = (tid >> 6) << 9, lane = tid & 63u;
#pragma unroll
    for (int it = 0; it < 8; ++it)
    {
        uint32_t ch = wbase + (uint32_t)it * 64u + lane;
        uint32_t rr = ch >> 3;
        lds2[(rr << 3) | ((ch & 7u) ^ (rr & 7u))] = in2[ch];
    }
    lds_wave_sync();
    const uint32_t myrow = tid;
    uint64_t x[16];
#pragma unroll
    for (int c = 0; c < 8; ++c)
    {
        ulonglong2 v = lds2[(myrow << 3) | ((uint32_t)c ^ (myrow & 7u))];
        // FP64 modes: any input below 2^52 (canonical or lazy, like the integer butterflies accept); FPN folds it to |.| <= q/2
        // here -- its schedule of sum reductions counts from there --, FPR folds in every butterfly anyway
        x[2 * c] = MODE == M_FPN ? d2u(fp_red(fp_from_u52(v.x), u2d(q), u2d(q2))) : (MODE == M_FPR ? d2u(fp_from_u52(v.x)) : v.x);
        x[2 * c + 1] = MODE == M_FPN ? d2u(fp_red(fp_from_u52(v.y), u2d(q), u2d(q2))) : (MODE == M_FPR ? d2u(fp_from_u52(v.y)) : v.y);
    }
#pragma unroll
    for (int u = 7; u >= 4; --u)
    {
        const int half = 8 >> (u - 4);
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            if (!(j & half))
            {
                Tw t = tb[(1 << (u - 4)) - 1 + (j >> (8 - u))];
                gs_bfly_tile<MODE>(x, j, half, t.w, t.wq, q, q2, (u & 3) == 0, z1.xk, 7 - u); // FPN: sums folded in every fourth stage
            }
        }
    }
    // rows are private to their thread: no barrier needed before writing them back
#pragma unroll
    for (int c = 0; c < 8; ++c)
    {
        ulonglong2 v;
        v.x = x[2 * c];
        v.y = x[2 * c + 1];
        lds2[(myrow << 3) | ((uint32_t)c ^ (myrow & 7u))] = v;
    }
    lds_wave_sync();
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        x[j] = lds[phys_contig((b << 8) | ((uint32_t)j << 4) | tl)];
    }
#pragma unroll
    for (int u = 3; u >= 0; --u)
    {
        const int half = 8 >> u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            if (!(j & half))
            {
                Tw t = ldstw ? ldstw[b * 15u + ((1u << u) - 1u) + (uint32_t)(j >> (4 - u))]
                             : tw[(1u << (R1 + u)) + (blk << u) + (uint32_t)(j >> (4 - u))];
                gs_bfly_tile<MODE>(x, j, half, t.w, t.wq, q, q2, (u & 3) == 0, z2.xk, 3 - u); // FPN: sums folded in every fourth stage
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        base[(b << 8) | ((uint32_t)j << 4) | tl] = x[j];
    }
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(256) void ntt_inv_contig(NttArgs a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    __shared__ ulonglong2 lds2[2048];
    const uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t pol = w % a.n_poly;
    const uint32_t rest = w / a.n_poly;
    const uint32_t tile = rest % TPR;
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.sel.idx[rest / TPR]);
    const uint32_t prime = __builtin_amdgcn_readfirstlane(a.selp.idx[rest / TPR]);
    const PrimeConst &pc = a.pc[prime];
    const uint64_t *srcp = a.src ? a.src + (((size_t)pol * a.src_stride + a.src_off + r) << LOGN) : nullptr;
    inv_contig_tile<LOGN, MODE>(a.data + (((size_t)pol * a.L + r) << LOGN), tile, a.tw + ((size_t)prime << LOGN), mode_q<MODE>(pc),
                                mode_q2<MODE>(pc), lds2, threadIdx.x, a.twb + (size_t)prime * ((size_t)TPR * 15 * 256), srcp);
}

// The same tile of two polynomials by one workgroup, every twiddle fetched once (fwd_contig_tile2 says why).  Both tiles' loads
// are issued first and wait in registers; the fifteen per-thread twiddles are fetched behind the staging, where they are used
// (inv_contig_tile holds all fifteen ahead of its tile, 60 registers, which do not fit beside 64 of data).  srcA / srcB (or
// null): NttArgs::src's rows of the two polynomials.
template <int LOGN, int MODE>
__device__ __forceinline__ void inv_contig_tile2(uint64_t *rowA, uint64_t *rowB, uint32_t tile, const Tw *__restrict__ tw, uint64_t q,
                                                 uint64_t q2, ulonglong2 *lds2, const uint32_t tid, const Tw *__restrict__ twb,
                                                 const uint64_t *srcA, const uint64_t *srcB)
{
    static_assert(contig_pair_mode(MODE) && MODE == M_LAZY16, "the paired pass takes M_LAZY16's schedule");
    constexpr int R1 = LOGN - 8;
    uint64_t *lds = reinterpret_cast<uint64_t *>(lds2);
    uint64_t *baseA = rowA + ((size_t)tile << 12);
    uint64_t *baseB = rowB + ((size_t)tile << 12);
    const uint32_t b = tid >> 4;
    const uint32_t tl = tid & 15u;
    const uint32_t blk = (tile << 4) + b;
    const Tw *__restrict__ twbt = twb + (size_t)tile * (15 * 256);
    constexpr Lazy16Inv z1 = lazy16_inv(4, 4, false), z2 = lazy16_inv(4, z1.out, false);
    static_assert(z1.peak <= 16 && z2.peak <= 16, "a value of 16q or more");
    static_assert(z2.out == lazy16_inv_handover(), "the strided pass starts from another bound");

    const ulonglong2 *inA = reinterpret_cast<const ulonglong2 *>(srcA ? srcA + ((size_t)tile << 12) : baseA);
    const ulonglong2 *inB = reinterpret_cast<const ulonglong2 *>(srcB ? srcB + ((size_t)tile << 12) : baseB);
    const uint32_t wbase = (tid >> 6) << 9, lane = tid & 63u;
    uint64_t ra[16], rb[16];
#pragma unroll
    for (int it = 0; it < 8; ++it)
    {
        const ulonglong2 v = inA[wbase + (uint32_t)it * 64u + lane];
        ra[2 * it] = v.x;
        ra[2 * it + 1] = v.y;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it)
    {
        const ulonglong2 v = inB[wbase + (uint32_t)it * 64u + lane];
        rb[2 * it] = v.x;
        rb[2 * it + 1] = v.y;
    }
    const uint32_t myrow = tid;
    uint64_t xa[16], xb[16];
    // every wave stages the 64 rows its own lanes transform, A's then B's
    auto stage_in = [&](const uint64_t(&raw)[16], uint64_t(&x)[16]) {
#pragma unroll
        for (int it = 0; it < 8; ++it)
        {
            const uint32_t ch = wbase + (uint32_t)it * 64u + lane;
            const uint32_t rr = ch >> 3;
            ulonglong2 v;
            v.x = raw[2 * it];
            v.y = raw[2 * it + 1];
            lds2[(rr << 3) | ((ch & 7u) ^ (rr & 7u))] = v;
        }
        lds_wave_sync();
#pragma unroll
        for (int c = 0; c < 8; ++c)
        {
            ulonglong2 v = lds2[(myrow << 3) | ((uint32_t)c ^ (myrow & 7u))];
            x[2 * c] = v.x;
            x[2 * c + 1] = v.y;
        }
    };
    stage_in(ra, xa);
    // the per-thread twiddles of the first four stages, slot s at twbt[s * 256 + tid]: the first ones arrive under B's staging
    Tw tq[15];
#pragma unroll
    for (int k = 0; k < PAIR_TW_AHEAD; ++k)
    {
        tq[inv_slot_of_order(k)] = twbt[((uint32_t)inv_slot_of_order(k) << 8) + tid];
    }
    lds_wave_order(); // B's chunks overwrite A's behind the reads of A's rows
    stage_in(rb, xb);
#pragma unroll
    for (int u = 7; u >= 4; --u)
    {
        const int half = 8 >> (u - 4);
#pragma unroll
        for (int i = 0; i < 8; ++i)
        {
            const int j = ((i & ~(half - 1)) << 1) | (i & (half - 1)); // the i-th register index without the bit `half`
            {
                const int slot = (1 << (u - 4)) - 1 + (j >> (8 - u));
                if ((j & ((1 << (8 - u)) - 1)) == 0)
                {
                    const int k = inv_order_of_slot(slot) + PAIR_TW_AHEAD;
                    if (k < 15)
                    {
                        tq[inv_slot_of_order(k)] = twbt[((uint32_t)inv_slot_of_order(k) << 8) + tid];
                    }
                }
                const Tw t = tq[slot];
                gs_bfly_tile<MODE>(xa, j, half, t.w, t.wq, q, q2, false, z1.xk, 7 - u);
                gs_bfly_tile<MODE>(xb, j, half, t.w, t.wq, q, q2, false, z1.xk, 7 - u);
                pair_fence(xa[j], xa[j + half], xb[j], xb[j + half]);
            }
        }
    }
    // (an opaque copy of the thread index: the eight swizzled row slots are computed again instead of staying in registers
    // across the four stages above)
    uint32_t t2 = tid;
    asm volatile("" : "+v"(t2));
    // the last four stages' twiddles, shared by the sixteen threads of a block: slot s of stage u at tw[2^(R1+u) + blk * 2^u + k]
    Tw ts[15];
#pragma unroll
    for (int k = 0; k < PAIR_TW_AHEAD; ++k)
    {
        const int sl = inv_slot_of_order(k), u = slot_stage(sl);
        ts[sl] = tw[(1u << (R1 + u)) + (blk << u) + (uint32_t)(sl + 1 - (1 << u))];
    }
    // rows to columns, A's then B's (a row is private to its thread: nothing to wait for before it is written back)
    auto transpose = [&](uint64_t(&x)[16]) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
        {
            ulonglong2 v;
            v.x = x[2 * c];
            v.y = x[2 * c + 1];
            lds2[(t2 << 3) | ((uint32_t)c ^ (t2 & 7u))] = v;
        }
        lds_wave_sync();
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            x[j] = lds[phys_contig((b << 8) | ((uint32_t)j << 4) | tl)];
        }
    };
    transpose(xa);
    lds_wave_order(); // B's rows overwrite A's behind the reads of A's columns
    transpose(xb);
#pragma unroll
    for (int u = 3; u >= 0; --u)
    {
        const int half = 8 >> u;
#pragma unroll
        for (int i = 0; i < 8; ++i)
        {
            const int j = ((i & ~(half - 1)) << 1) | (i & (half - 1)); // the i-th register index without the bit `half`
            {
                const int slot = (1 << u) - 1 + (j >> (4 - u));
                if ((j & ((1 << (4 - u)) - 1)) == 0)
                {
                    const int k = inv_order_of_slot(slot) + PAIR_TW_AHEAD;
                    if (k < 15)
                    {
                        const int sl = inv_slot_of_order(k), un = slot_stage(sl);
                        ts[sl] = tw[(1u << (R1 + un)) + (blk << un) + (uint32_t)(sl + 1 - (1 << un))];
                    }
                }
                const Tw t = ts[slot];
                gs_bfly_tile<MODE>(xa, j, half, t.w, t.wq, q, q2, false, z2.xk, 3 - u);
                gs_bfly_tile<MODE>(xb, j, half, t.w, t.wq, q, q2, false, z2.xk, 3 - u);
                pair_fence(xa[j], xa[j + half], xb[j], xb[j + half]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        baseA[(b << 8) | ((uint32_t)j << 4) | tl] = xa[j];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        baseB[(b << 8) | ((uint32_t)j << 4) | tl] = xb[j];
    }
}

// polynomials 2p and 2p + 1 of the launch per workgroup; a.n_poly is even (the launcher gives an odd last polynomial to
// ntt_inv_contig), a.total_work = n_poly / 2 * Lsel * TPR
template <int LOGN, int MODE>
__global__ __launch_bounds__(256, 4) void ntt_inv_contig2(NttArgs a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    __shared__ ulonglong2 lds2[2048];
    const uint32_t pairs = a.n_poly >> 1;
    const uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t pol = (w % pairs) << 1;
    const uint32_t rest = w / pairs;
    const uint32_t tile = rest % TPR;
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.sel.idx[rest / TPR]);
    const uint32_t prime = __builtin_amdgcn_readfirstlane(a.selp.idx[rest / TPR]);
    const PrimeConst &pc = a.pc[prime];
    const uint64_t *srcA = a.src ? a.src + (((size_t)pol * a.src_stride + a.src_off + r) << LOGN) : nullptr;
    uint64_t *rowA = a.data + (((size_t)pol * a.L + r) << LOGN);
    inv_contig_tile2<LOGN, MODE>(rowA, rowA + ((size_t)a.L << LOGN), tile, a.tw + ((size_t)prime << LOGN), mode_q<MODE>(pc), mode_q2<MODE>(pc), lds2,
                                 threadIdx.x, a.twb + (size_t)prime * ((size_t)TPR * 15 * 256), srcA,
                                 srcA ? srcA + ((size_t)a.src_stride << LOGN) : nullptr);
}

// =====================================================================================================
// inverse, strided pass: stages LOGN-9 .. 0, N^-1 folded into stage 0; writes canonical
// =====================================================================================================
// the lazy modes' pass is compiled for four workgroups per CU, the others for five; at N = 2^16 the former take phase B's twiddles
// through LDS (inv_strided_tile)
constexpr bool inv_strided_occ4(int mode)
{
    return mode_lazy(mode);
}
template <int LOGN, int MODE>
__device__ __forceinline__ void inv_strided_tile(uint64_t *__restrict__ rowp, uint32_t tile, const Tw *__restrict__ tw,
                                                 const PrimeConst *pc, uint64_t *lds, const uint32_t tid)
{
    static_assert(MODE != M_GUARD2 && MODE != M_NOGUARD, "M_GUARD2 and M_NOGUARD have no inverse butterflies");
    constexpr int R1 = LOGN - 8;
    constexpr int RB = R1 - 4;
    constexpr int GB = 12 - R1;
    constexpr uint32_t G = 1u << GB;
    const uint64_t q = mode_q<MODE>(*pc), q2 = mode_q2<MODE>(*pc);
    uint64_t *__restrict__ row = rowp + tile * G;
    // M_LAZY16: phase B's RB stages from what the contiguous pass hands over, then phase A's four, the transform's last among them
    constexpr Lazy16Inv zb = lazy16_inv(RB, lazy16_inv_handover(), false), za = lazy16_inv(4, zb.out, true);
    static_assert(zb.peak <= 16 && za.peak <= 16, "a value of 16q or more");
    static_assert(za.out <= 4 && za.xlast <= 2, "the final subtractions expect products below 4q and the sums times N^-1 below 2q");

    // LDSTW (the lazy modes at N = 2^16: four workgroups per CU either way): phase B's twiddles -- entries 16..255 of the table, shared by
    // the sixteen threads of a group -- through a copy in LDS (`lds` + 4096 words), as in the forward strided pass
    constexpr bool LDSTW = LOGN == 16 && inv_strided_occ4(MODE);
    Tw *ldstw = reinterpret_cast<Tw *>(lds + 4096);
    uint64_t x[16];
    if (RB > 0)
    {
        const uint32_t g = tid & (G - 1);
        const uint32_t th = tid >> GB;
        if (LDSTW)
        {
            ldstw[tid] = tw[tid];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            uint32_t t_ = (th << 4) | (uint32_t)j;
            x[j] = row[(t_ << 8) | g];
        }
        if (LDSTW)
        {
            lds_barrier();
        }
#pragma unroll
        for (int s = R1 - 1; s >= 4; --s)
        {
            const int half = 1 << (R1 - 1 - s);
#pragma unroll
            for (int j = 0; j < 16; ++j)
            {
                if (!(j & half))
                {
                    uint32_t t_ = (th << 4) | (uint32_t)j;
                    Tw t = LDSTW ? ldstw[(1u << s) + (t_ >> (R1 - s))] : tw[(1u << s) + (t_ >> (R1 - s))];
                    gs_bfly_tile<MODE>(x, j, half, t.w, t.wq, q, q2, ((R1 - 1 - s) & 3) == 3, zb.xk, R1 - 1 - s); // stage number in this pass
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            lds[phys_strided<GB>((th << (GB + 4)) | ((uint32_t)j << GB) | g)] = x[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            x[j] = lds[phys_strided<GB>((uint32_t)j * 256u + tid)];
        }
    }
    else
    {
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            uint32_t e = (uint32_t)j * 256u + tid;
            x[j] = row[((e >> GB) << 8) + (e & (G - 1))];
        }
    }
#pragma unroll
    for (int u = 3; u >= 1; --u)
    {
        const int half = 8 >> u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            if (!(j & half))
            {
                Tw t = tw[(1u << u) + (uint32_t)(j >> (4 - u))];
                gs_bfly_tile<MODE>(x, j, half, t.w, t.wq, q, q2, ((RB + 3 - u) & 3) == 3, za.xk, 3 - u);
            }
        }
    }
    {
        const Tw ninv = pc->ninv;
        const Tw ninv_w1 = pc->ninv_w1;
        const uint64_t qh = pc->qh;
#pragma unroll
        for (int j = 0; j < 8; ++j)
        {
            if constexpr (MODE == M_LAZY16)
            {
                if (lazy16_inv_kind(za.xk, 3, j, 8))
                {
                    gs_bfly_last_lazy16<1, LOGN>(x[j], x[j + 8], qh, ninv_w1, q, q2);
                }
                else
                {
                    gs_bfly_last_lazy16<0, LOGN>(x[j], x[j + 8], qh, ninv_w1, q, q2);
                }
            }
            else if constexpr (MODE == M_LAZY8)
            {
                gs_bfly_last_lazy8<LOGN>(x[j], x[j + 8], qh, ninv_w1, q, q2);
            }
            else
            {
                gs_bfly_last_t<MODE>(x[j], x[j + 8], ninv, ninv_w1, q, q2);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        uint64_t v;
        if (mode_fp(MODE))
        {
            v = fp_to_canonical(u2d(x[j]), u2d(q), u2d(q2));
        }
        else if (mode_lazy(MODE))
        {
            // registers 0..7 hold the last stage's sums times N^-1, below 2q: one conditional subtraction; registers 8..15 its
            // products, below 4q: two, with 2^64 - 2q = (2^64 - 4q) / 2 + 2^63.  (The quotient step of the forward pass would take
            // 10 vector instructions where these chains take 4 and 8.)
            v = j < 8 ? csub_sign(x[j], q) : csub_sign(csub_sign(x[j], (q2 >> 1) | 0x8000000000000000ull), q);
        }
        else
        {
            v = csub(x[j], q); // below 2q
        }
        row[((uint32_t)j << (16 - GB)) | ((tid >> GB) << 8) | (tid & (G - 1))] = v; // element j * 256 + tid, as in strided_load_raw
    }
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(256, inv_strided_occ4(MODE) ? 4 : 5) void ntt_inv_strided(NttArgs a)
{
    constexpr uint32_t TPR = 1u << (LOGN - 12);
    __shared__ uint64_t lds[4096 + ((LOGN == 16 && inv_strided_occ4(MODE)) ? 512 : 0)]; // the exchange buffer (+ phase B's twiddles, inv_strided_tile)
    const uint32_t w = xcd_remap(blockIdx.x, a.total_work);
    const uint32_t tile = w % TPR;
    const uint32_t srow = w / TPR; // over n_poly * Lsel selected rows
    const uint32_t si = srow % a.Lsel;
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.sel.idx[si]);
    const uint32_t prime = __builtin_amdgcn_readfirstlane(a.selp.idx[si]);
    inv_strided_tile<LOGN, MODE>(a.data + ((size_t)((srow / a.Lsel) * a.L + r) << LOGN), tile, a.tw + ((size_t)prime << LOGN), a.pc + prime, lds,
                               threadIdx.x);
}

// =====================================================================================================
// small transforms (N <= 2048): one workgroup per RNS row, whole row in LDS
// =====================================================================================================
template <bool INV>
__global__ __launch_bounds__(256) void ntt_small(NttArgs a, int logn)
{
    __shared__ uint64_t lds[2048];
    const uint32_t n = 1u << logn;
    const uint32_t prow = blockIdx.x;
    const uint32_t prime = a.rows.idx[prow % a.L];
    const Tw *__restrict__ tw = a.tw + ((size_t)prime << logn);
    const PrimeConst *pc = a.pc + prime;
    const uint64_t q = pc->q;
    const uint64_t q2 = pc->q2;
    uint64_t *__restrict__ row = a.data + ((size_t)prow << logn);
    const uint32_t tid = threadIdx.x;

    for (uint32_t i = tid; i < n; i += 256)
    {
        lds[i] = row[i];
    }
    __syncthreads();
    if (!INV)
    {
        for (int s = 0; s < logn; ++s)
        {
            const int lg = logn - 1 - s; // log2(gap)
            for (uint32_t bf = tid; bf < (n >> 1); bf += 256)
            {
                uint32_t blk = bf >> lg;
                uint32_t off = bf & ((1u << lg) - 1);
                uint32_t i0 = (blk << (lg + 1)) | off;
                Tw t = tw[(1u << s) + blk];
                uint64_t x = lds[i0], y = lds[i0 + (1u << lg)];
                ct_bfly(x, y, t.w, t.wq, q, q2);
                lds[i0] = x;
                lds[i0 + (1u << lg)] = y;
            }
            __syncthreads();
        }
        for (uint32_t i = tid; i < n; i += 256)
        {
            row[i] = csub(csub(lds[i], q2), q);
        }
    }
    else
    {
        for (int s = logn - 1; s >= 1; --s)
        {
            const int lg = logn - 1 - s;
            for (uint32_t bf = tid; bf < (n >> 1); bf += 256)
            {
                uint32_t blk = bf >> lg;
                uint32_t off = bf & ((1u << lg) - 1);
                uint32_t i0 = (blk << (lg + 1)) | off;
                Tw t = tw[(1u << s) + blk];
                uint64_t x = lds[i0], y = lds[i0 + (1u << lg)];
                gs_bfly(x, y, t.w, t.wq, q, q2);
                lds[i0] = x;
                lds[i0 + (1u << lg)] = y;
            }
            __syncthreads();
        }
        const Tw ninv = pc->ninv;
        const Tw ninv_w1 = pc->ninv_w1;
        for (uint32_t bf = tid; bf < (n >> 1); bf += 256)
        {
            uint64_t x = lds[bf], y = lds[bf + (n >> 1)];
            gs_bfly_last(x, y, ninv, ninv_w1, q, q2);
            lds[bf] = x;
            lds[bf + (n >> 1)] = y;
        }
        __syncthreads();
        for (uint32_t i = tid; i < n; i += 256)
        {
            row[i] = csub(lds[i], q);
        }
    }
}

// =====================================================================================================
// one radix-2 stage over global memory (debug / cross-check path: MOAI_NTT_NAIVE=1)
// =====================================================================================================
template <bool INV>
__global__ __launch_bounds__(256) void ntt_stage_global(NttArgs a, int logn, int s, int last)
{
    const uint32_t half_n = 1u << (logn - 1);
    const uint32_t bf = blockIdx.x * 256u + threadIdx.x;
    const uint32_t prow = blockIdx.y;
    if (bf >= half_n)
    {
        return;
    }
    const uint32_t prime = a.rows.idx[prow % a.L];
    const Tw *__restrict__ tw = a.tw + ((size_t)prime << logn);
    const PrimeConst *pc = a.pc + prime;
    const uint64_t q = pc->q;
    const uint64_t q2 = pc->q2;
    uint64_t *__restrict__ row = a.data + ((size_t)prow << logn);
    const int lg = logn - 1 - s;
    uint32_t blk = bf >> lg;
    uint32_t off = bf & ((1u << lg) - 1);
    uint32_t i0 = (blk << (lg + 1)) | off;
    uint32_t i1 = i0 + (1u << lg);
    uint64_t x = row[i0], y = row[i1];
    if (!INV)
    {
        Tw t = tw[(1u << s) + blk];
        ct_bfly(x, y, t.w, t.wq, q, q2);
        if (last)
        {
            x = csub(csub(x, q2), q);
            y = csub(csub(y, q2), q);
        }
    }
    else if (s > 0)
    {
        Tw t = tw[(1u << s) + blk];
        gs_bfly(x, y, t.w, t.wq, q, q2);
    }
    else
    {
        gs_bfly_last(x, y, pc->ninv, pc->ninv_w1, q, q2);
        x = csub(x, q);
        y = csub(y, q);
    }
    row[i0] = x;
    row[i1] = y;
}

} // namespace moai
