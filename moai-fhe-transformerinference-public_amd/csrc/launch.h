// launch.h -- host-side entry points shared between the translation units of the library.
#pragma once
#include <type_traits>

#include "common.h"
#include "rowlaunch.h"

namespace moai {

// Every tuning knob of the library: X(id, default, what it does).  The environment variable and the moai_set_tuning name
// of a knob is "MOAI_" #id.  Knobs change speed or memory use, never results.  (MOAI_STREAM_AUDIT is a debug switch with
// a path of its own, common.h; the seal:: shim's MOAI_SHIM_* / MOAI_BOOT_* / MOAI_POOL_* switches live in the shim.)
#define MOAI_KNOBS(X)                                                                                                          \
    X(NTT_FP, 1, "0: primes below 2^51 stay on the integer units in every transform, key switch and mod-down")                \
    X(NTT_LAZY8, 1, "0: integer primes below 2^60 take the exact butterflies instead of the approximate Shoup quotient")       \
    X(NTT_LAZY16, 1, "0: those primes keep values below 8q with a guard in every stage instead of below 16q with fewer (M_LAZY8)") \
    X(NTT_LDSTW, 1, "0: the forward contiguous pass loads its first stages' twiddles from memory instead of through LDS")      \
    X(NTT_PAIR, 1, "0: the contiguous passes of the 60-bit rows run one polynomial per workgroup instead of two that share their twiddles") \
    X(NTT_CHUNK_MB, 88, "> 0: launch the two passes of a transform per chunk of whole polynomials of at most this many MiB")    \
    X(NTT_CHUNK_KB, 0, "KiB added to MOAI_NTT_CHUNK_MB: chunks of rings whose polynomials are smaller than a MiB")             \
    X(NTT_PIPE, 2, "1..3: deal those chunks to this many side streams, so that a chunk's second pass runs beside the next one's first; 0: one stream") \
    X(NTT_PIPE_MIN, 32, "chunks per side stream below which a transform stays on the caller's stream")                         \
    X(NTT_PIPE_INNER, 0, "1: the transforms inside key switch, mod-down, encode and decode take the MOAI_NTT_PIPE schedule too") \
    X(NTT_NAIVE, 0, "1: one launch per radix-2 stage over global memory (cross-check path)")                                   \
    X(KS_FP_MIN_ROWS, 16, "batch * L from which the key switch uses the FP64 arithmetic modes")                                \
    X(KS_TMP_MB, 8192, "MiB of key-switch digits in flight: sets how many output moduli share a launch")                       \
    X(KS_P1_ITEMS, 8, "1: the key switch's strided pass at N = 2^16 runs one tile per workgroup instead of eight, pipelined")  \
    X(KS_HOIST_PAIR, 4, "rotations per pass of the hoisted MAC in the FP64 modes: 4, 2, or 0 for one")                         \
    X(MD_FP_MIN_ROWS, 256, "polynomials * L from which mod-down and rescale use the FP64 arithmetic modes")                    \
    X(MATMUL_FP, 1, "0: moai_ct_pt_matmul keeps primes below 2^51 on the integer kernel")                                      \
    X(DEC_TMP_MB, 1024, "MiB of scratch per chunk of moai_ckks_decode when the stream's arena is smaller")                     \
    X(CLIENT_TMP_KB, 1048576, "KiB of scratch per chunk of the encryption and key generation calls when the stream's arena is smaller") \
    X(HYBRID_TMP_KB, 16777216, "KiB of scratch per chunk of the hybrid key switch: sets how many ciphertexts of a batch are in flight") \
    X(HYBRID_HOIST_NR, 4, "rotations per pass of the hybrid hoisted MAC over the digits: 4, 2 or 1")

enum Knob
{
#define MOAI_KNOB_ID(id, dflt, what) K_##id,
    MOAI_KNOBS(MOAI_KNOB_ID)
#undef MOAI_KNOB_ID
    KNOB_COUNT
};
// a knob's value: what moai_set_tuning stored, else the environment variable (read once, on first use), else the default.
// One relaxed atomic load.
long tuning(Knob k);

// Calls f(std::integral_constant<int, V>) for the V among Vs that equals v and returns what f returns; a v outside the list is
// MOAI_ELOGIC "unsupported <what><v>", never a default case.  Every call site names the values it has kernels for, so no other
// instantiation can appear.
template <int... Vs, class F>
int dispatch(const char *what, int v, F &&f)
{
    int rc = MOAI_OK;
    const bool found = ((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return found ? rc : set_error(MOAI_ELOGIC, "unsupported %s%d", what, v);
}
// the tiled kernels exist for N = 2^12 .. 2^16
template <class F>
int dispatch_logn(int logn, F &&f)
{
    return dispatch<12, 13, 14, 15, 16>("poly_modulus_degree 2^", logn, f);
}
// f(x0, cnt) for consecutive chunks of at most `per` of n items, until one returns a code other than MOAI_OK
template <class F>
int for_chunks(size_t n, size_t per, F &&f)
{
    for (size_t x0 = 0; x0 < n; x0 += per)
    {
        MOAI_TRY(f(x0, n - x0 < per ? n - x0 : per));
    }
    return MOAI_OK;
}
// the same over the terms of a sum, where no terms at all is one empty chunk (out = base)
template <class F>
int for_term_chunks(size_t terms, size_t per, F &&f)
{
    return terms ? for_chunks(terms, per, f) : f(0, 0);
}
// whether the byte ranges [a, a + a_bytes) and [b, b + b_bytes) intersect
inline bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}
// operation census for the end-to-end bench (moai_op_trace): counts `units` (polynomials, ciphertexts or products, as the
// entry point's own batch argument counts them) per (entry point, level); a relaxed atomic load when it is off
void trace_op(const char *name, size_t L, size_t units);
bool noguard_ok(uint64_t q);
// makes the context's device current for the calling thread (contexts of several devices may live in one process);
// every operation entry point calls it before it allocates or launches
int enter_device(const moai_ctx *c);
// arithmetic mode (modarith.hip.h M_*) of a transform under a context prime: FP64 (M_FPN / M_FPR) below 2^51 unless MOAI_NTT_FP=0
// or the caller does not allow it, else integer with (M_GUARD) or without (M_NOGUARD) per-stage guards
int ntt_mode(const moai_ctx *c, uint32_t prime, bool allow_fp = true);
// the kernel class of the plain tiled transform for a row under a context prime (ntt.hip launch_fwd / launch_inv):
// forward M_LAZY16, M_LAZY8, M_GUARD2, M_NOGUARD, M_FPN or M_FPR; inverse M_LAZY16, M_LAZY8, M_GUARD (the exact integer
// butterflies), M_FPN or M_FPR.  In both directions the class is the MODE the kernels are instantiated with.
int fwd_class(const moai_ctx *c, uint32_t prime);
int inv_class(const moai_ctx *c, uint32_t prime);
// the twiddle tables of a mode: tw in natural order, twb in the contiguous pass's per-thread order
struct TwPair
{
    const Tw *tw, *twb;
};
TwPair twiddles(const moai_ctx *c, int mode, bool inverse);
// kernel arguments of a transform of data [n_poly][L][N] with every row selected and no grid size yet (ntt_kernels.hip.h)
struct NttArgs;
NttArgs ntt_args(const moai_ctx *c, uint64_t *data, size_t n_poly, size_t L, const RowMap &rows, bool inverse);
int make_rowmap(const moai_ctx *c, size_t L, const uint32_t *prime_index, RowMap *out);
// the head of an entry point that takes a level and a row selection: "null context", "invalid level" unless 1 <= L <= k, then
// make_rowmap
int rows_entry(const moai_ctx *c, size_t L, const uint32_t *prime_index, RowMap *out);
// src (inverse only): polynomial p's row r is read from src row p * src_stride_rows + src_off_rows + r, the result lands in
// `data` [n_poly][L][N] -- the inverse transform of a slice of a larger layout without copying the slice first
// entry: the call is moai_ntt_forward's or moai_ntt_inverse's own; the others take the side streams of MOAI_NTT_PIPE only under
// MOAI_NTT_PIPE_INNER
int ntt_launch(moai_ctx *c, uint64_t *data, size_t n_poly, size_t L, const RowMap &rows, bool inverse,
               hipStream_t s, const uint64_t *src = nullptr, size_t src_stride_rows = 0, size_t src_off_rows = 0, bool entry = false);
// The chunk schedule of a two-pass transform of n_poly polynomials of L rows of n coefficients, with chunks of chunk_bytes
// (rounded down to whole polynomials, at least one) dealt round-robin to k side streams: the number of chunks the busiest
// stream gets, or 0 for the caller's stream alone -- k < 1, no chunk size, fewer than two chunks (no second pass has a first
// pass to run beside), or fewer than min_chunks for the busiest stream.  More streams than NTT_PIPE_MAX or than chunks are not
// used.  Pure host arithmetic.
size_t ntt_pipe_plan(size_t n_poly, size_t L, size_t n, size_t chunk_bytes, long k, long min_chunks, size_t *chunk_polys = nullptr,
                     int *streams = nullptr);
// the side streams and events of caller's stream s, made on first use; nullptr when they could not be made (remembered)
moai_ctx::NttPipe *ntt_pipe(moai_ctx *c, hipStream_t s);
// returns the context workspace grown to at least `bytes` (grows only outside stream capture)
int workspace(moai_ctx *c, size_t bytes, hipStream_t s, void **out);
// items per chunk of a batch of n whose items need per_bytes of scratch each: as many as fit the stream's arena, or floor_bytes
// when the arena is smaller or absent; at least 1, at most cap and n.  The caller holds op_mutex and sizes workspace() with it.
size_t chunk_items(moai_ctx *c, hipStream_t s, size_t per_bytes, size_t n, size_t cap, size_t floor_bytes);
// headroom: allocate max(1.25 x bytes, 1.5 x the current size) when the arena has to grow
int reserve_for_stream(moai_ctx *c, void *stream, size_t bytes, void **out, bool headroom);
// device pointer to the Galois permutation table of `elt` (built on first use, on the NULL stream, and complete on return)
int galois_table(moai_ctx *c, uint32_t elt, const uint32_t **out);
// out [batch][L][N] = the Galois permutation of polynomial 0 of every ciphertext of in [batch][2][L][N]
int galois_permute_c0(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t batch, size_t L, uint32_t galois_elt, hipStream_t s);
// the hoisted rotations' kernels of keyswitch_kernels.hip.h for another translation unit (hybrid.hip):
// mask [copies][N], every copy = 1 where x -> x^elt negates the coefficient that lands there (galois_sign_mask_kernel)
int galois_sign_mask(moai_ctx *c, uint64_t *mask, uint32_t galois_elt, size_t copies, hipStream_t s);
// *found = one of the `words` (an even number) words at v is zero (any_zero_kernel): clears the device word `flag`, runs the
// kernel, copies the word back and synchronizes the stream
int probe_any_zero(moai_ctx *c, const uint64_t *v, size_t words, uint32_t *flag, hipStream_t s, bool *found);
// MOAI_EINVAL "Galois element is not valid" unless elt is odd and below 2N; with a null context only the oddness, which needs
// none, is tested (the entry points that refuse an even element before they look at the context)
int galois_elt_check(const moai_ctx *c, uint32_t elt);
// the last kernel of the unfused mod-down (moddown_finalize_kernel), for keyswitch.hip's small rings and for hybrid.hip:
// out [P][Lout][N] = addend + (acc - u) * inv[i] mod q_i with acc's row (p, i) at acc + (p * acc_stride + i) * N, u [P][Lout][N] in
// NTT form and inv[i] the Shoup pair of the divisor's inverse mod q_i (device memory); lst as in moddown
int moddown_finalize(moai_ctx *c, const uint64_t *acc, uint32_t acc_stride, const uint64_t *u, uint64_t *out, size_t P, size_t Lout,
                     const Tw *inv, const KsAddend &add, const KsList *lst, hipStream_t s);
// out [members][rows_per_member][N]: rows src_off_rows .. src_off_rows + rows_per_member - 1 of lst->ins[b], permuted by
// lst->tables[b]; lst is a device pointer (common.h KsList)
int galois_gather_list(moai_ctx *c, const KsList *lst, uint64_t *out, size_t members, size_t rows_per_member, size_t src_off_rows,
                       hipStream_t s);
// What the list forms of the key switches (moai_apply_galois_ptrs, moai_relinearize_ptrs and their hybrid counterparts) share
// (keyswitch.hip).  ks_list_write: one pass's record h goes to the device record d on stream s as a kernel argument
// (ks_list_write_kernel), never through a host-to-device copy.  ks_list_check_members: what needs no context -- "null list", then
// per member "member i: null pointer" and an even element; relin: one key for all, no elements.  ks_list_check_blocks: what needs the
// ring -- an element of 2N or more, then the overlaps: a member's output may be its input (not with relin) or its sum exactly, never a
// part of them, and never touches a block of another member; a member's input is in_bytes long, its output and its sum out_bytes
// (in_bytes >= out_bytes).
int ks_list_write(const KsList &h, KsList *d, hipStream_t s);
int ks_list_check_members(const uint64_t *const *ins, uint64_t *const *outs, const uint32_t *elts, const uint64_t *const *keys,
                          const uint64_t *one_key, size_t n, bool relin);
int ks_list_check_blocks(const moai_ctx *c, const uint64_t *const *ins, uint64_t *const *outs, const uint32_t *elts,
                         const uint64_t *const *sums, size_t n, size_t in_bytes, size_t out_bytes, bool relin);

// CKKSEncoder's tables (matrix_reps_index_map_, root_powers_, inv_root_powers_) on the device, built on first use under
// c->mutex (encoder.hip)
int ensure_ckks_tables(moai_ctx *c);
// ContextData::total_coeff_modulus_bit_count of the selected primes; 0, and no error set, when an index is out of range
// (encoder.hip)
int total_coeff_bits(const moai_ctx *c, size_t L, const uint32_t *prime_index);

// moai_rescale for a caller that already holds the context's op_mutex (client.hip): it uses the first
// rescale_ws_bytes(c, L, batch * size) bytes of the stream's arena, the caller's own scratch lies behind them
size_t rescale_ws_bytes(const moai_ctx *c, size_t L, size_t polys);
int rescale_nolock(moai_ctx *c, const uint64_t *in, uint64_t *out, size_t size, size_t L, size_t batch, hipStream_t s);

// moai_encrypt_symmetric of n_batch zeros over all k rows for another translation unit (hybrid.hip's key digits): the same
// validation and stream positions, not traced; takes op_mutex itself
int encrypt_zero_key_level(moai_ctx *c, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, uint64_t *out, size_t n_batch,
                           hipStream_t s);

// moai_seal_sample_uniform for a caller that has validated its arguments and holds op_mutex (client.hip's SEAL-seeded entry
// points): polynomial b of `count` lands at out + b * stride_words; cnt is device scratch [count][L] that the call zeroes itself
// (sealprng.hip)
int seal_uniform_launch(moai_ctx *c, const uint8_t *seeds, uint64_t *out, size_t stride_words, size_t count, size_t L,
                        const RowMap &rows, uint32_t *cnt, uint32_t *rejected, hipStream_t s);

} // namespace moai
