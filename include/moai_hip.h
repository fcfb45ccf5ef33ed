/*
 * moai_hip.h -- C ABI of the MI355X-native RNS-CKKS evaluator hot path.
 *
 * This is the drop-in boundary: everything MOAI's seal::Evaluator needs for ciphertext arithmetic,
 * as plain C entry points over device pointers.  The host-side seal:: shim (and any other binding:
 * ctypes, cgo, JNI) sits above this header; nothing below it is visible to callers.
 *
 * Each entry point names the reference interface it replaces.  Paths are relative to the
 * reference checkout; SEAL/ = thirdparty/SEAL-4.1-bs/native/src/seal/.
 *
 * Conventions
 *   - All residue data is uint64_t in the reference's own layout [poly][rns prime][coefficient]
 *     (SEAL/ciphertext.h:337-349), with an optional leading batch dimension.  Pointers are DEVICE
 *     pointers unless a parameter is documented "host".
 *   - Inputs are canonical residues in [0, q_i); outputs are canonical residues, bit-identical to
 *     the reference CPU path on the same inputs.
 *   - A data level with L primes uses context primes [0, L); the key level is all k primes and
 *     prime k-1 is the special prime (SEAL/context.cpp:455-522).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls enqueue work and
 *     return; they never synchronise the device.  Workspace is drawn from the context's arena,
 *     which grows (hipMalloc) only outside stream capture -- call moai_ctx_reserve first when
 *     capturing into a hipGraph.
 *   - Return value: 0 on success, a negative MOAI_E* code otherwise; moai_last_error() gives the
 *     message (thread local).  No exceptions cross this boundary: the C++ shim re-creates the
 *     reference's exceptions (std::invalid_argument / std::logic_error / std::out_of_range)
 *     BEFORE enqueueing, as the reference raises them synchronously.
 */
#ifndef MOAI_HIP_H
#define MOAI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOAI_OK 0
#define MOAI_EINVAL (-1)   /* bad argument (the shim maps it to std::invalid_argument) */
#define MOAI_ELOGIC (-2)   /* unsupported parameters (std::logic_error)                */
#define MOAI_ERANGE (-3)   /* index out of range (std::out_of_range)                   */
#define MOAI_EHIP (-4)     /* HIP runtime failure                                      */
#define MOAI_ENOMEM (-5)

#define MOAI_MAX_RNS 64    /* largest number of RNS rows one call may address */

typedef struct moai_ctx moai_ctx;

const char *moai_last_error(void);
int moai_version(void);

/* ---- context: per-prime tables on the device -------------------------------------------------
 * Replaces SEALContext's per-level ContextData precomputation for the hot path
 * (SEAL/context.cpp:422-522, NTTTables::initialize SEAL/util/ntt.cpp:241-300, RNSTool
 * inv_q_last_mod_q SEAL/util/rns.cpp:769-775, Modulus::const_ratio SEAL/modulus.cpp:36-77).
 * Tables are shared per prime, not duplicated per level.  primes: host, k entries, each an NTT
 * prime (= 1 mod 2N) below 2^61.  coeff_count_power in [1, 16].
 */
int moai_ctx_create(int coeff_count_power, const uint64_t *primes, size_t k, int device, moai_ctx **out);
void moai_ctx_destroy(moai_ctx *ctx);
int moai_ctx_reserve(moai_ctx *ctx, size_t workspace_bytes); /* arena of the default (NULL) stream */
/* arena of `stream`: call before capturing that stream into a hipGraph (arenas never grow under capture) */
int moai_ctx_reserve_stream(moai_ctx *ctx, void *stream, size_t workspace_bytes);
size_t moai_ctx_coeff_count(const moai_ctx *ctx);
size_t moai_ctx_prime_count(const moai_ctx *ctx);
/* psi = minimal primitive 2N-th root of prime i (NTTTables::get_root) */
uint64_t moai_ctx_root(const moai_ctx *ctx, size_t prime);
/* prime i of the context as moai_ctx_create received it; 0 when i is out of range */
uint64_t moai_ctx_prime(const moai_ctx *ctx, size_t prime);

/* ---- memory / streams (the device arena behind seal::DynArray / MemoryPool, SEAL/dynarray.h) -- */
int moai_malloc(void **dptr, size_t bytes);
/* page-locked host memory: copies from it are asynchronous for real (staging buffers of host-side callers) */
int moai_host_malloc(void **hptr, size_t bytes);
int moai_host_free(void *hptr);
int moai_free(void *dptr);
int moai_memcpy_h2d(void *dst, const void *src_host, size_t bytes, void *stream);
int moai_memcpy_d2h(void *dst_host, const void *src, size_t bytes, void *stream);
int moai_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
/* n <= 64 separate device blocks of `words` 64-bit words (even) each <-> one packed array [n][words], in ONE launch: what the shim's
 * call combiner does around a batched operation (it used to enqueue one copy per caller and direction).  src / dst: HOST arrays of
 * device pointers.  No counterpart in the reference (plumbing of SURVEY 8 row f4). */
int moai_gather_blocks(moai_ctx *ctx, const uint64_t *const *src, uint64_t *packed, size_t n, size_t words, void *stream);
int moai_scatter_blocks(moai_ctx *ctx, const uint64_t *packed, uint64_t *const *dst, size_t n, size_t words, void *stream);
int moai_memset_zero(void *dst, size_t bytes, void *stream);
int moai_stream_create(void **stream);
int moai_stream_destroy(void *stream);
int moai_stream_sync(void *stream);

/* ---- negacyclic NTT ----------------------------------------------------------------------------
 * data: uint64[n_poly][L][N] in place.  Row (p, r) is transformed under context prime
 * prime_index[r] (host array of L entries) or prime r when prime_index is NULL.
 * forward:  natural order in (values in [0, 4q), as the reference's lazy transform accepts) -> bit-reversed
 *           order out, canonical [0,q)
 *           (ntt_negacyclic_harvey, SEAL/util/ntt.cpp:408-437; Evaluator::transform_to_ntt_inplace
 *           SEAL/evaluator.cpp:2468-2514)
 * inverse:  bit-reversed in -> natural out, scaled by N^-1, canonical
 *           (inverse_ntt_negacyclic_harvey, SEAL/util/ntt.cpp:453-475;
 *           Evaluator::transform_from_ntt_inplace SEAL/evaluator.cpp:2516-2561)
 *           Input range: every row accepts [0, 2q), what the reference's lazy inverse accepts (dwthandler.h:226-250).
 *           Per class of row (moai_arith_mode, MOAI_MODE_OF_NTT_INVERSE), N >= 4096, the kernels accept no more than
 *             FPN, FPR        any value below 2^52 (the load converts with an exact 52-bit trick, csrc/modarith.hip.h
 *                             fp_from_u52, which drops bits 52 and up; FPN folds it to |.| <= q/2 at once, FPR in its
 *                             first butterfly, whose sum of two inputs stays below 2^53) -- at least [0, 2q) as q < 2^51
 *             LAZY16, LAZY8   [0, 4q)
 *             GUARD           [0, 2q)
 *           Every internal caller (key switch, mod-down / rescale, hoisted rotations, mod-raise, decode) passes canonical rows.
 */
int moai_ntt_forward(moai_ctx *ctx, uint64_t *data, size_t n_poly, size_t L, const uint32_t *prime_index,
                     void *stream);
int moai_ntt_inverse(moai_ctx *ctx, uint64_t *data, size_t n_poly, size_t L, const uint32_t *prime_index,
                     void *stream);

/* ---- element-wise RNS polynomial arithmetic (SEAL/util/polyarithsmallmod.cpp) -------------------
 * All operate on uint64[n_poly][L][N] with row r under prime r; out may alias an input.
 */
/* add_poly_coeffmod :43-86 / Evaluator::add_inplace SEAL/evaluator.cpp:155-240 */
int moai_add(moai_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n_poly, size_t L,
             void *stream);
/* sub_poly_coeffmod :88-133 / Evaluator::sub_inplace SEAL/evaluator.cpp:263-350 */
int moai_sub(moai_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n_poly, size_t L,
             void *stream);
/* negate_poly_coeffmod polyarithsmallmod.h:77-106 / Evaluator::negate_inplace SEAL/evaluator.cpp:130-153 */
int moai_negate(moai_ctx *ctx, const uint64_t *a, uint64_t *out, size_t n_poly, size_t L, void *stream);
/*
 * dyadic_product_coeffmod :226-278.  a: [n_poly][L][N]; b: [n_poly_b][L][N] with n_poly_b == n_poly
 * or n_poly_b == 1 (broadcast: Evaluator::multiply_plain_ntt SEAL/evaluator.cpp:2336-2373 multiplies
 * every ciphertext polynomial by the one plaintext).
 */
int moai_dyadic_mul(moai_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n_poly,
                    size_t n_poly_b, size_t L, void *stream);
/*
 * multiply_poly_scalar_coeffmod :197-224 with one scalar per RNS row (host array scalars[L], any
 * uint64; reduced mod q_r first like polyarithsmallmod.h:209-217).  This is multiply_plain by a
 * scalar-encoded plaintext, whose rows are constant (SEAL/ckks.cpp:131-150), without materialising
 * N*L words.
 */
int moai_mul_scalar_rows(moai_ctx *ctx, const uint64_t *a, const uint64_t *scalars, uint64_t *out, size_t n_poly,
                         size_t L, void *stream);
/* add_poly_scalar_coeffmod :135-164, one scalar per row (add_plain of a scalar-encoded plaintext
 * touches polynomial 0 only: Evaluator::add_plain_inplace SEAL/evaluator.cpp:2014-2018). */
int moai_add_scalar_rows(moai_ctx *ctx, const uint64_t *a, const uint64_t *scalars, uint64_t *out, size_t n_poly,
                         size_t L, void *stream);
/* Multiplication by the monomial X^(N/2), which is the slot-wise constant i of a CKKS ciphertext, on rows in NTT form:
 *     out = a + sign * X^(N/2) * b,  sign = +1 or -1;  a == NULL gives the plain product.  out may alias a or b.
 * The product is negacyclic_multiply_poly_mono_coeffmod (SEAL/util/polyarithsmallmod.h:634-655) composed with
 * ntt_negacyclic_harvey (SEAL/util/ntt.cpp:408-437): in the transform's output order X^(N/2) is +psi^(N/2) on indices
 * [0, N/2) and -psi^(N/2) on [N/2, N), so no plaintext is encoded or read.  With a given it is the `multiply_plain` by the
 * encoded constant i followed by `add` of include/source/bootstrapping/Bootstrapper.cpp:2760-2777.  Canonical residues in and
 * out, primes of at most 61 bits. */
int moai_mul_i_add(moai_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n_poly, size_t L, int sign,
                   void *stream);
/* Real and imaginary part of a ciphertext r given its conjugate rbar (both [n_poly][L][N], NTT form), up to the factor 2:
 *     out_re = r + rbar,   out_im = -X^(N/2) * (r - rbar)
 * in one pass: the `add_inplace_reduced_error(rtn, conj)` that ends bootstrap_full_real_3
 * (include/source/bootstrapping/Bootstrapper.cpp:3347-3350; Evaluator::add_inplace SEAL/evaluator.cpp:155-240) and its
 * counterpart for the imaginary part (sub_poly_coeffmod, SEAL/util/polyarithsmallmod.cpp:88-133, then the monomial product
 * above).  out_re may alias r and out_im may alias rbar; no other overlap. */
int moai_real_split(moai_ctx *ctx, const uint64_t *r, const uint64_t *rbar, uint64_t *out_re, uint64_t *out_im, size_t n_poly,
                    size_t L, void *stream);

/* out = base + sum_{t < terms} x[t] (*) scalars[t]   -- the accumulation chain of MOAI's column-packed ct x pt product
 * (include/source/matrix_mul/Ct_pt_matrix_mul.hpp:19-42: Evaluator::multiply_plain by a scalar-encoded plaintext,
 * SEAL/evaluator.cpp:2336-2373 with SEAL/ckks.cpp:131-150, then Evaluator::add_inplace, :155-240, once per row of W) as one
 * pass per sixteen terms.  x: HOST array of `terms` device pointers, each [size][L][N]; scalars: HOST [terms][L], the plaintexts'
 * constant rows, reduced; base: device [size][L][N] or NULL (may be `out`); out: device [size][L][N], not one of the terms.
 * Canonical residues out: the same bits as the reference's `terms` products and sums. */
int moai_scalar_dot(moai_ctx *ctx, const uint64_t *const *x, const uint64_t *scalars, size_t terms, const uint64_t *base,
                    uint64_t *out, size_t size, size_t L, void *stream);
/* The same chain with full plaintexts (MOAI's masked products, Ct_pt_matrix_mul.hpp:103-170: multiply_plain_ntt's dyadic
 * product, SEAL/evaluator.cpp:2336-2373, then add_inplace): out = base + sum_t x[t] (*) p[t].  x: HOST array of device
 * pointers as above; p: DEVICE [terms][L][N], the plaintexts back to back in NTT form (moai_ckks_encode_masked writes them so). */
int moai_vector_dot(moai_ctx *ctx, const uint64_t *const *x, const uint64_t *p, size_t terms, const uint64_t *base, uint64_t *out,
                    size_t size, size_t L, void *stream);
/* ... and for ciphertext operands: out[3][L][N] = base + sum_t multiply(x[t], y[t]) with size-2 operands in separate blocks
 * (Evaluator::multiply's ckks_multiply, SEAL/evaluator.cpp:770-909, then add_inplace: the inner loops of MOAI's
 * Ct_ct_matrix_mul.hpp:32-41 and :121-134).  x, y: HOST arrays of `terms` device pointers; base: device [3][L][N] or NULL. */
int moai_ct_dot_ptrs(moai_ctx *ctx, const uint64_t *const *x, const uint64_t *const *y, size_t terms, const uint64_t *base, uint64_t *out,
                     size_t L, void *stream);

/* ---- ciphertext products -------------------------------------------------------------------------
 * Evaluator::ckks_multiply SEAL/evaluator.cpp:770-909, size 2 x size 2 -> size 3:
 * out[b] = (x0*y0, x0*y1 + x1*y0, x1*y1).  x, y: [batch][2][L][N]; out: [batch][3][L][N]
 * (out must not alias x or y).
 */
int moai_ct_multiply(moai_ctx *ctx, const uint64_t *x, const uint64_t *y, uint64_t *out, size_t L, size_t batch,
                     void *stream);
/* Evaluator::ckks_square SEAL/evaluator.cpp:1223-1282: (x0^2, 2 x0 x1, x1^2) */
int moai_ct_square(moai_ctx *ctx, const uint64_t *x, uint64_t *out, size_t L, size_t batch, void *stream);
/* Evaluator::multiply for operands of any size, SEAL/evaluator.cpp:862-900 (the dest_size != 3 branch of ckks_multiply):
 * out[b][k] = sum over i + j = k of x[b][i] (*) y[b][j], k < size_x + size_y - 1.
 * x: [batch][size_x][L][N]; y: [batch][size_y][L][N]; out: [batch][size_x + size_y - 1][L][N], not an operand.
 * Sizes 2..16, product at most 16 polynomials (SEAL_CIPHERTEXT_SIZE_MAX). For 2 x 2 moai_ct_multiply is the same result. */
int moai_ct_multiply_general(moai_ctx *ctx, const uint64_t *x, size_t size_x, const uint64_t *y, size_t size_y,
                             uint64_t *out, size_t L, size_t batch, void *stream);
/* sum over j < count of ckks_multiply(x[j], y[j]) (evaluator.cpp:805-860) accumulated with add_inplace
 * (:155-240): the inner loop of include/source/matrix_mul/Ct_ct_matrix_mul.hpp:33-42 and :117-131 in one pass.
 * x, y: [count][2][L][N]; out: [3][L][N].  Same canonical residues as the reference's multiply-reduce-add
 * sequence.  Primes of at most 61 bits (SEAL's own bound, util/defines.h:40). */
int moai_ct_dot(moai_ctx *ctx, const uint64_t *x, const uint64_t *y, uint64_t *out, size_t count, size_t L,
                void *stream);
/* out[poly] = sum over t < terms of multiply_plain(x[x_index[t]][poly], p[p_index[t]]) (evaluator.cpp:2336-2373)
 * accumulated with add_inplace: the inner loop of the baby-step / giant-step linear transforms of MOAI's
 * bootstrapping (include/source/bootstrapping/Bootstrapper.cpp:2028-2046, 2095-2113) for a whole batch.
 * x: operands, operand k = x + k * n_poly * L * N, each [n_poly][L][N] (n_poly = batch * ciphertext size);
 * p: plaintexts in NTT form, [n_pt][L][N], shared by the batch; out: [n_poly][L][N]; x_index / p_index: host
 * arrays.  terms <= 64.  Same canonical residues as the reference's multiply-reduce-add sequence. */
int moai_ct_pt_dot(moai_ctx *ctx, const uint64_t *x, const uint64_t *p, uint64_t *out, const uint32_t *x_index,
                   const uint32_t *p_index, size_t terms, size_t n_poly, size_t L, void *stream);
/* Two such sums over the same operands in one pass -- two giant steps of one transform (Bootstrapper.cpp:2024-2062): every
 * baby-step ciphertext is read once for both.  out = sum over t < terms of x[x_index[t]] (.) p[p_index[t]];
 * out2 = sum over t < terms2 <= terms of x[x_index[t]] (.) p[p_index2[t]] (the last giant step of a transform is shorter).
 * The same residues as two moai_ct_pt_dot calls. */
int moai_ct_pt_dot2(moai_ctx *ctx, const uint64_t *x, const uint64_t *p, uint64_t *out, uint64_t *out2,
                    const uint32_t *x_index, const uint32_t *p_index, const uint32_t *p_index2, size_t terms, size_t terms2,
                    size_t n_poly, size_t L, void *stream);
/* out = sum over ALL r < rows of multiply_plain(x[r], p[r]) accumulated with add_inplace: one output column of
 * ct_pt_matrix_mul_wo_pre_w_mask (include/source/matrix_mul/Ct_pt_matrix_mul.hpp:120-150, every weight a full plaintext),
 * any number of rows in one call; with p2 / out2 (both or neither) a second column over the same ciphertexts in the same
 * pass.  x: [rows][n_poly][L][N]; p, p2: [rows][L][N] in NTT form; out, out2: [n_poly][L][N].  The sum is split over
 * workgroups and folded by a second small kernel (exact: every partial sum is a canonical residue).  Same residues as the
 * reference's multiply-reduce-add sequence. */
int moai_ct_pt_dot_rows(moai_ctx *ctx, const uint64_t *x, const uint64_t *p, const uint64_t *p2, uint64_t *out, uint64_t *out2,
                        size_t rows, size_t n_poly, size_t L, void *stream);

/*
 * Column-packed ciphertext x plaintext matrix product with scalar-encoded weights: the body of
 * ct_pt_matrix_mul_wo_pre (include/source/matrix_mul/Ct_pt_matrix_mul.hpp:4-49, :51-101) before its
 * rescale, i.e. out[c] = sum_j multiply_plain(X[j], encode(W[j][c])) for every output column c.
 * x: [rows][size][L][N]; w: DEVICE array uint64[L][rows][cols], w[r][j][c] = the residue under prime r
 * of the scalar plaintext CKKSEncoder::encode(W[j][c], scale) (SEAL/ckks.cpp:101-150), canonical;
 * out: [cols][size][L][N] (must not alias x).  Follow with moai_rescale(out, ..., batch = cols).
 */
int moai_ct_pt_matmul(moai_ctx *ctx, const uint64_t *x, const uint64_t *w, uint64_t *out, size_t rows, size_t cols,
                      size_t size, size_t L, void *stream);

/* ---- level changes ---------------------------------------------------------------------------------
 * Evaluator::rescale_to_next SEAL/evaluator.cpp:1682-1720 -> mod_switch_scale_to_next :1402-1481 ->
 * RNSTool::divide_and_round_q_last_ntt_inplace SEAL/util/rns.cpp:830-901.
 * in: [batch][size][L][N] -> out: [batch][size][L-1][N]; in is preserved; out may not alias in.
 */
int moai_rescale(moai_ctx *ctx, const uint64_t *in, uint64_t *out, size_t size, size_t L, size_t batch,
                 void *stream);
/* multiply_plain by a scalar plaintext (moai_mul_scalar_rows) followed by moai_rescale, in one pass over the
 * ciphertext: Evaluator::multiply_const + rescale_to_next_inplace of the fork (SEAL/evaluator.cpp:395-418,
 * :1682-1720), the pair the *_reduced_error compositions and MOAI's polynomial evaluations issue for every
 * coefficient.  Same residues as the two calls.  in: [batch][size][L][N], scalars[L] (host), out: [batch][size][L-1][N]. */
int moai_mul_scalar_rescale(moai_ctx *ctx, const uint64_t *in, const uint64_t *scalars, uint64_t *out, size_t size,
                            size_t L, size_t batch, void *stream);
/* moai_rescale / moai_mul_scalar_rescale followed by Evaluator::add_inplace (SEAL/evaluator.cpp:155-240) of `addend`, the
 * addition done by the rescale's last kernel: what add_[inplace_]reduced_error of the fork issues after its level adjustment
 * (SEAL/evaluator.cpp:447-480) and MOAI's polynomial evaluations issue per coefficient (rescale, then add to the running sum).
 * Same residues as the separate calls.  addend: [batch][size][L-1][N], may be `out` itself (accumulate in place). */
int moai_rescale_add(moai_ctx *ctx, const uint64_t *in, const uint64_t *addend, uint64_t *out, size_t size, size_t L,
                     size_t batch, void *stream);
int moai_mul_scalar_rescale_add(moai_ctx *ctx, const uint64_t *in, const uint64_t *scalars, const uint64_t *addend,
                                uint64_t *out, size_t size, size_t L, size_t batch, void *stream);
/* Evaluator::mod_switch_drop_to_next SEAL/evaluator.cpp:1483-1546 applied `drop` times:
 * in: [batch][size][L][N] -> out: [batch][size][L-drop][N].  out must not alias in (except batch*size == 1,
 * where the kept rows already are in place). */
int moai_mod_drop(moai_ctx *ctx, const uint64_t *in, uint64_t *out, size_t size, size_t L, size_t drop,
                  size_t batch, void *stream);

/* ---- Galois automorphism and key switching -----------------------------------------------------------
 * GaloisTool::apply_galois_ntt SEAL/util/galois.cpp:192-218 with the table of :18-51:
 * out[p][r][i] = in[p][r][table[i]].  galois_elt odd, < 2N.  out must not alias in.
 * One row per workgroup row like every elementwise entry point: n_poly * L above 65535 is MOAI_EINVAL.
 */
int moai_galois_permute(moai_ctx *ctx, const uint64_t *in, uint64_t *out, size_t n_poly, size_t L,
                        uint32_t galois_elt, void *stream);
/* GaloisTool::get_elt_from_step SEAL/util/galois.cpp:53-95 (generator 5 in this fork,
 * SEAL/util/galois.h:169).  Returns 0 and sets the error for |step| >= N/2. */
uint32_t moai_galois_elt_from_step(const moai_ctx *ctx, int step);
/*
 * Evaluator::switch_key_inplace SEAL/evaluator.cpp:2724-3020 (CKKS branch):
 *   ct[b] (2 polys, NTT form, L primes) += ModDown_p( sum_J NTT_{q_I}([INTT(target[b]_J)]_{q_I}) (*) key[J][.][I] )
 * ct: [batch][2][L][N] in place; target: [batch][L][N] (NTT form, not modified);
 * key: uint64[k-1][2][k][N] -- the reference's KSwitchKeys entry, vector<PublicKey> of k-1 size-2
 * ciphertexts at the key level (SEAL/kswitchkeys.h:340, keygenerator.cpp:303-336) flattened.
 * Every ciphertext of the batch is switched with the same key.
 */
int moai_switch_key(moai_ctx *ctx, uint64_t *ct, const uint64_t *target, const uint64_t *key, size_t L,
                    size_t batch, void *stream);
/* Evaluator::relinearize_internal SEAL/evaluator.cpp:1345-1400 for size 3 -> 2:
 * ct3: [batch][3][L][N]; out: [batch][2][L][N] (may not alias ct3). */
int moai_relinearize(moai_ctx *ctx, const uint64_t *ct3, const uint64_t *relin_key, uint64_t *out, size_t L,
                     size_t batch, void *stream);
/* Evaluator::apply_galois_inplace SEAL/evaluator.cpp:2563-2665 (rotate_vector / complex_conjugate
 * with the key present, rotate_internal :2667-2697): ct: [batch][2][L][N] in place. */
int moai_apply_galois(moai_ctx *ctx, uint64_t *ct, size_t L, uint32_t galois_elt, const uint64_t *galois_key,
                      size_t batch, void *stream);
/* The same with a separate destination (Evaluator::apply_galois / rotate_vector / complex_conjugate with a
 * `destination`, SEAL/evaluator.h:1093-1101, 1191-1227, 1262-1270: "destination = encrypted; ..._inplace(destination)"
 * without the deep copy): in, out: [batch][2][L][N]; out may be in. */
int moai_apply_galois_to(moai_ctx *ctx, const uint64_t *in, uint64_t *out, size_t L, uint32_t galois_elt,
                         const uint64_t *galois_key, size_t batch, void *stream);
/* acc = add_inplace(acc, apply_galois(in)): a rotation whose result is added to a running sum, the pair
 * rotate_vector + add_inplace_reduced_error (equal levels) of the giant steps of Bootstrapper::bsgs_linear_transform
 * (include/source/bootstrapping/Bootstrapper.cpp:2049-2059); the addition rides on the key switch's last kernel.
 * in, acc: [batch][2][L][N], distinct.  Same residues as moai_apply_galois_to followed by moai_add. */
int moai_apply_galois_acc(moai_ctx *ctx, const uint64_t *in, uint64_t *acc, size_t L, uint32_t galois_elt,
                          const uint64_t *galois_key, size_t batch, void *stream);
/* Key switches on a LIST of single ciphertexts, each in its own block with its own Galois element and key:
 * outs[i] = [sums[i] +] apply_galois(ins[i], galois_elts[i], galois_keys[i]), i < n -- n calls of moai_apply_galois_to /
 * moai_apply_galois_acc (Evaluator::apply_galois_inplace, SEAL/evaluator.cpp:2563-2665, switch_key_inplace :2724-3020) in one
 * chain of launches, bit-identical to them.  What the differently rotated ciphertexts of MOAI's OpenMP loops
 * (include/source/matrix_mul/Ct_ct_matrix_mul.hpp:22-31, 84-102, 142-149) need to share launches: the batch forms above take
 * one contiguous block and one key.  The members' keys may have different layouts (whole, moai_key_trim'med or born limited).
 *   ins / outs / galois_keys / sums: HOST arrays of n device pointers, each member [2][L][N]; sums may be NULL, and so may
 *   any sums[i].  outs[i] may be ins[i] or sums[i]; otherwise no output may overlap any member's input, output or sum.
 * Any n: 64 members per pass.  Nothing is enqueued when an argument is refused: MOAI_EINVAL for a null list or member, an even
 * element or one >= 2N, or an overlap; MOAI_ERANGE, naming the member, for a key limited below L.  n == 0 is MOAI_OK.  The
 * call does not synchronise.  moai_op_trace counts it as n units of "apply_galois_to". */
int moai_apply_galois_ptrs(moai_ctx *ctx, const uint64_t *const *ins, uint64_t *const *outs, size_t L, const uint32_t *galois_elts,
                           const uint64_t *const *galois_keys, const uint64_t *const *sums, size_t n, void *stream);
/* outs[i] = relinearize(ct3s[i]) with one key: n calls of moai_relinearize(..., batch 1) (Evaluator::relinearize_internal,
 * SEAL/evaluator.cpp:1345-1400) in one chain of launches, bit-identical to them.  ct3s / outs: HOST arrays of n device
 * pointers, ct3s[i] [3][L][N], outs[i] [2][L][N]; no output may overlap any member's input or output.  Errors, n and tracing
 * ("relinearize") as above. */
int moai_relinearize_ptrs(moai_ctx *ctx, const uint64_t *const *ct3s, uint64_t *const *outs, const uint64_t *relin_key, size_t L,
                          size_t n, void *stream);

/* ---- MOAI-owned integer kernel ---------------------------------------------------------------------------
 * Bootstrapper::modraise_inplace include/source/bootstrapping/Bootstrapper.cpp:2938-2992:
 * in: [batch][2][1][N] (NTT form under prime 0) -> out: [batch][2][L_out][N] (NTT form). */
int moai_modraise(moai_ctx *ctx, const uint64_t *in, uint64_t *out, size_t L_out, size_t batch, void *stream);

/* ---- CKKS encoder ---------------------------------------------------------
 * CKKSEncoder::encode_internal, vector form, SEAL/ckks.h:457-637, for n_batch value vectors in one call:
 * scatter into the conjugate-symmetric slot vector (matrix_reps_index_map_, ckks.cpp:34-52, generator 5),
 * FP64 inverse DWT with scale / N folded into the last stage (util/dwthandler.h:202-356 on
 * std::complex<double>, every product and sum rounded separately as the reference's x86-64 build does),
 * std::round, exact residues of the rounded integers, forward NTT.
 *   values     device, [n_batch][values_size] doubles (is_complex = 0) or (re, im) pairs (is_complex = 1);
 *              values_size <= N/2, shorter vectors are zero-padded like the reference
 *   dst        device, [n_batch][L][N], rows over context primes prime_index[0..L) (NULL = 0..L-1), NTT form
 *   max_coeff  device, [n_batch] doubles, or NULL: max |coefficient| before rounding, i.e. the quantity
 *              ckks.h:527-538 turns into max_coeff_bit_count; the caller compares it with
 *              moai_total_coeff_modulus_bit_count to raise "encoded values are too large"
 * The three decomposition branches of the reference (<= 64 bits, <= 128 bits, multi-word) all produce the
 * exact integer modulo each prime; so does the single device routine.
 * Errors: MOAI_EINVAL "values_size is too large" / "scale out of bounds" (ckks.h:469-497). */
int moai_ckks_encode(moai_ctx *ctx, const double *values, int is_complex, size_t values_size, size_t n_batch,
                     uint64_t *dst, size_t L, const uint32_t *prime_index, double scale, double *max_coeff,
                     void *stream);
/* The same for vectors of the form MOAI's masked matrix products encode
 * (include/source/matrix_mul/Ct_pt_matrix_mul.hpp:124-146): values[b][s] = constants[b] where mask[s] == 1, else
 * 0, for s < mask_size (the rest zero-padded).  constants: device, [n_batch] doubles; mask: device, [mask_size]
 * int32 (MOAI's bias_vec).  Saves building and uploading n_batch * N/2 doubles; same residues as
 * moai_ckks_encode on the expanded vectors. */
int moai_ckks_encode_masked(moai_ctx *ctx, const double *constants, const int32_t *mask, size_t mask_size,
                            size_t n_batch, uint64_t *dst, size_t L, const uint32_t *prime_index, double scale,
                            double *max_coeff, void *stream);
/* ---- decrypt and decode (the client's output path) ---------------------------------------------------------------
 * moai_decrypt: out[b] = sum_{i < size} ct[b][i] * s^i mod q_r in NTT form, one launch for the batch (s^i formed in
 * registers).  ct: device [n_batch][size][L][N], size >= 2; sk_ntt: device [L][N], the secret key's rows under the same
 * primes as the ciphertext's rows (prime_index[0..L), NULL = 0..L-1: the first L rows of a full [k][N] key); out: device
 * [n_batch][L][N], canonical residues.
 * moai_ckks_decode: for each of n_batch NTT-form plaintexts [L][N] (plain_ntt, device, never modified): inverse NTT of a
 * scratch copy, exact CRT composition, the reference's word-by-word conversion to double with 1/scales[b] (sign by
 * upper_half_threshold, no borrow between words, zero words skipped), forward DWT with root_powers_, and the
 * matrix_reps_index_map_ gather of all N/2 slots -- bit-identical to the reference's x86-64 build.  scales: HOST array
 * [n_batch], read during the call.  out: device [n_batch][N/2] doubles (is_complex = 0, real parts) or [n_batch][N/2][2]
 * (re, im).  Large batches are processed in chunks whose scratch fits the stream's arena or MOAI_DEC_TMP_MB (default
 * 1024 MiB), whichever is larger.  Errors (before anything is enqueued): MOAI_EINVAL "scale out of bounds" when
 * scale <= 0 or (int)log2(scale) >= total_coeff_modulus_bit_count (ckks.h:672-677; a non-finite scale too).
 * moai_ckks_decode_sparse: the same with the reference's sparse_slots_ (ckks.h:703-713, :757-760): after the CRT composition
 * every coefficient i with i mod (N/2 / sparse_slots) != 0 is zeroed (its double is +0.0), the conversion and the full-length
 * forward DWT run as above, and the gather returns the first sparse_slots entries.  out: device [n_batch][sparse_slots]
 * doubles or [n_batch][sparse_slots][2].  sparse_slots == N/2 gives exactly the bits of moai_ckks_decode.  Errors (before
 * anything is enqueued): MOAI_EINVAL when sparse_slots is not a power of two in [1, N/2], and those of moai_ckks_decode.
 * Neither call synchronises. */
/* Decryptor::ckks_decrypt, SEAL/decryptor.cpp:154-187 with dot_product_ct_sk_array :299-381 */
int moai_decrypt(moai_ctx *ctx, const uint64_t *ct, size_t size, const uint64_t *sk_ntt, uint64_t *out,
                 size_t n_batch, size_t L, const uint32_t *prime_index, void *stream);
/* CKKSEncoder::decode_internal, SEAL/ckks.h:644-761 (full slots) */
int moai_ckks_decode(moai_ctx *ctx, const uint64_t *plain_ntt, size_t n_batch, size_t L,
                     const uint32_t *prime_index, const double *scales /* host, [n_batch] */,
                     int is_complex, double *out /* device, [n_batch][N/2] or [n_batch][N/2][2] */, void *stream);
/* CKKSEncoder::decode_internal with sparse_slots_ != slots_, SEAL/ckks.h:644-761 */
int moai_ckks_decode_sparse(moai_ctx *ctx, const uint64_t *plain_ntt, size_t n_batch, size_t L,
                            const uint32_t *prime_index, const double *scales /* host, [n_batch] */, size_t sparse_slots,
                            int is_complex, double *out /* device, [n_batch][sparse_slots] or [..][2] */, void *stream);
/* ContextData::total_coeff_modulus_bit_count (SEAL/context.cpp:169-173): significant bits of the product of
 * the L primes; 0 on error. */
int moai_total_coeff_modulus_bit_count(const moai_ctx *ctx, size_t L, const uint32_t *prime_index);
/* The tables the encoder uses, for inspection by tests: matrix_reps_index_map_ (host copy, N entries) and
 * inv_root_powers_ (host copy, N (re, im) pairs; ckks.cpp:54-71 via util/croots.cpp). */
int moai_ckks_tables(moai_ctx *ctx, uint32_t *index_map, double *inv_root_powers);

/* ---- client randomness and encryption (the client's input path) --------------------------------------------------
 * Stream contract.  Generator: ChaCha20, the RFC 8439 block function (20 rounds), state words 0-3 "expand 32-byte k", 4-11
 * the 32-byte key (little-endian words), 12-13 a 64-bit block counter (low word first), 14-15 a 64-bit nonce (low word first)
 * -- the layout of the host seal::util::ChaCha20Rng(seed) with seed = key || nonce (8 bytes, little endian).  The stream of
 * (key, nonce) is the sequence of 64-bit words  W[w] = o[2j] | o[2j+1] << 32  where o[16] is the output of block c = w / 8
 * (counter c) and j = w % 8.  A sample depends on (key, nonce, coefficient index) only, never on launch geometry.
 *   uniform mod q_r   row r, coefficient i of an [L][N] draw: (W[2(rN+i)+1] * 2^64 + W[2(rN+i)]) mod q_r, exactly (a Barrett
 *                     reduction of the 128-bit value with Modulus::const_ratio; statistical distance from uniform < 2^-67)
 *   ternary           coefficient i: ((3 * W[i]) >> 64) - 1 in {-1, 0, 1}                     (sample_poly_ternary)
 *   CBD noise         coefficient i: bytes x[0..5] of W[i] (x[0] least significant), x[2] and x[5] masked to 5 bits,
 *                     popcount(x0) + popcount(x1) + popcount(x2) - popcount(x3) - popcount(x4) - popcount(x5), i.e.
 *                     popcount(W & 0x1fffff) - popcount((W >> 24) & 0x1fffff): Binomial(42, 1/2) - 21, sigma = 3.24,
 *                     |e| <= 21  (sample_poly_cbd, SEAL/util/rlwe.cpp:99-135, SEAL 4.1's default noise sampler)
 *   RNS               a small signed sample v is ONE integer per coefficient, written in every requested row r as
 *                     v + (v < 0 ? q_r : 0)  (the reference's flag & q)
 * Samplers: polynomial p of a call uses nonce + p (the range [nonce, nonce + n_poly) must not wrap), out [n_poly][L][N] with
 * rows under prime_index (NULL = 0..L-1).  Splitting a draw into several calls with the matching nonces gives the same words.
 *
 * Compositions use 64-bit nonces  purpose << 56 | sequence  with sequence < 2^56 and the purposes
 *   1 uniform a (c1 of a symmetric encryption or key digit)   2 ternary u   3 noise e / e0   4 noise e1
 * Ciphertext (or key digit) b of a call with sequence base `seq` uses sequence seq + b; a call therefore occupies the
 * sequence range [seq, seq + n_batch) (key generation: [seq, seq + k - 1)), which must lie below 2^56.  Callers hand out
 * disjoint ranges per key (the seal:: shim's util::DeviceRng).  The key is read from HOST memory during the call.
 *
 * moai_encrypt_symmetric: per ciphertext, e = CBD(purpose 3) over the L rows, forward NTT, then one kernel that draws
 * c1 = a = uniform(purpose 1) over the same rows directly in NTT form and writes c0 = e - a * s (+ plain), c1 = a
 * (encrypt_zero_symmetric SEAL/util/rlwe.cpp:311-383 with is_ntt_form, then Encryptor::encrypt_symmetric's add_plain).
 * sk_ntt: [L][N] rows under the same primes as the output (NULL prime_index: the first L rows of a full [k][N] key).
 * plain: NULL or device [n_batch][L][N] NTT form.  out: device [n_batch][2][L][N].
 * moai_encrypt_asymmetric: public-key encryption at the data level of L primes (prefix 0..L-1), SEAL/encryptor.cpp:88-173:
 * with M = L + 1 primes (the previous level; M = L = k at the key level itself) u = ternary(purpose 2), e0 = CBD(3),
 * e1 = CBD(4) over M rows, forward NTT, c_i = pk_i * u + e_i over pk rows [0, M) (encrypt_zero_asymmetric,
 * SEAL/util/rlwe.cpp:224-310); below the key level the dropped prime is divided out exactly as moai_rescale does
 * (divide_and_round_q_last_ntt_inplace); then plain (NULL or [n_batch][L][N]) is added to c0.  pk: device [2][k][N] (the
 * key-level public key).  out: device [n_batch][2][L][N].
 * moai_kswitch_keygen: the k-1 digits of a switching key for new_key_ntt [k][N] under sk_ntt [k][N] at the key level: digit J
 * is the symmetric encryption of zero with sequence seq + J plus (q_{k-1} mod q_J) * new_key[J] in row J of c0
 * (KeyGenerator::generate_one_kswitch_key, SEAL/keygenerator.cpp:303-336).  out: device [k-1][2][k][N], the layout every
 * key-switch entry point above takes.
 * Large batches are processed in chunks whose scratch fits the stream's arena or 1 GiB (MOAI_CLIENT_TMP_KB), whichever is larger.  Arguments are
 * validated before anything is enqueued (MOAI_EINVAL with a message: null context / key / argument, "invalid level", a
 * sequence range beyond 2^56, more than 65535 ciphertexts; MOAI_ELOGIC for k < 2 in key generation).  No call synchronises. */
/* sample_poly_uniform SEAL/util/rlwe.cpp:137-183 (the stream above instead of rejection sampling) */
int moai_sample_uniform(moai_ctx *ctx, const uint8_t *key /* host, 32 bytes */, uint64_t nonce, uint64_t *out, size_t n_poly,
                        size_t L, const uint32_t *prime_index, void *stream);
/* sample_poly_ternary SEAL/util/rlwe.cpp:14-38 */
int moai_sample_ternary(moai_ctx *ctx, const uint8_t *key, uint64_t nonce, uint64_t *out, size_t n_poly, size_t L,
                        const uint32_t *prime_index, void *stream);
/* sample_poly_cbd SEAL/util/rlwe.cpp:99-135 */
int moai_sample_cbd(moai_ctx *ctx, const uint8_t *key, uint64_t nonce, uint64_t *out, size_t n_poly, size_t L,
                    const uint32_t *prime_index, void *stream);
/* Encryptor::encrypt_symmetric / encrypt_zero_symmetric, SEAL/encryptor.cpp:88-120 over SEAL/util/rlwe.cpp:311-383 */
int moai_encrypt_symmetric(moai_ctx *ctx, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, const uint64_t *plain,
                           uint64_t *out, size_t n_batch, size_t L, const uint32_t *prime_index, void *stream);
/* Encryptor::encrypt / encrypt_zero with a public key, SEAL/encryptor.cpp:88-173 over SEAL/util/rlwe.cpp:224-310 */
int moai_encrypt_asymmetric(moai_ctx *ctx, const uint8_t *key, uint64_t seq, const uint64_t *pk, const uint64_t *plain,
                            uint64_t *out, size_t n_batch, size_t L, void *stream);
/* KeyGenerator::generate_kswitch_keys for one new key, SEAL/keygenerator.cpp:303-336 */
int moai_kswitch_keygen(moai_ctx *ctx, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, const uint64_t *new_key_ntt,
                        uint64_t *out, void *stream);

/* ---- wire form: seeded objects and bit-packed rows ---------------------------------------------------------------------
 * What lets a ciphertext or a key leave the process that made it at 38 % of its resident size.  Both reductions are exact.
 *
 * Packed rows.  Row r of a polynomial under prime q_r, with b_r the bit length of q_r, is a little-endian bit stream:
 * coefficient i occupies bits [i b_r, (i + 1) b_r) of the row, bit j of the stream is bit (j mod 64) of 64-bit word j / 64;
 * every row starts on a word boundary and takes ceil(N b_r / 64) words (nothing is padded for N >= 64; for smaller N the padding
 * bits are zero).  Rows follow each other in the order of the unpacked layout [n_poly][L][N], rows under prime_index (NULL =
 * 0..L-1).  The reference has no such form: it leaves compression to zlib / zstd (SEAL/serialization.cpp:224-320).
 * moai_packed_words: the words of ONE packed polynomial, sum over r of ceil(N b_r / 64); host arithmetic, no launch; 0 on error.
 * moai_pack_rows: in [n_poly][L][N] (canonical residues; the low b_r bits of a word are stored) -> packed.
 * moai_unpack_rows: the inverse.  invalid: NULL or a device uint32_t that the kernel sets to non-zero when any unpacked value is
 * >= q_r (a b_r-bit field can hold one) and otherwise leaves alone -- the residue check of is_data_valid_for where the data is
 * (SEAL/valcheck.cpp:302-335, "ciphertext data is invalid" SEAL/ciphertext.cpp:302,358).  The caller zeroes it beforehand.
 * in / out and packed must not overlap and out must be 16-byte aligned (MOAI_EINVAL); b_r from 2 to 61 is supported.
 *
 * Seeded objects.  In a symmetric encryption and in every digit of a switching key the second polynomial is the uniform a,
 * a function of (key, nonce, coefficient index) only (stream contract above), so the wire form carries a seed in its place
 * (save_seed: SEAL/util/rlwe.cpp:334-385, SEAL/encryptor.cpp:89-248, SEAL/keygenerator.h:321-360).  moai_encrypt_symmetric and
 * moai_kswitch_keygen draw a and the noise from the SAME key, which therefore must stay secret; the seeded entry points take
 * TWO keys as the reference does (rlwe.cpp:353-363): the secret noise_key for e (purpose 3) and the public seed for a (purpose 1).
 * Only seed and the sequence number travel.  With noise_key == seed a seeded call followed by moai_expand_seeded reproduces the
 * unseeded entry point bit for bit.
 *   purpose 5  public seed: the seed of the object with sequence seq is the first 32 bytes (words W[0..3], little endian) of
 *              the stream (noise key, 5 << 56 | seq), computed on the host (seal::util::ChaCha20Rng); ChaCha20 output does not
 *              reveal its key.  Inside a seeded object sequences start at 0.
 *   purpose 6  SEAL seed: the 64-byte Blake2xb seed of the object (ciphertext or key digit) with sequence seq is words W[0..7],
 *              little endian, of the stream (noise key, 6 << 56 | seq), computed on the host as purpose 5 is; it feeds the
 *              SEAL-seeded entry points of the next section, whose objects SEAL itself expands.
 * moai_encrypt_symmetric_seeded: out_c0 [n_batch][L][N] = c0 exactly as moai_encrypt_symmetric computes it with a from
 * (seed, 1 << 56 | seq + b) and e from (noise_key, 3 << 56 | seq + b); c1 is not written.
 * moai_kswitch_keygen_seeded: the same for the k-1 digits of a switching key, out_c0 [k-1][k][N].
 * moai_expand_seeded: c0 [count][L][N] -> out [count][2][L][N] with out[b][0] = c0[b] and out[b][1] = uniform(seed,
 * 1 << 56 | seq + b) in NTT form, i.e. what moai_sample_uniform draws there: a ciphertext batch, or with count = k-1 and L = k a
 * switching key in the layout every key-switch entry point takes (Ciphertext::expand_seed, SEAL/ciphertext.cpp:118-188).  c0 and
 * out must not overlap.
 * Validation as above: MOAI_EINVAL with a message before anything is enqueued; no call synchronises. */
size_t moai_packed_words(const moai_ctx *ctx, size_t L, const uint32_t *prime_index);
/* the exact counterpart of Serialization::Save's compression step, SEAL/serialization.cpp:224-320 */
int moai_pack_rows(moai_ctx *ctx, const uint64_t *in, uint64_t *packed, size_t n_poly, size_t L, const uint32_t *prime_index,
                   void *stream);
/* Serialization::Load's decompression plus is_data_valid_for, SEAL/serialization.cpp:365-383, SEAL/valcheck.cpp:302-335 */
int moai_unpack_rows(moai_ctx *ctx, const uint64_t *packed, uint64_t *out, size_t n_poly, size_t L, const uint32_t *prime_index,
                     uint32_t *invalid /* device, or NULL */, void *stream);
/* encrypt_zero_symmetric with save_seed, SEAL/util/rlwe.cpp:311-385 under Encryptor::encrypt_symmetric SEAL/encryptor.cpp:89-248 */
int moai_encrypt_symmetric_seeded(moai_ctx *ctx, const uint8_t *noise_key /* host, 32 bytes */, const uint8_t *seed /* host, 32 bytes */,
                                  uint64_t seq, const uint64_t *sk_ntt, const uint64_t *plain, uint64_t *out_c0, size_t n_batch,
                                  size_t L, const uint32_t *prime_index, void *stream);
/* KeyGenerator::generate_one_kswitch_key with save_seed, SEAL/keygenerator.cpp:303-336, SEAL/keygenerator.h:321-360 */
int moai_kswitch_keygen_seeded(moai_ctx *ctx, const uint8_t *noise_key, const uint8_t *seed, uint64_t seq, const uint64_t *sk_ntt,
                               const uint64_t *new_key_ntt, uint64_t *out_c0, void *stream);
/* Ciphertext::expand_seed, SEAL/ciphertext.cpp:118-188 */
int moai_expand_seeded(moai_ctx *ctx, const uint8_t *seed, uint64_t seq, const uint64_t *c0, uint64_t *out, size_t count, size_t L,
                       const uint32_t *prime_index, void *stream);

/* ---- SEAL's own format: the generator of seeded objects ------------------------------------------------------------------
 * A SEAL client ships symmetric ciphertexts and switching keys seeded: one polynomial of data and a 64-byte seed from which
 * Ciphertext::expand_seed redraws the other with SEAL's default generator, Blake2xb in counter mode (buffer c of 4096 bytes is a
 * hash of (seed, c) alone).  These entry points are that generator and the sampler on top of it, bit for bit; the byte format
 * itself is host work (seal_shim/seal/moai_seal_format.h).  Shake256-seeded objects are not supported.  The same generator
 * serves the other direction: moai_encrypt_symmetric_seal_seeded and moai_kswitch_keygen_seal_seeded make objects whose uniform
 * half IS the expansion of a SEAL seed, so that what leaves this side seeded is what SEAL's own load expands.
 * moai_seal_prng_bytes: out (device, n_blocks * 4096 bytes, 16-byte aligned) = buffers first_block .. first_block + n_blocks - 1
 * of Blake2xbPRNG(seed).
 * moai_seal_sample_uniform: for every b < count, out + b * stride_words as [L][N] (rows under prime_index, NULL = 0..L-1) is
 * what sample_poly_uniform writes from a fresh Blake2xbPRNG(seeds[b]): the first L N little-endian words of the stream are the
 * candidates in row-major order; in row j a word is accepted iff it is below (2^64 - 1) - ((2^64 - 1) mod q_j) - 1 and then
 * reduced mod q_j; a rejected word is replaced by the next unread word of the same stream until one is accepted, rejections
 * served in order of row, then coefficient.  With stride_words = 2 L N and out pointing at polynomial 1 this fills c1 of a
 * batch of ciphertexts or of the digits of a switching key; no word outside the count targets is touched.  stride_words >= L N,
 * and even when count > 1; out 16-byte aligned; count >= 1.
 * rejected: NULL, or two device uint32_t that the caller zeroes: [0] is incremented by the number of stream words rejected,
 * [1] is set to 1 when a polynomial's replacements ran over the bound of 2 L N + 512 tail words (no loop on the device is
 * unbounded); the words not yet replaced then stay 2^64 - 1, which moai_check_residues reports.
 * moai_check_residues: sets *invalid (device, zeroed by the caller) to non-zero when a residue of data [n_poly][L][N] is >= its
 * prime, and otherwise leaves it alone: the flag of moai_unpack_rows for rows that arrive unpacked.
 * moai_encrypt_symmetric_seal_seeded: moai_encrypt_symmetric_seeded with a from SEAL's generator instead of ChaCha20: for
 * ciphertext b, a_b is exactly what moai_seal_sample_uniform writes for seeds[b] over the same rows (NTT form, as SEAL samples
 * it), e_b is the CBD draw of (noise_key, 3 << 56 | seq + b), word for word the noise of the ChaCha20-seeded call, and
 * out_c0[b] = NTT(e_b) - a_b * s (+ plain_b); c1 is never written.  One 64-byte seed per ciphertext, as Ciphertext::expand_seed
 * takes one generator per ciphertext (callers draw them under purpose 6 of the stream contract, or anywhere else).
 * moai_kswitch_keygen_seal_seeded: the same for the k-1 digits of a switching key, digit J from seeds[J] and sequence seq + J
 * plus (q_{k-1} mod q_J) * new_key[J] in row J; out_c0 [k-1][k][N].
 * Both expand a into scratch [chunk][L][N] beside the noise with the sampler's own kernels on the caller's stream and read it
 * back in the kernel that writes c0; a chunk's scratch is 2 L N words and L counters per ciphertext or digit, within the
 * stream's arena or 1 GiB as for the other client calls.  rejected: as in moai_seal_sample_uniform, the overflow word included.
 * Validation as above: MOAI_EINVAL with a message before anything is enqueued (a null seeds pointer is "null seed"); no call
 * synchronises. */
/* Blake2xbPRNG::refill_buffer, SEAL/randomgen.cpp:201-211 over blake2xb, SEAL/util/blake2xb.c:32-181 */
int moai_seal_prng_bytes(moai_ctx *ctx, const uint8_t *seed /* host, 64 bytes */, uint64_t first_block, uint64_t n_blocks, void *out,
                         void *stream);
/* sample_poly_uniform, SEAL/util/rlwe.cpp:137-166, with a generator per polynomial as in Ciphertext::expand_seed,
 * SEAL/ciphertext.cpp:118-151 */
int moai_seal_sample_uniform(moai_ctx *ctx, const uint8_t *seeds /* host, [count][64] */, uint64_t *out, size_t stride_words, size_t count,
                             size_t L, const uint32_t *prime_index, uint32_t *rejected /* device [2], or NULL */, void *stream);
/* is_data_valid_for's residue check, SEAL/valcheck.cpp:302-335 */
int moai_check_residues(moai_ctx *ctx, const uint64_t *data, size_t n_poly, size_t L, const uint32_t *prime_index, uint32_t *invalid,
                        void *stream);
/* encrypt_zero_symmetric with save_seed, SEAL/util/rlwe.cpp:311-385, a from Ciphertext::expand_seed's generator,
 * SEAL/ciphertext.cpp:118-151 */
int moai_encrypt_symmetric_seal_seeded(moai_ctx *ctx, const uint8_t *noise_key /* host, 32 bytes */,
                                       const uint8_t *seeds /* host, [n_batch][64] */, uint64_t seq, const uint64_t *sk_ntt,
                                       const uint64_t *plain, uint64_t *out_c0, size_t n_batch, size_t L, const uint32_t *prime_index,
                                       uint32_t *rejected /* device [2], or NULL */, void *stream);
/* KeyGenerator::generate_one_kswitch_key with save_seed, SEAL/keygenerator.cpp:303-336: one 64-byte seed per digit */
int moai_kswitch_keygen_seal_seeded(moai_ctx *ctx, const uint8_t *noise_key, const uint8_t *seeds /* host, [k-1][64] */, uint64_t seq,
                                    const uint64_t *sk_ntt, const uint64_t *new_key_ntt, uint64_t *out_c0 /* [k-1][k][N] */,
                                    uint32_t *rejected, void *stream);

/* ---- tuning -------------------------------------------------------------------------------------------------------
 * moai_set_tuning overrides a performance knob for the whole process; it takes precedence over the environment variable
 * of the same name, which the library reads once, on its first use of a knob.  moai_reset_tuning drops every override, so
 * that the environment's value, else the default, applies again.  A name that is not in this list is MOAI_EINVAL.
 * Results never depend on a knob.  Name, default, meaning:
 *   MOAI_NTT_FP            1     0: primes below 2^51 stay on the integer units in every transform, key switch and mod-down
 *   MOAI_NTT_LAZY8         1     0: integer primes below 2^60 take the exact butterflies instead of the approximate Shoup quotient
 *   MOAI_NTT_LAZY16        1     0: those primes keep values below 8q with a guard in every stage instead of below 16q with fewer (M_LAZY8)
 *   MOAI_NTT_LDSTW         1     0: the forward contiguous pass loads its first stages' twiddles from memory instead of through LDS
 *   MOAI_NTT_PAIR          1     0: the contiguous passes of the 60-bit rows run one polynomial per workgroup instead of two that share their twiddles
 *   MOAI_NTT_CHUNK_MB      88    > 0: launch the two passes of a transform per chunk of whole polynomials of at most this many MiB
 *   MOAI_NTT_CHUNK_KB      0     KiB added to MOAI_NTT_CHUNK_MB: chunks of rings whose polynomials are smaller than a MiB
 *   MOAI_NTT_PIPE          2     1..3: deal those chunks to this many side streams, so that a chunk's second pass runs beside the next one's first; 0: one stream
 *   MOAI_NTT_PIPE_MIN      32    chunks per side stream below which a transform stays on the caller's stream
 *   MOAI_NTT_PIPE_INNER    0     1: the transforms inside key switch, mod-down, encode and decode take the MOAI_NTT_PIPE schedule too
 *   MOAI_NTT_NAIVE         0     1: one launch per radix-2 stage over global memory (cross-check path)
 *   MOAI_KS_FP_MIN_ROWS    16    batch * L from which the key switch uses the FP64 arithmetic modes
 *   MOAI_KS_TMP_MB         8192  MiB of key-switch digits in flight: sets how many output moduli share a launch
 *   MOAI_KS_P1_ITEMS       8     1: the key switch's strided pass at N = 2^16 runs one tile per workgroup instead of eight, pipelined
 *   MOAI_KS_HOIST_PAIR     4     rotations per pass of the hoisted MAC in the FP64 modes: 4, 2, or 0 for one
 *   MOAI_MD_FP_MIN_ROWS    256   polynomials * L from which mod-down and rescale use the FP64 arithmetic modes
 *   MOAI_MATMUL_FP         1     0: moai_ct_pt_matmul keeps primes below 2^51 on the integer kernel
 *   MOAI_DEC_TMP_MB        1024  MiB of scratch per chunk of moai_ckks_decode when the stream's arena is smaller
 *   MOAI_CLIENT_TMP_KB     1048576 KiB of scratch per chunk of the encryption and key generation calls when the stream's arena is smaller
 *   MOAI_HYBRID_TMP_KB     16777216 KiB of scratch per chunk of the hybrid key switch: sets how many ciphertexts of a batch are in flight
 *   MOAI_HYBRID_HOIST_NR   4     rotations per pass of the hybrid hoisted MAC over the digits: 4, 2 or 1 */
int moai_set_tuning(const char *name, long value);
int moai_reset_tuning(void);
/* The schedule moai_ntt_forward / moai_ntt_inverse would take for n_poly polynomials of L rows of n coefficients with chunks of
 * chunk_bytes (MOAI_NTT_CHUNK_MB and _KB, in bytes) and k side streams (MOAI_NTT_PIPE): the number of chunks the busiest side
 * stream gets, or 0 when the transform stays on the caller's stream -- k < 1, no chunk size, fewer than two chunks, or fewer than
 * min_chunks (MOAI_NTT_PIPE_MIN) for the busiest stream.  Chunks are whole polynomials, at least one; at most three side streams, and no more than there are chunks, are used.  The side streams
 * belong to the context (one set per caller's stream, destroyed with it); the caller's stream forks to them and joins them through
 * events, so the transform stays ordered on the caller's stream like any other call.  A stream that is being captured keeps the
 * single-stream form.  Read-only host arithmetic: no context, no launch.  No counterpart in the reference. */
size_t moai_ntt_pipe_plan(size_t n_poly, size_t L, size_t n, size_t chunk_bytes, long k, long min_chunks);
/* Which arithmetic a context prime takes (read-only; no launch, no stream; no counterpart in the reference, whose arithmetic
 * is the same for every modulus).  Every mode computes the same residues; each is exact only below a size limit on the prime,
 * and tests use this query to know which limit a row exercises.  *mode receives the code the launcher itself would pick NOW,
 * the tuning knobs included (the launchers and this query call the same host functions):
 *   MOAI_MODE_OF_KEY_SWITCH  the fused key-switch kernels for output modulus `prime` at L data primes and `rows` = batch
 *                            ciphertexts (MOAI_KS_FP_MIN_ROWS, MOAI_NTT_FP): GUARD, NOGUARD, FPN or FPR
 *   MOAI_MODE_OF_MOD_DOWN    mod-down and rescale for output modulus `prime` with `rows` = polynomials * kept primes
 *                            (MOAI_MD_FP_MIN_ROWS, MOAI_NTT_FP; L is ignored): GUARD, NOGUARD, FPN or FPR
 *   MOAI_MODE_OF_NTT_FORWARD moai_ntt_forward's tiled kernels (N >= 4096; L, rows ignored): LAZY16, LAZY8, GUARD2, NOGUARD, FPN, FPR
 *   MOAI_MODE_OF_NTT_INVERSE moai_ntt_inverse's tiled kernels: LAZY16, LAZY8, GUARD (the exact integer butterflies), FPN or FPR
 * Limits: FPN 33 q < 2^52; FPR q < 2^51; NOGUARD 36 q < 2^64 and, in the key switch, 36 q^2 L < 2^128; LAZY16 / LAZY8 q < 2^60;
 * GUARD / GUARD2 any q < 2^61.  MOAI_EINVAL for a null argument or an unknown `op`, MOAI_ERANGE for prime >= k.
 * The degrees below N = 4096 have no arithmetic modes: one set of integer kernels (Harvey butterflies, a 128-bit key-switch sum
 * that needs L q^2 < 2^128) serves every prime below 2^61 there, and the answer of this query says nothing about them. */
#define MOAI_MODE_LAZY16 (-3)
#define MOAI_MODE_LAZY8 (-2)
#define MOAI_MODE_GUARD2 (-1)
#define MOAI_MODE_GUARD 0
#define MOAI_MODE_NOGUARD 1
#define MOAI_MODE_FPN 2
#define MOAI_MODE_FPR 3
#define MOAI_MODE_OF_KEY_SWITCH 0
#define MOAI_MODE_OF_MOD_DOWN 1
#define MOAI_MODE_OF_NTT_FORWARD 2
#define MOAI_MODE_OF_NTT_INVERSE 3
int moai_arith_mode(const moai_ctx *ctx, size_t prime, int op, size_t L, size_t rows, int *mode);

/* ---- hoisted rotations -------------------------------------------------------------------------------------------
 * out[r] = apply_galois(in, galois_elts[r], galois_keys[r]) for r < R -- R calls of Evaluator::rotate_vector /
 * apply_galois on the SAME ciphertext (SEAL/evaluator.cpp:2563-2665 over :2724-3020; the baby steps of MOAI's
 * bootstrapping transforms, include/source/bootstrapping/Bootstrapper.cpp:2017-2022, 2082-2088) -- with ONE digit
 * decomposition (the l (l + 1) transforms of switch_key_inplace) shared by all of them.  Bit-identical to the R separate
 * calls: the digit of a permuted polynomial is the permuted digit plus (q_J mod q_I) times the rotation's sign mask, and
 * that second term is the per-(key, level) constant moai_hoist_correction computes once (csrc/keyswitch_kernels.hip.h
 * has the derivation).  The identity needs INTT(c1) free of zero coefficients; the call checks that on the device and
 * otherwise makes the R separate calls itself (*used_fallback = 1).  Below N = 4096 there is no hoisted kernel: the call
 * always makes the R separate calls and reports *used_fallback = 1.
 *   in, outs[r]  [batch][2][L][N] (no output may alias the input)   correction [2][L+1][N] (rows 0..L-1 under primes
 *   0..L-1, row L under the special prime), computed for the same (key, galois_elt, L).  outs / galois_keys /
 *   corrections: host arrays of R device pointers.
 * Any R: the accumulators of one pass hold 64 rotations, more are done 64 at a time (one decomposition per pass).
 * The call SYNCHRONISES the stream once (it reads the zero-coefficient flag back): unlike the other key-switch entry
 * points it cannot run under HIP-graph stream capture. */
int moai_hoist_correction(moai_ctx *ctx, const uint64_t *galois_key, uint32_t galois_elt, size_t L, uint64_t *correction,
                          void *stream);
int moai_apply_galois_hoisted(moai_ctx *ctx, const uint64_t *in, uint64_t *const *outs, size_t L, const uint32_t *galois_elts,
                              const uint64_t *const *galois_keys, const uint64_t *const *corrections, size_t R, size_t batch,
                              int *used_fallback, void *stream);

/* ---- level-trimmed key residency ------------------------------------------------------------------------------------
 * switch_key_inplace at l data primes reads only the digits J < l and the rows {0 .. l-1, special prime} of a key
 * (SEAL/evaluator.cpp:2818, 2831; the reference keeps every key whole, SEAL/kswitchkeys.h:340: 1.32 GB each at MOAI's
 * parameters).  moai_key_trim copies exactly that part of a key in the reference's layout [k-1][2][k][N] into
 * `trimmed`, [levels][2][levels+1][N] with the special prime's row last (moai_key_words(ctx, levels) words), and records
 * the layout of that pointer in the context: every key-switch entry point above accepts it in place of the full key for
 * l <= levels, with the same results bit for bit (the same words are read), and fails with MOAI_ERANGE for l > levels.
 * MOAI's 31 default rotation keys are only used at chain index <= 14 (Ct_ct_matrix_mul.hpp:29,95,112,147): 15 levels =
 * 19 % of the full size.  moai_key_forget drops the record (before the block is freed or reused). */
size_t moai_key_words(const moai_ctx *ctx, size_t levels);
int moai_key_trim(moai_ctx *ctx, const uint64_t *full_key, size_t levels, uint64_t *trimmed, void *stream);
int moai_key_forget(moai_ctx *ctx, const uint64_t *key);

/* ---- keys limited to a chain index ----------------------------------------------------------------------------------
 * The key that is BORN in moai_key_trim's layout: a client that knows a key is only used at l <= levels data primes
 * generates, ships and loads exactly the digits J < levels and the rows {0 .. levels-1, k-1} that switch_key_inplace reads
 * there (SEAL/evaluator.cpp:2818, 2831), never the full key of KeyGenerator::generate_one_kswitch_key
 * (SEAL/keygenerator.cpp:303-336).  1 <= levels <= k-1; the layout is [levels][2][levels+1][N] with the special prime's row
 * last, moai_key_words(ctx, levels) words.
 * Contract: every word equals the corresponding word of moai_key_trim(moai_kswitch_keygen(same key, same seq, ...), levels)
 * (the seeded forms: of moai_kswitch_keygen_seeded + moai_expand_seeded + trim).  Digit J draws its noise from (noise key,
 * 3 << 56 | seq + J) and its uniform half from (key or seed, 1 << 56 | seq + J), and coefficient i of the row under prime
 * index p takes the stream words 2(pN + i), 2(pN + i) + 1: the position of the FULL k-row draw, not of the compact one (the
 * entry points with a prime_index keep their compact positions).  The call occupies the sequence range [seq, seq + levels);
 * with levels == k-1 the output is word for word the full key.  sk_ntt and new_key_ntt stay full [k][N] keys.
 * moai_kswitch_keygen_limited: out [levels][2][levels+1][N]; records the layout of `out` in the context as moai_key_trim does,
 * so every key-switch entry point accepts it for l <= levels (MOAI_ERANGE above); moai_key_forget before the block is freed
 * or reused.
 * moai_kswitch_keygen_limited_seeded: out_c0 [levels][levels+1][N], a from the public seed, e from noise_key; nothing is
 * recorded.
 * moai_expand_seeded_limited: c0 [levels][levels+1][N] -> out [levels][2][levels+1][N], a usable limited key; records the
 * layout of `out`.  c0 and out must not overlap.
 * moai_key_register: records the trimmed layout for a block [levels][2][levels+1][N] that arrived unseeded from elsewhere.
 * MOAI_EINVAL for a null pointer, for levels outside 1 .. k-1, and for an address already recorded with another layout.
 * Validation as above (null context / key / seed / argument, levels out of range, a sequence range beyond 2^56; MOAI_ELOGIC for
 * k < 2) before anything is enqueued; no call synchronises; large keys are generated in chunks as moai_kswitch_keygen's are. */
/* KeyGenerator::generate_one_kswitch_key, SEAL/keygenerator.cpp:303-336, cut to what SEAL/evaluator.cpp:2818,2831 read */
int moai_kswitch_keygen_limited(moai_ctx *ctx, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, const uint64_t *new_key_ntt,
                                size_t levels, uint64_t *out, void *stream);
/* the same with save_seed, SEAL/keygenerator.cpp:303-336, SEAL/keygenerator.h:321-360; rows of SEAL/evaluator.cpp:2818,2831 */
int moai_kswitch_keygen_limited_seeded(moai_ctx *ctx, const uint8_t *noise_key, const uint8_t *seed, uint64_t seq,
                                       const uint64_t *sk_ntt, const uint64_t *new_key_ntt, size_t levels, uint64_t *out_c0,
                                       void *stream);
/* Ciphertext::expand_seed, SEAL/ciphertext.cpp:118-188, over the rows of SEAL/evaluator.cpp:2818,2831 */
int moai_expand_seeded_limited(moai_ctx *ctx, const uint8_t *seed, uint64_t seq, const uint64_t *c0, size_t levels, uint64_t *out,
                               void *stream);
/* the layout record of moai_key_trim for a block filled elsewhere (SEAL/evaluator.cpp:2818,2831) */
int moai_key_register(moai_ctx *ctx, const uint64_t *key, size_t levels);

/* ---- hybrid key switching: alpha special primes, digits of alpha primes ---------------------------------------------------
 * Evaluator::switch_key_inplace decomposes per RNS prime and has one special prime: at l data primes l^2 + 3l + 2 transforms
 * and a key of l digits.  The hybrid form groups alpha primes into a digit and takes the last alpha primes of the context as
 * the special modulus; SEAL's switch is exactly its alpha = 1 case (same key layout, same mod-up, same rounding mod-down), and
 * at alpha = 1 every entry point below is bit for bit its counterpart above.  For alpha > 1 the results differ from the
 * reference in noise only, and are bit for bit the integer restatement tests/hybrid_ref.py.  Opt-in: nothing else uses it.
 *
 * All values are canonical residues.  Context primes m_0 .. m_{k-1}, 1 <= alpha < k (and alpha <= 16):
 *   special primes  p_t = m_{k-alpha+t}, t < alpha;  P their product;  h = floor(P / 2)
 *   data primes     q_i = m_i, i < Lmax = k - alpha
 *   digits at L     R_j = { r : j alpha <= r < min((j+1) alpha, L) }, j < beta(L) = ceil(L / alpha);  D_j = prod_{r in R_j} q_r
 * Key for s' under s: [beta(Lmax)][2][k][N] at the key level.  Digit j is a symmetric encryption of zero over all k rows with
 * noise and uniform half from sequence seq + j of the stream contract above (as moai_kswitch_keygen), plus (P mod q_r) s'[r] in
 * row r of c0 for every r of the top-level digit j.  A switch at L reads digits j < beta(L), rows {0 .. L-1} and {k-alpha .. k-1}.
 * Switch of target c [L][N] (NTT form) into ct [2][L][N]:
 *   1. c_r = INTT(c[r]), r < L
 *   2. mod-up, per digit j: y_r = c_r [(D_j / q_r)^-1]_{q_r} mod q_r for r in R_j; for every row m among q_i (i < L, i not in R_j)
 *      and p_t:  chat_j mod m = (sum_{r in R_j} y_r ((D_j / q_r) mod m)) mod m;  for m = q_r, r in R_j, chat_j is the NTT-form row
 *      c[r] as it is
 *   3. forward NTT of the converted rows
 *   4. acc[p][row] = sum_j chat_j[row] (*) key[j][p][row] mod m_row, p in {0, 1}
 *   5. mod-down with rounding, per p: x_t = INTT(acc[p][p_t]);  y_t = ((x_t + h mod p_t) mod p_t) [(P / p_t)^-1]_{p_t} mod p_t;
 *      conv_i = ((sum_t y_t ((P / p_t) mod q_i)) - (h mod q_i)) mod q_i;  ct[p][i] += (acc[p][i] - NTT(conv_i)) [P^-1]_{q_i} mod q_i
 * Noise: with keys from moai_hybrid_keygen (|e| <= 21) the output satisfies d0 + d1 s = c s' + E (mod Q_L) with
 *   |E| <= beta(L) N alpha 21 D_max / P + (alpha - 1/2)(1 + |s|_1),  D_max the largest D_j at that level;
 * P >= D_max keeps the first term small (a precondition of use, not checked: SEAL does not impose it at alpha = 1).
 * Shapes and aliasing follow moai_switch_key, moai_relinearize and moai_apply_galois.  Nothing is enqueued when an argument is
 * refused: MOAI_EINVAL with a message for a null context or pointer, alpha = 0, alpha >= k or alpha > 16, L = 0 or
 * L > k - alpha, an even Galois element or one >= 2N, a sequence range beyond 2^56.  batch = 0 is MOAI_OK.  Scratch per
 * ciphertext is beta (L + alpha) + 4L + 4 alpha rows of N words (2L more for apply_galois) from the stream's workspace; a batch
 * runs in chunks that fit MOAI_HYBRID_TMP_KB.  The first call at a new (L, alpha) builds that pair's constants with a blocking
 * copy, as the first use of a Galois element builds its table; otherwise no call synchronises.  moai_op_trace counts the calls
 * as "switch_key_hybrid", "relinearize_hybrid", "apply_galois_hybrid" and "hybrid_keygen". */
/* beta(L) = ceil(L / alpha), the digits SEAL/evaluator.cpp:2724-3020 would loop over at alpha = 1; 0 and the error set when refused */
size_t moai_hybrid_digits(const moai_ctx *ctx, size_t alpha, size_t L);
/* KeyGenerator::generate_one_kswitch_key, SEAL/keygenerator.cpp:303-336, with digits of alpha primes and P for the special prime */
int moai_hybrid_keygen(moai_ctx *ctx, const uint8_t *key /* host, 32 */, uint64_t seq, const uint64_t *sk_ntt /* [k][N] */,
                       const uint64_t *new_key_ntt /* [k][N], rows < k-alpha read */, size_t alpha,
                       uint64_t *out /* [beta(k-alpha)][2][k][N] */, void *stream);
/* Evaluator::switch_key_inplace, SEAL/evaluator.cpp:2724-3020, in the hybrid form; ct [batch][2][L][N] in place, target [batch][L][N] */
int moai_switch_key_hybrid(moai_ctx *ctx, uint64_t *ct, const uint64_t *target, const uint64_t *key, size_t L, size_t alpha,
                           size_t batch, void *stream);
/* Evaluator::relinearize_internal over the hybrid switch (SEAL/evaluator.cpp:2724-3020): ct3 [batch][3][L][N] -> out [batch][2][L][N] */
int moai_relinearize_hybrid(moai_ctx *ctx, const uint64_t *ct3, const uint64_t *key, uint64_t *out, size_t L, size_t alpha,
                            size_t batch, void *stream);
/* Evaluator::apply_galois_inplace over the hybrid switch (SEAL/evaluator.cpp:2724-3020): ct [batch][2][L][N] in place */
int moai_apply_galois_hybrid(moai_ctx *ctx, uint64_t *ct, size_t L, size_t alpha, uint32_t galois_elt, const uint64_t *key,
                             size_t batch, void *stream);

/* ---- hoisted rotations over the hybrid key switch ------------------------------------------------------------------------------
 * R rotations of the SAME ciphertext, each with its own key (the baby steps of MOAI's bootstrapping transforms, include/source/
 * bootstrapping/Bootstrapper.cpp:2017-2022, 2082-2088), with steps 1-3 above -- INTT, mod-up, forward transforms: L +
 * beta (L + alpha) - L of the 2 alpha + 2 L + beta (L + alpha) transforms of a switch -- done ONCE per ciphertext, as
 * moai_apply_galois_hoisted does for the reference's switch.  Bit-identical to the R separate moai_apply_galois_hybrid calls.
 * With sigma the automorphism, mask_sigma[i] = 1 where sigma negates the coefficient that lands on i, t = INTT(c1), n_j = |R_j|:
 * a separate call converts sigma(t), whose residues are q_r - t_r under the mask (t_r != 0), so its scaled residues are
 * q_r - y_r, and since sum_{r in R_j} q_r (D_j / q_r) = n_j D_j, for every row m outside R_j
 *     modup_j(sigma(t)) = sigma(chat_j) + n_j (D_j mod m) mask_sigma   (mod m)
 * as long as no coefficient of t is zero in any row; on the rows of R_j the digit is the permuted row of c1 and D_j mod q_r = 0.
 * NTT_m is linear and turns sigma into the index permutation apply_galois_ntt uses (SEAL/util/galois.cpp:192-218), so
 *     acc_r[p][row]  = sum_j perm_r(NTT(chat_j)[row]) (*) key_r[j][p][row] + corr_r[p][row]
 *     corr_r[p][row] = NTT_row(mask_r) (*) sum_{j < beta(L)} (n_j D_j mod m_row) key_r[j][p][row]      (mod m_row)
 * is congruent to the separate call's sum: the canonical accumulators are the same bits, and step 5 is unchanged.  At alpha = 1
 * this is moai_hoist_correction / moai_apply_galois_hoisted word for word (csrc/keyswitch_kernels.hip.h has that derivation).
 *   in, outs[r]  [batch][2][L][N]; no output may overlap the input or another output.  keys[r] in moai_hybrid_keygen's layout
 *   [beta(k-alpha)][2][k][N].  corrections[r] [2][L+alpha][N] from moai_hybrid_hoist_correction for the same (key, galois_elt, L,
 *   alpha).  outs / keys / corrections: host arrays of R device pointers; any R.
 * The identity needs INTT(c1) free of zero coefficients.  The call checks that on the device per batch chunk and makes the R
 * separate rotations of a chunk itself where it fails (*used_fallback = 1, same bits).  It therefore SYNCHRONISES the stream once
 * per batch chunk -- once when the batch fits the scratch budget -- and cannot run under HIP-graph stream capture (the
 * synchronisation fails there with MOAI_EHIP, as in moai_apply_galois_hoisted).
 * Scratch from the stream's workspace, in rows of N words, for cb ciphertexts per chunk and G rotations in flight:
 *     cb beta (L + alpha)  +  cb G (2 (L + alpha) + 2 alpha + 2 L + L)      (t and the digits; acc, special rows, conv, permuted c0)
 * plus one 256-byte block for the flag.  cb is the largest count for which cb ciphertexts with one rotation in flight fit
 * MOAI_HYBRID_TMP_KB, G the largest for which G rotations fit beside them; at least one of each, at most batch and R, and
 * 2 cb G (L + alpha) <= 65535.  A ciphertext is decomposed once however many groups its rotations take, MOAI_HYBRID_HOIST_NR
 * rotations share a pass of the MAC over the digits, and results depend on neither.
 * Nothing is enqueued and nothing written when an argument is refused: MOAI_EINVAL with a message for what the hybrid entry
 * points above refuse, a null array or a null entry in one, an even Galois element or one >= 2N, an output that overlaps the
 * input or another output.  batch = 0 and R = 0 are MOAI_OK.  moai_op_trace counts "hybrid_hoist_correction" (1) and
 * "apply_galois_hybrid_hoisted" (batch R) at L. */
/* corr [2][L+alpha][N]: rows 0..L-1 under q_0..q_{L-1}, rows L..L+alpha-1 under p_0..p_{alpha-1}; per (key, galois_elt, L, alpha);
 * the mod-up of SEAL/evaluator.cpp:2724-3020 applied to a permuted polynomial, less the permuted mod-up */
int moai_hybrid_hoist_correction(moai_ctx *ctx, const uint64_t *key, uint32_t galois_elt, size_t L, size_t alpha,
                                 uint64_t *correction, void *stream);
/* outs[r] = moai_apply_galois_hybrid(copy of in, L, alpha, galois_elts[r], keys[r]) for r < R, bit for bit, with ONE
 * INTT + mod-up + forward transform of the digits per ciphertext (SEAL/evaluator.cpp:2724-3020 shared by R rotations) */
int moai_apply_galois_hybrid_hoisted(moai_ctx *ctx, const uint64_t *in, uint64_t *const *outs, size_t L, size_t alpha,
                                     const uint32_t *galois_elts, const uint64_t *const *keys,
                                     const uint64_t *const *corrections, size_t R, size_t batch, int *used_fallback,
                                     void *stream);

/* ---- plaintext-weighted sums of hoisted rotations, one mod-down per sum ---------------------------------------------------------
 * The inner sum of a baby-step / giant-step linear transform over hybrid keys: n_out outputs, each sum_r p_{g,r} (*) rot_r(ct) over
 * the same R rotations of ONE ciphertext.  A hybrid switch keeps its sum in the extended basis Q P until step 5, so the plaintext
 * products and the sum over r are taken THERE and one mod-down per output replaces one per rotation: no accumulator of a
 * rotation and no rotated ciphertext reaches memory.
 *   in [batch][2][L][N], NTT form;  outs[g] [batch][2][L][N], g < n_out;  rotation r < R: Galois element e_r, keys[r] in
 *   moai_hybrid_keygen's layout, corrections[r] from moai_hybrid_hoist_correction for the same (key, element, L, alpha);
 *   plains[g R + r]: p_{g,r}, [L+alpha][N] words in NTT form, rows 0..L-1 under q_i and rows L..L+alpha-1 under p_t (the row order of
 *   a correction; moai_ckks_encode with prime_index = {0..L-1, k-alpha..k-1}), shared by the batch, or NULL: the term is absent.
 * Per ciphertext (c0, c1) and output g, with steps 1-5 of "hybrid key switching" above, all residues canonical:
 *   A_r    (e_r != 1)  [2][L+alpha]: the accumulator of steps 1-4 for the target perm_r(c1) with keys[r], what a separate
 *          moai_apply_galois_hybrid forms before its step 5;  U_r[i] = perm_r(c0)[i], i < L
 *   S_g[p][row]  = sum_{r : e_r != 1, p_{g,r} present} p_{g,r}[row] (*) A_r[p][row]  mod m_row
 *   D_g          = step 5 of S_g: D_g[p][i] = (S_g[p][i] - NTT(conv_i(S_g[p]))) [P^-1]_{q_i}, the rounding terms as there; D_g = 0
 *                  and no step 5 when output g has no present term with e_r != 1
 *   out_g[0][i]  = D_g[0][i] + sum_{r : e_r != 1} p_{g,r}[i] (*) U_r[i] + sum_{r : e_r = 1} p_{g,r}[i] (*) c0[i]  mod q_i
 *   out_g[1][i]  = D_g[1][i] + sum_{r : e_r = 1} p_{g,r}[i] (*) c1[i]  mod q_i
 * e_r = 1 is the zeroth baby step, a plain product: its key and correction are not read and may be NULL.  Keys, corrections and
 * plaintexts may repeat.  The result is bit for bit the integer restatement tests/hybrid_dot_ref.py.  It is NOT the sum of the
 * separately switched rotations, whose roundings happen once each: it differs from that sum in noise only.
 * Noise: with keys from moai_hybrid_keygen for sigma_r(s) -> s,  out_g[0] + out_g[1] s = sum_r p_{g,r} sigma_r(c0 + c1 s) + E.
 * Before step 5, S_g[0] + S_g[1] s = P sum_r p_{g,r} sigma_r(c1) sigma_r(s) + sum_r p_{g,r} e'_r over Q_L P, where e'_r = sum_j
 * chat_{j,r} e_{j,r} is the key noise of rotation r, |e'_r| <= beta(L) N alpha 21 D_max as in the single switch (|chat_j| <=
 * alpha D_max, |e| <= 21, N coefficients per product).  A product p e' of polynomials has coefficients of at most |p|_1 |e'|_inf,
 * |p|_1 the sum of the absolute centred coefficients of the encoded integer polynomial, so the key noise of S_g is at most
 * (sum_r |p_{g,r}|_1) beta(L) N alpha 21 D_max, and step 5 divides it by P.  Step 5 itself rounds each of the two polynomials
 * once: its fast base conversion is off by at most alpha - 1 multiples of P besides the 1/2 of the rounding, (alpha - 1/2) on
 * d0 and (alpha - 1/2) |s|_1 through d1 s.  The products added after step 5 are exact.  Hence
 *   |E| <= (sum_{r : e_r != 1} |p_{g,r}|_1) beta(L) N alpha 21 D_max / P + (alpha - 1/2)(1 + |s|_1):
 * the single switch's first term scaled by the plaintexts, and ONE mod-down's rounding however many rotations are summed.
 * Hoisted as moai_apply_galois_hybrid_hoisted: steps 1-3 run once per ciphertext on the unpermuted c1, every rotation reads the
 * digits through its permutation table and adds its correction, and the kernel weights the accumulators it holds in registers
 * into S_g and the addend of every output in flight, MOAI_HYBRID_HOIST_NR rotations per pass; S_g and the addend travel between
 * passes as canonical residues.  The identity needs INTT(c1) free of zero coefficients: the call checks that on the device per
 * batch chunk, and a chunk where it fails takes every rotation through the unhoisted steps 1-4 on the permuted input instead
 * (*used_fallback = 1, same bits).  It therefore SYNCHRONISES the stream once per batch chunk and cannot run under HIP-graph stream
 * capture (MOAI_EHIP there), as moai_apply_galois_hybrid_hoisted.
 * Scratch from the stream's workspace, in rows of N words, for cb ciphertexts per chunk and G outputs in flight:
 *     cb (beta (L + alpha) + 2 L + 2 (L + alpha))  +  cb G (2 (L + alpha) + 2 alpha + 2 L + 2 L)
 * (t and the digits, the unhoisted route's permuted input and accumulators; S, special rows, conv, addend) plus one 256-byte block
 * for the flag: nothing grows with R.  cb is the largest count for which cb ciphertexts with one output in flight fit
 * MOAI_HYBRID_TMP_KB, G the largest for which G outputs fit beside them; at least one of each, at most batch and n_out, G <= 16 and
 * 2 cb G (L + alpha) <= 65535.  Outputs beyond G repeat the MAC over the digits, not the decomposition.  Results depend on neither
 * the budget nor MOAI_HYBRID_HOIST_NR.
 * Nothing is enqueued and nothing written when an argument is refused: MOAI_EINVAL with a message for what the hybrid entry
 * points above refuse, a null array, a null key or correction where e_r != 1, a null output, an even Galois element or one >= 2N,
 * an output that overlaps the input or another output, an output with no present term.  batch = 0 and n_out = 0 are MOAI_OK.
 * moai_op_trace counts "hybrid_rotate_pt_dot" (batch n_out) at L. */
/* outs[g] = sum_r plains[g R + r] (*) rotate(in, galois_elts[r]) with ONE mod-down per output: the rotate_vector / multiply_plain /
 * add_inplace loops of MOAI's bsgs_linear_transform (include/source/bootstrapping/Bootstrapper.cpp:2017-2042, 2082-2108) over the
 * hybrid form of SEAL/evaluator.cpp:2724-3020 */
int moai_hybrid_rotate_pt_dot(moai_ctx *ctx, const uint64_t *in, uint64_t *const *outs, size_t n_out, size_t L, size_t alpha,
                              const uint32_t *galois_elts, const uint64_t *const *keys, const uint64_t *const *corrections, size_t R,
                              const uint64_t *const *plains /* host array [n_out * R], entry g * R + r, NULL = absent */, size_t batch,
                              int *used_fallback, void *stream);

/* ---- giant steps summed in the extended basis: a whole BSGS linear transform with n_giant + 2 polynomial mod-downs -----------------
 * The second half of the double-hoisted baby-step / giant-step transform over hybrid keys.  The inner sums of the section above stay
 * in the extended basis Q P; each giant step takes ONE polynomial of its inner sum (c1) down to Q to feed its own key switch, whose
 * accumulator is again kept over Q P; everything is summed there and ONE step 5 of both polynomials ends the call.  No inner sum, no
 * rotated inner sum and no accumulator of a giant step is rounded or written out on its own.
 *   in, out [batch][2][L][N], NTT form;  baby step r < R: element e_r, baby_keys[r], baby_corrections[r] and plains[g R + r] exactly
 *   the operands of the section above with n_out = n_giant;  giant step g < n_giant: Galois element E_g and giant_keys[g], an ordinary
 *   hybrid Galois key for sigma_{E_g}(s) -> s in moai_hybrid_keygen's layout (what moai_apply_galois_hybrid takes; no correction).
 *   An element 1 on either side reads no key (and no correction): the entries may be NULL there.
 * Per ciphertext, all residues canonical, with S_g [2][L+alpha] and the addend a_g [2][L] (a_g[p][i] = out_g[p][i] - D_g[p][i]) of
 * the section above for output g, and Pq_i = P mod q_i:
 *   T_g    the inner sum lifted into Q P, nothing rounded: T_g[p][i] = S_g[p][i] + Pq_i a_g[p][i] mod q_i on the data rows i < L,
 *          T_g[p][row] = S_g[p][row] on the special rows (S_g = 0 where output g has no term with e_r != 1)
 *   c1'_g  [L] = out_g[1] of the section above, bit for bit: step 5 of S_g[1] plus a_g[1], and a_g[1] alone without a step 5 where
 *          output g has no term with e_r != 1.  The only mod-down a giant step takes, of one polynomial.
 *   E_g != 1:  B_g [2][L+alpha] = the accumulator of steps 1-4 for the target perm_{E_g}(c1'_g) with giant_keys[g];
 *              Z[0][row] += B_g[0][row] + perm_{E_g}(T_g[0])[row] over all L + alpha rows,  Z[1][row] += B_g[1][row]
 *   E_g = 1:   Z[p][row] += T_g[p][row]
 *   out = step 5 of Z, both polynomials, no addend.
 * Lifting is exact ((T[i] - conv_i) P^-1 = (S[i] - conv_i) P^-1 + a[i] mod q_i, the special rows untouched), so one giant step of
 * element 1 is the section above with one output, bit for bit; and R = 1, e_0 = 1, the all-ones plaintext and one giant step E with
 * key K is moai_apply_galois_hybrid on a copy of the input, bit for bit (c1' = c1 because no step 5 runs, Z = B + perm(P c0)).
 * Everything else differs from the composition of those calls in noise only.  The result is bit for bit the integer restatement
 * tests/hybrid_bsgs_ref.py.
 * Noise: with keys for sigma(s) -> s,  out[0] + out[1] s = sum_g sigma_{E_g}(sum_r p_{g,r} sigma_{e_r}(c0 + c1 s)) + E.  Write M_g for
 * the inner sum's message.  By the section above T_g[0] + T_g[1] s = P M_g + eps_g over Q_L P with |eps_g| <= l_g u P, where l_g =
 * sum_{r : e_r != 1} |p_{g,r}|_1 and u = beta(L) N alpha 21 D_max / P is the single switch's key-noise term.  The one-polynomial
 * mod-down gives T_g[1] = P c1'_g + rho_g with |rho_g| <= (alpha - 1/2) P (the fast base conversion is off by at most alpha - 1
 * multiples of P besides the 1/2 of the rounding; rho_g = 0 where no step 5 runs).  The giant switch gives B_g[0] + B_g[1] s = P
 * sigma_E(c1'_g) sigma_E(s) + eps'_g with |eps'_g| <= u P, so giant step g adds
 *   B_g[0] + sigma_E(T_g[0]) + B_g[1] s = P sigma_E(M_g) + sigma_E(eps_g) - sigma_E(rho_g s) + eps'_g,   |rho_g s| <= (alpha - 1/2) P |s|_1,
 * and a giant step of element 1 adds P M_g + eps_g.  The final step 5 divides the sum by P and rounds both polynomials once.  Hence
 *   |E| <= (alpha - 1/2)(1 + |s|_1) + sum_g [ l_g u + [E_g != 1] (u + (alpha - 1/2) |s|_1) ].
 * On the device the inner stage is that of the section above up to its step 5 (one decomposition of the unpermuted c1 per ciphertext,
 * the zero probe and its unhoisted route, MOAI_HYBRID_HOIST_NR rotations per pass), for the giant steps of a group at a time.  Then
 * one kernel takes S_g[1] and a_g[1] to c1'_g and writes it permuted by E_g, steps 1-3 run over all (giant step, ciphertext) pairs of
 * the group at once, and one MAC kernel sums the giant steps' digit-key products, the gathered T_g[0] and the terms of element 1 into
 * Z, which it reads (after the first group) and writes once per group.  The giant stage is not hoisted and needs no zero probe:
 * *used_fallback and the one synchronisation per batch chunk are the inner stage's, and the call cannot run under HIP-graph stream
 * capture (MOAI_EHIP there).
 * Scratch from the stream's workspace, in rows of N words, for cb ciphertexts per chunk and G giant steps in flight:
 *     cb (beta (L + alpha) + 2 L + 2 (L + alpha)  +  2 (L + alpha) + 2 alpha + 2 L)
 *   + cb G (2 (L + alpha) + 2 L  +  alpha + L  +  L + beta (L + alpha))
 * (the inner stage's shared rows; Z with the special rows and conv of its step 5; per giant step S and the addend; the special rows
 * and conv of c1'; the permuted c1' with its t and digits) plus one 256-byte block for the flag: nothing grows with R.  A group of giant
 * steps repeats the inner stage's MAC over the baby steps it uses and a batch chunk repeats nothing, so the giant steps come first:
 * G = min(n_giant, 16) when one ciphertext with G giant steps in flight fits MOAI_HYBRID_TMP_KB, and cb is then the largest count that
 * fits with them; else cb = 1 and G is the largest count that fits beside one ciphertext, at least one.  cb <= batch (the chunks of
 * a batch are evened out) and 2 cb G (L + alpha) <= 65535.  Results depend on neither the budget nor MOAI_HYBRID_HOIST_NR.
 * Nothing is enqueued and nothing written when an argument is refused: MOAI_EINVAL with a message for everything the section above
 * refuses, a null giant array, a null giant key where E_g != 1, an even giant element or one >= 2N, out null or overlapping in, a
 * giant step with no present term, R = 0 or n_giant = 0.  batch = 0 is MOAI_OK.
 * moai_op_trace counts "hybrid_bsgs_dot" (batch) at L and none of the calls it replaces. */
/* out = sum_g rotate( sum_r plains[g R + r] (*) rotate(in, baby_elts[r]), giant_elts[g] ), everything summed in the extended basis:
 * the whole of MOAI's bsgs_linear_transform / rotated_bsgs_linear_transform (include/source/bootstrapping/Bootstrapper.cpp:1997-2062,
 * 2064-2129) over the hybrid form of SEAL/evaluator.cpp:2724-3020 */
int moai_hybrid_bsgs_dot(moai_ctx *ctx, const uint64_t *in, uint64_t *out /* [batch][2][L][N] */, size_t L, size_t alpha,
                         const uint32_t *baby_elts, const uint64_t *const *baby_keys, const uint64_t *const *baby_corrections, size_t R,
                         const uint32_t *giant_elts, const uint64_t *const *giant_keys, size_t n_giant,
                         const uint64_t *const *plains /* host array [n_giant * R], entry g * R + r, NULL = absent */, size_t batch,
                         int *used_fallback, void *stream);

/* ---- hybrid relinearize + rescale: one mod-down by P and the last prime ---------------------------------------------------------------
 * multiply -> relinearize -> rescale over hybrid keys is moai_relinearize_hybrid (a mod-down by P: per polynomial alpha inverse and L
 * forward transforms) directly followed by moai_rescale (a divide-and-round by q_{L-1}: 1 inverse and L - 1 forward transforms, one
 * more pass over the ciphertext).  Both divide by a product of primes of the basis and round, so the calls below take ONE mod-down
 * by W = P q_{L-1} from the basis Q_L P straight to Q_{L-1}: 2L transforms fewer per ciphertext (305 -> 235 at L = 35, alpha = 12;
 * 138 -> 108 at L = 15) and one elementwise pass over [2][L][N] less.  Opt-in like the rest of the hybrid sections; every other
 * entry point keeps its bits.  `key` is a relinearization key (s^2 under s) in moai_hybrid_keygen's layout: no new key material.
 *
 * Definition of moai_relinearize_rescale_hybrid.  All residues canonical; notation and steps 1-4 are those of "hybrid key switching".
 * Per ciphertext (c_0, c_1, c_2), steps 1-4 on the target c_2 give acc[p][row] over the L data rows and the alpha special rows.
 * W = P q_{L-1}, H = floor(W / 2); the source base is S = {q_{L-1}, p_0, .., p_{alpha-1}}, alpha + 1 primes.  For p in {0, 1}:
 *   lift     Z_p[i] = (acc[p][i] + (P mod q_i) c_p[i]) mod q_i for i < L;  Z_p[p_t] = acc[p][p_t]
 *   inverse  x_m = INTT(Z_p[m]) for m in S (in the accumulator's row order [L data rows][alpha special rows] the contiguous rows
 *            L-1 .. L+alpha-1)
 *   scale    y_m = ((x_m + H mod m) mod m) [(W / m)^-1]_m mod m
 *   convert  conv_i = ((sum_{m in S} y_m ((W / m) mod q_i)) - (H mod q_i)) mod q_i for i < L - 1, then forward NTT
 *   finish   out[p][i] = (Z_p[i] - conv_i) [W^-1]_{q_i} mod q_i for i < L - 1
 * (the device finishes with c_p[i] [q_{L-1}^-1]_{q_i} + (acc[p][i] - conv_i) [W^-1]_{q_i}, which is the same residue, so only row
 * L - 1 is lifted before the inverse transform).  The result is bit for bit the integer restatement tests/hybrid_rescale_ref.py.
 * As an integer, coefficientwise, out_p = floor((Z_p + H) / W) - u'_p, where the integer u'_p in [0, alpha] is the overflow of the
 * fast conversion of alpha + 1 residues.  Three consequences:
 *   Not the composition's bits.  The call is NOT bit-equal to moai_rescale(moai_relinearize_hybrid(ct3)).  In coefficient form each
 *     coefficient of (out - composition) mod Q_{L-1}, centred, lies in [-(alpha + 1), +1]: the composition is round(X) + {-1, 0, 1}
 *     because its own overflow u is divided by q_{L-1}, the merged form is round(X) - u'.
 *   Noise.  With keys from moai_hybrid_keygen the centred value of q_{L-1} (out_0 + out_1 s) - (c_0 + c_1 s + c_2 s^2) mod Q_L is
 *     at most  beta(L) N alpha 21 D_max / P  +  q_{L-1} (alpha + 1/2)(1 + |s|_1)  in absolute value.  After the division by q_{L-1} the
 *     rounding term is (alpha + 1/2)(1 + |s|_1) where the composition's is about 1/2 (1 + |s|_1): the merged call buys its saved
 *     transforms with up to alpha more units of rounding per coefficient, the size of what every hybrid rotation already adds at the
 *     ciphertext's scale.
 *   Preconditions.  L >= 2 (a prime must be left to rescale to) and alpha + 1 <= 16 (the conversion holds its sources in registers).
 * moai_multiply_relin_rescale_hybrid is bit for bit moai_ct_multiply (moai_ct_square where y == x) followed by the call above; the
 * three-polynomial product lives only in the chunk's scratch, 3L more rows per ciphertext, and never reaches caller memory.
 *   ct3 [batch][3][L][N];  x, y [batch][2][L][N], y may be x;  out [batch][2][L-1][N];  inputs are never written.
 * Nothing is enqueued and nothing written when an argument is refused: MOAI_EINVAL with a message for everything the hybrid entry
 * points refuse, in their order (alpha = 0, L = 0, then L = 1 and alpha = 16, all answered before the context is touched; then a null
 * context, alpha >= k, alpha > 16, L > k - alpha), a null pointer, `out` overlapping an input or the key.  batch = 0 is MOAI_OK.
 * Scratch per ciphertext is beta (L + alpha) + 2 (L + alpha) + 2 (alpha + 1) + 2 (L - 1) rows of N words (3L more with the product)
 * from the stream's workspace; a batch runs in chunks that fit MOAI_HYBRID_TMP_KB and results do not depend on the budget.  The
 * first call at a new (L, alpha) builds that pair's constants with a blocking copy; otherwise neither call synchronises.
 * moai_op_trace counts "relinearize_rescale_hybrid" (batch) and "multiply_relin_rescale_hybrid" (batch) at L, and none of the calls
 * they replace. */
/* Evaluator::relinearize_internal over the hybrid switch (SEAL/evaluator.cpp:2724-3020) merged with Evaluator::rescale_to_next
 * (SEAL/evaluator.cpp:1682-1720 -> mod_switch_scale_to_next :1402-1481 -> RNSTool::divide_and_round_q_last_ntt_inplace
 * SEAL/util/rns.cpp:830-901): one mod-down by P q_{L-1} */
int moai_relinearize_rescale_hybrid(moai_ctx *ctx, const uint64_t *ct3 /* [batch][3][L][N] */, const uint64_t *key,
                                    uint64_t *out /* [batch][2][L-1][N] */, size_t L, size_t alpha, size_t batch, void *stream);
/* Evaluator::multiply (SEAL/evaluator.cpp:770-909; :1223-1282 where y == x), then the hybrid form of relinearize
 * (SEAL/evaluator.cpp:2724-3020) merged with rescale_to_next (SEAL/evaluator.cpp:1682-1720, :1402-1481, SEAL/util/rns.cpp:830-901) */
int moai_multiply_relin_rescale_hybrid(moai_ctx *ctx, const uint64_t *x, const uint64_t *y /* [batch][2][L][N], y may be x */,
                                       const uint64_t *key, uint64_t *out /* [batch][2][L-1][N] */, size_t L, size_t alpha,
                                       size_t batch, void *stream);

/* ---- hybrid key switches on a list of ciphertexts, each with its own key and element ---------------------------------------------------
 * What "Key switches on a LIST of single ciphertexts" (moai_apply_galois_ptrs, moai_relinearize_ptrs) is to the SEAL-style switch,
 * for hybrid keys: every hybrid entry point above takes ONE contiguous block [batch][..], one key and one Galois element, while the
 * differently rotated ciphertexts of MOAI's OpenMP loops (include/source/matrix_mul/Ct_ct_matrix_mul.hpp:22-31, 84-102, 142-149) sit
 * each in its own block with its own element and key.  The list forms are the n single calls at batch 1 in one chain of launches,
 * and the out-of-place and accumulating rotations are the same last kernel with an output pointer and a second addend.  All five
 * are bit for bit the calls they stand for: no restatement changes (tests/hybrid_ref.py, tests/hybrid_rescale_ref.py), and at
 * alpha = 1 moai_apply_galois_hybrid_ptrs and moai_relinearize_hybrid_ptrs are bit for bit moai_apply_galois_ptrs and
 * moai_relinearize_ptrs.  Opt-in like the rest of the hybrid sections; every other entry point keeps its bits.
 *   Keys: moai_hybrid_keygen's whole layout [beta(k-alpha)][2][k][N] only.
 *   Lists (ins / ct3s / outs / keys / sums / galois_elts): HOST arrays of n entries, read before the call returns; the pointer lists
 *     reach the device as kernel arguments, never through a host-to-device copy.  sums may be NULL, and so may any sums[i].
 *   Aliasing, as moai_apply_galois_ptrs: outs[i] may be ins[i] or sums[i] exactly; it may never be a part of ins[i] or sums[i], and
 *     never touch a block of another member; sums[i] may not be ins[i].  For the two relinearize forms the output may not be the
 *     input.  An output block of moai_relinearize_rescale_hybrid_ptrs is 2 (L - 1) N words.  Inputs, sums that are not outputs, and
 *     keys are only read.
 *   Refusals: everything is validated before anything is enqueued and nothing is written on refusal; MOAI_EINVAL, in this order:
 *     n == 0 is MOAI_OK whatever else is passed; "null list"; "member i: null pointer" or "member i: Galois element is not valid"
 *     (an even element); then what the hybrid entry points refuse, in their order and words (alpha = 0, L = 0, null context,
 *     alpha >= k, alpha > 16, L > k - alpha; the rescale form also L = 1 and alpha = 16, where moai_relinearize_rescale_hybrid
 *     answers them); then "member i: ..." for an element >= 2N and for the overlaps.  moai_apply_galois_hybrid_to / _acc refuse
 *     what moai_apply_galois_hybrid does, in its order, then a null pointer, `in` == `acc`, and any overlap of `out` with `in` (or
 *     of `acc` with `in`) other than out == in.
 *   Passes: a pass takes min(64, the chunk MOAI_HYBRID_TMP_KB allows) members, at least one.  Scratch per member, in rows of N
 *     words from the stream's workspace: the rotation beta (L + alpha) + 4L + 4 alpha + 2L (the permuted member; the same as a
 *     ciphertext of moai_apply_galois_hybrid), moai_relinearize_hybrid_ptrs beta (L + alpha) + 4L + 4 alpha + L (the gathered third
 *     polynomial), moai_relinearize_rescale_hybrid_ptrs beta (L + alpha) + 2 (L + alpha) + 2 (alpha + 1) + 2 (L - 1) + L; beta =
 *     ceil(L / alpha).  Results depend on neither the budget nor n.
 *   No call synchronises beyond the first-use builds of "hybrid key switching" (the constants of a new (L, alpha), the table of a
 *     new Galois element).  moai_op_trace counts the calls they replace: "apply_galois_hybrid", "relinearize_hybrid" and
 *     "relinearize_rescale_hybrid", n (or batch) units at L. */
/* Evaluator::apply_galois (SEAL/evaluator.cpp:2563-2665 with a `destination`, SEAL/evaluator.h:1093-1101) over the hybrid switch
 * (SEAL/evaluator.cpp:2724-3020): moai_apply_galois_hybrid on a copy of `in`, without the copy.  in, out [batch][2][L][N]; out may be
 * in, and moai_apply_galois_hybrid is this call with out == in. */
int moai_apply_galois_hybrid_to(moai_ctx *ctx, const uint64_t *in, uint64_t *out, size_t L, size_t alpha, uint32_t galois_elt,
                                const uint64_t *key, size_t batch, void *stream);
/* acc = add_inplace(acc, apply_galois(in)) (SEAL/evaluator.cpp:2563-2665 over the hybrid switch SEAL/evaluator.cpp:2724-3020), as
 * moai_apply_galois_acc: the bits of moai_apply_galois_hybrid_to followed by moai_add, canonical residues; the addition rides on the
 * last kernel's second addend.  in, acc [batch][2][L][N], distinct. */
int moai_apply_galois_hybrid_acc(moai_ctx *ctx, const uint64_t *in, uint64_t *acc, size_t L, size_t alpha, uint32_t galois_elt,
                                 const uint64_t *key, size_t batch, void *stream);
/* outs[i] = [sums[i] +] moai_apply_galois_hybrid(copy of ins[i], galois_elts[i], keys[i]), i < n: n calls of
 * moai_apply_galois_hybrid_to / _acc at batch 1 (Evaluator::apply_galois_inplace, SEAL/evaluator.cpp:2563-2665, over the hybrid
 * switch SEAL/evaluator.cpp:2724-3020) in one chain of launches per pass.  Each member [2][L][N]. */
int moai_apply_galois_hybrid_ptrs(moai_ctx *ctx, const uint64_t *const *ins, uint64_t *const *outs, size_t L, size_t alpha,
                                  const uint32_t *galois_elts, const uint64_t *const *keys,
                                  const uint64_t *const *sums /* NULL, or entries may be NULL */, size_t n, void *stream);
/* outs[i] = moai_relinearize_hybrid(ct3s[i]) with one key: n calls at batch 1 (Evaluator::relinearize_internal,
 * SEAL/evaluator.cpp:1345-1400, over the hybrid switch SEAL/evaluator.cpp:2724-3020) in one chain of launches per pass.  ct3s[i]
 * [3][L][N], outs[i] [2][L][N]. */
int moai_relinearize_hybrid_ptrs(moai_ctx *ctx, const uint64_t *const *ct3s, uint64_t *const *outs, const uint64_t *key, size_t L,
                                 size_t alpha, size_t n, void *stream);
/* outs[i] = moai_relinearize_rescale_hybrid(ct3s[i]) with one key: n calls at batch 1 (Evaluator::relinearize_internal,
 * SEAL/evaluator.cpp:1345-1400, over the hybrid switch SEAL/evaluator.cpp:2724-3020, merged with Evaluator::rescale_to_next,
 * SEAL/evaluator.cpp:1682-1720) in one chain of launches per pass; that call's documented rounding carries over unchanged.  ct3s[i]
 * [3][L][N], outs[i] [2][L-1][N]; L >= 2. */
int moai_relinearize_rescale_hybrid_ptrs(moai_ctx *ctx, const uint64_t *const *ct3s, uint64_t *const *outs /* [2][L-1][N] */,
                                         const uint64_t *key, size_t L, size_t alpha, size_t n, void *stream);

/* ---- hybrid rounding mode: the mod-down's overflow corrected in FP64 ----------------------------------------------------------------------
 * Step 5 of every hybrid entry point, and the merged mod-down of the relinearize + rescale forms, is a FAST base conversion: it returns
 * the rounded quotient less an overflow u in [0, n), n the number of source primes, which is where the (alpha - 1/2) and (alpha + 1/2)
 * of the noise bounds above come from.  MOAI_HYBRID_ROUND_EXACT estimates that overflow in binary64 and takes it out.  The mode is an
 * attribute of the context (an atomic; FAST when the context is created).  Every hybrid entry point reads it ONCE on entry, so a call
 * with several mod-downs (moai_hybrid_bsgs_dot), its batch chunks and the separate calls of a fallback all round alike.  It is not a
 * tuning knob: results depend on it, so it is not in MOAI_KNOBS and moai_reset_tuning leaves it alone.  With the default every entry
 * point launches the kernels and gives the bits it gave before the mode existed.  The mod-ups (step 2) keep the fast form in both modes:
 * their overflow is the approximation term of the key noise and part of the hoisted identity.
 *
 * The contract.  A mod-down from sources S (n = |S| primes m, in the order of the accumulator's rows: p_0 .. p_{alpha-1} for step 5,
 * q_{L-1}, p_0 .. p_{alpha-1} for the merged form; W their product, H = floor(W / 2)) to the targets q_i is, in the fast mode,
 *   y_m    = ((x_m + H mod m) mod m) [(W / m)^-1]_m  mod m
 *   conv_i = (sum_m y_m ((W / m) mod q_i)  -  (H mod q_i)) mod q_i
 * As integers sum_m y_m (W / m) = X' + v* W with X' = (x + H) mod W in [0, W) and v* = floor(sum_m y_m / m) in [0, n).  The exact mode:
 *   r_m    = 1.0 / (double)m                 IEEE binary64, computed on the host (two roundings, reproducible in numpy)
 *   f      = 0.0;  for m in S, in the source order:  f = f (+) ( (double)y_m (x) r_m )
 *                                            (double)y_m round-to-nearest-even; (x) and (+) are single rounded operations, NOT fused
 *   v      = min(max(floor(f), 0), n - 1)
 *   conv_i = (sum_m y_m ((W / m) mod q_i)  -  v (W mod q_i)  -  (H mod q_i)) mod q_i
 * Everything after the conversion (the forward transform and the last kernel) is the fast mode's.  The clamp is part of the contract:
 * with n = 1 and y = m - 1 the product rounds to 1.0.  AT alpha = 1 BOTH MODES GIVE THE SAME BITS for step 5 (one source: v* = 0 = v),
 * i.e. SEAL's; the merged form has two sources there and the modes differ.
 *
 * The property.  |f - sum_m y_m / m| <= eps with eps = 2^-40 promised here (csrc/hybrid_kernels.hip.h derives about 323 2^-53 for n <= 17
 * and m < 2^61).  When floor(f) != v*, X' / W is within eps of 0 or of 1 and the neighbouring integer is still within 1/2 + eps of the
 * real quotient.  So for EVERY coefficient and EVERY input, deterministically, with Z_p the lifted accumulator as an integer mod Q W (Q P
 * for step 5) and out_p the integer the mod-down returns:
 *   | out_p - Z_p / W |  <=  1/2 + 2^-40,
 * and out_p = floor((Z_p + H) / W) exactly whenever X' / W is outside [0, 2^-40) and (1 - 2^-40, 1).  The results are bit for bit the
 * integer-plus-numpy-float64 restatement tests/hybrid_exact_ref.py.
 *
 * The noise bounds in exact mode: every mod-down's (alpha - 1/2) or (alpha + 1/2) becomes (1/2 + 2^-40).
 *   hybrid key switching (switch, relinearize, rotations, their list and hoisted forms):
 *     |E| <= beta(L) N alpha 21 D_max / P + (1/2 + 2^-40)(1 + |s|_1)            -- the second term is SEAL's
 *   moai_hybrid_rotate_pt_dot:
 *     |E| <= (sum_{r : e_r != 1} |p_{g,r}|_1) beta(L) N alpha 21 D_max / P + (1/2 + 2^-40)(1 + |s|_1)
 *   moai_hybrid_bsgs_dot (|rho_g| <= (1/2 + 2^-40) P):
 *     |E| <= (1/2 + 2^-40)(1 + |s|_1) + sum_g [ l_g u + [E_g != 1] (u + (1/2 + 2^-40) |s|_1) ]
 *   moai_relinearize_rescale_hybrid, moai_multiply_relin_rescale_hybrid and the list form: the centred value of
 *     q_{L-1} (out_0 + out_1 s) - (c_0 + c_1 s + c_2 s^2) mod Q_L is at most beta(L) N alpha 21 D_max / P + q_{L-1} (1/2 + 2^-40)(1 + |s|_1);
 *     u'_p = 0 outside the 2^-40 band, and each coefficient of (out - composition) mod Q_{L-1}, centred, lies in [-1, +1] instead of
 *     [-(alpha + 1), +1].  It is still NOT the composition's bits: the merged form rounds once, the composition twice.
 * In every bound the first term, the key noise with the mod-up's approximation, is unchanged.
 *
 * Neither call below launches or synchronises anything.  The exact mode adds no synchronisation and no launch to any call (the same
 * conversion launch runs another instantiation of its kernel), uses the same scratch, works under HIP-graph stream capture wherever
 * the fast mode does, and its constants are part of the per-(L, alpha) blocks whatever the mode, so setting it builds nothing.
 * moai_op_trace counts are unchanged: a mode is not an operation.  A set while another thread is inside a hybrid call of the same
 * context takes effect for the calls entered after it.
 * Refusals: MOAI_EINVAL with a message for a null context, a null `mode` pointer, a mode that is neither of the two below. */
#define MOAI_HYBRID_ROUND_FAST 0  /* the default: the fast conversion, the bits of every release before the mode existed */
#define MOAI_HYBRID_ROUND_EXACT 1 /* the overflow of every mod-down estimated in binary64 and removed */
int moai_hybrid_set_rounding(moai_ctx *ctx, int mode);
int moai_hybrid_rounding(const moai_ctx *ctx, int *mode);

/* ---- stream audit (debug)----------------------------------------------------------------------------------------
 * A caller that recycles device blocks in a stream-ordered cache (the seal:: shim's util::DevicePool: a released block may be
 * handed out again on the SAME stream without synchronising, which is only safe when everything that touches the block is
 * enqueued on that stream) can have that invariant checked.  With MOAI_STREAM_AUDIT=1 in the environment, or after
 * moai_debug_stream_audit(1), moai_debug_block_label records the stream a block belongs to (state 1 = in use, 2 = released to
 * the cache, 0 = forget: back to the device allocator), and every entry point above that enqueues work fails with MOAI_ELOGIC
 * (and a line on stderr naming the function, the pointer and both streams) when handed a device pointer inside a block
 * labelled with another stream or inside a released block.  Unlabelled memory is not checked.  The reference's counterpart is
 * the single-threaded ownership of its MemoryPoolMT blocks (SEAL/util/mempool.h:228); it has no device streams.
 * moai_debug_stream_audit returns the previous setting; _counts reports pointers checked / violations found so far. */
int moai_debug_stream_audit(int enable);
void moai_debug_block_label(const void *ptr, size_t bytes, const void *stream, int state);
void moai_debug_stream_audit_counts(unsigned long long *checked, unsigned long long *violations);

/* ---- operation census ----------------------------------------------------------------------------------------------
 * moai_op_trace(1) clears and starts, moai_op_trace(0) stops counting what the entry points above were asked to do:
 * per (entry point, level L) the sum of the call's own batch argument (polynomials for the element-wise and NTT calls,
 * ciphertexts for the scheme-level ones, terms x polynomials for the fused sums).  bench.py uses it to price the same
 * operations on the CPU oracle.  moai_op_trace_dump writes "name L count" lines (NUL-terminated, truncated to cap)
 * and returns the size the whole text needs.  Off by default; costs one relaxed atomic load per call. */
int moai_op_trace(int enable);
size_t moai_op_trace_dump(char *buf, size_t cap);

/* ---- measurement support -----------------------------------------------------------------------------------
 * Average duration in milliseconds of the NTT kernels of the last moai_ntt_* call recorded with
 * HIP events on the caller's stream is not provided here; callers time with their own events
 * around the calls (bench.py does).  moai_device_info fills name (<= 255 chars) and CU count. */
int moai_device_info(int device, char *name, size_t name_cap, int *compute_units, size_t *hbm_bytes);
/* free and total device memory of the current device (hipMemGetInfo) */
int moai_mem_info(size_t *free_bytes, size_t *total_bytes);
/* hipEvent helpers so that pure-C / ctypes callers can time the stream the kernels run on */
int moai_event_create(void **event);
int moai_event_destroy(void *event);
int moai_event_record(void *event, void *stream);
int moai_event_synchronize(void *event);
int moai_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */

#ifdef __cplusplus
}
#endif
#endif
