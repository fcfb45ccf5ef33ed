// client.hip -- the client's input path on the device: a counter-based ChaCha20 generator, the samplers built on it
// (SEAL/util/rlwe.cpp:99-135 sample_poly_cbd, :137-183 sample_poly_uniform, :14-38 sample_poly_ternary), symmetric and
// public-key encryption (SEAL/util/rlwe.cpp:224-383, SEAL/encryptor.cpp:88-173) and switching-key generation
// (SEAL/keygenerator.cpp:303-336).  The stream contract (which words of which block feed which coefficient) is specified in
// include/moai_hip.h, section "client randomness and encryption"; tests/client_sampling.py restates it.
//
// Every sample is a function of (key, nonce, coefficient index) only: a thread computes the one ChaCha20 block its
// coefficients take and nothing depends on the launch geometry.
//
//   cl_uniform      : 4 coefficients (one block of 8 words) per thread, (hi * 2^64 + lo) mod q exactly (mod128)
//   cl_small        : 8 coefficients (one block) per thread, ternary or CBD, written as residues in every requested row
//   cl_sym_finish   : c1 = uniform a generated in place (NTT form, as SEAL samples it), c0 = e - a s (+ m) (+ (p mod q_J) s' in
//                     row J of a key digit); c1 is never stored before this kernel, and in the seeded form (a from a public seed,
//                     SEAL/util/rlwe.cpp:353-363) not stored at all
//                     A_MEM: a is not drawn but read from scratch [nb][L][N] that sealprng.hip's fill and fix-up kernels have
//                     just written on the same stream from a SEAL seed per ciphertext (the SEAL-seeded entry points)
//   cl_expand       : c1 of a seeded object drawn again from its seed beside a copy of c0 (Ciphertext::expand_seed)
//   FULLPOS (both)  : the rows are a selection {0 .. levels-1, k-1} of a key digit's k rows that keeps the FULL draw's stream
//                     positions (row r under prime p takes the words of row p), and sk / newkey stay full [k][N] keys read at
//                     row p: a level-limited key is word for word the trim of the full one (moai_kswitch_keygen_limited)
//   cl_pk_finish    : c_i = pk_i u + e_i over the rows of the previous level, u read once; then the existing rescale divides by
//                     the dropped prime (divide_and_round_q_last_ntt_inplace) and cl_add_c0 adds the plaintext to c0
#include <algorithm>
#include <mutex>

#include "launch.h"
#include "modarith.hip.h"

namespace moai {

struct ChaKey
{
    uint32_t w[8];
};

// purposes of the nonce (nonce = purpose << 56 | sequence), include/moai_hip.h
constexpr uint64_t CL_UNIFORM = 1, CL_TERNARY = 2, CL_NOISE0 = 3, CL_NOISE1 = 4;
constexpr uint64_t CL_SEQ_LIMIT = 1ull << 56;
// (purposes 5 and 6, the public ChaCha20 seed and the SEAL seed of a seeded object, are drawn on the host by the seal:: shim)

// where cl_sym_finish takes a from
enum
{
    A_CHACHA, // drawn in the kernel from (key, nonce_a + b)
    A_MEM     // read from SymArgs::a
};

__device__ __forceinline__ uint32_t rotl32(uint32_t v, int c)
{
    return (v << c) | (v >> (32 - c)); // one v_alignbit_b32
}

#define CL_QR(a, b, c, d)                 \
    x[a] += x[b];                         \
    x[d] = rotl32(x[d] ^ x[a], 16);       \
    x[c] += x[d];                         \
    x[b] = rotl32(x[b] ^ x[c], 12);       \
    x[a] += x[b];                         \
    x[d] = rotl32(x[d] ^ x[a], 8);        \
    x[c] += x[d];                         \
    x[b] = rotl32(x[b] ^ x[c], 7);

// RFC 8439 block function with a 64-bit counter in state words 12-13 and a 64-bit nonce in 14-15 (the layout of the host
// seal::util::ChaCha20Rng): out[16] = the block's 32-bit words
__device__ __forceinline__ void chacha_block(const ChaKey &k, uint64_t nonce, uint64_t ctr, uint32_t out[16])
{
    uint32_t s[16] = { 0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, k.w[0], k.w[1], k.w[2], k.w[3], k.w[4], k.w[5], k.w[6],
                       k.w[7], (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)nonce, (uint32_t)(nonce >> 32) };
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++)
    {
        x[i] = s[i];
    }
#pragma unroll
    for (int i = 0; i < 10; i++)
    {
        CL_QR(0, 4, 8, 12)
        CL_QR(1, 5, 9, 13)
        CL_QR(2, 6, 10, 14)
        CL_QR(3, 7, 11, 15)
        CL_QR(0, 5, 10, 15)
        CL_QR(1, 6, 11, 12)
        CL_QR(2, 7, 8, 13)
        CL_QR(3, 4, 9, 14)
    }
#pragma unroll
    for (int i = 0; i < 16; i++)
    {
        out[i] = x[i] + s[i];
    }
}
#undef CL_QR

// (hi * 2^64 + lo) mod q exactly, for ANY 128-bit value.  barrett128's truncated quotient (the low word of lo * cr0 is dropped)
// is below the true one by less than 3 for inputs up to 2^128: the remainder before its subtraction is below 3q, so a second
// conditional subtraction makes the result canonical always, not only for the products below q^2 the shared routine serves
__device__ __forceinline__ uint64_t mod128(uint64_t lo, uint64_t hi, const PrimeConst &pc)
{
    return csub(barrett128(lo, hi, pc.q, pc.cr0, pc.cr1), pc.q);
}

__device__ __forceinline__ uint64_t word64(const uint32_t b[16], int w)
{
    return (uint64_t)b[2 * w] | ((uint64_t)b[2 * w + 1] << 32);
}

// ((3 w) >> 64) - 1 in {-1, 0, 1}
__device__ __forceinline__ int ternary_of(uint64_t w)
{
    return (int)__umul64hi(w, 3ull) - 1;
}

// SEAL's cbd(): bytes x[0..5] of the word, x[2] and x[5] masked to 5 bits (rlwe.cpp:105-113)
__device__ __forceinline__ int cbd_of(uint64_t w)
{
    const uint32_t lo = (uint32_t)w & 0x1fffffu;
    const uint32_t hi = (uint32_t)(w >> 24) & 0x1fffffu;
    return __popc(lo) - __popc(hi);
}

// ---- raw samplers -----------------------------------------------------------------------------------------------------
struct UniformArgs
{
    ChaKey key;
    uint64_t nonce;  // polynomial p uses nonce + p
    uint64_t *out;   // polynomial p at out + p * stride
    size_t stride;   // words
    const PrimeConst *pc;
    RowMap rows;
    uint32_t L;
    uint32_t logn;
};

__global__ __launch_bounds__(256) void cl_uniform(UniformArgs g)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x; // block index of the stream = (r N + i) / 4
    if (t >= (g.L << g.logn) >> 2)
    {
        return;
    }
    const uint32_t p = blockIdx.y;
    const uint32_t f = t << 2;
    const uint32_t r = f >> g.logn;
    const PrimeConst &pc = g.pc[g.rows.idx[r]];
    uint32_t b[16];
    chacha_block(g.key, g.nonce + p, t, b);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(g.out + (size_t)p * g.stride + f);
    ulonglong2 v0, v1;
    v0.x = mod128(word64(b, 0), word64(b, 1), pc);
    v0.y = mod128(word64(b, 2), word64(b, 3), pc);
    v1.x = mod128(word64(b, 4), word64(b, 5), pc);
    v1.y = mod128(word64(b, 6), word64(b, 7), pc);
    dst[0] = v0;
    dst[1] = v1;
}

struct SmallArgs
{
    ChaKey key;
    uint64_t nonce; // polynomial p uses nonce + p
    uint64_t *out;  // polynomial p at out + p * stride, rows [L][N]
    size_t stride;
    const PrimeConst *pc;
    RowMap rows;
    uint32_t L;
    uint32_t logn;
};

template <bool CBD>
__global__ __launch_bounds__(256) void cl_small(SmallArgs g)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x; // coefficients 8t .. 8t+7
    if (t >= (1u << g.logn) >> 3)
    {
        return;
    }
    const uint32_t p = blockIdx.y;
    uint32_t b[16];
    chacha_block(g.key, g.nonce + p, t, b);
    int v[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
    {
        v[j] = CBD ? cbd_of(word64(b, j)) : ternary_of(word64(b, j));
    }
    uint64_t *base = g.out + (size_t)p * g.stride + ((size_t)t << 3);
    for (uint32_t r = 0; r < g.L; r++)
    {
        const uint64_t q = g.pc[g.rows.idx[r]].q;
        ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(base + ((size_t)r << g.logn));
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            ulonglong2 w;
            // the residue of a small signed integer: v + (v < 0 ? q : 0)  (SEAL's flag & q)
            w.x = (uint64_t)(int64_t)v[2 * j] + (v[2 * j] < 0 ? q : 0);
            w.y = (uint64_t)(int64_t)v[2 * j + 1] + (v[2 * j + 1] < 0 ? q : 0);
            dst[j] = w;
        }
    }
}

// ---- symmetric encryption / key digits --------------------------------------------------------------------------------
struct SymArgs
{
    ChaKey key;             // the stream a is drawn from: the caller's one key, or the public seed of a seeded object
    uint64_t nonce_a;       // ciphertext b (of this launch) draws a with nonce_a + b
    const uint64_t *a;      // A_MEM: [nb][L][N] NTT form, a of ciphertext b instead of the draw
    const uint64_t *e;      // [nb][L][N] NTT form
    const uint64_t *sk;     // [L][N]; FULLPOS: [k][N], row r read at its prime's index
    const uint64_t *plain;  // [nb][L][N] or null
    const uint64_t *newkey; // [L][N] ([k][N] with FULLPOS) or null: key digit b adds fac[b] * newkey[b] in row b of c0
    uint64_t *out;          // [nb][2][L][N]; seeded form: c0 only, [nb][L][N]
    uint32_t digit0;        // digit of ciphertext 0 of this launch
    const PrimeConst *pc;
    RowMap rows;
    uint64_t fac[MOAI_MAX_RNS];
    uint32_t L;
    uint32_t logn;
};

template <int A_SRC, bool SEEDED, bool FULLPOS>
__global__ __launch_bounds__(256) void cl_sym_finish(SymArgs g)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (g.L << g.logn) >> 2)
    {
        return;
    }
    const uint32_t b = blockIdx.y;
    const uint32_t f = t << 2;
    const uint32_t r = f >> g.logn;
    const size_t LN = (size_t)g.L << g.logn;
    const uint32_t p = g.rows.idx[r];
    const PrimeConst &pc = g.pc[p];
    const uint64_t q = pc.q;
    // coefficient offset of this thread in the full [k][N] layout (sk, newkey and the stream position), else the compact one
    const uint32_t ff = FULLPOS ? (p << g.logn) + (f & ((1u << g.logn) - 1)) : f;
    uint64_t a[4];
    if (A_SRC == A_MEM)
    {
        const ulonglong2 *a2 = reinterpret_cast<const ulonglong2 *>(g.a + b * LN + f);
        const ulonglong2 a01 = a2[0], a23 = a2[1];
        a[0] = a01.x;
        a[1] = a01.y;
        a[2] = a23.x;
        a[3] = a23.y;
    }
    else
    {
        uint32_t blk[16];
        chacha_block(g.key, g.nonce_a + b, ff >> 2, blk);
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            a[j] = mod128(word64(blk, 2 * j), word64(blk, 2 * j + 1), pc);
        }
    }
    const ulonglong2 *e2 = reinterpret_cast<const ulonglong2 *>(g.e + b * LN + f);
    const ulonglong2 *s2 = reinterpret_cast<const ulonglong2 *>(g.sk + ff);
    uint64_t c0[4];
    {
        ulonglong2 e01 = e2[0], e23 = e2[1], s01 = s2[0], s23 = s2[1];
        const uint64_t ev[4] = { e01.x, e01.y, e23.x, e23.y };
        const uint64_t sv[4] = { s01.x, s01.y, s23.x, s23.y };
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const uint64_t as = mulmod_barrett(a[j], sv[j], q, pc.cr0, pc.cr1);
            c0[j] = submod(ev[j], as, q);
        }
    }
    if (g.plain)
    {
        const ulonglong2 *p2 = reinterpret_cast<const ulonglong2 *>(g.plain + b * LN + f);
        ulonglong2 p01 = p2[0], p23 = p2[1];
        const uint64_t pv[4] = { p01.x, p01.y, p23.x, p23.y };
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            c0[j] = csub(c0[j] + pv[j], q);
        }
    }
    if (g.newkey && r == g.digit0 + b)
    {
        const ulonglong2 *k2 = reinterpret_cast<const ulonglong2 *>(g.newkey + ff);
        ulonglong2 k01 = k2[0], k23 = k2[1];
        const uint64_t kv[4] = { k01.x, k01.y, k23.x, k23.y };
        const uint64_t fac = g.fac[r];
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            c0[j] = csub(c0[j] + mulmod_barrett(kv[j], fac, q, pc.cr0, pc.cr1), q);
        }
    }
    ulonglong2 *o0 = reinterpret_cast<ulonglong2 *>(g.out + (SEEDED ? 1 : 2) * b * LN + f);
    o0[0] = make_ulonglong2(c0[0], c0[1]);
    o0[1] = make_ulonglong2(c0[2], c0[3]);
    if (!SEEDED)
    {
        ulonglong2 *o1 = reinterpret_cast<ulonglong2 *>(g.out + (2 * b + 1) * LN + f);
        o1[0] = make_ulonglong2(a[0], a[1]);
        o1[1] = make_ulonglong2(a[2], a[3]);
    }
}

// ---- seeded objects ---------------------------------------------------------------------------------------------------
struct ExpandArgs
{
    ChaKey seed;
    uint64_t nonce;     // object b draws c1 with nonce + b
    const uint64_t *c0; // [count][L][N]
    uint64_t *out;      // [count][2][L][N]
    const PrimeConst *pc;
    RowMap rows;
    uint32_t L;
    uint32_t logn;
};

template <bool FULLPOS>
__global__ __launch_bounds__(256) void cl_expand(ExpandArgs g)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x; // block index of the stream, as in cl_uniform (FULLPOS: see cl_sym_finish)
    if (t >= (g.L << g.logn) >> 2)
    {
        return;
    }
    const uint32_t b = blockIdx.y;
    const uint32_t f = t << 2;
    const size_t LN = (size_t)g.L << g.logn;
    const uint32_t p = g.rows.idx[f >> g.logn];
    const PrimeConst &pc = g.pc[p];
    const uint32_t tpos = FULLPOS ? ((p << g.logn) + (f & ((1u << g.logn) - 1))) >> 2 : t;
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(g.c0 + b * LN + f);
    const ulonglong2 c01 = src[0], c23 = src[1];
    uint32_t blk[16];
    chacha_block(g.seed, g.nonce + b, tpos, blk);
    ulonglong2 *o0 = reinterpret_cast<ulonglong2 *>(g.out + 2 * b * LN + f);
    ulonglong2 *o1 = reinterpret_cast<ulonglong2 *>(g.out + (2 * b + 1) * LN + f);
    o0[0] = c01;
    o0[1] = c23;
    o1[0] = make_ulonglong2(mod128(word64(blk, 0), word64(blk, 1), pc), mod128(word64(blk, 2), word64(blk, 3), pc));
    o1[1] = make_ulonglong2(mod128(word64(blk, 4), word64(blk, 5), pc), mod128(word64(blk, 6), word64(blk, 7), pc));
}

// ---- public-key encryption --------------------------------------------------------------------------------------------
struct PkArgs
{
    const uint64_t *u;     // [nb][M][N] NTT form
    const uint64_t *e;     // [nb][2][M][N] NTT form
    const uint64_t *pk;    // [2][k][N]: rows [0, M) of each polynomial are read
    const uint64_t *plain; // [nb][M][N] or null (key level only)
    uint64_t *out;         // [nb][2][M][N] (may be e)
    const PrimeConst *pc;
    size_t pk_poly;        // k N
    uint32_t M;
    uint32_t logn;
};

__global__ __launch_bounds__(256) void cl_pk_finish(PkArgs g)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x; // coefficient pair 2t, 2t+1 of the rows
    if (t >= (g.M << g.logn) >> 1)
    {
        return;
    }
    const uint32_t b = blockIdx.y;
    const uint32_t f = t << 1;
    const uint32_t r = f >> g.logn;
    const size_t MN = (size_t)g.M << g.logn;
    const PrimeConst &pc = g.pc[r];
    const uint64_t q = pc.q;
    const ulonglong2 u = *reinterpret_cast<const ulonglong2 *>(g.u + b * MN + f);
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
        const ulonglong2 pk = *reinterpret_cast<const ulonglong2 *>(g.pk + i * g.pk_poly + f);
        const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(g.e + (2 * b + i) * MN + f);
        ulonglong2 c;
        c.x = csub(mulmod_barrett(pk.x, u.x, q, pc.cr0, pc.cr1) + e.x, q);
        c.y = csub(mulmod_barrett(pk.y, u.y, q, pc.cr0, pc.cr1) + e.y, q);
        if (i == 0 && g.plain)
        {
            const ulonglong2 m = *reinterpret_cast<const ulonglong2 *>(g.plain + b * MN + f);
            c.x = csub(c.x + m.x, q);
            c.y = csub(c.y + m.y, q);
        }
        *reinterpret_cast<ulonglong2 *>(g.out + (2 * b + i) * MN + f) = c;
    }
}

// ct[b][0] += plain[b] over L rows (primes 0..L-1)
__global__ __launch_bounds__(256) void cl_add_c0(uint64_t *ct, const uint64_t *plain, const PrimeConst *pc, uint32_t L, uint32_t logn)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (L << logn) >> 1)
    {
        return;
    }
    const uint32_t b = blockIdx.y;
    const uint32_t f = t << 1;
    const uint64_t q = pc[f >> logn].q;
    const size_t LN = (size_t)L << logn;
    ulonglong2 *c = reinterpret_cast<ulonglong2 *>(ct + 2 * b * LN + f);
    const ulonglong2 m = *reinterpret_cast<const ulonglong2 *>(plain + b * LN + f);
    ulonglong2 v = *c;
    v.x = csub(v.x + m.x, q);
    v.y = csub(v.y + m.y, q);
    *c = v;
}

// ---- host side --------------------------------------------------------------------------------------------------------
static ChaKey load_key(const uint8_t *key)
{
    ChaKey k;
    for (int i = 0; i < 8; i++)
    {
        k.w[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) |
                 ((uint32_t)key[4 * i + 3] << 24);
    }
    return k;
}

static dim3 grid_of(size_t threads, size_t y)
{
    return dim3((uint32_t)((threads + 255) / 256), (uint32_t)y);
}

static int launch_small(moai_ctx *c, bool cbd, const ChaKey &key, uint64_t nonce, uint64_t *out, size_t stride, size_t n_poly,
                        size_t L, const RowMap &rows, hipStream_t s)
{
    SmallArgs a;
    a.key = key;
    a.nonce = nonce;
    a.out = out;
    a.stride = stride;
    a.pc = c->pc;
    a.rows = rows;
    a.L = (uint32_t)L;
    a.logn = (uint32_t)c->logn;
    hipLaunchKernelGGL(cbd ? cl_small<true> : cl_small<false>, grid_of(c->n / 8, n_poly), dim3(256), 0, s, a);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

// items per chunk (launch.h chunk_items): within the stream's arena or MOAI_CLIENT_TMP_KB (1 GiB), whichever is larger
static size_t chunk_floor()
{
    return (size_t)std::max(1l, tuning(K_CLIENT_TMP_KB)) << 10;
}

// what every entry point checks first; the samplers, which take a raw nonce, pass seq = count = 0
static int check_common(const moai_ctx *c, const uint8_t *key, uint64_t seq, size_t count)
{
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (!key)
    {
        return set_error(MOAI_EINVAL, "null key");
    }
    if (c->logn < 3)
    {
        return set_error(MOAI_ELOGIC, "client sampling needs N >= 8");
    }
    if (seq >= CL_SEQ_LIMIT || count > CL_SEQ_LIMIT - seq)
    {
        return set_error(MOAI_EINVAL, "nonce range [%llu, +%zu) exceeds 2^56", (unsigned long long)seq, count);
    }
    if (count > 65535)
    {
        return set_error(MOAI_EINVAL, "at most 65535 ciphertexts per call");
    }
    return MOAI_OK;
}

// symmetric encryptions (newkey == null) or the digits of a switching key: ciphertext b uses sequence seq + b.  seed == null:
// a and e from `key`, out [n_batch][2][L][N]; otherwise e from `key`, a from `seed`, and out holds c0 only, [n_batch][L][N].
// fullpos: sk and newkey are full [k][N] keys and a keeps the stream positions of the full k-row draw (cl_sym_finish FULLPOS)
// seal_seeds (with seed == null, never with fullpos): host [n_batch][64]; a of ciphertext b is SEAL's sample_poly_uniform of
// seal_seeds[b], expanded per chunk into scratch beside e, out holds c0 only, and `rejected` is moai_seal_sample_uniform's
static int sym_impl(moai_ctx *c, const uint8_t *key, const uint8_t *seed, uint64_t seq, const uint64_t *sk, const uint64_t *plain,
                    const uint64_t *newkey, uint64_t *out, size_t n_batch, size_t L, const RowMap &rows, bool fullpos, hipStream_t s,
                    const uint8_t *seal_seeds = nullptr, uint32_t *rejected = nullptr)
{
    MOAI_TRY(enter_device(c));
    const ChaKey k = load_key(key);
    const size_t n = c->n, LN = L * n;
    const bool c0_only = seed || seal_seeds;
    SymArgs a;
    a.key = seed ? load_key(seed) : k;
    a.a = nullptr;
    a.sk = sk;
    a.newkey = newkey;
    a.pc = c->pc;
    a.rows = rows;
    a.L = (uint32_t)L;
    a.logn = (uint32_t)c->logn;
    for (size_t r = 0; r < MOAI_MAX_RNS; r++)
    {
        // SEAL/keygenerator.cpp:315-319: the special prime modulo q_J
        a.fac[r] = r < L ? c->primes[c->k - 1] % c->primes[rows.idx[r]] : 0;
    }
    std::lock_guard<std::mutex> op(*static_cast<std::mutex *>(c->op_mutex));
    // scratch per ciphertext: e [L][N]; from SEAL seeds also a [L][N] and the sampler's mark counts [L]
    const size_t per = seal_seeds ? 2 * LN * sizeof(uint64_t) + L * sizeof(uint32_t) : LN * sizeof(uint64_t);
    const size_t cb = chunk_items(c, s, per, n_batch, 65535, chunk_floor());
    void *scratch = nullptr;
    MOAI_TRY(workspace(c, cb * per, s, &scratch));
    uint64_t *e = static_cast<uint64_t *>(scratch);
    uint64_t *a_mem = e + cb * LN;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(a_mem + cb * LN);
    return for_chunks(n_batch, cb, [&](size_t b0, size_t nb) {
        if (seal_seeds)
        {
            MOAI_TRY(seal_uniform_launch(c, seal_seeds + b0 * 64, a_mem, LN, nb, L, rows, cnt, rejected, s));
            a.a = a_mem;
        }
        MOAI_TRY(launch_small(c, true, k, (CL_NOISE0 << 56) | (seq + b0), e, LN, nb, L, rows, s));
        MOAI_TRY(ntt_launch(c, e, nb, L, rows, false, s));
        a.nonce_a = (CL_UNIFORM << 56) | (seq + b0);
        a.e = e;
        a.plain = plain ? plain + b0 * LN : nullptr;
        a.out = out + b0 * (c0_only ? 1 : 2) * LN;
        a.digit0 = (uint32_t)b0;
        return dispatch<A_CHACHA, A_MEM>("source of a ", seal_seeds ? A_MEM : A_CHACHA, [&](auto src) {
            constexpr int SRC = decltype(src)::value;
            void (*kernel)(SymArgs) = cl_sym_finish<SRC, true, false>; // a from memory exists in this form only
            if constexpr (SRC == A_CHACHA)
            {
                kernel = fullpos ? (seed ? cl_sym_finish<SRC, true, true> : cl_sym_finish<SRC, false, true>)
                                 : (seed ? cl_sym_finish<SRC, true, false> : cl_sym_finish<SRC, false, false>);
            }
            hipLaunchKernelGGL(kernel, grid_of(LN / 4, nb), dim3(256), 0, s, a);
            MOAI_LAUNCH_CHECK();
            return MOAI_OK;
        });
    });
}

} // namespace moai

using namespace moai;

static int sampler_entry(moai_ctx *c, int kind, const uint8_t *key, uint64_t nonce, uint64_t *out, size_t n_poly, size_t L,
                         const uint32_t *prime_index, void *stream)
{
    MOAI_TRY(check_common(c, key, 0, 0));
    RowMap rows;
    MOAI_TRY(rows_entry(c, L, prime_index, &rows));
    if (n_poly == 0)
    {
        return MOAI_OK;
    }
    if (n_poly > 65535)
    {
        return set_error(MOAI_EINVAL, "at most 65535 polynomials per call");
    }
    if (nonce + (n_poly - 1) < nonce)
    {
        return set_error(MOAI_EINVAL, "nonce range wraps around 2^64");
    }
    if (!out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    MOAI_TRY(enter_device(c));
    hipStream_t s = (hipStream_t)stream;
    const ChaKey k = load_key(key);
    const size_t LN = L * c->n;
    if (kind == 0)
    {
        UniformArgs a;
        a.key = k;
        a.nonce = nonce;
        a.out = out;
        a.stride = LN;
        a.pc = c->pc;
        a.rows = rows;
        a.L = (uint32_t)L;
        a.logn = (uint32_t)c->logn;
        hipLaunchKernelGGL(cl_uniform, grid_of(LN / 4, n_poly), dim3(256), 0, s, a);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    }
    return launch_small(c, kind == 2, k, nonce, out, LN, n_poly, L, rows, s);
}

// the three samplers: kind 0 uniform, 1 ternary, 2 centred binomial
#define MOAI_SAMPLER(name, kind)                                                                                                  \
    extern "C" int moai_sample_##name(moai_ctx *c, const uint8_t *key, uint64_t nonce, uint64_t *out, size_t n_poly, size_t L,   \
                                      const uint32_t *prime_index, void *stream)                                                 \
    {                                                                                                                             \
        MOAI_AUDIT(stream, out);                                                                                                  \
        trace_op("sample_" #name, L, n_poly);                                                                                     \
        return sampler_entry(c, kind, key, nonce, out, n_poly, L, prime_index, stream);                                           \
    }
MOAI_SAMPLER(uniform, 0)
MOAI_SAMPLER(ternary, 1)
MOAI_SAMPLER(cbd, 2)
#undef MOAI_SAMPLER

static int encrypt_symmetric_entry(moai_ctx *c, const uint8_t *key, const uint8_t *seed, uint64_t seq, const uint64_t *sk_ntt,
                                   const uint64_t *plain, uint64_t *out, size_t n_batch, size_t L, const uint32_t *prime_index,
                                   void *stream, const uint8_t *seal_seeds = nullptr, uint32_t *rejected = nullptr)
{
    MOAI_TRY(check_common(c, key, seq, n_batch));
    RowMap rows;
    MOAI_TRY(rows_entry(c, L, prime_index, &rows));
    if (n_batch == 0)
    {
        return MOAI_OK;
    }
    if (!sk_ntt || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    return sym_impl(c, key, seed, seq, sk_ntt, plain, nullptr, out, n_batch, L, rows, false, (hipStream_t)stream, seal_seeds, rejected);
}

extern "C" int moai_encrypt_symmetric(moai_ctx *c, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, const uint64_t *plain,
                                      uint64_t *out, size_t n_batch, size_t L, const uint32_t *prime_index, void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, plain, out);
    trace_op("encrypt_symmetric", L, n_batch);
    return encrypt_symmetric_entry(c, key, nullptr, seq, sk_ntt, plain, out, n_batch, L, prime_index, stream);
}

extern "C" int moai_encrypt_symmetric_seeded(moai_ctx *c, const uint8_t *noise_key, const uint8_t *seed, uint64_t seq,
                                             const uint64_t *sk_ntt, const uint64_t *plain, uint64_t *out_c0, size_t n_batch, size_t L,
                                             const uint32_t *prime_index, void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, plain, out_c0);
    trace_op("encrypt_symmetric_seeded", L, n_batch);
    if (c && noise_key && !seed)
    {
        return set_error(MOAI_EINVAL, "null seed");
    }
    return encrypt_symmetric_entry(c, noise_key, seed, seq, sk_ntt, plain, out_c0, n_batch, L, prime_index, stream);
}

namespace moai {
int encrypt_zero_key_level(moai_ctx *c, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, uint64_t *out, size_t n_batch,
                           hipStream_t s)
{
    return encrypt_symmetric_entry(c, key, nullptr, seq, sk_ntt, nullptr, out, n_batch, c ? c->k : 0, nullptr, (void *)s);
}
} // namespace moai

static int kswitch_keygen_entry(moai_ctx *c, const uint8_t *key, const uint8_t *seed, uint64_t seq, const uint64_t *sk_ntt,
                                const uint64_t *new_key_ntt, uint64_t *out, void *stream, const uint8_t *seal_seeds = nullptr,
                                uint32_t *rejected = nullptr)
{
    if (c->k < 2)
    {
        return set_error(MOAI_ELOGIC, "keyswitching is not supported by the context");
    }
    const size_t digits = c->k - 1;
    MOAI_TRY(check_common(c, key, seq, digits));
    if (!sk_ntt || !new_key_ntt || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    RowMap rows;
    MOAI_TRY(make_rowmap(c, c->k, nullptr, &rows));
    return sym_impl(c, key, seed, seq, sk_ntt, nullptr, new_key_ntt, out, digits, c->k, rows, false, (hipStream_t)stream, seal_seeds,
                    rejected);
}

extern "C" int moai_kswitch_keygen(moai_ctx *c, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt, const uint64_t *new_key_ntt,
                                   uint64_t *out, void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, new_key_ntt, out);
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    trace_op("kswitch_keygen", c->k, c->k - 1);
    return kswitch_keygen_entry(c, key, nullptr, seq, sk_ntt, new_key_ntt, out, stream);
}

extern "C" int moai_kswitch_keygen_seeded(moai_ctx *c, const uint8_t *noise_key, const uint8_t *seed, uint64_t seq,
                                          const uint64_t *sk_ntt, const uint64_t *new_key_ntt, uint64_t *out_c0, void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, new_key_ntt, out_c0);
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    trace_op("kswitch_keygen_seeded", c->k, c->k - 1);
    if (noise_key && !seed)
    {
        return set_error(MOAI_EINVAL, "null seed");
    }
    return kswitch_keygen_entry(c, noise_key, seed, seq, sk_ntt, new_key_ntt, out_c0, stream);
}

extern "C" int moai_encrypt_symmetric_seal_seeded(moai_ctx *c, const uint8_t *noise_key, const uint8_t *seeds, uint64_t seq,
                                                  const uint64_t *sk_ntt, const uint64_t *plain, uint64_t *out_c0, size_t n_batch, size_t L,
                                                  const uint32_t *prime_index, uint32_t *rejected, void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, plain, out_c0, rejected);
    trace_op("encrypt_symmetric_seal_seeded", L, n_batch);
    if (c && noise_key && !seeds)
    {
        return set_error(MOAI_EINVAL, "null seed");
    }
    return encrypt_symmetric_entry(c, noise_key, nullptr, seq, sk_ntt, plain, out_c0, n_batch, L, prime_index, stream, seeds, rejected);
}

extern "C" int moai_kswitch_keygen_seal_seeded(moai_ctx *c, const uint8_t *noise_key, const uint8_t *seeds, uint64_t seq,
                                               const uint64_t *sk_ntt, const uint64_t *new_key_ntt, uint64_t *out_c0, uint32_t *rejected,
                                               void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, new_key_ntt, out_c0, rejected);
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    trace_op("kswitch_keygen_seal_seeded", c->k, c->k - 1);
    if (noise_key && !seeds)
    {
        return set_error(MOAI_EINVAL, "null seed");
    }
    return kswitch_keygen_entry(c, noise_key, nullptr, seq, sk_ntt, new_key_ntt, out_c0, stream, seeds, rejected);
}

extern "C" int moai_expand_seeded(moai_ctx *c, const uint8_t *seed, uint64_t seq, const uint64_t *c0, uint64_t *out, size_t count, size_t L,
                                  const uint32_t *prime_index, void *stream)
{
    MOAI_AUDIT(stream, c0, out);
    trace_op("expand_seeded", L, count);
    MOAI_TRY(check_common(c, seed, seq, count));
    ExpandArgs a;
    MOAI_TRY(rows_entry(c, L, prime_index, &a.rows));
    if (count == 0)
    {
        return MOAI_OK;
    }
    if (!c0 || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t LN = L * c->n;
    if (overlap(c0, count * LN * 8, out, 2 * count * LN * 8))
    {
        return set_error(MOAI_EINVAL, "c0 and out overlap");
    }
    MOAI_TRY(enter_device(c));
    a.seed = load_key(seed);
    a.nonce = (CL_UNIFORM << 56) | seq;
    a.c0 = c0;
    a.out = out;
    a.pc = c->pc;
    a.L = (uint32_t)L;
    a.logn = (uint32_t)c->logn;
    hipLaunchKernelGGL(cl_expand<false>, grid_of(LN / 4, count), dim3(256), 0, (hipStream_t)stream, a);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

// ---- keys limited to a chain index (born in moai_key_trim's layout) -------------------------------------------------------------
// the rows of a key limited to `levels` data primes, {0 .. levels-1, k-1}, after the checks every limited entry point shares
static int limited_rows(const moai_ctx *c, size_t levels, RowMap *rows)
{
    if (!c)
    {
        return set_error(MOAI_EINVAL, "null context");
    }
    if (c->k < 2)
    {
        return set_error(MOAI_ELOGIC, "keyswitching is not supported by the context");
    }
    if (levels < 1 || levels > c->k - 1)
    {
        return set_error(MOAI_EINVAL, "levels must lie in 1 .. %zu", c->k - 1);
    }
    uint32_t idx[MOAI_MAX_RNS];
    for (size_t r = 0; r < levels; r++)
    {
        idx[r] = (uint32_t)r;
    }
    idx[levels] = (uint32_t)(c->k - 1);
    return make_rowmap(c, levels + 1, idx, rows);
}

static int kswitch_keygen_limited_entry(moai_ctx *c, const uint8_t *key, const uint8_t *seed, uint64_t seq, const uint64_t *sk_ntt,
                                        const uint64_t *new_key_ntt, size_t levels, uint64_t *out, bool record, void *stream)
{
    RowMap rows;
    MOAI_TRY(limited_rows(c, levels, &rows));
    MOAI_TRY(check_common(c, key, seq, levels));
    if (!sk_ntt || !new_key_ntt || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    if (record)
    {
        MOAI_TRY(moai_key_register(c, out, levels));
    }
    const int rc = sym_impl(c, key, seed, seq, sk_ntt, nullptr, new_key_ntt, out, levels, levels + 1, rows, true, (hipStream_t)stream);
    if (rc && record)
    {
        moai_key_forget(c, out);
    }
    return rc;
}

extern "C" int moai_kswitch_keygen_limited(moai_ctx *c, const uint8_t *key, uint64_t seq, const uint64_t *sk_ntt,
                                           const uint64_t *new_key_ntt, size_t levels, uint64_t *out, void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, new_key_ntt, out);
    trace_op("kswitch_keygen_limited", levels + 1, levels);
    return kswitch_keygen_limited_entry(c, key, nullptr, seq, sk_ntt, new_key_ntt, levels, out, true, stream);
}

extern "C" int moai_kswitch_keygen_limited_seeded(moai_ctx *c, const uint8_t *noise_key, const uint8_t *seed, uint64_t seq,
                                                  const uint64_t *sk_ntt, const uint64_t *new_key_ntt, size_t levels, uint64_t *out_c0,
                                                  void *stream)
{
    MOAI_AUDIT(stream, sk_ntt, new_key_ntt, out_c0);
    trace_op("kswitch_keygen_limited_seeded", levels + 1, levels);
    if (c && noise_key && !seed)
    {
        return set_error(MOAI_EINVAL, "null seed");
    }
    return kswitch_keygen_limited_entry(c, noise_key, seed, seq, sk_ntt, new_key_ntt, levels, out_c0, false, stream);
}

extern "C" int moai_expand_seeded_limited(moai_ctx *c, const uint8_t *seed, uint64_t seq, const uint64_t *c0, size_t levels, uint64_t *out,
                                          void *stream)
{
    MOAI_AUDIT(stream, c0, out);
    trace_op("expand_seeded_limited", levels + 1, levels);
    ExpandArgs a;
    MOAI_TRY(limited_rows(c, levels, &a.rows));
    MOAI_TRY(check_common(c, seed, seq, levels));
    if (!c0 || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    const size_t L = levels + 1, LN = L * c->n;
    if (overlap(c0, levels * LN * 8, out, 2 * levels * LN * 8))
    {
        return set_error(MOAI_EINVAL, "c0 and out overlap");
    }
    MOAI_TRY(enter_device(c));
    MOAI_TRY(moai_key_register(c, out, levels));
    a.seed = load_key(seed);
    a.nonce = (CL_UNIFORM << 56) | seq;
    a.c0 = c0;
    a.out = out;
    a.pc = c->pc;
    a.L = (uint32_t)L;
    a.logn = (uint32_t)c->logn;
    hipLaunchKernelGGL(cl_expand<true>, grid_of(LN / 4, levels), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        moai_key_forget(c, out);
        return set_error(MOAI_EHIP, "cl_expand launch failed: %s", hipGetErrorString(e));
    }
    return MOAI_OK;
}

extern "C" int moai_encrypt_asymmetric(moai_ctx *c, const uint8_t *key, uint64_t seq, const uint64_t *pk, const uint64_t *plain,
                                       uint64_t *out, size_t n_batch, size_t L, void *stream)
{
    MOAI_AUDIT(stream, pk, plain, out);
    trace_op("encrypt_asymmetric", L, n_batch);
    MOAI_TRY(check_common(c, key, seq, n_batch));
    RowMap rows;
    MOAI_TRY(rows_entry(c, L, nullptr, &rows));
    if (n_batch == 0)
    {
        return MOAI_OK;
    }
    if (!pk || !out)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    MOAI_TRY(enter_device(c));
    // SEAL/encryptor.cpp:122-162: below the key level, encrypt at the previous level (one more prime) and divide by it
    const bool divide = L < c->k;
    const size_t M = divide ? L + 1 : L;
    const size_t n = c->n, MN = M * n, LN = L * n;
    MOAI_TRY(make_rowmap(c, M, nullptr, &rows));
    hipStream_t s = (hipStream_t)stream;
    const ChaKey k = load_key(key);
    std::lock_guard<std::mutex> op(*static_cast<std::mutex *>(c->op_mutex));
    // scratch per ciphertext: u, e0, e1 [3][M][N], and the rescale's own workspace [2][M][N] at the head of the arena
    const size_t per = (divide ? 5 : 3) * MN * sizeof(uint64_t);
    const size_t cb = chunk_items(c, s, per, n_batch, 32767, chunk_floor());
    const size_t head = divide ? rescale_ws_bytes(c, M, 2 * cb) : 0;
    void *wsp = nullptr;
    MOAI_TRY(workspace(c, head + 3 * cb * MN * sizeof(uint64_t), s, &wsp));
    uint64_t *u = reinterpret_cast<uint64_t *>(static_cast<char *>(wsp) + head);
    return for_chunks(n_batch, cb, [&](size_t b0, size_t nb) {
        // u [nb][M][N] directly followed by e [nb][2][M][N]: laid out by THIS chunk's count, so that the 3 nb polynomials the
        // transform covers are exactly u and e also when the last chunk is short
        uint64_t *e = u + nb * MN;
        MOAI_TRY(launch_small(c, false, k, (CL_TERNARY << 56) | (seq + b0), u, MN, nb, M, rows, s));
        MOAI_TRY(launch_small(c, true, k, (CL_NOISE0 << 56) | (seq + b0), e, 2 * MN, nb, M, rows, s));
        MOAI_TRY(launch_small(c, true, k, (CL_NOISE1 << 56) | (seq + b0), e + MN, 2 * MN, nb, M, rows, s));
        // u and e are adjacent: one transform of 3 nb polynomials
        MOAI_TRY(ntt_launch(c, u, 3 * nb, M, rows, false, s));
        PkArgs a;
        a.u = u;
        a.e = e;
        a.pk = pk;
        a.plain = divide || !plain ? nullptr : plain + b0 * LN;
        a.out = divide ? e : out + b0 * 2 * LN;
        a.pc = c->pc;
        a.pk_poly = c->k * n;
        a.M = (uint32_t)M;
        a.logn = (uint32_t)c->logn;
        hipLaunchKernelGGL(cl_pk_finish, grid_of(MN / 2, nb), dim3(256), 0, s, a);
        MOAI_LAUNCH_CHECK();
        if (divide)
        {
            // divide_and_round_q_last_ntt_inplace (SEAL/util/rns.cpp:830-901), the rescale's kernels
            MOAI_TRY(rescale_nolock(c, e, out + b0 * 2 * LN, 2, M, nb, s));
            if (plain)
            {
                hipLaunchKernelGGL(cl_add_c0, grid_of(LN / 2, nb), dim3(256), 0, s, out + b0 * 2 * LN, plain + b0 * LN, c->pc,
                                   (uint32_t)L, (uint32_t)c->logn);
                MOAI_LAUNCH_CHECK();
            }
        }
        return MOAI_OK;
    });
}
