// wire.hip -- the packed-row wire form of RNS polynomials (include/moai_hip.h, "wire form"): row r of a polynomial under
// prime q_r is stored as a little-endian bit stream of N fields of b_r = bit_length(q_r) bits instead of N 64-bit words.
// tests/wire_format.py restates the format in numpy.
//
//   wire_pack    : one 64-bit packed word per thread (consecutive lanes store consecutive words of a row; no two lanes share a
//                  word, so there are no atomics), gathered from the 2 .. 33 coefficients whose fields overlap that word
//   wire_unpack  : two coefficients (one 16-byte store) per thread from the at most three packed words they overlap, with the
//                  residue check of SEAL's is_data_valid_for (SEAL/valcheck.cpp) folded in
//
// Both are streaming kernels: gridDim.y is the row of the polynomial, gridDim.z the polynomial, so that the field width, the
// row's offset in the packed polynomial and its modulus are uniform over a workgroup and live in scalar registers.
#include <algorithm>

#include "launch.h"

namespace moai {

struct WireArgs
{
    const uint64_t *src;
    uint64_t *dst;
    uint32_t *invalid;           // unpack only: set to 1 where a field holds a value >= q_r; may be null
    const PrimeConst *pc;
    RowMap rows;
    uint32_t bits[MOAI_MAX_RNS];  // b_r
    uint32_t magic[MOAI_MAX_RNS]; // floor(2^32 / b_r) + 1: (x * magic) >> 32 == x / b_r for every bit offset x <= 61 * 2^16
    uint32_t off[MOAI_MAX_RNS];   // first word of row r within a packed polynomial
    uint32_t words[MOAI_MAX_RNS]; // ceil(N b_r / 64)
    uint32_t poly_words;          // words of one packed polynomial
    uint32_t L;
    uint32_t logn;
};

__global__ __launch_bounds__(256) void wire_pack(WireArgs g)
{
    const uint32_t r = blockIdx.y;
    const uint32_t b = __builtin_amdgcn_readfirstlane(g.bits[r]);
    const uint32_t magic = __builtin_amdgcn_readfirstlane(g.magic[r]);
    const uint32_t words = __builtin_amdgcn_readfirstlane(g.words[r]);
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= words)
    {
        return;
    }
    const uint32_t n = 1u << g.logn;
    const size_t p = blockIdx.z;
    const uint64_t *in = g.src + (((p * g.L + r)) << g.logn);
    const uint64_t mask = (1ull << b) - 1;
    // the word holds stream bits [64 w, 64 w + 64): it starts `s` bits into field i
    const uint32_t bit0 = w << 6;
    const uint32_t i = (uint32_t)(((uint64_t)bit0 * magic) >> 32);
    const uint32_t s = bit0 - i * b;
    uint64_t acc;
    if (b >= 32)
    {
        // at most three fields overlap the word: all three loads are issued before the first is used
        const uint64_t v0 = in[i] & mask;
        const uint64_t v1 = in[min(i + 1, n - 1)] & mask;
        const uint64_t v2 = in[min(i + 2, n - 1)] & mask;
        const uint32_t f1 = b - s, f2 = 2 * b - s; // bit of the word where fields i + 1, i + 2 begin
        acc = v0 >> s;
        acc |= i + 1 < n ? v1 << f1 : 0; // f1 <= 61
        acc |= (f2 < 64 && i + 2 < n) ? v2 << (f2 & 63) : 0;
    }
    else
    {
        acc = (in[i] & mask) >> s;
        uint32_t f = b - s;
        for (uint32_t j = i + 1; f < 64 && j < n; j++, f += b)
        {
            acc |= (in[j] & mask) << f;
        }
    }
    g.dst[p * g.poly_words + g.off[r] + w] = acc;
}

__global__ __launch_bounds__(256) void wire_unpack(WireArgs g)
{
    const uint32_t r = blockIdx.y;
    const uint32_t b = __builtin_amdgcn_readfirstlane(g.bits[r]);
    const uint32_t last = __builtin_amdgcn_readfirstlane(g.words[r]) - 1;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x; // coefficients 2t, 2t + 1
    if (t >= (1u << g.logn) >> 1)
    {
        return;
    }
    const size_t p = blockIdx.z;
    const uint64_t q = g.pc[g.rows.idx[r]].q;
    const uint64_t *in = g.src + p * g.poly_words + g.off[r];
    const uint64_t mask = (1ull << b) - 1;
    const uint32_t bit0 = 2 * t * b, bit1 = bit0 + b;
    const uint32_t w0 = bit0 >> 6, s0 = bit0 & 63;
    const uint32_t w1 = bit1 >> 6, s1 = bit1 & 63;
    // the two fields lie in words w0 .. w0 + 2; an index clamped to the row's last word is only ever one whose bits are masked off
    const uint64_t p0 = in[w0];
    const uint64_t p1 = in[min(w0 + 1, last)];
    const uint64_t p2 = in[min(w0 + 2, last)];
    const uint64_t a1 = w1 == w0 ? p0 : p1, c1 = w1 == w0 ? p1 : p2;
    ulonglong2 v;
    v.x = ((p0 >> s0) | (s0 ? p1 << (64 - s0) : 0)) & mask;
    v.y = ((a1 >> s1) | (s1 ? c1 << (64 - s1) : 0)) & mask;
    *reinterpret_cast<ulonglong2 *>(g.dst + (((p * g.L + r)) << g.logn) + 2 * (size_t)t) = v;
    if (g.invalid && (v.x >= q || v.y >= q))
    {
        *g.invalid = 1; // every lane that finds one stores the same value: no atomic needed
    }
}

static uint32_t bit_length(uint64_t q)
{
    return 64 - (uint32_t)__builtin_clzll(q);
}

static size_t row_words(const moai_ctx *c, uint32_t prime)
{
    return (c->n * bit_length(c->primes[prime]) + 63) / 64;
}

static int wire_args(const moai_ctx *c, size_t L, const uint32_t *prime_index, WireArgs *a)
{
    MOAI_TRY(rows_entry(c, L, prime_index, &a->rows));
    size_t off = 0;
    for (size_t r = 0; r < MOAI_MAX_RNS; r++)
    {
        const uint32_t b = r < L ? bit_length(c->primes[a->rows.idx[r]]) : 0;
        a->bits[r] = b;
        a->magic[r] = b ? (uint32_t)((1ull << 32) / b) + 1 : 0;
        a->off[r] = (uint32_t)off;
        a->words[r] = r < L ? (uint32_t)row_words(c, a->rows.idx[r]) : 0;
        off += a->words[r];
    }
    a->poly_words = (uint32_t)off; // at most 64 rows of 61 * 2^16 / 64 words
    a->pc = c->pc;
    a->L = (uint32_t)L;
    a->logn = (uint32_t)c->logn;
    a->invalid = nullptr;
    return MOAI_OK;
}

// what pack and unpack share: validation, then one launch of `kernel` per 65535 polynomials (gridDim.z), `grid_x` workgroups
// per row.  rows [n_poly][L][N] and packed [n_poly][poly_words] are the two blocks: pack reads the first and writes the second,
// unpack the reverse (the one that is read is the caller's const block).
template <class Kernel>
static int wire_launch(Kernel kernel, bool unpack, moai_ctx *c, uint64_t *rows, uint64_t *packed, size_t n_poly, size_t L,
                       const uint32_t *prime_index, uint32_t *invalid, void *stream)
{
    WireArgs a;
    MOAI_TRY(wire_args(c, L, prime_index, &a));
    if (n_poly == 0)
    {
        return MOAI_OK;
    }
    if (!rows || !packed)
    {
        return set_error(MOAI_EINVAL, "null argument");
    }
    if (n_poly > ((size_t)1 << 40))
    {
        return set_error(MOAI_EINVAL, "too many polynomials");
    }
    if (unpack && ((uintptr_t)rows & 15))
    {
        return set_error(MOAI_EINVAL, "out must be 16-byte aligned");
    }
    const size_t row_words = L * c->n;
    if (overlap(rows, n_poly * row_words * 8, packed, n_poly * a.poly_words * 8))
    {
        return set_error(MOAI_EINVAL, unpack ? "packed and out overlap" : "in and packed overlap");
    }
    MOAI_TRY(enter_device(c));
    a.invalid = invalid;
    uint32_t grid_x = (uint32_t)((c->n / 2 + 255) / 256);
    if (!unpack)
    {
        // one thread per packed word of the widest row
        const uint32_t widest = *std::max_element(a.words, a.words + L);
        grid_x = (widest + 255) / 256;
    }
    return for_chunks(n_poly, 65535, [&](size_t p0, size_t np) {
        uint64_t *r = rows + p0 * row_words, *p = packed + p0 * a.poly_words;
        a.src = unpack ? p : r;
        a.dst = unpack ? r : p;
        hipLaunchKernelGGL(kernel, dim3(grid_x, (uint32_t)L, (uint32_t)np), dim3(256), 0, (hipStream_t)stream, a);
        MOAI_LAUNCH_CHECK();
        return MOAI_OK;
    });
}

} // namespace moai

using namespace moai;

extern "C" size_t moai_packed_words(const moai_ctx *c, size_t L, const uint32_t *prime_index)
{
    WireArgs a;
    if (wire_args(c, L, prime_index, &a))
    {
        return 0;
    }
    return a.poly_words;
}

extern "C" int moai_pack_rows(moai_ctx *c, const uint64_t *in, uint64_t *packed, size_t n_poly, size_t L, const uint32_t *prime_index,
                              void *stream)
{
    MOAI_AUDIT(stream, in, packed);
    trace_op("pack_rows", L, n_poly);
    return wire_launch(wire_pack, false, c, const_cast<uint64_t *>(in), packed, n_poly, L, prime_index, nullptr, stream);
}

extern "C" int moai_unpack_rows(moai_ctx *c, const uint64_t *packed, uint64_t *out, size_t n_poly, size_t L, const uint32_t *prime_index,
                                uint32_t *invalid, void *stream)
{
    MOAI_AUDIT(stream, packed, out, invalid);
    trace_op("unpack_rows", L, n_poly);
    return wire_launch(wire_unpack, true, c, out, const_cast<uint64_t *>(packed), n_poly, L, prime_index, invalid, stream);
}
