// rowlaunch.h -- the small host helpers every translation unit launches its row kernels and lays out its scratch with (included by
// launch.h).  Header only, and nothing here touches the device before launch_rows is called.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace moai {

// 256-thread workgroups that cover a row of N / 2 two-word chunks in x, one block row (blockIdx.y) per row
inline dim3 row_grid(const moai_ctx *c, size_t rows)
{
    const uint32_t n2 = (uint32_t)(c->n >> 1);
    return dim3(std::max(1u, (n2 + 255u) / 256u), (uint32_t)rows);
}

// the three fields every args struct describes its rows with
template <class Args>
void fill_rows(Args &g, const moai_ctx *c, size_t L)
{
    g.pc = c->pc;
    g.L = (uint32_t)L;
    g.n2 = (uint32_t)(c->n >> 1);
}

// `kernel` over `rows` block rows (blockIdx.y) of 256-thread workgroups that cover a row of N / 2 chunks.  A kernel that a
// bool selects is passed as  flag ? kernel<true> : kernel<false>.
template <class Kernel, class... Args>
int launch_rows(Kernel kernel, const moai_ctx *c, size_t rows, void *stream, const Args &...args)
{
    MOAI_CHECK_GRID_ROWS(rows);
    hipLaunchKernelGGL(kernel, row_grid(c, rows), dim3(256), 0, (hipStream_t)stream, args...);
    MOAI_LAUNCH_CHECK();
    return MOAI_OK;
}

// A kernel with a LIST form takes the plain argument struct with the list pointer behind it (ListArgs : Args { const KsList *lst; }).
// Calls f(args, std::false_type) with the plain struct, or, when lst is set, f(list args, std::true_type) and returns what f returns.
template <class ListArgs, class Args, class F>
int plain_or_list(const Args &a, const KsList *lst, F &&f)
{
    if (!lst)
    {
        return f(a, std::false_type{});
    }
    ListArgs al;
    static_cast<Args &>(al) = a;
    al.lst = lst;
    return f(al, std::true_type{});
}

// scratch blocks start on 256-byte boundaries
inline size_t align256(size_t x)
{
    return (x + 255) & ~(size_t)255;
}

inline uint64_t *at_bytes(void *base, size_t offset)
{
    return reinterpret_cast<uint64_t *>(static_cast<char *>(base) + offset);
}

// The rows a key switch reads, in NTT form: ciphertext b's row r is row b * stride_rows + off_rows + r of ptr.
struct KsTarget
{
    const uint64_t *ptr;
    size_t stride_rows, off_rows;
    const KsList *lst = nullptr; // keyswitch.hip: every ciphertext its own key and layout (device memory; key and key_rows unused)
    uint32_t key_rows = 0;       // keyswitch.hip: rows per key polynomial in the key's layout (key_rows_for fills it)
};

// What the last kernel of a key switch or mod-down adds to the quotient (ModDownArgs).  mode 0: nothing; 1: polynomial p of
// ciphertext b gets row block b * bstride + p * L of ptr; 2: polynomial 0 only.  second: one more summand with the output's layout
// (may be the output itself), or null.
struct KsAddend
{
    const uint64_t *ptr = nullptr;
    size_t bstride = 0;
    int mode = 0;
    const uint64_t *second = nullptr;
};

// ---- row order of the hybrid key switch (hybrid.hip): rows 0 .. L-1 are the data primes, rows L .. L+alpha-1 the special ones -----
// the context prime of such a row (32-bit in the kernels, size_t on the host)
template <class U>
__host__ __device__ inline U hy_row_prime(U row, U L, U alpha, U k)
{
    return row < L ? row : k - alpha + (row - L);
}

// rm = the primes of the rows [0, L + alpha) without [skip_lo, skip_hi), in order; returns how many
inline size_t hy_rowmap(const moai_ctx *c, size_t L, size_t alpha, size_t skip_lo, size_t skip_hi, RowMap *rm)
{
    size_t cnt = 0;
    for (size_t row = 0; row < L + alpha; ++row)
    {
        if (row < skip_lo || row >= skip_hi)
        {
            rm->idx[cnt++] = (uint32_t)hy_row_prime(row, L, alpha, c->k);
        }
    }
    return cnt;
}

} // namespace moai
