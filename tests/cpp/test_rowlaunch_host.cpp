// The host helpers of csrc/rowlaunch.h that lay out scratch and order the rows of the hybrid key switch, checked on the CPU: a program
// of its own that includes the header the library compiles and never touches a device.  hy_rowmap is compared with the three loops
// it replaced in hybrid.hip (the converted rows of a digit, the special rows of the mod-down, every row of the hoisted correction),
// copied here as they were.  Built with the address and undefined-behaviour sanitizers by tests/test_rowlaunch_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rowlaunch.h"

using namespace moai;

static int failures = 0;

#define CHECK(cond)                                                      \
    do                                                                   \
    {                                                                    \
        if (!(cond))                                                     \
        {                                                                \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// hy_decompose, before: the rows of [0, L + alpha) outside the digit [lo, hi)
static size_t old_digit_rows(size_t k, size_t L, size_t alpha, size_t lo, size_t hi, RowMap &rm)
{
    size_t tg = 0;
    for (size_t row = 0; row < L + alpha; ++row)
    {
        if (row < lo || row >= hi)
        {
            rm.idx[tg++] = (uint32_t)(row < L ? row : k - alpha + (row - L));
        }
    }
    return tg;
}

// hy_mod_down, before: the special rows
static size_t old_special_rows(size_t k, size_t alpha, RowMap &rm)
{
    for (size_t r = 0; r < alpha; ++r)
    {
        rm.idx[r] = (uint32_t)(k - alpha + r);
    }
    return alpha;
}

// hy_hoist_correction, before: every row
static size_t old_all_rows(size_t k, size_t L, size_t alpha, RowMap &rm)
{
    const size_t rows = L + alpha;
    for (size_t row = 0; row < rows; ++row)
    {
        rm.idx[row] = (uint32_t)(row < L ? row : k - alpha + (row - L));
    }
    return rows;
}

static void same(const RowMap &a, size_t na, const RowMap &b, size_t nb)
{
    CHECK(na == nb);
    CHECK(na <= MOAI_MAX_RNS);
    CHECK(std::memcmp(a.idx, b.idx, na * sizeof(uint32_t)) == 0);
}

static void check_rows(size_t k, size_t L, size_t alpha)
{
    moai_ctx c;
    c.k = k;
    for (size_t row = 0; row < L + alpha; ++row)
    {
        const size_t p = hy_row_prime(row, L, alpha, k);
        CHECK(p == (row < L ? row : k - alpha + (row - L)));
        CHECK(p < k);
        CHECK(hy_row_prime((uint32_t)row, (uint32_t)L, (uint32_t)alpha, (uint32_t)k) == (uint32_t)p);
    }
    // every digit, the last partial one included
    for (size_t lo = 0; lo < L; lo += alpha)
    {
        const size_t hi = lo + alpha < L ? lo + alpha : L;
        RowMap a{}, b{};
        const size_t na = old_digit_rows(k, L, alpha, lo, hi, a), nb = hy_rowmap(&c, L, alpha, lo, hi, &b);
        same(a, na, b, nb);
        CHECK(nb == L - (hi - lo) + alpha);
    }
    {
        RowMap a{}, b{};
        same(a, old_special_rows(k, alpha, a), b, hy_rowmap(&c, L, alpha, 0, L, &b)); // skip at the low end
    }
    {
        RowMap a{}, b{};
        same(a, old_all_rows(k, L, alpha, a), b, hy_rowmap(&c, L, alpha, 0, 0, &b)); // nothing skipped
    }
    {
        // skip at the high end: the data rows alone
        RowMap b{};
        const size_t nb = hy_rowmap(&c, L, alpha, L, L + alpha, &b);
        CHECK(nb == L);
        for (size_t r = 0; r < nb; ++r)
        {
            CHECK(b.idx[r] == r);
        }
    }
}

int main()
{
    // align256: the next multiple of 256, itself for a multiple
    const size_t xs[] = { 0, 1, 255, 256, 257, 511, 512, 65535, 65536, ((size_t)1 << 40) + 1 };
    for (size_t x : xs)
    {
        const size_t a = align256(x);
        CHECK(a >= x && a - x < 256 && a % 256 == 0);
    }
    // at_bytes: byte offsets into a block, first and last word
    std::vector<uint64_t> block(96, 0);
    CHECK(at_bytes(block.data(), 0) == block.data());
    CHECK(at_bytes(block.data(), 256) == block.data() + 32);
    CHECK(at_bytes(block.data(), 95 * sizeof(uint64_t)) == &block[95]);
    *at_bytes(block.data(), 95 * sizeof(uint64_t)) = 7;
    CHECK(block[95] == 7);

    // (k, L, alpha): L = 1, alpha = 1, alpha = 16, a last partial digit, the full chain
    check_rows(2, 1, 1);
    check_rows(5, 1, 1);
    check_rows(5, 4, 1);
    check_rows(20, 1, 16);
    check_rows(20, 4, 16);
    check_rows(40, 24, 16);
    check_rows(40, 23, 16);
    check_rows(13, 7, 3);
    check_rows(13, 10, 3);
    check_rows(MOAI_MAX_RNS, MOAI_MAX_RNS - 16, 16);
    check_rows(MOAI_MAX_RNS, MOAI_MAX_RNS - 1, 1);

    if (failures)
    {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("ALL PASS\n");
    return 0;
}
