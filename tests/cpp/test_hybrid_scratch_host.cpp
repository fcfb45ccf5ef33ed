// The scratch planner of the hybrid key switch (csrc/hybrid_scratch.h) on the CPU: a program of its own that includes the header the
// library compiles and never touches a device.  Three checks:
//   1. the row totals of every call family equal the formulas of include/moai_hip.h, written here as the header states them;
//   2. the plans (cb, G) equal the five chunk functions they replaced in hybrid.hip, copied here as they were with (n, budget) in
//      place of the context and the knob, and the anchors the GPU chunking tests state in words hold;
//   3. every layout is sound: 256-aligned ascending offsets, regions that hold their rows and do not overlap, the total at the end of
//      the last region, and rows that sum to the formulas at the plan's (cb, G).
// Built with the address and undefined-behaviour sanitizers by tests/test_hybrid_scratch_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "hybrid_scratch.h"

using namespace moai;

static int failures = 0;

#define CHECK(cond)                                                      \
    do                                                                   \
    {                                                                    \
        if (!(cond))                                                     \
        {                                                                \
            if (++failures <= 20)                                        \
            {                                                            \
                std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            }                                                            \
        }                                                                \
    } while (0)

static const size_t MAX_NG = 16, LIST_MAX = 64; // HY_DOT_MAX_NG and KS_LIST_MAX of the library

// ---- 1. the formulas of include/moai_hip.h, in rows of N words ---------------------------------------------------------------------
static size_t beta_of(size_t L, size_t alpha)
{
    return (L + alpha - 1) / alpha; // ceil(L / alpha)
}

// "Scratch per ciphertext is beta (L + alpha) + 4L + 4 alpha rows of N words (2L more for apply_galois)"; the list forms: "+ 2L (the
// permuted member)", "+ L (the gathered third polynomial)"
static size_t doc_switch(size_t L, size_t alpha, size_t more)
{
    return beta_of(L, alpha) * (L + alpha) + 4 * L + 4 * alpha + more;
}

// "cb beta (L + alpha)  +  cb G (2 (L + alpha) + 2 alpha + 2 L + L)"
static size_t doc_hoisted_shared(size_t L, size_t alpha)
{
    return beta_of(L, alpha) * (L + alpha);
}
static size_t doc_hoisted_group(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * alpha + 2 * L + L;
}

// "cb (beta (L + alpha) + 2 L + 2 (L + alpha))  +  cb G (2 (L + alpha) + 2 alpha + 2 L + 2 L)"
static size_t doc_dot_shared(size_t L, size_t alpha)
{
    return beta_of(L, alpha) * (L + alpha) + 2 * L + 2 * (L + alpha);
}
static size_t doc_dot_group(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * alpha + 2 * L + 2 * L;
}

// "cb (beta (L + alpha) + 2 L + 2 (L + alpha)  +  2 (L + alpha) + 2 alpha + 2 L)
//   + cb G (2 (L + alpha) + 2 L  +  alpha + L  +  L + beta (L + alpha))"
static size_t doc_bsgs_shared(size_t L, size_t alpha)
{
    return beta_of(L, alpha) * (L + alpha) + 2 * L + 2 * (L + alpha) + 2 * (L + alpha) + 2 * alpha + 2 * L;
}
static size_t doc_bsgs_group(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * L + alpha + L + L + beta_of(L, alpha) * (L + alpha);
}

// "beta (L + alpha) + 2 (L + alpha) + 2 (alpha + 1) + 2 (L - 1) rows of N words (3L more with the product)"; the list form: "+ L"
static size_t doc_rescale(size_t L, size_t alpha, size_t more)
{
    return beta_of(L, alpha) * (L + alpha) + 2 * (L + alpha) + 2 * (alpha + 1) + 2 * (L - 1) + more;
}

static void check_formulas()
{
    const size_t n = 4096, budget = (size_t)1 << 34;
    for (size_t alpha = 1; alpha <= 16; ++alpha)
    {
        for (size_t L = 1; L <= 48; ++L)
        {
            for (size_t more : { (size_t)0, L, 2 * L })
            {
                const HyPlan p = hy_plan_switch(n, L, alpha, 1, more, budget);
                CHECK(p.shared_rows == doc_switch(L, alpha, more) && p.group_rows == 0 && p.flag_bytes == 0);
            }
            const HyPlan h = hy_plan_hoisted(n, L, alpha, 1, 1, budget);
            CHECK(h.shared_rows == doc_hoisted_shared(L, alpha) && h.group_rows == doc_hoisted_group(L, alpha) && h.flag_bytes == 256);
            const HyPlan d = hy_plan_dot(n, L, alpha, 1, 1, MAX_NG, budget);
            CHECK(d.shared_rows == doc_dot_shared(L, alpha) && d.group_rows == doc_dot_group(L, alpha) && d.flag_bytes == 256);
            const HyPlan b = hy_plan_bsgs(n, L, alpha, 1, 1, MAX_NG, budget);
            CHECK(b.shared_rows == doc_bsgs_shared(L, alpha) && b.group_rows == doc_bsgs_group(L, alpha) && b.flag_bytes == 256);
            if (L >= 2 && alpha <= 15)
            {
                for (size_t more : { (size_t)0, L, 3 * L })
                {
                    const HyPlan r = hy_plan_rescale(n, L, alpha, 1, more, budget);
                    CHECK(r.shared_rows == doc_rescale(L, alpha, more) && r.group_rows == 0 && r.flag_bytes == 0);
                }
            }
        }
    }
}

// ---- 2. the chunk functions of hybrid.hip before the planner, with (n, budget) for the context and the knob -------------------------
namespace before {

static inline size_t hy_beta(size_t L, size_t alpha)
{
    return (L + alpha - 1) / alpha;
}

static size_t hy_rows_per_ct(size_t L, size_t alpha, size_t gal_rows)
{
    const size_t beta = hy_beta(L, alpha);
    return gal_rows + L + (beta * (L + alpha) - L) + 2 * (L + alpha) + 2 * alpha + 2 * L;
}

static size_t hy_chunk(size_t n, size_t budget, size_t L, size_t alpha, size_t batch, size_t gal_rows)
{
    const size_t per = hy_rows_per_ct(L, alpha, gal_rows) * n * sizeof(uint64_t);
    size_t cb = budget / per;
    cb = cb < 1 ? 1 : cb;
    // row-per-workgroup launches: 2 * cb * (L + alpha) rows in gridDim.y
    const size_t cap = 65535 / (2 * (L + alpha));
    cb = cb > cap ? cap : cb;
    return cb < batch ? cb : batch;
}

static inline size_t hy_hoist_shared_rows(size_t L, size_t alpha)
{
    return hy_beta(L, alpha) * (L + alpha);
}

static inline size_t hy_hoist_rotation_rows(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * alpha + 2 * L + L;
}

static void hy_hoist_chunk(size_t n, size_t budget, size_t L, size_t alpha, size_t batch, size_t R, size_t *cb_out, size_t *G_out)
{
    const size_t row = n * sizeof(uint64_t);
    const size_t shared = hy_hoist_shared_rows(L, alpha) * row, rot = hy_hoist_rotation_rows(L, alpha) * row;
    const size_t cap = 65535 / (2 * (L + alpha));
    size_t cb = budget / (shared + rot);
    cb = cb < 1 ? 1 : cb;
    cb = cb > cap ? cap : cb;
    cb = cb < batch ? cb : batch;
    size_t G = budget / cb > shared ? (budget / cb - shared) / rot : 0;
    G = G < 1 ? 1 : G;
    G = G > cap / cb ? cap / cb : G;
    *cb_out = cb;
    *G_out = G < R ? G : R;
}

static inline size_t hy_dot_shared_rows(size_t L, size_t alpha)
{
    return hy_beta(L, alpha) * (L + alpha) + 2 * L + 2 * (L + alpha);
}

static inline size_t hy_dot_output_rows(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * alpha + 2 * L + 2 * L;
}

static void hy_dot_chunk(size_t n, size_t budget, size_t L, size_t alpha, size_t batch, size_t n_out, size_t *cb_out, size_t *G_out)
{
    const size_t row = n * sizeof(uint64_t);
    const size_t shared = hy_dot_shared_rows(L, alpha) * row, out = hy_dot_output_rows(L, alpha) * row;
    const size_t cap = 65535 / (2 * (L + alpha));
    size_t cb = budget / (shared + out);
    cb = cb < 1 ? 1 : cb;
    cb = cb > cap ? cap : cb;
    cb = cb < batch ? cb : batch;
    size_t G = budget / cb > shared ? (budget / cb - shared) / out : 0;
    G = G < 1 ? 1 : G;
    G = G > cap / cb ? cap / cb : G;
    G = G > MAX_NG ? MAX_NG : G;
    *cb_out = cb;
    *G_out = G < n_out ? G : n_out;
}

static inline size_t hy_bsgs_shared_rows(size_t L, size_t alpha)
{
    return hy_dot_shared_rows(L, alpha) + 2 * (L + alpha) + 2 * alpha + 2 * L;
}

static inline size_t hy_bsgs_giant_rows(size_t L, size_t alpha)
{
    return 2 * (L + alpha) + 2 * L + alpha + L + L + hy_beta(L, alpha) * (L + alpha);
}

static void hy_bsgs_chunk(size_t n, size_t budget, size_t L, size_t alpha, size_t batch, size_t n_giant, size_t *cb_out, size_t *G_out)
{
    const size_t row = n * sizeof(uint64_t);
    const size_t shared = hy_bsgs_shared_rows(L, alpha) * row, giant = hy_bsgs_giant_rows(L, alpha) * row;
    const size_t cap = 65535 / (2 * (L + alpha));
    size_t G = std::min(std::min(n_giant, MAX_NG), cap);
    size_t cb = budget / (shared + G * giant);
    if (cb < 1)
    {
        cb = 1;
        G = budget > shared ? (budget - shared) / giant : 0;
        G = G < 1 ? 1 : G;
    }
    cb = cb > cap / G ? cap / G : cb;
    cb = cb < batch ? cb : batch;
    const size_t chunks = (batch + cb - 1) / cb;
    *cb_out = (batch + chunks - 1) / chunks;
    *G_out = G;
}

static size_t hy_rescale_rows_per_ct(size_t L, size_t alpha, size_t head_rows)
{
    const size_t beta = hy_beta(L, alpha);
    return head_rows + L + (beta * (L + alpha) - L) + 2 * (L + alpha) + 2 * (alpha + 1) + 2 * (L - 1);
}

static size_t hy_rescale_chunk(size_t n, size_t budget, size_t L, size_t alpha, size_t batch, size_t head_rows)
{
    const size_t per = hy_rescale_rows_per_ct(L, alpha, head_rows) * n * sizeof(uint64_t);
    size_t cb = budget / per;
    cb = cb < 1 ? 1 : cb;
    const size_t cap = 65535 / std::max(2 * (L + alpha), 3 * L);
    cb = cb > cap ? cap : cb;
    return cb < batch ? cb : batch;
}

} // namespace before

using namespace before;

// ---- 3. a plan's layout ---------------------------------------------------------------------------------------------------------------
// rows: what the formulas of (1) give at the plan's (cb, G)
static void check_layout(const HyPlan &p, size_t n, size_t rows)
{
    CHECK(p.cb >= 1 && p.G >= 1 && p.count >= 1 && p.count <= (size_t)HY_REGIONS);
    size_t end = p.flag_bytes, sum = 0;
    bool seen[HY_REGIONS] = {};
    for (size_t i = 0; i < p.count; ++i)
    {
        const HyRegion r = p.order[i];
        CHECK(r < HY_REGIONS && !seen[r]);
        seen[r] = true;
        const size_t mult = p.grouped[r] ? p.cb * p.G : p.cb;
        CHECK(p.copies(r) == mult);
        CHECK(p.off[r] % 256 == 0);
        CHECK(p.off[r] >= end); // ascending, and the region before it has ended
        const size_t next = i + 1 < p.count ? p.off[p.order[i + 1]] : p.total;
        CHECK(next >= p.off[r] && next - p.off[r] >= p.rows[r] * mult * 8 * n);
        end = p.off[r] + p.rows[r] * mult * 8 * n;
        sum += p.rows[r] * mult;
    }
    CHECK(p.total >= end && p.total - end < 256 && p.total % 256 == 0);
    CHECK(sum == rows);
    CHECK(sum == p.cb * p.shared_rows + p.cb * p.G * p.group_rows);
}

static void check_plans()
{
    const size_t ns[] = { 4096, 65536 };
    const size_t dims[][2] = { { 1, 1 }, { 3, 2 }, { 7, 3 }, { 2, 15 }, { 35, 12 }, { 35, 4 } };
    const size_t batches[] = { 1, 2, 5, 64, 1000 };
    const size_t groups[] = { 1, 2, 5, 16, 17, 40 };
    const size_t kib[] = { 1, 124 * 32, 154 * 32, 172 * 32, 185 * 32, 236 * 32, 266 * 32, 347 * 32, 5000, 6000, 16777216 };
    for (size_t n : ns)
    {
        for (const auto &la : dims)
        {
            const size_t L = la[0], alpha = la[1];
            for (size_t batch : batches)
            {
                for (size_t kb : kib)
                {
                    const size_t budget = kb << 10;
                    // switch: the batch forms with 0 and 2 L gathered rows, the list forms with 2 L and L under KS_LIST_MAX
                    for (size_t more : { (size_t)0, L, 2 * L })
                    {
                        const size_t old = hy_chunk(n, budget, L, alpha, batch, more);
                        const HyPlan p = hy_plan_switch(n, L, alpha, batch, more, budget);
                        CHECK(p.cb == old && p.G == 1);
                        check_layout(p, n, p.cb * doc_switch(L, alpha, more));
                        const HyPlan q = hy_plan_switch(n, L, alpha, batch, more, budget, LIST_MAX);
                        CHECK(q.cb == std::min(LIST_MAX, old) && q.G == 1);
                        check_layout(q, n, q.cb * doc_switch(L, alpha, more));
                    }
                    if (L >= 2 && alpha <= 15)
                    {
                        for (size_t more : { (size_t)0, L, 3 * L })
                        {
                            const size_t old = hy_rescale_chunk(n, budget, L, alpha, batch, more);
                            const HyPlan p = hy_plan_rescale(n, L, alpha, batch, more, budget);
                            CHECK(p.cb == old && p.G == 1);
                            check_layout(p, n, p.cb * doc_rescale(L, alpha, more));
                            const HyPlan q = hy_plan_rescale(n, L, alpha, batch, more, budget, LIST_MAX);
                            CHECK(q.cb == std::min(LIST_MAX, old) && q.G == 1);
                            check_layout(q, n, q.cb * doc_rescale(L, alpha, more));
                        }
                    }
                    for (size_t g : groups)
                    {
                        size_t cb, G;
                        hy_hoist_chunk(n, budget, L, alpha, batch, g, &cb, &G);
                        const HyPlan h = hy_plan_hoisted(n, L, alpha, batch, g, budget);
                        CHECK(h.cb == cb && h.G == G);
                        check_layout(h, n, h.cb * doc_hoisted_shared(L, alpha) + h.cb * h.G * doc_hoisted_group(L, alpha));
                        hy_dot_chunk(n, budget, L, alpha, batch, g, &cb, &G);
                        const HyPlan d = hy_plan_dot(n, L, alpha, batch, g, MAX_NG, budget);
                        CHECK(d.cb == cb && d.G == G);
                        check_layout(d, n, d.cb * doc_dot_shared(L, alpha) + d.cb * d.G * doc_dot_group(L, alpha));
                        hy_bsgs_chunk(n, budget, L, alpha, batch, g, &cb, &G);
                        const HyPlan b = hy_plan_bsgs(n, L, alpha, batch, g, MAX_NG, budget);
                        CHECK(b.cb == cb && b.G == G);
                        check_layout(b, n, b.cb * doc_bsgs_shared(L, alpha) + b.cb * b.G * doc_bsgs_group(L, alpha));
                    }
                }
            }
        }
    }
}

// what the GPU chunking tests state in words, all at n = 4096 (rows of 32 KiB)
static void check_anchors()
{
    const size_t n = 4096, row_kib = 32;
    // hoisted, L = 7, alpha = 3, batch 5, R 5: 30 shared rows and 47 per rotation
    HyPlan h = hy_plan_hoisted(n, 7, 3, 5, 5, (154 * row_kib) << 10);
    CHECK(h.cb == 2 && h.G == 1);
    h = hy_plan_hoisted(n, 7, 3, 5, 5, (124 * row_kib) << 10);
    CHECK(h.cb == 1 && h.G == 2);
    h = hy_plan_hoisted(n, 7, 3, 5, 5, (size_t)1 << 10);
    CHECK(h.cb == 1 && h.G == 1);
    // switch, L = 35, alpha = 12, batch 1000, the default budget: the grid cap binds (65535 / 94 = 697), not the budget, which would
    // hold 1593 ciphertexts of 329 rows
    const size_t dflt = (size_t)16777216 << 10;
    const HyPlan s = hy_plan_switch(n, 35, 12, 1000, 0, dflt);
    CHECK(doc_switch(35, 12, 0) == 329);
    CHECK(dflt / (329 * row_kib << 10) == 1593);
    CHECK(65535 / 94 == 697 && s.cb == 697);
}

int main()
{
    check_formulas();
    check_plans();
    check_anchors();
    if (failures)
    {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("ALL PASS\n");
    return 0;
}
