// hybrid_scratch.h -- the scratch plan of every hybrid key-switch call family (hybrid.hip): which regions a chunk's workspace holds,
// how many ciphertexts (cb) and groups (G: rotations, outputs or giant steps in flight) a chunk takes under a byte budget, and where
// each region lies.  Host only, pure integer arithmetic on (n, L, alpha, batch, groups, budget bytes): no context, no device.
//
// A family states its regions ONCE, in workspace order, with HyPlan::add: a name (HyRegion), a row count and whether the region is
// held per ciphertext (cb copies) or per (group, ciphertext) pair (cb * G copies).  From that one statement come the row totals the
// chunk sizing divides the budget by (shared_rows, group_rows), the 256-aligned byte offsets (place) and the total.  The formulas of
// include/moai_hip.h are the specification; tests/cpp/test_hybrid_scratch_host.cpp checks every family against them.
#pragma once
#include <algorithm>
#include <cstddef>

namespace moai {

inline size_t hy_beta(size_t L, size_t alpha)
{
    return (L + alpha - 1) / alpha;
}

// rows of N words
enum HyRegion
{
    HY_HEAD,  // rows in front of a switch: the permuted or gathered input, or the three-polynomial product
    HY_T,     // t = INTT(target)
    HY_EXT,   // the converted rows of every digit
    HY_ACC,   // the accumulators of one switch over L + alpha rows
    HY_X,     // the source rows of a mod-down in coefficient form
    HY_CONV,  // the converted rows of a mod-down
    HY_C0,    // hoisted: the permuted c0
    HY_GAL,   // pt-dot, bsgs: the unhoisted route's permuted input
    HY_S,     // pt-dot, bsgs: the sums S_g
    HY_ADD,   // pt-dot, bsgs: the addends a_g
    HY_Z,     // bsgs: the sum over the giant steps, with the special rows and conv of its step 5
    HY_ZX,
    HY_ZCONV,
    HY_TGT,   // bsgs: the permuted c1' of a giant step, with its t and digits
    HY_T2,
    HY_EXT2,
    HY_REGIONS
};

struct HyPlan
{
    size_t cb = 0, G = 1;                   // ciphertexts per chunk, groups in flight
    size_t shared_rows = 0, group_rows = 0; // rows per ciphertext, rows per (group, ciphertext) pair
    size_t flag_bytes = 0;                  // the block in front of the regions (the zero probe's flag), not counted against the budget
    size_t total = 0;                       // bytes
    size_t count = 0;                       // regions stated, in workspace order
    HyRegion order[HY_REGIONS] = {};
    size_t rows[HY_REGIONS] = {}, off[HY_REGIONS] = {};
    bool grouped[HY_REGIONS] = {};

    void add(HyRegion r, size_t n_rows, bool per_group = false)
    {
        order[count++] = r;
        rows[r] = n_rows;
        grouped[r] = per_group;
        (per_group ? group_rows : shared_rows) += n_rows;
    }
    // copies of region r in a chunk
    size_t copies(HyRegion r) const
    {
        return grouped[r] ? cb * G : cb;
    }
    // the byte offsets for rows of n words: every region starts on a 256-byte boundary
    void place(size_t n)
    {
        total = flag_bytes;
        for (size_t i = 0; i < count; ++i)
        {
            const HyRegion r = order[i];
            off[r] = total;
            total += (copies(r) * rows[r] * n * sizeof(unsigned long long) + 255) & ~(size_t)255;
        }
    }
};

// ---- what the families share --------------------------------------------------------------------------------------------------
// steps 1-3 of one target
inline void hy_add_digits(HyPlan &p, size_t L, size_t alpha, HyRegion t = HY_T, HyRegion ext = HY_EXT, bool per_group = false)
{
    p.add(t, L, per_group);
    p.add(ext, hy_beta(L, alpha) * (L + alpha) - L, per_group);
}

// an accumulator over L + alpha rows for both polynomials
inline void hy_add_acc(HyPlan &p, HyRegion acc, size_t L, size_t alpha, bool per_group = false)
{
    p.add(acc, 2 * (L + alpha), per_group);
}

// a mod-down of `polys` polynomials from nsrc source rows to ntgt rows
inline void hy_add_mod_down(HyPlan &p, HyRegion x, HyRegion conv, size_t polys, size_t nsrc, size_t ntgt, bool per_group = false)
{
    p.add(x, polys * nsrc, per_group);
    p.add(conv, polys * ntgt, per_group);
}

// the hoisted families keep the zero probe's flag in front; the digits of the unpermuted c1 follow
inline void hy_add_hoisted_head(HyPlan &p, size_t L, size_t alpha)
{
    p.flag_bytes = 256;
    hy_add_digits(p, L, alpha);
}

// the inner stage of pt-dot and bsgs: the digits, and the unhoisted route's permuted input and accumulators
inline void hy_add_dot_shared(HyPlan &p, size_t L, size_t alpha)
{
    hy_add_hoisted_head(p, L, alpha);
    p.add(HY_GAL, 2 * L);
    hy_add_acc(p, HY_ACC, L, alpha);
}

// row-per-workgroup launches run over 2 * cb * G polynomials of at most L + alpha rows in gridDim.y
inline size_t hy_grid_cap(size_t L, size_t alpha)
{
    return 65535 / (2 * (L + alpha));
}

// ---- the three chunk policies ---------------------------------------------------------------------------------------------------
// ciphertexts only: as many as the budget holds, at least one, at most grid_cap, limit and batch
inline void hy_size_cts(HyPlan &p, size_t n, size_t batch, size_t budget, size_t grid_cap, size_t limit)
{
    const size_t per = p.shared_rows * n * sizeof(unsigned long long);
    size_t cb = budget / per;
    cb = cb < 1 ? 1 : cb;
    cb = cb > grid_cap ? grid_cap : cb;
    cb = cb < batch ? cb : batch;
    p.cb = cb < limit ? cb : limit;
    p.G = 1;
    p.place(n);
}

// ciphertexts, then groups beside them: as many ciphertexts as fit with one group in flight, then as many groups as fit beside
// them; at least one of each, G at most max_groups and `groups`, and no grid above the cap
inline void hy_size_cts_then_groups(HyPlan &p, size_t n, size_t L, size_t alpha, size_t batch, size_t groups, size_t max_groups,
                                    size_t budget)
{
    const size_t row = n * sizeof(unsigned long long);
    const size_t shared = p.shared_rows * row, grp = p.group_rows * row;
    const size_t cap = hy_grid_cap(L, alpha);
    size_t cb = budget / (shared + grp);
    cb = cb < 1 ? 1 : cb;
    cb = cb > cap ? cap : cb;
    cb = cb < batch ? cb : batch;
    size_t G = budget / cb > shared ? (budget / cb - shared) / grp : 0;
    G = G < 1 ? 1 : G;
    G = G > cap / cb ? cap / cb : G;
    G = G > max_groups ? max_groups : G;
    p.cb = cb;
    p.G = G < groups ? G : groups;
    p.place(n);
}

// giant steps first, chunks evened out: all groups (at most max_groups) are in flight when one ciphertext fits beside them, and cb is
// the largest count that fits with them; else one ciphertext per chunk with as many groups as fit, at least one
inline void hy_size_groups_first(HyPlan &p, size_t n, size_t L, size_t alpha, size_t batch, size_t groups, size_t max_groups,
                                 size_t budget)
{
    const size_t row = n * sizeof(unsigned long long);
    const size_t shared = p.shared_rows * row, grp = p.group_rows * row;
    const size_t cap = hy_grid_cap(L, alpha);
    size_t G = std::min(std::min(groups, max_groups), cap);
    size_t cb = budget / (shared + G * grp);
    if (cb < 1)
    {
        cb = 1;
        G = budget > shared ? (budget - shared) / grp : 0;
        G = G < 1 ? 1 : G;
    }
    cb = cb > cap / G ? cap / G : cb;
    cb = cb < batch ? cb : batch;
    const size_t chunks = (batch + cb - 1) / cb;
    p.cb = (batch + chunks - 1) / chunks;
    p.G = G;
    p.place(n);
}

// ---- the families ---------------------------------------------------------------------------------------------------------------------
constexpr size_t HY_NO_LIMIT = ~(size_t)0;

// the switch: head_rows = 2 L (the permuted input of apply_galois), L (the third polynomial of a member of the relinearize list) or 0;
// limit: KS_LIST_MAX for the list forms
inline HyPlan hy_plan_switch(size_t n, size_t L, size_t alpha, size_t batch, size_t head_rows, size_t budget, size_t limit = HY_NO_LIMIT)
{
    HyPlan p;
    p.add(HY_HEAD, head_rows);
    hy_add_digits(p, L, alpha);
    hy_add_acc(p, HY_ACC, L, alpha);
    hy_add_mod_down(p, HY_X, HY_CONV, 2, alpha, L);
    hy_size_cts(p, n, batch, budget, hy_grid_cap(L, alpha), limit);
    return p;
}

// hoisted rotations: per rotation in flight acc, its step 5 and the permuted c0
inline HyPlan hy_plan_hoisted(size_t n, size_t L, size_t alpha, size_t batch, size_t R, size_t budget)
{
    HyPlan p;
    hy_add_hoisted_head(p, L, alpha);
    hy_add_acc(p, HY_ACC, L, alpha, true);
    hy_add_mod_down(p, HY_X, HY_CONV, 2, alpha, L, true);
    p.add(HY_C0, L, true);
    hy_size_cts_then_groups(p, n, L, alpha, batch, R, HY_NO_LIMIT, budget);
    return p;
}

// plaintext-weighted sums: per output in flight S, its step 5 and the addend.  Nothing grows with R.
inline HyPlan hy_plan_dot(size_t n, size_t L, size_t alpha, size_t batch, size_t n_out, size_t max_groups, size_t budget)
{
    HyPlan p;
    hy_add_dot_shared(p, L, alpha);
    hy_add_acc(p, HY_S, L, alpha, true);
    hy_add_mod_down(p, HY_X, HY_CONV, 2, alpha, L, true);
    p.add(HY_ADD, 2 * L, true);
    hy_size_cts_then_groups(p, n, L, alpha, batch, n_out, max_groups, budget);
    return p;
}

// the BSGS sum: per ciphertext the inner stage's shared rows and Z with its step 5; per giant step in flight S and the addend, the
// step 5 of c1' alone, and the permuted c1' with its t and digits
inline HyPlan hy_plan_bsgs(size_t n, size_t L, size_t alpha, size_t batch, size_t n_giant, size_t max_groups, size_t budget)
{
    HyPlan p;
    hy_add_dot_shared(p, L, alpha);
    hy_add_acc(p, HY_Z, L, alpha);
    hy_add_mod_down(p, HY_ZX, HY_ZCONV, 2, alpha, L);
    hy_add_acc(p, HY_S, L, alpha, true);
    p.add(HY_ADD, 2 * L, true);
    hy_add_mod_down(p, HY_X, HY_CONV, 1, alpha, L, true);
    p.add(HY_TGT, L, true);
    hy_add_digits(p, L, alpha, HY_T2, HY_EXT2, true);
    hy_size_groups_first(p, n, L, alpha, batch, n_giant, max_groups, budget);
    return p;
}

// relinearize + rescale (L >= 2): the merged mod-down has alpha + 1 sources and L - 1 targets; head_rows = 3 L (the product of
// moai_multiply_relin_rescale_hybrid), L (the gathered third polynomial of a list member) or 0.  The widest grid runs over 3 * cb * L
// rows with the product, 2 * cb * (L + alpha) without.
inline HyPlan hy_plan_rescale(size_t n, size_t L, size_t alpha, size_t batch, size_t head_rows, size_t budget, size_t limit = HY_NO_LIMIT)
{
    HyPlan p;
    p.add(HY_HEAD, head_rows);
    hy_add_digits(p, L, alpha);
    hy_add_acc(p, HY_ACC, L, alpha);
    hy_add_mod_down(p, HY_X, HY_CONV, 2, alpha + 1, L - 1);
    hy_size_cts(p, n, batch, budget, 65535 / std::max(2 * (L + alpha), 3 * L), limit);
    return p;
}

} // namespace moai
