// plan_sgm (csrc/dcmt_sgm.h) with the cost argument, on a CPU.  Built and run by tests/test_sgm_census.py; prints every failed check and
// returns their number.  With the absolute-difference cost the plan is field for field the old one; a cost other than 0 or 1 is
// refused; with census the rows kernel stages 16 bytes a column (18 with a guide: the right image's codes, the left image's stay in
// registers), so the LDS route ends at 4096 (3640) columns, and nothing else of the plan changes.
#include <climits>
#include <cstdio>
#include <initializer_list>

#include "dcmt_sgm.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kLeft = 0x100000000000ull, kRight = 0x200000000000ull, kDisp = 0x300000000000ull, kDepth = 0x400000000000ull,
                       kWork = 0x500000000000ull, kGuide = 0x600000000000ull;

static SgmPlan with_cost(int cols, int D, int paths, uintptr_t guide, int cost, int rows = 3, int batch = 5, size_t held = 2)
{
    return plan_sgm(rows, cols, batch, D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, held * sgm_frame_bytes(rows, cols, D), paths, guide, 100, 1000,
                    cost);
}

// every field the plan had before there was a choice of cost
static bool same_old_fields(const SgmPlan& a, const SgmPlan& b)
{
    return a.status == b.status && a.frame_bytes == b.frame_bytes && a.volume_elems == b.volume_elems && a.chunk == b.chunk && a.n_chunks == b.n_chunks &&
           a.per_lane == b.per_lane && a.lds_route == b.lds_route && a.lds == b.lds && a.rows_grid_x == b.rows_grid_x && a.cols_grid_x == b.cols_grid_x &&
           a.winner_grid_x == b.winner_grid_x && a.segments == b.segments && a.paths == b.paths && a.diag_grid_x == b.diag_grid_x &&
           a.guided == b.guided && a.guide_weight == b.guide_weight && a.guide_cap == b.guide_cap;
}

int main()
{
    static_assert(kSgmCostAbsdiff == 0 && kSgmCostCensus == 1, "DCMT_SGM_COST_ABSDIFF, DCMT_SGM_COST_CENSUS");
    static_assert(kSgmLdsPerColCensus == 16 && kSgmLdsPerColCensusGuided == kSgmLdsPerColCensus + 2, "one uint4 a column; an int16 hint behind them");
    static_assert(kSgmLdsBudget / kSgmLdsPerColCensus == 4096 && kSgmLdsBudget / kSgmLdsPerColCensusGuided == 3640, "the last widths on the LDS routes");
    static_assert(10 * 25 * 24 == 6000 && 6000 <= 6375, "C of census is within the bound every limit was derived from");
    CHECK(sgm_lds_per_col(kSgmCostAbsdiff, false) == 16 && sgm_lds_per_col(kSgmCostAbsdiff, true) == 18);
    CHECK(sgm_lds_per_col(kSgmCostCensus, false) == 16 && sgm_lds_per_col(kSgmCostCensus, true) == 18);

    const int widths[] = {1, 2, 9, 64, 65, 130, 257, 1216, 1242, 1927, 1928, 2048, 2049, 3640, 3641, 4096, 4097, 49160};

    // ---- cost 0: the old plan, with and without a guide ------------------------------------------------------------------------------
    for (int paths : {4, 8})
        for (int D : {16, 64, 128})
            for (int cols : widths)
                for (uintptr_t guide : {(uintptr_t)0, kGuide}) {
                    const size_t bytes = 2 * sgm_frame_bytes(3, cols, D);
                    const SgmPlan old_call = plan_sgm(3, cols, 5, D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, bytes, paths, guide, 100, 1000);
                    const SgmPlan p = with_cost(cols, D, paths, guide, 0);
                    CHECK(old_call.status == kOk && p.status == kOk && same_old_fields(p, old_call) && p.cost == 0 && old_call.cost == 0);
                    const size_t per = guide ? 18 : 16, last = guide ? 3640 : 4096;
                    CHECK(p.lds_route == ((size_t)cols <= last) && p.lds == ((size_t)cols <= last ? per * cols : 0));
                }

    // ---- a cost that does not exist ----------------------------------------------------------------------------------------------------
    for (int cost : {2, -1, 3, 256, INT_MAX, INT_MIN})
        for (uintptr_t guide : {(uintptr_t)0, kGuide}) {
            const SgmPlan p = with_cost(16, 16, 4, guide, cost, 8, 2);
            CHECK(p.status == kInvalid && p.chunk == 0 && p.n_chunks == 0 && p.lds == 0);
        }
    CHECK(with_cost(16, 16, 4, 0, 0, 8, 2).status == kOk && with_cost(16, 16, 4, 0, 1, 8, 2).status == kOk);
    CHECK(with_cost(16, 16, 8, kGuide, 1, 8, 2).status == kOk);

    // ---- census: the LDS bytes and the route follow from 16 / 18 bytes a column; everything else is the plan of cost 0 -----------------
    for (int paths : {4, 8})
        for (int D : {16, 64, 128})
            for (int cols : widths)
                for (uintptr_t guide : {(uintptr_t)0, kGuide}) {
                    const SgmPlan a = with_cost(cols, D, paths, guide, 0), c = with_cost(cols, D, paths, guide, 1);
                    const size_t per = kSgmLdsPerColCensus + (guide ? 2 : 0), last = kSgmLdsBudget / per;
                    CHECK(last == (guide ? 3640u : 4096u));
                    CHECK(c.status == kOk && c.cost == 1 && c.guided == (guide != 0));
                    CHECK(c.lds_route == ((size_t)cols <= last) && c.lds == ((size_t)cols <= last ? per * cols : 0) && c.lds <= kSgmLdsBudget);
                    SgmPlan h = c;
                    h.lds_route = a.lds_route; h.lds = a.lds;
                    CHECK(same_old_fields(h, a) && c.chunk == 2 && c.n_chunks == 3);
                }
    // the route flips: the last LDS width and the first global width, unguided and guided
    CHECK(with_cost(4096, 16, 4, 0, 1).lds_route && with_cost(4096, 16, 4, 0, 1).lds == 65536);
    CHECK(!with_cost(4097, 16, 4, 0, 1).lds_route && with_cost(4097, 16, 4, 0, 1).lds == 0);
    CHECK(with_cost(3640, 16, 4, kGuide, 1).lds_route && with_cost(3640, 16, 4, kGuide, 1).lds == 65520);
    CHECK(!with_cost(3641, 16, 4, kGuide, 1).lds_route && with_cost(3641, 16, 4, kGuide, 1).lds == 0);
    CHECK(with_cost(3641, 16, 4, 0, 1).lds_route);

    // ---- the older refusals are still there with census: once each ---------------------------------------------------------------------
    const size_t wb = 2 * sgm_frame_bytes(8, 16, 16);
    const auto census = [&](int D, int p1, int p2, int uniq, uintptr_t l, uintptr_t d, uintptr_t z, uintptr_t w, size_t bytes, int paths, uintptr_t g,
                            int weight, int cap) {
        return plan_sgm(8, 16, 2, D, p1, p2, uniq, l, kRight, d, z, w, bytes, paths, g, weight, cap, kSgmCostCensus).status;
    };
    CHECK(census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 4, kGuide, 100, 1000) == kOk);
    CHECK(census(24, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 4, kGuide, 100, 1000) == kInvalid);
    CHECK(census(16, 801, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 4, kGuide, 100, 1000) == kInvalid);
    CHECK(census(16, 200, 10001, 10, kLeft, kDisp, kDepth, kWork, wb, 4, 0, 0, 0) == kInvalid && census(16, 200, 10000, 10, kLeft, kDisp, kDepth, kWork, wb, 4, 0, 0, 0) == kOk);
    CHECK(census(16, 200, 1801, 10, kLeft, kDisp, kDepth, kWork, wb, 8, 0, 0, 0) == kInvalid && census(16, 200, 1800, 10, kLeft, kDisp, kDepth, kWork, wb, 8, 0, 0, 0) == kOk);
    CHECK(census(16, 200, 800, 101, kLeft, kDisp, kDepth, kWork, wb, 4, 0, 0, 0) == kInvalid && census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 5, 0, 0, 0) == kInvalid);
    CHECK(census(16, 200, 800, 10, 0, kDisp, kDepth, kWork, wb, 4, 0, 0, 0) == kInvalid && census(16, 200, 800, 10, kLeft, 0, 0, kWork, wb, 4, 0, 0, 0) == kInvalid);
    CHECK(census(16, 200, 800, 10, kLeft, kDisp + 1, kDepth, kWork, wb, 4, 0, 0, 0) == kInvalid && census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork + 8, wb, 4, 0, 0, 0) == kInvalid);
    CHECK(census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb / 2 - 1, 4, 0, 0, 0) == kInvalid && census(16, 200, 800, 10, kLeft, kLeft, kDepth, kWork, wb, 4, 0, 0, 0) == kInvalid);
    CHECK(census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 8, kGuide, 100, 1001) == kInvalid && census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 4, kGuide, 10001, 0) == kInvalid);
    CHECK(census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 4, kGuide + 2, 100, 1000) == kInvalid && census(16, 200, 800, 10, kLeft, kDisp, kDepth, kWork, wb, 4, kDisp, 100, 1000) == kInvalid);

    if (failures) std::printf("%d checks failed\n", failures); else std::printf("ok\n");
    return failures;
}
