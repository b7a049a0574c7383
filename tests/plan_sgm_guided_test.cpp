// plan_sgm (csrc/dcmt_sgm.h) with a guide, on a CPU.  Built and run by tests/test_sgm_guided.py; prints every failed check and returns
// their number.  Without a guide the plan is field for field the old one and the two integers are not looked at; with one the
// limit on p2 bounds p2 + guide_cap, the weight has its range, the guide is 4-byte aligned and apart from the outputs and the
// workspace, and the rows kernel stages 18 bytes a column, so the LDS route ends at 3640 columns.
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

static SgmPlan guided(int rows, int cols, int batch, int D, int p2, size_t held, int paths, uintptr_t guide, int weight, int cap)
{
    return plan_sgm(rows, cols, batch, D, 0, p2, 10, kLeft, kRight, kDisp, kDepth, kWork, held * sgm_frame_bytes(rows, cols, D), paths, guide, weight, cap);
}

// every field the plan had before there was a guide
static bool same_old_fields(const SgmPlan& a, const SgmPlan& b)
{
    return a.status == b.status && a.frame_bytes == b.frame_bytes && a.volume_elems == b.volume_elems && a.chunk == b.chunk && a.n_chunks == b.n_chunks &&
           a.per_lane == b.per_lane && a.lds_route == b.lds_route && a.lds == b.lds && a.rows_grid_x == b.rows_grid_x && a.cols_grid_x == b.cols_grid_x &&
           a.winner_grid_x == b.winner_grid_x && a.segments == b.segments && a.paths == b.paths && a.diag_grid_x == b.diag_grid_x;
}

int main()
{
    static_assert(kSgmLdsPerColGuided == kSgmLdsPerCol + 2 && kSgmMaxGuideWeight == 10000, "an int16 hint a column; the weight dcmt.h states");
    static_assert(4 * (6375 + kSgmMaxP2) == 65500 && 8 * (6375 + kSgmMaxP2Eight) == 65400, "S fits uint16 when the limit bounds p2 + guide_cap");
    static_assert(kSgmLdsBudget / kSgmLdsPerColGuided == 3640 && kSgmLdsBudget / kSgmLdsPerCol == 4096, "the last widths on the LDS routes");

    const int widths[] = {1, 2, 9, 64, 65, 130, 257, 1216, 1242, 3640, 3641, 4096, 4097, 49160};

    // ---- without a guide: the old plan, whatever the two integers are ------------------------------------------------------------
    for (int paths : {4, 8})
        for (int cols : widths) {
            const size_t bytes = 2 * sgm_frame_bytes(3, cols, 16);
            const SgmPlan old_call = plan_sgm(3, cols, 5, 16, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, bytes, paths);
            for (int junk : {0, -1, 100, INT_MAX, INT_MIN}) {
                const SgmPlan p = plan_sgm(3, cols, 5, 16, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, bytes, paths, 0, junk, junk);
                CHECK(p.status == kOk && same_old_fields(p, old_call) && !p.guided && p.guide_weight == 0 && p.guide_cap == 0);
            }
            CHECK(!old_call.guided && old_call.guide_weight == 0 && old_call.guide_cap == 0);
            CHECK(old_call.lds_route == (cols <= 4096) && old_call.lds == (cols <= 4096 ? (size_t)16 * cols : 0));
        }

    // ---- with a guide: the LDS bytes and the route follow from 18 bytes a column ----------------------------------------------------
    for (int paths : {4, 8})
        for (int D : {16, 64, 128})
            for (int cols : widths) {
                const SgmPlan u = guided(3, cols, 5, D, 800, 2, paths, 0, 0, 0), g = guided(3, cols, 5, D, 800, 2, paths, kGuide, 100, 1000);
                CHECK(u.status == kOk && g.status == kOk && g.guided && g.guide_weight == 100 && g.guide_cap == 1000);
                CHECK(g.lds_route == (cols <= 3640) && g.lds == (cols <= 3640 ? (size_t)18 * cols : 0) && g.lds <= kSgmLdsBudget);
                SgmPlan h = g;                           // everything else is the unguided plan
                h.lds_route = u.lds_route; h.lds = u.lds;
                CHECK(same_old_fields(h, u) && g.chunk == 2 && g.n_chunks == 3);
            }
    CHECK(guided(3, 3640, 1, 16, 800, 1, 4, kGuide, 100, 1000).lds == 65520 && !guided(3, 3641, 1, 16, 800, 1, 4, kGuide, 100, 1000).lds_route);
    CHECK(guided(3, 3641, 1, 16, 800, 1, 4, 0, 0, 0).lds_route && guided(3, 4096, 1, 16, 800, 1, 4, 0, 0, 0).lds == 65536);

    // ---- the two integers --------------------------------------------------------------------------------------------------------
    for (int w : {0, 1, 100, 10000}) CHECK(guided(8, 16, 2, 16, 800, 2, 4, kGuide, w, 1000).status == kOk);
    for (int w : {-1, 10001, INT_MAX, INT_MIN}) CHECK(guided(8, 16, 2, 16, 800, 2, 4, kGuide, w, 1000).status == kInvalid);
    CHECK(guided(8, 16, 2, 16, 800, 2, 4, kGuide, 100, 0).status == kOk && guided(8, 16, 2, 16, 800, 2, 4, kGuide, 0, 0).status == kOk);
    for (int cap : {-1, INT_MIN}) CHECK(guided(8, 16, 2, 16, 800, 2, 4, kGuide, 100, cap).status == kInvalid);
    // p2 + guide_cap against the limit of the path count
    CHECK(guided(8, 16, 2, 16, 800, 2, 8, kGuide, 100, 1000).status == kOk && guided(8, 16, 2, 16, 800, 2, 8, kGuide, 100, 1001).status == kInvalid);
    CHECK(guided(8, 16, 2, 16, 801, 2, 8, kGuide, 100, 1000).status == kInvalid && guided(8, 16, 2, 16, 900, 2, 8, kGuide, 900, 900).status == kOk);
    CHECK(guided(8, 16, 2, 16, 5000, 2, 4, kGuide, 5000, 5000).status == kOk && guided(8, 16, 2, 16, 5000, 2, 4, kGuide, 5000, 5001).status == kInvalid);
    CHECK(guided(8, 16, 2, 16, 0, 2, 4, kGuide, 1, 10000).status == kOk && guided(8, 16, 2, 16, 0, 2, 4, kGuide, 1, 10001).status == kInvalid);
    CHECK(guided(8, 16, 2, 16, 10000, 2, 4, kGuide, 1, 0).status == kOk && guided(8, 16, 2, 16, 10000, 2, 4, kGuide, 1, 1).status == kInvalid);
    CHECK(guided(8, 16, 2, 16, 800, 2, 4, kGuide, 100, INT_MAX).status == kInvalid);          // no overflow in the sum
    CHECK(guided(8, 16, 2, 16, 1800, 2, 8, 0, 100, 1000).status == kOk);                      // without a guide p2 alone is bounded

    // ---- the guide's address -------------------------------------------------------------------------------------------------------
    for (uintptr_t off : {1, 2, 3, 5}) CHECK(guided(8, 16, 2, 16, 800, 2, 4, kGuide + off, 100, 1000).status == kInvalid);
    CHECK(guided(8, 16, 2, 16, 800, 2, 4, kGuide + 4, 100, 1000).status == kOk);
    const size_t px = 2 * 8 * 16, work_bytes = 2 * sgm_frame_bytes(8, 16, 16);
    const auto at = [&](uintptr_t guide) { return guided(8, 16, 2, 16, 800, 2, 4, guide, 100, 1000).status; };
    CHECK(at(kDisp) == kInvalid && at(kDisp + 2 * px - 4) == kInvalid && at(kDisp + 2 * px) == kOk && at(kDisp - 4 * px + 4) == kInvalid && at(kDisp - 4 * px) == kOk);
    CHECK(at(kDepth) == kInvalid && at(kDepth + 4 * px - 4) == kInvalid && at(kDepth + 4 * px) == kOk && at(kDepth - 4 * px) == kOk);
    CHECK(at(kWork) == kInvalid && at(kWork + work_bytes - 4) == kInvalid && at(kWork + work_bytes) == kOk && at(kWork - 4 * px + 4) == kInvalid);
    CHECK(at(kLeft) == kOk && at(kRight) == kOk);            // the inputs may share memory
    // an output that is not there cannot overlap
    CHECK(plan_sgm(8, 16, 2, 16, 0, 800, 10, kLeft, kRight, 0, kDepth, kWork, work_bytes, 4, kDisp, 100, 1000).status == kOk);
    CHECK(plan_sgm(8, 16, 2, 16, 0, 800, 10, kLeft, kRight, kDisp, 0, kWork, work_bytes, 4, kDepth, 100, 1000).status == kOk);

    // ---- the old refusals are still there with a guide: once each --------------------------------------------------------------------
    CHECK(guided(8, 16, 2, 24, 800, 2, 4, kGuide, 100, 1000).status == kInvalid && guided(8, 16, 2, 16, 800, 0, 4, kGuide, 100, 1000).status == kInvalid);
    CHECK(guided(8, 16, 2, 16, 800, 2, 5, kGuide, 100, 1000).status == kInvalid && guided(8, 16, 2, 16, 10001, 2, 4, kGuide, 0, 0).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 801, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, work_bytes, 4, kGuide, 100, 1000).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 0, 800, 101, kLeft, kRight, kDisp, kDepth, kWork, work_bytes, 4, kGuide, 100, 1000).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 0, 800, 10, kLeft, kRight, 0, 0, kWork, work_bytes, 4, kGuide, 100, 1000).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 0, 800, 10, kLeft, kRight, kDisp + 1, kDepth, kWork, work_bytes, 4, kGuide, 100, 1000).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 0, 800, 10, kLeft, kRight, kLeft, kDepth, kWork, work_bytes, 4, kGuide, 100, 1000).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 0, 800, 10, 0, kRight, kDisp, kDepth, kWork, work_bytes, 4, kGuide, 100, 1000).status == kInvalid);

    if (failures) std::printf("%d checks failed\n", failures); else std::printf("ok\n");
    return failures;
}
