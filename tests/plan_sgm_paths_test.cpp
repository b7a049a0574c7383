// plan_sgm (csrc/dcmt_sgm.h) with the number of paths, on a CPU.  Built and run by tests/test_sgm_paths.py; prints every failed check
// and returns their number.  Paths other than 4 and 8 are refused; the limit on p2 is that of the chosen count; the diagonal launch
// has one wave a start column at widths that are and are not multiples of kSgmWaves; a call without the argument is the old plan.
#include <cstdio>
#include <initializer_list>

#include "dcmt_sgm.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kLeft = 0x100000000000ull, kRight = 0x200000000000ull, kDisp = 0x300000000000ull, kDepth = 0x400000000000ull,
                       kWork = 0x500000000000ull;

static SgmPlan with_paths(int rows, int cols, int batch, int D, int p1, int p2, size_t held, int paths)
{
    return plan_sgm(rows, cols, batch, D, p1, p2, 10, kLeft, kRight, kDisp, kDepth, kWork, held * sgm_frame_bytes(rows, cols, D), paths);
}

// everything the four-path plan says, the eight-path plan says too
static bool same_but_for_the_paths(const SgmPlan& a, const SgmPlan& b)
{
    return a.status == b.status && a.frame_bytes == b.frame_bytes && a.volume_elems == b.volume_elems && a.chunk == b.chunk && a.n_chunks == b.n_chunks &&
           a.per_lane == b.per_lane && a.lds_route == b.lds_route && a.lds == b.lds && a.rows_grid_x == b.rows_grid_x && a.cols_grid_x == b.cols_grid_x &&
           a.winner_grid_x == b.winner_grid_x && a.segments == b.segments;
}

int main()
{
    static_assert(kSgmMaxP2Eight == 1800 && kSgmMaxP2 == 10000, "the limits dcmt.h states");
    static_assert(8 * (6375 + kSgmMaxP2Eight) <= 65535 && 8 * (6375 + kSgmMaxP2Eight) == 65400, "S fits uint16 with eight paths");

    // ---- the path count --------------------------------------------------------------------------------------------------------
    for (int paths : {-8, -4, -1, 0, 1, 2, 3, 5, 6, 7, 9, 12, 16, 1 << 20}) CHECK(with_paths(8, 16, 2, 16, 200, 800, 2, paths).status == kInvalid);
    CHECK(with_paths(8, 16, 2, 16, 200, 800, 2, 4).status == kOk && with_paths(8, 16, 2, 16, 200, 800, 2, 8).status == kOk);
    CHECK(with_paths(8, 16, 2, 16, 200, 800, 2, 4).paths == 4 && with_paths(8, 16, 2, 16, 200, 800, 2, 8).paths == 8);

    // ---- p2: the limit of the chosen count ------------------------------------------------------------------------------------
    CHECK(with_paths(8, 16, 2, 16, 200, 1800, 2, 8).status == kOk && with_paths(8, 16, 2, 16, 1800, 1800, 2, 8).status == kOk);
    CHECK(with_paths(8, 16, 2, 16, 200, 1801, 2, 8).status == kInvalid && with_paths(8, 16, 2, 16, 200, 1801, 2, 4).status == kOk);
    CHECK(with_paths(8, 16, 2, 16, 0, 10000, 2, 8).status == kInvalid && with_paths(8, 16, 2, 16, 0, 10000, 2, 4).status == kOk);
    CHECK(with_paths(8, 16, 2, 16, 0, 10001, 2, 4).status == kInvalid && with_paths(8, 16, 2, 16, 0, 0, 2, 8).status == kOk);
    // the other refusals are still there with eight paths: once each
    CHECK(with_paths(8, 16, 2, 24, 200, 800, 2, 8).status == kInvalid && with_paths(8, 16, 2, 16, 801, 800, 2, 8).status == kInvalid);
    CHECK(with_paths(8, 16, 2, 16, -1, 800, 2, 8).status == kInvalid && with_paths(8, 16, 2, 16, 200, 800, 0, 8).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 200, 800, 101, kLeft, kRight, kDisp, kDepth, kWork, (size_t)1 << 20, 8).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 200, 800, 10, kLeft, kRight, 0, 0, kWork, (size_t)1 << 20, 8).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork + 8, (size_t)1 << 20, 8).status == kInvalid);
    CHECK(plan_sgm(8, 16, 2, 16, 200, 800, 10, kLeft, kRight, kLeft, kDepth, kWork, (size_t)1 << 20, 8).status == kInvalid);

    // ---- the diagonal launch: a wave a start column ------------------------------------------------------------------------------
    const int widths[] = {1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 130, 256, 257, 1216, 1241, 1242, 4096, 4097, 49160};
    for (int D : {16, 64, 128})
        for (int cols : widths)
            for (int rows : {1, 2, 23, 375}) {
                if ((uint64_t)rows * cols > (1u << 22)) continue;
                const SgmPlan e = with_paths(rows, cols, 5, D, 200, 800, 2, 8), f = with_paths(rows, cols, 5, D, 200, 800, 2, 4);
                CHECK(e.status == kOk && f.status == kOk && same_but_for_the_paths(e, f));
                CHECK((uint64_t)e.diag_grid_x * kSgmWaves >= (uint64_t)cols && (uint64_t)(e.diag_grid_x - 1) * kSgmWaves < (uint64_t)cols);
                CHECK(e.diag_grid_x == (unsigned)((cols + kSgmWaves - 1) / kSgmWaves) && e.diag_grid_x == e.cols_grid_x && e.diag_grid_x <= 0x7fffffffu);
                CHECK(f.diag_grid_x == 0 && f.paths == 4 && e.paths == 8);
                CHECK(e.chunk == 2 && e.n_chunks == 3 && sgm_chunk_frames(e, 5, 2) == 1);     // the workspace serves both: the same chunks
            }
    CHECK(with_paths(24, 256, 1, 64, 200, 800, 1, 8).diag_grid_x == 64 && with_paths(24, 257, 1, 64, 200, 800, 1, 8).diag_grid_x == 65);
    CHECK(with_paths(375, 1242, 1, 128, 200, 800, 1, 8).diag_grid_x == 311 && with_paths(1, 1, 1, 16, 0, 0, 1, 8).diag_grid_x == 1);

    // ---- a call without the argument is the four-path plan -----------------------------------------------------------------------
    for (int cols : widths) {
        const size_t bytes = 3 * sgm_frame_bytes(7, cols, 64);
        const SgmPlan old_call = plan_sgm(7, cols, 5, 64, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, bytes);
        const SgmPlan four = plan_sgm(7, cols, 5, 64, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, bytes, 4);
        CHECK(old_call.status == kOk && same_but_for_the_paths(old_call, four) && old_call.paths == 4 && four.paths == 4 && old_call.diag_grid_x == 0);
    }
    CHECK(plan_sgm(8, 16, 2, 16, 0, 10000, 10, kLeft, kRight, kDisp, kDepth, kWork, (size_t)1 << 20).status == kOk);

    if (failures) std::printf("%d checks failed\n", failures); else std::printf("ok\n");
    return failures;
}
