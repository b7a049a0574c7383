// plan_sgm (csrc/dcmt_sgm.h) on a CPU.  Built and run by tests/test_sgm.py; prints every failed check and returns their number.
// The chunks cover the batch exactly once whatever the workspace holds; the grids stay inside a launch's limits from 1 x 1 to
// 375 x 1242 x 128 with 65535 frames; byte offsets beyond 2^32 are computed in 64 bits; every refusal that is the plan's.
#include <cstdio>
#include <initializer_list>

#include "dcmt_sgm.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// far apart, 16-byte aligned: no overlap at any size used here
static const uintptr_t kLeft = 0x100000000000ull, kRight = 0x200000000000ull, kDisp = 0x300000000000ull, kDepth = 0x400000000000ull,
                       kWork = 0x500000000000ull;

static SgmPlan plan_of(int rows, int cols, int batch, int D, size_t work_bytes)
{
    return plan_sgm(rows, cols, batch, D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, work_bytes);
}

static SgmPlan good(int rows, int cols, int batch, int D, size_t held)
{
    const size_t frame = (size_t)4 * rows * cols * D;
    const SgmPlan p = plan_of(rows, cols, batch, D, held * frame + 15);     // a few bytes over: not another frame
    CHECK(p.status == kOk);
    CHECK(p.frame_bytes == frame && p.frame_bytes % 16 == 0 && p.volume_elems * 4 == frame);
    CHECK(p.chunk >= 1 && p.chunk <= 65535 && (size_t)p.chunk <= held && p.chunk <= batch);
    CHECK(p.chunk == batch || (size_t)p.chunk == held || p.chunk == 65535);
    // the chunks cover the batch exactly once
    long long covered = 0;
    for (int i = 0; i < p.n_chunks; ++i) {
        const int n = sgm_chunk_frames(p, batch, i);
        CHECK(n >= 1 && n <= p.chunk);
        CHECK((long long)i * p.chunk == covered);
        covered += n;
    }
    CHECK(covered == batch);
    CHECK(p.per_lane == (D > 64 ? 2 : 1) && 64 * p.per_lane >= D);
    CHECK(p.lds_route == ((size_t)cols * kSgmLdsPerCol <= kSgmLdsBudget));
    CHECK(p.lds == (p.lds_route ? (size_t)cols * kSgmLdsPerCol : 0) && p.lds <= 64 * 1024);
    // grids: x below 2^31, y (the frames of a chunk) below 65536; every row, column and segment has its wave
    CHECK(p.rows_grid_x == (unsigned)rows && p.rows_grid_x <= 0x7fffffffu);
    CHECK((uint64_t)p.cols_grid_x * kSgmWaves >= (uint64_t)cols && (uint64_t)(p.cols_grid_x - 1) * kSgmWaves < (uint64_t)cols);
    CHECK((uint64_t)p.segments * kSgmSegment >= (uint64_t)cols && (uint64_t)(p.segments - 1) * kSgmSegment < (uint64_t)cols);
    const uint64_t waves = (uint64_t)rows * p.segments;
    CHECK((uint64_t)p.winner_grid_x * kSgmWaves >= waves && (uint64_t)(p.winner_grid_x - 1) * kSgmWaves < waves && p.winner_grid_x <= 0x7fffffffu);
    return p;
}

int main()
{
    const int shapes[][2] = {{1, 1}, {1, 70}, {3, 33}, {7, 40}, {16, 70}, {9, 65}, {11, 130}, {24, 257}, {12, 1242}, {375, 1242}, {352, 1216},
                             {3, 4096}, {3, 4097}, {2, 49160}};
    for (int D : {16, 32, 48, 64, 80, 128})
        for (const auto& s : shapes) {
            const int rows = s[0], cols = s[1];
            for (int batch : {1, 2, 5, 64, 65535, 65536, 100000})
                for (size_t held : {(size_t)1, (size_t)2, (size_t)5, (size_t)16, (size_t)65535, (size_t)200000}) good(rows, cols, batch, D, held);
        }
    // batch 5 with room for 1, 2 and 5 frames: 5, 3 (2 + 2 + 1) and 1 chunks
    CHECK(good(24, 96, 5, 32, 1).n_chunks == 5 && good(24, 96, 5, 32, 2).n_chunks == 3 && good(24, 96, 5, 32, 5).n_chunks == 1);
    CHECK(sgm_chunk_frames(good(24, 96, 5, 32, 2), 5, 2) == 1 && good(24, 96, 5, 32, 9).chunk == 5);
    // the largest frame at the largest D and 65535 frames: one frame is 238 MB, the workspace of the batch beyond 2^43 bytes
    {
        const SgmPlan p = good(375, 1242, 65535, 128, 65535);
        CHECK(p.frame_bytes == (size_t)4 * 375 * 1242 * 128 && p.chunk == 65535 && p.n_chunks == 1);
        CHECK((uint64_t)p.frame_bytes * 65535ull > (1ull << 43) && sgm_frame_bytes(375, 1242, 128) * (size_t)65535 == (uint64_t)p.frame_bytes * 65535ull);
        CHECK(p.rows_grid_x == 375 && p.cols_grid_x == 311 && p.segments == 20 && p.winner_grid_x == 1875);
        // a frame of 2^29 pixels: volume_elems itself is beyond 2^32
        const SgmPlan q = good(1 << 14, 1 << 15, 1, 128, 1);
        CHECK(q.volume_elems == ((size_t)1 << 36) && q.frame_bytes == ((size_t)1 << 38));
    }
    const SgmPlan one = good(1, 1, 1, 16, 1);
    CHECK(one.frame_bytes == 64 && one.rows_grid_x == 1 && one.cols_grid_x == 1 && one.winner_grid_x == 1 && one.lds == 16);
    CHECK(good(12, 1242, 1, 64, 1).lds == 19872 && good(3, 4096, 1, 64, 1).lds_route && !good(3, 4097, 1, 64, 1).lds_route);

    // ---- refusals --------------------------------------------------------------------------------------------------------------
    const int rows = 8, cols = 16, batch = 2, D = 16;
    const size_t px = (size_t)batch * rows * cols, frame = (size_t)4 * rows * cols * D, wb = 2 * frame;
    const auto plan = [&](int d, int p1, int p2, int u, uintptr_t l, uintptr_t r, uintptr_t disp, uintptr_t depth, uintptr_t work, size_t bytes) {
        return plan_sgm(rows, cols, batch, d, p1, p2, u, l, r, disp, depth, work, bytes).status;
    };
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, wb) == kOk);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, 0, kDepth, kWork, wb) == kOk && plan(D, 200, 800, 10, kLeft, kRight, kDisp, 0, kWork, wb) == kOk);
    CHECK(plan(D, 0, 0, 0, kLeft, kLeft, kDisp, kDepth, kWork, frame) == kOk && plan(D, 10000, 10000, 100, kLeft, kRight, kDisp, kDepth, kWork, frame) == kOk);
    CHECK(plan(D, 200, 800, 10, 0, kRight, kDisp, kDepth, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, 0, kDisp, kDepth, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, 0, 0, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, 0, wb) == kInvalid);
    for (int d : {0, 8, 15, 17, 24, 144, 256, -16}) CHECK(plan(d, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, (size_t)1 << 30) == kInvalid);
    CHECK(plan(D, -1, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, wb) == kInvalid && plan(D, 801, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 10001, 10, kLeft, kRight, kDisp, kDepth, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 800, -1, kLeft, kRight, kDisp, kDepth, kWork, wb) == kInvalid && plan(D, 200, 800, 101, kLeft, kRight, kDisp, kDepth, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp + 1, kDepth, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDepth + 2, kWork, wb) == kInvalid);
    for (uintptr_t off : {1, 2, 4, 8}) CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork + off, wb) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, frame - 1) == kInvalid && plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, 0) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDepth, kWork, frame) == kOk);
    // overlaps: an output over an input, over the other output, over the workspace; the workspace over an input
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kLeft, kDepth, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, kRight, kDisp, kRight + px - 4, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kLeft - 2 * px + 2, kDepth, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, kRight, kLeft - 2 * px, kDepth, kWork, wb) == kOk);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDisp, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDisp + 2 * px - 4, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp, kDisp + 2 * px, kWork, wb) == kOk);
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kWork, kDepth, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, kRight, kDisp, kWork + wb - 16, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kWork + 16, kRight, kDisp, kDepth, kWork, wb) == kInvalid && plan(D, 200, 800, 10, kLeft, kWork + wb - 1, kDisp, kDepth, kWork, wb) == kInvalid);
    CHECK(plan(D, 200, 800, 10, kWork + wb, kRight, kDisp, kDepth, kWork, wb) == kOk);
    // the whole of what the caller calls workspace counts, not only the part a chunk uses
    CHECK(plan(D, 200, 800, 10, kLeft, kRight, kDisp, kWork + 10 * wb, kWork, 10 * wb + 16) == kInvalid);

    if (failures) std::printf("%d checks failed\n", failures); else std::printf("ok\n");
    return failures;
}
