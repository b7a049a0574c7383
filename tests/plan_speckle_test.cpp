// plan_speckles (csrc/dcmt_plan_side.h) on a CPU.  Built and run by tests/test_speckle.py; prints every failed check and returns
// their number.  The tiles cover the frame, every pixel pair across a tile edge has its thread, the grids stay inside a launch's
// limits from 1 x 1 to the largest frame a context admits, the wide apply kernel is chosen only where its accesses are aligned, and
// every refusal that is the plan's.
#include <cstdio>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// far apart (65535 frames of 2^29 pixels are 2^47 bytes of depth), 16-byte aligned: no overlap at any size used here
static const uintptr_t kDisp = 1ull << 56, kOut = 2ull << 56, kDepth = 3ull << 56, kRemoved = 4ull << 56;

static SpecklePlan good(int rows, int cols, int batch, uintptr_t disp = kDisp, uintptr_t out = kOut, uintptr_t depth = kDepth, uintptr_t removed = kRemoved)
{
    const SpecklePlan p = plan_speckles(rows, cols, batch, 200, 32, -16, disp, out, depth, removed);
    CHECK(p.status == kOk);
    const uint64_t n = (uint64_t)rows * cols;
    CHECK(p.g.n == n && (1u << p.g.kbits) >= (uint32_t)rows && (p.g.kbits == 0 || (1u << (p.g.kbits - 1)) < (uint32_t)rows));
    CHECK(((uint64_t)(cols - 1) << p.g.kbits | (uint64_t)(rows - 1)) < (1ull << 32));              // every key fits a word
    CHECK((uint64_t)p.g.tiles_x * kConnTW >= (uint64_t)cols && (uint64_t)(p.g.tiles_x - 1) * kConnTW < (uint64_t)cols);
    CHECK((uint64_t)p.g.tiles_y * kConnTH >= (uint64_t)rows && (uint64_t)(p.g.tiles_y - 1) * kConnTH < (uint64_t)rows);
    CHECK(p.g.local_x == (uint64_t)p.g.tiles_x * p.g.tiles_y && p.g.local_x <= 0x7fffffffu);
    CHECK(p.g.pairs_v == (uint64_t)(p.g.tiles_x - 1) * rows && p.g.pairs == (uint64_t)p.g.pairs_v + (uint64_t)(p.g.tiles_y - 1) * cols);
    CHECK((uint64_t)p.g.border_x * 256 >= p.g.pairs && (p.g.border_x == 0 || (uint64_t)(p.g.border_x - 1) * 256 < p.g.pairs));
    CHECK((p.g.border_x == 0) == (p.g.tiles_x == 1 && p.g.tiles_y == 1));
    CHECK((uint64_t)p.g.px_x * 256 >= n && (uint64_t)(p.g.px_x - 1) * 256 < n);
    CHECK(p.vec == 1 || p.vec == 4);
    CHECK((p.vec == 4) == (n % 4 == 0 && disp % 8 == 0 && out % 8 == 0));
    const uint64_t threads = n / p.vec;
    CHECK((uint64_t)p.apply_x * 256 >= threads && (uint64_t)(p.apply_x - 1) * 256 < threads);
    CHECK(((uint64_t)p.apply_x * 256 + 255) * p.vec < (1ull << 32));                              // the pixel index of the last thread fits 32 bits
    CHECK(p.clear_bytes == (removed ? (size_t)4 * batch : 0));
    return p;
}

int main()
{
    const int shapes[][2] = {{1, 1}, {1, 70}, {16, 64}, {17, 65}, {16, 65}, {17, 64}, {33, 129}, {5, 4097}, {375, 1242}, {352, 1216}, {8, 8},
                             {512, 512}, {1 << 14, 1 << 15}, {1, 0x1ffffff0}, {0x1ffffff0, 1}, {23169, 23169}};
    for (const auto& s : shapes)
        for (int batch : {1, 2, 5, 64, 65535}) {
            good(s[0], s[1], batch);
            good(s[0], s[1], batch, kDisp, kDisp);                       // in place
            good(s[0], s[1], batch, kDisp, kOut, 0, 0);
            good(s[0], s[1], batch, kDisp + 2, kOut);                    // 2-byte aligned only: one pixel a thread
            good(s[0], s[1], batch, kDisp, kOut + 6);
            good(s[0], s[1], batch, kDisp + 4, kDisp + 4);
        }
    {
        const SpecklePlan p = good(16, 64, 3);
        CHECK(p.g.tiles_x == 1 && p.g.tiles_y == 1 && p.g.local_x == 1 && p.g.pairs == 0 && p.g.border_x == 0 && p.g.px_x == 4 && p.vec == 4 && p.apply_x == 1);
        const SpecklePlan q = good(17, 65, 3);
        CHECK(q.g.tiles_x == 2 && q.g.tiles_y == 2 && q.g.pairs_v == 17 && q.g.pairs == 17 + 65 && q.g.border_x == 1 && q.vec == 1 && q.apply_x == 5 && q.g.kbits == 5);
        const SpecklePlan r = good(352, 1216, 64);
        CHECK(r.g.tiles_x == 19 && r.g.tiles_y == 22 && r.g.pairs_v == 18 * 352 && r.g.pairs == 18 * 352 + 21 * 1216 && r.vec == 4 && r.apply_x == 418);
        CHECK(good(1, 1, 1).g.kbits == 0 && good(1, 1, 1).g.local_x == 1 && good(1, 1, 1).vec == 1);
    }

    // ---- refusals --------------------------------------------------------------------------------------------------------------
    const int rows = 8, cols = 16, batch = 2;
    const size_t px = (size_t)batch * rows * cols;
    const auto plan = [&](int64_t size, int64_t diff, int64_t nv, uintptr_t disp, uintptr_t out, uintptr_t depth, uintptr_t removed) {
        return plan_speckles(rows, cols, batch, size, diff, nv, disp, out, depth, removed).status;
    };
    CHECK(plan(200, 32, -16, kDisp, kOut, kDepth, kRemoved) == kOk && plan(200, 32, -16, kDisp, kDisp, 0, 0) == kOk);
    CHECK(plan(0, 0, -32768, kDisp, kOut, kDepth, kRemoved) == kOk && plan(0x7fffffff, 65535, 32767, kDisp, kOut, kDepth, kRemoved) == kOk);
    CHECK(plan(200, 32, -16, 0, kOut, kDepth, kRemoved) == kInvalid && plan(200, 32, -16, kDisp, 0, kDepth, kRemoved) == kInvalid);
    CHECK(plan(-1, 32, -16, kDisp, kOut, kDepth, kRemoved) == kInvalid && plan(200, -1, -16, kDisp, kOut, kDepth, kRemoved) == kInvalid);
    CHECK(plan(200, 65536, -16, kDisp, kOut, kDepth, kRemoved) == kInvalid);
    CHECK(plan(200, 32, -32769, kDisp, kOut, kDepth, kRemoved) == kInvalid && plan(200, 32, 32768, kDisp, kOut, kDepth, kRemoved) == kInvalid);
    // alignment
    CHECK(plan(200, 32, -16, kDisp + 1, kOut, kDepth, kRemoved) == kInvalid && plan(200, 32, -16, kDisp, kOut + 1, kDepth, kRemoved) == kInvalid);
    CHECK(plan(200, 32, -16, kDisp + 1, kDisp + 1, kDepth, kRemoved) == kInvalid);
    for (uintptr_t off : {1, 2, 3}) {
        CHECK(plan(200, 32, -16, kDisp, kOut, kDepth + off, kRemoved) == kInvalid);
        CHECK(plan(200, 32, -16, kDisp, kOut, kDepth, kRemoved + off) == kInvalid);
    }
    CHECK(plan(200, 32, -16, kDisp + 2, kOut + 2, kDepth + 4, kRemoved + 4) == kOk);
    // overlaps: out over disp other than exactly; depth over either; removed over any
    CHECK(plan(200, 32, -16, kDisp, kDisp + 2, kDepth, kRemoved) == kInvalid && plan(200, 32, -16, kDisp, kDisp + 2 * px - 2, kDepth, kRemoved) == kInvalid);
    CHECK(plan(200, 32, -16, kDisp, kDisp - 2 * px + 2, kDepth, kRemoved) == kInvalid);
    CHECK(plan(200, 32, -16, kDisp, kDisp + 2 * px, kDepth, kRemoved) == kOk && plan(200, 32, -16, kDisp, kDisp - 2 * px, kDepth, kRemoved) == kOk);
    CHECK(plan(200, 32, -16, kDisp, kOut, kDisp, kRemoved) == kInvalid && plan(200, 32, -16, kDisp, kOut, kOut + 2 * px - 4, kRemoved) == kInvalid);
    CHECK(plan(200, 32, -16, kDisp, kDisp, kDisp, kRemoved) == kInvalid && plan(200, 32, -16, kDisp, kOut, kDisp - 4 * px + 4, kRemoved) == kInvalid);
    CHECK(plan(200, 32, -16, kDisp, kOut, kDisp + 2 * px, kRemoved) == kOk && plan(200, 32, -16, kDisp, kOut, kDisp - 4 * px, kRemoved) == kOk);
    CHECK(plan(200, 32, -16, kDisp, kOut, kDepth, kDisp) == kInvalid && plan(200, 32, -16, kDisp, kOut, kDepth, kOut + 2 * px - 4) == kInvalid);
    CHECK(plan(200, 32, -16, kDisp, kOut, kDepth, kDepth + 4 * px - 4) == kInvalid && plan(200, 32, -16, kDisp, kOut, kDepth, kDisp - 4) == kInvalid);
    CHECK(plan(200, 32, -16, kDisp, kOut, kDepth, kDepth + 4 * px) == kOk && plan(200, 32, -16, kDisp, kOut, kDepth, kDisp - 8) == kOk);
    CHECK(plan(200, 32, -16, kDisp, kOut, 0, kDisp + 2 * px) == kOk);

    if (failures) std::printf("%d checks failed\n", failures); else std::printf("ok\n");
    return failures;
}
