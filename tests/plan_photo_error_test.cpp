// plan_photo_error (csrc/dcmt_plan_side.h) on a CPU.  Built and run by tests/test_photo_error.py; prints every failed check and
// returns their number.  Pins the route, the grid and the LDS bytes of every shape tests/test_gpu_photo_error.py uses, for window
// 1..4, and that no plan exceeds 160 KB of LDS or 2^31 - 1 workgroups; names the shape that takes the fallback route.
#include <cstdio>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// far apart, 16-byte aligned: no overlap at any size used here
static const uintptr_t kDepth = 0x100000000000ull, kLeft = 0x200000000000ull, kRight = 0x300000000000ull, kErr = 0x400000000000ull,
                       kStats = 0x500000000000ull, kTable = 0x600000000000ull;

static PhotoPlan good(int rows, int cols, int batch, int window)
{
    const PhotoPlan p = plan_photo_error(rows, cols, batch, window, kDepth, kLeft, kRight, false, 0, kErr, kStats);
    CHECK(p.status == kOk);
    CHECK(p.grid_y == (unsigned)batch && p.clear_bytes == 32u * (size_t)batch);
    CHECK(p.lds <= 160 * 1024 && p.lds <= kPhotoLdsBudget);
    CHECK((uint64_t)p.grid_x * p.grid_y <= 0x7fffffffull && p.grid_x >= 1);
    CHECK(p.vec == (cols % 16 == 0));
    if (p.lds_route) {
        CHECK(p.band >= 1 && p.band <= (uint32_t)kPhotoBandRows);
        CHECK(p.pitch % 16 == 0 && p.pitch >= (uint32_t)cols + 32);
        CHECK(p.lds == (size_t)2 * (p.band + 2 * window - 1) * p.pitch);
        CHECK((uint64_t)p.grid_x * p.band >= (uint64_t)rows && (uint64_t)(p.grid_x - 1) * p.band < (uint64_t)rows);
        // what the kernel reads of a staged row stays inside its pitch: the left window's three dwords from column j0 - 4, the right
        // window's two or three aligned dwords around column pr - window, pr <= cols - 1
        const uint32_t j0 = ((uint32_t)cols - 1) & ~3u;
        CHECK(kPhotoPadLeft + j0 - 4 + 12 <= p.pitch);
        CHECK(((kPhotoPadLeft + (uint32_t)cols - 1 - window) & ~3u) + 12 <= p.pitch);
        CHECK(kPhotoPadLeft >= (uint32_t)window + 3);
    } else {
        CHECK(p.lds == 0 && (uint64_t)p.grid_x * kPhotoGlobalPx >= (uint64_t)rows * cols && (uint64_t)(p.grid_x - 1) * kPhotoGlobalPx < (uint64_t)rows * cols);
        CHECK(photo_lds_bytes(1, window, cols) > kPhotoLdsBudget);
    }
    return p;
}

struct Pin { int rows, cols, batch, window; bool lds_route; uint32_t band; size_t lds; unsigned grid_x; };

int main()
{
    // every shape of the GPU test at batch 1 and 3 and window 1..4: LDS = 2 * (band + 2 w - 1) * pitch, pitch = (cols + 32) up to 16
    const int small[][2] = {{1, 1}, {1, 9}, {9, 1}, {3, 5}, {5, 7}, {37, 131}, {64, 256}, {65, 257}, {352, 1216}};
    const uint32_t pitch[] = {48, 48, 48, 48, 48, 176, 288, 304, 1248};
    for (int s = 0; s < 9; ++s)
        for (int batch : {1, 3})
            for (int w = 1; w <= 4; ++w) {
                const int rows = small[s][0], cols = small[s][1];
                const PhotoPlan p = good(rows, cols, batch, w);
                // none of these calls makes 512 workgroups: bands of 2 rows
                CHECK(p.lds_route && p.band == 2 && p.pitch == pitch[s]);
                CHECK(p.lds == (size_t)2 * (2 * w + 1) * pitch[s] && p.grid_x == (unsigned)((rows + 1) / 2));
            }
    const Pin pins[] = {
        {352, 1216, 1, 2, true, 2, 12480, 176},         // the reference's frame and window, one at a time
        {352, 1216, 3, 4, true, 2, 22464, 176},
        {352, 1216, 12, 2, true, 8, 27456, 44},         // 44 * 12 >= 512: full bands, 11 staged rows of 1248 bytes, twice
        {352, 1216, 1024, 2, true, 8, 27456, 44},       // the measured batch
        {4096, 16, 1, 1, true, 8, 864, 512},            // the smallest calls of the GPU test with bands of 8 ...
        {4100, 20, 1, 3, true, 8, 1664, 513},
        {2100, 16, 1, 2, true, 4, 672, 525},            // ... and of 4 rows
        {5, 3000, 1, 4, true, 2, 54720, 3},             // 8 and 4 rows of window 4 do not fit 64 KB at 3000 columns; 2 do
        {5, 3000, 1, 2, true, 2, 30400, 3},             // (fewer than 512 workgroups)
        {3, 16400, 1, 1, false, 0, 0, 193},             // THE FALLBACK SHAPE of the GPU test: not even window 1's two rows fit
        {3, 16400, 3, 4, false, 0, 0, 193},
    };
    for (const Pin& k : pins) {
        const PhotoPlan p = good(k.rows, k.cols, k.batch, k.window);
        CHECK(p.lds_route == k.lds_route && p.band == k.band && p.lds == k.lds && p.grid_x == k.grid_x);
    }
    // the route's threshold, per window: the widest frame whose single-row band fits, and the next one
    for (int w = 1; w <= 4; ++w) {
        int cols = 1;
        while (photo_lds_bytes(1, w, cols + 1) <= kPhotoLdsBudget) ++cols;
        CHECK(good(2, cols, 1, w).lds_route && good(2, cols, 1, w).band == 1);
        CHECK(!good(2, cols + 1, 1, w).lds_route);
    }
    // the limits: the tallest and the widest frame a context admits (0x1ffffff0 pixels), the largest batch
    for (int w = 1; w <= 4; ++w) {
        CHECK(good(0x1ffffff0, 1, 1, w).grid_x == 0x1ffffff0 / 8);
        CHECK(good(1, 0x1ffffff0, 1, w).grid_x == (0x1ffffff0 + 255) / 256);
        CHECK(good(352, 1216, 65535, w).band == 8);
    }
    CHECK(plan_photo_error(4, 4, 65536, 2, kDepth, kLeft, kRight, false, 0, kErr, kStats).status == kInvalid);

    // outputs: either may be left out, not both; without statistics nothing is cleared
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kErr, 0).status == kOk);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kErr, 0).clear_bytes == 0);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, 0, kStats).status == kOk);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, 0, 0).status == kInvalid);
    // null inputs, the window, alignment
    CHECK(plan_photo_error(8, 16, 2, 2, 0, kLeft, kRight, false, 0, kErr, kStats).status == kInvalid);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, 0, kRight, false, 0, kErr, kStats).status == kInvalid);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, 0, false, 0, kErr, kStats).status == kInvalid);
    for (int w : {-1, 0, 5, 1 << 30}) CHECK(plan_photo_error(8, 16, 2, w, kDepth, kLeft, kRight, false, 0, kErr, kStats).status == kInvalid);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth + 2, kLeft, kRight, false, 0, kErr, kStats).status == kInvalid);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kErr, kStats + 4).status == kInvalid);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft + 1, kRight + 3, false, 0, kErr + 1, kStats).status == kOk);
    CHECK(!plan_photo_error(8, 16, 2, 2, kDepth, kLeft + 1, kRight, false, 0, kErr, kStats).vec);
    CHECK(!plan_photo_error(8, 16, 2, 2, kDepth + 4, kLeft, kRight, false, 0, kErr, kStats).vec);
    CHECK(!plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kErr + 2, kStats).vec);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, 0, kStats).vec);
    // the table: wanted by the table call only, 8-byte aligned
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, kErr, kStats).status == kOk);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, 0, kErr, kStats).status == kInvalid);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable + 4, kErr, kStats).status == kInvalid);
    // overlaps: each output against each input and the table, by its last and first byte; the outputs against each other
    const size_t px = 2 * 8 * 16, sb = 32 * 2, tb = 8 * 2;
    const struct { uintptr_t in; size_t bytes; } inputs[] = {{kDepth, 4 * px}, {kLeft, px}, {kRight, px}, {kTable, tb}};
    for (const auto& in : inputs) {
        CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, in.in + in.bytes - 1, kStats).status == kInvalid);
        CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, in.in - px + 1, kStats).status == kInvalid);
        CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, in.in + in.bytes, kStats).status == kOk);
        CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, in.in - px, kStats).status == kOk);
        CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, kErr, ((in.in + in.bytes - 1) & ~(uintptr_t)7)).status == kInvalid);
        CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, kErr, in.in - sb + 8).status == kInvalid);
        CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, true, kTable, kErr, in.in - sb).status == kOk);
    }
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kLeft, kStats).status == kInvalid);          // in place: refused
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, kErr, kErr, kStats).status == kOk);             // a uniform call has no table
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kErr, kErr + px - 8).status == kInvalid);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kErr, kErr + px).status == kOk);
    CHECK(plan_photo_error(8, 16, 2, 2, kDepth, kLeft, kRight, false, 0, kStats + 8, kStats).status == kInvalid);

    if (failures == 0) std::printf("ok\n");
    return failures;
}
