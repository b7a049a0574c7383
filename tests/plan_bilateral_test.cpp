// plan_bilateral5 (csrc/dcmt_plan_side.h) and the cascade's plan with the bilateral finish (csrc/dcmt_plan.h) on a CPU.  Built and
// run by tests/test_bilateral.py; prints every failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dcmt_plan.h"
#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// the waves k_bilateral5 makes of a plan, walked as the kernel walks them: every pixel of a frame is stored exactly once
static GaussPlan checked_bilateral(int rows, int cols, int batch)
{
    const GaussPlan p = plan_bilateral5(rows, cols, batch);
    CHECK(p.strips == (cols + kBilCols - 1) / kBilCols);
    CHECK(p.band_rows == 32 || p.band_rows == 16 || p.band_rows == 8);
    auto waves = [&](int br) { return (size_t)p.strips * ((rows + br - 1) / br) * batch; };
    for (int br = kBilRows; br > p.band_rows; br /= 2) CHECK(waves(br) < 2048);
    CHECK(p.band_rows == 8 || waves(p.band_rows) >= 2048);
    CHECK(p.bands == (rows + p.band_rows - 1) / p.band_rows);
    CHECK(p.grid_x == (unsigned)(((size_t)p.strips * p.bands + 3) / 4));
    std::vector<unsigned char> hit((size_t)rows * cols, 0);
    bool outside = false;
    for (unsigned wg = 0; wg < p.grid_x; ++wg)
        for (int w = 0; w < 4; ++w) {
            const int id = (int)wg * 4 + w;
            if (id >= p.strips * p.bands) continue;
            const int band = id / p.strips, strip = id - band * p.strips;
            const int y0 = band * p.band_rows, R = std::min(p.band_rows, rows - y0);
            for (int l = 2; l < 62; ++l) {
                const int gx = strip * kBilCols - 2 + l;
                if (gx >= cols) continue;
                for (int y = y0; y < y0 + R; ++y) {
                    if (gx < 0 || y < 0 || y >= rows) { outside = true; continue; }
                    ++hit[(size_t)y * cols + gx];
                }
            }
        }
    CHECK(!outside);
    size_t wrong = 0;
    for (unsigned char h : hit) wrong += h != 1;
    CHECK(wrong == 0);
    return p;
}

static void test_plan_bilateral5()
{
    const int shapes[][2] = {{1, 1}, {2, 2}, {1, 70}, {33, 70}, {352, 1216}, {375, 1242}};
    for (const auto& s : shapes)
        for (int batch : {1, 3, 1024}) checked_bilateral(s[0], s[1], batch);
    CHECK(checked_bilateral(352, 1216, 1024).band_rows == 32);
    CHECK(checked_bilateral(352, 1216, 1).band_rows == 8);           // 21 strips x 44 bands = 924 waves
    CHECK(checked_bilateral(352, 1216, 5).band_rows == 16);          // 21 x 22 x 5 = 2310 >= 2048 > 21 x 11 x 5
    CHECK(checked_bilateral(9, 61, 3).strips == 2 && checked_bilateral(9, 61, 3).bands == 2);
}

static bool ends_with(const char* s, const char* tail)
{
    const size_t n = std::strlen(s), m = std::strlen(tail);
    return n >= m && std::strcmp(s + n - m, tail) == 0;
}

// the cascade: with the bilateral finish a call is planned as the same call with stop_after = MEDIAN5 into context scratch, on every route
static void test_plan_call()
{
    const Knobs k;
    for (int batch : {1, 4, 64})
        for (int flags : {0, kFlagForceStaged, kFlagForceFused, kFlagNormalize})
            for (Input in : {Input::F32, Input::U16})
                for (int stop : {kStageBlur, kStageFinal})
                    for (uintptr_t dst : {(uintptr_t)0x200000000ull, (uintptr_t)0x100000000ull, (uintptr_t)0x100000004ull}) {     // apart, in place, one element in
                        if (in == Input::U16 && (flags & kFlagNormalize)) continue;
                        Call c;
                        c.rows = 64; c.cols = 96; c.batch = batch; c.input = in; c.src = 0x100000000ull; c.dst = dst;
                        c.gaussian = false; c.bilateral = true; c.stop_after = stop; c.flags = flags; c.q16_allowed = true;
                        const Plan p = plan_call(k, c);
                        Call m = c;
                        m.bilateral = false; m.stop_after = kStageMedian5; m.dst = 0;
                        const Plan q = plan_call(k, m);
                        CHECK(p.bilateral && !q.bilateral && p.bilateral_invert == (stop == kStageFinal));
                        CHECK(p.route == q.route && p.out == Out::DST && !p.fuse_fp && !p.q16 && !p.needs_x6q);
                        CHECK(p.route == route_of(k, c));
                        CHECK(std::string(p.path) == std::string(q.path) + " + bilateral5" && ends_with(p.path, " + bilateral5"));
                        CHECK(p.pre_grid == q.pre_grid && p.fill_grid == q.fill_grid && p.post_grid == q.post_grid && p.tiles_y == q.tiles_y);
                        // stop_after <= MEDIAN5 ignores the blur; the Gaussian's plans know nothing of it
                        Call e = c;
                        e.stop_after = kStageMedian5;
                        CHECK(!plan_call(k, e).bilateral);
                        Call g = c;
                        g.gaussian = true; g.bilateral = false;
                        CHECK(!plan_call(k, g).bilateral && !ends_with(plan_call(k, g).path, "bilateral5"));
                    }
}

int main()
{
    test_plan_bilateral5();
    test_plan_call();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
