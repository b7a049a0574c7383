// plan_depth_normals, normals_params_ok (csrc/dcmt_plan_side.h) and normals_intrinsics_ok (csrc/dcmt_normals.h) on hand-worked cases,
// on a CPU.  Built and run by tests/test_normals.py; prints every failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kIn = 0x100000000ull, kNrm = 0x300000000ull, kOut = 0x900000000ull, kCnt = 0xb00000000ull, kTab = 0xd00000000ull;

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static uint64_t bits(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static void test_routes()
{
    // out of place: one launch whatever the outputs, no scratch; with counts one more
    NormalsPlan p = plan_depth_normals(352, 1216, 1024, true, kIn, false, 0, kNrm, kOut, 0);
    CHECK(p.status == kOk && !p.in_place && p.out_mode == 1 && p.launches == 1 && p.scratch == 0 && p.apply_x == 0 && p.clear_bytes == 0);
    CHECK(p.strips == 19 && p.band_rows == 32 && p.bands == 11 && p.grid_x == (19 * 11 + 3) / 4 && p.words_x == 38);
    CHECK(p.normals_bytes == 16ull * 1024 * 352 * 1216 && p.normals_bytes > (1ull << 32));
    p = plan_depth_normals(352, 1216, 1024, true, kIn, false, 0, kNrm, 0, kCnt);
    CHECK(p.status == kOk && p.out_mode == 0 && p.launches == 2 && p.clear_bytes == 8 * 1024);
    p = plan_depth_normals(352, 1216, 8, true, kIn, false, 0, 0, kOut, 0);
    CHECK(p.status == kOk && p.out_mode == 1 && p.normals_bytes == 0 && p.launches == 1);
    // in place: two launches, the mask of one bit a pixel on the borrowed plane
    p = plan_depth_normals(352, 1216, 8, true, kIn, false, 0, 0, kIn, 0);
    CHECK(p.status == kOk && p.in_place && p.out_mode == 2 && p.launches == 2 && p.apply_x == (352 * 38 + 255) / 256 && p.scratch == 4ull * 8 * 352 * 38);
    p = plan_depth_normals(352, 1216, 8, true, kIn, true, kTab, kNrm, kIn, kCnt);
    CHECK(p.status == kOk && p.in_place && p.launches == 3 && p.clear_bytes == 64);
    // the short-band rule: fewer than 2048 waves halve the band down to 8 rows
    CHECK(plan_depth_normals(352, 1216, 1, true, kIn, false, 0, kNrm, 0, 0).band_rows == 8);
    CHECK(plan_depth_normals(352, 1216, 5, true, kIn, false, 0, kNrm, 0, 0).band_rows == 16);
    CHECK(plan_depth_normals(352, 1216, 640, true, kIn, false, 0, kNrm, 0, 0).band_rows == 32);
}

static void test_grids()
{
    const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 65}, {17, 1}, {5, 3}, {70, 131}, {33, 257}, {64, 64}, {64, 65}, {352, 1216}};
    for (const auto& s : shapes)
        for (int batch : {1, 3, 5})
            for (int in_place : {0, 1}) {
                const NormalsPlan p = plan_depth_normals(s[0], s[1], batch, true, kIn, false, 0, in_place ? 0 : kNrm, in_place ? kIn : kOut, 0);
                CHECK(p.status == kOk);
                CHECK(p.strips * 64 >= (uint32_t)s[1] && (p.strips - 1) * 64 < (uint32_t)s[1]);
                CHECK(p.bands * p.band_rows >= (uint32_t)s[0] && (p.bands - 1) * p.band_rows < (uint32_t)s[0] && p.band_rows >= 8 && p.band_rows <= 32);
                CHECK((size_t)p.grid_x * 4 >= (size_t)p.strips * p.bands && ((size_t)p.grid_x - 1) * 4 < (size_t)p.strips * p.bands);
                // a strip's ballot is two whole mask words, and the mask never exceeds a scratch plane of the call's own size
                CHECK(p.words_x * 32 >= (uint32_t)s[1] && (p.words_x - 1) * 32 < (uint32_t)s[1] && p.words_x <= 2 * p.strips && p.words_x + 1 >= 2 * p.strips);
                CHECK(p.words_x <= (uint32_t)s[1]);
                CHECK(in_place ? (p.scratch == 4 * (size_t)batch * s[0] * p.words_x && (size_t)p.apply_x * 256 >= (size_t)s[0] * p.words_x) : (p.scratch == 0 && p.apply_x == 0));
            }
}

static void test_refusals()
{
    const size_t px = 3 * 8 * 16;
    auto st = [&](uintptr_t z, uintptr_t n, uintptr_t o, uintptr_t c = kCnt, bool ok = true, bool twin = false, uintptr_t t = kTab) {
        return plan_depth_normals(8, 16, 3, ok, z, twin, t, n, o, c).status;
    };
    CHECK(st(kIn, kNrm, kOut) == kOk && st(kIn, kNrm, kIn) == kOk && st(kIn, 0, kOut) == kOk && st(kIn, kNrm, 0) == kOk && st(kIn, kNrm, kOut, 0) == kOk);
    CHECK(st(0, kNrm, kOut) == kInvalid && st(kIn, 0, 0) == kInvalid && st(kIn, kNrm, kOut, kCnt, false) == kInvalid);
    CHECK(st(kIn + 2, kNrm, kOut) == kInvalid && st(kIn, kNrm + 4, kOut) == kInvalid && st(kIn, kNrm + 8, kOut) == kInvalid && st(kIn, kNrm + 16, kOut) == kOk);
    CHECK(st(kIn, kNrm, kOut + 2) == kInvalid && st(kIn, kNrm, kOut, kCnt + 2) == kInvalid && st(kIn + 4, kNrm, kOut + 4, kCnt + 4) == kOk);
    // any overlap but out == depth exactly
    CHECK(st(kIn, kNrm, kIn + 4) == kInvalid && st(kIn, kNrm, kIn + 4 * px - 4) == kInvalid && st(kIn, kNrm, kIn + 4 * px) == kOk);
    CHECK(st(kIn, kIn, kOut) == kInvalid && st(kIn + 16 * px - 16, kIn, kOut) == kInvalid && st(kIn + 16 * px, kIn, kOut) == kOk);
    CHECK(st(kIn, kNrm, kNrm + 16 * px - 4) == kInvalid && st(kIn, kNrm, kNrm + 16 * px) == kOk && st(kIn, kNrm, kNrm) == kInvalid);
    CHECK(st(kIn, kNrm, kOut, kIn) == kInvalid && st(kIn, kNrm, kOut, kNrm + 16 * px - 4) == kInvalid && st(kIn, kNrm, kOut, kOut - 20) == kInvalid &&
          st(kIn, kNrm, kOut, kOut - 24) == kOk && st(kIn, kNrm, kIn, kIn + 8) == kInvalid);
    // the table: 8-byte aligned, clear of every output (it may share bytes with the input: both are only read)
    CHECK(st(kIn, kNrm, kOut, kCnt, true, true) == kOk && st(kIn, kNrm, kOut, kCnt, true, true, 0) == kInvalid && st(kIn, kNrm, kOut, kCnt, true, true, kTab + 4) == kInvalid);
    CHECK(st(kIn, kNrm, kOut, kCnt, true, true, kNrm + 16) == kInvalid && st(kIn, kNrm, kOut, kCnt, true, true, kOut - 88) == kInvalid &&
          st(kIn, kNrm, kOut, kCnt, true, true, kOut - 96) == kOk && st(kIn, kNrm, kOut, kCnt, true, true, kCnt + 16) == kInvalid);
    CHECK(st(kIn, kNrm, kIn, kCnt, true, true, kIn) == kInvalid && st(kIn, kNrm, kOut, kCnt, true, true, kIn) == kOk);
    CHECK(st(kIn, kNrm, kOut, kCnt, true, false, 0) == kOk);                     // a uniform call never looks at it
}

static void test_params()
{
    auto ok = [](float d, float vt, float md) { return normals_params_ok(bits(d), bits(vt), bits(md)); };
    CHECK(ok(0.4f, 0.1f, 100.0f) && ok(0.0f, 0.0625f, 16384.0f) && ok(1024.0f, 5.0f, 5.0f) && ok(1e-40f, 0.1f, 100.0f));
    CHECK(!ok(-0.0f, 0.1f, 100.0f) && !ok(-1.0f, 0.1f, 100.0f) && !ok(1024.5f, 0.1f, 100.0f));
    CHECK(!normals_params_ok(0x7f800000u, bits(0.1f), bits(100.0f)) && !normals_params_ok(0x7fc00000u, bits(0.1f), bits(100.0f)) &&
          !normals_params_ok(0xffc00000u, bits(0.1f), bits(100.0f)));
    CHECK(!ok(0.4f, 0.06f, 100.0f) && !ok(0.4f, 0.1f, 16385.0f) && !ok(0.4f, 0.1f, 0.05f));
    auto in = [](double fx, double fy, double cx, double cy) { return normals_intrinsics_ok(bits(fx), bits(fy), bits(cx), bits(cy)); };
    const double big = 1048576.0, small = 1.0 / 1024.0, nan = __builtin_nan(""), inf = __builtin_inf();
    CHECK(in(721.5, 721.5, 608.0, 176.0) && in(small, -big, big, -big) && in(-small, big, 0.0, -0.0) && in(1.0, 1.0, 1e-300, -1e-300));
    CHECK(!in(0.0, 1.0, 0.0, 0.0) && !in(1.0, -0.0, 0.0, 0.0) && !in(small / 2, 1.0, 0.0, 0.0) && !in(1.0, -2 * big, 0.0, 0.0) && !in(big + 1, 1.0, 0.0, 0.0));
    CHECK(!in(nan, 1.0, 0.0, 0.0) && !in(1.0, inf, 0.0, 0.0) && !in(1.0, 1.0, nan, 0.0) && !in(1.0, 1.0, 0.0, -inf) && !in(1.0, 1.0, big + 1, 0.0) && !in(1.0, 1.0, 0.0, -big - 1));
}

int main()
{
    test_routes();
    test_grids();
    test_refusals();
    test_params();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
