// plan_sparse_occlusion, occlusion_params_ok and occlusion_scale_ok (csrc/dcmt_plan_side.h) on hand-worked cases, on a CPU.  Built and
// run by tests/test_occlusion.py; prints every failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kIn = 0x100000000ull, kOut = 0x300000000ull, kRem = 0x500000000ull;

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static void test_routes()
{
    // out of place: one launch, no scratch; with removed one more
    OcclusionPlan p = plan_sparse_occlusion(352, 1216, 8, 4, true, 3, 6, kIn, kOut, 0);
    CHECK(p.status == kOk && !p.in_place && p.launches == 1 && p.scratch == 0 && p.apply_x == 0 && p.clear_bytes == 0);
    CHECK(p.tiles_x == 19 && p.tiles_y == 6 && p.grid == 114 && p.words_x == 38 && p.frame_words == 352 * 38);
    CHECK(p.lds_bytes == 4u * (64 + 12) * (64 + 6) && p.plane_bytes == 4ull * 8 * 352 * 1216);
    p = plan_sparse_occlusion(352, 1216, 8, 4, true, 3, 6, kIn, kOut, kRem);
    CHECK(p.status == kOk && !p.in_place && p.launches == 2 && p.clear_bytes == 32 && p.scratch == 0);
    // in place: two launches, the mask of one bit a pixel on the borrowed plane; with removed one more
    p = plan_sparse_occlusion(352, 1216, 8, 4, true, 3, 6, kIn, kIn, 0);
    CHECK(p.status == kOk && p.in_place && p.launches == 2 && p.grid == 114 && p.apply_x == (352 * 38 + 255) / 256 && p.scratch == 4ull * 8 * 352 * 38);
    p = plan_sparse_occlusion(352, 1216, 8, 4, true, 3, 6, kIn, kIn, kRem);
    CHECK(p.status == kOk && p.in_place && p.launches == 3 && p.clear_bytes == 32);
    // the payload: the same grids, half the bytes
    p = plan_sparse_occlusion(352, 1216, 8, 2, true, 3, 6, kIn, kIn, kRem);
    CHECK(p.status == kOk && p.in_place && p.launches == 3 && p.grid == 114 && p.words_x == 38 && p.plane_bytes == 2ull * 8 * 352 * 1216);
    // the LDS at the largest radii: 96 rows of 80 codes, 30 KiB; at none, the tile itself
    CHECK(occl_lds_bytes(8, 16) == 4u * 96 * 80 && occl_lds_bytes(8, 16) == 30720 && occl_lds_bytes(0, 0) == 4u * 64 * 64);
    CHECK(plan_sparse_occlusion(64, 64, 1, 4, true, 8, 16, kIn, kOut, 0).lds_bytes == 30720);
}

static void test_grids()
{
    // partial tiles in both directions, frames smaller than the window
    const int shapes[][2] = {{1, 1}, {1, 65}, {17, 1}, {5, 3}, {33, 130}, {65, 129}, {64, 64}, {64, 65}, {128, 32}, {352, 1216}};
    for (const auto& s : shapes)
        for (int batch : {1, 3, 5})
            for (int in_place : {0, 1}) {
                const OcclusionPlan p = plan_sparse_occlusion(s[0], s[1], batch, 4, true, 8, 16, kIn, in_place ? kIn : kOut, 0);
                CHECK(p.status == kOk);
                CHECK(p.tiles_x * 64 >= (uint32_t)s[1] && (p.tiles_x - 1) * 64 < (uint32_t)s[1]);
                CHECK(p.tiles_y * 64 >= (uint32_t)s[0] && (p.tiles_y - 1) * 64 < (uint32_t)s[0]);
                CHECK(p.grid == p.tiles_x * p.tiles_y);
                CHECK(p.words_x * 32 >= (uint32_t)s[1] && (p.words_x - 1) * 32 < (uint32_t)s[1] && p.words_x <= 2 * p.tiles_x && p.words_x + 1 >= 2 * p.tiles_x);
                CHECK(p.frame_words == (size_t)s[0] * p.words_x);
                // the mask never exceeds a scratch plane of the call's own size: words_x <= cols
                CHECK(4 * (size_t)batch * p.frame_words <= 4 * (size_t)batch * s[0] * s[1]);
                CHECK(in_place ? (p.scratch == 4 * (size_t)batch * p.frame_words && (size_t)p.apply_x * 256 >= p.frame_words && ((size_t)p.apply_x - 1) * 256 < p.frame_words)
                               : (p.scratch == 0 && p.apply_x == 0));
            }
    OcclusionPlan p = plan_sparse_occlusion(5, 3, 1, 4, true, 3, 6, kIn, kIn, 0);          // rows < ry, cols < rx: one tile, one word a row
    CHECK(p.status == kOk && p.grid == 1 && p.words_x == 1 && p.frame_words == 5 && p.apply_x == 1 && p.scratch == 20);
    p = plan_sparse_occlusion(65, 129, 1, 4, true, 3, 6, kIn, kIn, 0);
    CHECK(p.tiles_x == 3 && p.tiles_y == 2 && p.grid == 6 && p.words_x == 5 && p.frame_words == 325 && p.apply_x == 2);
    p = plan_sparse_occlusion(1, 65, 1, 2, true, 0, 0, kIn, kOut, 0);
    CHECK(p.tiles_x == 2 && p.tiles_y == 1 && p.words_x == 3 && p.lds_bytes == 16384);
    // a batch beyond 2^32 bytes: what the kernels' 64-bit offsets span, and the mask beside it
    p = plan_sparse_occlusion(352, 1216, 2600, 4, true, 3, 6, kIn, kIn, kRem);
    CHECK(p.status == kOk && p.plane_bytes == 4ull * 2600 * 352 * 1216 && p.plane_bytes > (1ull << 32) && p.scratch == 4ull * 2600 * 352 * 38 && p.clear_bytes == 4 * 2600);
    p = plan_sparse_occlusion(4096, 8192, 40, 4, true, 3, 6, kIn, kOut, 0);
    CHECK(p.status == kOk && p.plane_bytes == 4ull * 40 * 4096 * 8192 && p.plane_bytes > (1ull << 32) && p.grid == 64 * 128 && p.frame_words == 4096ull * 256);
}

static void test_refusals()
{
    const size_t px = 3 * 8 * 16;
    auto st = [&](uintptr_t z, uintptr_t o, uintptr_t rem = kRem, int elem = 4, bool ok = true) {
        return plan_sparse_occlusion(8, 16, 3, elem, ok, 3, 6, z, o, rem).status;
    };
    CHECK(st(kIn, kOut) == kOk && st(kIn, kIn) == kOk && st(kIn, kOut, 0) == kOk);
    CHECK(st(0, kOut) == kInvalid && st(kIn, 0) == kInvalid && st(kIn, kOut, kRem, 4, false) == kInvalid && st(kIn, kOut, kRem, 3) == kInvalid);
    // aligned to the element: 4 bytes for f32, 2 for the payload; removed to 4
    CHECK(st(kIn + 2, kOut) == kInvalid && st(kIn, kOut + 2) == kInvalid && st(kIn + 4, kOut + 4) == kOk && st(kIn, kOut, kRem + 2) == kInvalid);
    CHECK(st(kIn + 2, kOut + 2, kRem, 2) == kOk && st(kIn + 1, kOut, kRem, 2) == kInvalid && st(kIn, kOut + 1, kRem, 2) == kInvalid && st(kIn, kOut, kRem + 2, 2) == kInvalid);
    // any overlap but out == sparse exactly
    CHECK(st(kIn, kIn + 4) == kInvalid && st(kIn, kIn + 4 * px - 4) == kInvalid && st(kIn, kIn + 4 * px) == kOk && st(kIn + 4 * px, kIn) == kOk);
    CHECK(st(kIn, kIn + 2 * px - 2, kRem, 2) == kInvalid && st(kIn, kIn + 2 * px, kRem, 2) == kOk);
    CHECK(st(kIn, kOut, kIn) == kInvalid && st(kIn, kOut, kIn + 4 * px - 4) == kInvalid && st(kIn, kOut, kIn + 4 * px) == kOk);
    CHECK(st(kIn, kOut, kOut) == kInvalid && st(kIn, kOut, kOut - 8) == kInvalid && st(kIn, kOut, kOut - 12) == kOk && st(kIn, kIn, kIn + 8) == kInvalid);
}

static void test_params()
{
    auto ok = [](int64_t rx, int64_t ry, int64_t tol, float vt, float md) { return occlusion_params_ok(rx, ry, tol, bits(vt), bits(md)); };
    CHECK(ok(3, 6, 655, 0.1f, 100.0f) && ok(0, 0, 0, 0.0625f, 16384.0f) && ok(8, 16, 1 << 20, 5.0f, 5.0f));
    CHECK(!ok(-1, 6, 655, 0.1f, 100.0f) && !ok(9, 6, 655, 0.1f, 100.0f) && !ok(3, -1, 655, 0.1f, 100.0f) && !ok(3, 17, 655, 0.1f, 100.0f));
    CHECK(!ok(3, 6, -1, 0.1f, 100.0f) && !ok(3, 6, (1 << 20) + 1, 0.1f, 100.0f) && !ok(1ll << 32, 6, 655, 0.1f, 100.0f));
    CHECK(!ok(3, 6, 655, 0.06f, 100.0f) && !ok(3, 6, 655, 0.0f, 100.0f) && !ok(3, 6, 655, -1.0f, 100.0f) && !ok(3, 6, 655, -0.0f, 100.0f));
    CHECK(!occlusion_params_ok(3, 6, 655, 0x7f800000u, bits(100.0f)) && !occlusion_params_ok(3, 6, 655, 0x7fc00000u, bits(100.0f)));
    CHECK(!ok(3, 6, 655, 0.1f, 0.05f) && !ok(3, 6, 655, 0.1f, 16385.0f) && !ok(3, 6, 655, 0.1f, -100.0f));
    CHECK(!occlusion_params_ok(3, 6, 655, bits(0.1f), 0x7f800000u) && !occlusion_params_ok(3, 6, 655, bits(0.1f), 0x7fc00000u) && !occlusion_params_ok(3, 6, 655, bits(0.1f), 0xff800000u));
    CHECK(occlusion_scale_ok(bits(1.0f / 256.0f)) && occlusion_scale_ok(bits(1e-40f)) && occlusion_scale_ok(bits(3e38f)));
    CHECK(!occlusion_scale_ok(bits(0.0f)) && !occlusion_scale_ok(bits(-0.0f)) && !occlusion_scale_ok(bits(-1.0f)) && !occlusion_scale_ok(0x7f800000u) && !occlusion_scale_ok(0x7fc00000u));
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
