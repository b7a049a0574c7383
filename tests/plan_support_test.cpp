// plan_support_distance and support_params_ok (csrc/dcmt_plan_side.h) on hand-worked cases, on a CPU.  Built and run by
// tests/test_support.py; prints every failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kIn = 0x100000000ull, kDense = 0x300000000ull, kFb = 0x500000000ull, kOut = 0x700000000ull, kD2 = 0x900000000ull,
                       kBey = 0xb00000000ull;

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static void test_routes()
{
    // dist2 alone: two launches, the column distances on half the borrowed plane
    SupportPlan p = plan_support_distance(352, 1216, 8, 4, true, 9, kIn, 0, 0, 0, kD2, 0);
    CHECK(p.status == kOk && !p.in_place && p.ballots && p.launches == 2 && p.clear_bytes == 0);
    CHECK(p.cols_grid == 19 && p.cols_lds == 8u * 352 && p.tiles_x == 5 && p.bands == 88 && p.groups == 22 && p.rows_grid == 110);
    CHECK(p.rows_lds == 4u * 4 * (256 + 18) && p.scratch == 2ull * 8 * 352 * 1216 && p.plane_bytes == 4ull * 8 * 352 * 1216);
    // with beyond one more
    p = plan_support_distance(352, 1216, 8, 4, true, 9, kIn, 0, 0, 0, kD2, kBey);
    CHECK(p.status == kOk && p.launches == 3 && p.clear_bytes == 32);
    // the trust mask out of place, in place, with a fallback, with everything: the same two kernels
    p = plan_support_distance(352, 1216, 8, 4, true, 9, kIn, kDense, 0, kOut, 0, 0);
    CHECK(p.status == kOk && !p.in_place && p.launches == 2 && p.rows_grid == 110);
    p = plan_support_distance(352, 1216, 8, 4, true, 9, kIn, kDense, 0, kDense, 0, 0);
    CHECK(p.status == kOk && p.in_place && p.launches == 2);
    p = plan_support_distance(352, 1216, 8, 4, true, 9, kIn, kDense, kFb, kDense, kD2, kBey);
    CHECK(p.status == kOk && p.in_place && p.launches == 3 && p.clear_bytes == 32);
    // the payload: the same grids and the same scratch (the sparse plane alone changes its element)
    p = plan_support_distance(352, 1216, 8, 2, true, 9, kIn, kDense, kFb, kOut, kD2, kBey);
    CHECK(p.status == kOk && !p.in_place && p.launches == 3 && p.cols_grid == 19 && p.rows_grid == 110 && p.scratch == 2ull * 8 * 352 * 1216);
    // the LDS of the row pass at R = 1, 9, 255: 4 rows of 256 + 2 R squared distances
    CHECK(support_rows_lds_bytes(1) == 4u * 4 * 258 && support_rows_lds_bytes(9) == 4u * 4 * 274 && support_rows_lds_bytes(255) == 4u * 4 * 766);
    CHECK(support_rows_lds_bytes(255) == 12256 && support_rows_lds_bytes(255) <= 65536);
    for (int R : {1, 9, 255}) CHECK(plan_support_distance(64, 64, 1, 4, true, R, kIn, 0, 0, 0, kD2, 0).rows_lds == 16u * (256 + 2 * (uint32_t)R));
    // the LDS of the column pass: 8 bytes a row up to 4096 rows, then the route that reads the plane twice
    p = plan_support_distance(4096, 64, 1, 4, true, 9, kIn, 0, 0, 0, kD2, 0);
    CHECK(p.status == kOk && p.ballots && p.cols_lds == 32768 && p.cols_lds <= 65536);
    p = plan_support_distance(4097, 64, 1, 4, true, 9, kIn, 0, 0, 0, kD2, 0);
    CHECK(p.status == kOk && !p.ballots && p.cols_lds == 0 && p.bands == 1025 && p.groups == 257);
}

static void test_grids()
{
    const int shapes[][2] = {{1, 1}, {1, 65}, {17, 1}, {5, 3}, {33, 130}, {65, 129}, {3, 600}, {300, 70}, {64, 256}, {64, 257}, {352, 1216}};
    for (const auto& s : shapes)
        for (int batch : {1, 3, 5})
            for (int R : {1, 9, 255}) {
                const SupportPlan p = plan_support_distance(s[0], s[1], batch, 4, true, R, kIn, kDense, 0, kOut, kD2, 0);
                CHECK(p.status == kOk);
                CHECK(p.cols_grid * 64 >= (unsigned)s[1] && (p.cols_grid - 1) * 64 < (unsigned)s[1]);
                CHECK(p.tiles_x * 256 >= (uint32_t)s[1] && (p.tiles_x - 1) * 256 < (uint32_t)s[1]);
                CHECK(p.bands * 4 >= (uint32_t)s[0] && (p.bands - 1) * 4 < (uint32_t)s[0]);
                CHECK(p.groups * 4 >= p.bands && (p.groups - 1) * 4 < p.bands);
                CHECK(p.rows_grid == p.tiles_x * p.groups && p.cols_lds == 8u * (uint32_t)s[0]);
                // the scratch never exceeds a borrowed f32 plane of the call's own size
                CHECK(p.scratch == 2 * (size_t)batch * s[0] * s[1] && p.scratch <= 4 * (size_t)batch * s[0] * s[1]);
            }
    SupportPlan p = plan_support_distance(3, 600, 1, 4, true, 255, kIn, 0, 0, 0, kD2, 0);           // both halos clip, three column tiles
    CHECK(p.tiles_x == 3 && p.bands == 1 && p.groups == 1 && p.rows_grid == 3 && p.cols_grid == 10);
    p = plan_support_distance(300, 70, 1, 4, true, 255, kIn, 0, 0, 0, kD2, 0);
    CHECK(p.tiles_x == 1 && p.bands == 75 && p.groups == 19 && p.rows_grid == 19 && p.cols_grid == 2 && p.cols_lds == 2400);
    // 65535 frames, the most a grid's second dimension takes
    p = plan_support_distance(8, 16, 65535, 4, true, 9, kIn, kDense, kFb, kOut, kD2, kBey);
    CHECK(p.status == kOk && p.clear_bytes == 4 * 65535 && p.scratch == 2ull * 65535 * 128 && p.cols_grid == 1 && p.bands == 2 && p.rows_grid == 1);
    // a batch whose plane passes 2^32 bytes: what the kernels' 64-bit offsets span, and the scratch beside it
    p = plan_support_distance(352, 1216, 2600, 4, true, 9, kIn, kDense, 0, kDense, 0, kBey);
    CHECK(p.status == kOk && p.plane_bytes == 4ull * 2600 * 352 * 1216 && p.plane_bytes > (1ull << 32) && p.scratch == 2ull * 2600 * 352 * 1216 && p.clear_bytes == 4 * 2600);
    p = plan_support_distance(4096, 8192, 40, 4, true, 255, kIn, 0, 0, 0, 0x2000000000ull, 0);
    CHECK(p.status == kOk && p.plane_bytes == 4ull * 40 * 4096 * 8192 && p.plane_bytes > (1ull << 32) && p.rows_grid == 32 * 256 && p.cols_grid == 128);
}

static void test_refusals()
{
    const size_t px = 3 * 8 * 16;
    struct A { uintptr_t z = kIn, d = kDense, f = kFb, o = kOut, q = kD2, b = kBey; int elem = 4; bool ok = true; int R = 9; };
    auto st = [&](const A& a) { return plan_support_distance(8, 16, 3, a.elem, a.ok, a.R, a.z, a.d, a.f, a.o, a.q, a.b).status; };
    auto with = [](void (*f)(A&)) { A a; f(a); return a; };
    CHECK(st(A()) == kOk);
    // a null sparse plane, bad parameters, an element that is neither
    CHECK(st(with([](A& a) { a.z = 0; })) == kInvalid && st(with([](A& a) { a.ok = false; })) == kInvalid && st(with([](A& a) { a.elem = 3; })) == kInvalid);
    // neither output; out without dense; fallback without out (with dist2 alone)
    CHECK(st(with([](A& a) { a.o = 0; a.q = 0; a.f = 0; })) == kInvalid);
    CHECK(st(with([](A& a) { a.d = 0; })) == kInvalid && st(with([](A& a) { a.d = 0; a.f = 0; })) == kInvalid);
    CHECK(st(with([](A& a) { a.o = 0; })) == kInvalid && st(with([](A& a) { a.o = 0; a.f = 0; })) == kOk && st(with([](A& a) { a.o = 0; a.f = 0; a.d = 0; a.b = 0; })) == kOk);
    CHECK(st(with([](A& a) { a.q = 0; })) == kOk && st(with([](A& a) { a.q = 0; a.f = 0; a.b = 0; })) == kOk && st(with([](A& a) { a.o = a.d; })) == kOk);
    // aligned to the element: 4 bytes for the f32 planes, 2 for the payload and for dist2; beyond to 4
    CHECK(st(with([](A& a) { a.z += 2; })) == kInvalid && st(with([](A& a) { a.z += 4; })) == kOk && st(with([](A& a) { a.z += 2; a.elem = 2; })) == kOk);
    CHECK(st(with([](A& a) { a.z += 1; a.elem = 2; })) == kInvalid && st(with([](A& a) { a.d += 2; })) == kInvalid && st(with([](A& a) { a.f += 2; })) == kInvalid);
    CHECK(st(with([](A& a) { a.o += 2; })) == kInvalid && st(with([](A& a) { a.q += 1; })) == kInvalid && st(with([](A& a) { a.q += 2; })) == kOk);
    CHECK(st(with([](A& a) { a.b += 2; })) == kInvalid && st(with([](A& a) { a.b += 4; })) == kOk && st(with([](A& a) { a.d += 4; a.o = a.d; })) == kOk);
    // any overlap but out == dense exactly: every pair of the six buffers, at the first and at the last byte
    CHECK(st(with([](A& a) { a.o = a.d + 4; })) == kInvalid && st(with([](A& a) { a.o = a.d + 4 * 384 - 4; })) == kInvalid && st(with([](A& a) { a.o = a.d + 4 * 384; })) == kOk);
    CHECK(px == 384);
    CHECK(st(with([](A& a) { a.d = a.z; })) == kInvalid && st(with([](A& a) { a.f = a.z; })) == kInvalid && st(with([](A& a) { a.o = a.z; })) == kInvalid);
    CHECK(st(with([](A& a) { a.q = a.z; })) == kInvalid && st(with([](A& a) { a.b = a.z; })) == kInvalid && st(with([](A& a) { a.z = a.d + 4 * 384 - 4; })) == kInvalid);
    CHECK(st(with([](A& a) { a.z = a.d + 4 * 384; })) == kOk && st(with([](A& a) { a.z = a.d + 2 * 384 - 2; a.elem = 2; })) == kInvalid);
    CHECK(st(with([](A& a) { a.f = a.d; })) == kInvalid && st(with([](A& a) { a.f = a.o; })) == kInvalid && st(with([](A& a) { a.f = a.d; a.o = a.d; })) == kInvalid);
    CHECK(st(with([](A& a) { a.q = a.d; })) == kInvalid && st(with([](A& a) { a.q = a.f + 4; })) == kInvalid && st(with([](A& a) { a.q = a.o + 4 * 384 - 2; })) == kInvalid);
    CHECK(st(with([](A& a) { a.q = a.o + 4 * 384; })) == kOk && st(with([](A& a) { a.q = a.o - 2 * 384; })) == kOk && st(with([](A& a) { a.q = a.o - 2 * 384 + 2; })) == kInvalid);
    CHECK(st(with([](A& a) { a.b = a.d; })) == kInvalid && st(with([](A& a) { a.b = a.f + 8; })) == kInvalid && st(with([](A& a) { a.b = a.o + 4 * 384 - 4; })) == kInvalid);
    CHECK(st(with([](A& a) { a.b = a.q + 2 * 384 - 4; })) == kInvalid && st(with([](A& a) { a.b = a.q + 2 * 384; })) == kOk && st(with([](A& a) { a.b = a.o - 12; })) == kOk);
    CHECK(st(with([](A& a) { a.b = a.o - 8; })) == kInvalid);
    // a buffer that is not given overlaps nothing
    CHECK(st(with([](A& a) { a.f = 0; a.q = 0; a.b = 0; })) == kOk);
}

static void test_params()
{
    auto ok = [](int64_t R, float vt, float md) { return support_params_ok(R, bits(vt), bits(md)); };
    CHECK(ok(9, 0.1f, 100.0f) && ok(1, 0.0625f, 16384.0f) && ok(255, 5.0f, 5.0f));
    CHECK(!ok(0, 0.1f, 100.0f) && !ok(-1, 0.1f, 100.0f) && !ok(256, 0.1f, 100.0f) && !ok(1ll << 32, 0.1f, 100.0f) && !ok((1ll << 32) + 9, 0.1f, 100.0f));
    CHECK(!ok(9, 0.06f, 100.0f) && !ok(9, 0.0f, 100.0f) && !ok(9, -1.0f, 100.0f) && !ok(9, -0.0f, 100.0f));
    CHECK(!support_params_ok(9, 0x7f800000u, bits(100.0f)) && !support_params_ok(9, 0x7fc00000u, bits(100.0f)));
    CHECK(!ok(9, 0.1f, 0.05f) && !ok(9, 0.1f, 16385.0f) && !ok(9, 0.1f, -100.0f));
    CHECK(!support_params_ok(9, bits(0.1f), 0x7f800000u) && !support_params_ok(9, bits(0.1f), 0x7fc00000u) && !support_params_ok(9, bits(0.1f), 0xff800000u));
    // the same depth bounds as the occlusion filter's
    for (float vt : {0.05f, 0.0625f, 0.1f, 200.0f})
        for (float md : {0.05f, 100.0f, 16384.0f, 16385.0f}) CHECK(ok(9, vt, md) == occlusion_params_ok(3, 6, 655, bits(vt), bits(md)));
    // the marker is never a distance
    CHECK(kSupportMaxRadius * kSupportMaxRadius == 65025 && (uint32_t)(kSupportMaxRadius * kSupportMaxRadius) < kSupportBeyond && kSupportBeyond == 65535u);
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
