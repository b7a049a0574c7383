// plan_superpixel_planes, planes_max_labels and planes_params_ok (csrc/dcmt_plan_side.h) and the fit of one label from its moments
// (csrc/dcmt_planes.h: the code the device runs, compiled for the host) on a CPU.  Built and run by tests/test_planes.py; prints every
// failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <vector>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kZ = 0x100000000ull, kLab = 0x200000000ull, kOut = 0x300000000ull, kFits = 0x400000000ull;

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static void test_plans()
{
    const size_t plane = 4ull * 352 * 1216 * 8;              // a context of 352 x 1216 x 8
    CHECK(planes_max_labels(plane, 1) == 352 * 1216 * 8 / 24 && planes_max_labels(plane, 8) == 352 * 1216 / 24);
    CHECK(planes_max_labels(96, 1) == 1 && planes_max_labels(95, 1) == 0 && planes_max_labels(~(size_t)0, 1) == 0x00ffffff);
    const int shapes[][2] = {{1, 1}, {1, 70}, {3, 33}, {17, 65}, {40, 130}, {33, 257}, {24, 96}, {352, 1216}};
    for (const auto& s : shapes)
        for (int batch : {1, 3, 8})
            for (int nl : {1, 7, 2304})
                for (bool refit : {false, true}) {
                    const PlanesPlan p = plan_superpixel_planes(s[0], s[1], batch, nl, plane, true, refit, kZ, kLab, kOut, kFits);
                    CHECK(p.status == kOk && p.n == (uint32_t)(s[0] * s[1]));
                    CHECK(p.tiles_x * 64 >= (uint32_t)s[1] && (p.tiles_x - 1) * 64 < (uint32_t)s[1]);
                    CHECK(p.tiles_y * 64 >= (uint32_t)s[0] && (p.tiles_y - 1) * 64 < (uint32_t)s[0]);
                    CHECK(p.sum_grid == p.tiles_x * p.tiles_y);
                    CHECK(p.vec == (p.n % 4 == 0 ? 4 : 1) && (size_t)p.paint_x * 256 * p.vec >= p.n && ((size_t)p.paint_x - 1) * 256 * p.vec < p.n);
                    CHECK(p.records == (size_t)batch * nl && (size_t)p.solve_grid * 256 >= p.records && ((size_t)p.solve_grid - 1) * 256 < p.records);
                    CHECK(p.words == p.records * 24 && p.scratch0 == p.records * 96 && p.scratch0 <= plane && p.scratch1 == 0);
                    CHECK(p.clear_grid >= 1 && p.clear_grid <= 4096 && (p.clear_grid == 4096 || (size_t)p.clear_grid * 256 >= p.words));
                    CHECK(p.refit == refit && p.launches == (refit ? 7 : 4));
                    const PlanesPlan q = plan_superpixel_planes(s[0], s[1], batch, nl, plane, true, refit, kZ, kLab, kOut, 0);
                    CHECK(q.status == kOk && q.scratch1 == q.records * 48 && q.scratch1 <= plane);
                }
    const PlanesPlan k = plan_superpixel_planes(352, 1216, 8, 1340, plane, true, true, kZ, kLab, kZ, 0);     // in place
    CHECK(k.status == kOk && k.tiles_x == 19 && k.tiles_y == 6 && k.sum_grid == 114 && k.vec == 4 && k.paint_x == 418 && k.solve_grid == 42);
    // the wide paint needs 16-byte aligned planes and a frame of a multiple of 4 pixels
    CHECK(plan_superpixel_planes(8, 16, 1, 4, plane, true, false, kZ + 4, kLab, kOut, 0).vec == 1);
    CHECK(plan_superpixel_planes(8, 16, 1, 4, plane, true, false, kZ, kLab + 8, kOut, 0).vec == 1);
    CHECK(plan_superpixel_planes(8, 16, 1, 4, plane, true, false, kZ, kLab, kOut + 12, 0).vec == 1);
    CHECK(plan_superpixel_planes(3, 33, 1, 4, plane, true, false, kZ, kLab, kOut, 0).vec == 1);
    // every 32-bit word of the cleared records: sums and maxima 0, the three minima 2^32 - 1
    for (uint32_t j = 0; j < 48; ++j) CHECK(planes_clear_word(j) == ((j % 24 == 18 || j % 24 == 20 || j % 24 == 22) ? 0xffffffffu : 0u));
}

static void test_refusals()
{
    const size_t plane = 4ull * 150 * 260 * 4;
    const size_t px = 4ull * 3 * 8 * 16;
    auto st = [&](uintptr_t z, uintptr_t l, uintptr_t o, uintptr_t f = kFits, int nl = 4, bool ok = true, int batch = 3) {
        return plan_superpixel_planes(8, 16, batch, nl, plane, ok, false, z, l, o, f).status;
    };
    CHECK(st(kZ, kLab, kOut) == kOk && st(kZ, kLab, kOut, 0) == kOk && st(kZ, kLab, kZ) == kOk);                  // in place
    CHECK(st(0, kLab, kOut) == kInvalid && st(kZ, 0, kOut) == kInvalid && st(kZ, kLab, 0) == kInvalid);
    CHECK(st(kZ + 2, kLab, kOut) == kInvalid && st(kZ, kLab + 2, kOut) == kInvalid && st(kZ, kLab, kOut + 2) == kInvalid && st(kZ, kLab, kOut, kFits + 4) == kInvalid);
    CHECK(st(kZ, kLab, kOut, kFits, 4, false) == kInvalid);
    CHECK(st(kZ, kLab, kOut, kFits, 0) == kInvalid && st(kZ, kLab, kOut, kFits, -1) == kInvalid);
    const int most = planes_max_labels(plane, 3);
    CHECK(most == 150 * 260 * 4 / 24 / 3 && st(kZ, kLab, kOut, kFits, most) == kOk && st(kZ, kLab, kOut, kFits, most + 1) == kInvalid && st(kZ, kLab, kOut, 0, most + 1) == kInvalid);
    // any overlap but out == depth exactly
    CHECK(st(kZ, kLab, kZ + 4) == kInvalid && st(kZ, kLab, kZ + px - 4) == kInvalid && st(kZ, kLab, kZ + px) == kOk && st(kZ + px, kLab, kZ) == kOk);
    CHECK(st(kZ, kZ, kOut) == kInvalid && st(kZ, kZ + px - 4, kOut) == kInvalid && st(kZ, kZ + px, kOut) == kOk);
    CHECK(st(kZ, kLab, kLab) == kInvalid && st(kZ, kLab, kLab + px - 4) == kInvalid && st(kZ, kLab, kLab + px) == kOk);
    const size_t fb = 3 * 4 * 48;
    CHECK(st(kZ, kLab, kOut, kZ) == kInvalid && st(kZ, kLab, kOut, kLab + px - 8) == kInvalid && st(kZ, kLab, kOut, kOut - fb + 8) == kInvalid);
    CHECK(st(kZ, kLab, kOut, kOut - fb) == kOk && st(kZ, kLab, kOut, kZ + px) == kOk);
    // the frame: rows * cols <= 2^21
    const size_t big = ~(size_t)0 >> 8;
    CHECK(plan_superpixel_planes(1024, 2048, 1, 1, big, true, false, kZ, kLab, kOut, 0).status == kOk);
    CHECK(plan_superpixel_planes(1, 1 << 21, 1, 1, big, true, false, kZ, kLab, kOut, 0).status == kOk);
    CHECK(plan_superpixel_planes(1, (1 << 21) + 1, 1, 1, big, true, false, kZ, kLab, kOut, 0).status == kInvalid);
    CHECK(plan_superpixel_planes(1025, 2048, 1, 1, big, true, false, kZ, kLab, kOut, 0).status == kInvalid);
    CHECK(plan_superpixel_planes(16384, 32767, 1, 1, big, true, false, kZ, kLab, kOut, 0).status == kInvalid);
}

static void test_params()
{
    auto ok = [](float vt, float md, int64_t mp, int64_t me, float tol, int64_t keep) { return planes_params_ok(bits(vt), bits(md), mp, me, bits(tol), keep); };
    CHECK(ok(0.1f, 100.0f, 3, 2, 0.0f, 1) && ok(0.0625f, 16384.0f, 3, 1, 0.99f, 0) && ok(5.0f, 5.0f, 100, 50, -0.0f, 1));
    CHECK(!ok(0.06f, 100.0f, 3, 2, 0.0f, 1) && !ok(0.0f, 100.0f, 3, 2, 0.0f, 1) && !ok(-1.0f, 100.0f, 3, 2, 0.0f, 1));
    CHECK(!planes_params_ok(0x7f800000u, bits(100.0f), 3, 2, 0, 1) && !planes_params_ok(0x7fc00000u, bits(100.0f), 3, 2, 0, 1));
    CHECK(!ok(0.1f, 0.05f, 3, 2, 0.0f, 1) && !ok(0.1f, 16385.0f, 3, 2, 0.0f, 1) && !ok(0.1f, -100.0f, 3, 2, 0.0f, 1));
    CHECK(!planes_params_ok(bits(0.1f), 0x7f800000u, 3, 2, 0, 1) && !planes_params_ok(bits(0.1f), 0x7fc00000u, 3, 2, 0, 1));
    CHECK(!ok(0.1f, 100.0f, 2, 2, 0.0f, 1) && !ok(0.1f, 100.0f, 3, 0, 0.0f, 1) && !ok(0.1f, 100.0f, -3, 2, 0.0f, 1));
    CHECK(!ok(0.1f, 100.0f, 3, 2, 1.0f, 1) && !ok(0.1f, 100.0f, 3, 2, -0.1f, 1) && !ok(0.1f, 100.0f, 3, 2, 0.0f, 2) && !ok(0.1f, 100.0f, 3, 2, 0.0f, -1));
    CHECK(!planes_params_ok(bits(0.1f), bits(100.0f), 3, 2, 0x7f800000u, 1) && !planes_params_ok(bits(0.1f), bits(100.0f), 3, 2, 0x7fc00000u, 1));
}

static bool near(double x, double y) { return x - y < 1e-9 && y - x < 1e-9; }      // c = wbar - a ubar - b vbar rounds four times

// the moments of a list of returns
static PlaneMoments moments(const std::vector<uint32_t>& uvw)
{
    PlaneMoments q = {};
    q.umin = q.vmin = q.wmin = 0xffffffffu;
    for (size_t i = 0; i + 2 < uvw.size(); i += 3) {
        const uint64_t u = uvw[i], v = uvw[i + 1], w = uvw[i + 2];
        q.n += 1; q.su += u; q.sv += v; q.suu += u * u; q.suv += u * v; q.svv += v * v; q.sw += w; q.suw += u * w; q.svw += v * w;
        q.umin = u < q.umin ? (uint32_t)u : q.umin; q.umax = u > q.umax ? (uint32_t)u : q.umax;
        q.vmin = v < q.vmin ? (uint32_t)v : q.vmin; q.vmax = v > q.vmax ? (uint32_t)v : q.vmax;
        q.wmin = w < q.wmin ? (uint32_t)w : q.wmin; q.wmax = w > q.wmax ? (uint32_t)w : q.wmax;
    }
    return q;
}

static void test_fit()
{
    // three returns exactly on w = 3 u + 5 v + 1000: Cuu = 3 * 4 - 2 * 2 = 8, Cuv = -4, Cvv = 8, D = 48, Cuw = 4, Cvw = 28: a and b come out exact
    PlaneFit f = planes_fit(moments({0, 0, 1000, 2, 0, 1006, 0, 2, 1010}), 3, 2);
    CHECK(f.kind == kPlanesPlane && f.a == 3.0 && f.b == 5.0 && near(f.c, 1000.0) && f.seen == 3 && f.used == 3 && f.wmin == 1000 && f.wmax == 1010);
    CHECK(near(planes_eval(f.a, f.b, f.c, 1200, 300), 6100.0));
    // the same plane far from the origin: the centred system does not care
    f = planes_fit(moments({1200, 300, 6101, 1202, 300, 6107, 1200, 302, 6111}), 3, 2);
    CHECK(f.kind == kPlanesPlane && f.a == 3.0 && f.b == 5.0 && near(f.c, 1001.0));
    // collinear returns (D == 0, exactly), one row under min_extent = 2, too few points: the mean
    f = planes_fit(moments({0, 0, 1000, 1, 1, 1001, 2, 2, 1005, 5, 5, 1006}), 3, 2);
    CHECK(f.kind == kPlanesConstant && f.a == 0.0 && f.b == 0.0 && f.c == 1003.0 && f.seen == 4 && f.wmin == 1000 && f.wmax == 1006);
    f = planes_fit(moments({0, 4, 10, 5, 4, 20, 9, 4, 30}), 3, 2);
    CHECK(f.kind == kPlanesConstant && f.c == 20.0);
    f = planes_fit(moments({0, 4, 10, 5, 4, 20, 9, 4, 30}), 3, 1);           // extent passes, the determinant does not
    CHECK(f.kind == kPlanesConstant && f.c == 20.0);
    f = planes_fit(moments({0, 0, 10, 5, 1, 20, 1, 7, 31}), 4, 2);
    CHECK(f.kind == kPlanesConstant && f.c == planes_div(61.0, 3.0));
    f = planes_fit(moments({}), 3, 2);
    CHECK(f.kind == kPlanesNone && f.a == 0.0 && f.c == 0.0 && f.seen == 0 && f.wmin == 0 && f.wmax == 0);
    // f64 of a 128-bit integer: nearest, ties to even, across 2^64
    typedef __int128 I;
    const I one = 1;
    CHECK(planes_f64(0) == 0.0 && planes_f64(-5) == -5.0 && planes_f64((one << 53) + 1) == 9007199254740992.0 && planes_f64((one << 53) + 3) == 9007199254740996.0);
    CHECK(planes_f64((one << 100) + (one << 47)) == 0x1p100 && planes_f64((one << 100) + (one << 47) + 1) == 0x1.0000000000001p100);
    CHECK(planes_f64((one << 100) + 3 * (one << 47)) == 0x1.0000000000002p100 && planes_f64(-((one << 100) + (one << 47) + 1)) == -0x1.0000000000001p100);
    CHECK(planes_f64((one << 64) - 1) == 0x1p64 && planes_f64(one << 64) == 0x1p64 && planes_f64((one << 64) + (one << 12) + 1) == 0x1.0000000000001p64);
    CHECK(planes_f64((one << 126) + (one << 73) - 1) == 0x1p126 && planes_f64(((one << 53) - 1) << 70) == 0x1.fffffffffffffp122);
    // a whole frame of 1024 x 2048 returns of one label at the largest code: the terms pass 2^64 and stay exact
    PlaneMoments q = {};
    const uint64_t n = 1ull << 21, C = 2048, R = 1024, w = 1ull << 20;
    q.n = n; q.su = R * (C * (C - 1) / 2); q.sv = C * (R * (R - 1) / 2);
    q.suu = R * ((C - 1) * C * (2 * C - 1) / 6); q.svv = C * ((R - 1) * R * (2 * R - 1) / 6); q.suv = (C * (C - 1) / 2) * (R * (R - 1) / 2);
    q.sw = n * w; q.suw = q.su * w; q.svw = q.sv * w;
    q.umin = 0; q.umax = 2047; q.vmin = 0; q.vmax = 1023; q.wmin = q.wmax = (uint32_t)w;
    f = planes_fit(q, 3, 2);
    CHECK(f.kind == kPlanesPlane && f.a == 0.0 && f.b == 0.0 && f.c == 1048576.0);
}

int main()
{
    test_plans();
    test_refusals();
    test_params();
    test_fit();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
