// plan_joint_bilateral and joint_params_ok (csrc/dcmt_plan_side.h) on hand-worked cases, on a CPU.  Built and run by
// tests/test_joint.py; prints every failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kDepth = 0x100000000ull, kGuide = 0x300000000ull, kTab = 0x500000000ull, kOut = 0x700000000ull, kCnt = 0x900000000ull;

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static const uint32_t kLo = bits(0.1f), kHi = bits(100.0f);

static JointPlan jp(int rows, int cols, int batch, int ch, int R, uintptr_t counts = 0)
{
    return plan_joint_bilateral(rows, cols, batch, ch, R, 1u, 1u, kLo, kHi, kDepth, kGuide, kTab, kOut, counts);
}

static void test_grids()
{
    // one launch, one more with the counts; the dynamic LDS is the tile with its halo, 8 bytes a pixel, rows 82 pixels apart
    JointPlan p = jp(352, 1216, 8, 1, 9);
    CHECK(p.status == kOk && p.launches == 1 && p.clear_bytes == 0 && p.tiles_x == 19 && p.tiles_y == 22 && p.grid == 418);
    CHECK(p.lds_bytes == 8u * 82 * 34 && p.lds_bytes == 22304 && kJointTableLds == 1152 && p.plane_bytes == 4ull * 8 * 352 * 1216 && p.guide_bytes == 8ull * 352 * 1216);
    p = jp(352, 1216, 8, 3, 1, kCnt);
    CHECK(p.status == kOk && p.launches == 2 && p.clear_bytes == 64 && p.grid == 418 && p.lds_bytes == 8u * 82 * 18 && p.guide_bytes == 24ull * 352 * 1216);
    p = jp(1, 1, 1, 1, 1);
    CHECK(p.status == kOk && p.tiles_x == 1 && p.tiles_y == 1 && p.grid == 1 && p.lds_bytes == 8u * 82 * 18);
    p = jp(1, 1, 1, 3, 9, kCnt);
    CHECK(p.status == kOk && p.grid == 1 && p.lds_bytes == 22304 && p.clear_bytes == 8 && p.launches == 2);
    for (int R = 1; R <= 9; ++R) {
        CHECK(joint_lds_bytes(R) == 8u * 82 * (16 + 2 * R) && joint_lds_bytes(R) + kJointTableLds <= 65536 && kJointPitch == 82);
        CHECK(jp(33, 130, 3, 1, R).lds_bytes == joint_lds_bytes(R));
    }
    const int shapes[][2] = {{1, 1}, {1, 65}, {17, 1}, {5, 3}, {33, 130}, {65, 129}, {16, 64}, {17, 65}, {352, 1216}};
    for (const auto& s : shapes)
        for (int batch : {1, 3, 5}) {
            p = jp(s[0], s[1], batch, 3, 9, kCnt);
            CHECK(p.status == kOk && p.tiles_x * 64 >= (uint32_t)s[1] && (p.tiles_x - 1) * 64 < (uint32_t)s[1]);
            CHECK(p.tiles_y * 16 >= (uint32_t)s[0] && (p.tiles_y - 1) * 16 < (uint32_t)s[0] && p.grid == p.tiles_x * p.tiles_y);
            CHECK(p.clear_bytes == 8u * (size_t)batch);
        }
    // 65535 frames, the most a grid's second dimension takes
    p = jp(8, 16, 65535, 1, 9, kCnt);
    CHECK(p.status == kOk && p.grid == 1 && p.clear_bytes == 8 * 65535 && p.plane_bytes == 4ull * 65535 * 128);
    // a batch whose plane passes 2^32 bytes: what the kernel's 64-bit offsets span
    p = plan_joint_bilateral(352, 1216, 2600, 3, 9, 3u, 1u, kLo, kHi, kDepth, 0x2000000000ull, kTab, 0x4000000000ull, kCnt);
    CHECK(p.status == kOk && p.plane_bytes == 4ull * 2600 * 352 * 1216 && p.plane_bytes > (1ull << 32) && p.guide_bytes == 3ull * 2600 * 352 * 1216 &&
          p.guide_bytes > (1ull << 31) && p.clear_bytes == 8 * 2600 && p.grid == 418);
}

static void test_refusals()
{
    struct A { uintptr_t z = kDepth, g = kGuide, t = kTab, o = kOut, n = kCnt; int ch = 1; int64_t R = 9; uint32_t flags = 1, mw = 1, lo = kLo, hi = kHi; };
    auto st = [&](const A& a) { return plan_joint_bilateral(8, 16, 3, a.ch, a.R, a.flags, a.mw, a.lo, a.hi, a.z, a.g, a.t, a.o, a.n).status; };
    auto with = [](void (*f)(A&)) { A a; f(a); return a; };
    const size_t px = 3 * 8 * 16;
    CHECK(px == 384 && st(A()) == kOk && st(with([](A& a) { a.n = 0; })) == kOk && st(with([](A& a) { a.ch = 3; })) == kOk);
    // null pointers
    CHECK(st(with([](A& a) { a.z = 0; })) == kInvalid && st(with([](A& a) { a.g = 0; })) == kInvalid && st(with([](A& a) { a.t = 0; })) == kInvalid);
    CHECK(st(with([](A& a) { a.o = 0; })) == kInvalid);
    // channels other than 1 or 3
    for (int ch : {0, 2, 4, -1}) { A a; a.ch = ch; CHECK(st(a) == kInvalid); }
    // radius outside 1..9
    for (int64_t R : {0ll, -1ll, 10ll, 255ll, 1ll << 32, (1ll << 32) + 9}) { A a; a.R = R; CHECK(st(a) == kInvalid); }
    for (int64_t R = 1; R <= 9; ++R) { A a; a.R = R; CHECK(st(a) == kOk); }
    // no flag set, a flag that does not exist; each combination that does
    CHECK(st(with([](A& a) { a.flags = 0; })) == kInvalid && st(with([](A& a) { a.flags = 4; })) == kInvalid && st(with([](A& a) { a.flags = 5; })) == kInvalid);
    CHECK(st(with([](A& a) { a.flags = 2; })) == kOk && st(with([](A& a) { a.flags = 3; })) == kOk);
    // min_weight 0
    CHECK(st(with([](A& a) { a.mw = 0; })) == kInvalid && st(with([](A& a) { a.mw = 0xffffffffu; })) == kOk);
    // the thresholds: the support call's refused ranges
    CHECK(st(with([](A& a) { a.lo = bits(0.06f); })) == kInvalid && st(with([](A& a) { a.lo = bits(0.0f); })) == kInvalid);
    CHECK(st(with([](A& a) { a.lo = bits(-1.0f); })) == kInvalid && st(with([](A& a) { a.lo = 0x7f800000u; })) == kInvalid && st(with([](A& a) { a.lo = 0x7fc00000u; })) == kInvalid);
    CHECK(st(with([](A& a) { a.hi = bits(0.05f); })) == kInvalid && st(with([](A& a) { a.hi = bits(16385.0f); })) == kInvalid);
    CHECK(st(with([](A& a) { a.hi = 0x7f800000u; })) == kInvalid && st(with([](A& a) { a.hi = 0x7fc00000u; })) == kInvalid && st(with([](A& a) { a.hi = bits(-100.0f); })) == kInvalid);
    CHECK(st(with([](A& a) { a.lo = bits(0.0625f); a.hi = bits(16384.0f); })) == kOk && st(with([](A& a) { a.lo = bits(5.0f); a.hi = bits(5.0f); })) == kOk);
    for (float vt : {0.05f, 0.0625f, 0.1f, 200.0f})
        for (float md : {0.05f, 100.0f, 16384.0f, 16385.0f})
            CHECK(joint_params_ok(9, 1u, 1u, bits(vt), bits(md)) == support_params_ok(9, bits(vt), bits(md)));
    // alignment: depth, out and counts to 4 bytes, the tables to 2; the guide to nothing
    CHECK(st(with([](A& a) { a.z += 2; })) == kInvalid && st(with([](A& a) { a.z += 1; })) == kInvalid && st(with([](A& a) { a.z += 4; })) == kOk);
    CHECK(st(with([](A& a) { a.o += 2; })) == kInvalid && st(with([](A& a) { a.o += 4; })) == kOk && st(with([](A& a) { a.n += 2; })) == kInvalid);
    CHECK(st(with([](A& a) { a.n += 4; })) == kOk && st(with([](A& a) { a.t += 1; })) == kInvalid && st(with([](A& a) { a.t += 2; })) == kOk);
    CHECK(st(with([](A& a) { a.g += 1; })) == kOk && st(with([](A& a) { a.g += 3; a.ch = 3; })) == kOk);
    // every pair of the five buffers, at the first and at the last byte: depth 1536 B, guide 384 B (1152 with three channels), the
    // tables 1792 B, out 1536 B, the counts 24 B
    CHECK(st(with([](A& a) { a.o = a.z; })) == kInvalid && st(with([](A& a) { a.o = a.z + 4; })) == kInvalid && st(with([](A& a) { a.o = a.z + 1532; })) == kInvalid);
    CHECK(st(with([](A& a) { a.o = a.z + 1536; })) == kOk && st(with([](A& a) { a.o = a.z - 1536; })) == kOk && st(with([](A& a) { a.o = a.z - 1532; })) == kInvalid);
    CHECK(st(with([](A& a) { a.g = a.z; })) == kInvalid && st(with([](A& a) { a.g = a.z + 1535; })) == kInvalid && st(with([](A& a) { a.g = a.z + 1536; })) == kOk);
    CHECK(st(with([](A& a) { a.g = a.z - 383; })) == kInvalid && st(with([](A& a) { a.g = a.z - 384; })) == kOk && st(with([](A& a) { a.g = a.z - 384; a.ch = 3; })) == kInvalid);
    CHECK(st(with([](A& a) { a.g = a.z - 1152; a.ch = 3; })) == kOk);
    CHECK(st(with([](A& a) { a.t = a.z; })) == kInvalid && st(with([](A& a) { a.t = a.z + 1534; })) == kInvalid && st(with([](A& a) { a.t = a.z + 1536; })) == kOk);
    CHECK(st(with([](A& a) { a.t = a.z - 1790; })) == kInvalid && st(with([](A& a) { a.t = a.z - 1792; })) == kOk);
    CHECK(st(with([](A& a) { a.n = a.z; })) == kInvalid && st(with([](A& a) { a.n = a.z + 1532; })) == kInvalid && st(with([](A& a) { a.n = a.z + 1536; })) == kOk);
    CHECK(st(with([](A& a) { a.n = a.z - 20; })) == kInvalid && st(with([](A& a) { a.n = a.z - 24; })) == kOk);
    CHECK(st(with([](A& a) { a.t = a.g; })) == kInvalid && st(with([](A& a) { a.t = a.g + 382; })) == kInvalid && st(with([](A& a) { a.t = a.g + 384; })) == kOk);
    CHECK(st(with([](A& a) { a.o = a.g; })) == kInvalid && st(with([](A& a) { a.o = a.g + 380; })) == kInvalid && st(with([](A& a) { a.o = a.g + 384; })) == kOk);
    CHECK(st(with([](A& a) { a.o = a.g + 384; a.ch = 3; })) == kInvalid && st(with([](A& a) { a.o = a.g + 1152; a.ch = 3; })) == kOk);
    CHECK(st(with([](A& a) { a.n = a.g; })) == kInvalid && st(with([](A& a) { a.n = a.g + 380; })) == kInvalid && st(with([](A& a) { a.n = a.g + 384; })) == kOk);
    CHECK(st(with([](A& a) { a.o = a.t; })) == kInvalid && st(with([](A& a) { a.o = a.t + 1788; })) == kInvalid && st(with([](A& a) { a.o = a.t + 1792; })) == kOk);
    CHECK(st(with([](A& a) { a.n = a.t; })) == kInvalid && st(with([](A& a) { a.n = a.t + 1788; })) == kInvalid && st(with([](A& a) { a.n = a.t + 1792; })) == kOk);
    CHECK(st(with([](A& a) { a.n = a.o; })) == kInvalid && st(with([](A& a) { a.n = a.o + 1532; })) == kInvalid && st(with([](A& a) { a.n = a.o + 1536; })) == kOk);
    CHECK(st(with([](A& a) { a.n = a.o - 20; })) == kInvalid && st(with([](A& a) { a.n = a.o - 24; })) == kOk);
    // counts that are not given overlap nothing
    CHECK(st(with([](A& a) { a.n = 0; a.o = a.z + 1536; })) == kOk);
}

static void test_params()
{
    CHECK(joint_params_ok(6, 1u, 1u, kLo, kHi) && joint_params_ok(1, 2u, 5000u, kLo, kHi) && joint_params_ok(9, 3u, 0xffffffffu, kLo, kHi));
    CHECK(!joint_params_ok(0, 1u, 1u, kLo, kHi) && !joint_params_ok(10, 1u, 1u, kLo, kHi) && !joint_params_ok(6, 0u, 1u, kLo, kHi));
    CHECK(!joint_params_ok(6, 8u, 1u, kLo, kHi) && !joint_params_ok(6, 1u, 0u, kLo, kHi));
    // why R stops at 9: the disc's taps at the largest weight stay below 2^24, and one more radius does not
    auto taps = [](int R) { int n = 0; for (int dy = -R; dy <= R; ++dy) for (int dx = -R; dx <= R; ++dx) n += dy * dy + dx * dx <= R * R; return n; };
    CHECK(taps(9) == 253 && taps(kJointMaxRadius) * 65025 == 16451325 && taps(kJointMaxRadius) * 65025 < (1 << 24) && taps(10) * 65025 > (1 << 24));
    CHECK(kJointMaxRadius * kJointMaxRadius < kJointSpace && 3 * 255 < kJointGuide && kJointGuide < kJointGuideLds);
    CHECK(2 * (kJointSpace + kJointGuide) == 1792);                     // sizeof(dcmt_joint_tables)
}

int main()
{
    test_grids();
    test_refusals();
    test_params();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
