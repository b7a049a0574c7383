// plan_bgr_convert (csrc/dcmt_plan_side.h), the launch plan of dcmt_bgr_convert_dev, on a CPU: the buffer checks, the segments at
// the 2^31 cap, the aligned / unaligned choice per pointer, the passes per workgroup.  Built and run by tests/test_bgr_convert.py;
// prints every failed check and returns their number.
#include <algorithm>
#include <cstdio>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

constexpr uintptr_t kBgr = 0x100000000ull, kLab = 0x900000000ull, kGray = 0x1100000000ull;      // 16-byte aligned, far apart
constexpr uint64_t k2p31 = 0x80000000ull;
constexpr size_t kKitti = 352u * 1216u;

// what holds for every plan that is accepted: the segments tile the run in order, each fits 32-bit pixel indices with the last
// workgroup's overhang, each starts at a multiple of 4 pixels, and the grid covers it exactly
static BgrPlan checked(size_t px, uintptr_t bgr, uintptr_t lab, uintptr_t gray)
{
    const BgrPlan p = plan_bgr_convert(px, bgr, lab, gray);
    CHECK(p.status == kOk);
    if (p.status != kOk) return p;
    CHECK(p.px == px && p.count >= 1 && p.passes >= 1 && p.passes <= kBgrMaxPasses && (p.passes & (p.passes - 1)) == 0);
    CHECK(p.share() == p.passes * kBgrPxPerPass);
    CHECK(p.passes == 1 || px / p.share() >= 512);                                   // longer shares only where the GPU stays full
    CHECK(p.passes == kBgrMaxPasses || px / (2 * (size_t)p.share()) < 512);
    CHECK(p.aligned == (bgr % 4 == 0 && lab % 4 == 0 && gray % 4 == 0));
    size_t next = 0;
    for (size_t i = 0; i < p.count; ++i) {
        const BgrSegment s = p.segment(i);
        CHECK(s.first == next && s.total >= 1 && s.first % 4 == 0);
        CHECK(i + 1 == p.count || s.total == kBgrSegPx);
        CHECK((uint64_t)s.total <= kBgrSegPx);
        CHECK((uint64_t)s.grid * p.share() >= s.total && (uint64_t)(s.grid - 1) * p.share() < s.total);
        CHECK((uint64_t)s.grid * p.share() <= k2p31);                                // the kernel's 32-bit p0 + kBgrPxPerPass and 4 * g + i
        CHECK((3 * s.first) % 4 == 0);                                               // bgr / lab bases of the segment: as aligned as the call's
        next = s.first + s.total;
    }
    CHECK(next == px);
    return p;
}

static void test_checks()
{
    const size_t px = 1000;
    CHECK(plan_bgr_convert(px, 0, kLab, kGray).status == kInvalid);                  // no source
    CHECK(plan_bgr_convert(px, kBgr, 0, 0).status == kInvalid);                      // no output
    CHECK(plan_bgr_convert(0, kBgr, kLab, kGray).status == kInvalid);
    checked(px, kBgr, kLab, 0); checked(px, kBgr, 0, kGray); checked(px, kBgr, kLab, kGray);
    checked(px, kBgr, kBgr, 0); checked(px, kBgr, kBgr, kGray);                      // in place
    // lab overlapping bgr anywhere but exactly: by one byte at either end, and wholly inside a larger picture
    CHECK(plan_bgr_convert(px, kBgr, kBgr + 3, 0).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, kBgr - 3, 0).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, kBgr + 3 * px - 1, 0).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, kBgr - 3 * px + 1, 0).status == kInvalid);
    checked(px, kBgr, kBgr + 3 * px, 0); checked(px, kBgr, kBgr - 3 * px, 0);        // touching is not overlapping
    // gray inside, at the ends of and next to bgr
    CHECK(plan_bgr_convert(px, kBgr, 0, kBgr).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, 0, kBgr + px).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, 0, kBgr + 3 * px - 1).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, 0, kBgr - px + 1).status == kInvalid);
    checked(px, kBgr, 0, kBgr + 3 * px); checked(px, kBgr, 0, kBgr - px);
    // gray against lab, also with lab in place
    CHECK(plan_bgr_convert(px, kBgr, kLab, kLab + 5).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, kLab, kLab - px + 1).status == kInvalid);
    CHECK(plan_bgr_convert(px, kBgr, kBgr, kBgr + 5).status == kInvalid);
    checked(px, kBgr, kLab, kLab + 3 * px); checked(px, kBgr, kLab, kLab - px);
}

static void test_alignment()
{
    for (size_t px : {(size_t)1, (size_t)3, (size_t)4096, kKitti})
        for (uintptr_t off = 0; off < 8; ++off) {
            // each of the three pointers decides alone; a pointer that is not wanted (0) never does
            CHECK(checked(px, kBgr + off, kLab, kGray).aligned == (off % 4 == 0));
            CHECK(checked(px, kBgr, kLab + off, kGray).aligned == (off % 4 == 0));
            CHECK(checked(px, kBgr, kLab, kGray + off).aligned == (off % 4 == 0));
            CHECK(checked(px, kBgr + off, kLab, 0).aligned == (off % 4 == 0));
            CHECK(checked(px, kBgr + off, 0, kGray).aligned == (off % 4 == 0));
            CHECK(checked(px, kBgr, kLab + off, 0).aligned == (off % 4 == 0));
            CHECK(checked(px, kBgr, 0, kGray + off).aligned == (off % 4 == 0));
            CHECK(checked(px, kBgr + off, kBgr + off, 0).aligned == (off % 4 == 0));    // in place
        }
}

static void test_shapes()
{
    // 1-pixel frames, alone and as the largest batch
    BgrPlan p = checked(1, kBgr, kLab, kGray);
    CHECK(p.count == 1 && p.passes == 1 && p.segment(0).grid == 1 && p.segment(0).total == 1);
    p = checked(65535, kBgr, kLab, kGray);
    CHECK(p.count == 1 && p.passes == 1 && p.segment(0).grid == 16);
    // around one workgroup's share
    for (size_t px : {(size_t)kBgrPxPerPass - 1, (size_t)kBgrPxPerPass, (size_t)kBgrPxPerPass + 1}) {
        p = checked(px, kBgr, kLab, 0);
        CHECK(p.passes == 1 && p.segment(0).grid == (px > kBgrPxPerPass ? 2u : 1u));
    }
    // passes: one KITTI frame, three of them, the colour cube, 1024 KITTI frames
    CHECK(checked(kKitti, kBgr, kLab, 0).passes == 1 && checked(3 * kKitti, kBgr, kLab, 0).passes == 1);
    CHECK(checked((size_t)512 * 2 * kBgrPxPerPass - 1, kBgr, kLab, 0).passes == 1 && checked((size_t)512 * 2 * kBgrPxPerPass, kBgr, kLab, 0).passes == 2);
    CHECK(checked((size_t)1 << 24, kBgr, kLab, kGray).passes == 4);
    p = checked(1024 * kKitti, kBgr, kLab, kGray);
    CHECK(p.passes == kBgrMaxPasses && p.count == 1 && p.segment(0).grid == (1024 * kKitti + p.share() - 1) / p.share());
}

static void test_segments()
{
    // the cap: one segment up to kBgrSegPx pixels, two from one more
    BgrPlan p = checked(kBgrSegPx, kBgr, kLab, kGray);
    CHECK(p.count == 1 && p.segment(0).total == kBgrSegPx && (uint64_t)p.segment(0).grid * p.share() == kBgrSegPx);
    p = checked((size_t)kBgrSegPx + 1, kBgr, kLab, kGray);
    CHECK(p.count == 2 && p.segment(0).total == kBgrSegPx && p.segment(1).first == kBgrSegPx && p.segment(1).total == 1 && p.segment(1).grid == 1);
    for (uint64_t px : {k2p31 - 1, k2p31, k2p31 + 1}) {
        p = checked((size_t)px, kBgr, kLab, kGray);
        CHECK(p.count == 2 && p.segment(1).total == px - kBgrSegPx);
    }
    // 5018 KITTI frames: the first batch plan_colorize cuts; an odd frame (375 x 1242) in a batch beyond the cap
    p = checked(5018 * kKitti, kBgr, kLab, kGray);
    CHECK(p.count == 2);
    p = checked((size_t)375 * 1242 * 9000, kBgr + 1, kLab + 2, kGray + 3);
    CHECK(p.count == 2 && !p.aligned);
    // the largest call dcmt_create admits: 65535 frames of 0x1ffffff0 pixels (segment() is a closed form: look at the ends)
    const size_t huge = (size_t)65535 * 0x1ffffff0u;
    p = plan_bgr_convert(huge, kBgr, kBgr, kBgr + 3 * huge);
    CHECK(p.status == kOk && p.count == (huge + kBgrSegPx - 1) / kBgrSegPx && p.passes == kBgrMaxPasses);
    const BgrSegment last = p.segment(p.count - 1);
    CHECK(last.first == (p.count - 1) * (size_t)kBgrSegPx && last.first + last.total == huge && last.total >= 1 && last.total <= kBgrSegPx);
    CHECK(p.segment(0).total == kBgrSegPx && p.segment(p.count - 2).total == kBgrSegPx);
}

int main()
{
    static_assert(kBgrPxPerPass == 4u * kBgrGroupsPerLane * kBgrThreads && kBgrSegPx % 4 == 0, "constants");
    test_checks();
    test_alignment();
    test_shapes();
    test_segments();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
