// The dispatch of DCMT_FLAG_NO_EXTRAPOLATE (csrc/dcmt_plan.h) on a CPU: route, row bands, grid, output plane and dcmt_last_path of
// a flagged call, and that a call without the flag plans as it did.  Built and run by tests/test_no_extrapolate.py; prints every
// failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dcmt_plan.h"

using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

constexpr int kRows = 352, kCols = 1216;
constexpr uintptr_t kSrc = 0x100000000ull, kDst = 0x900000000ull, kLabels = 0x1100000000ull;

static Call call(int batch, bool flag = true)
{
    Call c;
    c.rows = kRows; c.cols = kCols; c.batch = batch;
    c.src = kSrc; c.dst = kDst;
    c.q16_allowed = true;
    if (flag) c.flags |= kFlagNoExtrapolate;
    return c;
}

static bool is(const Plan& p, const char* path) { return std::strcmp(p.path, path) == 0; }

// every field of two plans, and every byte of their paths (the padding between fields holds nothing)
static bool same(const Plan& a, const Plan& b)
{
    bool eq = true;
#define F(f) eq = eq && a.f == b.f;
    F(route) F(k0kind) F(norm) F(xcd_map) F(out) F(needs_x6q) F(needs_colstat) F(needs_bbox) F(few) F(tile_h) F(tiles_x) F(tiles_y)
    F(u16_convert) F(dump) F(bbox_lds) F(lpair) F(label_pairs) F(label_group) F(label_grid_x) F(table) F(wide) F(pair) F(q16) F(bands)
    F(fb_s) F(pre_strips) F(fill_strips) F(post_strips) F(q_strips) F(pre_grid) F(fill_grid) F(post_grid) F(fp_s_grid) F(fp_q_grid)
    F(fuse_fp) F(filled) F(tail) F(fp_s_launch) F(n_redo) F(bilateral) F(bilateral_invert) F(no_extrapolate) F(local_bands) F(local_strips)
    F(local_grid)
#undef F
    return eq && std::memcmp(a.path, b.path, sizeof a.path) == 0;
}

// every plan of a flagged call from stop_after = MEDIAN5 on: nothing of the fill, the 16-bit form or the table
static Plan checked(const Knobs& k, const Call& c)
{
    const Plan p = plan_call(k, c);
    CHECK(p.no_extrapolate);
    CHECK(p.route == Route::LOCAL || p.route == Route::STAGED);
    CHECK(p.route == route_of(k, c));
    CHECK(!p.q16 && !p.needs_x6q && !p.table && !p.fuse_fp && !p.tail && p.n_redo == 0);
    CHECK(p.needs_colstat == (p.route == Route::STAGED));
    CHECK(p.needs_bbox == (c.input == Input::LABELED && p.route == Route::LOCAL));
    CHECK((std::strstr(p.path, kPathCopy) != nullptr) == (p.out != Out::DST));
    CHECK(std::strstr(p.path, "fill") == nullptr && std::strstr(p.path, "k_fp") == nullptr && std::strstr(p.path, "k_pre_p") == nullptr);
    if (p.route == Route::LOCAL) {
        CHECK(p.local_bands >= 1 && p.local_bands <= c.rows);
        CHECK(p.local_strips == (c.cols + local_vw(c.k0kind) - 1) / local_vw(c.k0kind));
        CHECK(p.local_grid == wave_grid(p.local_strips * p.local_bands, c.batch, p.xcd_map));
    }
    return p;
}
static Plan checked(const Call& c) { return checked(Knobs{}, c); }

static void test_batches()
{
    struct { int batch, bands; unsigned grid; int xcd; } want[] = {
        {1, 22, 171u, 0},       // 31 strips; 2560 / 31 = 83 bands asked, 352 / 16 = 22 allowed; 682 waves
        {2, 22, 341u, 0},
        {3, 22, 512u, 0},       // 2046 waves
        {8, 11, 688u, 1},       // 248 strips: 11 bands; per XCD 341 waves in 86 workgroups
        {1024, 1, 7936u, 1},    // 128 frames x 31 strips per XCD
    };
    for (const auto& w : want) {
        const Plan p = checked(call(w.batch));
        CHECK(p.route == Route::LOCAL && p.local_strips == 31 && p.local_bands == w.bands && p.local_grid == w.grid && p.xcd_map == w.xcd);
        CHECK(p.out == Out::DST && p.k0kind == kK0AsCompiled && !p.norm);
        CHECK(is(p, w.bands > 1 ? "k_local (row bands)" : "k_local"));
    }
    // min_fused_batch and FORCE_FUSED do not apply
    Knobs k;
    k.min_fused_batch = 100;
    CHECK(checked(k, call(1)).route == Route::LOCAL);
    Call c = call(1);
    c.flags |= kFlagForceFused;
    CHECK(same(checked(c), checked(call(1))));
}

static void test_bands_knob()
{
    for (int b : {1, 2, 3, 8, 40}) {
        Knobs k;
        k.local_bands = b;
        const Plan p = checked(k, call(3));
        CHECK(p.local_bands == b && p.local_grid == (3u * 31 * b + 3) / 4);
        CHECK(is(p, b > 1 ? "k_local (row bands)" : "k_local"));
    }
    Knobs k;
    k.local_bands = 1000;                                  // never more bands than rows
    Call c = call(1);
    c.rows = 9; c.cols = 70;
    CHECK(checked(k, c).local_bands == 9);
    CHECK(checked(c).local_bands == 1);                    // 9 / 16 = 0 allowed: one band
}

static void test_shapes_and_inputs()
{
    {
        Call c = call(3);
        c.cols = 1215;                                     // an odd width: the same kernel, one column per lane
        const Plan p = checked(c);
        CHECK(p.route == Route::LOCAL && p.local_strips == 31 && is(p, "k_local (row bands)"));
        c.src += 4;                                        // and any alignment
        CHECK(is(checked(c), "k_local (row bands)"));
    }
    {
        Call c = call(3);
        c.k0kind = kK0Diamond;
        const Plan p = checked(c);
        CHECK(p.route == Route::LOCAL && p.k0kind == kK0Diamond && p.local_strips == 32);      // 1216 / 38
    }
    for (int stop : {kStageMedian5, kStageBlur, kStageFinal}) {
        Call c = call(3);
        c.stop_after = stop;
        CHECK(checked(c).route == Route::LOCAL);
    }
    {
        Call c = call(1024);
        c.input = Input::U16; c.in_scale = 0.00390625f;
        const Plan p = checked(c);
        CHECK(p.route == Route::LOCAL && !p.u16_convert && is(p, "k_local<U16>"));
    }
    {
        Call c = call(1024);
        c.flags |= kFlagNormalize;
        const Plan p = checked(c);
        CHECK(p.route == Route::LOCAL && p.norm && is(p, "k_local<NORM>"));
    }
    {
        Call c = call(3);
        c.input = Input::LABELED; c.labels = kLabels; c.n_labels = 500;
        const Plan p = checked(c);
        CHECK(p.route == Route::LOCAL && p.needs_bbox && p.label_grid_x > 0 && p.out == Out::DST);
        CHECK(is(p, "k_label_bbox + k_label_stage + k_local<START4> (row bands)"));
        c.dst = c.src;                                     // the kernel reads X4 in scratch: no copy
        const Plan q = checked(c);
        CHECK(q.out == Out::DST && is(q, p.path));
        c.n_labels = 0;                                    // no label to run: the staged kernels
        CHECK(checked(c).route == Route::STAGED);
    }
}

static void test_staged()
{
    const char* staged = "k_pre_v1 + k_post_v1 (staged tile kernels)";
    {
        Call c = call(3);
        c.k0kind = -1;                                     // a custom k0
        const Plan p = checked(c);
        CHECK(p.route == Route::STAGED && p.few && p.tile_h == FTH_FEW && p.dump == 0 && p.out == Out::DST && is(p, staged));
        c.dst = c.src + 4;                                 // k_post_v1 writes dst behind the only kernel that reads the frames
        CHECK(checked(c).out == Out::DST && is(checked(c), staged));
    }
    {
        Call c = call(64);
        c.flags |= kFlagForceStaged;
        const Plan p = checked(c);
        CHECK(p.route == Route::STAGED && !p.few && p.tile_h == TH && is(p, staged));
        c.input = Input::U16;
        CHECK(checked(c).u16_convert);
        c.input = Input::LABELED; c.labels = kLabels; c.n_labels = 500;
        CHECK(is(checked(c), "k_pre_labeled_v1 + k_post_v1 (staged tile kernels)") && !checked(c).needs_bbox);
    }
    {
        Call c = call(3);
        c.rows = 7; c.cols = 100;                          // under 8 x 8
        CHECK(checked(c).route == Route::STAGED);
        c.rows = 100; c.cols = 7;
        CHECK(checked(c).route == Route::STAGED);
    }
}

static void test_bilateral()
{
    for (int stop : {kStageBlur, kStageFinal}) {
        Call c = call(3);
        c.gaussian = false; c.bilateral = true; c.stop_after = stop;
        const Plan p = checked(c);
        CHECK(p.route == Route::LOCAL && p.bilateral && p.bilateral_invert == (stop == kStageFinal) && p.out == Out::DST);
        CHECK(is(p, "k_local (row bands) + bilateral5"));
        c.dst = c.src;                                     // the chain writes the median plane, k_bilateral5 is dst's only writer
        CHECK(is(checked(c), "k_local (row bands) + bilateral5") && checked(c).out == Out::DST);
        c.flags |= kFlagForceStaged;
        CHECK(is(checked(c), "k_pre_v1 + k_post_v1 (staged tile kernels) + bilateral5"));
    }
    Call c = call(3);
    c.gaussian = false; c.bilateral = true; c.stop_after = kStageMedian5;
    CHECK(!checked(c).bilateral && is(checked(c), "k_local (row bands)"));
}

static void test_overlap()
{
    const size_t frame = (size_t)kRows * kCols * 4;
    for (uintptr_t shift : {(uintptr_t)0, (uintptr_t)4, (uintptr_t)kCols * 4, (uintptr_t)(3 * frame - 4)}) {
        Call c = call(3);
        c.dst = c.src + shift;
        const Plan p = checked(c);
        CHECK(p.route == Route::LOCAL && p.out == Out::PP0 && is(p, "k_local (row bands) + copy to dst"));
        c.dst = c.src - shift;
        CHECK(checked(c).out == Out::PP0);
    }
    Call c = call(3);
    c.dst = c.src + 3 * frame;                             // touching, not overlapping
    CHECK(checked(c).out == Out::DST);
    c = call(3);
    c.input = Input::U16;
    c.dst = c.src + 3 * frame / 2 - 4;                     // the last two bytes of the uint16 frames inside dst
    CHECK(checked(c).out == Out::PP0 && is(checked(c), "k_local<U16> (row bands) + copy to dst"));
    c.dst = c.src + 3 * frame / 2;
    CHECK(checked(c).out == Out::DST);
}

// without the flag -- and with it up to stop_after = FILL7 -- a call plans as it did: the same plan whatever DCMT_LOCAL_BANDS says,
// and none of the new fields set
static void test_unflagged()
{
    Knobs kb;
    kb.local_bands = 5;
    for (int batch : {1, 2, 8, 128, 236, 237, 1024})
        for (int input = 0; input < 3; ++input)
            for (int stop = 2; stop <= kStageFinal; ++stop)
                for (int flags : {0, kFlagForceStaged, kFlagForceFused, kFlagNormalize})
                    for (uintptr_t dst : {kDst, kSrc, kSrc + 4}) {
                        Call c = call(batch, false);
                        c.input = input == 0 ? Input::F32 : input == 1 ? Input::U16 : Input::LABELED;
                        if (input == 2) { c.labels = kLabels; c.n_labels = 500; }
                        if (input == 1 && (flags & kFlagNormalize)) continue;
                        c.stop_after = stop; c.flags = flags; c.dst = dst;
                        const Plan a = plan_call(Knobs{}, c), b = plan_call(kb, c);
                        CHECK(same(a, b));
                        CHECK(!a.no_extrapolate && a.local_bands == 1 && a.local_strips == 0 && a.local_grid == 0 && a.route != Route::LOCAL);
                        CHECK(std::strstr(a.path, "k_local") == nullptr);
                        if (stop <= kStageFill7) {
                            c.flags |= kFlagNoExtrapolate;
                            CHECK(same(a, plan_call(Knobs{}, c)));
                        }
                    }
    // the parent's plans of the cases tests/plan_test.cpp names, as that file pins them
    CHECK(is(plan_call(Knobs{}, call(1, false)), "k_pre_v1 + k_fill31_v1 + k_post_v1 (staged tile kernels)"));
    CHECK(is(plan_call(Knobs{}, call(8, false)), "k_pre_p (row bands) + k_fp_s (row bands)"));
    CHECK(is(plan_call(Knobs{}, call(128, false)), "k_pre_p (row bands) + k_fp_s"));
    CHECK(is(plan_call(Knobs{}, call(1024, false)), "k_pre_p<Q16OUT> + k_fp_q"));
    // the flag's environment name
    bool found = false;
    for (const KnobEnv& e : kKnobEnv) found |= std::strcmp(e.name, "DCMT_LOCAL_BANDS") == 0 && e.member == &Knobs::local_bands && e.parse == 'i';
    CHECK(found);
    CHECK(Knobs{}.local_bands == 0);
}

int main()
{
    test_batches();
    test_bands_knob();
    test_shapes_and_inputs();
    test_staged();
    test_bilateral();
    test_overlap();
    test_unflagged();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
