// The cascade's plan with DCMT_BLUR_GAUSSIAN_VALID (csrc/dcmt_plan.h) on a CPU: a kind of the finishing kernel on the two routes
// without extrapolation, a step of its own behind the chain to MEDIAN5 with it.  Built and run by tests/test_gauss_valid.py; prints
// every failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <string>

#include "dcmt_plan.h"

using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static bool has(const char* s, const char* part) { return std::strstr(s, part) != nullptr; }
static bool ends_with(const char* s, const char* tail)
{
    const size_t n = std::strlen(s), m = std::strlen(tail);
    return n >= m && std::strcmp(s + n - m, tail) == 0;
}

static Call base(int rows, int cols, int batch, Input in, int stop, int flags)
{
    Call c;
    c.rows = rows; c.cols = cols; c.batch = batch; c.input = in; c.src = 0x100000000ull; c.dst = 0x200000000ull;
    c.n_labels = in == Input::LABELED ? 12 : 0; c.labels = in == Input::LABELED ? 0x300000000ull : 0;
    c.gaussian = false; c.bilateral = false; c.valid = true; c.stop_after = stop; c.flags = flags; c.q16_allowed = true;
    return c;
}

// the same launches, whatever the kind: everything but the kind and the path
static bool same_launches(const Plan& a, const Plan& b)
{
    return a.route == b.route && a.k0kind == b.k0kind && a.norm == b.norm && a.xcd_map == b.xcd_map && a.out == b.out && a.few == b.few &&
           a.tile_h == b.tile_h && a.tiles_x == b.tiles_x && a.tiles_y == b.tiles_y && a.u16_convert == b.u16_convert && a.dump == b.dump &&
           a.needs_colstat == b.needs_colstat && a.needs_bbox == b.needs_bbox && a.needs_x6q == b.needs_x6q &&
           a.no_extrapolate == b.no_extrapolate && a.local_bands == b.local_bands && a.local_strips == b.local_strips && a.local_grid == b.local_grid;
}

// without the extrapolation: one kernel on route LOCAL, the staged pair elsewhere; the kind changes the instance, never the launches
static void test_no_extrapolate()
{
    const Knobs k;
    const int ne = kFlagNoExtrapolate;
    for (int batch : {1, 3, 8, 128})
        for (int stop : {kStageBlur, kStageFinal})
            for (uintptr_t dst : {(uintptr_t)0x200000000ull, (uintptr_t)0x100000000ull}) {
                struct { Input in; int flags; const char* name; } local[] = {
                    {Input::F32, ne, "k_local<VALID>"}, {Input::U16, ne, "k_local<U16,VALID>"}, {Input::F32, ne | kFlagNormalize, "k_local<NORM,VALID>"},
                    {Input::LABELED, ne, "k_local<START4,VALID>"}};
                for (const auto& l : local)
                    for (int k0 : {kK0AsCompiled, kK0Diamond}) {
                        Call c = base(352, 1216, batch, l.in, stop, l.flags);
                        c.k0kind = k0; c.dst = dst;
                        const Plan p = plan_call(k, c);
                        CHECK(p.route == Route::LOCAL && p.valid_kind && !p.gauss_valid && !p.bilateral && p.no_extrapolate);
                        CHECK(has(p.path, l.name) && !has(p.path, "gauss5_valid"));
                        Call g = c;
                        g.valid = false; g.gaussian = true;
                        const Plan q = plan_call(k, g);
                        CHECK(same_launches(p, q) && !q.valid_kind && !has(q.path, "VALID"));
                        // the probe at MEDIAN5 ignores the blur
                        Call m = c;
                        m.stop_after = kStageMedian5;
                        const Plan r = plan_call(k, m);
                        CHECK(r.route == Route::LOCAL && !r.valid_kind && !r.gauss_valid && !has(r.path, "VALID"));
                    }
                // STAGED: forced, a custom k0, frames under 8 rows or columns, labels that are not used
                struct { int rows, cols, flags, k0; } staged[] = {{352, 1216, ne | kFlagForceStaged, kK0AsCompiled}, {64, 96, ne, -1}, {5, 3, ne, kK0Diamond},
                                                                   {1, 65, ne, kK0AsCompiled}, {70, 7, ne, kK0AsCompiled}};
                for (const auto& s : staged)
                    for (Input in : {Input::F32, Input::U16}) {
                        Call c = base(s.rows, s.cols, batch, in, stop, s.flags);
                        c.k0kind = s.k0; c.dst = dst;
                        const Plan p = plan_call(k, c);
                        CHECK(p.route == Route::STAGED && p.valid_kind && !p.gauss_valid && p.no_extrapolate && p.out == Out::DST);
                        CHECK(ends_with(p.path, "k_pre_v1 + k_post_v1<VALID> (staged tile kernels)"));
                        Call g = c;
                        g.valid = false; g.gaussian = true;
                        const Plan q = plan_call(k, g);
                        CHECK(same_launches(p, q) && !q.valid_kind && ends_with(q.path, "k_pre_v1 + k_post_v1 (staged tile kernels)"));
                    }
            }
    // up to FILL7 the flag and the blur are ignored
    Call c = base(64, 96, 4, Input::F32, kStageFill7, ne);
    CHECK(!plan_call(k, c).valid_kind && !plan_call(k, c).gauss_valid && !plan_call(k, c).no_extrapolate);
}

// with the extrapolation: the same call with stop_after = MEDIAN5 into context scratch on every route, then k_gauss5<VALID>
static void test_extrapolating()
{
    const Knobs k;
    for (int batch : {1, 4, 64, 256})
        for (int flags : {0, kFlagForceStaged, kFlagForceFused, kFlagNormalize})
            for (Input in : {Input::F32, Input::U16, Input::LABELED})
                for (int stop : {kStageBlur, kStageFinal})
                    for (uintptr_t dst : {(uintptr_t)0x200000000ull, (uintptr_t)0x100000000ull, (uintptr_t)0x100000004ull}) {
                        if (in == Input::U16 && (flags & kFlagNormalize)) continue;
                        Call c = base(64, 96, batch, in, stop, flags);
                        c.dst = dst;
                        const Plan p = plan_call(k, c);
                        Call m = c;
                        m.valid = false; m.stop_after = kStageMedian5; m.dst = 0;
                        const Plan q = plan_call(k, m);
                        CHECK(p.gauss_valid && !q.gauss_valid && !p.valid_kind && !p.bilateral && p.gauss_valid_invert == (stop == kStageFinal));
                        CHECK(p.route == q.route && p.out == Out::DST && !p.fuse_fp && !p.q16 && !p.needs_x6q && !p.no_extrapolate);
                        CHECK(std::string(p.path) == std::string(q.path) + " + gauss5_valid");
                        CHECK(p.pre_grid == q.pre_grid && p.fill_grid == q.fill_grid && p.post_grid == q.post_grid && p.tiles_y == q.tiles_y);
                        Call e = c;
                        e.stop_after = kStageMedian5;
                        CHECK(!plan_call(k, e).gauss_valid && !has(plan_call(k, e).path, "gauss5_valid"));
                    }
}

// every other blur plans what it planned: no kind, no extra step, the path strings of the routes as they were
static void test_other_blurs()
{
    const Knobs k;
    for (int flags : {0, kFlagNoExtrapolate, kFlagNoExtrapolate | kFlagForceStaged, kFlagForceStaged})
        for (int batch : {1, 16, 256})
            for (int blur = 0; blur < 3; ++blur) {
                Call c = base(352, 1216, batch, Input::F32, kStageFinal, flags);
                c.valid = false; c.gaussian = blur == 1; c.bilateral = blur == 2;
                const Plan p = plan_call(k, c);
                CHECK(!p.valid_kind && !p.gauss_valid && !has(p.path, "VALID") && !has(p.path, "gauss5_valid"));
                CHECK(p.bilateral == (blur == 2));
            }
    Call c = base(352, 1216, 1, Input::F32, kStageFinal, kFlagNoExtrapolate);
    c.valid = false; c.gaussian = true;
    CHECK(std::string(plan_call(k, c).path) == "k_local (row bands)");
    c.flags |= kFlagForceStaged;
    CHECK(std::string(plan_call(k, c).path) == "k_pre_v1 + k_post_v1 (staged tile kernels)");
    c.flags = 0; c.batch = 16; c.q16_allowed = false;
    CHECK(has(plan_call(k, c).path, "k_pre_p") && has(plan_call(k, c).path, " + k_fp_s"));
    c.valid = true; c.gaussian = false;
    CHECK(has(plan_call(k, c).path, "k_pre_p") && has(plan_call(k, c).path, "k_post_s") == false && ends_with(plan_call(k, c).path, " + gauss5_valid"));
}

int main()
{
    test_no_extrapolate();
    test_extrapolating();
    test_other_blurs();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
