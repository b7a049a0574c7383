// The cascade's dispatch (csrc/dcmt_plan.h) on a CPU: which route, kernels, strips, bands and scratch plane a call gets.
// Built and run by tests/test_plan.py; prints every failed check and returns their number.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "dcmt_plan.h"

using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

constexpr int kRows = 352, kCols = 1216;
constexpr uintptr_t kSrc = 0x100000000ull, kDst = 0x900000000ull, kLabels = 0x1100000000ull;   // 16-byte aligned, 32 GiB apart
constexpr int kStageFillLoop = 8;

// frames of 352 x 1216, f32, aligned, not overlapping, default params, through the device entry point, an attempt allowed
static Call call(int batch)
{
    Call c;
    c.rows = kRows; c.cols = kCols; c.batch = batch;
    c.src = kSrc; c.dst = kDst;
    c.q16_allowed = true;
    return c;
}
static Call labeled_call(int batch, int n_labels)
{
    Call c = call(batch);
    c.input = Input::LABELED; c.labels = kLabels; c.n_labels = n_labels;
    return c;
}

// what holds for every plan: the scratch it names is the scratch its route uses
static Plan checked(const Knobs& k, const Call& c)
{
    const Plan p = plan_call(k, c);
    CHECK(p.needs_x6q == p.q16);
    CHECK(p.q16_own_flag == (p.q16 && c.capturing));
    CHECK(!p.q16 || (p.route == Route::STREAMING && p.pair && p.table && p.fuse_fp));
    CHECK(p.needs_colstat == (p.route == Route::STAGED));
    CHECK(p.needs_bbox == (c.input == Input::LABELED && (p.route == Route::LABEL_PROBE || p.route == Route::STREAMING)));
    CHECK(p.route == route_of(k, c));
    CHECK((std::strstr(p.path, kPathCopy) != nullptr) == (p.out != Out::DST));
    CHECK(p.bands >= 1 && p.bands <= kMaxBands && p.fb_s >= 1 && p.label_group >= 1 && p.label_group <= kLabelGroupMax);
    return p;
}
static Plan checked(const Call& c) { return checked(Knobs{}, c); }

static bool ends_with(const char* s, const char* tail)
{
    const size_t n = std::strlen(s), m = std::strlen(tail);
    return n >= m && std::strcmp(s + n - m, tail) == 0;
}

// the names of the fields in which two plans differ, in declaration order
static std::string diff(const Plan& a, const Plan& b)
{
    std::string d;
#define F(f) if (a.f != b.f) d += std::string(d.empty() ? "" : ",") + #f;
    F(route) F(k0kind) F(norm) F(xcd_map) F(out) F(needs_x6q) F(needs_colstat) F(needs_bbox) F(few) F(tile_h) F(tiles_x) F(tiles_y)
    F(u16_convert) F(dump) F(bbox_lds) F(lpair) F(label_pairs) F(label_group) F(label_grid_x) F(table) F(wide) F(pair) F(q16) F(bands)
    F(fb_s) F(pre_strips) F(fill_strips) F(post_strips) F(q_strips) F(pre_grid) F(fill_grid) F(post_grid) F(fp_s_grid) F(fp_q_grid)
    F(fuse_fp) F(filled) F(tail) F(fp_s_launch) F(n_redo) F(q16_own_flag)
#undef F
    if (std::strcmp(a.path, b.path) != 0) d += std::string(d.empty() ? "" : ",") + "path";
    return d;
}
#define CHECK_DIFF(a, b, want) do { const std::string d_ = diff(a, b); if (d_ != (want)) { ++failures; \
    std::printf("line %d: the plans differ in {%s}, expected {%s}\n", __LINE__, d_.c_str(), want); } } while (0)

static void test_table()
{
    for (int batch : {1, 2}) {
        const Plan p = checked(call(batch));
        CHECK(p.route == Route::STAGED && p.few && p.tile_h == FTH_FEW && p.tiles_y == (kRows + FTH_FEW - 1) / FTH_FEW && p.tiles_x == kCols / TW);
        CHECK(std::strcmp(p.path, "k_pre_v1 + k_fill31_v1 + k_post_v1 (staged tile kernels)") == 0);
    }
    {
        const Plan p = checked(call(8));
        CHECK(p.route == Route::STREAMING && p.pair && p.pre_strips == 12 && p.bands == 8 && p.fb_s == 11 && !p.q16);
        CHECK(std::strcmp(p.path, "k_pre_p (row bands) + k_fp_s (row bands)") == 0);
    }
    {
        const Plan p = checked(call(128));
        CHECK(p.bands == 2 && p.fb_s == 1 && !p.q16);
        CHECK(std::strcmp(p.path, "k_pre_p (row bands) + k_fp_s") == 0);
    }
    CHECK(!checked(call(236)).q16);               // 236 * 11 = 2596 < 2600 <= 237 * 11
    CHECK(checked(call(237)).q16);
    {
        const Plan p = checked(call(1024));
        CHECK(p.q16 && p.bands == 1 && p.pre_strips == 12 && p.q_strips == 11 && p.fill_strips == 36 && p.post_strips == 22);
        CHECK(p.filled && p.n_redo == 1 && p.tail && !p.fp_s_launch && p.xcd_map == 1 && p.wide);
        CHECK(p.pre_grid == 8u * 128 * 12 / 4 && p.fp_q_grid == 8u * 128 * 11 / 4 && p.fill_grid == 9u * 1024 && p.post_grid == 6u * 1024);
        CHECK(std::strcmp(p.path, "k_pre_p<Q16OUT> + k_fp_q") == 0);
        Call c = call(1024);
        c.q16_allowed = false;                    // the context is skipping attempts
        CHECK_DIFF(p, checked(c), "needs_x6q,q16,fp_s_launch,path");
        Knobs off;
        off.fp_q16 = 0;
        CHECK(!checked(off, call(1024)).q16);
        // the same call while its stream is being captured into a graph: the same kernels on the same grids, the attempt's flag its own
        Call g = call(1024);
        g.capturing = true;
        CHECK_DIFF(p, checked(g), "q16_own_flag");
        CHECK(checked(g).q16_own_flag && !p.q16_own_flag);
        g.q16_allowed = false;
        CHECK_DIFF(checked(c), checked(g), "");            // no attempt: capturing changes nothing
        CHECK(!checked(off, g).q16 && !checked(off, g).q16_own_flag);
    }
    for (int batch : {1, 2, 8, 128, 236}) {               // every plan without an attempt is the eager plan, field for field
        Call g = call(batch);
        g.capturing = true;
        CHECK_DIFF(checked(call(batch)), checked(g), "");
        Call l = labeled_call(batch, 1200), lg = l;
        lg.capturing = true;
        CHECK_DIFF(checked(l), checked(lg), "");
    }
    for (int blur = 0; blur < 2; ++blur) {                // the two finishes plan their chain with the call's fields: capturing among them
        Call f = call(1024);
        f.gaussian = false; f.bilateral = blur == 0; f.valid = blur == 1;
        Call g = f;
        g.capturing = true;
        CHECK_DIFF(checked(f), checked(g), checked(f).q16 ? "q16_own_flag" : "");
    }
    {
        Call c = call(1024);
        c.spec_fill_iters = 0;
        const Plan p = checked(c);
        CHECK(p.q16 && !p.tail && p.fp_s_launch && p.n_redo == 0 && !p.filled);   // k_fp_s is not dropped behind the attempt
    }
    {
        Call c = call(1024);
        c.dst = c.src;
        CHECK(!checked(c).q16 && checked(c).out == Out::DST);
        c.dst = c.src + sizeof(float) * kRows * kCols;       // shifted by one frame
        CHECK(!checked(c).q16 && checked(c).out == Out::DST);
        c.dst = c.src + sizeof(float) * kRows * kCols * 1024;   // right behind the frames
        CHECK(checked(c).q16);
    }
    {
        Call c = call(1024);
        c.flags = kFlagNormalize;
        const Plan p = checked(c);
        CHECK(!p.q16 && p.norm && std::strcmp(p.path, "k_pre_p<NORM> + k_fp_s") == 0);
        c.stop_after = kStageNormalize;
        CHECK(checked(c).route == Route::NORMALIZE_ONLY && std::strcmp(checked(c).path, "k_minmax + k_norm_coef + k_norm_write") == 0);
        c.dst = c.src;
        CHECK(checked(c).out == Out::PP0);
    }
    {
        Call c = call(1024);
        c.input = Input::U16;
        c.in_scale = 1.0f / 256.0f;
        CHECK(checked(c).q16 && !checked(c).wide && std::strcmp(checked(c).path, "k_pre_p<U16,Q16OUT> + k_fp_q") == 0);
        c.in_scale = 1.0f / 128.0f;
        CHECK(!checked(c).q16 && std::strcmp(checked(c).path, "k_pre_p<U16> + k_fp_s") == 0);
    }
    {
        Call c = call(1024);
        c.max_depth = 80.0f;
        CHECK(!checked(c).q16);
        c = call(1024);
        c.valid_thresh = 0.2f;
        CHECK(!checked(c).q16);
    }
    {
        Call c = call(16);
        c.cols = 1215;
        const Plan p = checked(c);
        CHECK(p.route == Route::STREAMING && !p.pair && !p.wide && p.bands == 1 && p.pre_strips == (1215 + 47) / 48);
        CHECK(std::strncmp(p.path, "k_pre_s + ", 10) == 0);
    }
    {
        Call c = call(16);
        c.src += 4;                               // 4-byte but not 8-byte aligned
        const Plan p = checked(c);
        CHECK(!p.pair && !p.wide && std::strncmp(p.path, "k_pre_s + ", 10) == 0);
        c.src += 4;                               // 8-byte but not 16-byte aligned: two columns per lane again
        CHECK(checked(c).pair && !checked(c).wide);
    }
    {
        Call c = call(16);
        c.stop_after = kStageExtend;
        CHECK(checked(c).out == Out::DST && std::strcmp(checked(c).path, "k_pre_p") == 0);
        c.dst = c.src;
        const Plan p = checked(c);                // output to X6 (= the X5 plane), then one copy
        CHECK(p.route == Route::STREAMING && p.out == Out::X5 && p.pair && ends_with(p.path, " + copy to dst"));
    }
    {
        Call c = call(16);
        c.stop_after = kStageFill7;
        c.flags = kFlagForceStaged;
        c.dst = c.src;
        const Plan p = checked(c);
        CHECK(p.route == Route::STAGED && !p.few && p.tile_h == TH && p.out == Out::X5 && p.dump == 0 && ends_with(p.path, " + copy to dst"));
        c.stop_after = kStageClose5;
        CHECK(checked(c).out == Out::PP0 && checked(c).dump == kStageClose5);
        c.stop_after = kStageFillLoop;            // past the probes the staged kernels write dst last
        CHECK(checked(c).out == Out::DST);
    }
    {
        Call c = labeled_call(16, 1200);
        c.stop_after = kStageClose5;
        CHECK(checked(c).route == Route::LABEL_PROBE && checked(c).out == Out::DST);
        c.dst = c.src;
        const Plan p = checked(c);                // X4 in pp[0], then one copy
        CHECK(p.route == Route::LABEL_PROBE && p.out == Out::PP0 && std::strcmp(p.path, "k_label_bbox + k_label_stage + copy to dst") == 0);
        c.stop_after = kStageFinal;               // the whole chain reads X4 from scratch: in place like any other call
        CHECK(checked(c).route == Route::STREAMING && checked(c).out == Out::DST);
        c.n_labels = 0;
        CHECK(checked(c).route == Route::STAGED);
    }
    {
        Call c = call(16);
        c.k0kind = kK0Diamond;
        CHECK(checked(c).route == Route::STREAMING && checked(c).pre_strips == (kCols + 103) / 104);
        CHECK(checked(c).bands == 8);             // counted with the as-compiled width: 16 * 12 strips
        c.k0kind = -1;
        CHECK(checked(c).route == Route::STAGED);
    }
}

// The geometries of tests/large_batch_cases.py whose batches the cascade takes: 65535 frames of 96 x 176 (the largest batch: the
// frame is a grid's z or y dimension in the staged and the label kernels) and 2512 frames of 352 x 1216 (f32 planes beyond 2^32 bytes).
// Every grid of every plan fits in 31 bits, and on-grid input gets the 16-bit attempt.
static bool grids_fit(const Plan& p, int batch)
{
    for (unsigned g : {p.pre_grid, p.fill_grid, p.post_grid, p.fp_s_grid, p.fp_q_grid, p.local_grid})
        if (g > 0x7fffffffu) return false;
    return p.tiles_x >= 0 && p.tiles_y >= 0 && p.tiles_y <= 65535 && p.label_grid_x >= 0 && p.label_grid_x <= 0x7fffffff && batch <= 65535;
}

static void test_large_batches()
{
    const struct { int rows, cols, batch; } geo[] = {{96, 176, 65535}, {352, 1216, 2512}};
    for (const auto& g : geo) {
        Call c = call(g.batch);
        c.rows = g.rows; c.cols = g.cols;
        CHECK((uint64_t)g.batch * g.rows * g.cols * 4 > 0x100000000ull && kSrc + (uint64_t)g.batch * g.rows * g.cols * 4 <= kDst);
        const Plan p = checked(c);
        CHECK(p.route == Route::STREAMING && p.q16 && p.needs_x6q && p.pair && p.table && p.bands == 1 && p.fb_s == 1 && p.tail && !p.fp_s_launch && p.filled);
        CHECK(p.xcd_map == (g.batch % 8 == 0 ? 1 : 0));
        CHECK(std::strcmp(p.path, "k_pre_p<Q16OUT> + k_fp_q") == 0);
        CHECK(grids_fit(p, g.batch));
        CHECK(p.pre_grid == wave_grid(p.pre_strips, g.batch, p.xcd_map) && p.fp_q_grid == wave_grid(p.q_strips, g.batch, p.xcd_map));
        CHECK(p.pre_grid >= (unsigned)(((uint64_t)g.batch * p.pre_strips) / 4) && p.fp_q_grid >= (unsigned)(((uint64_t)g.batch * p.q_strips) / 4));
        CHECK(p.fill_grid == (unsigned)((p.fill_strips + 3) / 4) * (unsigned)g.batch && p.post_grid == (unsigned)((p.post_strips + 3) / 4) * (unsigned)g.batch);
        {
            Call u = c;
            u.input = Input::U16; u.in_scale = 1.0f / 256.0f;
            CHECK(checked(u).q16 && grids_fit(checked(u), g.batch) && std::strcmp(checked(u).path, "k_pre_p<U16,Q16OUT> + k_fp_q") == 0);
        }
        {
            Call n = c;
            n.flags = kFlagNormalize;
            CHECK(!checked(n).q16 && grids_fit(checked(n), g.batch) && std::strcmp(checked(n).path, "k_pre_p<NORM> + k_fp_s") == 0);
            CHECK(checked(n).fp_s_grid == wave_grid(checked(n).post_strips, g.batch, checked(n).xcd_map));
            n.stop_after = kStageNormalize;
            CHECK(checked(n).route == Route::NORMALIZE_ONLY && checked(n).out == Out::DST);
        }
        {
            Call s = c;
            s.flags = kFlagForceStaged;
            const Plan ps = checked(s);
            CHECK(ps.route == Route::STAGED && !ps.few && ps.tiles_x == (g.cols + TW - 1) / TW && ps.tiles_y == (g.rows + TH - 1) / TH && grids_fit(ps, g.batch));
        }
        {
            Call l = c;
            l.flags = kFlagNoExtrapolate;
            const Plan pl = checked(l);
            CHECK(pl.route == Route::LOCAL && pl.local_bands == 1 && std::strcmp(pl.path, "k_local") == 0 && grids_fit(pl, g.batch));
            CHECK(pl.local_grid == wave_grid(pl.local_strips, g.batch, pl.xcd_map) && pl.local_grid >= (unsigned)(((uint64_t)g.batch * pl.local_strips) / 4));
        }
        {
            Call e = c;
            e.stop_after = kStageExtend;
            CHECK(checked(e).out == Out::DST && std::strcmp(checked(e).path, "k_pre_p") == 0 && grids_fit(checked(e), g.batch));
            e.stop_after = kStageMedian5;
            e.bilateral = true;       // (what blur = BILATERAL_CLONE plans from stop_after = BLUR on: the chain up to the median)
            e.stop_after = kStageBlur;
            CHECK(checked(e).bilateral && std::strcmp(checked(e).path, "k_pre_p + bilateral5") == 0 && grids_fit(checked(e), g.batch));
        }
        for (int n_labels : {40, 1200, 3500}) {
            Call l = c;
            l.input = Input::LABELED; l.labels = kLabels; l.n_labels = n_labels;
            const Plan pl = checked(l);
            CHECK(pl.route == Route::STREAMING && pl.needs_bbox && pl.q16 && grids_fit(pl, g.batch));
            CHECK(pl.bbox_lds == (16 * n_labels <= 48 * 1024));
            CHECK(std::strncmp(pl.path, "k_label_bbox + k_label_stage + k_pre_p", 38) == 0);
        }
    }
}

// batch 16, DCMT_FP_Q16 on, DCMT_Q16_MIN_WAVES=0: one knob at a time.  The expected sets are read off the parent's dispatch: a knob
// moves the field it names and what the dispatch derives from that field (fields a route does not reach keep their defaults).
static void test_knobs()
{
    Knobs base;
    base.q16_min_waves = 0;
    const Call c = call(16), lc = labeled_call(16, 1200);
    const Plan p = checked(base, c), lp = checked(base, lc);
    CHECK(p.route == Route::STREAMING && p.q16 && p.pair && p.wide && p.table && p.bands == 8 && p.fb_s == 9 && p.xcd_map == 1);
    CHECK(p.pre_grid == 384 && p.fp_q_grid == 48 && p.fp_s_grid == 792 && p.fill_grid == 144 && p.post_grid == 96 && p.filled && p.tail);
    CHECK(std::strcmp(p.path, "k_pre_p<Q16OUT> (row bands) + k_fp_q") == 0);
    CHECK(lp.route == Route::STREAMING && lp.q16 && lp.bbox_lds && lp.lpair && lp.label_group == 4 && lp.label_pairs && lp.label_grid_x == 75);
    CHECK(lp.pre_strips == 11 && std::strcmp(lp.path, "k_label_bbox + k_label_stage + k_pre_p<Q16OUT> (row bands) + k_fp_q") == 0);
    Knobs k;
    k = base; k.xcd_map = 0;         CHECK_DIFF(p, checked(k, c), "xcd_map,fp_q_grid");        // (the other grids round to the same size)
    k = base; k.wide = 0;            CHECK_DIFF(p, checked(k, c), "wide");
    k = base; k.fuse_fp = 0;         CHECK_DIFF(p, checked(k, c), "needs_x6q,table,q16,bands,fb_s,pre_grid,fp_s_grid,fp_q_grid,fuse_fp,filled,tail,n_redo,path");
    k = base; k.top_table = 0;       CHECK_DIFF(p, checked(k, c), "needs_x6q,table,q16,bands,fb_s,pre_grid,fp_s_grid,fp_s_launch,path");
    k = base; k.pair = 0;            CHECK_DIFF(p, checked(k, c), "needs_x6q,pair,q16,bands,pre_strips,pre_grid,fp_s_launch,path");
    k = base; k.bands = 3;           CHECK_DIFF(p, checked(k, c), "bands,pre_grid");
    k = base; k.fbands = 2;          CHECK_DIFF(p, checked(k, c), "fb_s,fp_s_grid");
    k = base; k.assume_filled = 0;   CHECK_DIFF(p, checked(k, c), "filled");
    k = base; k.min_fused_batch = 16; CHECK_DIFF(p, checked(k, c), "");
    k = base; k.min_fused_batch = 17; CHECK(checked(k, c).route == Route::STAGED && !checked(k, c).q16 && !checked(k, c).few);
    k = base; k.label_pairs = 0;     CHECK_DIFF(lp, checked(k, lc), "label_pairs");            // (the grid is k_label_stage_p's)
    k = base; k.label_group = 1;     CHECK_DIFF(lp, checked(k, lc), "label_group,label_grid_x");
    k = base; k.bbox_global = 1;     CHECK_DIFF(lp, checked(k, lc), "bbox_lds");
    k = base; k.label_pairs = 0; k.label_group = 1; k.bbox_global = 1; CHECK_DIFF(p, checked(k, c), "");   // nothing without labels
    k = base; k.pair = 0; k.label_pairs = 0; CHECK(!checked(k, lc).lpair && checked(k, lc).label_grid_x == 300);
    k = base; k.pair = 0;            CHECK(checked(k, lc).label_grid_x == 150);
}

// one table row per Knobs member, each variable read the way dcmt_create always read it
static void test_env()
{
    constexpr size_t n = sizeof kKnobEnv / sizeof kKnobEnv[0];
    CHECK(n * sizeof(int) == sizeof(Knobs));
    for (const KnobEnv& e : kKnobEnv) unsetenv(e.name);
    const Knobs d = knobs_from_env(), init;
    for (size_t i = 0; i < n; ++i) {
        CHECK(d.*kKnobEnv[i].member == init.*kKnobEnv[i].member);
        for (size_t j = 0; j < i; ++j) CHECK(kKnobEnv[i].member != kKnobEnv[j].member);
        setenv(kKnobEnv[i].name, "17", 1);
        const Knobs k = knobs_from_env();
        CHECK(k.*kKnobEnv[i].member == (kKnobEnv[i].parse == 'i' ? 17 : 1));
        for (size_t j = 0; j < n; ++j) CHECK(j == i || k.*kKnobEnv[j].member == init.*kKnobEnv[j].member);
        unsetenv(kKnobEnv[i].name);
    }
    setenv("DCMT_POISON", "0", 1);
    setenv("DCMT_BBOX_GLOBAL", "0", 1);
    CHECK(knobs_from_env().poison == 0 && knobs_from_env().bbox_global == 1);
}

int main()
{
    test_table();
    test_large_batches();
    test_knobs();
    test_env();
    std::printf(failures ? "%d checks failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
