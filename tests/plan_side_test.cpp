// The launch geometry and scratch layout of the entry points beside the cascade (csrc/dcmt_plan_side.h, csrc/dcmt_chunks.h) on a
// CPU.  Built and run by tests/test_plan.py; prints every failed check and returns their number.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

constexpr uint32_t kKitti = 352u * 1216u;
constexpr uintptr_t kSrc = 0x100000000ull, kBgr = 0x900000000ull;      // 16-byte aligned
constexpr uint64_t k2p31 = 0x80000000ull;

// ---- colorize -----------------------------------------------------------------------------------------------------------
// the most frames a run of kColorPxPerWg pixels that starts at a multiple of kColorPxPerWg touches, in a run of `total` pixels
static uint32_t max_frames_touched(uint32_t n, uint32_t total)
{
    uint32_t m = 0;
    for (uint64_t p0 = 0; p0 < total; p0 += kColorPxPerWg) {
        const uint64_t last = std::min<uint64_t>(p0 + kColorPxPerWg, total) - 1;
        m = std::max<uint32_t>(m, (uint32_t)(last / n - p0 / n) + 1);
    }
    return m;
}

// what holds for the segments of every plan; brute: also count the frames every map workgroup touches
static ColorPlan checked_color(uint32_t n, int batch, uintptr_t src, uintptr_t bgr, bool brute)
{
    const ColorPlan p = plan_colorize(n, batch, src, bgr);
    CHECK(p.n == n && p.batch == (uint32_t)batch && p.chunks == eval_chunks(n) && p.count >= 1 && p.seg >= 1);
    uint32_t next = 0;
    for (uint32_t i = 0; i < p.count; ++i) {
        const ColorSegment s = p.segment(i);
        CHECK(s.first == next && s.frames >= 1);                                      // in order, no gap, no overlap
        next = s.first + s.frames;
        CHECK(i + 1 == p.count || s.frames == p.seg);
        CHECK((uint64_t)s.frames * n == s.total && s.total > 0 && s.total <= k2p31 - kColorPxPerWg);
        CHECK(s.span == std::min<uint32_t>(s.frames, (kColorPxPerWg - 1) / n + 2));
        if (brute && (i == 0 || i + 1 == p.count)) CHECK(s.span >= max_frames_touched(n, s.total));   // (the segments between have segment 0's n and total)
        CHECK(s.lds == 4u * 256 + 8u * s.span);
        CHECK(s.map_grid == (s.total + kColorPxPerWg - 1) / kColorPxPerWg);
        CHECK(s.minmax_x == eval_chunks(n) && s.minmax_y == s.frames);
        const uint64_t px0 = (uint64_t)s.first * n;
        CHECK(s.aligned == ((src + 4 * px0) % 16 == 0 && (bgr + 3 * px0) % 4 == 0));
    }
    CHECK(next == (uint32_t)batch);
    CHECK(p.count == 1 || p.seg < 4 || p.seg % 4 == 0);
    return p;
}

static void test_colorize()
{
    const struct { uint32_t n; int batch; } whole[] = {{kKitti, 1}, {kKitti, 1024}, {1, 65535}, {kKitti, 5016}};
    for (const auto& c : whole) {
        const ColorPlan p = checked_color(c.n, c.batch, kSrc, kBgr, true);
        CHECK(p.count == 1 && p.seg == (uint32_t)c.batch && p.segment(0).first == 0 && p.segment(0).frames == (uint32_t)c.batch);
    }
    const struct { uint32_t n; int batch; } cut[] = {{kKitti, 5017}, {kKitti, 65535}, {32769, 65535}, {0x1ffffff0u, 7}, {0x1ffffff0u, 3}};
    for (const auto& c : cut) {
        const ColorPlan p = checked_color(c.n, c.batch, kSrc, kBgr, true);
        CHECK((p.count > 1) == ((uint64_t)c.n * c.batch > k2p31 - kColorPxPerWg));
    }
    // 352 x 1216: the cap is 5017 frames (2^31 - 4096 - 5017 * n = 42,752 pixels to spare), so 5017 still go whole; 5018 go as 5016 + 2
    CHECK(plan_colorize(kKitti, 5017, kSrc, kBgr).count == 1 && plan_colorize(kKitti, 5017, kSrc, kBgr).seg == 5017);
    CHECK(checked_color(kKitti, 5018, kSrc, kBgr, true).seg == 5016 && plan_colorize(kKitti, 5018, kSrc, kBgr).count == 2);
    CHECK(plan_colorize(kKitti, 65535, kSrc, kBgr).seg == 5016 && plan_colorize(kKitti, 65535, kSrc, kBgr).count == 14);
    CHECK(plan_colorize(0x1ffffff0u, 7, kSrc, kBgr).seg == 3 && plan_colorize(0x1ffffff0u, 7, kSrc, kBgr).count == 3);
    // small frames, where a workgroup's run spans many of them
    for (uint32_t n : {1u, 2u, 3u, 5u, 1000u, 4095u, 4096u, 4097u, 8191u})
        for (int batch : {1, 2, 3, 7, 4097, 65535}) CHECK(checked_color(n, batch, kSrc + 4, kBgr + 1, true).count == 1);
    {
        // an odd frame size with a cap of 3: segment 1 starts 3 * n pixels in, 12 (mod 16) bytes into the source
        const uint32_t n = 0x1fffffefu;
        const ColorPlan p = checked_color(n, 7, kSrc, kBgr, true);
        CHECK(p.seg == 3 && p.count == 3);
        CHECK(p.segment(0).aligned && !p.segment(1).aligned);
        CHECK(!plan_colorize(n, 7, kSrc + 4, kBgr).segment(0).aligned && !plan_colorize(n, 7, kSrc, kBgr + 2).segment(0).aligned);
    }
    std::mt19937_64 rng(20240917);
    for (int t = 0; t < 4000; ++t) {
        // n log-uniform in [32769, 0x1ffffff0], batch uniform among those with batch * n >= 2^31
        const double u = std::uniform_real_distribution<double>(0.0, 1.0)(rng);
        uint32_t n = (uint32_t)(32769.0 * std::pow((double)0x1ffffff0u / 32769.0, u));
        n = std::min<uint32_t>(std::max<uint32_t>(n, 32769u), 0x1ffffff0u);
        const int lo = (int)((k2p31 + n - 1) / n);
        const int batch = std::uniform_int_distribution<int>(lo, 65535)(rng);
        const uintptr_t src = kSrc + 4 * (rng() % 4), bgr = kBgr + rng() % 4;
        const ColorPlan p = checked_color(n, batch, src, bgr, t % 50 == 0);
        CHECK(p.count > 1 || (uint64_t)n * batch <= k2p31 - kColorPxPerWg);
    }
}

// ---- the winner plane ---------------------------------------------------------------------------------------------------
static Winner checked_winner(int bits, unsigned gen, bool fresh, size_t n_index)
{
    const Winner w = winner_next(bits, gen, fresh, n_index);
    if (w.status == kOk) {
        CHECK(w.bits >= 24 && w.bits <= 30 && w.gen >= 1 && ((uint64_t)w.gen << w.bits) <= 0xffffffffull && w.tag == w.gen << w.bits);
        CHECK(((size_t)1 << w.bits) > n_index);
        CHECK(!w.clear || w.gen == 1);
    }
    return w;
}

static void test_winner()
{
    Winner w = checked_winner(0, 0, true, 1000);                 // a fresh plane
    CHECK(w.status == kOk && w.bits == 24 && w.clear && w.gen == 1 && w.tag == 1u << 24);
    for (int call = 2; call <= 255; ++call) {
        w = checked_winner(w.bits, w.gen, false, 1000);
        CHECK(w.status == kOk && !w.clear && w.gen == (unsigned)call && w.bits == 24);
    }
    w = checked_winner(w.bits, w.gen, false, 1000);              // the 256th: the generations have run out
    CHECK(w.clear && w.gen == 1 && w.bits == 24);
    w = checked_winner(24, 7, false, ((size_t)1 << 24) - 1);
    CHECK(!w.clear && w.bits == 24 && w.gen == 8);
    w = checked_winner(24, 7, false, (size_t)1 << 24);           // one more index bit: a new layout
    CHECK(w.status == kOk && w.clear && w.bits == 25 && w.gen == 1 && w.tag == 1u << 25);
    w = checked_winner(25, 1, false, 5);                         // a layout never shrinks
    CHECK(!w.clear && w.bits == 25 && w.gen == 2);
    w = checked_winner(0, 0, true, ((size_t)1 << 30) - 1);
    CHECK(w.status == kOk && w.bits == 30 && w.clear && w.gen == 1);
    w = checked_winner(w.bits, w.gen, false, 5);
    CHECK(!w.clear && w.gen == 2);
    w = checked_winner(w.bits, w.gen, false, 5);
    CHECK(!w.clear && w.gen == 3 && w.tag == 3u << 30);
    w = checked_winner(w.bits, w.gen, false, 5);                 // three generations with 30 bits
    CHECK(w.clear && w.gen == 1 && w.bits == 30);
    CHECK(winner_next(24, 7, false, (size_t)1 << 30).status == kInvalid && winner_next(0, 0, true, (size_t)1 << 31).status == kInvalid);
    w = checked_winner(30, 2, true, 0);                          // fresh resets both fields
    CHECK(w.status == kOk && w.clear && w.bits == 24 && w.gen == 1);
    CHECK(checked_winner(24, 0, false, 0).clear);                // generation 0: nothing written yet
    // an eager call keeps the generation it took: the state it leaves is the plan it always was
    for (unsigned gen : {0u, 1u, 7u, 254u, 255u}) {
        const Winner a = winner_next(24, gen, false, 1000), b = winner_next(24, gen, false, 1000, false);
        CHECK(a.keep == a.gen && a.status == b.status && a.bits == b.bits && a.gen == b.gen && a.clear == b.clear && a.tag == b.tag && a.keep == b.keep);
    }
    // a call whose stream is being captured: the clear is part of every replay, the generation is 1 whatever the context's was, and
    // the context is left at generation 0, so that the next call clears as well
    for (unsigned gen : {0u, 1u, 7u, 254u, 255u}) {
        const Winner c = winner_next(24, gen, false, 1000, true);
        CHECK(c.status == kOk && c.clear && c.gen == 1 && c.bits == 24 && c.tag == 1u << 24 && c.keep == 0);
        const Winner next = checked_winner(c.bits, c.keep, false, 1000);             // the eager call behind the capture
        CHECK(next.clear && next.gen == 1 && next.keep == 1);
        const Winner after = checked_winner(next.bits, next.keep, false, 1000);      // ... and the one behind that: above every replay's tags
        CHECK(!after.clear && after.gen == 2 && after.tag > (c.tag | 999u));
    }
    {
        const Winner c = winner_next(24, 7, false, (size_t)1 << 24, true);           // a captured call that needs a new layout
        CHECK(c.clear && c.bits == 25 && c.gen == 1 && c.tag == 1u << 25 && c.keep == 0);
        const Winner f = winner_next(30, 2, true, 5, true);                          // ... and one on a fresh plane
        CHECK(f.clear && f.bits == 24 && f.gen == 1 && f.keep == 0);
        CHECK(winner_next(24, 7, false, (size_t)1 << 30, true).status == kInvalid);
        // a graph captured under an older, narrower layout: an eager call of a later generation stays above its tags
        const Winner wide = checked_winner(25, 1, false, 5);
        CHECK(wide.gen == 2 && wide.tag > ((1u << 24) | ((1u << 24) - 1u)));
    }
}

// ---- SLIC ---------------------------------------------------------------------------------------------------------------
static int num_centers_loop(int rows, int cols, int step)       // dcmt_slic_num_centers as include/dcmt.h documents it (slic.cpp:33-34)
{
    int nx = 0, ny = 0;
    for (int i = step; i < cols - step / 2; i += step) ++nx;
    for (int j = step; j < rows - step / 2; j += step) ++ny;
    return nx * ny;
}

static SlicPlan checked_slic(int rows, int cols, int batch, int max_batch, int step, int scale, int th_override)
{
    const SlicPlan p = plan_slic(rows, cols, batch, max_batch, step, scale, th_override);
    const size_t b = (size_t)batch, per = b * p.cells;
    CHECK(p.n == num_centers_loop(rows, cols, step));
    CHECK(p.cell_px == (scale > 1 ? scale * step : step) && p.gx == (cols + p.cell_px - 1) / p.cell_px && p.gy == (rows + p.cell_px - 1) / p.cell_px);
    CHECK(p.cells == (size_t)p.gx * p.gy);
    // six ranges in the documented order, back to back: counts 0, flags 0, counts 1, flags 1, lists 0, lists 1
    CHECK(p.cnt[0] == 0 && p.ovf[0] == p.cnt[0] + per && p.cnt[1] == p.ovf[0] + b && p.ovf[1] == p.cnt[1] + per);
    CHECK(p.list[0] == p.ovf[1] + b && p.list[1] == p.list[0] + per * kSlicCellCap);
    const size_t end = p.list[1] + per * kSlicCellCap;
    CHECK(end == plan_slic(rows, cols, batch, batch, step, scale, th_override).reserve_cells && end <= p.reserve_cells);
    CHECK(p.reserve_cells == 2 * ((size_t)max_batch * p.cells * (1 + kSlicCellCap) + max_batch));
    CHECK(p.n_cnt == per + b && p.clear_cnt == p.list[0] - p.cnt[0]);             // the memset from cnt[0] covers exactly the four ranges in front of the lists
    CHECK(p.reserve_centers == 5 * (size_t)p.n * max_batch && p.reserve_sums == 6 * (size_t)p.n * max_batch);
    CHECK(p.clear_labels == b * rows * cols && p.clear_sums == 6 * (size_t)p.n * b && p.clear_sums <= p.reserve_sums);
    const int th_max = slic_tile_rows(p.cell_px);
    CHECK((p.th == 16 || p.th == 32 || p.th == 64) && p.th <= th_max);
    CHECK(p.tiles_x == (unsigned)((cols + kSlicTW - 1) / kSlicTW) && p.tiles_y == (unsigned)((rows + p.th - 1) / p.th));
    const bool honoured = (th_override == 16 || th_override == 32 || th_override == 64) && th_override <= th_max;
    if (honoured) CHECK(p.th == th_override);
    else {
        // halved while the grid has fewer than 1024 workgroups: no taller tile has 1024, and this one has unless it is the shortest
        auto wgs = [&](int th) { return (size_t)p.tiles_x * ((rows + th - 1) / th) * b; };
        for (int th = th_max; th > p.th; th /= 2) CHECK(wgs(th) < 1024);
        CHECK(p.th == 16 || wgs(p.th) >= 1024);
    }
    CHECK(p.init_x == (unsigned)((p.n + 63) / 64));
    CHECK(p.nb_threads == std::max((size_t)p.n * b, p.n_cnt) && p.bin_x == (unsigned)((p.nb_threads + 255) / 256));
    return p;
}

static void test_slic()
{
    const struct { int rows, cols, step; } shapes[] = {{352, 1216, 18}, {375, 1242, 68}, {8, 8, 6}};
    for (const auto& s : shapes)
        for (int batch : {1, 7})
            for (int scale : {0, 1, 3})
                for (int th : {0, 16, 32, 64, 48, 8}) checked_slic(s.rows, s.cols, batch, 7, s.step, scale, th);
    CHECK(plan_slic(8, 8, 1, 7, 6, 0, 0).n == 0);
    CHECK(plan_slic(352, 1216, 1, 7, 18, 0, 0).n == 19 * 67 && plan_slic(352, 1216, 1, 7, 18, 3, 0).cell_px == 54);
    // one 352 x 1216 frame: 19 x 6 = 114 tiles of 64 rows, 209 of 32, 418 of 16
    CHECK(plan_slic(352, 1216, 1, 7, 18, 0, 0).th == 16 && plan_slic(352, 1216, 1, 7, 18, 0, 64).th == 64);
    CHECK(plan_slic(352, 1216, 7, 7, 18, 0, 0).th == 32);        // 7 * 209 = 1463 >= 1024 > 7 * 114
    CHECK(plan_slic(352, 1216, 16, 16, 18, 0, 0).th == 64);      // 16 * 114 = 1824
    CHECK(plan_slic(352, 1216, 16, 16, 12, 0, 64).th == 32);     // steps 11 to 15 allow 32 rows: the override is not honoured
    CHECK(plan_slic(352, 1216, 16, 16, 12, 0, 16).th == 16 && plan_slic(352, 1216, 16, 16, 6, 0, 32).th == 16);
}

// ---- Gaussian, stereo, resolve ------------------------------------------------------------------------------------------
static GaussPlan checked_gauss(int rows, int cols, int batch)
{
    const GaussPlan p = plan_gauss5(rows, cols, batch);
    CHECK(p.strips == (cols + kGaussCols - 1) / kGaussCols);
    CHECK(p.band_rows == 32 || p.band_rows == 16 || p.band_rows == 8);
    auto waves = [&](int br) { return (size_t)p.strips * ((rows + br - 1) / br) * batch; };
    for (int br = kGaussRows; br > p.band_rows; br /= 2) CHECK(waves(br) < 2048);
    CHECK(p.band_rows == 8 || waves(p.band_rows) >= 2048);
    CHECK(p.bands == (rows + p.band_rows - 1) / p.band_rows);
    CHECK(p.grid_x == (unsigned)(((size_t)p.strips * p.bands + 3) / 4));
    return p;
}

static void test_gauss_stereo_vec()
{
    CHECK(checked_gauss(352, 1216, 1024).band_rows == 32);
    CHECK(checked_gauss(8, 8, 1).band_rows == 8 && checked_gauss(8, 8, 1).grid_x == 1);
    CHECK(checked_gauss(352, 1216, 1).band_rows == 8);           // 21 strips x 44 bands = 924 waves
    CHECK(checked_gauss(352, 1216, 5).band_rows == 16);          // 21 x 22 x 5 = 2310 >= 2048 > 21 x 11 x 5
    CHECK(checked_gauss(352, 1216, 9).band_rows == 32);          // 21 x 11 x 9 = 2079
    for (int batch : {1, 2, 3, 4, 8, 9, 16, 100}) { checked_gauss(375, 1242, batch); checked_gauss(61, 121, batch); }

    StereoPlan s = plan_stereo(352, 48 * 1024 - 4, 2);           // cols + 4 = 48 KiB: the last width whose row fits
    CHECK(s.status == kOk && s.lds_row && s.lds == 48u * 1024 && s.gx == 1 && s.gy == 352 && s.gz == 2);
    s = plan_stereo(352, 48 * 1024 - 3, 2);
    CHECK(s.status == kOk && !s.lds_row && s.lds == 0 && s.gx == (48u * 1024 - 3 + 255) / 256 && s.gy == 352 && s.gz == 2);
    s = plan_stereo(352, 1216, 1);
    CHECK(s.status == kOk && s.lds_row && s.lds == 1220 && s.gx == 1);
    CHECK(plan_stereo(65535, 8, 65535).status == kOk && plan_stereo(65536, 8, 1).status == kInvalid && plan_stereo(8, 8, 65536).status == kInvalid);

    const struct { size_t n_px; int by_count; } counts[] = {{352 * 1216, 4}, {375 * 1242, 2}, {375 * 1241, 1}};
    const struct { uintptr_t addr; int by_addr; } addrs[] = {{kSrc, 4}, {kSrc + 8, 2}, {kSrc + 4, 1}};
    for (const auto& c : counts)
        for (const auto& a : addrs) CHECK(resolve_vec(c.n_px, a.addr) == std::min(c.by_count, a.by_addr));
}

// ---- the chunking (dcmt_chunks.h) -----------------------------------------------------------------------------------------
static void test_chunks()
{
    CHECK(eval_chunks(kKitti) == 53 && eval_chunks(1) == 1 && eval_chunks(8192) == 1 && eval_chunks(8193) == 2);
    CHECK(eval_chunks(0x1ffffff0u) == kEvalMaxChunks);
    for (uint32_t n : {1u, 5u, 8192u, 8193u, kKitti, 375u * 1242u, 0x1ffffff0u})
        CHECK((uint64_t)eval_chunks(n) * eval_chunk_groups(n) >= (n + 3) / 4 && (uint64_t)(eval_chunks(n) - 1) * eval_chunk_groups(n) < (n + 3) / 4);
}

// ---- geometry C of tests/large_batch_cases.py: 65535 frames of 128 x 260 ------------------------------------------------
// 2,181,004,800 pixels: more than 2^31 and more than the segments' 0x7fff0000, so each of the three segmented entry points runs
// exactly two segments; the launch loops in dcmt.hip and dcmt_cloud.hip advance their pointers by `first`.
static void test_geometry_c()
{
    constexpr uint32_t n = 128u * 260u;
    constexpr int batch = 65535;
    constexpr uint64_t px = (uint64_t)n * batch;
    static_assert(px == 2181004800ull && px > k2p31 && px > kBgrSegPx && px > kU16SegPx && px < 2ull * kBgrSegPx, "geometry C");
    constexpr uintptr_t kLab = 0xC00000000ull, kGray = 0xE00000000ull, kOut = 0x400000000ull;     // clear of kSrc + 4 px and kBgr + 3 px

    // the colourisation: whole frames, a multiple of 4 of them in all segments but the last
    const ColorPlan c = checked_color(n, batch, kSrc, kBgr, true);
    CHECK(c.count == 2 && c.seg == 64524 && c.seg % 4 == 0);
    const ColorSegment c0 = c.segment(0), c1 = c.segment(1);
    CHECK(c0.first == 0 && c0.frames == 64524 && c0.total == 64524u * n && c0.minmax_y == 64524);
    CHECK(c1.first == 64524 && c1.frames == 1011 && c1.total == 1011u * n && c1.minmax_y == 1011);
    CHECK((uint64_t)c0.total + c1.total == px && (uint64_t)(c0.frames + 4) * n > k2p31 - kColorPxPerWg);     // (the next multiple of 4 would not fit)
    CHECK(c0.aligned && c1.aligned);                       // `aligned` follows each segment's own addresses:
    CHECK(!plan_colorize(n, batch, kSrc + 4, kBgr).segment(0).aligned && !plan_colorize(n, batch, kSrc + 4, kBgr).segment(1).aligned);
    CHECK(!plan_colorize(n, batch, kSrc, kBgr + 2).segment(0).aligned && !plan_colorize(n, batch, kSrc, kBgr + 2).segment(1).aligned);
    CHECK(plan_colorize(n, batch, kSrc + 16, kBgr + 4).segment(1).aligned);

    // the BGR ingest: a flat run cut at kBgrSegPx, wherever that falls in a frame (here inside frame 64525)
    const BgrPlan b = plan_bgr_convert(px, kBgr, kLab, kGray);
    CHECK(b.status == kOk && b.px == px && b.count == 2 && b.passes == kBgrMaxPasses && b.aligned);
    const BgrSegment b0 = b.segment(0), b1 = b.segment(1);
    CHECK(b0.first == 0 && b0.total == kBgrSegPx && b0.grid == (kBgrSegPx + b.share() - 1) / b.share());
    CHECK(b1.first == kBgrSegPx && b1.total == (uint32_t)(px - kBgrSegPx) && b1.total == 33586688u && b1.grid == (b1.total + b.share() - 1) / b.share());
    CHECK(b1.first / n == 64525 && b1.first % n != 0 && b1.first % 4 == 0);
    CHECK(!plan_bgr_convert(px, kBgr, kLab + 1, kGray).aligned && !plan_bgr_convert(px, kBgr + 2, kLab, kGray).aligned &&
          !plan_bgr_convert(px, kBgr, kLab, kGray + 3).aligned && plan_bgr_convert(px, kBgr, kLab, 0).aligned);
    CHECK(plan_bgr_convert(px, kBgr, kBgr, kGray).status == kOk && plan_bgr_convert(px, kBgr, kBgr + 3 * px - 1, 0).status == kInvalid);

    // the uint16 export
    const U16Plan u = plan_depth_to_u16(px, kSrc, kOut);
    CHECK(u.status == kOk && u.px == px && u.count == 2 && u.aligned);
    const U16Segment u0 = u.segment(0), u1 = u.segment(1);
    CHECK(u0.first == 0 && u0.total == kU16SegPx && u0.grid == kU16SegPx / kU16PxPerWg);
    CHECK(u1.first == kU16SegPx && u1.total == (uint32_t)(px - kU16SegPx) && u1.grid == (u1.total + kU16PxPerWg - 1) / kU16PxPerWg);
    CHECK((4 * u1.first) % 16 == 0 && (2 * u1.first) % 16 == 0);
    CHECK(!plan_depth_to_u16(px, kSrc + 4, kOut).aligned && !plan_depth_to_u16(px, kSrc, kOut + 2).aligned);
    CHECK(plan_depth_to_u16(px, kSrc, kSrc + 4 * px - 2).status == kInvalid);
}

int main()
{
    test_colorize();
    test_geometry_c();
    test_winner();
    test_slic();
    test_gauss_stereo_vec();
    test_chunks();
    std::printf(failures ? "%d checks failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
