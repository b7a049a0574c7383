// dcmt_plan_side.h -- the launch geometry and scratch layout of the entry points beside the cascade, as values: one pure function
// per entry point that has something to decide; dcmt.hip and dcmt_cloud.hip check, plan, reserve, and then launch what the plan
// says.  Plain C++17, no HIP, like dcmt_plan.h: tested on a CPU (tests/plan_test.cpp).  The kernels' constants come from the
// HIP-free headers their kernel headers include; only the two status values are restated (dcmt.hip checks them).
#ifndef DCMT_PLAN_SIDE_H
#define DCMT_PLAN_SIDE_H

#include <cstddef>
#include <cstdint>

#include "dcmt_chunks.h"
#include "dcmt_cloud.h"
#include "dcmt_connect.h"
#include "dcmt_contour.h"
#include "dcmt_crop.h"
#include "dcmt_occlusion.h"
#include "dcmt_photo.h"
#include "dcmt_joint.h"
#include "dcmt_normals.h"
#include "dcmt_plan.h"         // ranges_overlap
#include "dcmt_planes.h"
#include "dcmt_rectify.h"
#include "dcmt_support.h"
#include "dcmt_tiles.h"

#pragma GCC visibility push(hidden)       // internal names: none of them in libdcmt_hip.so's dynamic symbol table
namespace dcmt {
namespace plan {

constexpr int kOk = 0, kInvalid = -1;        // dcmt.h: DCMT_OK, DCMT_E_INVALID

// ---- dcmt_colorize_dev --------------------------------------------------------------------------------------------------
// A min/max pass over the frames, then one map pass over their flat pixel run (dcmt_kernels_color.h).  Batches of 2^31 pixels or
// more go in segments of whole frames, each a pair of launches of its own: a segment holds at most 2^31 - kColorPxPerWg pixels
// (32-bit pixel indices, the last workgroup's overhang included).  All segments but the last have `seg` frames, a multiple of 4
// where the cap allows 4, so that they start as aligned as the batch does; frames above ~2^29 pixels have a cap of 3, and there a
// later segment may be less aligned than the first -- `aligned` is decided per segment, from its own addresses.  (Measured, 1024
// frames of 352 x 1216: segments of 128 / 64 / 32 frames, whose re-read could come from the Infinity Cache, take 0.90 / 0.91 /
// 1.03 ms against 0.85 ms for the whole batch in one pair.)
struct ColorSegment {
    uint32_t first, frames;          // frames [first, first + frames) of the batch
    uint32_t total;                  // its pixels
    uint32_t span;                   // frames one map workgroup can touch
    size_t lds;                      // k_color_map's dynamic LDS: the palette, then (scale, shift) for `span` frames
    unsigned map_grid;               // k_color_map
    unsigned minmax_x, minmax_y;     // k_color_minmax: (chunks, frames)
    bool aligned;                    // k_color_map<true>: source 16-byte, output 4-byte aligned
};

struct ColorPlan {
    uint32_t n, batch, chunks;       // pixels per frame, frames, eval_chunks(n)
    uint32_t seg, count;             // frames per segment (the last one: what is left), segments
    uintptr_t src, bgr;
    ColorSegment segment(uint32_t i) const
    {
        ColorSegment s;
        s.first = i * seg;
        s.frames = batch - s.first < seg ? batch - s.first : seg;
        s.total = s.frames * n;
        const uint32_t reach = (kColorPxPerWg - 1) / n + 2;
        s.span = s.frames < reach ? s.frames : reach;
        s.lds = sizeof(uint32_t) * 256 + sizeof(float) * 2 * s.span;
        s.map_grid = (s.total + kColorPxPerWg - 1) / kColorPxPerWg;
        s.minmax_x = chunks;
        s.minmax_y = s.frames;
        s.aligned = (src + sizeof(float) * (size_t)s.first * n) % 16 == 0 && (bgr + (size_t)3 * s.first * n) % 4 == 0;
        return s;
    }
};

// n = rows * cols >= 1 (at most 0x1ffffff0: dcmt_create), batch >= 1
inline ColorPlan plan_colorize(uint32_t n, int batch, uintptr_t src_addr, uintptr_t bgr_addr)
{
    ColorPlan p;
    p.n = n; p.batch = (uint32_t)batch; p.chunks = eval_chunks(n);
    p.src = src_addr; p.bgr = bgr_addr;
    const uint32_t cap = (0x80000000u - kColorPxPerWg) / n;                 // frames per segment the 32-bit pixel run allows (>= 3)
    p.seg = p.batch < cap ? p.batch : cap;
    if (p.seg >= 4 && p.seg < p.batch) p.seg &= ~3u;
    p.count = (p.batch + p.seg - 1) / p.seg;
    return p;
}

// ---- the winner plane of dcmt_project_points_dev and dcmt_reproject_depth_dev (winner_generation, dcmt_ctx.h) -----------
// One call's step of the plane's state: (bits, gen) = the index bits of the tag layout and the last call's generation, fresh = the
// plane has just been (re)allocated, n_index = the call stores indices below n_index.  The plane is cleared when it is fresh,
// when the call needs more index bits than the layout has, and when the generations have run out.
// capturing = the call's stream is being captured into a graph: the call's kernels run later, any number of times, with the tag
// they were given here, and what the plane holds by then is anybody's.  Such a call always clears (the clear is a node of the graph,
// in front of its kernels), takes generation 1 and leaves `keep` = 0 for the context, so that the next call clears as well: a call
// that runs between two replays finds the replay's tags of generation 1 under whatever generation it would have taken.
struct Winner {
    int status;                      // kInvalid: 2^30 indices or more (nothing else is meaningful then)
    int bits;
    unsigned gen;
    bool clear;                      // zero the plane before the call's kernels
    unsigned tag;                    // gen << bits
    unsigned keep;                   // the generation the context remembers: gen, or 0 behind a captured call
};

inline Winner winner_next(int bits, unsigned gen, bool fresh, size_t n_index, bool capturing = false)
{
    int need_bits = 1;
    while (need_bits < 31 && ((size_t)1 << need_bits) <= n_index) ++need_bits;
    if (need_bits > 30) return {kInvalid, bits, gen, false, 0, gen};
    if (fresh) { bits = 0; gen = 0; }
    const bool relayout = need_bits > bits;
    if (relayout) bits = need_bits < 24 ? 24 : need_bits;                  // (room for 16 M indices per call before the next re-layout)
    const unsigned gen_max = (1u << (32 - bits)) - 1u;
    const bool clear = capturing || relayout || gen == 0 || gen >= gen_max;
    gen = clear ? 1 : gen + 1;
    return {kOk, bits, gen, clear, gen << bits, capturing ? 0u : gen};
}

// k_project_resolve / k_reproject_resolve: pixels per thread, as wide as the pixel count and the output's address allow
inline int resolve_vec(size_t n_px, uintptr_t addr)
{
    return n_px % 4 == 0 && addr % 16 == 0 ? 4 : n_px % 2 == 0 && addr % 8 == 0 ? 2 : 1;
}

// ---- the per-frame calibration tables of the *_calib_dev calls ----------------------------------------------------------------
// A table of `batch` records of `rec` bytes at address `table`: present and aligned to `align` ...
inline bool calib_table_aligned(uintptr_t table, size_t align) { return table != 0 && table % align == 0; }
// ... and clear of an output buffer of the same call (`out_bytes` bytes at `out`)
inline bool calib_table_clear_of(uintptr_t table, size_t rec, int batch, uintptr_t out, size_t out_bytes)
{
    return !ranges_overlap(table, rec * (size_t)batch, out, out_bytes);
}

// ---- dcmt_project_points_nearest*_dev, dcmt_reproject_depth_nearest*_dev ----------------------------------------------------
// A clear of the output plane, a scatter of keys into it, one fix-up pass over it in place (dcmt_kernels_nearest.h).  The output is
// cleared before the inputs are read, so it must be clear of every input, the table included; the checks on the buffers are here,
// tested without a device.  Nothing of the context is touched: no scratch, no state.
struct NearestPlan {
    int status;                      // kInvalid: a null or misaligned pointer, 2^30 points or more, an output that overlaps an input
    size_t n_px;                     // pixels of the output plane, the whole batch
    size_t clear_bytes;              // hipMemsetAsync of the output
    unsigned scatter_x, scatter_y;   // the scatter kernel's grid, 256 threads; scatter_x == 0: nothing to scatter, no launch
    int vec;                         // k_nearest_fixup<vec>
    unsigned fixup_x;                // its grid, 256 threads
};

inline NearestPlan nearest_plane(size_t n_px, uintptr_t out)
{
    NearestPlan p = {kOk, n_px, sizeof(float) * n_px, 0, 1, resolve_vec(n_px, out), 0};
    p.fixup_x = (unsigned)((n_px / (size_t)p.vec + 255) / 256);
    return p;
}

// rows, cols, batch >= 1 and within the context's limits; table: 0 for the uniform call (table_call says which call it is)
inline NearestPlan plan_project_nearest(int rows, int cols, int batch, int n_points, uintptr_t points, uintptr_t offsets, bool table_call,
                                        uintptr_t table, uintptr_t out)
{
    const NearestPlan bad = {kInvalid, 0, 0, 0, 0, 0, 0};
    if (!offsets || !out || n_points < 0 || n_points >= (1 << 30) || (n_points > 0 && !points)) return bad;
    if (points % 16 != 0 || offsets % 4 != 0 || out % 4 != 0) return bad;      // whole 16-byte records; integer atomics on the plane
    if (table_call && !calib_table_aligned(table, 16)) return bad;
    NearestPlan p = nearest_plane((size_t)batch * (size_t)rows * (size_t)cols, out);
    if (ranges_overlap(out, p.clear_bytes, points, (size_t)16 * (size_t)n_points) ||
        ranges_overlap(out, p.clear_bytes, offsets, sizeof(int32_t) * ((size_t)batch + 1)) ||
        (table_call && !calib_table_clear_of(table, 96, batch, out, p.clear_bytes)))
        return bad;
    p.scatter_x = (unsigned)((n_points + 255) / 256);
    return p;
}

// both shapes and batch >= 1 and within the context's limits
inline NearestPlan plan_reproject_nearest(int rows, int cols, int out_rows, int out_cols, int batch, uintptr_t depth, bool table_call,
                                          uintptr_t table, uintptr_t out)
{
    const NearestPlan bad = {kInvalid, 0, 0, 0, 0, 0, 0};
    if (!depth || !out || depth % 4 != 0 || out % 4 != 0) return bad;
    if (table_call && !calib_table_aligned(table, 8)) return bad;
    const size_t n = (size_t)rows * (size_t)cols;
    NearestPlan p = nearest_plane((size_t)batch * (size_t)out_rows * (size_t)out_cols, out);
    if (ranges_overlap(out, p.clear_bytes, depth, sizeof(float) * n * (size_t)batch) ||
        (table_call && !calib_table_clear_of(table, 136, batch, out, p.clear_bytes)))
        return bad;
    p.scatter_x = (unsigned)((n + kReprojectPxPerWg - 1) / kReprojectPxPerWg);
    p.scatter_y = (unsigned)batch;
    return p;
}

// ---- dcmt_slic_labels_dev -----------------------------------------------------------------------------------------------
inline int slic_num_centers(int rows, int cols, int step)
{
    if (rows < 1 || cols < 1 || step < 1) return 0;
    int nx = 0, ny = 0;
    for (int i = step; i < cols - step / 2; i += step) ++nx;     // slic.cpp:33-34
    for (int j = step; j < rows - step / 2; j += step) ++ny;
    return nx * ny;
}

// slic_cells holds two cell sets (the assignment reads one while the next centres are binned into the other), laid out for this
// call's batch: set 0's counts [batch][cells] with its [batch] overflow flags right behind, set 1's the same, then set 0's and
// set 1's centre indices [batch][cells][kSlicCellCap].  All four buffers are reserved for max_batch frames, so they grow only with
// the cells / centres per frame.
struct SlicPlan {
    int n;                           // centres per frame (0: the call only sets the labels to -1)
    int cell_px, gx, gy;             // cells of cell_px x cell_px pixels, gx x gy of them
    size_t cells;
    size_t cnt[2], ovf[2], list[2];  // element offsets into slic_cells
    size_t n_cnt;                    // one set's counts and flags (k_slic_norm_bin clears the set it has read)
    size_t reserve_cells, reserve_centers, reserve_sums;   // slic_cells; slic_centers[0] and [1] each; slic_sums
    size_t clear_labels, clear_cnt, clear_sums;            // elements the three memsets cover: d_labels; both sets' counts and flags, from cnt[0]; slic_sums
    int th;                          // tile height of k_slic_assign: 64, 32 or 16
    unsigned tiles_x, tiles_y;       // k_slic_assign: (tiles_x, tiles_y, batch)
    unsigned init_x;                 // k_slic_init: (init_x, batch), 64 threads
    size_t nb_threads;               // k_slic_norm_bin: one thread per centre and per count / flag
    unsigned bin_x;
};

// cell_scale > 1: cells of cell_scale x step pixels (crowded cells, for tests); th_override: 16, 32 or 64 where the step allows it
// (the DCMT_SLIC_CELL_SCALE / DCMT_SLIC_TH values of the call, 0 where unset)
inline SlicPlan plan_slic(int rows, int cols, int batch, int max_batch, int step, int cell_scale, int th_override)
{
    SlicPlan p;
    const size_t b = (size_t)batch, mb = (size_t)max_batch;
    p.n = slic_num_centers(rows, cols, step);
    p.cell_px = cell_scale > 1 ? step * cell_scale : step;
    p.gx = (cols - 1) / p.cell_px + 1; p.gy = (rows - 1) / p.cell_px + 1;
    p.cells = (size_t)p.gx * p.gy;
    p.n_cnt = b * p.cells + b;
    p.cnt[0] = 0; p.cnt[1] = p.n_cnt;
    p.ovf[0] = p.cnt[0] + b * p.cells; p.ovf[1] = p.cnt[1] + b * p.cells;
    p.list[0] = 2 * p.n_cnt; p.list[1] = p.list[0] + b * p.cells * kSlicCellCap;
    p.reserve_cells = 2 * (mb * p.cells * (1 + kSlicCellCap) + mb);
    p.reserve_centers = 5 * (size_t)p.n * mb;                              // the three centre buffers grow together
    p.reserve_sums = 6 * (size_t)p.n * mb;
    p.clear_labels = b * rows * cols;
    p.clear_cnt = 2 * p.n_cnt;
    p.clear_sums = 6 * (size_t)p.n * b;
    // tile height: the tallest the step allows, unless that leaves the GPU short of workgroups (a caller streaming single frames:
    // 114 tiles of 64 x 64 per 1216 x 352 image for 256 CUs) -- then shorter tiles, more of them, shorter columns per thread
    p.tiles_x = (unsigned)((cols + kSlicTW - 1) / kSlicTW);
    p.th = slic_tile_rows(p.cell_px);
    if ((th_override == 16 || th_override == 32 || th_override == 64) && th_override <= p.th) p.th = th_override;
    else while (p.th > 16 && (size_t)p.tiles_x * ((rows + p.th - 1) / p.th) * b < 1024) p.th /= 2;
    p.tiles_y = (unsigned)((rows + p.th - 1) / p.th);
    p.init_x = (unsigned)((p.n + 63) / 64);
    p.nb_threads = (size_t)p.n * b > p.n_cnt ? (size_t)p.n * b : p.n_cnt;
    p.bin_x = (unsigned)((p.nb_threads + 255) / 256);
    return p;
}

// ---- dcmt_slic_connectivity_dev ------------------------------------------------------------------------------------------
// Connected-component labelling of the label plane and the reference's relabelling of it (dcmt_kernels_connect.h): seven launches
// whose grids depend on the shape alone (the border merge is left out where a frame is one tile), on the context's two 4 B/px
// planes and a slab of one word per (frame, strip of kConnStripCols columns).  The checks on the arguments are here as well, tested
// without a device: out may BE labels (the last kernel is the only writer of out and reads no labels), any other overlap among
// labels, out and counts is refused.
inline int connectivity_lims(int rows, int cols, int n_centers)      // slic.cpp:188; 0 where it cannot be formed
{
    if (rows < 1 || cols < 1 || n_centers < 1 || (int64_t)rows * cols > 0x1ffffff0) return 0;
    return (rows * cols) / n_centers;
}

// the bound on a frame's label count, kInvalid where the call refuses the shape: every non-small component holds more than
// lims >> 2 pixels
inline int connectivity_max_labels(int rows, int cols, int n_centers)
{
    const int lims = connectivity_lims(rows, cols, n_centers);
    if (lims < 4) return kInvalid;
    const int m = (rows * cols) / ((lims >> 2) + 1);
    return m < 1 ? 1 : m;
}

struct ConnPlan {
    int status;                      // kInvalid: a null or misaligned pointer, n_centers < 1, lims < 4, buffers that overlap
    ConnGeom g;                      // k_conn_local, k_conn_border, k_conn_flatten; k_conn_relabel: (g.px_x, batch) as well
    uint32_t lim4;                   // lims >> 2: a component is small iff size + (size >= 2) <= lim4
    int max_labels;
    uint32_t strips, band_rows;      // k_conn_seed, k_conn_rank: (strips, batch); k_conn_scan: (batch)
    size_t slab;                     // words of the slab this call uses: [batch][strips]
};

// the slab a context keeps for its largest call
inline size_t connectivity_slab_words(int max_cols, int max_batch)
{
    return (size_t)max_batch * (size_t)((max_cols + kConnStripCols - 1) / kConnStripCols);
}

// rows, cols, batch >= 1 and within the context's limits
inline ConnPlan plan_connectivity(int rows, int cols, int batch, int n_centers, uintptr_t labels, uintptr_t out, uintptr_t counts)
{
    ConnPlan p = {};
    p.status = kInvalid;
    if (!labels || !out || labels % 4 != 0 || out % 4 != 0 || counts % 4 != 0) return p;
    p.max_labels = connectivity_max_labels(rows, cols, n_centers);
    if (p.max_labels == kInvalid) return p;
    const size_t bytes = sizeof(int32_t) * (size_t)batch * (size_t)rows * (size_t)cols;
    if (out != labels && ranges_overlap(labels, bytes, out, bytes)) return p;
    if (counts && (ranges_overlap(counts, sizeof(int32_t) * (size_t)batch, labels, bytes) ||
                   ranges_overlap(counts, sizeof(int32_t) * (size_t)batch, out, bytes)))
        return p;
    p.status = kOk;
    p.g = conn_geom(rows, cols);
    p.lim4 = (uint32_t)(connectivity_lims(rows, cols, n_centers) >> 2);
    p.strips = ((uint32_t)cols + kConnStripCols - 1) / kConnStripCols;
    p.band_rows = ((uint32_t)rows + kConnWaves - 1) / kConnWaves;
    p.slab = (size_t)batch * p.strips;
    return p;
}

// ---- dcmt_filter_speckles_dev ---------------------------------------------------------------------------------------------
// The speckle filter of a 16-bit disparity map (dcmt_kernels_speckle.h): a clear of the counts (where they are wanted) and four
// launches whose grids depend on the shape alone (the border merge is left out where a frame is one tile), on the context's two
// 4 B/px planes; the tiles and the pairs are conn_geom's, as for plan_connectivity.  The checks on the arguments are here as well, tested
// without a device: out may BE disp (the last kernel is the only writer of out and depth, and a thread reads its pixels before it
// writes them), any other overlap among disp, out, depth and removed is refused.
struct SpecklePlan {
    int status;                      // kInvalid: a null or misaligned pointer, max_size < 0, max_diff outside 0..65535, new_val outside
                                     // int16, buffers that overlap
    ConnGeom g;                      // k_spk_local, k_spk_border, k_conn_flatten
    int vec;                         // k_spk_apply<vec>: 4 where a frame is a multiple of 4 pixels and disp and out are 8-byte aligned, else 1
    unsigned apply_x;                // its grid: (apply_x, batch)
    size_t clear_bytes;              // hipMemsetAsync of removed: 4 bytes a frame (0: no counts wanted)
};

// rows, cols, batch >= 1 and within the context's limits; depth, removed: 0 = not wanted
inline SpecklePlan plan_speckles(int rows, int cols, int batch, int64_t max_size, int64_t max_diff, int64_t new_val, uintptr_t disp, uintptr_t out,
                                 uintptr_t depth, uintptr_t removed)
{
    SpecklePlan p = {};
    p.status = kInvalid;
    if (!disp || !out || disp % 2 != 0 || out % 2 != 0 || depth % 4 != 0 || removed % 4 != 0) return p;
    if (max_size < 0 || max_size > 0x7fffffff || max_diff < 0 || max_diff > 65535 || new_val < -32768 || new_val > 32767) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols, rb = sizeof(uint32_t) * (size_t)batch;
    if (out != disp && ranges_overlap(disp, 2 * px, out, 2 * px)) return p;
    if (depth && (ranges_overlap(depth, 4 * px, disp, 2 * px) || ranges_overlap(depth, 4 * px, out, 2 * px))) return p;
    if (removed && (ranges_overlap(removed, rb, disp, 2 * px) || ranges_overlap(removed, rb, out, 2 * px) ||
                    (depth && ranges_overlap(removed, rb, depth, 4 * px))))
        return p;
    p.status = kOk;
    p.g = conn_geom(rows, cols);
    p.vec = p.g.n % 4 == 0 && disp % 8 == 0 && out % 8 == 0 ? 4 : 1;
    p.apply_x = (p.g.n / (uint32_t)p.vec + 255) / 256;
    p.clear_bytes = removed ? rb : 0;
    return p;
}

// ---- dcmt_slic_contours_dev, dcmt_slic_cluster_means_dev ------------------------------------------------------------------
// The two pixel renderings of SLIC (dcmt_kernels_contour.h), three launches each whose grids depend on the shape alone.  The
// contours borrow pp[0] for the code bytes and pp[1] for the taken bytes, 1 B/px each, both [batch][cols][rows]; the means borrow
// pp[0] for the sums where the caller passes none.  The checks on the arguments are here as well, tested without a device: every
// overlap among the device buffers of a call is refused.
struct ContourPlan {
    int status;                      // kInvalid: no labels, neither output, no colour, a misaligned label plane, more than
                                     // 64 * kContMaxChunks rows, buffers that overlap
    uint32_t chunks;                 // ceil(rows / 64): the steps of a column in k_cont_walk, the tile rows of the other two
    uint32_t tiles_x;
    unsigned tile_grid;              // k_cont_classify, k_cont_paint: (tile_grid, batch)
    uint32_t steps;                  // k_cont_walk: (batch) waves of cols * chunks steps
    size_t walk_lds;                 // ... its dynamic LDS: one 64-bit mask per chunk
    size_t scratch;                  // bytes of each of the two borrowed planes this call uses
};

// rows, cols, batch >= 1 and within the context's limits (a frame of at most 2^29 - 16 pixels)
inline ContourPlan plan_contours(int rows, int cols, int batch, uintptr_t labels, uintptr_t bgr, uintptr_t mask, uintptr_t colour)
{
    ContourPlan p = {};
    p.status = kInvalid;
    if (!labels || labels % 4 != 0 || (!bgr && !mask) || !colour) return p;
    const uint32_t chunks = ((uint32_t)rows + kContTile - 1) / kContTile;
    if (chunks > (uint32_t)kContMaxChunks) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols;
    if (bgr && ranges_overlap(labels, 4 * px, bgr, 3 * px)) return p;
    if (mask && ranges_overlap(labels, 4 * px, mask, px)) return p;
    if (bgr && mask && ranges_overlap(bgr, 3 * px, mask, px)) return p;
    p.status = kOk;
    p.chunks = chunks;
    p.tiles_x = ((uint32_t)cols + kContTile - 1) / kContTile;
    p.tile_grid = p.tiles_x * p.chunks;
    p.steps = (uint32_t)cols * p.chunks;                 // < 2^29 / 64 + 2^29
    p.walk_lds = sizeof(uint64_t) * p.chunks;
    p.scratch = px;
    return p;
}

// the largest n_labels a call with `batch` frames may name: batch * n_labels * 16 bytes of sums fit in one borrowed plane of
// plane_bytes (4 * max_batch * max_rows * max_cols), and a frame's sums are addressed with 32-bit words
inline int cluster_means_max_labels(size_t plane_bytes, int batch)
{
    const size_t m = plane_bytes / 16 / (size_t)(batch < 1 ? 1 : batch);
    return m > 0x0fffffff ? 0x0fffffff : (int)m;
}

struct MeansPlan {
    int status;                      // kInvalid: a null or misaligned pointer, n_labels < 1 or beyond cluster_means_max_labels, a frame
                                     // whose sums could pass 2^32 (255 * rows * cols), buffers that overlap
    uint32_t n;                      // pixels per frame
    uint32_t tiles_x, tiles_y;
    unsigned sum_grid;               // k_means_sum: (sum_grid, batch)
    unsigned px_x;                   // k_means_paint: (px_x, batch)
    size_t words;                    // the sums: batch * n_labels * 4
    unsigned clear_grid;             // k_means_clear
};

inline MeansPlan plan_cluster_means(int rows, int cols, int batch, int n_labels, size_t plane_bytes, uintptr_t labels, uintptr_t bgr,
                                    uintptr_t sums)
{
    MeansPlan p = {};
    p.status = kInvalid;
    if (!labels || !bgr || labels % 4 != 0 || sums % 4 != 0) return p;
    if (n_labels < 1 || n_labels > cluster_means_max_labels(plane_bytes, batch)) return p;
    if ((uint64_t)rows * (uint64_t)cols * 255u > 0xffffffffull) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols;
    p.words = (size_t)batch * (size_t)n_labels * 4;
    if (ranges_overlap(labels, 4 * px, bgr, 3 * px)) return p;
    if (sums && (ranges_overlap(sums, 4 * p.words, labels, 4 * px) || ranges_overlap(sums, 4 * p.words, bgr, 3 * px))) return p;
    p.status = kOk;
    p.n = (uint32_t)rows * (uint32_t)cols;
    p.tiles_x = ((uint32_t)cols + kContTile - 1) / kContTile;
    p.tiles_y = ((uint32_t)rows + kContTile - 1) / kContTile;
    p.sum_grid = p.tiles_x * p.tiles_y;
    p.px_x = (p.n + 255) / 256;
    const size_t blocks = (p.words + 255) / 256;
    p.clear_grid = blocks > 4096 ? 4096u : (unsigned)blocks;
    return p;
}

// ---- dcmt_superpixel_planes_dev -------------------------------------------------------------------------------------------
// One plane of inverse depth per superpixel (dcmt_kernels_planes.h): clear, sum, solve, paint, with clear, sum and solve a second
// time in front of the paint where a refit is asked for; the grids depend on the shape and n_labels alone.  The moment records
// borrow pp[0], the fits pp[1] where the caller passes none.  The checks on the arguments are here as well, tested without a
// device: out may BE depth (k_planes_paint is the only writer of out, and a lane reads its pixels before it writes them), every
// other overlap is refused.  The float parameters come as their bits: the library is built with -ffinite-math-only.

// the largest n_labels a call with `batch` frames may name: batch * n_labels * 96 bytes of moment records fit in one borrowed plane
// of plane_bytes (4 * max_batch * max_rows * max_cols)
inline int planes_max_labels(size_t plane_bytes, int batch)
{
    const size_t m = plane_bytes / (8 * (size_t)kPlanesMomWords) / (size_t)(batch < 1 ? 1 : batch);
    return m > 0x00ffffff ? 0x00ffffff : (int)m;
}

// what dcmt_planes_params may hold (dcmt.h); positive finite floats order as their bits do
inline bool planes_params_ok(uint32_t valid_thresh_bits, uint32_t max_depth_bits, int64_t min_points, int64_t min_extent, uint32_t refit_tol_bits,
                             int64_t keep_returns)
{
    if (valid_thresh_bits < kPlanesMinThreshBits || valid_thresh_bits >= 0x7f800000u) return false;
    if (max_depth_bits < valid_thresh_bits || max_depth_bits > kPlanesMaxDepthBits) return false;
    if (min_points < 3 || min_points > 0x7fffffff || min_extent < 1 || min_extent > 0x7fffffff) return false;
    if (refit_tol_bits >= 0x3f800000u && refit_tol_bits != 0x80000000u) return false;      // [0, 1), -0.0 included; NaN, inf, negatives: above 1.0f's bits
    return keep_returns == 0 || keep_returns == 1;
}

struct PlanesPlan {
    int status;                      // kInvalid: a null or misaligned pointer, n_labels < 1 or beyond planes_max_labels, more than
                                     // kPlanesMaxPixels pixels a frame, bad parameters, buffers that overlap
    uint32_t n;                      // pixels per frame
    uint32_t tiles_x, tiles_y;
    unsigned sum_grid;               // k_planes_sum: (sum_grid, batch)
    int vec;                         // k_planes_paint<vec>: 4 where a frame is a multiple of 4 pixels and depth, labels and out are 16-byte aligned, else 1
    unsigned paint_x;                // its grid: (paint_x, batch)
    size_t records;                  // batch * n_labels: the lanes of k_planes_solve
    unsigned solve_grid;
    size_t words;                    // the moment records as 32-bit words: records * 24
    unsigned clear_grid;             // k_planes_clear
    bool refit;                      // refit_tol > 0: clear, sum<true>, solve<true> in front of the paint
    int launches;                    // 4 or 7
    size_t scratch0, scratch1;       // bytes of pp[0] and of pp[1] this call uses (scratch1 = 0 where the caller gives d_fits)
};

// rows, cols, batch >= 1 and within the context's limits; params_ok: planes_params_ok of the call's parameters
inline PlanesPlan plan_superpixel_planes(int rows, int cols, int batch, int n_labels, size_t plane_bytes, bool params_ok, bool refit,
                                         uintptr_t depth, uintptr_t labels, uintptr_t out, uintptr_t fits)
{
    PlanesPlan p = {};
    p.status = kInvalid;
    if (!depth || !labels || !out || depth % 4 != 0 || labels % 4 != 0 || out % 4 != 0 || fits % 8 != 0 || !params_ok) return p;
    if (n_labels < 1 || n_labels > planes_max_labels(plane_bytes, batch)) return p;
    if ((uint64_t)rows * (uint64_t)cols > kPlanesMaxPixels) return p;
    const size_t px = 4 * (size_t)batch * (size_t)rows * (size_t)cols;
    p.records = (size_t)batch * (size_t)n_labels;
    const size_t fb = p.records * (size_t)kPlanesFitBytes;
    if (out != depth && ranges_overlap(depth, px, out, px)) return p;
    if (ranges_overlap(labels, px, depth, px) || ranges_overlap(labels, px, out, px)) return p;
    if (fits && (ranges_overlap(fits, fb, depth, px) || ranges_overlap(fits, fb, labels, px) || ranges_overlap(fits, fb, out, px))) return p;
    p.status = kOk;
    p.n = (uint32_t)rows * (uint32_t)cols;
    p.tiles_x = ((uint32_t)cols + kPlanesTile - 1) / kPlanesTile;
    p.tiles_y = ((uint32_t)rows + kPlanesTile - 1) / kPlanesTile;
    p.sum_grid = p.tiles_x * p.tiles_y;
    p.vec = p.n % 4 == 0 && depth % 16 == 0 && labels % 16 == 0 && out % 16 == 0 ? 4 : 1;
    p.paint_x = (p.n / (uint32_t)p.vec + 255) / 256;
    p.solve_grid = (unsigned)((p.records + 255) / 256);
    p.words = p.records * 2 * (size_t)kPlanesMomWords;
    const size_t blocks = (p.words + 255) / 256;
    p.clear_grid = blocks > 4096 ? 4096u : (unsigned)blocks;
    p.refit = refit;
    p.launches = refit ? 7 : 4;
    p.scratch0 = 4 * p.words;
    p.scratch1 = fits ? 0 : fb;
    return p;
}

// ---- dcmt_sparse_occlusion_dev, dcmt_sparse_occlusion_u16_dev --------------------------------------------------------------
// The occlusion filter of a sparse depth plane (dcmt_kernels_occlusion.h).  Out of place: one fused kernel that decides and writes.
// In place (out == sparse exactly): a neighbouring workgroup may already have zeroed a pixel of another workgroup's halo, and every
// decision is taken on the input; so k_occl<T, false> decides into a mask plane of one bit per pixel on pp[0], [frame][row][words_x]
// 32-bit words, and k_occl_apply zeroes and counts.  words_x <= cols, so the mask of a call never exceeds the borrowed plane.  A clear
// of `removed` goes in front where it is given.  The checks on the arguments are here as well, tested without a device.

// what dcmt_occlusion_params may hold (dcmt.h); the depth bounds are the planes' and come as their bits
inline bool occlusion_params_ok(int64_t rx, int64_t ry, int64_t tol_code, uint32_t valid_thresh_bits, uint32_t max_depth_bits)
{
    if (rx < 0 || rx > kOcclMaxRx || ry < 0 || ry > kOcclMaxRy || tol_code < 0 || tol_code > kOcclMaxTol) return false;
    if (valid_thresh_bits < kPlanesMinThreshBits || valid_thresh_bits >= 0x7f800000u) return false;
    return max_depth_bits >= valid_thresh_bits && max_depth_bits <= kPlanesMaxDepthBits;
}

// the payload's metres per unit: a positive finite float
inline bool occlusion_scale_ok(uint32_t scale_bits) { return scale_bits > 0u && scale_bits < 0x7f800000u; }

struct OcclusionPlan {
    int status;                      // kInvalid: a null or misaligned pointer, bad parameters, buffers that overlap
    bool in_place;                   // out == sparse: decide into the mask, then apply; else the fused kernel
    uint32_t tiles_x, tiles_y;
    unsigned grid;                   // k_occl: (grid, batch)
    uint32_t lds_bytes;              // ... its dynamic LDS
    uint32_t words_x;                // mask words per row: ceil(cols / 32)
    size_t frame_words;              // ... per frame: rows * words_x
    unsigned apply_x;                // k_occl_apply: (apply_x, batch); 0 out of place
    size_t scratch;                  // bytes of pp[0] the call uses: 4 * batch * frame_words in place, 0 out of place
    size_t plane_bytes;              // batch * rows * cols * elem: what the kernels' 64-bit offsets span
    size_t clear_bytes;              // hipMemsetAsync of removed: 4 bytes a frame (0: no counts wanted)
    int launches;                    // 1 or 2, one more with removed
};

// rows, cols, batch >= 1 and within the context's limits; elem: 4 (f32) or 2 (the payload); params_ok: occlusion_params_ok (and
// occlusion_scale_ok) of the call's parameters; removed: 0 = not wanted
inline OcclusionPlan plan_sparse_occlusion(int rows, int cols, int batch, int elem, bool params_ok, int rx, int ry, uintptr_t sparse,
                                           uintptr_t out, uintptr_t removed)
{
    OcclusionPlan p = {};
    p.status = kInvalid;
    if (!sparse || !out || !params_ok || (elem != 2 && elem != 4)) return p;
    if (sparse % (uintptr_t)elem != 0 || out % (uintptr_t)elem != 0 || removed % 4 != 0) return p;
    const size_t bytes = (size_t)elem * (size_t)batch * (size_t)rows * (size_t)cols, rb = sizeof(uint32_t) * (size_t)batch;
    if (out != sparse && ranges_overlap(sparse, bytes, out, bytes)) return p;
    if (removed && (ranges_overlap(removed, rb, sparse, bytes) || ranges_overlap(removed, rb, out, bytes))) return p;
    p.status = kOk;
    p.in_place = out == sparse;
    p.tiles_x = ((uint32_t)cols + kOcclTile - 1) / kOcclTile;
    p.tiles_y = ((uint32_t)rows + kOcclTile - 1) / kOcclTile;
    p.grid = p.tiles_x * p.tiles_y;
    p.lds_bytes = occl_lds_bytes(rx, ry);
    p.words_x = ((uint32_t)cols + 31) / 32;
    p.frame_words = (size_t)rows * p.words_x;
    p.apply_x = p.in_place ? (unsigned)((p.frame_words + 255) / 256) : 0u;
    p.scratch = p.in_place ? 4 * (size_t)batch * p.frame_words : 0;
    p.plane_bytes = bytes;
    p.clear_bytes = removed ? rb : 0;
    p.launches = (p.in_place ? 2 : 1) + (removed ? 1 : 0);
    return p;
}

// ---- dcmt_support_distance_dev, dcmt_support_distance_u16_dev ----------------------------------------------------------------
// The distance to the nearest return and the trust mask (dcmt_kernels_support.h): k_support_cols leaves the capped column distances
// of every pixel as uint16 on pp[0], [frame][row][col] (2 bytes a pixel on a plane of 4: the scratch of a call never exceeds the
// borrowed plane), k_support_rows takes the minimum along the row and writes dist2, selects into out and counts.  Two launches, in
// place or not; a clear of `beyond` goes in front where it is given.  The checks on the arguments are here as well, tested without a
// device.

// what dcmt_support_params may hold (dcmt.h); the depth bounds are the occlusion filter's
inline bool support_params_ok(int64_t max_radius, uint32_t valid_thresh_bits, uint32_t max_depth_bits)
{
    return max_radius >= 1 && max_radius <= kSupportMaxRadius && occlusion_params_ok(0, 0, 0, valid_thresh_bits, max_depth_bits);
}

struct SupportPlan {
    int status;                      // kInvalid: a null or misaligned pointer, bad parameters, outputs that do not go together, buffers that overlap
    bool in_place;                   // out == dense: k_support_rows touches only the pixels beyond the radius
    bool ballots;                    // k_support_cols keeps the rows' ballots in LDS; false: it reads the sparse plane twice
    unsigned cols_grid;              // k_support_cols: (cols_grid, batch), 64 threads
    uint32_t cols_lds;               // ... its dynamic LDS
    uint32_t tiles_x, bands, groups; // segments of 256 columns; bands of 4 rows; groups of 4 bands, one workgroup each
    unsigned rows_grid;              // k_support_rows: (rows_grid, batch) = (tiles_x * groups, batch), 256 threads
    uint32_t rows_lds;               // ... its dynamic LDS
    size_t scratch;                  // bytes of pp[0] the call uses: 2 * batch * rows * cols
    size_t plane_bytes;              // batch * rows * cols * 4: what the kernels' 64-bit offsets span on an f32 plane
    size_t clear_bytes;              // hipMemsetAsync of beyond: 4 bytes a frame (0: no counts wanted)
    int launches;                    // 2, one more with beyond
};

// rows, cols, batch >= 1 and within the context's limits; elem: 4 (f32) or 2 (the payload), of the sparse plane alone; params_ok:
// support_params_ok (and occlusion_scale_ok) of the call's parameters; dense, fallback, out, dist2, beyond: 0 = not given
inline SupportPlan plan_support_distance(int rows, int cols, int batch, int elem, bool params_ok, int max_radius, uintptr_t sparse, uintptr_t dense,
                                         uintptr_t fallback, uintptr_t out, uintptr_t dist2, uintptr_t beyond)
{
    SupportPlan p = {};
    p.status = kInvalid;
    if (!sparse || !params_ok || (elem != 2 && elem != 4)) return p;
    if ((!out && !dist2) || (out && !dense) || (fallback && !out)) return p;
    if (sparse % (uintptr_t)elem != 0 || dense % 4 != 0 || fallback % 4 != 0 || out % 4 != 0 || dist2 % 2 != 0 || beyond % 4 != 0) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols;
    const uintptr_t at[6] = {sparse, dense, fallback, out, dist2, beyond};
    const size_t bytes[6] = {(size_t)elem * px, 4 * px, 4 * px, 4 * px, 2 * px, sizeof(uint32_t) * (size_t)batch};
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j) {
            if (!at[i] || !at[j]) continue;
            if (i == 1 && j == 3 && dense == out) continue;            // the one overlap allowed: in place, exactly
            if (ranges_overlap(at[i], bytes[i], at[j], bytes[j])) return p;
        }
    p.status = kOk;
    p.in_place = out && out == dense;
    p.ballots = rows <= kSupportLdsRows;
    p.cols_grid = ((unsigned)cols + kSupportColsWave - 1) / kSupportColsWave;
    p.cols_lds = support_cols_lds_bytes(rows);
    p.tiles_x = ((uint32_t)cols + kSupportTile - 1) / kSupportTile;
    p.bands = ((uint32_t)rows + kSupportBand - 1) / kSupportBand;
    p.groups = (p.bands + kSupportGroup - 1) / kSupportGroup;
    p.rows_grid = p.tiles_x * p.groups;
    p.rows_lds = support_rows_lds_bytes(max_radius);
    p.scratch = 2 * px;
    p.plane_bytes = 4 * px;
    p.clear_bytes = beyond ? sizeof(uint32_t) * (size_t)batch : 0;
    p.launches = 2 + (beyond ? 1 : 0);
    return p;
}

// ---- dcmt_joint_bilateral_dev ---------------------------------------------------------------------------------------------
// The joint bilateral filter (dcmt_kernels_joint.h): one kernel, one workgroup per tile of 64 x 16 outputs, whatever the frame; a clear
// of `counts` goes in front where they are given.  No scratch.  Every refusal of the call that needs no context is here, tested
// without a device.

// what dcmt_joint_params may hold (dcmt.h); the depth bounds are the occlusion filter's
inline bool joint_params_ok(int64_t radius, uint32_t flags, uint32_t min_weight, uint32_t valid_thresh_bits, uint32_t max_depth_bits)
{
    return radius >= 1 && radius <= kJointMaxRadius && flags != 0u && (flags & ~kJointFlags) == 0u && min_weight >= 1u &&
           occlusion_params_ok(0, 0, 0, valid_thresh_bits, max_depth_bits);
}

struct JointPlan {
    int status;                      // kInvalid: a null or misaligned pointer, bad channels or parameters, buffers that overlap
    uint32_t tiles_x, tiles_y;       // tiles of 64 x 16 outputs
    unsigned grid;                   // k_joint: (grid, batch) = (tiles_x * tiles_y, batch), 256 threads
    uint32_t lds_bytes;              // ... its dynamic LDS (the tile with its halo; the tables are static LDS beside it)
    size_t plane_bytes;              // batch * rows * cols * 4: what the kernel's 64-bit offsets span on the depth plane
    size_t guide_bytes;              // batch * rows * cols * channels
    size_t clear_bytes;              // hipMemsetAsync of counts: 8 bytes a frame (0: no counts wanted)
    int launches;                    // 1, one more with counts
};

// rows, cols, batch >= 1 and within the context's limits; the fields of dcmt_joint_params, the two bounds as their bits; counts: 0 =
// not wanted
inline JointPlan plan_joint_bilateral(int rows, int cols, int batch, int channels, int64_t radius, uint32_t flags, uint32_t min_weight,
                                      uint32_t valid_thresh_bits, uint32_t max_depth_bits, uintptr_t depth, uintptr_t guide, uintptr_t tables,
                                      uintptr_t out, uintptr_t counts)
{
    JointPlan p = {};
    p.status = kInvalid;
    if (!depth || !guide || !tables || !out || (channels != 1 && channels != 3)) return p;
    if (!joint_params_ok(radius, flags, min_weight, valid_thresh_bits, max_depth_bits)) return p;
    if (depth % 4 != 0 || out % 4 != 0 || counts % 4 != 0 || tables % 2 != 0) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols;
    const uintptr_t at[5] = {depth, guide, tables, out, counts};
    const size_t bytes[5] = {4 * px, (size_t)channels * px, 2 * (size_t)(kJointSpace + kJointGuide), 4 * px, 2 * sizeof(uint32_t) * (size_t)batch};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            if (at[i] && at[j] && ranges_overlap(at[i], bytes[i], at[j], bytes[j])) return p;
    p.status = kOk;
    p.tiles_x = ((uint32_t)cols + kJointTileX - 1) / kJointTileX;
    p.tiles_y = ((uint32_t)rows + kJointTileY - 1) / kJointTileY;
    p.grid = p.tiles_x * p.tiles_y;
    p.lds_bytes = joint_lds_bytes((int)radius);
    p.plane_bytes = 4 * px;
    p.guide_bytes = (size_t)channels * px;
    p.clear_bytes = counts ? 2 * sizeof(uint32_t) * (size_t)batch : 0;
    p.launches = 1 + (counts ? 1 : 0);
    return p;
}

// ---- dcmt_gaussian5_dev -------------------------------------------------------------------------------------------------
struct GaussPlan {
    int strips, band_rows, bands;    // one wave per (strip of kGaussCols columns, band of band_rows rows)
    unsigned grid_x;                 // k_gauss5: (grid_x, batch), four waves per workgroup
};

inline GaussPlan plan_gauss5(int rows, int cols, int batch)
{
    GaussPlan p;
    p.strips = (cols + kGaussCols - 1) / kGaussCols;
    p.band_rows = kGaussRows;                        // shorter bands while the call makes fewer than ~2 waves per SIMD
    while (p.band_rows > 8 && (size_t)p.strips * ((rows + p.band_rows - 1) / p.band_rows) * batch < 2048) p.band_rows /= 2;
    p.bands = (rows + p.band_rows - 1) / p.band_rows;
    p.grid_x = (unsigned)(((size_t)p.strips * p.bands + 3) / 4);
    return p;
}

// ---- dcmt_bilateral5_dev, and the cascade's bilateral finish ------------------------------------------------------------------
// k_bilateral5 takes k_gauss5's shape, and its plan the same short-band rule
inline GaussPlan plan_bilateral5(int rows, int cols, int batch)
{
    GaussPlan p;
    p.strips = (cols + kBilCols - 1) / kBilCols;
    p.band_rows = kBilRows;
    while (p.band_rows > 8 && (size_t)p.strips * ((rows + p.band_rows - 1) / p.band_rows) * batch < 2048) p.band_rows /= 2;
    p.bands = (rows + p.band_rows - 1) / p.band_rows;
    p.grid_x = (unsigned)(((size_t)p.strips * p.bands + 3) / 4);
    return p;
}

// ---- dcmt_bgr_convert_dev ----------------------------------------------------------------------------------------------
// One kernel over the batch as ONE flat run of pixels (dcmt_kernels_bgr.h): nothing in it depends on where a frame ends.  Runs of
// more than kBgrSegPx pixels go in segments of kBgrSegPx, a launch each; kBgrSegPx is a multiple of 4, so every segment's three
// base pointers are as aligned as the call's and `aligned` is decided once.  A workgroup takes `passes` passes of kBgrPxPerPass
// pixels: kBgrMaxPasses, so that the copy of the Lab tables to LDS (6.5 KiB) is small against its pixels (48 KiB read), halved
// while the run makes fewer than two workgroups per CU.
// The checks on the three buffers are here as well, so that they are tested without a device: at least one output; lab may BE bgr
// (in place: every lane has read its pixels before it writes them, and no other lane reads them); any other overlap is refused.
struct BgrSegment {
    size_t first;                    // the segment's first pixel in the run
    uint32_t total;                  // its pixels
    unsigned grid;                   // k_bgr_convert: workgroups
};

struct BgrPlan {
    int status;                      // kInvalid: no output, or buffers that overlap (nothing else is meaningful then)
    size_t px;                       // pixels of the run
    size_t count;                    // segments
    uint32_t passes;                 // per workgroup
    bool aligned;                    // k_bgr_convert<.., .., true>: bgr and every output wanted are 4-byte aligned
    uint32_t share() const { return passes * kBgrPxPerPass; }        // pixels per workgroup
    BgrSegment segment(size_t i) const
    {
        BgrSegment s;
        s.first = i * (size_t)kBgrSegPx;
        s.total = px - s.first < kBgrSegPx ? (uint32_t)(px - s.first) : kBgrSegPx;
        s.grid = (unsigned)((s.total + share() - 1) / share());
        return s;
    }
};

// px = batch * rows * cols >= 1; lab_addr / gray_addr: 0 = that output is not wanted
inline BgrPlan plan_bgr_convert(size_t px, uintptr_t bgr_addr, uintptr_t lab_addr, uintptr_t gray_addr)
{
    BgrPlan p = {kInvalid, px, 0, 0, false};
    if (!bgr_addr || (!lab_addr && !gray_addr) || px < 1) return p;
    if (lab_addr && lab_addr != bgr_addr && ranges_overlap(bgr_addr, 3 * px, lab_addr, 3 * px)) return p;
    if (gray_addr && ranges_overlap(bgr_addr, 3 * px, gray_addr, px)) return p;
    if (lab_addr && gray_addr && ranges_overlap(lab_addr, 3 * px, gray_addr, px)) return p;
    p.status = kOk;
    p.count = (px + kBgrSegPx - 1) / kBgrSegPx;
    p.passes = kBgrMaxPasses;
    while (p.passes > 1 && px / p.share() < 512) p.passes /= 2;
    p.aligned = bgr_addr % 4 == 0 && lab_addr % 4 == 0 && gray_addr % 4 == 0;
    return p;
}

// ---- dcmt_crop_frames_dev ----------------------------------------------------------------------------------------------
// One launch for the whole ragged batch (dcmt_kernels_crop.h): grid (bands, frames) -- the frame is blockIdx.y, so nothing is
// multiplied up to a flat index and 65535 frames are 65535 rows of the grid.  A workgroup takes a band of `band` destination rows,
// its four waves a row at a time: kCropBandRows, so that a wave reads its frame's record once for four rows, halved while the call
// makes fewer than 1024 workgroups, and doubled while a frame has more than 2^20 bands (a grid's x dimension times the workgroup
// size stays below 2^32 for the tallest frame dcmt_create admits).  The checks on the buffers are here as well, tested without a device.
struct CropPlan {
    int status;                      // kInvalid: a null or misaligned pointer, elem outside 1..4, no source bytes, overlapping buffers
    uint32_t band;                   // destination rows per workgroup
    unsigned grid_x, grid_y;         // k_crop_frames: (bands, frames), kCropThreads threads
    size_t dst_bytes;
};

// out_rows, out_cols, batch >= 1 and within the context's limits (out_rows * out_cols <= 0x1ffffff0, batch <= 65535)
inline CropPlan plan_crop(int out_rows, int out_cols, int batch, int elem, uintptr_t src, size_t src_bytes, uintptr_t table, uintptr_t dst)
{
    CropPlan p = {kInvalid, 0, 0, 0, 0};
    if (!src || !table || !dst || elem < 1 || elem > 4 || src_bytes == 0 || table % 8 != 0) return p;
    p.dst_bytes = (size_t)batch * (size_t)out_rows * (size_t)out_cols * (size_t)elem;
    if (ranges_overlap(dst, p.dst_bytes, src, src_bytes) || ranges_overlap(dst, p.dst_bytes, table, (size_t)32 * (size_t)batch)) return p;
    p.status = kOk;
    p.band = kCropBandRows;
    const auto bands = [&] { return ((uint32_t)out_rows + p.band - 1) / p.band; };
    while (p.band > (uint32_t)kCropWaves && (size_t)bands() * (size_t)batch < 1024) p.band /= 2;
    while (bands() > (1u << 20)) p.band *= 2;
    p.grid_x = bands();
    p.grid_y = (unsigned)batch;
    return p;
}

// ---- dcmt_depth_to_u16_dev ---------------------------------------------------------------------------------------------
// One kernel over the batch as one flat run of pixels, in segments of kU16SegPx like the BGR ingest; `aligned` (eight pixels per
// access) is decided once: a segment starts 4 * kU16SegPx and 2 * kU16SegPx bytes behind the last, multiples of 16.
struct U16Segment {
    size_t first;
    uint32_t total;
    unsigned grid;
};

struct U16Plan {
    int status;                      // kInvalid: a null or misaligned pointer, buffers that overlap
    size_t px, count;
    bool aligned;                    // k_depth_to_u16<true>: both pointers 16-byte aligned
    U16Segment segment(size_t i) const
    {
        U16Segment s;
        s.first = i * (size_t)kU16SegPx;
        s.total = px - s.first < kU16SegPx ? (uint32_t)(px - s.first) : kU16SegPx;
        s.grid = (unsigned)((s.total + kU16PxPerWg - 1) / kU16PxPerWg);
        return s;
    }
};

// px = batch * rows * cols >= 1
inline U16Plan plan_depth_to_u16(size_t px, uintptr_t depth, uintptr_t out)
{
    U16Plan p = {kInvalid, px, 0, false};
    if (!depth || !out || px < 1 || depth % 4 != 0 || out % 2 != 0) return p;
    if (ranges_overlap(depth, 4 * px, out, 2 * px)) return p;
    p.status = kOk;
    p.count = (px + kU16SegPx - 1) / kU16SegPx;
    p.aligned = depth % 16 == 0 && out % 16 == 0;
    return p;
}

// ---- dcmt_rectify_map_dev, dcmt_rectify_dev ------------------------------------------------------------------------------
// The map: one kernel, a lane per element, grid (ceil(rows * cols / kRectifyThreads), n_maps).  The remap: ONE launch of k_rectify
// (dcmt_kernels_rectify.h), grid (tiles, groups, chunks).  Without an index table a group is a map and the frames that use it
// (f % n_maps), so that a workgroup reads its tile of the map once for all of them: min(n_maps, batch) groups, and the frames of a
// group are split into `chunks` runs of per_chunk while the call has fewer than kRectifyTargetWgs workgroups (one map and a large
// batch would otherwise be one round of tiles, each looping over the whole batch).  With an index table a group is a frame: nothing
// is known about the table's contents here, and the bytes are the same.  The route, LDS or gather, is the kernel's, per tile.  The
// checks on the buffers are here as well, tested without a device.
struct RectifyMapPlan {
    int status;                      // kInvalid: a null or misaligned pointer, n_maps outside 1..65535, a map that overlaps the table
    unsigned grid_x, grid_y;
    size_t map_bytes;
};

// rows, cols >= 1 and within the context's limits (rows * cols <= 0x1ffffff0)
inline RectifyMapPlan plan_rectify_map(int rows, int cols, int n_maps, uintptr_t table, uintptr_t map)
{
    RectifyMapPlan p = {kInvalid, 0, 0, 0};
    if (!table || !map || n_maps < 1 || n_maps > 65535 || table % 8 != 0 || map % 8 != 0) return p;
    const size_t n = (size_t)rows * (size_t)cols;
    p.map_bytes = 8 * n * (size_t)n_maps;
    if (ranges_overlap(map, p.map_bytes, table, (size_t)176 * (size_t)n_maps)) return p;
    p.status = kOk;
    p.grid_x = (unsigned)((n + kRectifyThreads - 1) / kRectifyThreads);
    p.grid_y = (unsigned)n_maps;
    return p;
}

struct RectifyPlan {
    int status;                      // kInvalid: see dcmt.h
    bool indexed;                    // a group is a frame and its map comes from the table
    uint32_t tiles_x, per_chunk;     // kernel arguments: tiles per tile row, frames of a group per chunk
    unsigned grid_x, grid_y, grid_z; // (tiles, groups, chunks)
    size_t src_bytes, dst_bytes, map_bytes;
};

// rows, cols, batch >= 1 and within the context's limits (batch <= 65535)
inline RectifyPlan plan_rectify(int src_rows, int src_cols, int channels, int rows, int cols, int batch, int n_maps, uint32_t flags, uintptr_t src,
                                uintptr_t map, uintptr_t index, uintptr_t dst)
{
    RectifyPlan p = {kInvalid, false, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!src || !map || !dst || (channels != 1 && channels != 3) || n_maps < 1 || (flags & ~1u) != 0) return p;
    if (src_rows < 1 || src_cols < 1 || src_rows > kRectifyMaxSrcSide || src_cols > kRectifyMaxSrcSide) return p;
    if (map % 8 != 0 || index % 4 != 0) return p;
    const size_t n = (size_t)rows * (size_t)cols;
    if ((size_t)n_maps > SIZE_MAX / 8 / n) return p;
    p.src_bytes = (size_t)batch * (size_t)src_rows * (size_t)src_cols * (size_t)channels;
    p.dst_bytes = (size_t)batch * n * (size_t)channels;
    p.map_bytes = 8 * n * (size_t)n_maps;
    if (ranges_overlap(dst, p.dst_bytes, src, p.src_bytes) || ranges_overlap(dst, p.dst_bytes, map, p.map_bytes) ||
        (index && ranges_overlap(dst, p.dst_bytes, index, sizeof(int32_t) * (size_t)batch)))
        return p;
    p.status = kOk;
    p.indexed = index != 0;
    p.tiles_x = ((uint32_t)cols + kRectifyTileW - 1) / kRectifyTileW;
    const uint32_t tiles_y = ((uint32_t)rows + kRectifyTileH - 1) / kRectifyTileH;
    p.grid_x = p.tiles_x * tiles_y;
    if (p.indexed) {
        p.grid_y = (unsigned)batch; p.grid_z = 1; p.per_chunk = 1;
        return p;
    }
    const uint32_t groups = (uint32_t)(n_maps < batch ? n_maps : batch);
    const uint32_t frames = ((uint32_t)batch + groups - 1) / groups;          // of the largest group: map 0's
    const size_t wgs = (size_t)p.grid_x * groups;
    uint32_t chunks = wgs >= kRectifyTargetWgs ? 1u : (uint32_t)((kRectifyTargetWgs + wgs - 1) / wgs);
    if (chunks > frames) chunks = frames;
    p.per_chunk = (frames + chunks - 1) / chunks;
    p.grid_y = groups;
    p.grid_z = (frames + p.per_chunk - 1) / p.per_chunk;
    return p;
}

// ---- dcmt_photo_error_dev, dcmt_photo_error_calib_dev ----------------------------------------------------------------------
// A clear of the statistics (where they are wanted) and ONE kernel (dcmt_kernels_photo.h), whatever the data.  The route depends on
// the shape and the window alone: the LDS route (k_photo_error: a workgroup stages the band's rows of both images, full width) where
// a band of at least one row fits kPhotoLdsBudget, the global route (k_photo_error_global: a thread per pixel, the taps from global
// memory) for wider frames.  The band starts at kPhotoBandRows and is halved while it does not fit, and then while the call makes
// fewer than 512 workgroups (a single frame on 256 CUs), but not below 2 rows for that: a band of b rows reads b + 2 * window - 1.
// `vec` says whether the kernels may use their wide accesses (16-byte loads of depth and images, 4-byte stores of the map): columns
// a multiple of 16, so that every row of every frame starts as aligned as its plane does, and the planes aligned.  The same bytes
// either way.  The checks on the buffers are here as well, tested without a device: every overlap between an output and an input,
// the table included, and between the two outputs, is refused.
struct PhotoPlan {
    int status;                      // kInvalid: a null input, no output, window outside 1..4, a misaligned depth plane, statistics or
                                     // table, more than 65535 frames, buffers that overlap
    bool lds_route;                  // k_photo_error<window>; otherwise k_photo_error_global
    bool vec;
    uint32_t band;                   // LDS route: output rows per workgroup
    uint32_t pitch;                  // ... bytes between staged rows
    size_t lds;                      // ... dynamic LDS: two images of photo_staged_rows(band, window) rows (0 on the global route)
    unsigned grid_x, grid_y;         // (bands, frames) or (ceil(rows * cols / kPhotoGlobalPx), frames)
    size_t clear_bytes;              // hipMemsetAsync of the statistics: 32 bytes a frame (0: no statistics wanted)
};

inline size_t photo_lds_bytes(uint32_t band, uint32_t window, uint32_t cols)
{
    return (size_t)2 * photo_staged_rows(band, window) * photo_pitch(cols);
}

// rows, cols, batch >= 1 and within the context's limits; table: 0 for the uniform call (table_call says which call it is)
inline PhotoPlan plan_photo_error(int rows, int cols, int batch, int window, uintptr_t depth, uintptr_t left, uintptr_t right, bool table_call,
                                  uintptr_t table, uintptr_t err, uintptr_t stats)
{
    PhotoPlan p = {};
    p.status = kInvalid;
    if (!depth || !left || !right || (!err && !stats) || window < 1 || window > kPhotoMaxWindow || batch > 65535) return p;
    if (depth % 4 != 0 || stats % 8 != 0) return p;
    if (table_call && !calib_table_aligned(table, 8)) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols, sb = (size_t)32 * (size_t)batch;
    const auto clear_of_inputs = [&](uintptr_t out, size_t ob) {
        return !out || (!ranges_overlap(out, ob, depth, 4 * px) && !ranges_overlap(out, ob, left, px) && !ranges_overlap(out, ob, right, px) &&
                        (!table_call || calib_table_clear_of(table, 8, batch, out, ob)));
    };
    if (!clear_of_inputs(err, px) || !clear_of_inputs(stats, sb)) return p;
    if (err && stats && ranges_overlap(err, px, stats, sb)) return p;
    p.status = kOk;
    const uint32_t w = (uint32_t)window, c = (uint32_t)cols, r = (uint32_t)rows;
    p.vec = c % 16 == 0 && depth % 16 == 0 && left % 16 == 0 && right % 16 == 0 && err % 4 == 0;
    p.grid_y = (unsigned)batch;
    p.clear_bytes = stats ? sb : 0;
    p.lds_route = photo_lds_bytes(1, w, c) <= kPhotoLdsBudget;
    if (!p.lds_route) {
        p.grid_x = (unsigned)(((size_t)r * c + kPhotoGlobalPx - 1) / kPhotoGlobalPx);
        return p;
    }
    p.band = (uint32_t)kPhotoBandRows;
    const auto bands = [&] { return (r + p.band - 1) / p.band; };
    while (photo_lds_bytes(p.band, w, c) > kPhotoLdsBudget) p.band /= 2;
    while (p.band > 2 && (size_t)bands() * (size_t)batch < 512) p.band /= 2;
    p.pitch = photo_pitch(c);
    p.lds = photo_lds_bytes(p.band, w, c);
    p.grid_x = bands();
    return p;
}

// ---- dcmt_depth_normals_dev, dcmt_depth_normals_calib_dev --------------------------------------------------------------------
// Normals and the flying-pixel filter of a depth plane (dcmt_kernels_normals.h): one kernel in k_gauss5's shape and with its short-band
// rule, one wave per (strip of kNormCols columns, band of band_rows rows).  Out of place it writes the records and the filtered
// plane itself.  In place (out == depth exactly) a neighbouring wave may already have zeroed what another still has to read, and
// every decision is taken on the input: the decisions go to a mask of one bit per pixel on pp[0], in the occlusion filter's layout
// ([frame][row][words_x] 32-bit words; words_x <= cols, so the mask never exceeds the borrowed plane), and k_occl_apply zeroes.  A
// clear of `counts` goes in front where they are given.  The checks on the arguments are here as well, tested without a device.

// what dcmt_normals_params may hold (dcmt.h), as the bits of its three floats; the depth bounds are the occlusion filter's
inline bool normals_params_ok(uint32_t min_plane_dist_bits, uint32_t valid_thresh_bits, uint32_t max_depth_bits)
{
    return min_plane_dist_bits <= kNormMaxDistBits && occlusion_params_ok(0, 0, 0, valid_thresh_bits, max_depth_bits);
}

struct NormalsPlan {
    int status;                      // kInvalid: a null or misaligned pointer, no output, bad parameters, buffers that overlap
    bool in_place;                   // out == depth: decide into the mask, then apply
    int out_mode;                    // k_normals' OUT: 0 none, 1 fused, 2 mask
    uint32_t strips, band_rows, bands;
    unsigned grid_x;                 // k_normals: (grid_x, batch), four waves per workgroup
    uint32_t words_x;                // mask words per row: ceil(cols / 32)
    unsigned apply_x;                // k_occl_apply: (apply_x, batch); 0 unless in place
    size_t scratch;                  // bytes of pp[0] the call uses: 4 * batch * rows * words_x in place, else 0
    size_t normals_bytes;            // 16 * batch * rows * cols: what the kernel's 64-bit offsets span (0 without records)
    size_t clear_bytes;              // hipMemsetAsync of counts: 8 bytes a frame (0: no counts wanted)
    int launches;                    // 1 or 2, one more with counts
};

// rows, cols, batch >= 1 and within the context's limits; params_ok: normals_params_ok, and normals_intrinsics_ok of the uniform
// call's record; normals, out, counts: 0 = not given; table: looked at in a table call only
inline NormalsPlan plan_depth_normals(int rows, int cols, int batch, bool params_ok, uintptr_t depth, bool table_call, uintptr_t table,
                                      uintptr_t normals, uintptr_t out, uintptr_t counts)
{
    NormalsPlan p = {};
    p.status = kInvalid;
    if (!depth || (!normals && !out) || !params_ok) return p;
    if (depth % 4 != 0 || normals % 16 != 0 || out % 4 != 0 || counts % 4 != 0) return p;
    if (table_call && !calib_table_aligned(table, 8)) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols;
    const uintptr_t at[4] = {depth, normals, out, counts};
    const size_t bytes[4] = {4 * px, 16 * px, 4 * px, 2 * sizeof(uint32_t) * (size_t)batch};
    for (int i = 0; i < 4; ++i) {
        if (!at[i]) continue;
        if (table_call && i > 0 && !calib_table_clear_of(table, 32, batch, at[i], bytes[i])) return p;
        for (int j = i + 1; j < 4; ++j)
            if (at[j] && !(i == 0 && j == 2 && out == depth) && ranges_overlap(at[i], bytes[i], at[j], bytes[j])) return p;
    }
    p.status = kOk;
    p.in_place = out == depth;
    p.out_mode = !out ? 0 : (p.in_place ? 2 : 1);
    p.strips = ((uint32_t)cols + kNormCols - 1) / kNormCols;
    p.band_rows = kNormRows;                         // shorter bands while the call makes fewer than ~2 waves per SIMD
    while (p.band_rows > 8 && (size_t)p.strips * (((uint32_t)rows + p.band_rows - 1) / p.band_rows) * (size_t)batch < 2048) p.band_rows /= 2;
    p.bands = ((uint32_t)rows + p.band_rows - 1) / p.band_rows;
    p.grid_x = (unsigned)(((size_t)p.strips * p.bands + 3) / 4);
    p.words_x = ((uint32_t)cols + 31) / 32;
    p.apply_x = p.in_place ? (unsigned)(((size_t)rows * p.words_x + 255) / 256) : 0u;
    p.scratch = p.in_place ? 4 * (size_t)batch * (size_t)rows * p.words_x : 0;
    p.normals_bytes = normals ? 16 * px : 0;
    p.clear_bytes = counts ? bytes[3] : 0;
    p.launches = (p.in_place ? 2 : 1) + (counts ? 1 : 0);
    return p;
}

// ---- dcmt_stereo_refine_dev ---------------------------------------------------------------------------------------------
struct StereoPlan {
    int status;                      // kInvalid: rows or batch beyond a grid's y / z dimension
    bool lds_row;                    // k_stereo_refine<true>: the right-image row fits the workgroup's LDS, one workgroup stages it and walks the whole row
    size_t lds;                      // its dynamic LDS (0 for the global variant)
    unsigned gx, gy, gz;
};

inline StereoPlan plan_stereo(int rows, int cols, int batch)
{
    if (rows > 65535 || batch > 65535) return {kInvalid, false, 0, 0, 0, 0};
    const bool lds_row = cols + 4 <= 48 * 1024;
    return {kOk, lds_row, lds_row ? (size_t)cols + 4 : 0, lds_row ? 1u : (unsigned)((cols + 255) / 256), (unsigned)rows, (unsigned)batch};
}

}  // namespace plan
}  // namespace dcmt
#pragma GCC visibility pop

#endif
