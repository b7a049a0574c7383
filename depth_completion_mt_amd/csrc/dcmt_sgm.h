// dcmt_sgm.h -- the constants dcmt_kernels_sgm.h (k_sgm_rows, k_sgm_cols, k_sgm_diag, k_sgm_winner) shares with its
// plan, and the plan itself (plan_sgm): the checks on the arguments of dcmt_sgm_dev / dcmt_sgm_paths_dev / dcmt_sgm_guided_dev / dcmt_sgm_cost_dev, the
// workspace layout, the chunking of the batch and the launch shapes.
// Plain C++, no HIP: the plan is tested on a CPU (tests/plan_sgm_test.cpp).
#ifndef DCMT_SGM_H
#define DCMT_SGM_H

#include <cstddef>
#include <cstdint>

#include "dcmt_plan_side.h"    // kOk, kInvalid, ranges_overlap

namespace dcmt {

constexpr int kSgmMinDisp = 16, kSgmMaxDisp = 128;      // D: a multiple of 16 in this range; D > 64: two disparities a lane
constexpr int kSgmMaxP2 = 10000;                        // S <= 4 * (6375 + p2) <= 65500 fits uint16
constexpr int kSgmMaxP2Eight = 1800;                    // eight paths: S <= 8 * (6375 + p2) <= 65400
constexpr int kSgmMaxGuideWeight = 10000;               // with a guide: 0 <= guide_weight <= this, and p2 + guide_cap <= the limit on p2
constexpr int kSgmRowThreads = 64;                      // k_sgm_rows: one wave = one row, lane = disparity
constexpr int kSgmWaves = 4;                            // k_sgm_cols, k_sgm_diag, k_sgm_winner: waves per workgroup
constexpr int kSgmSegment = 64;                         // k_sgm_winner: pixels of a row per wave, one result a lane
constexpr size_t kSgmLdsBudget = 64 * 1024;             // k_sgm_rows stages 16 bytes a column: up to 4096 columns, wider rows from global memory
constexpr uint32_t kSgmLdsPerCol = 16;                  // rows y-2..y+2 of one column, left (8 bytes: 4 + 1 used) and right (8 bytes)
constexpr uint32_t kSgmLdsPerColGuided = 18;            // GUIDED: the column's hint as well, an int16 behind the images: up to 3640 columns
constexpr int kSgmCostAbsdiff = 0, kSgmCostCensus = 1;  // DCMT_SGM_COST_*: the pixel cost of steps 1 / 2, or of steps 1c / 2c
constexpr uint32_t kSgmLdsPerColCensus = 16;            // census: the five 24-bit codes of one column of the right image in a uint4 (the left
                                                        // image's stay in registers): up to 4096 columns, as many workgroups a CU as with absolute differences
constexpr uint32_t kSgmLdsPerColCensusGuided = 18;      // and the column's int16 hint behind them: up to 3640 columns

namespace plan {

// bytes of one frame's two volumes (C and S, uint16 [rows][cols][D] each), a multiple of 16 since D is one
inline size_t sgm_frame_bytes(int rows, int cols, int disparities)
{
    return (size_t)4 * (size_t)rows * (size_t)cols * (size_t)disparities;
}

inline bool sgm_disparities_ok(int d) { return d >= kSgmMinDisp && d <= kSgmMaxDisp && d % 16 == 0; }
inline bool sgm_paths_ok(int paths) { return paths == 4 || paths == 8; }
inline int sgm_max_p2(int paths) { return paths == 8 ? kSgmMaxP2Eight : kSgmMaxP2; }

struct SgmPlan {
    int status;                      // kInvalid: see dcmt.h's list for dcmt_sgm_dev (the float parameters are the caller's check)
    size_t frame_bytes;              // one frame of the workspace
    size_t volume_elems;             // uint16 elements of one volume of one frame: S of frame f starts volume_elems behind its C
    int chunk;                       // frames per chunk: min(batch, frames work_bytes holds, 65535)
    int n_chunks;                    // ceil(batch / chunk); chunk i covers frames [i * chunk, min(batch, (i + 1) * chunk))
    int per_lane;                    // disparities a lane carries: 1 (D <= 64) or 2
    bool lds_route;                  // k_sgm_rows stages its five rows in LDS; otherwise it reads them from global memory
    size_t lds;                      // its dynamic LDS bytes (0 on the global route)
    unsigned rows_grid_x;            // k_sgm_rows: (rows, frames of the chunk), kSgmRowThreads threads
    unsigned cols_grid_x;            // k_sgm_cols: (ceil(cols / kSgmWaves), frames), 64 * kSgmWaves threads, a wave a column
    unsigned winner_grid_x;          // k_sgm_winner: (ceil(rows * ceil(cols / kSgmSegment) / kSgmWaves), frames), a wave a segment
    unsigned segments;               // ceil(cols / kSgmSegment)
    int paths;                       // 4, or 8: k_sgm_diag runs twice between k_sgm_cols and k_sgm_winner, once per orientation
    unsigned diag_grid_x;            // k_sgm_diag: (ceil(cols / kSgmWaves), frames), 64 * kSgmWaves threads, a wave a start column; 0 with 4 paths
    bool guided;                     // a guide was given: the GUIDED instances of k_sgm_rows, kSgmLdsPerColGuided bytes a column
    int guide_weight, guide_cap;     // its penalty min(guide_weight * |d - h|, guide_cap); 0, 0 without a guide
    int cost;                        // kSgmCostAbsdiff, or kSgmCostCensus: k_sgm_rows' COST, with census kSgmLdsPerColCensus(Guided) bytes a column
};

// the LDS bytes a column of the rows kernel of (cost, guided)
inline uint32_t sgm_lds_per_col(int cost, bool guided)
{
    if (cost == kSgmCostCensus) return guided ? kSgmLdsPerColCensusGuided : kSgmLdsPerColCensus;
    return guided ? kSgmLdsPerColGuided : kSgmLdsPerCol;
}

// frames of chunk i
inline int sgm_chunk_frames(const SgmPlan& p, int batch, int i)
{
    const long long first = (long long)i * p.chunk;
    return (int)(first + p.chunk <= batch ? p.chunk : batch - first);
}

// rows, cols, batch >= 1 and within the context's limits; paths: 4 (dcmt_sgm_dev) or 8 (the four diagonals as well); guide: the f32
// depth plane of dcmt_sgm_guided_dev or 0, without which guide_weight and guide_cap are not looked at; cost: dcmt_sgm_cost_dev's, with
// kSgmCostAbsdiff every field is what it was before there was a choice
inline SgmPlan plan_sgm(int rows, int cols, int batch, int disparities, int p1, int p2, int uniqueness, uintptr_t left, uintptr_t right,
                        uintptr_t disp16, uintptr_t depth, uintptr_t work, size_t work_bytes, int paths = 4, uintptr_t guide = 0,
                        int guide_weight = 0, int guide_cap = 0, int cost = kSgmCostAbsdiff)
{
    SgmPlan p = {};
    p.status = kInvalid;
    if (!left || !right || (!disp16 && !depth) || !work || !sgm_disparities_ok(disparities) || !sgm_paths_ok(paths)) return p;
    if (cost != kSgmCostAbsdiff && cost != kSgmCostCensus) return p;
    if (p1 < 0 || p1 > p2 || p2 > sgm_max_p2(paths) || uniqueness < 0 || uniqueness > 100) return p;
    if (disp16 % 2 != 0 || depth % 4 != 0 || work % 16 != 0) return p;
    if (guide && (guide % 4 != 0 || guide_weight < 0 || guide_weight > kSgmMaxGuideWeight || guide_cap < 0 ||
                  (long long)p2 + (long long)guide_cap > (long long)sgm_max_p2(paths)))
        return p;
    p.frame_bytes = sgm_frame_bytes(rows, cols, disparities);
    if (work_bytes < p.frame_bytes) return p;
    const size_t px = (size_t)batch * (size_t)rows * (size_t)cols;
    const uintptr_t at[6] = {left, right, guide, disp16, depth, work};
    const size_t bytes[6] = {px, px, 4 * px, 2 * px, 4 * px, work_bytes};
    for (int i = 0; i < 6; ++i)
        for (int j = (i < 3 ? 3 : i + 1); j < 6; ++j)         // the inputs may share memory; every other pair is apart
            if (at[i] && at[j] && ranges_overlap(at[i], bytes[i], at[j], bytes[j])) return p;
    p.status = kOk;
    p.volume_elems = p.frame_bytes / 4;
    const size_t fit = work_bytes / p.frame_bytes;
    p.chunk = (int)(fit < (size_t)batch ? fit : (size_t)batch);
    if (p.chunk > 65535) p.chunk = 65535;
    p.n_chunks = (batch + p.chunk - 1) / p.chunk;
    p.per_lane = disparities > 64 ? 2 : 1;
    p.guided = guide != 0;
    p.guide_weight = p.guided ? guide_weight : 0;
    p.guide_cap = p.guided ? guide_cap : 0;
    p.cost = cost;
    const size_t lds = (size_t)sgm_lds_per_col(cost, p.guided) * (size_t)cols;
    p.lds_route = lds <= kSgmLdsBudget;
    p.lds = p.lds_route ? lds : 0;
    p.rows_grid_x = (unsigned)rows;
    p.cols_grid_x = ((unsigned)cols + kSgmWaves - 1) / kSgmWaves;
    p.segments = ((unsigned)cols + kSgmSegment - 1) / kSgmSegment;
    p.winner_grid_x = (unsigned)(((uint64_t)rows * p.segments + kSgmWaves - 1) / kSgmWaves);
    p.paths = paths;
    p.diag_grid_x = paths == 8 ? p.cols_grid_x : 0;
    return p;
}

}  // namespace plan
}  // namespace dcmt

#endif
