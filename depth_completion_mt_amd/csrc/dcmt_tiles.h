// dcmt_tiles.h -- the workgroup and tile sizes of the colourisation, BGR-ingest and SLIC kernels (dcmt_kernels_color.h,
// dcmt_kernels_bgr.h, dcmt_kernels_slic.h) that the host reads when it sizes their scratch and grids (dcmt_plan_side.h).  No HIP; each value has its one definition here.
#pragma once
#include <cstdint>

#include "dcmt_chunks.h"

namespace dcmt {

// k_color_minmax / k_color_map
constexpr int kColorThreads = 256;
constexpr int kColorGroupsPerLane = 4;
constexpr uint32_t kColorPxPerWg = 4u * kColorGroupsPerLane * kColorThreads;    // 4096 pixels per map workgroup
constexpr int kColorSlabStride = 2;                                            // floats per slab entry: min, max

// k_bgr_convert: a workgroup makes up to kBgrMaxPasses passes of kBgrPxPerPass consecutive pixels, each lane kBgrGroupsPerLane
// groups of 4 pixels per pass; a launch covers at most kBgrSegPx pixels (32-bit pixel indices, the last workgroup's overhang
// included), a multiple of a workgroup's largest share so that every segment starts as aligned as the run does
constexpr int kBgrThreads = 256;
constexpr int kBgrGroupsPerLane = 4;
constexpr uint32_t kBgrPxPerPass = 4u * kBgrGroupsPerLane * kBgrThreads;         // 4096
constexpr uint32_t kBgrMaxPasses = 4;
constexpr uint32_t kBgrSegPx = 0x7fff0000u;
static_assert(kBgrSegPx % (kBgrPxPerPass * kBgrMaxPasses) == 0 && (uint64_t)kBgrSegPx + kBgrPxPerPass * kBgrMaxPasses <= 0x80000000ull, "kBgrSegPx");

// k_slic_*
constexpr int kSlicCellCap = 4;                                     // centre indices a cell's list holds
// Tile of k_slic_assign: kSlicTW x TH pixels, TH (a template parameter) as tall as the tile's cells fit -- the staging is paid once
// per tile and a thread's runs get longer -- 64 rows = 16 per thread for steps from 16 up (at most 7 x 7 staged cells), 32 for steps
// 11 to 15 (9 x 6), 16 for the steps below (6: at most 14 x 6 = 84 of the 128 cells a tile may stage).
constexpr int kSlicTW = 64;
DCMT_HD constexpr int slic_tile_rows(int step) { return step >= 16 ? 64 : (step >= 11 ? 32 : 16); }

}  // namespace dcmt
