// dcmt_connect.h -- what the kernels of dcmt_kernels_connect.h and dcmt_kernels_speckle.h (compiled in dcmt_cloud.hip) share with the host code that plans
// their launches (dcmt_plan_side.h).  No HIP.
#pragma once
#include <cstdint>

namespace dcmt {

constexpr int kConnTW = 64, kConnTH = 16;       // k_conn_local: one workgroup per tile of kConnTW columns x kConnTH rows
constexpr int kConnPad = kConnTH + 1;           // its LDS arrays hold pixel (lx, ly) of the tile at lx * kConnPad + ly
constexpr int kConnStripCols = 64;              // k_conn_seed / k_conn_rank: one workgroup per strip of columns, one lane per column
constexpr int kConnWaves = 4;                   // ... its waves each walk a band of ceil(rows / kConnWaves) rows
constexpr uint32_t kConnNone = 0x7fffffffu;     // a small component's link: no labelled neighbour (the component of pixel (0, 0))
constexpr uint32_t kConnRank = 0x80000000u;     // a non-small seed's word: this bit | its label

// A pixel's key: (x << kbits) | y with 2^kbits >= rows -- ordered as the reference's scan order s = x * rows + y (column outer, row
// inner), and taken apart with a shift and a mask instead of a division.  Below 2^30 for every frame dcmt_create admits.
inline int conn_key_bits(int rows)
{
    int k = 0;
    while ((1 << k) < rows) ++k;
    return k;
}

// The tiles of a frame, the pixel pairs across their edges and the grids of the first three stages of a component labelling
// (tile-local union-find, border merge, flatten; conn_label_enqueue in dcmt_cloud.hip): the shape decides them, whatever the relation.
struct ConnGeom {
    uint32_t n;                      // pixels per frame
    uint32_t kbits;                  // conn_key_bits(rows)
    uint32_t tiles_x, tiles_y;
    unsigned local_x;                // the tile-local kernel: (tiles_x * tiles_y, batch)
    uint32_t pairs_v, pairs;         // pixel pairs across vertical tile edges, across all tile edges
    unsigned border_x;               // the border kernel: (border_x, batch); 0: one tile, no launch
    unsigned px_x;                   // k_conn_flatten (and k_conn_relabel): (px_x, batch), one thread per pixel
};

// rows, cols >= 1, a frame of fewer than 2^29 pixels
inline ConnGeom conn_geom(int rows, int cols)
{
    ConnGeom g;
    g.n = (uint32_t)rows * (uint32_t)cols;
    g.kbits = (uint32_t)conn_key_bits(rows);
    g.tiles_x = ((uint32_t)cols + kConnTW - 1) / kConnTW;
    g.tiles_y = ((uint32_t)rows + kConnTH - 1) / kConnTH;
    g.local_x = g.tiles_x * g.tiles_y;
    g.pairs_v = (g.tiles_x - 1) * (uint32_t)rows;
    g.pairs = g.pairs_v + (g.tiles_y - 1) * (uint32_t)cols;
    g.border_x = (g.pairs + 255) / 256;
    g.px_x = (g.n + 255) / 256;
    return g;
}

}  // namespace dcmt
