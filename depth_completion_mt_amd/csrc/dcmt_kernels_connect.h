// dcmt_kernels_connect.h -- Slic::create_connectivity (DC_lidar_camera/slic.cpp:186-254, called at main_lc.cpp:202) as include/dcmt.h
// states it, batched on the device: the 4-connected components of the label plane, and for each either a fresh label in the scan
// order of its seed (its pixel that the reference's scan meets first) or, where it is small, the final label of a neighbour of its
// seed.  Integer arithmetic throughout: the result is the same bits whatever the batch, the launch geometry or the run.
//
// Keys.  Pixel (x, y) has the key (x << kbits) | y, 2^kbits >= rows (dcmt_connect.h): ordered as the reference's scan (column outer,
// row inner), taken apart without a division.  The planes are row-major like the labels; what they HOLD are keys.
//
// Two scratch planes of one word per pixel, A and B (the context's pp[0] and pp[1]), and a slab of one word per (frame, strip).  The
// first two kernels are conn_local_body and conn_border_body under the relation "equal labels" (ConnLabelRel, below); the speckle
// filter (dcmt_kernels_speckle.h) runs the same bodies under its own relation, and k_conn_flatten as it is.
//   k_conn_local    one workgroup per tile of 64 x 16 pixels: union-find in LDS over the tile's pixels.  A[p] = the key of the
//                   smallest pixel of p's component WITHIN the tile; B[p] = that component's pixel count at that pixel, 0 elsewhere.
//   k_conn_border   one thread per pair of pixels across a tile edge: equal labels -> union of the two trees in A, the larger
//                   root pointed at the smaller with atomicMin.  A root is therefore its component's smallest key: its seed.  A
//                   pair whose neighbour one step back along the edge, in the same tiles, has the same label on both sides is
//                   left out: that pair joins the same two tile components.
//   k_conn_flatten  one thread per pixel, of which the tile-local roots (B[p] != 0) work: A[p] = the root, and the tile's count
//                   moves to the root, one integer add per (tile, component) -- the counting inside a tile was done in LDS, per
//                   wave first.  From here on a pixel's root is two plain loads away: A[p] is its tile's root or the root, and
//                   A of that is the root (conn_root).
//   k_conn_seed     one workgroup per strip of 64 columns, lane = column, four waves a quarter of the rows each: a pixel with
//                   A[p] == its own key is a seed (a root keeps its own key; every other pixel holds a smaller one).  count =
//                   size + (size >= 2); small iff count <= lims >> 2.  A small seed's B word becomes its link: the root of the
//                   LAST of its neighbours (x-1, y), (x, y-1), (x+1, y), (x, y+1) whose root is smaller than the seed, or
//                   kConnNone; a non-small seed's becomes kConnRank.  The strip's number of non-small seeds goes to the slab.
//   k_conn_scan     one workgroup per frame: the exclusive scan of the frame's strip counts, and d_counts.
//   k_conn_rank     the walk of k_conn_seed again: a non-small seed's B word becomes kConnRank | its rank among the frame's
//                   non-small seeds in key order = strip base + the columns in front of it in the strip + the rows above it.
//   k_conn_relabel  one thread per pixel: root -> links -> rank, stored to d_out.  The only writer of d_out, and it reads no labels:
//                   d_out may be d_labels.
// Labels and planes are walked with lanes along a row, so every wave access is one run of consecutive words; the column-major
// order of the scan lives in the keys, in a lane's own running count down its column (registers) and in the sums across a strip's
// columns (LDS, shuffles).  The one exception are the pairs across vertical tile edges (rows * (tiles_x - 1) pairs, 1.5 % of a
// 352 x 1216 frame), whose lanes run down a column.
//
// Words another workgroup may write in the same launch are only ever touched by atomics in that launch: A in k_conn_border
// (atomicMin, agent-scope atomic loads) and in k_conn_flatten (agent-scope atomic loads and stores; whichever of a word's old
// and new value a walk sees is an ancestor), B in k_conn_flatten (atomicAdd to the roots' words, agent-scope atomic loads).
// Everything else is read in a later launch than it is written.  No workgroup waits for another: there is no spin, flag
// or ordered hand-off, and every loop steps to a strictly smaller key (or clears a bit of a mask), as the comment at each says.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcmt_connect.h"

namespace dcmt {

constexpr int kConnLds = kConnTW * kConnPad;

__device__ __forceinline__ uint32_t conn_key(uint32_t x, uint32_t y, uint32_t kbits) { return (x << kbits) | y; }
// the row-major index of the pixel a key names
__device__ __forceinline__ size_t conn_px(uint32_t key, uint32_t kbits, uint32_t cols)
{
    return (size_t)(key & ((1u << kbits) - 1u)) * cols + (key >> kbits);
}

__device__ __forceinline__ uint32_t conn_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void conn_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of key k in the frame's plane A.  Ends: a pixel's word never exceeds its own key (it starts as a key of its tile's
// component that is <= its own and is only ever lowered, by atomicMin or to an ancestor), and every step goes to a strictly smaller key.
__device__ __forceinline__ uint32_t conn_find(const uint32_t* A, uint32_t k, uint32_t kbits, uint32_t cols)
{
    for (;;) {
        const uint32_t p = conn_load(A + conn_px(k, kbits, cols));
        if (p >= k) return k;
        k = p;
    }
}

// Joins the trees of keys a and b in A.  Ends: with a > b, atomicMin(A[a], b) either found a a root (old == a: done) or returns
// a's parent old < a, which still has to be joined to b -- and max(old, b) < a, so the larger key of the pair falls with every pass.
__device__ __forceinline__ void conn_unite(uint32_t* A, uint32_t a, uint32_t b, uint32_t kbits, uint32_t cols)
{
    a = conn_find(A, a, kbits, cols);
    b = conn_find(A, b, kbits, cols);
    while (a != b) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(A + conn_px(a, kbits, cols), b);
        if (old >= a) break;
        a = old;
    }
}

// the same two in a tile's LDS array P, whose words hold LDS indices (lx * kConnPad + ly: ordered as the keys)
__device__ __forceinline__ uint32_t conn_lds_find(const uint32_t* P, uint32_t u)
{
    for (;;) {                                             // ends: every step goes to a strictly smaller index
        const uint32_t p = __hip_atomic_load(P + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p >= u) return u;
        u = p;
    }
}

__device__ __forceinline__ void conn_lds_unite(uint32_t* P, uint32_t a, uint32_t b)
{
    a = conn_lds_find(P, a);
    b = conn_lds_find(P, b);
    while (a != b) {                                       // ends: as conn_unite
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(P + a, b);
        if (old >= a) break;
        a = old;
    }
}

// C[r] += 1 for every active lane, lanes with the same r first summed in the wave: one LDS add per distinct r.  Called by whole waves.
__device__ __forceinline__ void conn_count(uint32_t* C, uint32_t r, bool active)
{
    const uint32_t l = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo != 0) {                                    // ends: every pass clears at least the lowest bit of todo that is set
        const uint32_t first = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t rr = (uint32_t)__shfl((int)r, (int)first, 64);
        const unsigned long long same = __ballot(active && r == rr) & todo;
        if (l == first) atomicAdd(C + rr, (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// The first two stages are written once, over the RELATION under which 4-neighbours are joined.  A relation R supplies
//   R::Src                   the element type of the source plane
//   int32_t word(Src)        a loaded element as the word a tile's LDS holds
//   bool live(int32_t)       whether an in-frame pixel with that word takes part; one that does not is a singleton that joins nothing
//                            and counts nothing: its B word stays 0, so k_conn_flatten passes it by
//   bool edge(int32_t a, int32_t b)   on the words of two in-frame 4-neighbours: both take part and are joined
// and the bodies decide "inside the frame" themselves (no word is set aside for it: a label may be any int32_t).  An edge need not be
// transitive (|a - b| <= max_diff is not), so whatever concludes "these two are joined already" does so from EDGES, never from one
// pixel's value compared all round: [[-32, 32], [0, 0]] at max_diff 32 is one component whose top pair is no edge.
struct ConnLabelRel {                                      // equal labels; every in-frame pixel takes part
    using Src = int32_t;
    __device__ __forceinline__ int32_t word(int32_t s) const { return s; }
    __device__ __forceinline__ bool live(int32_t) const { return true; }
    __device__ __forceinline__ bool edge(int32_t a, int32_t b) const { return a == b; }
};

// The tile-local stage.  grid (tiles_x * tiles_y, frames), 256 threads: lane = column of the tile, wave w its rows 4w .. 4w + 3
template <class R>
__device__ __forceinline__ void conn_local_body(const R rel, const typename R::Src* __restrict__ src, uint32_t rows, uint32_t cols, uint32_t tiles_x,
                                                uint32_t kbits, uint32_t* __restrict__ A, uint32_t* __restrict__ B)
{
    __shared__ int32_t L[kConnLds];
    __shared__ uint32_t P[kConnLds];
    __shared__ uint32_t C[kConnLds];
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x0 = tx * kConnTW, y0 = ty * kConnTH;
    const uint32_t lx = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t gx = x0 + lx;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    int32_t v[4];
    bool in[4];
    uint32_t r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ly = 4 * w + i, gy = y0 + ly, u = lx * kConnPad + ly;
        in[i] = gx < cols && gy < rows;
        v[i] = in[i] ? rel.word(src[fo + (size_t)gy * cols + gx]) : 0;      // (nobody asks for the word of a pixel outside the frame)
        L[u] = v[i];
        C[u] = 0u;
    }
    __syncthreads();
    // a column's runs as chains: a pixel points at the pixel above it where the two are an edge (the pixel above an inside pixel
    // of the tile is inside) ...
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ly = 4 * w + i, u = lx * kConnPad + ly;
        P[u] = in[i] && ly > 0 && rel.edge(v[i], L[u - 1]) ? u - 1 : u;
    }
    __syncthreads();
    // ... and then at the head of its run: walked while nobody writes, stored behind the barrier
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t u = lx * kConnPad + 4 * w + i;
        for (;;) {                                         // ends: every step goes one pixel up the column
            const uint32_t p = P[u];
            if (p >= u) break;
            u = p;
        }
        r[i] = u;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) P[lx * kConnPad + 4 * w + i] = r[i];
    __syncthreads();
    // the runs of neighbouring columns (the pixel to the left of an inside pixel of the tile is inside)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t u = lx * kConnPad + 4 * w + i;
        if (!in[i] || lx == 0 || !rel.edge(v[i], L[u - kConnPad])) continue;
        // Not where u-up, up-upleft and upleft-left are edges: u and left are joined through them, u-up and upleft-left by the
        // column chains, up-upleft by its own union or, by induction up the column, by this same argument.  (Under ==, with u-left
        // an edge, the third test follows from the other two.)
        if (4 * w + i > 0 && rel.edge(v[i], L[u - 1]) && rel.edge(L[u - 1], L[u - kConnPad - 1]) &&
            rel.edge(L[u - kConnPad - 1], L[u - kConnPad]))
            continue;
        conn_lds_unite(P, u, u - kConnPad);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = conn_lds_find(P, lx * kConnPad + 4 * w + i);
        conn_count(C, r[i], in[i] && rel.live(v[i]));
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ly = 4 * w + i, u = lx * kConnPad + ly;
        if (in[i]) {
            const uint32_t rx = r[i] / kConnPad, ry = r[i] - rx * kConnPad;
            const size_t p = fo + (size_t)(y0 + ly) * cols + gx;
            A[p] = conn_key(x0 + rx, y0 + ry, kbits);
            B[p] = r[i] == u ? C[u] : 0u;                  // (a pixel that takes no part is its own root with a count of 0)
        }
    }
}

// The border stage.  grid (ceil(pairs / 256), frames), 256 threads.  Pair j < pairs_v: edge j / rows between tile columns, row
// j % rows; the others: edge / cols between tile rows, column % cols
template <class R>
__device__ __forceinline__ void conn_border_body(const R rel, const typename R::Src* __restrict__ src, uint32_t rows, uint32_t cols, uint32_t pairs_v,
                                                 uint32_t pairs, uint32_t kbits, uint32_t* A)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= pairs) return;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    uint32_t xa, ya, xb, yb;
    size_t back;                                           // the pair one step back along the edge, where it lies in the same two tiles (else 0)
    if (j < pairs_v) {
        const uint32_t e = j / rows;
        ya = yb = j - e * rows;
        xb = (e + 1) * kConnTW;
        xa = xb - 1;
        back = ya % kConnTH != 0 ? cols : 0;
    } else {
        const uint32_t jj = j - pairs_v, e = jj / cols;
        xa = xb = jj - e * cols;
        yb = (e + 1) * kConnTH;
        ya = yb - 1;
        back = xa % kConnTW != 0 ? 1 : 0;
    }
    const size_t pa = fo + (size_t)ya * cols + xa, pb = fo + (size_t)yb * cols + xb;
    const int32_t a = rel.word(src[pa]), b = rel.word(src[pb]);
    if (!rel.edge(a, b)) return;
    if (back != 0) {
        // Not where pa-pa', pb-pb' and pa'-pb' are edges: pa-pa' and pb-pb' are joined inside their tiles, pa'-pb' by its own union
        // or, by induction along the edge, by this same argument.  (Under ==, the third test follows from pa-pb and the other two.)
        const int32_t a1 = rel.word(src[pa - back]), b1 = rel.word(src[pb - back]);
        if (rel.edge(a, a1) && rel.edge(b, b1) && rel.edge(a1, b1)) return;
    }
    conn_unite(A + fo, conn_key(xa, ya, kbits), conn_key(xb, yb, kbits), kbits, cols);
}

__global__ __launch_bounds__(256)
void k_conn_local(const int32_t* __restrict__ labels, uint32_t rows, uint32_t cols, uint32_t tiles_x, uint32_t kbits,
                  uint32_t* __restrict__ A, uint32_t* __restrict__ B)
{
    conn_local_body(ConnLabelRel{}, labels, rows, cols, tiles_x, kbits, A, B);
}

__global__ __launch_bounds__(256)
void k_conn_border(const int32_t* __restrict__ labels, uint32_t rows, uint32_t cols, uint32_t pairs_v, uint32_t pairs, uint32_t kbits,
                   uint32_t* A)
{
    conn_border_body(ConnLabelRel{}, labels, rows, cols, pairs_v, pairs, kbits, A);
}

// grid (ceil(n / 256), frames), 256 threads
__global__ __launch_bounds__(256)
void k_conn_flatten(uint32_t n, uint32_t cols, uint32_t kbits, uint32_t* A, uint32_t* B)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const size_t fo = (size_t)blockIdx.y * n;
    const uint32_t size = conn_load(B + fo + p);           // != 0: the root of a tile's component (a root's own word may be growing: any value of it is != 0)
    if (size == 0u) return;
    const uint32_t y = p / cols, x = p - y * cols, own = conn_key(x, y, kbits);
    const uint32_t r = conn_find(A + fo, own, kbits, cols);
    if (r == own) return;                                  // a root: its words are the ones the others add to and walk to
    conn_store(A + fo + p, r);
    atomicAdd(B + fo + conn_px(r, kbits, cols), size);
}

// the root of the pixel at row-major index i of a frame, behind k_conn_flatten
__device__ __forceinline__ uint32_t conn_root(const uint32_t* __restrict__ a, size_t i, uint32_t kbits, uint32_t cols)
{
    return a[conn_px(a[i], kbits, cols)];
}

// the band of wave w and the column of lane l of a strip's workgroup
struct ConnWalk { uint32_t x, y0, y1; bool active; };
__device__ __forceinline__ ConnWalk conn_walk(uint32_t rows, uint32_t cols, uint32_t band_rows)
{
    ConnWalk k;
    const uint32_t w = threadIdx.x >> 6;
    k.x = blockIdx.x * kConnStripCols + (threadIdx.x & 63);
    k.active = k.x < cols;
    k.y0 = min(w * band_rows, rows);
    k.y1 = min(k.y0 + band_rows, rows);
    return k;
}

constexpr int kConnBatch = 8;       // rows whose loads go out together

// grid (strips, frames), 256 threads.  slab: [frames][strips]
__global__ __launch_bounds__(256)
void k_conn_seed(const uint32_t* __restrict__ A, uint32_t* __restrict__ B, uint32_t rows, uint32_t cols, uint32_t kbits, uint32_t band_rows,
                 uint32_t lim4, uint32_t* __restrict__ slab)
{
    __shared__ uint32_t wsum[kConnWaves];
    const ConnWalk k = conn_walk(rows, cols, band_rows);
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const uint32_t* __restrict__ a = A + fo;
    uint32_t* __restrict__ b = B + fo;
    uint32_t cnt = 0;
    for (uint32_t yb = k.y0; yb < k.y1; yb += kConnBatch) {
        uint32_t v[kConnBatch];
#pragma unroll
        for (int j = 0; j < kConnBatch; ++j) v[j] = k.active && yb + j < k.y1 ? a[(size_t)(yb + j) * cols + k.x] : 0xffffffffu;
#pragma unroll
        for (int j = 0; j < kConnBatch; ++j) {
            const uint32_t y = yb + j, own = conn_key(k.x, y, kbits);
            if (v[j] != own) continue;                     // (0xffffffff is no key)
            const size_t p = (size_t)y * cols + k.x;
            const uint32_t size = b[p], count = size + (size >= 2u ? 1u : 0u);
            if (count > lim4) { b[p] = kConnRank; ++cnt; continue; }
            uint32_t link = kConnNone, r;
            if (k.x > 0 && (r = conn_root(a, p - 1, kbits, cols)) < own) link = r;
            if (y > 0 && (r = conn_root(a, p - cols, kbits, cols)) < own) link = r;
            if (k.x + 1 < cols && (r = conn_root(a, p + 1, kbits, cols)) < own) link = r;
            if (y + 1 < rows && (r = conn_root(a, p + cols, kbits, cols)) < own) link = r;
            b[p] = link;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int i = 0; i < kConnWaves; ++i) s += wsum[i];
        slab[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// grid (frames), 256 threads: slab [frames][strips] counts in, exclusive bases out; counts: [frames] or null
__global__ __launch_bounds__(256)
void k_conn_scan(uint32_t* __restrict__ slab, uint32_t strips, int32_t* __restrict__ counts)
{
    __shared__ uint32_t ws[4];
    uint32_t* __restrict__ s = slab + (size_t)blockIdx.x * strips;
    const uint32_t l = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t run = 0;
    for (uint32_t base = 0; base < strips; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < strips ? s[i] : 0u;
        uint32_t inc = v;
        for (int m = 1; m < 64; m <<= 1) { const uint32_t o = __shfl_up(inc, m, 64); if ((int)l >= m) inc += o; }
        if (l == 63) ws[w] = inc;
        __syncthreads();
        uint32_t front = 0, total = 0;
        for (uint32_t j = 0; j < 4; ++j) { if (j < w) front += ws[j]; total += ws[j]; }
        if (i < strips) s[i] = run + front + inc - v;
        run += total;
        __syncthreads();
    }
    if (threadIdx.x == 0 && counts) counts[blockIdx.x] = (int32_t)run;
}

// grid (strips, frames), 256 threads.  slab: the bases k_conn_scan left
__global__ __launch_bounds__(256)
void k_conn_rank(uint32_t* __restrict__ B, uint32_t rows, uint32_t cols, uint32_t band_rows, const uint32_t* __restrict__ slab)
{
    __shared__ uint32_t cc[kConnWaves][64];
    const ConnWalk k = conn_walk(rows, cols, band_rows);
    const uint32_t l = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t* __restrict__ b = B + (size_t)blockIdx.y * rows * cols;
    uint32_t cnt = 0;
    for (uint32_t yb = k.y0; yb < k.y1; yb += kConnBatch) {
        uint32_t v[kConnBatch];
#pragma unroll
        for (int j = 0; j < kConnBatch; ++j) v[j] = k.active && yb + j < k.y1 ? b[(size_t)(yb + j) * cols + k.x] : 0u;
#pragma unroll
        for (int j = 0; j < kConnBatch; ++j) cnt += v[j] >> 31;
    }
    cc[w][l] = cnt;
    __syncthreads();
    // the seeds in the columns in front of this one, and above this band in this column
    uint32_t column = 0, above = 0;
    for (uint32_t i = 0; i < (uint32_t)kConnWaves; ++i) { column += cc[i][l]; if (i < w) above += cc[i][l]; }
    uint32_t inc = column;
    for (int m = 1; m < 64; m <<= 1) { const uint32_t o = __shfl_up(inc, m, 64); if ((int)l >= m) inc += o; }
    uint32_t rank = slab[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + inc - column + above;
    if (cnt == 0u) return;
    for (uint32_t y = k.y0; y < k.y1; ++y) {
        const size_t p = (size_t)y * cols + k.x;
        if (b[p] >> 31) b[p] = kConnRank | rank++;
    }
}

// grid (ceil(n / 256), frames), 256 threads
__global__ __launch_bounds__(256)
void k_conn_relabel(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, uint32_t n, uint32_t cols, uint32_t kbits,
                    int32_t* __restrict__ out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const size_t fo = (size_t)blockIdx.y * n;
    uint32_t r = conn_root(A + fo, p, kbits, cols), label;
    for (;;) {                                             // ends: a link is a key strictly smaller than its seed's; anything else stops the walk
        const uint32_t v = B[fo + conn_px(r, kbits, cols)];
        if (v & kConnRank) { label = v & ~kConnRank; break; }
        if (v >= r) { label = 0u; break; }                 // kConnNone: the small component of pixel (0, 0) keeps the reference's initial 0
        r = v;
    }
    out[fo + p] = (int32_t)label;
}

}  // namespace dcmt
