// dcmt_kernels_sgm.h -- semi-global stereo matching as include/dcmt.h states it (dcmt_sgm_dev), three kernels per chunk of frames
// (five launches with eight paths):
//   k_sgm_rows    one wave per image row, lane = disparity (D = 128: lanes carry d and d + 64).  The grey rows y-2..y+2 of both images
//                 are staged in LDS, packed by column (four rows in one dword, the fifth in the next), so that the column sum of
//                 absolute differences of one (x, d) is two v_sad_u8; the 5-column box runs along the row in registers.  C is written,
//                 the left->right path is carried in registers and written as S; then the wave walks back over the C it has just
//                 written (every lane reads what it wrote itself) and adds the right->left path into S.
//                 Template parameters choose the variant, <NPL, LDS, GUIDED, COST>.  GUIDED (dcmt_sgm_guided_dev): the row's hints are
//                 staged behind the columns as int16, and the capped penalty joins the block cost before the path and the store, so C
//                 holds C' for every later pass.  COST = kSgmCostCensus (dcmt_sgm_cost_dev, DCMT_SGM_COST_CENSUS): the staging loop makes
//                 the 24-bit census codes of rows y-2..y+2 of the right image from its grey rows y-4..y+4, five codes of a column in one
//                 uint4 in LDS; the left image's stay in registers, 64 columns at a time; the column sum of Hamming distances of one
//                 (x, d) is four v_xor and four v_bcnt; 10 * the box is the block cost.
//   k_sgm_cols    one wave per image column: down, then up, adding both paths into S.
//   k_sgm_diag    with eight paths (dcmt_sgm_paths_dev), twice between k_sgm_cols and k_sgm_winner, once per orientation of the
//                 diagonals: one wave per start column on a line that wraps around the frame's sides, down, then up.
//   k_sgm_winner  one wave per 64 pixels of a row, four pixels in flight: steps 4..9 of the definition; the right disparity is a strided
//                 read of S.  Lane i keeps pixel i's result, so the outputs are stored coalesced.
// A path step is two DPP wave shifts (the neighbours d-1, d+1), a DPP min-scan whose result is read from lane 63, and four v_min.
// Volumes are uint16 [y][x][d], d innermost: a wave's access is one contiguous 2 D-byte run in every kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dcmt_sgm.h"

namespace dcmt {

constexpr int kSgmAbsent = 1 << 24;          // a disparity that does not exist: larger than any L_r + p2, small enough to add to

struct SgmK {                                // the scalars of the winner kernel
    int disparities, uniqueness, disp12;
    float bf, max_depth;                     // baseline * focal, rounded once
};

__device__ __forceinline__ int sgm_lane() { return (int)(threadIdx.x & 63u); }

// lane i <- lane i - 1 (lane 0 keeps `edge`), lane i <- lane i + 1 (lane 63 keeps `edge`)
__device__ __forceinline__ int sgm_from_below(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138 /*wave_shr:1*/, 0xf, 0xf, false); }
__device__ __forceinline__ int sgm_from_above(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x130 /*wave_shl:1*/, 0xf, 0xf, false); }

// the minimum over the wave, in every lane: a DPP scan inside each row of 16, two row broadcasts, lane 63 read back
__device__ __forceinline__ unsigned sgm_wave_min(unsigned v)
{
    int x = (int)v;
#define DCMT_SGM_MIN_STEP(ctrl, rows) x = (int)min((unsigned)x, (unsigned)__builtin_amdgcn_update_dpp(x, x, ctrl, rows, 0xf, false))
    DCMT_SGM_MIN_STEP(0x111 /*row_shr:1*/, 0xf);
    DCMT_SGM_MIN_STEP(0x112 /*row_shr:2*/, 0xf);
    DCMT_SGM_MIN_STEP(0x114 /*row_shr:4*/, 0xf);
    DCMT_SGM_MIN_STEP(0x118 /*row_shr:8*/, 0xf);
    DCMT_SGM_MIN_STEP(0x142 /*row_bcast:15*/, 0xa);
    DCMT_SGM_MIN_STEP(0x143 /*row_bcast:31*/, 0xc);
#undef DCMT_SGM_MIN_STEP
    return (unsigned)__builtin_amdgcn_readlane(x, 63);
}

// One path of one wave: prev[k] is L_r of the previous pixel for disparity lane + 64 k (kSgmAbsent where that is >= D).
template <int NPL>
struct SgmPath {
    int prev[NPL];
    // the first pixel of a path
    __device__ __forceinline__ void start(const int (&c)[NPL])
    {
#pragma unroll
        for (int k = 0; k < NPL; ++k) prev[k] = c[k];
    }
    // every other pixel: c[k] is C of this pixel (kSgmAbsent for an absent disparity); prev becomes this pixel's L_r
    __device__ __forceinline__ void step(const int (&c)[NPL], int p1, int p2)
    {
        unsigned mm = (unsigned)prev[0];
#pragma unroll
        for (int k = 1; k < NPL; ++k) mm = min(mm, (unsigned)prev[k]);
        const int m = (int)sgm_wave_min(mm);
        int next[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int below_edge = k > 0 ? __builtin_amdgcn_readlane(prev[k > 0 ? k - 1 : 0], 63) : kSgmAbsent;
            const int above_edge = k + 1 < NPL ? __builtin_amdgcn_readlane(prev[k + 1 < NPL ? k + 1 : k], 0) : kSgmAbsent;
            const int lo = sgm_from_below(prev[k], below_edge) + p1;
            const int hi = sgm_from_above(prev[k], above_edge) + p1;
            const int best = min(min(prev[k], m + p2), min(lo, hi));
            next[k] = c[k] >= kSgmAbsent ? kSgmAbsent : c[k] + best - m;
        }
#pragma unroll
        for (int k = 0; k < NPL; ++k) prev[k] = next[k];
    }
    // a pixel that may be the first of a path, without a branch: behind a previous pixel whose L_r is 0 at every disparity a step gives
    // m = 0 and min(0, p1, p1, p2) = 0, that is L_r = C, which is what start() gives (an absent disparity stays absent: c decides)
    __device__ __forceinline__ void restart_or_step(bool first, const int (&c)[NPL], int p1, int p2)
    {
#pragma unroll
        for (int k = 0; k < NPL; ++k) prev[k] = first ? 0 : prev[k];
        step(c, p1, p2);
    }
};

// One path along a line of n pixels of a frame's volumes, added into S: pixel i is at element first + i * stride (+ the lane's
// disparity) of C and of S.  The loads run kSgmAhead pixels in front of the dependent chain of path steps; within a line every
// pixel has its own addresses, and every lane reads and writes only its own disparities.
constexpr int kSgmAhead = 4;
template <int NPL>
__device__ __forceinline__ void sgm_line(const uint16_t* C, uint16_t* S, ptrdiff_t first, ptrdiff_t stride, int n, int lane, int D, int p1, int p2)
{
    int cb[kSgmAhead][NPL], sb[kSgmAhead][NPL];
    const auto load = [&](int i, int (&c)[NPL], int (&sv)[NPL]) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const bool have = i < n && lane + 64 * k < D;
            const ptrdiff_t at = first + (ptrdiff_t)i * stride + (ptrdiff_t)(lane + 64 * k);
            c[k] = have ? (int)C[at] : kSgmAbsent;
            sv[k] = have ? (int)S[at] : 0;
        }
    };
#pragma unroll
    for (int j = 0; j < kSgmAhead; ++j) load(j, cb[j], sb[j]);
    SgmPath<NPL> path;
    for (int i = 0; i < n; i += kSgmAhead) {
#pragma unroll
        for (int j = 0; j < kSgmAhead; ++j) {
            if (i + j < n) {
                if (i + j == 0) path.start(cb[j]); else path.step(cb[j], p1, p2);
#pragma unroll
                for (int k = 0; k < NPL; ++k)
                    if (lane + 64 * k < D)
                        S[first + (ptrdiff_t)(i + j) * stride + (ptrdiff_t)(lane + 64 * k)] = (uint16_t)(sb[j][k] + path.prev[k]);
            }
            load(i + j + kSgmAhead, cb[j], sb[j]);
        }
    }
}

// One wrapped diagonal walk of a frame's volumes, added into S: the wave of start column w visits pixel (y, (w + SX y) mod cols) of
// every row, top to bottom (dy = +1) or bottom to top (dy = -1).  The path restarts on the walk's first pixel and wherever the column
// wrapped on the way to this pixel -- the previous pixel of the walk is then not its diagonal predecessor inside the frame -- so
// every run between restarts is one maximal diagonal of the frame in direction (dy, SX dy), and the cols waves cover every pixel
// once.  C, S: the frame's volumes; w, and with it every cursor, is the same in all lanes.  The loads run kSgmAhead pixels in front
// of the path steps, as in sgm_line.
template <int NPL, int SX>
__device__ __forceinline__ void sgm_wrapped_line(const uint16_t* C, uint16_t* S, int w, int rows, int cols, int dy, int lane, int D, int p1, int p2)
{
    const ptrdiff_t pitch = (ptrdiff_t)cols * (ptrdiff_t)D;
    const int dx = SX * dy, y0 = dy > 0 ? 0 : rows - 1;
    int x0 = (int)(((long long)w + (long long)SX * (long long)y0) % (long long)cols);
    if (x0 < 0) x0 += cols;
    // a cursor: the column and the element offset of (y, x, 0); one row on, the column moves by dx and wraps
    const ptrdiff_t onward = (ptrdiff_t)dy * pitch + (ptrdiff_t)dx * (ptrdiff_t)D, back = -(ptrdiff_t)dx * pitch;
    const auto advance = [&](int& x, ptrdiff_t& at) {
        x += dx;
        at += onward;
        const bool wrap = dx > 0 ? x == cols : x < 0;
        x = wrap ? (dx > 0 ? 0 : cols - 1) : x;
        at = wrap ? at + back : at;
    };
    int xl = x0, xp = x0;                                    // the cursor of the loads and, kSgmAhead pixels behind it, that of the path
    ptrdiff_t al = (ptrdiff_t)y0 * pitch + (ptrdiff_t)x0 * (ptrdiff_t)D, ap = al;
    int cb[kSgmAhead][NPL], sb[kSgmAhead][NPL];
    // pixel i of the walk, which the load cursor stands on: called for i = 0, 1, 2, ... in turn (beyond the walk nothing is read)
    const auto load = [&](int i, int (&c)[NPL], int (&sv)[NPL]) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const bool have = i < rows && lane + 64 * k < D;
            c[k] = have ? (int)C[al + (ptrdiff_t)(lane + 64 * k)] : kSgmAbsent;
            sv[k] = have ? (int)S[al + (ptrdiff_t)(lane + 64 * k)] : 0;
        }
        advance(xl, al);
    };
#pragma unroll
    for (int j = 0; j < kSgmAhead; ++j) load(j, cb[j], sb[j]);
    SgmPath<NPL> path = {};
    for (int i = 0; i < rows; i += kSgmAhead) {
#pragma unroll
        for (int j = 0; j < kSgmAhead; ++j) {
            if (i + j < rows) {
                const bool wrapped = dx > 0 ? xp == 0 : xp == cols - 1;
                path.restart_or_step(i + j == 0 || wrapped, cb[j], p1, p2);
#pragma unroll
                for (int k = 0; k < NPL; ++k)
                    if (lane + 64 * k < D) S[ap + (ptrdiff_t)(lane + 64 * k)] = (uint16_t)(sb[j][k] + path.prev[k]);
                advance(xp, ap);
            }
            load(i + j + kSgmAhead, cb[j], sb[j]);
        }
    }
}

// rows y-2..y+1 of column x of an image in one dword (byte i = row clamp(y - 2 + i)), row y+2 in the low byte of the next
__device__ __forceinline__ uint2 sgm_pack_column(const uint8_t* img, int rows, int cols, int y, int x)
{
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int yy = min(max(y - 2 + i, 0), rows - 1);
        w[i] = img[(size_t)yy * (size_t)cols + (size_t)x];
    }
    return make_uint2(w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24), w[4]);
}

// The guide of dcmt_sgm_guided_dev as k_sgm_rows takes it (all zero without one): the f32 depth planes [frames][rows][cols], read as their bits;
// baseline * focal, rounded once (SgmK's); the two integers of the penalty.
struct SgmGuide {
    const uint32_t* plane;
    float bf;
    int weight, cap;
};

// Step 2b: the hint of a guide value with the bits zb, -1 where there is none.  z is finite and > 0 on its bits; bf is finite or +inf
// and >= 0, so q is +0 .. +inf and t = q + 0.5f is 0.5 .. +inf, whose bits order as the numbers do: t < D is decided on them.
__device__ __forceinline__ int sgm_hint(uint32_t zb, float bf, int D)
{
    if (!((int32_t)zb > 0 && zb < 0x7f800000u)) return -1;
    const float t = __fadd_rn(__fdiv_rn(bf, __uint_as_float(zb)), 0.5f);
    return __float_as_uint(t) < __float_as_uint((float)D) ? (int)t : -1;
}

// Step 1c for one column of an image: the census codes of rows clamp(y-2) .. clamp(y+2) of column x, 24 bits each, in one uint4
// (code i in bits 24 i .. 24 i + 23 of the 128; codes straddle dwords, which is free: only the popcount of the XOR of two such
// words is ever taken).  w[j][c] is the grey value at (clamp(y - 4 + j), clamp(x - 2 + c)); for a row y - 2 + i inside the frame the
// window of its code is w[i..i+4][.].  A row beyond the frame is the nearest row inside -- the clamp of step 2c replicates the H
// plane -- so its code is that row's code, not the code of the window around it.
__device__ __forceinline__ uint4 sgm_census_column(const uint8_t* img, int rows, int cols, int y, int x)
{
    int xs[5], w[9][5];
#pragma unroll
    for (int c = 0; c < 5; ++c) xs[c] = min(max(x - 2 + c, 0), cols - 1);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const uint8_t* row = img + (size_t)min(max(y - 4 + j, 0), rows - 1) * (size_t)cols;
#pragma unroll
        for (int c = 0; c < 5; ++c) w[j][c] = row[xs[c]];
    }
    uint32_t code[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int centre = w[i + 2][2];
        uint32_t k = 0;
#pragma unroll
        for (int n = 0; n < 25; ++n)
            if (n != 12) k |= (uint32_t)(w[i + n / 5][n % 5] < centre) << (n < 12 ? n : n - 1);       // strict: equal is 0
        code[i] = k;
    }
    code[1] = y - 1 >= 0 ? code[1] : code[2];
    code[0] = y - 2 >= 0 ? code[0] : code[1];
    code[3] = y + 1 <= rows - 1 ? code[3] : code[2];
    code[4] = y + 2 <= rows - 1 ? code[4] : code[3];
    const uint64_t lo = (uint64_t)code[0] | (uint64_t)code[1] << 24 | (uint64_t)code[2] << 48;            // code 2's upper byte: in hi
    const uint64_t hi = (uint64_t)(code[2] >> 16) | (uint64_t)code[3] << 8 | (uint64_t)code[4] << 32;
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// The rows kernel, one template for every variant.  left, right: [frames][rows][cols]; vol: the chunk's workspace, per frame C then S
// ([rows][cols][D] uint16 each); g: the guide, looked at only if GUIDED.
//   NPL     disparities a lane (1: D <= 64; 2).
//   LDS     the row's operands are staged in LDS; otherwise every column is made from global memory where it is used.
//   GUIDED  step 2b: the staging loop converts the guide row to hints, a lane per column -- one division a pixel -- and keeps them as
//           int16 behind the staged columns; C' = C + the penalty goes into the path and into the volume, so every later pass reads C'.
//   COST    kSgmCostAbsdiff (steps 1, 2): the grey rows y-2..y+2 of both images are staged packed by column (sgm_pack_column), 8 + 8
//           bytes a column, and the column sum of one (x, d) is two v_sad_u8.  kSgmCostCensus (steps 1c, 2c): the staging loop makes
//           the codes of rows y-2..y+2 of the RIGHT image from its grey rows y-4..y+4, one uint4 a column: 16 bytes a column as well,
//           so as many workgroups share a CU -- the chain of path steps is bound by latency, and with both images' codes in LDS (32
//           bytes a column, half the workgroups) the kernel took 1.7 times as long.  The LEFT column of a step is the same in every
//           lane, so its codes stay in registers: the wave holds those of 64 columns at a time, a column a lane, reads column x's
//           with four v_readlane and makes the next 64 when the walk reaches them.  The column sum of the five Hamming distances of
//           one (x, d) is four v_xor and four accumulating v_bcnt; 10 * the box is the block cost.
// The two costs also differ in when column x + 3 is fetched: absolute differences behind the path step, census -- its codes and the
// hint of column x + 1 -- ahead of it, used behind it (sections 30 and 31).
template <int NPL, bool LDS, bool GUIDED, int COST>
__global__ __launch_bounds__(kSgmRowThreads) void k_sgm_rows(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                                                             uint16_t* __restrict__ vol, int rows, int cols, int D, int p1, int p2, SgmGuide g)
{
    constexpr bool CENSUS = COST == kSgmCostCensus;
    extern __shared__ uint2 sgm_lds[];                      // absolute differences: [cols] left, then [cols] right
    extern __shared__ uint4 sgm_lds_census[];               // census: [cols] the right image's codes
    const int y = (int)blockIdx.x, lane = sgm_lane();
    const size_t frame = blockIdx.y, px = (size_t)rows * (size_t)cols, ve = px * (size_t)D;
    const uint8_t* L = left + frame * px;
    const uint8_t* R = right + frame * px;
    uint16_t* C = vol + frame * 2 * ve + (size_t)y * (size_t)cols * (size_t)D;
    uint16_t* S = C + ve;
    const uint32_t* G = GUIDED ? g.plane + frame * px + (size_t)y * (size_t)cols : nullptr;      // the guide's row y
    int16_t* hints = CENSUS ? reinterpret_cast<int16_t*>(sgm_lds_census + (size_t)cols)           // behind either: [cols] int16 hints
                            : reinterpret_cast<int16_t*>(sgm_lds + 2 * (size_t)cols);
    if constexpr (LDS) {
        for (int x = lane; x < cols; x += 64) {
            if constexpr (CENSUS) {
                sgm_lds_census[x] = sgm_census_column(R, rows, cols, y, x);
            } else {
                sgm_lds[x] = sgm_pack_column(L, rows, cols, y, x);
                sgm_lds[cols + x] = sgm_pack_column(R, rows, cols, y, x);
            }
            if constexpr (GUIDED) hints[x] = (int16_t)sgm_hint(G[x], g.bf, D);
        }
        __syncthreads();
    }
    // census: the left image's codes of columns 64 j .. 64 j + 63, lane i those of column 64 j + i (the last column again beyond the
    // row's end, which is never asked for); column x of the window is read from lane x & 63, x the same in every lane
    uint4 window = {};
    if constexpr (CENSUS) window = sgm_census_column(L, rows, cols, y, min(lane, cols - 1));
    const auto left_codes = [&](int x) -> uint4 {
        const int at = x & 63;
        return make_uint4((uint32_t)__builtin_amdgcn_readlane((int)window.x, at), (uint32_t)__builtin_amdgcn_readlane((int)window.y, at),
                          (uint32_t)__builtin_amdgcn_readlane((int)window.z, at), (uint32_t)__builtin_amdgcn_readlane((int)window.w, at));
    };
    bool have[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) have[k] = lane + 64 * k < D;
    // census, V(x, d): the sum over the five rows of popcount(K_left(., x) ^ K_right(., max(x - d, 0))), 0..120, in two halves: the
    // codes are asked for, and their distance is taken when it is needed, a path step later
    const auto codes_of = [&](int x, int d, uint4& l, uint4& r) {
        const int xr = max(x - d, 0);
        l = left_codes(x);
        if constexpr (LDS) r = sgm_lds_census[xr]; else r = sgm_census_column(R, rows, cols, y, xr);
    };
    const auto hamming = [](const uint4& l, const uint4& r) -> int {
        return __builtin_popcount(l.x ^ r.x) + __builtin_popcount(l.y ^ r.y) + __builtin_popcount(l.z ^ r.z) + __builtin_popcount(l.w ^ r.w);
    };
    // V(x, d) of either cost; absolute differences: the sum over the five rows of |left(., x) - right(., max(x - d, 0))|
    const auto column_sum = [&](int x, int d) -> int {
        if constexpr (CENSUS) {
            uint4 l, r;
            codes_of(x, d, l, r);
            return hamming(l, r);
        } else {
            const int xr = max(x - d, 0);
            uint2 l, r;
            if constexpr (LDS) { l = sgm_lds[x]; r = sgm_lds[cols + xr]; }
            else { l = sgm_pack_column(L, rows, cols, y, x); r = sgm_pack_column(R, rows, cols, y, xr); }
            return (int)__builtin_amdgcn_sad_u8(l.x, r.x, __builtin_amdgcn_sad_u8(l.y, r.y, 0u));
        }
    };
    // the box over columns x-2..x+2, clamped: v[k][0..4] its five column sums
    int v[NPL][5], box[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int d = lane + 64 * k;
        const int v0 = column_sum(0, d), v1 = column_sum(min(1, cols - 1), d), v2 = column_sum(min(2, cols - 1), d);
        v[k][0] = v[k][1] = v[k][2] = v0; v[k][3] = v1; v[k][4] = v2;
        box[k] = 3 * v0 + v1 + v2;
    }
    // pen[k] is the penalty of column x, min(weight |d - h|, cap) or 0 without a hint.  The hint is the same in every lane (an
    // LDS broadcast, or a wave-uniform address on the global route) and the penalty hangs on x and the lane alone, so it is made one
    // column ahead, beside the box, off the chain of path steps.  The hint goes to a scalar register, where "no hint" becomes a
    // weight of 0; weight <= 10000 and |d - h| <= 127 fit the 24-bit multiply.  Absolute differences read the hint of column x here;
    // census has asked for it ahead of the path step and hands it in as `fetched`.
    int pen[NPL] = {};
    const auto hint_of = [&](int x) -> int { return LDS ? (int)hints[x] : sgm_hint(G[x], g.bf, D); };
    const auto penalties = [&](int x, int fetched) {
        const int h = __builtin_amdgcn_readfirstlane(CENSUS ? fetched : hint_of(x));
        const int weight = h >= 0 ? g.weight : 0;
#pragma unroll
        for (int k = 0; k < NPL; ++k) pen[k] = min(__mul24(weight, abs(lane + 64 * k - h)), g.cap);
    };
    if constexpr (GUIDED) penalties(0, CENSUS ? hint_of(0) : -1);
    SgmPath<NPL> path;
    for (int x = 0; x < cols; ++x) {
        // census: the codes of column x + 3 and the hint of column x + 1 are asked for here and used behind the path step, which hides
        // their way from LDS; column x + 3 may be the first of the next 64 of the left image
        [[maybe_unused]] uint4 nl[NPL], nr[NPL];
        const bool more = x + 3 <= cols - 1;
        int next_hint = -1;
        if constexpr (CENSUS) {
            if (more) {
                if (((x + 3) & 63) == 0) window = sgm_census_column(L, rows, cols, y, min(x + 3 + lane, cols - 1));
#pragma unroll
                for (int k = 0; k < NPL; ++k) codes_of(x + 3, lane + 64 * k, nl[k], nr[k]);
            }
            if constexpr (GUIDED) { if (x + 1 < cols) next_hint = hint_of(x + 1); }
        }
        int cost[NPL], c[NPL];                                  // C (C' with a guide) of this column; census: 10 * the box <= 6000
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            cost[k] = (CENSUS ? 10 * box[k] : box[k]) + pen[k];
            c[k] = have[k] ? cost[k] : kSgmAbsent;
        }
        if (x == 0) path.start(c); else path.step(c, p1, p2);
#pragma unroll
        for (int k = 0; k < NPL; ++k)
            if (have[k]) {
                const size_t at = (size_t)x * (size_t)D + (size_t)(lane + 64 * k);
                C[at] = (uint16_t)cost[k];
                S[at] = (uint16_t)path.prev[k];
            }
        // the box of column x + 1: column x + 3 comes in (the last column again beyond the edge; absolute differences fetch it
        // here), column x - 2 goes out
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int in = more ? (CENSUS ? hamming(nl[k], nr[k]) : column_sum(x + 3, lane + 64 * k)) : v[k][4];
            box[k] += in - v[k][0];
            v[k][0] = v[k][1]; v[k][1] = v[k][2]; v[k][2] = v[k][3]; v[k][3] = v[k][4]; v[k][4] = in;
        }
        if constexpr (GUIDED) { if (x + 1 < cols) penalties(x + 1, next_hint); }
    }
    // right -> left over the C this wave wrote: lane d reads the addresses lane d stored
    sgm_line<NPL>(C, S, (ptrdiff_t)(cols - 1) * D, -(ptrdiff_t)D, cols, lane, D, p1, p2);
}

template <int NPL>
__global__ __launch_bounds__(64 * kSgmWaves) void k_sgm_cols(uint16_t* __restrict__ vol, int rows, int cols, int D, int p1, int p2)
{
    const int x = (int)(blockIdx.x * kSgmWaves + threadIdx.x / 64u), lane = sgm_lane();
    if (x >= cols) return;                                  // whole waves: no barrier follows
    const size_t frame = blockIdx.y, ve = (size_t)rows * (size_t)cols * (size_t)D, pitch = (size_t)cols * (size_t)D;
    const uint16_t* C = vol + frame * 2 * ve + (size_t)x * (size_t)D;
    uint16_t* S = vol + frame * 2 * ve + ve + (size_t)x * (size_t)D;
    sgm_line<NPL>(C, S, 0, (ptrdiff_t)pitch, rows, lane, D, p1, p2);                                   // top -> bottom
    sgm_line<NPL>(C, S, (ptrdiff_t)(rows - 1) * (ptrdiff_t)pitch, -(ptrdiff_t)pitch, rows, lane, D, p1, p2);   // bottom -> top
}

// The two diagonal paths of one orientation, added into S: SX = +1 the "\" lines, (+1,+1) going down and (-1,-1) going up; SX = -1 the
// "/" lines, (+1,-1) and (-1,+1).  One wave per start column, walking wrapped lines (sgm_wrapped_line), so that every wave has rows
// pixels whatever the lengths of the diagonals it is made of.  Within one orientation every pixel is on exactly one line, so S is
// read and written plainly; the two orientations are two launches because their lines cross.
template <int NPL, int SX>
__global__ __launch_bounds__(64 * kSgmWaves) void k_sgm_diag(uint16_t* __restrict__ vol, int rows, int cols, int D, int p1, int p2)
{
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kSgmWaves + threadIdx.x / 64u)), lane = sgm_lane();
    if (w >= cols) return;                                  // whole waves: no barrier follows
    const size_t frame = blockIdx.y, ve = (size_t)rows * (size_t)cols * (size_t)D;
    const uint16_t* C = vol + frame * 2 * ve;
    uint16_t* S = vol + frame * 2 * ve + ve;
    sgm_wrapped_line<NPL, SX>(C, S, w, rows, cols, +1, lane, D, p1, p2);
    sgm_wrapped_line<NPL, SX>(C, S, w, rows, cols, -1, lane, D, p1, p2);
}

// disp16 and depth: [frames][rows][cols], either may be null
template <int NPL>
__global__ __launch_bounds__(64 * kSgmWaves) void k_sgm_winner(const uint16_t* __restrict__ vol, int16_t* __restrict__ disp16,
                                                               float* __restrict__ depth, int rows, int cols, unsigned segments, SgmK K)
{
    const uint64_t wave = (uint64_t)blockIdx.x * kSgmWaves + threadIdx.x / 64u;
    if (wave >= (uint64_t)rows * segments) return;
    const int y = (int)(wave / segments), x0 = (int)(wave % segments) * kSgmSegment, lane = sgm_lane();
    const int D = K.disparities;
    const size_t frame = blockIdx.y, px = (size_t)rows * (size_t)cols, ve = px * (size_t)D;
    const uint16_t* S = vol + frame * 2 * ve + ve + (size_t)y * (size_t)cols * (size_t)D;
    const int n = min(kSgmSegment, cols - x0);
    int mine = -16;
    // S of disparity d of a pixel whose S the wave holds (sv[k]: disparity lane + 64 k); d is the same in every lane
    const auto held = [&](const unsigned (&sv)[NPL], int d) -> unsigned {
        unsigned v = (unsigned)__builtin_amdgcn_readlane((int)sv[0], d & 63);
        if constexpr (NPL > 1) { if (d >= 64) v = (unsigned)__builtin_amdgcn_readlane((int)sv[1], d & 63); }
        return v;
    };
    // kSgmAhead pixels at a time, so that their loads, reductions and gathers overlap; a pixel beyond the segment repeats the last one
    for (int i0 = 0; i0 < n; i0 += kSgmAhead) {
        unsigned s[kSgmAhead][NPL], key[kSgmAhead], rkey[kSgmAhead];
        int xs[kSgmAhead];
        bool ok[kSgmAhead];
        // 4. the lowest d of the least S: the minimum of S << 8 | d
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u) {
            xs[u] = x0 + min(i0 + u, n - 1);
            const uint16_t* Sp = S + (size_t)xs[u] * (size_t)D;
            key[u] = 0xffffffffu;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const int d = lane + 64 * k;
                s[u][k] = d < D ? (unsigned)Sp[d] : 0u;
                if (d < D) key[u] = min(key[u], (s[u][k] << 8) | (unsigned)d);
            }
        }
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u) key[u] = sgm_wave_min(key[u]);
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u) {
            const int dstar = (int)(key[u] & 0xffu);
            const unsigned best = key[u] >> 8;
            // 5. uniqueness
            bool rival = false;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const int d = lane + 64 * k;
                rival = rival || (d < D && abs(d - dstar) > 1 && s[u][k] * (unsigned)(100 - K.uniqueness) < best * 100u);
            }
            // 6. inside
            ok[u] = __ballot(rival) == 0ull && xs[u] - dstar >= 0;
            // 7. left-right check: the gather (from column 0 for a pixel that is not inside: its result is not used)
            rkey[u] = 0xffffffffu;
            if (K.disp12 >= 0) {
                const int xp = max(xs[u] - dstar, 0);
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const int d = lane + 64 * k;
                    if (d < D && xp + d < cols) rkey[u] = min(rkey[u], ((unsigned)S[(size_t)(xp + d) * (size_t)D + (size_t)d] << 8) | (unsigned)d);
                }
            }
        }
        if (K.disp12 >= 0) {
#pragma unroll
            for (int u = 0; u < kSgmAhead; ++u) {
                const int dr = (int)(sgm_wave_min(rkey[u]) & 0xffu);
                ok[u] = ok[u] && abs(dr - (int)(key[u] & 0xffu)) <= K.disp12;
            }
        }
        // 8. sub-pixel
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u) {
            const int dstar = (int)(key[u] & 0xffu);
            const unsigned best = key[u] >> 8;
            int d16 = 16 * dstar;
            if (dstar > 0 && dstar < D - 1) {
                const unsigned a = held(s[u], dstar - 1), b = held(s[u], dstar + 1);
                const unsigned den = max(a + b - 2u * best, 1u);
                d16 += (int)(((a - b + den) * 16u + den) / (2u * den)) - 8;
            }
            if (lane == i0 + u) mine = ok[u] ? d16 : -16;       // (a repeated pixel has no lane: i0 + u >= n > every lane that stores)
        }
    }
    if (lane < n) {
        const size_t at = frame * px + (size_t)y * (size_t)cols + (size_t)(x0 + lane);
        if (disp16) disp16[at] = (int16_t)mine;
        if (depth) depth[at] = mine > 0 ? fminf(K.bf / ((float)mine / 16.0f), K.max_depth) : 0.0f;
    }
}

}  // namespace dcmt
