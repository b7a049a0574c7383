// dcmt_kernels_joint.h -- the kernel of dcmt_joint_bilateral_dev (include/dcmt.h): the joint (cross) bilateral filter that fills and
// smooths a depth plane under the guidance of a camera image.  Compiled in dcmt_cloud.hip; the validity test is the planes'
// (dcmt_kernels_planes.h), called and not restated; the sums follow dcmt_dot_rn.h's discipline: every operation rounded once.
//   k_joint   one workgroup of four waves per tile of kJointTileX x kJointTileY outputs.  The tile with a halo of R is staged in LDS
//             as ONE PAIR of dwords per pixel: the depth's bits -- 0 on a hole and outside the frame, so that "is a tap valid" is one
//             compare with zero and a hole's bits never enter float arithmetic -- and the guide's one or three bytes in the low bytes
//             of a dword, so that a tap's guide distance is one v_sad_u8 for either channel count.  A tap is one 8-byte LDS read, its
//             lanes on consecutive pairs: conflict-free.  The rows are kJointPitch pixels apart whatever R: a lane's four pixels and
//             the step to the next tap are constant offsets of one address.  The two tables go to static LDS once per workgroup,
//             clamped to 255, a byte an entry (four entries a bank word: lanes whose guide distances are close share a word);
//             w_guide is extended with zeros, and a tap on a hole reads entry kJointGuide: w = 0 without a branch.  A lane owns four
//             pixels of one tile column (rows r, r + 4, r + 8, r + 12 of the tile): four independent accumulation chains, each in
//             tap order.  The base of a hole is tracked through sw itself: base = sw != 0 ? base : v, a valid centre's sw starting
//             at a bias of 2^24 that is taken off at the end (sw < 2^24, so the sum never wraps).  What the definition lets it skip
//             without changing a bit: taps whose w_space is 0 (wave-uniform); the staging of a tile none of whose pixels is to be
//             processed -- with FILL alone behind a completed plane that is most tiles --; the tap loop of a wave none of whose
//             sixty-four columns by four rows is, or whose tile has no valid pixel within reach: the empty upper third of a KITTI
//             frame.  The same kernel counts: integer adds, reduced per wave, at most two atomics a wave.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dcmt.h"
#include "dcmt_joint.h"
#include "dcmt_kernels_planes.h"

namespace dcmt {

// grid (tiles_x * tiles_y, frames), 256 threads, joint_lds_bytes(R) of dynamic LDS beside the kJointTableLds bytes of the tables.
// depth, out: the bits of f32 planes; out overlaps nothing.  counts: [frames][2] or null.
__global__ __launch_bounds__(256)
void k_joint(const uint32_t* __restrict__ depth, const uint8_t* __restrict__ guide, int channels, const dcmt_joint_tables* __restrict__ tables,
             uint32_t* __restrict__ out, uint32_t rows, uint32_t cols, uint32_t tiles_x, int R, uint32_t flags, uint32_t min_weight, uint32_t lo_bits,
             uint32_t hi_bits, uint32_t* __restrict__ counts)
{
    extern __shared__ uint2 joint_px[];
    __shared__ uint8_t joint_tab[kJointGuideLds + kJointSpace];              // static: a table read's address is the index itself
    constexpr int P = kJointPitch;                                           // the rows' pitch whatever R: a lane's four pixels and a
                                                                             // tap's column step are constant offsets of one address
    const int Wt = kJointTileX + 2 * R, Ht = kJointTileY + 2 * R;
    uint8_t* wg = joint_tab;
    uint8_t* wsp = joint_tab + kJointGuideLds;
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = (int)(tile_x * kJointTileX), y0 = (int)(tile_y * kJointTileY);
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);

    // the lane's own four pixels first: what they hold and whether any of them is to be processed.  A tile none of whose pixels is
    // -- with FILL alone behind a completed plane that is most tiles -- stages nothing and copies
    const int x = x0 + lane;
    uint32_t cg[kJointPix], orig[kJointPix], sw[kJointPix];
    float base[kJointPix], acc[kJointPix];
    bool in[kJointPix], hole[kJointPix], proc[kJointPix], any = false;
#pragma unroll
    for (int i = 0; i < kJointPix; ++i) {
        const int y = y0 + wave + 4 * i;
        in[i] = x < (int)cols && y < (int)rows;
        orig[i] = depth[fo + (size_t)min(y, (int)rows - 1) * cols + (size_t)min(x, (int)cols - 1)];
        hole[i] = !(in[i] && planes_is_return(orig[i], lo_bits, hi_bits));
        sw[i] = hole[i] ? 0u : kJointBias;       // a valid centre's sum starts at a bias, taken off at the end: "no weighted tap yet" is sw == 0
        base[i] = __uint_as_float(hole[i] ? 0u : orig[i]);
        proc[i] = in[i] && (flags & (hole[i] ? (uint32_t)DCMT_JOINT_FILL : (uint32_t)DCMT_JOINT_SMOOTH)) != 0u;
        any = any || proc[i];
        acc[i] = 0.0f;
    }
    if (__syncthreads_or(any ? 1 : 0) != 0) {   // (the same for the whole workgroup)
        for (int i = (int)threadIdx.x; i < kJointGuideLds; i += 256) wg[i] = (uint8_t)(i < kJointGuide ? min((uint32_t)tables->w_guide[i], 255u) : 0u);
        if (threadIdx.x < (uint32_t)kJointSpace) wsp[threadIdx.x] = (uint8_t)min((uint32_t)tables->w_space[threadIdx.x], 255u);
        bool staged_valid = false;
        for (int ty = wave; ty < Ht; ty += 4) {
            const int gy = y0 - R + ty;
            for (int tx = lane; tx < Wt; tx += 64) {
                const int gx = x0 - R + tx;
                const bool inside = gy >= 0 && gy < (int)rows && gx >= 0 && gx < (int)cols;
                const size_t at = fo + (size_t)min(max(gy, 0), (int)rows - 1) * cols + (size_t)min(max(gx, 0), (int)cols - 1);     // loads from clamped addresses
                const uint32_t zb = depth[at];
                uint32_t g;
                if (channels == 1) g = guide[at];
                else g = (uint32_t)guide[3 * at] | (uint32_t)guide[3 * at + 1] << 8 | (uint32_t)guide[3 * at + 2] << 16;
                const bool valid = inside && planes_is_return(zb, lo_bits, hi_bits);
                staged_valid = staged_valid || valid;
                joint_px[ty * P + tx] = make_uint2(valid ? zb : 0u, g);
            }
        }
        // the last barrier: from here a wave goes its own way.  A tile with no valid pixel in reach has no weighted tap at all
        const bool reach_valid = __syncthreads_or(staged_valid ? 1 : 0) != 0;
        if (reach_valid && __any(any)) {
            const uint2* centre = joint_px + (R + wave) * P + R + lane;      // the lane's first pixel; pixel i is 4 i rows below
#pragma unroll
            for (int i = 0; i < kJointPix; ++i) cg[i] = centre[4 * i * P].y;
            for (int dy = -R; dy <= R; ++dy) {
                // the row's w_space, lane l holding the one of dx = l - R and 0 outside the disc: one LDS read a row, then a lane read a tap
                const int d2 = dy * dy + (lane - R) * (lane - R);
                const int ws_row = d2 <= R * R ? (int)wsp[d2] : 0;
                for (int dx = -R; dx <= R; ++dx) {
                    const uint32_t ws = (uint32_t)__builtin_amdgcn_readlane(ws_row, dx + R);
                    if (ws == 0u) continue;                                  // wave-uniform: outside the disc, or a tap whose w is 0 for every pixel
                    const uint2* tap = centre + dy * P + dx;
#pragma unroll
                    for (int i = 0; i < kJointPix; ++i) {
                        const uint2 p = tap[4 * i * P];
                        const uint32_t s = __builtin_amdgcn_sad_u8(p.y, cg[i], 0u);
                        const uint32_t w = __umul24(ws, (uint32_t)wg[p.x != 0u ? s : (uint32_t)kJointGuide]);      // both at most 255
                        const float v = __uint_as_float(p.x);
                        base[i] = sw[i] != 0u ? base[i] : v;                 // a hole takes its first weighted tap; before that w = 0
                        sw[i] += w;
                        acc[i] = __fadd_rn(acc[i], __fmul_rn((float)w, __fsub_rn(v, base[i])));
                    }
                }
            }
        }
    }
    uint32_t filled = 0u, left = 0u;
#pragma unroll
    for (int i = 0; i < kJointPix; ++i) {
        const uint32_t sum = sw[i] - (hole[i] ? 0u : kJointBias);
        const bool done = proc[i] && sum >= min_weight;
        const float yv = __fadd_rn(base[i], __fdiv_rn(acc[i], (float)max(sum, 1u)));
        if (in[i]) out[fo + (size_t)(y0 + wave + 4 * i) * cols + (size_t)x] = done ? __float_as_uint(yv) : orig[i];
        const bool was_hole = in[i] && hole[i];
        filled += was_hole && done ? 1u : 0u;
        left += was_hole && !done ? 1u : 0u;
    }
    if (counts) {                               // (the whole grid's)
        for (int m = 32; m >= 1; m >>= 1) {
            filled += (uint32_t)__shfl_xor((int)filled, m, 64);
            left += (uint32_t)__shfl_xor((int)left, m, 64);
        }
        if (lane == 0 && filled != 0u) atomicAdd(counts + 2 * (size_t)blockIdx.y, filled);
        if (lane == 0 && left != 0u) atomicAdd(counts + 2 * (size_t)blockIdx.y + 1, left);
    }
}

}  // namespace dcmt
