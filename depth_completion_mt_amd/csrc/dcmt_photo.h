// dcmt_photo.h -- the constants dcmt_kernels_photo.h (k_photo_error, k_photo_error_global) and its plan (plan_photo_error,
// dcmt_plan_side.h) share.  Plain C++, no HIP: the plan is tested on a CPU.
#ifndef DCMT_PHOTO_H
#define DCMT_PHOTO_H

#include <cstddef>
#include <cstdint>

namespace dcmt {

constexpr int kPhotoThreads = 256;           // both kernels
constexpr int kPhotoMaxWindow = 4;           // window 1..4: 2 * window taps a side, at most 8 bytes = two dwords of a row
constexpr int kPhotoBandRows = 8;            // output rows per workgroup of the LDS route, halved by the plan where that serves
constexpr uint32_t kPhotoPadLeft = 16;       // LDS bytes in front of column 0 of a staged row (>= window + 3 of an aligned dword read)
constexpr uint32_t kPhotoPadRight = 16;      // ... and behind its last column (>= window + 8)
constexpr size_t kPhotoLdsBudget = 64 * 1024;   // what a workgroup may stage: two workgroups per CU by LDS alone at the worst
constexpr uint32_t kPhotoGlobalPx = 256;     // pixels per workgroup of the fallback route, one per thread

// bytes between the staged rows of one image: the row, its pads, rounded up to the 16 bytes the staging stores write
constexpr uint32_t photo_pitch(uint32_t cols) { return (cols + kPhotoPadLeft + kPhotoPadRight + 15u) & ~15u; }
// rows a band of `band` output rows reads: p runs over [-window, window)
constexpr uint32_t photo_staged_rows(uint32_t band, uint32_t window) { return band + 2u * window - 1u; }

}  // namespace dcmt

#endif
