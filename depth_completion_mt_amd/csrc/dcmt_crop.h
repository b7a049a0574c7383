// dcmt_crop.h -- what k_crop_frames (dcmt_kernels_crop.h, compiled in dcmt_cloud.hip) does with a record and with a row, as plain
// functions: the test of one dcmt_crop_src record, the cutting of a destination row into pieces, and the copy of one piece through
// a memory the caller supplies.  No HIP: the kernel instantiates them with device loads and stores, tests/plan_crop_test.cpp with a
// memory that checks every access, and both run the same statements.
//
// A destination row is `len` = out_cols * elem_bytes bytes whose source starts at ANY byte.  It is cut into
//     head    the bytes in front of the first 16-byte boundary of the DESTINATION (all of a row that reaches none),
//     pieces  runs of 16 bytes, each written with one 16-byte store to an address that is a multiple of 16,
//     tail    the bytes behind the last piece;
// head and tail are at most 15 bytes each and move as single bytes.  A piece's 16 source bytes start at byte `sh` = 0..15 of a
// naturally aligned 16-byte quad, and sh is the same for every piece of the row.  sh = 0: the piece IS that quad.  Otherwise it is
// assembled from that quad and the next, both loaded whole at their natural alignment -- eight dwords, of which five consecutive ones
// starting at dword sh / 4 are funnel-shifted right by sh % 4 bytes (v_alignbyte_b32 with a wave-uniform shift): no access ever
// rests on the hardware's handling of unaligned addresses.  The quads reach up to 15 bytes in front of and 16 behind the piece's own
// bytes: where that would leave the source buffer [lo, hi) -- possible only at its two ends -- the piece loads its 16 bytes one by one.
#pragma once
#include <cstdint>

#include "dcmt_chunks.h"       // DCMT_HD

namespace dcmt {

constexpr int kCropThreads = 256;                // k_crop_frames: four waves, each a row at a time
constexpr int kCropWaves = kCropThreads / 64;
constexpr uint32_t kCropBandRows = 16;           // rows of a workgroup's band at most (plan_crop, dcmt_plan_side.h)

// k_depth_to_u16: kU16PxPerLane pixels per lane; a launch covers at most kU16SegPx pixels (32-bit pixel indices, the last
// workgroup's overhang included), a multiple of a workgroup's share so that every segment starts as aligned as the run does
constexpr int kU16Threads = 256;
constexpr uint32_t kU16PxPerLane = 8;
constexpr uint32_t kU16PxPerWg = kU16PxPerLane * kU16Threads;                    // 2048
constexpr uint32_t kU16SegPx = 0x7fff0000u;
static_assert(kU16SegPx % kU16PxPerWg == 0, "kU16SegPx");

// One dcmt_crop_src record against the call's window, element size and source size: every comparison in 64 bits, on values that
// cannot wrap -- rows, cols, x0, y0, out_rows, out_cols are 32-bit, elem is 1..4, so a sum of two is below 2^32, cols * elem below
// 2^34 and (rows - 1) * row_stride below 2^63.  True: every byte of the window lies in [offset, src_bytes) of the source.
DCMT_HD inline bool crop_record_ok(uint64_t offset, uint32_t row_stride, int32_t rows, int32_t cols, int32_t x0, int32_t y0,
                                   uint32_t elem, int32_t out_rows, int32_t out_cols, uint64_t src_bytes)
{
    if (rows < 1 || cols < 1 || x0 < 0 || y0 < 0 || out_rows < 1 || out_cols < 1) return false;
    if ((int64_t)x0 + (int64_t)out_cols > (int64_t)cols || (int64_t)y0 + (int64_t)out_rows > (int64_t)rows) return false;
    const uint64_t row_bytes = (uint64_t)(uint32_t)cols * elem;
    if ((uint64_t)row_stride < row_bytes) return false;
    if (offset > src_bytes) return false;
    return (uint64_t)(uint32_t)(rows - 1) * row_stride + row_bytes <= src_bytes - offset;
}

// The byte addresses of row r of frame f's window: its first source byte (a record that has passed: inside the source for every
// r < out_rows) and its first destination byte.  src, dst: the addresses of the two buffers; len = out_cols * elem.
DCMT_HD inline uint64_t crop_row_src(uint64_t src, uint64_t offset, uint32_t row_stride, int32_t x0, int32_t y0, uint32_t elem, uint32_t r)
{
    return src + offset + (uint64_t)((uint32_t)y0 + r) * row_stride + (uint64_t)(uint32_t)x0 * elem;
}
DCMT_HD inline uint64_t crop_row_dst(uint64_t dst, uint32_t f, uint32_t out_rows, uint32_t len, uint32_t r)
{
    return dst + ((uint64_t)f * out_rows + r) * len;
}

struct RowCut {
    uint32_t head, pieces, tail;     // bytes, 16-byte pieces, bytes: head + 16 * pieces + tail = len
    uint32_t sh;                     // byte 0..15 of its aligned 16-byte quad at which every piece's source starts
};

// dst, src: the byte addresses of the row's first destination and source byte
DCMT_HD inline RowCut crop_cut_row(uint64_t dst, uint64_t src, uint32_t len)
{
    RowCut c;
    const uint32_t to_boundary = (uint32_t)((16u - (uint32_t)(dst & 15u)) & 15u);
    c.head = len < to_boundary ? len : to_boundary;
    c.pieces = (len - c.head) / 16u;
    c.tail = len - c.head - 16u * c.pieces;
    c.sh = (uint32_t)((src + c.head) & 15u);
    return c;
}

// byte e = 0 .. head + tail - 1 of the row's ends -> its position in the row
DCMT_HD inline uint32_t crop_edge_pos(const RowCut& c, uint32_t e) { return e < c.head ? e : e + 16u * c.pieces; }

// the aligned source bytes [first, last) piece p loads when it loads quads; src as for crop_cut_row
DCMT_HD inline uint64_t crop_piece_first(const RowCut& c, uint64_t src, uint32_t p) { return (src + c.head + 16ull * p) & ~15ull; }
DCMT_HD inline uint64_t crop_piece_last(const RowCut& c, uint64_t src, uint32_t p) { return crop_piece_first(c, src, p) + (c.sh ? 32u : 16u); }
// ... and whether it may: both quads inside the source buffer [lo, hi)
DCMT_HD inline bool crop_piece_wide(const RowCut& c, uint64_t src, uint32_t p, uint64_t lo, uint64_t hi)
{
    return crop_piece_first(c, src, p) >= lo && crop_piece_last(c, src, p) <= hi;
}

// ({hi, lo} >> 8 * b) & 0xffffffff, b = 0..3
DCMT_HD inline uint32_t crop_alignbyte(uint32_t hi, uint32_t lo, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, b);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * b));
#endif
}

// w[0..7]: two consecutive quads (w[4..7] are not read where sh = 0); o[0..3]: the 16 bytes from byte sh on -- or w[0..3] as they
// are where `direct` (a piece that was loaded byte by byte).  sh is uniform over the row, so the switch is a scalar branch and every
// register index is static; direct is a lane's own.
DCMT_HD inline void crop_assemble(const uint32_t w[8], uint32_t sh, bool direct, uint32_t o[4])
{
    const uint32_t b = sh & 3u;
    switch (sh >> 2) {
    case 0:
        for (int i = 0; i < 4; ++i) o[i] = b ? crop_alignbyte(w[i + 1], w[i], b) : w[i];
        break;
    case 1:
        for (int i = 0; i < 4; ++i) o[i] = b ? crop_alignbyte(w[i + 2], w[i + 1], b) : w[i + 1];
        break;
    case 2:
        for (int i = 0; i < 4; ++i) o[i] = b ? crop_alignbyte(w[i + 3], w[i + 2], b) : w[i + 2];
        break;
    default:
        for (int i = 0; i < 4; ++i) o[i] = b ? crop_alignbyte(w[i + 4], w[i + 3], b) : w[i + 3];
        break;
    }
    for (int i = 0; i < 4; ++i) o[i] = direct ? w[i] : o[i];
}

// Piece p of the row through memory M:  m.load16(addr, w) four dwords from a multiple of 16, m.load8(addr), m.store16(addr, o) to a
// multiple of 16.  lo, hi: the source buffer.  Fetching is apart from assembling and storing so that a lane can have the loads of
// several pieces in flight before it needs the first: crop_fetch_piece issues the loads into w[0..7] and returns `direct`.
template <typename M>
DCMT_HD inline bool crop_fetch_piece(M& m, const RowCut& c, uint64_t src, uint32_t p, uint64_t lo, uint64_t hi, uint32_t w[8])
{
    for (int i = 0; i < 8; ++i) w[i] = 0;
    if (crop_piece_wide(c, src, p, lo, hi)) {
        const uint64_t q = crop_piece_first(c, src, p);
        m.load16(q, w);
        if (c.sh) m.load16(q + 16, w + 4);
        return false;
    }
    const uint64_t s = src + c.head + 16ull * p;
    for (int i = 0; i < 4; ++i)
        w[i] = (uint32_t)m.load8(s + 4 * i) | ((uint32_t)m.load8(s + 4 * i + 1) << 8) | ((uint32_t)m.load8(s + 4 * i + 2) << 16) |
               ((uint32_t)m.load8(s + 4 * i + 3) << 24);
    return true;
}
DCMT_HD inline uint64_t crop_piece_dst(const RowCut& c, uint64_t dst, uint32_t p) { return dst + c.head + 16ull * p; }

template <typename M>
DCMT_HD inline void crop_copy_piece(M& m, const RowCut& c, uint64_t dst, uint64_t src, uint32_t p, uint64_t lo, uint64_t hi)
{
    uint32_t w[8], o[4];
    const bool direct = crop_fetch_piece(m, c, src, p, lo, hi, w);
    crop_assemble(w, c.sh, direct, o);
    m.store16(crop_piece_dst(c, dst, p), o);
}

// Edge byte e of the row (crop_edge_pos): m.load8, m.store8(addr, value)
template <typename M>
DCMT_HD inline void crop_copy_edge(M& m, const RowCut& c, uint64_t dst, uint64_t src, uint32_t e)
{
    const uint32_t pos = crop_edge_pos(c, e);
    m.store8(dst + pos, m.load8(src + pos));
}

}  // namespace dcmt
