// dcmt_crop_frames_dev and dcmt_depth_to_u16_dev on a CPU: the record test, the cutting of a destination row and the copy of its
// pieces (csrc/dcmt_crop.h -- the statements k_crop_frames runs, here through a memory that checks every access), and the two
// launch plans (csrc/dcmt_plan_side.h).  Built and run by tests/test_crop.py; prints every failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <vector>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// A source buffer at byte address lo .. hi and a destination row at d .. d + len of a pretend address space.  Loads: every byte
// inside the source buffer; a byte load inside the row's own window; a 16-byte load at a multiple of 16 and inside the aligned quads
// around the window.  Stores: inside the destination row, a 16-byte store at a multiple of 16; every byte counted.
struct CheckedMem {
    uint64_t lo, hi;                         // the source buffer
    const uint8_t* src;                      // its bytes, src[0] at lo
    uint64_t win, win_end;                   // the row's window in the source
    uint64_t d, d_end;                       // the destination row
    std::vector<uint8_t> out;
    std::vector<int> written;
    int bad = 0;
    void row(uint64_t s, uint64_t dst, uint32_t len)
    {
        win = s; win_end = s + len; d = dst; d_end = dst + len;
        out.assign(len, 0xEE); written.assign(len, 0);
    }
    uint8_t byte(uint64_t a) { if (a < lo || a >= hi) { ++bad; return 0; } return src[a - lo]; }
    uint32_t load8(uint64_t a) { if (a < win || a >= win_end) ++bad; return byte(a); }
    void load16(uint64_t a, uint32_t* w)
    {
        if (a % 16 != 0 || a < (win & ~15ull) || a + 16 > ((win_end + 15) & ~15ull)) ++bad;
        for (int i = 0; i < 4; ++i)
            w[i] = (uint32_t)byte(a + 4 * i) | ((uint32_t)byte(a + 4 * i + 1) << 8) | ((uint32_t)byte(a + 4 * i + 2) << 16) | ((uint32_t)byte(a + 4 * i + 3) << 24);
    }
    void put(uint64_t a, uint8_t v) { if (a < d || a >= d_end) { ++bad; return; } out[a - d] = v; ++written[a - d]; }
    void store8(uint64_t a, uint32_t v) { put(a, (uint8_t)v); }
    void store16(uint64_t a, const uint32_t* o)
    {
        if (a % 16 != 0) ++bad;
        for (int i = 0; i < 16; ++i) put(a + i, (uint8_t)(o[i / 4] >> (8 * (i % 4))));
    }
};

// one row as a wave of k_crop_frames copies it (every lane's share, in any order)
static void copy_row(CheckedMem& m, uint64_t d, uint64_t s, uint32_t len)
{
    const RowCut c = crop_cut_row(d, s, len);
    CHECK(c.head + 16 * c.pieces + c.tail == len && c.head < 16 && c.tail < 16 && c.sh < 16);
    CHECK(c.head == len || (d + c.head) % 16 == 0);
    CHECK(c.sh == (s + c.head) % 16);
    for (uint32_t p = 0; p < c.pieces; ++p) {
        CHECK(crop_piece_first(c, s, p) % 16 == 0 && crop_piece_first(c, s, p) <= s + c.head + 16 * p);
        CHECK(crop_piece_last(c, s, p) >= s + c.head + 16 * p + 16 && crop_piece_last(c, s, p) - crop_piece_first(c, s, p) <= 32);
        crop_copy_piece(m, c, d, s, p, m.lo, m.hi);
    }
    for (uint32_t e = 0; e < c.head + c.tail; ++e) crop_copy_edge(m, c, d, s, e);
}

static void test_rows()
{
    uint8_t buf[400];
    for (int i = 0; i < 400; ++i) buf[i] = (uint8_t)(i * 7 + 13);
    int wide = 0, narrow = 0;
    for (uint32_t len = 1; len <= 70; ++len)
        for (uint32_t smis = 0; smis < 16; ++smis)               // 0..3 and every other position in a 16-byte quad
            for (uint32_t dmis = 0; dmis < 16; ++dmis)
                for (int place = 0; place < 3; ++place) {        // the row at the very start, at the very end, in the middle of the source
                    CheckedMem m;
                    m.lo = 0x1000 + smis;
                    const uint32_t src_bytes = place == 2 ? len + 80 : len + 37;
                    m.hi = m.lo + src_bytes;
                    m.src = buf;
                    const uint64_t s = place == 0 ? m.lo : place == 1 ? m.hi - len : m.lo + 40;
                    const uint64_t d = 0x9000 + dmis;
                    m.row(s, d, len);
                    copy_row(m, d, s, len);
                    CHECK(m.bad == 0);
                    bool all = true;
                    for (uint32_t i = 0; i < len; ++i) all = all && m.written[i] == 1 && m.out[i] == buf[s - m.lo + i];
                    CHECK(all);
                    const RowCut c = crop_cut_row(d, s, len);
                    for (uint32_t p = 0; p < c.pieces; ++p) (crop_piece_wide(c, s, p, m.lo, m.hi) ? wide : narrow)++;
                }
    CHECK(wide > 1000 && narrow > 1000);                         // both ways of loading a piece were taken
}

// whole frames, as the kernel walks them: record test, row addresses, rows; elem 1..4, pitched, the last row ending at src_bytes
static void test_frames()
{
    std::vector<uint8_t> buf(4096);
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = (uint8_t)(i * 31 + 5);
    for (uint32_t elem = 1; elem <= 4; ++elem)
        for (uint32_t len = elem; len <= 70; len += elem)
            for (uint32_t smis = 0; smis < 4; ++smis)
                for (uint32_t dmis = 0; dmis < 4; ++dmis) {
                    const int32_t out_cols = (int32_t)(len / elem), out_rows = 3, cols = out_cols + 3, rows = 5, x0 = (int32_t)(len % 4), y0 = 2;
                    const uint32_t stride = (uint32_t)cols * elem + 5;
                    const uint64_t offset = smis, src_bytes = offset + (uint64_t)(rows - 1) * stride + (uint64_t)cols * elem;   // ends with the frame
                    CHECK(x0 + out_cols <= cols);
                    CHECK(crop_record_ok(offset, stride, rows, cols, x0, y0, elem, out_rows, out_cols, src_bytes));
                    CHECK(!crop_record_ok(offset, stride, rows, cols, x0, y0, elem, out_rows, out_cols, src_bytes - 1));
                    CheckedMem m;
                    m.lo = 0x2000; m.hi = m.lo + src_bytes; m.src = buf.data();
                    const uint64_t dst = 0xA000 + dmis;
                    for (uint32_t r = 0; r < (uint32_t)out_rows; ++r) {
                        const uint64_t s = crop_row_src(m.lo, offset, stride, x0, y0, elem, r), d = crop_row_dst(dst, 2, out_rows, len, r);
                        CHECK(s == m.lo + offset + (uint64_t)(y0 + r) * stride + (uint64_t)x0 * elem && d == dst + (2ull * out_rows + r) * len);
                        m.row(s, d, len);
                        copy_row(m, d, s, len);
                        bool all = m.bad == 0;
                        for (uint32_t i = 0; i < len; ++i) all = all && m.written[i] == 1 && m.out[i] == buf[s - m.lo + i];
                        CHECK(all);
                    }
                }
}

static void test_assemble()
{
    uint8_t bytes[32];
    for (int i = 0; i < 32; ++i) bytes[i] = (uint8_t)(0x40 + i);
    uint32_t w[8];
    std::memcpy(w, bytes, 32);
    for (uint32_t sh = 0; sh < 16; ++sh) {
        uint32_t o[4];
        crop_assemble(w, sh, false, o);
        CHECK(std::memcmp(o, bytes + sh, 16) == 0);
        crop_assemble(w, sh, true, o);
        CHECK(std::memcmp(o, bytes, 16) == 0);
    }
    CHECK(crop_alignbyte(0x44332211u, 0xddccbbaau, 1) == 0x11ddccbbu && crop_alignbyte(0x44332211u, 0xddccbbaau, 3) == 0x332211ddu);
}

static void test_records()
{
    const uint64_t big = 1ull << 40;
    // a 375 x 1242 frame of uint16, KITTI window
    CHECK(crop_record_ok(0, 2484, 375, 1242, 13, 23, 2, 352, 1216, 375ull * 2484));
    // the window touching each of the four borders, and all of them
    CHECK(crop_record_ok(0, 40, 10, 20, 0, 3, 2, 4, 8, 400));
    CHECK(crop_record_ok(0, 40, 10, 20, 12, 3, 2, 4, 8, 400));
    CHECK(crop_record_ok(0, 40, 10, 20, 5, 0, 2, 4, 8, 400));
    CHECK(crop_record_ok(0, 40, 10, 20, 5, 6, 2, 4, 8, 400));
    CHECK(crop_record_ok(0, 40, 10, 20, 0, 0, 2, 10, 20, 400));
    // one step over each border
    CHECK(!crop_record_ok(0, 40, 10, 20, 13, 3, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 40, 10, 20, 5, 7, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 40, 10, 20, -1, 3, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 40, 10, 20, 5, -1, 2, 4, 8, 400));
    // sizes, stride
    CHECK(!crop_record_ok(0, 40, 0, 20, 0, 0, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 40, 10, 0, 0, 0, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 40, -10, 20, 0, 0, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 39, 10, 20, 0, 0, 2, 4, 8, 400));
    CHECK(crop_record_ok(0, 41, 10, 20, 0, 0, 2, 4, 8, 9 * 41 + 40));
    // the last frame ending exactly at src_bytes; one byte over; an offset at and behind the end
    CHECK(crop_record_ok(1000, 40, 10, 20, 0, 0, 2, 4, 8, 1400));
    CHECK(!crop_record_ok(1001, 40, 10, 20, 0, 0, 2, 4, 8, 1400));
    CHECK(!crop_record_ok(1000, 40, 10, 20, 0, 0, 2, 4, 8, 1399));
    CHECK(!crop_record_ok(1400, 40, 10, 20, 0, 0, 2, 4, 8, 1400));
    CHECK(!crop_record_ok(1401, 40, 10, 20, 0, 0, 2, 4, 8, 1400));
    CHECK(crop_record_ok(1399, 1, 1, 1, 0, 0, 1, 1, 1, 1400));
    // bait: values that wrap in 32 or 64 bits
    CHECK(!crop_record_ok(~0ull, 40, 10, 20, 0, 0, 2, 4, 8, 400));
    CHECK(!crop_record_ok(~0ull, 40, 10, 20, 0, 0, 2, 4, 8, ~0ull - 1));
    CHECK(!crop_record_ok(~0ull - 100, 40, 10, 20, 0, 0, 2, 4, 8, ~0ull));              // offset + extent wraps; src_bytes - offset does not
    CHECK(!crop_record_ok(0, 0xffffffffu, INT32_MAX, 20, 0, 0, 2, 4, 8, big));         // (2^31 - 2) * (2^32 - 1): near 2^63, no wrap
    CHECK(crop_record_ok(0, 0xffffffffu, INT32_MAX, 20, 0, 0, 2, 4, 8, (uint64_t)(INT32_MAX - 1) * 0xffffffffull + 40));
    CHECK(!crop_record_ok(0, 0xffffffffu, INT32_MAX, 20, 0, 0, 2, 4, 8, (uint64_t)(INT32_MAX - 1) * 0xffffffffull + 39));
    CHECK(!crop_record_ok(0, 40, 10, 20, INT32_MAX, 0, 2, 4, 8, 400));                 // x0 + out_cols wraps in 32 bits
    CHECK(!crop_record_ok(0, 40, 10, 20, INT32_MAX - 7, 0, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 40, 10, 20, 0, INT32_MAX, 2, 4, 8, 400));
    CHECK(!crop_record_ok(0, 40, 10, INT32_MAX, INT32_MAX - 8, 0, 4, 4, 8, big));      // cols * elem = 2^33 - 4 > row_stride
    CHECK(!crop_record_ok(0, 0xffffffffu, 2, INT32_MAX, INT32_MAX - 8, 0, 4, 2, 8, big));
    CHECK(crop_record_ok(0, 0xfffffffeu, 2, INT32_MAX, INT32_MAX - 8, 0, 2, 2, 8, 3ull * 0xfffffffeull));
    CHECK(!crop_record_ok(0, 40, INT32_MIN, 20, 0, 0, 2, 4, 8, big));
    CHECK(!crop_record_ok(0, 40, 10, 20, INT32_MIN, INT32_MIN, 2, 4, 8, big));
}

constexpr uintptr_t kSrc = 0x100000000ull, kTab = 0x900000000ull, kDst = 0x1100000000ull;

static CropPlan checked_crop(int out_rows, int out_cols, int batch, int elem)
{
    const CropPlan p = plan_crop(out_rows, out_cols, batch, elem, kSrc, 1000, kTab, kDst);
    CHECK(p.status == kOk);
    CHECK(p.band >= (uint32_t)kCropWaves && (p.band & (p.band - 1)) == 0);
    CHECK(p.grid_y == (unsigned)batch && p.grid_y <= 65535u);
    CHECK((uint64_t)p.grid_x * p.band >= (uint64_t)out_rows && (uint64_t)(p.grid_x - 1) * p.band < (uint64_t)out_rows);
    CHECK((uint64_t)p.grid_x * kCropThreads < (1ull << 32));                            // a grid dimension in threads
    CHECK((uint64_t)p.grid_x * p.band < (1ull << 32));                                   // the kernel's 32-bit blockIdx.x * band
    CHECK(p.dst_bytes == (size_t)batch * out_rows * out_cols * elem);
    return p;
}

static void test_crop_plan()
{
    CropPlan p = checked_crop(352, 1216, 1024, 2);
    CHECK(p.band == kCropBandRows && p.grid_x == 22);
    p = checked_crop(352, 1216, 65535, 3);
    CHECK(p.band == kCropBandRows && p.grid_x == 22);
    p = checked_crop(352, 1216, 1, 4);
    CHECK(p.band == (uint32_t)kCropWaves && p.grid_x == 88);
    p = checked_crop(1, 1, 1, 1);                                                       // the smallest frame
    CHECK(p.grid_x == 1);
    p = checked_crop(1, 1, 65535, 1);
    CHECK(p.grid_x == 1);
    p = checked_crop(0x1ffffff0, 1, 1, 4);                                              // the largest frames dcmt_create admits
    CHECK(p.grid_x <= (1u << 20));
    p = checked_crop(0x1ffffff0, 1, 65535, 4);
    CHECK(p.grid_x <= (1u << 20));
    p = checked_crop(1, 0x1ffffff0, 65535, 4);
    CHECK(p.grid_x == 1 && (uint64_t)0x1ffffff0 * 4 < (1ull << 31));                     // a row's bytes fit the kernel's 32-bit len
    // the checks
    CHECK(plan_crop(8, 8, 2, 0, kSrc, 1000, kTab, kDst).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 5, kSrc, 1000, kTab, kDst).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, 0, 1000, kTab, kDst).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, 0, kDst).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, 0).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 0, kTab, kDst).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab + 4, kDst).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, kSrc + 3, 1000, kTab + 8, kDst + 1).status == kOk);        // any byte alignment of source and destination
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kSrc + 999).status == kInvalid);          // dst against the source range, both ends
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kSrc + 1000).status == kOk);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kSrc - 255).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kSrc - 256).status == kOk);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kTab + 63).status == kInvalid);           // dst against the table's batch * 32 bytes
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kTab + 64).status == kOk);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kTab - 255).status == kInvalid);
    CHECK(plan_crop(8, 8, 2, 2, kSrc, 1000, kTab, kTab - 256).status == kOk);
}

static void test_u16_plan()
{
    const uintptr_t in = kSrc, out = kDst;
    U16Plan p = plan_depth_to_u16(1024 * 352 * 1216, in, out);
    CHECK(p.status == kOk && p.count == 1 && p.aligned && p.segment(0).total == 1024u * 352 * 1216 && p.segment(0).grid == (1024u * 352 * 1216 + 2047) / 2048);
    p = plan_depth_to_u16(1, in, out);
    CHECK(p.status == kOk && p.count == 1 && p.segment(0).grid == 1 && p.segment(0).total == 1);
    for (uintptr_t off = 0; off < 32; off += 2) {
        CHECK(plan_depth_to_u16(100, in, out + off).status == kOk && plan_depth_to_u16(100, in, out + off).aligned == (off % 16 == 0));
        CHECK(plan_depth_to_u16(100, in + 2 * off, out).status == kOk && plan_depth_to_u16(100, in + 2 * off, out).aligned == ((2 * off) % 16 == 0));
    }
    CHECK(plan_depth_to_u16(100, in + 2, out).status == kInvalid && plan_depth_to_u16(100, in, out + 1).status == kInvalid);
    CHECK(plan_depth_to_u16(100, 0, out).status == kInvalid && plan_depth_to_u16(100, in, 0).status == kInvalid && plan_depth_to_u16(0, in, out).status == kInvalid);
    // any overlap: out inside, at both ends of and next to depth
    CHECK(plan_depth_to_u16(100, in, in).status == kInvalid && plan_depth_to_u16(100, in, in + 398).status == kInvalid);
    CHECK(plan_depth_to_u16(100, in, in + 400).status == kOk);
    CHECK(plan_depth_to_u16(100, in, in - 198).status == kInvalid && plan_depth_to_u16(100, in, in - 200).status == kOk);
    // segments: the cap, one more, the largest call
    p = plan_depth_to_u16(kU16SegPx, in, out);
    CHECK(p.count == 1 && (uint64_t)p.segment(0).grid * kU16PxPerWg == kU16SegPx);
    p = plan_depth_to_u16((size_t)kU16SegPx + 1, in, out);
    CHECK(p.count == 2 && p.segment(1).first == kU16SegPx && p.segment(1).total == 1 && p.segment(1).grid == 1);
    CHECK((4 * (uint64_t)kU16SegPx) % 16 == 0 && (2 * (uint64_t)kU16SegPx) % 16 == 0);
    CHECK((uint64_t)kU16SegPx + kU16PxPerWg <= (1ull << 32));                            // the kernel's 32-bit pixel index with the overhang
    const size_t huge = (size_t)65535 * 0x1ffffff0u;
    p = plan_depth_to_u16(huge, in, in + 4 * huge);
    const U16Segment last = p.segment(p.count - 1);
    CHECK(p.status == kOk && last.first + last.total == huge && last.total >= 1 && last.total <= kU16SegPx);
}

int main()
{
    test_assemble();
    test_rows();
    test_frames();
    test_records();
    test_crop_plan();
    test_u16_plan();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
