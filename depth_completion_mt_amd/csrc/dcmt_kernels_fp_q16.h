// dcmt_kernels_fp_q16.h -- k_fp_q: H7, H9..H11 for frames whose depths are multiples of 1/256 m (the KITTI depth format: every
// frame the reference's lidar-only and lidar-camera callers feed the path is a uint16 PNG payload / 256, LO/main.cpp:75-82).
//
// H2..H9 only ever SELECT values (max, min, median), so on such a frame every value of X2..X9 is one of
//     j / 256,   j in [-5119, 25600]         (an empty pixel k / 256 with k < 26, an inverted depth (25600 - k) / 256, or the 100
//                                             of a column without valid pixels, LO :110)
// -- with max_depth = 100 and thr = 0.1 (the reference's constants; other values run the f32 kernels).  code = j + 6143 (Q16,
// dcmt_kernels_fused.h) is 0x0400 .. 0x7bff: the map is strictly increasing, so maxima / minima / medians of codes are the codes of the
// f32 results, and a hole (x < 0.1f) is code <= 6168.  Two adjacent columns then fit ONE register (low half = column 2l, high half =
// column 2l + 1) and packed instructions work on both at the price of one v_max_f32: two columns per lane without a doubled register
// state -- this kernel keeps 3 waves per SIMD.
//
// Which packed instructions: the code range is the bit patterns of the positive NORMAL half-floats, which order as f16 exactly as they
// do as u16.  gfx950 has packed two-input minima / maxima for u16 AND packed THREE-input ones for f16 (v_pk_maximum3_f16 /
// v_pk_minimum3_f16, VOP3P, new on gfx950; tools/pk3_probe.hip: exact on these patterns, one v_pk_max_u16's issue cost) -- but no packed
// med3 of any type.  (Round 2 wrote "no packed three-input min / max" here; that was wrong.)  So: the vertical 31-row maximum is 4
// three-input instructions per register instead of 6; the median keeps its two-input MERGE55 (26), takes MID20 with two exchanges folded
// (34, median_pk3_nets.h), sort5 from min3 / max3 and XORs (10 + 5), the closing selection with its minimum in two min3 (8): 53 + 4
// neighbour moves per row for two columns (k_fp_s: 38.5 per column with v_med3_f32).  The three-input networks of
// median_shared_nets3.h are half med3 and gain nothing here: a med3 emulated from min3 + max3 + two XORs (or two v_med3_f16 on the
// halves) costs what the exchange it replaces costs.
// Behind the median: where the redo chain follows (FILLED), Gaussian and final invert run on the codes as integer-valued floats --
// exact arithmetic, nothing rounds in the oracle's sequence either (PostPipeP::after_median_codes has the argument); otherwise the
// median is converted back (code -> f32 is exact: one v_cvt and one fused multiply-add) and the Gaussian, the masked select and the
// final invert run in f32 (PostPipeP::after_median).  Either way the output is bit-identical to k_fp_s's.
//
// Lane layout: a wave owns 128 columns, lane l the columns c0 + 2l ("E", low half) and c0 + 2l + 1 ("O", high half), 120 of them output
// (2 + 2 per side go to the median and the Gaussian).  The 15 + 15 halo columns of the 31-wide maximum ride in a second register B, one
// column per lane, unpacked: even columns of the right halo in lanes 0..7, odd ones in 8..15, even columns of the left halo in lanes
// 56..63, odd ones in 48..55; lanes 16..47 are dead.  144..152 VGPRs: 3 waves per SIMD.
// Fill: the vertical 31-maximum runs packed; the horizontal one, on rows that have a hole, works on the unpacked halves (unsigned
// integers: 0 is the neutral element).  tests/test_lane_schemes.py restates this index arithmetic in numpy and checks it lane by lane
// against the definition.  m = max(E, O) per lane; PX / SX = EXCLUSIVE prefix / suffix maxima of m inside each 16-lane DPP row (the
// inclusive row scans, then one row_shr:1 / row_shl:1 that leaves 0 in the lane without a source).  The window of column 2l is O[l-8],
// lanes l-7 .. l+7; that of column 2l+1 is lanes l-7 .. l+7, E[l+8]:
//     out_E(l) = max( SO(l-8), PX(l+8) )        SO = max(O, SX)   (suffix starting at a lane's odd column)
//     out_O(l) = max( SX(l-8), PE(l+8) )        PE = max(E, PX)   (prefix ending at a lane's even column)
// -- lanes l-8 and l+8 lie in neighbouring DPP rows, each term covers its row's part of the window, and where the window lies inside
// ONE row (l = 8 mod 16 for E, 7 mod 16 for O) the other term is the 0 of an exclusive scan's first lane.  The halo: virtual lanes
// 64..71 (the 16 columns right of the strip) and -8..-1 (left) wrap onto physical lanes 0..7 and 56..63 of B's scans; one row_ror:8
// puts a virtual lane's odd column beside its even one, and the values handed on are selected per SOURCE lane.  The two values a lane
// fetches from lane l - 8 ride in one word, so do the two from lane l + 8: two ds_bpermutes.
//
// X6 arrives as the codes themselves (k_pre_p<Q16OUT>, which has checked the frame's values and raised a flag otherwise -- dcmt.hip
// reruns the f32 kernels behind that flag, so what this kernel makes of a frame that is no grid is never looked at).
#pragma once

#include "dcmt_kernels_pair.h"
#include "median_pk3_nets.h"

namespace dcmt {

typedef unsigned short us2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned qmax(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2v, a), __builtin_bit_cast(us2v, b)));
}
__device__ __forceinline__ unsigned qmin(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(us2v, a), __builtin_bit_cast(us2v, b)));
}
__device__ __forceinline__ unsigned umax2(unsigned a, unsigned b) { return a > b ? a : b; }

// The codes are ordered as f16 too (Q16, dcmt_kernels_fused.h), and for f16 -- for nothing else 16 bits wide -- gfx950 has packed THREE-input
// minima / maxima: v_pk_maximum3_f16 / v_pk_minimum3_f16 (tools/pk3_probe.hip: exact on these bit patterns, the price of one v_pk_max_u16).
typedef _Float16 hf2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned hmax2(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_maximum(__builtin_bit_cast(hf2v, a), __builtin_bit_cast(hf2v, b)));
}
__device__ __forceinline__ unsigned hmin2(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_minimum(__builtin_bit_cast(hf2v, a), __builtin_bit_cast(hf2v, b)));
}
__device__ __forceinline__ unsigned hmax3(unsigned a, unsigned b, unsigned c)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(hf2v, a), __builtin_bit_cast(hf2v, b)), __builtin_bit_cast(hf2v, c)));
}
__device__ __forceinline__ unsigned hmin3(unsigned a, unsigned b, unsigned c)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_minimum(__builtin_elementwise_minimum(__builtin_bit_cast(hf2v, a), __builtin_bit_cast(hf2v, b)), __builtin_bit_cast(hf2v, c)));
}

// shifts with 0 in the lane without a source (unsigned codes: 0 is the neutral element of max)
__device__ __forceinline__ unsigned u_left(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned u_right(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /*wave_shl:1*/, 0xf, 0xf, true); }
// (bound_ctrl: a lane without a source reads 0 -- what `old = 0` gave, without the v_mov that sets it up)
__device__ __forceinline__ unsigned u_row_shr1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned u_row_shl1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned u_row_ror8(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true); }
// The inclusive prefix / suffix maxima inside each 16-lane DPP row.  The first step writes the two scans from the source itself
// (bound_ctrl: max(0, x) = x in a lane without a source): no copies.  A's scans take four steps (1, 2, 4, 8 lanes); B's are only
// looked at in lanes 0..7 (prefix) and 56..63 (suffix) -- eight lanes each, three steps -- and only on rows with a hole in those
// lanes (fill_step), so they are a block of their own.
// (a DPP read of a register needs two wait states behind the VALU write: with two chains side by side, one instruction and an s_nop)
#define DCMT_U2(N) "s_nop 0\n\t" \
                   "v_max_u32_dpp %0, %0, %0 row_shr:" #N " row_mask:0xf bank_mask:0xf\n\t" \
                   "v_max_u32_dpp %1, %1, %1 row_shl:" #N " row_mask:0xf bank_mask:0xf\n\t"
#define DCMT_U2_FIRST "s_nop 1\n\t" \
                      "v_max_u32_dpp %0, %2, %2 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
                      "v_max_u32_dpp %1, %2, %2 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
// (the compiler does not see the writes of an asm block: whatever shifts a scan next finds its two wait states here)
#define DCMT_U2_LAST "s_nop 1\n\t"
__device__ __forceinline__ void u_row_scans_a(unsigned a, unsigned& pa, unsigned& sa)
{
    asm(DCMT_U2_FIRST DCMT_U2(2) DCMT_U2(4) DCMT_U2(8) DCMT_U2_LAST : "=&v"(pa), "=&v"(sa) : "v"(a));
}
__device__ __forceinline__ void u_row_scans_b(unsigned b, unsigned& pb, unsigned& sb)
{
    asm(DCMT_U2_FIRST DCMT_U2(2) DCMT_U2(4) DCMT_U2_LAST : "=&v"(pb), "=&v"(sb) : "v"(b));
}
#undef DCMT_U2_LAST
#undef DCMT_U2_FIRST
#undef DCMT_U2

// The exact 5x5 median of dcmt_median.h on packed pairs: the two-input MERGE55 of median_shared_nets.h (the three-input forms
// need a packed med3, which does not exist), MID20 from median_pk3_nets.h, sort5 and the closing selection below.
#define DCMT_QCX(a, b)   { const unsigned lo_ = qmin(v[a], v[b]); v[b] = qmax(v[a], v[b]); v[a] = lo_; }
#define DCMT_QCMIN(a, b) { v[a] = qmin(v[a], v[b]); }
#define DCMT_QCMAX(a, b) { v[b] = qmax(v[a], v[b]); }
// sort5 with the three-input instructions: (a, b, c) = sort3(v0, v1, v2) as min3 / max3 and the middle one as the XOR of the five (a
// multiset identity, exact on bit patterns, ties included: v_bitop3_b32 0x96), (d, e) = sort2(v3, v4), then the merge of 3 + 2 by rank:
//     s0 = min(a, d)   s1 = min3(max(a, d), b, e)   s3 = max3(min(c, e), b, d)   s4 = max(c, e)   s2 = XOR of the five inputs and the other four
// 10 min / max + 5 XORs (3.9 cycles each, tools/pk3_probe.hip) instead of 18 min / max.  Checked exhaustively against sorted() on
// five values of five levels (tests/test_lane_schemes.py restates it).
__device__ __forceinline__ unsigned xor3(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ void q_sort5(unsigned (&v)[5])
{
    const unsigned a = hmin3(v[0], v[1], v[2]), c = hmax3(v[0], v[1], v[2]), t = xor3(v[0], v[1], v[2]), b = xor3(t, a, c);
    const unsigned d = hmin2(v[3], v[4]), e = hmax2(v[3], v[4]);
    const unsigned s0 = hmin2(a, d), s4 = hmax2(c, e);
    const unsigned s1 = hmin3(hmax2(a, d), b, e), s3 = hmax3(hmin2(c, e), b, d);
    const unsigned s2 = xor3(xor3(t, v[3], v[4]), xor3(s0, s1, s3), s4);
    v[0] = s0; v[1] = s1; v[2] = s2; v[3] = s3; v[4] = s4;
}
__device__ __forceinline__ void q_merge55(const unsigned (&a)[5], const unsigned (&b)[5], unsigned (&P)[10])
{
    constexpr int out[10] = DCMT_MERGE55_OUT;
    unsigned v[10];
#pragma unroll
    for (int k = 0; k < 5; ++k) { v[k] = a[k]; v[5 + k] = b[k]; }
    DCMT_MERGE55_NET(DCMT_QCX, DCMT_QCMIN, DCMT_QCMAX)
#pragma unroll
    for (int k = 0; k < 10; ++k) P[k] = v[out[k]];
}
__device__ __forceinline__ void q_mid20(const unsigned (&pa)[10], const unsigned (&pb)[10], unsigned (&C)[6])
{
    // (median_pk3_nets.h: the two-input network with two of its exchanges folded into min3 / max3)
#define DCMT_IN_(k) ((k) < 10 ? pa[(k) < 10 ? (k) : 0] : pb[(k) >= 10 ? (k) - 10 : 0])
#define DCMT_OUT_(k) C[k]
    DCMT_MID20_PK3(DCMT_IN_, DCMT_OUT_)
#undef DCMT_IN_
#undef DCMT_OUT_
}
#undef DCMT_QCX
#undef DCMT_QCMIN
#undef DCMT_QCMAX
// 6th smallest of sorted C (6) u sorted a (5): min(C5, max(a0,C4), max(a1,C3), max(a2,C2), max(a3,C1), max(a4,C0)); the six-way minimum
// in three-input instructions: 5 + 3 instead of 5 + 5
__device__ __forceinline__ unsigned q_final6(const unsigned (&C)[6], const unsigned (&a)[5])
{
    const unsigned m0 = hmax2(a[0], C[4]), m1 = hmax2(a[1], C[3]), m2 = hmax2(a[2], C[2]), m3 = hmax2(a[3], C[1]), m4 = hmax2(a[4], C[0]);
    return hmin2(hmin3(C[5], m0, m1), hmin3(m2, m3, m4));
}
struct MedianColumnQ {       // MedianColumn (dcmt_median.h) on packed pairs
    unsigned SE[4][5], SO[5], P[2][10], C[6];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 5; ++k) SE[q][k] = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) SO[k] = 0;
#pragma unroll
        for (int k = 0; k < 10; ++k) { P[0][k] = 0; P[1][k] = 0; }
#pragma unroll
        for (int k = 0; k < 6; ++k) C[k] = 0;
    }
    template <int PP>
    __device__ __forceinline__ unsigned step(const unsigned (&s)[5])
    {
        unsigned m;
        if constexpr ((PP & 1) == 0) {
            constexpr int qs = (PP >> 1) & 3;
            q_merge55(SO, s, P[(PP >> 1) & 1]);
            q_mid20(P[((PP >> 1) + 1) & 1], P[(PP >> 1) & 1], C);
            m = q_final6(C, SE[(qs + 2) & 3]);
#pragma unroll
            for (int k = 0; k < 5; ++k) SE[qs][k] = s[k];
        } else {
            m = q_final6(C, s);
#pragma unroll
            for (int k = 0; k < 5; ++k) SO[k] = s[k];
        }
        return m;
    }
};

struct FpQ {
    static constexpr int H = 4;                  // columns lost per side: 2 (median) + 2 (Gaussian)
    static constexpr int VW = 128 - 2 * H;       // output columns per wave
};

// The output rows: written once, read by nobody in the launch (k_tail reads the few frames it redoes, a launch later).  As ordinary
// stores the 1.75 GB of a 1024-frame call pass through the L2 beside the X6 rows and halo columns that neighbouring strips are
// about to read again; with the `nt` bit (non-temporal: streamed, not kept) the step takes about 5 % less time -- DESIGN.md section 5.
__device__ __forceinline__ void st2_nt(const FrameBuf& b, unsigned lane_bytes, int row, int cols, F2 v)
{
    const f2v f = {v.e, v.o};
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, f), b.rs, lane_bytes, row * cols * 4, 2 /* nt */);
}

// k_fp_q's tail behind the median, two columns per lane.  Step u finishes the output of image row u - 6 from the median of image
// row u - 4.
template <bool BLUR>
struct PostPipeP {
    F2 G1[8], MR[8];
    F2 last_out;
    FrameBuf of;
    unsigned ob;             // byte offset of this lane's (clamped) column pair
    int rows, cols, gx, rle, rlo;
    bool outlane, edge_strip, outside;
    float max_depth, thr;

    __device__ __forceinline__ void init(float* out_frame, int rows_, int cols_, int gx0, int lane, float max_depth_, float thr_)
    {
        of.init(out_frame, (size_t)rows_ * cols_); rows = rows_; cols = cols_; max_depth = max_depth_; thr = thr_;
        gx = gx0 + 2 * lane;
        ob = 4u * (unsigned)min(max(gx, 0), cols - 2);
        outside = gx < 0 || gx >= cols;                            // cols and gx are even: both columns inside or both outside
        outlane = !outside && 2 * lane >= FpQ::H && 2 * lane < 128 - FpQ::H;
        // reflect-101 sources of the Gaussian's out-of-image columns: parity is preserved (cols is even), so E comes from an E slot, O from an O slot
        rle = (reflect101(gx, cols) - gx0) >> 1;
        rlo = (reflect101(gx + 1, cols) - 1 - gx0) >> 1;
        edge_strip = gx0 < 0 || gx0 + 127 >= cols;
        last_out = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 8; ++q) { G1[q] = {0.f, 0.f}; MR[q] = {0.f, 0.f}; }
    }

    // MODE: what the caller knows about the step at compile time.  BORDER: nothing -- every row-range test runs.  INNER: the output
    // row u - 6 lies in [2, rows - 3] -- no row test, the Gaussian's plain rows.  (edge_strip stays a wave-uniform branch in both:
    // a second instantiation of the interior body for edge strips costs 70 VGPRs, k_fp_q's main loop has the figures.)
    enum { BORDER = 0, INNER = 1 };

    // everything behind the median of image row u - 4 (me, mo = its two columns) in f32: H10, H11, the store of output row u - 6
    template <int PP, int MODE = BORDER>
    __device__ __forceinline__ void after_median(float me, float mo, int u)
    {
        MR[(PP + 4) & 7] = {me, mo};
        // ---- H10 (LO :179): horizontal [1 4 6 4 1]/16 with reflect-101 columns
        if constexpr (BLUR) {
            F2 mf = {me, mo};
            if (edge_strip) {
                const float re = __shfl(me, rle, 64), ro = __shfl(mo, rlo, 64);
                if (outside) mf = {re, ro};
            }
            const float el = from_left(mf.e), ol = from_left(mf.o), er = from_right(mf.e), orr = from_right(mf.o);
            // column 2l: neighbours O[l-1], O | E[l-1], E[l+1];  column 2l+1: E, E[l+1] | O[l-1], O[l+1]
            G1[(PP + 4) & 7] = {gauss_taps(mf.e, __fadd_rn(ol, mf.o), __fadd_rn(el, er)), gauss_taps(mf.o, __fadd_rn(mf.e, er), __fadd_rn(ol, orr))};
        }
        // ---- vertical pass + select + invert for output row o = u - 6
        const int o = u - 6;
        if (MODE != BORDER || (unsigned)o < (unsigned)rows) {
            const F2 mo_ = MR[(PP + 2) & 7];
            auto finish = [&](F2 u1, F2 u2, F2 d1, F2 d2) {
                F2 val = mo_;
                if constexpr (BLUR) {
                    const F2 g0 = G1[(PP + 2) & 7];
                    const float ae = gauss_taps(g0.e, __fadd_rn(u1.e, d1.e), __fadd_rn(u2.e, d2.e));
                    const float ao = gauss_taps(g0.o, __fadd_rn(u1.o, d1.o), __fadd_rn(u2.o, d2.o));
                    if (mo_.e >= thr) val.e = ae;                        // LO :184
                    if (mo_.o >= thr) val.o = ao;
                }
                val = {invert_valid(val.e, max_depth, thr), invert_valid(val.o, max_depth, thr)};   // LO :191-202
                st2_nt(of, outlane ? ob : kDropOffset, o, cols, val);
                last_out = val;
            };
            const F2 g_p2 = G1[(PP + 4) & 7], g_p1 = G1[(PP + 3) & 7], g_0 = G1[(PP + 2) & 7], g_m1 = G1[(PP + 1) & 7], g_m2 = G1[PP];
            if (BLUR && MODE == BORDER && (o < 2 || o + 2 >= rows)) {    // reflect-101 rows (rows >= 8 guaranteed)
                finish(o >= 1 ? g_m1 : g_p1,
                       o >= 2 ? g_m2 : (o == 1 ? g_0 : g_p2),
                       o + 1 < rows ? g_p1 : g_m1,
                       o + 2 < rows ? g_p2 : (o + 2 == rows ? g_0 : g_m2));
            } else {
                finish(g_m1, g_m2, g_p1, g_p2);
            }
        }
    }

    // The same on the packed medians m = (code_E, code_O), where the redo chain follows (k_fp_q<BLUR, FILLED>): IN EXACT ARITHMETIC.  A code is an integer
    // below 2^15, value = (code - 6143) / 256.  The horizontal pass of the reference order  c*k0 + s1*k1 + s2*k2  on such values only
    // ever forms multiples of 2^-12 below 128 (19 bits), the vertical pass multiples of 2^-16 below 128 (23 bits), and the final
    // 100 - value is a multiple of 2^-16 below 128 too: no operation of the oracle's sequence rounds, so any other sequence
    // without a rounding gives the same bits.  This one works on the codes as integer-valued floats with the weights 1 4 6 4 1
    // (horizontal sums <= 16 * 31743 < 2^19, vertical <= 256 * 31743 < 2^23) and scales once at the end:
    //     out = 100 - (N / 65536 - 6143 / 256) = fma(N, -2^-16, 123.99609375).
    // Horizontal, two columns per lane, four lane shifts (each folded into an add):  S1 = O[l-1] + O,  S2 = E + E[l+1],
    //     G_E = 4 (E + S1) + (S2[l-1] + S2) = 6 E + 4 (O[l-1] + O) + E[l-1] + E[l+1],   G_O = 4 (O + S2) + (S1 + S1[l+1]):
    // 2 conversions + 8 + 2 * 4 + 2 instructions per row step instead of 4 + 14 + 10 + 2.
    template <int PP, int MODE = BORDER>
    __device__ __forceinline__ void after_median_codes(unsigned m, int u)
    {
        static_assert(BLUR, "exact only on grid values; the select of LO :184 is not in here");
        float ce = (float)(m & 0xffffu), co = (float)(m >> 16);
        if (edge_strip) {
            const float re = __shfl(ce, rle, 64), ro = __shfl(co, rlo, 64);
            if (outside) { ce = re; co = ro; }
        }
        // (each of the four sums is ONE v_add_f32 with the lane shift as its DPP operand -- as long as the two sums of a line are
        // not paired into a v_pk_add_f32, which has no DPP form and takes a v_mov_b32_dpp per shift: the empty asm makes the
        // second sum's operand a value that exists only behind the first, so the two cannot be bundled)
        float s1 = __fadd_rn(from_left(co), co);
        asm("" : "+v"(ce) : "v"(s1));
        const float s2 = __fadd_rn(ce, from_right(ce));
        const float ue = __fadd_rn(from_left(s2), s2);
        asm("" : "+v"(s1) : "v"(ue));
        const float wo = __fadd_rn(from_right(s1), s1);
        G1[(PP + 4) & 7] = {__builtin_fmaf(__fadd_rn(ce, s1), 4.0f, ue), __builtin_fmaf(__fadd_rn(co, s2), 4.0f, wo)};
        const int o = u - 6;
        if (MODE != BORDER || (unsigned)o < (unsigned)rows) {
            const float top = __fadd_rn(max_depth, (float)Q16::OFFSET * 0.00390625f);     // 100 + 6143 / 256: exact
            auto finish = [&](F2 u1, F2 u2, F2 d1, F2 d2) {
                const F2 g0 = G1[(PP + 2) & 7];
                const float ne = __builtin_fmaf(g0.e, 6.0f, __builtin_fmaf(__fadd_rn(u1.e, d1.e), 4.0f, __fadd_rn(u2.e, d2.e)));
                const float no = __builtin_fmaf(g0.o, 6.0f, __builtin_fmaf(__fadd_rn(u1.o, d1.o), 4.0f, __fadd_rn(u2.o, d2.o)));
                const F2 val = {__builtin_fmaf(ne, -0x1p-16f, top), __builtin_fmaf(no, -0x1p-16f, top)};
                st2_nt(of, outlane ? ob : kDropOffset, o, cols, val);
                last_out = val;
            };
            const F2 g_p2 = G1[(PP + 4) & 7], g_p1 = G1[(PP + 3) & 7], g_0 = G1[(PP + 2) & 7], g_m1 = G1[(PP + 1) & 7], g_m2 = G1[PP];
            if (MODE == BORDER && (o < 2 || o + 2 >= rows)) {            // reflect-101 rows, as above
                finish(o >= 1 ? g_m1 : g_p1,
                       o >= 2 ? g_m2 : (o == 1 ? g_0 : g_p2),
                       o + 1 < rows ? g_p1 : g_m1,
                       o + 2 < rows ? g_p2 : (o + 2 == rows ? g_0 : g_m2));
            } else {
                finish(g_m1, g_m2, g_p1, g_p2);
            }
        }
    }
};

#ifndef DCMT_FPQ_WAVES
#define DCMT_FPQ_WAVES 0
#endif
#ifndef DCMT_FPQ_PFD
#define DCMT_FPQ_PFD 6
#endif
template <bool BLUR, bool FILLED>
__global__ __launch_bounds__(256)
#if DCMT_FPQ_WAVES
__attribute__((amdgpu_waves_per_eu(DCMT_FPQ_WAVES, DCMT_FPQ_WAVES)))
#endif
void k_fp_q(const void* __restrict__ x6_, float* __restrict__ dst, int* __restrict__ counters,
            int rows_all, int cols, int strips, int batch, int xcd_map, float max_depth, float thr, const int* __restrict__ tb,
            int tbands)
{
    // per wave: centre values and A's 18-row maxima (packed pairs, one word per lane), B's 18-row maxima
    __shared__ unsigned s_delay[4][16 * (64 + 64 + 32)];            // 10 KiB per wave, 40 KiB per workgroup
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int f, strip;
    if (!wave_strip(blockIdx.x, wave, strips, batch, xcd_map, f, strip)) return;
    int* cnt = frame_counters(counters, f);
    const size_t fo = (size_t)f * rows_all * cols;
    const int gx0 = strip * FpQ::VW - FpQ::H;
    const int gxe = gx0 + 2 * lane;
    // B, one column per lane, unpacked (header comment).  The dead lanes 16..47 (two whole DPP rows) shadow lane 0: same column,
    // same values, same delay-line word -- their stores write what lane 0 writes
    const int gxb = lane < 8 ? gx0 + 128 + 2 * lane : (lane < 16 ? gx0 + 128 + 2 * (lane - 8) + 1 :
                    (lane >= 56 ? gx0 - 16 + 2 * (lane - 56) : (lane >= 48 ? gx0 - 16 + 2 * (lane - 48) + 1 : gx0 + 128)));
    const int gxec = min(max(gxe, 0), cols - 2), gxoc = gxec + 1, gxbc = min(max(gxb, 0), cols - 1);
    int tie = 0, tio = 0, tib = 0, bie = rows_all - 1, bio = rows_all - 1, bib = rows_all - 1, V = 0;
    if (tb) {
        table_rows(tb, f, cols, tbands, rows_all, gxec, tie, bie);
        table_rows(tb, f, cols, tbands, rows_all, gxoc, tio, bio);
        table_rows(tb, f, cols, tbands, rows_all, gxbc, tib, bib);
        V = __builtin_amdgcn_readfirstlane(max(wave_min_i(min(min(tie, tio), tib)) - 8, 0));
    }
    const int rows = rows_all - V;
    constexpr unsigned EB = 2;                                       // bytes per code
    FrameBuf sf;
    sf.init(reinterpret_cast<const float*>(static_cast<const char*>(x6_) + fo * EB), (size_t)rows_all * cols * EB / 4);
    const unsigned rowb = EB * (unsigned)cols;
    const unsigned sbe = EB * (unsigned)gxec + (unsigned)V * rowb, sbo = sbe + EB, sbb = EB * (unsigned)gxbc + (unsigned)V * rowb;
    const unsigned fle = EB * (unsigned)gxec + (unsigned)max(tie, V) * rowb, cee = EB * (unsigned)gxec + (unsigned)max(bie, V) * rowb;
    const unsigned flo = EB * (unsigned)gxoc + (unsigned)max(tio, V) * rowb, ceo = EB * (unsigned)gxoc + (unsigned)max(bio, V) * rowb;
    const unsigned flb = EB * (unsigned)gxbc + (unsigned)max(tib, V) * rowb, ceb = EB * (unsigned)gxbc + (unsigned)max(bib, V) * rowb;
    auto clamp3 = [](unsigned a, unsigned lo, unsigned hi) -> unsigned { unsigned r; asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(lo), "v"(hi)); return r; };
    // one column's code at a (clamped) byte offset
    // (what the load instruction returned, 16 bits: widening and packing are arithmetic on the result and belong to the step that consumes it)
    auto ld_code = [&](unsigned off) -> unsigned short { return (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(sf.rs, off, 0, 0); };
    struct Raw { unsigned short e, o, b; };
    auto ld_row = [&](int row) -> Raw {                              // row relative to V, already clamped to [0, rows)
        return Raw{ld_code(clamp3(sbe + (unsigned)row * rowb, fle, cee)), ld_code(clamp3(sbo + (unsigned)row * rowb, flo, ceo)),
                   ld_code(clamp3(sbb + (unsigned)row * rowb, flb, ceb))};
    };
    auto pack = [](unsigned short e, unsigned short o) -> unsigned { return (unsigned)e | ((unsigned)o << 16); };
    const bool outside = gxe < 0 || gxe >= cols;
    const bool own = !outside && 2 * lane >= FpQ::H && 2 * lane < 128 - FpQ::H;
    const unsigned long long own_mask = __ballot(own);
    const bool edge_strip = gx0 < 0 || gx0 + 127 >= cols;
    const int rep_l = min(max((0 - gx0) >> 1, 0), 63), rep_r = min(max((cols - 2 - gx0) >> 1, 0), 63);
    const int a_m8 = ((lane - 8) & 63) * 4, a_p8 = ((lane + 8) & 63) * 4;
    const bool b_lo = lane < 8, b_hi = lane >= 56;
    unsigned* sd = s_delay[wave];
    unsigned (*dl_c)[64] = reinterpret_cast<unsigned (*)[64]>(sd);
    unsigned (*dl_a)[64] = reinterpret_cast<unsigned (*)[64]>(sd + 16 * 64);
    unsigned (*dl_b)[32] = reinterpret_cast<unsigned (*)[32]>(sd + 16 * 128);
    const int lb = lane < 16 ? lane : (lane >= 48 ? lane - 32 : 0);

    PostPipeP<BLUR> pipe;
    pipe.init(dst + fo + (size_t)V * cols, rows, cols, gx0, lane, max_depth, thr);
    MedianColumnQ mc;
    mc.init();

    const bool warm = V > 0;
    unsigned xa0 = 0, xb0 = 0;                                       // cold start: 0 is the neutral element
    if (warm) { const Raw r = ld_row(0); xa0 = pack(r.e, r.o); xb0 = r.b; }
    // The prefetch rings, slot = step mod 16, PFD of them in flight.  They are carried round the loops as the load instructions left
    // them -- a value COMPUTED from a load result and carried over a back edge makes the compiler wait there for every load in flight
    // (one drain of the whole lookahead per 16 row steps).  The border body loads three 16-bit codes per row
    // (PFE, PFO, PFB), the interior body one dword for the (E, O) pair (PFA) and PFB; the two formats meet only where the main
    // loop changes bodies (twice per wave).
    unsigned short PFE[16], PFO[16], PFB[16];
    unsigned PFA[16], W2A[16], W6A[16], W2B[16], W6B[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { PFE[q] = PFO[q] = PFB[q] = 0; PFA[q] = 0; W2A[q] = W6A[q] = xa0; W2B[q] = W6B[q] = xb0; }
#pragma unroll
    for (int q = 0; q < 16; ++q) { dl_c[q][lane] = xa0; dl_a[q][lane] = xa0; dl_b[q][lb] = xb0; }
    constexpr int PFD = DCMT_FPQ_PFD;        // rows of load lookahead
#pragma unroll
    for (int q = 0; q < PFD; ++q) {
        const Raw r = ld_row(min(max(q + (warm ? 16 : 0) - 15, 0), rows - 1));
        PFE[q] = r.e; PFO[q] = r.o; PFB[q] = r.b;
    }
    unsigned vpa = xa0, vpb = xb0, x7_prev = xa0;
    int before = 0, after = 0;
    unsigned pend_v = xa0, pend_f1 = 0, pend_f2 = 0;
    unsigned long long pend_hme = 0, pend_hmo = 0;
    unsigned nxt_c = xa0, nxt_a = xa0, nxt_b = xb0;

    using Pipe = PostPipeP<BLUR>;
    using BorderMode = std::integral_constant<int, Pipe::BORDER>;
    // the fill front end of step t: returns X7 (packed codes) of image row t - 31.  M_: Pipe::BORDER, or Pipe::INNER -- the caller
    // vouches that row t + PFD - 15 is a row of the stream no column clamps (one aligned dword holds E and O, the row offset is
    // wave-uniform) and that X7 row t - 31 is a row of the frame
    auto fill_step = [&](auto P_, auto M_, int t) -> unsigned {
        constexpr int p = decltype(P_)::value;
        constexpr int MODE = decltype(M_)::value;
        unsigned xa;
        const unsigned xb = PFB[p];
        if constexpr (MODE == Pipe::BORDER) {
            xa = pack(PFE[p], PFO[p]);
            const Raw r = ld_row(min(max(t + PFD - 15, 0), rows - 1));
            PFE[(p + PFD) & 15] = r.e; PFO[(p + PFD) & 15] = r.o; PFB[(p + PFD) & 15] = r.b;
        } else {
            xa = PFA[p];
            const unsigned srow = (unsigned)(t + PFD - 15) * rowb;   // wave-uniform: an SGPR offset
            PFA[(p + PFD) & 15] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(sf.rs, sbe, srow, 0);
            PFB[(p + PFD) & 15] = (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(sf.rs, sbb, srow, 0);
        }
        const int o = t - 31;
        unsigned x7 = pend_v;
        if ((pend_hme | pend_hmo) != 0ull) {
            const unsigned d = qmax(pend_f1, pend_f2);
            const bool he = __builtin_amdgcn_inverse_ballot_w64(pend_hme), ho = __builtin_amdgcn_inverse_ballot_w64(pend_hmo);
            const unsigned m = (he ? 0xffffu : 0u) | (ho ? 0xffff0000u : 0u);
            x7 = (d & m) | (pend_v & ~m);
            if (MODE != Pipe::BORDER || (unsigned)o < (unsigned)rows) {
                before += __builtin_popcountll(pend_hme & own_mask) + __builtin_popcountll(pend_hmo & own_mask);
                after += __builtin_popcountll(__builtin_amdgcn_ballot_w64((x7 << 16) <= Q16::HOLE_MAX_HI) & own_mask) +
                         __builtin_popcountll(__builtin_amdgcn_ballot_w64(x7 <= Q16::HOLE_MAX_HI) & own_mask);
            }
        }
        if (edge_strip) {                                           // out-of-image columns replicate the edge column
            const unsigned l0 = (unsigned)__shfl((int)x7, rep_l, 64), r0 = (unsigned)__shfl((int)x7, rep_r, 64);
            if (gxe < 0) x7 = (l0 & 0xffffu) | (l0 << 16);
            if (gxe >= cols) x7 = (r0 >> 16) | (r0 & 0xffff0000u);
        }
        if (MODE == Pipe::BORDER && o >= rows) { asm volatile("" ::); x7 = x7_prev; }
        x7_prev = x7;
        // vertical 31-max: A packed (two-input instructions), B unpacked
        const unsigned w2a = hmax2(xa, vpa);
        vpa = xa;
        W2A[p] = w2a;
        const unsigned w6a = hmax3(w2a, W2A[(p + 14) & 15], W2A[(p + 12) & 15]);
        W6A[p] = w6a;
        const unsigned w18a = hmax3(w6a, W6A[(p + 10) & 15], W6A[(p + 4) & 15]);
        const unsigned v = nxt_c, w18a_old = nxt_a;
        nxt_c = dl_c[(p + 2) & 15][lane];
        nxt_a = dl_a[(p + 4) & 15][lane];
        dl_c[p][lane] = xa;
        dl_a[p][lane] = w18a;
        const unsigned w31a = hmax2(w18a, w18a_old);
        // (B: one code per lane in the low half, 0 above it: the packed f16 forms order these words too, and their three-input one is
        // formed reliably -- of two chained v_max_u32 the compiler fuses only one)
        const unsigned w2b = hmax2(xb, vpb);
        vpb = xb;
        W2B[p] = w2b;
        const unsigned w6b = hmax3(w2b, W2B[(p + 14) & 15], W2B[(p + 12) & 15]);
        W6B[p] = w6b;
        const unsigned w18b = hmax3(w6b, W6B[(p + 10) & 15], W6B[(p + 4) & 15]);
        const unsigned w18b_old = nxt_b;
        nxt_b = dl_b[(p + 4) & 15][lb];
        dl_b[p][lb] = w18b;
        const unsigned w31b = hmax2(w18b, w18b_old);
        const unsigned long long vme = __builtin_amdgcn_ballot_w64((v << 16) <= Q16::HOLE_MAX_HI), vmo = __builtin_amdgcn_ballot_w64(v <= Q16::HOLE_MAX_HI);
        if ((vme | vmo) != 0ull) {
            // horizontal 31-max (header comment) on the unpacked halves
            // pp, ss: the inclusive scans a lane hands on; oo, ee: the odd / even column that closes SO / PE.  A's, and in the halo
            // lanes B's -- but B's words reach the output only through lanes 0..7 and 56..63 (lanes 8..55 fetch from lanes 0..47
            // and 16..63, where SO, SX / PX, PE are formed from A alone), and a fill value is looked at only in a hole lane: a row
            // whose holes all lie in lanes 8..55 leaves B out (wave-uniform; tests/test_lane_schemes_halo_free.py)
            unsigned ee = w31a & 0xffffu, oo = w31a >> 16;
            unsigned pp, ss;
            u_row_scans_a(umax2(ee, oo), pp, ss);
            if (((vme | vmo) & 0xff000000000000ffull) != 0ull) {
                const unsigned bo = u_row_ror8(w31b);
                unsigned pb, sb;
                u_row_scans_b(umax2(w31b, bo), pb, sb);
                // which register a lane hands on is chosen at the SOURCE lane (lanes 0..6 feed the halo lanes 1..7, lane 7 feeds
                // lane 8 of A; lanes 57..63 likewise)
                if (lane < 7) pp = pb;
                if (lane > 56) ss = sb;
                if (b_hi) oo = bo;
                if (b_lo) ee = w31b;
            }
            // exclusive scans = the inclusive ones shifted by a lane, the choice above made BEFORE the shift: two shifts, not four
            const unsigned px = u_row_shr1(pp), sx = u_row_shl1(ss);
            const unsigned so = umax2(oo, sx);
            const unsigned pe = umax2(ee, px);
            // out_E(l) = max(SO(l-8), PX(l+8)), out_O(l) = max(SX(l-8), PE(l+8)): the two values a lane fetches from lane l-8 ride in one
            // word (SO low, SX high), so do the two from lane l+8 (PX low, PE high) -- two ds_bpermutes, not four, and their packed maximum
            // is the pair (out_E, out_O) as it is needed
            pend_f1 = (unsigned)__builtin_amdgcn_ds_bpermute(a_m8, (int)(so | (sx << 16)));
            pend_f2 = (unsigned)__builtin_amdgcn_ds_bpermute(a_p8, (int)(px | (pe << 16)));
        }
        pend_v = v;
        pend_hme = vme; pend_hmo = vmo;
        return x7;
    };
    // post step u: the median of image row u - 4 on packed pairs, then PostPipeP's f32 tail
    auto post_step = [&](auto PP_, auto M_, unsigned x, int u) {
        constexpr int PP = decltype(PP_)::value;
        constexpr int MODE = decltype(M_)::value;
        const unsigned rl = u_left(x), rr = u_right(x);              // columns 2l-2, 2l-1 | 2l+2, 2l+3
        unsigned s[5] = {rl, __builtin_amdgcn_alignbit(x, rl, 16), x, __builtin_amdgcn_alignbit(rr, x, 16), rr};
        q_sort5(s);
        const unsigned m = mc.template step<PP>(s);
        if constexpr (BLUR && FILLED) pipe.template after_median_codes<PP, MODE>(m, u);       // codes all the way: exact (PostPipeP)
        else pipe.template after_median<PP, MODE>(Q16::value(m & 0xffffu), Q16::value(m >> 16), u);
    };

    // steps 0..31 (16..31 after a warm start): fill only.  The last of them returns X7 row 0, which the post pipeline takes three times
    // (its replicated rows -2 and -1, and row 0: post steps 0, 1, 2)
    for (int t0 = warm ? 16 : 0; t0 < 32; t0 += 16) {
        static_for<0, 16>([&](auto P_) {
            constexpr int p = decltype(P_)::value;
            const unsigned x7 = fill_step(P_, BorderMode{}, t0 + p);
            if constexpr (p == 15) {
                if (t0 == 16) {
                    post_step(std::integral_constant<int, 0>{}, BorderMode{}, x7, 0);
                    post_step(std::integral_constant<int, 1>{}, BorderMode{}, x7, 1);
                    post_step(std::integral_constant<int, 2>{}, BorderMode{}, x7, 2);
                }
            }
        });
    }
    // steps 32..rows+34: post step u = t - 29 takes X7 row u - 2 = t - 31, the row this step's fill front end returns
    const int nsteps = rows + 35;
    int t0 = 32;
    // The V rows above the stream equal output row 0 of the shifted frame (image row V).  That row's value is kept (top_val) and the V
    // rows leave behind the wave's last row step, non-temporal like every other output row: stored where the value first exists (step
    // t = 35) they are a burst of V back-to-back stores in front of the wave's load lookahead, in every wave of the launch at once
    // (DESIGN.md section 5 has the series: the burst in place with `nt`, paced one row per step, and this).
    F2 top_val = {0.f, 0.f};
    auto main_step = [&](auto P_) {
        constexpr int p = decltype(P_)::value;
        const int t = t0 + p, u = t - 29;
        const unsigned x7 = fill_step(P_, BorderMode{}, t);
        post_step(std::integral_constant<int, ((p + 3) & 7)>{}, BorderMode{}, x7, u);
        if constexpr (p == 3) {
            // u == 6: output row 0 of the shifted frame has just been stored.  (Selects, not a branch: with the assignment under
            // `if (t0 == 32)` the allocation of <false, false> and <true, true> is 187 and 202 VGPRs, two waves per SIMD.)
            const bool first = t0 == 32;
            top_val.e = first ? pipe.last_out.e : top_val.e; top_val.o = first ? pipe.last_out.o : top_val.o;
        }
    };
    // (the sixteen steps of a block in four quarters with a way out behind each: the last block of a wave is 7.5 steps too long on
    // average otherwise -- 3 % of its row steps)
    //
    // Interior blocks.  A block of 16 steps t0 .. t0 + 15 loads the stream rows t0 + PFD - 15 .. t0 + PFD, returns the X7 rows
    // t0 - 31 .. t0 - 16 and stores the output rows t0 - 35 .. t0 - 20.  Where every one of those load rows lies inside the frame AND
    // inside [first, last] valid row of every column the wave reads, ld_row's clamps are the identity; where the output rows lie in
    // [2, rows - 3] (t0 >= 48 for the first, the load rows' bound covers the last), every row-range test of the step has one known
    // answer.  Such blocks are one contiguous run of t0; they take a body without the clamps, the tests and the selects, with one
    // dword load for (E, O).  Everything else -- the first and the last blocks, ragged tops and bottoms -- takes the border body
    // above, which also keeps the quarter exits and picks up the value of the V top rows.
    // edge_strip is a wave-uniform branch in both bodies.  As a compile-time property of the interior body (two loops chosen per
    // wave, or one loop with the choice per block) it took k_fp_q<true, true> from 148 to 216..221 VGPRs -- the register allocator
    // keeps the state of both instantiations apart -- and to 58..70 spilled VGPRs with three waves per SIMD asked for.
    const int r_first = max(__builtin_amdgcn_readfirstlane(wave_max_i(max(max(tie, tio), tib))) - V, 0);
    const int r_last = min(__builtin_amdgcn_readfirstlane(wave_min_i(min(min(bie, bio), bib))) - V, rows - 1);
    auto interior = [&](int t) -> bool { return t >= 48 && t + PFD - 15 >= r_first && t + PFD <= r_last; };
    using InnerMode = std::integral_constant<int, Pipe::INNER>;
    for (; t0 < nsteps; t0 += 16) {
        if (interior(t0)) {
            // the rows in flight change format: the only places that wait for the whole lookahead, twice per wave
#pragma unroll
            for (int q = 0; q < PFD; ++q) PFA[q] = pack(PFE[q], PFO[q]);
            do {
                static_for<0, 16>([&](auto P_) {
                    constexpr int p = decltype(P_)::value;
                    int t = t0 + p;
                    asm volatile("" : "+s"(t));      // (the row offsets from t, step by step: left to itself the compiler keeps 30 multiples of the row pitch in SGPRs and spills)
                    const unsigned x7 = fill_step(P_, InnerMode{}, t);
                    post_step(std::integral_constant<int, ((p + 3) & 7)>{}, InnerMode{}, x7, t - 29);
                });
                t0 += 16;
            } while (interior(t0));
#pragma unroll
            for (int q = 0; q < PFD; ++q) { PFE[q] = (unsigned short)PFA[q]; PFO[q] = (unsigned short)(PFA[q] >> 16); }
            // (the block behind an interior run exists and is no interior one: t0 + PFD > r_last and t0 - 16 + PFD <= rows - 1 < nsteps - 16)
        }
        static_for<0, 4>(main_step);
        if (t0 + 4 >= nsteps) break;
        static_for<4, 8>(main_step);
        if (t0 + 8 >= nsteps) break;
        static_for<8, 12>(main_step);
        if (t0 + 12 >= nsteps) break;
        static_for<12, 16>(main_step);
    }
    if (V > 0) {
        FrameBuf top;
        top.init(dst + fo, (size_t)V * cols);
        const unsigned tbo = pipe.outlane ? pipe.ob : kDropOffset;
        for (int r = 0; r < V; ++r) st2_nt(top, tbo, r, cols, top_val);
    }
    if (lane == 0) {
        if (before) atomicAdd(&cnt[0], before);
        if (after) atomicAdd(&cnt[1], after);
    }
}

}  // namespace dcmt
