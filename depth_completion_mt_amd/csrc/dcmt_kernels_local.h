// dcmt_kernels_local.h -- the cascade without its extrapolation (DCMT_FLAG_NO_EXTRAPOLATE): H2..H5, then H9..H11 on X5, in one
// streaming kernel.  Without the column extension (H6), the 31x31 fill (H7) and the hole-closure loop (H8) the cascade is a local
// stencil: an output pixel depends on the input 13 rows either way (2 + 4 + 3 for H3..H5, 2 + 2 for the median and the Gaussian)
// and, sideways, on PreS::HL + 4 columns to its left and PreS::HR + 4 to its right.  So one wave64 streams down a strip of columns
// once, reads the sparse plane once and writes the dense plane once: no X6 plane, no column table, no hole counters, no redo chain.
//
//   front half   the rolling-register H2..H5 pipeline of k_pre_s (dcmt_kernels_fused.h), one column per lane, without the H6
//                bookkeeping and without a store: step i finishes X5 row i - 9 in a register;
//   back half    PostPipe<MODE, BLUR, /*FILLED=*/false> (the body of k_post_s), fed from that register two steps later.
//
// What joins them:
//  * columns: the median wants X5 with BORDER_REPLICATE.  A front-half lane outside the image holds no X5 (morphology ignores taps
//    outside the image, and such lanes load clamped addresses), so on an edge strip every lane takes the value of the lane that
//    holds column clamp(gx, 0, cols - 1) -- what PostPipe itself does with `rl` for the Gaussian's reflect-101 columns;
//  * rows: PostPipe's step u wants X5 row clamp(u - 2, 0, rows - 1).  The front half finishes row m = u at that step, so the value
//    is delayed by two steps in a register ring; the first row is fed three times (kept in x0) and the last one five times (the ring
//    holds it once the front half runs past the image);
//  * row bands: a wave may own only the output rows [so0, so1) of its strip (PostPipe::so0 / so1).  It starts streaming 13 rows
//    above so0, rounded down to a multiple of 8 so that the ring phases stay compile-time, and stops 14 steps below so1; X5 rows
//    from S + 9 on see only rings filled from real rows.  Replication and reflection happen at the image's first and last row
//    only, never at a band seam: a band's halo rows are real rows.
//
//  * leading empty rows: a wave first looks for the first row of its range that holds a non-zero value, stores zeros above
//    its reach and treats the row where values may begin as the top of its band.
//
// MODE / BLUR (a POST_BLUR_* kind) as PostPipe's, except that MODE 9 is never instantiated: PostPipe<9> stores the median of every row it sees, whatever
// the band; the median alone is PostPipe<10, false>, which stores through the band test.
#pragma once

#include "dcmt_kernels_fused.h"

namespace dcmt {

enum { LOCAL_F32 = 0, LOCAL_U16 = 1, LOCAL_NORM = 2, LOCAL_START4 = 3 };      // what k_local loads: as k_pre_s's START4 / U16 / NORM

template <int K0KIND>
struct LocalS {
    using F = PreS<K0KIND, false>;
    static constexpr int HL = F::HL + PostS::H, HR = F::HR + PostS::H;         // lanes lost to the left / right of a strip
    static constexpr int VW = 64 - HL - HR;                                    // output columns per wave
    static constexpr int REACH = 13;                                           // input rows an output row needs above and below it
    static constexpr int LAT = F::LAT + 6;                                     // rows between the input row and the finished output row
};

template <int K0KIND, int IN, int MODE, int BLUR>
__global__ __launch_bounds__(256)
void k_local(const void* __restrict__ src_, float* __restrict__ dst, int rows, int cols, int strips, int bands,
             int batch, int xcd_map, float max_depth, float thr, float in_scale, const float* __restrict__ coef)
{
    static_assert(MODE == 10 || MODE == 11, "the median alone is PostPipe<10, false>");
    constexpr bool START4 = IN == LOCAL_START4, U16 = IN == LOCAL_U16, NORM = IN == LOCAL_NORM;
    const float* src = static_cast<const float*>(src_);
    using G = LocalS<K0KIND>;
    constexpr int ROFF = START4 ? 6 : 0;         // image row of stream row s is s - ROFF
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);             // wave-uniform: keep it scalar
    int f, unit;
    if (!wave_strip(blockIdx.x, wave, strips * bands, batch, xcd_map, f, unit)) return;   // whole waves leave; no barrier is used below
    const int strip = unit / bands, band = unit - strip * bands;
    int so0 = (int)((long long)band * rows / bands);
    const int so1 = (int)((long long)(band + 1) * rows / bands);
    if (so0 >= so1) return;
    const int gx0 = strip * G::VW - G::HL;
    const int gx = gx0 + lane;
    const bool incol = gx >= 0 && gx < cols;
    const size_t fo = (size_t)f * rows * cols;
    const int gxc = min(max(gx, 0), cols - 1);       // loads are unconditional, from clamped addresses
    float na = 1.0f, nb = 0.0f;
    if constexpr (NORM) { na = coef[2 * f]; nb = coef[2 * f + 1]; }
    const uint16_t* sp16 = static_cast<const uint16_t*>(src_) + fo + gxc;
    FrameBuf ib;                                  // the input frame; this lane's column at byte offset oc
    ib.init(src + fo, (size_t)rows * cols);
    const unsigned oc = 4u * (unsigned)gxc;
    auto load_row = [&](int r) -> float {          // image row r (already clamped) of this lane's column
        if constexpr (U16) return __fmul_rn((float)sp16[(size_t)r * cols], in_scale);
        else return ib.ld(oc, r, cols);
    };
    PostPipe<MODE, BLUR, false> pipe;
    pipe.init(dst + fo, rows, cols, gx0, lane, max_depth, thr);
    pipe.outlane = incol && lane >= G::HL && lane < G::HL + G::VW;

    // ---- leading rows without a measurement (the upper third of a velodyne frame): nothing to compute there.  Where every value
    // this wave loads from the rows o - REACH .. o + REACH is zero, output row o is zero: maxima, minima and medians of zeros and of
    // the borders' -FLT_MAX / +FLT_MAX (which never win against an in-image zero) are zero, a zero is not blurred and not inverted.
    // (Zero, not "below thr": an invalid value that is not zero travels through the stages like any other.)  With zv the first
    // 16-row chunk, from the band's first input row on, that holds a non-zero value (N1 and the uint16 scale applied), the output
    // rows above zv - REACH are stored as zeros and the stream starts below them as it does below a band seam.
    {
        const int r0 = max(so0 - G::REACH, 0), r1 = min(so1 + G::REACH, rows);
        int zv = r1;
        for (int z = r0; z < r1; z += 16) {
            float v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                float x = load_row(min(z + q, rows - 1));
                if constexpr (NORM) x = norm_apply(x, na, nb);
                v[q] = x;
            }
            bool any = false;
#pragma unroll
            for (int q = 0; q < 16; ++q) any |= v[q] != 0.0f;
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) { zv = z; break; }
        }
        const int z0 = zv >= r1 ? so1 : min(max(zv - G::REACH, so0), so1);      // the band's first output row that may hold a value
        for (int r = so0; r < z0; ++r) pipe.of.st(pipe.outlane ? pipe.ob : kDropOffset, r, cols, 0.0f);
        if (z0 >= so1) return;
        so0 = z0;
    }
    pipe.so0 = so0; pipe.so1 = so1;
    const int cl = gxc - gx0;                    // the lane that holds this lane's column, replicated at the image's edges

    constexpr float NEG = -FLT_MAX, POS = FLT_MAX;
    // rolling rows, indexed by (row & 7); fully unrolled below so every index is static
    float PF[8];                                 // prefetched input rows
    float XR[8];                                 // diamond only: x2 rows
    float A3[8];                                 // diamond only: horizontal 3-max rows
    float S1[8];                                 // as-compiled only: x2 shifted by one column
    float H4[8], HE[8], H7[8], E4[8], T7[8];
    float XD[8];                                 // finished X5 rows (the last image row from there on), for the two steps of delay
#pragma unroll
    for (int q = 0; q < 8; ++q) { XR[q] = NEG; A3[q] = NEG; S1[q] = NEG; H4[q] = NEG; HE[q] = POS; H7[q] = NEG; E4[q] = NEG; T7[q] = NEG; PF[q] = 0.f; XD[q] = 0.f; }
    constexpr int PFD = 4;                       // rows of load lookahead

    // cold rings at stream row S: X5 rows from S + 9 on are right (S = 0: all of them, the rings start as the borders do)
    const int S = max(so0 - G::REACH, 0) & ~7;
#pragma unroll
    for (int q = 0; q < PFD; ++q) PF[q] = load_row(min(max(S + q - ROFF, 0), rows - 1));

    float x0 = 0.f, hold = 0.f;                  // X5 row 0; the newest X5 row inside the image
    const int nsteps = so1 + G::LAT;             // the last output row o = i - LAT = so1 - 1
    for (int i0 = S; i0 < nsteps; i0 += 8) {
        static_for<0, 8>([&](auto P_) {
            constexpr int p = decltype(P_)::value;
            const int i = i0 + p;
            // ---- H2 on load (LO :55-67); outside the image: the dilate border value
            float raw = PF[p];
            PF[(p + PFD) & 7] = load_row(min(max(i + PFD - ROFF, 0), rows - 1));
            float e4;
            const int l = i - 6;
            if constexpr (START4) {
                e4 = raw;                                               // X4 row l
            } else {
                if constexpr (NORM) raw = norm_apply(raw, na, nb);
                const float x2 = (incol && i < rows) ? invert_valid(raw, max_depth, thr) : NEG;
                // ---- H3 (LO :71-80), row j = i - 2
                const int j = i - 2;
                float y3;
                if constexpr (K0KIND == K0_AS_COMPILED) {
                    // dst(r,c) = max(src(r-1,c+1), src(r+2,c+2))
                    const float s1 = from_right(x2);
                    const float s2 = from_right(s1);
                    S1[p] = s1;
                    y3 = fmax2(S1[(p + 5) & 7] /* row i-3 = j-1 */, s2 /* row i = j+2 */);
                } else {
                    // 13-tap diamond: rows j-2 and j+2 centre only, j-1 and j+1 three wide, j five wide
                    const float a3 = hmax3(x2);
                    XR[p] = x2;
                    A3[p] = a3;
                    const float a3j = A3[(p + 6) & 7];                       // row j
                    const float a5j = hgrow_max(a3j);
                    y3 = fmax2(fmax3(XR[(p + 4) & 7] /* j-2 */, A3[(p + 5) & 7] /* j-1 */, a5j),
                               fmax2(A3[(p + 7) & 7] /* j+1 */, x2 /* j+2 */));
                }
                y3 = (incol && (unsigned)j < (unsigned)rows) ? y3 : NEG;
                // ---- H4 dilate 5x5 (LO :85): horizontal on row j, vertical gives row k = j - 2
                H4[(p + 6) & 7] = hgrow_max(hmax3(y3));                      // slot of row j = i-2
                const int k = i - 4;
                float d4 = fmax3(fmax3(H4[(p + 2) & 7], H4[(p + 3) & 7], H4[(p + 4) & 7]), H4[(p + 5) & 7], H4[(p + 6) & 7]);
                d4 = (incol && (unsigned)k < (unsigned)rows) ? d4 : POS;     // border value of the erode
                // ---- H4 erode 5x5: row l = k - 2
                HE[(p + 4) & 7] = hgrow_min(hmin3(d4));                      // slot of row k = i-4
                e4 = fmin3(fmin3(HE[(p + 0) & 7], HE[(p + 1) & 7], HE[(p + 2) & 7]), HE[(p + 3) & 7], HE[(p + 4) & 7]);
            }
            e4 = (incol && (unsigned)l < (unsigned)rows) ? e4 : NEG;     // border value of the 7x7 dilate
            E4[(p + 2) & 7] = e4;                                        // slot of row l = i-6
            // ---- H5 (LO :88-100): dilate 7x7, row m = l - 3, then fill where x < 0.1
            H7[(p + 2) & 7] = hgrow_max(hgrow_max(hmax3(e4)));
            const int m = i - 9;
            T7[p] = fmax3(H7[(p + 0) & 7], H7[(p + 1) & 7], H7[(p + 2) & 7]);      // rows i-8 .. i-6
            const float d7 = fmax3(T7[p], T7[(p + 5) & 7] /* rows i-11 .. i-9 */, H7[(p + 4) & 7] /* row i-12 */);
            const float e = E4[(p + 7) & 7];                             // row m = i-9
            float x5 = e < thr ? d7 : e;
            // ---- X5 with replicated columns ...
            if (pipe.edge_strip) x5 = __shfl(x5, cl, 64);
            // ---- ... and replicated rows: step u = m of the back half takes X5 row clamp(m - 2, 0, rows - 1)
            x0 = m == 0 ? x5 : x0;
            hold = m < rows ? x5 : hold;
            XD[p] = hold;
            const float feed = m < 2 ? x0 : XD[(p + 6) & 7];
            pipe.template step<(p + 7) & 7>(feed, m);
        });
    }
}

}  // namespace dcmt
