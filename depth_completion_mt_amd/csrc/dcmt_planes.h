// dcmt_planes.h -- what the kernels of dcmt_kernels_planes.h (compiled in dcmt_cloud.hip) share with the host code that plans their
// launches (dcmt_plan_side.h): the constants, the moment record and the fit of one label from its moments, in the order
// include/dcmt.h fixes (dcmt_superpixel_planes_dev).  No HIP: the fit is plain C++ that compiles for the host as well, where
// tests/plan_planes_test.cpp runs it on hand-worked moments.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DCMT_PLANES_HD __host__ __device__
#else
#define DCMT_PLANES_HD
#endif

namespace dcmt {

constexpr int kPlanesTile = 64;                 // k_planes_sum: one workgroup per tile of 64 x 64 pixels
constexpr int kPlanesRun = 16;                  // ... a thread walks 16 rows of one column of the tile
constexpr int kPlanesSlots = 512;               // ... labels [lowest label of the tile's returns, + kPlanesSlots) are summed in LDS (48 KiB), the others in global memory
constexpr int kPlanesMomWords = 12;             // a moment record: 9 sums of 64 bits, then umin, umax, vmin, vmax, wmin, wmax of 32 bits (96 bytes)
constexpr int kPlanesFitBytes = 48;             // sizeof(dcmt_plane_fit)
constexpr uint32_t kPlanesMaxPixels = 1u << 21; // rows * cols at most: the bounds of the sums and of the determinant (dcmt.h)
constexpr float kPlanesW = 65536.0f;            // the code of a depth z is rne(kPlanesW / z)
constexpr uint32_t kPlanesMinThreshBits = 0x3d800000u;   // valid_thresh >= 0.0625f: codes <= 2^20
constexpr uint32_t kPlanesMaxDepthBits = 0x46800000u;    // max_depth <= 16384.0f: codes >= 4

enum { kPlanesNone = 0, kPlanesConstant = 1, kPlanesPlane = 2 };

// word j (of 32 bits) of a cleared moment record: the three minima start at 2^32 - 1, everything else at 0
DCMT_PLANES_HD inline uint32_t planes_clear_word(uint32_t j)
{
    const uint32_t k = j % (2u * kPlanesMomWords);
    return k == 18u || k == 20u || k == 22u ? 0xffffffffu : 0u;
}

struct PlaneMoments {
    uint64_t n, su, sv, suu, suv, svv, sw, suw, svw;
    uint32_t umin, umax, vmin, vmax, wmin, wmax;
};

DCMT_PLANES_HD inline PlaneMoments planes_load(const unsigned long long* m)
{
    PlaneMoments q;
    q.n = m[0]; q.su = m[1]; q.sv = m[2]; q.suu = m[3]; q.suv = m[4]; q.svv = m[5]; q.sw = m[6]; q.suw = m[7]; q.svw = m[8];
    q.umin = (uint32_t)m[9]; q.umax = (uint32_t)(m[9] >> 32);
    q.vmin = (uint32_t)m[10]; q.vmax = (uint32_t)(m[10] >> 32);
    q.wmin = (uint32_t)m[11]; q.wmax = (uint32_t)(m[11] >> 32);
    return q;
}

struct PlaneFit {                               // dcmt_plane_fit's fields
    double a, b, c;
    uint32_t seen, used, wmin, wmax, kind;
};

// every f64 operation of the fit rounded once, never contracted
#if defined(__HIP_DEVICE_COMPILE__)
DCMT_PLANES_HD inline double planes_mul(double x, double y) { return __dmul_rn(x, y); }
DCMT_PLANES_HD inline double planes_sub(double x, double y) { return __dsub_rn(x, y); }
DCMT_PLANES_HD inline double planes_add(double x, double y) { return __dadd_rn(x, y); }
DCMT_PLANES_HD inline double planes_div(double x, double y) { return __ddiv_rn(x, y); }
#else
DCMT_PLANES_HD inline double planes_mul(double x, double y) { volatile double r = x * y; return r; }
DCMT_PLANES_HD inline double planes_sub(double x, double y) { volatile double r = x - y; return r; }
DCMT_PLANES_HD inline double planes_add(double x, double y) { volatile double r = x + y; return r; }
DCMT_PLANES_HD inline double planes_div(double x, double y) { volatile double r = x / y; return r; }
#endif

// An exact 128-bit integer as the nearest f64, ties to even: below 2^64 the conversion of a 64-bit integer, which rounds once; above,
// the top 64 bits with every bit below them folded into the lowest one (a sticky bit under the rounding position), converted, and
// scaled by an exact power of two.
DCMT_PLANES_HD inline double planes_f64(__int128 x)
{
    const bool neg = x < 0;
    const unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)x : (unsigned __int128)x;
    const uint64_t hi = (uint64_t)(m >> 64);
    double r;
    if (hi == 0) {
        r = (double)(uint64_t)m;
    } else {
        const int s = 64 - __builtin_clzll(hi);                        // 1 .. 64: m has 64 + s bits
        uint64_t top = (uint64_t)(m >> s);
        if ((m & (((unsigned __int128)1 << s) - 1)) != 0) top |= 1u;
        const uint64_t pb = (uint64_t)(1023 + s) << 52;                // 2^s
        double p;
        __builtin_memcpy(&p, &pb, sizeof p);
        r = (double)top * p;
    }
    return neg ? -r : r;
}

// dcmt.h's FIT of one label from its moments.  Returns kind none / constant / plane with seen = used = n.
DCMT_PLANES_HD inline PlaneFit planes_fit(const PlaneMoments& q, uint32_t min_points, uint32_t min_extent)
{
    PlaneFit f = {};
    if (q.n == 0) return f;
    f.seen = f.used = (uint32_t)q.n;
    f.wmin = q.wmin;
    f.wmax = q.wmax;
    const double nd = (double)q.n;
    const double wbar = planes_div((double)q.sw, nd);
    f.kind = kPlanesConstant;
    f.c = wbar;
    if (q.n < min_points || q.umax - q.umin + 1u < min_extent || q.vmax - q.vmin + 1u < min_extent) return f;
    typedef __int128 I;
    const I n = (I)q.n, su = (I)q.su, sv = (I)q.sv, sw = (I)q.sw;
    const I cuu = n * (I)q.suu - su * su, cuv = n * (I)q.suv - su * sv, cvv = n * (I)q.svv - sv * sv;
    const I cuw = n * (I)q.suw - su * sw, cvw = n * (I)q.svw - sv * sw;
    const I det = cuu * cvv - cuv * cuv;
    if (det <= 0) return f;
    const double duu = planes_f64(cuu), duv = planes_f64(cuv), dvv = planes_f64(cvv), duw = planes_f64(cuw), dvw = planes_f64(cvw), d = planes_f64(det);
    f.a = planes_div(planes_sub(planes_mul(duw, dvv), planes_mul(dvw, duv)), d);
    f.b = planes_div(planes_sub(planes_mul(dvw, duu), planes_mul(duw, duv)), d);
    const double ubar = planes_div((double)q.su, nd), vbar = planes_div((double)q.sv, nd);
    f.c = planes_sub(planes_sub(wbar, planes_mul(f.a, ubar)), planes_mul(f.b, vbar));
    f.kind = kPlanesPlane;
    return f;
}

// w^(u, v) = (a u + b v) + c
DCMT_PLANES_HD inline double planes_eval(double a, double b, double c, uint32_t u, uint32_t v)
{
    return planes_add(planes_add(planes_mul(a, (double)u), planes_mul(b, (double)v)), c);
}

}  // namespace dcmt
