// The key of the nearest-wins calls (csrc/dcmt_depth_key.h) on a CPU: over a fixed list of finite f32 values in ascending total order
// (-0 below +0) the key is strictly DEcreasing (ord strictly increasing), never 0, and the inverse gives the bits back.  Built and
// run by tests/test_nearest.py (also with -fsanitize=address,undefined: a plain executable); prints every failed check and returns
// their number.
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dcmt_depth_key.h"

using namespace dcmt;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, sizeof b); return b; }
static float from_bits(uint32_t b) { float v; std::memcpy(&v, &b, sizeof v); return v; }
static uint32_t neg(uint32_t b) { return b | 0x80000000u; }

int main()
{
    // the positive half, ascending, as bit patterns: +0, the denormals' ends, FLT_MIN, neighbours by one ulp, KITTI-like depths, FLT_MAX
    const std::vector<uint32_t> pos = {
        0x00000000u,                                     // +0
        0x00000001u, 0x00000002u,                        // the smallest denormal and its neighbour
        0x007ffffeu, 0x007fffffu,                        // the largest denormal and its neighbour
        bits(FLT_MIN), bits(FLT_MIN) + 1,
        bits(0.5f), bits(1.0f) - 1, bits(1.0f), bits(1.0f) + 1,
        bits(1.9140625f), bits(5.37f), bits(5.37f) + 1, bits(27.25f), bits(79.99609375f), bits(80.0f), bits(85.0f), bits(255.99609375f),
        bits(65535.0f), bits(1e30f),
        bits(FLT_MAX) - 1, bits(FLT_MAX),
    };
    CHECK(bits(FLT_MIN) == 0x00800000u && bits(FLT_MAX) == 0x7f7fffffu && bits(1.0f) == 0x3f800000u);
    std::vector<uint32_t> all;                           // ascending in the total order: -FLT_MAX ... -0, +0 ... FLT_MAX
    for (size_t i = pos.size(); i-- > 0;) all.push_back(neg(pos[i]));
    for (uint32_t b : pos) all.push_back(b);
    for (size_t i = 0; i < all.size(); ++i) {
        const uint32_t b = all[i], k = depth_key(b);
        CHECK(k != 0u);
        CHECK(k >= 0x00800000u && k <= 0xff7fffffu);
        CHECK(depth_unkey(k) == b);
        CHECK(depth_key_to_bits(k) == b);
        CHECK(depth_key(b) == ~depth_ord(b));
        if (i > 0) {
            CHECK(depth_ord(all[i - 1]) < depth_ord(b));                 // strictly monotone, -0 below +0 included
            CHECK(depth_key(all[i - 1]) > k);
            if (!(all[i - 1] == 0x80000000u && b == 0u)) CHECK(from_bits(all[i - 1]) < from_bits(b));    // the list IS ascending as floats
        }
    }
    CHECK(depth_key_to_bits(0u) == 0u);                                  // nothing landed -> +0.0f
    CHECK(depth_key(bits(FLT_MAX)) == 0x00800000u && depth_key(neg(bits(FLT_MAX))) == 0xff7fffffu);
    CHECK(depth_ord(0x80000000u) == 0x7fffffffu && depth_ord(0u) == 0x80000000u);
    // an integer max of keys is the smallest value: every pair
    for (uint32_t a : all)
        for (uint32_t b : all) {
            const uint32_t ka = depth_key(a), kb = depth_key(b), m = ka > kb ? ka : kb;
            const uint32_t smaller = depth_ord(a) < depth_ord(b) ? a : b;
            CHECK(depth_unkey(m) == smaller);
        }
    if (failures == 0) std::printf("ok\n");
    return failures;
}
