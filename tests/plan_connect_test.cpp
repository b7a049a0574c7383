// plan_connectivity and its bound (csrc/dcmt_plan_side.h) on a CPU.  Built and run by tests/test_connectivity.py; prints every failed
// check and returns their number.
#include <cstdio>
#include <vector>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kLab = 0x100000000ull, kOut = 0x200000000ull, kCnt = 0x300000000ull;

// the plan of a good call, with its grids walked as the kernels walk them
static ConnPlan checked(int rows, int cols, int batch, int nc)
{
    const ConnPlan p = plan_connectivity(rows, cols, batch, nc, kLab, kOut, kCnt);
    CHECK(p.status == kOk);
    CHECK(p.g.n == (uint32_t)rows * (uint32_t)cols);
    // keys: ordered as s = x * rows + y, below 2^30, and taken apart again
    CHECK((1u << p.g.kbits) >= (uint32_t)rows && (p.g.kbits == 0 || (1u << (p.g.kbits - 1)) < (uint32_t)rows));
    CHECK(((uint64_t)(cols - 1) << p.g.kbits | (uint64_t)(rows - 1)) < (1ull << 30));
    CHECK(p.lim4 == (uint32_t)(((rows * cols) / nc) >> 2) && p.lim4 >= 1);
    CHECK(p.max_labels == connectivity_max_labels(rows, cols, nc) && p.max_labels >= 1);
    CHECK((uint64_t)p.max_labels * (p.lim4 + 1) <= p.g.n || p.max_labels == 1);
    // k_conn_local: every pixel in exactly one tile
    CHECK(p.g.tiles_x == (uint32_t)(cols + kConnTW - 1) / kConnTW && p.g.tiles_y == (uint32_t)(rows + kConnTH - 1) / kConnTH);
    CHECK(p.g.local_x == p.g.tiles_x * p.g.tiles_y);
    // k_conn_border: the pairs as the kernel takes them apart -- every pair inside the frame, across a tile edge, none twice
    CHECK(p.g.pairs_v == (p.g.tiles_x - 1) * (uint32_t)rows && p.g.pairs == p.g.pairs_v + (p.g.tiles_y - 1) * (uint32_t)cols);
    CHECK(p.g.border_x == (p.g.pairs + 255) / 256 && (p.g.border_x == 0) == (p.g.tiles_x == 1 && p.g.tiles_y == 1));
    if (p.g.n <= 1u << 16) {
        std::vector<unsigned char> right((size_t)p.g.n, 0), below((size_t)p.g.n, 0);
        for (uint32_t j = 0; j < p.g.pairs; ++j) {
            if (j < p.g.pairs_v) {
                const uint32_t e = j / rows, y = j - e * rows, xb = (e + 1) * kConnTW;
                CHECK(xb < (uint32_t)cols && y < (uint32_t)rows);
                ++right[(size_t)y * cols + xb - 1];
            } else {
                const uint32_t jj = j - p.g.pairs_v, e = jj / cols, x = jj - e * cols, yb = (e + 1) * kConnTH;
                CHECK(yb < (uint32_t)rows && x < (uint32_t)cols);
                ++below[(size_t)(yb - 1) * cols + x];
            }
        }
        size_t wrong = 0;
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) {
                wrong += right[(size_t)y * cols + x] != ((x + 1) % kConnTW == 0 && x + 1 < cols ? 1 : 0);
                wrong += below[(size_t)y * cols + x] != ((y + 1) % kConnTH == 0 && y + 1 < rows ? 1 : 0);
            }
        CHECK(wrong == 0);
    }
    CHECK(p.g.px_x == (p.g.n + 255) / 256);
    // k_conn_seed / k_conn_rank: the strips cover the columns, the four bands the rows
    CHECK(p.strips == (uint32_t)(cols + kConnStripCols - 1) / kConnStripCols);
    CHECK(p.band_rows * kConnWaves >= (uint32_t)rows && (p.band_rows - 1) * kConnWaves < (uint32_t)rows);
    CHECK(p.slab == (size_t)batch * p.strips && p.slab <= connectivity_slab_words(cols, batch));
    return p;
}

static void test_plans()
{
    const int shapes[][2] = {{1, 4}, {4, 1}, {2, 2}, {1, 70}, {70, 1}, {15, 63}, {16, 64}, {17, 65}, {67, 133}, {150, 260}, {352, 1216}, {375, 1242}};
    for (const auto& s : shapes)
        for (int batch : {1, 5, 256}) {
            const int n = s[0] * s[1];
            for (int nc : {1, 2, n / 64 > 0 ? n / 64 : 1, n / 4})
                if (n / nc >= 4) checked(s[0], s[1], batch, nc);
        }
    const ConnPlan k = checked(352, 1216, 256, 1273);
    CHECK(k.g.kbits == 9 && k.lim4 == 84 && k.max_labels == 5035 && k.g.tiles_x == 19 && k.g.tiles_y == 22 && k.strips == 19 && k.band_rows == 88);
    CHECK(checked(16, 64, 1, 4).g.border_x == 0 && checked(17, 64, 1, 4).g.border_x == 1 && checked(16, 65, 1, 4).g.pairs == 16);
    CHECK(checked(1, 4, 1, 1).max_labels == 2 && checked(2, 2, 1, 1).g.kbits == 1 && checked(1, 70, 1, 1).g.kbits == 0);
    // the largest frames dcmt_create admits
    CHECK(checked(1, 0x1ffffff0, 1, 7).status == kOk && checked(0x1ffffff0, 1, 1, 7).g.kbits == 29);
    CHECK(checked(16384, 32767, 1, 1200).status == kOk);
}

static void test_bound()
{
    CHECK(connectivity_max_labels(352, 1216, 1273) == 5035);
    CHECK(connectivity_max_labels(4, 4, 4) == 8 && connectivity_max_labels(4, 4, 5) == kInvalid);        // lims = 4, 3
    CHECK(connectivity_max_labels(4, 4, 1) == 3 && connectivity_max_labels(1, 4, 1) == 2 && connectivity_max_labels(1, 3, 1) == kInvalid);
    CHECK(connectivity_max_labels(0, 4, 1) == kInvalid && connectivity_max_labels(4, 0, 1) == kInvalid && connectivity_max_labels(4, 4, 0) == kInvalid);
    CHECK(connectivity_max_labels(4, 4, -1) == kInvalid && connectivity_max_labels(-4, -4, 1) == kInvalid);
    CHECK(connectivity_max_labels(65536, 65536, 1) == kInvalid && connectivity_max_labels(1, 0x1ffffff1, 1) == kInvalid);
    CHECK(connectivity_max_labels(1, 0x1ffffff0, 1) == 3);
}

static void test_refusals()
{
    const size_t bytes = sizeof(int32_t) * 3 * 8 * 16;
    auto st = [](uintptr_t l, uintptr_t o, uintptr_t c, int nc = 4) { return plan_connectivity(8, 16, 3, nc, l, o, c).status; };
    CHECK(st(kLab, kOut, kCnt) == kOk && st(kLab, kOut, 0) == kOk);
    CHECK(st(kLab, kLab, kCnt) == kOk);                                        // in place
    CHECK(st(kLab, kLab + 4, kCnt) == kInvalid && st(kLab + 64, kLab, kCnt) == kInvalid);
    CHECK(st(kLab, kLab + bytes - 4, kCnt) == kInvalid && st(kLab, kLab + bytes, kCnt) == kOk);
    CHECK(st(kLab, kOut, kLab) == kInvalid && st(kLab, kOut, kLab + bytes - 4) == kInvalid && st(kLab, kOut, kLab + bytes) == kOk);
    CHECK(st(kLab, kOut, kOut + 8) == kInvalid && st(kLab, kOut, kOut - 8) == kInvalid && st(kLab, kOut, kOut - 12) == kOk);
    CHECK(st(kLab, kLab, kLab + 4) == kInvalid);
    CHECK(st(0, kOut, kCnt) == kInvalid && st(kLab, 0, kCnt) == kInvalid);
    CHECK(st(kLab + 2, kOut, kCnt) == kInvalid && st(kLab, kOut + 1, kCnt) == kInvalid && st(kLab, kOut, kCnt + 2) == kInvalid);
    CHECK(st(kLab, kOut, kCnt, 0) == kInvalid && st(kLab, kOut, kCnt, -1) == kInvalid);
    CHECK(st(kLab, kOut, kCnt, 32) == kOk && st(kLab, kOut, kCnt, 33) == kInvalid);      // lims = 128 / 32 = 4, 128 / 33 = 3
}

int main()
{
    test_plans();
    test_bound();
    test_refusals();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
