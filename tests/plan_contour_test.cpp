// plan_contours and plan_cluster_means (csrc/dcmt_plan_side.h) on a CPU.  Built and run by tests/test_contours.py; prints every failed
// check and returns their number.
#include <cstdio>
#include <vector>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static const uintptr_t kLab = 0x100000000ull, kBgr = 0x200000000ull, kMask = 0x300000000ull, kSums = 0x400000000ull, kCol = 0x500000000ull;

// the plan of a good contour call, with its grids walked as the kernels walk them
static ContourPlan contours(int rows, int cols, int batch)
{
    const ContourPlan p = plan_contours(rows, cols, batch, kLab, kBgr, kMask, kCol);
    CHECK(p.status == kOk);
    CHECK(p.chunks * 64 >= (uint32_t)rows && (p.chunks - 1) * 64 < (uint32_t)rows && p.chunks <= (uint32_t)kContMaxChunks);
    CHECK(p.tiles_x * 64 >= (uint32_t)cols && (p.tiles_x - 1) * 64 < (uint32_t)cols);
    CHECK(p.tile_grid == p.tiles_x * p.chunks);
    CHECK(p.steps == (uint32_t)cols * p.chunks && (uint64_t)cols * p.chunks < (1ull << 31));
    CHECK(p.walk_lds == 8 * (size_t)p.chunks && p.walk_lds <= 32768);
    CHECK(p.scratch == (size_t)batch * rows * cols);         // 1 B/px in each plane, of the 4 B/px a plane holds
    if ((uint64_t)rows * cols <= 1u << 16) {
        // k_cont_classify / k_cont_paint: every pixel in exactly one (tile, wave, lane, i); k_cont_walk: in exactly one (step, lane)
        std::vector<unsigned char> tile((size_t)rows * cols, 0), step((size_t)rows * cols, 0);
        for (unsigned b = 0; b < p.tile_grid; ++b) {
            const uint32_t k = b / p.tiles_x, tx = b - k * p.tiles_x;
            for (uint32_t t = 0; t < 256; ++t)
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint32_t x = tx * 64 + 4 * i + (t >> 6), y = k * 64 + (t & 63);
                    if (x < (uint32_t)cols && y < (uint32_t)rows) ++tile[(size_t)x * rows + y];
                }
        }
        uint32_t x = 0, k = 0;
        for (uint32_t s = 0; s < p.steps; ++s) {
            for (uint32_t l = 0; l < 64; ++l)
                if (64 * k + l < (uint32_t)rows) ++step[(size_t)x * rows + 64 * k + l];
            if (++k == p.chunks) { k = 0; ++x; }
        }
        CHECK(x == (uint32_t)cols && k == 0);
        size_t wrong = 0;
        for (size_t i = 0; i < tile.size(); ++i) wrong += (tile[i] != 1) + (step[i] != 1);
        CHECK(wrong == 0);
    }
    return p;
}

static void test_contour_plans()
{
    const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {65, 9}, {130, 3}, {67, 133}, {64, 64}, {63, 65}, {150, 260}, {352, 1216}, {375, 1242}};
    for (const auto& s : shapes)
        for (int batch : {1, 5, 256}) contours(s[0], s[1], batch);
    const ContourPlan k = contours(352, 1216, 256);
    CHECK(k.chunks == 6 && k.tiles_x == 19 && k.tile_grid == 114 && k.steps == 7296 && k.walk_lds == 48);
    CHECK(contours(64, 64, 1).tile_grid == 1 && contours(65, 64, 1).chunks == 2 && contours(64, 65, 1).tiles_x == 2);
    // the tallest and the widest frames
    CHECK(contours(64 * kContMaxChunks, 2048, 1).walk_lds == 32768);
    CHECK(plan_contours(64 * kContMaxChunks + 1, 1, 1, kLab, kBgr, kMask, kCol).status == kInvalid);
    CHECK(contours(1, 0x1ffffff0, 1).steps == 0x1ffffff0u && contours(16384, 32767, 1).status == kOk);
}

static void test_contour_refusals()
{
    const size_t px = 3 * 8 * 16;
    auto st = [](uintptr_t l, uintptr_t b, uintptr_t m, uintptr_t c = kCol) { return plan_contours(8, 16, 3, l, b, m, c).status; };
    CHECK(st(kLab, kBgr, kMask) == kOk && st(kLab, 0, kMask) == kOk && st(kLab, kBgr, 0) == kOk);
    CHECK(st(kLab, 0, 0) == kInvalid && st(0, kBgr, kMask) == kInvalid && st(kLab, kBgr, kMask, 0) == kInvalid);
    CHECK(st(kLab + 2, kBgr, kMask) == kInvalid && st(kLab, kBgr + 1, kMask + 1) == kOk);
    CHECK(st(kLab, kLab, kMask) == kInvalid && st(kLab, kBgr, kLab) == kInvalid && st(kLab, kBgr, kBgr) == kInvalid);
    CHECK(st(kLab, kLab + 4 * px - 1, 0) == kInvalid && st(kLab, kLab + 4 * px, 0) == kOk);
    CHECK(st(kLab, kLab - 3 * px + 1, 0) == kInvalid && st(kLab, kLab - 3 * px, 0) == kOk);
    CHECK(st(kLab, 0, kLab + 4 * px - 1) == kInvalid && st(kLab, 0, kLab + 4 * px) == kOk && st(kLab, 0, kLab - px) == kOk && st(kLab, 0, kLab - px + 1) == kInvalid);
    CHECK(st(kLab, kBgr, kBgr + 3 * px - 1) == kInvalid && st(kLab, kBgr, kBgr + 3 * px) == kOk && st(kLab, kBgr, kBgr - px) == kOk && st(kLab, kBgr, kBgr - 1) == kInvalid);
}

static void test_means()
{
    const size_t plane = 4ull * 150 * 260 * 32;              // a context of 150 x 260 x 32
    CHECK(cluster_means_max_labels(plane, 32) == 150 * 260 / 4 && cluster_means_max_labels(plane, 1) == 150 * 260 * 8);
    CHECK(cluster_means_max_labels(64, 1) == 4 && cluster_means_max_labels(15, 1) == 0 && cluster_means_max_labels(~(size_t)0, 1) == 0x0fffffff);
    const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {65, 9}, {130, 3}, {67, 133}, {150, 260}};
    for (const auto& s : shapes)
        for (int batch : {1, 5, 32})
            for (int nl : {1, 7, 5000}) {
                const MeansPlan p = plan_cluster_means(s[0], s[1], batch, nl, plane, kLab, kBgr, kSums);
                CHECK(p.status == kOk && p.n == (uint32_t)(s[0] * s[1]));
                CHECK(p.tiles_x * 64 >= (uint32_t)s[1] && (p.tiles_x - 1) * 64 < (uint32_t)s[1]);
                CHECK(p.tiles_y * 64 >= (uint32_t)s[0] && (p.tiles_y - 1) * 64 < (uint32_t)s[0]);
                CHECK(p.sum_grid == p.tiles_x * p.tiles_y && p.px_x == (p.n + 255) / 256);
                CHECK(p.words == (size_t)batch * nl * 4 && 4 * p.words <= plane);
                CHECK(p.clear_grid >= 1 && p.clear_grid <= 4096 && (p.clear_grid == 4096 || (size_t)p.clear_grid * 256 >= p.words));
            }
    auto st = [&](int nl, uintptr_t l = kLab, uintptr_t b = kBgr, uintptr_t s = kSums, int batch = 3) {
        return plan_cluster_means(8, 16, batch, nl, plane, l, b, s).status;
    };
    const size_t px = 3 * 8 * 16;
    CHECK(st(4) == kOk && st(4, kLab, kBgr, 0) == kOk);
    CHECK(st(0) == kInvalid && st(-1) == kInvalid);
    CHECK(st(cluster_means_max_labels(plane, 3)) == kOk && st(cluster_means_max_labels(plane, 3) + 1) == kInvalid);
    CHECK(st(cluster_means_max_labels(plane, 3) + 1, kLab, kBgr, 0) == kInvalid);      // with or without d_sums
    CHECK(st(4, 0) == kInvalid && st(4, kLab, 0) == kInvalid && st(4, kLab + 2) == kInvalid && st(4, kLab, kBgr, kSums + 2) == kInvalid);
    CHECK(st(4, kLab, kLab) == kInvalid && st(4, kLab, kLab + 4 * px - 1) == kInvalid && st(4, kLab, kLab + 4 * px) == kOk);
    CHECK(st(4, kLab, kBgr, kLab) == kInvalid && st(4, kLab, kBgr, kLab + 4 * px - 4) == kInvalid && st(4, kLab, kBgr, kLab + 4 * px) == kOk);
    CHECK(st(4, kLab, kBgr, kBgr + 4) == kInvalid && st(4, kLab, kBgr, kBgr - 3 * 4 * 16 + 4) == kInvalid && st(4, kLab, kBgr, kBgr - 3 * 4 * 16) == kOk);
    // 32-bit sums: 255 * rows * cols below 2^32
    const size_t big = ~(size_t)0 >> 8;
    CHECK(plan_cluster_means(4096, 4112, 1, 1, big, kLab, kBgr, 0).status == kOk);           // 16842752 pixels
    CHECK(plan_cluster_means(1, 16843009, 1, 1, big, kLab, kBgr, 0).status == kOk);          // 255 * it = 2^32 - 1
    CHECK(plan_cluster_means(1, 16843010, 1, 1, big, kLab, kBgr, 0).status == kInvalid);
    CHECK(plan_cluster_means(16384, 32767, 1, 1, big, kLab, kBgr, 0).status == kInvalid);
}

int main()
{
    test_contour_plans();
    test_contour_refusals();
    test_means();
    if (failures == 0) std::printf("ok\n");
    return failures;
}
