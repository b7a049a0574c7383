// The launches of the nearest-wins calls as values (csrc/dcmt_plan_side.h: plan_project_nearest, plan_reproject_nearest), walked on a
// CPU: the clear's byte count, the scatter grids, the fix-up's vector width and grid -- every pixel covered, no access beyond the
// plane -- and the checks on the buffers (null, misaligned, every overlapping input / output pair).  Built and run by
// tests/test_nearest.py; prints every failed check and returns their number.
#include <cstdio>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// what every good plan must satisfy for an output plane of n_px pixels at address out
static void check_plane(const NearestPlan& p, size_t n_px, uintptr_t out)
{
    CHECK(p.status == kOk);
    CHECK(p.n_px == n_px && p.clear_bytes == 4 * n_px);
    CHECK(p.vec == 1 || p.vec == 2 || p.vec == 4);
    CHECK(n_px % (size_t)p.vec == 0 && out % (4 * (size_t)p.vec) == 0);                    // whole, aligned accesses
    CHECK(p.vec == resolve_vec(n_px, out));
    const size_t threads = (size_t)p.fixup_x * 256, need = n_px / (size_t)p.vec;
    CHECK(threads >= need && threads < need + 256);                                        // every pixel, less than one workgroup to spare
}

int main()
{
    const uintptr_t A = 0x7f0000100000ull;               // a pretend device address space: 16-byte aligned bases, well apart
    const uintptr_t pts = A, off = A + 0x100000, tab = A + 0x200000, out = A + 0x300000, depth = A + 0x400000;

    // ---- projection: the shapes of the GPU tests and a real batch
    struct { int rows, cols, batch, n; uintptr_t out; int vec; } pc[] = {
        {5, 7, 3, 1500, out, 1},                         // 105 pixels: odd, the scalar fix-up
        {6, 7, 3, 1500, out, 2},                         // 126: pairs
        {8, 16, 3, 1500, out, 4},                        // 384: quads
        {8, 16, 3, 1500, out + 4, 1},                    // the same plane 4 bytes on: the alignment fallback
        {8, 16, 3, 1500, out + 8, 2},
        {352, 1216, 256, 256 * 120000, A + 0x800000000ull, 4},    // (0.49 GB of records in front of it)
        {1, 1, 1, 1, out, 1},
        {8, 16, 3, 0, out, 4},                           // no points: clear and fix-up only
    };
    for (const auto& c : pc)
        for (int table = 0; table < 2; ++table) {
            const NearestPlan p = plan_project_nearest(c.rows, c.cols, c.batch, c.n, c.n ? pts : 0, off, table != 0, table ? tab : 0, c.out);
            check_plane(p, (size_t)c.batch * c.rows * c.cols, c.out);
            CHECK(p.vec == c.vec);
            CHECK((size_t)p.scatter_x * 256 >= (size_t)c.n && (size_t)p.scatter_x * 256 < (size_t)c.n + 256 && p.scatter_y == 1);
            CHECK((p.scatter_x == 0) == (c.n == 0));
        }
    {   // refused: null, misaligned, too many points
        CHECK(plan_project_nearest(8, 16, 3, 1500, 0, off, false, 0, out).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, 0, false, 0, out).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, 0).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, -1, pts, off, false, 0, out).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1 << 30, pts, off, false, 0, out).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, (1 << 30) - 1, pts, off, false, 0, A + 0x800000000ull).status == kOk);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts + 4, off, false, 0, out).status == kInvalid);        // d_points: 16-byte records
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts + 8, off, false, 0, out).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off + 2, false, 0, out).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, out + 2).status == kInvalid);        // atomics on the plane
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, true, 0, out).status == kInvalid);             // a table call without a table
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, true, tab + 8, out).status == kInvalid);       // the table: 16 bytes
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, out).status == kOk);
    }
    {   // every overlapping input / output pair; the output is 3 * 8 * 16 * 4 = 1536 bytes
        const size_t ob = 1536, pb = 16 * 1500, fb = 4 * 4, tb = 96 * 3;
        // d_points: the output right behind it, its last byte on the first record, inside, its first byte on the last record, right in front
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, pts + pb).status == kOk);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, pts + pb - 4).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, pts + 1600).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, pts).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts + ob, off, false, 0, pts).status == kOk);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts + ob - 16, off, false, 0, pts).status == kInvalid);
        // d_offsets: batch + 1 ints
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, off + fb).status == kOk);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, off + fb - 4).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, 0, off).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off + ob, false, 0, off).status == kOk);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off + ob - 4, false, 0, off).status == kInvalid);
        // the table: batch records of 96 bytes; only a table call looks at it
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, true, tab, tab + tb).status == kOk);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, true, tab, tab + tb - 4).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, true, tab, tab).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, true, tab + ob, tab).status == kOk);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, true, tab + ob - 16, tab).status == kInvalid);
        CHECK(plan_project_nearest(8, 16, 3, 1500, pts, off, false, tab, tab).status == kOk);
    }

    // ---- reprojection
    struct { int rows, cols, orows, ocols, batch; uintptr_t out; int vec; } rc[] = {
        {9, 13, 5, 7, 3, out, 1},
        {16, 24, 8, 16, 3, out, 4},
        {16, 24, 8, 16, 3, out + 4, 1},
        {16, 24, 6, 7, 3, out, 2},
        {352, 1216, 352, 1216, 1024, out, 4},
        {1, 1, 1, 1, 1, out, 1},
        {1, 1025, 3, 3, 2, out, 2},
    };
    for (const auto& c : rc)
        for (int table = 0; table < 2; ++table) {
            const NearestPlan p = plan_reproject_nearest(c.rows, c.cols, c.orows, c.ocols, c.batch, A + 0x1000000000ull, table != 0, table ? tab : 0, c.out);
            check_plane(p, (size_t)c.batch * c.orows * c.ocols, c.out);
            CHECK(p.vec == c.vec);
            const size_t n = (size_t)c.rows * c.cols;
            CHECK((size_t)p.scatter_x * kReprojectPxPerWg >= n && (size_t)p.scatter_x * kReprojectPxPerWg < n + kReprojectPxPerWg);
            CHECK(p.scatter_y == (unsigned)c.batch);
        }
    {
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, 0, false, 0, out).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, false, 0, 0).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth + 2, false, 0, out).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, false, 0, out + 1).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, 0, out).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, tab + 4, out).status == kInvalid);     // the table: 8 bytes
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, tab + 8, out).status == kOk);
        const size_t ob = 1536, db = 4 * 16 * 24 * 3, tb = 136 * 3;
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, false, 0, depth + db).status == kOk);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, false, 0, depth + db - 4).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, false, 0, depth + 400).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, false, 0, depth).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth + ob, false, 0, depth).status == kOk);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth + ob - 4, false, 0, depth).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, tab, tab + tb).status == kOk);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, tab, tab + tb - 4).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, tab, tab).status == kInvalid);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, tab + ob, tab).status == kOk);
        CHECK(plan_reproject_nearest(16, 24, 8, 16, 3, depth, true, tab + ob - 8, tab).status == kInvalid);
    }
    if (failures == 0) std::printf("ok\n");
    return failures;
}
