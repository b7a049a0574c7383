// plan_rectify / plan_rectify_map (dcmt_plan_side.h) and the box arithmetic of dcmt_rectify.h on a CPU: what dcmt_rectify_dev and
// dcmt_rectify_map_dev refuse, and the grid they launch.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt;
using namespace dcmt::plan;

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

int main()
{
    const uintptr_t src = 0x100000, map = 0x200000, idx = 0x300000, dst = 0x400000, table = 0x500000;
    const auto ok = [&](const RectifyPlan& p) { return p.status == kOk; };
    // the refusals of dcmt_rectify_dev
    CHECK(ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, dst)));
    CHECK(ok(plan_rectify(41, 150, 3, 37, 131, 5, 2, 1, src, map, 0, dst)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, 0, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, 0, idx, dst)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, 0)));
    CHECK(!ok(plan_rectify(41, 150, 2, 37, 131, 5, 2, 0, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 150, 4, 37, 131, 5, 2, 0, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 0, 0, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, -1, 0, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 2, src, map, idx, dst)));            // an unknown flag bit
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0x80000000u, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(0, 150, 1, 37, 131, 5, 2, 0, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 0, 1, 37, 131, 5, 2, 0, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(16385, 150, 1, 37, 131, 5, 2, 0, src, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 16385, 1, 37, 131, 5, 2, 0, src, map, idx, dst)));
    CHECK(ok(plan_rectify(16384, 16384, 3, 37, 131, 1, 1, 0, src + 0x40000000u, map, idx, dst)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map + 4, idx, dst)));        // a misaligned map, a misaligned index
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx + 2, dst)));
    CHECK(ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src + 3, map, idx, dst + 1)));     // source and destination: any byte
    // no in-place form: the destination against the source, the map and the index
    const size_t sb = 5 * 41 * 150, db = 5 * 37 * 131, mb = 2 * 37 * 131 * 8;
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, src)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, src + sb - 1)));
    CHECK(ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, src + sb)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, src - db + 1)));
    CHECK(ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, src - db)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, map + mb - 1)));
    CHECK(ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, map + mb)));
    CHECK(!ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, idx + 19)));
    CHECK(ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, idx, idx + 20)));
    CHECK(ok(plan_rectify(41, 150, 1, 37, 131, 5, 2, 0, src, map, 0, idx + 19)));          // no index: nothing to overlap
    // ... and of dcmt_rectify_map_dev
    const auto mok = [&](const RectifyMapPlan& p) { return p.status == kOk; };
    CHECK(mok(plan_rectify_map(37, 131, 3, table, map)));
    CHECK(!mok(plan_rectify_map(37, 131, 3, 0, map)) && !mok(plan_rectify_map(37, 131, 3, table, 0)));
    CHECK(!mok(plan_rectify_map(37, 131, 0, table, map)) && !mok(plan_rectify_map(37, 131, 65536, table, map)));
    CHECK(!mok(plan_rectify_map(37, 131, 3, table + 4, map)) && !mok(plan_rectify_map(37, 131, 3, table, map + 4)));
    CHECK(!mok(plan_rectify_map(37, 131, 3, table, table + 3 * 176 - 8)) && mok(plan_rectify_map(37, 131, 3, table, table + 3 * 176)));
    const RectifyMapPlan mp = plan_rectify_map(37, 131, 3, table, map);
    CHECK(mp.grid_x == (37 * 131 + 255) / 256 && mp.grid_y == 3 && mp.map_bytes == 3 * 37 * 131 * 8);

    // the grid: every frame of every group is in exactly one chunk
    for (int batch : {1, 2, 5, 9, 64, 1024})
        for (int n_maps : {1, 2, 3, batch, batch + 3}) {
            const RectifyPlan p = plan_rectify(41, 150, 1, 37, 131, batch, n_maps, 0, src, map, 0, dst + 0x10000000u);
            CHECK(ok(p) && !p.indexed && p.tiles_x == 3 && p.grid_x == 9);
            const unsigned groups = (unsigned)(n_maps < batch ? n_maps : batch);
            CHECK(p.grid_y == groups && p.grid_z >= 1 && p.per_chunk >= 1 && p.grid_z <= 65535);
            unsigned covered = 0;
            for (unsigned m = 0; m < groups; ++m) {
                const unsigned total = ((unsigned)batch - m + (unsigned)n_maps - 1) / (unsigned)n_maps;
                CHECK((uint64_t)p.per_chunk * p.grid_z >= total);                            // the chunks reach the group's last frame
                covered += total;
            }
            CHECK(covered == (unsigned)batch);
            CHECK((p.grid_z - 1) * p.per_chunk < ((unsigned)batch + groups - 1) / groups);   // and the last chunk is not empty for group 0
        }
    const RectifyPlan one = plan_rectify(512, 1392, 3, 352, 1216, 1024, 1, 0, src, map, 0, (uintptr_t)0x1000000000ull);
    CHECK(one.grid_x == 19 * 22 && one.grid_y == 1 && one.grid_z == 5 && one.per_chunk == 205);       // 418 tiles: five chunks reach 2048 workgroups
    const RectifyPlan each = plan_rectify(512, 1392, 3, 352, 1216, 1024, 1024, 0, src, map, 0, (uintptr_t)0x1000000000ull);
    CHECK(each.grid_y == 1024 && each.grid_z == 1 && each.per_chunk == 1);
    const RectifyPlan ind = plan_rectify(41, 150, 3, 37, 131, 9, 2, 0, src, map, idx, dst);
    CHECK(ind.indexed && ind.grid_y == 9 && ind.grid_z == 1 && ind.per_chunk == 1);

    // the staged box: a pitch that holds the row at any byte shift, an odd number of quads; the budget
    for (uint32_t ch : {1u, 3u})
        for (uint32_t w = 1; w <= 16384; w += (w < 300 ? 1 : 97)) {
            const uint32_t p = rectify_pitch(w, ch);
            CHECK(p % 16 == 0 && (p / 16) % 2 == 1 && p >= 16 * ((15 + w * ch + 15) / 16) && p <= w * ch + 15 + 31);
            CHECK(rectify_box_fits(w, 1, ch) == (p <= kRectifyLdsBytes));
        }
    CHECK(rectify_box_fits(86, 24, 3) && rectify_box_fits(51, 23, 3));                       // a KITTI tile's box, BGR
    CHECK(!rectify_box_fits(2560, 640, 1) && !rectify_box_fits(16384, 16384, 3));
    std::printf("ok\n");
    return 0;
}
