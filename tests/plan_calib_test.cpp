// The table checks of the *_calib_dev entry points (csrc/dcmt_plan_side.h: calib_table_aligned, calib_table_clear_of) on a CPU: the
// two pure functions every one of the four calls decides "null or misaligned table" and "table overlaps an output buffer" with.
// Built and run by tests/test_calib.py; prints every failed check, or "ok", and returns their number.
#include <cstdio>
#include <initializer_list>

#include "dcmt_plan_side.h"

using namespace dcmt::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 50) std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

int main()
{
    constexpr uintptr_t kTable = 0x700000000ull;            // 16-byte aligned
    // null and misaligned: 16 bytes for dcmt_project_calib, 8 for the other three records
    CHECK(!calib_table_aligned(0, 16) && !calib_table_aligned(0, 8));
    CHECK(calib_table_aligned(kTable, 16) && calib_table_aligned(kTable, 8));
    CHECK(!calib_table_aligned(kTable + 4, 16) && !calib_table_aligned(kTable + 8, 16) && !calib_table_aligned(kTable + 12, 16));
    CHECK(!calib_table_aligned(kTable + 4, 8) && calib_table_aligned(kTable + 8, 8) && !calib_table_aligned(kTable + 1, 8));
    // overlap with an output buffer, for each record size (96, 32, 136, 8 bytes) and a few batch sizes: the table is [t, t + rec * batch)
    for (size_t rec : {96u, 32u, 136u, 8u})
        for (int batch : {1, 3, 1024}) {
            const size_t bytes = rec * (size_t)batch;
            const size_t out_bytes = 4 * 5 * 7 * (size_t)batch;
            CHECK(calib_table_clear_of(kTable, rec, batch, kTable + bytes, out_bytes));               // the output right behind the table
            CHECK(calib_table_clear_of(kTable, rec, batch, kTable - out_bytes, out_bytes));           // right in front of it
            CHECK(!calib_table_clear_of(kTable, rec, batch, kTable + bytes - 1, out_bytes));          // the table's last byte
            CHECK(!calib_table_clear_of(kTable, rec, batch, kTable - out_bytes + 1, out_bytes));      // its first byte
            CHECK(!calib_table_clear_of(kTable, rec, batch, kTable, out_bytes));                      // the same start
            CHECK(!calib_table_clear_of(kTable + 16, rec, batch, kTable, bytes + 64));                // the table inside the output
            CHECK(!calib_table_clear_of(kTable, rec, batch, kTable + 4, 4));                          // the output inside the table
            CHECK(calib_table_clear_of(kTable, rec, batch, 0x900000000ull, out_bytes));               // far apart
        }
    // only the records of THIS call's batch count: a table with room for more may be followed by the output
    CHECK(calib_table_clear_of(kTable, 96, 2, kTable + 192, 560) && !calib_table_clear_of(kTable, 96, 3, kTable + 192, 560));
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures;
}
