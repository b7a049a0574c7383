// Exercises the connectivity pass through include/img_completion.h: dcmt_shim::slic_enforce_connectivity on clusters[col][row]
// against dcmt_slic_connectivity on the same labels row-major, label for label and count for count, on a raw int32 plane written
// by the pytest driver.  A shape the pass refuses must throw.  Writes the shim's result row-major as raw int32 and prints its count.
// Returns 0 when everything agreed.
//   shim_connectivity_test <rows> <cols> <n_centers> <in.i32> <out.i32>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), nc = std::atoi(argv[3]);
    const size_t px = (size_t)rows * cols;
    std::vector<int32_t> packed(px);
    FILE* f = std::fopen(argv[4], "rb");
    if (!f || std::fread(packed.data(), sizeof(int32_t), px, f) != px) return 3;
    std::fclose(f);
    std::vector<std::vector<int> > clusters(cols, std::vector<int>(rows));
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) clusters[j][i] = packed[(size_t)i * cols + j];
    const int count = dcmt_shim::slic_enforce_connectivity(clusters, nc);

    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 4;
    std::vector<int32_t> want(px, -1);
    int32_t want_count = -1;
    const size_t row = sizeof(int32_t) * (size_t)cols;
    if (dcmt_slic_connectivity(ctx, packed.data(), row, rows, cols, nc, want.data(), row, &want_count) != DCMT_OK) return 5;
    dcmt_destroy(ctx);
    if (count != want_count || count > dcmt_slic_connectivity_max_labels(rows, cols, nc)) return 6;
    std::vector<int32_t> got(px);
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) {
            got[(size_t)i * cols + j] = clusters[j][i];
            if (clusters[j][i] != want[(size_t)i * cols + j]) return 7;
            if (clusters[j][i] < 0 || clusters[j][i] >= (count > 1 ? count : 1)) return 8;
        }

    // fewer than 4 pixels per centre, a ragged or an empty vector: refused
    int thrown = 0;
    try { std::vector<std::vector<int> > c = clusters; dcmt_shim::slic_enforce_connectivity(c, (int)px); } catch (const std::runtime_error&) { ++thrown; }
    try { std::vector<std::vector<int> > c = clusters; c[cols - 1].push_back(0); if (cols > 1) dcmt_shim::slic_enforce_connectivity(c, nc); else throw std::runtime_error(""); }
    catch (const std::runtime_error&) { ++thrown; }
    try { std::vector<std::vector<int> > c; dcmt_shim::slic_enforce_connectivity(c, nc); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 3) return 9;

    FILE* o = std::fopen(argv[5], "wb");
    if (!o || std::fwrite(got.data(), sizeof(int32_t), px, o) != px) return 10;
    std::fclose(o);
    std::printf("%d\n", count);
    return 0;
}
