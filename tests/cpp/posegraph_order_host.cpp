// posegraph_order.hpp, the text posegraph.hip compiles for its symbolic phase, built for the host (tests/test_posegraph_sparse_cpu.py).
//   IN  = per problem, one after the other: int32 E, n_tgt, dense_limit, slack | int64 max_blocks | int32 tgt_a [n_tgt] | tgt_b [n_tgt]
//   OUT = per problem, int64: ok (0 / 1), count, E, eliminated, core, levels, blocks, updates, max_degree, then each of order, level_ptr, col_ptr,
//         col_struct, col_tgt, row_ptr, row_k, row_slot, core_tgt as its length and its entries (none of them when ok is 0)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "posegraph_order.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    std::vector<int64_t> out;
    while (std::fread(hdr, 4, 4, f) == 4) {                      // one problem after the other until the file ends
        int64_t max_blocks = 0;
        if (std::fread(&max_blocks, 8, 1, f) != 1 || hdr[0] < 0 || hdr[1] < hdr[0]) return 2;
        const int E = hdr[0], n_tgt = hdr[1];
        std::vector<int32_t> a(n_tgt), b(n_tgt);
        if (n_tgt && (std::fread(a.data(), 4, n_tgt, f) != (size_t)n_tgt || std::fread(b.data(), 4, n_tgt, f) != (size_t)n_tgt)) return 2;
        mrs::pgo::SparseOrder o;
        long long count = 0;
        const bool ok = mrs::pgo::sparse_order(E, n_tgt, a.data(), b.data(), hdr[2], hdr[3], max_blocks, &o, &count);
        out.insert(out.end(), {ok ? 1 : 0, count, o.E, o.eliminated, o.core, o.levels, o.blocks, o.updates, o.max_degree});
        if (!ok) continue;
        for (const std::vector<int>* v : {&o.order, &o.level_ptr, &o.col_ptr, &o.col_struct, &o.col_tgt, &o.row_ptr, &o.row_k, &o.row_slot, &o.core_tgt}) {
            out.push_back((int64_t)v->size());
            out.insert(out.end(), v->begin(), v->end());
        }
    }
    std::fclose(f);
    FILE* w = std::fopen(argv[2], "wb");
    if (!w) return 2;
    std::fwrite(out.data(), sizeof(int64_t), out.size(), w);
    std::fclose(w);
    return 0;
}
