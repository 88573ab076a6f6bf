// Drives mrslam::GlobalElevationMap (include/mrslam/gem.hpp) on a scene written by tests/test_gem_adapter.py:
//   in : int32 K, n_opt | K x (int32 n | cells [n][10] words | float pose [16] | float centre [2]) | float opt [n_opt][16]
//   out: int64 matched, dropped, cells | K x int64 submap sizes | the composed cells [cells][10] words | uint8 costmap [23][25]
#include <cstdio>
#include <vector>

#include "mrslam/gem.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[2];
    if (!f || std::fread(hdr, sizeof(int32_t), 2, f) != 2 || hdr[0] < 0 || hdr[1] < 0) return 2;
    const int K = hdr[0], n_opt = hdr[1];
    try {
        mrslam::GlobalElevationMap gem(0.2);
        for (int i = 0; i < K; ++i) {
            int32_t n = 0;
            float pose[16], centre[2];
            if (std::fread(&n, sizeof(int32_t), 1, f) != 1 || n < 0) return 2;
            std::vector<mrslam::ElevationCell> cells((size_t)n);
            if (std::fread(cells.data(), sizeof(mrslam::ElevationCell), cells.size(), f) != cells.size() || std::fread(pose, 4, 16, f) != 16 ||
                std::fread(centre, 4, 2, f) != 2)
                return 2;
            gem.appendCells(cells.data(), n);
            gem.closeSubmap(pose, centre);
        }
        std::vector<float> opt((size_t)n_opt * 16);
        if (std::fread(opt.data(), 4, opt.size(), f) != opt.size()) return 2;
        std::fclose(f);
        const int64_t matched = gem.updateGlobal(opt.data(), n_opt);
        const std::vector<mrslam::ElevationCell> all = gem.compose();
        const std::vector<uint8_t> grid = gem.costmap(all, -2.0, -2.0, 25, 23, 0.2, 0, 0.5);
        const int64_t head[3] = {matched, gem.dropped(), (int64_t)all.size()};
        std::printf("submaps=%d matched=%lld dropped=%lld cells=%lld\n", gem.size(), (long long)head[0], (long long)head[1], (long long)head[2]);
        FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(head, sizeof(int64_t), 3, o);
        for (int i = 0; i < gem.size(); ++i) {
            const int64_t n = (int64_t)gem.submap(i).size();
            std::fwrite(&n, sizeof(int64_t), 1, o);
        }
        std::fwrite(all.data(), sizeof(mrslam::ElevationCell), all.size(), o);
        std::fwrite(grid.data(), 1, grid.size(), o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
    return 0;
}
