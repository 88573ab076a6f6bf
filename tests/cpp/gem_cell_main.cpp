// Stand-alone host program over the per-cell arithmetic of the global elevation map (mr_slam_amd/csrc/gem_cell.hpp), for a sanitizer build
// on the CPU (tests/test_gem_cpu.py compiles it with -fsanitize=address,undefined and -ffp-contract=off and compares what it writes with
// the NumPy restatement, bit for bit).
//   in : int32 n, m, w, c | float [n][4] (zo, vo, zn, vn) | float [m] coordinates | double resolution | float [2][16] (opt, pose)
//        | float [w][7] (px, py, elevation, cx, cy, dx, dy) | float half
//        | float [c][4] (x, y, z, travers) | double [5] (origin x, y, costmap resolution, traversability threshold, elevation threshold)
//        | int32 [2] grid size
//   out: float [n][4] (z, var weighted; z, var as written) | int32 [m][2] (keyed, key) | float [m] cell centres | float [16] correction
//        | int32 [w] window verdicts
//        | int32 [c][5] (inside, mx, my, cost by traversability, cost by elevation) | float [c][3] the point moved by the correction
//        | uint64 [m] pack_key(key, key of the next coordinate) where both are keyed, else 0
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mr_slam_amd/csrc/gem_cell.hpp"

namespace G = mrs::gem;

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t nmw[4] = {0, 0, 0, 0};
    if (fread(nmw, sizeof(int32_t), 4, f) != 4) return 2;
    for (int32_t v : nmw)
        if (v < 0 || v > (1 << 20)) return 2;
    const size_t n = (size_t)nmw[0], m = (size_t)nmw[1], w = (size_t)nmw[2], c = (size_t)nmw[3];
    std::vector<float> quad(n * 4), coord(m), mats(32), win(w * 7), pts(c * 4);
    double res = 0.0, cm[5] = {0, 0, 0, 0, 0};
    int32_t size[2] = {0, 0};
    float half = 0.0f;
    bool ok = fread(quad.data(), sizeof(float), quad.size(), f) == quad.size() && fread(coord.data(), sizeof(float), m, f) == m &&
              fread(&res, sizeof(double), 1, f) == 1 && fread(mats.data(), sizeof(float), 32, f) == 32 &&
              fread(win.data(), sizeof(float), win.size(), f) == win.size() && fread(&half, sizeof(float), 1, f) == 1 &&
              fread(pts.data(), sizeof(float), pts.size(), f) == pts.size() && fread(cm, sizeof(double), 5, f) == 5 && fread(size, sizeof(int32_t), 2, f) == 2;
    fclose(f);
    if (!ok) return 2;

    std::vector<float> fused(n * 4), centre(m, 0.0f), T(16);
    std::vector<int32_t> key(m * 2, 0), verdict(w), cost(c * 5, 0);
    std::vector<float> moved(c * 3);
    std::vector<uint64_t> packed(m, 0);
    for (size_t i = 0; i < n; ++i) {
        const float* q = &quad[i * 4];
        G::fuse_zvar(G::kWeighted, q[0], q[1], q[2], q[3], &fused[i * 4 + 0], &fused[i * 4 + 1]);
        G::fuse_zvar(G::kAsWritten, q[0], q[1], q[2], q[3], &fused[i * 4 + 2], &fused[i * 4 + 3]);
    }
    for (size_t i = 0; i < m; ++i) {
        int32_t k = 0;
        key[i * 2] = G::cell_key(coord[i], res, &k) ? 1 : 0;
        key[i * 2 + 1] = k;
        if (key[i * 2]) centre[i] = G::cell_centre(k, res);
    }
    G::correction(&mats[0], &mats[16], T.data());
    for (size_t i = 0; i < w; ++i) {
        const float* p = &win[i * 7];
        verdict[i] = G::leaves_window(p[0], p[1], p[2], p[3], p[4], p[5], p[6], half) ? 1 : 0;
    }
    for (size_t i = 0; i < m; ++i)
        if (key[i * 2] && key[((i + 1) % m) * 2]) packed[i] = G::pack_key(key[i * 2 + 1], key[((i + 1) % m) * 2 + 1]);
    for (size_t i = 0; i < c; ++i) {
        const float* p = &pts[i * 4];
        int mx = 0, my = 0;
        cost[i * 5] = G::world_to_map(p[0], p[1], cm[0], cm[1], cm[2], size[0], size[1], &mx, &my) ? 1 : 0;
        cost[i * 5 + 1] = mx;
        cost[i * 5 + 2] = my;
        cost[i * 5 + 3] = G::cell_cost(p[2], p[3], 0, cm[3]);
        cost[i * 5 + 4] = G::cell_cost(p[2], p[3], 1, cm[4]);
        G::move_point(T.data(), p[0], p[1], p[2], &moved[i * 3], &moved[i * 3 + 1], &moved[i * 3 + 2]);
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    ok = fwrite(fused.data(), sizeof(float), fused.size(), o) == fused.size() && fwrite(key.data(), sizeof(int32_t), key.size(), o) == key.size() &&
         fwrite(centre.data(), sizeof(float), m, o) == m && fwrite(T.data(), sizeof(float), 16, o) == 16 &&
         fwrite(verdict.data(), sizeof(int32_t), w, o) == w && fwrite(cost.data(), sizeof(int32_t), cost.size(), o) == cost.size() &&
         fwrite(moved.data(), sizeof(float), moved.size(), o) == moved.size() && fwrite(packed.data(), sizeof(uint64_t), m, o) == m;
    fclose(o);
    printf("gem_cell: %zu fusions, %zu keys, %zu window verdicts, %zu costmap points\n", n, m, w, c);
    return ok ? 0 : 1;
}
