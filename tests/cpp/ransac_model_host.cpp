// Host build of mr_slam_amd/csrc/ransac_model.hpp (the text the device kernels compile) for tests/test_ransac_cpu.py: two C entry points
// (shared-library build) and a main() that runs them over a file of correspondences (stand-alone build, also under the sanitizers).
#include "../../mr_slam_amd/csrc/ransac_model.hpp"

#include <cstdio>
#include <vector>

static void widen(const float* x, int stride, long row, double* out)
{
    for (int k = 0; k < 3; ++k) out[k] = (double)x[row * stride + k];
}

// every hypothesis 0 .. H - 1 of one pair (M >= 3): idx [H][3], ok [H], D [H][16] (untouched where ok = 0)
extern "C" void ransac_host_hypotheses(const float* src, const float* dst, int stride, long M, unsigned long long seed, int H,
                                       double edge_similarity, double min_sin2, long long* idx, unsigned char* ok, double* D)
{
    const double s2 = edge_similarity * edge_similarity;
    for (int h = 0; h < H; ++h) {
        int64_t i[3];
        mrs::ransac_draw(seed, (uint32_t)h, (uint64_t)M, i);
        double p[9], q[9];
        for (int k = 0; k < 3; ++k) {
            idx[3 * (long)h + k] = i[k];
            widen(src, stride, (long)i[k], p + 3 * k);
            widen(dst, stride, (long)i[k], q + 3 * k);
        }
        ok[h] = mrs::ransac_triple_ok(p, q, s2, min_sin2) ? 1 : 0;
        if (ok[h]) mrs::ransac_triple_fit(p, q, D + 16 * (long)h);
    }
}

// the inlier mask of one model over the pair; returns the count
extern "C" int ransac_host_score(const float* src, const float* dst, int stride, long M, const double* D, double max_distance,
                                 unsigned char* mask)
{
    const double d2 = max_distance * max_distance;
    int count = 0;
    for (long m = 0; m < M; ++m) {
        double p[3], q[3];
        widen(src, stride, m, p);
        widen(dst, stride, m, q);
        const bool in = mrs::ransac_finite3(p) && mrs::ransac_finite3(q) &&
                        mrs::ransac_inlier(mrs::ransac_residual2(D, p[0], p[1], p[2], q[0], q[1], q[2]), d2);
        mask[m] = in ? 1 : 0;
        count += in ? 1 : 0;
    }
    return count;
}

// ransac_model_host IN OUT SEED H MAX_DISTANCE: IN holds M x 6 floats (src xyz, dst xyz per row); OUT receives, per hypothesis, the three
// indices, the verdict, the 16 doubles of the model (zeros when rejected) and its inlier count (-1 when rejected), all as doubles
int main(int argc, char** argv)
{
    if (argc != 6) { std::fprintf(stderr, "usage: %s in.bin out.bin seed hypotheses max_distance\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> rows;
    float buf[6];
    while (std::fread(buf, sizeof(float), 6, f) == 6) rows.insert(rows.end(), buf, buf + 6);
    std::fclose(f);
    const long M = (long)(rows.size() / 6);
    unsigned long long seed = 0;
    int H = 0;
    double d = 0.0;
    if (std::sscanf(argv[3], "%llu", &seed) != 1 || std::sscanf(argv[4], "%d", &H) != 1 || std::sscanf(argv[5], "%lf", &d) != 1 || H < 1 || M < 3)
        return 2;
    std::vector<long long> idx(3 * (size_t)H);
    std::vector<unsigned char> ok((size_t)H), mask((size_t)M);
    std::vector<double> D(16 * (size_t)H, 0.0), out;
    ransac_host_hypotheses(rows.data(), rows.data() + 3, 6, M, seed, H, 0.9, 1e-6, idx.data(), ok.data(), D.data());
    int valid = 0;
    for (int h = 0; h < H; ++h) {
        for (int k = 0; k < 3; ++k) out.push_back((double)idx[3 * (size_t)h + k]);
        out.push_back((double)ok[h]);
        out.insert(out.end(), D.begin() + 16 * (size_t)h, D.begin() + 16 * (size_t)(h + 1));
        out.push_back(ok[h] ? (double)ransac_host_score(rows.data(), rows.data() + 3, 6, M, D.data() + 16 * (size_t)h, d, mask.data()) : -1.0);
        valid += ok[h];
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool good = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("%ld correspondences, %d of %d hypotheses valid\n", M, valid, H);
    return good ? 0 : 5;
}
