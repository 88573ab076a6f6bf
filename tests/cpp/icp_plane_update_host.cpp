// Host build of mr_slam_amd/csrc/icp_plane_update.hpp (the text the device kernel compiles) for tests/test_icp_plane_cpu.py: C entry points
// (shared-library build) and a main() that runs the fit over a file of sums (stand-alone build, also under the sanitizers); and of
// eig3.hpp's eigenvalues, whose deviation from LAPACK sets the curvature tolerance of tests/test_icp_plane_gpu.py.
#include "../../mr_slam_amd/csrc/icp_plane_update.hpp"

#include <cstdio>
#include <vector>

// per system: ok [n] (0 = rank-deficient), x [n][6], D [n][16], mse [n]
extern "C" void icp_plane_host_fit(const double* sums /* [n][29] */, int n, int* ok, double* x, double* D, double* mse)
{
    for (int i = 0; i < n; ++i) {
        const double* s = sums + mrs::kIcpPlaneTerms * (long)i;
        for (int j = 0; j < 6; ++j) x[6 * (long)i + j] = 0.0;
        (void)mrs::icp_plane_solve(s, x + 6 * (long)i);
        ok[i] = mrs::icp_plane_fit(s, D + 16 * (long)i, mse + i) ? 1 : 0;
    }
}

extern "C" void icp_plane_host_delta(const double* x /* [n][6] */, int n, double* D /* [n][16] */)
{
    for (int i = 0; i < n; ++i) mrs::icp_plane_delta(x + 6 * (long)i, D + 16 * (long)i);
}

// eigenvalues (descending) of n symmetric 3x3 matrices (row-major, 9 doubles each)
extern "C" void eig3_host_eigvals(const double* C /* [n][9] */, int n, double* w /* [n][3] */)
{
    for (int i = 0; i < n; ++i) mrs::sym3_eigvals(C + 9 * (long)i, w + 3 * (long)i);
}

// icp_plane_update_host IN OUT: IN holds n x 29 doubles (sums), OUT receives per system 1 + 6 + 16 doubles (ok, x, D)
int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> S;
    double buf[mrs::kIcpPlaneTerms];
    while (std::fread(buf, sizeof(double), mrs::kIcpPlaneTerms, f) == (size_t)mrs::kIcpPlaneTerms) S.insert(S.end(), buf, buf + mrs::kIcpPlaneTerms);
    std::fclose(f);
    const int n = (int)(S.size() / mrs::kIcpPlaneTerms);
    std::vector<int> ok(n);
    std::vector<double> x(6 * (size_t)n), D(16 * (size_t)n), mse(n), out;
    icp_plane_host_fit(S.data(), n, ok.data(), x.data(), D.data(), mse.data());
    for (int i = 0; i < n; ++i) {
        out.push_back(ok[i]);
        out.insert(out.end(), x.begin() + 6 * (size_t)i, x.begin() + 6 * (size_t)i + 6);
        out.insert(out.end(), D.begin() + 16 * (size_t)i, D.begin() + 16 * (size_t)i + 16);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool fine = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("%d systems\n", n);
    return fine ? 0 : 5;
}
