// Host build of mr_slam_amd/csrc/icp_update.hpp (the text the device kernel compiles) for tests/test_icp_cpu.py: three C entry points
// (shared-library build) and a main() that runs the rotation fit over a file of matrices (stand-alone build, also under the sanitizers).
#include "../../mr_slam_amd/csrc/icp_update.hpp"

#include <cstdio>
#include <vector>

extern "C" void icp_host_rotation(const double* H /* [n][9] */, int n, double* R /* [n][9] */)
{
    for (int i = 0; i < n; ++i) mrs::icp_rotation(H + 9 * (long)i, R + 9 * (long)i);
}

extern "C" void icp_host_rigid_fit(const double* sums /* [n][17] */, int n, double* D /* [n][16] */, double* mse /* [n] */)
{
    for (int i = 0; i < n; ++i) mse[i] = mrs::icp_rigid_fit(sums + mrs::kIcpTerms * (long)i, D + 16 * (long)i);
}

// one call of the state machine; *prev_mse is updated like the kernel's copy
extern "C" int icp_host_converged(int max_iter, int force_iters, double trans_eps, double rot_eps, double fit_eps, int it, const double* D,
                                  double mse, double* prev_mse)
{
    mrs::IcpCriteria c;
    c.trans_eps = trans_eps;
    c.rot_thr = mrs::icp_rotation_threshold(rot_eps, trans_eps);
    c.fit_eps = fit_eps;
    c.max_iter = max_iter;
    c.force_iters = force_iters;
    return mrs::icp_converged(c, it, D, mse, *prev_mse);
}

// icp_update_host IN OUT: IN holds n x 9 doubles (row-major H), OUT receives n x 9 doubles (row-major R)
int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> H;
    double buf[9];
    while (std::fread(buf, sizeof(double), 9, f) == 9) H.insert(H.end(), buf, buf + 9);
    std::fclose(f);
    const int n = (int)(H.size() / 9);
    std::vector<double> R(H.size());
    icp_host_rotation(H.data(), n, R.data());
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = std::fwrite(R.data(), sizeof(double), R.size(), f) == R.size();
    std::fclose(f);
    std::printf("%d matrices\n", n);
    return ok ? 0 : 5;
}
