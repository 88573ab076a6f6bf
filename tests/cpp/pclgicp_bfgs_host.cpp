// Host build of mr_slam_amd/csrc/pclgicp_bfgs.hpp (the text the device kernel compiles) for tests/test_pclgicp_cpu.py: C entry points
// (shared-library build) and a main() that runs the inner minimisation over a file of (sums, start) records (stand-alone build, also under
// the sanitizers).
#include "../../mr_slam_amd/csrc/pclgicp_bfgs.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" double pcl_host_objective(const double* sums /* [74] */, const double* x /* [6] */, double* g /* [6] or null */)
{
    return mrs::pcl_objective(sums, x, g);
}

extern "C" void pcl_host_bfgs(const double* sums /* [n][74] */, int n, double grad_tol, int max_inner, double* x /* [n][6], in and out */,
                              int* iterations /* [n] */, int* ending /* [n] */)
{
    for (int i = 0; i < n; ++i) ending[i] = mrs::pcl_bfgs(sums + mrs::kPclTerms * (long)i, grad_tol, max_inner, x + 6 * (long)i, iterations + i);
}

// steps 5-7 of one pair: X in and out; returns the inner ending, *state the outer state after iteration `it`
extern "C" int pcl_host_iterate(const double* sums, const double* pivot, double rot_eps, double trans_eps, double grad_tol, int max_iter,
                                int max_inner, int force_iters, int it, double* X, double* delta, int* inner_iterations, int* state)
{
    mrs::PclGicpCriteria c;
    c.rot_eps = rot_eps; c.trans_eps = trans_eps; c.grad_tol = grad_tol;
    c.max_iter = max_iter; c.max_inner = max_inner; c.force_iters = force_iters; c.pad = 0;
    const int end = mrs::pcl_gicp_iterate(sums, pivot, c, X, delta, inner_iterations);
    *state = mrs::pcl_gicp_converged(c, it, *delta);
    return end;
}

// pclgicp_bfgs_host IN OUT GRAD_TOL MAX_INNER: IN holds n x 80 doubles (74 sums, the start x), OUT receives n x 8 doubles (x, iterations, ending)
int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s in.bin out.bin gradient_tolerance max_inner_iterations\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> in;
    double buf[80];
    while (std::fread(buf, sizeof(double), 80, f) == 80) in.insert(in.end(), buf, buf + 80);
    std::fclose(f);
    const double tol = std::atof(argv[3]);
    const int max_inner = std::atoi(argv[4]);
    const int n = (int)(in.size() / 80);
    std::vector<double> out((size_t)n * 8);
    for (int i = 0; i < n; ++i) {
        double x[6];
        for (int k = 0; k < 6; ++k) x[k] = in[(size_t)i * 80 + 74 + k];
        int its = 0;
        const int end = mrs::pcl_bfgs(&in[(size_t)i * 80], tol, max_inner, x, &its);
        for (int k = 0; k < 6; ++k) out[(size_t)i * 8 + k] = x[k];
        out[(size_t)i * 8 + 6] = its; out[(size_t)i * 8 + 7] = end;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("%d minimisations\n", n);
    return ok ? 0 : 5;
}
