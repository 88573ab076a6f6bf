// ransac_model.hpp -- the per-hypothesis arithmetic of the RANSAC pose from correspondences in fp64:
// the seeded draw of three distinct correspondences, the two pre-rejection tests (edge lengths, collinearity), the 3-point model through
// icp_rigid_fit (icp_update.hpp: Kabsch with a proper rotation from the 17 sums) and the inlier test.  open3d's
// registration_ransac_based_on_feature_matching is not part of the reference tree: the definition in DESIGN.md 4.22 is the contract,
// tests/golden/ransac_restate.py restates it in NumPy, parity with open3d itself is unpinned.
//
// Every expression below is written in the operation order of the contract and compiled without contraction (-ffp-contract=off), so the
// draw and the rejection verdicts are the same bits on the device, on the host and in the restatement; the model differs from LAPACK's
// by rounding only.  Compiled for the device by hipcc (ransac.hip) and for the host by g++ (tests/cpp/ransac_model_host.cpp,
// tests/test_ransac_cpu.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "icp_update.hpp"

namespace mrs {

// the splitmix64 finaliser
MRS_HD uint64_t ransac_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// three distinct indices in [0, M), M >= 3: a function of (seed, h, M) only
MRS_HD void ransac_draw(uint64_t seed, uint32_t h, uint64_t M, int64_t* idx)
{
    const uint64_t g = 0x9E3779B97F4A7C15ull;
    const uint64_t r0 = ransac_mix(seed + (3ull * h + 1ull) * g);
    const uint64_t r1 = ransac_mix(seed + (3ull * h + 2ull) * g);
    const uint64_t r2 = ransac_mix(seed + (3ull * h + 3ull) * g);
    const uint64_t i0 = r0 % M;
    uint64_t i1 = r1 % (M - 1);
    if (i1 >= i0) ++i1;
    const uint64_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    uint64_t i2 = r2 % (M - 2);
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
    idx[0] = (int64_t)i0; idx[1] = (int64_t)i1; idx[2] = (int64_t)i2;
}

// a correspondence is dead when a coordinate of either side is NaN or infinite
MRS_HD bool ransac_finite3(const double* p)
{
    return fabs(p[0]) <= DBL_MAX && fabs(p[1]) <= DBL_MAX && fabs(p[2]) <= DBL_MAX;
}

MRS_HD double ransac_norm2(double x, double y, double z) { return (x * x + y * y) + z * z; }

// one side of the collinearity test: |e1 x e2|^2 > min_sin2 (|e1|^2 |e2|^2); the cross product is written out (eig3_cross contracts)
MRS_HD bool ransac_spread(const double* e1, const double* e2, double min_sin2)
{
    const double cx = e1[1] * e2[2] - e1[2] * e2[1];
    const double cy = e1[2] * e2[0] - e1[0] * e2[2];
    const double cz = e1[0] * e2[1] - e1[1] * e2[0];
    const double c2 = ransac_norm2(cx, cy, cz);
    const double n1 = ransac_norm2(e1[0], e1[1], e1[2]), n2 = ransac_norm2(e2[0], e2[1], e2[2]);
    return !(c2 <= min_sin2 * (n1 * n2));
}

MRS_HD bool ransac_edge(double dp, double dq, double s2)
{
    return dp > 0.0 && dq > 0.0 && dp >= s2 * dq && dq >= s2 * dp;
}

// the pre-rejection of a triple p[3][3] -> q[3][3] (drawn order); s2 = edge_similarity^2, formed once by the caller
MRS_HD bool ransac_triple_ok(const double* p, const double* q, double s2, double min_sin2)
{
    for (int k = 0; k < 3; ++k)
        if (!ransac_finite3(p + 3 * k) || !ransac_finite3(q + 3 * k)) return false;
    const int ea[3] = {0, 0, 1}, eb[3] = {1, 2, 2};
    for (int e = 0; e < 3; ++e) {
        const double* pa = p + 3 * ea[e]; const double* pb = p + 3 * eb[e];
        const double* qa = q + 3 * ea[e]; const double* qb = q + 3 * eb[e];
        const double dp = ransac_norm2(pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]);
        const double dq = ransac_norm2(qb[0] - qa[0], qb[1] - qa[1], qb[2] - qa[2]);
        if (!ransac_edge(dp, dq, s2)) return false;
    }
    const double p1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, p2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    const double q1[3] = {q[3] - q[0], q[4] - q[1], q[5] - q[2]}, q2[3] = {q[6] - q[0], q[7] - q[1], q[8] - q[2]};
    return ransac_spread(p1, p2, min_sin2) && ransac_spread(q1, q2, min_sin2);
}

// one correspondence a -> b added to the 17 sums of icp_update.hpp
MRS_HD void ransac_accumulate(double* s, const double* a, const double* b)
{
    s[0] += 1.0;
    for (int r = 0; r < 3; ++r) {
        s[1 + r] += a[r];
        s[4 + r] += b[r];
        for (int c = 0; c < 3; ++c) s[7 + 3 * r + c] += a[r] * b[c];
    }
    s[16] += ransac_norm2(b[0] - a[0], b[1] - a[1], b[2] - a[2]);
}

// the 3-point model: the sums over the triple in drawn order, left to right from 0, through icp_rigid_fit -> D row-major 4x4
MRS_HD void ransac_triple_fit(const double* p, const double* q, double* D)
{
    double s[kIcpTerms];
    for (int i = 0; i < kIcpTerms; ++i) s[i] = 0.0;
    for (int k = 0; k < 3; ++k) ransac_accumulate(s, p + 3 * k, q + 3 * k);
    icp_rigid_fit(s, D);
}

// squared residual of p -> q under D (row-major 4x4; only its first three rows are read)
MRS_HD double ransac_residual2(const double* D, double px, double py, double pz, double qx, double qy, double qz)
{
    const double ex = (((D[0] * px + D[1] * py) + D[2] * pz) + D[3]) - qx;
    const double ey = (((D[4] * px + D[5] * py) + D[6] * pz) + D[7]) - qy;
    const double ez = (((D[8] * px + D[9] * py) + D[10] * pz) + D[11]) - qz;
    return (ex * ex + ey * ey) + ez * ez;
}

// inlier iff e2 <= d2 (d2 = max_distance max_distance, formed once); false for a NaN residual
MRS_HD bool ransac_inlier(double e2, double d2) { return e2 <= d2; }

}  // namespace mrs
