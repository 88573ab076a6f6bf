// pcm_pose.hpp -- the pose arithmetic of pairwise consistency (pcm.hip), for the device and, compiled by g++, for the CPU tests.
//
// A pose is 12 doubles, the row-major 3x4 [R | t].  Rot3::Logmap and Pose3::Logmap are restated from upstream GTSAM 4.0 (gtsam is not in
// the reference tree), thresholds included.  Everything is fp64; the caller compiles without contraction.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define MRS_PCM_HD __host__ __device__ inline
#else
#define MRS_PCM_HD inline
#endif

namespace mrs {
namespace pcm {

constexpr int kPose = 12;                // doubles per pose
constexpr int kRecord = 2 * kPose;       // doubles per loop record: P = XA_i Z XB_k^-1, then B = XB_k

// rows 0..2 of a row-major 4x4
MRS_PCM_HD void pose_from_4x4(const double* m, double* p)
{
    for (int i = 0; i < kPose; ++i) p[i] = m[i];
}

// out = a b (out must not alias a or b)
MRS_PCM_HD void pose_mul(const double* a, const double* b, double* out)
{
    for (int r = 0; r < 3; ++r) {
        const double a0 = a[4 * r], a1 = a[4 * r + 1], a2 = a[4 * r + 2];
        for (int c = 0; c < 4; ++c) out[4 * r + c] = (a0 * b[c] + a1 * b[4 + c]) + a2 * b[8 + c];
        out[4 * r + 3] += a[4 * r + 3];
    }
}

// gtsam Pose3::inverse: (R^T, -R^T t) (out must not alias a)
MRS_PCM_HD void pose_inv(const double* a, double* out)
{
    for (int r = 0; r < 3; ++r) {
        out[4 * r] = a[r]; out[4 * r + 1] = a[4 + r]; out[4 * r + 2] = a[8 + r];
        out[4 * r + 3] = -((a[r] * a[3] + a[4 + r] * a[7]) + a[8 + r] * a[11]);
    }
}

// Rot3::Logmap of the rotation part of p
MRS_PCM_HD void rot_logmap(const double* p, double* w)
{
    const double R11 = p[0], R12 = p[1], R13 = p[2], R21 = p[4], R22 = p[5], R23 = p[6], R31 = p[8], R32 = p[9], R33 = p[10];
    const double kPi = 3.14159265358979323846;
    const double tr = (R11 + R22) + R33;
    if (fabs(tr + 1.0) < 1e-10) {                   // a turn by pi, up to rounding: the axis comes from a column
        if (fabs(R33 + 1.0) > 1e-10) {
            const double s = kPi / sqrt(2.0 + 2.0 * R33);
            w[0] = s * R13; w[1] = s * R23; w[2] = s * (1.0 + R33);
        } else if (fabs(R22 + 1.0) > 1e-10) {
            const double s = kPi / sqrt(2.0 + 2.0 * R22);
            w[0] = s * R12; w[1] = s * (1.0 + R22); w[2] = s * R32;
        } else {
            const double s = kPi / sqrt(2.0 + 2.0 * R11);
            w[0] = s * (1.0 + R11); w[1] = s * R21; w[2] = s * R31;
        }
        return;
    }
    const double tr_3 = tr - 3.0;
    double m;
    if (tr_3 < -1e-7) {
        const double theta = acos((tr - 1.0) / 2.0);
        m = theta / (2.0 * sin(theta));
    } else {
        m = 0.5 - tr_3 * tr_3 / 12.0;
    }
    w[0] = m * (R32 - R23); w[1] = m * (R13 - R31); w[2] = m * (R21 - R12);
}

// Pose3::Logmap: xi = [omega, u]
MRS_PCM_HD void pose_logmap(const double* p, double* xi)
{
    double w[3];
    rot_logmap(p, w);
    const double T0 = p[3], T1 = p[7], T2 = p[11];
    const double t = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    xi[0] = w[0]; xi[1] = w[1]; xi[2] = w[2];
    if (t < 1e-10) {
        xi[3] = T0; xi[4] = T1; xi[5] = T2;
        return;
    }
    const double a0 = w[0] / t, a1 = w[1] / t, a2 = w[2] / t;
    const double WT0 = a1 * T2 - a2 * T1, WT1 = a2 * T0 - a0 * T2, WT2 = a0 * T1 - a1 * T0;                 // W T = a x T
    const double WWT0 = a1 * WT2 - a2 * WT1, WWT1 = a2 * WT0 - a0 * WT2, WWT2 = a0 * WT1 - a1 * WT0;
    const double h = 0.5 * t, k = 1.0 - t / (2.0 * tan(0.5 * t));
    xi[3] = (T0 - h * WT0) + k * WWT0;
    xi[4] = (T1 - h * WT1) + k * WWT1;
    xi[5] = (T2 - h * WT2) + k * WWT2;
}

// |Logmap(p)|: the reference's "squared Mahalanobis distance" under its identity covariance, which is the square root
MRS_PCM_HD double pose_log_norm(const double* p)
{
    double xi[6];
    pose_logmap(p, xi);
    return sqrt((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + (xi[3] * xi[3] + xi[4] * xi[4])) + xi[5] * xi[5]);
}

// the record of loop (i, k, Z): P = XA_i Z XB_k^-1 and B = XB_k, from row-major 4x4 inputs
MRS_PCM_HD void loop_record(const double* XA_i, const double* Z, const double* XB_k, double* rec)
{
    double a[kPose], z[kPose], b[kPose], binv[kPose], az[kPose];
    pose_from_4x4(XA_i, a);
    pose_from_4x4(Z, z);
    pose_from_4x4(XB_k, b);
    pose_inv(b, binv);
    pose_mul(a, z, az);
    pose_mul(az, binv, rec);
    for (int i = 0; i < kPose; ++i) rec[kPose + i] = b[i];
}

// consistency distance of loops u < v from their records: E = B_u^-1 (P_u^-1 P_v) B_u, which is
// Z_u^-1 (XA_i^-1 XA_j) Z_v (XB_l^-1 XB_k) (pairwise_consistency.cpp:99-137) in another order of products
MRS_PCM_HD double pair_distance(const double* rec_u, const double* rec_v)
{
    double pinv[kPose], m[kPose], binv[kPose], mb[kPose], e[kPose];
    pose_inv(rec_u, pinv);
    pose_mul(pinv, rec_v, m);
    pose_inv(rec_u + kPose, binv);
    pose_mul(m, rec_u + kPose, mb);
    pose_mul(binv, mb, e);
    return pose_log_norm(e);
}

}  // namespace pcm
}  // namespace mrs
