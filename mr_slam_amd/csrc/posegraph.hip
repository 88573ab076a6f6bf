// posegraph.hip -- pose-graph optimisation of the Mapping back end (C ABI mrs_pgo_*).
//
// What it replaces: evaluation_utils::centralizedGNEstimation (distributed_mapper/evaluation_utils.cpp:273-329, called at
// global_manager.cpp:1354 after every accepted loop closure): a chordal-relaxation solve for all rotations and then 200 unconditional
// Gauss-Newton iterations, each a re-linearisation of every factor and a sparse elimination on one host thread.  Here both stages go
// through one direct solver, templated on the block size B and the number of right-hand sides NR (3 and 3 for the rotations, 6 and 1 for
// Gauss-Newton), that uses the structure of the workload: a few odometry chains plus a comparatively small set of loop factors.
//   separators : every pose a loop factor touches, and cut poses so that no run of other poses is longer than the segment length.  The
//                runs between them (segments) are block-tridiagonal and independent of each other;
//   linearize  : k_pgo_linearize, a thread per factor: e, Hi^T Hi, Hi^T Hj, -Hi^T e, -Hj^T e (posegraph_factor.hpp), factor-major;
//                k_pgo_gather, a thread per pose, sums them in ascending factor order through a CSR.  No float atomics anywhere;
//   eliminate  : k_pgo_eliminate, a lane per segment walks its run: a B x B Cholesky of the pivot block per pose, the fill towards the
//                left separator carried along, the Schur contributions to the bounding separators left per segment, the per-pose factors
//                left for the way back;
//   reduced    : k_pgo_assemble sums, per block of the dense lower system of order B E, the separator's own block, the loop blocks and
//                the segment contributions in a fixed order (a list per block, built on the host).  The right-hand sides are appended as
//                NR extra rows, so that the blocked right-looking Cholesky (k_pgo_chol_panel on one workgroup, k_pgo_chol_trail over a
//                grid, per panel of kNB columns) performs the forward substitution on its way; k_pgo_chol_back is the other solve;
//   backsolve  : k_pgo_backsolve, a lane per segment, from its right separator down; k_pgo_scatter copies the separators' solutions;
//   retract    : k_pgo_retract, a thread per pose; max|delta| by an integer atomicMax on the bits of a non-negative double;
//   error      : 0.5 sum |e|^2 by a fixed two-level tree (k_pgo_sum1, k_pgo_sum2);
//   project    : k_pgo_project, stage 1: the closest rotation of each solved 3x3.
// Beyond the reference's settings: a covariance per factor, converted as convertToChordalNoise converts it
// (k_pgo_information after stage 1; the <true> instantiations of k_pgo_linearize, k_pgo_error and k_pgo_gather; the <false> ones keep the
// unit model's arithmetic), Levenberg-Marquardt step control (mrs_pgo_optimize_lm: lambda enters the gather, k_pgo_predicted and the sum
// tree give the predicted decrease, one previous copy of the poses) and robust kernels on the loop factors (weights in the linearisation).
// Past the dense system's MRS_PGO_MAX_SEPARATORS a handle may opt into a sparse elimination tier in front of it (DESIGN.md 4.23(j);
// posegraph_order.hpp for the pattern, k_pgo_sp_* here).  The marginal covariances of a result read the same factor
// backwards: the inverse of the dense system by tiles (k_pgo_inv_*), then the segments (k_pgo_marginal_walk, posegraph_marginal.hpp).
// No kernel waits for another workgroup, every device loop is bounded by a size known at launch, and a pivot block that is not positive
// definite becomes a status word (the walk goes on with a unit pivot; the host ends the call).  The host reads 16 bytes per iteration.
#include "common.hpp"
#include "posegraph_factor.hpp"
#include "posegraph_marginal.hpp"
#include "posegraph_order.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <utility>
#include <vector>

namespace {

using u64 = unsigned long long;
constexpr int kThreads = 256;
constexpr int kMaxChains = MRS_PGO_MAX_CHAINS, kMaxPoses = MRS_PGO_MAX_POSES, kMaxLoops = MRS_PGO_MAX_LOOPS, kMaxSep = MRS_PGO_MAX_SEPARATORS;
constexpr int kNB = MRS_PGO_PANEL_WIDTH;  // panel width of the dense Cholesky: a multiple of both block sizes
constexpr int kTile = 32;                // the trailing update works on kTile x kTile tiles
constexpr int kMT = MRS_PGO_MARGINAL_TILE;   // the tile of the reduced system's inverse (marginal covariances)
static_assert(kThreads % kMT == 0 && kMT % (kThreads / kMT) == 0 && kMT <= kThreads, "a workgroup covers a tile in whole rows");
constexpr int kBig = 1 << 30;            // a failed pivot is recorded as kBig - index by atomicMax: the lowest index wins, 0 = none
constexpr int kMarkTierDown = 8, kMarkTierUp = 9;   // StageMarks of the sparse tier: after its way down, before its way back
constexpr int kTypeShift = 24;           // a contribution is type << 24 | index
static_assert(kMaxPoses + kMaxLoops + 2 < (1 << kTypeShift), "a contribution's index must fit below its type");
enum : int { kNodeDiag = 0, kFactor = 1, kFactorT = 2, kSegLL = 3, kSegRR = 4, kSegRL = 5, kSegRLT = 6 };

struct Status {
    u64 max_delta;       // bits of max|delta|
    int seg_fail;        // kBig - pose of the lowest pose whose pivot block failed in a segment walk
    int dense_fail;      // kBig - row of the lowest failed pivot of the dense factorisation
};
static_assert(sizeof(Status) == 16, "the host reads 16 bytes per iteration");

inline unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// ------------------------------------------------------------------ small dense pieces, row-major B x B in registers

// lower Cholesky in place (only the lower triangle is read); a pivot that is not positive and finite is replaced by 1 -> false
template <int B>
__device__ __forceinline__ bool chol_inplace(double* D)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < B; ++j) {
        double d = D[j * B + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= D[j * B + k] * D[j * B + k];
        if (!(d > 0.0) || !isfinite(d)) {
            ok = false;
            d = 1.0;
        }
        d = sqrt(d);
        D[j * B + j] = d;
#pragma unroll
        for (int i = j + 1; i < B; ++i) {
            double s = D[i * B + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= D[i * B + k] * D[j * B + k];
            D[i * B + j] = s / d;
        }
    }
    return ok;
}

// M <- L^-1 M for M [B][C]
template <int B, int C>
__device__ __forceinline__ void lower_solve(const double* L, double* M)
{
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int i = 0; i < B; ++i) {
            double s = M[i * C + c];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= L[i * B + k] * M[k * C + c];
            M[i * C + c] = s / L[i * B + i];
        }
}

// v <- L^-T v
template <int B>
__device__ __forceinline__ void upper_solve(const double* L, double* v)
{
#pragma unroll
    for (int i = B - 1; i >= 0; --i) {
        double s = v[i];
#pragma unroll
        for (int k = i + 1; k < B; ++k) s -= L[k * B + i] * v[k];
        v[i] = s / L[i * B + i];
    }
}

// ------------------------------------------------------------------ linearisation

// What the weighted instantiations read and write per factor, 10 doubles each: wr and Lt [9] (posegraph_factor.hpp).
//   lam : the factor's information, fixed for a call (k_pgo_information);
//   eff : the information the last linearisation used, lam times the kernel's weight: what k_pgo_gather<true> sums for Hj^T L Hj;
//   r2, wk : e^T L e and the kernel's weight at the poses last looked at.
// A loop factor (f >= first_loop) under a kernel costs rho(r); `irls` = 0 leaves its blocks unscaled (the first solve).
struct Weights {
    const double* lam;
    double *eff, *r2, *wk;
    int first_loop, kernel, irls;
    double k;
};
constexpr int kInfo = 10;

// stage 2: a thread per factor
template <bool W>
__global__ __launch_bounds__(kThreads) void k_pgo_linearize(const double* __restrict__ T, const int* __restrict__ fi, const int* __restrict__ fj,
                                                            const double* __restrict__ Z, int F, double* __restrict__ Hii, double* __restrict__ Hij,
                                                            double* __restrict__ gi, double* __restrict__ gj, double* __restrict__ err, Weights wt)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    double Ti[12], Tj[12], z[12], e[12], hii[36], hij[36], a[6], b[6];
    const int i = fi[f], j = fj[f];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        Ti[k] = T[(size_t)i * 12 + k];
        Tj[k] = T[(size_t)j * 12 + k];
        z[k] = Z[(size_t)f * 12 + k];
    }
    double cost = 0.0;
    if (W) {
        double l[kInfo], RiRij[9];
#pragma unroll
        for (int k = 0; k < kInfo; ++k) l[k] = wt.lam[(size_t)f * kInfo + k];
        mrs::pgo::factor_error(Ti, Tj, z, RiRij, e);
        const double r2 = mrs::pgo::factor_sq_weighted(e, l[0], l + 1);
        const int kernel = f >= wt.first_loop ? wt.kernel : (int)mrs::pgo::kKernelNone;
        const double w = mrs::pgo::kernel_weight(kernel, wt.k, r2);
        cost = mrs::pgo::kernel_cost(kernel, wt.k, r2);
        if (wt.irls) {
#pragma unroll
            for (int k = 0; k < kInfo; ++k) l[k] *= w;
        }
        mrs::pgo::factor_normal_weighted(Ti, Tj, z, l[0], l + 1, e, hii, hij, a, b);
#pragma unroll
        for (int k = 0; k < kInfo; ++k) wt.eff[(size_t)f * kInfo + k] = l[k];
        wt.r2[f] = r2;
        wt.wk[f] = w;
    } else {
        mrs::pgo::factor_normal(Ti, Tj, z, e, hii, hij, a, b);
    }
#pragma unroll
    for (int k = 0; k < 36; ++k) {
        Hii[(size_t)f * 36 + k] = hii[k];
        Hij[(size_t)f * 36 + k] = hij[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        gi[(size_t)f * 6 + k] = a[k];
        gj[(size_t)f * 6 + k] = b[k];
    }
    err[f] = W ? cost : mrs::pgo::factor_half_sq(e);
}

// the error alone
template <bool W>
__global__ __launch_bounds__(kThreads) void k_pgo_error(const double* __restrict__ T, const int* __restrict__ fi, const int* __restrict__ fj,
                                                        const double* __restrict__ Z, int F, double* __restrict__ err, Weights wt)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    double Ti[12], Tj[12], z[12], e[12], RiRij[9];
    const int i = fi[f], j = fj[f];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        Ti[k] = T[(size_t)i * 12 + k];
        Tj[k] = T[(size_t)j * 12 + k];
        z[k] = Z[(size_t)f * 12 + k];
    }
    mrs::pgo::factor_error(Ti, Tj, z, RiRij, e);
    if (W) {
        double l[kInfo];
#pragma unroll
        for (int k = 0; k < kInfo; ++k) l[k] = wt.lam[(size_t)f * kInfo + k];
        const double r2 = mrs::pgo::factor_sq_weighted(e, l[0], l + 1);
        const int kernel = f >= wt.first_loop ? wt.kernel : (int)mrs::pgo::kKernelNone;
        wt.r2[f] = r2;
        wt.wk[f] = mrs::pgo::kernel_weight(kernel, wt.k, r2);
        err[f] = mrs::pgo::kernel_cost(kernel, wt.k, r2);
    } else {
        err[f] = mrs::pgo::factor_half_sq(e);
    }
}

// after stage 1, a thread per factor: the information of a factor that carries a covariance, from noise [F][10] = 1 / max(C00, C11, C22)
// and C[3:6, 3:6] + 0.01 I, and the stage-1 rotation of the factor's first pose; the unit model where noise[f][0] is 0
__global__ __launch_bounds__(kThreads) void k_pgo_information(const double* __restrict__ T0, const int* __restrict__ fi,
                                                              const double* __restrict__ noise, int F, double* __restrict__ lam)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    double l[kInfo] = {1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    const double wr = noise[(size_t)f * kInfo];
    if (wr != 0.0) {
        double Tk[12], P[9];
#pragma unroll
        for (int k = 0; k < 12; ++k) Tk[k] = T0[(size_t)fi[f] * 12 + k];
#pragma unroll
        for (int k = 0; k < 9; ++k) P[k] = noise[(size_t)f * kInfo + 1 + k];
        l[0] = wr;
        mrs::pgo::translation_information(Tk, P, l + 1);
    }
#pragma unroll
    for (int k = 0; k < kInfo; ++k) lam[(size_t)f * kInfo + k] = l[k];
}

// stage 1: the residual of factor (i, j) is Rij x_j - x_i per row of the rotations, so Hi^T Hj = -Rij and both diagonal blocks are I
__global__ __launch_bounds__(kThreads) void k_pgo_linearize_rot(const double* __restrict__ Z, int F1, double* __restrict__ Hij)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F1) return;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Hij[(size_t)f * 9 + 3 * r + c] = -Z[(size_t)f * 12 + 4 * r + c];
}

// stage 2: Hpp [36] and g [6] of pose p from its factors in ascending order; an entry of the CSR is factor << 1 | (1 if p is the factor's j)
// Levenberg-Marquardt: `diag` (optional) receives the diagonal of Hpp, which then gains lambda times itself
template <bool W>
__global__ __launch_bounds__(kThreads) void k_pgo_gather(const int* __restrict__ ptr, const int* __restrict__ ent, int N, int F,
                                                         const double* __restrict__ Hii, const double* __restrict__ gi, const double* __restrict__ gj,
                                                         double* __restrict__ Hpp, double* __restrict__ g, const double* __restrict__ eff,
                                                         double lambda, double* __restrict__ diag)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= N) return;
    double H[36], v[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = 0.0;
    const int u1 = ptr[p + 1];
    for (int u = ptr[p]; u < u1; ++u) {
        const int f = ent[u] >> 1;
        if (f >= F) continue;                                    // the anchor's factor belongs to stage 1
        if (ent[u] & 1) {
            if (W) {
                const double* l = eff + (size_t)f * kInfo;
#pragma unroll
                for (int k = 0; k < 3; ++k) H[7 * k] += l[0] * mrs::pgo::hjj_diagonal(k);
#pragma unroll
                for (int k = 0; k < 9; ++k) H[6 * (3 + k / 3) + 3 + k % 3] += l[1 + k];
#pragma unroll
                for (int k = 0; k < 6; ++k) v[k] += gj[(size_t)f * 6 + k];
            } else {
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    H[7 * k] += mrs::pgo::hjj_diagonal(k);
                    v[k] += gj[(size_t)f * 6 + k];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 36; ++k) H[k] += Hii[(size_t)f * 36 + k];
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] += gi[(size_t)f * 6 + k];
        }
    }
    if (diag) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            diag[(size_t)p * 6 + k] = H[7 * k];
            H[7 * k] += lambda * H[7 * k];
        }
    }
#pragma unroll
    for (int k = 0; k < 36; ++k) Hpp[(size_t)p * 36 + k] = H[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[(size_t)p * 6 + k] = v[k];
}

// Levenberg-Marquardt: the pose's share of delta^T (lambda diag(H) delta + g); half their sum is the predicted decrease
__global__ __launch_bounds__(kThreads) void k_pgo_predicted(const double* __restrict__ delta, const double* __restrict__ diag,
                                                            const double* __restrict__ g, double lambda, int N, double* __restrict__ out)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= N) return;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double d = delta[(size_t)p * 6 + k];
        s += d * (lambda * diag[(size_t)p * 6 + k] * d + g[(size_t)p * 6 + k]);
    }
    out[p] = s;
}

// stage 1: Hpp = (number of factors) I, plus I for the anchor's own prior, whose right-hand sides are the rows of the identity
__global__ __launch_bounds__(kThreads) void k_pgo_gather_rot(const int* __restrict__ ptr, int N, double* __restrict__ Hpp, double* __restrict__ g)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p > N) return;                                           // node N is the anchor
    const double d = (double)(ptr[p + 1] - ptr[p]) + (p == N ? 1.0 : 0.0);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Hpp[(size_t)p * 9 + 3 * r + c] = r == c ? d : 0.0;
            g[(size_t)p * 9 + 3 * r + c] = (p == N && r == c) ? 1.0 : 0.0;
        }
}

// ------------------------------------------------------------------ segments

struct SegView {
    int n;
    const int *first, *len, *chain, *left, *right;      // left / right: reduced index of the bounding separator, or -1
};

// the odometry factor between poses p and p + 1 of chain c is factor p - c
template <int B, int NR>
__global__ __launch_bounds__(64) void k_pgo_eliminate(SegView sv, const double* __restrict__ Hpp, const double* __restrict__ g,
                                                      const double* __restrict__ Hij, double* __restrict__ Lk, double* __restrict__ Ak,
                                                      double* __restrict__ Wk, double* __restrict__ yk, double* __restrict__ Sll,
                                                      double* __restrict__ Srr, double* __restrict__ Srl, double* __restrict__ gl,
                                                      double* __restrict__ gr, Status* st)
{
    constexpr int BB = B * B, BV = B * NR;
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= sv.n) return;
    const int first = sv.first[s], m = sv.len[s], chain = sv.chain[s], left = sv.left[s], right = sv.right[s];
    double Ct[BB], D[BB], W[BB], A[BB], y[BV], cD[BB], cy[BV], sll[BB], sgl[BV];
#pragma unroll
    for (int k = 0; k < BB; ++k) {
        cD[k] = 0.0;
        sll[k] = 0.0;
        Ct[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < BV; ++k) {
        cy[k] = 0.0;
        sgl[k] = 0.0;
    }
    if (left >= 0) {                                             // H(left, first) is the block of factor first - 1 - chain: Ct is its transpose
        const double* h = Hij + (size_t)(first - 1 - chain) * BB;
#pragma unroll
        for (int r = 0; r < B; ++r)
#pragma unroll
            for (int c = 0; c < B; ++c) Ct[r * B + c] = h[c * B + r];
    }
    for (int k = 0; k < m; ++k) {
        const int p = first + k;
#pragma unroll
        for (int e = 0; e < BB; ++e) D[e] = Hpp[(size_t)p * BB + e] - cD[e];
#pragma unroll
        for (int e = 0; e < BV; ++e) y[e] = g[(size_t)p * BV + e] - cy[e];
        if (!chol_inplace<B>(D)) atomicMax(&st->seg_fail, kBig - p);
        const bool has_next = k + 1 < m || right >= 0;
#pragma unroll
        for (int e = 0; e < BB; ++e) {
            W[e] = has_next ? Hij[(size_t)(p - chain) * BB + e] : 0.0;
            A[e] = Ct[e];
        }
        lower_solve<B, B>(D, W);
        lower_solve<B, B>(D, A);
#pragma unroll
        for (int q = 0; q < NR; ++q) lower_solve<B, 1>(D, y + q * B);
#pragma unroll
        for (int a = 0; a < B; ++a)
#pragma unroll
            for (int b = 0; b < B; ++b) {
                double aa = 0.0, ww = 0.0, wa = 0.0;
#pragma unroll
                for (int i = 0; i < B; ++i) {
                    aa += A[i * B + a] * A[i * B + b];
                    ww += W[i * B + a] * W[i * B + b];
                    wa += W[i * B + a] * A[i * B + b];
                }
                sll[a * B + b] += aa;
                cD[a * B + b] = ww;
                Ct[a * B + b] = -wa;
            }
#pragma unroll
        for (int q = 0; q < NR; ++q)
#pragma unroll
            for (int a = 0; a < B; ++a) {
                double ay = 0.0, wy = 0.0;
#pragma unroll
                for (int i = 0; i < B; ++i) {
                    ay += A[i * B + a] * y[q * B + i];
                    wy += W[i * B + a] * y[q * B + i];
                }
                sgl[q * B + a] += ay;
                cy[q * B + a] = wy;
            }
#pragma unroll
        for (int e = 0; e < BB; ++e) {
            Lk[(size_t)p * BB + e] = D[e];
            Ak[(size_t)p * BB + e] = A[e];
            Wk[(size_t)p * BB + e] = W[e];
        }
#pragma unroll
        for (int e = 0; e < BV; ++e) yk[(size_t)p * BV + e] = y[e];
    }
#pragma unroll
    for (int e = 0; e < BB; ++e) {
        Sll[(size_t)s * BB + e] = -sll[e];
        Srr[(size_t)s * BB + e] = -cD[e];
        Srl[(size_t)s * BB + e] = Ct[e];                         // rows of the right separator, columns of the left one
    }
#pragma unroll
    for (int e = 0; e < BV; ++e) {
        gl[(size_t)s * BV + e] = -sgl[e];
        gr[(size_t)s * BV + e] = -cy[e];
    }
}

// xr: the solved right-hand-side rows of the reduced system, row q at xr + q * ld
template <int B, int NR>
__global__ __launch_bounds__(64) void k_pgo_backsolve(SegView sv, const double* __restrict__ Lk, const double* __restrict__ Ak,
                                                      const double* __restrict__ Wk, const double* __restrict__ yk, const double* __restrict__ xr,
                                                      size_t ld, double* __restrict__ delta)
{
    constexpr int BB = B * B, BV = B * NR;
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= sv.n) return;
    const int first = sv.first[s], m = sv.len[s], left = sv.left[s], right = sv.right[s];
    double xl[BV], xn[BV], L[BB], v[B];
#pragma unroll
    for (int q = 0; q < NR; ++q)
#pragma unroll
        for (int i = 0; i < B; ++i) {
            xl[q * B + i] = left >= 0 ? xr[q * ld + (size_t)B * left + i] : 0.0;
            xn[q * B + i] = right >= 0 ? xr[q * ld + (size_t)B * right + i] : 0.0;
        }
    for (int k = m - 1; k >= 0; --k) {
        const int p = first + k;
#pragma unroll
        for (int e = 0; e < BB; ++e) L[e] = Lk[(size_t)p * BB + e];
#pragma unroll
        for (int q = 0; q < NR; ++q) {
#pragma unroll
            for (int i = 0; i < B; ++i) {
                double t = yk[(size_t)p * BV + q * B + i];
#pragma unroll
                for (int c = 0; c < B; ++c) t -= Ak[(size_t)p * BB + i * B + c] * xl[q * B + c];
#pragma unroll
                for (int c = 0; c < B; ++c) t -= Wk[(size_t)p * BB + i * B + c] * xn[q * B + c];
                v[i] = t;
            }
            upper_solve<B>(L, v);
#pragma unroll
            for (int i = 0; i < B; ++i) {
                xn[q * B + i] = v[i];
                delta[(size_t)p * BV + q * B + i] = v[i];
            }
        }
    }
}

template <int B, int NR>
__global__ __launch_bounds__(kThreads) void k_pgo_scatter(const int* __restrict__ sep_node, int E, const double* __restrict__ xr, size_t ld,
                                                          double* __restrict__ delta)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= E * B * NR) return;
    const int a = t / (B * NR), q = (t / B) % NR, i = t % B;
    delta[(size_t)sep_node[a] * (B * NR) + q * B + i] = xr[q * ld + (size_t)B * a + i];
}

// ------------------------------------------------------------------ the reduced system: S [n + NR][ld], lower, the right-hand sides as rows n ..

struct Parts {
    const double *Hpp, *g, *Hij, *Sll, *Srr, *Srl, *gl, *gr;
};

// entry e (et: of the transpose) of contribution c to a block of the reduced system
template <int B>
__device__ __forceinline__ double block_contribution(const Parts& P, int c, int e, int et)
{
    const int type = c >> kTypeShift;
    const size_t idx = (size_t)(c & ((1 << kTypeShift) - 1)) * (B * B);
    double v = 0.0;
    if (type == kNodeDiag) v = P.Hpp[idx + e];
    else if (type == kFactor) v = P.Hij[idx + e];
    else if (type == kFactorT) v = P.Hij[idx + et];
    else if (type == kSegLL) v = P.Sll[idx + e];
    else if (type == kSegRR) v = P.Srr[idx + e];
    else if (type == kSegRL) v = P.Srl[idx + e];
    else if (type == kSegRLT) v = P.Srl[idx + et];
    return v;
}

// entry e of contribution c (of a diagonal block's list) to the right-hand sides [NR][B] of its separator
template <int BV>
__device__ __forceinline__ double rhs_contribution(const Parts& P, int c, int e)
{
    const int type = c >> kTypeShift;
    const size_t idx = (size_t)(c & ((1 << kTypeShift) - 1)) * BV;
    double v = 0.0;
    if (type == kNodeDiag) v = P.g[idx + e];
    else if (type == kSegLL) v = P.gl[idx + e];
    else if (type == kSegRR) v = P.gr[idx + e];
    return v;
}

// a thread per (block, entry): the block's contributions in their listed order
template <int B>
__global__ __launch_bounds__(kThreads) void k_pgo_assemble(const int* __restrict__ tgt_a, const int* __restrict__ tgt_b, const int* __restrict__ tgt_ptr,
                                                           const int* __restrict__ contrib, int n_tgt, Parts P, double* __restrict__ S, size_t ld)
{
    constexpr int BB = B * B;
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_tgt * BB) return;
    const int blk = t / BB, e = t % BB, r = e / B, c = e % B, et = c * B + r;
    double sum = 0.0;
    const int u1 = tgt_ptr[blk + 1];
    for (int u = tgt_ptr[blk]; u < u1; ++u) sum += block_contribution<B>(P, contrib[u], e, et);
    S[((size_t)B * tgt_a[blk] + r) * ld + (size_t)B * tgt_b[blk] + c] = sum;
}

// a thread per (separator, right-hand side, row): the first E blocks are the diagonal ones, in the separators' order
template <int B, int NR>
__global__ __launch_bounds__(kThreads) void k_pgo_assemble_rhs(const int* __restrict__ tgt_ptr, const int* __restrict__ contrib, int E, Parts P,
                                                               double* __restrict__ rhs, size_t ld)
{
    constexpr int BV = B * NR;
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= E * BV) return;
    const int a = t / BV, e = t % BV, q = e / B, i = e % B;
    double sum = 0.0;
    const int u1 = tgt_ptr[a + 1];
    for (int u = tgt_ptr[a]; u < u1; ++u) sum += rhs_contribution<BV>(P, contrib[u], e);
    rhs[q * ld + (size_t)B * a + i] = sum;
}

// One panel: the Cholesky of the diagonal block [k0, k0 + nb) in LDS, then every row below it (the right-hand-side rows included) times the
// inverse transpose of that factor.  One workgroup.
__global__ __launch_bounds__(kThreads) void k_pgo_chol_panel(double* __restrict__ S, int n, int nt, size_t ld, int k0, Status* st)
{
    __shared__ double Ls[kNB][kNB + 1];
    const int tid = threadIdx.x, nb = min(kNB, n - k0);
    for (int e = tid; e < nb * nb; e += kThreads) {
        const int r = e / nb, c = e % nb;
        Ls[r][c] = c <= r ? S[(size_t)(k0 + r) * ld + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        if (tid == 0) {
            double d = Ls[j][j];
            if (!(d > 0.0) || !isfinite(d)) {
                atomicMax(&st->dense_fail, kBig - (k0 + j));
                d = 1.0;
            }
            Ls[j][j] = sqrt(d);
        }
        __syncthreads();
        if (tid > j && tid < nb) Ls[tid][j] /= Ls[j][j];
        __syncthreads();
        for (int e = tid; e < nb * nb; e += kThreads) {
            const int r = e / nb, c = e % nb;
            if (c > j && c <= r) Ls[r][c] -= Ls[r][j] * Ls[c][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < nb * nb; e += kThreads) {
        const int r = e / nb, c = e % nb;
        if (c <= r) S[(size_t)(k0 + r) * ld + k0 + c] = Ls[r][c];
    }
    for (int r = k0 + nb + tid; r < nt; r += kThreads) {
        double x[kNB];
        double* row = S + (size_t)r * ld + k0;
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
            if (c < nb) {
                double s = row[c];
#pragma unroll
                for (int d = 0; d < c; ++d) s -= x[d] * Ls[c][d];
                x[c] = s / Ls[c][c];
            } else {
                x[c] = 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < kNB; ++c)
            if (c < nb) row[c] = x[c];
    }
}

// the trailing update of one panel: S[i][j] -= sum_c S[i][k0 + c] S[j][k0 + c] for k0 + nb <= j <= i, j < n, i < nt; a workgroup per tile of
// the lower triangle
__global__ __launch_bounds__(kThreads) void k_pgo_chol_trail(double* __restrict__ S, int n, int nt, size_t ld, int k0, int nb)
{
    __shared__ double Lr[kTile][kNB + 1], Lc[kTile][kNB + 1];
    if (blockIdx.x > blockIdx.y) return;
    const int k1 = k0 + nb, i0 = k1 + blockIdx.y * kTile, j0 = k1 + blockIdx.x * kTile, tid = threadIdx.x;
    if (j0 >= n || i0 >= nt) return;
    for (int e = tid; e < kTile * kNB; e += kThreads) {
        const int r = e / kNB, c = e % kNB;
        Lr[r][c] = (i0 + r < nt && c < nb) ? S[(size_t)(i0 + r) * ld + k0 + c] : 0.0;
        Lc[r][c] = (j0 + r < n && c < nb) ? S[(size_t)(j0 + r) * ld + k0 + c] : 0.0;
    }
    __syncthreads();
    const int tx = tid % kTile, j = j0 + tx;
    for (int rr = tid / kTile; rr < kTile; rr += kThreads / kTile) {
        const int i = i0 + rr;
        if (i < nt && j < n && j <= i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < kNB; ++c) s += Lr[rr][c] * Lc[tx][c];
            S[(size_t)i * ld + j] -= s;
        }
    }
}

// L^T x = y on the nr right-hand-side rows, in place, panel after panel from the last; one workgroup
__global__ __launch_bounds__(kThreads) void k_pgo_chol_back(double* __restrict__ S, int n, size_t ld, int nr)
{
    __shared__ double Ls[kNB][kNB + 1];
    __shared__ double xs[3][kNB];
    const int tid = threadIdx.x;
    double* rhs = S + (size_t)n * ld;
    for (int blk = (n + kNB - 1) / kNB - 1; blk >= 0; --blk) {
        const int c0 = blk * kNB, nb = min(kNB, n - c0);
        for (int e = tid; e < nb * nb; e += kThreads) {
            const int r = e / nb, c = e % nb;
            Ls[r][c] = c <= r ? S[(size_t)(c0 + r) * ld + c0 + c] : 0.0;
        }
        __syncthreads();
        if (tid < nr) {
            for (int c = nb - 1; c >= 0; --c) {
                double s = rhs[(size_t)tid * ld + c0 + c];
                for (int d = c + 1; d < nb; ++d) s -= Ls[d][c] * xs[tid][d];
                s /= Ls[c][c];
                xs[tid][c] = s;
                rhs[(size_t)tid * ld + c0 + c] = s;
            }
        }
        __syncthreads();
        for (int r = tid; r < c0; r += kThreads)
            for (int q = 0; q < nr; ++q) {
                double s = rhs[(size_t)q * ld + r];
                for (int c = 0; c < nb; ++c) s -= S[(size_t)(c0 + c) * ld + r] * xs[q][c];
                rhs[(size_t)q * ld + r] = s;
            }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ marginal covariances (posegraph_marginal.hpp)
//
// The inverse of the reduced system from its Cholesky factor L (lower, in S): M = L^-1 by tiles of kMT, block row after block row, then
// Sigma = M^T M by independent tiles.  M is zero above its diagonal (the caller clears it), rows and columns past n read as zero.

// M[I, I] = L[I, I]^-1 of every diagonal tile: a column per thread, forward substitution from LDS
__global__ __launch_bounds__(kThreads) void k_pgo_inv_diag(const double* __restrict__ S, double* __restrict__ M, int n, size_t ld)
{
    __shared__ double Ls[kMT][kMT + 1], Xs[kMT][kMT + 1];
    const int tid = threadIdx.x, k0 = blockIdx.x * kMT, nb = min(kMT, n - k0);
    for (int e = tid; e < kMT * kMT; e += kThreads) {
        const int r = e / kMT, c = e % kMT;
        Ls[r][c] = (r < nb && c <= r) ? S[(size_t)(k0 + r) * ld + k0 + c] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    if (tid < nb) {
        const int c = tid;
        for (int i = c; i < nb; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= Ls[i][k] * Xs[k][c];
            Xs[i][c] = s / Ls[i][i];
        }
        for (int i = c; i < nb; ++i) M[(size_t)(k0 + i) * ld + k0 + c] = Xs[i][c];
    }
}

// block row I of M below the diagonal, a workgroup per tile J < I: M[I, J] = -M[I, I] sum_{K = J}^{I - 1} L[I, K] M[K, J], K ascending.
// Rows K < I of M are complete when row I is launched.
__global__ __launch_bounds__(kThreads) void k_pgo_inv_row(const double* __restrict__ S, double* __restrict__ M, int n, size_t ld, int I)
{
    __shared__ double As[kMT][kMT + 1], Bs[kMT][kMT + 1];
    const int tid = threadIdx.x, J = blockIdx.x, tx = tid % kMT, ty = tid / kMT, i0 = I * kMT, j0 = J * kMT;
    constexpr int kRows = kThreads / kMT, kPer = kMT / kRows;
    double acc[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) acc[q] = 0.0;
    for (int K = J; K < I; ++K) {
        const int k0 = K * kMT;
        __syncthreads();
        for (int e = tid; e < kMT * kMT; e += kThreads) {
            const int r = e / kMT, c = e % kMT;
            As[r][c] = i0 + r < n ? S[(size_t)(i0 + r) * ld + k0 + c] : 0.0;
            Bs[r][c] = M[(size_t)(k0 + r) * ld + j0 + c];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            double s = acc[q];
#pragma unroll
            for (int k = 0; k < kMT; ++k) s += As[ty + q * kRows][k] * Bs[k][tx];
            acc[q] = s;
        }
    }
    __syncthreads();
    for (int e = tid; e < kMT * kMT; e += kThreads) {
        const int r = e / kMT, c = e % kMT;
        As[r][c] = (i0 + r < n && i0 + c < n) ? M[(size_t)(i0 + r) * ld + i0 + c] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) Bs[ty + q * kRows][tx] = acc[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int r = ty + q * kRows;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kMT; ++k) s -= As[r][k] * Bs[k][tx];
        if (i0 + r < n) M[(size_t)(i0 + r) * ld + j0 + tx] = s;
    }
}

// Sigma = M^T M, a workgroup per tile (I, J) of the lower triangle: sum_{K >= I} M[K, I]^T M[K, J], K and the rows within a tile ascending;
// the tile and its mirror image are written, so Sigma is full and symmetric to the bit
__global__ __launch_bounds__(kThreads) void k_pgo_inv_product(const double* __restrict__ M, double* __restrict__ Sig, int n, size_t ld)
{
    __shared__ double As[kMT][kMT + 1], Bs[kMT][kMT + 1];
    if (blockIdx.x > blockIdx.y) return;
    const int tid = threadIdx.x, I = blockIdx.y, J = blockIdx.x, tx = tid % kMT, ty = tid / kMT, i0 = I * kMT, j0 = J * kMT;
    const int nblk = (n + kMT - 1) / kMT;
    constexpr int kRows = kThreads / kMT, kPer = kMT / kRows;
    double acc[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) acc[q] = 0.0;
    for (int K = I; K < nblk; ++K) {
        const int k0 = K * kMT;
        __syncthreads();
        for (int e = tid; e < kMT * kMT; e += kThreads) {
            const int r = e / kMT, c = e % kMT;
            const bool in = k0 + r < n;
            As[r][c] = (in && i0 + c < n) ? M[(size_t)(k0 + r) * ld + i0 + c] : 0.0;
            Bs[r][c] = (in && j0 + c < n) ? M[(size_t)(k0 + r) * ld + j0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            double s = acc[q];
#pragma unroll
            for (int k = 0; k < kMT; ++k) s += As[k][ty + q * kRows] * Bs[k][tx];
            acc[q] = s;
        }
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int i = i0 + ty + q * kRows, j = j0 + tx;
        if (i < n && j < n) {
            Sig[(size_t)i * ld + j] = acc[q];
            if (I != J) Sig[(size_t)j * ld + i] = acc[q];
        }
    }
}

// The segments backwards, a lane per segment (posegraph_marginal.hpp): from the blocks (r, r), (r, l), (l, l) of Sigma it leaves, per pose
// p of the segment, Spp [p] = S_pp and Spn [p] = S_{p, p + 1}, and Spn [l] of a left separator whose successor is the segment's first pose.
// A bounding separator that is missing (a chain's end, or the held pose 0) enters as zero blocks.
__global__ __launch_bounds__(64) void k_pgo_marginal_walk(SegView sv, const double* __restrict__ Lk, const double* __restrict__ Ak,
                                                          const double* __restrict__ Wk, const double* __restrict__ Sig, size_t ld,
                                                          double* __restrict__ Spp, double* __restrict__ Spn)
{
    constexpr int B = 6, BB = 36;
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= sv.n) return;
    const int first = sv.first[s], m = sv.len[s], left = sv.left[s], right = sv.right[s];
    double Sll[BB], Snl[BB], Snn[BB], L[BB], A[BB], W[BB], pl[BB], pn[BB], pp[BB];
#pragma unroll
    for (int r = 0; r < B; ++r)
#pragma unroll
        for (int c = 0; c < B; ++c) {
            Sll[r * B + c] = left >= 0 ? Sig[((size_t)B * left + r) * ld + (size_t)B * left + c] : 0.0;
            Snn[r * B + c] = right >= 0 ? Sig[((size_t)B * right + r) * ld + (size_t)B * right + c] : 0.0;
            Snl[r * B + c] = (left >= 0 && right >= 0) ? Sig[((size_t)B * right + r) * ld + (size_t)B * left + c] : 0.0;
        }
    for (int k = m - 1; k >= 0; --k) {
        const int p = first + k;
#pragma unroll
        for (int e = 0; e < BB; ++e) {
            L[e] = Lk[(size_t)p * BB + e];
            A[e] = Ak[(size_t)p * BB + e];
            W[e] = Wk[(size_t)p * BB + e];
        }
        mrs::pgo::marginal_step<B>(L, A, W, Sll, Snl, Snn, pl, pn, pp);
        const bool has_next = k + 1 < m || right >= 0;
#pragma unroll
        for (int e = 0; e < BB; ++e) {
            Spp[(size_t)p * BB + e] = pp[e];
            Spn[(size_t)p * BB + e] = has_next ? pn[e] : 0.0;
            Snl[e] = pl[e];
            Snn[e] = pp[e];
        }
    }
    if (left >= 0) {                                             // the left separator is pose first - 1: S_{l, first} = S_{first, l}^T
#pragma unroll
        for (int r = 0; r < B; ++r)
#pragma unroll
            for (int c = 0; c < B; ++c) Spn[(size_t)(first - 1) * BB + r * B + c] = Snl[c * B + r];
    }
}

// the block S_ab [36] of two poses the queries may name: a == b, both separators (or pose 0), or |a - b| == 1 within a chain
__device__ __forceinline__ void marginal_block(int a, int b, const int* __restrict__ sep_of, const double* __restrict__ Sig, size_t ld,
                                               const double* __restrict__ Spp, const double* __restrict__ Spn, double* X)
{
    const int sa = sep_of[a], sb = sep_of[b];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
            if (a == 0 || b == 0) v = 0.0;                       // the held pose
            else if (sa >= 0 && sb >= 0) v = Sig[((size_t)6 * sa + r) * ld + (size_t)6 * sb + c];
            else if (a == b) v = Spp[(size_t)a * 36 + r * 6 + c];
            else if (a < b) v = Spn[(size_t)a * 36 + r * 6 + c];
            else v = Spn[(size_t)b * 36 + c * 6 + r];
            X[r * 6 + c] = v;
        }
}

// A thread per query.  qj null: the marginal [36] of pose qi[u] (qi null: of pose u); otherwise the joint marginal [144] of (qi[u], qj[u]).
// The diagonal blocks are symmetric to the bit in either frame, the two cross blocks are each other's transpose.
__global__ __launch_bounds__(kThreads) void k_pgo_marginal_gather(const int* __restrict__ qi, const int* __restrict__ qj, int nq, int frame,
                                                                  const double* __restrict__ T, const int* __restrict__ sep_of,
                                                                  const double* __restrict__ Sig, size_t ld, const double* __restrict__ Spp,
                                                                  const double* __restrict__ Spn, double* __restrict__ out)
{
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= nq) return;
    const int i = qi ? qi[u] : u;
    double Ti[12], Tj[12], X[36];
#pragma unroll
    for (int k = 0; k < 12; ++k) Ti[k] = T[(size_t)i * 12 + k];
    marginal_block(i, i, sep_of, Sig, ld, Spp, Spn, X);
    if (frame == MRS_PGO_FRAME_POSE3) {
        mrs::pgo::marginal_to_pose3(Ti, Ti, X);
        mrs::pgo::marginal_symmetrize<6>(X);
    }
    if (!qj) {
#pragma unroll
        for (int e = 0; e < 36; ++e) out[(size_t)u * 36 + e] = X[e];
        return;
    }
    const int j = qj[u];
    double* o = out + (size_t)u * 144;
#pragma unroll
    for (int k = 0; k < 12; ++k) Tj[k] = T[(size_t)j * 12 + k];
#pragma unroll
    for (int e = 0; e < 36; ++e) o[(e / 6) * 12 + e % 6] = X[e];
    marginal_block(j, j, sep_of, Sig, ld, Spp, Spn, X);
    if (frame == MRS_PGO_FRAME_POSE3) {
        mrs::pgo::marginal_to_pose3(Tj, Tj, X);
        mrs::pgo::marginal_symmetrize<6>(X);
    }
#pragma unroll
    for (int e = 0; e < 36; ++e) o[(6 + e / 6) * 12 + 6 + e % 6] = X[e];
    marginal_block(i, j, sep_of, Sig, ld, Spp, Spn, X);
    if (frame == MRS_PGO_FRAME_POSE3) mrs::pgo::marginal_to_pose3(Ti, Tj, X);
#pragma unroll
    for (int e = 0; e < 36; ++e) {
        o[(e / 6) * 12 + 6 + e % 6] = X[e];
        o[(6 + e % 6) * 12 + e / 6] = X[e];
    }
}

// ------------------------------------------------------------------ the sparse tier in front of the dense system (posegraph_order.hpp)
//
// Column k (an elimination position) owns d + 1 blocks of Lb from block col_ptr[k] + k: L_k, then W_k[s] = A_rk L_k^-T for the rows r of its
// struct, and y_k [NR][B] in ysp.  Left-looking and pulled by the target: a block subtracts the products W_m[.] W_m[.]^T of the earlier
// columns m that reach both of its ends, found by merging the two ends' row lists, in ascending m.  Every entry has one thread and a fixed
// order of sums.

struct SpView {
    const int *order;                                            // position -> node (reduced index of the separator)
    const int *col_ptr, *col_struct, *col_tgt;                   // col_tgt: target << 1 | transposed, or -1
    const int *row_ptr, *row_k, *row_blk;                        // rows(p): the columns k reaching position p, and the block of W_k there
    int n_elim;
};

// entry (i, j) of sum over the columns m in both lists [a, a1) and [b, b1) of W_m[.] W_m[.]^T, subtracted from acc in ascending m
template <int B>
__device__ __forceinline__ double sp_pull(const SpView& v, int a, int a1, int b, int b1, const double* __restrict__ Lb, int i, int j, double acc)
{
    while (a < a1 && b < b1) {                                   // every turn moves a or b on: at most the two lengths together
        const int ka = v.row_k[a], kb = v.row_k[b];
        if (ka == kb) {
            const double *Wa = Lb + (size_t)v.row_blk[a] * (B * B) + i * B, *Wb = Lb + (size_t)v.row_blk[b] * (B * B) + j * B;
            double p = 0.0;
#pragma unroll
            for (int c = 0; c < B; ++c) p += Wa[c] * Wb[c];
            acc -= p;
        }
        a += ka <= kb;
        b += kb <= ka;
    }
    return acc;
}

// entry (q, i) of sum over rows(p) = [a, a1) of W_m[.] y_m, subtracted from acc in ascending m
template <int B, int NR>
__device__ __forceinline__ double sp_pull_rhs(const SpView& v, int a, int a1, const double* __restrict__ Lb, const double* __restrict__ ysp, int q,
                                              int i, double acc)
{
    for (; a < a1; ++a) {
        const double *W = Lb + (size_t)v.row_blk[a] * (B * B) + i * B, *y = ysp + (size_t)v.row_k[a] * (B * NR) + q * B;
        double p = 0.0;
#pragma unroll
        for (int c = 0; c < B; ++c) p += W[c] * y[c];
        acc -= p;
    }
    return acc;
}

// one launch per level, a workgroup per column k = k0 + blockIdx.x of it; tgt_ptr / contrib are the stage's own lists
template <int B, int NR>
__global__ __launch_bounds__(kThreads) void k_pgo_sp_column(SpView v, int k0, const int* __restrict__ tgt_ptr, const int* __restrict__ contrib,
                                                            const int* __restrict__ sep_node, Parts P, double* __restrict__ Lb,
                                                            double* __restrict__ ysp, Status* st)
{
    constexpr int BB = B * B, BV = B * NR;
    __shared__ double Ls[BB];
    const int k = k0 + blockIdx.x, tid = threadIdx.x, node = v.order[k], c0 = v.col_ptr[k], d = v.col_ptr[k + 1] - c0;
    const int rk0 = v.row_ptr[k], rk1 = v.row_ptr[k + 1];
    double* col = Lb + (size_t)(c0 + k) * BB;
    for (int it = tid; it < (d + 1) * BB + BV; it += kThreads) {
        if (it < (d + 1) * BB) {
            const int blk = it / BB, e = it % BB, i = e / B, j = e % B, et = j * B + i;
            const int ct = blk ? v.col_tgt[c0 + blk - 1] : node << 1, p = blk ? v.col_struct[c0 + blk - 1] : k;
            double sum = 0.0;
            if (ct >= 0) {
                const int tgt = ct >> 1, u1 = tgt_ptr[tgt + 1];
                for (int u = tgt_ptr[tgt]; u < u1; ++u) sum += (ct & 1) ? block_contribution<B>(P, contrib[u], et, e) : block_contribution<B>(P, contrib[u], e, et);
            }
            col[it] = sp_pull<B>(v, v.row_ptr[p], v.row_ptr[p + 1], rk0, rk1, Lb, i, j, sum);
        } else {
            const int e = it - (d + 1) * BB, q = e / B, i = e % B;
            double sum = 0.0;
            const int u1 = tgt_ptr[node + 1];
            for (int u = tgt_ptr[node]; u < u1; ++u) sum += rhs_contribution<BV>(P, contrib[u], e);
            ysp[(size_t)k * BV + e] = sp_pull_rhs<B, NR>(v, rk0, rk1, Lb, ysp, q, i, sum);
        }
    }
    __syncthreads();
    if (tid == 0) {
        double D[BB];
#pragma unroll
        for (int e = 0; e < BB; ++e) D[e] = col[e];
        if (!chol_inplace<B>(D)) atomicMax(&st->seg_fail, kBig - sep_node[node]);
#pragma unroll
        for (int e = 0; e < BB; ++e) {
            col[e] = D[e];
            Ls[e] = D[e];
        }
    }
    __syncthreads();
    for (int it = tid; it < d * B; it += kThreads) {             // a row w of a block below: w L_k^T = a
        double* row = col + BB + (size_t)it * B;
        double w[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            double s = row[j];
#pragma unroll
            for (int c = 0; c < j; ++c) s -= w[c] * Ls[j * B + c];
            w[j] = s / Ls[j * B + j];
        }
#pragma unroll
        for (int j = 0; j < B; ++j) row[j] = w[j];
    }
    if (tid < NR) {
        double y[B];
#pragma unroll
        for (int i = 0; i < B; ++i) y[i] = ysp[(size_t)k * BV + tid * B + i];
        lower_solve<B, 1>(Ls, y);
#pragma unroll
        for (int i = 0; i < B; ++i) ysp[(size_t)k * BV + tid * B + i] = y[i];
    }
}

// after the assembly of the core's own contributions: a grid row per core separator a, a thread per entry of its blocks (a, b <= a) and of
// its right-hand sides
template <int B, int NR>
__global__ __launch_bounds__(kThreads) void k_pgo_sp_core(SpView v, int core, const double* __restrict__ Lb, const double* __restrict__ ysp,
                                                          double* __restrict__ S, size_t ld)
{
    constexpr int BB = B * B, BV = B * NR;
    const int a = blockIdx.y, it = blockIdx.x * kThreads + threadIdx.x;
    const int ra0 = v.row_ptr[v.n_elim + a], ra1 = v.row_ptr[v.n_elim + a + 1];
    if (ra0 == ra1) return;
    if (it < (a + 1) * BB) {
        const int b = it / BB, e = it % BB, i = e / B, j = e % B;
        double* s = S + ((size_t)B * a + i) * ld + (size_t)B * b + j;
        *s = sp_pull<B>(v, ra0, ra1, v.row_ptr[v.n_elim + b], v.row_ptr[v.n_elim + b + 1], Lb, i, j, *s);
    } else if (it < (a + 1) * BB + BV) {
        const int e = it - (a + 1) * BB, q = e / B, i = e % B;
        double* s = S + ((size_t)B * core + q) * ld + (size_t)B * a + i;
        *s = sp_pull_rhs<B, NR>(v, ra0, ra1, Lb, ysp, q, i, *s);
    }
}

// the core's solution (the right-hand-side rows of S) into X [NR][ldx], which is in the separators' own order
template <int B, int NR>
__global__ __launch_bounds__(kThreads) void k_pgo_sp_expand(SpView v, int core, const double* __restrict__ xr, size_t ld, double* __restrict__ X,
                                                            size_t ldx)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= core * B * NR) return;
    const int a = t / (B * NR), q = (t / B) % NR, i = t % B;
    X[q * ldx + (size_t)B * v.order[v.n_elim + a] + i] = xr[q * ld + (size_t)B * a + i];
}

// one launch per level, the levels in reverse, a workgroup per column: x_k = L_k^-T (y_k - sum_s W_k[s]^T x_r).  The sum over the d blocks
// is dealt to kThreads / BV chunks whose partial sums are added in their order.
template <int B, int NR>
__global__ __launch_bounds__(kThreads) void k_pgo_sp_back(SpView v, int k0, const double* __restrict__ Lb, const double* __restrict__ ysp,
                                                          double* __restrict__ X, size_t ldx)
{
    constexpr int BB = B * B, BV = B * NR, kChunks = kThreads / BV;
    __shared__ double part[kChunks][BV];
    const int k = k0 + blockIdx.x, tid = threadIdx.x, c0 = v.col_ptr[k], d = v.col_ptr[k + 1] - c0;
    const double* col = Lb + (size_t)(c0 + k) * BB;
    const int e = tid % BV, ch = tid / BV, q = e / B, i = e % B;
    if (ch < kChunks) {
        double s = 0.0;
        for (int t = ch; t < d; t += kChunks) {
            const double *W = col + BB + (size_t)t * BB, *x = X + q * ldx + (size_t)B * v.order[v.col_struct[c0 + t]];
#pragma unroll
            for (int c = 0; c < B; ++c) s += W[c * B + i] * x[c];
        }
        part[ch][e] = s;
    }
    __syncthreads();
    if (tid < NR) {
        double x[B], L[BB];
#pragma unroll
        for (int r = 0; r < BB; ++r) L[r] = col[r];
#pragma unroll
        for (int r = 0; r < B; ++r) {
            double t = ysp[(size_t)k * BV + tid * B + r];
            for (int c = 0; c < kChunks; ++c) t -= part[c][tid * B + r];
            x[r] = t;
        }
        upper_solve<B>(L, x);
#pragma unroll
        for (int r = 0; r < B; ++r) X[tid * ldx + (size_t)B * v.order[k] + r] = x[r];
    }
}

// ------------------------------------------------------------------ per pose

__global__ __launch_bounds__(kThreads) void k_pgo_retract(double* __restrict__ T, const double* __restrict__ delta, int N, Status* st)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= N) return;
    double t[12], d[6], m = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = T[(size_t)p * 12 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        d[k] = delta[(size_t)p * 6 + k];
        const double a = fabs(d[k]);
        m = (a > m || a != a) ? a : m;                            // a NaN stays: its bits are above every finite value's
    }
    mrs::pgo::retract(t, d, t);
#pragma unroll
    for (int k = 0; k < 12; ++k) T[(size_t)p * 12 + k] = t[k];
    atomicMax(&st->max_delta, (u64)__double_as_longlong(m));      // m >= 0 or NaN with a clear sign: the order of the bits is the order of the values
}

// stage 1: T [p] = [closest rotation of the solved 3x3 | 0]
__global__ __launch_bounds__(kThreads) void k_pgo_project(const double* __restrict__ X, int N, double* __restrict__ T)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= N) return;
    double x[9], R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = X[(size_t)p * 9 + k];
    mrs::pgo::closest_rotation(x, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        T[(size_t)p * 12 + 4 * r] = R[3 * r];
        T[(size_t)p * 12 + 4 * r + 1] = R[3 * r + 1];
        T[(size_t)p * 12 + 4 * r + 2] = R[3 * r + 2];
        T[(size_t)p * 12 + 4 * r + 3] = 0.0;
    }
}

// ------------------------------------------------------------------ the error sum: a fixed two-level tree

__device__ __forceinline__ double block_tree_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(kThreads) void k_pgo_sum1(const double* __restrict__ v, int n, double* __restrict__ partial)
{
    __shared__ double sh[kThreads];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const double s = block_tree_sum(i < n ? v[i] : 0.0, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void k_pgo_sum2(const double* __restrict__ partial, int n, double* __restrict__ out)
{
    __shared__ double sh[kThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) s += partial[i];
    s = block_tree_sum(s, sh);
    if (threadIdx.x == 0) *out = s;
}

// ------------------------------------------------------------------ host: the topology of one stage

struct Topology {
    int n_nodes = 0, E = 0;
    std::vector<int> sep_node;                                   // [E] ascending; the anchor, where there is one, is last
    std::vector<int> seg_first, seg_len, seg_chain, seg_left, seg_right;
    std::vector<int> tgt_a, tgt_b, tgt_ptr, contrib;             // the first E blocks are the diagonal ones
};

struct Graph {
    int nr = 0, N = 0;
    std::vector<int> start;                                      // [nr + 1]
    std::vector<int> li, lj;                                     // the loops
    std::vector<int> marks;                                      // poses stage 2 treats as separators anyway (mrs_pgo_mark_poses), ascending
};

// is_sep [N] for the loops given: the touched poses (pose 0 too), in stage 2 the marked poses, and the cuts.  Pose 0 ends a run in both
// stages, so without marks both have the same cuts.
void mark_separators(const Graph& g, int seglen, int stage, std::vector<char>* is_sep)
{
    is_sep->assign(g.N, 0);
    for (size_t u = 0; u < g.li.size(); ++u) (*is_sep)[g.li[u]] = (*is_sep)[g.lj[u]] = 1;
    if (stage == 2)
        for (int p : g.marks) (*is_sep)[p] = 1;
    (*is_sep)[0] = 1;
    for (int c = 0; c < g.nr; ++c) {
        int run = 0;
        for (int p = g.start[c]; p < g.start[c + 1]; ++p) {
            if ((*is_sep)[p]) {
                run = 0;
            } else if (seglen > 0 && run == seglen) {
                (*is_sep)[p] = 1;
                run = 0;
            } else {
                ++run;
            }
        }
    }
}

// the separators of stage 2: pose 0 is held and does not count
int count_separators(const Graph& g, int seglen)
{
    std::vector<char> is_sep;
    mark_separators(g, seglen, 2, &is_sep);
    return (int)std::count(is_sep.begin(), is_sep.end(), 1) - 1;
}

// stage 1: the nodes are the poses and the anchor (node N), factor F is anchor -> pose 0; stage 2: pose 0 is held and drops out
void build_topology(const Graph& g, int seglen, int stage, Topology* t)
{
    const int N = g.N, F = N - g.nr + (int)g.li.size();
    std::vector<char> is_sep;
    mark_separators(g, seglen, stage, &is_sep);
    const bool rot = stage == 1;
    *t = Topology();
    t->n_nodes = rot ? N + 1 : N;
    std::vector<int> sep_of(N + 1, -1);
    for (int p = rot ? 0 : 1; p < N; ++p)
        if (is_sep[p]) {
            sep_of[p] = (int)t->sep_node.size();
            t->sep_node.push_back(p);
        }
    if (rot) {
        sep_of[N] = (int)t->sep_node.size();
        t->sep_node.push_back(N);
    }
    const int E = t->E = (int)t->sep_node.size();
    for (int c = 0; c < g.nr; ++c) {
        int p = g.start[c];
        const int end = g.start[c + 1];
        while (p < end) {
            if (is_sep[p]) {
                ++p;
                continue;
            }
            int q = p;
            while (q < end && !is_sep[q]) ++q;
            t->seg_first.push_back(p);
            t->seg_len.push_back(q - p);
            t->seg_chain.push_back(c);
            t->seg_left.push_back(p > g.start[c] ? sep_of[p - 1] : -1);       // -1 too when the pose before is the held pose 0
            t->seg_right.push_back(q < end ? sep_of[q] : -1);
            p = q;
        }
    }
    std::vector<std::vector<int>> diag(E);
    std::map<std::pair<int, int>, std::vector<int>> off;
    for (int a = 0; a < E; ++a) diag[a].push_back(kNodeDiag << kTypeShift | t->sep_node[a]);
    const auto factor = [&](int f, int i, int j) {
        const int a = sep_of[i], b = sep_of[j];
        if (a < 0 || b < 0) return;
        if (a > b) off[{a, b}].push_back(kFactor << kTypeShift | f);
        else off[{b, a}].push_back(kFactorT << kTypeShift | f);
    };
    for (int c = 0; c < g.nr; ++c)
        for (int p = g.start[c]; p + 1 < g.start[c + 1]; ++p) factor(p - c, p, p + 1);
    for (size_t u = 0; u < g.li.size(); ++u) factor(N - g.nr + (int)u, g.li[u], g.lj[u]);
    if (rot) factor(F, N, 0);
    for (size_t s = 0; s < t->seg_first.size(); ++s) {
        const int l = t->seg_left[s], r = t->seg_right[s];
        if (l >= 0) diag[l].push_back(kSegLL << kTypeShift | (int)s);
        if (r >= 0) diag[r].push_back(kSegRR << kTypeShift | (int)s);
        if (l >= 0 && r >= 0) {
            if (r > l) off[{r, l}].push_back(kSegRL << kTypeShift | (int)s);
            else off[{l, r}].push_back(kSegRLT << kTypeShift | (int)s);
        }
    }
    t->tgt_ptr.push_back(0);
    for (int a = 0; a < E; ++a) {
        t->tgt_a.push_back(a);
        t->tgt_b.push_back(a);
        t->contrib.insert(t->contrib.end(), diag[a].begin(), diag[a].end());
        t->tgt_ptr.push_back((int)t->contrib.size());
    }
    for (const auto& kv : off) {
        t->tgt_a.push_back(kv.first.first);
        t->tgt_b.push_back(kv.first.second);
        t->contrib.insert(t->contrib.end(), kv.second.begin(), kv.second.end());
        t->tgt_ptr.push_back((int)t->contrib.size());
    }
}

// the symbolic phase of a stage's sparse tier (posegraph_order.hpp); a pattern past the block budget is MRS_ERR_UNSUPPORTED
int pgo_sparse_order(const Topology& t, int stage, int dense_limit, int max_blocks, mrs::pgo::SparseOrder* o)
{
    long long count = 0;
    if (!mrs::pgo::sparse_order(t.E, (int)t.tgt_a.size(), t.tgt_a.data(), t.tgt_b.data(), dense_limit, MRS_PGO_SPARSE_DEGREE_SLACK, max_blocks, o,
                                &count)) {
        mrs::set_error("stage %d: eliminating %d separators down to %d reached %lld blocks, past the budget of %d", stage, t.E, dense_limit, count,
                       max_blocks);
        return MRS_ERR_UNSUPPORTED;
    }
    return MRS_OK;
}

// one stage's topology on the device: a single int buffer
struct DeviceTopology {
    mrs::DeviceBuffer<int> ints;
    int E = 0, n_tgt = 0;
    SegView sv = {};
    const int *sep_node = nullptr, *tgt_a = nullptr, *tgt_b = nullptr, *tgt_ptr = nullptr, *contrib = nullptr;

    int upload(const Topology& t)
    {
        std::vector<int> h;
        const auto put = [&](const std::vector<int>& v) {
            const size_t at = h.size();
            h.insert(h.end(), v.begin(), v.end());
            return at;
        };
        const size_t o_sep = put(t.sep_node), o_f = put(t.seg_first), o_l = put(t.seg_len), o_c = put(t.seg_chain), o_sl = put(t.seg_left),
                     o_sr = put(t.seg_right), o_a = put(t.tgt_a), o_b = put(t.tgt_b), o_p = put(t.tgt_ptr), o_k = put(t.contrib);
        h.push_back(0);                                           // never empty
        MRS_TRY(ints.reserve(h.size(), h.size() + h.size() / 4));
        MRS_HIP_TRY(hipMemcpy(ints.get(), h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
        const int* d = ints.get();
        E = t.E;
        n_tgt = (int)t.tgt_a.size();
        sv = SegView{(int)t.seg_first.size(), d + o_f, d + o_l, d + o_c, d + o_sl, d + o_sr};
        sep_node = d + o_sep; tgt_a = d + o_a; tgt_b = d + o_b; tgt_ptr = d + o_p; contrib = d + o_k;
        return MRS_OK;
    }
};

// one stage's sparse tier on the device: the pattern (a single int buffer) and the core's own assembly lists
struct DeviceSparse {
    mrs::DeviceBuffer<int> ints;
    SpView v = {};
    int core = 0, n_core_tgt = 0;
    const int *core_a = nullptr, *core_b = nullptr, *core_ptr = nullptr, *core_contrib = nullptr;

    int upload(const mrs::pgo::SparseOrder& o, const Topology& t)
    {
        std::vector<int> h, row_blk(o.row_k.size()), ca, cb, cp(1, 0), cc;
        for (size_t u = 0; u < o.row_k.size(); ++u) row_blk[u] = o.col_ptr[o.row_k[u]] + o.row_k[u] + 1 + o.row_slot[u];
        std::vector<int> pos(o.E);
        for (int p = 0; p < o.E; ++p) pos[o.order[p]] = p;
        for (int tgt : o.core_tgt) {                             // the core's blocks in the core's numbering, their lists as they were
            ca.push_back(pos[t.tgt_a[tgt]] - o.eliminated);
            cb.push_back(pos[t.tgt_b[tgt]] - o.eliminated);
            cc.insert(cc.end(), t.contrib.begin() + t.tgt_ptr[tgt], t.contrib.begin() + t.tgt_ptr[tgt + 1]);
            cp.push_back((int)cc.size());
        }
        const auto put = [&](const std::vector<int>& x) {
            const size_t at = h.size();
            h.insert(h.end(), x.begin(), x.end());
            return at;
        };
        const size_t o_ord = put(o.order), o_cp = put(o.col_ptr), o_cs = put(o.col_struct), o_ct = put(o.col_tgt), o_rp = put(o.row_ptr),
                     o_rk = put(o.row_k), o_rb = put(row_blk), o_a = put(ca), o_b = put(cb), o_p = put(cp), o_c = put(cc);
        h.push_back(0);                                           // never empty
        MRS_TRY(ints.reserve(h.size(), h.size() + h.size() / 4));
        MRS_HIP_TRY(hipMemcpy(ints.get(), h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
        const int* d = ints.get();
        v = SpView{d + o_ord, d + o_cp, d + o_cs, d + o_ct, d + o_rp, d + o_rk, d + o_rb, o.eliminated};
        core = o.core;
        n_core_tgt = (int)ca.size();
        core_a = d + o_a; core_b = d + o_b; core_ptr = d + o_p; core_contrib = d + o_c;
        return MRS_OK;
    }
};

bool finite16(const double* m)
{
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(m[k])) return false;
    return true;
}

}  // namespace

struct mrs_pgo {
    mrs_ctx* ctx = nullptr;
    Graph g;
    int seglen = MRS_PGO_DEFAULT_SEGMENT_LENGTH;
    int solver = MRS_PGO_SOLVER_DENSE, dense_limit = MRS_PGO_MAX_SEPARATORS, max_blocks = MRS_PGO_MAX_SPARSE_BLOCKS;
    bool odometry_set = false;
    std::vector<double> odom, loopZ;                             // [.][16] as given
    std::vector<double> odomC, loopC;                            // covariances [.][36]: odomC is empty or complete, loopC has an entry per loop
    std::vector<char> loop_has_C;                                // whether loopC's entry was given
    int kernel = MRS_PGO_KERNEL_NONE;                            // on the loop factors, under mrs_pgo_optimize_lm
    double kernel_k = 1.0;
    bool result_valid = false, result_weighted = false;          // the device holds the loops' state at the last result, and where
    double prior[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    bool dirty = true;                                           // the device copy of the graph and of the topologies is behind
    bool init_valid = false;                                     // T0 holds stage 1 of the current graph
    Topology topo[2];                                            // stage 1, stage 2
    DeviceTopology dtopo[2];
    mrs::pgo::SparseOrder sp[2];                                 // the sparse tier of each stage; nothing eliminated under the dense solver
    DeviceSparse dsp[2];
    mrs::DeviceBuffer<double> Lb, ysp, X;                        // the sparse columns' blocks, their y, the separators' solution [NR][B E]
    int F = 0;                                                   // factors without the anchor's
    mrs::DeviceBuffer<int> fints;                                // fi [F + 1] | fj [F + 1] | csr ptr [N + 2] | csr entries [2 (F + 1)]
    mrs::DeviceBuffer<double> Z, T0, T, delta, Hii, Hij, gi, gj, err, partial, Hpp, gp, Lk, Ak, Wk, yk, seg, S;
    mrs::DeviceBuffer<double> noise, lam, eff, r2, wk;           // per factor: see Weights
    mrs::DeviceBuffer<double> Tprev, diag, predv, partial_p;     // Levenberg-Marquardt: the poses before the step, diag(H), the terms of pred
    mrs::DeviceBuffer<Status> status;
    mrs::DeviceBuffer<double> err_out;
    float stage_ms[6] = {0, 0, 0, 0, 0, 0};
    float tier_ms[2] = {0, 0};                                   // of stage 2's sparse tier: its way down with the core's update, its way back
    // marginal covariances of the last result (mrs_pgo_compute_marginals): in force while marg_valid && result_valid && !dirty
    bool marg_valid = false;
    mrs::DeviceBuffer<double> Sig, Spp, Spn;                     // the reduced system's inverse [6 E][6 E]; per pose S_pp and S_{p, p + 1}
    mrs::DeviceBuffer<int> sep_of, query;                        // per pose its reduced index or -1; the poses of a query
    mrs::DeviceBuffer<double> cov;                               // a query's blocks
    std::vector<int> h_sep_of;
    float marg_ms[4] = {0, 0, 0, 0};

    // what the marginals hold is dropped with the result they belong to
    void drop_marginals()
    {
        marg_valid = false;
        Sig.reset();
        Spp.reset();
        Spn.reset();
    }
};

namespace {

int pgo_chain_of(const Graph& g, int p) { return (int)(std::upper_bound(g.start.begin(), g.start.end(), p) - g.start.begin()) - 1; }

bool pgo_connected(const Graph& g)
{
    std::vector<int> root(g.nr);
    for (int c = 0; c < g.nr; ++c) root[c] = c;
    const auto find = [&](int c) {
        while (root[c] != c) c = root[c] = root[root[c]];
        return c;
    };
    for (size_t u = 0; u < g.li.size(); ++u) {
        const int a = find(pgo_chain_of(g, g.li[u])), b = find(pgo_chain_of(g, g.lj[u]));
        if (a != b) root[std::max(a, b)] = std::min(a, b);
    }
    for (int c = 0; c < g.nr; ++c)
        if (find(c) != 0) return false;
    return true;
}

// the graph, both topologies and the workspace they need, on the device
int pgo_sync(mrs_pgo* h)
{
    if (!h->dirty) return MRS_OK;
    const Graph& g = h->g;
    const int N = g.N, L = (int)g.li.size(), F = N - g.nr + L, F1 = F + 1;
    h->F = F;
    h->init_valid = false;
    h->drop_marginals();
    build_topology(g, h->seglen, 1, &h->topo[0]);
    build_topology(g, h->seglen, 2, &h->topo[1]);
    MRS_TRY(h->dtopo[0].upload(h->topo[0]));
    MRS_TRY(h->dtopo[1].upload(h->topo[1]));
    for (int s = 0; s < 2; ++s) {
        h->sp[s] = mrs::pgo::SparseOrder();
        if (h->solver == MRS_PGO_SOLVER_SPARSE && h->topo[s].E > h->dense_limit) {
            MRS_TRY(pgo_sparse_order(h->topo[s], s + 1, h->dense_limit, h->max_blocks, &h->sp[s]));
            MRS_TRY(h->dsp[s].upload(h->sp[s], h->topo[s]));
        }
    }
    // factors and the CSR of factors per node, ascending (the anchor's factor F is the last of pose 0 and the only one of node N)
    std::vector<int> ints((size_t)2 * F1 + (N + 2) + 2 * (size_t)F1);
    int *fi = ints.data(), *fj = fi + F1, *ptr = fj + F1, *ent = ptr + N + 2;
    std::vector<double> Z((size_t)F1 * 12);
    int f = 0;
    for (int c = 0; c < g.nr; ++c)
        for (int p = g.start[c]; p + 1 < g.start[c + 1]; ++p, ++f) {
            fi[f] = p;
            fj[f] = p + 1;
            std::copy(h->odom.begin() + (size_t)f * 16, h->odom.begin() + (size_t)f * 16 + 12, Z.begin() + (size_t)f * 12);
        }
    for (int u = 0; u < L; ++u, ++f) {
        fi[f] = g.li[u];
        fj[f] = g.lj[u];
        std::copy(h->loopZ.begin() + (size_t)u * 16, h->loopZ.begin() + (size_t)u * 16 + 12, Z.begin() + (size_t)f * 12);
    }
    fi[F] = N;
    fj[F] = 0;
    std::copy(h->prior, h->prior + 12, Z.begin() + (size_t)F * 12);
    std::vector<int> deg(N + 2, 0);
    for (int k = 0; k < F1; ++k) {
        ++deg[fi[k] + 1];
        ++deg[fj[k] + 1];
    }
    ptr[0] = 0;
    for (int p = 0; p <= N; ++p) ptr[p + 1] = ptr[p] + deg[p + 1];
    std::vector<int> fill(ptr, ptr + N + 1);
    for (int k = 0; k < F1; ++k) {
        ent[fill[fi[k]]++] = k << 1;
        ent[fill[fj[k]]++] = k << 1 | 1;
    }
    MRS_TRY(h->fints.reserve(ints.size(), ints.size() + ints.size() / 4));
    MRS_HIP_TRY(hipMemcpy(h->fints.get(), ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
    const auto grow = [](mrs::DeviceBuffer<double>& b, size_t need) { return b.reserve(std::max<size_t>(need, 1), std::max<size_t>(need + need / 4, 16)); };
    MRS_TRY(grow(h->Z, Z.size()));
    MRS_HIP_TRY(hipMemcpy(h->Z.get(), Z.data(), Z.size() * sizeof(double), hipMemcpyHostToDevice));
    const size_t nodes = (size_t)N + 1, nseg = std::max(h->topo[0].seg_first.size(), h->topo[1].seg_first.size());
    const auto dense_order = [&](int s) { return (size_t)(h->sp[s].eliminated ? h->sp[s].core : h->topo[s].E); };
    const size_t n1 = 3 * dense_order(0), n2 = 6 * dense_order(1);
    MRS_TRY(grow(h->Lb, std::max((size_t)h->sp[0].blocks * 9, (size_t)h->sp[1].blocks * 36)));
    MRS_TRY(grow(h->ysp, std::max((size_t)h->sp[0].eliminated * 9, (size_t)h->sp[1].eliminated * 6)));
    MRS_TRY(grow(h->X, std::max(9 * (size_t)h->topo[0].E, 6 * (size_t)h->topo[1].E)));
    MRS_TRY(grow(h->T0, nodes * 12));
    MRS_TRY(grow(h->T, nodes * 12));
    MRS_TRY(grow(h->delta, nodes * 9));
    MRS_TRY(grow(h->Hii, (size_t)F1 * 36));
    MRS_TRY(grow(h->Hij, (size_t)F1 * 36));
    MRS_TRY(grow(h->gi, (size_t)F1 * 6));
    MRS_TRY(grow(h->gj, (size_t)F1 * 6));
    MRS_TRY(grow(h->err, (size_t)F1));
    MRS_TRY(grow(h->partial, (size_t)blocks_for(F1, kThreads)));
    MRS_TRY(grow(h->Hpp, nodes * 36));
    MRS_TRY(grow(h->gp, nodes * 9));
    MRS_TRY(grow(h->Lk, nodes * 36));
    MRS_TRY(grow(h->Ak, nodes * 36));
    MRS_TRY(grow(h->Wk, nodes * 36));
    MRS_TRY(grow(h->yk, nodes * 9));
    MRS_TRY(grow(h->seg, nseg * (3 * 36 + 2 * 9)));
    MRS_TRY(grow(h->S, std::max((n1 + 3) * n1, (n2 + 1) * n2)));
    // 1 / max(C00, C11, C22) and C[3:6, 3:6] + 0.01 I of the factors that carry a covariance; zeros for the others
    std::vector<double> noise((size_t)F1 * kInfo, 0.0);
    const auto put_noise = [&](int k, const double* C) { mrs::pgo::covariance_terms(C, noise.data() + (size_t)k * kInfo); };
    if (!h->odomC.empty())
        for (int k = 0; k < N - g.nr; ++k) put_noise(k, h->odomC.data() + (size_t)k * 36);
    for (int u = 0; u < L; ++u)
        if (h->loop_has_C[u]) put_noise(N - g.nr + u, h->loopC.data() + (size_t)u * 36);
    MRS_TRY(grow(h->noise, noise.size()));
    MRS_HIP_TRY(hipMemcpy(h->noise.get(), noise.data(), noise.size() * sizeof(double), hipMemcpyHostToDevice));
    MRS_TRY(grow(h->lam, (size_t)F1 * kInfo));
    MRS_TRY(grow(h->eff, (size_t)F1 * kInfo));
    MRS_TRY(grow(h->r2, (size_t)F1));
    MRS_TRY(grow(h->wk, (size_t)F1));
    MRS_TRY(grow(h->Tprev, nodes * 12));
    MRS_TRY(grow(h->diag, nodes * 6));
    MRS_TRY(grow(h->predv, nodes));
    MRS_TRY(grow(h->partial_p, (size_t)blocks_for((long long)nodes, kThreads)));
    MRS_TRY(h->status.reserve(2, 2));                            // the second slot holds the two doubles of a Levenberg-Marquardt solve
    MRS_TRY(h->err_out.reserve(1, 1));
    h->result_valid = false;
    h->dirty = false;
    return MRS_OK;
}

// the blocked Cholesky of the dense S [n + nr][ld] with the forward substitution of its nr right-hand-side rows, and the way back
void pgo_dense_solve(double* S, int n, int nr, size_t ld, Status* st)
{
    const int nt = n + nr;
    for (int k0 = 0; k0 < n; k0 += kNB) {
        const int nb = std::min(kNB, n - k0), k1 = k0 + nb;
        hipLaunchKernelGGL(k_pgo_chol_panel, dim3(1), dim3(kThreads), 0, nullptr, S, n, nt, ld, k0, st);
        if (k1 < n) {
            const unsigned tiles = blocks_for(nt - k1, kTile);
            hipLaunchKernelGGL(k_pgo_chol_trail, dim3(tiles, tiles), dim3(kThreads), 0, nullptr, S, n, nt, ld, k0, nb);
        }
    }
    hipLaunchKernelGGL(k_pgo_chol_back, dim3(1), dim3(kThreads), 0, nullptr, S, n, ld, nr);
}

// pgo_solve from the segments' Schur contributions on, with the stage's sparse tier: the sparse columns level after
// level, the core's dense system less what the columns send it, the columns' way back in reverse, then the separators' solution X in their
// own order for k_pgo_scatter and k_pgo_backsolve
template <int B, int NR>
int pgo_solve_sparse(mrs_pgo* h, int stage, mrs::StageMarks* marks, int base)
{
    constexpr int BB = B * B, BV = B * NR;
    const DeviceTopology& t = h->dtopo[stage - 1];
    const DeviceSparse& sp = h->dsp[stage - 1];
    const std::vector<int>& level = h->sp[stage - 1].level_ptr;
    const int E = t.E, core = sp.core, n = B * core, nt = n + NR;
    const size_t ld = (size_t)n, ldx = (size_t)B * E, nseg = (size_t)t.sv.n;
    double* seg = h->seg.get();
    double *Sll = seg, *Srr = Sll + nseg * BB, *Srl = Srr + nseg * BB, *gl = Srl + nseg * BB, *gr = gl + nseg * BV;
    double *S = h->S.get(), *Lb = h->Lb.get(), *ysp = h->ysp.get(), *X = h->X.get();
    Status* st = h->status.get();
    const Parts P = {h->Hpp.get(), h->gp.get(), h->Hij.get(), Sll, Srr, Srl, gl, gr};
    if (core) {
        MRS_HIP_TRY(hipMemsetAsync(S, 0, (size_t)nt * ld * sizeof(double), nullptr));
        hipLaunchKernelGGL((k_pgo_assemble<B>), dim3(blocks_for((long long)sp.n_core_tgt * BB, kThreads)), dim3(kThreads), 0, nullptr, sp.core_a,
                           sp.core_b, sp.core_ptr, sp.core_contrib, sp.n_core_tgt, P, S, ld);
        hipLaunchKernelGGL((k_pgo_assemble_rhs<B, NR>), dim3(blocks_for((long long)core * BV, kThreads)), dim3(kThreads), 0, nullptr, sp.core_ptr,
                           sp.core_contrib, core, P, S + (size_t)n * ld, ld);
    }
    if (marks) marks->mark(base + 1);
    for (size_t l = 0; l + 1 < level.size(); ++l)
        hipLaunchKernelGGL((k_pgo_sp_column<B, NR>), dim3(level[l + 1] - level[l]), dim3(kThreads), 0, nullptr, sp.v, level[l], t.tgt_ptr, t.contrib,
                           t.sep_node, P, Lb, ysp, st);
    if (core) {
        hipLaunchKernelGGL((k_pgo_sp_core<B, NR>), dim3(blocks_for((long long)core * BB + BV, kThreads), core), dim3(kThreads), 0, nullptr, sp.v, core,
                           Lb, ysp, S, ld);
        if (marks) marks->mark(kMarkTierDown);
        pgo_dense_solve(S, n, NR, ld, st);
        hipLaunchKernelGGL((k_pgo_sp_expand<B, NR>), dim3(blocks_for((long long)core * BV, kThreads)), dim3(kThreads), 0, nullptr, sp.v, core,
                           S + (size_t)n * ld, ld, X, ldx);
        if (marks) marks->mark(kMarkTierUp);
    } else if (marks) {
        marks->mark(kMarkTierDown);
        marks->mark(kMarkTierUp);
    }
    for (size_t l = level.size() - 1; l-- > 0;)
        hipLaunchKernelGGL((k_pgo_sp_back<B, NR>), dim3(level[l + 1] - level[l]), dim3(kThreads), 0, nullptr, sp.v, level[l], Lb, ysp, X, ldx);
    if (marks) marks->mark(base + 2);
    hipLaunchKernelGGL((k_pgo_scatter<B, NR>), dim3(blocks_for((long long)E * BV, kThreads)), dim3(kThreads), 0, nullptr, t.sep_node, E, X, ldx,
                       h->delta.get());
    if (nseg)
        hipLaunchKernelGGL((k_pgo_backsolve<B, NR>), dim3(blocks_for((long long)nseg, 64)), dim3(64), 0, nullptr, t.sv, h->Lk.get(), h->Ak.get(),
                           h->Wk.get(), h->yk.get(), X, ldx, h->delta.get());
    if (marks) marks->mark(base + 3);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

// One solve of the assembled per-node system (Hpp, gp, Hij) of a stage -> delta [n_nodes][NR][B]; entries of held nodes are zero.
// `marks` (optional) gets marks base .. base + 3: after the walk, the assembly, the dense solve and the way back.
template <int B, int NR>
int pgo_solve(mrs_pgo* h, int stage, mrs::StageMarks* marks, int base)
{
    constexpr int BB = B * B, BV = B * NR;
    const DeviceTopology& t = h->dtopo[stage - 1];
    const int nodes = h->topo[stage - 1].n_nodes, E = t.E, n = B * E, nt = n + NR;
    const size_t ld = (size_t)n, nseg = (size_t)t.sv.n;
    double* seg = h->seg.get();
    double *Sll = seg, *Srr = Sll + nseg * BB, *Srl = Srr + nseg * BB, *gl = Srl + nseg * BB, *gr = gl + nseg * BV;
    double* S = h->S.get();
    Status* st = h->status.get();
    MRS_HIP_TRY(hipMemsetAsync(h->delta.get(), 0, (size_t)nodes * BV * sizeof(double), nullptr));
    if (nseg)
        hipLaunchKernelGGL((k_pgo_eliminate<B, NR>), dim3(blocks_for((long long)nseg, 64)), dim3(64), 0, nullptr, t.sv, h->Hpp.get(), h->gp.get(),
                           h->Hij.get(), h->Lk.get(), h->Ak.get(), h->Wk.get(), h->yk.get(), Sll, Srr, Srl, gl, gr, st);
    if (marks) marks->mark(base);
    if (h->sp[stage - 1].eliminated) return pgo_solve_sparse<B, NR>(h, stage, marks, base);
    if (E) {
        const Parts P = {h->Hpp.get(), h->gp.get(), h->Hij.get(), Sll, Srr, Srl, gl, gr};
        MRS_HIP_TRY(hipMemsetAsync(S, 0, (size_t)nt * ld * sizeof(double), nullptr));
        hipLaunchKernelGGL((k_pgo_assemble<B>), dim3(blocks_for((long long)t.n_tgt * BB, kThreads)), dim3(kThreads), 0, nullptr, t.tgt_a, t.tgt_b,
                           t.tgt_ptr, t.contrib, t.n_tgt, P, S, ld);
        hipLaunchKernelGGL((k_pgo_assemble_rhs<B, NR>), dim3(blocks_for((long long)E * BV, kThreads)), dim3(kThreads), 0, nullptr, t.tgt_ptr, t.contrib,
                           E, P, S + (size_t)n * ld, ld);
        if (marks) marks->mark(base + 1);
        pgo_dense_solve(S, n, NR, ld, st);
        if (marks) marks->mark(base + 2);
        hipLaunchKernelGGL((k_pgo_scatter<B, NR>), dim3(blocks_for((long long)E * BV, kThreads)), dim3(kThreads), 0, nullptr, t.sep_node, E,
                           S + (size_t)n * ld, ld, h->delta.get());
    } else if (marks) {
        marks->mark(base + 1);
        marks->mark(base + 2);
    }
    if (nseg)
        hipLaunchKernelGGL((k_pgo_backsolve<B, NR>), dim3(blocks_for((long long)nseg, 64)), dim3(64), 0, nullptr, t.sv, h->Lk.get(), h->Ak.get(),
                           h->Wk.get(), h->yk.get(), S + (size_t)n * ld, ld, h->delta.get());
    if (marks) marks->mark(base + 3);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

// the status words of the solves since the last reset -> MRS_OK, or MRS_ERR_NOT_CONVERGED with the pose named
int pgo_check_pivots(const mrs_pgo* h, const Status& st, int stage)
{
    if (st.seg_fail) {                                           // a segment walk's pose, or a separator of the sparse tier
        if (stage == 1 && kBig - st.seg_fail == h->g.N) mrs::set_error("stage 1: the pivot block of the anchor is not positive definite");
        else mrs::set_error("stage %d: the pivot block of pose %d is not positive definite", stage, kBig - st.seg_fail);
        return MRS_ERR_NOT_CONVERGED;
    }
    if (st.dense_fail) {
        const Topology& t = h->topo[stage - 1];
        const mrs::pgo::SparseOrder& sp = h->sp[stage - 1];
        const int row = kBig - st.dense_fail, c = row / (stage == 1 ? 3 : 6), a = sp.eliminated && c < sp.core ? sp.order[sp.eliminated + c] : c;
        const int pose = a >= 0 && a < t.E ? t.sep_node[a] : -1;
        if (stage == 1 && pose == h->g.N) mrs::set_error("stage 1: the pivot block of the anchor is not positive definite (row %d)", row);
        else mrs::set_error("stage %d: the pivot block of pose %d is not positive definite (row %d of the reduced system)", stage, pose, row);
        return MRS_ERR_NOT_CONVERGED;
    }
    return MRS_OK;
}

int pgo_ready(mrs_pgo* h)
{
    MRS_REQUIRE(h->odometry_set || h->g.N == h->g.nr, "set the odometry first");
    if (!pgo_connected(h->g)) {
        mrs::set_error("bad argument: a chain is not connected to chain 0 through loop factors");
        return MRS_ERR_ARG;
    }
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    return pgo_sync(h);
}

// stage 1 into T0, unless it is there already
int pgo_stage1(mrs_pgo* h)
{
    if (h->init_valid) return MRS_OK;
    const int N = h->g.N, F1 = h->F + 1;
    const int* ptr = h->fints.get() + 2 * (size_t)F1;
    MRS_HIP_TRY(hipMemsetAsync(h->status.get(), 0, sizeof(Status), nullptr));
    hipLaunchKernelGGL(k_pgo_linearize_rot, dim3(blocks_for(F1, kThreads)), dim3(kThreads), 0, nullptr, h->Z.get(), F1, h->Hij.get());
    hipLaunchKernelGGL(k_pgo_gather_rot, dim3(blocks_for(N + 1, kThreads)), dim3(kThreads), 0, nullptr, ptr, N, h->Hpp.get(), h->gp.get());
    MRS_TRY((pgo_solve<3, 3>(h, 1, nullptr, 0)));
    hipLaunchKernelGGL(k_pgo_project, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, nullptr, h->delta.get(), N, h->T0.get());
    MRS_HIP_TRY(hipGetLastError());
    Status st;
    MRS_HIP_TRY(hipMemcpy(&st, h->status.get(), sizeof(st), hipMemcpyDeviceToHost));
    MRS_TRY(pgo_check_pivots(h, st, 1));
    h->init_valid = true;
    return MRS_OK;
}

// the fixed two-level tree over v [n] -> *d_out on the device
void pgo_tree_sum(const double* v, int n, double* partial, double* d_out)
{
    const int nb = (int)blocks_for(n, kThreads);
    hipLaunchKernelGGL(k_pgo_sum1, dim3(nb), dim3(kThreads), 0, nullptr, v, n, partial);
    hipLaunchKernelGGL(k_pgo_sum2, dim3(1), dim3(kThreads), 0, nullptr, partial, nb, d_out);
}

int pgo_error_sum(mrs_pgo* h, double* out)
{
    const int F = h->F;
    *out = 0.0;
    if (F == 0) return MRS_OK;
    pgo_tree_sum(h->err.get(), F, h->partial.get(), h->err_out.get());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpy(out, h->err_out.get(), sizeof(double), hipMemcpyDeviceToHost));
    return MRS_OK;
}

// ------------------------------------------------------------------ host: the weighted and the plain instantiations behind one call each

int pgo_check_size(const mrs_pgo* h, const Graph& g, int seglen);

bool pgo_has_noise(const mrs_pgo* h)
{
    return !h->odomC.empty() || std::find(h->loop_has_C.begin(), h->loop_has_C.end(), (char)1) != h->loop_has_C.end();
}

struct FactorPass {
    mrs_pgo* h;
    bool weighted;
    int kernel;                                                  // applies to the weighted instantiation only
    const int *fi, *fj, *ptr, *ent;

    FactorPass(mrs_pgo* handle, bool w, int kern) : h(handle), weighted(w), kernel(kern)
    {
        const int F1 = h->F + 1;
        fi = h->fints.get();
        fj = fi + F1;
        ptr = fj + F1;
        ent = ptr + h->g.N + 2;
    }
    Weights weights(bool irls) const
    {
        return Weights{h->lam.get(), h->eff.get(), h->r2.get(), h->wk.get(), h->g.N - h->g.nr, kernel, irls ? 1 : 0, h->kernel_k};
    }
    // the factors' information from the stage-1 values in T0
    void information() const
    {
        if (weighted && h->F)
            hipLaunchKernelGGL(k_pgo_information, dim3(blocks_for(h->F, kThreads)), dim3(kThreads), 0, nullptr, h->T0.get(), fi, h->noise.get(), h->F,
                               h->lam.get());
    }
    void linearize(const double* T, bool irls) const
    {
        const int F = h->F;
        if (!F) return;
        if (weighted)
            hipLaunchKernelGGL(k_pgo_linearize<true>, dim3(blocks_for(F, kThreads)), dim3(kThreads), 0, nullptr, T, fi, fj, h->Z.get(), F, h->Hii.get(),
                               h->Hij.get(), h->gi.get(), h->gj.get(), h->err.get(), weights(irls));
        else
            hipLaunchKernelGGL(k_pgo_linearize<false>, dim3(blocks_for(F, kThreads)), dim3(kThreads), 0, nullptr, T, fi, fj, h->Z.get(), F, h->Hii.get(),
                               h->Hij.get(), h->gi.get(), h->gj.get(), h->err.get(), Weights{});
    }
    void error(const double* T) const
    {
        const int F = h->F;
        if (!F) return;
        if (weighted)
            hipLaunchKernelGGL(k_pgo_error<true>, dim3(blocks_for(F, kThreads)), dim3(kThreads), 0, nullptr, T, fi, fj, h->Z.get(), F, h->err.get(),
                               weights(true));
        else
            hipLaunchKernelGGL(k_pgo_error<false>, dim3(blocks_for(F, kThreads)), dim3(kThreads), 0, nullptr, T, fi, fj, h->Z.get(), F, h->err.get(),
                               Weights{});
    }
    // lambda enters only with `damped`
    void gather(double lambda, bool damped) const
    {
        const int N = h->g.N;
        double* diag = damped ? h->diag.get() : nullptr;
        if (weighted)
            hipLaunchKernelGGL(k_pgo_gather<true>, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, nullptr, ptr, ent, N, h->F, h->Hii.get(),
                               h->gi.get(), h->gj.get(), h->Hpp.get(), h->gp.get(), h->eff.get(), lambda, diag);
        else
            hipLaunchKernelGGL(k_pgo_gather<false>, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, nullptr, ptr, ent, N, h->F, h->Hii.get(),
                               h->gi.get(), h->gj.get(), h->Hpp.get(), h->gp.get(), nullptr, lambda, diag);
    }
};

// a covariance as mrs_pgo_set_odometry_noise and mrs_pgo_add_loops_noise take it
bool pgo_covariance_ok(const double* C, const char** why)
{
    for (int k = 0; k < 36; ++k)
        if (!std::isfinite(C[k])) {
            *why = "a covariance is not finite";
            return false;
        }
    if (!(std::max(C[0], std::max(C[7], C[14])) > 0.0)) {
        *why = "a covariance has no positive rotation variance";
        return false;
    }
    double P[9];                                                 // the lower triangle of C[3:6, 3:6] + 0.01 I, factored in place
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) P[3 * r + c] = C[6 * (3 + r) + 3 + c] + (r == c ? mrs::pgo::kTranslationFloor : 0.0);
    for (int j = 0; j < 3; ++j) {
        double d = P[3 * j + j];
        for (int k = 0; k < j; ++k) d -= P[3 * j + k] * P[3 * j + k];
        if (!(d > 0.0) || !std::isfinite(d)) {
            *why = "a translation covariance plus 0.01 I is not positive definite";
            return false;
        }
        d = std::sqrt(d);
        P[3 * j + j] = d;
        for (int i = j + 1; i < 3; ++i) {
            double s = P[3 * i + j];
            for (int k = 0; k < j; ++k) s -= P[3 * i + k] * P[3 * j + k];
            P[3 * i + j] = s / d;
        }
    }
    return true;
}

// the loops' validation and append shared by mrs_pgo_add_loops and mrs_pgo_add_loops_noise (h_C may be null)
int pgo_add_loops(mrs_pgo* pgo, const int32_t* h_i, const int32_t* h_j, const double* h_Z, const double* h_C, int32_t n)
{
    for (int u = 0; u < n; ++u) {
        MRS_REQUIRE(h_i[u] >= 0 && h_i[u] < pgo->g.N && h_j[u] >= 0 && h_j[u] < pgo->g.N, "a loop names a pose outside the graph");
        MRS_REQUIRE(h_i[u] != h_j[u], "a loop joins a pose with itself");
        MRS_REQUIRE(finite16(h_Z + (size_t)u * 16), "a loop pose is not finite");
        const char* why = "";
        if (h_C && !pgo_covariance_ok(h_C + (size_t)u * 36, &why)) {
            mrs::set_error("bad argument: %s (loop %d of the call)", why, u);
            return MRS_ERR_ARG;
        }
    }
    if ((long long)pgo->g.li.size() + n > kMaxLoops) {
        mrs::set_error("%zu loops held and %d more exceed the %d a pose graph holds", pgo->g.li.size(), n, kMaxLoops);
        return MRS_ERR_UNSUPPORTED;
    }
    Graph g = pgo->g;
    g.li.insert(g.li.end(), h_i, h_i + n);
    g.lj.insert(g.lj.end(), h_j, h_j + n);
    MRS_TRY(pgo_check_size(pgo, g, pgo->seglen));
    pgo->g = std::move(g);
    pgo->loopZ.insert(pgo->loopZ.end(), h_Z, h_Z + (size_t)n * 16);
    if (h_C) pgo->loopC.insert(pgo->loopC.end(), h_C, h_C + (size_t)n * 36);
    else pgo->loopC.insert(pgo->loopC.end(), (size_t)n * 36, 0.0);
    pgo->loop_has_C.insert(pgo->loop_has_C.end(), (size_t)n, h_C ? 1 : 0);
    pgo->dirty = true;
    return MRS_OK;
}

// T [N][12] on the device -> h_T [N][16]
int pgo_download(const double* d_T, int N, double* h_T)
{
    std::vector<double> t((size_t)N * 12);
    MRS_HIP_TRY(hipMemcpy(t.data(), d_T, t.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < N; ++p) {
        std::copy(t.begin() + (size_t)p * 12, t.begin() + (size_t)p * 12 + 12, h_T + (size_t)p * 16);
        h_T[(size_t)p * 16 + 12] = h_T[(size_t)p * 16 + 13] = h_T[(size_t)p * 16 + 14] = 0.0;
        h_T[(size_t)p * 16 + 15] = 1.0;
    }
    return MRS_OK;
}

// validates on a copy: the handle changes only when everything holds
int pgo_check_size(int solver, int dense_limit, int max_blocks, const Graph& g, int seglen)
{
    if (solver == MRS_PGO_SOLVER_SPARSE) {                       // the block budget of both stages' sparse tiers
        for (int stage = 1; stage <= 2; ++stage) {
            Topology t;
            mrs::pgo::SparseOrder o;
            build_topology(g, seglen, stage, &t);
            MRS_TRY(pgo_sparse_order(t, stage, dense_limit, max_blocks, &o));
        }
        return MRS_OK;
    }
    const int E = count_separators(g, seglen);
    if (E > kMaxSep) {
        mrs::set_error("%d separators (poses touched by loops and cut poses) exceed the %d the reduced system holds", E, kMaxSep);
        return MRS_ERR_UNSUPPORTED;
    }
    return MRS_OK;
}

int pgo_check_size(const mrs_pgo* h, const Graph& g, int seglen) { return pgo_check_size(h->solver, h->dense_limit, h->max_blocks, g, seglen); }

// a query of the marginals: its poses to the device, k_pgo_marginal_gather, its blocks of `doubles` each back to the host
int pgo_marginal_query(mrs_pgo* h, const int32_t* h_i, const int32_t* h_j, int n, int frame, int doubles, double* h_cov)
{
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    const size_t nq = (size_t)n, ld = (size_t)6 * h->topo[1].E;
    MRS_TRY(h->query.reserve(2 * nq, 2 * nq + nq / 2));
    MRS_TRY(h->cov.reserve(nq * doubles, nq * doubles + nq * doubles / 4));
    int *qi = nullptr, *qj = nullptr;
    if (h_i) {
        qi = h->query.get();
        MRS_HIP_TRY(hipMemcpy(qi, h_i, nq * sizeof(int), hipMemcpyHostToDevice));
    }
    if (h_j) {
        qj = h->query.get() + nq;
        MRS_HIP_TRY(hipMemcpy(qj, h_j, nq * sizeof(int), hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_pgo_marginal_gather, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, nullptr, qi, qj, n, frame, h->T.get(),
                       h->sep_of.get(), h->Sig.get(), ld, h->Spp.get(), h->Spn.get(), h->cov.get());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpy(h_cov, h->cov.get(), nq * doubles * sizeof(double), hipMemcpyDeviceToHost));
    return MRS_OK;
}

}  // namespace

extern "C" {

int mrs_pgo_create(mrs_ctx* ctx, int32_t nr, const int32_t* h_chain_lengths, mrs_pgo** out)
{
    MRS_REQUIRE(ctx && out && h_chain_lengths, "null pointer");
    MRS_REQUIRE(nr >= 1 && nr <= kMaxChains, "1 .. MRS_PGO_MAX_CHAINS chains");
    long long total = 0;
    for (int c = 0; c < nr; ++c) {
        MRS_REQUIRE(h_chain_lengths[c] >= 1, "a chain has at least one pose");
        total += h_chain_lengths[c];
    }
    if (total > kMaxPoses) {
        mrs::set_error("%lld poses exceed the %d a pose graph holds", total, kMaxPoses);
        return MRS_ERR_UNSUPPORTED;
    }
    Graph g;
    g.nr = nr;
    g.N = (int)total;
    g.start.assign(1, 0);
    for (int c = 0; c < nr; ++c) g.start.push_back(g.start.back() + h_chain_lengths[c]);
    int seglen = MRS_PGO_DEFAULT_SEGMENT_LENGTH;
    while (count_separators(g, seglen) > kMaxSep) seglen *= 2;    // 65 536 poses at most: ends at 64 or 128
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    mrs_pgo* h = new mrs_pgo;
    h->ctx = ctx;
    h->g = g;
    h->seglen = seglen;
    *out = h;
    return MRS_OK;
}

int mrs_pgo_destroy(mrs_pgo* pgo)
{
    if (!pgo) return MRS_OK;
    (void)hipSetDevice(pgo->ctx->device);
    (void)hipStreamSynchronize(nullptr);
    delete pgo;
    return MRS_OK;
}

int mrs_pgo_set_odometry(mrs_pgo* pgo, const double* h_Z, int32_t n)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(n == pgo->g.N - pgo->g.nr, "one odometry factor per consecutive pair of a chain");
    MRS_REQUIRE(h_Z || n == 0, "null pointer");
    for (int k = 0; k < n; ++k) MRS_REQUIRE(finite16(h_Z + (size_t)k * 16), "an odometry pose is not finite");
    pgo->odom.assign(h_Z, h_Z + (size_t)n * 16);
    pgo->odometry_set = true;
    pgo->dirty = true;
    return MRS_OK;
}

int mrs_pgo_add_loops(mrs_pgo* pgo, const int32_t* h_i, const int32_t* h_j, const double* h_Z, int32_t n)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(n >= 0, "n must not be negative");
    if (n == 0) return MRS_OK;
    MRS_REQUIRE(h_i && h_j && h_Z, "null pointer");
    return pgo_add_loops(pgo, h_i, h_j, h_Z, nullptr, n);
}

int mrs_pgo_add_loops_noise(mrs_pgo* pgo, const int32_t* h_i, const int32_t* h_j, const double* h_Z, const double* h_C, int32_t n)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(n >= 0, "n must not be negative");
    if (n == 0) return MRS_OK;
    MRS_REQUIRE(h_i && h_j && h_Z && h_C, "null pointer");
    return pgo_add_loops(pgo, h_i, h_j, h_Z, h_C, n);
}

int mrs_pgo_set_odometry_noise(mrs_pgo* pgo, const double* h_C, int32_t n)
{
    MRS_REQUIRE(pgo, "null pointer");
    if (!h_C) {
        MRS_REQUIRE(n == 0, "null pointer");
        pgo->odomC.clear();
        pgo->dirty = true;
        return MRS_OK;
    }
    MRS_REQUIRE(n == pgo->g.N - pgo->g.nr, "one covariance per odometry factor");
    for (int k = 0; k < n; ++k) {
        const char* why = "";
        if (!pgo_covariance_ok(h_C + (size_t)k * 36, &why)) {
            mrs::set_error("bad argument: %s (odometry factor %d)", why, k);
            return MRS_ERR_ARG;
        }
    }
    pgo->odomC.assign(h_C, h_C + (size_t)n * 36);
    pgo->dirty = true;
    return MRS_OK;
}

int mrs_pgo_set_loop_kernel(mrs_pgo* pgo, int32_t kernel, double k)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(kernel >= MRS_PGO_KERNEL_NONE && kernel <= MRS_PGO_KERNEL_GEMAN_MCCLURE, "the kernel must be one of MRS_PGO_KERNEL_*");
    MRS_REQUIRE(k > 0.0 && std::isfinite(k), "the kernel's parameter must be positive and finite");
    pgo->kernel = kernel;
    pgo->kernel_k = k;
    pgo->result_valid = false;
    pgo->marg_valid = false;
    return MRS_OK;
}

int mrs_pgo_get_loop_state(mrs_pgo* pgo, double* h_w, double* h_r2, int32_t capacity)
{
    MRS_REQUIRE(pgo && h_w && h_r2, "null pointer");
    const int L = (int)pgo->g.li.size(), first = pgo->g.N - pgo->g.nr;
    MRS_REQUIRE(capacity >= L, "capacity is below the number of loops");
    MRS_REQUIRE(pgo->result_valid && !pgo->dirty, "no optimisation of the graph as it stands has finished");
    if (L == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(pgo->ctx->device));
    if (pgo->result_weighted) {
        MRS_HIP_TRY(hipMemcpy(h_w, pgo->wk.get() + first, (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
        MRS_HIP_TRY(hipMemcpy(h_r2, pgo->r2.get() + first, (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
    } else {                                                     // the plain pass leaves 0.5 |e|^2
        MRS_HIP_TRY(hipMemcpy(h_r2, pgo->err.get() + first, (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
        for (int u = 0; u < L; ++u) {
            h_r2[u] *= 2.0;
            h_w[u] = 1.0;
        }
    }
    return MRS_OK;
}

int mrs_pgo_clear_loops(mrs_pgo* pgo)
{
    MRS_REQUIRE(pgo, "null pointer");
    pgo->g.li.clear();
    pgo->g.lj.clear();
    pgo->loopZ.clear();
    pgo->loopC.clear();
    pgo->loop_has_C.clear();
    pgo->dirty = true;
    return MRS_OK;
}

int mrs_pgo_count(mrs_pgo* pgo, int32_t* h_count)
{
    MRS_REQUIRE(pgo && h_count, "null pointer");
    *h_count = (int32_t)pgo->g.li.size();
    return MRS_OK;
}

int mrs_pgo_set_prior(mrs_pgo* pgo, const double* h_T)
{
    MRS_REQUIRE(pgo && h_T, "null pointer");
    MRS_REQUIRE(finite16(h_T), "the prior is not finite");
    std::copy(h_T, h_T + 16, pgo->prior);
    pgo->dirty = true;
    return MRS_OK;
}

int mrs_pgo_set_segment_length(mrs_pgo* pgo, int32_t length)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(length >= 0, "the segment length must not be negative");
    if (length == pgo->seglen) return MRS_OK;
    MRS_TRY(pgo_check_size(pgo, pgo->g, length));
    pgo->seglen = length;
    pgo->dirty = true;
    return MRS_OK;
}

int mrs_pgo_initialize(mrs_pgo* pgo, double* h_T)
{
    MRS_REQUIRE(pgo && h_T, "null pointer");
    MRS_TRY(pgo_ready(pgo));
    MRS_TRY(pgo_stage1(pgo));
    return pgo_download(pgo->T0.get(), pgo->g.N, h_T);
}

int mrs_pgo_optimize(mrs_pgo* pgo, double eps, int32_t max_iterations, double* h_T, double* h_info)
{
    MRS_REQUIRE(pgo && h_T && h_info, "null pointer");
    MRS_REQUIRE(eps >= 0.0 && std::isfinite(eps), "eps must be finite and not negative");
    MRS_REQUIRE(max_iterations >= 1, "max_iterations must be positive");
    MRS_REQUIRE(pgo->kernel == MRS_PGO_KERNEL_NONE, "a robust kernel needs the step control of mrs_pgo_optimize_lm");
    MRS_TRY(pgo_ready(pgo));
    mrs_pgo* h = pgo;
    h->result_valid = false;
    h->drop_marginals();
    const bool timing = mrs::dev_env("MRS_PGO_TIMING") != nullptr;
    std::fill(h->stage_ms, h->stage_ms + 6, 0.0f);
    std::fill(h->tier_ms, h->tier_ms + 2, 0.0f);
    {
        mrs::StageMarks m1(timing && !h->init_valid, nullptr);
        m1.mark(0);
        MRS_TRY(pgo_stage1(h));
        m1.mark(1);
        if (m1) {
            MRS_HIP_TRY(hipStreamSynchronize(nullptr));
            h->stage_ms[0] = m1.ms(0);
        }
    }
    const int N = h->g.N, F = h->F;
    const FactorPass pass(h, pgo_has_noise(h), MRS_PGO_KERNEL_NONE);
    double* T = h->T.get();
    Status* st = h->status.get();
    MRS_HIP_TRY(hipMemcpyAsync(T, h->T0.get(), (size_t)N * 12 * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    pass.information();
    int its = 0, converged = 0;
    double max_delta = 0.0, e0 = 0.0, e1 = 0.0;
    while (its < max_iterations) {
        mrs::StageMarks m(timing, nullptr);
        MRS_HIP_TRY(hipMemsetAsync(st, 0, sizeof(Status), nullptr));
        m.mark(0);
        if (F) {
            pass.linearize(T, true);
            if (its == 0) MRS_TRY(pgo_error_sum(h, &e0));
        }
        pass.gather(0.0, false);
        m.mark(1);
        MRS_TRY((pgo_solve<6, 1>(h, 2, &m, 2)));                  // marks 2 .. 5
        hipLaunchKernelGGL(k_pgo_retract, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, nullptr, T, h->delta.get(), N, st);
        m.mark(6);
        MRS_HIP_TRY(hipGetLastError());
        Status hs;
        MRS_HIP_TRY(hipMemcpy(&hs, st, sizeof(hs), hipMemcpyDeviceToHost));      // the 16 bytes of this iteration
        if (m) {
            h->stage_ms[1] += m.ms(0);
            h->stage_ms[2] += m.ms(1) + m.ms(4);
            h->stage_ms[3] += m.ms(2);
            h->stage_ms[4] += m.ms(3);
            h->stage_ms[5] += m.ms(5);
            h->tier_ms[0] += m.ms(3, kMarkTierDown);
            h->tier_ms[1] += m.ms(kMarkTierUp, 4);
        }
        ++its;
        MRS_TRY(pgo_check_pivots(h, hs, 2));
        std::memcpy(&max_delta, &hs.max_delta, sizeof(double));
        if (!std::isfinite(max_delta)) {
            mrs::set_error("Gauss-Newton iteration %d produced a step that is not finite", its);
            return MRS_ERR_NOT_CONVERGED;
        }
        if (max_delta < eps) {
            converged = 1;
            break;
        }
    }
    if (F) {
        pass.error(T);
        MRS_TRY(pgo_error_sum(h, &e1));
    }
    MRS_TRY(pgo_download(T, N, h_T));
    h->result_valid = true;
    h->result_weighted = pass.weighted;
    h_info[0] = its;
    h_info[1] = converged;
    h_info[2] = max_delta;
    h_info[3] = e0;
    h_info[4] = e1;
    h_info[5] = h->topo[1].E;
    return MRS_OK;
}

// Levenberg-Marquardt step control on the same solves.  Per solve the host reads the status words and two doubles.
int mrs_pgo_optimize_lm(mrs_pgo* pgo, double eps, int32_t max_solves, double* h_T, double* h_info)
{
    MRS_REQUIRE(pgo && h_T && h_info, "null pointer");
    MRS_REQUIRE(eps >= 0.0 && std::isfinite(eps), "eps must be finite and not negative");
    MRS_REQUIRE(max_solves >= 1, "max_solves must be positive");
    MRS_TRY(pgo_ready(pgo));
    mrs_pgo* h = pgo;
    h->result_valid = false;
    h->drop_marginals();
    const bool timing = mrs::dev_env("MRS_PGO_TIMING") != nullptr;
    std::fill(h->stage_ms, h->stage_ms + 6, 0.0f);
    std::fill(h->tier_ms, h->tier_ms + 2, 0.0f);
    {
        mrs::StageMarks m1(timing && !h->init_valid, nullptr);
        m1.mark(0);
        MRS_TRY(pgo_stage1(h));
        m1.mark(1);
        if (m1) {
            MRS_HIP_TRY(hipStreamSynchronize(nullptr));
            h->stage_ms[0] = m1.ms(0);
        }
    }
    const int N = h->g.N, F = h->F;
    const FactorPass pass(h, pgo_has_noise(h) || h->kernel != MRS_PGO_KERNEL_NONE, h->kernel);
    double *T = h->T.get(), *Tprev = h->Tprev.get();
    Status* st = h->status.get();
    double* d_pair = reinterpret_cast<double*>(st + 1);          // the cost after the step, twice the predicted decrease
    const size_t pose_bytes = (size_t)N * 12 * sizeof(double);
    MRS_HIP_TRY(hipMemcpyAsync(T, h->T0.get(), pose_bytes, hipMemcpyDeviceToDevice, nullptr));
    pass.information();
    double c0 = 0.0;
    if (F) {
        pass.error(T);
        MRS_TRY(pgo_error_sum(h, &c0));
    }
    double c = c0, lambda = MRS_PGO_LM_LAMBDA_INITIAL, nu = 2.0, max_delta = 0.0;
    int solves = 0, accepted = 0, converged = 0;
    while (solves < max_solves) {
        const bool first = solves == 0;
        const double lam = first ? 0.0 : lambda;
        mrs::StageMarks m(timing, nullptr);
        MRS_HIP_TRY(hipMemsetAsync(st, 0, 2 * sizeof(Status), nullptr));
        m.mark(0);
        pass.linearize(T, !first);
        pass.gather(lam, true);
        m.mark(1);
        MRS_TRY((pgo_solve<6, 1>(h, 2, &m, 2)));                  // marks 2 .. 5
        hipLaunchKernelGGL(k_pgo_predicted, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, nullptr, h->delta.get(), h->diag.get(), h->gp.get(), lam,
                           N, h->predv.get());
        pgo_tree_sum(h->predv.get(), N, h->partial_p.get(), d_pair + 1);
        MRS_HIP_TRY(hipMemcpyAsync(Tprev, T, pose_bytes, hipMemcpyDeviceToDevice, nullptr));
        hipLaunchKernelGGL(k_pgo_retract, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, nullptr, T, h->delta.get(), N, st);
        if (F) {
            pass.error(T);
            pgo_tree_sum(h->err.get(), F, h->partial.get(), d_pair);
        }
        m.mark(6);
        MRS_HIP_TRY(hipGetLastError());
        struct {
            Status st;
            double cost, pred2;
        } hs;
        static_assert(sizeof(hs) == 2 * sizeof(Status), "one copy of 32 bytes per solve");
        MRS_HIP_TRY(hipMemcpy(&hs, st, sizeof(hs), hipMemcpyDeviceToHost));
        if (m) {
            h->stage_ms[1] += m.ms(0);
            h->stage_ms[2] += m.ms(1) + m.ms(4);
            h->stage_ms[3] += m.ms(2);
            h->stage_ms[4] += m.ms(3);
            h->stage_ms[5] += m.ms(5);
            h->tier_ms[0] += m.ms(3, kMarkTierDown);
            h->tier_ms[1] += m.ms(kMarkTierUp, 4);
        }
        ++solves;
        MRS_TRY(pgo_check_pivots(h, hs.st, 2));
        double step;
        std::memcpy(&step, &hs.st.max_delta, sizeof(double));
        const double c_new = hs.cost, pred = 0.5 * hs.pred2;
        if (!std::isfinite(step) || !std::isfinite(c_new)) {
            mrs::set_error("Levenberg-Marquardt solve %d produced a step or a cost that is not finite", solves);
            return MRS_ERR_NOT_CONVERGED;
        }
        const bool below = pred <= MRS_PGO_LM_PRED_FLOOR * c;    // the cost cannot resolve this step: neither the decision nor the gain
        if (first || c_new <= c || below) {
            if (!first) {
                const double rho = below ? 1.0 : (c - c_new) / pred, q = 2.0 * rho - 1.0;
                double factor = 1.0 - q * q * q;
                if (!(factor > 1.0 / 3.0)) factor = 1.0 / 3.0;   // a rho that is not a number too
                lambda = std::min(std::max(lambda * factor, MRS_PGO_LM_LAMBDA_MIN), MRS_PGO_LM_LAMBDA_MAX);
                nu = 2.0;
            }
            ++accepted;
            c = c_new;
            max_delta = step;
            if (max_delta < eps) {
                converged = 1;
                break;
            }
        } else {
            MRS_HIP_TRY(hipMemcpyAsync(T, Tprev, pose_bytes, hipMemcpyDeviceToDevice, nullptr));
            lambda = std::min(std::max(lambda * nu, MRS_PGO_LM_LAMBDA_MIN), MRS_PGO_LM_LAMBDA_MAX);
            nu *= 2.0;
        }
    }
    if (F) pass.error(T);                                        // the loops' state at the result
    MRS_HIP_TRY(hipGetLastError());
    MRS_TRY(pgo_download(T, N, h_T));
    h->result_valid = true;
    h->result_weighted = pass.weighted;
    h_info[0] = solves;
    h_info[1] = accepted;
    h_info[2] = converged;
    h_info[3] = max_delta;
    h_info[4] = c0;
    h_info[5] = c;
    h_info[6] = h->topo[1].E;
    h_info[7] = lambda;
    return MRS_OK;
}

int mrs_pgo_set_solver(mrs_pgo* pgo, int32_t solver, int32_t dense_limit, int32_t max_blocks)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(solver == MRS_PGO_SOLVER_DENSE || solver == MRS_PGO_SOLVER_SPARSE, "the solver must be one of MRS_PGO_SOLVER_*");
    MRS_REQUIRE(dense_limit >= -1 && dense_limit <= kMaxSep, "dense_limit must be in 0 .. MRS_PGO_MAX_SEPARATORS, or -1 for the default");
    MRS_REQUIRE(max_blocks >= 0, "max_blocks must be positive, or 0 for the default");
    if (dense_limit < 0 || solver == MRS_PGO_SOLVER_DENSE) dense_limit = kMaxSep;
    if (max_blocks == 0 || solver == MRS_PGO_SOLVER_DENSE) max_blocks = MRS_PGO_MAX_SPARSE_BLOCKS;
    if (solver == pgo->solver && dense_limit == pgo->dense_limit && max_blocks == pgo->max_blocks) return MRS_OK;
    MRS_TRY(pgo_check_size(solver, dense_limit, max_blocks, pgo->g, pgo->seglen));
    pgo->solver = solver;
    pgo->dense_limit = dense_limit;
    pgo->max_blocks = max_blocks;
    pgo->dirty = true;
    return MRS_OK;
}

int mrs_pgo_get_solver_stats(mrs_pgo* pgo, int32_t stage, int64_t* h_stats)
{
    MRS_REQUIRE(pgo && h_stats, "null pointer");
    MRS_REQUIRE(stage == 1 || stage == 2, "the stage must be 1 or 2");
    Topology t;
    mrs::pgo::SparseOrder o;
    build_topology(pgo->g, pgo->seglen, stage, &t);
    o.E = o.core = t.E;
    if (pgo->solver == MRS_PGO_SOLVER_SPARSE) MRS_TRY(pgo_sparse_order(t, stage, pgo->dense_limit, pgo->max_blocks, &o));
    const int64_t stats[MRS_PGO_SOLVER_STATS] = {o.E, o.eliminated, o.core, o.levels, o.blocks, o.updates, o.max_degree, pgo->solver};
    std::copy(stats, stats + MRS_PGO_SOLVER_STATS, h_stats);
    return MRS_OK;
}

int mrs_pgo_last_tier_ms(mrs_pgo* pgo, float* h_ms)
{
    MRS_REQUIRE(pgo && h_ms, "null pointer");
    std::copy(pgo->tier_ms, pgo->tier_ms + 2, h_ms);
    return MRS_OK;
}

int mrs_pgo_last_stage_ms(mrs_pgo* pgo, float* h_ms)
{
    MRS_REQUIRE(pgo && h_ms, "null pointer");
    std::copy(pgo->stage_ms, pgo->stage_ms + 6, h_ms);
    return MRS_OK;
}

// ---- marginal covariances of the last result

int mrs_pgo_mark_poses(mrs_pgo* pgo, const int32_t* h_poses, int32_t n)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(n >= 0, "n must not be negative");
    MRS_REQUIRE(h_poses || n == 0, "null pointer");
    std::vector<int> marks(h_poses, h_poses + n);
    std::sort(marks.begin(), marks.end());
    MRS_REQUIRE(marks.empty() || (marks.front() >= 0 && marks.back() < pgo->g.N), "a marked pose lies outside the graph");
    MRS_REQUIRE(std::adjacent_find(marks.begin(), marks.end()) == marks.end(), "a pose is marked twice");
    if (marks == pgo->g.marks) return MRS_OK;
    Graph g = pgo->g;
    g.marks = marks;
    MRS_TRY(pgo_check_size(pgo, g, pgo->seglen));
    pgo->g = std::move(g);
    pgo->dirty = true;
    pgo->result_valid = false;
    pgo->marg_valid = false;
    return MRS_OK;
}

int mrs_pgo_compute_marginals(mrs_pgo* pgo, int64_t* h_info)
{
    MRS_REQUIRE(pgo, "null pointer");
    MRS_REQUIRE(pgo->result_valid && !pgo->dirty, "no optimisation of the graph as it stands has finished");
    mrs_pgo* h = pgo;
    if (h->sp[1].eliminated > 0) {
        mrs::set_error("marginals are not built through the sparse tier: it eliminated %d of stage 2's %d separators", h->sp[1].eliminated,
                       h->topo[1].E);
        return MRS_ERR_UNSUPPORTED;
    }
    const int N = h->g.N, F = h->F, E = h->topo[1].E, n = 6 * E, nblk = (int)blocks_for(n, kMT);
    const size_t ld = (size_t)n, nseg = (size_t)h->dtopo[1].sv.n;
    if (!h->marg_valid) {
        MRS_HIP_TRY(hipSetDevice(h->ctx->device));
        const bool timing = mrs::dev_env("MRS_PGO_TIMING") != nullptr;
        std::fill(h->marg_ms, h->marg_ms + 4, 0.0f);
        h->h_sep_of.assign(N, -1);
        for (int a = 0; a < E; ++a) h->h_sep_of[h->topo[1].sep_node[a]] = a;
        MRS_TRY(h->sep_of.reserve((size_t)N, (size_t)N));
        MRS_TRY(h->Sig.reserve(std::max<size_t>(ld * ld, 1), std::max<size_t>(ld * ld, 1)));
        MRS_TRY(h->Spp.reserve((size_t)N * 36, (size_t)N * 36));
        MRS_TRY(h->Spn.reserve((size_t)N * 36, (size_t)N * 36));
        MRS_HIP_TRY(hipMemcpy(h->sep_of.get(), h->h_sep_of.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
        // the factor at the result: the weights of the loops' state, no damping, zero right-hand sides
        const FactorPass pass(h, h->result_weighted, h->result_weighted ? h->kernel : (int)MRS_PGO_KERNEL_NONE);
        double *T = h->T.get(), *S = h->S.get(), *M = h->Sig.get();
        Status* st = h->status.get();
        mrs::StageMarks m(timing, nullptr);
        MRS_HIP_TRY(hipMemsetAsync(st, 0, sizeof(Status), nullptr));
        m.mark(0);
        pass.linearize(T, true);
        pass.gather(0.0, false);
        MRS_HIP_TRY(hipMemsetAsync(h->gp.get(), 0, (size_t)N * 6 * sizeof(double), nullptr));
        MRS_TRY((pgo_solve<6, 1>(h, 2, nullptr, 0)));
        if (F) pass.error(T);                                    // the loops' state as the optimiser left it
        m.mark(1);
        Status hs;
        MRS_HIP_TRY(hipMemcpy(&hs, st, sizeof(hs), hipMemcpyDeviceToHost));
        MRS_TRY(pgo_check_pivots(h, hs, 2));
        MRS_HIP_TRY(hipMemsetAsync(h->Spp.get(), 0, (size_t)N * 36 * sizeof(double), nullptr));
        MRS_HIP_TRY(hipMemsetAsync(h->Spn.get(), 0, (size_t)N * 36 * sizeof(double), nullptr));
        m.mark(2);
        if (E) {
            MRS_HIP_TRY(hipMemsetAsync(M, 0, ld * ld * sizeof(double), nullptr));
            hipLaunchKernelGGL(k_pgo_inv_diag, dim3(nblk), dim3(kThreads), 0, nullptr, S, M, n, ld);
            for (int I = 1; I < nblk; ++I) hipLaunchKernelGGL(k_pgo_inv_row, dim3(I), dim3(kThreads), 0, nullptr, S, M, n, ld, I);
            m.mark(3);
            // Sigma takes the factor's place in S and is then copied over M: the handle keeps one array, apart from the optimiser's own
            hipLaunchKernelGGL(k_pgo_inv_product, dim3(nblk, nblk), dim3(kThreads), 0, nullptr, M, S, n, ld);
            MRS_HIP_TRY(hipMemcpyAsync(M, S, ld * ld * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
        } else {
            m.mark(3);
        }
        m.mark(4);
        if (nseg)
            hipLaunchKernelGGL(k_pgo_marginal_walk, dim3(blocks_for((long long)nseg, 64)), dim3(64), 0, nullptr, h->dtopo[1].sv, h->Lk.get(),
                               h->Ak.get(), h->Wk.get(), M, ld, h->Spp.get(), h->Spn.get());
        m.mark(5);
        MRS_HIP_TRY(hipGetLastError());
        MRS_HIP_TRY(hipStreamSynchronize(nullptr));
        if (m) {
            h->marg_ms[0] = m.ms(0);
            h->marg_ms[1] = m.ms(2);
            h->marg_ms[2] = m.ms(3);
            h->marg_ms[3] = m.ms(4);
        }
        h->marg_valid = true;
    }
    if (h_info) {
        h_info[0] = E;
        h_info[1] = n;
        h_info[2] = (int64_t)((h->Sig.capacity() + h->Spp.capacity() + h->Spn.capacity()) * sizeof(double));
        h_info[3] = 0;
    }
    return MRS_OK;
}

int mrs_pgo_get_marginals(mrs_pgo* pgo, const int32_t* h_poses, int32_t n, int32_t frame, double* h_cov)
{
    MRS_REQUIRE(pgo && h_cov, "null pointer");
    MRS_REQUIRE(frame == MRS_PGO_FRAME_CHORDAL || frame == MRS_PGO_FRAME_POSE3, "the frame must be one of MRS_PGO_FRAME_*");
    MRS_REQUIRE(pgo->result_valid && !pgo->dirty, "no optimisation of the graph as it stands has finished");
    MRS_REQUIRE(pgo->marg_valid, "mrs_pgo_compute_marginals has not run on the result as it stands");
    if (h_poses) {
        MRS_REQUIRE(n >= 0, "n must not be negative");
        for (int u = 0; u < n; ++u) MRS_REQUIRE(h_poses[u] >= 0 && h_poses[u] < pgo->g.N, "a query names a pose outside the graph");
    } else {
        MRS_REQUIRE(n == pgo->g.N, "without a list of poses n is the number of poses");
    }
    if (n == 0) return MRS_OK;
    return pgo_marginal_query(pgo, h_poses, nullptr, n, frame, 36, h_cov);
}

int mrs_pgo_get_joint_marginals(mrs_pgo* pgo, const int32_t* h_i, const int32_t* h_j, int32_t n, int32_t frame, double* h_cov)
{
    MRS_REQUIRE(pgo && h_cov, "null pointer");
    MRS_REQUIRE(n >= 0, "n must not be negative");
    MRS_REQUIRE((h_i && h_j) || n == 0, "null pointer");
    MRS_REQUIRE(frame == MRS_PGO_FRAME_CHORDAL || frame == MRS_PGO_FRAME_POSE3, "the frame must be one of MRS_PGO_FRAME_*");
    MRS_REQUIRE(pgo->result_valid && !pgo->dirty, "no optimisation of the graph as it stands has finished");
    MRS_REQUIRE(pgo->marg_valid, "mrs_pgo_compute_marginals has not run on the result as it stands");
    const Graph& g = pgo->g;
    for (int u = 0; u < n; ++u) {
        const int i = h_i[u], j = h_j[u];
        MRS_REQUIRE(i >= 0 && i < g.N && j >= 0 && j < g.N, "a query names a pose outside the graph");
        MRS_REQUIRE(i != j, "a joint marginal is of two different poses");
        const bool si = i == 0 || pgo->h_sep_of[i] >= 0, sj = j == 0 || pgo->h_sep_of[j] >= 0;
        if (si && sj) continue;
        if (std::abs(i - j) == 1 && pgo_chain_of(g, i) == pgo_chain_of(g, j)) continue;
        mrs::set_error("bad argument: the joint marginal of poses %d and %d is not held: pose %d is not a separator of stage 2, mark it with "
                       "mrs_pgo_mark_poses (pair %d of the call)", i, j, si ? j : i, u);
        return MRS_ERR_ARG;
    }
    if (n == 0) return MRS_OK;
    return pgo_marginal_query(pgo, h_i, h_j, n, frame, 144, h_cov);
}

int mrs_pgo_last_marginal_ms(mrs_pgo* pgo, float* h_ms)
{
    MRS_REQUIRE(pgo && h_ms, "null pointer");
    std::copy(pgo->marg_ms, pgo->marg_ms + 4, h_ms);
    return MRS_OK;
}

}  // extern "C"
