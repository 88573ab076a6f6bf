// mrslam/posegraph.hpp -- C++ host-side pose-graph optimisation for the Mapping workspace.
//
// Stands where GlobalManager calls evaluation_utils::centralizedGNEstimation (Mapping/src/global_manager/src/global_manager.cpp:1354;
// distributed_mapper/evaluation_utils.cpp:273-329): the rotations by chordal relaxation, then Gauss-Newton on BetweenChordalFactor errors.
// All arithmetic happens in libmrslam_hip.so through the C ABI (mrs_pgo_*); this header only adapts types.  Plain arrays
// in, std::vector<double> out: no gtsam and no Eigen.  A pose is 16 doubles, the row-major 4x4 (gtsam: pose.matrix(), copied row by row).
//
// Poses are numbered chain after chain (robot after robot); a factor (i, j, Z) measures the pose of j in the frame of i.
#pragma once
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "mrslam_hip.h"

namespace mrslam {

class PoseGraph {
public:
    struct Result {
        std::vector<double> poses;       // [poses][16]
        int iterations = 0;
        bool converged = false;
        double max_delta = 0.0;          // the last Gauss-Newton step's largest component
        double error_initial = 0.0;      // 0.5 sum |e|^2 at the chordal start: the reference's "Initial Error"
        double error_final = 0.0;        // and at the result: its "GN Error"
        int separators = 0;
    };

    explicit PoseGraph(const std::vector<int32_t>& chain_lengths, int device = 0)
        : poses_(std::accumulate(chain_lengths.begin(), chain_lengths.end(), 0))
    {
        check(mrs_ctx_create(device, &ctx_), "mrs_ctx_create");
        const int st = mrs_pgo_create(ctx_, static_cast<int32_t>(chain_lengths.size()), chain_lengths.data(), &h_);
        if (st != MRS_OK) {
            const std::string why = std::string(mrs_status_str(st)) + ": " + mrs_last_error();
            mrs_ctx_destroy(ctx_);
            throw std::runtime_error("mrs_pgo_create: " + why);
        }
    }
    ~PoseGraph()
    {
        mrs_pgo_destroy(h_);
        mrs_ctx_destroy(ctx_);
    }
    PoseGraph(const PoseGraph&) = delete;
    PoseGraph& operator=(const PoseGraph&) = delete;

    int poses() const { return poses_; }
    // one between-pose per consecutive pair of a chain, chain after chain: Z [n][16]
    void setOdometry(const double* Z, int n) { check(mrs_pgo_set_odometry(h_, Z, n), "mrs_pgo_set_odometry"); }
    // n loop factors: Z [n][16], the measured pose of j[u] in the frame of i[u]
    void addLoops(const int32_t* i, const int32_t* j, const double* Z, int n) { check(mrs_pgo_add_loops(h_, i, j, Z, n), "mrs_pgo_add_loops"); }
    void clearLoops() { check(mrs_pgo_clear_loops(h_), "mrs_pgo_clear_loops"); }
    int loops() const
    {
        int32_t n = 0;
        check(mrs_pgo_count(h_, &n), "mrs_pgo_count");
        return n;
    }
    void setPrior(const double* T) { check(mrs_pgo_set_prior(h_, T), "mrs_pgo_set_prior"); }
    void setSegmentLength(int length) { check(mrs_pgo_set_segment_length(h_, length), "mrs_pgo_set_segment_length"); }

    // stage 1 alone: the relaxed rotations projected to SO(3), zero translations, [poses][16]
    std::vector<double> initialize()
    {
        std::vector<double> T(static_cast<size_t>(poses_) * 16);
        check(mrs_pgo_initialize(h_, T.data()), "mrs_pgo_initialize");
        return T;
    }

    // centralizedGNEstimation with a stop rule: eps = 0 and max_iterations = 200 is the reference's loop, max_iterations = 1 is
    // centralizedEstimation
    Result optimize(double eps = 1e-9, int max_iterations = MRS_PGO_DEFAULT_MAX_ITERATIONS)
    {
        Result r;
        r.poses.resize(static_cast<size_t>(poses_) * 16);
        double info[MRS_PGO_INFO_DOUBLES] = {};
        check(mrs_pgo_optimize(h_, eps, max_iterations, r.poses.data(), info), "mrs_pgo_optimize");
        r.iterations = static_cast<int>(info[0]);
        r.converged = info[1] != 0.0;
        r.max_delta = info[2];
        r.error_initial = info[3];
        r.error_final = info[4];
        r.separators = static_cast<int>(info[5]);
        return r;
    }

    // ---- per-factor noise, Levenberg-Marquardt step control, robust kernels on the loops
    struct ResultLM {
        std::vector<double> poses;       // [poses][16]
        int solves = 0, accepted = 0;
        bool converged = false;
        double max_delta = 0.0;          // the last accepted step's largest component
        double cost_initial = 0.0;       // sum 0.5 r^2 over the odometry factors + sum rho(r) over the loops, at the chordal start
        double cost_final = 0.0;         // and at the result
        int separators = 0;
        double lambda = 0.0;
    };
    struct LoopState {
        std::vector<double> weight, r2;  // per loop: the kernel's weight and e^T L e at the last result
    };

    // one Pose3 covariance (gtsam's order: rotation xyz, translation xyz) per odometry factor, C [n][36]; nullptr, 0 clears them
    void setOdometryNoise(const double* C, int n) { check(mrs_pgo_set_odometry_noise(h_, C, n), "mrs_pgo_set_odometry_noise"); }
    // addLoops with a covariance per loop, C [n][36]
    void addLoops(const int32_t* i, const int32_t* j, const double* Z, const double* C, int n)
    {
        check(mrs_pgo_add_loops_noise(h_, i, j, Z, C, n), "mrs_pgo_add_loops_noise");
    }
    // MRS_PGO_KERNEL_*: in force under optimizeLM only; optimize refuses a handle with a kernel
    void setLoopKernel(int kernel, double k = 1.0) { check(mrs_pgo_set_loop_kernel(h_, kernel, k), "mrs_pgo_set_loop_kernel"); }

    ResultLM optimizeLM(double eps = 1e-9, int max_solves = MRS_PGO_DEFAULT_MAX_ITERATIONS)
    {
        ResultLM r;
        r.poses.resize(static_cast<size_t>(poses_) * 16);
        double info[MRS_PGO_LM_INFO_DOUBLES] = {};
        check(mrs_pgo_optimize_lm(h_, eps, max_solves, r.poses.data(), info), "mrs_pgo_optimize_lm");
        r.solves = static_cast<int>(info[0]);
        r.accepted = static_cast<int>(info[1]);
        r.converged = info[2] != 0.0;
        r.max_delta = info[3];
        r.cost_initial = info[4];
        r.cost_final = info[5];
        r.separators = static_cast<int>(info[6]);
        r.lambda = info[7];
        return r;
    }

    LoopState loopState() const
    {
        LoopState s;
        const int n = loops();
        s.weight.resize(static_cast<size_t>(n) + 1);
        s.r2.resize(static_cast<size_t>(n) + 1);
        check(mrs_pgo_get_loop_state(h_, s.weight.data(), s.r2.data(), n), "mrs_pgo_get_loop_state");
        s.weight.resize(n);
        s.r2.resize(n);
        return s;
    }

    // ---- the sparse elimination tier in front of the dense Cholesky
    struct SolverStats {
        long long separators = 0, eliminated = 0, core = 0, levels = 0, blocks = 0, updates = 0, max_degree = 0;
        int solver = MRS_PGO_SOLVER_DENSE;
    };
    // MRS_PGO_SOLVER_*; dense_limit -1 and max_blocks 0 are the defaults
    void setSolver(int solver, int dense_limit = -1, int max_blocks = 0)
    {
        check(mrs_pgo_set_solver(h_, solver, dense_limit, max_blocks), "mrs_pgo_set_solver");
    }
    SolverStats solverStats(int stage = 2) const
    {
        int64_t st[MRS_PGO_SOLVER_STATS] = {};
        check(mrs_pgo_get_solver_stats(h_, stage, st), "mrs_pgo_get_solver_stats");
        SolverStats s;
        s.separators = st[0];
        s.eliminated = st[1];
        s.core = st[2];
        s.levels = st[3];
        s.blocks = st[4];
        s.updates = st[5];
        s.max_degree = st[6];
        s.solver = static_cast<int>(st[7]);
        return s;
    }

    // ---- marginal covariances of the last result by selected inversion
    struct MarginalInfo {
        long long separators = 0, order = 0, bytes = 0;
    };
    // the poses stage 2 keeps as separators whether or not a loop touches them; an empty list clears the set.  The last result is gone.
    void markPoses(const std::vector<int32_t>& poses)
    {
        check(mrs_pgo_mark_poses(h_, poses.empty() ? nullptr : poses.data(), static_cast<int32_t>(poses.size())), "mrs_pgo_mark_poses");
    }
    // factors and inverts the information matrix at the last result unless that is held already
    MarginalInfo computeMarginals()
    {
        int64_t info[MRS_PGO_MARGINAL_INFO] = {};
        check(mrs_pgo_compute_marginals(h_, info), "mrs_pgo_compute_marginals");
        MarginalInfo m;
        m.separators = info[0];
        m.order = info[1];
        m.bytes = info[2];
        return m;
    }
    // [n][36] of the poses named, or [poses][36] of all poses; frame: MRS_PGO_FRAME_*
    std::vector<double> marginals(const std::vector<int32_t>& poses, int frame = MRS_PGO_FRAME_CHORDAL)
    {
        computeMarginals();
        std::vector<double> cov(poses.size() * 36);
        if (!poses.empty())
            check(mrs_pgo_get_marginals(h_, poses.data(), static_cast<int32_t>(poses.size()), frame, cov.data()), "mrs_pgo_get_marginals");
        return cov;
    }
    std::vector<double> marginals(int frame = MRS_PGO_FRAME_CHORDAL)
    {
        computeMarginals();
        std::vector<double> cov(static_cast<size_t>(poses_) * 36);
        check(mrs_pgo_get_marginals(h_, nullptr, poses_, frame, cov.data()), "mrs_pgo_get_marginals");
        return cov;
    }
    // [n][144]: [[S_ii, S_ij], [S_ji, S_jj]] per pair; answered between separators (and pose 0) and between consecutive poses of a chain
    std::vector<double> jointMarginals(const std::vector<int32_t>& i, const std::vector<int32_t>& j, int frame = MRS_PGO_FRAME_CHORDAL)
    {
        if (i.size() != j.size()) throw std::invalid_argument("jointMarginals: i and j must have one entry per pair");
        computeMarginals();
        std::vector<double> cov(i.size() * 144);
        if (!i.empty())
            check(mrs_pgo_get_joint_marginals(h_, i.data(), j.data(), static_cast<int32_t>(i.size()), frame, cov.data()),
                  "mrs_pgo_get_joint_marginals");
        return cov;
    }

private:
    static void check(int st, const char* what)
    {
        if (st != MRS_OK) throw std::runtime_error(std::string(what) + ": " + mrs_status_str(st) + ": " + mrs_last_error());
    }

    mrs_ctx* ctx_ = nullptr;
    mrs_pgo* h_ = nullptr;
    int poses_ = 0;
};

}  // namespace mrslam
