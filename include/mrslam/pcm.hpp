// mrslam/pcm.hpp -- C++ host-side pairwise consistency maximisation for the Mapping workspace.
//
// Stands where GlobalManager reaches distributed_pcm::DistributedPCM::solveCentralized (Mapping/src/global_manager/src/global_manager.cpp:
// 1301-1310), which for every robot pair builds a global_map::GlobalMap and calls pairwiseConsistencyMaximization(): the consistency matrix
// of pairwise_consistency.cpp:40-137, a Matrix-Market file under /tmp/log/, and FMC::maxCliqueHeu.  All arithmetic happens in
// libmrslam_hip.so through the C ABI (mrs_pcm_*); this header only adapts types.  Plain arrays in, std::vector<int> out: no gtsam and no
// Eigen.  A pose is 16 doubles, the row-major 4x4 (gtsam: pose.matrix(), copied row by row).
//
// Vertex numbers follow the order of addLoops.  The reference numbers the loops of a pair in the std::map order of (key1, key2) and keeps
// the first of equal key pairs: sort and deduplicate that way (referenceOrder) to get its member lists number for number.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mrslam_hip.h"

namespace mrslam {

class PairwiseConsistency {
public:
    // getChiSquaredThreshold (pairwise_consistency.cpp:7-38) for 6 degrees of freedom; the reference aborts on any other p
    static double chiSquaredThreshold(double p)
    {
        static const std::pair<int, double> table[] = {{1, 0.872}, {5, 1.635}, {10, 2.204}, {25, 3.455}, {50, 5.348}, {75, 7.840}};
        const double scaled = p * 100.0;
        for (const auto& row : table)
            if (scaled > row.first - 1e-9 && scaled < row.first + 1e-9) return row.second;
        throw std::invalid_argument("PairwiseConsistency: confidence probability " + std::to_string(p) + " is not supported");
    }

    // the order in which the reference numbers loops (ia[u], kb[u]): ascending (ia, kb), the first of equal pairs kept, the others dropped
    static std::vector<int> referenceOrder(const int32_t* ia, const int32_t* kb, int n)
    {
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::make_pair(ia[a], kb[a]) < std::make_pair(ia[b], kb[b]); });
        order.erase(std::unique(order.begin(), order.end(), [&](int a, int b) { return ia[a] == ia[b] && kb[a] == kb[b]; }), order.end());
        return order;
    }

    // the upper quantile q of chi-squared with 6 degrees of freedom: the threshold of a handle with covariances
    static double chiSquaredUpper(double q)
    {
        static const std::pair<int, double> table[] = {{900, 10.645}, {950, 12.592}, {990, 16.812}, {999, 22.458}};
        const double scaled = q * 1000.0;
        for (const auto& row : table)
            if (scaled > row.first - 1e-9 && scaled < row.first + 1e-9) return row.second;
        throw std::invalid_argument("PairwiseConsistency: quantile " + std::to_string(q) + " is not supported");
    }

    struct Threshold {
        double value;
    };
    // a handle whose threshold is given as a number (chiSquaredUpper(q) for a handle with covariances)
    PairwiseConsistency(int capacity, Threshold threshold, int device = 0) { create(capacity, threshold.value, device); }

    explicit PairwiseConsistency(int capacity = MRS_PCM_MAX_LOOPS, double pcm_threshold = 0.01, int device = 0)
    {
        create(capacity, chiSquaredThreshold(pcm_threshold), device);
    }

private:
    void create(int capacity, double threshold, int device)
    {
        check(mrs_ctx_create(device, &ctx_), "mrs_ctx_create");
        const int st = mrs_pcm_create(ctx_, capacity, threshold, &h_);
        if (st != MRS_OK) {
            const std::string why = std::string(mrs_status_str(st)) + ": " + mrs_last_error();
            mrs_ctx_destroy(ctx_);
            throw std::runtime_error("mrs_pcm_create: " + why);
        }
    }

public:
    ~PairwiseConsistency()
    {
        mrs_pcm_destroy(h_);
        mrs_ctx_destroy(ctx_);
    }
    PairwiseConsistency(const PairwiseConsistency&) = delete;
    PairwiseConsistency& operator=(const PairwiseConsistency&) = delete;

    // trajectory poses (buildTrajectory's chain from the identity), [na][16] and [nb][16]; clears the loops
    void setTrajectories(const double* XA, int na, const double* XB, int nb)
    {
        check(mrs_pcm_set_trajectories(h_, XA, na, XB, nb), "mrs_pcm_set_trajectories");
    }
    // n loops: Z [n][16], the measured pose of B_kb[u] in the frame of A_ia[u]
    void addLoops(const int32_t* ia, const int32_t* kb, const double* Z, int n) { check(mrs_pcm_add_loops(h_, ia, kb, Z, n), "mrs_pcm_add_loops"); }
    // Consistency under covariances, after setTrajectories; clears the loops.  mode: MRS_PCM_COV_SPAN (recommended),
    // MRS_PCM_COV_REFERENCE or MRS_PCM_COV_NONE.  QA [na - 1][36], QB [nb - 1][36]: the covariance of every odometry step, first [36]: that
    // of the first pose (REFERENCE only); row-major 6x6 in gtsam's Pose3 tangent order, nullptr: FIXED_COVARIANCE.  The threshold is then
    // compared with the squared Mahalanobis distance: construct with chiSquaredUpper(q) through the threshold constructor.
    void setCovariances(int mode, const double* QA = nullptr, const double* QB = nullptr, const double* first = nullptr)
    {
        check(mrs_pcm_set_covariances(h_, mode, QA, QB, first), "mrs_pcm_set_covariances");
    }
    // n loops with a covariance each, C [n][36] (nullptr: FIXED_COVARIANCE)
    void addLoops(const int32_t* ia, const int32_t* kb, const double* Z, const double* C, int n)
    {
        check(mrs_pcm_add_loops_cov(h_, ia, kb, Z, C, n), "mrs_pcm_add_loops_cov");
    }
    void clearLoops() { check(mrs_pcm_clear_loops(h_), "mrs_pcm_clear_loops"); }
    int size() const
    {
        int32_t n = 0;
        check(mrs_pcm_count(h_, &n), "mrs_pcm_count");
        return n;
    }

    // FMC::maxCliqueHeu's max_clique_data: the loops that may enter the pose graph, in the reference's order
    std::vector<int> solve()
    {
        std::vector<int32_t> members(std::max(size(), 1));
        int32_t n = 0;
        check(mrs_pcm_solve(h_, members.data(), &n, &rounds_), "mrs_pcm_solve");
        return std::vector<int>(members.begin(), members.begin() + n);
    }
    int rounds() const { return rounds_; }

    // FMC::maxClique's max_clique_data, the `use_heuristics = false` side of GlobalMap's constructor: a MAXIMUM clique in ascending order,
    // searched with a budget of max_nodes nodes.  proof(): 2 = size proven and list canonical, 1 = size proven, 0 = the budget ran out and
    // the list is the best clique found (never smaller than solve()'s).  Unlike the reference it never returns a size with an empty list.
    std::vector<int> solveExact(int64_t max_nodes = MRS_PCM_EXACT_DEFAULT_NODES)
    {
        std::vector<int32_t> members(std::max(size(), 1));
        int32_t n = 0;
        check(mrs_pcm_solve_exact(h_, max_nodes, members.data(), &n, &proof_, &nodes_), "mrs_pcm_solve_exact");
        return std::vector<int>(members.begin(), members.begin() + n);
    }
    int proof() const { return proof_; }
    int64_t nodes() const { return nodes_; }

    // the consistency matrix, [size][size] of 0 / 1
    std::vector<uint8_t> matrix() const
    {
        const size_t n = static_cast<size_t>(size());
        std::vector<uint8_t> m(n * n);
        if (n) check(mrs_pcm_get_matrix(h_, m.data()), "mrs_pcm_get_matrix");
        return m;
    }

private:
    static void check(int st, const char* what)
    {
        if (st != MRS_OK) throw std::runtime_error(std::string(what) + ": " + mrs_status_str(st) + ": " + mrs_last_error());
    }

    mrs_ctx* ctx_ = nullptr;
    mrs_pcm* h_ = nullptr;
    int32_t rounds_ = 0;
    int32_t proof_ = 0;
    int64_t nodes_ = 0;
};

}  // namespace mrslam
