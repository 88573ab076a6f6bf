// mrslam/gicp.hpp -- C++ host-side mirror of pcl::GeneralizedIterativeClosestPoint for the Mapping workspace.
//
// Drop-in for the class the PCL_GICP branch of GlobalManager::select_registration_method builds at
// Mapping/src/global_manager/src/global_manager.cpp:2419-2426 (`pcl::GeneralizedIterativeClosestPoint<PointTI, PointTI>::Ptr gicp(new ...)`,
// setTransformationEpsilon / setMaximumIterations / setMaxCorrespondenceDistance / setEuclideanFitnessEpsilon) and returns as a
// pcl::Registration<PointTI, PointTI>::Ptr, which ICPCheck drives at :2018-2021 and :2058-2071.  All arithmetic happens in
// libmrslam_hip.so through the C ABI (mrs_gicp_batch_align_pcl: DESIGN.md section 4.15 is its definition, parity with PCL is unpinned); this
// header only adapts types, like mrslam/icp.hpp, whose shared library context it reuses.  It needs PCL, which is not in the build image:
// tests/cpp/ compiles it against a minimal mock of the pcl::Registration surface it touches.
//
// getFitnessScore: not virtual in pcl::Registration, so through a pcl::Registration::Ptr PCL's own host implementation runs; on the derived
// type the GPU score of the same definition answers.
#pragma once
#include <cfloat>

#include "fast_gicp/gicp/fast_gicp_mrslam.hpp"

namespace mrslam {

template <typename PointSource, typename PointTarget>
class GeneralizedIterativeClosestPoint : public pcl::Registration<PointSource, PointTarget, float> {
public:
    using Base = pcl::Registration<PointSource, PointTarget, float>;
#if defined(PCL_VERSION) && PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
    using Ptr = pcl::shared_ptr<GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
    using ConstPtr = pcl::shared_ptr<const GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
#else
    using Ptr = boost::shared_ptr<GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
    using ConstPtr = boost::shared_ptr<const GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
#endif
    using PointCloudSource = typename Base::PointCloudSource;
    using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
    using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
    using Matrix4 = typename Base::Matrix4;

    GeneralizedIterativeClosestPoint()
    {
        this->reg_name_ = "GeneralizedIterativeClosestPoint(mrslam_hip)";
        mrs_pclgicp_default_params(&prm_);
        mrs_gicp_default_params(&gicp_prm_);
        this->max_iterations_ = prm_.max_iterations;
        this->transformation_epsilon_ = prm_.transformation_epsilon;
        this->corr_dist_threshold_ = prm_.max_correspondence_distance;
        ctx_ = fast_gicp::detail::shared_ctx(fast_gicp::detail::default_device());
        check(mrs_gicp_batch_create(ctx_, 1, &h_), "mrs_gicp_batch_create");
    }
    ~GeneralizedIterativeClosestPoint() override { mrs_gicp_batch_destroy(h_); }
    GeneralizedIterativeClosestPoint(const GeneralizedIterativeClosestPoint&) = delete;
    GeneralizedIterativeClosestPoint& operator=(const GeneralizedIterativeClosestPoint&) = delete;

    // pcl::GeneralizedIterativeClosestPoint's own setters
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    double getRotationEpsilon() const { return prm_.rotation_epsilon; }
    void setCorrespondenceRandomness(int k)     // the neighbours of a covariance: the handle's k_correspondences
    {
        gicp_prm_.k_correspondences = k;
        check(mrs_gicp_batch_set_params(h_, &gicp_prm_), "mrs_gicp_batch_set_params");
    }
    int getCorrespondenceRandomness() const { return gicp_prm_.k_correspondences; }
    void setMaximumOptimizerIterations(int n) { prm_.max_inner_iterations = n; }
    int getMaximumOptimizerIterations() const { return prm_.max_inner_iterations; }
    // stored and unused, as in PCL's GICP (kept here so that the adapter does not depend on which PCL declares the setter)
    void setEuclideanFitnessEpsilon(double e) { euclidean_fitness_epsilon_ = e; }
    double getEuclideanFitnessEpsilon() const { return euclidean_fitness_epsilon_; }

    // handing over the SAME cloud object again keeps what is on the device (sorted points, box hierarchy and covariances)
    void setInputSource(const PointCloudSourceConstPtr& cloud) override
    {
        if (cloud && this->input_ == cloud && uploaded_[0] == cloud.get()) return;
        Base::setInputSource(cloud);
        upload(0, *cloud);
        uploaded_[0] = cloud.get();
    }
    void setInputTarget(const PointCloudTargetConstPtr& cloud) override
    {
        if (cloud && this->target_ == cloud && uploaded_[1] == cloud.get()) return;
        Base::setInputTarget(cloud);
        upload(1, *cloud);
        uploaded_[1] = cloud.get();
    }

    // pcl::Registration::getFitnessScore(max_range): routed to the GPU NN pass (G6)
    double getFitnessScore(double max_range = DBL_MAX)
    {
        double pose[16], score = DBL_MAX;
        to_row_major(this->final_transformation_, pose);
        check(mrs_gicp_batch_fitness(h_, pose, max_range, &score, nullptr), "mrs_gicp_batch_fitness");
        return score;
    }

    // the state that ended the last align (0, 1, 2 or 5, see mrs_gicp_batch_align_pcl)
    int getConvergenceState() const { return state_; }

protected:
    void computeTransformation(PointCloudSource& output, const Matrix4& guess) override
    {
        prm_.max_iterations = this->max_iterations_;
        prm_.transformation_epsilon = this->transformation_epsilon_;
        prm_.max_correspondence_distance = this->corr_dist_threshold_;
        double g[16], f[16];
        to_row_major(guess, g);
        int32_t conv = 0, iters = 0, state = 0;
        check(mrs_gicp_batch_align_pcl(h_, &prm_, g, f, &conv, &iters, &state, nullptr), "mrs_gicp_batch_align_pcl");
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) this->final_transformation_(r, c) = static_cast<float>(f[4 * r + c]);
        this->converged_ = conv != 0;
        this->nr_iterations_ = iters;
        state_ = state;
        pcl::transformPointCloud(*this->input_, output, this->final_transformation_);
    }

private:
    template <class Cloud>
    void upload(int which, const Cloud& cloud)
    {
        const int stride = static_cast<int>(sizeof(typename Cloud::PointType) / sizeof(float));
        const int64_t offs[2] = {0, static_cast<int64_t>(cloud.points.size())};
        check(mrs_gicp_batch_set_clouds_host(h_, which, reinterpret_cast<const float*>(cloud.points.data()), stride, offs),
              "mrs_gicp_batch_set_clouds_host");
    }
    template <class M>
    static void to_row_major(const M& m, double* out)
    {
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) out[4 * r + c] = static_cast<double>(m(r, c));
    }
    static void check(int st, const char* what)
    {
        if (st != MRS_OK) throw std::runtime_error(std::string(what) + ": " + mrs_status_str(st) + ": " + mrs_last_error());
    }

    mrs_ctx* ctx_ = nullptr;
    mrs_gicp_batch* h_ = nullptr;
    mrs_pclgicp_params prm_;
    mrs_gicp_params gicp_prm_;
    double euclidean_fitness_epsilon_ = -DBL_MAX;
    int state_ = 0;
    const void* uploaded_[2] = {nullptr, nullptr};   // the cloud objects whose points are on the device (source, target)
};

}  // namespace mrslam
