// mrslam/icp.hpp -- C++ host-side mirror of pcl::IterativeClosestPoint for the Mapping workspace.
//
// Drop-in for the class GlobalManager::performLoopClosure instantiates at Mapping/src/global_manager/src/global_manager.cpp:890
// (`pcl::IterativeClosestPoint<PointTI, PointTI> icp;`, configured and driven at :891-906: setInputSource / setInputTarget /
// setMaxCorrespondenceDistance / setMaximumIterations / setTransformationEpsilon / setEuclideanFitnessEpsilon / align / hasConverged /
// getFitnessScore / getFinalTransformation) and the PCL_ICP branch of select_registration_method builds at :2427-2434 and returns as a
// pcl::Registration<PointTI, PointTI>::Ptr.  All arithmetic happens in libmrslam_hip.so through the C ABI (mrs_gicp_batch_align_icp);
// this header only adapts types, like fast_gicp_mrslam.hpp, whose shared library context it reuses.  It needs PCL, which is not in the
// build image: tests/cpp/ compiles it against a minimal mock of the pcl::Registration surface it touches.
//
// getFitnessScore: not virtual in pcl::Registration, so through a pcl::Registration::Ptr PCL's own host implementation runs; on the derived
// type (the object of :890 is one) the GPU score of the same definition answers.
#pragma once
#include <cfloat>

#include "fast_gicp/gicp/fast_gicp_mrslam.hpp"

namespace mrslam {

template <typename PointSource, typename PointTarget>
class IterativeClosestPoint : public pcl::Registration<PointSource, PointTarget, float> {
public:
    using Base = pcl::Registration<PointSource, PointTarget, float>;
#if defined(PCL_VERSION) && PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
    using Ptr = pcl::shared_ptr<IterativeClosestPoint<PointSource, PointTarget>>;
    using ConstPtr = pcl::shared_ptr<const IterativeClosestPoint<PointSource, PointTarget>>;
#else
    using Ptr = boost::shared_ptr<IterativeClosestPoint<PointSource, PointTarget>>;
    using ConstPtr = boost::shared_ptr<const IterativeClosestPoint<PointSource, PointTarget>>;
#endif
    using PointCloudSource = typename Base::PointCloudSource;
    using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
    using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
    using Matrix4 = typename Base::Matrix4;

    IterativeClosestPoint()
    {
        this->reg_name_ = "IterativeClosestPoint(mrslam_hip)";
        mrs_icp_default_params(&prm_);
        this->max_iterations_ = prm_.max_iterations;
        this->transformation_epsilon_ = prm_.transformation_epsilon;
        this->corr_dist_threshold_ = prm_.max_correspondence_distance;
        ctx_ = fast_gicp::detail::shared_ctx(fast_gicp::detail::default_device());
        check(mrs_gicp_batch_create(ctx_, 1, &h_), "mrs_gicp_batch_create");
    }
    ~IterativeClosestPoint() override { mrs_gicp_batch_destroy(h_); }
    IterativeClosestPoint(const IterativeClosestPoint&) = delete;
    IterativeClosestPoint& operator=(const IterativeClosestPoint&) = delete;

    // pcl::Registration has both setters; they are kept here so that the adapter does not depend on which PCL declares them
    void setEuclideanFitnessEpsilon(double e) { prm_.euclidean_fitness_epsilon = e; }
    double getEuclideanFitnessEpsilon() const { return prm_.euclidean_fitness_epsilon; }
    void setTransformationRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    double getTransformationRotationEpsilon() const { return prm_.rotation_epsilon; }

    // handing over the SAME cloud object again keeps what is on the device (sorted points and box hierarchy)
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

    // pcl::registration::DefaultConvergenceCriteria::ConvergenceState of the last align (0 .. 5, see mrs_gicp_batch_align_icp)
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
        check(mrs_gicp_batch_align_icp(h_, &prm_, g, f, &conv, &iters, &state, nullptr), "mrs_gicp_batch_align_icp");
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
    mrs_icp_params prm_;
    int state_ = 0;
    const void* uploaded_[2] = {nullptr, nullptr};   // the cloud objects whose points are on the device (source, target)
};

}  // namespace mrslam
