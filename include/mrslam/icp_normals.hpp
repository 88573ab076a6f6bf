// mrslam/icp_normals.hpp -- C++ host-side mirror of pcl::IterativeClosestPointWithNormals and of the Mapping workspace's addNormal helper
// (SURVEY.md 8(a) row G12).
//
// mrslam::addNormal is the twin of GlobalManager's addNormal (Mapping/src/global_manager/src/global_manager.cpp:2679-2693:
// pcl::NormalEstimation over a kd-tree with setKSearch(15), then pcl::concatenateFields into PointXYZINormal, typedefs.h:64-68);
// mrslam::IterativeClosestPointWithNormals is the class that helper exists to feed.  All arithmetic happens in libmrslam_hip.so through the
// C ABI (mrs_gicp_batch_compute_normals, mrs_gicp_batch_align_icp_plane; DESIGN.md 4.16 is the definition); this header only adapts types,
// like mrslam/icp.hpp, whose pattern it follows.  It needs PCL, which is not in the build image: tests/cpp/ compiles it against a minimal
// mock of the surface it touches.
//
// Target normals: a target point type with normal_x / normal_y / normal_z fields hands its own normals over (PCL's class reads them from
// there); any other target type gets normals computed on the GPU with setKSearch / setViewPoint of this class (15, the origin).  Source
// normals are not used, as in PCL's TransformationEstimationPointToPlaneLLS.
#pragma once
#include <cfloat>
#include <type_traits>
#include <vector>

#include "fast_gicp/gicp/fast_gicp_mrslam.hpp"

namespace mrslam {

namespace detail {

template <class P, class = void>
struct has_normal : std::false_type {};
template <class P>
struct has_normal<P, std::void_t<decltype(std::declval<P>().normal_x), decltype(std::declval<P>().normal_y), decltype(std::declval<P>().normal_z)>>
    : std::true_type {};
template <class P, class = void>
struct has_curvature : std::false_type {};
template <class P>
struct has_curvature<P, std::void_t<decltype(std::declval<P>().curvature)>> : std::true_type {};
template <class P, class = void>
struct has_intensity : std::false_type {};
template <class P>
struct has_intensity<P, std::void_t<decltype(std::declval<P>().intensity)>> : std::true_type {};

inline void check(int st, const char* what)
{
    if (st != MRS_OK) throw std::runtime_error(std::string(what) + ": " + mrs_status_str(st) + ": " + mrs_last_error());
}

template <class Cloud>
void upload_points(mrs_gicp_batch* h, int which, const Cloud& cloud)
{
    const int stride = static_cast<int>(sizeof(typename Cloud::PointType) / sizeof(float));
    const int64_t offs[2] = {0, static_cast<int64_t>(cloud.points.size())};
    check(mrs_gicp_batch_set_clouds_host(h, which, reinterpret_cast<const float*>(cloud.points.data()), stride, offs),
          "mrs_gicp_batch_set_clouds_host");
}

// an RAII batch of one pair
struct Batch {
    mrs_gicp_batch* h = nullptr;
    Batch() { check(mrs_gicp_batch_create(fast_gicp::detail::shared_ctx(fast_gicp::detail::default_device()), 1, &h), "mrs_gicp_batch_create"); }
    ~Batch() { mrs_gicp_batch_destroy(h); }
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;
};

}  // namespace detail

// addNormal(cloud, cloudWithNormals) of global_manager.cpp:2679-2693: normals of `cloud` from its k nearest neighbours (viewpoint at the
// origin, as pcl::NormalEstimation's default), written with the points' own fields into *cloudWithNormals (pcl::concatenateFields).
// CloudPtr / CloudWithNormalsPtr: (smart) pointers to pcl::PointCloud<PointXYZI> and pcl::PointCloud<PointXYZINormal> or alike.
template <class CloudPtr, class CloudWithNormalsPtr>
void addNormal(const CloudPtr& cloud, const CloudWithNormalsPtr& cloudWithNormals, int k = 15)
{
    using PointOut = typename std::decay_t<decltype(*cloudWithNormals)>::PointType;
    using PointIn = typename std::decay_t<decltype(*cloud)>::PointType;
    static_assert(detail::has_normal<PointOut>::value, "the output point type needs normal_x / normal_y / normal_z");
    const size_t n = cloud->points.size();
    std::vector<float> nrm(4 * n);
    if (n > 0) {
        detail::Batch b;
        detail::upload_points(b.h, 1, *cloud);
        detail::check(mrs_gicp_batch_compute_normals(b.h, 1, k, nullptr, nullptr), "mrs_gicp_batch_compute_normals");
        detail::check(mrs_gicp_batch_get_normals(b.h, 1, nrm.data()), "mrs_gicp_batch_get_normals");
    }
    cloudWithNormals->points.assign(n, PointOut{});
    for (size_t i = 0; i < n; ++i) {
        PointOut& q = cloudWithNormals->points[i];
        const PointIn& p = cloud->points[i];
        q.x = p.x; q.y = p.y; q.z = p.z;
        if constexpr (detail::has_intensity<PointIn>::value && detail::has_intensity<PointOut>::value) q.intensity = p.intensity;
        q.normal_x = nrm[4 * i]; q.normal_y = nrm[4 * i + 1]; q.normal_z = nrm[4 * i + 2];
        if constexpr (detail::has_curvature<PointOut>::value) q.curvature = nrm[4 * i + 3];
    }
}

template <typename PointSource, typename PointTarget>
class IterativeClosestPointWithNormals : public pcl::Registration<PointSource, PointTarget, float> {
public:
    using Base = pcl::Registration<PointSource, PointTarget, float>;
#if defined(PCL_VERSION) && PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
    using Ptr = pcl::shared_ptr<IterativeClosestPointWithNormals<PointSource, PointTarget>>;
    using ConstPtr = pcl::shared_ptr<const IterativeClosestPointWithNormals<PointSource, PointTarget>>;
#else
    using Ptr = boost::shared_ptr<IterativeClosestPointWithNormals<PointSource, PointTarget>>;
    using ConstPtr = boost::shared_ptr<const IterativeClosestPointWithNormals<PointSource, PointTarget>>;
#endif
    using PointCloudSource = typename Base::PointCloudSource;
    using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
    using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
    using Matrix4 = typename Base::Matrix4;

    IterativeClosestPointWithNormals()
    {
        this->reg_name_ = "IterativeClosestPointWithNormals(mrslam_hip)";
        mrs_icp_plane_default_params(&prm_);
        this->max_iterations_ = prm_.max_iterations;
        this->transformation_epsilon_ = prm_.transformation_epsilon;
        this->corr_dist_threshold_ = prm_.max_correspondence_distance;
    }
    IterativeClosestPointWithNormals(const IterativeClosestPointWithNormals&) = delete;
    IterativeClosestPointWithNormals& operator=(const IterativeClosestPointWithNormals&) = delete;

    void setEuclideanFitnessEpsilon(double e) { prm_.euclidean_fitness_epsilon = e; }
    double getEuclideanFitnessEpsilon() const { return prm_.euclidean_fitness_epsilon; }
    void setTransformationRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    double getTransformationRotationEpsilon() const { return prm_.rotation_epsilon; }
    // pcl::NormalEstimation's setters, for a target type without normal fields (the normals are then computed at the next align)
    void setKSearch(int k) { prm_.normal_k = k; stale_normals_ = true; }
    void setViewPoint(float vx, float vy, float vz)
    {
        prm_.viewpoint[0] = vx; prm_.viewpoint[1] = vy; prm_.viewpoint[2] = vz;
        stale_normals_ = true;
    }

    // handing over the SAME cloud object again keeps what is on the device (sorted points, box hierarchy, normals)
    void setInputSource(const PointCloudSourceConstPtr& cloud) override
    {
        if (cloud && this->input_ == cloud && uploaded_[0] == cloud.get()) return;
        Base::setInputSource(cloud);
        detail::upload_points(b_.h, 0, *cloud);
        uploaded_[0] = cloud.get();
    }
    void setInputTarget(const PointCloudTargetConstPtr& cloud) override
    {
        if (cloud && this->target_ == cloud && uploaded_[1] == cloud.get()) return;
        Base::setInputTarget(cloud);
        detail::upload_points(b_.h, 1, *cloud);
        if constexpr (detail::has_normal<PointTarget>::value) {
            std::vector<float> nrm(4 * cloud->points.size());
            for (size_t i = 0; i < cloud->points.size(); ++i) {
                const PointTarget& p = cloud->points[i];
                nrm[4 * i] = p.normal_x; nrm[4 * i + 1] = p.normal_y; nrm[4 * i + 2] = p.normal_z;
                if constexpr (detail::has_curvature<PointTarget>::value) nrm[4 * i + 3] = p.curvature;
            }
            detail::check(mrs_gicp_batch_set_normals_host(b_.h, 1, nrm.data(), 4), "mrs_gicp_batch_set_normals_host");
        }
        stale_normals_ = false;               // new clouds carry no normals: the next align computes them
        uploaded_[1] = cloud.get();
    }

    // pcl::Registration::getFitnessScore(max_range): routed to the GPU NN pass (G6)
    double getFitnessScore(double max_range = DBL_MAX)
    {
        double pose[16], score = DBL_MAX;
        to_row_major(this->final_transformation_, pose);
        detail::check(mrs_gicp_batch_fitness(b_.h, pose, max_range, &score, nullptr), "mrs_gicp_batch_fitness");
        return score;
    }

    // the ConvergenceState of the last align: 0 .. 5 as pcl::registration::DefaultConvergenceCriteria, 6 = rank-deficient system
    int getConvergenceState() const { return state_; }

protected:
    void computeTransformation(PointCloudSource& output, const Matrix4& guess) override
    {
        prm_.max_iterations = this->max_iterations_;
        prm_.transformation_epsilon = this->transformation_epsilon_;
        prm_.max_correspondence_distance = this->corr_dist_threshold_;
        if constexpr (!detail::has_normal<PointTarget>::value) {
            if (stale_normals_)               // k or the viewpoint changed since the normals on the device were computed
                detail::check(mrs_gicp_batch_compute_normals(b_.h, 1, prm_.normal_k, prm_.viewpoint, nullptr), "mrs_gicp_batch_compute_normals");
        }
        stale_normals_ = false;
        double g[16], f[16];
        to_row_major(guess, g);
        int32_t conv = 0, iters = 0, state = 0;
        detail::check(mrs_gicp_batch_align_icp_plane(b_.h, &prm_, g, f, &conv, &iters, &state, nullptr), "mrs_gicp_batch_align_icp_plane");
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) this->final_transformation_(r, c) = static_cast<float>(f[4 * r + c]);
        this->converged_ = conv != 0;
        this->nr_iterations_ = iters;
        state_ = state;
        pcl::transformPointCloud(*this->input_, output, this->final_transformation_);
    }

private:
    template <class M>
    static void to_row_major(const M& m, double* out)
    {
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) out[4 * r + c] = static_cast<double>(m(r, c));
    }

    detail::Batch b_;
    mrs_icp_plane_params prm_;
    int state_ = 0;
    bool stale_normals_ = false;
    const void* uploaded_[2] = {nullptr, nullptr};   // the cloud objects whose points are on the device (source, target)
};

}  // namespace mrslam
