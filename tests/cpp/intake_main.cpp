// Drives mrs_keyframes_ingest / mrs_keyframes_get_points the way INTEGRATION.md section 2a, edit 1, tells the Mapping node to: the point blob
// of a sensor_msgs/PointCloud2 that pcl::toROSMsg made from a pcl::PointXYZI cloud (point_step 32; x, y, z at 0, 4, 8; intensity at 16) handed
// over as it is, then the filtered keyframe read back for keyframe_pub.  PCL is not in the image: the struct below has PointXYZI's layout.
// Prints the hand case of tests/test_intake_cpu.py; tests/test_intake_gpu.py compares the lines with the restatement.
#include "mrslam_hip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

struct alignas(16) PointXYZI {       // pcl::PointXYZI: float data[4] (x, y, z, padding), then the intensity and three more words of padding
    float x, y, z, pad0;
    float intensity, pad1[3];
};
static_assert(sizeof(PointXYZI) == 32 && offsetof(PointXYZI, intensity) == 16, "the layout pcl::toROSMsg describes");

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float rows[9][4] = {{0.1f, 0.1f, 0.1f, 10}, {0.2f, 0.25f, 0.05f, 20}, {0.1f, 0.1f, -1.0f, 5}, {5.0f, 0.1f, std::nextafterf(-1.0f, -inf), 5},
                              {5.0f, 5.0f, 30.0f, 7}, {5.0f, -5.0f, std::nextafterf(30.0f, inf), 9}, {nan, 0, 0, 1}, {0, 0, inf, 1},
                              {-0.05f, -0.05f, -0.05f, 2}};
    std::vector<PointXYZI> cloud(9);                     // msg->keyframePC.data
    for (int i = 0; i < 9; ++i) cloud[i] = PointXYZI{rows[i][0], rows[i][1], rows[i][2], 1.0f, rows[i][3], {0, 0, 0}};
    const int robotid = 2;
    const float pose[16] = {1, 0, 0, 3, 0, 1, 0, 4, 0, 0, 1, 5, 0, 0, 0, 1};

    mrs_ctx* ctx = nullptr;
    mrs_keyframes* kf = nullptr;
    if (mrs_ctx_create(0, &ctx) != MRS_OK || mrs_keyframes_create(ctx, 1 << 16, &kf) != MRS_OK) { std::printf("create failed: %s\n", mrs_last_error()); return 2; }

    // edit 1: fromROSMsg + VoxelGrid(0.3) + PassThrough z [-1, 30] + intensity = robotid * 30 + keyframes.emplace_back, in one call
    const int64_t offsets[2] = {0, (int64_t)cloud.size()};
    int32_t id = -1;
    int64_t kept = -1;
    if (mrs_keyframes_ingest(kf, 1, cloud.data(), 0, offsets, (int32_t)sizeof(PointXYZI), 0, 4, 8, 16, 0.3f, -1.0f, 30.0f, 1, (float)(robotid * 30), pose,
                             &id, &kept, nullptr) != MRS_OK) { std::printf("ingest failed: %s\n", mrs_last_error()); return 2; }
    std::printf("keyframe %d: %lld points\n", id, (long long)kept);

    // the filtered cloud for keyframe_pub
    std::vector<float> out((size_t)kept * 4);
    int64_t n = -1;
    if (mrs_keyframes_get_points(kf, id, out.data(), 0, kept, &n, nullptr) != MRS_OK) { std::printf("get_points failed: %s\n", mrs_last_error()); return 2; }
    for (int64_t i = 0; i < n; ++i) std::printf("point %lld %.9g %.9g %.9g %.9g\n", (long long)i, out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);

    // a capacity one point short is refused
    int64_t m = -1;
    const bool refused = mrs_keyframes_get_points(kf, id, out.data(), 0, kept - 1, &m, nullptr) == MRS_ERR_ARG;
    int32_t stored = -1;
    int64_t total = -1;
    float back[16];
    mrs_keyframes_size(kf, &stored, &total);
    mrs_keyframes_get_pose(kf, id, back, nullptr);
    std::printf("store: %d keyframes, %lld points\n", stored, (long long)total);
    const bool ok = id == 0 && kept == 4 && n == 4 && refused && back[3] == 3 && back[7] == 4 && back[11] == 5;
    mrs_keyframes_destroy(kf);
    return ok ? 0 : 1;
}
