// The point type with normals of the Mapping workspace (typedefs.h:64-68: pcl::PointXYZINormal) for the adapter tests of
// mrslam/icp_normals.hpp, on top of the mock of the pcl::Registration surface.  Layout of pcl/impl/point_types.hpp: 12 floats.
// Test scaffolding only.
#pragma once
#include "mock_pcl.hpp"

namespace pcl {
struct alignas(16) PointXYZINormal {
    float x, y, z, pad;
    float normal_x, normal_y, normal_z, pad_n;
    float intensity, curvature, p2, p3;
};
}  // namespace pcl
