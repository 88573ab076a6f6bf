// mrslam/gem.hpp -- C++ host-side globally consistent elevation map for the Mapping workspace.
//
// Stands where the elevation node keeps its submap stack (ElevationMapping::updateLocalMap, elevation_mapping/src/ElevationMapping.cpp:
// 653-815: localMap_, globalMap_, trajectory_, localMapLoc_), corrects it after an optimisation (updateGlobalMap, :821-962) and hands it out
// (composingGlobalMap, :501-509), and where PointMapLayer::updateBounds (pointMap_layer.cpp:100-135) turns the cloud into costs.  All
// arithmetic happens in libmrslam_hip.so through the C ABI (mrs_gem_*); this header only adapts types.  Plain arrays in, std::vector out: no
// PCL, no grid_map, no Eigen.  A pose is 16 floats, the row-major 4x4 (Eigen: T.matrix(), copied row by row).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "mrslam_hip.h"

namespace mrslam {

// one cell record: the fields of Anypoint / GridPointData (GridUtilHash.hpp:23-39) as ten 32-bit values
struct ElevationCell {
    float x, y, z, var;
    int32_t r, g, b, frontier;
    float intensity, travers;
};
static_assert(sizeof(ElevationCell) == 40, "a cell record is ten 32-bit values");

class GlobalElevationMap {
public:
    enum Rule { Weighted = MRS_GEM_WEIGHTED, AsWritten = MRS_GEM_AS_WRITTEN };

    explicit GlobalElevationMap(double resolution = 0.2, Rule rule = Weighted, float radius = 15.0f, int min_neighbours = 3, int device = 0)
    {
        check(mrs_ctx_create(device, &ctx_), "mrs_ctx_create");
        const int st = mrs_gem_create(ctx_, resolution, rule, radius, min_neighbours, &h_);
        if (st != MRS_OK) {
            const std::string why = std::string(mrs_status_str(st)) + ": " + mrs_last_error();
            mrs_ctx_destroy(ctx_);
            throw std::runtime_error("mrs_gem_create: " + why);
        }
    }
    ~GlobalElevationMap()
    {
        mrs_gem_destroy(h_);
        mrs_ctx_destroy(ctx_);
    }
    GlobalElevationMap(const GlobalElevationMap&) = delete;
    GlobalElevationMap& operator=(const GlobalElevationMap&) = delete;

    // localMap_ insertion (:796-803): a position met again replaces the stored record
    void appendCells(const ElevationCell* cells, int64_t n) { check(mrs_gem_append_cells(h_, cells, nullptr, n), "mrs_gem_append_cells"); }
    // the same behind the window predicate of :770-779; positions are the caller's (grid_map's getPosition)
    void appendLeaving(const ElevationCell* cells, int64_t n, const float current_xy[2], const float shift_xy[2], int length, float resolution)
    {
        check(mrs_gem_append_leaving(h_, cells, nullptr, n, current_xy, shift_xy, length, resolution), "mrs_gem_append_leaving");
    }
    // globalMap_.push_back(localHashtoPointCloud(localMap_)) with trajectory_ / localMapLoc_ (:682-685)
    void closeSubmap(const float pose[16], const float centre_xy[2]) { check(mrs_gem_close_submap(h_, pose, centre_xy), "mrs_gem_close_submap"); }
    int size() const
    {
        int32_t k = 0;
        check(mrs_gem_count(h_, &k, nullptr, nullptr), "mrs_gem_count");
        return k;
    }
    // updateGlobalMap with optGlobalMapLoc_ [n_poses][16]; returns the number of cells fused
    int64_t updateGlobal(const float* opt_poses, int n_poses)
    {
        check(mrs_gem_update_global(h_, opt_poses, n_poses), "mrs_gem_update_global");
        int64_t matched = 0;
        check(mrs_gem_stats(h_, &dropped_, &matched), "mrs_gem_stats");
        return matched;
    }
    int64_t dropped() const { return dropped_; }        // records the last updateGlobal left out for want of a key

    std::vector<ElevationCell> submap(int i) const
    {
        int64_t n = 0;
        check(mrs_gem_get_submap(h_, i, nullptr, nullptr, 0, &n, nullptr, nullptr), "mrs_gem_get_submap");
        std::vector<ElevationCell> out(static_cast<size_t>(n));
        if (n) check(mrs_gem_get_submap(h_, i, out.data(), nullptr, n, &n, nullptr, nullptr), "mrs_gem_get_submap");
        return out;
    }
    // composingGlobalMap: every submap in index order
    std::vector<ElevationCell> compose() const
    {
        int64_t n = 0;
        check(mrs_gem_compose(h_, nullptr, nullptr, 0, &n), "mrs_gem_compose");
        std::vector<ElevationCell> out(static_cast<size_t>(n));
        if (n) check(mrs_gem_compose(h_, out.data(), nullptr, n, &n), "mrs_gem_compose");
        return out;
    }
    // PointMapLayer::updateBounds over `cloud`: [size_y][size_x] costs; thresh_type 0 = traversability below thresh, 1 = elevation above it
    std::vector<uint8_t> costmap(const std::vector<ElevationCell>& cloud, double origin_x, double origin_y, int size_x, int size_y, double resolution,
                                 int thresh_type, double thresh) const
    {
        std::vector<uint8_t> grid(static_cast<size_t>(size_x) * static_cast<size_t>(size_y));
        check(mrs_gem_costmap(ctx_, cloud.empty() ? nullptr : cloud.data(), nullptr, static_cast<int64_t>(cloud.size()), origin_x, origin_y, size_x, size_y,
                              resolution, thresh_type, thresh, grid.data(), nullptr),
              "mrs_gem_costmap");
        return grid;
    }

private:
    static void check(int st, const char* what)
    {
        if (st != MRS_OK) throw std::runtime_error(std::string(what) + ": " + mrs_status_str(st) + ": " + mrs_last_error());
    }

    mrs_ctx* ctx_ = nullptr;
    mrs_gem* h_ = nullptr;
    int64_t dropped_ = 0;
};

}  // namespace mrslam
