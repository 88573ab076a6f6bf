// C entry to mr_slam_amd/csrc/radon_deal.hpp for tests/test_radon_dealing.py (host compiler only, no HIP)
#include "radon_deal.hpp"

extern "C" int deal_rays_c(const int* meta, const int* base, const float* q, const float* vm, int rays, int stride, int wg, int per_lane,
                           int* out_table)
{
    const radon_deal::RayTable t = {meta, base, q, vm, rays, stride};
    const std::vector<int> table = radon_deal::deal_rays(t, wg, per_lane);
    std::copy(table.begin(), table.end(), out_table);
    return (int)table.size();
}
