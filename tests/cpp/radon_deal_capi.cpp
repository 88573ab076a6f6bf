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

// padded device images of a slot table (radon_deal::slot_images): returns their length in entries (0: the routine refused the table); each
// out_* holds `capacity` entries; slot_ray holds n_slot_ray entries
extern "C" int slot_images_c(const int* meta, const int* base, const float* q, const float* vm, const float* nrm, int rays, int stride, int wg,
                             int per_lane, const int* slot_ray, int n_slot_ray, int capacity, int* out_slot4, float* out_nrm, int* out_ray)
{
    const radon_deal::RayTable t = {meta, base, q, vm, rays, stride};
    const std::vector<int> table(slot_ray, slot_ray + n_slot_ray);
    const radon_deal::SlotImages im = radon_deal::slot_images(t, nrm, table, wg, per_lane);
    const int n = (int)im.ray.size();
    if (n > capacity || im.slot.size() != im.ray.size() || im.nrm.size() != im.ray.size()) return -n;
    memcpy(out_slot4, im.slot.data(), sizeof(radon_deal::SlotEntry) * (size_t)n);
    std::copy(im.nrm.begin(), im.nrm.end(), out_nrm);
    std::copy(im.ray.begin(), im.ray.end(), out_ray);
    return n;
}
