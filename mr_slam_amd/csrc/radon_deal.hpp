// radon_deal.hpp -- which ray marches in which lane slot of the two-image Radon kernels (mrs_radon_plan::d_slot_ray).  Host code only, plain
// C++ (radon.hip calls it when a plan is built; tests/test_radon_dealing.py compiles it with the host compiler).
//
// march2 (radon_device.hpp) reads one 8-byte cell per tap and sample with ds_read_b64: the LDS serves the lanes 0-31 and 32-63 of a wave one
// after the other, 32 cell banks wide, equal cells broadcast, so a lane group pays per sample and tap the largest number of DISTINCT cells
// that fall on one bank (cell index mod 32).  Which 32 rays share a lane group is free: every ray is marched alone in its lane, and the
// sinogram is put back into ray order afterwards, so any table that holds every ray once gives the same bits.  The geometry does not depend
// on the images, so the assignment is searched once per plan against that cost model (tools/radon_order_sim.py is its numpy twin):
//   * rays of one orientation, sorted by step count, are cut into windows of similar length (kWindow steps, at least 64 rays, a multiple
//     of 32, at most kMaxWindow);
//   * inside a window P[i][j] counts the steps at which rays i and j sit on the same bank in different cells; lane groups of 32 are grown
//     from the free ray with the largest conflict sum by adding the free ray with the smallest sum against the group;
//   * a bounded refinement swaps rays between groups of a window while the true group cost (the per-step maximum) falls;
//   * groups are paired by length into wave-rounds of 64, and the wave-rounds are dealt to the 16 waves longest first, each to the wave
//     with the smallest step sum so far (slot s = k * 1024 + wave * 64 + lane), idle slots last.
// A wave-round never mixes the two orientations, except one that takes the shortest leftovers of both.  Everything is deterministic: stable
// sorts, first-index ties, no threads.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace radon_deal {

constexpr int kWave = 64;
constexpr int kGroup = 32;       // lanes the LDS serves together for ds_read_b64
constexpr int kBanks = 32;       // banks of 8-byte cells
constexpr int kWindow = 12;      // step counts inside a window differ by less than this
constexpr int kMaxWindow = 1024; // bounds the pairwise table (2 bytes per pair)
constexpr int kRefineSweeps = 4;    // passes of the swap refinement over a window's groups,
constexpr int kRefineTry = 8;       // ... pricing this many candidate swaps per group with the true cost

// ray table as mrs_radon_plan_create builds it: meta = n_steps | ydom << 16, base = byte offset of the first texel line (4-byte texels)
struct RayTable {
    const int* meta;
    const int* base;
    const float* q;
    const float* vm;
    int rays;
    int stride;   // texels per tile row
};

inline int steps_of(const RayTable& t, int r) { return t.meta[r] & 0xffff; }
inline int ydom_of(const RayTable& t, int r) { return t.meta[r] >> 16; }

// cell index of tap 0 at every step, with the arithmetic of march2: serial fp32 q += vm, (int)q
inline void ray_cells(const RayTable& t, int r, int* out)
{
    const int n = steps_of(t, r), yd = ydom_of(t, r), line = t.base[r] / 4;
    float q = t.q[r];
    const float vm = t.vm[r];
    for (int k = 0; k < n; ++k) {
        out[k] = yd ? line + k * t.stride + (int)q : line + k + (int)q * t.stride;
        q += vm;
    }
}

// ---- true cost of a lane group, kept per step so that "member i replaced by ray x" is cheap to price ----------------------------------
// One tap only: the second tap sits one cell (one row) further for every lane, which shifts every bank alike.
struct GroupState {
    int size = 0, nmax = 0, cost = 0;
    std::vector<int> member;          // window-local ray index per lane
    std::vector<int> cell;            // [nmax][kGroup] cell per step and lane, -1 = lane idle at that step
    std::vector<uint8_t> alone;       // [nmax][kGroup] 1 = no other lane reads this lane's cell at that step
    std::vector<uint8_t> cnt;         // [nmax][kBanks] distinct cells per bank
    std::vector<uint8_t> mx, at_mx;   // [nmax] their maximum = LDS cycles of the step; how many banks reach it
};

inline void group_build(GroupState& g, const std::vector<int>& member, const int* const* cells, const int* n, int nmax)
{
    g.size = (int)member.size(); g.nmax = nmax; g.member = member; g.cost = 0;
    g.cell.assign((size_t)nmax * kGroup, -1);
    g.alone.assign((size_t)nmax * kGroup, 0);
    g.cnt.assign((size_t)nmax * kBanks, 0);
    g.mx.assign(nmax, 0);
    g.at_mx.assign(nmax, 0);
    for (int s = 0; s < nmax; ++s) {
        int* c = g.cell.data() + (size_t)s * kGroup;
        uint8_t* alone = g.alone.data() + (size_t)s * kGroup;
        uint8_t* cnt = g.cnt.data() + (size_t)s * kBanks;
        for (int i = 0; i < g.size; ++i)
            if (s < n[member[i]]) c[i] = cells[member[i]][s];
        int mx = 0, at = 0, head[kBanks], next[kGroup];   // lanes chained per bank: a cell is compared with its bank's only
        for (int b = 0; b < kBanks; ++b) head[b] = -1;
        for (int i = 0; i < g.size; ++i) {
            if (c[i] < 0) continue;
            const int b = c[i] & (kBanks - 1);
            bool dup = false;
            for (int k = head[b]; k >= 0; k = next[k])
                if (c[k] == c[i]) { dup = true; alone[k] = 0; }
            alone[i] = !dup;
            if (!dup) ++cnt[b];
            next[i] = head[b];
            head[b] = i;
        }
        for (int b = 0; b < kBanks; ++b) {
            if (cnt[b] > mx) { mx = cnt[b]; at = 0; }
            at += cnt[b] == mx;
        }
        g.mx[s] = (uint8_t)mx;
        g.at_mx[s] = (uint8_t)at;
        g.cost += mx;
    }
}

// cost of the group with lane i marching ray x (cells xc[0..xn)) instead of its own
inline int group_replaced_cost(const GroupState& g, int i, const int* xc, int xn)
{
    int cost = 0;
    for (int s = 0; s < g.nmax; ++s) {
        const int* c = g.cell.data() + (size_t)s * kGroup;
        const int old = c[i], nw = s < xn ? xc[s] : -1;
        int m = g.mx[s];
        if (old != nw) {
            int same_new = 0;
            for (int k = 0; k < kGroup; ++k) same_new += c[k] == nw;
            const bool rem = old >= 0 && g.alone[(size_t)s * kGroup + i], add = nw >= 0 && same_new == 0;
            const int bo = old & (kBanks - 1), bn = nw & (kBanks - 1);
            const uint8_t* cnt = g.cnt.data() + (size_t)s * kBanks;
            if (!(rem && add && bo == bn)) {
                if (rem && cnt[bo] == m && g.at_mx[s] == 1) --m;   // the step's maximum falls only if no other bank holds it
                if (add) m = std::max(m, cnt[bn] + 1);
            }
        }
        cost += m;
    }
    return cost;
}

// by how many cycles the group gets cheaper when lane i goes idle, for every lane at once
inline void group_relief(const GroupState& g, int* relief)
{
    for (int i = 0; i < kGroup; ++i) relief[i] = 0;
    for (int s = 0; s < g.nmax; ++s) {
        if (g.at_mx[s] != 1) continue;
        const int* c = g.cell.data() + (size_t)s * kGroup;
        const uint8_t* alone = g.alone.data() + (size_t)s * kGroup;
        const uint8_t* cnt = g.cnt.data() + (size_t)s * kBanks;
        for (int i = 0; i < kGroup; ++i) relief[i] += (c[i] >= 0) & alone[i] & (cnt[c[i] & (kBanks - 1)] == g.mx[s]);
    }
}

// Swap refinement of one window's full groups.  Costliest group first: the member whose removal relieves it most is offered to every other
// group; the pairwise counts rank the rays it could be swapped for, the kRefineTry best are priced with the true cost of both groups, and
// the best swap is made if it lowers their sum.  Bounded: kRefineSweeps passes.
template <typename PT>
inline void refine_window(std::vector<std::vector<int>>& groups, size_t first, const int* const* cells, const int* n, int nmax, const PT* P, int m)
{
    std::vector<int> full;
    for (size_t g = first; g < groups.size(); ++g)
        if ((int)groups[g].size() == kGroup) full.push_back((int)g);
    const int G = (int)full.size();
    if (G < 2 || nmax > 255) return;
    std::vector<GroupState> st(G);
    std::vector<int> gid(m, -1), lane(m, 0), own(m, 0), to_w(m), from_wi(G);
    for (int g = 0; g < G; ++g) {
        group_build(st[g], groups[full[g]], cells, n, nmax);
        for (int i = 0; i < kGroup; ++i) { gid[st[g].member[i]] = g; lane[st[g].member[i]] = i; }
    }
    auto own_sum = [&](int x) {   // pairwise conflicts of ray x inside its own group
        const PT* row = P + (size_t)x * m;
        int v = 0;
        for (int k : st[gid[x]].member) v += row[k];
        return v;
    };
    for (int x = 0; x < m; ++x)
        if (gid[x] >= 0) own[x] = own_sum(x);
    for (int sweep = 0; sweep < kRefineSweeps; ++sweep) {
        std::vector<int> by_cost(G);
        for (int g = 0; g < G; ++g) by_cost[g] = g;
        std::stable_sort(by_cost.begin(), by_cost.end(), [&](int a, int b) { return st[a].cost > st[b].cost; });
        for (int gi : by_cost) {
            GroupState& gw = st[gi];
            int wi = 0, relief = 0, rel[kGroup];
            group_relief(gw, rel);
            for (int i = 0; i < kGroup; ++i)
                if (rel[i] > relief) { relief = rel[i]; wi = i; }
            if (relief <= 0) continue;
            const int wray = gw.member[wi];
            // pairwise price of swapping wray for x: what x meets in gw (without wray) + what wray meets in x's group (without x)
            std::fill(to_w.begin(), to_w.end(), 0);
            for (int k : gw.member) {
                if (k == wray) continue;
                const PT* row = P + (size_t)k * m;
                for (int x = 0; x < m; ++x) to_w[x] += row[x];
            }
            std::fill(from_wi.begin(), from_wi.end(), 0);
            const PT* wrow = P + (size_t)wray * m;
            for (int x = 0; x < m; ++x)
                if (gid[x] >= 0) from_wi[gid[x]] += wrow[x];
            int cand[kRefineTry], cval[kRefineTry], nc = 0;
            for (int x = 0; x < m; ++x) {
                if (gid[x] < 0 || gid[x] == gi) continue;
                const int d = (to_w[x] - own[wray]) + (from_wi[gid[x]] - wrow[x] - own[x]);
                if (d >= 0) continue;
                int at = nc < kRefineTry ? nc++ : (d < cval[kRefineTry - 1] ? kRefineTry - 1 : -1);
                if (at < 0) continue;
                while (at > 0 && cval[at - 1] > d) { cand[at] = cand[at - 1]; cval[at] = cval[at - 1]; --at; }
                cand[at] = x; cval[at] = d;
            }
            int best = 0, bx = -1;
            for (int c = 0; c < nc; ++c) {
                const int x = cand[c];
                const GroupState& gh = st[gid[x]];
                const int dw = group_replaced_cost(gw, wi, cells[x], n[x]) - gw.cost;
                if (dw >= best) continue;
                const int d = dw + group_replaced_cost(gh, lane[x], cells[wray], n[wray]) - gh.cost;
                if (d < best) { best = d; bx = x; }
            }
            if (bx < 0) continue;
            const int h = gid[bx], hj = lane[bx];
            std::vector<int> mw = gw.member, mh = st[h].member;
            std::swap(mw[wi], mh[hj]);
            group_build(gw, mw, cells, n, nmax);
            group_build(st[h], mh, cells, n, nmax);
            gid[bx] = gi; lane[bx] = wi; gid[wray] = h; lane[wray] = hj;
            for (int k : mw) own[k] = own_sum(k);
            for (int k : mh) own[k] = own_sum(k);
        }
    }
    for (int g = 0; g < G; ++g) groups[full[g]] = st[g].member;
}

// One window: rays w[0..m) (same orientation, similar length) -> lane groups of up to 32, appended to `groups`.
// PT: type of the pairwise counts (bytes while no ray has more than 255 steps)
template <typename PT>
inline void group_window(const int* const* ray_cells_of, const RayTable& t, const int* w, int m, std::vector<std::vector<int>>& groups)
{
    std::vector<const int*> cells(m);
    std::vector<int> n(m);
    int nmax = 0;
    for (int i = 0; i < m; ++i) {
        cells[i] = ray_cells_of[w[i]];
        n[i] = steps_of(t, w[i]);
        nmax = std::max(nmax, n[i]);
    }
    // P[i][j]: steps at which rays i and j meet on one bank in different cells.  Per step the live rays are bucketed by bank in index
    // order, so that the upper triangle fills row by row; it is mirrored afterwards
    std::vector<PT> P((size_t)m * m, 0);
    {
        std::vector<int> bid(m), bcell(m), start(kBanks + 1);
        for (int s = 0; s < nmax; ++s) {
            std::fill(start.begin(), start.end(), 0);
            for (int i = 0; i < m; ++i)
                if (s < n[i]) ++start[(cells[i][s] & (kBanks - 1)) + 1];
            for (int b = 0; b < kBanks; ++b) start[b + 1] += start[b];
            int fill[kBanks];
            for (int b = 0; b < kBanks; ++b) fill[b] = start[b];
            for (int i = 0; i < m; ++i)
                if (s < n[i]) {
                    const int c = cells[i][s], p = fill[c & (kBanks - 1)]++;
                    bid[p] = i; bcell[p] = c;
                }
            for (int b = 0; b < kBanks; ++b)
                for (int x = start[b]; x < start[b + 1]; ++x) {
                    PT* row = P.data() + (size_t)bid[x] * m;
                    const int c = bcell[x];
                    for (int y = x + 1; y < start[b + 1]; ++y) row[bid[y]] += (PT)(bcell[y] != c);
                }
        }
        constexpr int T = 64;
        for (int i0 = 0; i0 < m; i0 += T)
            for (int j0 = i0; j0 < m; j0 += T)
                for (int i = i0; i < std::min(i0 + T, m); ++i)
                    for (int j = std::max(j0, i + 1); j < std::min(j0 + T, m); ++j) P[(size_t)j * m + i] = P[(size_t)i * m + j];
    }
    std::vector<int> rs(m, 0);    // conflict sum against the rays still free
    for (int i = 0; i < m; ++i) {
        const PT* row = P.data() + (size_t)i * m;
        int s = 0;
        for (int j = 0; j < m; ++j) s += row[j];
        rs[i] = s;
    }
    constexpr int kTaken = 1 << 30;   // acc of a ray that is no longer free
    std::vector<char> free_(m, 1);
    std::vector<int> acc(m);
    int nfree = m;
    const size_t first = groups.size();
    while (nfree > 0) {
        int seed = -1;
        for (int i = 0; i < m; ++i)
            if (free_[i] && (seed < 0 || rs[i] > rs[seed])) seed = i;
        std::vector<int> grp(1, seed);
        std::fill(acc.begin(), acc.end(), 0);
        for (int i = 0; i < m; ++i)
            if (!free_[i]) acc[i] = kTaken;
        int last = seed;
        for (;;) {
            // `last` joins the group: it leaves the free rays' sums, its conflicts join the group's; the next member is the free ray
            // with the smallest sum against the group (first index on ties)
            const PT* row = P.data() + (size_t)last * m;
            free_[last] = 0; acc[last] = kTaken; --nfree;
            int best = -1, bv = kTaken;
            for (int i = 0; i < m; ++i) {
                const int p = row[i];
                rs[i] -= p;
                const int a = acc[i] + (acc[i] < kTaken ? p : 0);
                acc[i] = a;
                if (a < bv) { bv = a; best = i; }
            }
            if ((int)grp.size() == kGroup || nfree == 0) break;
            grp.push_back(best);
            last = best;
        }
        groups.push_back(grp);
    }
    refine_window(groups, first, cells.data(), n.data(), nmax, P.data(), m);
    for (size_t g = first; g < groups.size(); ++g)
        for (int& i : groups[g]) i = w[i];
}

// slot table [per_lane * wg]: ray id per lane slot s = k * wg + lane, -1 = idle.  wg: lanes of the workgroup (a multiple of 64).
inline std::vector<int> deal_rays(const RayTable& t, int wg, int per_lane)
{
    const int R = t.rays, waves = wg / kWave;
    std::vector<int> table((size_t)per_lane * wg, -1);
    // the order the plan used before: (orientation, step count, ray id)
    std::vector<int> sorted(R);
    for (int i = 0; i < R; ++i) sorted[i] = i;
    std::stable_sort(sorted.begin(), sorted.end(), [&](int a, int b) {
        const int ya = ydom_of(t, a), yb = ydom_of(t, b), na = steps_of(t, a), nb = steps_of(t, b);
        return ya != yb ? ya > yb : na > nb;
    });
    int nA = 0;
    while (nA < R && ydom_of(t, sorted[nA])) ++nA;
    const int nB = R - nA;
    // the shortest leftovers of both orientations share the one mixed wave-round
    const int la = nA % kWave, lb = la ? std::min(nB, kWave - la) : 0;
    std::vector<std::vector<int>> rounds;   // wave-rounds: up to 64 ray ids each
    std::vector<int> cellbuf;
    std::vector<const int*> cells_of(R, nullptr);
    {
        std::vector<size_t> at(R + 1, 0);
        for (int r = 0; r < R; ++r) at[r + 1] = at[r] + steps_of(t, r);
        cellbuf.resize(at[R] + 1);
        for (int r = 0; r < R; ++r) {
            cells_of[r] = cellbuf.data() + at[r];
            ray_cells(t, r, cellbuf.data() + at[r]);
        }
    }
    auto deal_region = [&](int lo, int hi) {   // sorted[lo, hi): one orientation, longest first
        const int size = hi - lo;
        if (size <= 0) return;
        std::vector<int> asc(sorted.begin() + lo, sorted.begin() + hi);
        std::stable_sort(asc.begin(), asc.end(), [&](int a, int b) { return steps_of(t, a) < steps_of(t, b); });
        std::vector<std::vector<int>> groups;
        int pos = 0;
        while (pos < size) {
            const int n0 = steps_of(t, asc[pos]);
            int end = pos;
            while (end < size && (steps_of(t, asc[end]) < n0 + kWindow || end - pos < kWave)) ++end;
            int m = (end - pos) / kGroup * kGroup;
            if (size - end < kGroup) m = size - pos;
            m = std::min(m, kMaxWindow);
            if (m < kWave) {   // too few rays to choose from: the previous order
                for (int i = 0; i < m; i += kGroup) groups.emplace_back(asc.begin() + pos + i, asc.begin() + pos + std::min(i + kGroup, m));
            } else {
                int nmax = 0;
                for (int i = 0; i < m; ++i) nmax = std::max(nmax, steps_of(t, asc[pos + i]));
                if (nmax < 256) group_window<uint8_t>(cells_of.data(), t, asc.data() + pos, m, groups);
                else group_window<uint16_t>(cells_of.data(), t, asc.data() + pos, m, groups);
            }
            pos += m;
        }
        // pair the groups by length: full groups longest first, a partial group last
        std::vector<int> gmax(groups.size()), idx(groups.size());
        for (size_t g = 0; g < groups.size(); ++g) {
            idx[g] = (int)g;
            int mx = 0;
            for (int r : groups[g]) mx = std::max(mx, steps_of(t, r));
            gmax[g] = mx;
        }
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
            const bool fa = (int)groups[a].size() == kGroup, fb = (int)groups[b].size() == kGroup;
            return fa != fb ? fa : gmax[a] > gmax[b];
        });
        std::vector<int> cur;
        for (int g : idx) {
            if ((int)cur.size() + (int)groups[g].size() > kWave) { rounds.push_back(cur); cur.clear(); }
            cur.insert(cur.end(), groups[g].begin(), groups[g].end());
            if ((int)cur.size() == kWave) { rounds.push_back(cur); cur.clear(); }
        }
        if (!cur.empty()) rounds.push_back(cur);
    };
    deal_region(0, nA - la);
    deal_region(nA, R - lb);
    if (la) {
        std::vector<int> mixed(sorted.begin() + (nA - la), sorted.begin() + nA);
        mixed.insert(mixed.end(), sorted.begin() + (R - lb), sorted.end());
        rounds.push_back(mixed);
    }
    if ((int)rounds.size() > waves * per_lane) {   // cannot happen for per_lane = ceil(rays / wg); keep the previous order if it does
        std::copy(sorted.begin(), sorted.end(), table.begin());
        return table;
    }
    // wave-rounds to waves: longest first, each to the wave with the smallest step sum that still has a free round
    std::vector<int> cost(rounds.size()), idx(rounds.size());
    for (size_t i = 0; i < rounds.size(); ++i) {
        int mx[2] = {0, 0};
        for (int r : rounds[i]) mx[ydom_of(t, r)] = std::max(mx[ydom_of(t, r)], steps_of(t, r));
        cost[i] = mx[0] + mx[1];
        idx[i] = (int)i;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
        const bool fa = (int)rounds[a].size() == kWave, fb = (int)rounds[b].size() == kWave;
        return fa != fb ? fa : cost[a] > cost[b];
    });
    std::vector<long> load(waves, 0);
    std::vector<int> used(waves, 0);
    for (int i : idx) {
        int w = -1;
        for (int v = 0; v < waves; ++v)
            if (used[v] < per_lane && (w < 0 || load[v] < load[w])) w = v;
        int* dst = table.data() + (size_t)used[w] * wg + (size_t)w * kWave;
        std::copy(rounds[i].begin(), rounds[i].end(), dst);
        load[w] += cost[i];
        ++used[w];
    }
    return table;
}

// ---- device images of the slot table -------------------------------------------------------------------------------------------------
// The slot-table kernels (k_bev_radon3, fused.hip) are instantiated for 15 or 16 rays per lane and walk ALL of those lane slots, whatever
// the plan's own ceil(rays / wg) is: the tables they read are padded to that length with idle entries (ray -1, norm 0, a zero slot), which
// the kernels' `ray >= 0` test skips.
inline int walked_per_lane(int per_lane) { return per_lane <= 15 ? 15 : 16; }

struct SlotEntry { int meta, base, q_bits, vm_bits; };   // the int4 the kernel loads: {n_steps | ydom << 16, byte offset, q bits, vm bits}
static_assert(sizeof(SlotEntry) == 16, "SlotEntry is uploaded as int4");

struct SlotImages {
    std::vector<SlotEntry> slot;
    std::vector<float> nrm;
    std::vector<int> ray;
};

// slot_ray: deal_rays' table [per_lane * wg]; nrm: step length per ray.  Every image has walked_per_lane(per_lane) * wg entries; a table
// of any other length than per_lane * wg is an error: the images come back empty.
inline SlotImages slot_images(const RayTable& t, const float* nrm, const std::vector<int>& slot_ray, int wg, int per_lane)
{
    const size_t dealt = (size_t)per_lane * wg, padded = (size_t)walked_per_lane(per_lane) * wg;
    SlotImages im;
    if (slot_ray.size() != dealt) return im;
    im.slot.assign(padded, SlotEntry{0, 0, 0, 0});
    im.nrm.assign(padded, 0.0f);
    im.ray.assign(padded, -1);
    for (size_t i = 0; i < dealt; ++i) {
        const int r = slot_ray[i];
        if (r < 0) continue;
        int qb, vb;
        memcpy(&qb, &t.q[r], 4); memcpy(&vb, &t.vm[r], 4);
        im.slot[i] = SlotEntry{t.meta[r], t.base[r], qb, vb};
        im.nrm[i] = nrm[r];
        im.ray[i] = r;
    }
    return im;
}

}  // namespace radon_deal
