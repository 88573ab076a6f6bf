// pcm.hip -- pairwise consistency of the inter-robot loops of one robot pair (C ABI mrs_pcm_*).
//
// What it replaces: global_map::GlobalMap::pairwiseConsistencyMaximization (pairwise_consistency_maximization/global_map/global_map.cpp:
// 35-61), run for every robot pair before every optimisation (global_manager.cpp:1301-1310): L (L - 1) / 2 consistency evaluations on one
// host thread (pairwise_consistency.cpp:40-97), a Matrix-Market file written and read back, and FMC::maxCliqueHeu (findCliqueHeu.cpp:
// 120-243), whose intersection step is a doubly nested linear search from every start vertex.  Here:
//   records : k_pcm_records, a thread per new loop: P = XA_i Z XB_k^-1 and B = XB_k (pcm_pose.hpp), so that a pair costs one product, one
//             conjugation and one Logmap;
//   rows    : k_pcm_rows, the consistency matrix as bit rows of `words` 64-bit words.  A wave computes 64 columns of one row, a lane
//             evaluates one pair, the wave ballot is the word and lane 0 stores it.  No atomics and no sums across lanes: a bit depends
//             on its two loops only, whatever the launch.  Both triangles are written (pair (u, v) is always evaluated as (min, max)), so
//             a row read of the clique kernel is contiguous.  Appending launches only the (row, word) tiles that touch a new row or column;
//   degrees : k_pcm_degrees, a popcount per row;
//   clique  : the start vertices of the heuristic interact only through the running best size, which never decreases.  A round evaluates
//             every remaining start under the current best size (k_pcm_greedy, a wave per start; the candidate set is one 64-bit word per
//             lane; a step is a ballot of the non-empty lanes, the highest lane, a count of leading zeros, and one coalesced row load) and
//             the lowest start that improves is adopted (a 64-bit atomicMin on start << 32 | size: a minimum does not depend on the order of
//             arrival).  Starts below it were evaluated exactly as the sequential heuristic would; those above it are evaluated again in the
//             next round.  Every round but the last raises the best size, so there are at most size + 1 of them.  The member list comes
//             from running the last winner again in one wave.
//   covariances : after mrs_pcm_set_covariances the records and rows come from k_pcm_records_cov / k_pcm_rows_cov (pcm_cov.hpp, DESIGN.md
//             4.24): the same tiling, the squared Mahalanobis distance of the cycle pose under the covariance propagated around the cycle,
//             from per-pose world-frame prefixes built once on the host.  A handle without covariances runs the kernels above, untouched.
#include "common.hpp"
#include "pcm_pose.hpp"
#include "pcm_cov.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using u64 = unsigned long long;
constexpr int kMaxLoops = MRS_PCM_MAX_LOOPS;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRec = mrs::pcm::kRecord;
constexpr int kRecCov = mrs::pcm::kCovRecord, kSym = mrs::pcm::kSym;
constexpr u64 kNoWinner = ~0ull;
static_assert(kMaxLoops == 64 * 64, "the candidate set of k_pcm_greedy is one 64-bit word per lane");

// rec [first + t] for the n new loops: ia / kb / Z are the new loops only
__global__ __launch_bounds__(kThreads) void k_pcm_records(const double* __restrict__ XA, const double* __restrict__ XB, const int* __restrict__ ia,
                                                          const int* __restrict__ kb, const double* __restrict__ Z, int n, int first,
                                                          double* __restrict__ rec)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    double r[kRec];
    mrs::pcm::loop_record(XA + (size_t)ia[t] * 16, Z + (size_t)t * 16, XB + (size_t)kb[t] * 16, r);
#pragma unroll
    for (int i = 0; i < kRec; ++i) rec[(size_t)(first + t) * kRec + i] = r[i];
}

__device__ __forceinline__ double pair_distance_of(const double* __restrict__ rec, int u, int v)
{
    const int a = min(u, v), b = max(u, v);
    double ra[kRec], rb[mrs::pcm::kPose];
#pragma unroll
    for (int i = 0; i < kRec; ++i) ra[i] = rec[(size_t)a * kRec + i];
#pragma unroll
    for (int i = 0; i < mrs::pcm::kPose; ++i) rb[i] = rec[(size_t)b * kRec + i];
    return mrs::pcm::pair_distance(ra, rb);
}

// the words [word0, word0 + nwords) of the rows [row0, row0 + nrows): a wave per (row, word)
__global__ __launch_bounds__(kThreads) void k_pcm_rows(const double* __restrict__ rec, int L, double threshold, int row0, int nrows, int word0,
                                                       int nwords, int words, u64* __restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (tile >= (long long)nrows * nwords) return;               // the same for a whole wave
    const int u = row0 + (int)(tile / nwords), w = word0 + (int)(tile % nwords);
    const int v = 64 * w + lane;
    bool bit = false;
    if (v < L && v != u) bit = pair_distance_of(rec, u, v) < threshold;      // false for a distance that is not a number
    const u64 word = __ballot(bit);
    if (lane == 0) rows[(size_t)u * words + w] = word;
}

// ---- the covariance instantiations: the same tiling, a record of kRecCov doubles and the two prefix tables
__global__ __launch_bounds__(kThreads) void k_pcm_records_cov(const double* __restrict__ XA, const double* __restrict__ XB,
                                                              const int* __restrict__ ia, const int* __restrict__ kb, const double* __restrict__ Z,
                                                              const double* __restrict__ Csym, int n, int first, double* __restrict__ rec)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    double r[kRecCov], c[kSym];
#pragma unroll
    for (int e = 0; e < kSym; ++e) c[e] = Csym[(size_t)t * kSym + e];
    mrs::pcm::loop_record_cov(XA + (size_t)ia[t] * 16, Z + (size_t)t * 16, XB + (size_t)kb[t] * 16, c, ia[t], kb[t], r);
#pragma unroll
    for (int i = 0; i < kRecCov; ++i) rec[(size_t)(first + t) * kRecCov + i] = r[i];
}

// the squared Mahalanobis distance of the pair, always evaluated as (min, max); the records and tables are read where they lie
__device__ __forceinline__ double pair_mahalanobis2_of(const double* __restrict__ rec, const double* __restrict__ WA, const double* __restrict__ WB,
                                                       int mode, int u, int v)
{
    const int a = min(u, v), b = max(u, v);
    return mrs::pcm::pair_mahalanobis2(rec + (size_t)a * kRecCov, rec + (size_t)b * kRecCov, WA, WB, mode);
}

__global__ __launch_bounds__(kThreads) void k_pcm_rows_cov(const double* __restrict__ rec, const double* __restrict__ WA,
                                                           const double* __restrict__ WB, int mode, int L, double threshold, int row0, int nrows,
                                                           int word0, int nwords, int words, u64* __restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (tile >= (long long)nrows * nwords) return;               // the same for a whole wave
    const int u = row0 + (int)(tile / nwords), w = word0 + (int)(tile % nwords);
    const int v = 64 * w + lane;
    bool bit = false;
    if (v < L && v != u) bit = pair_mahalanobis2_of(rec, WA, WB, mode, u, v) < threshold;      // false for NaN
    const u64 word = __ballot(bit);
    if (lane == 0) rows[(size_t)u * words + w] = word;
}

__global__ __launch_bounds__(kThreads) void k_pcm_distances_cov(const double* __restrict__ rec, const double* __restrict__ WA,
                                                                const double* __restrict__ WB, int mode, int L, double* __restrict__ d)
{
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (long long)L * L) return;
    const int u = (int)(e / L), v = (int)(e % L);
    d[e] = u == v ? 0.0 : pair_mahalanobis2_of(rec, WA, WB, mode, u, v);
}

// d [L][L], a thread per entry
__global__ __launch_bounds__(kThreads) void k_pcm_distances(const double* __restrict__ rec, int L, double* __restrict__ d)
{
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (long long)L * L) return;
    const int u = (int)(e / L), v = (int)(e % L);
    d[e] = u == v ? 0.0 : pair_distance_of(rec, u, v);
}

// a wave per row
__global__ __launch_bounds__(kThreads) void k_pcm_degrees(const u64* __restrict__ rows, int L, int words, int* __restrict__ deg)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (u >= L) return;
    int c = lane < words ? __popcll(rows[(size_t)u * words + lane]) : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) deg[u] = c;
}

// elig [64]: the vertices whose degree is at least max_clq, as bit words; one workgroup.  Also resets the round's winner word.
__global__ __launch_bounds__(kThreads) void k_pcm_eligible(const int* __restrict__ deg, int L, int max_clq, u64* __restrict__ elig, u64* __restrict__ winner)
{
    const int lane = threadIdx.x & 63;
    for (int w = threadIdx.x >> 6; w < 64; w += kWaves) {
        const int v = 64 * w + lane;
        const u64 word = __ballot(v < L && deg[v] >= max_clq);
        if (lane == 0) elig[w] = word;
    }
    if (threadIdx.x == 0) *winner = kNoWinner;
}

// One greedy chain per start vertex c in [start, end), a wave each, under the fixed best size max_clq (findCliqueHeu.cpp:143-239): c stays
// in the reference's list S to the end, so the chain is T = N(c) & E; while T is not empty: m = its highest vertex, T &= N(m); its size is
// 1 + the number of steps and its members are c, m1, m2, ...  E needs no second application: max_clq does not change within a chain.
// With `list` (end == start + 1) the members are written out; otherwise an improving chain competes for the lowest start.
__global__ __launch_bounds__(kThreads) void k_pcm_greedy(const u64* __restrict__ rows, const int* __restrict__ deg, const u64* __restrict__ elig,
                                                         int words, int start, int end, int max_clq, u64* __restrict__ winner, int* __restrict__ list)
{
    const int lane = threadIdx.x & 63, c = start + blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (c >= end) return;
    if (max_clq > deg[c]) return;                                // Pruning 1
    u64 T = lane < words ? rows[(size_t)c * words + lane] & elig[lane] : 0ull;
    int icc = 1;
    if (list && lane == 0) list[0] = c;
    // every step clears at least the bit of m (the diagonal is zero), so the loop ends after at most L steps; the bound is a second fence
    for (int step = 0; step < kMaxLoops - 1; ++step) {          // c and at most kMaxLoops - 1 others: list[] holds kMaxLoops
        const u64 lanes = __ballot(T != 0ull);
        if (!lanes) break;
        const int hi = 63 - __clzll((long long)lanes);
        const unsigned lo32 = (unsigned)__shfl((int)(unsigned)T, hi, 64), hi32 = (unsigned)__shfl((int)(unsigned)(T >> 32), hi, 64);
        const u64 word = ((u64)hi32 << 32) | lo32;
        const int m = 64 * hi + 63 - __clzll((long long)word);   // hi < words, so m < 64 words <= the rows allocated
        if (list && lane == 0) list[icc] = m;
        ++icc;
        T &= lane < words ? rows[(size_t)m * words + lane] : 0ull;
    }
    if (!list && lane == 0 && icc > max_clq) atomicMin(winner, ((u64)(unsigned)c << 32) | (unsigned)icc);
}

// ------------------------------------------------------------------ the exact maximum clique (mrs_pcm_solve_exact)
//   seed    : the heuristic's size is the first incumbent;
//   shrink  : k_pcm_peel, the k-core of the bit rows: a vertex with fewer than `need_deg` living neighbours dies, until nothing changes
//             (the k-core is unique, so neither the order of the removals nor a stale read of `alive` changes the result);
//   search  : k_pcm_exact, a wave per slot and a subproblem per top vertex c (c and its living smaller neighbours), handed out from L - 1
//             down by a ticket counter.  Within a subproblem the depth-first search is strictly descending: a level holds its candidate
//             set P (a 64-bit word per lane), the branch vertex is the highest of P (a ballot and two counts of leading zeros), and taking
//             it is one coalesced row load and an AND.  A level is left when it is empty, when its size bound fails (d + |P| < need), or
//             when its highest vertex lies below the level's colouring cut.  Phase 1 looks for a clique larger than the shared incumbent
//             (need = best + 1, best rises by atomicMax: a hint that only tightens pruning), phase 2 for the first clique of the proven size
//             omega in every subproblem (need = omega); the winner of phase 2 is the highest top vertex that finds one (atomicMax), which
//             does not depend on the order of arrival.
//   colour  : greedy sequential colouring of P in ASCENDING vertex order, class by class on the bit words.  A vertex of colour k has a
//             neighbour of every lower colour below it, and P below any vertex m is properly coloured by the colours handed out so far.
//             With k0 = need - d, only the classes 1 .. k0 - 1 are built: the lowest vertex they leave uncoloured is the cut, and a branch
//             on any m below it cannot reach `need` (its candidates have k0 - 1 colours at most, itself included).  One colouring per level,
//             not per child, and it keeps the descending order phase 2 needs.
//   launches: a wave takes at most kExactSteps steps (vertices taken, levels left, vertices coloured, tickets) per launch and then stores
//             its level; everything below is already in its stack, so that the host re-launches until no slot has work or the node budget
//             is spent.  No wave waits for another.
constexpr int kExactWaves = MRS_PCM_EXACT_MAX_WAVES, kExactSteps = MRS_PCM_EXACT_LAUNCH_NODES;
constexpr int kIdle = -1, kRetired = -2, kFound = -3, kCutUnset = -1;
constexpr size_t kExactStackBytes = (size_t)64 << 20;          // cap of all slots' stacks together; the number of slots follows from it
static_assert((long long)kExactWaves * kExactSteps == MRS_PCM_EXACT_OVERSHOOT, "the overshoot is concurrent waves x the per-launch cap");
static_assert(kExactWaves < (1 << 16),"the winner word of phase 2 is (top + 1) << 16 | slot");

struct ExactStatus {
    u64 nodes;          // vertices taken into a clique so far, both phases
    int active;         // slots that still have work after this launch
    int best;           // the incumbent's size
    unsigned winner;    // phase 2: (top vertex + 1) << 16 | slot of the highest top vertex that found a clique of size omega; 0 = none
    int ticket;         // the next subproblem is the top vertex L - 1 - ticket
    int pad[2];
};

__device__ __forceinline__ u64 shfl64(u64 x, int src)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)x, src, 64), hi = (unsigned)__shfl((int)(unsigned)(x >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ int wave_sum(int c)
{
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
}

// a wave per vertex: dies if fewer than need_deg of its neighbours are alive
__global__ __launch_bounds__(kThreads) void k_pcm_peel(const u64* __restrict__ rows, int L, int words, int need_deg, u64* alive, int* changed)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (u >= L) return;
    if (!((alive[u >> 6] >> (u & 63)) & 1ull)) return;
    const int c = wave_sum(lane < words ? __popcll(rows[(size_t)u * words + lane] & alive[lane]) : 0);
    if (lane == 0 && c < need_deg) {
        atomicAnd(&alive[u >> 6], ~(1ull << (u & 63)));
        *changed = 1;
    }
}

// deg [L]: the living neighbours of a living vertex, 0 for a dead one; a wave per vertex
__global__ __launch_bounds__(kThreads) void k_pcm_alive_degrees(const u64* __restrict__ rows, const u64* __restrict__ alive, int L, int words,
                                                                int* __restrict__ deg)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (u >= L) return;
    const bool lives = (alive[u >> 6] >> (u & 63)) & 1ull;
    const int c = wave_sum(lane < words && lives ? __popcll(rows[(size_t)u * words + lane] & alive[lane]) : 0);
    if (lane == 0) deg[u] = c;
}

// One launch of the search: see above.  Per slot: top [1] (the top vertex, or kIdle / kRetired / kFound), depth [1], and maxd + 1 levels of
// path / cut / stack (level d holds the candidates of the clique path [0, d)); phase 1 also keeps the largest clique the slot has found
// (best_size, best_list).  A slot's state is written and read by lane-matched accesses of its own wave only.
__global__ __launch_bounds__(kThreads) void k_pcm_exact(const u64* __restrict__ rows, const u64* __restrict__ alive, int L, int words, int maxd,
                                                        int nslots, int phase, int omega, ExactStatus* st, int* s_top, int* s_depth, int* path,
                                                        int* cut, u64* stack, int* s_best, int* best_list)
{
    const int lane = threadIdx.x & 63, slot = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (slot >= nslots) return;
    int v = s_top[slot];
    if (v == kRetired || v == kFound) return;
    int* mypath = path + (size_t)slot * (maxd + 1);
    int* mycut = cut + (size_t)slot * (maxd + 1);
    int* mybest = best_list + (size_t)slot * (maxd + 1);
    u64* mystack = stack + (size_t)slot * (maxd + 1) * words;
    const u64 A = lane < words ? alive[lane] : 0ull;
    int d = 0, cutv = kCutUnset;
    u64 P = 0ull;
    if (v >= 0) {
        d = s_depth[slot];                                       // 1 .. maxd, as stored below
        P = lane < words ? mystack[(size_t)d * words + lane] : 0ull;
        cutv = __shfl(lane == 0 ? mycut[d] : 0, 0, 64);
    }
    int need = phase == 1 ? __hip_atomic_load(&st->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 : omega;
    int win_top = -1;                                            // phase 2: the highest top vertex known to have found its clique
    unsigned nodes = 0;
    int tick = 0;
    for (int step = 0; step < kExactSteps; ++step) {
        if ((++tick & 15) == 0) {
            if (phase == 1) {
                need = __hip_atomic_load(&st->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
            } else {
                win_top = (int)(__hip_atomic_load(&st->winner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 16) - 1;
                if (v >= 0 && win_top > v) v = kIdle;            // a higher top vertex has won: this subproblem no longer matters
            }
        }
        if (v < 0) {                                             // take the next subproblem
            int t = 0;
            if (lane == 0) t = atomicAdd(&st->ticket, 1);
            t = __shfl(t, 0, 64);
            const int c = L - 1 - t;
            if (c < 0 || c < win_top) {                          // tickets only go down from here
                v = kRetired;
                break;
            }
            if (!((alive[c >> 6] >> (c & 63)) & 1ull)) continue;
            const int w = c >> 6;
            const u64 below = lane < w ? ~0ull : lane == w ? (1ull << (c & 63)) - 1ull : 0ull;
            v = c;
            d = 1;
            P = (lane < words ? rows[(size_t)c * words + lane] : 0ull) & A & below;
            cutv = kCutUnset;
            if (lane == 0) mypath[0] = c;
            ++nodes;
            continue;
        }
        // level d: the clique path [0, d) and its candidates P, all of them below path [d - 1]
        const u64 lanes = __ballot(P != 0ull);
        bool leave = false;
        int hi = 0, m = 0;
        if (!lanes) {                                            // nothing extends the clique: it has d members
            if (d >= need) {
                if (phase == 1) {
                    if (lane == 0) {
                        atomicMax(&st->best, d);
                        if (d > s_best[slot]) {
                            s_best[slot] = d;
                            for (int i = 0; i < kMaxLoops; ++i) {    // d <= maxd: lane 0 wrote the path, lane 0 copies it
                                if (i >= d) break;
                                mybest[i] = mypath[i];
                            }
                        }
                    }
                    need = d + 1;
                } else {
                    if (lane == 0) {
                        s_depth[slot] = d;
                        atomicMax(&st->winner, ((unsigned)(v + 1) << 16) | (unsigned)slot);
                    }
                    v = kFound;                                  // the path stays in the slot for the host
                    break;
                }
            }
            leave = true;
        } else if (d + wave_sum(__popcll(P)) < need || d >= maxd) {     // the size bound; d >= maxd cannot happen with candidates left: a fence
            leave = true;
        } else {
            if (cutv == kCutUnset) {                             // colour the level once
                const int k0 = need - d;
                cutv = 0;
                if (k0 > 1) {
                    u64 U = P;
                    for (int k = 1; k < kMaxLoops + 1; ++k) {
                        if (k >= k0 || !__ballot(U != 0ull)) break;
                        u64 Q = U;
                        for (int i = 0; i < kMaxLoops; ++i) {    // every pass colours one vertex
                            const u64 ql = __ballot(Q != 0ull);
                            if (!ql) break;
                            const int lo = __ffsll((long long)ql) - 1;
                            const int b = __ffsll((long long)shfl64(Q, lo)) - 1;
                            const int x = 64 * lo + b;           // a bit of P: a living vertex, so x < L <= the rows allocated
                            if (lane == lo) {
                                U &= ~(1ull << b);
                                Q &= ~(1ull << b);
                            }
                            Q &= ~(lane < words ? rows[(size_t)x * words + lane] : 0ull);
                            ++step;
                        }
                    }
                    const u64 ul = __ballot(U != 0ull);
                    const int lo = ul ? __ffsll((long long)ul) - 1 : 0;
                    const u64 word = shfl64(U, lo);
                    cutv = ul ? 64 * lo + __ffsll((long long)word) - 1 : kMaxLoops;      // nothing left: no branch of this level can reach `need`
                }
            }
            hi = 63 - __clzll((long long)lanes);
            m = 64 * hi + 63 - __clzll((long long)shfl64(P, hi));    // a bit of P: a living vertex, so m < L <= the rows allocated
            leave = m < cutv;
        }
        if (leave) {
            if (--d == 0) {
                v = kIdle;
                continue;
            }
            P = lane < words ? mystack[(size_t)d * words + lane] : 0ull;
            cutv = __shfl(lane == 0 ? mycut[d] : 0, 0, 64);
            continue;
        }
        // take m: what stays of this level goes to the stack, the next level is P & N(m); here 1 <= d < maxd
        if (lane == hi) P &= ~(1ull << (m & 63));
        if (lane < words) mystack[(size_t)d * words + lane] = P;
        if (lane == 0) {
            mycut[d] = cutv;
            mypath[d] = m;
        }
        P &= lane < words ? rows[(size_t)m * words + lane] : 0ull;
        ++d;
        cutv = kCutUnset;
        ++nodes;
    }
    if (v >= 0 && lane < words) mystack[(size_t)d * words + lane] = P;      // 1 <= d <= maxd: the stack has maxd + 1 levels
    if (lane == 0) {
        s_top[slot] = v;
        if (v >= 0) {
            s_depth[slot] = d;
            mycut[d] = cutv;
        }
        if (v >= 0 || v == kIdle) atomicAdd(&st->active, 1);
        if (nodes) atomicAdd(&st->nodes, (u64)nodes);
    }
}

inline unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

struct mrs_pcm {
    mrs_ctx* ctx = nullptr;
    int capacity = 0, words = 0;             // words per bit row: ceil(capacity / 64)
    double threshold = 0.0;
    int na = 0, nb = 0, L = 0;
    bool given_matrix = false;               // the vertices came from mrs_pcm_set_matrix: no records behind them
    bool degrees_stale = true;
    mrs::DeviceBuffer<double> XA, XB, rec;
    // covariances (mrs_pcm_set_covariances): the mode, the host poses the prefixes are built from, the per-pose prefix
    // tables on both sides (the host side serves mrs_pcm_get_pair) and the wider records
    int cov_mode = MRS_PCM_COV_NONE;
    std::vector<double> h_XA, h_XB, h_WA, h_WB;
    mrs::DeviceBuffer<double> WA, WB, rec_cov;
    mrs::DeviceBuffer<u64> rows, elig, winner;
    mrs::DeviceBuffer<int> deg, list;
    // mrs_pcm_solve_exact only, allocated by its first call and sized by the matrix it met (ExactLayout)
    mrs::DeviceBuffer<u64> x_alive, x_stack;
    mrs::DeviceBuffer<int> x_ints;
    mrs::DeviceBuffer<ExactStatus> x_status;
    int64_t x_launches = 0;                  // launches of k_pcm_exact in the last mrs_pcm_solve_exact
};

namespace {

int pcm_clear(mrs_pcm* p)
{
    p->L = 0;
    p->given_matrix = false;
    p->degrees_stale = true;
    MRS_HIP_TRY(hipMemsetAsync(p->rows.get(), 0, (size_t)p->capacity * p->words * sizeof(u64), nullptr));
    return MRS_OK;
}

// the tiles of the matrix that touch the loops [L0, L1): the new rows whole, and of the old rows the words from L0 / 64 on
int pcm_fill_rows(mrs_pcm* p, int L0, int L1)
{
    const int nw = (L1 + 63) / 64;
    const int w0 = L0 / 64;
    if (p->cov_mode != MRS_PCM_COV_NONE) {
        hipLaunchKernelGGL(k_pcm_rows_cov, dim3(blocks_for((long long)(L1 - L0) * nw, kWaves)), dim3(kThreads), 0, nullptr, p->rec_cov.get(),
                           p->WA.get(), p->WB.get(), p->cov_mode, L1, p->threshold, L0, L1 - L0, 0, nw, p->words, p->rows.get());
        if (L0 > 0)
            hipLaunchKernelGGL(k_pcm_rows_cov, dim3(blocks_for((long long)L0 * (nw - w0), kWaves)), dim3(kThreads), 0, nullptr, p->rec_cov.get(),
                               p->WA.get(), p->WB.get(), p->cov_mode, L1, p->threshold, 0, L0, w0, nw - w0, p->words, p->rows.get());
        MRS_HIP_TRY(hipGetLastError());
        return MRS_OK;
    }
    hipLaunchKernelGGL(k_pcm_rows, dim3(blocks_for((long long)(L1 - L0) * nw, kWaves)), dim3(kThreads), 0, nullptr, p->rec.get(), L1, p->threshold,
                       L0, L1 - L0, 0, nw, p->words, p->rows.get());
    if (L0 > 0)
        hipLaunchKernelGGL(k_pcm_rows, dim3(blocks_for((long long)L0 * (nw - w0), kWaves)), dim3(kThreads), 0, nullptr, p->rec.get(), L1,
                           p->threshold, 0, L0, w0, nw - w0, p->words, p->rows.get());
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

// ---- host side of the covariances
// [n][6][6] lower triangles (nullptr: FIXED_COVARIANCE each) -> [n][21]; false when one is not finite or not positive definite
bool pcm_sym_inputs(const double* h, size_t n, std::vector<double>* out)
{
    out->resize(n * kSym);
    for (size_t e = 0; e < n; ++e) {
        double* s = out->data() + e * kSym;
        if (!h) {
            mrs::pcm::sym_fixed(s);
            continue;
        }
        mrs::pcm::sym_from_lower(h + e * 36, s);
        if (!mrs::pcm::sym_is_pd(s)) return false;
    }
    return true;
}

// the world-frame prefixes of one trajectory: W_0 = base, W_m+1 = W_m + Ad(X_m+1) Q_m Ad(X_m+1)^T, in sequence
void pcm_prefixes(const std::vector<double>& X, int n, const std::vector<double>& Q, const double* base, std::vector<double>* W)
{
    W->assign((size_t)n * kSym, 0.0);
    mrs::pcm::prefix_table(X.data(), n, Q.data(), base, W->data());
}

// ---- host side of the exact search
// the slots of k_pcm_exact: `ints` holds top | depth | best size [nslots] and path | cut | best list [nslots][maxd + 1]
struct ExactLayout {
    int nslots = 0, maxd = 0;
    int *top = nullptr, *depth = nullptr, *best = nullptr, *path = nullptr, *cut = nullptr, *best_list = nullptr;
};

// maxd: an upper bound on the size of any clique the phase can hold.  The stacks take (maxd + 1) * words words per slot, kExactStackBytes
// in all at most, and the number of slots follows from that.
int pcm_exact_layout(mrs_pcm* p, int maxd, ExactLayout* lay)
{
    const size_t level = (size_t)(maxd + 1), per_slot = level * p->words;
    size_t n = kExactStackBytes / (per_slot * sizeof(u64));
    n = std::min<size_t>(std::min<size_t>(std::max<size_t>(n, 1), kExactWaves), (size_t)p->L);
    MRS_TRY(p->x_stack.reserve(n * per_slot, n * per_slot));
    const size_t ints = 3 * n + 3 * n * level;
    MRS_TRY(p->x_ints.reserve(ints, ints));
    MRS_TRY(p->x_status.reserve(1, 1));
    lay->nslots = (int)n;
    lay->maxd = maxd;
    lay->top = p->x_ints.get();
    lay->depth = lay->top + n;
    lay->best = lay->depth + n;
    lay->path = lay->best + n;
    lay->cut = lay->path + n * level;
    lay->best_list = lay->cut + n * level;
    return MRS_OK;
}

// the need_deg-core of the matrix into x_alive -> the number of living vertices and the largest degree among them
int pcm_exact_peel(mrs_pcm* p, int need_deg, int* n_alive, int* max_deg)
{
    const int L = p->L;
    MRS_TRY(p->x_alive.reserve(64, 64));
    u64 alive[64] = {};
    for (int v = 0; v < L; ++v) alive[v >> 6] |= 1ull << (v & 63);
    MRS_HIP_TRY(hipMemcpy(p->x_alive.get(), alive, sizeof(alive), hipMemcpyHostToDevice));
    mrs::Scratch tmp;                                             // deg [L] | changed [1]
    MRS_TRY(tmp.alloc((size_t)(L + 1) * sizeof(int), nullptr));
    int* d_deg = tmp.as<int>();
    int* d_changed = d_deg + L;
    for (int round = 0; need_deg > 0 && round <= L; ++round) {    // every round but the last removes a vertex: at most L + 1 of them
        MRS_HIP_TRY(hipMemsetAsync(d_changed, 0, sizeof(int), nullptr));
        hipLaunchKernelGGL(k_pcm_peel, dim3(blocks_for(L, kWaves)), dim3(kThreads), 0, nullptr, p->rows.get(), L, p->words, need_deg, p->x_alive.get(),
                           d_changed);
        MRS_HIP_TRY(hipGetLastError());
        int changed = 0;
        MRS_HIP_TRY(hipMemcpy(&changed, d_changed, sizeof(int), hipMemcpyDeviceToHost));
        if (!changed) break;
    }
    hipLaunchKernelGGL(k_pcm_alive_degrees, dim3(blocks_for(L, kWaves)), dim3(kThreads), 0, nullptr, p->rows.get(), p->x_alive.get(), L, p->words,
                       d_deg);
    MRS_HIP_TRY(hipGetLastError());
    std::vector<int> deg(L);
    MRS_HIP_TRY(hipMemcpy(deg.data(), d_deg, (size_t)L * sizeof(int), hipMemcpyDeviceToHost));
    MRS_HIP_TRY(hipMemcpy(alive, p->x_alive.get(), sizeof(alive), hipMemcpyDeviceToHost));
    *n_alive = 0;
    for (int w = 0; w < 64; ++w) *n_alive += __builtin_popcountll(alive[w]);
    *max_deg = *std::max_element(deg.begin(), deg.end());
    return MRS_OK;
}

// launches of one phase until no slot has work left (*done) or the node budget is spent
int pcm_exact_phase(mrs_pcm* p, const ExactLayout& lay, int phase, int omega, int64_t max_nodes, ExactStatus* hs, bool* done)
{
    constexpr long long kMaxLaunches = 1ll << 32;                // every launch takes a step in every slot that has work: a fence
    *done = false;
    MRS_HIP_TRY(hipMemsetAsync(lay.top, 0xff, (size_t)lay.nslots * sizeof(int), nullptr));      // kIdle
    if (phase == 1) MRS_HIP_TRY(hipMemsetAsync(lay.best, 0, (size_t)lay.nslots * sizeof(int), nullptr));
    hs->ticket = 0;
    hs->winner = 0;
    for (long long launch = 0; launch < kMaxLaunches; ++launch) {
        if ((int64_t)hs->nodes >= max_nodes) return MRS_OK;
        hs->active = 0;
        MRS_HIP_TRY(hipMemcpy(p->x_status.get(), hs, sizeof(*hs), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_pcm_exact, dim3(blocks_for(lay.nslots, kWaves)), dim3(kThreads), 0, nullptr, p->rows.get(), p->x_alive.get(), p->L,
                           p->words, lay.maxd, lay.nslots, phase, omega, p->x_status.get(), lay.top, lay.depth, lay.path, lay.cut,
                           p->x_stack.get(), lay.best, lay.best_list);
        MRS_HIP_TRY(hipGetLastError());
        ++p->x_launches;
        MRS_HIP_TRY(hipMemcpy(hs, p->x_status.get(), sizeof(*hs), hipMemcpyDeviceToHost));
        if (hs->active == 0) {
            *done = true;
            return MRS_OK;
        }
    }
    mrs::set_error("the exact clique search did not end within %lld launches", kMaxLaunches);
    return MRS_ERR_HIP;
}

// mrs_pcm_add_loops and mrs_pcm_add_loops_cov: h_C [n][6][6] or nullptr (FIXED_COVARIANCE each; not read at all without a covariance mode)
int pcm_add_loops(mrs_pcm* pcm, const int32_t* h_ia, const int32_t* h_kb, const double* h_Z, const double* h_C, int32_t n)
{
    MRS_REQUIRE(pcm, "null pointer");
    MRS_REQUIRE(n >= 0, "n must not be negative");
    if (n == 0) return MRS_OK;
    MRS_REQUIRE(h_ia && h_kb && h_Z, "null pointer");
    MRS_REQUIRE(pcm->na > 0, "set the trajectories first");
    MRS_REQUIRE(!pcm->given_matrix, "the vertices came from mrs_pcm_set_matrix: clear them first");
    MRS_REQUIRE(!h_C || pcm->cov_mode != MRS_PCM_COV_NONE, "loop covariances need mrs_pcm_set_covariances first");
    for (int t = 0; t < n; ++t)
        MRS_REQUIRE(h_ia[t] >= 0 && h_ia[t] < pcm->na && h_kb[t] >= 0 && h_kb[t] < pcm->nb, "a loop names a pose outside its trajectory");
    if ((long long)pcm->L + n > pcm->capacity) {
        mrs::set_error("%d loops held and %d more exceed the capacity of %d", pcm->L, n, pcm->capacity);
        return MRS_ERR_UNSUPPORTED;
    }
    if (pcm->cov_mode != MRS_PCM_COV_NONE) {
        std::vector<double> Csym;
        MRS_REQUIRE(pcm_sym_inputs(h_C, (size_t)n, &Csym), "a loop covariance is not finite or not positive definite");
        MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
        // one upload: Z [n][16] | C [n][21] doubles | ia [n] | kb [n]
        const size_t b_Z = (size_t)n * 16 * sizeof(double), b_C = (size_t)n * kSym * sizeof(double), b_idx = (size_t)n * sizeof(int32_t);
        mrs::Scratch in;
        MRS_TRY(in.alloc(b_Z + b_C + 2 * b_idx, nullptr));
        double* d_Z = in.as<double>();
        double* d_C = d_Z + (size_t)n * 16;
        int* d_ia = reinterpret_cast<int*>(in.as<char>() + b_Z + b_C);
        int* d_kb = d_ia + n;
        MRS_HIP_TRY(hipMemcpy(d_Z, h_Z, b_Z, hipMemcpyHostToDevice));
        MRS_HIP_TRY(hipMemcpy(d_C, Csym.data(), b_C, hipMemcpyHostToDevice));
        MRS_HIP_TRY(hipMemcpy(d_ia, h_ia, b_idx, hipMemcpyHostToDevice));
        MRS_HIP_TRY(hipMemcpy(d_kb, h_kb, b_idx, hipMemcpyHostToDevice));
        const int L0 = pcm->L, L1 = L0 + n;
        hipLaunchKernelGGL(k_pcm_records_cov, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, nullptr, pcm->XA.get(), pcm->XB.get(), d_ia, d_kb,
                           d_Z, d_C, n, L0, pcm->rec_cov.get());
        MRS_TRY(pcm_fill_rows(pcm, L0, L1));
        MRS_HIP_TRY(hipStreamSynchronize(nullptr));
        pcm->L = L1;
        pcm->degrees_stale = true;
        return MRS_OK;
    }
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    // one upload: Z [n][16] doubles | ia [n] | kb [n]
    const size_t b_Z = (size_t)n * 16 * sizeof(double), b_idx = (size_t)n * sizeof(int32_t);
    mrs::Scratch in;
    int st = in.alloc(b_Z + 2 * b_idx, nullptr);
    if (st != MRS_OK) return st;
    double* d_Z = in.as<double>();
    int* d_ia = reinterpret_cast<int*>(in.as<char>() + b_Z);
    int* d_kb = d_ia + n;
    MRS_HIP_TRY(hipMemcpy(d_Z, h_Z, b_Z, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(d_ia, h_ia, b_idx, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(d_kb, h_kb, b_idx, hipMemcpyHostToDevice));
    const int L0 = pcm->L, L1 = L0 + n;
    hipLaunchKernelGGL(k_pcm_records, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, nullptr, pcm->XA.get(), pcm->XB.get(), d_ia, d_kb, d_Z, n, L0,
                       pcm->rec.get());
    if ((st = pcm_fill_rows(pcm, L0, L1)) != MRS_OK) return st;
    MRS_HIP_TRY(hipStreamSynchronize(nullptr));
    pcm->L = L1;
    pcm->degrees_stale = true;
    return MRS_OK;
}

}  // namespace

extern "C" {

int mrs_pcm_create(mrs_ctx* ctx, int32_t capacity, double threshold, mrs_pcm** out)
{
    MRS_REQUIRE(ctx && out, "null pointer");
    MRS_REQUIRE(capacity >= 1, "capacity must be positive");
    MRS_REQUIRE(threshold > 0.0 && std::isfinite(threshold), "threshold must be positive and finite");
    if (capacity > kMaxLoops) {
        mrs::set_error("at most %d loops per robot pair (capacity %d)", kMaxLoops, capacity);
        return MRS_ERR_UNSUPPORTED;
    }
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    mrs_pcm* p = new mrs_pcm;
    p->ctx = ctx;
    p->capacity = capacity;
    p->words = (capacity + 63) / 64;
    p->threshold = threshold;
    const size_t cap = (size_t)capacity;
    int st = p->rec.reserve(cap * kRec, cap * kRec);
    if (st == MRS_OK) st = p->rows.reserve(cap * p->words, cap * p->words);
    if (st == MRS_OK) st = p->elig.reserve(64, 64);
    if (st == MRS_OK) st = p->winner.reserve(1, 1);
    if (st == MRS_OK) st = p->deg.reserve(cap, cap);
    if (st == MRS_OK) st = p->list.reserve(kMaxLoops, kMaxLoops);      // whatever the capacity: a chain of k_pcm_greedy has at most kMaxLoops members
    if (st == MRS_OK) st = pcm_clear(p);
    if (st != MRS_OK) {
        delete p;
        return st;
    }
    *out = p;
    return MRS_OK;
}

int mrs_pcm_destroy(mrs_pcm* pcm)
{
    if (!pcm) return MRS_OK;
    (void)hipSetDevice(pcm->ctx->device);
    (void)hipStreamSynchronize(nullptr);
    delete pcm;
    return MRS_OK;
}

int mrs_pcm_set_trajectories(mrs_pcm* pcm, const double* h_XA, int32_t na, const double* h_XB, int32_t nb)
{
    MRS_REQUIRE(pcm && h_XA && h_XB, "null pointer");
    MRS_REQUIRE(na >= 1 && nb >= 1, "a trajectory has at least one pose");
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    int st = pcm->XA.reserve((size_t)na * 16, (size_t)na * 16);
    if (st != MRS_OK) return st;
    if ((st = pcm->XB.reserve((size_t)nb * 16, (size_t)nb * 16)) != MRS_OK) return st;
    pcm->na = pcm->nb = 0;
    if ((st = pcm_clear(pcm)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(pcm->XA.get(), h_XA, (size_t)na * 16 * sizeof(double), hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(pcm->XB.get(), h_XB, (size_t)nb * 16 * sizeof(double), hipMemcpyHostToDevice));
    pcm->na = na;
    pcm->nb = nb;
    pcm->cov_mode = MRS_PCM_COV_NONE;
    pcm->h_XA.assign(h_XA, h_XA + (size_t)na * 16);
    pcm->h_XB.assign(h_XB, h_XB + (size_t)nb * 16);
    return MRS_OK;
}

int mrs_pcm_set_covariances(mrs_pcm* pcm, int32_t mode, const double* h_QA, const double* h_QB, const double* h_first)
{
    MRS_REQUIRE(pcm, "null pointer");
    MRS_REQUIRE(mode == MRS_PCM_COV_NONE || mode == MRS_PCM_COV_SPAN || mode == MRS_PCM_COV_REFERENCE, "mode must be MRS_PCM_COV_NONE, _SPAN or _REFERENCE");
    MRS_REQUIRE(pcm->na > 0, "set the trajectories first");
    MRS_REQUIRE(pcm->na > 1 || !h_QA, "a trajectory of one pose has no odometry covariances");
    MRS_REQUIRE(pcm->nb > 1 || !h_QB, "a trajectory of one pose has no odometry covariances");
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    if (mode == MRS_PCM_COV_NONE) {
        MRS_TRY(pcm_clear(pcm));
        pcm->cov_mode = mode;
        return MRS_OK;
    }
    const int na = pcm->na, nb = pcm->nb;
    std::vector<double> QA, QB, first, WA, WB;
    MRS_REQUIRE(pcm_sym_inputs(h_QA, (size_t)na - 1, &QA), "an odometry covariance of A is not finite or not positive definite");
    MRS_REQUIRE(pcm_sym_inputs(h_QB, (size_t)nb - 1, &QB), "an odometry covariance of B is not finite or not positive definite");
    MRS_REQUIRE(pcm_sym_inputs(h_first, 1, &first), "the covariance of the first pose is not finite or not positive definite");
    // REFERENCE: every prefix also carries the first pose's covariance, moved to the world frame through that pose
    double fa[kSym], fb[kSym], x0[mrs::pcm::kPose];
    mrs::pcm::pose_from_4x4(pcm->h_XA.data(), x0);
    mrs::pcm::adj_conj(x0, first.data(), fa);
    mrs::pcm::pose_from_4x4(pcm->h_XB.data(), x0);
    mrs::pcm::adj_conj(x0, first.data(), fb);
    const bool ref = mode == MRS_PCM_COV_REFERENCE;
    pcm_prefixes(pcm->h_XA, na, QA, ref ? fa : nullptr, &WA);
    pcm_prefixes(pcm->h_XB, nb, QB, ref ? fb : nullptr, &WB);
    const size_t cap = (size_t)pcm->capacity;
    MRS_TRY(pcm->rec_cov.reserve(cap * kRecCov, cap * kRecCov));
    MRS_TRY(pcm->WA.reserve(WA.size(), WA.size()));
    MRS_TRY(pcm->WB.reserve(WB.size(), WB.size()));
    MRS_TRY(pcm_clear(pcm));
    pcm->cov_mode = MRS_PCM_COV_NONE;                            // until the tables are in place
    MRS_HIP_TRY(hipMemcpy(pcm->WA.get(), WA.data(), WA.size() * sizeof(double), hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(pcm->WB.get(), WB.data(), WB.size() * sizeof(double), hipMemcpyHostToDevice));
    pcm->h_WA.swap(WA);
    pcm->h_WB.swap(WB);
    pcm->cov_mode = mode;
    return MRS_OK;
}

int mrs_pcm_add_loops(mrs_pcm* pcm, const int32_t* h_ia, const int32_t* h_kb, const double* h_Z, int32_t n)
{
    return pcm_add_loops(pcm, h_ia, h_kb, h_Z, nullptr, n);
}

int mrs_pcm_add_loops_cov(mrs_pcm* pcm, const int32_t* h_ia, const int32_t* h_kb, const double* h_Z, const double* h_C, int32_t n)
{
    return pcm_add_loops(pcm, h_ia, h_kb, h_Z, h_C, n);
}

int mrs_pcm_get_pair(mrs_pcm* pcm, int32_t u, int32_t v, double* h_xi, double* h_cov, double* h_d)
{
    MRS_REQUIRE(pcm && h_xi && h_cov && h_d, "null pointer");
    MRS_REQUIRE(!pcm->given_matrix, "the vertices came from mrs_pcm_set_matrix: they have no distances");
    MRS_REQUIRE(u >= 0 && u < pcm->L && v >= 0 && v < pcm->L && u != v, "two different loops of the handle");
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    const int a = std::min(u, v), b = std::max(u, v);
    if (pcm->cov_mode == MRS_PCM_COV_NONE) {
        double ra[kRec], rb[kRec];
        MRS_HIP_TRY(hipMemcpy(ra, pcm->rec.get() + (size_t)a * kRec, sizeof(ra), hipMemcpyDeviceToHost));
        MRS_HIP_TRY(hipMemcpy(rb, pcm->rec.get() + (size_t)b * kRec, sizeof(rb), hipMemcpyDeviceToHost));
        double pinv[mrs::pcm::kPose], m[mrs::pcm::kPose], binv[mrs::pcm::kPose], mb[mrs::pcm::kPose], e[mrs::pcm::kPose];
        mrs::pcm::pose_inv(ra, pinv);
        mrs::pcm::pose_mul(pinv, rb, m);
        mrs::pcm::pose_inv(ra + mrs::pcm::kPose, binv);
        mrs::pcm::pose_mul(m, ra + mrs::pcm::kPose, mb);
        mrs::pcm::pose_mul(binv, mb, e);
        mrs::pcm::pose_logmap(e, h_xi);
        for (int i = 0; i < 36; ++i) h_cov[i] = i % 7 == 0 ? 1.0 : 0.0;       // the reference's identity
        *h_d = mrs::pcm::pose_log_norm(e);
        return MRS_OK;
    }
    double ra[kRecCov], rb[kRecCov];
    MRS_HIP_TRY(hipMemcpy(ra, pcm->rec_cov.get() + (size_t)a * kRecCov, sizeof(ra), hipMemcpyDeviceToHost));
    MRS_HIP_TRY(hipMemcpy(rb, pcm->rec_cov.get() + (size_t)b * kRecCov, sizeof(rb), hipMemcpyDeviceToHost));
    *h_d = mrs::pcm::pair_mahalanobis2_full(ra, rb, pcm->h_WA.data(), pcm->h_WB.data(), pcm->cov_mode, h_xi, h_cov);
    return MRS_OK;
}

int mrs_pcm_clear_loops(mrs_pcm* pcm)
{
    MRS_REQUIRE(pcm, "null pointer");
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    return pcm_clear(pcm);
}

int mrs_pcm_count(mrs_pcm* pcm, int32_t* h_count)
{
    MRS_REQUIRE(pcm && h_count, "null pointer");
    *h_count = pcm->L;
    return MRS_OK;
}

int mrs_pcm_solve(mrs_pcm* pcm, int32_t* h_clique, int32_t* h_n_clique, int32_t* h_n_rounds)
{
    MRS_REQUIRE(pcm && h_n_clique, "null pointer");
    const int L = pcm->L;
    MRS_REQUIRE(h_clique || L == 0, "null pointer");
    *h_n_clique = 0;
    if (h_n_rounds) *h_n_rounds = 0;
    if (L == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    if (pcm->degrees_stale) {
        hipLaunchKernelGGL(k_pcm_degrees, dim3(blocks_for(L, kWaves)), dim3(kThreads), 0, nullptr, pcm->rows.get(), L, pcm->words, pcm->deg.get());
        pcm->degrees_stale = false;
    }
    int max_clq = -1, start = 0, rounds = 0, best_start = -1, best_bound = -1;
    while (start < L && rounds <= L) {                            // every round but the last raises max_clq: at most L + 1 of them
        hipLaunchKernelGGL(k_pcm_eligible, dim3(1), dim3(kThreads), 0, nullptr, pcm->deg.get(), L, max_clq, pcm->elig.get(), pcm->winner.get());
        hipLaunchKernelGGL(k_pcm_greedy, dim3(blocks_for(L - start, kWaves)), dim3(kThreads), 0, nullptr, pcm->rows.get(), pcm->deg.get(),
                           pcm->elig.get(), pcm->words, start, L, max_clq, pcm->winner.get(), (int*)nullptr);
        MRS_HIP_TRY(hipGetLastError());
        u64 w = kNoWinner;
        MRS_HIP_TRY(hipMemcpy(&w, pcm->winner.get(), sizeof(w), hipMemcpyDeviceToHost));
        ++rounds;
        if (w == kNoWinner) break;
        best_start = (int)(w >> 32);
        best_bound = max_clq;                                     // the bound its chain ran under
        max_clq = (int)(w & 0xffffffffu);
        start = best_start + 1;
    }
    if (best_start < 0 || max_clq < 1 || max_clq > L) {
        mrs::set_error("the clique rounds ended without a result (%d loops, %d rounds)", L, rounds);
        return MRS_ERR_HIP;
    }
    hipLaunchKernelGGL(k_pcm_eligible, dim3(1), dim3(kThreads), 0, nullptr, pcm->deg.get(), L, best_bound, pcm->elig.get(), pcm->winner.get());
    hipLaunchKernelGGL(k_pcm_greedy, dim3(1), dim3(64), 0, nullptr, pcm->rows.get(), pcm->deg.get(), pcm->elig.get(), pcm->words, best_start,
                       best_start + 1, best_bound, pcm->winner.get(), pcm->list.get());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpy(h_clique, pcm->list.get(), (size_t)max_clq * sizeof(int32_t), hipMemcpyDeviceToHost));
    *h_n_clique = max_clq;
    if (h_n_rounds) *h_n_rounds = rounds;
    return MRS_OK;
}

int mrs_pcm_solve_exact(mrs_pcm* pcm, int64_t max_nodes, int32_t* h_clique, int32_t* h_n_clique, int32_t* h_proof, int64_t* h_nodes)
{
    MRS_REQUIRE(max_nodes >= 0, "max_nodes must not be negative");
    MRS_REQUIRE(pcm && h_n_clique && h_proof && h_nodes, "null pointer");
    const int L = pcm->L;
    MRS_REQUIRE(h_clique || L == 0, "null pointer");
    *h_n_clique = 0;
    *h_proof = 2;
    *h_nodes = 0;
    pcm->x_launches = 0;
    if (L == 0) return MRS_OK;
    // the seed: the heuristic's clique, ascending
    std::vector<int32_t> incumbent(L);
    int32_t seed = 0;
    MRS_TRY(mrs_pcm_solve(pcm, incumbent.data(), &seed, nullptr));
    incumbent.resize(seed);
    std::sort(incumbent.begin(), incumbent.end());
    ExactStatus hs = {};
    hs.best = seed;
    const auto finish = [&](const std::vector<int32_t>& members, int proof) {
        std::copy(members.begin(), members.end(), h_clique);
        *h_n_clique = (int32_t)members.size();
        *h_proof = proof;
        *h_nodes = (int64_t)hs.nodes;
        return MRS_OK;
    };
    if (max_nodes == 0) return finish(incumbent, 0);
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));

    // phase 1: the size.  A member of a clique larger than the seed has at least `seed` neighbours among the members.
    ExactLayout lay;
    int n_alive = 0, max_deg = 0;
    MRS_TRY(pcm_exact_peel(pcm, seed, &n_alive, &max_deg));
    if (n_alive > 0) {
        bool done = false;
        MRS_TRY(pcm_exact_layout(pcm, std::min(n_alive, max_deg + 1), &lay));
        MRS_TRY(pcm_exact_phase(pcm, lay, 1, 0, max_nodes, &hs, &done));
        if (hs.best < seed || hs.best > lay.maxd) {
            mrs::set_error("the exact clique search returned the size %d (seed %d, bound %d)", hs.best, seed, lay.maxd);
            return MRS_ERR_HIP;
        }
        if (hs.best > seed) {                                     // the slot that found the incumbent holds its members
            std::vector<int> sizes(lay.nslots);
            MRS_HIP_TRY(hipMemcpy(sizes.data(), lay.best, sizes.size() * sizeof(int), hipMemcpyDeviceToHost));
            const int slot = (int)(std::find(sizes.begin(), sizes.end(), hs.best) - sizes.begin());
            if (slot == lay.nslots) {
                mrs::set_error("no slot of the exact clique search holds the clique of size %d", hs.best);
                return MRS_ERR_HIP;
            }
            incumbent.resize(hs.best);
            MRS_HIP_TRY(hipMemcpy(incumbent.data(), lay.best_list + (size_t)slot * (lay.maxd + 1), (size_t)hs.best * sizeof(int32_t),
                                  hipMemcpyDeviceToHost));
            std::sort(incumbent.begin(), incumbent.end());
        }
        if (!done) return finish(incumbent, 0);
    }
    const int omega = hs.best;
    if ((int64_t)hs.nodes >= max_nodes) return finish(incumbent, 1);

    // phase 2: the canonical list.  A member of a clique of size omega has omega - 1 neighbours among the members.
    bool done = false;
    MRS_TRY(pcm_exact_peel(pcm, omega - 1, &n_alive, &max_deg));
    MRS_TRY(pcm_exact_layout(pcm, omega, &lay));
    MRS_TRY(pcm_exact_phase(pcm, lay, 2, omega, max_nodes, &hs, &done));
    if (!done) return finish(incumbent, 1);
    const int slot = (int)(hs.winner & 0xffffu);
    if (hs.winner == 0 || slot >= lay.nslots) {
        mrs::set_error("the exact clique search proved the size %d and found no clique of it", omega);
        return MRS_ERR_HIP;
    }
    std::vector<int32_t> members(omega);
    MRS_HIP_TRY(hipMemcpy(members.data(), lay.path + (size_t)slot * (lay.maxd + 1), (size_t)omega * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::reverse(members.begin(), members.end());                // the path is descending
    return finish(members, 2);
}

int mrs_pcm_exact_launches(mrs_pcm* pcm, int64_t* h_launches)
{
    MRS_REQUIRE(pcm && h_launches, "null pointer");
    *h_launches = pcm->x_launches;
    return MRS_OK;
}

int mrs_pcm_get_matrix(mrs_pcm* pcm, uint8_t* h_dense)
{
    MRS_REQUIRE(pcm, "null pointer");
    const int L = pcm->L, words = pcm->words;
    if (L == 0) return MRS_OK;
    MRS_REQUIRE(h_dense, "null pointer");
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    std::vector<u64> bits((size_t)L * words);
    MRS_HIP_TRY(hipMemcpy(bits.data(), pcm->rows.get(), bits.size() * sizeof(u64), hipMemcpyDeviceToHost));
    for (int u = 0; u < L; ++u)
        for (int v = 0; v < L; ++v) h_dense[(size_t)u * L + v] = (uint8_t)((bits[(size_t)u * words + v / 64] >> (v % 64)) & 1ull);
    return MRS_OK;
}

int mrs_pcm_set_matrix(mrs_pcm* pcm, int32_t count, const uint8_t* h_dense)
{
    MRS_REQUIRE(pcm && (h_dense || count == 0), "null pointer");
    MRS_REQUIRE(count >= 0, "count must not be negative");
    if (count > pcm->capacity) {
        mrs::set_error("%d vertices exceed the capacity of %d", count, pcm->capacity);
        return MRS_ERR_UNSUPPORTED;
    }
    const int L = count, words = pcm->words;
    std::vector<u64> bits((size_t)L * words, 0ull);
    for (int u = 0; u < L; ++u) {
        MRS_REQUIRE(!h_dense[(size_t)u * L + u], "the diagonal must be zero");
        for (int v = 0; v < L; ++v) {
            const bool e = h_dense[(size_t)u * L + v] != 0;
            MRS_REQUIRE(e == (h_dense[(size_t)v * L + u] != 0), "the adjacency must be symmetric");
            if (e) bits[(size_t)u * words + v / 64] |= 1ull << (v % 64);
        }
    }
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    int st = pcm_clear(pcm);
    if (st != MRS_OK) return st;
    if (L > 0) MRS_HIP_TRY(hipMemcpy(pcm->rows.get(), bits.data(), bits.size() * sizeof(u64), hipMemcpyHostToDevice));
    pcm->L = L;
    pcm->given_matrix = L > 0;
    return MRS_OK;
}

int mrs_pcm_get_distances(mrs_pcm* pcm, double* h_d)
{
    MRS_REQUIRE(pcm, "null pointer");
    MRS_REQUIRE(!pcm->given_matrix, "the vertices came from mrs_pcm_set_matrix: they have no distances");
    const int L = pcm->L;
    if (L == 0) return MRS_OK;
    MRS_REQUIRE(h_d, "null pointer");
    MRS_HIP_TRY(hipSetDevice(pcm->ctx->device));
    mrs::Scratch d;
    int st = d.alloc((size_t)L * L * sizeof(double), nullptr);
    if (st != MRS_OK) return st;
    if (pcm->cov_mode != MRS_PCM_COV_NONE)
        hipLaunchKernelGGL(k_pcm_distances_cov, dim3(blocks_for((long long)L * L, kThreads)), dim3(kThreads), 0, nullptr, pcm->rec_cov.get(),
                           pcm->WA.get(), pcm->WB.get(), pcm->cov_mode, L, d.as<double>());
    else
        hipLaunchKernelGGL(k_pcm_distances, dim3(blocks_for((long long)L * L, kThreads)), dim3(kThreads), 0, nullptr, pcm->rec.get(), L, d.as<double>());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpy(h_d, d.p, (size_t)L * L * sizeof(double), hipMemcpyDeviceToHost));
    return MRS_OK;
}

}  // extern "C"
