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
#include "common.hpp"
#include "pcm_pose.hpp"

#include <cmath>

namespace {

using u64 = unsigned long long;
constexpr int kMaxLoops = MRS_PCM_MAX_LOOPS;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRec = mrs::pcm::kRecord;
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
    mrs::DeviceBuffer<u64> rows, elig, winner;
    mrs::DeviceBuffer<int> deg, list;
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
    hipLaunchKernelGGL(k_pcm_rows, dim3(blocks_for((long long)(L1 - L0) * nw, kWaves)), dim3(kThreads), 0, nullptr, p->rec.get(), L1, p->threshold,
                       L0, L1 - L0, 0, nw, p->words, p->rows.get());
    const int w0 = L0 / 64;
    if (L0 > 0)
        hipLaunchKernelGGL(k_pcm_rows, dim3(blocks_for((long long)L0 * (nw - w0), kWaves)), dim3(kThreads), 0, nullptr, p->rec.get(), L1,
                           p->threshold, 0, L0, w0, nw - w0, p->words, p->rows.get());
    MRS_HIP_TRY(hipGetLastError());
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
    return MRS_OK;
}

int mrs_pcm_add_loops(mrs_pcm* pcm, const int32_t* h_ia, const int32_t* h_kb, const double* h_Z, int32_t n)
{
    MRS_REQUIRE(pcm, "null pointer");
    MRS_REQUIRE(n >= 0, "n must not be negative");
    if (n == 0) return MRS_OK;
    MRS_REQUIRE(h_ia && h_kb && h_Z, "null pointer");
    MRS_REQUIRE(pcm->na > 0, "set the trajectories first");
    MRS_REQUIRE(!pcm->given_matrix, "the vertices came from mrs_pcm_set_matrix: clear them first");
    for (int t = 0; t < n; ++t)
        MRS_REQUIRE(h_ia[t] >= 0 && h_ia[t] < pcm->na && h_kb[t] >= 0 && h_kb[t] < pcm->nb, "a loop names a pose outside its trajectory");
    if ((long long)pcm->L + n > pcm->capacity) {
        mrs::set_error("%d loops held and %d more exceed the capacity of %d", pcm->L, n, pcm->capacity);
        return MRS_ERR_UNSUPPORTED;
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
    hipLaunchKernelGGL(k_pcm_distances, dim3(blocks_for((long long)L * L, kThreads)), dim3(kThreads), 0, nullptr, pcm->rec.get(), L, d.as<double>());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpy(h_d, d.p, (size_t)L * L * sizeof(double), hipMemcpyDeviceToHost));
    return MRS_OK;
}

}  // extern "C"
