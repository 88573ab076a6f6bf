// ransac.hip -- RANSAC pose from point correspondences for a ragged batch of pairs.
//
// One chain on the caller's stream, no host synchronisation (every scratch size follows from h_offsets and the hypothesis count):
//   k_verdict  one thread per (pair, h): draw + pre-rejection -> a flag byte and the number of valid hypotheses of every chunk of 256
//   k_models   the same grid: the ranks of a chunk's valid hypotheses (chunk base + rank in the chunk = rank in h order), then the first
//              lanes of the block fit the compacted triples, so the Jacobi of icp_rigid_fit runs on full lanes, not on 1 in 20
//   k_score    grid (tile of kTile correspondences, block of 256 models): a lane keeps one model in registers, the tile is widened once
//              into LDS and read by all lanes at the same address (a broadcast); integer atomicAdd of the tile's count per model
//   k_refit    one workgroup per pair: the best model by a 64-bit integer atomicMax of count << 32 | ~h, then the refit loop
// All arithmetic that decides anything is integer or one of the fp64 expressions of ransac_model.hpp; there are no float atomics.
#include "common.hpp"
#include "ransac_model.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using u64 = unsigned long long;

constexpr int kThreads = 256;             // threads of every kernel here; also the models of one score block and the hypotheses of one chunk
constexpr int kTile = 512;                // correspondences of one LDS tile: 512 x 6 doubles = 24 KiB, six workgroups per CU
constexpr int kModelDoubles = 12;         // the first three rows of D
constexpr int64_t kGroupModels = 1 << 20; // hypotheses of the pairs that share one scratch allocation (about 110 MB)

struct Params {
    int H;
    int refine;
    double d2, s2, min_sin2;
};

__device__ __forceinline__ void load_pair(const float* __restrict__ src, const float* __restrict__ dst, int stride, int64_t row, double* p, double* q)
{
    const float* a = src + row * stride;
    const float* b = dst + row * stride;
    for (int k = 0; k < 3; ++k) { p[k] = (double)a[k]; q[k] = (double)b[k]; }
}

// the triple of hypothesis h (M >= 3), widened, in drawn order
__device__ __forceinline__ void triple_of(const float* __restrict__ src, const float* __restrict__ dst, int stride, int64_t first, int64_t M,
                                          uint64_t seed, int h, double* p, double* q)
{
    int64_t idx[3];
    mrs::ransac_draw(seed, (uint32_t)h, (uint64_t)M, idx);
    for (int k = 0; k < 3; ++k) load_pair(src, dst, stride, first + idx[k], p + 3 * k, q + 3 * k);
}

// flags [pairs][H], chunk_count [pairs][n_chunks]; grid (n_chunks, pairs)
__global__ __launch_bounds__(kThreads) void k_verdict(const float* __restrict__ src, const float* __restrict__ dst, int stride,
                                                      const int64_t* __restrict__ offs, const uint64_t* __restrict__ seeds, int pair0, Params P,
                                                      uint8_t* __restrict__ flags, int* __restrict__ chunk_count)
{
    __shared__ int s_count;
    const int pl = blockIdx.y, pair = pair0 + pl, h = blockIdx.x * kThreads + threadIdx.x;
    const int64_t first = offs[pair], M = offs[pair + 1] - first;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    bool ok = false;
    if (h < P.H && M >= 3) {
        double p[9], q[9];
        triple_of(src, dst, stride, first, M, seeds[pair], h, p, q);
        ok = mrs::ransac_triple_ok(p, q, P.s2, P.min_sin2);
    }
    if (h < P.H) flags[(size_t)pl * P.H + h] = ok ? 1 : 0;
    const u64 b = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_count, __popcll(b));
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[(size_t)pl * gridDim.x + blockIdx.x] = s_count;
}

// models [pairs][H][12] and model_h [pairs][H] in h order, n_valid [pairs]; grid (n_chunks, pairs)
__global__ __launch_bounds__(kThreads) void k_models(const float* __restrict__ src, const float* __restrict__ dst, int stride,
                                                     const int64_t* __restrict__ offs, const uint64_t* __restrict__ seeds, int pair0, Params P,
                                                     const uint8_t* __restrict__ flags, const int* __restrict__ chunk_count,
                                                     double* __restrict__ models, int* __restrict__ model_h, int* __restrict__ n_valid)
{
    __shared__ int s_base, s_total, s_wave[kThreads / 64], s_list[kThreads];
    const int pl = blockIdx.y, pair = pair0 + pl, chunk = blockIdx.x, n_chunks = gridDim.x, tid = threadIdx.x;
    const int h = chunk * kThreads + tid;
    if (tid == 0) { s_base = 0; s_total = 0; }
    __syncthreads();
    // integer sums: the order of the atomics does not matter
    for (int c = tid; c < n_chunks; c += kThreads) {
        const int v = chunk_count[(size_t)pl * n_chunks + c];
        if (v) {
            atomicAdd(&s_total, v);
            if (c < chunk) atomicAdd(&s_base, v);
        }
    }
    const bool ok = h < P.H && flags[(size_t)pl * P.H + h] != 0;
    const u64 b = __ballot(ok);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (ok) s_list[before + __popcll(b & ((1ull << lane) - 1ull))] = h;
    int count = 0;
    for (int w = 0; w < kThreads / 64; ++w) count += s_wave[w];
    __syncthreads();
    if (chunk == 0 && tid == 0) n_valid[pl] = s_total;
    if (tid >= count) return;
    const int hh = s_list[tid];
    const size_t slot = (size_t)pl * P.H + (size_t)(s_base + tid);      // s_base + count <= n_valid <= H
    const int64_t first = offs[pair], M = offs[pair + 1] - first;
    double p[9], q[9], D[16];
    triple_of(src, dst, stride, first, M, seeds[pair], hh, p, q);
    mrs::ransac_triple_fit(p, q, D);
    for (int k = 0; k < kModelDoubles; ++k) models[slot * kModelDoubles + k] = D[k];
    model_h[slot] = hh;
}

// tiles int2 {pair, first correspondence of the tile within the pair}; counts [pairs][H] by rank; grid (n_tiles, n_chunks)
__global__ __launch_bounds__(kThreads) void k_score(const float* __restrict__ src, const float* __restrict__ dst, int stride,
                                                    const int64_t* __restrict__ offs, const int2* __restrict__ tiles, int pair0, Params P,
                                                    const double* __restrict__ models, const int* __restrict__ n_valid, int* __restrict__ counts)
{
    __shared__ double s_c[kTile * 6];
    const int2 t = tiles[blockIdx.x];
    const int pl = t.x - pair0, tid = threadIdx.x;
    const int nv = n_valid[pl], rank = blockIdx.y * kThreads + tid;
    if (blockIdx.y * kThreads >= nv) return;                      // the same for every thread of the block
    const int64_t first = offs[t.x], M = offs[t.x + 1] - first;
    const int64_t left = M - (int64_t)t.y;
    const int n = left < kTile ? (int)left : kTile;
    for (int i = tid; i < n; i += kThreads) {
        double p[3], q[3];
        load_pair(src, dst, stride, first + t.y + i, p, q);
        if (!mrs::ransac_finite3(p) || !mrs::ransac_finite3(q)) p[0] = NAN;      // dead: its residual is NaN under every model
        for (int k = 0; k < 3; ++k) { s_c[6 * i + k] = p[k]; s_c[6 * i + 3 + k] = q[k]; }
    }
    double D[kModelDoubles];
    const bool live = rank < nv;
    const size_t slot = (size_t)pl * P.H + (size_t)(live ? rank : 0);
    for (int k = 0; k < kModelDoubles; ++k) D[k] = models[slot * kModelDoubles + k];
    __syncthreads();
    int count = 0;
    const int n_wave = rank - (tid & 63) < nv ? n : 0;           // a wave whose 64 ranks are all past the valid models has nothing to score
    for (int i = 0; i < n_wave; ++i) {
        const double* c = s_c + 6 * i;
        count += mrs::ransac_inlier(mrs::ransac_residual2(D, c[0], c[1], c[2], c[3], c[4], c[5]), P.d2) ? 1 : 0;
    }
    if (live && count) atomicAdd(&counts[(size_t)pl * P.H + rank], count);
}

struct PassResult {
    int count, changed;
};

// One pass of a workgroup over its pair under model D (shared memory): the inlier count, the 17 sums over the inliers, the number of
// verdicts that differ from cur_mask (which then holds the new ones).  Every thread returns the same values; sums[] is shared memory.
// Thread t adds the correspondences t, t + 256, ... in ascending order, a wave adds its lanes by a fixed butterfly, thread 0 adds the
// four waves in order: the shape depends on the pair's size alone.
__device__ PassResult refit_pass(const float* __restrict__ src, const float* __restrict__ dst, int stride, int64_t first, int64_t M,
                                 const double* D, double d2, uint8_t* __restrict__ cur_mask, uint8_t* __restrict__ out_mask, bool want_sums,
                                 double* sums, double (*s_part)[mrs::kIcpTerms], int* s_int)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double s[mrs::kIcpTerms];
    for (int k = 0; k < mrs::kIcpTerms; ++k) s[k] = 0.0;
    int count = 0, changed = 0;
    double Dl[kModelDoubles];
    for (int k = 0; k < kModelDoubles; ++k) Dl[k] = D[k];
    for (int64_t m = tid; m < M; m += kThreads) {
        double p[3], q[3];
        load_pair(src, dst, stride, first + m, p, q);
        const bool in = mrs::ransac_finite3(p) && mrs::ransac_finite3(q) &&
                        mrs::ransac_inlier(mrs::ransac_residual2(Dl, p[0], p[1], p[2], q[0], q[1], q[2]), d2);
        if (cur_mask) {
            changed += (cur_mask[first + m] != 0) != in;
            cur_mask[first + m] = in ? 1 : 0;
        }
        if (out_mask) out_mask[first + m] = in ? 1 : 0;
        if (in) {
            ++count;
            if (want_sums) mrs::ransac_accumulate(s, p, q);
        }
    }
    if (tid == 0) { s_int[0] = 0; s_int[1] = 0; }
    __syncthreads();
    if (count) atomicAdd(&s_int[0], count);
    if (changed) atomicAdd(&s_int[1], changed);
    if (want_sums) {
        for (int k = 0; k < mrs::kIcpTerms; ++k) {
            double v = s[k];
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) s_part[wave][k] = v;
        }
    }
    __syncthreads();
    if (want_sums && tid < mrs::kIcpTerms) {
        double v = s_part[0][tid];
        for (int w = 1; w < kThreads / 64; ++w) v += s_part[w][tid];
        sums[tid] = v;
    }
    PassResult r = {s_int[0], s_int[1]};
    __syncthreads();
    return r;
}

// grid (pairs)
__global__ __launch_bounds__(kThreads) void k_refit(const float* __restrict__ src, const float* __restrict__ dst, int stride,
                                                    const int64_t* __restrict__ offs, int pair0, Params P, const double* __restrict__ models,
                                                    const int* __restrict__ model_h, const int* __restrict__ n_valid, const int* __restrict__ counts,
                                                    uint8_t* __restrict__ cur_mask, double* __restrict__ out_T, int* __restrict__ out_info,
                                                    uint8_t* __restrict__ out_mask)
{
    __shared__ u64 s_best;
    __shared__ double s_D[kModelDoubles], s_bestD[kModelDoubles], s_sums[mrs::kIcpTerms], s_part[kThreads / 64][mrs::kIcpTerms];
    __shared__ int s_int[2];
    const int pl = blockIdx.x, pair = pair0 + pl, tid = threadIdx.x;
    const int64_t first = offs[pair], M = offs[pair + 1] - first;
    const int nv = n_valid[pl];
    double* T = out_T + (size_t)pair * 16;
    int* info = out_info + (size_t)pair * 4;
    if (nv == 0) {                                               // M < 3, or every triple rejected: no pose is a result
        if (tid < 16) T[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
        if (tid == 0) { info[0] = 0; info[1] = -1; info[2] = 0; info[3] = 0; }
        if (out_mask)
            for (int64_t m = tid; m < M; m += kThreads) out_mask[first + m] = 0;
        return;
    }
    if (tid == 0) s_best = 0;
    __syncthreads();
    u64 key = 0;
    for (int r = tid; r < nv; r += kThreads) {
        const size_t slot = (size_t)pl * P.H + r;
        const u64 k = ((u64)(unsigned)counts[slot] << 32) | (u64)(0xFFFFFFFFu - (unsigned)model_h[slot]);
        key = k > key ? k : key;
    }
    atomicMax(&s_best, key);
    __syncthreads();
    const int best_h = (int)(0xFFFFFFFFu - (unsigned)(s_best & 0xFFFFFFFFull));
    // the rank of best_h: model_h ascends with the rank
    if (tid == 0) {
        int lo = 0, hi = nv - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (model_h[(size_t)pl * P.H + mid] < best_h) lo = mid + 1; else hi = mid;
        }
        s_int[0] = lo;
    }
    __syncthreads();
    const int best_rank = s_int[0];
    __syncthreads();
    if (tid < kModelDoubles) s_D[tid] = s_bestD[tid] = models[((size_t)pl * P.H + best_rank) * kModelDoubles + tid];
    __syncthreads();
    // S_0 under T_0; cur_mask starts undefined, so the first pass's `changed` is not used
    PassResult r = refit_pass(src, dst, stride, first, M, s_D, P.d2, cur_mask, nullptr, P.refine > 0, s_sums, s_part, s_int);
    int best_count = r.count, prev_count = r.count, done = 0;
    for (int j = 1; j <= P.refine; ++j) {
        if (prev_count < 3) break;
        if (tid == 0) {
            double D[16];
            mrs::icp_rigid_fit(s_sums, D);
            for (int k = 0; k < kModelDoubles; ++k) s_D[k] = D[k];
        }
        __syncthreads();
        r = refit_pass(src, dst, stride, first, M, s_D, P.d2, cur_mask, nullptr, j < P.refine, s_sums, s_part, s_int);
        done = j;
        if (r.count > best_count) {
            best_count = r.count;
            if (tid < kModelDoubles) s_bestD[tid] = s_D[tid];
        }
        prev_count = r.count;
        __syncthreads();
        if (r.changed == 0) break;
    }
    if (out_mask) refit_pass(src, dst, stride, first, M, s_bestD, P.d2, nullptr, out_mask, false, s_sums, s_part, s_int);
    if (tid < kModelDoubles) T[tid] = s_bestD[tid];
    if (tid >= kModelDoubles && tid < 16) T[tid] = tid == 15 ? 1.0 : 0.0;
    if (tid == 0) { info[0] = best_count; info[1] = best_h; info[2] = nv; info[3] = done; }
}

bool finite_in(double v, double lo, double hi) { return v >= lo && v <= hi; }       // false for NaN


// stage_ms (optional, [3]): the times of the three stages (models = verdict + fit, score, refit) between events, summed over the
// rounds; the call then waits for the stream
int ransac_run(mrs_ctx* ctx, const float* d_src, const float* d_dst, int32_t stride_floats, const int64_t* d_offsets,
               const int64_t* h_offsets, int32_t n_pairs, const uint64_t* h_seeds, const mrs_ransac_params* params, double* d_T,
               int32_t* d_info, uint8_t* d_mask, hipStream_t s, float* stage_ms)
{
    MRS_REQUIRE(ctx && h_offsets && params, "null pointer");
    MRS_REQUIRE(n_pairs >= 0 && n_pairs <= mrs::kMaxGridY, "n_pairs in 0..65535");
    MRS_REQUIRE(stride_floats >= 3, "stride_floats >= 3");
    MRS_REQUIRE(h_offsets[0] == 0, "offsets start at 0");
    for (int i = 0; i < n_pairs; ++i)
        MRS_REQUIRE(h_offsets[i + 1] >= h_offsets[i] && h_offsets[i + 1] - h_offsets[i] < (1ll << 31) - 1, "offsets ascend, a pair holds fewer than 2^31 - 1 correspondences");
    const int64_t total = h_offsets[n_pairs];
    MRS_REQUIRE(params->hypotheses >= 1 && params->hypotheses <= MRS_RANSAC_MAX_HYPOTHESES, "hypotheses in 1..65536");
    MRS_REQUIRE(params->refine_iters >= 0 && params->refine_iters <= MRS_RANSAC_MAX_REFINE, "refine_iters in 0..16");
    MRS_REQUIRE(params->max_distance > 0.0 && params->max_distance <= DBL_MAX, "max_distance finite and > 0");
    MRS_REQUIRE(finite_in(params->edge_similarity, 0.0, 1.0), "edge_similarity in [0, 1]");
    MRS_REQUIRE(params->min_sin2 >= 0.0 && params->min_sin2 < 1.0, "min_sin2 in [0, 1)");
    MRS_REQUIRE(n_pairs == 0 || (d_offsets && h_seeds && d_T && d_info), "null pointer");
    MRS_REQUIRE(total == 0 || (d_src && d_dst), "null pointer");
    if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = 0.f;
    if (n_pairs == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    mrs::Event ev[4];                                            // the four timed events of a profiled call
    if (stage_ms)
        for (mrs::Event& e : ev) MRS_TRY(e.create(hipEventDefault));

    Params P;
    P.H = params->hypotheses;
    P.refine = params->refine_iters;
    P.d2 = params->max_distance * params->max_distance;
    P.s2 = params->edge_similarity * params->edge_similarity;
    P.min_sin2 = params->min_sin2;
    const int H = P.H, n_chunks = (H + kThreads - 1) / kThreads;
    const int group = (int)std::max<int64_t>(1, std::min<int64_t>(n_pairs, kGroupModels / H));

    int st;
    mrs::Scratch seeds, cur_mask, flags, chunk_count, models, model_h, n_valid, counts, tiles;
    if ((st = seeds.alloc((size_t)n_pairs * sizeof(uint64_t), s)) != MRS_OK) return st;
    if ((st = cur_mask.alloc((size_t)total, s)) != MRS_OK) return st;
    if ((st = flags.alloc((size_t)group * H, s)) != MRS_OK) return st;
    if ((st = chunk_count.alloc((size_t)group * n_chunks * sizeof(int), s)) != MRS_OK) return st;
    if ((st = models.alloc((size_t)group * H * kModelDoubles * sizeof(double), s)) != MRS_OK) return st;
    if ((st = model_h.alloc((size_t)group * H * sizeof(int), s)) != MRS_OK) return st;
    if ((st = n_valid.alloc((size_t)group * sizeof(int), s)) != MRS_OK) return st;
    if ((st = counts.alloc((size_t)group * H * sizeof(int), s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpyAsync(seeds.p, h_seeds, (size_t)n_pairs * sizeof(uint64_t), hipMemcpyHostToDevice, s));

    // the tiles of every pair, in pair order: a round of pairs scores the range [tile_first[round], tile_first[round + 1])
    std::vector<int2> h_tiles;
    std::vector<size_t> tile_first;
    for (int pair0 = 0; pair0 < n_pairs; pair0 += group) {
        tile_first.push_back(h_tiles.size());
        for (int i = pair0; i < std::min(n_pairs, pair0 + group); ++i) {
            const int64_t M = h_offsets[i + 1] - h_offsets[i];
            if (M < 3) continue;                                 // no valid hypothesis: nothing to score
            for (int64_t t = 0; t < M; t += kTile) h_tiles.push_back(make_int2(i, (int)t));
        }
    }
    tile_first.push_back(h_tiles.size());
    if ((st = tiles.alloc(h_tiles.size() * sizeof(int2), s)) != MRS_OK) return st;
    if (!h_tiles.empty()) MRS_HIP_TRY(hipMemcpyAsync(tiles.p, h_tiles.data(), h_tiles.size() * sizeof(int2), hipMemcpyHostToDevice, s));

    for (int pair0 = 0, round = 0; pair0 < n_pairs; pair0 += group, ++round) {
        const int np = std::min(group, n_pairs - pair0);
        const size_t n_tiles = tile_first[round + 1] - tile_first[round];
        const dim3 grid_h((unsigned)n_chunks, (unsigned)np);
        if (stage_ms) MRS_HIP_TRY(hipEventRecord(ev[0], s));
        hipLaunchKernelGGL(k_verdict, grid_h, dim3(kThreads), 0, s, d_src, d_dst, stride_floats, d_offsets, seeds.as<uint64_t>(), pair0, P,
                           flags.as<uint8_t>(), chunk_count.as<int>());
        hipLaunchKernelGGL(k_models, grid_h, dim3(kThreads), 0, s, d_src, d_dst, stride_floats, d_offsets, seeds.as<uint64_t>(), pair0, P,
                           flags.as<uint8_t>(), chunk_count.as<int>(), models.as<double>(), model_h.as<int>(), n_valid.as<int>());
        if (stage_ms) MRS_HIP_TRY(hipEventRecord(ev[1], s));
        if (n_tiles) {
            MRS_HIP_TRY(hipMemsetAsync(counts.p, 0, (size_t)np * H * sizeof(int), s));
            // the grid's x holds the tiles (up to 2^31 - 1), y the model blocks (at most 256)
            hipLaunchKernelGGL(k_score, dim3((unsigned)n_tiles, (unsigned)n_chunks), dim3(kThreads), 0, s, d_src, d_dst, stride_floats, d_offsets,
                               tiles.as<int2>() + tile_first[round], pair0, P, models.as<double>(), n_valid.as<int>(), counts.as<int>());
        }
        if (stage_ms) MRS_HIP_TRY(hipEventRecord(ev[2], s));
        hipLaunchKernelGGL(k_refit, dim3((unsigned)np), dim3(kThreads), 0, s, d_src, d_dst, stride_floats, d_offsets, pair0, P, models.as<double>(),
                           model_h.as<int>(), n_valid.as<int>(), counts.as<int>(), cur_mask.as<uint8_t>(), d_T, d_info, d_mask);
        MRS_HIP_TRY(hipGetLastError());
        if (stage_ms) {
            MRS_HIP_TRY(hipEventRecord(ev[3], s));
            MRS_HIP_TRY(hipEventSynchronize(ev[3]));
            for (int k = 0; k < 3; ++k) {
                float ms = 0.f;
                MRS_HIP_TRY(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
                stage_ms[k] += ms;
            }
        }
    }
    return MRS_OK;
}

}  // namespace

extern "C" {

int mrs_ransac_pose_batch(mrs_ctx* ctx, const float* d_src, const float* d_dst, int32_t stride_floats, const int64_t* d_offsets,
                          const int64_t* h_offsets, int32_t n_pairs, const uint64_t* h_seeds, const mrs_ransac_params* params,
                          double* d_T, int32_t* d_info, uint8_t* d_mask, mrs_stream stream)
{
    return ransac_run(ctx, d_src, d_dst, stride_floats, d_offsets, h_offsets, n_pairs, h_seeds, params, d_T, d_info, d_mask, (hipStream_t)stream,
                      nullptr);
}

int mrs_ransac_pose_batch_profile(mrs_ctx* ctx, const float* d_src, const float* d_dst, int32_t stride_floats, const int64_t* d_offsets,
                                  const int64_t* h_offsets, int32_t n_pairs, const uint64_t* h_seeds, const mrs_ransac_params* params,
                                  double* d_T, int32_t* d_info, uint8_t* d_mask, float* h_stage_ms, mrs_stream stream)
{
    MRS_REQUIRE(h_stage_ms, "null pointer");
    return ransac_run(ctx, d_src, d_dst, stride_floats, d_offsets, h_offsets, n_pairs, h_seeds, params, d_T, d_info, d_mask, (hipStream_t)stream,
                      h_stage_ms);
}

}  // extern "C"
