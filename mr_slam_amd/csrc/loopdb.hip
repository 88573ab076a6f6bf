// loopdb.hip -- device-resident, append-as-you-go descriptor database of one robot (C ABI mrs_loopdb_*).
//
// What it replaces: the Python lists the LoopDetection nodes keep per robot and walk for every new scan --
// TIRING1/2/3 + `for idx in range(len(pc_candidates)): fast_corr(TIRING_current, TIRING_candidates[idx])`
// (RING_ros/main_RING.py:126-140, 284-288), the RING++ twin (main_RINGplusplus.py:126-134) and the DiSCO node's
// `KDTree(np.array(DiSCO_candidates)).query(...)` + `phase_corr(FFT_candidates[idx], fft_current)` (disco_ros/main.py:276-291).
// There one descriptor is appended per callback (host tensors) and a query costs one torch FFT correlation per stored
// entry; here the entries live in HBM in the format the sweep kernels stream (RING: DMA-tiled half spectra, ringfft.hip),
// an append is one small copy / transform into the next slot (capacity doubles when it runs out: no re-upload), and a
// query is ONE sweep launch + one copy of (dist, angle) per entry + the `dist < threshold` filter in index order.
// All work of a handle runs on the handle's own stream; calls are serialised by a mutex (the reference's callbacks run on
// concurrent rospy threads, each appending to its own list and reading the other robots').
// Scan Context (MRS_LOOPDB_SC) replaces the ring-key KDTree + dist_align_sc of main_SC.py:153-172: entries are packed descriptors with their
// sector keys and column norms (scancontext.hip), the ring keys a dense [n][120] array; a query is a nearest-key sweep + one alignment launch.
// M2DP (MRS_LOOPDB_M2DP) keeps the 192-d descriptors of m2dp.hip as float32 rows; a query is mrs_signature_knn over them.
// Fast Histogram (MRS_LOOPDB_FH) keeps the range histograms of fasthist.hip as fp64 rows of `bins` doubles; a query is one sweep that evaluates
// getEMD (pr_methods/FastHistogram.py:66-72) against every entry with the reference's order of additions, then the k smallest on the host.
//
// The handle (struct mrs_loopdb) owns everything through members that free themselves: its stream and the ev_in / ev_out pair
// (mrs::HandleStream, declared first and so destroyed last), every device array (mrs::DeviceBuffer<T>), every pinned array
// (mrs::PinnedBuffer<T>), the stage slots (pinned block + event).  Destroying a handle is `delete`; a create that fails half way deletes what
// it has.  Growing (reserve_locked) allocates the new arrays as locals, copies, synchronises and only then moves them into the handle.
// What a kind keeps per entry and takes as an argument is one table: layout_of() below.  The small result of a top-k query is one struct
// per kind (ScTopK, M2dpTopK, DiscoBest); the distance rows of an all-entries query are bytes read through dist_angle() / dist_f64().
//
// Arguments.  A call's descriptor is on the host or on the device (`form` / `on_device`); `stream` is the caller's stream for a device one.
//   in   arg_in():  device -> HandleStream::join_in(stream), the handle's stream then reads the caller's pointer;
//                   host   -> upload(): the next of four pinned slots (waiting for the slot's previous copy), ONE copy to d_in or to the
//                             place the call names, the slot's event recorded.
//   out  arg_out(): device -> HandleStream::release_to(stream): the caller's stream passes once the handle's has read the argument; host -> nothing.
// Per call, in stream order (H = host argument, D = device argument; "sync" = hipStreamSynchronize of the handle's stream):
//   call                 H                                               D
//   append  RING         upload -> d_query; tile                         join; copy -> d_query; tile; release
//   append  RING++       upload -> d_in; normalise; spectrum; tile       join; normalise; spectrum; tile; release
//   append  half spectra -                                               join; tile from the caller's pointer; release
//   query   RING family  as append up to d_query; sweep; copy rows; sync the same, no release (the sync covers it)
//   query_multi          per descriptor as append into scratch; sweep;   join; ONE copy of all spectra (or per descriptor as append);
//                        2 x copy 2D; sync                               sweep; 2 x copy 2D; release; sync
//   append_disco         upload -> signature slot; upload -> spectrum    join (once, for both); copy; copy; release
//                        slot (two pinned slots, two copies)
//   query_disco          upload of signature | spectrum -> d_in (ONE     join (once); nearest; phase (writes the pinned result); sync
//                        slot, ONE copy); nearest; phase; sync
//   append_sc            upload -> d_in; pack                            join; pack; release
//   query_sc             upload -> d_in; pack; nearest; align;           join; pack; nearest; align; release; copy result; sync
//                        copy result; sync
//   query_sc_all         upload -> d_in; pack; align; copy rows; sync    join; pack; align; release; copy rows; sync
//   append_m2dp          upload -> d_in; to float32 in the slot          join; to float32; release
//   query_m2dp           upload -> d_in; to float32; knn; copy result;   join; to float32; release; knn; copy result; sync
//                        sync
//   append_fh            upload -> the entry's slot                      join; copy -> the slot; release
//   query_fh             upload -> d_in; distances; copy rows; sync      join; distances; release; copy rows; sync
//   distances_fh         join (for d_dist); upload -> d_in; distances;   join (for d_dist); join; distances; release
//                        release
#include "common.hpp"
#include "fft_codelets.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <memory>

namespace {

constexpr int kA = 120, kD = 120, kHalf = 61;
constexpr size_t kSpecFloats = (size_t)kHalf * kD * 2;       // one [61][120] complex64 plane
constexpr size_t kTiledFloats = MRS_RING_TILED_ENTRY_BYTES / 4;
constexpr int kStageSlots = 4;

constexpr int kScDim = 120, kScMaxK = 64;
constexpr int kM2dpDim = 192, kM2dpMaxK = 32;

// Fast Histogram sweep: a workgroup scores kFhEntries entries, kFhChunk buckets at a time
constexpr int kFhMaxBins = MRS_FH_MAX_BINS, kFhMaxK = 32, kFhEntries = 64, kFhChunk = 64, kFhThreads = 256;

// The small result of a query, one block per kind: the kernels write its fields on the device and ONE copy brings the block to the host
// (DiSCO's kernel writes the pinned block itself).
struct ScTopK { int32_t idx[kScMaxK]; float dist[kScMaxK]; int32_t shift[kScMaxK]; double key_d2[kScMaxK]; };   // key_d2: squared key distance
struct M2dpTopK { int32_t idx[kM2dpMaxK]; float d2[kM2dpMaxK]; };
struct DiscoBest { int32_t index; float dist2; int32_t argmax; int32_t pad; };
static_assert(sizeof(ScTopK) == 5 * kScMaxK * 4 && offsetof(ScTopK, key_d2) == 3 * kScMaxK * 4, "SC result block layout");
static_assert(sizeof(M2dpTopK) == 2 * kM2dpMaxK * 4, "M2DP result block layout");
static_assert(sizeof(DiscoBest) == 16, "DiSCO result block layout");

// What a kind keeps and takes, from (kind, channels of RING++ or bins of FH):
//   kind    entry (floats to the next)              argument in the reference's form (floats)  sig_dim          stage slot         slack
//   RING    one DMA-tiled plane                     [120][120] complex64                       -                the argument       1 entry
//   RING++  C DMA-tiled planes                      [C][120][120] float32                      -                the argument       1 entry
//   DiSCO   spectrum [40][120] complex64            the spectrum                               1024 signature   signature|spectrum -
//   SC      packed entry (scancontext.hip)          [120][120] float32                         120 ring key     the argument       -
//   M2DP    192 float32                             192 doubles                                -                the argument       -
//   FH      `bins` doubles                          `bins` doubles                             -                the argument       -
// slack: the tiled sweep reads up to 1 KiB past the last entry, so the tiled kinds keep one zeroed entry behind the capacity.
struct Layout {
    size_t entry_floats = 0;      // floats from one entry of d_entries to the next
    size_t in_floats = 0;         // floats of one argument
    int sig_dim = 0;              // floats per row of d_sigs (0: the kind keeps none)
    size_t stage_bytes = 0;       // bytes of one pinned stage slot
    bool slack = false;
};
constexpr int kPR = 40, kPS = 120;      // DiSCO spectrum rows x columns
Layout layout_of(int kind, int channels_or_bins)
{
    const size_t c = (size_t)channels_or_bins;
    Layout L;
    switch (kind) {
    case MRS_LOOPDB_RING: L.entry_floats = kTiledFloats; L.in_floats = (size_t)kA * kD * 2; L.slack = true; break;
    case MRS_LOOPDB_RINGPP: L.entry_floats = c * kTiledFloats; L.in_floats = c * kA * kD; L.slack = true; break;
    case MRS_LOOPDB_DISCO: L.entry_floats = L.in_floats = (size_t)kPR * kPS * 2; L.sig_dim = 1024; break;
    case MRS_LOOPDB_SC: L.entry_floats = mrs::sc_entry_floats(kScDim, kScDim); L.in_floats = (size_t)kScDim * kScDim; L.sig_dim = kScDim; break;
    case MRS_LOOPDB_M2DP: L.entry_floats = kM2dpDim; L.in_floats = 2 * (size_t)kM2dpDim; break;
    default: L.entry_floats = L.in_floats = 2 * c; break;      // MRS_LOOPDB_FH
    }
    L.stage_bytes = (L.in_floats + (kind == MRS_LOOPDB_DISCO ? (size_t)L.sig_dim : 0)) * sizeof(float);
    return L;
}

// A pinned block a host argument passes through, and the event after which it may be overwritten
struct StageSlot {
    mrs::PinnedBuffer<char> p;
    mrs::Event ev;
    bool used = false;
};

template <class T>
struct ResultBlock {
    mrs::DeviceBuffer<T> d;
    mrs::PinnedBuffer<T> h;
    int alloc()
    {
        MRS_TRY(d.reserve(1, 1));
        return h.reserve(1, 1);
    }
};

// ---- DiSCO query kernels ---------------------------------------------------------------------------------------------
// nearest signature by squared L2 distance in the difference form (what a kd-tree's L2 metric evaluates); one wave per signature
// at a time, 4 KiB per signature streamed as 4 x float4 per lane; winners merged with a 64-bit atomicMin on (distance bits, index).
__global__ __launch_bounds__(256) void k_sig_nearest(const float* __restrict__ q, const float* __restrict__ db, int n, int dim,
                                                     unsigned long long* __restrict__ best)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    unsigned long long mine = ~0ull;
    for (int i = wave; i < n; i += nwaves) {
        const float* r = db + (size_t)i * dim;
        float acc = 0.0f;
        for (int c = lane * 4; c < dim; c += 256) {
            const float4 a = *reinterpret_cast<const float4*>(q + c);
            const float4 b = *reinterpret_cast<const float4*>(r + c);
            float d = a.x - b.x; acc = __builtin_fmaf(d, d, acc);
            d = a.y - b.y; acc = __builtin_fmaf(d, d, acc);
            d = a.z - b.z; acc = __builtin_fmaf(d, d, acc);
            d = a.w - b.w; acc = __builtin_fmaf(d, d, acc);
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        const unsigned long long key = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)i;
        mine = key < mine ? key : mine;
    }
    if (lane == 0 && mine != ~0ull) atomicMin(best, mine);
}

// phase_corr(a = candidate, b = current) for the ONE candidate the search picked (disco_ros/main.py:260-272, 288-291):
// corr = ifft2(a conj(b), ortho), |corr| (+ 1e-15 under the root), fftshift2d, first maximum.  One workgroup, everything in LDS, 40 x 120:
// rows: 120-point inverse transforms as two in-register 60-point codelets (even / odd samples; 80 lanes) + one radix-2 step;
// columns: 40-point direct transforms (192 k complex multiply-adds spread over 960 work items, the lane's 40 inputs in registers).
constexpr int kPhaseThreads = 512;
__global__ __launch_bounds__(kPhaseThreads) void k_disco_phase_one(const float2* __restrict__ spectra, unsigned long long* __restrict__ best,
                                                                   const float2* __restrict__ cur, const float2* __restrict__ tw,
                                                                   int* __restrict__ out_index, float* __restrict__ out_d2, int* __restrict__ out_arg)
{
    extern __shared__ float2 sm[];        // A [R][S] | B [R][S] | twiddles exp(+2 pi i k / S), k < S | exp(+2 pi i k / R), k < R
    float2* A = sm;
    float2* B = sm + kPR * kPS;
    float2* twS = B + kPR * kPS;
    float2* twR = twS + kPS;
    __shared__ float bv[kPhaseThreads / 64];
    __shared__ int bi[kPhaseThreads / 64];
    const int t = threadIdx.x;
    const unsigned long long won = *best;                      // (distance bits, index) of the nearest signature
    const int idx = (int)(unsigned)(won & 0xffffffffull);
    const float2* a = spectra + (size_t)idx * kPR * kPS;
    for (int i = t; i < kPR * kPS; i += kPhaseThreads) {
        const float2 x = a[i], y = cur[i];                     // x conj(y)
        A[i] = make_float2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y);
    }
    for (int i = t; i < kPS; i += kPhaseThreads) twS[i] = tw[i];
    for (int i = t; i < kPR; i += kPhaseThreads) twR[i] = tw[kPS + i];
    __syncthreads();
    if (t < 2 * kPR) {                                         // E / O: 60-point inverse transforms of a row's even / odd samples
        const int r = t >> 1, par = t & 1;
        v2f x[60];
#pragma unroll
        for (int m = 0; m < 60; ++m) { const float2 v = A[r * kPS + 2 * m + par]; x[m] = (v2f){v.x, v.y}; }
        cfft60_inv(x);
#pragma unroll
        for (int k = 0; k < 60; ++k) B[r * kPS + par * 60 + k] = make_float2(x[k].x, x[k].y);
    }
    __syncthreads();
    for (int o = t; o < kPR * kPS; o += kPhaseThreads) {      // X[n] = E[n mod 60] + w^n O[n mod 60]
        const int r = o / kPS, n = o - r * kPS, k = n >= 60 ? n - 60 : n;
        const float2 e = B[r * kPS + k], od = B[r * kPS + 60 + k], w = twS[n];
        A[o] = make_float2(e.x + (w.x * od.x - w.y * od.y), e.y + (w.x * od.y + w.y * od.x));
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)(kPR * kPS));
    float bestv = -1.0f;
    int bidx = 0x7fffffff;
    for (int wi = t; wi < 8 * kPS; wi += kPhaseThreads) {     // work item = (column n, 5 consecutive output rows)
        const int g = wi / kPS, n = wi - g * kPS;
        float2 in[kPR];
#pragma unroll
        for (int j = 0; j < kPR; ++j) in[j] = A[j * kPS + n];
        for (int mm = 0; mm < 5; ++mm) {
            const int m = g * 5 + mm;
            float re = 0.0f, im = 0.0f;
            int k = 0;
#pragma unroll
            for (int j = 0; j < kPR; ++j) {
                const float2 w = twR[k];
                re = __builtin_fmaf(in[j].x, w.x, __builtin_fmaf(-in[j].y, w.y, re));
                im = __builtin_fmaf(in[j].x, w.y, __builtin_fmaf(in[j].y, w.x, im));
                k += m; if (k >= kPR) k -= kPR;
            }
            re *= scale; im *= scale;
            const float tot = sqrtf(re * re + im * im + 1e-15f);
            // fftshift2d (even sizes): source (m, n) appears at ((m + R/2) % R, (n + S/2) % S) of the shifted map
            const int flat = ((m + kPR / 2) % kPR) * kPS + (n + kPS / 2) % kPS;
            if (tot > bestv || (tot == bestv && flat < bidx)) { bestv = tot; bidx = flat; }
        }
    }
    const int wave = t >> 6, lane = t & 63;
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bestv, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (ov > bestv || (ov == bestv && oi < bidx)) { bestv = ov; bidx = oi; }
    }
    if (lane == 0) { bv[wave] = bestv; bi[wave] = bidx; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kPhaseThreads / 64; ++w)
            if (bv[w] > bestv || (bv[w] == bestv && bi[w] < bidx)) { bestv = bv[w]; bidx = bi[w]; }
        // the three results go straight to pinned host memory (no copy after the kernel: the stream synchronisation that follows makes them
        // visible), and `best` is armed for the next query (no memset before it)
        *out_arg = bidx;
        *out_index = idx;
        *out_d2 = __uint_as_float((unsigned)(won >> 32));
        __threadfence_system();
        *best = ~0ull;
    }
}

// an M2DP descriptor as the builder writes it (fp64) -> the float32 row the database keeps
__global__ void k_m2dp_to_float(const double* __restrict__ src, float* __restrict__ dst)
{
    if (threadIdx.x < kM2dpDim) dst[threadIdx.x] = (float)src[threadIdx.x];
}

// getEMD(q, entry) for every entry: dist[e] = (sum over i, in index order, of |q_i - entry_i|) / bins, all fp64 -- the order of the
// additions is the reference's, so the bits are.  A workgroup takes kFhEntries consecutive entries (rows of `bins` doubles, contiguous in
// memory): all its threads bring a [kFhEntries][kFhChunk] block of buckets into LDS with coalesced reads (row stride kFhChunk + 1 doubles:
// the lanes of the walk below hit different banks), then lane e of the first wave walks row e of the block in order, its running sum kept
// in a register from one block to the next.
__global__ __launch_bounds__(kFhThreads) void k_fh_distances(const double* __restrict__ q, const double* __restrict__ entries, int n, int bins,
                                                             double* __restrict__ dist)
{
    __shared__ double blk[kFhEntries * (kFhChunk + 1)];
    __shared__ double qs[kFhMaxBins];
    const int t = threadIdx.x;
    const int e0 = blockIdx.x * kFhEntries;
    const int ne = min(kFhEntries, n - e0);
    for (int i = t; i < bins; i += kFhThreads) qs[i] = q[i];
    double acc = 0.0;
    for (int c0 = 0; c0 < bins; c0 += kFhChunk) {
        const int nc = min(kFhChunk, bins - c0);
        __syncthreads();                                     // the previous block has been walked (and qs is written, the first time)
        for (int i = t; i < ne * nc; i += kFhThreads) {
            const int r = i / nc, c = i - r * nc;
            blk[r * (kFhChunk + 1) + c] = entries[(size_t)(e0 + r) * bins + c0 + c];
        }
        __syncthreads();
        if (t < ne)
            for (int c = 0; c < nc; ++c) acc += fabs(qs[c0 + c] - blk[t * (kFhChunk + 1) + c]);
    }
    if (t < ne) dist[e0 + t] = acc / (double)bins;
}

}  // namespace

struct mrs_loopdb {
    mrs::HandleStream s;                      // first: destroyed last, after the buffers whose work it carried
    mrs_ctx* ctx = nullptr;
    int kind = 0;
    int channels = 1;                         // RING: 1; RING++: planes per entry
    int bins = 0;                             // FH: buckets per histogram
    Layout L;
    int n = 0, cap = 0;
    mrs::DeviceBuffer<float> d_entries;       // [cap (+ 1 of slack)] entries, L.entry_floats apart (FH: rows of doubles)
    mrs::DeviceBuffer<float> d_sigs;          // [cap][L.sig_dim]: DiSCO signatures, SC ring keys
    // Distance rows of an all-entries query, kRowBytes per entry of capacity: [n] float distances | [n] int32 angles or shifts back to back
    // (wherever n stands: ONE copy brings both to the host), or [n] doubles (FH).  Read through dist_angle() / dist_f64() only.
    mrs::DeviceBuffer<char> d_rows;
    mrs::PinnedBuffer<char> h_rows;
    mrs::DeviceBuffer<float> d_in;            // a host argument on the device (L.stage_bytes)
    mrs::DeviceBuffer<float> d_tmp;           // RING++: the normalised channels; SC: the query's ring key
    mrs::DeviceBuffer<float> d_query;         // the query in database form (RING family: row layout [C][61][120] complex64)
    ResultBlock<ScTopK> sc;
    ResultBlock<M2dpTopK> m2dp;
    struct {
        int R = kPR, S = kPS;
        mrs::DeviceBuffer<float> d_tw;                  // exp(+2 pi i k / S), k < S, then exp(+2 pi i k / R), k < R
        mrs::DeviceBuffer<unsigned long long> d_best;   // packed (distance bits, index)
        mrs::PinnedBuffer<DiscoBest> h_result;          // written by k_disco_phase_one
        bool phase_attr_set = false;                    // the phase kernel's LDS attribute has been set on this handle's device
    } disco;
    StageSlot stage[kStageSlots];
    int stage_next = 0;
    std::mutex mu;

    ~mrs_loopdb() { if (s) (void)hipStreamSynchronize(s); }      // nothing queued outlives the buffers
};

namespace {

constexpr size_t kRowBytes = sizeof(float) + sizeof(int32_t);
static_assert(kRowBytes == sizeof(double), "a distance row holds (float, int32) pairs or doubles");
struct DistAngle { float* dist; int32_t* angle; };
DistAngle dist_angle(char* rows, int n)
{
    float* d = reinterpret_cast<float*>(rows);
    return {d, reinterpret_cast<int32_t*>(d + n)};
}
double* dist_f64(char* rows) { return reinterpret_cast<double*>(rows); }

// The one place that tells a call it has the wrong kind of database
enum Want { kWantRingAppend, kWantRingQuery, kWantDisco, kWantSc, kWantM2dp, kWantFh };
int require_kind(const mrs_loopdb* db, Want w)
{
    static const struct { int kind; const char *msg, *cond; } rule[] = {
        {MRS_LOOPDB_RING, "not a RING / RING++ database (DiSCO: mrs_loopdb_append_disco, SC: mrs_loopdb_append_sc, M2DP: mrs_loopdb_append_m2dp, FH: mrs_loopdb_append_fh)",
         "db->kind == MRS_LOOPDB_RING || db->kind == MRS_LOOPDB_RINGPP"},
        {MRS_LOOPDB_RING, "not a RING / RING++ database (DiSCO: mrs_loopdb_query_disco, SC: mrs_loopdb_query_sc, M2DP: mrs_loopdb_query_m2dp, FH: mrs_loopdb_query_fh)",
         "db->kind == MRS_LOOPDB_RING || db->kind == MRS_LOOPDB_RINGPP"},
        {MRS_LOOPDB_DISCO, "not a DiSCO database", "db->kind == MRS_LOOPDB_DISCO"},
        {MRS_LOOPDB_SC, "not a Scan Context database (FH: mrs_loopdb_append_fh / mrs_loopdb_query_fh)", "db->kind == MRS_LOOPDB_SC"},
        {MRS_LOOPDB_M2DP, "not an M2DP database (FH: mrs_loopdb_append_fh / mrs_loopdb_query_fh)", "db->kind == MRS_LOOPDB_M2DP"},
        {MRS_LOOPDB_FH, "not a Fast Histogram database", "db->kind == MRS_LOOPDB_FH"},
    };
    if (db->kind == rule[w].kind || (rule[w].kind == MRS_LOOPDB_RING && db->kind == MRS_LOOPDB_RINGPP)) return MRS_OK;
    mrs::set_error("bad argument: %s (%s)", rule[w].msg, rule[w].cond);
    return MRS_ERR_ARG;
}

// Capacity >= want (doubling), lock held: new buffers as locals, what is there copied on the handle's stream, one synchronisation, then the
// handle takes them.  Nothing of the handle is touched before every allocation and copy has succeeded, and a failure frees the locals on the
// way out: a retry after an out-of-memory error starts from where the first attempt did.
int reserve_locked(mrs_loopdb* db, int want)
{
    if (want <= db->cap) return MRS_OK;
    int cap = std::max(db->cap, 256);
    while (cap < want) cap *= 2;
    const Layout& L = db->L;
    mrs::DeviceBuffer<float> entries, sigs;
    mrs::DeviceBuffer<char> d_rows;
    mrs::PinnedBuffer<char> h_rows;
    const size_t ne = ((size_t)cap + (L.slack ? 1 : 0)) * L.entry_floats, ns = (size_t)cap * L.sig_dim, nr = (size_t)cap * kRowBytes;
    MRS_TRY(entries.reserve(ne, ne));
    if (L.slack) MRS_HIP_TRY(hipMemsetAsync(entries.get() + (size_t)cap * L.entry_floats, 0, L.entry_floats * sizeof(float), db->s));
    if (ns > 0) MRS_TRY(sigs.reserve(ns, ns));
    MRS_TRY(d_rows.reserve(nr, nr));
    MRS_TRY(h_rows.reserve(nr, nr));
    if (db->n > 0) {
        MRS_HIP_TRY(hipMemcpyAsync(entries.get(), db->d_entries.get(), (size_t)db->n * L.entry_floats * sizeof(float), hipMemcpyDeviceToDevice, db->s));
        if (ns > 0) MRS_HIP_TRY(hipMemcpyAsync(sigs.get(), db->d_sigs.get(), (size_t)db->n * L.sig_dim * sizeof(float), hipMemcpyDeviceToDevice, db->s));
    }
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    db->d_entries = std::move(entries); db->d_sigs = std::move(sigs); db->d_rows = std::move(d_rows); db->h_rows = std::move(h_rows);
    db->cap = cap;
    return MRS_OK;
}

// ---- Arguments in and out ------------------------------------------------------------------------------------------------------------
// Host parts -> device buffer `dst` through ONE pinned slot and ONE copy (the caller's memory is free again when this returns).  Two parts
// land back to back: DiSCO's signature | spectrum.
struct Part { const void* p; size_t bytes; };
int upload(mrs_loopdb* db, void* dst, Part a, Part b = {nullptr, 0})
{
    StageSlot& slot = db->stage[db->stage_next];
    db->stage_next = (db->stage_next + 1) % kStageSlots;
    if (slot.used) MRS_HIP_TRY(hipEventSynchronize(slot.ev));
    memcpy(slot.p.get(), a.p, a.bytes);
    if (b.bytes) memcpy(slot.p.get() + a.bytes, b.p, b.bytes);
    MRS_HIP_TRY(hipMemcpyAsync(dst, slot.p.get(), a.bytes + b.bytes, hipMemcpyHostToDevice, db->s));
    MRS_HIP_TRY(hipEventRecord(slot.ev, db->s));
    slot.used = true;
    return MRS_OK;
}

// Argument in: *src is where the handle's stream may read the `bytes` of `arg`.  A device argument is the caller's own pointer once the
// handle's stream has joined `user`; a host argument is staged into `host_dst` (d_in unless a call has a better place) and read from there.
int arg_in(mrs_loopdb* db, const void* arg, size_t bytes, bool on_device, mrs_stream user, const void** src, void* host_dst = nullptr)
{
    if (on_device) {
        *src = arg;
        return db->s.join_in((hipStream_t)user);
    }
    if (!host_dst) host_dst = db->d_in.get();
    *src = host_dst;
    return upload(db, host_dst, {arg, bytes});
}

// Argument out: the caller may overwrite its device argument (or read a device result) once ITS stream has passed this point
int arg_out(mrs_loopdb* db, bool on_device, mrs_stream user)
{
    return on_device ? db->s.release_to((hipStream_t)user) : MRS_OK;
}

// a RING / RING++ descriptor in the given form -> row-layout half spectra [C][61][120] at `d_spec` (device), on the handle's stream
int to_half_spectrum(mrs_loopdb* db, const void* desc, int form, float* d_spec, mrs_stream user)
{
    const int C = db->channels;
    const bool on_device = form != MRS_LOOPDB_FORM_HOST;
    const void* src = nullptr;
    if (form == MRS_LOOPDB_FORM_DEVICE_SPEC || db->kind == MRS_LOOPDB_RING) {
        // half spectra already, or the reference's TIRING [1][120][120] complex64 (util.py:198) whose first 61 angle-frequency rows ARE the half
        // spectrum (C = 1): a host argument is staged straight into place, a device one copied there
        const size_t bytes = (size_t)C * kSpecFloats * sizeof(float);
        MRS_TRY(arg_in(db, desc, bytes, on_device, user, &src, d_spec));
        if (on_device) MRS_HIP_TRY(hipMemcpyAsync(d_spec, src, bytes, hipMemcpyDeviceToDevice, db->s));
        return MRS_OK;
    }
    // RING++: the reference's TIRING [C][120][120] float32 magnitudes; fast_corr_RINGplusplus normalises jointly and transforms along the
    // angle axis at every comparison (util.py:339-343) -- done once here
    MRS_TRY(arg_in(db, desc, db->L.in_floats * sizeof(float), on_device, user, &src));
    MRS_TRY(mrs_normalize_groups(db->ctx, static_cast<const float*>(src), db->d_tmp.get(), 1, C * kA * kD, db->s));
    return mrs_ring_half_spectrum(db->ctx, db->d_tmp.get(), C, kA, kD, d_spec, db->s);
}

}  // namespace

extern "C" {

int mrs_loopdb_create(mrs_ctx* ctx, int32_t kind, int32_t channels, int32_t capacity_hint, mrs_loopdb** out)
{
    MRS_REQUIRE(ctx && out, "null pointer");
    *out = nullptr;
    MRS_REQUIRE(kind == MRS_LOOPDB_RING || kind == MRS_LOOPDB_RINGPP || kind == MRS_LOOPDB_DISCO || kind == MRS_LOOPDB_SC ||
                kind == MRS_LOOPDB_M2DP || kind == MRS_LOOPDB_FH, "unknown kind");
    const int bins = kind == MRS_LOOPDB_FH ? channels : 0;                   // FH: `channels` carries the number of buckets
    MRS_REQUIRE(kind != MRS_LOOPDB_FH || (bins >= 1 && bins <= kFhMaxBins), "bins in 1..256 (the channels argument of a Fast Histogram database)");
    if (kind == MRS_LOOPDB_SC || kind == MRS_LOOPDB_M2DP || kind == MRS_LOOPDB_FH) channels = 1;      // ignored: one descriptor per entry
    MRS_REQUIRE(kind != MRS_LOOPDB_RING || channels == 1, "RING descriptors have one channel");
    MRS_REQUIRE(channels >= 1 && channels <= 16, "channels out of range");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mrs_loopdb> db(new mrs_loopdb());      // an early return deletes it: every member frees itself
    db->ctx = ctx; db->kind = kind; db->channels = channels; db->bins = bins;
    const Layout& L = db->L = layout_of(kind, kind == MRS_LOOPDB_FH ? bins : channels);
    MRS_TRY(db->s.create());
    for (StageSlot& p : db->stage) {
        MRS_TRY(p.p.reserve(L.stage_bytes, L.stage_bytes));
        MRS_TRY(p.ev.create());
    }
    const size_t n_in = L.stage_bytes / sizeof(float), n_query = std::max((size_t)channels * kSpecFloats, L.entry_floats);
    MRS_TRY(db->d_in.reserve(n_in, n_in));
    MRS_TRY(db->d_tmp.reserve(L.in_floats, L.in_floats));
    MRS_TRY(db->d_query.reserve(n_query, n_query));
    if (kind == MRS_LOOPDB_DISCO) {
        auto& D = db->disco;
        std::vector<float> tw(2 * (size_t)(D.S + D.R));
        for (int k = 0; k < D.S; ++k) { tw[2 * k] = (float)cos(2.0 * M_PI * k / D.S); tw[2 * k + 1] = (float)sin(2.0 * M_PI * k / D.S); }
        for (int k = 0; k < D.R; ++k) { tw[2 * (D.S + k)] = (float)cos(2.0 * M_PI * k / D.R); tw[2 * (D.S + k) + 1] = (float)sin(2.0 * M_PI * k / D.R); }
        MRS_TRY(D.d_tw.reserve(tw.size(), tw.size()));
        MRS_HIP_TRY(hipMemcpy(D.d_tw.get(), tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
        MRS_TRY(D.d_best.reserve(1, 1));
        MRS_HIP_TRY(hipMemset(D.d_best.get(), 0xff, sizeof(unsigned long long)));       // armed; k_disco_phase_one re-arms it after every query
        MRS_TRY(D.h_result.reserve(1, 1));
    }
    if (kind == MRS_LOOPDB_SC) MRS_TRY(db->sc.alloc());
    if (kind == MRS_LOOPDB_M2DP) MRS_TRY(db->m2dp.alloc());
    MRS_TRY(reserve_locked(db.get(), std::max(capacity_hint, 1)));      // nobody else holds the handle yet
    *out = db.release();
    return MRS_OK;
}

int mrs_loopdb_destroy(mrs_loopdb* db)
{
    if (!db) return MRS_OK;
    (void)hipSetDevice(db->ctx->device);
    delete db;
    return MRS_OK;
}

int mrs_loopdb_size(mrs_loopdb* db, int32_t* out_n)
{
    MRS_REQUIRE(db && out_n, "null pointer");
    std::lock_guard<std::mutex> lk(db->mu);
    *out_n = db->n;
    return MRS_OK;
}

int mrs_loopdb_reserve(mrs_loopdb* db, int32_t capacity)
{
    MRS_REQUIRE(db, "null pointer");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    return reserve_locked(db, capacity);
}

int mrs_loopdb_clear(mrs_loopdb* db)
{
    MRS_REQUIRE(db, "null pointer");
    std::lock_guard<std::mutex> lk(db->mu);
    db->n = 0;
    return MRS_OK;
}

int mrs_loopdb_append(mrs_loopdb* db, const void* descriptor, int32_t form, int32_t count, mrs_stream stream)
{
    MRS_REQUIRE(db && descriptor, "null pointer");
    MRS_TRY(require_kind(db, kWantRingAppend));
    MRS_REQUIRE(form == MRS_LOOPDB_FORM_HOST || form == MRS_LOOPDB_FORM_DEVICE || form == MRS_LOOPDB_FORM_DEVICE_SPEC, "unknown form");
    MRS_REQUIRE(count >= 1 && (count == 1 || form == MRS_LOOPDB_FORM_DEVICE_SPEC), "several entries per call only as device half spectra");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    MRS_TRY(reserve_locked(db, db->n + count));
    const int C = db->channels;
    const void* spec = db->d_query.get();
    if (form == MRS_LOOPDB_FORM_DEVICE_SPEC)               // already row-layout half spectra on the device: permuted straight into the slots
        MRS_TRY(arg_in(db, descriptor, 0, true, stream, &spec));
    else
        MRS_TRY(to_half_spectrum(db, descriptor, form, db->d_query.get(), stream));
    MRS_TRY(mrs_ring_spec_to_tiled(db->ctx, static_cast<const float*>(spec), count * C, db->d_entries.get() + (size_t)db->n * db->L.entry_floats, db->s));
    MRS_TRY(arg_out(db, form != MRS_LOOPDB_FORM_HOST, stream));
    db->n += count;
    return MRS_OK;
}

int mrs_loopdb_query(mrs_loopdb* db, const void* descriptor, int32_t form, float dist_threshold, int32_t max_out, int32_t* h_index,
                     float* h_dist, int32_t* h_angle, int32_t* h_count, int32_t all_capacity, float* h_all_dist, int32_t* h_all_angle, int32_t* h_n,
                     mrs_stream stream)
{
    MRS_REQUIRE(db && descriptor && h_count, "null pointer");
    MRS_TRY(require_kind(db, kWantRingQuery));
    MRS_REQUIRE(form == MRS_LOOPDB_FORM_HOST || form == MRS_LOOPDB_FORM_DEVICE || form == MRS_LOOPDB_FORM_DEVICE_SPEC, "unknown form");
    MRS_REQUIRE(max_out >= 0 && (max_out == 0 || (h_index && h_dist && h_angle)), "output arrays");
    MRS_REQUIRE(all_capacity >= 0 && (all_capacity == 0 || h_all_dist || h_all_angle), "all_capacity without an array");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    *h_count = 0;
    const int n = db->n;
    if (h_n) *h_n = n;                                     // the entries this call scored (another thread may append right after)
    if (n == 0) return MRS_OK;                             // `for idx in range(0)`: no candidates, no work
    MRS_TRY(to_half_spectrum(db, descriptor, form, db->d_query.get(), stream));
    const DistAngle d = dist_angle(db->d_rows.get(), n), h = dist_angle(db->h_rows.get(), n);
    MRS_TRY(mrs_ring_corr_fft_sweep_tiled(db->ctx, db->d_query.get(), db->d_entries.get(), n, db->channels, d.dist, d.angle, db->s));
    MRS_HIP_TRY(hipMemcpyAsync(h.dist, d.dist, (size_t)n * kRowBytes, hipMemcpyDeviceToHost, db->s));
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    // `if dist < cfg.dist_threshold: idxs.append(idx) ...` in index order (main_RING.py:133-140)
    int cnt = 0;
    for (int i = 0; i < n; ++i)
        if (h.dist[i] < dist_threshold) {
            if (cnt < max_out) { h_index[cnt] = i; h_dist[cnt] = h.dist[i]; h_angle[cnt] = h.angle[i]; }
            ++cnt;
        }
    *h_count = cnt;                                         // may exceed max_out: the caller then asks again with larger arrays
    const size_t m = (size_t)std::min(n, all_capacity);     // never past the caller's arrays, whatever was appended since it sized them
    if (h_all_dist) memcpy(h_all_dist, h.dist, m * sizeof(float));
    if (h_all_angle) memcpy(h_all_angle, h.angle, m * sizeof(int32_t));
    return MRS_OK;
}

int mrs_loopdb_query_multi(mrs_loopdb* db, const void* descriptors, int32_t form, int32_t count, int32_t all_capacity, float* h_all_dist,
                           int32_t* h_all_angle, int32_t* h_n, mrs_stream stream)
{
    MRS_REQUIRE(db && descriptors && h_all_dist && h_all_angle && h_n, "null pointer");
    MRS_TRY(require_kind(db, kWantRingQuery));
    MRS_REQUIRE(form == MRS_LOOPDB_FORM_HOST || form == MRS_LOOPDB_FORM_DEVICE || form == MRS_LOOPDB_FORM_DEVICE_SPEC, "unknown form");
    MRS_REQUIRE(count >= 1 && count <= 1024 && all_capacity >= 0, "count in 1..1024");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    const int n = db->n;
    *h_n = n;
    if (n == 0) return MRS_OK;
    const int C = db->channels;
    const size_t spec_floats = (size_t)C * kSpecFloats;
    mrs::Scratch qbuf, out;
    MRS_TRY(qbuf.alloc((size_t)count * spec_floats * sizeof(float), db->s));
    MRS_TRY(out.alloc((size_t)count * 2 * n * sizeof(float), db->s));
    float* d_q = qbuf.as<float>();
    if (form == MRS_LOOPDB_FORM_DEVICE_SPEC) {
        const void* src = nullptr;
        MRS_TRY(arg_in(db, descriptors, 0, true, stream, &src));
        MRS_HIP_TRY(hipMemcpyAsync(d_q, src, (size_t)count * spec_floats * sizeof(float), hipMemcpyDeviceToDevice, db->s));
    } else {
        for (int i = 0; i < count; ++i) {      // the caller's descriptors lie L.in_floats apart
            MRS_TRY(to_half_spectrum(db, static_cast<const float*>(descriptors) + (size_t)i * db->L.in_floats, form, d_q + (size_t)i * spec_floats, stream));
        }
    }
    float* d_dist = out.as<float>();                                     // [count][n] distances, then [count][n] angles
    int32_t* d_angle = reinterpret_cast<int32_t*>(d_dist + (size_t)count * n);
    MRS_TRY(mrs_ring_corr_fft_sweep_tiled_q(db->ctx, d_q, count, db->d_entries.get(), n, C, d_dist, d_angle, db->s));
    const size_t m = (size_t)std::min(n, all_capacity);
    if (m > 0) {
        MRS_HIP_TRY(hipMemcpy2DAsync(h_all_dist, (size_t)all_capacity * sizeof(float), d_dist, (size_t)n * sizeof(float), m * sizeof(float), count,
                                     hipMemcpyDeviceToHost, db->s));
        MRS_HIP_TRY(hipMemcpy2DAsync(h_all_angle, (size_t)all_capacity * sizeof(int32_t), d_angle, (size_t)n * sizeof(int32_t), m * sizeof(int32_t), count,
                                     hipMemcpyDeviceToHost, db->s));
    }
    MRS_TRY(arg_out(db, form != MRS_LOOPDB_FORM_HOST, stream));
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    return MRS_OK;
}

int mrs_loopdb_append_disco(mrs_loopdb* db, const float* signature, const float* spectrum, int32_t on_device, mrs_stream stream)
{
    MRS_REQUIRE(db && signature && spectrum, "null pointer");
    MRS_TRY(require_kind(db, kWantDisco));
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    MRS_TRY(reserve_locked(db, db->n + 1));
    float* sig = db->d_sigs.get() + (size_t)db->n * db->L.sig_dim;
    float* spec = db->d_entries.get() + (size_t)db->n * db->L.entry_floats;
    const size_t sb = (size_t)db->L.sig_dim * sizeof(float), eb = db->L.entry_floats * sizeof(float);
    // two arguments with a destination each, so not arg_in: one join covers a device pair, a host pair takes a slot and a copy each
    if (on_device) {
        MRS_TRY(db->s.join_in((hipStream_t)stream));
        MRS_HIP_TRY(hipMemcpyAsync(sig, signature, sb, hipMemcpyDeviceToDevice, db->s));
        MRS_HIP_TRY(hipMemcpyAsync(spec, spectrum, eb, hipMemcpyDeviceToDevice, db->s));
    } else {
        MRS_TRY(upload(db, sig, {signature, sb}));
        MRS_TRY(upload(db, spec, {spectrum, eb}));
    }
    MRS_TRY(arg_out(db, on_device, stream));
    db->n += 1;
    return MRS_OK;
}

int mrs_loopdb_query_disco(mrs_loopdb* db, const float* signature, const float* spectrum, int32_t on_device, int32_t* h_index, float* h_dist2,
                           int32_t* h_flat_argmax, mrs_stream stream)
{
    MRS_REQUIRE(db && signature && spectrum && h_index && h_dist2 && h_flat_argmax, "null pointer");
    MRS_TRY(require_kind(db, kWantDisco));
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    *h_index = -1; *h_dist2 = INFINITY; *h_flat_argmax = 0;
    const int n = db->n;
    if (n == 0) return MRS_OK;
    auto& D = db->disco;
    const float *sig = signature, *spec = spectrum;
    if (on_device) {
        MRS_TRY(db->s.join_in((hipStream_t)stream));
    } else {
        // signature | spectrum through ONE pinned slot and ONE copy
        MRS_TRY(upload(db, db->d_in.get(), {signature, (size_t)db->L.sig_dim * sizeof(float)}, {spectrum, db->L.entry_floats * sizeof(float)}));
        sig = db->d_in.get(); spec = db->d_in.get() + db->L.sig_dim;
    }
    const int blocks = std::max(1, std::min((n + 3) / 4, 4 * (db->ctx->num_cu > 0 ? db->ctx->num_cu : 256)));
    hipLaunchKernelGGL(k_sig_nearest, dim3(blocks), dim3(256), 0, db->s, sig, db->d_sigs.get(), n, db->L.sig_dim, D.d_best.get());
    const size_t lds = (size_t)(2 * D.R * D.S + D.S + D.R) * sizeof(float2);
    if (!D.phase_attr_set) {
        MRS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_disco_phase_one), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        D.phase_attr_set = true;
    }
    DiscoBest* res = D.h_result.get();
    hipLaunchKernelGGL(k_disco_phase_one, dim3(1), dim3(kPhaseThreads), lds, db->s, reinterpret_cast<const float2*>(db->d_entries.get()),
                       D.d_best.get(), reinterpret_cast<const float2*>(spec), reinterpret_cast<const float2*>(D.d_tw.get()), &res->index,
                       &res->dist2, &res->argmax);
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    *h_index = res->index;
    *h_dist2 = res->dist2;
    *h_flat_argmax = res->argmax;
    return MRS_OK;
}

// ---- Scan Context -------------------------------------------------------------------------------------------------------------------

namespace {
// the query descriptor -> packed entry at d_query + its ring key at d_tmp, on the handle's stream (lock held)
int sc_query_prep(mrs_loopdb* db, const float* sc, int32_t on_device, mrs_stream stream)
{
    const void* src = nullptr;
    MRS_TRY(arg_in(db, sc, db->L.in_floats * sizeof(float), on_device, stream, &src));
    return mrs::sc_pack(static_cast<const float*>(src), 1, kScDim, kScDim, db->d_query.get(), db->L.entry_floats, db->d_tmp.get(), nullptr, db->s);
}
}  // namespace

int mrs_loopdb_append_sc(mrs_loopdb* db, const float* sc, int32_t on_device, mrs_stream stream)
{
    MRS_REQUIRE(db && sc, "null pointer");
    MRS_TRY(require_kind(db, kWantSc));
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    MRS_TRY(reserve_locked(db, db->n + 1));
    const void* src = nullptr;
    MRS_TRY(arg_in(db, sc, db->L.in_floats * sizeof(float), on_device, stream, &src));
    MRS_TRY(mrs::sc_pack(static_cast<const float*>(src), 1, kScDim, kScDim, db->d_entries.get() + (size_t)db->n * db->L.entry_floats, db->L.entry_floats,
                      db->d_sigs.get() + (size_t)db->n * db->L.sig_dim, nullptr, db->s));
    MRS_TRY(arg_out(db, on_device, stream));
    db->n += 1;
    return MRS_OK;
}

int mrs_loopdb_query_sc(mrs_loopdb* db, const float* sc, int32_t on_device, int32_t num_candidates, double search_ratio, int32_t* h_index,
                        float* h_key_dist, float* h_dist, int32_t* h_shift, int32_t* h_count, mrs_stream stream)
{
    MRS_REQUIRE(db && sc && h_index && h_key_dist && h_dist && h_shift && h_count, "null pointer");
    MRS_TRY(require_kind(db, kWantSc));
    MRS_REQUIRE(num_candidates >= 1 && num_candidates <= kScMaxK, "num_candidates in 1..64");
    MRS_REQUIRE(std::isfinite(search_ratio) && search_ratio >= 0.0, "search_ratio >= 0");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    const int k = num_candidates;
    for (int i = 0; i < k; ++i) { h_index[i] = -1; h_key_dist[i] = INFINITY; h_dist[i] = 1.0f; h_shift[i] = 0; }
    *h_count = 0;
    const int n = db->n;
    if (n == 0) return MRS_OK;                             // `if len(Ringkey_candidates) < 1: return`
    MRS_TRY(sc_query_prep(db, sc, on_device, stream));
    ScTopK* d = db->sc.d.get();
    const ScTopK* h = db->sc.h.get();
    const int cnt = std::min(k, n);
    // KDTree(ring keys).query(k) then dist_align_sc(SC_candidate, SC_current, search_ratio) for each candidate (main_SC.py:159-167)
    MRS_TRY(mrs::sc_nearest(db->d_tmp.get(), db->d_sigs.get(), n, kScDim, k, d->idx, d->key_d2, db->s));
    MRS_TRY(mrs::sc_align(db->ctx, db->d_entries.get(), db->L.entry_floats, d->idx, cnt, db->d_query.get(), 0, kScDim, kScDim, 0,
                       mrs::sc_search_radius(search_ratio, kScDim), d->dist, d->shift, db->s));
    MRS_TRY(arg_out(db, on_device, stream));
    MRS_HIP_TRY(hipMemcpyAsync(db->sc.h.get(), d, sizeof(ScTopK), hipMemcpyDeviceToHost, db->s));
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    for (int i = 0; i < cnt; ++i) {
        h_index[i] = h->idx[i];
        h_key_dist[i] = (float)std::sqrt(h->key_d2[i]);
        h_dist[i] = h->dist[i];
        h_shift[i] = h->shift[i];
    }
    *h_count = cnt;
    return MRS_OK;
}

int mrs_loopdb_query_sc_all(mrs_loopdb* db, const float* sc, int32_t on_device, double search_ratio, int32_t all_capacity, float* h_all_dist,
                            int32_t* h_all_shift, int32_t* h_best, int32_t* h_n, mrs_stream stream)
{
    MRS_REQUIRE(db && sc && h_best && h_n, "null pointer");
    MRS_TRY(require_kind(db, kWantSc));
    MRS_REQUIRE(std::isfinite(search_ratio) && search_ratio >= 0.0, "search_ratio >= 0");
    MRS_REQUIRE(all_capacity >= 0 && (all_capacity == 0 || (h_all_dist && h_all_shift)), "all_capacity without arrays");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    const int n = db->n;
    *h_n = n;
    *h_best = -1;
    if (n == 0) return MRS_OK;
    MRS_TRY(sc_query_prep(db, sc, on_device, stream));
    const DistAngle d = dist_angle(db->d_rows.get(), n), h = dist_angle(db->h_rows.get(), n);
    MRS_TRY(mrs::sc_align(db->ctx, db->d_entries.get(), db->L.entry_floats, nullptr, n, db->d_query.get(), 0, kScDim, kScDim, 0,
                       mrs::sc_search_radius(search_ratio, kScDim), d.dist, d.angle, db->s));
    MRS_TRY(arg_out(db, on_device, stream));
    MRS_HIP_TRY(hipMemcpyAsync(h.dist, d.dist, (size_t)n * kRowBytes, hipMemcpyDeviceToHost, db->s));
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    int best = 0;                                          // first minimum over the entries, as a loop over them would keep it
    for (int i = 1; i < n; ++i)
        if (h.dist[i] < h.dist[best]) best = i;
    *h_best = best;
    const size_t m = (size_t)std::min(n, all_capacity);    // never past the caller's arrays
    if (m > 0) {
        memcpy(h_all_dist, h.dist, m * sizeof(float));
        memcpy(h_all_shift, h.angle, m * sizeof(int32_t));
    }
    return MRS_OK;
}

// ---- M2DP ---------------------------------------------------------------------------------------------------------------------------

namespace {
// the descriptor argument (192 doubles, host or device) -> float32 [192] at `dst`, on the handle's stream (lock held)
int m2dp_to_row(mrs_loopdb* db, const double* desc, int32_t on_device, mrs_stream stream, float* dst)
{
    const void* src = nullptr;
    MRS_TRY(arg_in(db, desc, kM2dpDim * sizeof(double), on_device, stream, &src));
    hipLaunchKernelGGL(k_m2dp_to_float, dim3(1), dim3(256), 0, db->s, static_cast<const double*>(src), dst);
    MRS_HIP_TRY(hipGetLastError());
    return arg_out(db, on_device, stream);
}
}  // namespace

int mrs_loopdb_append_m2dp(mrs_loopdb* db, const double* desc, int32_t on_device, mrs_stream stream)
{
    MRS_REQUIRE(db && desc, "null pointer");
    MRS_TRY(require_kind(db, kWantM2dp));
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    MRS_TRY(reserve_locked(db, db->n + 1));
    MRS_TRY(m2dp_to_row(db, desc, on_device, stream, db->d_entries.get() + (size_t)db->n * db->L.entry_floats));
    db->n += 1;
    return MRS_OK;
}

int mrs_loopdb_query_m2dp(mrs_loopdb* db, const double* desc, int32_t on_device, int32_t k, int32_t* h_index, float* h_dist2, int32_t* h_count,
                          mrs_stream stream)
{
    MRS_REQUIRE(db && desc && h_index && h_dist2 && h_count, "null pointer");
    MRS_TRY(require_kind(db, kWantM2dp));
    MRS_REQUIRE(k >= 1 && k <= kM2dpMaxK, "k in 1..32");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < k; ++i) { h_index[i] = -1; h_dist2[i] = INFINITY; }
    *h_count = 0;
    const int n = db->n;
    if (n == 0) return MRS_OK;
    MRS_TRY(m2dp_to_row(db, desc, on_device, stream, db->d_query.get()));
    M2dpTopK* d = db->m2dp.d.get();
    const M2dpTopK* h = db->m2dp.h.get();
    MRS_TRY(mrs_signature_knn(db->ctx, db->d_query.get(), 1, db->d_entries.get(), n, kM2dpDim, k, d->idx, d->d2, db->s));
    MRS_HIP_TRY(hipMemcpyAsync(db->m2dp.h.get(), d, sizeof(M2dpTopK), hipMemcpyDeviceToHost, db->s));
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    const int cnt = std::min(k, n);
    for (int i = 0; i < cnt; ++i) { h_index[i] = h->idx[i]; h_dist2[i] = h->d2[i]; }
    *h_count = cnt;
    return MRS_OK;
}

// ---- Fast Histogram -----------------------------------------------------------------------------------------------------------------

namespace {
// distances of `hist` (`bins` doubles, host or device) to the n entries -> d_dist [n] on the handle's stream (lock held, n > 0)
int fh_sweep(mrs_loopdb* db, const double* hist, int32_t on_device, mrs_stream stream, int n, double* d_dist)
{
    const void* src = nullptr;
    MRS_TRY(arg_in(db, hist, (size_t)db->bins * sizeof(double), on_device, stream, &src));
    hipLaunchKernelGGL(k_fh_distances, dim3((n + kFhEntries - 1) / kFhEntries), dim3(kFhThreads), 0, db->s, static_cast<const double*>(src),
                       reinterpret_cast<const double*>(db->d_entries.get()), n, db->bins, d_dist);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}
}  // namespace

int mrs_loopdb_append_fh(mrs_loopdb* db, const double* hist, int32_t on_device, mrs_stream stream)
{
    MRS_REQUIRE(db && hist, "null pointer");
    MRS_TRY(require_kind(db, kWantFh));
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    MRS_TRY(reserve_locked(db, db->n + 1));
    float* slot = db->d_entries.get() + (size_t)db->n * db->L.entry_floats;
    const size_t bytes = (size_t)db->bins * sizeof(double);
    const void* src = nullptr;
    MRS_TRY(arg_in(db, hist, bytes, on_device, stream, &src, slot));      // a host histogram is staged straight into its slot
    if (on_device) MRS_HIP_TRY(hipMemcpyAsync(slot, src, bytes, hipMemcpyDeviceToDevice, db->s));
    MRS_TRY(arg_out(db, on_device, stream));
    db->n += 1;
    return MRS_OK;
}

int mrs_loopdb_query_fh(mrs_loopdb* db, const double* hist, int32_t on_device, int32_t k, int32_t* h_index, double* h_dist, int32_t* h_count,
                        mrs_stream stream)
{
    MRS_REQUIRE(db && hist && h_index && h_dist && h_count, "null pointer");
    MRS_TRY(require_kind(db, kWantFh));
    MRS_REQUIRE(k >= 1 && k <= kFhMaxK, "k in 1..32");
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < k; ++i) { h_index[i] = -1; h_dist[i] = INFINITY; }
    *h_count = 0;
    const int n = db->n;
    if (n == 0) return MRS_OK;
    double* d_all = dist_f64(db->d_rows.get());
    double* h_all = dist_f64(db->h_rows.get());
    MRS_TRY(fh_sweep(db, hist, on_device, stream, n, d_all));
    MRS_TRY(arg_out(db, on_device, stream));
    MRS_HIP_TRY(hipMemcpyAsync(h_all, d_all, (size_t)n * kRowBytes, hipMemcpyDeviceToHost, db->s));
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    // the k smallest, ascending, ties to the lower index; a NaN distance (a NaN in either histogram) orders after every number
    const int cnt = std::min(k, n);
    std::vector<int32_t> order((size_t)n);
    for (int i = 0; i < n; ++i) order[i] = i;
    auto before = [h_all](int32_t a, int32_t b) {
        const double da = h_all[a], db_ = h_all[b];
        const bool na = da != da, nb = db_ != db_;
        if (na != nb) return nb;
        if (!na && da != db_) return da < db_;
        return a < b;
    };
    std::partial_sort(order.begin(), order.begin() + cnt, order.end(), before);
    for (int i = 0; i < cnt; ++i) { h_index[i] = order[i]; h_dist[i] = h_all[order[i]]; }
    *h_count = cnt;
    return MRS_OK;
}

int mrs_loopdb_distances_fh(mrs_loopdb* db, const double* hist, int32_t on_device, double* d_dist, mrs_stream stream)
{
    MRS_REQUIRE(db && hist, "null pointer");
    MRS_TRY(require_kind(db, kWantFh));
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    std::lock_guard<std::mutex> lk(db->mu);
    const int n = db->n;
    if (n == 0) return MRS_OK;
    MRS_REQUIRE(d_dist, "null pointer");
    MRS_TRY(db->s.join_in((hipStream_t)stream));             // the caller's earlier work on d_dist comes first
    MRS_TRY(fh_sweep(db, hist, on_device, stream, n, d_dist));
    return arg_out(db, true, stream);                        // `stream` waits for the sweep: its later work sees d_dist
}

int mrs_loopdb_device_entries(mrs_loopdb* db, const float** d_entries, const float** d_signatures, int32_t* out_n, int64_t* entry_floats)
{
    MRS_REQUIRE(db && d_entries && out_n, "null pointer");
    std::lock_guard<std::mutex> lk(db->mu);
    MRS_HIP_TRY(hipSetDevice(db->ctx->device));
    MRS_HIP_TRY(hipStreamSynchronize(db->s));
    *d_entries = db->d_entries.get();
    if (d_signatures) *d_signatures = db->d_sigs.get();
    *out_n = db->n;
    if (entry_floats) *entry_floats = (int64_t)db->L.entry_floats;
    return MRS_OK;
}

}  // extern "C"
