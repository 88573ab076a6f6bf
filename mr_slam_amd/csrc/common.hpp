// common.hpp -- shared host-side plumbing of libmrslam_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/mrslam_hip.h"

namespace mrs {
constexpr int kMaxGridY = 65535;  // HIP grid limit in y: entry points that put the batch there check or chunk


void set_error(const char* fmt, ...);

// Development switches (they force a production path, or the reference a test compares against) are read from the environment ONLY when
// MRS_DEV=1 is set as well, and each active one is announced on stderr once: a stray variable in a production environment can neither
// change results nor add synchronisation silently.  Returns the variable's value, or nullptr.
const char* dev_env(const char* name);

#define MRS_HIP_TRY(expr)                                                                   \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess) {                                                            \
            ::mrs::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                             __LINE__);                                                     \
            return MRS_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

// a step that returns a status of its own (and has set the error text): anything but MRS_OK ends the calling function with it
#define MRS_TRY(expr)                         \
    do {                                      \
        const int st__ = (expr);              \
        if (st__ != MRS_OK) return st__;      \
    } while (0)

#define MRS_REQUIRE(cond, msg)                                  \
    do {                                                           \
        if (!(cond)) {                                             \
            ::mrs::set_error("bad argument: %s (%s)", msg, #cond); \
            return MRS_ERR_ARG;                                    \
        }                                                          \
    } while (0)

// Scratch buffer of one call, handed out by a small caching allocator of this library (capi.hip): blocks are
// hipMalloc'ed once and recycled.  A released block carries an event recorded on the stream that used it; it is handed
// out again to the SAME stream at once (stream order makes that safe) and to another stream only after the event has
// completed.  Not hipMallocAsync: with a second process active on the same GPU, small stream-ordered-pool allocations
// were observed to come back overlapping (the memset of one scratch buffer zeroed its neighbour: 6-7 of 30 runs of the
// adapter test under a GPU-holding parent process; 0 of 40 with plain allocations), silently corrupting results.
void* scratch_acquire(size_t bytes, hipStream_t stream);
void scratch_release(void* p, hipStream_t stream);
// A handle that owns a stream calls this before hipStreamDestroy: it waits for the stream and gives every idle block last used on it a
// fresh event and no stream, so that the cache never queries an event whose stream no longer exists and never takes a new stream at
// the old address for the old one.  (Seen in some runs of a long process, DESIGN.md has the counts: a RING query's launch check reported "operation not permitted when
// stream is capturing" although nothing captures; the only unchecked runtime calls before it were the cache's event queries.)
void scratch_forget_stream(hipStream_t stream);

struct Scratch {
    void* p = nullptr;
    hipStream_t s = nullptr;
    ~Scratch() {
        if (p) scratch_release(p, s);
    }
    int alloc(size_t bytes, hipStream_t stream) {
        s = stream;
        p = scratch_acquire(bytes ? bytes : 16, stream);
        if (!p) {
            set_error("scratch allocation of %zu bytes failed: %s", bytes, hipGetErrorString(hipGetLastError()));
            return MRS_ERR_HIP;
        }
        return MRS_OK;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// Owner of one plain hipMalloc allocation of T (move-only; freed by the destructor -- the owner's device must be current by then).
// For buffers that live as long as a handle; per-call temporaries use Scratch.
template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; cap_ = 0;
    }
    // Grow-only: the allocation is kept when it holds `need` elements; otherwise it is freed and one of `cap` >= need elements takes its place
    // (contents are not carried over).  MRS_OK / MRS_ERR_HIP; the buffer is empty after a failure.
    int reserve(size_t need, size_t cap)
    {
        if (need <= cap_) return MRS_OK;
        reset();
        const hipError_t e = hipMalloc(&p_, cap * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            set_error("device allocation of %zu bytes failed: %s", cap * sizeof(T), hipGetErrorString(e));
            return MRS_ERR_HIP;
        }
        cap_ = cap;
        return MRS_OK;
    }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }      // elements
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// The hipHostMalloc twin of DeviceBuffer: owner of one pinned host allocation of T (move-only; freed by the destructor).
template <class T>
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    PinnedBuffer(PinnedBuffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~PinnedBuffer() { reset(); }
    void reset()
    {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr; cap_ = 0;
    }
    // Grow-only, as DeviceBuffer::reserve: contents are not carried over, and nothing queued may still use the old block.
    int reserve(size_t need, size_t cap)
    {
        if (need <= cap_) return MRS_OK;
        reset();
        const hipError_t e = hipHostMalloc(&p_, cap * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            p_ = nullptr;
            set_error("pinned allocation of %zu bytes failed: %s", cap * sizeof(T), hipGetErrorString(e));
            return MRS_ERR_HIP;
        }
        cap_ = cap;
        return MRS_OK;
    }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }      // elements
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// Owner of one event (created by create(), destroyed by the destructor; neither copied nor moved): without timing unless create() is given
// hipEventDefault.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int create(unsigned flags = hipEventDisableTiming)
    {
        MRS_HIP_TRY(hipEventCreateWithFlags(&e, flags));
        return MRS_OK;
    }
    operator hipEvent_t() const { return e; }
};

// The development aid "events between the steps of a call" (MRS_DEV=1 with the entry point's MRS_*_TIMING switch): mark(i) records timed
// event i on the stream, ms(from) is the time from event `from` to event from + 1 (ms(from, to): to event `to`), or 0 when either is missing.  Switched off it makes no
// runtime call at all; switched on, a call that fails only costs a figure.  The events are destroyed on every way out.
class StageMarks {
public:
    static constexpr int kMax = 10;
    StageMarks(bool on, hipStream_t s) : on_(on), s_(s) {}
    explicit operator bool() const { return on_; }
    void mark(int i)
    {
        if (on_ && hipEventCreate(&ev_[i].e) == hipSuccess) (void)hipEventRecord(ev_[i], s_);
    }
    float ms(int from) const { return ms(from, from + 1); }
    float ms(int from, int to) const
    {
        float t = 0.0f;
        if (ev_[from].e && ev_[to].e) (void)hipEventElapsedTime(&t, ev_[from], ev_[to]);
        return t;
    }

private:
    bool on_;
    hipStream_t s_;
    Event ev_[kMax];
};

// The two timed events of a profiling entry point, and the time of one launch averaged over `reps` of them.
struct RepTimer {
    Event e0, e1;
    int create()
    {
        MRS_TRY(e0.create(hipEventDefault));
        return e1.create(hipEventDefault);
    }
    template <class F>
    int timed(float& ms, int reps, hipStream_t s, F&& launch)
    {
        launch();                                     // warm
        MRS_HIP_TRY(hipEventRecord(e0, s));
        for (int r = 0; r < reps; ++r) launch();
        MRS_HIP_TRY(hipEventRecord(e1, s));
        MRS_HIP_TRY(hipEventSynchronize(e1));
        MRS_HIP_TRY(hipGetLastError());
        MRS_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        ms /= (float)reps;
        return MRS_OK;
    }
};

// The non-blocking stream all work of one handle runs on, with the event pair that orders it against a caller's stream.  Stands in for its
// hipStream_t wherever one is expected.  Declare it FIRST in a handle: it is then destroyed last, after the buffers whose work it carried.
// The destructor waits for the stream, has the scratch cache forget it (scratch_forget_stream above: the rule of every stream-owning handle,
// written here once) and only then destroys it; the handle's device must be current.
struct HandleStream {
    hipStream_t s = nullptr;
    Event ev_in, ev_out;
    HandleStream() = default;
    HandleStream(const HandleStream&) = delete;
    HandleStream& operator=(const HandleStream&) = delete;
    ~HandleStream()
    {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        scratch_forget_stream(s);
        (void)hipStreamDestroy(s);
    }
    int create()
    {
        MRS_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        MRS_TRY(ev_in.create());
        return ev_out.create();
    }
    // what `user` has queued so far (a device argument being produced, an output buffer still in use) comes before the handle's later work
    int join_in(hipStream_t user)
    {
        MRS_HIP_TRY(hipEventRecord(ev_in, user));
        MRS_HIP_TRY(hipStreamWaitEvent(s, ev_in, 0));
        return MRS_OK;
    }
    // the reverse: `user`'s later work comes after what the handle's stream has queued so far
    int release_to(hipStream_t user)
    {
        MRS_HIP_TRY(hipEventRecord(ev_out, s));
        MRS_HIP_TRY(hipStreamWaitEvent(user, ev_out, 0));
        return MRS_OK;
    }
    operator hipStream_t() const { return s; }
};

// Device lookup table that reproduces the reference's sector() step function exactly
// (built on the host with the host libm, see bev.hip).
struct SectorLut {
    DeviceBuffer<float> d_thr;  // [4][stride] ascending change points of q=|y|/|x| per quadrant
    DeviceBuffer<int> d_val;    // [4][stride] sector value from thr[j] on
    int stride = 0;
    int cnt[4] = {0, 0, 0, 0};
};

}  // namespace mrs

namespace mrs {
// Scan Context building blocks (scancontext.hip), shared with the MRS_LOOPDB_SC database of loopdb.hip.  An entry is a header (sector keys,
// column norms) followed by the [R][S] descriptor; sc_entry_floats(R, S) floats from one entry to the next.
size_t sc_entry_floats(int R, int S);
int sc_search_radius(double search_ratio, int S);
int sc_pack(const float* d_sc, int n, int R, int S, float* d_entries, size_t entry_stride, float* d_ring, float* d_sector, hipStream_t s);
int sc_nearest(const float* d_q, const float* d_keys, int n, int R, int k, int* d_idx, double* d_d2, hipStream_t s);
// mode 0: dist_align_sc(F, Q) with the given search radius; 1: distance_sc(Q, F); 2: dist_direct_sc(F, Q)
int sc_align(mrs_ctx* ctx, const float* d_F, size_t f_stride, const int* d_list, int npairs, const float* d_Q, size_t q_stride, int R, int S,
             int mode, int radius, float* d_dist, int* d_shift, hipStream_t s);
}  // namespace mrs

namespace mrs {
// A second stream + fork / join events + a small pinned buffer, kept in a per-context pool: a registration of one pair (the nodes' shape)
// borrows one for the duration of mrs_gicp_batch_align.  Creating them per handle cost 0.4 ms per FastGICP object (the nodes construct one
// per registration, main_RING.py:84); concurrent callers (three rospy callback threads) each get their own slot.
constexpr int kSidePinnedInts = 64;
struct SideSlot {
    HandleStream stream;        // its ev_in is the fork event, its ev_out the join event
    PinnedBuffer<int> pinned;   // kSidePinnedInts ints
    int create()
    {
        MRS_TRY(stream.create());
        return pinned.reserve(kSidePinnedInts, kSidePinnedInts);
    }
};
int side_acquire(mrs_ctx* ctx, std::unique_ptr<SideSlot>* out);   // MRS_OK / MRS_ERR_HIP
void side_release(mrs_ctx* ctx, std::unique_ptr<SideSlot> slot);  // an empty pointer is ignored
}  // namespace mrs

// mrs_ctx_destroy deletes the context with its device current.  Members are destroyed in reverse order of declaration, and the order below is
// chosen for that: first the tables (sector_luts, then twiddles), then the point-feature cache, then the side slots.
struct mrs_ctx {
    int device = 0;
    int num_cu = 0;
    size_t lds_bytes = 0;
    std::mutex side_mu;
    std::vector<std::unique_ptr<mrs::SideSlot>> side_free;
    // mrs_pointfeat_batch keeps its Morton-ordered cloud container between calls (keyed by the number of scans per call, at most 4 sizes):
    // creating and freeing ~1.5 GB of device buffers per call cost as much as the kernels on some boxes.  One caller at a time uses a cached
    // container (try_lock); a concurrent caller works on a temporary one.  gicp.hip binds each container's deleter when it caches it.
    std::mutex pointfeat_mu;
    std::map<int, std::shared_ptr<void>> pointfeat_cache;
    std::mutex mu;
    // device-resident constant tables for the correlation / Radon kernels (lazily built)
    std::map<int, mrs::DeviceBuffer<float>> twiddles;   // keyed by FFT length
    std::map<int, mrs::SectorLut> sector_luts;          // keyed by num_sector
};
