// libhbmrag.so — host side of the C ABI declared in include/hbmrag.h.
// Owns the in-HBM shard store (dense tiles + sparse postings) of ONE GPU and
// launches the gfx950 kernels in dense.h / select.h / sparse.h / fuse.h.
// There is deliberately no CPU fallback in this file: without a HIP device
// hr_create fails and every caller sees the error.
#include "../../include/hbmrag.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"
#include "attention.h"
#include "boost.h"
#include "compact.h"
#include "decay.h"
#include "deep.h"
#include "encoder_layer.h"
#include "scan_plan.h"
#include "dense.h"
#include "encoder_ops.h"
#include "filter.h"
#include "finish.h"
#include "fuse.h"
#include "fuse_lists.h"
#include "group.h"
#include "maxsim.h"
#include "mmr.h"
#include "query.h"
#include "text.h"
#include "select.h"
#include "sparse.h"

using namespace hbmrag;

namespace {

thread_local std::string g_last_error;  // for calls without a handle

// A device allocation and its owner: freed when the buffer goes out of scope, movable, never copied.  hipFree needs the
// buffer's device to be current (every holder is destroyed under a DeviceGuard) and waits for work that still uses it.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // Exactly `bytes` (no growth slack), whatever the buffer held before; empty on failure.
    hipError_t alloc_exact(size_t bytes) {
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    hipError_t ensure(size_t bytes) { return bytes <= cap ? hipSuccess : alloc_exact(bytes + bytes / 8 + 256); }
    // Capacity for `bytes`, KEEPING the first `keep` bytes (device-to-device copy on stream s into a buffer 1.5x the
    // size asked for, so that repeated appends cost amortised O(appended bytes)).
    hipError_t grow(size_t bytes, size_t keep, hipStream_t s) {
        if (bytes <= cap) return hipSuccess;
        DevBuf nb;
        hipError_t e = nb.alloc_exact(bytes + bytes / 2 + 256);
        if (e == hipSuccess && p && keep) {
            e = hipMemcpyAsync(nb.p, p, keep, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
        }
        if (e == hipSuccess) *this = std::move(nb);
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

enum Phase { PH_PREP = 0, PH_SCAN, PH_GSEL, PH_REFINE, PH_TOPK, PH_SSCAN, PH_SGSEL, PH_SREFINE, PH_STOPK, PH_FINISH, PH_COUNT };
static_assert(PH_COUNT == HR_N_PHASES, "phase table and ABI out of step");

// A workspace's streams and events.  A base of Workspace so that they outlive its buffers: members are destroyed first,
// and the hipFree of a buffer waits for the work that still uses it, on these streams included.
struct WorkspaceQueues {
    hipStream_t stream = nullptr;  // own stream (host-form calls)
    hipStream_t side = nullptr;    // side stream + events of hr_search_hybrid_dev
    hipEvent_t ev_scan = nullptr, ev_side = nullptr;
    ~WorkspaceQueues() {
        if (stream) (void)hipStreamDestroy(stream);
        if (side) (void)hipStreamDestroy(side);
        if (ev_scan) (void)hipEventDestroy(ev_scan);
        if (ev_side) (void)hipEventDestroy(ev_side);
    }
};

// `delete w`, with the workspace's device current, is the whole release.
struct Workspace : WorkspaceQueues {
    std::mutex mu;                 // held while one call enqueues: calls sharing a workspace must not interleave their kernels
    int users = 0;                 // calls that hold or wait for this workspace (guarded by hr_index::pool_mu): never pruned while > 0
    struct Workspace* sparse_ws = nullptr;  // private buffers of the sparse chain when it runs concurrently
    DevBuf qfrag, qn2, gmax, bmax, cand, acut, cscore, crow, flags, qscale, qeps, qfloor, pq_n, pq_idx, pq_w;
    DevBuf qcoef, dqeps;   // L2 shards: per query slot, the row term's coefficient 1 / |q| and the per-query error term
    DevBuf rbounds, rhi, rlo;   // range search: per query the two canonical bounds, per query slot the scan's ceiling and floor
    DevBuf d_radius, d_rfilter;                   // range search, host form: the callers' bounds
    DevBuf d_q, d_ids, d_scores, d_mask;          // host-form staging
    DevBuf d_qptr, d_qidx, d_qval;                // sparse query staging
    DevBuf f_ids, f_sc, f_out_ids, f_out_scores, f_out_meth, f_n;  // hr_fuse_rrf / hr_fuse_scores staging
    ~Workspace() { delete sparse_ws; }
};

struct EventSpan {
    int phase;
    hipEvent_t a, b;
};

}  // namespace

struct hr_index {
    int device = 0;
    int64_t dim = 0, sparse_dim = 0;
    int dtype = HR_F16, metric = HR_METRIC_COSINE;
    int KT = 0;  // 1 KiB tiles per row block along k
    int group_rows_override = 0;  // hr_debug_option(HR_DEBUG_GROUP_ROWS) at creation pins the candidate-group size (default: by shard size)
    int64_t row_offset = 0;

    // dense shard
    DevBuf tiles, scale, norm2, max_norm;
    int64_t cap_rows = 0, n_rows = 0, n_normed = 0;
    float max_row_norm = 0.f;
    DevBuf stage;  // ingest staging
    DevBuf bad_row;  // one u64, all ones between calls: tile_rows_kernel lowers it to a batch row that is not finite
    hipStream_t ingest_stream = nullptr;

    // sparse shard: the CSR lives on the device; the host only stages the rows appended since the last hr_finalize
    std::vector<int64_t> pend_indptr{0};  // relative to the first pending entry
    std::vector<int32_t> pend_idx;
    std::vector<float> pend_val;
    std::vector<int64_t> h_range_base{0};  // first posting of every range's block (+ total), host copy
    std::vector<unsigned> h_range_dense;   // dense runs per range (sparse.h)
    // n_sparse rows added; n_csr / nnz_csr of them in the device CSR; n_sparse_built of them in the postings
    int64_t n_sparse = 0, n_csr = 0, nnz_csr = 0, n_sparse_built = 0;
    float max_sparse_abs = 0.f;  // max |doc weight|: bounds the scan's fixed-point range
    bool sparse_signed = false;  // some stored weight is negative: the scan's products can cancel (sparse.h)
    DevBuf s_indptr, s_idx, s_val, rt_off, range_base, post;  // post: packed (fp16 weight | u16 accumulator slot)
    DevBuf idle_post;  // 64 x 4 idle postings: what scan lanes with nothing to fetch read (sparse.h)
    int64_t n_ranges = 0;
    int64_t n_dense_runs = 0;      // (term, range) runs in the dense form (sparse.h): the scan's variant is chosen by it

    bool finalized = false;
    int profiling = 0;
    int cu_count = 256;
    int scan_cus = 0;              // compute units the scans' stream may use (hr_set_scan_cus); 0 = all
    int fault_inject = 0;          // hr_debug_inject_fault: fail the next build_sparse after its CSR upload (tests)
    float compact_ms[3] = {};      // the last hr_compact under profiling: tile gather (events), whole call, posting rebuild (wall)
    bool slot_prepped[HR_MAX_SLOTS] = {};  // hr_hybrid_prep_dev has prepared the slot's queries for the next scan

    mutable std::shared_mutex rw;  // searches shared, add/finalize exclusive
    std::mutex pool_mu;
    std::vector<Workspace*> free_ws;
    std::map<void*, Workspace*> stream_ws;
    Workspace* slot_ws[HR_MAX_SLOTS][2] = {};  // [slot][dense|sparse] of the two-phase forms
    std::mutex prof_mu;
    std::vector<EventSpan> spans;
    std::vector<hipEvent_t> event_pool;
    mutable std::mutex err_mu;
    mutable std::string err;

    // Deleted with the device current and idle (hr_destroy; hr_create's failure path).  The workspaces go before the
    // handle's own stream; the buffers above free themselves after this body.
    ~hr_index() {
        for (Workspace* w : free_ws) delete w;
        for (auto& kv : stream_ws) delete kv.second;
        for (auto& pair : slot_ws)
            for (Workspace* w : pair) delete w;
        for (auto& sp : spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
        for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
        if (ingest_stream) (void)hipStreamDestroy(ingest_stream);
    }
};

namespace {

int fail(const hr_index* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) {
        std::lock_guard<std::mutex> g(h->err_mu);
        h->err = buf;
    }
    g_last_error = buf;
    return code;
}

#define HIP_TRY(h, expr)                                                                   \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) return fail(h, HR_EHIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

#define HR_TRY(expr)               \
    do {                           \
        int rc__ = (expr);         \
        if (rc__ != HR_OK) return rc__; \
    } while (0)

inline size_t elem_size(int dtype) { return dtype == HR_F16 ? 2 : 4; }
inline int elems_per_chunk(int dtype) { return dtype == HR_F16 ? 8 : 4; }
inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline size_t tile_bytes_for_rows(const hr_index* h, int64_t rows) {
    return (size_t)(rows / kRowsPerBlock) * h->KT * 1024;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

Workspace* take_ws(hr_index* h) {
    std::lock_guard<std::mutex> g(h->pool_mu);
    if (!h->free_ws.empty()) {
        Workspace* w = h->free_ws.back();
        h->free_ws.pop_back();
        return w;
    }
    Workspace* w = new (std::nothrow) Workspace();
    if (!w) return nullptr;
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
        delete w;
        return nullptr;
    }
    return w;
}
void give_ws(hr_index* h, Workspace* w) {
    std::lock_guard<std::mutex> g(h->pool_mu);
    h->free_ws.push_back(w);
}
// The workspace of a caller-owned stream, returned LOCKED: `*_dev` calls that share a stream share its workspace
// (query fragments, group maxima, candidates), so one call's enqueue must not interleave with another's — their
// kernels then run in stream order.  The handle-wide pool lock is held only for the map lookup: a call that waits for a
// busy workspace (its owner may be inside hipMalloc) does not stall the other streams of the handle.  The map is
// pruned when it grows — a long-lived handle used from many short-lived streams would otherwise keep every stream's
// buffers for ever — and the pruned workspaces are freed after the pool lock is dropped (hipFree synchronises the device).
constexpr size_t kMaxStreamWorkspaces = 32;
struct StreamWs {
    hr_index* h = nullptr;
    Workspace* w = nullptr;
    std::unique_lock<std::mutex> held;
    StreamWs() = default;
    StreamWs(const StreamWs&) = delete;
    StreamWs& operator=(const StreamWs&) = delete;
    ~StreamWs() {
        if (!w) return;
        if (held.owns_lock()) held.unlock();
        std::lock_guard<std::mutex> g(h->pool_mu);
        --w->users;
    }
};
Workspace* ws_for_stream(hr_index* h, void* stream, StreamWs& out) {
    std::vector<Workspace*> pruned;
    Workspace* w = nullptr;
    {
        std::lock_guard<std::mutex> g(h->pool_mu);
        auto it = h->stream_ws.find(stream);
        if (it != h->stream_ws.end()) {
            w = it->second;
        } else {
            if (h->stream_ws.size() >= kMaxStreamWorkspaces) {
                for (auto jt = h->stream_ws.begin(); jt != h->stream_ws.end();) {
                    if (jt->second->users == 0) {  // nobody holds or waits for it, and nobody can get it while pool_mu is held
                        pruned.push_back(jt->second);
                        jt = h->stream_ws.erase(jt);
                    } else {
                        ++jt;
                    }
                }
            }
            w = new (std::nothrow) Workspace();
            if (w) h->stream_ws[stream] = w;
        }
        if (w) ++w->users;
    }
    for (Workspace* old : pruned) delete old;  // hipFree waits for the work that still uses the buffers
    if (!w) return nullptr;
    out.h = h;
    out.w = w;
    out.held = std::unique_lock<std::mutex>(w->mu);
    return w;
}

// ---- profiling spans -------------------------------------------------------
struct Span {
    hr_index* h;
    hipStream_t s;
    int phase;
    hipEvent_t a = nullptr, b = nullptr;
    Span(hr_index* h_, hipStream_t s_, int phase_) : h(h_), s(s_), phase(phase_) {
        const bool on = h->profiling >= 2 || (h->profiling == 1 && (phase == PH_SCAN || phase == PH_SSCAN));
        if (!on) return;
        std::lock_guard<std::mutex> g(h->prof_mu);
        auto get = [&]() -> hipEvent_t {
            hipEvent_t e = nullptr;
            if (!h->event_pool.empty()) {
                e = h->event_pool.back();
                h->event_pool.pop_back();
            } else if (hipEventCreate(&e) != hipSuccess) {
                e = nullptr;
            }
            return e;
        };
        a = get();
        b = get();
        if (a && b) (void)hipEventRecord(a, s);
    }
    ~Span() {
        if (!a || !b) return;
        (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> g(h->prof_mu);
        h->spans.push_back({phase, a, b});
    }
};

// Compute units the scans may occupy: their persistent grids are sized to it (hr_set_scan_cus for a masked stream).
inline int scan_cus(const hr_index* h) { return h->scan_cus > 0 ? std::min(h->scan_cus, h->cu_count) : h->cu_count; }

int group_rows_for(const hr_index* h, int64_t n) { return scan_group_rows(n, h->group_rows_override); }

// ---- dense launch helpers ----------------------------------------------------
// One launcher per scan kernel (grid and LDS sizing), then launch_scan: the one place that maps a ScanPlan
// (scan_plan.h) onto the template instantiation.  n_super counts SUPER-groups (64 rows) = the scans' loop bound.
struct ScanArgs {
    const hr_index* h;
    hipStream_t s;
    const chunk_t* qfrag;
    const uint8_t* mask;
    float* gmax;
    int nq;
    int64_t n_super;
    const float* qcoef;  // L2 passes: the coefficients of this pass's query slots
    const float* qhi;    // range passes: the ceilings of this pass's query slots
};

template <typename STORE, int G, int NRB, bool L2, bool RANGE>
hipError_t launch_scan_lds(const ScanArgs& a) {
    constexpr int RS = 2, PF = 4;
    auto kern = dense_scan_kernel<STORE, G, RS, PF, NRB, L2, RANGE>;
    const hr_index* h = a.h;
    const size_t lds = (size_t)G * h->KT * 1024;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // One 1024-thread block per CU when the query tile is large, several
    // 256-thread blocks per CU otherwise; waves take groups in a grid-stride loop.
    int threads, per_cu;
    if (lds > 40 * 1024) {
        threads = 512;
        per_cu = 1;
    } else {
        threads = 256;
        per_cu = (int)std::min<size_t>(8, (150 * 1024) / std::max<size_t>(lds, 1));
    }
    const int64_t waves_per_block = threads / 64;
    int64_t blocks = std::min<int64_t>((a.n_super + waves_per_block - 1) / waves_per_block,
                                       (int64_t)scan_cus(h) * per_cu);
    blocks = std::max<int64_t>(blocks, 1);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(threads), lds, a.s, h->tiles.as<chunk_t>(), a.qfrag,
                       h->scale.as<float>(), a.mask, a.gmax, a.nq, h->KT, h->n_rows, a.n_super, a.qcoef, a.qhi);
    return hipGetLastError();
}

// Large-batch pass (dense_scan_bigq_kernel): GQ query groups streamed through LDS in k-chunks.
template <typename STORE, int GQ, int NRB, bool L2, bool RANGE>
hipError_t launch_scan_bigq(const ScanArgs& a) {
    auto kern = dense_scan_bigq_kernel<STORE, GQ, NRB, L2, RANGE>;
    const hr_index* h = a.h;
    const size_t lds = (size_t)2 * GQ * 2 * 1024;  // 2 buffers x GQ groups x BKT(2) fragments of 1 KiB
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int64_t blocks = std::min<int64_t>((a.n_super + 7) / 8, (int64_t)scan_cus(h));
    blocks = std::max<int64_t>(blocks, 1);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), lds, a.s, h->tiles.as<chunk_t>(), a.qfrag,
                       h->scale.as<float>(), a.mask, a.gmax, a.nq, h->KT, h->n_rows, a.n_super, a.qcoef, a.qhi);
    return hipGetLastError();
}

// 256-query pass with the queries in registers and the corpus streamed through LDS (dense_scan_qreg_kernel):
// fp16 shards whose rows are 24 tiles long (D = 768 after padding; 2 x 24 x 4 fragment registers per wave);
// 8 waves x 32 queries, one block per CU.
template <int KT, int NRB, int GW, int NW>
hipError_t launch_scan_qreg(const ScanArgs& a) {
    const hr_index* h = a.h;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(a.n_super, (int64_t)scan_cus(h) * (8 / NW)));
    hipLaunchKernelGGL((dense_scan_qreg_kernel<KT, NRB, GW, NW>), dim3((unsigned)blocks), dim3(64 * NW), 0, a.s,
                       h->tiles.as<chunk_t>(), a.qfrag, h->scale.as<float>(), a.mask, a.gmax, a.nq, h->n_rows, a.n_super);
    return hipGetLastError();
}
// 256 queries per pass, second form: 4 waves x 64 queries in registers (one wave per SIMD, the whole 512-entry register
// file), the corpus through the same LDS-DMA ring with half the LDS reads (dense_scan_q64_kernel).
template <int NRB>
hipError_t launch_scan_q64(const ScanArgs& a) {
    const hr_index* h = a.h;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(a.n_super, (int64_t)scan_cus(h)));
    const size_t lds = (size_t)kQregStages * 24 * 1024 + 2 * kSuperRows * sizeof(float);
    static bool ready = false;  // per group size
    if (!ready) {
        hipError_t e = hipFuncSetAttribute((const void*)dense_scan_q64_kernel<24, NRB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        ready = true;
    }
    hipLaunchKernelGGL((dense_scan_q64_kernel<24, NRB>), dim3((unsigned)blocks), dim3(256), lds, a.s, h->tiles.as<chunk_t>(),
                       a.qfrag, h->scale.as<float>(), a.mask, a.gmax, a.nq, h->n_rows, a.n_super);
    return hipGetLastError();
}
// 256-query pass as a tiled contraction (dense_scan_gemm_kernel): fp16 shards of any row length from 8 tiles up;
// serves the shapes the register-resident form cannot (D = 1024: BASELINE config 5).
template <int NRB>
hipError_t launch_scan_gemm(const ScanArgs& a) {
    const hr_index* h = a.h;
    const int64_t n_tiles = (a.n_super * kRowBlocksPerSuper + kGemmRowBlocks - 1) / kGemmRowBlocks;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_tiles, scan_cus(h)));
    hipLaunchKernelGGL((dense_scan_gemm_kernel<16, NRB>), dim3(blocks), dim3(512), 0, a.s, h->tiles.as<chunk_t>(), a.qfrag,
                       h->scale.as<float>(), a.mask, a.gmax, a.nq, h->KT, h->n_rows, a.n_super);
    return hipGetLastError();
}

// f(std::integral_constant<int, V>) for the V among Vs that equals v
template <int... Vs, typename F>
hipError_t with_constant(int v, F f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs ? (e = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return e;
}

// f(STORE{}) for the element type of a dense store of `dtype`: _Float16 or float
template <typename F>
auto with_store(int dtype, F f) {
    if (dtype == HR_F16) return f(_Float16{});
    return f(float{});
}

// The two generic kernels: STORE x L2 x RANGE here, NRB x G below.
template <typename STORE, bool L2, bool RANGE>
hipError_t launch_scan_generic(const ScanPlan& p, const ScanArgs& a) {
    return with_constant<1, 4>(p.NRB, [&](auto nrb) {
        if (p.kind == SCAN_BIGQ) return launch_scan_bigq<STORE, 8, decltype(nrb)::value, L2, RANGE>(a);
        return with_constant<1, 2, 3, 4>(
            p.G, [&](auto g) { return launch_scan_lds<STORE, decltype(g)::value, decltype(nrb)::value, L2, RANGE>(a); });
    });
}

hipError_t launch_scan(const ScanPlan& p, const ScanArgs& a) {
    switch (p.kind) {
        case SCAN_QREG: return with_constant<1, 4>(p.NRB, [&](auto nrb) { return launch_scan_qreg<24, decltype(nrb)::value, 2, 8>(a); });
        case SCAN_Q64: return with_constant<1, 4>(p.NRB, [&](auto nrb) { return launch_scan_q64<decltype(nrb)::value>(a); });
        case SCAN_GEMM: return with_constant<1, 4>(p.NRB, [&](auto nrb) { return launch_scan_gemm<decltype(nrb)::value>(a); });
        case SCAN_LDS:
        case SCAN_BIGQ:
            return with_store(a.h->dtype, [&](auto store) {
                using STORE = decltype(store);
                if (p.range) return p.l2 ? launch_scan_generic<STORE, true, true>(p, a) : launch_scan_generic<STORE, false, true>(p, a);
                return p.l2 ? launch_scan_generic<STORE, true, false>(p, a) : launch_scan_generic<STORE, false, false>(p, a);
            });
        default: return hipErrorInvalidValue;
    }
}

// A range search's bounds as the device sees them: [B] doubles each, null = that side unbounded for every query.
struct DenseRange {
    const double* d_radius;
    const double* d_range_filter;
};

int g_dense_kernels = 0;  // HR_DEBUG_DENSE_KERNELS: bit mask that takes scan kernels out of the selection (scan_plan.h)
int g_sparse_rpb = 0;     // HR_DEBUG_SPARSE_RPB: doc ranges per sparse-scan block (0 = by shard size)
int g_no_trim = 0;        // HR_DEBUG_NO_TRIM: 1 = refine all C candidate groups (A/B of the data-dependent candidate set)
int g_group_rows = 0;     // HR_DEBUG_GROUP_ROWS: candidate-group size of handles created from now on (0 = by shard size)
int g_no_range_clamp = 0; // HR_DEBUG_NO_RANGE_CLAMP: 1 = the range scans get +inf ceilings (what the clamp proves, A/B)

// Two-level candidate selection: per-bucket maxima, then one block per query — for one modality or for both
// modalities of a hybrid search in one pair of launches (select.h: GroupSelPair).
inline int64_t bucket_count(int64_t n_groups) { return (n_groups + kBucketGroups - 1) / kBucketGroups; }
int launch_group_select_pair(hr_index* h, hipStream_t s, int B, const GroupSelPair& p) {
    int64_t blocks = 0;
    for (int m = 0; m < p.n; ++m)
        if (p.m[m].two_level) blocks = std::max(blocks, (p.m[m].n_buckets + 4 * kBucketsPerWave - 1) / (4 * kBucketsPerWave));
    if (blocks > 0) {
        hipLaunchKernelGGL(bucket_max_kernel, dim3((unsigned)blocks, B, p.n), dim3(256), 0, s, p);
        HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(select_groups_kernel, dim3(B, p.n), dim3(1024), 0, s, p);
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}
int launch_topk_pair(hr_index* h, hipStream_t s, int B, const TopkPair& p) {
    hipLaunchKernelGGL(select_topk_kernel, dim3(B, p.n), dim3(1024), 0, s, p);
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}

// Escalation ladder of the host forms when a list is not provably exact:
// default -> 4x (bounded by the selection kernel's bucket table) -> every group.
constexpr int kMaxSelectGroups = 448;
int next_candidate_count(int C, int64_t n_groups) {
    const int64_t all = round_up(n_groups, 16);
    if (C < kMaxSelectGroups && (int64_t)C * 4 < all) return std::min(C * 4, kMaxSelectGroups);
    return (int)all;
}

int candidate_groups_for_k(int k) {
    int c = k + std::max(16, k / 2);
    return (int)round_up(c, 16);
}

// L2 (norm_mode 2).  The scan's value of row x for query q is a = fl(acc - fl(fl(R) * fl(c))), R = |x|^2 / 2, c = 1 / |q|,
// against the exact t = x.q / |q| - R c = (|q|^2 - D) / (2 |q|).  |acc - x.q / |q|| <= unit * |x| as for IP; fl(R), fl(c) and
// their product carry 2^-24 each (3 * 2^-24 * R c, second-order terms in the margin), the subtraction 2^-24 (|acc| + R c)
// with |acc| <= |x| (1 + unit).  With M = the largest row norm:
//   |a - t| <= (unit + 2^-24 * 1.01) M  +  2^-22 * 1.01 * (M^2 / 2) / |q|
// The first term is eps_abs, the second is per query: dense_l2_rt_eps() / |q|, written by prep_queries_kernel into
// TopkArgs::eps_abs_q (for a zero query c = 1, acc = 0, and the same expression bounds the error of -fl(R)).
// select_topk_block carries the K-th returned distance into this domain (select.h, norm_mode 2).
float dense_l2_rt_eps(const hr_index* h) {
    const double M = (double)h->max_row_norm * 1.0001;
    return (float)std::min(std::ldexp(1.0, -22) * 1.01 * 0.5 * M * M, 3.0e38);
}
void dense_eps(const hr_index* h, float* eps_abs, int* norm_mode) {
    const double Dp = (double)h->KT * 4 * elems_per_chunk(h->dtype);
    double unit = 2.0 * Dp * std::ldexp(1.0, -24) + 1e-6;        // fp32 accumulation + scale rounding
    unit += (h->dtype == HR_F16) ? std::ldexp(1.0, -11) * 1.01  // query rounded to fp16
                                 : std::ldexp(1.0, -22);        // query normalised in fp32
    if (h->metric == HR_METRIC_COSINE) {
        *eps_abs = (float)unit;
        *norm_mode = 0;
    } else if (h->metric == HR_METRIC_L2) {
        *eps_abs = (float)((unit + std::ldexp(1.0, -24) * 1.01) * (double)h->max_row_norm * 1.0001);
        *norm_mode = 2;
    } else {
        *eps_abs = (float)(unit * (double)h->max_row_norm * 1.0001);
        *norm_mode = 1;
    }
}

// ---- the finish of one modality ---------------------------------------------------------------------------------
// "Finishing" = select the candidate groups from the scan's group maxima, refine them exactly, take the top k and set the
// exactness flag.  A FinishSide says what that takes for one modality of one call.  dense_side / sparse_side fill it
// once; the selection arguments, the fused kernel's FinishMod, the refine launch and the chain's TopkArgs all come from it.
struct OutLists {  // where a call's lists go: [B][k] ids and scores, [B] exactness flags (may be null)
    int64_t* ids;
    float* scores;
    int32_t* flags;
};
struct FinishSide {
    Workspace* ws;
    bool sparse;
    int GR;            // rows per candidate group
    int64_t n_groups;  // group SLOTS the scan wrote per query (dense: a whole number of super-groups, the tail slots hold -inf)
    int C;             // candidate groups per query
    const uint8_t* mask;
    TopkArgs topk;
    const float* d_q;  // dense refine
    const double* range_bounds;  // dense refine of a range search: [B][2] radius, range_filter
    const int64_t* q_ptr;  // sparse refine: the query CSR and the fixed stride of the scan's query layout
    const int32_t* q_idx;
    const float* q_val;
    int stride;
    int ph_select, ph_refine, ph_topk;  // profiling phases of the side on its own
};

// What both modalities fill alike.  Ensures the workspace buffers the finish reads and writes — here, before the call's
// first launch and before TopkArgs takes their addresses.  dense_side / sparse_side rely on the enqueue functions
// having sized what the prep and scan phases write (qn2, dqeps; qeps, qfloor): a finish follows a scan on the same
// workspace.
int side_common(hr_index* h, Workspace* ws, int B, int k, int C, int GR, int64_t n_groups, const uint8_t* d_mask,
                const OutLists& out, FinishSide* f) {
    HIP_TRY(h, ws->gmax.ensure((size_t)B * n_groups * sizeof(float)));
    HIP_TRY(h, ws->bmax.ensure((size_t)B * bucket_count(n_groups) * sizeof(float)));
    HIP_TRY(h, ws->cand.ensure((size_t)B * C * sizeof(int32_t)));
    HIP_TRY(h, ws->acut.ensure((size_t)B * sizeof(float)));
    HIP_TRY(h, ws->cscore.ensure((size_t)B * C * GR * sizeof(float)));
    HIP_TRY(h, ws->crow.ensure((size_t)B * C * GR * sizeof(int32_t)));
    *f = FinishSide{};
    f->ws = ws;
    f->GR = GR;
    f->n_groups = n_groups;
    f->C = C;
    f->mask = d_mask;
    TopkArgs& t = f->topk;
    t.cscore = ws->cscore.as<float>();
    t.crow = ws->crow.as<int32_t>();
    t.n = C * GR;
    t.K = k;
    t.row_offset = h->row_offset;
    t.a_cut = ws->acut.as<float>();
    t.out_ids = out.ids;
    t.out_scores = out.scores;
    t.flags = out.flags;
    return HR_OK;
}
inline int64_t dense_super_groups(const hr_index* h) { return (h->n_rows + kSuperRows - 1) / kSuperRows; }
// ranged: the finish of a range search: the refine tests ws->rbounds and the proof takes the per-query floors ws->rlo
// (both written by the range search's query prep).
int dense_side(hr_index* h, Workspace* ws, const float* d_q, int B, int k, int C, const uint8_t* d_mask, const OutLists& out,
               FinishSide* f, bool ranged = false) {
    const int GR = group_rows_for(h, h->n_rows);
    HR_TRY(side_common(h, ws, B, k, C, GR, dense_super_groups(h) * (kSuperRows / GR), d_mask, out, f));
    f->d_q = d_q;
    f->ph_select = PH_GSEL, f->ph_refine = PH_REFINE, f->ph_topk = PH_TOPK;
    TopkArgs& t = f->topk;
    dense_eps(h, &t.eps_abs, &t.norm_mode);
    t.cut_floor = -INFINITY;
    t.eps_abs_q = t.norm_mode == 2 ? ws->dqeps.as<float>() : nullptr;   // L2: the row term's share, 1 / |q| times a constant
    t.qn2 = ws->qn2.as<double>();
    if (ranged) {
        f->range_bounds = ws->rbounds.as<double>();
        t.cut_floor_q = ws->rlo.as<float>();   // a_cut <= lo_a: no row outside the candidates is in range
    }
    return HR_OK;
}
int sparse_side(hr_index* h, Workspace* ws, const int64_t* d_qptr, const int32_t* d_qidx, const float* d_qval, int B,
                int max_q_nnz, int k, int C, const uint8_t* d_mask, const OutLists& out, FinishSide* f) {
    const int GR = group_rows_for(h, h->n_sparse);
    HR_TRY(side_common(h, ws, B, k, C, GR, (h->n_sparse + GR - 1) / GR, d_mask, out, f));
    f->sparse = true;
    f->q_ptr = d_qptr;
    f->q_idx = d_qidx;
    f->q_val = d_qval;
    f->stride = (int)round_up(std::max(max_q_nnz, 1), 64);  // fixed-stride query layout for the scan
    f->ph_select = PH_SGSEL, f->ph_refine = PH_SREFINE, f->ph_topk = PH_STOPK;
    // scan error = fixed-point rounding ((nnz+1)/scale per query, from the prep kernel) + fp32 rounding of w*scale, of
    // the product and of the int->float conversion (relative, 2^-22 with margin).
    TopkArgs& t = f->topk;
    t.cut_floor_q = ws->qfloor.as<float>();   // 0, or -q_eps when products can be negative (sparse_query_prep_kernel)
    t.eps_abs_q = ws->qeps.as<float>();
    t.eps_rel = (float)(std::ldexp(1.0, -11) * 1.01 + std::ldexp(1.0, -22));  // fp16 posting weights
    return HR_OK;
}

GroupSelArgs sel_args(const FinishSide& f) {
    GroupSelArgs a{};
    a.gmax = f.ws->gmax.as<float>();
    a.bmax = f.ws->bmax.as<float>();
    a.n_groups = f.n_groups;
    a.n_buckets = bucket_count(f.n_groups);
    a.C = f.C;
    a.two_level = f.n_groups > f.C && a.n_buckets > f.C;
    a.cand = f.ws->cand.as<int32_t>();
    a.a_cut = f.ws->acut.as<float>();
    // the data-dependent candidate set: trim against the K-th largest group maximum with the error bound of the list's proof
    a.K_trim = g_no_trim ? 0 : f.topk.K;
    a.eps_abs = f.topk.eps_abs;
    a.eps_rel = f.topk.eps_rel;
    a.eps_abs_q = f.topk.eps_abs_q;
    return a;
}
FinishMod finish_mod(const hr_index* h, const FinishSide& f) {
    FinishMod m{};
    m.kind = f.sparse;
    m.group_rows = f.GR;
    m.sel = sel_args(f);
    m.topk = f.topk;
    m.rowmask = f.mask;
    if (f.sparse) {
        m.indptr = h->s_indptr.as<int64_t>();
        m.idx = h->s_idx.as<int32_t>();
        m.val = h->s_val.as<float>();
        m.q_indptr = f.q_ptr;
        m.q_idx = f.q_idx;
        m.q_val = f.q_val;
        m.q_cap = f.stride;
        m.n_rows = h->n_sparse;
    } else {
        m.tiles = h->tiles.as<chunk_t>();
        m.KT = h->KT;
        m.dim = (int)h->dim;
        m.metric = h->metric;
        m.dtype = h->dtype;
        m.q = f.d_q;
        m.qn2 = f.ws->qn2.as<double>();
        m.norm2 = h->norm2.as<double>();
        m.range_bounds = f.range_bounds;
        m.n_rows = h->n_rows;
    }
    return m;
}
// Where a refine reads its candidate groups and leaves its slots: the workspace's buffers (the finishing chain), or
// buffers the call owns (deep search).
struct RefineBufs {
    const double* qn2;     // dense: [B] squared query norms
    const int32_t* cand;   // [B][C]
    float* cscore;         // [B][C * GR]
    int32_t* crow;
};
int launch_refine(hr_index* h, hipStream_t s, int B, const FinishSide& f, const RefineBufs& b) {
    if (!f.sparse) {
        const bool f16 = h->dtype == HR_F16, l2 = h->metric == HR_METRIC_L2;
        auto kern = f16 ? (l2 ? refine_dense_kernel<_Float16, true> : refine_dense_kernel<_Float16, false>)
                        : (l2 ? refine_dense_kernel<float, true> : refine_dense_kernel<float, false>);
        hipLaunchKernelGGL(kern, dim3((f.C * f.GR + 63) / 64, B), dim3(64), 0, s, h->tiles.as<chunk_t>(), h->KT, (int)h->dim,
                           f.d_q, b.qn2, h->norm2.as<double>(), f.mask, b.cand, f.C, f.GR,
                           h->n_rows, h->metric, b.cscore, b.crow, f.range_bounds);
    } else {
        // 64 docs per wave: shorter chains finish this kernel sooner (0.60 -> 0.55 ms at 10M docs, 0.168 -> 0.136 ms at 1.25M
        // with 16) but the step does not gain — the kernel runs beside the scans, and what it takes from the HBM sooner they
        // get later (round 2 A/B).
        const int dpw = 64;
        const bool hashed = f.stride <= kHashMaxTerms;   // the query's terms as a hash table behind the filter (sparse.h)
        const size_t lds = (size_t)kFilterBits / 8 + (hashed ? (size_t)sparse_hash_slots(f.stride) * 8 : (size_t)f.stride * 8);
        hipLaunchKernelGGL(hashed ? refine_sparse_kernel<true> : refine_sparse_kernel<false>,
                           dim3((f.C * f.GR + 4 * dpw - 1) / (4 * dpw), B), dim3(256), lds, s, h->s_indptr.as<int64_t>(),
                           h->s_idx.as<int32_t>(), h->s_val.as<float>(), f.q_ptr, f.q_idx, f.q_val, f.mask,
                           b.cand, f.C, f.GR, h->n_sparse, f.stride, dpw, b.cscore, b.crow);
    }
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}
int launch_refine(hr_index* h, hipStream_t s, int B, const FinishSide& f) {
    Workspace* ws = f.ws;
    return launch_refine(h, s, B, f, {ws->qn2.as<double>(), ws->cand.as<int32_t>(), ws->cscore.as<float>(), ws->crow.as<int32_t>()});
}

enum { PHASE_SCAN = 1, PHASE_FINISH = 2, PHASE_PREP = 4, PHASE_ALL = 7 };

// ---- the finishing chain as one launch (finish.h) --------------------------------------------------------------
// One block per (query, modality): worth it when the batch fills a good part of the chip that way and the candidate
// set fits LDS; otherwise the multi-launch chain, whose refine kernels spread ONE query over many compute units
// (single-query latency path, escalated searches with hundreds of candidate groups).
int g_finish_mode = 0;  // hr_debug_option(HR_DEBUG_FINISH_MODE): 0 = by batch size, 1 = always the chain, 2 = fused whenever it fits
int g_maxsim_scan_blocks = 0;  // hr_debug_option(HR_DEBUG_MAXSIM_SCAN_BLOCKS): blocks per query of hr_maxsim_scan_dev (0 = by size)
bool finish_fused_ok(int B, int n_mod, const FinishSide& f) {
    if (g_finish_mode == 1) return false;
    return ((int64_t)B * n_mod >= 64 || g_finish_mode == 2) && f.C <= kFinishMaxCand && (int64_t)f.C * f.GR <= kFinishMaxSlots &&
           bucket_count(f.n_groups) <= kFinishMaxBuckets;
}
int launch_finish(hr_index* h, hipStream_t s, int B, FinishPair& p) {
    p.key_slots = 0;
    for (int i = 0; i < p.n; ++i) p.key_slots = std::max(p.key_slots, p.m[i].sel.C * p.m[i].group_rows);
    const size_t lds = finish_lds_bytes(p);
    static bool attr_set = false;  // benign race: the attribute is idempotent
    if (!attr_set) {
        HIP_TRY(h, hipFuncSetAttribute((const void*)finish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_set = true;
    }
    hipLaunchKernelGGL(finish_kernel, dim3(B, p.n), dim3(kFinishThreads), lds, s, p);
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}

// Finish one modality, or both modalities of a hybrid search (dense first), on stream s: the fused kernel when every side
// fits it, else the chain with the selection steps of all sides in one launch each — with two sides 5 dependent launches
// (+ bucket_max) instead of 8, their spans booked on the first side's phases (group_select, topk).
int finish_enqueue(hr_index* h, hipStream_t s, int B, const FinishSide* f, int n) {
    bool fused = true;
    for (int i = 0; i < n; ++i) fused = fused && finish_fused_ok(B, n, f[i]);
    if (fused) {
        Span sp(h, s, PH_FINISH);
        FinishPair p{};
        p.n = n;
        for (int i = 0; i < n; ++i) p.m[i] = finish_mod(h, f[i]);
        return launch_finish(h, s, B, p);
    }
    {
        Span sp(h, s, f[0].ph_select);
        GroupSelPair p{};
        p.n = n;
        for (int i = 0; i < n; ++i) p.m[i] = sel_args(f[i]);
        HR_TRY(launch_group_select_pair(h, s, B, p));
    }
    for (int i = 0; i < n; ++i) {
        Span sp(h, s, f[i].ph_refine);
        HR_TRY(launch_refine(h, s, B, f[i]));
    }
    {
        Span sp(h, s, f[0].ph_topk);
        TopkPair p{};
        p.n = n;
        for (int i = 0; i < n; ++i) p.m[i] = f[i].topk;
        HR_TRY(launch_topk_pair(h, s, B, p));
    }
    return HR_OK;
}

// Enqueue a dense search on stream s (all pointers are device pointers): PHASE_PREP = query prep, PHASE_SCAN = the
// shard scan (leaves the group maxima in ws), PHASE_FINISH = candidate select + refine + top-k from those maxima.
int dense_search_enqueue(hr_index* h, Workspace* ws, hipStream_t s, const float* d_q, int B, int k,
                         const uint8_t* d_mask, const OutLists& out, int C, hipEvent_t scan_done = nullptr,
                         int phases = PHASE_ALL, const DenseRange* rng = nullptr) {
    // one plan per pass (scan_plan.h); the full-batch plan gives the queries per pass
    const bool ranged = rng != nullptr;
    auto plan_for = [&](int nq) {
        return scan_plan(h->KT, h->dtype, h->metric, h->n_rows, h->group_rows_override, g_dense_kernels, B, nq, ranged);
    };
    const ScanPlan first = plan_for(B);
    if (first.kind == SCAN_NONE)
        return fail(h, HR_ELIMIT, "dim=%lld: the query tile does not fit LDS and the k-chunked pass is switched off",
                    (long long)h->dim);
    const bool l2 = first.l2;
    const int chunk_q = first.chunk_q, Gmax = chunk_q / 16;
    const int n_chunks = (B + chunk_q - 1) / chunk_q;
    const size_t chunk_frag = (size_t)Gmax * h->KT * kTileChunks;   // 16-byte chunks of one pass's query fragments
    HIP_TRY(h, ws->qfrag.ensure((size_t)n_chunks * chunk_frag * sizeof(chunk_t)));
    HIP_TRY(h, ws->qn2.ensure((size_t)B * sizeof(double)));
    if (l2) {  // one entry per query SLOT (the scans read the padding slots of a pass too)
        HIP_TRY(h, ws->qcoef.ensure((size_t)n_chunks * chunk_q * sizeof(float)));
        HIP_TRY(h, ws->dqeps.ensure((size_t)n_chunks * chunk_q * sizeof(float)));
    }
    float* const d_coef = l2 ? ws->qcoef.as<float>() : nullptr;
    float* const d_qeps = l2 ? ws->dqeps.as<float>() : nullptr;
    const float rt_eps = l2 ? dense_l2_rt_eps(h) : 0.f;
    RangePrep rp{};
    if (ranged) {  // ceilings and floors per query SLOT, as the coefficients
        HIP_TRY(h, ws->rbounds.ensure((size_t)B * 2 * sizeof(double)));
        HIP_TRY(h, ws->rhi.ensure((size_t)n_chunks * chunk_q * sizeof(float)));
        HIP_TRY(h, ws->rlo.ensure((size_t)n_chunks * chunk_q * sizeof(float)));
        int norm_mode;
        dense_eps(h, &rp.eps_abs, &norm_mode);
        rp.radius = rng->d_radius;
        rp.range_filter = rng->d_range_filter;
        rp.bounds = ws->rbounds.as<double>();
        rp.hi_a = ws->rhi.as<float>();
        rp.lo_a = ws->rlo.as<float>();
        rp.max_norm = h->max_row_norm;
        rp.metric = h->metric;
        rp.no_clamp = g_no_range_clamp;
    }
    FinishSide f;
    HR_TRY(dense_side(h, ws, d_q, B, k, C, d_mask, out, &f, ranged));

    if (phases & PHASE_PREP) {
        // every pass's queries in one launch: pass c owns fragment groups [c * Gmax, ...) of qfrag (slot = query number)
        Span sp(h, s, PH_PREP);
        const int G_total = (n_chunks - 1) * Gmax + plan_for(B - (n_chunks - 1) * chunk_q).G;
        hipLaunchKernelGGL(h->dtype == HR_F16 ? prep_queries_kernel<_Float16> : prep_queries_kernel<float>, dim3(16 * G_total),
                           dim3(256), 0, s, d_q, B, (int)h->dim, h->KT, ws->qfrag.as<chunk_t>(), ws->qn2.as<double>(), d_coef,
                           d_qeps, rt_eps, rp);
        HIP_TRY(h, hipGetLastError());
    }
    for (int c0 = 0; (phases & PHASE_SCAN) && c0 < B; c0 += chunk_q) {
        const int nq = std::min(chunk_q, B - c0);
        Span sp(h, s, PH_SCAN);
        const ScanArgs a{h, s, ws->qfrag.as<chunk_t>() + (size_t)(c0 / chunk_q) * chunk_frag, d_mask,
                         ws->gmax.as<float>() + (int64_t)c0 * f.n_groups, nq, dense_super_groups(h), l2 ? d_coef + c0 : nullptr,
                         ranged ? ws->rhi.as<float>() + c0 : nullptr};
        HIP_TRY(h, launch_scan(plan_for(nq), a));
    }
    if (scan_done) HIP_TRY(h, hipEventRecord(scan_done, s));
    return (phases & PHASE_FINISH) ? finish_enqueue(h, s, B, &f, 1) : HR_OK;
}

// Doc ranges one scan block walks (sparse_scan_kernel pipelines over them): as many as leave the chip
// about six rounds of blocks (two blocks per CU), at most 16; gridDim.y must stay below 65536.
int sparse_ranges_per_block(const hr_index* h, int B) {
    const int forced = g_sparse_rpb;
    const int64_t pairs = (int64_t)B * h->n_ranges;
    int64_t rpb = forced > 0 ? forced : std::min<int64_t>(16, pairs / (6 * 2 * (int64_t)scan_cus(h)));
    rpb = std::max<int64_t>(rpb, (h->n_ranges + 65534) / 65535);
    return (int)std::max<int64_t>(1, rpb);
}

int sparse_search_enqueue(hr_index* h, Workspace* ws, hipStream_t s, const int64_t* d_qptr, const int32_t* d_qidx,
                          const float* d_qval, int B, int max_q_nnz, int k, const uint8_t* d_mask, const OutLists& out,
                          int C, int phases = PHASE_ALL) {
    HIP_TRY(h, ws->qscale.ensure((size_t)B * sizeof(float)));
    HIP_TRY(h, ws->qeps.ensure((size_t)B * sizeof(float)));
    HIP_TRY(h, ws->qfloor.ensure((size_t)B * sizeof(float)));
    FinishSide f;
    HR_TRY(sparse_side(h, ws, d_qptr, d_qidx, d_qval, B, max_q_nnz, k, C, d_mask, out, &f));
    if (phases & PHASE_PREP) {
        HIP_TRY(h, ws->pq_n.ensure((size_t)B * 4));
        HIP_TRY(h, ws->pq_idx.ensure((size_t)B * f.stride * 4));
        HIP_TRY(h, ws->pq_w.ensure((size_t)B * f.stride * 4));
        // the largest posting weight after fp16 rounding: a nonzero weight below 2^-24 is stored as 2^-24 (sparse.h)
        const float max_post_w = h->max_sparse_abs > 0.f ? std::max(h->max_sparse_abs, 0x1p-24f) : 0.f;
        hipLaunchKernelGGL(sparse_query_prep_kernel, dim3(B), dim3(256), 0, s, d_qptr, d_qidx, d_qval, max_post_w,
                           (int)h->sparse_signed, f.stride, (int)h->sparse_dim, ws->qscale.as<float>(),
                           ws->qeps.as<float>(), ws->qfloor.as<float>(), ws->pq_n.as<int32_t>(),
                           ws->pq_idx.as<int32_t>(), ws->pq_w.as<float>());
        HIP_TRY(h, hipGetLastError());
    }
    if (phases & PHASE_SCAN) {
        Span sp(h, s, PH_SSCAN);
        const int rpb = sparse_ranges_per_block(h, B);
        const unsigned chunks = (unsigned)((h->n_ranges + rpb - 1) / rpb);
        hipLaunchKernelGGL(h->n_dense_runs > 0 ? sparse_scan_kernel<true> : sparse_scan_kernel<false>,
                           dim3((unsigned)B, chunks), dim3(kScanThreads), 0, s, h->rt_off.as<unsigned int>(),
                           h->sparse_dim + 1, h->range_base.as<int64_t>(), h->post.as<uint32_t>(), ws->pq_n.as<int32_t>(),
                           ws->pq_idx.as<int32_t>(), ws->pq_w.as<float>(), f.stride, ws->qscale.as<float>(), d_mask,
                           h->n_sparse, f.n_groups, f.GR, h->n_ranges, rpb, h->idle_post.as<uint32_t>(),
                           ws->gmax.as<float>());
        HIP_TRY(h, hipGetLastError());
    }
    return (phases & PHASE_FINISH) ? finish_enqueue(h, s, B, &f, 1) : HR_OK;
}

int check_search_args(hr_index* h, int B, int k, bool dense) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (B <= 0) return fail(h, HR_EINVAL, "batch size must be positive (got %d)", B);
    if (k <= 0) return fail(h, HR_EINVAL, "k must be positive (got %d)", k);
    if (k > HR_MAX_TOPK) return fail(h, HR_ELIMIT, "k=%d exceeds HR_MAX_TOPK=%d", k, HR_MAX_TOPK);
    if (!h->finalized) return fail(h, HR_ESTATE, "search before hr_finalize");
    if (dense && h->dim == 0) return fail(h, HR_ESTATE, "handle has no dense collection");
    if (!dense && h->sparse_dim == 0) return fail(h, HR_ESTATE, "handle has no sparse collection");
    return HR_OK;
}

// Results for an empty collection: all padding, proven exact.
int fill_empty(hr_index* h, hipStream_t s, int B, int k, int64_t* d_ids, float* d_scores, int32_t* d_flags) {
    HIP_TRY(h, hipMemsetAsync(d_ids, 0xFF, (size_t)B * k * sizeof(int64_t), s));
    HIP_TRY(h, hipMemsetAsync(d_scores, 0, (size_t)B * k * sizeof(float), s));
    if (d_flags) {
        std::vector<int32_t> ones(B, 1);
        HIP_TRY(h, hipMemcpyAsync(d_flags, ones.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return HR_OK;
}

// ---- the host-buffer forms' shared run ---------------------------------------------------------------------------
struct PooledWs {  // a workspace of the handle's pool for the length of one host-form call
    hr_index* h;
    Workspace* w;
    explicit PooledWs(hr_index* h_) : h(h_), w(take_ws(h_)) {}
    ~PooledWs() {
        if (w) give_ws(h, w);
    }
};

// What the host forms share, after their own argument checks.  rows names the modality's row count (n_rows or
// n_sparse), read here under the handle's lock.  stage_queries(ws, s) uploads the queries; enqueue(ws, s, d_mask, out,
// C) enqueues one search with C candidate groups per query, and is repeated with more of them until every list is
// proven exact or every group that holds rows was a candidate.
template <typename Stage, typename Enqueue>
int search_host(hr_index* h, int B, int k, int64_t hr_index::*rows, const uint8_t* rowmask, bool mask_on_device,
                int64_t* out_ids, float* out_scores, Stage stage_queries, Enqueue enqueue) {
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    const int64_t n_rows = h->*rows;
    if (n_rows == 0) {
        std::fill(out_ids, out_ids + (size_t)B * k, (int64_t)-1);
        std::fill(out_scores, out_scores + (size_t)B * k, 0.f);
        return HR_OK;
    }
    PooledWs pooled(h);
    Workspace* ws = pooled.w;
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    hipStream_t s = ws->stream;
    HR_TRY(stage_queries(ws, s));
    HIP_TRY(h, ws->d_ids.ensure((size_t)B * k * 8));
    HIP_TRY(h, ws->d_scores.ensure((size_t)B * k * 4));
    HIP_TRY(h, ws->flags.ensure((size_t)B * 4));
    const uint8_t* d_mask = mask_on_device ? rowmask : nullptr;
    if (rowmask && !mask_on_device) {
        const size_t mb = (size_t)(n_rows + 7) / 8;
        HIP_TRY(h, ws->d_mask.ensure(mb));
        HIP_TRY(h, hipMemcpyAsync(ws->d_mask.p, rowmask, mb, hipMemcpyHostToDevice, s));
        d_mask = ws->d_mask.as<uint8_t>();
    }
    const OutLists out{ws->d_ids.as<int64_t>(), ws->d_scores.as<float>(), ws->flags.as<int32_t>()};
    // the groups that hold rows — not the group slots of FinishSide::n_groups, which for dense include the -inf tail
    const int GR = group_rows_for(h, n_rows);
    const int64_t n_row_groups = (n_rows + GR - 1) / GR;
    int C = candidate_groups_for_k(k);
    std::vector<int32_t> flags(B);
    for (;;) {
        HR_TRY(enqueue(ws, s, d_mask, out, C));
        HIP_TRY(h, hipMemcpyAsync(flags.data(), ws->flags.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const bool all_exact = std::all_of(flags.begin(), flags.end(), [](int32_t f) { return f != 0; });
        if (all_exact || C >= n_row_groups) break;
        C = next_candidate_count(C, n_row_groups);  // widen the candidate set and redo
    }
    HIP_TRY(h, hipMemcpyAsync(out_ids, out.ids, (size_t)B * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_scores, out.scores, (size_t)B * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return HR_OK;
}

// ---- the dense store's capacity ------------------------------------------------------------------------------------
// The one rule.  Capacity is a whole number of super-groups (kSuperRows).  hr_reserve on an EMPTY handle gets exactly
// what it asks for, one super-group at least.  Every other growth — an append, and hr_reserve on a handle that already
// has a store — takes at least 1.5x the old capacity and at least 1024 rows, so that repeated appends copy amortised
// O(rows appended).
int64_t dense_capacity_for(int64_t cap_rows, int64_t need_rows, bool reserving) {
    const int64_t need = round_up(need_rows, kSuperRows);
    if (reserving && cap_rows == 0) return std::max<int64_t>(need, kSuperRows);
    return std::max<int64_t>({need, round_up(cap_rows + cap_rows / 2, kSuperRows), 1024});
}

// Gives the dense store `rows` rows of capacity (a multiple of kSuperRows, not below cap_rows): the old contents in
// front, zeros behind them — every scan and snapshot expects zeros beyond n_rows.  The handle changes only after the
// last call that can fail; until then the new buffers belong to this scope, and an early return frees them.
int set_dense_capacity(hr_index* h, int64_t rows) {
    DevBuf tiles, scale, norm2;
    const size_t tb = tile_bytes_for_rows(h, rows);
    if (tiles.alloc_exact(tb) != hipSuccess || scale.alloc_exact((size_t)rows * 4) != hipSuccess ||
        norm2.alloc_exact((size_t)rows * 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "cannot allocate dense shard for %lld rows (%zu bytes)", (long long)rows, tb);
    }
    hipStream_t s = h->ingest_stream;
    HIP_TRY(h, hipMemsetAsync(tiles.p, 0, tiles.cap, s));
    HIP_TRY(h, hipMemsetAsync(scale.p, 0, scale.cap, s));
    HIP_TRY(h, hipMemsetAsync(norm2.p, 0, norm2.cap, s));
    if (h->cap_rows > 0) {
        HIP_TRY(h, hipMemcpyAsync(tiles.p, h->tiles.p, tile_bytes_for_rows(h, h->cap_rows), hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(scale.p, h->scale.p, (size_t)h->cap_rows * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(norm2.p, h->norm2.p, (size_t)h->cap_rows * 8, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    h->tiles = std::move(tiles);
    h->scale = std::move(scale);
    h->norm2 = std::move(norm2);
    h->cap_rows = rows;
    return HR_OK;
}

int grow_dense(hr_index* h, int64_t need_rows) {
    if (need_rows <= h->cap_rows) return HR_OK;
    return set_dense_capacity(h, dense_capacity_for(h->cap_rows, need_rows, false));
}

constexpr unsigned long long kNoBadRow = ~0ull;

template <typename SRC>
int add_dense_impl(hr_index* h, const SRC* rows, int64_t n, bool src_on_device, hipStream_t user_stream) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (h->dim == 0) return fail(h, HR_ESTATE, "handle has no dense collection");
    if (n < 0 || (n > 0 && !rows)) return fail(h, HR_EINVAL, "bad rows/n");
    if (n == 0) return HR_OK;
    std::unique_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    HR_TRY(grow_dense(h, h->n_rows + n));
    hipStream_t s = src_on_device && user_stream ? user_stream : h->ingest_stream;
    const int64_t chunk_rows = std::max<int64_t>(1, (64ll << 20) / (h->dim * (int64_t)sizeof(SRC)));
    const int kchunks = h->KT * 4;
    unsigned long long* d_bad = h->bad_row.as<unsigned long long>();
    for (int64_t r0 = 0; r0 < n; r0 += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - r0);
        const SRC* src = rows + r0 * h->dim;
        if (!src_on_device) {
            HIP_TRY(h, h->stage.ensure((size_t)m * h->dim * sizeof(SRC)));
            HIP_TRY(h, hipMemcpyAsync(h->stage.p, src, (size_t)m * h->dim * sizeof(SRC), hipMemcpyHostToDevice, s));
            src = h->stage.as<SRC>();
        }
        const int64_t threads = m * kchunks;
        const unsigned blocks = (unsigned)((threads + 255) / 256);
        with_store(h->dtype, [&](auto store) {
            using STORE = decltype(store);
            // an fp32 store is only ever fed fp32 rows (hr_add_dense_raw*); an fp16 store takes fp32 or fp16 ones
            using IN = std::conditional_t<std::is_same<STORE, float>::value, float, SRC>;
            hipLaunchKernelGGL((tile_rows_kernel<STORE, IN>), dim3(blocks), dim3(256), 0, s, reinterpret_cast<const IN*>(src), m,
                               (int)h->dim, h->KT, h->n_rows + r0, h->tiles.as<chunk_t>(), r0, d_bad);
        });
        HIP_TRY(h, hipGetLastError());
        if (!src_on_device) HIP_TRY(h, hipStreamSynchronize(s));  // staging buffer is reused
    }
    // the flag rides on the synchronisation the append needs anyway
    unsigned long long bad = kNoBadRow;
    HIP_TRY(h, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (bad != kNoBadRow) {
        // refused: the handle stays as it was.  The rows beyond n_rows go back to the zeros every scan and snapshot
        // expects there, and the flag to its rest value.
        const int64_t threads = n * kchunks;
        hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, n, h->KT,
                           h->n_rows, h->tiles.as<chunk_t>());
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemsetAsync(d_bad, 0xFF, sizeof bad, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        return fail(h, HR_EINVAL, "dense row %lld of the batch holds a value that is NaN or infinite in the shard's %s store",
                    (long long)bad, h->dtype == HR_F16 ? "fp16" : "fp32");
    }
    h->n_rows += n;
    h->finalized = false;
    return HR_OK;
}

// One CSR batch as hr_add_sparse and hr_load accept it: indptr monotone, indices in [0, sparse_dim) and strictly
// ascending inside a row, values finite and within the fp16 posting range.  *batch_max receives max |value|, *batch_neg
// whether some value is negative.
int validate_csr(const hr_index* h, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                 float* batch_max, bool* batch_neg) {
    float mx = 0.f;
    bool neg = false;
    for (int64_t r = 0; r < n; ++r) {
        if (indptr[r + 1] < indptr[r]) return fail(h, HR_EINVAL, "indptr not monotone at row %lld", (long long)r);
        int32_t prev = -1;
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            const int32_t t = indices[e];
            if (t < 0 || t >= h->sparse_dim)
                return fail(h, HR_EINVAL, "sparse index %d out of range [0,%lld) in row %lld", t, (long long)h->sparse_dim, (long long)r);
            if (t <= prev) return fail(h, HR_EINVAL, "sparse indices must be strictly ascending (row %lld)", (long long)r);
            if (!std::isfinite(values[e])) return fail(h, HR_EINVAL, "non-finite sparse value in row %lld", (long long)r);
            if (std::fabs(values[e]) > 60000.f)
                return fail(h, HR_ELIMIT, "sparse weight %g in row %lld exceeds the fp16 posting range", (double)values[e], (long long)r);
            mx = std::max(mx, std::fabs(values[e]));
            neg |= values[e] < 0.f;
            prev = t;
        }
    }
    *batch_max = mx;
    *batch_neg = neg;
    return HR_OK;
}

// Bring the device-side sparse shard up to date with the rows staged since the last call.
// The staged CSR rows are appended to the device CSR (kept for the canonical refine); the range-major postings are
// rebuilt only from the range that holds the first new doc onwards — earlier ranges' posting blocks and offset rows
// stay where they are — so a flush after a small append costs O(batch + one range), not O(corpus), and the host
// keeps no copy of the corpus (reference indexing.py:377-431: insert + flush per index_chunks call).
int build_sparse(hr_index* h) {
    hipStream_t s = h->ingest_stream;
    const int64_t n = h->n_sparse;
    const int64_t V1 = h->sparse_dim + 1;
    if (h->n_csr == n && h->n_sparse_built == n) return HR_OK;
    // 1. append the staged rows to the device CSR.  Restartable: the staging vectors are only read here (the absolute
    //    row pointers are built in a temporary), and the CSR watermark (n_csr, nnz_csr) is committed together with the
    //    release of the staging vectors — a failure before that leaves everything as it was, a failure after it
    //    (step 2) is retried from the device CSR alone.
    if (h->n_csr < n) {
        const int64_t n0 = h->n_csr, nnz0 = h->nnz_csr;
        const int64_t new_nnz = (int64_t)h->pend_idx.size();
        const int64_t nnz = nnz0 + new_nnz;
        if ((int64_t)h->pend_indptr.size() != n - n0 + 1) return fail(h, HR_ESTATE, "sparse staging out of step with the row count");
        std::vector<int64_t> abs_ptr;
        try {
            abs_ptr.resize(h->pend_indptr.size());
        } catch (const std::exception&) {
            return fail(h, HR_ENOMEM, "out of host memory building sparse row pointers");
        }
        for (size_t i = 0; i < abs_ptr.size(); ++i) abs_ptr[i] = h->pend_indptr[i] + nnz0;  // absolute entry numbers
        HIP_TRY(h, h->s_indptr.grow((size_t)(n + 1) * 8, (size_t)(n0 + 1) * 8, s));
        HIP_TRY(h, h->s_idx.grow((size_t)std::max<int64_t>(nnz, 1) * 4, (size_t)nnz0 * 4, s));
        HIP_TRY(h, h->s_val.grow((size_t)std::max<int64_t>(nnz, 1) * 4, (size_t)nnz0 * 4, s));
        HIP_TRY(h, hipMemcpyAsync(h->s_indptr.as<int64_t>() + n0, abs_ptr.data(), (size_t)(n - n0 + 1) * 8,
                                  hipMemcpyHostToDevice, s));
        if (new_nnz) {
            HIP_TRY(h, hipMemcpyAsync(h->s_idx.as<int32_t>() + nnz0, h->pend_idx.data(), (size_t)new_nnz * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(h, hipMemcpyAsync(h->s_val.as<float>() + nnz0, h->pend_val.data(), (size_t)new_nnz * 4, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(h, hipStreamSynchronize(s));  // the staging vectors are released below
        std::vector<int64_t>{0}.swap(h->pend_indptr);
        std::vector<int32_t>().swap(h->pend_idx);
        std::vector<float>().swap(h->pend_val);
        h->n_csr = n;
        h->nnz_csr = nnz;
    }
    if (h->fault_inject == 1) {  // test hook: what an allocation failure in step 2 leaves behind
        h->fault_inject = 0;
        return fail(h, HR_ENOMEM, "injected failure after the CSR upload (hr_debug_inject_fault)");
    }
    // 2. rebuild the posting blocks of ranges r_d .. n_ranges-1 from the device CSR.  Nothing is committed before the
    //    last kernel has finished: a retry starts again from the same r_d (h_range_base[0 .. r_d] is never rewritten).
    const int64_t n0 = h->n_sparse_built;
    const int64_t r_d = n0 / kRangeDocs;          // range of the first new doc
    const int64_t doc0 = r_d * kRangeDocs;
    const int64_t n_ranges = (n + kRangeDocs - 1) / kRangeDocs;
    const int64_t dirty = n_ranges - r_d;
    HIP_TRY(h, h->rt_off.grow((size_t)n_ranges * V1 * 4, (size_t)r_d * V1 * 4, s));
    HIP_TRY(h, hipMemsetAsync(h->rt_off.as<unsigned int>() + r_d * V1, 0, (size_t)dirty * V1 * 4, s));
    const unsigned doc_blocks = (unsigned)((n - doc0 + 255) / 256);
    hipLaunchKernelGGL(sparse_count_kernel, dim3(doc_blocks), dim3(256), 0, s, h->s_indptr.as<int64_t>(),
                       h->s_idx.as<int32_t>(), doc0, n, V1, h->rt_off.as<unsigned int>());
    HIP_TRY(h, hipGetLastError());
    DevBuf totals, cursor;  // scratch of this call
    HIP_TRY(h, totals.ensure((size_t)dirty * 8));
    hipLaunchKernelGGL(sparse_scan_offsets_kernel, dim3((unsigned)dirty), dim3(1024), 0, s,
                       h->rt_off.as<unsigned int>(), V1, r_d, totals.as<unsigned long long>());
    HIP_TRY(h, hipGetLastError());
    std::vector<unsigned long long> ht(dirty);
    HIP_TRY(h, hipMemcpyAsync(ht.data(), totals.p, (size_t)dirty * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->h_range_base.resize(n_ranges + 1);
    h->h_range_dense.resize(n_ranges);
    for (int64_t r = r_d; r < n_ranges; ++r) {
        h->h_range_base[r + 1] = h->h_range_base[r] + (int64_t)(ht[r - r_d] & 0xFFFFFFFFull);
        h->h_range_dense[r] = (unsigned)(ht[r - r_d] >> 32);
    }
    // runs are padded to 4 postings (filler postings); + slack: the scan fetches 16 bytes at a time
    HIP_TRY(h, h->post.grow((size_t)h->h_range_base[n_ranges] * 4 + 64, (size_t)h->h_range_base[r_d] * 4, s));
    HIP_TRY(h, h->range_base.grow((size_t)(n_ranges + 1) * 8, 0, s));
    HIP_TRY(h, hipMemcpyAsync(h->range_base.p, h->h_range_base.data(), (size_t)(n_ranges + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(h, cursor.ensure((size_t)dirty * V1 * 4));
    HIP_TRY(h, hipMemcpyAsync(cursor.p, h->rt_off.as<unsigned int>() + r_d * V1, (size_t)dirty * V1 * 4,
                              hipMemcpyDeviceToDevice, s));
    // dense runs (sparse.h) hold one fp16 weight per doc of the range: every word of the rebuilt blocks starts as "absent /
    // absent"; sparse runs and their fillers are overwritten whole by the two kernels below
    {
        const int64_t w0 = h->h_range_base[r_d], w1 = h->h_range_base[n_ranges];
        if (w1 > w0)
            HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)(h->post.as<uint32_t>() + w0), (int)0x80008000u, (size_t)(w1 - w0), s));
    }
    // (the fill kernel permutes docs inside aligned blocks of 128: its grid covers whole blocks)
    hipLaunchKernelGGL(sparse_fill_kernel, dim3((unsigned)((round_up(n - doc0, 128) + 255) / 256)), dim3(256), 0, s, h->s_indptr.as<int64_t>(),
                       h->s_idx.as<int32_t>(), h->s_val.as<float>(), doc0, n, V1, cursor.as<unsigned int>(),
                       h->rt_off.as<unsigned int>(), h->range_base.as<int64_t>(), h->post.as<uint32_t>());
    HIP_TRY(h, hipGetLastError());
    const int64_t pairs = dirty * h->sparse_dim;
    hipLaunchKernelGGL(sparse_pad_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s,
                       h->rt_off.as<unsigned int>(), cursor.as<unsigned int>(), V1, r_d, n_ranges,
                       h->range_base.as<int64_t>(), h->post.as<uint32_t>());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    h->n_ranges = n_ranges;
    h->n_sparse_built = n;
    h->n_dense_runs = 0;
    for (unsigned c : h->h_range_dense) h->n_dense_runs += c;
    return HR_OK;
}

// ---- compaction (compact.h) ------------------------------------------------------------------------------------------
// Exclusive scan of f(0 .. n) on stream s: on return (enqueued) block_off holds the exclusive prefix of the sums of
// blocks of kCompactBlock elements, d_total[0] their total.
template <typename F>
int compact_scan_blocks(hr_index* h, hipStream_t s, F f, int64_t n, DevBuf& block_off, unsigned long long* d_total) {
    const int64_t nb = (n + kCompactBlock - 1) / kCompactBlock;
    if (block_off.alloc_exact((size_t)std::max<int64_t>(nb, 1) * 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "cannot allocate the compaction scan (%lld blocks)", (long long)nb);
    }
    hipLaunchKernelGGL((compact_block_sums_kernel<F>), dim3((unsigned)nb), dim3(kCompactBlock), 0, s, f, n,
                       block_off.as<unsigned long long>());
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(compact_scan_sums_kernel, dim3(1), dim3(kCompactBlock), 0, s, block_off.as<unsigned long long>(), nb, d_total);
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}

// The row map of the first n rows under the keep mask: src_of[new row] = old row (ascending), *kept = its length.
int compact_row_map(hr_index* h, hipStream_t s, const unsigned long long* d_mask, int64_t n, DevBuf& src_of, int64_t* kept) {
    *kept = 0;
    if (n == 0) return HR_OK;
    const int64_t n_words = (n + 63) / 64;
    DevBuf block_off, total;
    if (total.alloc_exact(8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "cannot allocate the compaction scan");
    }
    HR_TRY(compact_scan_blocks(h, s, KeepCount{d_mask, n}, n_words, block_off, total.as<unsigned long long>()));
    unsigned long long n_kept = 0;
    HIP_TRY(h, hipMemcpyAsync(&n_kept, total.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *kept = (int64_t)n_kept;
    if (n_kept == 0 || (int64_t)n_kept == n) return HR_OK;  // nothing to gather / nothing to drop: no map needed
    if (src_of.alloc_exact((size_t)n_kept * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "cannot allocate the row map of %llu rows", n_kept);
    }
    const unsigned blocks = (unsigned)((n_words + kCompactBlock - 1) / kCompactBlock);
    hipLaunchKernelGGL(compact_row_map_kernel, dim3(blocks), dim3(kCompactBlock), 0, s, d_mask, n, n_words,
                       block_off.as<unsigned long long>(), (int64_t)n_kept, src_of.as<uint32_t>());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));  // block_off is scratch of this scope
    return HR_OK;
}

// The new dense store of the survivors (the handle is not touched): gathered tiles, per-row values and the maximum norm.
struct CompactDense {
    DevBuf tiles, scale, norm2, max_norm;
    int64_t cap_rows = 0;
};
int compact_dense(hr_index* h, hipStream_t s, const uint32_t* d_src_of, int64_t kept, CompactDense* out, hipEvent_t* span) {
    out->cap_rows = dense_capacity_for(0, kept, true);
    const size_t tb = tile_bytes_for_rows(h, out->cap_rows);
    if (out->tiles.alloc_exact(tb) != hipSuccess || out->scale.alloc_exact((size_t)out->cap_rows * 4) != hipSuccess ||
        out->norm2.alloc_exact((size_t)out->cap_rows * 8) != hipSuccess || out->max_norm.alloc_exact(4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "cannot allocate the compacted dense shard for %lld rows (%zu bytes) beside the old one",
                    (long long)out->cap_rows, tb);
    }
    // zeros beyond the last row block that holds a survivor (the gather writes that block whole, its ragged lanes as zeros)
    const int64_t n_dst_blocks = (kept + kRowsPerBlock - 1) / kRowsPerBlock;
    const size_t written = (size_t)n_dst_blocks * h->KT * 1024;
    if (tb > written) HIP_TRY(h, hipMemsetAsync((char*)out->tiles.p + written, 0, tb - written, s));
    HIP_TRY(h, hipMemsetAsync(out->scale.p, 0, out->scale.cap, s));
    HIP_TRY(h, hipMemsetAsync(out->norm2.p, 0, out->norm2.cap, s));
    HIP_TRY(h, hipMemsetAsync(out->max_norm.p, 0, 4, s));
    if (kept == 0) return HR_OK;
    if (span) HIP_TRY(h, hipEventRecord(span[0], s));
    hipLaunchKernelGGL(compact_tiles_kernel, dim3((unsigned)((n_dst_blocks + kCompactWaves - 1) / kCompactWaves)),
                       dim3(kCompactWaves * 64), 0, s, h->tiles.as<chunk_t>(), d_src_of, kept, h->KT, n_dst_blocks,
                       out->tiles.as<chunk_t>());
    HIP_TRY(h, hipGetLastError());
    if (span) HIP_TRY(h, hipEventRecord(span[1], s));
    hipLaunchKernelGGL(compact_row_values_kernel, dim3((unsigned)((kept + 255) / 256)), dim3(256), 0, s, h->scale.as<float>(),
                       h->norm2.as<double>(), d_src_of, kept, out->scale.as<float>(), out->norm2.as<double>(),
                       out->max_norm.as<unsigned int>());
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}

// The new CSR of the surviving sparse rows (the handle is not touched), exactly as large as it has to be.
struct CompactSparse {
    DevBuf indptr, idx, val, stats;
    int64_t nnz = 0;
};
int compact_sparse(hr_index* h, hipStream_t s, const uint32_t* d_src_of, int64_t kept, CompactSparse* out) {
    if (kept == 0) return HR_OK;
    DevBuf block_off, total;
    if (out->indptr.alloc_exact((size_t)(kept + 1) * 8) != hipSuccess || out->stats.alloc_exact(8) != hipSuccess ||
        total.alloc_exact(8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "cannot allocate the compacted sparse rows (%lld) beside the old ones", (long long)kept);
    }
    const RowLength len{h->s_indptr.as<int64_t>(), d_src_of};
    HR_TRY(compact_scan_blocks(h, s, len, kept, block_off, total.as<unsigned long long>()));
    hipLaunchKernelGGL(compact_indptr_kernel, dim3((unsigned)((kept + kCompactBlock - 1) / kCompactBlock)), dim3(kCompactBlock), 0, s,
                       len, kept, block_off.as<unsigned long long>(), out->indptr.as<int64_t>());
    HIP_TRY(h, hipGetLastError());
    unsigned long long nnz = 0;
    HIP_TRY(h, hipMemcpyAsync(&nnz, total.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // the entry buffers are sized by it
    out->nnz = (int64_t)nnz;
    if (out->idx.alloc_exact((size_t)std::max<int64_t>(out->nnz, 1) * 4) != hipSuccess ||
        out->val.alloc_exact((size_t)std::max<int64_t>(out->nnz, 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "cannot allocate the compacted sparse entries (%lld) beside the old ones", (long long)out->nnz);
    }
    HIP_TRY(h, hipMemsetAsync(out->stats.p, 0, 8, s));
    hipLaunchKernelGGL(compact_csr_kernel, dim3((unsigned)((kept + 3) / 4)), dim3(256), 0, s, h->s_indptr.as<int64_t>(),
                       h->s_idx.as<int32_t>(), h->s_val.as<float>(), d_src_of, kept, out->indptr.as<int64_t>(),
                       out->idx.as<int32_t>(), out->val.as<float>(), out->stats.as<unsigned int>());
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}

}  // namespace

// =============================================================================
extern "C" {

int hr_version(void) { return 12200; }  // 1.22.0: MaxSim as a first-stage search (hr_maxsim_scan_dev)

const char* hr_last_error(const hr_index* h) {
    if (!h) return g_last_error.c_str();
    std::lock_guard<std::mutex> g(h->err_mu);
    g_last_error = h->err;  // hand back a pointer that outlives the lock
    return g_last_error.c_str();
}

int hr_create(int device, int64_t dim, int dtype, int metric, int64_t sparse_dim, hr_index** out) {
    if (!out) return fail(nullptr, HR_EINVAL, "out is null");
    *out = nullptr;
    if (dim < 0 || sparse_dim < 0 || (dim == 0 && sparse_dim == 0))
        return fail(nullptr, HR_EINVAL, "need dim > 0 and/or sparse_dim > 0");
    if (dim > HR_MAX_DIM) return fail(nullptr, HR_ELIMIT, "dim=%lld exceeds HR_MAX_DIM=%d", (long long)dim, HR_MAX_DIM);
    if (dtype != HR_F32 && dtype != HR_F16) return fail(nullptr, HR_EINVAL, "unknown dtype %d", dtype);
    if (metric != HR_METRIC_IP && metric != HR_METRIC_COSINE && metric != HR_METRIC_L2) return fail(nullptr, HR_EINVAL, "unknown metric %d", metric);
    if (sparse_dim > (1ll << 24)) return fail(nullptr, HR_ELIMIT, "sparse_dim too large");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, HR_EHIP, "no HIP device available (%s); libhbmrag has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    }
    if (device < 0 || device >= count) return fail(nullptr, HR_EINVAL, "device %d out of range (0..%d)", device, count - 1);
    hr_index* h = new (std::nothrow) hr_index();
    if (!h) return fail(nullptr, HR_ENOMEM, "out of host memory");
    h->device = device;
    h->dim = dim;
    h->dtype = dtype;
    h->metric = metric;
    h->sparse_dim = sparse_dim;
    if (dim > 0) {
        const int tile_elems = 4 * elems_per_chunk(dtype);
        h->KT = (int)round_up((dim + tile_elems - 1) / tile_elems, 4);  // multiple of the scan's prefetch depth
    }
    h->group_rows_override = g_group_rows;
    DeviceGuard dg(device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->cu_count = prop.multiProcessorCount;
    uint32_t idle[256];  // idle postings of scan lane l: weight 0, accumulator pad word l
    for (unsigned l = 0; l < 256; ++l) idle[l] = filler_posting(l / 4);
    if (hipStreamCreateWithFlags(&h->ingest_stream, hipStreamNonBlocking) != hipSuccess ||
        h->max_norm.alloc_exact(4) != hipSuccess || hipMemset(h->max_norm.p, 0, 4) != hipSuccess ||
        h->bad_row.alloc_exact(8) != hipSuccess || hipMemset(h->bad_row.p, 0xFF, 8) != hipSuccess ||
        h->idle_post.alloc_exact(sizeof idle) != hipSuccess ||
        hipMemcpy(h->idle_post.p, idle, sizeof idle, hipMemcpyHostToDevice) != hipSuccess) {
        int rc = fail(nullptr, HR_EHIP, "device %d initialisation failed: %s", device, hipGetErrorString(hipGetLastError()));
        delete h;  // under dg: the handle frees what it got so far on its own device
        return rc;
    }
    *out = h;
    return HR_OK;
}

void hr_destroy(hr_index* h) {
    if (!h) return;
    DeviceGuard dg(h->device);  // outlives the handle: every buffer is freed on its own device
    (void)hipDeviceSynchronize();
    delete h;
}

int hr_set_row_offset(hr_index* h, int64_t first_row) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (first_row < 0) return fail(h, HR_EINVAL, "row offset must be >= 0");
    h->row_offset = first_row;
    return HR_OK;
}

int hr_reserve(hr_index* h, int64_t n_rows) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (h->dim == 0) return fail(h, HR_ESTATE, "handle has no dense collection");
    if (n_rows < 0 || n_rows > (1ll << 31) - 64) return fail(h, HR_ELIMIT, "row count out of range");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    if (n_rows <= h->cap_rows) return HR_OK;
    return set_dense_capacity(h, dense_capacity_for(h->cap_rows, n_rows, true));
}

int hr_add_dense(hr_index* h, const float* rows, int64_t n) {
    return add_dense_impl<float>(h, rows, n, false, nullptr);
}

int hr_add_dense_raw(hr_index* h, const void* rows, int64_t n) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (h->dtype == HR_F16) return add_dense_impl<_Float16>(h, static_cast<const _Float16*>(rows), n, false, nullptr);
    return add_dense_impl<float>(h, static_cast<const float*>(rows), n, false, nullptr);
}

int hr_add_dense_raw_dev(hr_index* h, const void* d_rows, int64_t n, void* stream) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (h->dtype == HR_F16)
        return add_dense_impl<_Float16>(h, static_cast<const _Float16*>(d_rows), n, true, (hipStream_t)stream);
    return add_dense_impl<float>(h, static_cast<const float*>(d_rows), n, true, (hipStream_t)stream);
}

int hr_add_sparse(hr_index* h, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (h->sparse_dim == 0) return fail(h, HR_ESTATE, "handle has no sparse collection");
    if (n < 0 || (n > 0 && !indptr)) return fail(h, HR_EINVAL, "bad indptr/n");
    if (n == 0) return HR_OK;
    const int64_t nnz = indptr[n] - indptr[0];
    if (nnz < 0 || (nnz > 0 && (!indices || !values))) return fail(h, HR_EINVAL, "bad indices/values");
    float batch_max = 0.f;
    bool batch_neg = false;
    HR_TRY(validate_csr(h, indptr, indices, values, n, &batch_max, &batch_neg));
    std::unique_lock<std::shared_mutex> lk(h->rw);
    if (h->n_sparse + n > (1ll << 31) - 64) return fail(h, HR_ELIMIT, "too many sparse rows");
    try {  // staged on the host only until the next hr_finalize uploads them
        const int64_t base = h->pend_indptr.back() - indptr[0];
        h->pend_indptr.reserve(h->pend_indptr.size() + n);
        for (int64_t r = 1; r <= n; ++r) h->pend_indptr.push_back(indptr[r] + base);
        h->pend_idx.insert(h->pend_idx.end(), indices + indptr[0], indices + indptr[n]);
        h->pend_val.insert(h->pend_val.end(), values + indptr[0], values + indptr[n]);
    } catch (const std::exception&) {
        return fail(h, HR_ENOMEM, "out of host memory staging sparse rows");
    }
    h->n_sparse += n;
    h->max_sparse_abs = std::max(h->max_sparse_abs, batch_max);
    h->sparse_signed = h->sparse_signed || batch_neg;
    h->finalized = false;
    return HR_OK;
}

int hr_finalize(hr_index* h) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    hipStream_t s = h->ingest_stream;
    // `*_dev` searches drop their shared lock once their kernels are enqueued: a scan still running on a caller's stream
    // must not see the run tables and posting blocks of the dirty ranges while they are rebuilt in place
    if ((h->dim > 0 && h->n_normed < h->n_rows) || (h->sparse_dim > 0 && h->n_sparse_built != h->n_sparse))
        HIP_TRY(h, hipDeviceSynchronize());
    if (h->dim > 0 && h->n_normed < h->n_rows) {
        const int64_t n = h->n_rows - h->n_normed;
        const unsigned blocks = (unsigned)((n + 255) / 256);
        with_store(h->dtype, [&](auto store) {
            hipLaunchKernelGGL((row_norms_kernel<decltype(store)>), dim3(blocks), dim3(256), 0, s, h->tiles.as<chunk_t>(), h->KT,
                               h->n_normed, n, h->metric, h->norm2.as<double>(), h->scale.as<float>(),
                               h->max_norm.as<unsigned int>());
        });
        HIP_TRY(h, hipGetLastError());
        unsigned int bits = 0;
        HIP_TRY(h, hipMemcpyAsync(&bits, h->max_norm.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        std::memcpy(&h->max_row_norm, &bits, 4);
        h->n_normed = h->n_rows;
    }
    if (h->sparse_dim > 0 && (h->n_sparse_built != h->n_sparse || h->n_csr != h->n_sparse)) HR_TRY(build_sparse(h));
    h->finalized = true;
    return HR_OK;
}

int hr_compact(hr_index* h, const uint8_t* keep, int on_device, int64_t* kept_dense, int64_t* kept_sparse) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (!keep) return fail(h, HR_EINVAL, "null keep mask");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    if (!h->finalized) return fail(h, HR_ESTATE, "hr_compact before hr_finalize (pending rows must be flushed first)");
    using clk = std::chrono::steady_clock;
    const clk::time_point t_call = clk::now();
    struct Events {  // hr_set_profiling: the tile gather between two events
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    bool timed = false;
    if (h->profiling && (hipEventCreate(&ev.e[0]) != hipSuccess || hipEventCreate(&ev.e[1]) != hipSuccess))
        return fail(h, HR_EHIP, "cannot create the profiling events");
    // `*_dev` searches drop their shared lock once their kernels are enqueued: none may still read the old store
    HIP_TRY(h, hipDeviceSynchronize());
    hipStream_t s = h->ingest_stream;
    const bool dense = h->dim > 0 && h->n_rows > 0, sparse = h->sparse_dim > 0 && h->n_sparse > 0;
    const int64_t n = std::max(h->n_rows, h->n_sparse);
    if (kept_dense) *kept_dense = h->n_rows;
    if (kept_sparse) *kept_sparse = h->n_sparse;
    if (n == 0) return HR_OK;

    // ---- everything new is built beside the old store; the handle is untouched until the commit below ----
    DevBuf mask_buf;
    const unsigned long long* d_mask = reinterpret_cast<const unsigned long long*>(keep);
    if (!on_device) {
        const size_t words = (size_t)((n + 63) / 64);
        if (mask_buf.alloc_exact(words * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, HR_ENOMEM, "cannot allocate the keep mask");
        }
        HIP_TRY(h, hipMemsetAsync(mask_buf.p, 0, words * 8, s));
        HIP_TRY(h, hipMemcpyAsync(mask_buf.p, keep, (size_t)((n + 7) / 8), hipMemcpyHostToDevice, s));
        d_mask = mask_buf.as<unsigned long long>();
    }
    DevBuf map_d, map_s;  // one map serves both collections when they hold the same rows
    int64_t kd = 0, ks = 0;
    if (dense) HR_TRY(compact_row_map(h, s, d_mask, h->n_rows, map_d, &kd));
    if (sparse) {
        if (dense && h->n_sparse == h->n_rows) ks = kd;
        else HR_TRY(compact_row_map(h, s, d_mask, h->n_sparse, map_s, &ks));
    }
    if (kd == h->n_rows && ks == h->n_sparse) return HR_OK;  // every row stays: nothing changes, capacity included
    const uint32_t* src_d = map_d.as<uint32_t>();
    const uint32_t* src_s = map_s.p ? map_s.as<uint32_t>() : src_d;
    CompactDense nd;
    CompactSparse nsp;
    if (dense && kd < h->n_rows) {
        timed = h->profiling && kd > 0;
        HR_TRY(compact_dense(h, s, src_d, kd, &nd, timed ? ev.e : nullptr));
    }
    if (sparse && ks < h->n_sparse) HR_TRY(compact_sparse(h, s, src_s, ks, &nsp));
    unsigned int norm_bits = 0, stats[2] = {0u, 0u};
    if (nd.max_norm.p) HIP_TRY(h, hipMemcpyAsync(&norm_bits, nd.max_norm.p, 4, hipMemcpyDeviceToHost, s));
    if (nsp.stats.p) HIP_TRY(h, hipMemcpyAsync(stats, nsp.stats.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));

    auto wall_ms = [](clk::time_point a) { return std::chrono::duration<float, std::milli>(clk::now() - a).count(); };
    h->compact_ms[0] = h->compact_ms[2] = 0.f;
    if (timed) (void)hipEventElapsedTime(&h->compact_ms[0], ev.e[0], ev.e[1]);

    // ---- commit: nothing below can fail before the posting rebuild ----
    if (dense && kd < h->n_rows) {
        h->tiles = std::move(nd.tiles);
        h->scale = std::move(nd.scale);
        h->norm2 = std::move(nd.norm2);
        h->max_norm = std::move(nd.max_norm);
        h->cap_rows = nd.cap_rows;
        h->n_rows = h->n_normed = kd;
        std::memcpy(&h->max_row_norm, &norm_bits, 4);
    }
    if (kept_dense) *kept_dense = h->n_rows;
    if (sparse && ks < h->n_sparse) {
        h->s_indptr = std::move(nsp.indptr);
        h->s_idx = std::move(nsp.idx);
        h->s_val = std::move(nsp.val);
        h->n_sparse = h->n_csr = ks;
        h->nnz_csr = nsp.nnz;
        std::memcpy(&h->max_sparse_abs, &stats[0], 4);
        h->sparse_signed = stats[1] != 0;
        // the postings are rebuilt from range 0: until that has happened the handle is what a failed hr_finalize leaves
        h->rt_off.release();
        h->range_base.release();
        h->post.release();
        std::vector<int64_t>{0}.swap(h->h_range_base);
        std::vector<unsigned>().swap(h->h_range_dense);
        h->n_sparse_built = 0;
        h->n_ranges = 0;
        h->n_dense_runs = 0;
        h->finalized = false;
        if (kept_sparse) *kept_sparse = ks;
        const clk::time_point t_build = clk::now();
        HR_TRY(build_sparse(h));
        h->compact_ms[2] = wall_ms(t_build);
        h->finalized = true;
    }
    h->compact_ms[1] = wall_ms(t_call);
    return HR_OK;
}

namespace {
struct SnapHeader {
    char magic[8];
    int32_t version, dtype, metric, KT;
    int64_t dim, sparse_dim, n_rows, cap_rows, n_sparse, nnz, row_offset;
    float max_row_norm, max_sparse_abs;
    int64_t file_bytes;  // header + every section: a truncated file is refused before anything is uploaded
};
const char kSnapMagic[8] = {'H', 'B', 'M', 'R', 'A', 'G', '0', '2'};

struct File {
    FILE* f = nullptr;
    ~File() { if (f) fclose(f); }
};

// device <-> file in 64 MiB pieces through a host bounce buffer
int stream_out(hr_index* h, FILE* f, const void* dptr, size_t bytes) {
    std::vector<char> buf(std::min<size_t>(bytes, 64u << 20));
    for (size_t off = 0; off < bytes; off += buf.size()) {
        const size_t n = std::min(buf.size(), bytes - off);
        HIP_TRY(h, hipMemcpy(buf.data(), (const char*)dptr + off, n, hipMemcpyDeviceToHost));
        if (fwrite(buf.data(), 1, n, f) != n) return fail(h, HR_EINVAL, "snapshot write failed");
    }
    return HR_OK;
}
int stream_in(hr_index* h, FILE* f, void* dptr, size_t bytes) {
    std::vector<char> buf(std::min<size_t>(bytes, 64u << 20));
    for (size_t off = 0; off < bytes; off += buf.size()) {
        const size_t n = std::min(buf.size(), bytes - off);
        if (fread(buf.data(), 1, n, f) != n) return fail(h, HR_EINVAL, "snapshot truncated");
        HIP_TRY(h, hipMemcpy((char*)dptr + off, buf.data(), n, hipMemcpyHostToDevice));
    }
    return HR_OK;
}

// The snapshot's body, the one definition of its layout: the sections that follow the header, in file order, each the
// device buffer it is read from (written to, on load) and its length.  Dense shards with rows hold tiles, scale and
// norm2 up to the header's row capacity; sparse shards with rows hold the device CSR.
struct Section {
    void* dev;
    size_t bytes;
};
struct Sections {
    Section s[6];
    int n_dense = 0, n = 0;  // s[0 .. n_dense) dense, s[n_dense .. n) sparse
    Sections(const hr_index* h, const SnapHeader& hd) {
        if (hd.dim > 0 && hd.n_rows > 0) {
            s[n++] = {h->tiles.p, tile_bytes_for_rows(h, hd.cap_rows)};
            s[n++] = {h->scale.p, (size_t)hd.cap_rows * 4};
            s[n++] = {h->norm2.p, (size_t)hd.cap_rows * 8};
        }
        n_dense = n;
        if (hd.n_sparse > 0) {
            s[n++] = {h->s_indptr.p, (size_t)(hd.n_sparse + 1) * 8};
            s[n++] = {h->s_idx.p, (size_t)hd.nnz * 4};
            s[n++] = {h->s_val.p, (size_t)hd.nnz * 4};
        }
    }
    int64_t bytes() const {
        int64_t t = 0;
        for (int i = 0; i < n; ++i) t += (int64_t)s[i].bytes;
        return t;
    }
};

int save_to(hr_index* h, FILE* f) {
    SnapHeader hd{};
    std::memcpy(hd.magic, kSnapMagic, 8);
    hd.version = 2; hd.dtype = h->dtype; hd.metric = h->metric; hd.KT = h->KT;
    hd.dim = h->dim; hd.sparse_dim = h->sparse_dim; hd.n_rows = h->n_rows;
    hd.cap_rows = h->dim ? round_up(std::max<int64_t>(h->n_rows, 1), kSuperRows) : 0;
    hd.n_sparse = h->n_sparse; hd.nnz = h->nnz_csr; hd.row_offset = h->row_offset;
    hd.max_row_norm = h->max_row_norm; hd.max_sparse_abs = h->max_sparse_abs;
    const Sections body(h, hd);  // the CSR too is read back from the device: the host keeps no copy of it
    hd.file_bytes = (int64_t)sizeof hd + body.bytes();
    if (fwrite(&hd, sizeof hd, 1, f) != 1) return fail(h, HR_EINVAL, "snapshot write failed");
    for (int i = 0; i < body.n; ++i) HR_TRY(stream_out(h, f, body.s[i].dev, body.s[i].bytes));
    return HR_OK;
}

// A handle's error, for a caller that never gets the handle (hr_load destroys it on failure)
int forward_error(const hr_index* h, int rc, const char* prefix = "") {
    return fail(nullptr, rc, "%s%s", prefix, hr_last_error(h));
}
}  // namespace

int hr_save(hr_index* h, const char* path) {
    if (!h || !path) return fail(h, HR_EINVAL, "null argument");
    if (!h->finalized) return fail(h, HR_ESTATE, "hr_save before hr_finalize");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    HIP_TRY(h, hipDeviceSynchronize());
    // written beside the target and renamed once complete: a full disk or a crash leaves the old snapshot intact
    std::string tmp_path;
    try {
        tmp_path = std::string(path) + ".tmp";
    } catch (const std::exception&) {
        return fail(h, HR_ENOMEM, "out of host memory");
    }
    int rc;
    {
        File file;
        file.f = fopen(tmp_path.c_str(), "wb");
        if (!file.f) return fail(h, HR_EINVAL, "cannot open %s for writing", tmp_path.c_str());
        rc = save_to(h, file.f);
        if (rc == HR_OK && fflush(file.f) != 0) rc = fail(h, HR_EINVAL, "snapshot write failed (flush)");
        FILE* f = file.f;
        file.f = nullptr;
        if (fclose(f) != 0 && rc == HR_OK) rc = fail(h, HR_EINVAL, "snapshot write failed (close)");
    }
    if (rc == HR_OK && std::rename(tmp_path.c_str(), path) != 0) rc = fail(h, HR_EINVAL, "cannot move snapshot into place at %s", path);
    if (rc != HR_OK) (void)std::remove(tmp_path.c_str());
    return rc;
}

static int load_impl(const char* path, int device, hr_index** out) {
    File file;
    file.f = fopen(path, "rb");
    if (!file.f) return fail(nullptr, HR_EINVAL, "cannot open %s", path);
    SnapHeader hd{};
    if (fread(&hd, sizeof hd, 1, file.f) != 1 || std::memcmp(hd.magic, kSnapMagic, 8) != 0 || hd.version != 2)
        return fail(nullptr, HR_EINVAL, "%s is not a libhbmrag snapshot (version 2)", path);
    if (hd.n_rows < 0 || hd.n_sparse < 0 || hd.nnz < 0 || hd.cap_rows < hd.n_rows || hd.n_sparse > (1ll << 31) - 64 ||
        hd.nnz > (1ll << 40) || !(hd.max_sparse_abs >= 0.f) || !(hd.max_row_norm >= 0.f) ||
        !std::isfinite(hd.max_row_norm))
        return fail(nullptr, HR_EINVAL, "corrupt snapshot header");
    if (fseek(file.f, 0, SEEK_END) != 0 || (int64_t)ftell(file.f) != hd.file_bytes || fseek(file.f, (long)sizeof hd, SEEK_SET) != 0)
        return fail(nullptr, HR_EINVAL, "snapshot truncated or padded: %s does not hold the %lld bytes its header announces", path,
                    (long long)hd.file_bytes);
    hr_index* h = nullptr;
    HR_TRY(hr_create(device, hd.dim, hd.dtype, hd.metric, hd.sparse_dim, &h));
    struct Guard { hr_index* h; bool keep = false; ~Guard() { if (!keep) hr_destroy(h); } } guard{h};
    if (h->KT != hd.KT) return fail(nullptr, HR_EINVAL, "snapshot tile layout (KT=%d) differs from this build (KT=%d)", hd.KT, h->KT);
    h->row_offset = hd.row_offset;
    DeviceGuard dg(device);
    const bool dense = hd.dim > 0 && hd.n_rows > 0;
    if (dense) {
        if (hd.cap_rows != round_up(hd.n_rows, kSuperRows)) return fail(nullptr, HR_EINVAL, "corrupt snapshot header (row capacity)");
        HR_TRY(hr_reserve(h, hd.cap_rows));
    }
    const Sections body(h, hd);
    for (int i = 0; i < body.n_dense; ++i) {
        const int rc = stream_in(h, file.f, body.s[i].dev, body.s[i].bytes);
        if (rc != HR_OK) return forward_error(h, rc);
    }
    if (dense) {
        h->n_rows = h->n_normed = hd.n_rows;
        h->max_row_norm = hd.max_row_norm;
        unsigned int bits;
        std::memcpy(&bits, &hd.max_row_norm, 4);
        if (hipMemcpy(h->max_norm.p, &bits, 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail(nullptr, HR_EHIP, "snapshot upload failed");
    }
    if (hd.n_sparse > 0) {
        if (hd.sparse_dim <= 0) return fail(nullptr, HR_EINVAL, "corrupt snapshot header (sparse rows without a sparse collection)");
        // the file is not trusted: the CSR goes through the host and the same checks as hr_add_sparse before any kernel
        // indexes with it (the sections name only its lengths here: the device CSR does not exist yet)
        const Section* sp = body.s + body.n_dense;
        std::vector<int64_t> ptr(sp[0].bytes / 8);
        std::vector<int32_t> idx(sp[1].bytes / 4);
        std::vector<float> val(sp[2].bytes / 4);
        const bool ok = fread(ptr.data(), 1, sp[0].bytes, file.f) == sp[0].bytes &&
                        fread(idx.data(), 1, sp[1].bytes, file.f) == sp[1].bytes &&
                        fread(val.data(), 1, sp[2].bytes, file.f) == sp[2].bytes;
        if (!ok || ptr.front() != 0 || ptr.back() != hd.nnz)
            return fail(nullptr, HR_EINVAL, "snapshot truncated or corrupt (sparse section)");
        for (int64_t r = 0; r < hd.n_sparse; ++r)
            if (ptr[r + 1] < ptr[r] || ptr[r + 1] > hd.nnz) return fail(nullptr, HR_EINVAL, "snapshot corrupt (sparse row pointers)");
        const int rc = hr_add_sparse(h, ptr.data(), idx.data(), val.data(), hd.n_sparse);  // validates; recomputes max |weight|
        if (rc != HR_OK) return forward_error(h, rc, "snapshot corrupt (sparse section): ");
    }
    const int rc = hr_finalize(h);
    if (rc != HR_OK) return forward_error(h, rc);
    guard.keep = true;
    *out = h;
    return HR_OK;
}

int hr_load(const char* path, int device, hr_index** out) {
    if (!path || !out) return fail(nullptr, HR_EINVAL, "null argument");
    *out = nullptr;
    try {
        return load_impl(path, device, out);
    } catch (const std::bad_alloc&) {
        return fail(nullptr, HR_ENOMEM, "out of host memory loading snapshot");
    } catch (const std::exception& e) {  // e.g. std::length_error from an absurd size in a damaged header
        return fail(nullptr, HR_EINVAL, "snapshot refused: %s", e.what());
    }
}

int hr_get_info(const hr_index* h, int64_t* dim, int32_t* dtype, int32_t* metric, int64_t* sparse_dim) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (dim) *dim = h->dim;
    if (dtype) *dtype = h->dtype;
    if (metric) *metric = h->metric;
    if (sparse_dim) *sparse_dim = h->sparse_dim;
    return HR_OK;
}

int64_t hr_num_rows(const hr_index* h) { return h ? h->n_rows : 0; }
int64_t hr_num_sparse_rows(const hr_index* h) { return h ? h->n_sparse : 0; }
int64_t hr_device_bytes(const hr_index* h) {
    if (!h) return 0;
    size_t t = 0;
    for (const DevBuf* b : {&h->tiles, &h->scale, &h->norm2, &h->s_indptr, &h->s_idx, &h->s_val, &h->rt_off,
                            &h->range_base, &h->post})
        t += b->cap;
    return (int64_t)t;
}
int64_t hr_dense_scan_bytes(const hr_index* h) {
    if (!h || h->dim == 0) return 0;
    const int64_t dpad = (int64_t)h->KT * 4 * elems_per_chunk(h->dtype);
    return h->n_rows * dpad * (int64_t)elem_size(h->dtype) + h->n_rows * 4;
}

// ---- device-pointer, asynchronous forms -----------------------------------------
static int check_query_nnz(hr_index* h, int max_q_nnz) {
    if (max_q_nnz < 0 || max_q_nnz > HR_MAX_QUERY_NNZ) return fail(h, HR_ELIMIT, "query nnz exceeds HR_MAX_QUERY_NNZ");
    return HR_OK;
}

int hr_search_dense_dev(hr_index* h, const float* d_q, int B, int k, const uint8_t* d_rowmask, int64_t* d_ids,
                        float* d_scores, int32_t* d_flags, void* stream) {
    HR_TRY(check_search_args(h, B, k, true));
    if (!d_q || !d_ids || !d_scores) return fail(h, HR_EINVAL, "null buffer");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (h->n_rows == 0) return fill_empty(h, s, B, k, d_ids, d_scores, d_flags);
    StreamWs ws_held;
    Workspace* ws = ws_for_stream(h, stream, ws_held);
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    return dense_search_enqueue(h, ws, s, d_q, B, k, d_rowmask, {d_ids, d_scores, d_flags}, candidate_groups_for_k(k));
}

int hr_search_dense_range_dev(hr_index* h, const float* d_q, int B, int k, const uint8_t* d_rowmask, const double* d_radius,
                              const double* d_range_filter, int64_t* d_ids, float* d_scores, int32_t* d_flags,
                              void* stream) {
    HR_TRY(check_search_args(h, B, k, true));
    if (!d_q || !d_ids || !d_scores) return fail(h, HR_EINVAL, "null buffer");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (h->n_rows == 0) return fill_empty(h, s, B, k, d_ids, d_scores, d_flags);
    StreamWs ws_held;
    Workspace* ws = ws_for_stream(h, stream, ws_held);
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    const DenseRange rng{d_radius, d_range_filter};
    return dense_search_enqueue(h, ws, s, d_q, B, k, d_rowmask, {d_ids, d_scores, d_flags}, candidate_groups_for_k(k), nullptr,
                                PHASE_ALL, &rng);
}

int hr_search_sparse_dev(hr_index* h, const int64_t* d_q_indptr, const int32_t* d_q_idx, const float* d_q_val, int B,
                         int64_t q_nnz_total, int max_q_nnz, int k, const uint8_t* d_rowmask, int64_t* d_ids,
                         float* d_scores, int32_t* d_flags, void* stream) {
    HR_TRY(check_search_args(h, B, k, false));
    if (!d_q_indptr || !d_ids || !d_scores || (q_nnz_total > 0 && (!d_q_idx || !d_q_val)))
        return fail(h, HR_EINVAL, "null buffer");
    HR_TRY(check_query_nnz(h, max_q_nnz));
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (h->n_sparse == 0) return fill_empty(h, s, B, k, d_ids, d_scores, d_flags);
    StreamWs ws_held;
    Workspace* ws = ws_for_stream(h, stream, ws_held);
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    return sparse_search_enqueue(h, ws, s, d_q_indptr, d_q_idx, d_q_val, B, max_q_nnz, k, d_rowmask,
                                 {d_ids, d_scores, d_flags}, candidate_groups_for_k(k));
}

// The hybrid forms' shared preamble.  buffers_ok: the entry point's own null-buffer rule (those that produce lists need
// somewhere to put them; the finish takes no q_nnz_total to judge the query arrays by).
static int check_hybrid_args(hr_index* h, int B, int k, bool buffers_ok) {
    HR_TRY(check_search_args(h, B, k, true));
    HR_TRY(check_search_args(h, B, k, false));
    return buffers_ok ? HR_OK : fail(h, HR_EINVAL, "null buffer");
}
// [2][B][k] outputs, dense first: the sparse half
static OutLists sparse_half(int B, int k, int64_t* d_ids, float* d_scores, int32_t* d_flags) {
    return {d_ids + (size_t)B * k, d_scores + (size_t)B * k, d_flags ? d_flags + B : nullptr};
}

int hr_search_hybrid_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                         const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k,
                         const uint8_t* d_rowmask, int64_t* d_ids, float* d_scores, int32_t* d_flags, void* stream) {
    HR_TRY(check_hybrid_args(h, B, k, d_q && d_q_indptr && d_ids && d_scores && (q_nnz_total <= 0 || (d_q_idx && d_q_val))));
    HR_TRY(check_query_nnz(h, max_q_nnz));
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    const OutLists so = sparse_half(B, k, d_ids, d_scores, d_flags);
    StreamWs ws_held;
    Workspace* ws = ws_for_stream(h, stream, ws_held);
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    if (!ws->side) {
        HIP_TRY(h, hipStreamCreateWithFlags(&ws->side, hipStreamNonBlocking));
        HIP_TRY(h, hipEventCreateWithFlags(&ws->ev_scan, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&ws->ev_side, hipEventDisableTiming));
        ws->sparse_ws = new (std::nothrow) Workspace();
        if (!ws->sparse_ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    }
    const int C = candidate_groups_for_k(k);
    if (h->n_rows == 0) {
        HR_TRY(fill_empty(h, s, B, k, d_ids, d_scores, d_flags));
        HIP_TRY(h, hipEventRecord(ws->ev_scan, s));
    } else {
        HR_TRY(dense_search_enqueue(h, ws, s, d_q, B, k, d_rowmask, {d_ids, d_scores, d_flags}, C, ws->ev_scan));
    }
    // sparse chain: starts when the dense scan is done, overlaps the dense tail
    HIP_TRY(h, hipStreamWaitEvent(ws->side, ws->ev_scan, 0));
    if (h->n_sparse == 0) {
        HR_TRY(fill_empty(h, ws->side, B, k, so.ids, so.scores, so.flags));
    } else {
        HR_TRY(sparse_search_enqueue(h, ws->sparse_ws, ws->side, d_q_indptr, d_q_idx, d_q_val, B, max_q_nnz, k,
                                     d_rowmask, so, C));
    }
    HIP_TRY(h, hipEventRecord(ws->ev_side, ws->side));
    HIP_TRY(h, hipStreamWaitEvent(s, ws->ev_side, 0));
    return HR_OK;
}

// The two workspaces of a slot of the two-phase forms, locked while one call enqueues
struct SlotWs {
    Workspace *dense = nullptr, *sparse = nullptr;
    std::unique_lock<std::mutex> held;
};
static int lock_slot(hr_index* h, int slot, SlotWs* out) {
    if (slot < 0 || slot >= HR_MAX_SLOTS) return fail(h, HR_EINVAL, "slot %d out of range [0,%d)", slot, HR_MAX_SLOTS);
    {
        std::lock_guard<std::mutex> g(h->pool_mu);
        for (int m = 0; m < 2; ++m)
            if (!h->slot_ws[slot][m]) {
                h->slot_ws[slot][m] = new (std::nothrow) Workspace();
                if (!h->slot_ws[slot][m]) return fail(h, HR_ENOMEM, "workspace allocation failed");
            }
        out->dense = h->slot_ws[slot][0];
        out->sparse = h->slot_ws[slot][1];
    }
    out->held = std::unique_lock<std::mutex>(out->dense->mu);
    return HR_OK;
}

// phases = PHASE_PREP (hr_hybrid_prep_dev) or the scans (+ the prep when the slot was not prepared beforehand)
static int hybrid_scan_phases(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                              const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k,
                              const uint8_t* d_rowmask, int slot, void* stream, bool prep_only) {
    HR_TRY(check_hybrid_args(h, B, k, d_q && d_q_indptr && (q_nnz_total <= 0 || (d_q_idx && d_q_val))));
    HR_TRY(check_query_nnz(h, max_q_nnz));
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    SlotWs w;
    HR_TRY(lock_slot(h, slot, &w));
    hipStream_t s = (hipStream_t)stream;
    const int C = candidate_groups_for_k(k);
    int phases = PHASE_PREP;
    if (!prep_only) {
        phases = h->slot_prepped[slot] ? PHASE_SCAN : (PHASE_PREP | PHASE_SCAN);
        h->slot_prepped[slot] = false;
    }
    if (h->n_rows > 0) HR_TRY(dense_search_enqueue(h, w.dense, s, d_q, B, k, d_rowmask, {}, C, nullptr, phases));
    if (h->n_sparse > 0)
        HR_TRY(sparse_search_enqueue(h, w.sparse, s, d_q_indptr, d_q_idx, d_q_val, B, max_q_nnz, k, d_rowmask, {}, C, phases));
    if (prep_only) h->slot_prepped[slot] = true;
    return HR_OK;
}

int hr_hybrid_prep_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                       const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k, int slot, void* stream) {
    return hybrid_scan_phases(h, d_q, d_q_indptr, d_q_idx, d_q_val, B, q_nnz_total, max_q_nnz, k, nullptr, slot, stream, true);
}

int hr_hybrid_scan_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                       const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k,
                       const uint8_t* d_rowmask, int slot, void* stream) {
    return hybrid_scan_phases(h, d_q, d_q_indptr, d_q_idx, d_q_val, B, q_nnz_total, max_q_nnz, k, d_rowmask, slot, stream, false);
}

// Finish of the slot's scans: both modalities in one finish_enqueue; an empty collection's lists are all padding, and
// the other modality then finishes as a single side.
int hr_hybrid_finish_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                         const float* d_q_val, int B, int max_q_nnz, int k, const uint8_t* d_rowmask, int slot,
                         int64_t* d_ids, float* d_scores, int32_t* d_flags, void* stream) {
    HR_TRY(check_hybrid_args(h, B, k, d_q && d_q_indptr && d_ids && d_scores));
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    SlotWs w;
    HR_TRY(lock_slot(h, slot, &w));
    hipStream_t s = (hipStream_t)stream;
    const int C = candidate_groups_for_k(k);
    const OutLists so = sparse_half(B, k, d_ids, d_scores, d_flags);
    FinishSide f[2];
    int n = 0;
    if (h->n_rows > 0)
        HR_TRY(dense_side(h, w.dense, d_q, B, k, C, d_rowmask, {d_ids, d_scores, d_flags}, &f[n++]));
    else
        HR_TRY(fill_empty(h, s, B, k, d_ids, d_scores, d_flags));
    if (h->n_sparse > 0)
        HR_TRY(sparse_side(h, w.sparse, d_q_indptr, d_q_idx, d_q_val, B, max_q_nnz, k, C, d_rowmask, so, &f[n++]));
    else
        HR_TRY(fill_empty(h, s, B, k, so.ids, so.scores, so.flags));
    return n ? finish_enqueue(h, s, B, f, n) : HR_OK;
}

int hr_fuse_rrf_dev(const int64_t* d_ids_a, int ka, const int64_t* d_ids_b, int kb, const int64_t* d_ids_c, int kc,
                    int B, double wa, double wb, double wc, int rrf_k, int top_k, int64_t* d_out_ids,
                    double* d_out_scores, int32_t* d_out_methods, int32_t* d_n_out, void* stream) {
    if (B <= 0 || ka < 0 || kb < 0 || kc < 0 || top_k <= 0) return fail(nullptr, HR_EINVAL, "bad fuse sizes");
    if (ka > HR_MAX_TOPK || kb > HR_MAX_TOPK || kc > HR_MAX_TOPK)
        return fail(nullptr, HR_ELIMIT, "list longer than HR_MAX_TOPK=%d", HR_MAX_TOPK);
    if ((ka && !d_ids_a) || (kb && !d_ids_b) || (kc && !d_ids_c) || !d_out_ids || !d_out_scores || !d_out_methods || !d_n_out)
        return fail(nullptr, HR_EINVAL, "null buffer");
    hipLaunchKernelGGL(rrf_fuse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids_a, ka, d_ids_b, kb, d_ids_c, kc,
                       wa, wb, wc, rrf_k, top_k, d_out_ids, d_out_scores, d_out_methods, d_n_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "rrf_fuse_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_fuse_scores_dev(const int64_t* d_ids_a, const float* d_sc_a, int ka, int norm_a, const int64_t* d_ids_b,
                       const float* d_sc_b, int kb, int norm_b, const int64_t* d_ids_c, const float* d_sc_c, int kc,
                       int norm_c, int B, double wa, double wb, double wc, const double* d_w_query, int top_k,
                       int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_methods, int32_t* d_n_out, void* stream) {
    if (B <= 0 || ka < 0 || kb < 0 || kc < 0 || top_k <= 0) return fail(nullptr, HR_EINVAL, "bad fuse sizes");
    if (ka > HR_MAX_TOPK || kb > HR_MAX_TOPK || kc > HR_MAX_TOPK)
        return fail(nullptr, HR_ELIMIT, "list longer than HR_MAX_TOPK=%d", HR_MAX_TOPK);
    if ((ka && !d_ids_a) || (kb && !d_ids_b) || (kc && !d_ids_c) || !d_out_ids || !d_out_scores || !d_out_methods || !d_n_out)
        return fail(nullptr, HR_EINVAL, "null buffer");
    if ((ka && !d_sc_a) || (kb && !d_sc_b) || (kc && !d_sc_c)) return fail(nullptr, HR_EINVAL, "null score buffer of a used list");
    const int norm[3] = {norm_a, norm_b, norm_c}, k[3] = {ka, kb, kc};
    for (int m = 0; m < 3; ++m)
        if (k[m] && (norm[m] < HR_NORM_COSINE || norm[m] > HR_NORM_MINMAX_DIST))
            return fail(nullptr, HR_EINVAL, "norm code %d of list %d is not one of HR_NORM_*", norm[m], m);
    ScoreContribution c{{d_sc_a, d_sc_b, d_sc_c}, {norm_a, norm_b, norm_c}};
    hipLaunchKernelGGL(score_fuse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids_a, ka, d_ids_b, kb, d_ids_c, kc,
                       c, wa, wb, wc, d_w_query, top_k, d_out_ids, d_out_scores, d_out_methods, d_n_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "score_fuse_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_fuse_lists_dev(const int64_t* d_ids, const float* d_scores, int n_lists, int k_in, int B, int mode, int rrf_k,
                      const int32_t* norms, const double* weights, const double* d_w_query, int top_k, int64_t* d_out_ids,
                      double* d_out_scores, int32_t* d_out_lists, int32_t* d_n_out, void* stream) {
    if (n_lists < 1 || k_in < 1 || top_k < 1 || B < 0) return fail(nullptr, HR_EINVAL, "bad fuse-lists sizes");
    if (mode != HR_FUSE_RRF && mode != HR_FUSE_WEIGHTED) return fail(nullptr, HR_EINVAL, "mode %d is neither HR_FUSE_RRF nor HR_FUSE_WEIGHTED", mode);
    if (n_lists > HR_MAX_FUSE_LISTS) return fail(nullptr, HR_ELIMIT, "more than HR_MAX_FUSE_LISTS=%d lists", HR_MAX_FUSE_LISTS);
    if (k_in > HR_MAX_TOPK) return fail(nullptr, HR_ELIMIT, "list longer than HR_MAX_TOPK=%d", HR_MAX_TOPK);
    if (top_k > 3 * HR_MAX_TOPK) return fail(nullptr, HR_ELIMIT, "top_k beyond 3 * HR_MAX_TOPK=%d", 3 * HR_MAX_TOPK);
    if (!d_ids || !d_out_ids || !d_out_scores || !d_out_lists || !d_n_out) return fail(nullptr, HR_EINVAL, "null buffer");
    if (!weights && !d_w_query) return fail(nullptr, HR_EINVAL, "neither host weights nor per-query weights");
    const bool weighted = mode == HR_FUSE_WEIGHTED;
    if (weighted && (!d_scores || !norms)) return fail(nullptr, HR_EINVAL, "weighted fusion needs the scores and the norm codes");
    auto off = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
    if (off(d_ids, 8) || off(d_out_ids, 8) || off(d_out_scores, 8) || off(d_w_query, 8) || off(weights, 8) ||
        off(d_scores, 4) || off(norms, 4) || off(d_out_lists, 4) || off(d_n_out, 4))
        return fail(nullptr, HR_EINVAL, "misaligned buffer");
    FuseListsArgs a{};
    a.rrf_k = rrf_k;
    for (int l = 0; l < n_lists; ++l) {
        if (weighted) {
            if (norms[l] < HR_NORM_COSINE || norms[l] > HR_NORM_MINMAX_DIST)
                return fail(nullptr, HR_EINVAL, "norm code %d of list %d is not one of HR_NORM_*", norms[l], l);
            a.norm[l] = norms[l];
        }
        if (weights) {
            if (!std::isfinite(weights[l])) return fail(nullptr, HR_EINVAL, "non-finite weight of list %d", l);
            a.w[l] = weights[l];
        }
    }
    if (B == 0) return HR_OK;
    const FuseListsShape sh = fuse_lists_shape(n_lists, k_in);
    const size_t lds = fuse_lists_lds_bytes(sh);
    const void* kern = weighted ? (const void*)fuse_lists_kernel<true> : (const void*)fuse_lists_kernel<false>;
    if (lds > 48 * 1024) {   // the attribute is per device and idempotent: set on every large launch, it costs no launch
        hipError_t e0 = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fuse_lists_lds_bytes(fuse_lists_shape(HR_MAX_FUSE_LISTS, HR_MAX_TOPK)));
        if (e0 != hipSuccess) return fail(nullptr, HR_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e0));
    }
    if (weighted)
        hipLaunchKernelGGL(fuse_lists_kernel<true>, dim3(B), dim3(256), lds, (hipStream_t)stream, d_ids, d_scores, sh, a,
                           d_w_query, top_k, d_out_ids, d_out_scores, d_out_lists, d_n_out);
    else
        hipLaunchKernelGGL(fuse_lists_kernel<false>, dim3(B), dim3(256), lds, (hipStream_t)stream, d_ids, d_scores, sh, a,
                           d_w_query, top_k, d_out_ids, d_out_scores, d_out_lists, d_n_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "fuse_lists_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

namespace {
int merge_topk_impl(const float* d_scores, const int64_t* d_ids, int n_lists, int64_t score_stride, int64_t id_stride,
                    int B, int k_in, int k_out, int64_t* d_out_ids, float* d_out_scores, void* stream, int asc) {
    if (n_lists <= 0 || B <= 0 || k_in <= 0 || k_out <= 0) return fail(nullptr, HR_EINVAL, "bad merge sizes");
    if (score_stride < (int64_t)B * k_in || id_stride < (int64_t)B * k_in)
        return fail(nullptr, HR_EINVAL, "list stride smaller than one list");
    if (!d_scores || !d_ids || !d_out_ids || !d_out_scores) return fail(nullptr, HR_EINVAL, "null buffer");
    const size_t lds = merge_lds_bytes(n_lists, k_in);
    if (lds <= kMergeLdsMax)
        hipLaunchKernelGGL(merge_topk_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, d_scores, d_ids, n_lists,
                           score_stride, id_stride, k_in, k_out, d_out_ids, d_out_scores, asc);
    else
        hipLaunchKernelGGL(merge_topk_big_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_scores, d_ids, n_lists,
                           score_stride, id_stride, k_in, k_out, d_out_ids, d_out_scores, asc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "merge_topk_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}
}  // namespace

int hr_merge_topk_dev(const float* d_scores, const int64_t* d_ids, int n_lists, int64_t score_stride, int64_t id_stride,
                      int B, int k_in, int k_out, int64_t* d_out_ids, float* d_out_scores, void* stream) {
    return merge_topk_impl(d_scores, d_ids, n_lists, score_stride, id_stride, B, k_in, k_out, d_out_ids, d_out_scores, stream, 0);
}
int hr_merge_topk_asc_dev(const float* d_scores, const int64_t* d_ids, int n_lists, int64_t score_stride, int64_t id_stride,
                          int B, int k_in, int k_out, int64_t* d_out_ids, float* d_out_scores, void* stream) {
    return merge_topk_impl(d_scores, d_ids, n_lists, score_stride, id_stride, B, k_in, k_out, d_out_ids, d_out_scores, stream, 1);
}

int hr_post_lists_dev(const hr_post_args* a, int B, void* stream) {
    if (!a || B <= 0) return fail(nullptr, HR_EINVAL, "bad post-lists arguments");
    if (a->n_lists < 1 || a->top_k <= 0 || a->k_in[0] <= 0) return fail(nullptr, HR_EINVAL, "bad post-lists sizes");
    if (a->asc_mask & ~7) return fail(nullptr, HR_EINVAL, "asc_mask has bits beyond the three modalities");
    if (a->fusion < 0 || a->fusion > 1) return fail(nullptr, HR_EINVAL, "fusion must be 0 (RRF) or 1 (weighted)");
    size_t lds = 0;
    for (int m = 0; m < 3; ++m) {
        if (a->k_in[m] < 0 || a->k_in[m] > HR_MAX_TOPK || a->k_fuse[m] > HR_MAX_TOPK)
            return fail(nullptr, HR_ELIMIT, "list longer than HR_MAX_TOPK=%d", HR_MAX_TOPK);
        if (!a->k_in[m]) continue;
        if (!a->ids[m] || a->k_fuse[m] <= 0) return fail(nullptr, HR_EINVAL, "null list / bad k_fuse of modality %d", m);
        if (a->fusion == 1 && (!a->scores[m] || a->norm[m] < HR_NORM_COSINE || a->norm[m] > HR_NORM_MINMAX_DIST))
            return fail(nullptr, HR_EINVAL, "weighted fusion needs the scores and a HR_NORM_* code of modality %d", m);
        if (a->n_lists == 1) {
            if (a->k_fuse[m] != a->k_in[m]) return fail(nullptr, HR_EINVAL, "k_fuse must equal k_in without a merge");
        } else {
            if (!a->scores[m] || !a->merged_ids[m] || !a->merged_scores[m])
                return fail(nullptr, HR_EINVAL, "null merge buffer of modality %d", m);
            if (a->score_stride < (int64_t)B * a->k_in[m] || a->id_stride < (int64_t)B * a->k_in[m])
                return fail(nullptr, HR_EINVAL, "list stride smaller than one list");
            lds = std::max(lds, merge_lds_bytes(a->n_lists, a->k_in[m]));
        }
    }
    if (lds > kMergeLdsMax) return fail(nullptr, HR_ELIMIT, "merge of %d lists does not fit LDS; use hr_merge_topk_dev", a->n_lists);
    if (!a->fused_ids || !a->fused_scores || !a->fused_methods || !a->fused_n) return fail(nullptr, HR_EINVAL, "null fusion buffer");
    if (a->rerank && (a->k_out <= 0 || a->top_k > HR_MAX_TOPK || !a->rr_ids || !a->rr_scores || !a->rr_orig))
        return fail(nullptr, HR_EINVAL, "bad rerank buffers");
    if (a->agg_flags && a->n_lists > 1 && (!a->flags || a->n_flag_rows <= 0 || a->flag_stride < a->n_flag_rows))
        return fail(nullptr, HR_EINVAL, "bad flag buffers");
    PostArgs pa;
    pa.a = *a;
    if (a->fusion == 1)
        hipLaunchKernelGGL(post_lists_kernel<true>, dim3(B), dim3(256), lds, (hipStream_t)stream, pa);
    else
        hipLaunchKernelGGL(post_lists_kernel<false>, dim3(B), dim3(256), lds, (hipStream_t)stream, pa);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "post_lists_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_filter_eval_dev(const hr_filter_term* terms, int n_terms, int64_t n_rows, const uint8_t* d_deleted, uint8_t* d_mask,
                       uint8_t* d_undecided, int32_t* d_counts, void* stream) {
    if (n_terms < 0 || n_terms > kFilterMaxTerms) return fail(nullptr, HR_ELIMIT, "a filter expression may hold up to %d terms", kFilterMaxTerms);
    if (n_rows < 0 || (n_terms > 0 && !terms) || !d_mask || !d_undecided || !d_counts) return fail(nullptr, HR_EINVAL, "bad filter arguments");
    if (((uintptr_t)d_mask | (uintptr_t)d_undecided) & 7) return fail(nullptr, HR_EINVAL, "mask buffers must be 8-byte aligned");
    FilterArgs a{};
    for (int i = 0; i < n_terms; ++i) {
        if (terms[i].kind < HR_COL_I64 || terms[i].kind > HR_COL_STR16 || terms[i].op < HR_OP_EQ || terms[i].op > HR_OP_GE || !terms[i].col)
            return fail(nullptr, HR_EINVAL, "bad filter term %d", i);
        a.t[i] = terms[i];
    }
    a.n_terms = n_terms;
    a.n_rows = n_rows;
    a.deleted = d_deleted;
    a.mask = (unsigned long long*)d_mask;
    a.undecided = (unsigned long long*)d_undecided;
    a.counts = d_counts;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_counts, 0, 8, s);
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    if (n_rows == 0) return HR_OK;
    const int64_t n_words = (n_rows + 63) / 64;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_words + 3) / 4, 4096));
    hipLaunchKernelGGL(filter_eval_kernel, dim3(blocks), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "filter_eval_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_filter_eval_expr_dev(const hr_filter_leaf* leaves, int n_leaves, const int32_t* program, int n_program, int64_t n_rows,
                            const uint8_t* d_deleted, uint8_t* d_mask, uint8_t* d_undecided, int32_t* d_counts, void* stream) {
    if (n_leaves < 0 || n_leaves > kFilterMaxTerms) return fail(nullptr, HR_ELIMIT, "a filter expression may hold up to %d terms", kFilterMaxTerms);
    if (n_program < 0 || n_program > kFilterMaxProgram)
        return fail(nullptr, HR_ELIMIT, "a filter program may hold up to %d codes", kFilterMaxProgram);
    if (n_rows < 0 || n_leaves == 0 || n_program == 0 || !leaves || !program || !d_mask || !d_undecided || !d_counts)
        return fail(nullptr, HR_EINVAL, "bad filter arguments");
    if (((uintptr_t)d_mask | (uintptr_t)d_undecided) & 7) return fail(nullptr, HR_EINVAL, "mask buffers must be 8-byte aligned");
    FilterExprArgs a{};
    size_t set_bytes = 0;
    bool has_match = false;   // a keyword leaf: the launch takes the kernel variant that carries the wave-cooperative leaf
    for (int i = 0; i < n_leaves; ++i) {
        const hr_filter_term& t = leaves[i].term;
        if ((t.kind == HR_COL_TOKENS) != (t.op == HR_OP_MATCH))   // the keyword leaf's two constants come together or not at all
            return fail(nullptr, HR_EINVAL, "bad filter term %d", i);
        if (t.op == HR_OP_MATCH) {
            const int64_t tok_rows = (int64_t)t.key[1];
            if (!t.col || ((uintptr_t)t.col & 7) || tok_rows < 0 || (t.key[0] & 3) || (t.key[0] == 0 && tok_rows > 0) || t.ival < 1 ||
                leaves[i].n_set < 0 || (leaves[i].set == nullptr) != (leaves[i].n_set == 0) || ((uintptr_t)leaves[i].set & 3))
                return fail(nullptr, HR_EINVAL, "bad filter term %d (keyword match: word sets, minimum_should_match or set)", i);
            if ((size_t)leaves[i].n_set > kFilterMaxSetBytes / 4) return fail(nullptr, HR_ELIMIT, "the sets of a filter expression may hold up to %d bytes", kFilterMaxSetBytes);
            a.t[i] = t;
            a.set[i] = leaves[i].set;
            a.n_set[i] = leaves[i].n_set;
            a.set_off[i] = (int32_t)set_bytes;
            set_bytes += ((size_t)leaves[i].n_set * 4 + 15) & ~(size_t)15;
            if (set_bytes > (size_t)kFilterMaxSetBytes)
                return fail(nullptr, HR_ELIMIT, "the sets of a filter expression may hold up to %d bytes", kFilterMaxSetBytes);
            has_match = true;
            continue;
        }
        if (t.kind < HR_COL_I64 || t.kind > HR_COL_STR16 || t.op < HR_OP_EQ || t.op > HR_OP_IN || !t.col)
            return fail(nullptr, HR_EINVAL, "bad filter term %d", i);
        a.t[i] = t;
        if (t.op != HR_OP_IN) continue;
        const size_t member = t.kind == HR_COL_F32 ? 4 : t.kind == HR_COL_I64 ? 8 : 16, align = member == 4 ? 4 : 8;
        if (t.kind == HR_COL_I64_VS_F64 || leaves[i].n_set < 0 || (leaves[i].set == nullptr) != (leaves[i].n_set == 0) ||
            ((uintptr_t)leaves[i].set & (align - 1)))
            return fail(nullptr, HR_EINVAL, "bad filter term %d (membership: kind, set pointer or set size)", i);
        if ((size_t)leaves[i].n_set > kFilterMaxSetBytes / member) return fail(nullptr, HR_ELIMIT, "the sets of a filter expression may hold up to %d bytes", kFilterMaxSetBytes);
        a.set[i] = leaves[i].set;
        a.n_set[i] = leaves[i].n_set;
        a.set_off[i] = (int32_t)set_bytes;
        set_bytes += ((size_t)leaves[i].n_set * member + 15) & ~(size_t)15;
        if (set_bytes > (size_t)kFilterMaxSetBytes)
            return fail(nullptr, HR_ELIMIT, "the sets of a filter expression may hold up to %d bytes", kFilterMaxSetBytes);
    }
    int depth = 0;
    for (int pc = 0; pc < n_program; ++pc) {
        const int32_t code = program[pc];
        if (code >= 0) {
            if (code >= n_leaves) return fail(nullptr, HR_EINVAL, "filter program: code %d names leaf %d of %d", pc, code, n_leaves);
            if (++depth > kFilterMaxDepth) return fail(nullptr, HR_EINVAL, "filter program: deeper than %d at code %d", kFilterMaxDepth, pc);
        } else if (code == HR_FILTER_AND || code == HR_FILTER_OR) {
            if (depth < 2) return fail(nullptr, HR_EINVAL, "filter program: code %d pops from an empty stack", pc);
            --depth;
        } else if (code == HR_FILTER_NOT) {
            if (depth < 1) return fail(nullptr, HR_EINVAL, "filter program: code %d pops from an empty stack", pc);
        } else {
            return fail(nullptr, HR_EINVAL, "filter program: unknown code %d at %d", code, pc);
        }
        a.program[pc] = (int8_t)code;
    }
    if (depth != 1) return fail(nullptr, HR_EINVAL, "filter program: %d values left at the end, not 1", depth);
    a.n_leaves = n_leaves;
    a.n_program = n_program;
    a.n_rows = n_rows;
    a.deleted = d_deleted;
    a.mask = (unsigned long long*)d_mask;
    a.undecided = (unsigned long long*)d_undecided;
    a.counts = d_counts;
    hipStream_t s = (hipStream_t)stream;
    static bool attr_set = false;  // benign race: the attribute is idempotent
    if (!attr_set) {
        hipError_t e0 = hipFuncSetAttribute((const void*)filter_expr_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kFilterMaxSetBytes);
        if (e0 == hipSuccess)
            e0 = hipFuncSetAttribute((const void*)filter_expr_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kFilterMaxSetBytes);
        if (e0 != hipSuccess) return fail(nullptr, HR_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e0));
        attr_set = true;
    }
    hipError_t e = hipMemsetAsync(d_counts, 0, 8, s);
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    if (n_rows == 0) return HR_OK;
    const int64_t n_words = (n_rows + 63) / 64;
    // every block stages the sets before its first row: past a few KiB of them, fewer blocks with more trips each (two
    // blocks of 64 KiB fit a CU: 1024 blocks are two rounds of the device) stage less than the column read costs
    const int64_t cap = set_bytes > 4096 ? 1024 : 4096;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_words + 3) / 4, cap));
    if (has_match) hipLaunchKernelGGL(filter_expr_kernel<true>, dim3(blocks), dim3(256), set_bytes, s, a);
    else hipLaunchKernelGGL(filter_expr_kernel<false>, dim3(blocks), dim3(256), set_bytes, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "filter_expr_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_bm25_encode_dev(const uint8_t* d_text, const int64_t* d_off, int n_docs, int sparse_dim, double k1, double b,
                       double avgdl, int cap, int32_t* d_idx, float* d_val, int32_t* d_nnz, int32_t* d_flags, void* stream) {
    if (n_docs < 0 || !d_off || !d_nnz || !d_flags || (n_docs > 0 && (!d_text || !d_idx || !d_val)))
        return fail(nullptr, HR_EINVAL, "bad bm25 arguments");
    if (sparse_dim < 1 || sparse_dim > kBm25MaxDim) return fail(nullptr, HR_ELIMIT, "sparse_dim must be 1..%d for the device encoder", kBm25MaxDim);
    if (cap < 1 || !(avgdl > 0.0) || !(k1 >= 0.0) || !(b >= 0.0 && b <= 1.0)) return fail(nullptr, HR_EINVAL, "bad bm25 parameters");
    if (n_docs == 0) return HR_OK;
    Bm25Args a{};
    a.text = d_text; a.off = d_off; a.n_docs = n_docs; a.sparse_dim = sparse_dim; a.cap = cap;
    a.k1 = k1; a.b = b; a.avgdl = avgdl;
    a.idx = d_idx; a.val = d_val; a.nnz = d_nnz; a.flags = d_flags;
    const size_t lds = (size_t)((sparse_dim + 1) / 2) * 4;
    static bool attr_set = false;  // benign race: the attribute is idempotent
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)bm25_encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (kBm25MaxDim / 2) * 4);
        if (e != hipSuccess) return fail(nullptr, HR_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(bm25_encode_kernel, dim3((unsigned)n_docs), dim3(kBm25Threads), lds, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "bm25_encode_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_hash_tokenize_dev(const uint8_t* d_text, const int64_t* d_off, int n, int max_len, int vocab, int64_t* d_ids,
                         int32_t* d_lens, int32_t* d_flags, void* stream) {
    if (n < 0 || !d_off || !d_lens || !d_flags || (n > 0 && (!d_text || !d_ids))) return fail(nullptr, HR_EINVAL, "bad tokenizer arguments");
    if (max_len < 3 || vocab <= 1000) return fail(nullptr, HR_EINVAL, "max_len must be >= 3 and the vocabulary larger than 1000");
    if (n == 0) return HR_OK;
    TokArgs a{};
    a.text = d_text; a.off = d_off; a.n = n; a.max_len = max_len; a.vocab = vocab;
    a.ids = d_ids; a.lens = d_lens; a.flags = d_flags;
    hipLaunchKernelGGL(hash_tokenize_kernel, dim3((unsigned)n), dim3(kTokThreads), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "hash_tokenize_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_stream_create(int device, int priority, const uint32_t* cu_mask, int n_words, void** out_stream) {
    if (!out_stream || n_words < 0 || (n_words > 0 && !cu_mask)) return fail(nullptr, HR_EINVAL, "bad stream arguments");
    *out_stream = nullptr;
    DeviceGuard dg(device);
    hipStream_t s = nullptr;
    hipError_t e;
    if (n_words > 0) {
        // (a masked stream takes the default priority: HIP has no entry point that sets both)
        e = hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, cu_mask);
    } else {
        int lo = 0, hi = 0;  // lo = numerically greatest = lowest priority
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, std::max(hi, std::min(lo, priority)));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(nullptr, HR_EHIP, "stream creation failed: %s", hipGetErrorString(e));
    }
    *out_stream = (void*)s;
    return HR_OK;
}

int hr_stream_destroy(int device, void* stream) {
    if (!stream) return HR_OK;
    DeviceGuard dg(device);
    hipError_t e = hipStreamDestroy((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "hipStreamDestroy: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_set_scan_cus(hr_index* h, int n_cus) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (n_cus < 0) return fail(h, HR_EINVAL, "n_cus must be >= 0");
    h->scan_cus = n_cus;
    return HR_OK;
}

int hr_debug_option(hr_index* h, int key, int value) {
    switch (key) {
        case HR_DEBUG_FINISH_MODE:
            if (value < 0 || value > 2) return fail(h, HR_EINVAL, "finish mode must be 0, 1 or 2");
            g_finish_mode = value;
            return HR_OK;
        case HR_DEBUG_DENSE_KERNELS:
            if (value < 0 || value > 31) return fail(h, HR_EINVAL, "dense kernel mask must be 0..31");
            g_dense_kernels = value;
            return HR_OK;
        case HR_DEBUG_SPARSE_RPB:
            if (value < 0 || value > 64) return fail(h, HR_EINVAL, "ranges per block must be 0..64");
            g_sparse_rpb = value;
            return HR_OK;
        case HR_DEBUG_GROUP_ROWS:
            if (value != 0 && value != 16 && value != 64) return fail(h, HR_EINVAL, "group rows must be 0, 16 or 64");
            g_group_rows = value;
            return HR_OK;
        case HR_DEBUG_NO_TRIM:
            g_no_trim = value != 0;
            return HR_OK;
        case HR_DEBUG_NO_RANGE_CLAMP:
            g_no_range_clamp = value != 0;
            return HR_OK;
        case HR_DEBUG_MAXSIM_SCAN_BLOCKS:
            if (value < 0 || value > 65535) return fail(h, HR_EINVAL, "maxsim scan blocks must be 0..65535");
            g_maxsim_scan_blocks = value;
            return HR_OK;
        case HR_DEBUG_FAIL_NEXT_BUILD:
            if (!h) return fail(nullptr, HR_EINVAL, "null handle");
            h->fault_inject = value ? 1 : 0;
            return HR_OK;
        default:
            return fail(h, HR_EINVAL, "unknown debug option %d", key);
    }
}

int hr_rerank_linear_dev(const int64_t* d_ids, const double* d_scores, const int32_t* d_methods, const int32_t* d_n,
                         const double* d_recency, int B, int k_in, double base_w, double method_bonus,
                         double recency_w, int k_out, int64_t* d_out_ids, double* d_out_scores, double* d_out_orig,
                         void* stream) {
    if (B <= 0 || k_in <= 0 || k_out <= 0) return fail(nullptr, HR_EINVAL, "bad rerank sizes");
    if (k_in > HR_MAX_TOPK) return fail(nullptr, HR_ELIMIT, "k_in exceeds HR_MAX_TOPK=%d", HR_MAX_TOPK);
    if (!d_ids || !d_scores || !d_methods || !d_n || !d_out_ids || !d_out_scores || !d_out_orig)
        return fail(nullptr, HR_EINVAL, "null buffer");
    hipLaunchKernelGGL(rerank_linear_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids, d_scores, d_methods, d_n,
                       d_recency, k_in, base_w, method_bonus, recency_w, k_out, d_out_ids, d_out_scores, d_out_orig);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "rerank_linear_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_mmr_select_dev(const int64_t* d_ids, const double* d_scores, const int32_t* d_n, int B, int k_in,
                      const int64_t* d_tok_indptr, const int32_t* d_tok, int64_t tok_rows, int64_t first_row,
                      const double* d_lambda, int k_out, int32_t* d_out_pos, int32_t* d_out_n, void* stream) {
    if (B <= 0 || k_in <= 0 || k_out <= 0 || k_out > k_in || tok_rows < 0) return fail(nullptr, HR_EINVAL, "bad mmr sizes");
    if (k_in > kFuseMax) return fail(nullptr, HR_ELIMIT, "k_in exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if (!d_ids || !d_scores || !d_n || !d_lambda || !d_out_pos || !d_out_n) return fail(nullptr, HR_EINVAL, "null buffer");
    if (tok_rows > 0 ? (!d_tok_indptr || !d_tok) : (d_tok_indptr || d_tok))   // a column without rows has no arrays, and only it
        return fail(nullptr, HR_EINVAL, "token arrays must be given exactly when tok_rows > 0");
    hipLaunchKernelGGL(mmr_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids, d_scores, d_n, k_in, d_tok_indptr,
                       d_tok, tok_rows, first_row, d_lambda, k_out, d_out_pos, d_out_n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "mmr_select_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_group_select_dev(const int64_t* d_ids, const int32_t* d_n, int B, int k_in, const int64_t* d_keys, int64_t key_rows,
                        int64_t first_row, int k_out, int32_t* d_out_pos, int64_t* d_out_keys, int32_t* d_out_n, int32_t* d_flags,
                        void* stream) {
    if (B < 0 || k_in <= 0 || k_out <= 0 || k_out > k_in || key_rows < 0 || first_row < 0) return fail(nullptr, HR_EINVAL, "bad group sizes");
    if (k_in > kFuseMax) return fail(nullptr, HR_ELIMIT, "k_in exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if (B == 0) return HR_OK;
    if (!d_ids || !d_out_pos || !d_out_n) return fail(nullptr, HR_EINVAL, "null buffer");
    if (key_rows > 0 && !d_keys) return fail(nullptr, HR_EINVAL, "key_rows > 0 needs the key column");
    hipLaunchKernelGGL(group_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids, d_n, k_in, d_keys, key_rows, first_row,
                       k_out, d_out_pos, d_out_keys, d_out_n, d_flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "group_select_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_decay_rerank_dev(const int64_t* d_ids, const void* d_scores, int score_is_f64, const int32_t* d_n, int B, int k_in,
                        const void* d_col, int col_kind, int64_t col_rows, int64_t first_row, const hr_decay_query* d_params,
                        int norm, int k_out, int32_t* d_out_pos, int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_n,
                        void* stream) {
    if (B < 0 || k_in <= 0 || k_out <= 0 || k_out > k_in || col_rows < 0 || first_row < 0) return fail(nullptr, HR_EINVAL, "bad decay sizes");
    if (k_in > kFuseMax) return fail(nullptr, HR_ELIMIT, "k_in exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if (norm < HR_NORM_NONE || norm > HR_NORM_MINMAX_DIST) return fail(nullptr, HR_EINVAL, "bad norm code %d", norm);
    if (col_kind != HR_COL_I64 && col_kind != HR_COL_F32 && col_kind != HR_COL_F64) return fail(nullptr, HR_EINVAL, "bad column kind %d", col_kind);
    if (B == 0) return HR_OK;
    if (!d_ids || !d_scores || !d_params || !d_out_pos || !d_out_ids || !d_out_scores || !d_out_n) return fail(nullptr, HR_EINVAL, "null buffer");
    if (col_rows > 0 && !d_col) return fail(nullptr, HR_EINVAL, "col_rows > 0 needs the column");
    hipLaunchKernelGGL(decay_rerank_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids, d_scores, score_is_f64, d_n, k_in, d_col,
                       col_kind, col_rows, first_row, d_params, norm, k_out, d_out_pos, d_out_ids, d_out_scores, d_out_n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "decay_rerank_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_boost_rerank_dev(const int64_t* d_ids, const void* d_scores, int score_is_f64, const int32_t* d_n, int B, int k_in,
                        const hr_boost_func* d_funcs, int n_funcs, int64_t first_row, int function_mode, int boost_mode, int norm,
                        int ascending, int k_out, int32_t* d_out_pos, int64_t* d_out_ids, double* d_out_scores,
                        int32_t* d_out_matched, int32_t* d_out_n, void* stream) {
    if (B < 0 || k_in <= 0 || k_out <= 0 || k_out > k_in || n_funcs <= 0 || first_row < 0) return fail(nullptr, HR_EINVAL, "bad boost sizes");
    if (k_in > kFuseMax) return fail(nullptr, HR_ELIMIT, "k_in exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if (n_funcs > HR_MAX_BOOST_FUNCS) return fail(nullptr, HR_ELIMIT, "n_funcs exceeds HR_MAX_BOOST_FUNCS = %d", HR_MAX_BOOST_FUNCS);
    if (norm < HR_NORM_NONE || norm > HR_NORM_MINMAX_DIST) return fail(nullptr, HR_EINVAL, "bad norm code %d", norm);
    if (function_mode < HR_BOOST_MULTIPLY || function_mode > HR_BOOST_SUM || boost_mode < HR_BOOST_MULTIPLY || boost_mode > HR_BOOST_SUM)
        return fail(nullptr, HR_EINVAL, "bad boost modes %d / %d", function_mode, boost_mode);
    if (B == 0) return HR_OK;
    if (!d_ids || !d_scores || !d_funcs || !d_out_pos || !d_out_ids || !d_out_scores || !d_out_matched || !d_out_n)
        return fail(nullptr, HR_EINVAL, "null buffer");
    hipLaunchKernelGGL(boost_rerank_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids, d_scores, score_is_f64, d_n, k_in, d_funcs,
                       n_funcs, first_row, function_mode, boost_mode, norm, ascending ? 1 : 0, k_out, d_out_pos, d_out_ids, d_out_scores,
                       d_out_matched, d_out_n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "boost_rerank_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_maxsim_rerank_dev(const int64_t* d_ids, const int32_t* d_n, int B, int k_in, const void* d_qtok, const int32_t* d_qn, int tq_stride,
                         int dim, const int64_t* d_indptr, const void* d_tok, int64_t tok_rows, int64_t first_row, int k_out,
                         int32_t* d_out_pos, int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_n, void* stream) {
    if (B < 0 || k_in <= 0 || k_out <= 0 || k_out > k_in || tq_stride <= 0 || tok_rows < 0 || first_row < 0)
        return fail(nullptr, HR_EINVAL, "bad maxsim sizes");
    if (k_in > kFuseMax) return fail(nullptr, HR_ELIMIT, "k_in exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if (tq_stride > HR_MAX_QUERY_TOKENS) return fail(nullptr, HR_ELIMIT, "tq_stride exceeds HR_MAX_QUERY_TOKENS = %d", HR_MAX_QUERY_TOKENS);
    if (dim > HR_MAX_TOKEN_DIM) return fail(nullptr, HR_ELIMIT, "token dim exceeds %d", HR_MAX_TOKEN_DIM);
    if (dim < 8 || dim % 8 != 0) return fail(nullptr, HR_EINVAL, "token dim must be a multiple of 8, at least 8 (got %d)", dim);
    if (B == 0) return HR_OK;
    if (!d_ids || !d_qtok || !d_qn || !d_out_pos || !d_out_ids || !d_out_scores || !d_out_n) return fail(nullptr, HR_EINVAL, "null buffer");
    if (tok_rows > 0 && (!d_indptr || !d_tok)) return fail(nullptr, HR_EINVAL, "tok_rows > 0 needs the token store");
    if (((uintptr_t)d_qtok | (uintptr_t)d_tok) & 15) return fail(nullptr, HR_EINVAL, "token buffers must be 16-byte aligned");
    const size_t lds = maxsim_lds_bytes(tq_stride, dim, k_in);
    if (lds > 48 * 1024) {   // the attribute is per device and idempotent: set on every large launch, it costs no launch
        hipError_t e0 = hipFuncSetAttribute((const void*)maxsim_rerank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)maxsim_lds_bytes(HR_MAX_QUERY_TOKENS, HR_MAX_TOKEN_DIM, kFuseMax));
        if (e0 != hipSuccess) return fail(nullptr, HR_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e0));
    }
    hipLaunchKernelGGL(maxsim_rerank_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, d_ids, d_n, k_in, (const chunk_t*)d_qtok, d_qn,
                       tq_stride, dim, d_indptr, (const chunk_t*)d_tok, tok_rows, first_row, k_out, d_out_pos, d_out_ids, d_out_scores,
                       d_out_n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "maxsim_rerank_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_maxsim_scan_dev(const void* d_qtok, const int32_t* d_qn, int B, int tq_stride, int dim, const int64_t* d_indptr, const void* d_tok,
                       int64_t tok_rows, int64_t n_rows, const uint8_t* d_rowmask, float* d_scores, int32_t* d_rows, void* stream) {
    if (B < 0 || tq_stride <= 0 || tok_rows < 0 || n_rows < 0) return fail(nullptr, HR_EINVAL, "bad maxsim scan sizes");
    if (tq_stride > HR_MAX_QUERY_TOKENS) return fail(nullptr, HR_ELIMIT, "tq_stride exceeds HR_MAX_QUERY_TOKENS = %d", HR_MAX_QUERY_TOKENS);
    if (dim > HR_MAX_TOKEN_DIM) return fail(nullptr, HR_ELIMIT, "token dim exceeds %d", HR_MAX_TOKEN_DIM);
    if (n_rows > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "n_rows exceeds the int32 row range");
    if (B > 65535) return fail(nullptr, HR_ELIMIT, "batch size %d exceeds one grid (65535)", B);
    if (dim < 8 || dim % 8 != 0) return fail(nullptr, HR_EINVAL, "token dim must be a multiple of 8, at least 8 (got %d)", dim);
    if (B == 0 || n_rows == 0) return HR_OK;
    if (!d_qtok || !d_qn || !d_scores || !d_rows) return fail(nullptr, HR_EINVAL, "null buffer");
    if (tok_rows > 0 && (!d_indptr || !d_tok)) return fail(nullptr, HR_EINVAL, "tok_rows > 0 needs the token store");
    if (((uintptr_t)d_qtok | (uintptr_t)d_tok) & 15) return fail(nullptr, HR_EINVAL, "token buffers must be 16-byte aligned");
    // Blocks per query: about eight blocks per compute unit over the whole batch, so that one query still fills the chip;
    // rows per wave and range: as many as keep that many blocks busy, 8 .. 64.  More ranges than blocks are walked in turn.
    const int64_t want = g_maxsim_scan_blocks > 0 ? g_maxsim_scan_blocks : std::max(1, 2048 / B);
    const int rpw = (int)std::min<int64_t>(kMaxSimScanLanes, std::max<int64_t>(8, (n_rows + want * kMaxSimWaves - 1) / (want * kMaxSimWaves)));
    const int64_t n_ranges = (n_rows + (int64_t)rpw * kMaxSimWaves - 1) / ((int64_t)rpw * kMaxSimWaves);
    const unsigned blocks = (unsigned)std::min<int64_t>(n_ranges, want);
    const size_t lds = maxsim_scan_lds_bytes(tq_stride, dim);
    if (lds > 48 * 1024) {   // per device and idempotent, as for the rerank
        hipError_t e0 = hipFuncSetAttribute((const void*)maxsim_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)maxsim_scan_lds_bytes(HR_MAX_QUERY_TOKENS, HR_MAX_TOKEN_DIM));
        if (e0 != hipSuccess) return fail(nullptr, HR_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e0));
    }
    hipLaunchKernelGGL(maxsim_scan_kernel, dim3(blocks, B), dim3(256), lds, (hipStream_t)stream, (const chunk_t*)d_qtok, d_qn, tq_stride, dim,
                       d_indptr, (const chunk_t*)d_tok, tok_rows, n_rows, d_rowmask, rpw, d_scores, d_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "maxsim_scan_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_group_select_n_dev(const int64_t* d_ids, const int32_t* d_n, int B, int k_in, const int64_t* d_keys, int64_t key_rows,
                          int64_t first_row, int k_out, int group_size, int32_t* d_out_pos, int64_t* d_out_keys, int32_t* d_out_cnt,
                          int32_t* d_out_n, int32_t* d_flags, void* stream) {
    if (B < 0 || k_in <= 0 || k_out <= 0 || k_out > k_in || group_size <= 0 || key_rows < 0 || first_row < 0)
        return fail(nullptr, HR_EINVAL, "bad group sizes");
    if (k_in > kFuseMax) return fail(nullptr, HR_ELIMIT, "k_in exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if ((int64_t)k_out * group_size > kFuseMax) return fail(nullptr, HR_ELIMIT, "k_out * group_size exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if (B == 0) return HR_OK;
    if (!d_ids || !d_out_pos || !d_out_cnt || !d_out_n) return fail(nullptr, HR_EINVAL, "null buffer");
    if (key_rows > 0 && !d_keys) return fail(nullptr, HR_EINVAL, "key_rows > 0 needs the key column");
    hipLaunchKernelGGL(group_select_n_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d_ids, d_n, k_in, d_keys, key_rows,
                       first_row, k_out, group_size, d_out_pos, d_out_keys, d_out_cnt, d_out_n, d_flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "group_select_n_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

// hr_mask_drop_groups_dev (keep = false) and hr_mask_keep_groups_dev (keep = true): one kernel, the sense compiled in.
static int mask_groups(bool keep, const uint8_t* d_mask_in, uint8_t* d_mask_out, int64_t n_rows, const int64_t* d_keys,
                       const int64_t* d_set, int n_set, void* stream) {
    const char* what = keep ? "n_keep" : "n_drop";
    if (n_rows < 0 || n_set < 0) return fail(nullptr, HR_EINVAL, "bad group mask sizes");
    if (n_set > kFuseMax) return fail(nullptr, HR_ELIMIT, "%s exceeds 3 * HR_MAX_TOPK = %d", what, kFuseMax);
    if (n_rows == 0) return HR_OK;
    if (!d_mask_out || !d_keys || (n_set > 0 && !d_set)) return fail(nullptr, HR_EINVAL, "null buffer");
    if (((uintptr_t)d_mask_in | (uintptr_t)d_mask_out) & 7) return fail(nullptr, HR_EINVAL, "mask buffers must be 8-byte aligned");
    const int64_t n_words = (n_rows + 63) / 64;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_words + 3) / 4, 1024));
    hipLaunchKernelGGL(keep ? mask_groups_kernel<true> : mask_groups_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)d_mask_in, (unsigned long long*)d_mask_out, n_rows, d_keys, d_set, n_set);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "mask_groups_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_mask_drop_groups_dev(const uint8_t* d_mask_in, uint8_t* d_mask_out, int64_t n_rows, const int64_t* d_keys,
                            const int64_t* d_drop, int n_drop, void* stream) {
    return mask_groups(false, d_mask_in, d_mask_out, n_rows, d_keys, d_drop, n_drop, stream);
}

int hr_mask_keep_groups_dev(const uint8_t* d_mask_in, uint8_t* d_mask_out, int64_t n_rows, const int64_t* d_keys,
                            const int64_t* d_keep, int n_keep, void* stream) {
    return mask_groups(true, d_mask_in, d_mask_out, n_rows, d_keys, d_keep, n_keep, stream);
}

// ---- read path (query.h) -----------------------------------------------------------------------------------------------
size_t hr_mask_rows_scratch_bytes(int64_t n_rows) {
    if (n_rows < 0) return 0;
    const int64_t n_words = (n_rows + 63) / 64;
    const int64_t nb = (n_words + kCompactBlock - 1) / kCompactBlock;
    return (size_t)(std::max<int64_t>(nb, 1) + 1) * 8;  // the blocks' prefix, then the total
}

int hr_mask_rows_dev(const uint8_t* d_mask, int64_t n_rows, int64_t first_row, int64_t offset, int64_t limit, int64_t* d_rows,
                     int64_t* d_counts, void* d_scratch, void* stream) {
    constexpr int64_t kMax = 1ll << 62;
    if (n_rows < 0 || offset < 0 || limit < 0) return fail(nullptr, HR_EINVAL, "n_rows, offset and limit must be >= 0");
    if (n_rows >= kMax || offset >= kMax || limit >= kMax) return fail(nullptr, HR_EINVAL, "n_rows, offset and limit must be below 2^62");
    if (!d_counts || (!d_rows && limit > 0)) return fail(nullptr, HR_EINVAL, "null buffer");
    if ((uintptr_t)d_mask & 7) return fail(nullptr, HR_EINVAL, "the mask must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (!d_mask || n_rows == 0) {
        const int64_t n_out = n_rows > offset ? std::min(n_rows - offset, limit) : 0;
        const int64_t blocks = std::max<int64_t>(1, (n_out + 255) / 256);
        if (blocks > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "page too large");
        hipLaunchKernelGGL(mask_rows_all_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n_rows, first_row, offset, limit, d_rows, d_counts);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(nullptr, HR_EHIP, "mask_rows_all_kernel: %s", hipGetErrorString(e));
        return HR_OK;
    }
    if (!d_scratch || ((uintptr_t)d_scratch & 7)) return fail(nullptr, HR_EINVAL, "scratch of hr_mask_rows_scratch_bytes bytes, 8-byte aligned, is required");
    const int64_t n_words = (n_rows + 63) / 64;
    const int64_t nb = (n_words + kCompactBlock - 1) / kCompactBlock;
    if (nb > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "too many rows");
    unsigned long long* block_off = (unsigned long long*)d_scratch;
    unsigned long long* total = block_off + nb;
    const unsigned long long* mask = (const unsigned long long*)d_mask;
    hipLaunchKernelGGL((compact_block_sums_kernel<KeepCount>), dim3((unsigned)nb), dim3(kCompactBlock), 0, s, KeepCount{mask, n_rows},
                       n_words, block_off);
    hipLaunchKernelGGL(compact_scan_sums_kernel, dim3(1), dim3(kCompactBlock), 0, s, block_off, nb, total);
    hipLaunchKernelGGL(mask_rows_window_kernel, dim3((unsigned)nb), dim3(kCompactBlock), 0, s, mask, n_rows, n_words, block_off, total,
                       first_row, offset, limit, d_rows, d_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "mask_rows_window_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

namespace {
// Caller holds h->rw (shared) and has h's device current.
int get_rows_enqueue(hr_index* h, hipStream_t s, const int64_t* d_rows, int64_t n, int out_dtype, void* d_out, int64_t out_stride,
                     int32_t* d_missing) {
    if (d_missing) HIP_TRY(h, hipMemsetAsync(d_missing, 0, sizeof(int32_t), s));
    if (n == 0) return HR_OK;
    const int64_t blocks = ((n + kRowsPerBlock - 1) / kRowsPerBlock + kGetRowsWaves - 1) / kGetRowsWaves;
    if (blocks > 0x7fffffffll) return fail(h, HR_ELIMIT, "too many rows");
    const size_t out_elem = out_dtype == HR_F16 ? 2 : 4;
    const bool vec = ((uintptr_t)d_out & 15) == 0 && (out_stride * out_elem) % 16 == 0;
    const dim3 grid((unsigned)blocks), block(kGetRowsWaves * 64);
#define HR_GET_ROWS(SRC, OUT, VEC)                                                                                              \
    hipLaunchKernelGGL((get_rows_kernel<SRC, OUT, VEC>), grid, block, 0, s, h->tiles.as<chunk_t>(), h->n_rows, h->row_offset, h->KT, \
                       h->dim, d_rows, n, d_out, out_stride, d_missing)
    if (h->dtype == HR_F16 && out_dtype == HR_F16) { if (vec) HR_GET_ROWS(true, true, true); else HR_GET_ROWS(true, true, false); }
    else if (h->dtype == HR_F16) { if (vec) HR_GET_ROWS(true, false, true); else HR_GET_ROWS(true, false, false); }
    else { if (vec) HR_GET_ROWS(false, false, true); else HR_GET_ROWS(false, false, false); }
#undef HR_GET_ROWS
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}

int check_get_rows(hr_index* h, int64_t n) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (h->dim == 0) return fail(h, HR_ESTATE, "handle has no dense collection");
    if (!h->finalized) return fail(h, HR_ESTATE, "rows are read after hr_finalize");
    if (n < 0) return fail(h, HR_EINVAL, "n must be >= 0 (got %lld)", (long long)n);
    return HR_OK;
}
}  // namespace

int hr_get_dense_rows_dev(hr_index* h, const int64_t* d_rows, int64_t n, int out_dtype, void* d_out, int64_t out_stride,
                          int32_t* d_missing, void* stream) {
    HR_TRY(check_get_rows(h, n));
    if (out_dtype != HR_F32 && out_dtype != HR_F16) return fail(h, HR_EINVAL, "unknown out_dtype %d", out_dtype);
    if (out_dtype == HR_F16 && h->dtype != HR_F16) return fail(h, HR_EINVAL, "HR_F16 output needs an fp16 shard (this one stores fp32)");
    if (out_stride < h->dim) return fail(h, HR_EINVAL, "out_stride %lld is below dim %lld", (long long)out_stride, (long long)h->dim);
    if (n > 0 && (!d_rows || !d_out)) return fail(h, HR_EINVAL, "null buffer");
    if ((uintptr_t)d_out & (out_dtype == HR_F16 ? 1 : 3)) return fail(h, HR_EINVAL, "d_out is not aligned to its element type");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    return get_rows_enqueue(h, (hipStream_t)stream, d_rows, n, out_dtype, d_out, out_stride, d_missing);
}

// ---- vector MMR (mmr.h: mmr_select_vec_kernel) ------------------------------------------------------------------------
namespace {
// Elements between two gathered rows: dim rounded up to whole 16-byte chunks of the shard's element type.
int64_t mmr_vec_stride(const hr_index* h) {
    const int64_t e = h->dtype == HR_F16 ? 8 : 4;
    return (h->dim + e - 1) / e * e;
}
}  // namespace

size_t hr_mmr_vec_scratch_bytes(const hr_index* h, int B, int k_in) {
    if (!h || h->dim == 0 || B <= 0 || k_in <= 0) return 0;
    return (size_t)B * (size_t)k_in * (size_t)mmr_vec_stride(h) * (h->dtype == HR_F16 ? 2 : 4);
}

int hr_mmr_select_vec_dev(hr_index* h, const int64_t* d_ids, const void* d_scores, int score_is_f64, int norm,
                          const int32_t* d_n, int B, int k_in, const double* d_lambda, int k_out, void* d_scratch,
                          int32_t* d_out_pos, double* d_out_val, int32_t* d_out_n, void* stream) {
    HR_TRY(check_get_rows(h, 0));
    if (B < 0 || k_in <= 0 || k_out <= 0 || k_out > k_in) return fail(h, HR_EINVAL, "bad mmr sizes");
    if (k_in > kFuseMax) return fail(h, HR_ELIMIT, "k_in exceeds 3 * HR_MAX_TOPK = %d", kFuseMax);
    if (norm < HR_NORM_NONE || norm > HR_NORM_MINMAX_DIST) return fail(h, HR_EINVAL, "bad norm code %d", norm);
    if (B == 0) return HR_OK;
    if (!d_ids || !d_scores || !d_n || !d_lambda || !d_scratch || !d_out_pos || !d_out_val || !d_out_n)
        return fail(h, HR_EINVAL, "null buffer");
    if (((uintptr_t)d_ids | (uintptr_t)d_lambda | (uintptr_t)d_out_val | (score_is_f64 ? (uintptr_t)d_scores : 0)) & 7)
        return fail(h, HR_EINVAL, "d_ids, d_lambda, d_out_val and fp64 scores must be 8-byte aligned");
    if (((uintptr_t)d_scores | (uintptr_t)d_n | (uintptr_t)d_out_pos | (uintptr_t)d_out_n) & 3)
        return fail(h, HR_EINVAL, "fp32 scores, d_n, d_out_pos and d_out_n must be 4-byte aligned");
    if ((uintptr_t)d_scratch & 15) return fail(h, HR_EINVAL, "d_scratch must be 16-byte aligned");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t stride = mmr_vec_stride(h);
    HR_TRY(get_rows_enqueue(h, s, d_ids, (int64_t)B * k_in, h->dtype == HR_F16 ? HR_F16 : HR_F32, d_scratch, stride, nullptr));
#define HR_MMR_VEC(STORE)                                                                                                      \
    hipLaunchKernelGGL(mmr_select_vec_kernel<STORE>, dim3(B), dim3(256), 0, s, d_ids, d_scores, score_is_f64, norm, d_n, k_in, \
                       (const STORE*)d_scratch, stride, (int)h->dim, h->norm2.as<double>(), h->n_rows, h->row_offset, d_lambda, \
                       k_out, d_out_pos, d_out_val, d_out_n)
    if (h->dtype == HR_F16) HR_MMR_VEC(_Float16);
    else HR_MMR_VEC(float);
#undef HR_MMR_VEC
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, HR_EHIP, "mmr_select_vec_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_get_dense_rows(hr_index* h, const int64_t* rows, int64_t n, float* out) {
    HR_TRY(check_get_rows(h, n));
    if (n == 0) return HR_OK;
    if (!rows || !out) return fail(h, HR_EINVAL, "null buffer");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    for (int64_t i = 0; i < n; ++i)   // refused before anything is read or written
        if (rows[i] < h->row_offset || rows[i] - h->row_offset >= h->n_rows)
            return fail(h, HR_EINVAL, "row id %lld (entry %lld) is outside this shard's rows [%lld, %lld)", (long long)rows[i],
                        (long long)i, (long long)h->row_offset, (long long)(h->row_offset + h->n_rows));
    DeviceGuard dg(h->device);
    Workspace* ws = take_ws(h);
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    int rc = [&]() -> int {
        hipStream_t s = ws->stream;
        const size_t out_bytes = (size_t)n * h->dim * sizeof(float);
        if (ws->d_ids.ensure((size_t)n * 8) != hipSuccess || ws->d_q.ensure(out_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, HR_ENOMEM, "cannot stage %lld rows", (long long)n);
        }
        HIP_TRY(h, hipMemcpyAsync(ws->d_ids.p, rows, (size_t)n * 8, hipMemcpyHostToDevice, s));
        HR_TRY(get_rows_enqueue(h, s, ws->d_ids.as<int64_t>(), n, HR_F32, ws->d_q.p, h->dim, nullptr));
        HIP_TRY(h, hipMemcpyAsync(out, ws->d_q.p, out_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        return HR_OK;
    }();
    give_ws(h, ws);
    return rc;
}

size_t hr_get_sparse_rows_scratch_bytes(int64_t n) {
    if (n < 0) return 0;
    const int64_t nb = (n + kCompactBlock - 1) / kCompactBlock;
    return (size_t)(std::max<int64_t>(nb, 1) + 1) * 8;  // the blocks' prefix, then the total
}

namespace {
int check_get_sparse_rows(hr_index* h, int64_t n) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (h->sparse_dim == 0) return fail(h, HR_ESTATE, "handle has no sparse collection");
    if (!h->finalized) return fail(h, HR_ESTATE, "sparse rows are read after hr_finalize (rows added since are staged on the host)");
    if (n < 0) return fail(h, HR_EINVAL, "n must be >= 0 (got %lld)", (long long)n);
    return HR_OK;
}

// Caller holds h->rw (shared), has h's device current and has checked the arguments.  cap == 0: sizes only.
int get_sparse_rows_enqueue(hr_index* h, hipStream_t s, const int64_t* d_rows, int64_t n, int64_t* d_out_indptr, int32_t* d_out_idx,
                            float* d_out_val, int64_t cap, int64_t* d_counts, void* d_scratch) {
    const int64_t nb = (n + kCompactBlock - 1) / kCompactBlock;
    const int64_t gather_blocks = (n + kGetSparseWaves - 1) / kGetSparseWaves;
    if (nb > 0x7fffffffll || gather_blocks > 0x7fffffffll) return fail(h, HR_ELIMIT, "too many rows (%lld)", (long long)n);
    if (n == 0) {
        hipLaunchKernelGGL(get_sparse_empty_kernel, dim3(1), dim3(64), 0, s, d_out_indptr, d_counts);
        HIP_TRY(h, hipGetLastError());
        return HR_OK;
    }
    unsigned long long* block_off = (unsigned long long*)d_scratch;
    unsigned long long* total = block_off + nb;
    const RequestedLength len{h->s_indptr.as<int64_t>(), d_rows, h->n_sparse, h->row_offset};
    HIP_TRY(h, hipMemsetAsync(d_counts + 1, 0, 8, s));
    hipLaunchKernelGGL((compact_block_sums_kernel<RequestedLength>), dim3((unsigned)nb), dim3(kCompactBlock), 0, s, len, n, block_off);
    hipLaunchKernelGGL(compact_scan_sums_kernel, dim3(1), dim3(kCompactBlock), 0, s, block_off, nb, total);
    hipLaunchKernelGGL(get_sparse_indptr_kernel, dim3((unsigned)nb), dim3(kCompactBlock), 0, s, len, n, block_off, total, d_out_indptr,
                       d_counts);
    if (cap > 0 && h->n_sparse > 0)
        hipLaunchKernelGGL(get_sparse_rows_kernel, dim3((unsigned)gather_blocks), dim3(kGetSparseWaves * 64), 0, s, h->s_indptr.as<int64_t>(),
                           h->s_idx.as<int32_t>(), h->s_val.as<float>(), h->n_sparse, h->row_offset, d_rows, n, d_out_indptr, d_out_idx,
                           d_out_val, cap);
    HIP_TRY(h, hipGetLastError());
    return HR_OK;
}
}  // namespace

int hr_get_sparse_rows_dev(hr_index* h, const int64_t* d_rows, int64_t n, int64_t* d_out_indptr, int32_t* d_out_idx, float* d_out_val,
                           int64_t cap, int64_t* d_counts, void* d_scratch, void* stream) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    HR_TRY(check_get_sparse_rows(h, n));
    if (cap < 0) return fail(h, HR_EINVAL, "cap must be >= 0 (got %lld)", (long long)cap);
    if (!d_out_indptr || !d_counts || !d_scratch || (n > 0 && !d_rows)) return fail(h, HR_EINVAL, "null buffer");
    if (cap > 0 && (!d_out_idx || !d_out_val)) return fail(h, HR_EINVAL, "null entry buffers with cap %lld", (long long)cap);
    if (((uintptr_t)d_rows | (uintptr_t)d_out_indptr | (uintptr_t)d_counts | (uintptr_t)d_scratch) & 7)
        return fail(h, HR_EINVAL, "d_rows, d_out_indptr, d_counts and d_scratch must be 8-byte aligned");
    if (((uintptr_t)d_out_idx | (uintptr_t)d_out_val) & 3) return fail(h, HR_EINVAL, "the entry buffers must be 4-byte aligned");
    DeviceGuard dg(h->device);
    return get_sparse_rows_enqueue(h, (hipStream_t)stream, d_rows, n, d_out_indptr, d_out_idx, d_out_val, cap, d_counts, d_scratch);
}

int hr_get_sparse_rows(hr_index* h, const int64_t* rows, int64_t n, int64_t* out_indptr, int32_t* out_idx, float* out_val, int64_t cap,
                       int64_t* nnz_total) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    HR_TRY(check_get_sparse_rows(h, n));
    if (cap < 0) return fail(h, HR_EINVAL, "cap must be >= 0 (got %lld)", (long long)cap);
    if (!out_indptr || !nnz_total || (n > 0 && !rows)) return fail(h, HR_EINVAL, "null buffer");
    if (cap > 0 && (!out_idx || !out_val)) return fail(h, HR_EINVAL, "null entry buffers with cap %lld", (long long)cap);
    for (int64_t i = 0; i < n; ++i)   // refused before anything is read or written
        if (rows[i] < h->row_offset || rows[i] - h->row_offset >= h->n_sparse)
            return fail(h, HR_EINVAL, "row id %lld (entry %lld) is outside this shard's sparse rows [%lld, %lld)", (long long)rows[i],
                        (long long)i, (long long)h->row_offset, (long long)(h->row_offset + h->n_sparse));
    if (n == 0) {
        out_indptr[0] = 0;
        *nnz_total = 0;
        return HR_OK;
    }
    DeviceGuard dg(h->device);
    Workspace* ws = take_ws(h);
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    int rc = [&]() -> int {
        hipStream_t s = ws->stream;
        // d_q: the output indptr [n + 1], the two counts, then the scan's scratch
        const size_t scratch_at = (size_t)(n + 3) * 8;
        if (ws->d_ids.ensure((size_t)n * 8) != hipSuccess || ws->d_q.ensure(scratch_at + hr_get_sparse_rows_scratch_bytes(n)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, HR_ENOMEM, "cannot stage %lld rows", (long long)n);
        }
        int64_t* d_indptr = ws->d_q.as<int64_t>();
        int64_t* d_counts = d_indptr + n + 1;
        void* d_scratch = (char*)ws->d_q.p + scratch_at;
        HIP_TRY(h, hipMemcpyAsync(ws->d_ids.p, rows, (size_t)n * 8, hipMemcpyHostToDevice, s));
        HR_TRY(get_sparse_rows_enqueue(h, s, ws->d_ids.as<int64_t>(), n, d_indptr, nullptr, nullptr, 0, d_counts, d_scratch));
        int64_t total = 0;
        HIP_TRY(h, hipMemcpyAsync(&total, d_counts, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out_indptr, d_indptr, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));  // the entry buffers are sized by it
        *nnz_total = total;
        if (total == 0 || total > cap) return HR_OK;  // the caller sizes its buffers from *nnz_total and calls again
        if (ws->d_qidx.ensure((size_t)total * 4) != hipSuccess || ws->d_qval.ensure((size_t)total * 4) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, HR_ENOMEM, "cannot stage %lld entries", (long long)total);
        }
        HR_TRY(get_sparse_rows_enqueue(h, s, ws->d_ids.as<int64_t>(), n, d_indptr, ws->d_qidx.as<int32_t>(), ws->d_qval.as<float>(), total,
                                       d_counts, d_scratch));
        HIP_TRY(h, hipMemcpyAsync(out_idx, ws->d_qidx.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out_val, ws->d_qval.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        return HR_OK;
    }();
    give_ws(h, ws);
    return rc;
}

int hr_add_layernorm_f16_dev(const void* d_x, const void* d_residual, const void* d_gamma, const void* d_beta, void* d_out,
                             int64_t rows, int hidden, float eps, void* stream) {
    if (rows < 0 || hidden <= 0 || hidden % 8 != 0) return fail(nullptr, HR_EINVAL, "hidden must be a positive multiple of 8");
    if (hidden > 1024) return fail(nullptr, HR_ELIMIT, "hidden exceeds 1024");
    if (!d_x || !d_gamma || !d_beta || !d_out) return fail(nullptr, HR_EINVAL, "null buffer");
    if (((uintptr_t)d_x | (uintptr_t)d_residual | (uintptr_t)d_gamma | (uintptr_t)d_beta | (uintptr_t)d_out) & 15)
        return fail(nullptr, HR_EINVAL, "buffers must be 16-byte aligned");
    if (rows == 0) return HR_OK;
    const int chunks = hidden / 8;
    const dim3 grid((unsigned)((rows + 15) / 16)), block(256);
    auto* x = (const half8_t*)d_x;
    auto* r = (const half8_t*)d_residual;
    auto* g = (const half8_t*)d_gamma;
    auto* b = (const half8_t*)d_beta;
    auto* o = (half8_t*)d_out;
    hipStream_t s = (hipStream_t)stream;
    if (chunks <= 16) hipLaunchKernelGGL((add_layernorm_f16_kernel<1>), grid, block, 0, s, x, r, g, b, o, rows, chunks, eps);
    else if (chunks <= 32) hipLaunchKernelGGL((add_layernorm_f16_kernel<2>), grid, block, 0, s, x, r, g, b, o, rows, chunks, eps);
    else if (chunks <= 48) hipLaunchKernelGGL((add_layernorm_f16_kernel<3>), grid, block, 0, s, x, r, g, b, o, rows, chunks, eps);
    else if (chunks <= 64) hipLaunchKernelGGL((add_layernorm_f16_kernel<4>), grid, block, 0, s, x, r, g, b, o, rows, chunks, eps);
    else hipLaunchKernelGGL((add_layernorm_f16_kernel<8>), grid, block, 0, s, x, r, g, b, o, rows, chunks, eps);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "add_layernorm_f16_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_embed_layernorm_f16_dev(const int64_t* d_ids, const int64_t* d_types, const void* d_word, const void* d_pos, const void* d_seg,
                               const void* d_gamma, const void* d_beta, void* d_out, int64_t n_seq, int T, int hidden, float eps,
                               int64_t n_word, int64_t n_seg, void* stream) {
    if (n_word <= 0 || n_seg <= 0) return fail(nullptr, HR_EINVAL, "empty embedding table");
    if (n_seq < 0 || T <= 0 || hidden <= 0 || hidden % 8 != 0) return fail(nullptr, HR_EINVAL, "hidden must be a positive multiple of 8");
    if (hidden > 1024) return fail(nullptr, HR_ELIMIT, "hidden exceeds 1024");
    if (!d_ids || !d_types || !d_word || !d_pos || !d_seg || !d_gamma || !d_beta || !d_out) return fail(nullptr, HR_EINVAL, "null buffer");
    if (((uintptr_t)d_word | (uintptr_t)d_pos | (uintptr_t)d_seg | (uintptr_t)d_gamma | (uintptr_t)d_beta | (uintptr_t)d_out) & 15)
        return fail(nullptr, HR_EINVAL, "buffers must be 16-byte aligned");
    const int64_t rows = n_seq * T;
    if (rows == 0) return HR_OK;
    const int chunks = hidden / 8;
    const dim3 grid((unsigned)((rows + 15) / 16)), block(256);
    auto* w = (const half8_t*)d_word;
    auto* p = (const half8_t*)d_pos;
    auto* sg = (const half8_t*)d_seg;
    auto* g = (const half8_t*)d_gamma;
    auto* b = (const half8_t*)d_beta;
    auto* o = (half8_t*)d_out;
    hipStream_t s = (hipStream_t)stream;
    if (chunks <= 16) hipLaunchKernelGGL((embed_layernorm_f16_kernel<1>), grid, block, 0, s, d_ids, d_types, w, p, sg, g, b, o, rows, T, chunks, eps, n_word, n_seg);
    else if (chunks <= 32) hipLaunchKernelGGL((embed_layernorm_f16_kernel<2>), grid, block, 0, s, d_ids, d_types, w, p, sg, g, b, o, rows, T, chunks, eps, n_word, n_seg);
    else if (chunks <= 48) hipLaunchKernelGGL((embed_layernorm_f16_kernel<3>), grid, block, 0, s, d_ids, d_types, w, p, sg, g, b, o, rows, T, chunks, eps, n_word, n_seg);
    else if (chunks <= 64) hipLaunchKernelGGL((embed_layernorm_f16_kernel<4>), grid, block, 0, s, d_ids, d_types, w, p, sg, g, b, o, rows, T, chunks, eps, n_word, n_seg);
    else hipLaunchKernelGGL((embed_layernorm_f16_kernel<8>), grid, block, 0, s, d_ids, d_types, w, p, sg, g, b, o, rows, T, chunks, eps, n_word, n_seg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "embed_layernorm_f16_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

static int attention_launch(const _Float16* q, int64_t q_seq, int64_t q_tok, const _Float16* k, const _Float16* v, int64_t kv_seq,
                            int64_t kv_tok, const int32_t* d_lengths, _Float16* out, int64_t n_seq, int T, int n_queries, int heads,
                            int head_dim, float scale, hipStream_t stream, bool out_fr = false) {
    if (n_seq < 0 || T <= 0 || heads <= 0 || n_queries <= 0 || n_queries > T) return fail(nullptr, HR_EINVAL, "bad attention sizes");
    if (head_dim != 32 && head_dim != 64) return fail(nullptr, HR_ELIMIT, "the attention kernels serve head dimensions 32 and 64 (got %d)", head_dim);
    const int max_t = kAttnLdsBytes / (4 * head_dim);                  // K + V of a (sequence, head) must fit the block's LDS
    if (T > max_t) return fail(nullptr, HR_ELIMIT, "sequence length %d exceeds %d at head dimension %d", T, max_t, head_dim);
    if (!q || !k || !v || !out) return fail(nullptr, HR_EINVAL, "null buffer");
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return fail(nullptr, HR_EINVAL, "buffers must be 16-byte aligned");
    if ((q_seq | q_tok | kv_seq | kv_tok) & 7) return fail(nullptr, HR_EINVAL, "strides must be multiples of 8 halves");
    if (n_seq == 0) return HR_OK;
    if (n_seq * heads > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "too many (sequence, head) pairs");
    const int n_chunks = (T + 31) / 32;
    const size_t lds = (size_t)n_chunks * 32 * 4 * head_dim;           // K and V^T of a (sequence, head)
    static bool attr_set = false;
    if (!attr_set) {
        const void* kernels[4] = {(const void*)attention_kernel<4, 32>, (const void*)attention_kernel<8, 32>,
                                  (const void*)attention_kernel<4, 64>, (const void*)attention_kernel<8, 64>};
        for (const void* f : kernels) {
            hipError_t e0 = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kAttnLdsBytes);
            if (e0 != hipSuccess) return fail(nullptr, HR_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e0));
        }
        attr_set = true;
    }
    const int NW = n_queries <= 128 ? 4 : 8;                           // waves (x 32 queries) per block
    const int HG = head_dim == 32 ? 2 : 1;                             // heads per 128-byte line of the QKV buffer
    AttnArgs a{};
    a.q = q; a.k = k; a.v = v; a.out = out; a.lengths = d_lengths;
    a.q_seq = q_seq; a.q_tok = q_tok; a.kv_seq = kv_seq; a.kv_tok = kv_tok;
    a.T = T; a.n_queries = n_queries; a.heads = heads;
    a.n_qblocks = (n_queries + 32 * NW - 1) / (32 * NW);
    a.n_pairs = n_seq * ((heads + HG - 1) / HG);                       // head groups: the blocks of a group share an XCD
    a.scale_log2e = scale * 1.4426950408889634f;
    a.out_fr = out_fr ? 1 : 0;
    const int64_t n_blocks = ((a.n_pairs + 7) / 8) * 8 * HG * a.n_qblocks;
    if (n_blocks > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "too many attention blocks");
    if (head_dim == 32) {
        if (NW == 4) hipLaunchKernelGGL((attention_kernel<4, 32>), dim3((unsigned)n_blocks), dim3(256), lds, stream, a);
        else hipLaunchKernelGGL((attention_kernel<8, 32>), dim3((unsigned)n_blocks), dim3(512), lds, stream, a);
    } else {
        if (NW == 4) hipLaunchKernelGGL((attention_kernel<4, 64>), dim3((unsigned)n_blocks), dim3(256), lds, stream, a);
        else hipLaunchKernelGGL((attention_kernel<8, 64>), dim3((unsigned)n_blocks), dim3(512), lds, stream, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "attention_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_attention_f16_dev(const void* d_qkv, const int32_t* d_lengths, void* d_out, int64_t n_seq, int T, int heads,
                         int head_dim, float scale, void* stream) {
    if (!d_qkv) return fail(nullptr, HR_EINVAL, "null buffer");
    const int64_t H = (int64_t)heads * head_dim;
    const _Float16* qkv = (const _Float16*)d_qkv;
    return attention_launch(qkv, (int64_t)T * 3 * H, 3 * H, qkv + H, qkv + 2 * H, (int64_t)T * 3 * H, 3 * H, d_lengths, (_Float16*)d_out,
                            n_seq, T, T, heads, head_dim, scale, (hipStream_t)stream);
}

int hr_attention_fr_f16_dev(const void* d_qkv, const int32_t* d_lengths, void* d_out_fr, int64_t n_seq, int T, int heads,
                            int head_dim, float scale, void* stream) {
    if (!d_qkv) return fail(nullptr, HR_EINVAL, "null buffer");
    const int64_t H = (int64_t)heads * head_dim;
    if (H % 32 != 0) return fail(nullptr, HR_EINVAL, "fragment-order output needs a hidden size that is a multiple of 32");
    const _Float16* qkv = (const _Float16*)d_qkv;
    return attention_launch(qkv, (int64_t)T * 3 * H, 3 * H, qkv + H, qkv + 2 * H, (int64_t)T * 3 * H, 3 * H, d_lengths, (_Float16*)d_out_fr,
                            n_seq, T, T, heads, head_dim, scale, (hipStream_t)stream, true);
}

int hr_attention_rows_f16_dev(const void* d_q, int64_t q_seq_stride, int64_t q_token_stride, const void* d_k, const void* d_v,
                              int64_t kv_seq_stride, int64_t kv_token_stride, const int32_t* d_lengths, void* d_out, int64_t n_seq,
                              int T, int n_queries, int heads, int head_dim, float scale, void* stream) {
    return attention_launch((const _Float16*)d_q, q_seq_stride, q_token_stride, (const _Float16*)d_k, (const _Float16*)d_v, kv_seq_stride,
                            kv_token_stride, d_lengths, (_Float16*)d_out, n_seq, T, n_queries, heads, head_dim, scale,
                            (hipStream_t)stream);
}

// ---- encoder layer kernels (csrc/encoder_layer.h) -----------------------------------------------------------------
static int el_allow_lds(const void* kernel, size_t bytes) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e == hipSuccess ? HR_OK : fail(nullptr, HR_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
}

int hr_linear_rows_f16_dev(const void* d_x, int x_fr, const void* d_w_packed, const float* d_bias, void* d_out, int64_t rows, int K, int N,
                           int64_t out_stride, void* stream) {
    if (rows < 0 || K <= 0 || N <= 0 || N % 32 != 0 || out_stride < N || out_stride % 4 != 0) return fail(nullptr, HR_EINVAL, "bad linear sizes");
    if (K != 384) return fail(nullptr, HR_ELIMIT, "the hand-written linear kernel serves K = 384 (got %d)", K);
    if (N > 4096) return fail(nullptr, HR_ELIMIT, "N exceeds 4096");
    if (!d_x || !d_w_packed || !d_bias || !d_out) return fail(nullptr, HR_EINVAL, "null buffer");
    if (((uintptr_t)d_x | (uintptr_t)d_w_packed | (uintptr_t)d_bias | (uintptr_t)d_out) & 15) return fail(nullptr, HR_EINVAL, "buffers must be 16-byte aligned");
    if (rows == 0) return HR_OK;
    constexpr int KS = 12;
    const size_t lds = (size_t)(kElRingStages + 1) * 2 * KS * 1024 + (size_t)N * 4;
    static bool ready = false;
    if (!ready) {
        HR_TRY(el_allow_lds((const void*)linear_rows_kernel<KS, 2>, 160 * 1024));
        HR_TRY(el_allow_lds((const void*)linear_rows_kernel<KS, 4>, 160 * 1024));
        ready = true;
    }
    LinearArgs a{};
    a.x = (const _Float16*)d_x; a.w = (const chunk_t*)d_w_packed; a.bias = d_bias; a.out = (_Float16*)d_out;
    a.M = rows; a.out_stride = out_stride; a.N = N; a.x_fr = x_fr ? 1 : 0;
    // Four token tiles per wave (a weight fragment read from LDS feeds four MFMAs instead of two: 0.367 -> 0.335 ms for
    // 327 680 rows x 1 152 outputs) once blocks of 256 rows still fill the chip; two below that, where a block's latency counts
    const bool wide = rows >= 256 * 256;
    const int rows_per_block = wide ? 256 : 128;
    const int64_t blocks = (rows + rows_per_block - 1) / rows_per_block;
    if (blocks > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "too many rows");
    if (wide) hipLaunchKernelGGL((linear_rows_kernel<KS, 4>), dim3((unsigned)blocks), dim3(64 * kElWaves), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((linear_rows_kernel<KS, 2>), dim3((unsigned)blocks), dim3(64 * kElWaves), lds, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "linear_rows_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_encoder_tail_f16_dev(const void* d_attn_fr, const void* d_x, int x_fr, void* d_out, int out_fr, const void* d_wstream,
                            const float* d_tables, int64_t rows, int hidden, int intermediate, float eps, int gelu_erf, void* stream) {
    if (rows < 0 || hidden <= 0 || intermediate <= 0) return fail(nullptr, HR_EINVAL, "bad encoder-tail sizes");
    if (hidden != 384 || intermediate != 1536)
        return fail(nullptr, HR_ELIMIT, "the fused layer tail serves (hidden, intermediate) = (384, 1536) (got %d, %d)", hidden, intermediate);
    if (!d_attn_fr || !d_x || !d_out || !d_wstream || !d_tables) return fail(nullptr, HR_EINVAL, "null buffer");
    if (((uintptr_t)d_attn_fr | (uintptr_t)d_x | (uintptr_t)d_out | (uintptr_t)d_wstream | (uintptr_t)d_tables) & 15)
        return fail(nullptr, HR_EINVAL, "buffers must be 16-byte aligned");
    if (rows == 0) return HR_OK;
    constexpr int HS = 12, IS = 48, TT = 2;
    const size_t lds = (size_t)kElRingStages * 2 * HS * 1024 + (size_t)(6 * hidden + intermediate) * 4;
    static bool ready = false;
    if (!ready) {
        HR_TRY(el_allow_lds((const void*)encoder_tail_kernel<HS, IS, TT, false>, 160 * 1024));
        HR_TRY(el_allow_lds((const void*)encoder_tail_kernel<HS, IS, TT, true>, 160 * 1024));
        ready = true;
    }
    TailArgs a{};
    a.a = (const _Float16*)d_attn_fr; a.x = (const _Float16*)d_x; a.out = (_Float16*)d_out; a.x_fr = x_fr ? 1 : 0; a.out_fr = out_fr ? 1 : 0;
    a.wstream = (const chunk_t*)d_wstream; a.tables = d_tables; a.M = rows; a.eps = eps;
    const int64_t blocks = (rows + 64 * TT - 1) / (64 * TT);
    if (blocks > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "too many rows");
    if (gelu_erf)
        hipLaunchKernelGGL((encoder_tail_kernel<HS, IS, TT, true>), dim3((unsigned)blocks), dim3(64 * kElWaves), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((encoder_tail_kernel<HS, IS, TT, false>), dim3((unsigned)blocks), dim3(64 * kElWaves), lds, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, HR_EHIP, "encoder_tail_kernel: %s", hipGetErrorString(e));
    return HR_OK;
}

// ---- host-buffer, synchronous forms -------------------------------------------------
// ranged: a range search with host arrays radius / range_filter ([B] each, null = unbounded).
static int search_dense_host(hr_index* h, const float* q, int B, int k, const uint8_t* rowmask, bool mask_on_device,
                             int64_t* out_ids, float* out_scores, bool ranged = false, const double* radius = nullptr,
                             const double* range_filter = nullptr) {
    HR_TRY(check_search_args(h, B, k, true));
    if (!q || !out_ids || !out_scores) return fail(h, HR_EINVAL, "null buffer");
    for (int64_t i = 0; i < (int64_t)B * h->dim; ++i)   // the scan's bound (and the ranking) assume finite queries
        if (!std::isfinite(q[i])) return fail(h, HR_EINVAL, "non-finite value in query %lld", (long long)(i / h->dim));
    for (int b = 0; ranged && b < B; ++b) {  // refused before anything is launched or written
        const bool l2 = h->metric == HR_METRIC_L2;
        const double r = radius ? radius[b] : (l2 ? INFINITY : -INFINITY);
        const double f = range_filter ? range_filter[b] : (l2 ? -INFINITY : INFINITY);
        if (std::isnan(r) || std::isnan(f)) return fail(h, HR_EINVAL, "NaN range bound in query %d", b);
        if (l2 ? f >= r : r >= f)
            return fail(h, HR_EINVAL, "empty range in query %d: radius %g, range_filter %g (%s)", b, r, f,
                        l2 ? "L2 keeps range_filter <= distance < radius" : "kept are radius < score <= range_filter");
    }
    DenseRange rng{nullptr, nullptr};
    return search_host(
        h, B, k, &hr_index::n_rows, rowmask, mask_on_device, out_ids, out_scores,
        [&](Workspace* ws, hipStream_t s) {
            HIP_TRY(h, ws->d_q.ensure((size_t)B * h->dim * 4));
            HIP_TRY(h, hipMemcpyAsync(ws->d_q.p, q, (size_t)B * h->dim * 4, hipMemcpyHostToDevice, s));
            if (radius) {
                HIP_TRY(h, ws->d_radius.ensure((size_t)B * sizeof(double)));
                HIP_TRY(h, hipMemcpyAsync(ws->d_radius.p, radius, (size_t)B * sizeof(double), hipMemcpyHostToDevice, s));
                rng.d_radius = ws->d_radius.as<double>();
            }
            if (range_filter) {
                HIP_TRY(h, ws->d_rfilter.ensure((size_t)B * sizeof(double)));
                HIP_TRY(h, hipMemcpyAsync(ws->d_rfilter.p, range_filter, (size_t)B * sizeof(double), hipMemcpyHostToDevice, s));
                rng.d_range_filter = ws->d_rfilter.as<double>();
            }
            return (int)HR_OK;
        },
        [&](Workspace* ws, hipStream_t s, const uint8_t* d_mask, const OutLists& out, int C) {
            return dense_search_enqueue(h, ws, s, ws->d_q.as<float>(), B, k, d_mask, out, C, nullptr, PHASE_ALL,
                                        ranged ? &rng : nullptr);
        });
}

int hr_search_dense_range(hr_index* h, const float* q, int B, int k, const uint8_t* rowmask, int mask_on_device,
                          const double* radius, const double* range_filter, int64_t* out_ids, float* out_scores) {
    return search_dense_host(h, q, B, k, rowmask, mask_on_device != 0, out_ids, out_scores, true, radius, range_filter);
}

int hr_search_dense(hr_index* h, const float* q, int B, int k, const uint8_t* rowmask, int64_t* out_ids,
                    float* out_scores) {
    return search_dense_host(h, q, B, k, rowmask, false, out_ids, out_scores);
}
int hr_search_dense_dmask(hr_index* h, const float* q, int B, int k, const uint8_t* d_rowmask, int64_t* out_ids,
                          float* out_scores) {
    return search_dense_host(h, q, B, k, d_rowmask, true, out_ids, out_scores);
}

// The sparse host forms' query prep: the checked, dropped and index-ordered queries as one CSR, and how to stage it.
struct SparseQueries {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx;
    std::vector<float> val;
    int max_nnz = 0;
    int stage(hr_index* h, Workspace* ws, hipStream_t s) const {
        const size_t B1 = ptr.size(), nnz = idx.size();
        HIP_TRY(h, ws->d_qptr.ensure(B1 * 8));
        HIP_TRY(h, ws->d_qidx.ensure(std::max<size_t>(nnz, 1) * 4));
        HIP_TRY(h, ws->d_qval.ensure(std::max<size_t>(nnz, 1) * 4));
        HIP_TRY(h, hipMemcpyAsync(ws->d_qptr.p, ptr.data(), B1 * 8, hipMemcpyHostToDevice, s));
        if (nnz) {
            HIP_TRY(h, hipMemcpyAsync(ws->d_qidx.p, idx.data(), nnz * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(h, hipMemcpyAsync(ws->d_qval.p, val.data(), nnz * 4, hipMemcpyHostToDevice, s));
        }
        return HR_OK;
    }
};
static int prep_sparse_queries(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B,
                               float drop_ratio, SparseQueries* out) {
    if (!(drop_ratio >= 0.f && drop_ratio < 1.f)) return fail(h, HR_EINVAL, "drop_ratio must be in [0,1)");
    // Host prep: drop the floor(drop_ratio*nnz) smallest-|value| entries (ties:
    // the later entry goes first), then order by index.
    std::vector<int64_t>& ptr = out->ptr;
    std::vector<int32_t>& idx = out->idx;
    std::vector<float>& val = out->val;
    int& max_nnz = out->max_nnz;
    ptr.assign(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        const int64_t e0 = q_indptr[b], e1 = q_indptr[b + 1];
        if (e1 < e0) return fail(h, HR_EINVAL, "query indptr not monotone");
        const int nnz = (int)(e1 - e0);
        if (nnz > 0 && (!q_idx || !q_val)) return fail(h, HR_EINVAL, "null query arrays");
        for (int64_t e = e0; e < e1; ++e)   // before drop_ratio: a NaN has no place in the |value| order
            if (!std::isfinite(q_val[e])) return fail(h, HR_EINVAL, "non-finite value in sparse query %d", b);
        std::vector<int> order(nnz);
        for (int i = 0; i < nnz; ++i) order[i] = i;
        const int n_drop = (int)std::floor((double)drop_ratio * nnz);
        std::stable_sort(order.begin(), order.end(), [&](int a, int c) {
            const float fa = std::fabs(q_val[e0 + a]), fc = std::fabs(q_val[e0 + c]);
            if (fa != fc) return fa < fc;
            return a > c;
        });
        std::vector<int> keep(order.begin() + n_drop, order.end());
        std::sort(keep.begin(), keep.end(), [&](int a, int c) { return q_idx[e0 + a] < q_idx[e0 + c]; });
        int32_t prev = -1;
        for (int i : keep) {
            const int32_t t = q_idx[e0 + i];
            if (t < 0 || t >= h->sparse_dim) return fail(h, HR_EINVAL, "query index %d out of range", t);
            if (t == prev) return fail(h, HR_EINVAL, "duplicate query index %d", t);
            prev = t;
            idx.push_back(t);
            val.push_back(q_val[e0 + i]);
        }
        ptr[b + 1] = (int64_t)idx.size();
        max_nnz = std::max(max_nnz, (int)keep.size());
    }
    if (max_nnz > HR_MAX_QUERY_NNZ) return fail(h, HR_ELIMIT, "query nnz %d exceeds HR_MAX_QUERY_NNZ", max_nnz);
    return HR_OK;
}

static int search_sparse_host(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B, int k,
                              float drop_ratio, const uint8_t* rowmask, bool mask_on_device, int64_t* out_ids,
                              float* out_scores) {
    HR_TRY(check_search_args(h, B, k, false));
    if (!q_indptr || !out_ids || !out_scores) return fail(h, HR_EINVAL, "null buffer");
    SparseQueries sq;
    HR_TRY(prep_sparse_queries(h, q_indptr, q_idx, q_val, B, drop_ratio, &sq));
    return search_host(
        h, B, k, &hr_index::n_sparse, rowmask, mask_on_device, out_ids, out_scores,
        [&](Workspace* ws, hipStream_t s) { return sq.stage(h, ws, s); },
        [&](Workspace* ws, hipStream_t s, const uint8_t* d_mask, const OutLists& out, int C) {
            return sparse_search_enqueue(h, ws, s, ws->d_qptr.as<int64_t>(), ws->d_qidx.as<int32_t>(),
                                         ws->d_qval.as<float>(), B, sq.max_nnz, k, d_mask, out, C);
        });
}

int hr_search_sparse(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B, int k,
                     float drop_ratio, const uint8_t* rowmask, int64_t* out_ids, float* out_scores) {
    return search_sparse_host(h, q_indptr, q_idx, q_val, B, k, drop_ratio, rowmask, false, out_ids, out_scores);
}
int hr_search_sparse_dmask(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B, int k,
                           float drop_ratio, const uint8_t* d_rowmask, int64_t* out_ids, float* out_scores) {
    return search_sparse_host(h, q_indptr, q_idx, q_val, B, k, drop_ratio, d_rowmask, true, out_ids, out_scores);
}

// ---- deep search (deep.h) ----------------------------------------------------------------------------------------
namespace {
inline size_t deep_align(size_t b) { return (b + 255) / 256 * 256; }
inline size_t deep_zeroed_bytes(int B) { return deep_align((size_t)B * sizeof(DeepState)) + (size_t)B * kDeepPasses * 256 * sizeof(unsigned); }
inline int deep_sort_slots(int W) {   // keys the sort holds in LDS: W padded to a power of two, 64 at least
    int P = 64;
    while (P < W) P <<= 1;
    return P;
}
int check_deep_window(const hr_index* h, int k, int offset) {
    if (k < 1) return fail(h, HR_EINVAL, "k must be positive (got %d)", k);
    if (offset < 0) return fail(h, HR_EINVAL, "offset must not be negative (got %d)", offset);
    if ((int64_t)k + offset > HR_MAX_DEEP_K)
        return fail(h, HR_ELIMIT, "k + offset = %lld exceeds HR_MAX_DEEP_K=%d", (long long)k + offset, HR_MAX_DEEP_K);
    return HR_OK;
}
}  // namespace

size_t hr_deep_topk_scratch_bytes(int64_t n, int B, int window) {
    (void)n;   // the per-query tables do not grow with the candidates
    if (B < 1 || window < 1) return 0;
    return deep_zeroed_bytes(B) + (size_t)B * window * sizeof(unsigned long long);
}

namespace {
// hr_deep_topk_dev and, with d_bounds, hr_deep_topk_window_dev: the same sixteen + two launches, the hist and gather
// kernels in their windowed instantiation when there is an interval to apply.
int deep_topk_launch(const float* d_scores, const int32_t* d_rows, int64_t n, int B, int k, int offset, int ascending,
                     int64_t row_offset, int64_t* d_out_ids, float* d_out_scores, void* d_scratch, void* stream,
                     const unsigned long long* d_bounds) {
    HR_TRY(check_deep_window(nullptr, k, offset));
    if (n < 0) return fail(nullptr, HR_EINVAL, "n must not be negative");
    if (B < 1) return fail(nullptr, HR_EINVAL, "batch size must be positive (got %d)", B);
    if (B > 65535) return fail(nullptr, HR_ELIMIT, "batch size %d exceeds one grid (65535)", B);
    if (n > 0x7fffffffll) return fail(nullptr, HR_ELIMIT, "n exceeds the int32 row range");
    if (!d_out_ids || !d_out_scores) return fail(nullptr, HR_EINVAL, "null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(nullptr, hipMemsetAsync(d_out_ids, 0xFF, (size_t)B * k * sizeof(int64_t), s));
        HIP_TRY(nullptr, hipMemsetAsync(d_out_scores, 0, (size_t)B * k * sizeof(float), s));
        return HR_OK;
    }
    if (!d_scores || !d_rows || !d_scratch) return fail(nullptr, HR_EINVAL, "null buffer");
    if ((uintptr_t)d_scratch % 8) return fail(nullptr, HR_EINVAL, "scratch buffer not 8-byte aligned");
    const int W = k + offset;
    DeepArgs a{};
    a.score = d_scores;
    a.row = d_rows;
    a.n = n;
    a.W = W;
    char* base = static_cast<char*>(d_scratch);
    a.state = reinterpret_cast<DeepState*>(base);
    a.hist = reinterpret_cast<unsigned*>(base + deep_align((size_t)B * sizeof(DeepState)));
    a.keys = reinterpret_cast<unsigned long long*>(base + deep_zeroed_bytes(B));
    a.bounds = d_bounds;
    HIP_TRY(nullptr, hipMemsetAsync(base, 0, deep_zeroed_bytes(B), s));
    // blocks per query: 8 keys per thread at least, and no more than a few rounds of the chip
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((n + kDeepHistThreads * 8 - 1) / (kDeepHistThreads * 8), 1),
                                                        std::max(1, 4096 / B));
    const auto hist = d_bounds ? deep_hist_kernel<true> : deep_hist_kernel<false>;
    for (int pass = 0; pass < kDeepPasses; ++pass) {
        hipLaunchKernelGGL(hist, dim3(blocks, B), dim3(kDeepHistThreads), 0, s, a, pass);
        hipLaunchKernelGGL(deep_pick_kernel, dim3(B), dim3(64), 0, s, a, pass);
    }
    hipLaunchKernelGGL(d_bounds ? deep_gather_kernel<true> : deep_gather_kernel<false>, dim3(blocks, B), dim3(kDeepHistThreads), 0,
                       s, a);
    HIP_TRY(nullptr, hipGetLastError());
    const int P = deep_sort_slots(W);
    if ((size_t)P * sizeof(unsigned long long) > 48 * 1024)   // per device, idempotent: set where the default does not reach
        HIP_TRY(nullptr, hipFuncSetAttribute((const void*)deep_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             deep_sort_slots(HR_MAX_DEEP_K) * (int)sizeof(unsigned long long)));
    hipLaunchKernelGGL(deep_sort_kernel, dim3(B), dim3(kDeepSortThreads), (size_t)P * sizeof(unsigned long long), s, a, P, k, offset,
                       ascending != 0, row_offset, d_out_ids, d_out_scores);
    HIP_TRY(nullptr, hipGetLastError());
    return HR_OK;
}
}  // namespace

int hr_deep_topk_dev(const float* d_scores, const int32_t* d_rows, int64_t n, int B, int k, int offset, int ascending,
                     int64_t row_offset, int64_t* d_out_ids, float* d_out_scores, void* d_scratch, void* stream) {
    return deep_topk_launch(d_scores, d_rows, n, B, k, offset, ascending, row_offset, d_out_ids, d_out_scores, d_scratch, stream,
                            nullptr);
}

int hr_deep_topk_window_dev(const float* d_scores, const int32_t* d_rows, int64_t n, int B, int k, int ascending,
                            int64_t row_offset, const unsigned long long* d_bounds, int64_t* d_out_ids, float* d_out_scores,
                            void* d_scratch, void* stream) {
    return deep_topk_launch(d_scores, d_rows, n, B, k, 0, ascending, row_offset, d_out_ids, d_out_scores, d_scratch, stream,
                            d_bounds);
}

namespace {
constexpr size_t kDeepCandidateCap = (size_t)512 << 20;   // transient candidate arrays of one pass of queries

// What the two deep host forms share, after their own argument checks and query prep.  stage(ws, s) uploads the queries
// and runs their device prep; refine(s, c0, nq, d_mask, C, GR, bufs) refines all C candidate groups for queries
// c0 .. c0 + nq - 1 into bufs.  Every buffer that grows with the shard is a local of this call.
extern "C++" template <typename Stage, typename Refine>
int deep_host(hr_index* h, int B, int k, int offset, int64_t hr_index::*rows, bool ascending, int ph_refine, int ph_topk,
              const uint8_t* rowmask, bool mask_on_device, int64_t* out_ids, float* out_scores, Stage stage, Refine refine,
              const unsigned long long* bounds = nullptr) {
    std::shared_lock<std::shared_mutex> lk(h->rw);
    DeviceGuard dg(h->device);
    const int64_t n_rows = h->*rows;
    if (n_rows == 0) {
        std::fill(out_ids, out_ids + (size_t)B * k, (int64_t)-1);
        std::fill(out_scores, out_scores + (size_t)B * k, 0.f);
        return HR_OK;
    }
    const int GR = group_rows_for(h, n_rows);
    const int64_t n_groups = (n_rows + GR - 1) / GR;
    const int64_t C64 = round_up(n_groups, 16), n_slots = C64 * GR;   // every group, as the last rung of next_candidate_count
    if (n_slots > 0x7fffffffll) return fail(h, HR_ELIMIT, "shard too large for a full refine");
    const int C = (int)C64;
    const size_t per_query = (size_t)n_slots * 8 + (size_t)C * 4;
    int Bp = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, kDeepCandidateCap / per_query));
    DevBuf cscore, crow, cand, acut, scratch, d_ids, d_scores, d_bounds;
    for (;; Bp = (Bp + 1) / 2) {
        const bool ok = cscore.alloc_exact((size_t)Bp * n_slots * 4) == hipSuccess &&
                        crow.alloc_exact((size_t)Bp * n_slots * 4) == hipSuccess &&
                        cand.alloc_exact((size_t)Bp * C * 4) == hipSuccess;
        if (ok) break;
        (void)hipGetLastError();
        cscore.release(), crow.release(), cand.release();
        if (Bp == 1)
            return fail(h, HR_ENOMEM, "deep search: %zu bytes of candidate arrays for one query do not fit", per_query);
    }
    if (acut.alloc_exact((size_t)Bp * 4) != hipSuccess || d_ids.alloc_exact((size_t)B * k * 8) != hipSuccess ||
        d_scores.alloc_exact((size_t)B * k * 4) != hipSuccess ||
        scratch.alloc_exact(hr_deep_topk_scratch_bytes(n_slots, Bp, k + offset)) != hipSuccess ||
        (bounds && d_bounds.alloc_exact((size_t)B * 16) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(h, HR_ENOMEM, "deep search: list buffers do not fit");
    }
    PooledWs pooled(h);
    Workspace* ws = pooled.w;
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    hipStream_t s = ws->stream;
    HR_TRY(stage(ws, s));
    if (bounds) HIP_TRY(h, hipMemcpyAsync(d_bounds.p, bounds, (size_t)B * 16, hipMemcpyHostToDevice, s));
    const uint8_t* d_mask = mask_on_device ? rowmask : nullptr;
    if (rowmask && !mask_on_device) {
        const size_t mb = (size_t)(n_rows + 7) / 8;
        HIP_TRY(h, ws->d_mask.ensure(mb));
        HIP_TRY(h, hipMemcpyAsync(ws->d_mask.p, rowmask, mb, hipMemcpyHostToDevice, s));
        d_mask = ws->d_mask.as<uint8_t>();
    }
    {   // n_groups <= C: select_groups_block writes the identity list (and -1 behind the last group); no maxima are read
        GroupSelPair p{};
        p.n = 1;
        GroupSelArgs& g = p.m[0];
        g.n_groups = n_groups;
        g.n_buckets = bucket_count(n_groups);
        g.C = C;
        g.cand = cand.as<int32_t>();
        g.a_cut = acut.as<float>();
        HR_TRY(launch_group_select_pair(h, s, Bp, p));
    }
    int rc = HR_OK;
    for (int c0 = 0; c0 < B && rc == HR_OK; c0 += Bp) {
        const int nq = std::min(Bp, B - c0);
        {
            Span sp(h, s, ph_refine);
            rc = refine(s, c0, nq, d_mask, C, GR, RefineBufs{nullptr, cand.as<int32_t>(), cscore.as<float>(), crow.as<int32_t>()});
        }
        if (rc != HR_OK) break;
        Span sp(h, s, ph_topk);
        rc = deep_topk_launch(cscore.as<float>(), crow.as<int32_t>(), n_slots, nq, k, offset, ascending, h->row_offset,
                              d_ids.as<int64_t>() + (size_t)c0 * k, d_scores.as<float>() + (size_t)c0 * k, scratch.p, s,
                              bounds ? d_bounds.as<unsigned long long>() + (size_t)c0 * 2 : nullptr);
        if (rc != HR_OK) rc = fail(h, rc, "deep selection: %s", std::string(g_last_error).c_str());
    }
    if (rc != HR_OK) {
        (void)hipStreamSynchronize(s);   // the locals are freed on return
        return rc;
    }
    HIP_TRY(h, hipMemcpyAsync(out_ids, d_ids.p, (size_t)B * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_scores, d_scores.p, (size_t)B * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return HR_OK;
}

int check_deep_args(hr_index* h, int B, int k, int offset, bool dense) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (B <= 0) return fail(h, HR_EINVAL, "batch size must be positive (got %d)", B);
    HR_TRY(check_deep_window(h, k, offset));
    if (!h->finalized) return fail(h, HR_ESTATE, "search before hr_finalize");
    if (dense && h->dim == 0) return fail(h, HR_ESTATE, "handle has no dense collection");
    if (!dense && h->sparse_dim == 0) return fail(h, HR_ESTATE, "handle has no sparse collection");
    return HR_OK;
}
}  // namespace

namespace {
// The dense deep forms after their argument checks; bounds: the cursor form's key intervals ([B][2], host), or null.
int dense_deep_host(hr_index* h, const float* q, int B, int k, int offset, const uint8_t* rowmask, int mask_on_device,
                    int64_t* out_ids, float* out_scores, const unsigned long long* bounds) {
    Workspace* held = nullptr;
    return deep_host(
        h, B, k, offset, &hr_index::n_rows, h->metric == HR_METRIC_L2, PH_REFINE, PH_TOPK, rowmask, mask_on_device != 0, out_ids,
        out_scores,
        [&](Workspace* ws, hipStream_t s) {
            held = ws;
            HIP_TRY(h, ws->d_q.ensure((size_t)B * h->dim * 4));
            HIP_TRY(h, hipMemcpyAsync(ws->d_q.p, q, (size_t)B * h->dim * 4, hipMemcpyHostToDevice, s));
            // the query prep of a plain search (squared norms for the refine); no scan, no finish
            return dense_search_enqueue(h, ws, s, ws->d_q.as<float>(), B, 1, nullptr, OutLists{nullptr, nullptr, nullptr},
                                        candidate_groups_for_k(1), nullptr, PHASE_PREP);
        },
        [&](hipStream_t s, int c0, int nq, const uint8_t* d_mask, int C, int GR, RefineBufs b) {
            FinishSide f{};
            f.GR = GR;
            f.C = C;
            f.mask = d_mask;
            f.d_q = held->d_q.as<float>() + (size_t)c0 * h->dim;
            b.qn2 = held->qn2.as<double>() + c0;
            return launch_refine(h, s, nq, f, b);
        },
        bounds);
}

int check_dense_deep_buffers(hr_index* h, const float* q, int B, const int64_t* out_ids, const float* out_scores) {
    if (!q || !out_ids || !out_scores) return fail(h, HR_EINVAL, "null buffer");
    for (int64_t i = 0; i < (int64_t)B * h->dim; ++i)
        if (!std::isfinite(q[i])) return fail(h, HR_EINVAL, "non-finite value in query %lld", (long long)(i / h->dim));
    return HR_OK;
}

int sparse_deep_host(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B, int k, int offset,
                     float drop_ratio, const uint8_t* rowmask, int mask_on_device, int64_t* out_ids, float* out_scores,
                     const unsigned long long* bounds) {
    SparseQueries sq;
    HR_TRY(prep_sparse_queries(h, q_indptr, q_idx, q_val, B, drop_ratio, &sq));
    Workspace* held = nullptr;
    return deep_host(
        h, B, k, offset, &hr_index::n_sparse, false, PH_SREFINE, PH_STOPK, rowmask, mask_on_device != 0, out_ids, out_scores,
        [&](Workspace* ws, hipStream_t s) {
            held = ws;
            return sq.stage(h, ws, s);
        },
        [&](hipStream_t s, int c0, int nq, const uint8_t* d_mask, int C, int GR, RefineBufs b) {
            FinishSide f{};
            f.sparse = true;
            f.GR = GR;
            f.C = C;
            f.mask = d_mask;
            f.q_ptr = held->d_qptr.as<int64_t>() + c0;   // the entries are positions in the whole batch's arrays
            f.q_idx = held->d_qidx.as<int32_t>();
            f.q_val = held->d_qval.as<float>();
            f.stride = (int)round_up(std::max(sq.max_nnz, 1), 64);
            return launch_refine(h, s, nq, f, b);
        },
        bounds);
}
}  // namespace

int hr_search_dense_deep(hr_index* h, const float* q, int B, int k, int offset, const uint8_t* rowmask, int mask_on_device,
                         int64_t* out_ids, float* out_scores) {
    HR_TRY(check_deep_args(h, B, k, offset, true));
    HR_TRY(check_dense_deep_buffers(h, q, B, out_ids, out_scores));
    return dense_deep_host(h, q, B, k, offset, rowmask, mask_on_device, out_ids, out_scores, nullptr);
}

int hr_search_sparse_deep(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B, int k,
                          int offset, float drop_ratio, const uint8_t* rowmask, int mask_on_device, int64_t* out_ids,
                          float* out_scores) {
    HR_TRY(check_deep_args(h, B, k, offset, false));
    if (!q_indptr || !out_ids || !out_scores) return fail(h, HR_EINVAL, "null buffer");
    return sparse_deep_host(h, q_indptr, q_idx, q_val, B, k, offset, drop_ratio, rowmask, mask_on_device, out_ids, out_scores,
                            nullptr);
}

namespace {
// The cursor forms' operands -> the key interval of every query ([B][2], deep_key_interval), refused before anything is
// launched or written.  A cursor counts where all three arrays are given and has_after[b] is set; ids become rows here.
int deep_after_intervals(hr_index* h, int B, bool l2, const float* after_score, const int64_t* after_id, const uint8_t* has_after,
                         const float* radius, const float* range_filter, std::vector<unsigned long long>* out) {
    out->resize((size_t)B * 2);
    const bool cursors = after_score && after_id && has_after;
    for (int b = 0; b < B; ++b) {
        const float r = radius ? radius[b] : (l2 ? INFINITY : -INFINITY);
        const float f = range_filter ? range_filter[b] : (l2 ? -INFINITY : INFINITY);
        if (std::isnan(r) || std::isnan(f)) return fail(h, HR_EINVAL, "NaN range bound in query %d", b);
        if (l2 ? f >= r : r >= f)
            return fail(h, HR_EINVAL, "empty range in query %d: radius %g, range_filter %g (%s)", b, (double)r, (double)f,
                        l2 ? "L2 keeps range_filter <= distance < radius" : "kept are radius < score <= range_filter");
        const bool has = cursors && has_after[b];
        float s = 0.f;
        int64_t row = 0;
        if (has) {
            if (!std::isfinite(after_score[b])) return fail(h, HR_EINVAL, "non-finite after_score in query %d", b);
            s = l2 ? -after_score[b] : after_score[b];
            if (__builtin_sub_overflow(after_id[b], h->row_offset, &row)) row = after_id[b] < 0 ? -1 : INT64_MAX;
        }
        deep_key_interval(has, s, row, l2 ? -r : r, l2 ? -f : f, out->data() + (size_t)b * 2);
    }
    return HR_OK;
}
}  // namespace

int hr_search_dense_deep_after(hr_index* h, const float* q, int B, int k, const float* after_score, const int64_t* after_id,
                               const uint8_t* has_after, const float* radius, const float* range_filter, const uint8_t* rowmask,
                               int mask_on_device, int64_t* out_ids, float* out_scores) {
    HR_TRY(check_deep_args(h, B, k, 0, true));
    HR_TRY(check_dense_deep_buffers(h, q, B, out_ids, out_scores));
    std::vector<unsigned long long> bounds;
    HR_TRY(deep_after_intervals(h, B, h->metric == HR_METRIC_L2, after_score, after_id, has_after, radius, range_filter, &bounds));
    return dense_deep_host(h, q, B, k, 0, rowmask, mask_on_device, out_ids, out_scores, bounds.data());
}

int hr_search_sparse_deep_after(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B, int k,
                                const float* after_score, const int64_t* after_id, const uint8_t* has_after, float drop_ratio,
                                const uint8_t* rowmask, int mask_on_device, int64_t* out_ids, float* out_scores) {
    HR_TRY(check_deep_args(h, B, k, 0, false));
    if (!q_indptr || !out_ids || !out_scores) return fail(h, HR_EINVAL, "null buffer");
    std::vector<unsigned long long> bounds;
    HR_TRY(deep_after_intervals(h, B, false, after_score, after_id, has_after, nullptr, nullptr, &bounds));
    return sparse_deep_host(h, q_indptr, q_idx, q_val, B, k, 0, drop_ratio, rowmask, mask_on_device, out_ids, out_scores,
                            bounds.data());
}

int hr_fuse_rrf(hr_index* h, const int64_t* ids_a, int na, const int64_t* ids_b, int nb, const int64_t* ids_c, int nc,
                double wa, double wb, double wc, int rrf_k, int64_t* out_ids, double* out_scores, int32_t* out_methods,
                int32_t* n_out) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (na < 0 || nb < 0 || nc < 0 || na + nb + nc == 0) {
        if (n_out) *n_out = 0;
        return (na < 0 || nb < 0 || nc < 0) ? fail(h, HR_EINVAL, "negative list length") : HR_OK;
    }
    if (na > HR_MAX_TOPK || nb > HR_MAX_TOPK || nc > HR_MAX_TOPK)
        return fail(h, HR_ELIMIT, "list longer than HR_MAX_TOPK=%d", HR_MAX_TOPK);
    if (!out_ids || !out_scores || !out_methods || !n_out) return fail(h, HR_EINVAL, "null buffer");
    DeviceGuard dg(h->device);
    PooledWs pooled(h);
    Workspace* ws = pooled.w;
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    hipStream_t s = ws->stream;
    const int total = na + nb + nc;
    const int ka = std::max(na, 1);  // kernel wants a readable first list
    std::vector<int64_t> staged((size_t)ka + nb + nc, -1);
    if (na) std::memcpy(staged.data(), ids_a, (size_t)na * 8);
    if (nb) std::memcpy(staged.data() + ka, ids_b, (size_t)nb * 8);
    if (nc) std::memcpy(staged.data() + ka + nb, ids_c, (size_t)nc * 8);
    HIP_TRY(h, ws->f_ids.ensure(staged.size() * 8));
    HIP_TRY(h, ws->f_out_ids.ensure((size_t)total * 8));
    HIP_TRY(h, ws->f_out_scores.ensure((size_t)total * 8));
    HIP_TRY(h, ws->f_out_meth.ensure((size_t)total * 4));
    HIP_TRY(h, ws->f_n.ensure(4));
    HIP_TRY(h, hipMemcpyAsync(ws->f_ids.p, staged.data(), staged.size() * 8, hipMemcpyHostToDevice, s));
    int64_t* d = ws->f_ids.as<int64_t>();
    HR_TRY(hr_fuse_rrf_dev(d, ka, nb ? d + ka : nullptr, nb, nc ? d + ka + nb : nullptr, nc, 1, wa, wb, wc, rrf_k, total,
                           ws->f_out_ids.as<int64_t>(), ws->f_out_scores.as<double>(), ws->f_out_meth.as<int32_t>(),
                           ws->f_n.as<int32_t>(), s));
    HIP_TRY(h, hipMemcpyAsync(out_ids, ws->f_out_ids.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_scores, ws->f_out_scores.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_methods, ws->f_out_meth.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(n_out, ws->f_n.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return HR_OK;
}

int hr_fuse_scores(hr_index* h, const int64_t* ids_a, const float* sc_a, int na, int norm_a, const int64_t* ids_b,
                   const float* sc_b, int nb, int norm_b, const int64_t* ids_c, const float* sc_c, int nc, int norm_c,
                   double wa, double wb, double wc, int64_t* out_ids, double* out_scores, int32_t* out_methods,
                   int32_t* n_out) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    if (na < 0 || nb < 0 || nc < 0) return fail(h, HR_EINVAL, "negative list length");
    if (na > HR_MAX_TOPK || nb > HR_MAX_TOPK || nc > HR_MAX_TOPK)
        return fail(h, HR_ELIMIT, "list longer than HR_MAX_TOPK=%d", HR_MAX_TOPK);
    if ((na && (!ids_a || !sc_a)) || (nb && (!ids_b || !sc_b)) || (nc && (!ids_c || !sc_c)))
        return fail(h, HR_EINVAL, "null list or score buffer of a used list");
    const int norm[3] = {norm_a, norm_b, norm_c}, len[3] = {na, nb, nc};
    for (int m = 0; m < 3; ++m)
        if (len[m] && (norm[m] < HR_NORM_COSINE || norm[m] > HR_NORM_MINMAX_DIST))
            return fail(h, HR_EINVAL, "norm code %d of list %d is not one of HR_NORM_*", norm[m], m);
    if (na + nb + nc == 0) {
        if (n_out) *n_out = 0;
        return HR_OK;
    }
    if (!out_ids || !out_scores || !out_methods || !n_out) return fail(h, HR_EINVAL, "null buffer");
    DeviceGuard dg(h->device);
    PooledWs pooled(h);
    Workspace* ws = pooled.w;
    if (!ws) return fail(h, HR_ENOMEM, "workspace allocation failed");
    hipStream_t s = ws->stream;
    const int total = na + nb + nc;
    const int ka = std::max(na, 1);  // kernel wants a readable first list
    std::vector<int64_t> staged((size_t)ka + nb + nc, -1);
    std::vector<float> staged_sc(staged.size(), 0.f);
    if (na) std::memcpy(staged.data(), ids_a, (size_t)na * 8), std::memcpy(staged_sc.data(), sc_a, (size_t)na * 4);
    if (nb) std::memcpy(staged.data() + ka, ids_b, (size_t)nb * 8), std::memcpy(staged_sc.data() + ka, sc_b, (size_t)nb * 4);
    if (nc) std::memcpy(staged.data() + ka + nb, ids_c, (size_t)nc * 8), std::memcpy(staged_sc.data() + ka + nb, sc_c, (size_t)nc * 4);
    HIP_TRY(h, ws->f_ids.ensure(staged.size() * 8));
    HIP_TRY(h, ws->f_sc.ensure(staged.size() * 4));
    HIP_TRY(h, ws->f_out_ids.ensure((size_t)total * 8));
    HIP_TRY(h, ws->f_out_scores.ensure((size_t)total * 8));
    HIP_TRY(h, ws->f_out_meth.ensure((size_t)total * 4));
    HIP_TRY(h, ws->f_n.ensure(4));
    HIP_TRY(h, hipMemcpyAsync(ws->f_ids.p, staged.data(), staged.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(ws->f_sc.p, staged_sc.data(), staged.size() * 4, hipMemcpyHostToDevice, s));
    int64_t* d = ws->f_ids.as<int64_t>();
    float* ds = ws->f_sc.as<float>();
    HR_TRY(hr_fuse_scores_dev(d, ds, ka, na ? norm_a : HR_NORM_COSINE, nb ? d + ka : nullptr, nb ? ds + ka : nullptr, nb, norm_b,
                              nc ? d + ka + nb : nullptr, nc ? ds + ka + nb : nullptr, nc, norm_c, 1, wa, wb, wc, nullptr,
                              total, ws->f_out_ids.as<int64_t>(), ws->f_out_scores.as<double>(),
                              ws->f_out_meth.as<int32_t>(), ws->f_n.as<int32_t>(), s));
    HIP_TRY(h, hipMemcpyAsync(out_ids, ws->f_out_ids.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_scores, ws->f_out_scores.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_methods, ws->f_out_meth.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(n_out, ws->f_n.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return HR_OK;
}

// ---- measurement hooks -----------------------------------------------------------------
int hr_set_profiling(hr_index* h, int enabled) {
    if (!h) return fail(nullptr, HR_EINVAL, "null handle");
    h->profiling = enabled;
    return HR_OK;
}

#ifdef HR_STAMP
HR_API int hr_debug_finish_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(hbmrag::hr_finish_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
HR_API int hr_debug_gemm_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(hbmrag::hr_gemm_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif
int hr_last_compact_ms(hr_index* h, float* out_ms, int n) {
    if (!h || !out_ms || n < 3) return fail(h, HR_EINVAL, "need a handle and room for 3 values");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    for (int i = 0; i < 3; ++i) out_ms[i] = h->compact_ms[i];
    return HR_OK;
}

int hr_last_kernel_ms(hr_index* h, float* out_ms, int n) {
    if (!h || !out_ms || n < 2 * PH_COUNT) return fail(h, HR_EINVAL, "need room for %d floats", 2 * PH_COUNT);
    DeviceGuard dg(h->device);
    std::lock_guard<std::mutex> g(h->prof_mu);
    double sum[PH_COUNT] = {0};
    int cnt[PH_COUNT] = {0};
    for (auto& sp : h->spans) {
        float ms = 0.f;
        if (hipEventSynchronize(sp.b) == hipSuccess && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            sum[sp.phase] += ms;
            cnt[sp.phase] += 1;
        }
        h->event_pool.push_back(sp.a);
        h->event_pool.push_back(sp.b);
    }
    h->spans.clear();
    // out[0..8] = mean ms per launch of each phase, out[9..17] = launches averaged
    for (int p = 0; p < PH_COUNT; ++p) {
        out_ms[p] = cnt[p] ? (float)(sum[p] / cnt[p]) : 0.f;
        out_ms[PH_COUNT + p] = (float)cnt[p];
    }
    return HR_OK;
}

}  // extern "C"
