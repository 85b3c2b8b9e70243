// evplp_group: the multi-GPU entry of the C ABI (SURVEY 8b "Threading", 8e).  n contexts -- one per GPU of the node -- own interleaved
// row strips of the image (include/evplp.h); the scene and the BVH are replicated; large light-path sets are traced 1/n per rank and
// shared by an in-place all-gather of the record buffers; every rank gathers / splats its own rows; the composited strips are
// all-gathered so that every GPU holds the frame.  No other exchange exists on the path.  The collectives are RCCL (ncclAllGather over
// xGMI, one communicator per GPU; the library is opened at run time so that hosts without it can still use single contexts).  Ranks that
// share one device ("virtual ranks": tests, single-GPU boxes) exchange by device-to-device copies instead.
//
// EVPLP_PARTITION_ITERATIONS shares out the ITERATIONS of a progressive run instead of the image: every rank is a whole-image context,
// the single-rank pass calls go to the rank evplp_group_select_rank chose, and a written frame is the rank-order sum of the ranks'
// accumulators, formed on every GPU by reduce_shards_kernel (kernels_splat.hip) -- from an all-gather into a staging buffer (RCCL) or
// straight from the peers' planes (virtual ranks).
//
// (round 5) ONE WORKER THREAD PER RANK.  Until round 4 the caller's thread issued every rank's launches in turn: at eight ranks that is
// ~50 enqueue calls per iteration against config #4's 0.15-0.6 ms iteration -- the host, not the GPUs, would have set that
// configuration's pace.  Now a group call only POSTS a small task to each rank's single-producer ring (host/cmd_ring.hpp: no lock taken by a
// waiting party, no system call while the workers are awake) and returns; every worker is bound to its device, runs its rank's calls in
// order -- waits for a photon splat's verdict included: nobody else waits with it -- and issues its rank's side of a collective itself
// (RCCL's one-thread-per-GPU model).  Per-pixel results do not depend on any of this: the same calls reach every context in the same order.
//   * errors are sticky: the first failing call of a rank is kept, every later command of that rank is skipped, and the next group call
//     (at the latest evplp_group_synchronize / evplp_group_resolve) returns it;
//   * every worker meets the others at a host-side barrier in front of a collective and looks at the group's failure flag THERE, so that
//     either all ranks enter the collective or none does;
//   * a call made directly on a rank's context (evplp_group_context: statistics, buffers) first waits until that rank's worker has
//     nothing queued (evplp_context::quiesce).
#include "context.hpp"
#include "host/cmd_ring.hpp"

#include <rccl/rccl.h>      // types only: the entry points are resolved with dlsym

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace evplp {
int resolve_to_device(evplp_context *c, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, bool settle, bool as_pass);   // context.cpp
int settle(evplp_context *c);                                                                                                  // context.cpp
int frame_error_rows(evplp_context *c);                                                                                        // context.cpp
void place_row_errors(const evplp_context *c, const std::vector<RowError> &local, std::vector<RowError> &rows, std::vector<char> &held);   // context.cpp
}

struct evplp_group;
namespace {
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool open(std::string &err) {
        for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) { lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) { err = std::string("cannot open RCCL (librccl.so.1): ") + dlerror(); return false; }
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll"); CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        AllGather = (decltype(AllGather))dlsym(lib, "ncclAllGather"); GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !AllGather || !GetErrorString) { err = "librccl lacks an expected entry point"; return false; }
        return true;
    }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Worker;
// One posted call: what the rank's worker does, with the call's arguments captured by name (plain data; pointers must stay valid until the
// caller has drained: load_scene, set_proxy, resolve do).  The largest state is a gather's: the frame params and the kind.
constexpr size_t kTaskBytes = 96;
using Task = evplp::Task<Worker, kTaskBytes>;
static_assert(sizeof(Task) <= 176, "a ring slot (120 B) stays within the 176 B of the positional command record it replaced");
using evplp::SpinBarrier;
struct Worker {
    evplp_group *g = nullptr; int rank = 0;
    evplp_context *c = nullptr;                       // the rank's context
    std::thread th;
    evplp::Ring<Task> ring;
    std::atomic<int> status{ 0 };                     // first failing call's status (sticky)
    char error[512] = "";
    // host time of this worker (evplp_group_host_stats): inside its rank's enqueue calls / inside exchanges (barriers, copies, collectives)
    double t_calls = 0.0, t_exchange = 0.0; uint64_t n_cmds = 0;
    bool ok() const { return status.load(std::memory_order_relaxed) == 0; }
    void fail(int rc, const char *msg);
    void hip_fail(hipError_t e) { (void)hipGetLastError(); fail(e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP, hipGetErrorString(e)); }
};
} // namespace

struct evplp_group {
    int n = 0;
    std::vector<evplp_context *> ctx;
    std::vector<int> device;
    bool virtual_ranks = false;             // all ranks on one device: exchange by copies
    Rccl rccl; std::vector<ncclComm_t> comms;
    std::vector<float *> d_frame;           // per rank: [n][local_rows * W * 3] the all-gathered composite
    float *d_assembled = nullptr;           // rank 0's device: [H][W][3] the frame in image order (evplp_group_resolve)
    size_t strip_floats = 0;                // local_rows * W * 3
    bool split_paths = false; uint32_t per_rank_paths = 0;
    // EVPLP_PARTITION_STRIPS: the blocks as dealt (evplp_group_rebalance); empty = block b belongs to rank b % n
    std::vector<int32_t> owner;             // [image blocks] rank
    uint32_t *d_owner = nullptr;            // rank 0's device: [image blocks] rank << 16 | local block (assemble_strips_kernel)
    int strip_rows = 16, image_blocks = 0, cap_blocks = 0;
    size_t strip_floats_cap = 0;            // d_frame's chunk size (the capacity); strip_floats <= it is what an exchange moves
    // EVPLP_PARTITION_ITERATIONS: every rank renders whole frames; the pass calls go to `selected`; a present with exchange / a resolve sums
    // the ranks' planes (worker_reduce).  sums_fresh (caller's thread): no pass was posted since the last reduction -- the cached sums still hold
    bool iterations = false; int selected = 0; bool sums_fresh = false;
    bool have_reference = false;            // evplp_group_set_error_reference has given every rank an image (caller's thread)
    bool noise_on = false;                  // evplp_group_noise_track is on on every rank (caller's thread)
    bool adapt_on = false;                  // evplp_group_adaptive_enable is on on every rank (caller's thread)
    bool adapt_pt = false;                  // ... and in path-trace mode (evplp_group_adaptive_enable_pt)
    bool adapt_budget = false;              // budget mode (on = 2), the path tracer's or the gathers'
    bool adapt_gather_budget = false;       // ... the gathers' (evplp_group_adaptive_enable(g, 2))
    uint64_t pt_batch_cap = 1ull << 30;     // evplp_group_path_trace_batch_scratch: every rank's bound (caller's thread)
    // EVPLP_PARTITION_ITERATIONS, evplp_group_noise_*: rank 0's pooled moments (Q then S, [3][stride] fp64 each) and K / B summed over the
    // ranks (written by rank 0's worker); RCCL only: per rank [n][noise_bytes] every rank's NoisePlanes (all-gathered)
    double *d_noise_pool = nullptr; double pool_k = 0.0, pool_b = 0.0;
    std::vector<char *> d_noise_stage;
    // evplp_group_denoise.  Strips: per rank [n][chunk rows * W] packed pixels (kernels.h DenoisePixel) all-gathered from the ranks, and rank 0's
    // assembled frame [H * W].  Iterations: last_primary = the rank the last evplp_group_primary went to (caller's thread), and on rank 0 the
    // four G-buffer planes copied from it when it is another device ([4][plane_px])
    std::vector<float *> d_dn_recv;
    evplp::DenoisePixel *d_dn_frame = nullptr;
    int last_primary = 0;
    float4 *d_dn_guides = nullptr;
    // evplp_group_denoise_temporal (temporal_on: enabled on every rank; caller's thread).  Strips: per rank [n][chunk rows * W] previous-pose
    // texels (kernels.h TemporalPrev) all-gathered beside the packed pixels; rank 0 assembles them into its context's d_tp_prev_frame and keeps
    // the history in image layout (its context's d_tp_hist), so a rebalance between two frames does not disturb it.  Iterations: rank 0 reads
    // the texels of the rank of the last primary.
    bool temporal_on = false;
    std::vector<float *> d_tp_recv;
    size_t plane_px = 0;                    // W * local_rows: the pixels of one accumulator plane
    std::vector<float4 *> d_sum;            // per rank: [3][plane_px] VPL, photon and light planes reduced over the ranks (the first reduction)
    std::vector<float4 *> d_stage;          // per rank, RCCL only: [n][plane_px] one plane of every rank (all-gathered)
    std::vector<int> num_cus;               // per rank: the reduction's grid
    std::vector<Worker *> workers;
    SpinBarrier barrier;
    std::atomic<int> failed{ 0 };           // some rank has failed: collectives are skipped by everybody
    char error[512] = "";
    void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(error, sizeof(error), fmt, ap); va_end(ap); }
};

static thread_local char g_group_create_error[512] = "";

// ------------------------------------------------------------------------------------------------ the workers
void Worker::fail(int rc, const char *msg) {
    int expected = 0;
    if (status.compare_exchange_strong(expected, rc)) { std::snprintf(error, sizeof(error), "%s", msg ? msg : ""); g->failed.store(1, std::memory_order_release); }
}
// all-gather of equal chunks, this rank's side: it contributes `count` floats at all_send[rank] and receives n * count floats at `recv`
static void worker_all_gather(Worker *w, float *recv, size_t count, const std::vector<const float *> &all_send) {
    evplp_group *g = w->g; evplp_context *c = g->ctx[(size_t)w->rank];
    const float *send = all_send[(size_t)w->rank];
    if (g->n == 1 && g->virtual_ranks) {       // one rank: its chunk goes to its place in stream order, the host does not wait
        if (w->ok() && recv != send) {
            hipError_t e = hipMemcpyAsync(recv, send, count * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) w->fail(EVPLP_ERR_HIP, hipGetErrorString(e));
        }
        return;
    }
    // everybody arrives, then everybody gets the SAME answer to "has somebody failed": all enter the collective or none (the barrier's last
    // arriver reads the flag once for all; a rank that reads it for itself could see a failure its peers, already past the barrier, raised
    // in their NEXT command and skip a collective they have entered)
    if (g->barrier.wait(&g->failed) != 0) return;
    if (!g->virtual_ranks) {
        ncclResult_t nr = g->rccl.AllGather(send, recv, count, ncclFloat, g->comms[(size_t)w->rank], c->stream);
        if (nr != ncclSuccess) w->fail(EVPLP_ERR_HIP, g->rccl.GetErrorString(nr));
        return;
    }
    // virtual ranks share a device: every producer finishes, then plain device copies on the receiver's stream; the producers' buffers
    // may be overwritten by their next pass only after every receiver has its copy
    hipError_t e = hipStreamSynchronize(c->stream);
    g->barrier.wait();
    for (int q = 0; q < g->n && e == hipSuccess; q++) {
        float *dst = recv + (size_t)q * count;
        if (dst != all_send[(size_t)q]) e = hipMemcpyAsync(dst, all_send[(size_t)q], count * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    g->barrier.wait();
    if (e != hipSuccess) w->fail(EVPLP_ERR_HIP, hipGetErrorString(e));
}
// The collectives a command can end in (its `always` stage: reached by every rank, failed or not).  Every rank's source, this rank's destination:
// the composited strips (a present, the strips' variance) ...
static void exchange_strips(Worker &w) {
    evplp_group *g = w.g;
    std::vector<const float *> all((size_t)g->n);
    for (int q = 0; q < g->n; q++) all[(size_t)q] = g->ctx[(size_t)q]->d_rgb;
    worker_all_gather(&w, g->d_frame[(size_t)w.rank], g->strip_floats, all);
}
// ... the split light paths' records, in place: rank q's slice lies at offset q * chunk of its record buffer ...
static void exchange_records(Worker &w) {
    evplp_group *g = w.g;
    std::vector<const float *> all((size_t)g->n);
    const size_t chunk = (size_t)g->per_rank_paths * w.c->cfg.photons_per_path * (sizeof(evplp_record) / sizeof(float));
    for (int q = 0; q < g->n; q++) all[(size_t)q] = (const float *)g->ctx[(size_t)q]->buf[EVPLP_BUF_RECORDS] + (size_t)q * chunk;
    worker_all_gather(&w, (float *)w.c->buf[EVPLP_BUF_RECORDS], chunk, all);
}
// ... and the denoiser's packed pixels of the rows an exchange moves, with their previous-pose texels when the call is temporal
static void exchange_denoise(Worker &w, bool temporal) {
    evplp_group *g = w.g;
    std::vector<const float *> all((size_t)g->n);
    for (int q = 0; q < g->n; q++) all[(size_t)q] = (const float *)g->ctx[(size_t)q]->d_dn_pack;
    worker_all_gather(&w, g->d_dn_recv[(size_t)w.rank], g->strip_floats / 3 * evplp::kDenoiseFloats, all);
    if (!temporal) return;
    for (int q = 0; q < g->n; q++) all[(size_t)q] = (const float *)g->ctx[(size_t)q]->d_tp_prev;
    worker_all_gather(&w, g->d_tp_recv[(size_t)w.rank], g->strip_floats / 3 * evplp::kTemporalPrevFloats, all);
}

// EVPLP_PARTITION_ITERATIONS: the three accumulator planes of every rank summed -- VPL and photon in rank order in fp32, light as the first
// non-zero pixel in rank order -- into this rank's d_sum, then composited from there.  exchange = false: no pass since the last reduction, the
// cached sums are composited again and nothing is exchanged.  The planes are read through the contexts' CURRENT buffer pointers.
static const int kSumPlanes[3] = { EVPLP_BUF_VPL_ACCUM, EVPLP_BUF_PHOTON_ACCUM, EVPLP_BUF_LIGHT };
static void worker_reduce(Worker *w, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, bool exchange) {
    evplp_group *g = w->g; const int r = w->rank; evplp_context *c = w->c;
    const size_t px = g->plane_px;
    const double t0 = now_ms();
    if (exchange && w->ok()) {
        const int rc = evplp::settle(c);                   // (the sums must be exact: every splat has its verdict, a re-run is enqueued)
        if (rc < 0) w->fail(rc, evplp_last_error(c));
        hipError_t e = hipSuccess;
        if (w->ok() && !g->d_sum[(size_t)r]) e = hipMalloc((void **)&g->d_sum[(size_t)r], sizeof(float4) * 3 * px);
        if (e == hipSuccess && w->ok() && !g->virtual_ranks && !g->d_stage[(size_t)r]) e = hipMalloc((void **)&g->d_stage[(size_t)r], sizeof(float4) * (size_t)g->n * px);
        if (e != hipSuccess) w->hip_fail(e);
    }
    if (!exchange && w->ok() && !g->d_sum[(size_t)r]) w->fail(EVPLP_ERR_INVALID, "evplp_group_resolve: no reduction to composite");
    const double t1 = now_ms();
    if (exchange) {            // (reached by every rank, failed or not: the barrier decides for all)
        float4 *sum = g->d_sum[(size_t)r];
        evplp::ShardPlanes src; std::memset(&src, 0, sizeof(src));
        if (g->n == 1 && g->virtual_ranks) {               // one rank: its planes, copied in stream order
            if (w->ok()) for (int k = 0; k < 3; k++) {
                src.p[0] = (const float4 *)c->buf[kSumPlanes[k]];
                evplp::launch_reduce_shards(src, 1, k == 2, px, sum + (size_t)k * px, g->num_cus[(size_t)r], c->stream);
            }
        } else if (g->virtual_ranks) {
            // every rank's planes are final when its stream is idle; nobody writes them again before every reader has finished (second barrier)
            hipError_t e = w->ok() ? hipStreamSynchronize(c->stream) : hipSuccess;
            if (e != hipSuccess) w->hip_fail(e);
            if (g->barrier.wait(&g->failed) == 0) {
                for (int k = 0; k < 3; k++) {
                    for (int q = 0; q < g->n; q++) src.p[q] = (const float4 *)g->ctx[(size_t)q]->buf[kSumPlanes[k]];
                    evplp::launch_reduce_shards(src, g->n, k == 2, px, sum + (size_t)k * px, g->num_cus[(size_t)r], c->stream);
                }
                e = hipGetLastError();
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                g->barrier.wait();
                if (e != hipSuccess) w->hip_fail(e);
            }
        } else if (g->barrier.wait(&g->failed) == 0) {
            // distinct devices: one plane at a time all-gathered into the staging buffer, then reduced from there (stream order; no
            // ncclAllReduce: its association is not fixed)
            float4 *stage = g->d_stage[(size_t)r];
            for (int q = 0; q < g->n; q++) src.p[q] = stage + (size_t)q * px;
            for (int k = 0; k < 3; k++) {
                ncclResult_t nr = g->rccl.AllGather(c->buf[kSumPlanes[k]], stage, px * 4, ncclFloat, g->comms[(size_t)r], c->stream);
                if (nr != ncclSuccess) w->fail(EVPLP_ERR_HIP, g->rccl.GetErrorString(nr));
                evplp::launch_reduce_shards(src, g->n, k == 2, px, sum + (size_t)k * px, g->num_cus[(size_t)r], c->stream);
            }
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) w->hip_fail(e);
        }
        w->t_exchange += now_ms() - t1;
    }
    const double t2 = now_ms();
    if (w->ok()) {
        const float4 *sum = g->d_sum[(size_t)r];
        evplp::launch_resolve(c->st, sum, sum + px, sum + 2 * px, vs, ps, ls, mask_emitter, gamma, c->d_rgb, c->stream);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) w->hip_fail(e);
    }
    w->t_calls += (t1 - t0) + (now_ms() - t2); w->n_cmds++;
}

// EVPLP_PARTITION_ITERATIONS, evplp_group_noise_estimate / _variance: every rank's moments pooled on rank 0 -- Q and S summed in rank order
// (noise_pool_kernel, once per rank), K and B summed -- the way worker_reduce moves the accumulators: virtual ranks are read where they are,
// distinct devices all-gather their NoisePlanes into a staging buffer first.
static void worker_noise_pool(Worker *w) {
    evplp_group *g = w->g; const int r = w->rank; evplp_context *c = w->c;
    const double t0 = now_ms();
    const size_t px = g->plane_px, stride = c->noise_stride, bytes = evplp::noise_bytes(c);
    hipError_t e = hipSuccess;
    if (w->ok() && r == 0 && !g->d_noise_pool) e = hipMalloc((void **)&g->d_noise_pool, sizeof(double) * 6 * stride);
    if (e == hipSuccess && w->ok() && !g->virtual_ranks && !g->d_noise_stage[(size_t)r]) e = hipMalloc((void **)&g->d_noise_stage[(size_t)r], bytes * (size_t)g->n);
    if (e != hipSuccess) w->hip_fail(e);
    // rank 0, behind every rank's last command: K, B and the n launches, src(q) = rank q's moments
    auto pool = [&](auto src) {
        double k = 0.0, b = 0.0;
        for (int q = 0; q < g->n; q++) {
            k += (double)g->ctx[(size_t)q]->noise_k; b += (double)g->ctx[(size_t)q]->noise_b;
            evplp::launch_noise_pool(src(q), q == 0, g->d_noise_pool, g->d_noise_pool + 3 * stride, px, c->stream);
        }
        g->pool_k = k; g->pool_b = b;
        hipError_t le = hipGetLastError();
        if (le != hipSuccess) w->hip_fail(le);
    };
    if (g->n == 1 && g->virtual_ranks) { if (w->ok()) pool([&](int) { return evplp::noise_moments_of(c); }); }
    else if (g->virtual_ranks) {
        // every rank's planes are final when its stream is idle; nobody folds again before rank 0 has read them (second barrier)
        e = w->ok() ? hipStreamSynchronize(c->stream) : hipSuccess;
        if (e != hipSuccess) w->hip_fail(e);
        if (g->barrier.wait(&g->failed) == 0) {
            if (r == 0) {
                pool([&](int q) { return evplp::noise_moments_of(g->ctx[(size_t)q]); });
                e = hipStreamSynchronize(c->stream);
                if (e != hipSuccess) w->hip_fail(e);
            }
            g->barrier.wait();
        }
    } else if (g->barrier.wait(&g->failed) == 0) {
        // distinct devices: the whole NoisePlanes allocation of every rank, all-gathered (stream order), then rank 0 pools from the stage
        char *stage = g->d_noise_stage[(size_t)r];
        ncclResult_t nr = g->rccl.AllGather(c->d_noise, stage, bytes / sizeof(float), ncclFloat, g->comms[(size_t)r], c->stream);
        if (nr != ncclSuccess) w->fail(EVPLP_ERR_HIP, g->rccl.GetErrorString(nr));
        else if (r == 0) pool([&](int q) {
            const double *sq = (const double *)(stage + (size_t)q * bytes);
            const float4 *prev = (const float4 *)(sq + 3 * stride);
            return evplp::NoiseMoments{ sq, nullptr, prev, prev + px, stride };
        });
    }
    w->t_exchange += now_ms() - t0; w->n_cmds++;
}

static evplp::NoiseMoments noise_pooled(const evplp_group *g, const evplp_context *c0) {
    return evplp::NoiseMoments{ g->d_noise_pool, g->d_noise_pool + 3 * c0->noise_stride, nullptr, nullptr, c0->noise_stride };
}
// this context's previous-pose texels (zeros on a first call), stream order
static int worker_temporal_pose(evplp_context *c) {
    if (c->tp_frames > 0) return evplp::temporal_prev_pose(c);
    const hipError_t e = hipMemsetAsync(c->d_tp_prev, 0, sizeof(evplp::TemporalPrev) * (size_t)c->st.W * c->st.local_rows, c->stream);
    if (e != hipSuccess) { c->set_error("evplp_group_denoise_temporal: %s", hipGetErrorString(e)); return EVPLP_ERR_HIP; }
    return EVPLP_OK;
}
// evplp_group_denoise.  Strips (every rank, then exchange_denoise): this rank's variance, composite and packed pixels.
// Iterations (rank 0, behind the pooled variance and the reduction): the packed pixels of the reduced composite and light plane with the
// guides of rank guides_rank, copied to rank 0's device first when that is another GPU.
static int worker_denoise_prep(Worker *w, float scale, float ls, int32_t mask_emitter, bool temporal, int guides_rank) {
    evplp_group *g = w->g; evplp_context *c = w->c;
    const float4 *gb[4]; const float4 *light;
    int rc;
    if (!g->iterations) {
        if ((rc = evplp::noise_variance_to_device(c, evplp::noise_moments_of(c), (double)c->noise_k, (double)c->noise_b, scale)) < 0) return rc;
        if ((rc = evplp::denoise_keep_variance(c)) < 0) return rc;
        if ((rc = evplp::resolve_to_device(c, scale, scale, ls, mask_emitter, 0, true, false)) < 0) return rc;
        for (int k = 0; k < 4; k++) gb[k] = (const float4 *)c->buf[EVPLP_BUF_GBUF_POSITION + k];
        light = (const float4 *)c->buf[EVPLP_BUF_LIGHT];
    } else {
        const evplp_context *src = g->ctx[(size_t)guides_rank];
        const size_t px = g->plane_px;
        for (int k = 0; k < 4; k++) gb[k] = (const float4 *)src->buf[EVPLP_BUF_GBUF_POSITION + k];
        if (src != c && g->device[(size_t)guides_rank] != g->device[0]) {
            hipError_t e = hipSuccess;
            if (!g->d_dn_guides) e = hipMalloc((void **)&g->d_dn_guides, sizeof(float4) * 4 * px);
            for (int k = 0; k < 4 && e == hipSuccess; k++)
                e = hipMemcpyPeerAsync(g->d_dn_guides + (size_t)k * px, g->device[0], gb[k], g->device[(size_t)guides_rank], sizeof(float4) * px, c->stream);
            if (e != hipSuccess) { (void)hipGetLastError(); c->set_error("evplp_group_denoise: guides of rank %d: %s", guides_rank, hipGetErrorString(e)); return EVPLP_ERR_HIP; }
            for (int k = 0; k < 4; k++) gb[k] = g->d_dn_guides + (size_t)k * px;
        }
        light = g->d_sum[0] + 2 * px;
    }
    rc = evplp::denoise_prepare(c, gb[0], gb[1], gb[2], gb[3], light);
    if (rc >= 0 && temporal && !g->iterations) rc = worker_temporal_pose(c);      // (evplp_group_denoise_temporal: this rank's rows on the previous pose)
    return rc;
}
// rank 0: the strips a rank's worker gathered (`gathered`: n chunks in rank order, `channels` floats per pixel) in image order
static void assemble_strips(const evplp_group *g, const float *gathered, float *frame, int channels = 3) {
    const evplp_context *c = g->ctx[0];
    evplp::launch_assemble_strips(c->st, g->n, g->owner.empty() ? nullptr : g->d_owner, (int)(g->strip_floats / ((size_t)c->st.W * 3)), gathered, frame, c->stream, channels);
}
// rank 0: the frame of packed pixels (strips: assembled from the all-gathered rows), the accumulation stage of evplp_group_denoise_temporal
// (iterations: on the texels of rank texels_rank), the passes, the frame to the caller (out_rgb)
static int worker_denoise_filter(Worker *w, evplp::DenoiseSettings ds, bool temporal, evplp::TemporalSettings ts, int texels_rank, float *out_rgb) {
    evplp_group *g = w->g; evplp_context *c = w->c;
    const size_t frame_px = (size_t)c->st.W * c->st.H;
    const evplp::DenoisePixel *frame = c->d_dn_pack;
    int rows = c->st.local_rows;
    float *out = c->d_rgb;
    hipError_t e = hipSuccess;
    if (!g->iterations) {
        if (!g->d_dn_frame) e = hipMalloc((void **)&g->d_dn_frame, sizeof(evplp::DenoisePixel) * frame_px);
        if (e == hipSuccess && !g->d_assembled) e = hipMalloc((void **)&g->d_assembled, sizeof(float) * 3 * frame_px);
        if (e != hipSuccess) { (void)hipGetLastError(); c->set_error("evplp_group_denoise: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP; }
        assemble_strips(g, g->d_dn_recv[0], (float *)g->d_dn_frame, evplp::kDenoiseFloats);
        frame = g->d_dn_frame; rows = c->st.H; out = g->d_assembled;
    }
    int rc;
    if (temporal) {            // the accumulation stage in front of the passes
        const evplp::TemporalPrev *prev = c->d_tp_prev;
        if (!g->iterations) {
            if (!c->d_tp_prev_frame) e = hipMalloc((void **)&c->d_tp_prev_frame, sizeof(evplp::TemporalPrev) * frame_px);
            if (e != hipSuccess) { (void)hipGetLastError(); c->d_tp_prev_frame = nullptr; c->set_error("evplp_group_denoise_temporal: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP; }
            assemble_strips(g, g->d_tp_recv[0], (float *)c->d_tp_prev_frame, evplp::kTemporalPrevFloats);
            prev = c->d_tp_prev_frame;
        } else if (texels_rank != 0) {
            const evplp_context *src = g->ctx[(size_t)texels_rank];
            prev = src->d_tp_prev;
            if (g->device[(size_t)texels_rank] != g->device[0]) {
                e = hipMemcpyPeerAsync(c->d_tp_prev, g->device[0], src->d_tp_prev, g->device[(size_t)texels_rank], sizeof(evplp::TemporalPrev) * g->plane_px, c->stream);
                if (e != hipSuccess) { (void)hipGetLastError(); c->set_error("evplp_group_denoise_temporal: texels of rank %u: %s", (unsigned)texels_rank, hipGetErrorString(e)); return EVPLP_ERR_HIP; }
                prev = c->d_tp_prev;
            }
        }
        if ((rc = evplp::temporal_accumulate(c, const_cast<evplp::DenoisePixel *>(frame), prev, rows, ds, ts, c->bounding_radius)) < 0) return rc;
    }
    rc = evplp::denoise_filter(c, frame, rows, ds, c->bounding_radius, out);
    if (rc < 0) return rc;
    e = hipMemcpyAsync(out_rgb, out, sizeof(float) * 3 * frame_px, hipMemcpyDeviceToHost, c->stream);     // (rows 0 .. H - 1 in image order)
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->set_error("evplp_group_denoise: %s", hipGetErrorString(e)); return EVPLP_ERR_HIP; }
    return EVPLP_OK;
}

// ------------------------------------------------------------------------------------------------ a posted command
// `run(w)` is the rank's call: skipped when the rank has failed, its negative return is the rank's failure (with the context's message),
// its time goes to t_calls.  `always(w)` is the collective the command ends in, stated by the wrapper that posts it: EVERY rank reaches it,
// failed or not (the barrier inside decides for all), and its time goes to t_exchange -- which nothing else touches.
template <class Run> static double run_stage(Worker &w, const Run &run) {
    const double t0 = now_ms();
    if (w.ok()) { const int rc = run(w); if (rc < 0) w.fail(rc, evplp_last_error(w.c)); }
    const double t1 = now_ms();
    w.t_calls += t1 - t0; w.n_cmds++;
    return t1;
}
template <class Run> static Task command(Run run) { return Task([run](Worker &w) { run_stage(w, run); return 0; }); }
template <class Run, class Always> static Task command(Run run, Always always) {
    return Task([run, always](Worker &w) { const double t1 = run_stage(w, run); always(w); w.t_exchange += now_ms() - t1; return 0; });
}
// The commands that are posted from several places.  A rank's composite (as_pass = false: the one evplp_group_frame_error and
// evplp_group_noise_estimate measure); with `exchange` the strips are all-gathered behind it, so that every GPU holds the frame:
// the per-frame exchange of a run that presents every frame; nothing comes to the host.
static Task present(float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, bool settle, bool exchange, bool as_pass = true) {
    auto run = [=](Worker &w) { return evplp::resolve_to_device(w.c, vs, ps, ls, mask_emitter, gamma, settle || !w.c->aux_stream, as_pass); };
    return exchange ? command(run, exchange_strips) : command(run);
}
// the variance into the rank's d_rgb -- of its own moments, or (pooled: rank 0, behind noise_pool) of the ranks' pooled ones; keep: it is
// evplp_group_denoise's; exchange: all-gathered as a present's composite is
static Task noise_variance(float scale, bool pooled, bool keep, bool exchange) {
    auto run = [=](Worker &w) {
        evplp_context *c = w.c;
        int rc = pooled ? evplp::noise_variance_to_device(c, noise_pooled(w.g, c), w.g->pool_k, w.g->pool_b, scale)
                        : evplp::noise_variance_to_device(c, evplp::noise_moments_of(c), (double)c->noise_k, (double)c->noise_b, scale);
        if (rc >= 0 && keep) rc = evplp::denoise_keep_variance(c);
        return rc;
    };
    return exchange ? command(run, exchange_strips) : command(run);
}
static Task noise_pool() { return Task([](Worker &w) { worker_noise_pool(&w); return 0; }); }
static Task synchronize() { return command([](Worker &w) { return evplp_synchronize(w.c); }); }
// rank 0 puts the strips into image order on the device; one copy lands the frame in the caller's buffer (no host-side assembly: a run that
// writes every frame resolves every iteration)
static Task assemble(float *out_rgb) {
    return command([out_rgb](Worker &w) {
        evplp_group *g = w.g; evplp_context *c = w.c;
        hipSetDevice(g->device[0]);
        const size_t frame_floats = (size_t)c->st.W * c->st.H * 3;
        hipError_t e = hipSuccess;
        if (g->iterations) e = hipMemcpyAsync(out_rgb, c->d_rgb, frame_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream);   // (whole-image ranks: rows in image order)
        else if (!g->d_assembled) e = hipMalloc((void **)&g->d_assembled, sizeof(float) * frame_floats);
        if (e == hipSuccess && !g->iterations) {
            assemble_strips(g, g->d_frame[0], g->d_assembled);
            e = hipMemcpyAsync(out_rgb, g->d_assembled, frame_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) w.hip_fail(e);
        return EVPLP_OK;
    });
}

static void worker_main(Worker *w) {
    hipSetDevice(w->g->device[(size_t)w->rank]);
    w->ring.consume(*w);
}
static void post(Worker *w, const Task &task) { w->ring.post(task); }
static void drain(evplp_group *g) { for (Worker *w : g->workers) w->ring.drain(); }
static void quiesce_hook(void *arg) { ((Worker *)arg)->ring.drain(); }
// the sticky error of the group, if any: the lowest failing rank's
static int group_status(evplp_group *g) {
    for (Worker *w : g->workers) { const int st = w->status.load(std::memory_order_acquire); if (st < 0) { g->set_error("rank %d: %s", w->rank, w->error); return st; } }
    return EVPLP_OK;
}
// a failed group takes no new command: the workers finish what they have and the call reports the failure
static int post_all(evplp_group *g, const Task &task) {
    if (g->failed.load(std::memory_order_acquire)) { drain(g); return group_status(g); }
    for (Worker *w : g->workers) post(w, task);
    return EVPLP_OK;
}
static int post_one(evplp_group *g, int rank, const Task &task) {
    if (g->failed.load(std::memory_order_acquire)) { drain(g); return group_status(g); }
    post(g->workers[(size_t)rank], task);
    return EVPLP_OK;
}
// a pass call: every rank (strips), or the selected rank alone (EVPLP_PARTITION_ITERATIONS; the cached sums are stale from here on)
static int post_pass(evplp_group *g, const Task &task) {
    // (refused here, on the caller's thread, so that a forgotten refit is not a sticky worker failure; the flag only changes in calls that wait)
    if (g->ctx[0]->scene_dirty) { g->set_error("vertices were updated (evplp_group_update_mesh): call evplp_group_refit_accel, or evplp_build_accel on every rank, first"); return EVPLP_ERR_INVALID; }
    if (!g->iterations) return post_all(g, task);
    g->sums_fresh = false;
    return post_one(g, g->selected, task);
}
// calls whose arguments must outlive them, or whose result the caller needs: post, wait until every worker is idle, report
static int post_and_wait(evplp_group *g, const Task &task) {
    int rc = post_all(g, task);
    if (rc < 0) return rc;
    drain(g);
    return group_status(g);
}
// The mesh, refit and tree calls go to every rank (each holds the whole scene, in both partitions).  What the context refuses without
// touching a device is refused here first -- once the workers are idle, against rank 0's copy (the ranks' scenes are the same), with the
// context's own message -- so that a refusal is not a sticky worker failure.
template <class Check> static int rank0_refuses(evplp_group *g, Check check) {
    drain(g);
    if (check(g->ctx[0])) return EVPLP_OK;
    g->set_error("%s", g->ctx[0]->error);
    return EVPLP_ERR_INVALID;
}

struct Vec3 { float v[3]; };
#define GRP_CHECK(g) do { if (!(g)) return EVPLP_ERR_INVALID; } while (0)
// What a pass call can refuse without touching a device is refused HERE, on the caller's thread, at once -- as the plain context does -- and
// leaves the group usable; only failures of the device side are sticky.  (The configuration is the same on every rank and never changes.)
static int check_frame_params(evplp_group *g, const evplp_frame_params *fp, const char *name, bool splat) {
    const evplp_config &cf = g->ctx[0]->cfg;
    if (fp->photons_per_path != cf.photons_per_path || fp->num_light_paths != cf.num_light_paths || fp->num_vpl_light_paths > cf.num_vpl_light_paths) {
        g->set_error("%s: frame params disagree with the configuration (paths / photons per path)", name); return EVPLP_ERR_INVALID;
    }
    if (fp->mis_mode > 5u) { g->set_error("%s: mis_mode %u out of range", name, fp->mis_mode); return EVPLP_ERR_INVALID; }
    if (!splat && fp->num_vpl_light_paths == 0) { g->set_error("%s: num_vpl_light_paths is 0 (the reference disables the pass, rtcomphoton.h:200-203)", name); return EVPLP_ERR_INVALID; }
    if (splat && !(fp->photon_radius > 0.0f)) { g->set_error("%s: photon_radius must be > 0", name); return EVPLP_ERR_INVALID; }
    if (splat && fp->splat_footprint > (uint32_t)EVPLP_FOOTPRINT_PROXY) { g->set_error("%s: splat_footprint %u out of range", name, fp->splat_footprint); return EVPLP_ERR_INVALID; }
    return EVPLP_OK;
}

extern "C" const char *evplp_group_last_error(const evplp_group *g) { return g ? g->error : g_group_create_error; }
extern "C" int evplp_group_size(const evplp_group *g) { return g ? g->n : EVPLP_ERR_INVALID; }
extern "C" evplp_context *evplp_group_context(evplp_group *g, int32_t rank) {
    if (!g || rank < 0 || rank >= g->n) return nullptr;
    g->sums_fresh = false;                 // (the caller may write the accumulators through it)
    return g->ctx[(size_t)rank];
}
extern "C" int evplp_group_select_rank(evplp_group *g, int32_t rank) {
    GRP_CHECK(g);
    if (!g->iterations) { g->set_error("evplp_group_select_rank: the group shares out the image (strips): every pass runs on every rank"); return EVPLP_ERR_INVALID; }
    if (rank < 0 || rank >= g->n) { g->set_error("evplp_group_select_rank: rank %d out of range (%d ranks)", rank, g->n); return EVPLP_ERR_INVALID; }
    g->selected = rank;
    return EVPLP_OK;
}
extern "C" int evplp_group_synchronize_rank(evplp_group *g, int32_t rank) {
    GRP_CHECK(g);
    if (rank < 0 || rank >= g->n) { g->set_error("evplp_group_synchronize_rank: rank %d out of range (%d ranks)", rank, g->n); return EVPLP_ERR_INVALID; }
    const int rc = post_one(g, rank, synchronize());
    if (rc < 0) return rc;
    g->workers[(size_t)rank]->ring.drain();
    return group_status(g);
}
extern "C" int evplp_group_host_stats(evplp_group *g, int32_t rank, double out[3]) {
    GRP_CHECK(g);
    if (rank < 0 || rank >= g->n || !out) { g->set_error("evplp_group_host_stats: bad arguments"); return EVPLP_ERR_INVALID; }
    g->workers[(size_t)rank]->ring.drain();
    out[0] = g->workers[(size_t)rank]->t_calls; out[1] = g->workers[(size_t)rank]->t_exchange; out[2] = (double)g->workers[(size_t)rank]->n_cmds;
    return EVPLP_OK;
}

extern "C" int evplp_group_profile_passes(evplp_group *g, int32_t on) {
    GRP_CHECK(g);
    drain(g);                                                             // (the flag belongs to the workers' contexts: set between their commands)
    for (evplp_context *c : g->ctx) c->profile_passes = on != 0;
    return EVPLP_OK;
}

extern "C" void evplp_group_destroy(evplp_group *g) {
    if (!g) return;
    for (Worker *w : g->workers) if (w->th.joinable()) post(w, Task([](Worker &) { return 1; }));      // (non-zero: the worker's loop ends)
    for (Worker *w : g->workers) { if (w->th.joinable()) w->th.join(); delete w; }
    g->workers.clear();
    for (int r = 0; r < (int)g->d_frame.size(); r++) if (g->d_frame[(size_t)r]) { hipSetDevice(g->device[(size_t)r]); hipFree(g->d_frame[(size_t)r]); }
    for (int r = 0; r < (int)g->d_sum.size(); r++) if (g->d_sum[(size_t)r] || g->d_stage[(size_t)r]) { hipSetDevice(g->device[(size_t)r]); hipFree(g->d_sum[(size_t)r]); hipFree(g->d_stage[(size_t)r]); }
    for (int r = 0; r < (int)g->d_noise_stage.size(); r++) if (g->d_noise_stage[(size_t)r]) { hipSetDevice(g->device[(size_t)r]); hipFree(g->d_noise_stage[(size_t)r]); }
    for (int r = 0; r < (int)g->d_dn_recv.size(); r++) if (g->d_dn_recv[(size_t)r]) { hipSetDevice(g->device[(size_t)r]); hipFree(g->d_dn_recv[(size_t)r]); }
    for (int r = 0; r < (int)g->d_tp_recv.size(); r++) if (g->d_tp_recv[(size_t)r]) { hipSetDevice(g->device[(size_t)r]); hipFree(g->d_tp_recv[(size_t)r]); }
    if (g->d_dn_frame || g->d_dn_guides) { hipSetDevice(g->device[0]); hipFree(g->d_dn_frame); hipFree(g->d_dn_guides); }
    if (g->d_assembled || g->d_owner || g->d_noise_pool) { hipSetDevice(g->device[0]); hipFree(g->d_assembled); hipFree(g->d_owner); hipFree(g->d_noise_pool); }
    for (ncclComm_t c : g->comms) if (c && g->rccl.CommDestroy) g->rccl.CommDestroy(c);
    for (evplp_context *c : g->ctx) { c->quiesce = nullptr; evplp_destroy(c); }
    delete g;
}

// the floats an exchange moves under the round-robin deal (n > 1)
static size_t round_robin_floats(const evplp_group *g) { return (size_t)((g->image_blocks + g->n - 1) / g->n) * (size_t)g->strip_rows * g->ctx[0]->st.W * 3; }

extern "C" int evplp_group_create(const evplp_config *cfg, const evplp_group_config *gc, evplp_group **out) {
    auto fail = [&](int code, const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_group_create_error, sizeof(g_group_create_error), fmt, ap); va_end(ap); return code; };
    if (!cfg || !gc || !out) return fail(EVPLP_ERR_INVALID, "evplp_group_create: null argument");
    *out = nullptr;
    if (gc->n_ranks < 1 || gc->n_ranks > 64) return fail(EVPLP_ERR_INVALID, "evplp_group_create: n_ranks must be 1..64");
    evplp_group *g = new evplp_group();
    g->n = gc->n_ranks;
    for (int r = 0; r < g->n; r++) g->device.push_back(gc->devices ? gc->devices[r] : r);
    bool all_same = true, all_distinct = true;
    for (int r = 0; r < g->n; r++) for (int q = 0; q < r; q++) { if (g->device[(size_t)r] == g->device[(size_t)q]) all_distinct = false; else all_same = false; }
    if (g->n > 1 && !all_same && !all_distinct) { delete g; return fail(EVPLP_ERR_INVALID, "evplp_group_create: the ranks' devices must be all distinct (RCCL) or all the same (virtual ranks)"); }
    g->virtual_ranks = g->n > 1 ? all_same : !gc->use_rccl;
    if (gc->use_rccl && g->n > 1 && !all_distinct) { delete g; return fail(EVPLP_ERR_INVALID, "evplp_group_create: RCCL needs one distinct device per rank"); }
    // Strips of 16 rows keep a rank's tile rows in neighbouring pairs -- the gathers' entry cuts then cover groups of 2 x 2 tiles as on one
    // GPU (8-row strips: 2 x 1, twice as many cuts per pixel) -- but interleave the image half as finely.  Round 5 took 8 rows from eight
    // ranks on for that; with the blocks dealt by cost and launched most expensive first (evplp_group_rebalance) the finer interleave buys
    // nothing any more and the cheaper cuts win at every rank count (single-GPU projection of config #2, profiles/r06_strip_projection.json:
    // n = 8, 8- / 16-row blocks: slowest rank 8.49 / 8.06 ms; n = 4: 14.97 / 14.60).
    const int strip_rows = gc->strip_rows > 0 ? gc->strip_rows : 16;
    if (gc->partition != EVPLP_PARTITION_STRIPS && gc->partition != EVPLP_PARTITION_ITERATIONS) { delete g; return fail(EVPLP_ERR_INVALID, "evplp_group_create: partition %d unknown", gc->partition); }
    g->iterations = gc->partition == EVPLP_PARTITION_ITERATIONS;
    if (g->iterations && gc->split_light_paths > 0) { delete g; return fail(EVPLP_ERR_INVALID, "evplp_group_create: split_light_paths = 1 with EVPLP_PARTITION_ITERATIONS (every rank traces its own iteration's paths)"); }
    for (int r = 0; r < g->n; r++) {
        evplp_config c = *cfg;
        c.device = g->device[(size_t)r]; c.strip_rank = r; c.strip_count = g->n; c.strip_rows = strip_rows;
        {   // room for a deal by cost: strip_capacity_pct of the equal share of blocks, rounded up (0 = 150 %)
            const int nb = (cfg->res_y + strip_rows - 1) / strip_rows, share = (nb + g->n - 1) / g->n, pct = gc->strip_capacity_pct > 0 ? std::max(gc->strip_capacity_pct, 100) : 150;
            c.strip_capacity_rows = g->n > 1 ? std::min(nb, (share * pct + 99) / 100) * strip_rows : 0;
        }
        if (g->iterations) { c.strip_rank = 0; c.strip_count = 1; c.strip_capacity_rows = 0; }     // a whole-image context, as on one GPU
        evplp_context *h = nullptr;
        int rc = evplp_create(&c, &h);
        if (rc < 0) { int code = fail(rc, "rank %d: %s", r, evplp_last_error(nullptr)); evplp_group_destroy(g); return code; }
        g->ctx.push_back(h);
    }
    g->strip_rows = g->ctx[0]->st.strip_rows; g->image_blocks = g->ctx[0]->image_blocks; g->cap_blocks = g->ctx[0]->st.cap_blocks;
    g->strip_floats_cap = (size_t)g->ctx[0]->st.local_rows * g->ctx[0]->st.W * 3;
    // an exchange moves the rows in use: the equal share under the round-robin deal (the capacity beyond it holds nothing), the fullest rank's
    // blocks after a deal by cost
    g->strip_floats = g->n == 1 ? g->strip_floats_cap : round_robin_floats(g);
    g->d_frame.assign((size_t)g->n, nullptr);
    g->plane_px = (size_t)g->ctx[0]->st.W * g->ctx[0]->st.local_rows;
    g->d_sum.assign((size_t)g->n, nullptr); g->d_stage.assign((size_t)g->n, nullptr); g->d_noise_stage.assign((size_t)g->n, nullptr); g->d_dn_recv.assign((size_t)g->n, nullptr); g->d_tp_recv.assign((size_t)g->n, nullptr); g->num_cus.assign((size_t)g->n, 256);
    for (int r = 0; r < g->n; r++) {
        hipSetDevice(g->device[(size_t)r]);
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device[(size_t)r]) == hipSuccess && cus > 0) g->num_cus[(size_t)r] = cus;
        if (g->iterations) continue;      // (no strips to all-gather; the reduction's buffers come with the first reduction)
        hipError_t e = hipMalloc((void **)&g->d_frame[(size_t)r], sizeof(float) * g->strip_floats_cap * (size_t)g->n);
        if (e != hipSuccess) { int code = fail(EVPLP_ERR_OOM, "rank %d: hipMalloc(frame): %s", r, hipGetErrorString(e)); evplp_group_destroy(g); return code; }
    }
    if (!g->virtual_ranks) {
        std::string err;
        if (!g->rccl.open(err)) { int code = fail(EVPLP_ERR_NO_DEVICE, "%s", err.c_str()); evplp_group_destroy(g); return code; }
        g->comms.assign((size_t)g->n, nullptr);
        ncclResult_t nr = g->rccl.CommInitAll(g->comms.data(), g->n, g->device.data());
        if (nr != ncclSuccess) { int code = fail(EVPLP_ERR_HIP, "ncclCommInitAll: %s", g->rccl.GetErrorString(nr)); g->comms.clear(); evplp_group_destroy(g); return code; }
    }
    // a light-tracing launch is latency-bound (0.26 ms for 1024 paths, 0.25 ms for 128): small path counts are traced redundantly by
    // every rank (identical records, no exchange); large ones are split by path range and shared by one all-gather
    // (round 6: until round 5 the rule was "sets of >= 16 384 paths are split".  Config #4 at four ranks: 75 000 paths take 0.24 ms where 300 000
    // take 0.46, and the exchange moves 28.8 MB over every link -- more than the 0.22 ms the split saves at any plausible xGMI rate.)
    g->split_paths = !g->iterations && g->n > 1 && cfg->num_light_paths % (uint32_t)g->n == 0 &&
                     (gc->split_light_paths > 0 || (gc->split_light_paths == 0 && evplp_group_split_model(cfg->num_light_paths, cfg->photons_per_path, g->n, nullptr) == 1));
    g->per_rank_paths = g->split_paths ? cfg->num_light_paths / (uint32_t)g->n : cfg->num_light_paths;
    g->barrier.n = g->n;
    for (int r = 0; r < g->n; r++) { Worker *w = new Worker(); w->g = g; w->rank = r; w->c = g->ctx[(size_t)r]; g->workers.push_back(w); }
    for (Worker *w : g->workers) {
        w->th = std::thread(worker_main, w);
        w->c->worker_tid = w->th.get_id(); w->c->quiesce_arg = w; w->c->quiesce = quiesce_hook;
    }
    *out = g;
    return EVPLP_OK;
}

// The blocks dealt by the cost the gathers clocked (evplp_group_calibrate).  The ranks take their tables first and the owner table of the
// assembly follows only once all of them have: whatever fails, everybody returns to the round-robin deal, so d_owner, g->owner and the
// contexts never disagree.
extern "C" int evplp_group_rebalance(evplp_group *g) {
    GRP_CHECK(g);
    if (g->iterations && g->n > 1) { g->set_error("evplp_group_rebalance: the group shares out iterations, not the image: nothing to deal"); return EVPLP_ERR_INVALID; }
    drain(g);
    int rc = group_status(g); if (rc < 0) return rc;
    const int n = g->n, nb = g->image_blocks;
    if (n == 1) return EVPLP_OK;
    std::vector<uint64_t> cost((size_t)nb, 0), mine((size_t)nb);
    uint64_t total = 0;
    for (int r = 0; r < n; r++) {
        rc = evplp_block_costs(g->ctx[(size_t)r], mine.data(), nb);
        if (rc < 0) { g->set_error("rank %d: %s", r, evplp_last_error(g->ctx[(size_t)r])); return rc; }
        for (int b = 0; b < nb; b++) { cost[(size_t)b] += mine[(size_t)b]; total += mine[(size_t)b]; }
    }
    if (total == 0) { g->set_error("evplp_group_rebalance: no block cost was clocked (evplp_group_calibrate, then a frame with a gather)"); return EVPLP_ERR_INVALID; }
    std::vector<int32_t> owner((size_t)nb);
    rc = evplp_deal_blocks(cost.data(), nb, n, g->cap_blocks, owner.data());
    if (rc < 0) { g->set_error("evplp_group_rebalance: %d blocks do not fit %d ranks of %d", nb, n, g->cap_blocks); return rc; }
    // every rank's blocks, the most expensive first (evplp_rank_blocks: the launch order); all tables are built before any is set
    std::vector<std::vector<int32_t>> lists((size_t)n);
    std::vector<uint32_t> packed((size_t)nb);
    size_t most = 0;
    for (int r = 0; r < n; r++) {
        auto &l = lists[(size_t)r];
        l.resize((size_t)nb);
        l.resize((size_t)evplp_rank_blocks(cost.data(), owner.data(), nb, r, l.data(), nb));
        for (size_t i = 0; i < l.size(); i++) packed[(size_t)l[i]] = ((uint32_t)r << 16) | (uint32_t)i;
        most = std::max(most, l.size());
    }
    // (a table evplp_deal_blocks made for this capacity is not refused; if one is, the fallback below still holds)
    for (int r = 0; r < n && rc >= 0; r++) {
        rc = evplp_set_blocks(g->ctx[(size_t)r], lists[(size_t)r].data(), (int32_t)lists[(size_t)r].size());
        if (rc >= 0) rc = evplp_calibrate_blocks(g->ctx[(size_t)r], 0);
        if (rc < 0) g->set_error("rank %d: %s", r, evplp_last_error(g->ctx[(size_t)r]));
    }
    if (rc >= 0) {
        hipSetDevice(g->device[0]);
        if (!g->d_owner && hipMalloc((void **)&g->d_owner, sizeof(uint32_t) * (size_t)nb) != hipSuccess) { g->set_error("evplp_group_rebalance: hipMalloc(owner table)"); rc = EVPLP_ERR_OOM; }
        else if (hipMemcpy(g->d_owner, packed.data(), sizeof(uint32_t) * packed.size(), hipMemcpyHostToDevice) != hipSuccess) { g->set_error("evplp_group_rebalance: hipMemcpy(owner table)"); rc = EVPLP_ERR_HIP; }
        if (rc < 0) (void)hipGetLastError();
    }
    if (rc < 0) {
        for (int r = 0; r < n; r++) evplp_set_blocks(g->ctx[(size_t)r], nullptr, 0);
        g->owner.clear(); g->strip_floats = round_robin_floats(g);
        return rc;
    }
    g->owner.swap(owner);
    g->strip_floats = most * (size_t)g->strip_rows * g->ctx[0]->st.W * 3;
    return EVPLP_OK;
}

extern "C" int evplp_group_split_model(uint32_t num_light_paths, uint32_t photons_per_path, int32_t n_ranks, double out_ms[2]) {
    if (n_ranks < 1) return EVPLP_ERR_INVALID;
    auto trace_ms = [](double paths) { return 0.20 + 1.2e-6 * std::max(0.0, paths - 131072.0); };
    const double all = trace_ms((double)num_light_paths);
    const double chunk_bytes = (double)num_light_paths * photons_per_path * sizeof(evplp_record) / n_ranks;
    const double shared = trace_ms((double)num_light_paths / n_ranks) + (n_ranks > 1 ? 0.02 + chunk_bytes / 48.0e9 * 1.0e3 : 0.0);
    if (out_ms) { out_ms[0] = all; out_ms[1] = shared; }
    return n_ranks > 1 && shared < all ? 1 : 0;
}
extern "C" int evplp_group_calibrate(evplp_group *g, int32_t on) {
    GRP_CHECK(g);
    if (g->iterations) { g->set_error("evplp_group_calibrate: the group shares out iterations, not the image: no blocks to clock"); return EVPLP_ERR_INVALID; }
    drain(g);
    int rc = group_status(g); if (rc < 0) return rc;
    for (int r = 0; r < g->n; r++) {
        int rb = evplp_calibrate_blocks(g->ctx[(size_t)r], on);
        if (rb < 0) { g->set_error("rank %d: %s", r, evplp_last_error(g->ctx[(size_t)r])); return rb; }
    }
    return EVPLP_OK;
}
extern "C" int evplp_group_block_owners(evplp_group *g, int32_t *owner_rank, int32_t capacity) {
    GRP_CHECK(g);
    if (g->iterations) { g->set_error("evplp_group_block_owners: the group shares out iterations, not blocks"); return EVPLP_ERR_INVALID; }
    for (int b = 0; b < g->image_blocks && owner_rank && b < capacity; b++) owner_rank[b] = g->owner.empty() ? b % g->n : g->owner[(size_t)b];
    return g->image_blocks;
}

extern "C" int evplp_group_load_scene_json(evplp_group *g, const char *json_path) {
    GRP_CHECK(g);
    g->sums_fresh = false;
    return post_and_wait(g, command([json_path](Worker &w) { return evplp_load_scene_json(w.c, json_path); }));
}
extern "C" int evplp_group_clear_accumulators(evplp_group *g) { GRP_CHECK(g); g->sums_fresh = false; return post_all(g, command([](Worker &w) { return evplp_clear_accumulators(w.c); })); }
extern "C" int evplp_group_synchronize(evplp_group *g) { GRP_CHECK(g); return post_and_wait(g, synchronize()); }
extern "C" int evplp_group_primary(evplp_group *g, const float jitter[2], int32_t light_flags) {
    GRP_CHECK(g);
    const float jx = jitter ? jitter[0] : 0.f, jy = jitter ? jitter[1] : 0.f;
    if (g->iterations) g->last_primary = g->selected;          // (whose G-buffer evplp_group_denoise reads)
    return post_pass(g, command([jx, jy, light_flags](Worker &w) { const float j[2] = { jx, jy }; return evplp_primary(w.c, j, light_flags); }));
}
extern "C" int evplp_group_trace_light_paths(evplp_group *g, uint32_t rng_seed) {
    GRP_CHECK(g);
    if (!g->split_paths) return post_pass(g, command([rng_seed](Worker &w) { return evplp_trace_light_paths(w.c, rng_seed, 0, w.c->cfg.num_light_paths); }));
    // every rank traces its own path range and the records are all-gathered in place: rank r's slice goes to offset r * chunk of its record
    // buffer.  A partial path range never goes to the second record buffer of overlap_light_tracing (context.cpp only double-buffers whole path
    // sets), so EVPLP_BUF_RECORDS must be the same buffer before and after the call -- checked, because the exchange would otherwise gather
    // the wrong buffer.
    return post_pass(g, command([rng_seed](Worker &w) {
        evplp_context *c = w.c; const uint32_t per_rank_paths = w.g->per_rank_paths;
        const void *before = c->buf[EVPLP_BUF_RECORDS];
        const int rc = evplp_trace_light_paths(c, rng_seed, (uint32_t)w.rank * per_rank_paths, per_rank_paths);
        if (rc >= 0 && c->buf[EVPLP_BUF_RECORDS] != before) w.fail(EVPLP_ERR_INVALID, "evplp_group_trace_light_paths: a partial path range went into a flipped record buffer");
        return rc;
    }, exchange_records));
}
extern "C" int evplp_group_gather(evplp_group *g, const evplp_frame_params *fp, int32_t kind) {
    GRP_CHECK(g);
    if (kind < 0 || kind > 2) { g->set_error("evplp_group_gather: kind must be 0 (VPL), 1 (VSL) or 2 (light-path windows)"); return EVPLP_ERR_INVALID; }
    if (!fp) { g->set_error("evplp_group_gather: null frame params"); return EVPLP_ERR_INVALID; }
    { int rc = check_frame_params(g, fp, "evplp_group_gather", false); if (rc < 0) return rc; }
    if (g->adapt_pt) { g->set_error("evplp_group_gather: adaptivity is on in path-trace mode (evplp_group_adaptive_enable_pt): evplp_group_path_trace only"); return EVPLP_ERR_INVALID; }
    if (g->adapt_on && (kind == 2 || fp->do_accumulate == 0)) {
        g->set_error("evplp_group_gather: adaptivity is on (evplp_group_adaptive_enable): accumulating VPL and VSL gathers only"); return EVPLP_ERR_INVALID;
    }
    return post_pass(g, command([params = *fp, kind](Worker &w) { return kind == 0 ? evplp_gather_vpl(w.c, &params) : kind == 1 ? evplp_gather_vsl(w.c, &params) : evplp_gather_lvc(w.c, &params); }));
}
extern "C" int evplp_group_splat_photons(evplp_group *g, const evplp_frame_params *fp, int32_t clear) {
    GRP_CHECK(g);
    if (!fp) { g->set_error("evplp_group_splat_photons: null frame params"); return EVPLP_ERR_INVALID; }
    { int rc = check_frame_params(g, fp, "evplp_group_splat_photons", true); if (rc < 0) return rc; }
    if (g->adapt_gather_budget) { g->set_error("evplp_group_splat_photons: gather budget mode (evplp_group_adaptive_enable(g, 2)): one set of moments cannot price n_t VPL samples and N photon passes"); return EVPLP_ERR_INVALID; }
    return post_pass(g, command([params = *fp, clear](Worker &w) { return evplp_splat_photons(w.c, &params, clear); }));
}
extern "C" int evplp_group_set_splat_proxy(evplp_group *g, const float *vertices, int32_t nverts, const int32_t *indices, int32_t ntris) {
    GRP_CHECK(g);
    return post_and_wait(g, command([=](Worker &w) { return evplp_set_splat_proxy(w.c, vertices, nverts, indices, ntris); }));
}
extern "C" int evplp_group_update_mesh(evplp_group *g, int32_t mesh, const float *vertices, int32_t nverts) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::update_mesh_check(c0, mesh, vertices, nverts); })) return rc;
    g->sums_fresh = false;
    return post_and_wait(g, command([=](Worker &w) { return evplp_update_mesh(w.c, mesh, vertices, nverts); }));
}
extern "C" int evplp_group_transform_mesh(evplp_group *g, int32_t mesh, const float *m) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::transform_mesh_check(c0, mesh, m); })) return rc;
    g->sums_fresh = false;
    return post_and_wait(g, command([=](Worker &w) { return evplp_transform_mesh(w.c, mesh, m); }));
}
// (the skin and the palette are copied by every rank before the call returns: it waits for the workers)
extern "C" int evplp_group_set_mesh_skin(evplp_group *g, int32_t mesh, int32_t nbones, const int32_t *bone_index, const float *weight, int32_t nverts) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::set_mesh_skin_check(c0, mesh, nbones, bone_index, weight, nverts); })) return rc;
    return post_and_wait(g, command([=](Worker &w) { return evplp_set_mesh_skin(w.c, mesh, nbones, bone_index, weight, nverts); }));
}
extern "C" int evplp_group_pose_mesh(evplp_group *g, int32_t mesh, const float *bone_matrices, int32_t nbones) {
    GRP_CHECK(g);
    std::vector<float> posed;           // (the check skins rank 0's rest pose; every rank takes these positions: the call waits for the workers)
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::pose_mesh_check(c0, mesh, bone_matrices, nbones, &posed); })) return rc;
    g->sums_fresh = false;
    const float *positions = posed.data();
    const int rc = post_and_wait(g, command([=](Worker &w) { return evplp::pose_mesh_apply(w.c, mesh, bone_matrices, nbones, positions); }));
    drain(g);                           // (whatever the outcome, no worker reads `posed` behind this line)
    return rc;
}
// (the targets and the weights are copied by every rank before the call returns: it waits for the workers)
extern "C" int evplp_group_set_mesh_morph(evplp_group *g, int32_t mesh, int32_t ntargets, const float *deltas, int32_t nverts) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::set_mesh_morph_check(c0, mesh, ntargets, deltas, nverts); })) return rc;
    return post_and_wait(g, command([=](Worker &w) { return evplp_set_mesh_morph(w.c, mesh, ntargets, deltas, nverts); }));
}
extern "C" int evplp_group_morph_mesh(evplp_group *g, int32_t mesh, const float *weights, int32_t ntargets) {
    GRP_CHECK(g);
    std::vector<float> base, moved;     // (the check morphs rank 0's rest pose; every rank takes these positions: the call waits for the workers)
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::morph_mesh_check(c0, mesh, weights, ntargets, &base, &moved); })) return rc;
    g->sums_fresh = false;
    base.resize(moved.size());          // (unused without weights)
    const float *base_positions = base.data(), *positions = moved.data();
    const int rc = post_and_wait(g, command([=](Worker &w) { return evplp::morph_mesh_apply(w.c, mesh, weights, ntargets, base_positions, positions); }));
    drain(g);                           // (whatever the outcome, no worker reads the positions behind this line)
    return rc;
}
extern "C" int evplp_group_refit_accel(evplp_group *g) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::refit_check(c0); })) return rc;
    g->sums_fresh = false;
    return post_and_wait(g, command([](Worker &w) { return evplp_refit_accel(w.c); }));
}
// The scene and the tree are replicated, so every rank measures the same doubles (and a policy decides the same on each): rank 0's are the
// group's, and a rank that differs is an error.
extern "C" int evplp_group_accel_quality(evplp_group *g, struct evplp_accel_quality *out) {
    GRP_CHECK(g);
    if (!out) { g->set_error("evplp_group_accel_quality: null destination"); return EVPLP_ERR_INVALID; }
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::accel_quality_check(c0, "evplp_group_accel_quality"); })) return rc;
    std::vector<struct evplp_accel_quality> q((size_t)g->n);            // (one record per rank)
    struct evplp_accel_quality *per_rank = q.data();
    const int rc = post_and_wait(g, command([per_rank](Worker &w) { return evplp_accel_quality(w.c, per_rank + w.rank); }));
    if (rc < 0) return rc;
    for (int r = 1; r < g->n; r++)
        if (std::memcmp(&q[(size_t)r], &q[0], 6 * sizeof(double)) != 0 || q[(size_t)r].last_action != q[0].last_action || q[(size_t)r].policy_rebuilds != q[0].policy_rebuilds) {
            g->set_error("evplp_group_accel_quality: rank %d's tree differs from rank 0's (cost %.17g against %.17g, %d policy rebuilds against %d): the ranks' scenes are not the same",
                         r, q[(size_t)r].cost, q[0].cost, q[(size_t)r].policy_rebuilds, q[0].policy_rebuilds);
            return EVPLP_ERR_INVALID;
        }
    *out = q[0];
    return EVPLP_OK;
}
extern "C" int evplp_group_set_refit_policy(evplp_group *g, double max_cost_ratio, int32_t rebuild_builder) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::refit_policy_check(c0, max_cost_ratio, rebuild_builder); })) return rc;
    return post_and_wait(g, command([=](Worker &w) { return evplp_set_refit_policy(w.c, max_cost_ratio, rebuild_builder); }));
}
// Tree rotations: every rank runs the same sweeps over its copy of the tree and must take the same rotations; rank 0's count is the group's.
extern "C" int evplp_group_optimize_accel(evplp_group *g, int32_t passes, int32_t *rotations) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::optimize_accel_check(c0, "evplp_group_optimize_accel", passes); })) return rc;
    std::vector<int32_t> n((size_t)g->n, 0);                            // (one count per rank)
    int32_t *per_rank = n.data();
    const int rc = post_and_wait(g, command([=](Worker &w) { return evplp_optimize_accel(w.c, passes, per_rank + w.rank); }));
    if (rc < 0) return rc;
    for (int r = 1; r < g->n; r++)
        if (n[(size_t)r] != n[0]) {
            g->set_error("evplp_group_optimize_accel: rank %d took %d rotations, rank 0 took %d: the ranks' trees are not the same", r, n[(size_t)r], n[0]);
            return EVPLP_ERR_INVALID;
        }
    if (rotations) *rotations = n[0];
    return EVPLP_OK;
}
extern "C" int evplp_group_set_refit_rotations(evplp_group *g, int32_t passes) {
    GRP_CHECK(g);
    if (int rc = rank0_refuses(g, [&](evplp_context *c0) { return evplp::refit_rotations_check(c0, "evplp_group_set_refit_rotations", passes); })) return rc;
    return post_and_wait(g, command([passes](Worker &w) { return evplp_set_refit_rotations(w.c, passes); }));
}
// Ray queries.  Scene and tree are replicated (both partitions), so a batch is dealt by index: rank r of N traces rays [r n / N, (r + 1) n / N)
// into the caller's arrays, which stay valid because the call waits for the ranks.  A ray's result does not depend on the rays beside it, so
// the output is one context's byte for byte.  What the context refuses is refused on the caller's thread against rank 0's copy.
static Task trace_share(bool closest, const void *rays, int32_t n, int32_t filter, int32_t flags, void *out) {
    return command([=](Worker &w) {
        const int64_t ranks = w.g->n, begin = (int64_t)w.rank * n / ranks, end = ((int64_t)w.rank + 1) * n / ranks;
        const evplp_ray *r = (const evplp_ray *)rays + begin;
        return closest ? evplp_trace_closest(w.c, r, (int32_t)(end - begin), filter, flags, (evplp_hit *)out + begin)
                       : evplp_trace_occluded(w.c, r, (int32_t)(end - begin), flags, (uint8_t *)out + begin);
    });
}
extern "C" int evplp_group_trace_closest(evplp_group *group, const evplp_ray *rays, int32_t n, int32_t filter, int32_t flags, evplp_hit *hits) {
    GRP_CHECK(group);
    if (int rc = rank0_refuses(group, [&](evplp_context *c0) { return evplp::ray_query_check(c0, "evplp_group_trace_closest", rays, n, filter, flags, hits); })) return rc;
    return n == 0 ? group_status(group) : post_and_wait(group, trace_share(true, rays, n, filter, flags, hits));
}
extern "C" int evplp_group_trace_occluded(evplp_group *group, const evplp_ray *rays, int32_t n, int32_t flags, uint8_t *out) {
    GRP_CHECK(group);
    if (int rc = rank0_refuses(group, [&](evplp_context *c0) { return evplp::ray_query_check(c0, "evplp_group_trace_occluded", rays, n, 0, flags, out); })) return rc;
    return n == 0 ? group_status(group) : post_and_wait(group, trace_share(false, rays, n, 0, flags, out));
}
extern "C" int evplp_group_path_trace(evplp_group *g, const float camera_pos[3], uint32_t rng_seed, uint32_t max_bounces, int32_t do_accumulate) {
    GRP_CHECK(g);
    if (!camera_pos) { g->set_error("evplp_group_path_trace: null camera position"); return EVPLP_ERR_INVALID; }
    if (g->adapt_on && !g->adapt_pt) { g->set_error("evplp_group_path_trace: adaptivity is on (evplp_group_adaptive_enable): VPL and VSL gathers only"); return EVPLP_ERR_INVALID; }
    if (g->adapt_budget) { g->set_error("evplp_group_path_trace: budget mode (evplp_group_adaptive_enable_pt(g, 2)): evplp_group_path_trace_batch only"); return EVPLP_ERR_INVALID; }
    if (g->adapt_pt && !do_accumulate) { g->set_error("evplp_group_path_trace: adaptivity is on (evplp_group_adaptive_enable_pt): a sample must accumulate"); return EVPLP_ERR_INVALID; }
    const Vec3 camera{ { camera_pos[0], camera_pos[1], camera_pos[2] } };
    return post_pass(g, command([=](Worker &w) { return evplp_path_trace(w.c, camera.v, rng_seed, max_bounces, do_accumulate); }));
}

// Refused here, on the caller's thread, as the context refuses them (the workers' failures are sticky): the sample count, null arrays, a
// jitter that is not finite, gather-mode adaptivity, a scratch bound below one slot.  Strips: every rank runs the call for its own rows
// (a rank's active-tile list is over its own tiles); iterations: the selected rank.
extern "C" int evplp_group_path_trace_batch(evplp_group *g, const float camera_pos[3], int32_t samples, const float *jitters, const uint32_t *rng_seeds, uint32_t max_bounces) {
    GRP_CHECK(g);
    const char *name = "evplp_group_path_trace_batch";
    if (samples < 1 || samples > evplp::kPtBatchMaxSamples) { g->set_error("%s: samples must be 1 .. %d (got %d)", name, evplp::kPtBatchMaxSamples, samples); return EVPLP_ERR_INVALID; }
    if (!camera_pos || !jitters || !rng_seeds) { g->set_error("%s: null camera position, jitters or seeds", name); return EVPLP_ERR_INVALID; }
    if (g->adapt_on && !g->adapt_pt) { g->set_error("%s: adaptivity is on (evplp_group_adaptive_enable): VPL and VSL gathers only", name); return EVPLP_ERR_INVALID; }
    if (g->pt_batch_cap < evplp::kPtBatchSlotBytes) {
        g->set_error("%s: the scratch bound (%llu B, evplp_group_path_trace_batch_scratch) is below one tile x one sample (%zu B)", name, (unsigned long long)g->pt_batch_cap, evplp::kPtBatchSlotBytes);
        return EVPLP_ERR_INVALID;
    }
    auto sm = std::make_shared<evplp::PtBatchSamples>();
    std::memset(sm.get(), 0, sizeof(*sm));
    for (int s = 0; s < samples; s++) {
        sm->jitter[s][0] = jitters[2 * s]; sm->jitter[s][1] = jitters[2 * s + 1]; sm->seed[s] = rng_seeds[s];
        if (!std::isfinite(sm->jitter[s][0]) || !std::isfinite(sm->jitter[s][1])) { g->set_error("%s: jitter %d is not finite", name, s); return EVPLP_ERR_INVALID; }
    }
    if (g->iterations) g->last_primary = g->selected;          // (the call ends with a primary pass: whose G-buffer evplp_group_denoise reads)
    // (the call returns before the workers run it: every posted copy of the task shares the 768 B of jitters and seeds and keeps them alive)
    const Vec3 camera{ { camera_pos[0], camera_pos[1], camera_pos[2] } };
    return post_pass(g, command([=](Worker &w) { return evplp_path_trace_batch(w.c, camera.v, samples, &sm->jitter[0][0], sm->seed, max_bounces); }));
}
extern "C" int evplp_group_path_trace_batch_scratch(evplp_group *g, uint64_t bytes) {
    GRP_CHECK(g);
    drain(g);
    int rc = group_status(g); if (rc < 0) return rc;
    for (int r = 0; r < g->n; r++) evplp_path_trace_batch_scratch(g->ctx[(size_t)r], bytes);
    g->pt_batch_cap = bytes;
    return EVPLP_OK;
}

// EVPLP_PARTITION_ITERATIONS: every rank sums the ranks' planes and composites the sums -- or, with no pass since the last reduction, the
// cached sums again (nothing is exchanged).  worker_reduce keeps its own accounts: its exchange lies between two stretches of its calls.
static int post_reduce(evplp_group *g, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma) {
    const bool exchange = !g->sums_fresh;
    const int rc = post_all(g, Task([=](Worker &w) { worker_reduce(&w, vs, ps, ls, mask_emitter, gamma, exchange); return 0; }));
    if (rc >= 0) g->sums_fresh = true;
    return rc;
}
extern "C" int evplp_group_present(evplp_group *g, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma) {
    GRP_CHECK(g);
    if (g->iterations) return post_reduce(g, vs, ps, ls, mask_emitter, gamma);
    return post_all(g, present(vs, ps, ls, mask_emitter, gamma, false, true));       // (the per-iteration composite: no wait for the splat's verdict)
}
// exchange = 0: every rank composites its strip where it is and nobody waits for anybody -- no host barrier, no collective: the iteration of
// a loop whose frame is looked at only now and then (a sub-millisecond iteration pays for the exchange otherwise: DESIGN section 5)
extern "C" int evplp_group_present_ex(evplp_group *g, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, int32_t exchange) {
    GRP_CHECK(g);
    if (g->iterations) {        // exchange = 0: the selected rank composites its own accumulators
        if (exchange != 0) return post_reduce(g, vs, ps, ls, mask_emitter, gamma);
        return post_one(g, g->selected, present(vs, ps, ls, mask_emitter, gamma, false, false));
    }
    return post_all(g, present(vs, ps, ls, mask_emitter, gamma, false, exchange != 0));
}

// evplp_group_present (settled), then the frame in image order on rank 0's device and one copy to the caller.
extern "C" int evplp_group_resolve(evplp_group *g, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, float *out_rgb) {
    GRP_CHECK(g);
    if (!out_rgb) { g->set_error("evplp_group_resolve: null output"); return EVPLP_ERR_INVALID; }
    int rc = g->iterations ? post_reduce(g, vs, ps, ls, mask_emitter, gamma) : post_all(g, present(vs, ps, ls, mask_emitter, gamma, true, true));
    if (rc < 0) return rc;
    post(g->workers[0], assemble(out_rgb));          // (rank 0's stream: behind its side of the exchange)
    drain(g);
    return group_status(g);
}

// The error of the frame against a reference image (include/evplp.h).  Strips: every rank composites its rows and reduces them on its GPU,
// and 32 bytes per row come to the host -- no all-gather.  Iterations: the reduction evplp_group_resolve runs (or its cached sums), then
// rank 0 reduces the summed composite.  The rows are added on the caller's thread in image row order, by the helper a single context uses.
extern "C" int evplp_group_set_error_reference(evplp_group *g, const float *rgb, const uint8_t *mask) {
    GRP_CHECK(g);
    if (!rgb && mask) { g->set_error("evplp_group_set_error_reference: a mask without a reference image"); return EVPLP_ERR_INVALID; }
    const int rc = post_and_wait(g, command([rgb, mask](Worker &w) { return evplp_set_error_reference(w.c, rgb, mask); }));     // (the caller's images are read before the call returns)
    g->have_reference = rc >= 0 && rgb != nullptr;
    return rc;
}
extern "C" int evplp_group_frame_error(evplp_group *g, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, double out[3]) {
    GRP_CHECK(g);
    if (!out) { g->set_error("evplp_group_frame_error: null output"); return EVPLP_ERR_INVALID; }
    if (!g->have_reference) { g->set_error("evplp_group_frame_error: no reference image (evplp_group_set_error_reference)"); return EVPLP_ERR_INVALID; }
    const Task error_rows = command([](Worker &w) { return evplp::frame_error_rows(w.c); });          // (behind the rank's composite, on its stream)
    int rc;
    if (g->iterations) {
        rc = post_reduce(g, vs, ps, ls, mask_emitter, gamma);
        if (rc >= 0) post(g->workers[0], error_rows);
    } else {
        rc = post_all(g, present(vs, ps, ls, mask_emitter, gamma, true, false, false));      // (every rank's own rows: nothing is exchanged; not a pass)
        if (rc >= 0) rc = post_all(g, error_rows);
    }
    if (rc < 0) return rc;
    drain(g);
    if ((rc = group_status(g)) < 0) return rc;
    const evplp_context *c0 = g->ctx[0];
    std::vector<evplp::RowError> rows((size_t)c0->st.H); std::vector<char> held((size_t)c0->st.H, 0);
    for (int r = 0; r < (g->iterations ? 1 : g->n); r++) evplp::place_row_errors(g->ctx[(size_t)r], g->ctx[(size_t)r]->err_rows, rows, held);
    evplp::sum_row_errors(rows, held, (double)c0->st.W * c0->st.H, out);
    return EVPLP_OK;
}

// Per-pixel noise from the running sums (include/evplp.h).  Strips: every rank tracks, folds and reduces its own rows, and 32 bytes per row
// come to the host.  Iterations: a fold closes a batch of the selected rank's iterations; an estimate pools the ranks' moments on rank 0.
// What can be refused without a device is refused here, on the caller's thread, and leaves the group usable.
extern "C" int evplp_group_noise_track(evplp_group *g, int32_t on, const uint8_t *mask) {
    GRP_CHECK(g);
    if (!on && mask) { g->set_error("evplp_group_noise_track: a mask without tracking"); return EVPLP_ERR_INVALID; }
    if (g->adapt_on) {
        drain(g);
        for (evplp_context *x : g->ctx)
            if (x->adapt_n > 0) { g->set_error("evplp_group_noise_track: adaptivity is on and %lld gather(s) accumulated", (long long)x->adapt_n); return EVPLP_ERR_INVALID; }
    }
    const int rc = post_and_wait(g, command([on, mask](Worker &w) { return evplp_noise_track(w.c, on, mask); }));     // (the caller's mask is read before the call returns)
    g->noise_on = rc >= 0 && on != 0;
    return rc;
}
extern "C" int evplp_group_noise_fold(evplp_group *g, int32_t iterations) {
    GRP_CHECK(g);
    if (!g->noise_on) { g->set_error("evplp_group_noise_fold: tracking is off (evplp_group_noise_track)"); return EVPLP_ERR_INVALID; }
    if (iterations < 1) { g->set_error("evplp_group_noise_fold: a batch holds >= 1 iterations, not %d", iterations); return EVPLP_ERR_INVALID; }
    const Task fold = command([iterations](Worker &w) { return evplp_noise_fold(w.c, iterations); });
    return g->iterations ? post_one(g, g->selected, fold) : post_all(g, fold);
}
// tracking on and B >= 2 (the ranks' folds summed under the iteration partition); drains the workers to read their counts
static int noise_group_ready(evplp_group *g, const char *name) {
    if (!g->noise_on) { g->set_error("%s: tracking is off (evplp_group_noise_track)", name); return EVPLP_ERR_INVALID; }
    drain(g);
    int rc = group_status(g);
    if (rc < 0) return rc;
    int64_t b = 0;
    for (int r = 0; r < (g->iterations ? g->n : 1); r++) b += g->ctx[(size_t)r]->noise_b;
    if (b < 2) { g->set_error("%s: %lld fold(s): the estimate needs >= 2", name, (long long)b); return EVPLP_ERR_INVALID; }
    return EVPLP_OK;
}
extern "C" int evplp_group_noise_estimate(evplp_group *g, float scale, float ls, int32_t mask_emitter, double out[3]) {
    GRP_CHECK(g);
    if (!out) { g->set_error("evplp_group_noise_estimate: null output"); return EVPLP_ERR_INVALID; }
    int rc = noise_group_ready(g, "evplp_group_noise_estimate");
    if (rc < 0) return rc;
    if (g->iterations) {
        // rank 0's moments pooled over the ranks (noise_pool before), with the summed light plane of the reduction
        rc = post_reduce(g, scale, scale, ls, mask_emitter, 0);
        if (rc >= 0) rc = post_all(g, noise_pool());
        if (rc >= 0) post(g->workers[0], command([=](Worker &w) {
            return evplp::noise_rows(w.c, noise_pooled(w.g, w.c), w.g->d_sum[0] + 2 * w.g->plane_px, w.g->pool_k, w.g->pool_b, scale, ls, mask_emitter);
        }));
    } else {
        rc = post_all(g, present(scale, scale, ls, mask_emitter, 0, true, false, false));      // (every rank's own rows: nothing is exchanged; not a pass)
        if (rc >= 0) rc = post_all(g, command([=](Worker &w) {
            evplp_context *c = w.c;
            return evplp::noise_rows(c, evplp::noise_moments_of(c), (const float4 *)c->buf[EVPLP_BUF_LIGHT], (double)c->noise_k, (double)c->noise_b, scale, ls, mask_emitter);
        }));
    }
    if (rc < 0) return rc;
    drain(g);
    if ((rc = group_status(g)) < 0) return rc;
    const evplp_context *c0 = g->ctx[0];
    std::vector<evplp::RowError> all((size_t)c0->st.H); std::vector<char> held((size_t)c0->st.H, 0);
    for (int r = 0; r < (g->iterations ? 1 : g->n); r++) evplp::place_row_errors(g->ctx[(size_t)r], g->ctx[(size_t)r]->noise_rows, all, held);
    evplp::sum_row_errors(all, held, (double)c0->st.W * c0->st.H, out);
    return EVPLP_OK;
}
extern "C" int evplp_group_noise_variance(evplp_group *g, float scale, float *out_rgb) {
    GRP_CHECK(g);
    if (!out_rgb) { g->set_error("evplp_group_noise_variance: null output"); return EVPLP_ERR_INVALID; }
    int rc = noise_group_ready(g, "evplp_group_noise_variance");
    if (rc < 0) return rc;
    // every rank's variance into its d_rgb, all-gathered as a present's composite (strips), or rank 0's pooled one; then the assembly
    if (g->iterations) {
        rc = post_all(g, noise_pool());
        if (rc >= 0) post(g->workers[0], noise_variance(scale, true, false, false));
    } else rc = post_all(g, noise_variance(scale, false, false, true));
    if (rc < 0) return rc;
    post(g->workers[0], assemble(out_rgb));
    drain(g);
    return group_status(g);
}

// The denoiser of a written frame (include/evplp.h evplp_group_denoise).  Strips: every rank packs its rows, the packed rows are all-gathered
// and assembled on rank 0 as a resolve's strips are, and rank 0 filters the frame.  Iterations: rank 0 packs the pooled variance, the reduced
// composite and light plane and the guides of the rank of the last primary, and filters them.
static int group_denoise(evplp_group *g, const char *name, float scale, float ls, int32_t mask_emitter, const evplp_denoise_params *p, const evplp_temporal_params *t,
                         bool temporal, float *out_rgb, evplp_temporal_info *info) {
    evplp::DenoiseSettings ds; evplp::TemporalSettings ts{ 0, 0.f }; char why[200];
    if (!evplp::denoise_settings(p, &ds, why, sizeof why) || (temporal && !evplp::temporal_settings(t, &ts, why, sizeof why))) { g->set_error("%s: %s", name, why); return EVPLP_ERR_INVALID; }
    if (!out_rgb) { g->set_error("%s: null output", name); return EVPLP_ERR_INVALID; }
    int rc = noise_group_ready(g, name);
    if (rc < 0) return rc;
    if (!g->ctx[0]->accel_built) { g->set_error("%s: no scene (evplp_group_load_scene_json / evplp_build_accel)", name); return EVPLP_ERR_INVALID; }
    if (g->ctx[0]->scene_dirty) { g->set_error("%s: vertices were updated (evplp_group_update_mesh): call evplp_group_refit_accel first", name); return EVPLP_ERR_INVALID; }
    if (temporal) {
        // (the workers are idle: noise_group_ready has drained them).  The ranks whose walk is repeated must hold the G-buffer of their last primary
        if (!g->temporal_on) { g->set_error("%s: temporal accumulation is off (evplp_group_temporal_enable)", name); return EVPLP_ERR_INVALID; }
        for (int r = 0; r < g->n; r++) {
            evplp_context *c = g->ctx[(size_t)r];
            if (!evplp::temporal_check(c, name, !g->iterations || r == g->last_primary)) { g->set_error("%s", c->error); return EVPLP_ERR_INVALID; }
        }
        // (another triangle count since the last call: every rank makes its previous pose anew and the call is a first call)
        for (int r = 0; r < g->n; r++) if ((rc = evplp::temporal_pose_array(g->ctx[(size_t)r])) < 0) { g->set_error("%s", g->ctx[(size_t)r]->error); return rc; }
    }
    if (!g->iterations) {
        // every rank's packed pixels and receive buffer exist before any worker names them in the all-gather (the workers are idle here)
        for (int r = 0; r < g->n; r++) {
            evplp_context *c = g->ctx[(size_t)r];
            const size_t px = std::max<size_t>((size_t)c->st.W * c->st.local_rows, 1);
            hipError_t e = hipSetDevice(g->device[(size_t)r]);
            if (e == hipSuccess && !c->d_dn_pack) e = hipMalloc((void **)&c->d_dn_pack, sizeof(evplp::DenoisePixel) * px);
            if (e == hipSuccess && !g->d_dn_recv[(size_t)r]) e = hipMalloc((void **)&g->d_dn_recv[(size_t)r], sizeof(float) * (g->strip_floats_cap / 3) * evplp::kDenoiseFloats * (size_t)g->n);
            if (e == hipSuccess && temporal && !g->d_tp_recv[(size_t)r]) e = hipMalloc((void **)&g->d_tp_recv[(size_t)r], sizeof(float) * (g->strip_floats_cap / 3) * evplp::kTemporalPrevFloats * (size_t)g->n);
            if (e != hipSuccess) { (void)hipGetLastError(); g->set_error("%s: rank %d: %s", name, r, hipGetErrorString(e)); return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP; }
        }
    }
    const int guides_rank = g->iterations ? g->last_primary : 0;          // (iterations: whose G-buffer, and whose previous-pose texels, rank 0 reads)
    auto prep = [=](Worker &w) { return worker_denoise_prep(&w, scale, ls, mask_emitter, temporal, guides_rank); };
    if (g->iterations) {
        // (the rank of the last primary; it waits, so that rank 0 -- behind the reduction's barrier -- reads finished texels)
        if (temporal) post(g->workers[(size_t)g->last_primary], command([](Worker &w) { const int rp = worker_temporal_pose(w.c); return rp < 0 ? rp : evplp_synchronize(w.c); }));
        rc = post_all(g, noise_pool());
        if (rc >= 0) post(g->workers[0], noise_variance(scale, true, true, false));
        if (rc >= 0) rc = post_reduce(g, scale, scale, ls, mask_emitter, 0);
        if (rc >= 0) post(g->workers[0], command(prep));
    } else rc = post_all(g, command(prep, [temporal](Worker &w) { exchange_denoise(w, temporal); }));
    if (rc < 0) return rc;
    post(g->workers[0], command([=](Worker &w) { return worker_denoise_filter(&w, ds, temporal, ts, guides_rank, out_rgb); }));
    if (temporal) { rc = post_all(g, command([](Worker &w) { return evplp::temporal_snapshot(w.c); })); if (rc < 0) return rc; }
    drain(g);
    rc = group_status(g);
    if (rc >= 0 && temporal && info) { rc = evplp::temporal_info(g->ctx[0], info); if (rc < 0) g->set_error("%s", g->ctx[0]->error); }
    return rc;
}
extern "C" int evplp_group_denoise(evplp_group *g, float scale, float ls, int32_t mask_emitter, const evplp_denoise_params *p, float *out_rgb) {
    GRP_CHECK(g);
    return group_denoise(g, "evplp_group_denoise", scale, ls, mask_emitter, p, nullptr, false, out_rgb, nullptr);
}
// Temporal accumulation for the whole frame (include/evplp.h evplp_group_denoise_temporal): every rank keeps the previous pose and camera and
// evaluates its own rows on it; rank 0 holds the history in image layout and runs the stage in front of the passes.
extern "C" int evplp_group_temporal_enable(evplp_group *g, int32_t on) {
    GRP_CHECK(g);
    drain(g);
    const int rc = post_and_wait(g, command([on](Worker &w) { return evplp::temporal_enable(w.c, on); }));
    g->temporal_on = rc >= 0 && on != 0;
    return rc;
}
extern "C" int evplp_group_temporal_reset(evplp_group *g) {
    GRP_CHECK(g);
    if (!g->temporal_on) { g->set_error("evplp_group_temporal_reset: temporal accumulation is off (evplp_group_temporal_enable)"); return EVPLP_ERR_INVALID; }
    return post_and_wait(g, command([](Worker &w) { evplp::temporal_forget(w.c); return EVPLP_OK; }));
}
extern "C" int evplp_group_denoise_temporal(evplp_group *g, float scale, float ls, int32_t mask_emitter, const evplp_denoise_params *p,
                                            const evplp_temporal_params *t, float *out_rgb, evplp_temporal_info *info) {
    GRP_CHECK(g);
    return group_denoise(g, "evplp_group_denoise_temporal", scale, ls, mask_emitter, p, t, true, out_rgb, info);
}
extern "C" int evplp_group_temporal_download(evplp_group *g, int32_t which, float *out) {
    GRP_CHECK(g);
    const char *name = "evplp_group_temporal_download";
    if (!out || which < EVPLP_TEMPORAL_HISTORY_U || which > EVPLP_TEMPORAL_PREV_NRM) { g->set_error("%s: a null output or a plane the group does not hold (%d)", name, which); return EVPLP_ERR_INVALID; }
    if (!g->temporal_on) { g->set_error("%s: temporal accumulation is off (evplp_group_temporal_enable)", name); return EVPLP_ERR_INVALID; }
    drain(g);
    int rc = group_status(g);
    if (rc < 0) return rc;
    evplp_context *c = g->ctx[0];
    const size_t frame_px = (size_t)c->st.W * c->st.H;
    hipError_t e = hipSetDevice(g->device[0]);
    if (which <= EVPLP_TEMPORAL_HISTORY_NRM) {
        if (!c->d_tp_hist || c->tp_frames == 0) { g->set_error("%s: no call has written a history", name); return EVPLP_ERR_INVALID; }
        if (e == hipSuccess) e = hipMemcpy(out, c->d_tp_hist + ((size_t)c->tp_cur * 3 + (size_t)which) * c->tp_hist_px, sizeof(float4) * frame_px, hipMemcpyDeviceToHost);
    } else {
        const evplp::TemporalPrev *src = g->iterations ? g->ctx[(size_t)g->last_primary]->d_tp_prev : c->d_tp_prev_frame;
        if (!src) { g->set_error("%s: no call has evaluated a previous pose", name); return EVPLP_ERR_INVALID; }
        if (g->iterations) e = hipSetDevice(g->device[(size_t)g->last_primary]);
        std::vector<evplp::TemporalPrev> host(frame_px);
        if (e == hipSuccess) e = hipMemcpy(host.data(), src, sizeof(evplp::TemporalPrev) * frame_px, hipMemcpyDeviceToHost);
        for (size_t i = 0; i < frame_px; i++) std::memcpy(out + 4 * i, which == EVPLP_TEMPORAL_PREV_POS ? &host[i].pos : &host[i].nrm, 16);
    }
    if (e != hipSuccess) { g->set_error("%s: %s", name, hipGetErrorString(e)); return EVPLP_ERR_HIP; }
    return EVPLP_OK;
}

// Adaptive gather (include/evplp.h evplp_adaptive_*).  Row strips only: every rank decides for its own tiles; the counts are summed and the
// tile map is put together from the block owners.  The iteration partition would have to pool its ranks' decisions: refused.
static int adapt_group_ready(evplp_group *g, const char *name) {
    if (g->iterations) { g->set_error("%s: not under EVPLP_PARTITION_ITERATIONS (the ranks' decisions are not pooled)", name); return EVPLP_ERR_INVALID; }
    drain(g);
    return group_status(g);
}
static int group_adaptive_enable(evplp_group *g, int32_t on, bool pt, const char *name) {
    int rc = adapt_group_ready(g, name);
    if (rc < 0) return rc;
    for (evplp_context *c : g->ctx)
        if (c->adapt_n > 0) { g->set_error("%s: %lld gather(s) have accumulated since the last clear", name, (long long)c->adapt_n); return EVPLP_ERR_INVALID; }
    if (on && !g->noise_on) { g->set_error("%s: noise tracking is off (evplp_group_noise_track)", name); return EVPLP_ERR_INVALID; }
    if (on == 2 && !pt)
        for (evplp_context *c : g->ctx)
            if (c->splat_n > 0) { g->set_error("%s: %lld photon splat(s) since the last clear: gather budget mode has no place for them", name, (long long)c->splat_n); return EVPLP_ERR_INVALID; }
    rc = post_and_wait(g, command([on, pt](Worker &w) { return pt ? evplp_adaptive_enable_pt(w.c, on) : evplp_adaptive_enable(w.c, on); }));
    g->adapt_on = rc >= 0 && on != 0;
    g->adapt_pt = g->adapt_on && pt;
    g->adapt_budget = g->adapt_on && on == 2;
    g->adapt_gather_budget = g->adapt_budget && !pt;
    return rc;
}
extern "C" int evplp_group_adaptive_enable(evplp_group *g, int32_t on) { GRP_CHECK(g); return group_adaptive_enable(g, on, false, "evplp_group_adaptive_enable"); }
extern "C" int evplp_group_adaptive_enable_pt(evplp_group *g, int32_t on) { GRP_CHECK(g); return group_adaptive_enable(g, on, true, "evplp_group_adaptive_enable_pt"); }
extern "C" int evplp_group_adaptive_retire(evplp_group *g, float scale, float ls, int32_t mask_emitter, double tau, int32_t min_batches) {
    GRP_CHECK(g);
    int rc = adapt_group_ready(g, "evplp_group_adaptive_retire");
    if (rc < 0) return rc;
    if (!g->ctx[0]->d_adapt_tiles) { g->set_error("evplp_group_adaptive_retire: adaptivity is off (evplp_group_adaptive_enable)"); return EVPLP_ERR_INVALID; }
    if (g->adapt_budget) { g->set_error("evplp_group_adaptive_retire: budget mode (evplp_group_adaptive_enable(g, 2) / evplp_group_adaptive_enable_pt(g, 2)): set the tile's budget to 0 instead"); return EVPLP_ERR_INVALID; }
    if (!(tau >= 0.0)) { g->set_error("evplp_group_adaptive_retire: tile_rel_mse must be >= 0, not %g", tau); return EVPLP_ERR_INVALID; }
    if (min_batches < 2) { g->set_error("evplp_group_adaptive_retire: min_batches must be >= 2, not %d", min_batches); return EVPLP_ERR_INVALID; }
    // (the count of tiles a rank retired stays in its context's adapt_last)
    rc = post_and_wait(g, command([=](Worker &w) { const int retired = evplp_adaptive_retire(w.c, scale, ls, mask_emitter, tau, min_batches); return retired < 0 ? retired : EVPLP_OK; }));
    if (rc < 0) return rc;
    int32_t n = 0;
    for (evplp_context *x : g->ctx) n += x->adapt_last;
    return n;
}
extern "C" int evplp_group_adaptive_tiles(evplp_group *g, int32_t *out, int32_t capacity) {
    GRP_CHECK(g);
    int rc = adapt_group_ready(g, "evplp_group_adaptive_tiles");
    if (rc < 0) return rc;
    const evplp_context *c0 = g->ctx[0];
    if (!c0->d_adapt_tiles) { g->set_error("evplp_group_adaptive_tiles: adaptivity is off (evplp_group_adaptive_enable)"); return EVPLP_ERR_INVALID; }
    const int64_t n = (int64_t)((c0->st.W + 7) / 8) * ((c0->st.H + 7) / 8);
    if (!out || capacity < n) { g->set_error("evplp_group_adaptive_tiles: the image has %lld tiles, the output holds %d", (long long)n, capacity); return EVPLP_ERR_INVALID; }
    std::fill(out, out + n, 0);
    for (const evplp_context *c : g->ctx) evplp::adaptive_tiles_into(c, out);
    return (int)n;
}
// Budget mode (include/evplp.h evplp_adaptive_set_budgets).  A tile never straddles two row blocks, so a rank decides nothing: it takes its own
// tiles from the whole-image array, and the figures that come back are put together per tile.  What the context would refuse is refused
// here, on the caller's thread (the workers' failures are sticky), and the group stays usable.
static int64_t group_image_tiles(const evplp_group *g) { const evplp_context *c0 = g->ctx[0]; return (int64_t)((c0->st.W + 7) / 8) * ((c0->st.H + 7) / 8); }
extern "C" int evplp_group_adaptive_set_budgets(evplp_group *g, const int32_t *samples_per_image_tile, int32_t count) {
    GRP_CHECK(g);
    const char *name = "evplp_group_adaptive_set_budgets";
    int rc = adapt_group_ready(g, name);
    if (rc < 0) return rc;
    if (!g->adapt_budget) { g->set_error("%s: budget mode is off (evplp_group_adaptive_enable(g, 2) / evplp_group_adaptive_enable_pt(g, 2))", name); return EVPLP_ERR_INVALID; }
    const int64_t n = group_image_tiles(g);
    if (!samples_per_image_tile || count != n) { g->set_error("%s: the image has %lld tiles, the call gives %d", name, (long long)n, samples_per_image_tile ? count : 0); return EVPLP_ERR_INVALID; }
    for (int64_t t = 0; t < n; t++)
        if (samples_per_image_tile[t] < 0 || samples_per_image_tile[t] > evplp::kPtBatchMaxSamples) {
            g->set_error("%s: tile %lld: a budget is 0 .. %d samples, not %d", name, (long long)t, evplp::kPtBatchMaxSamples, samples_per_image_tile[t]); return EVPLP_ERR_INVALID;
        }
    for (const evplp_context *c : g->ctx) {
        if (c->noise_b < 2) { g->set_error("%s: %lld fold(s): budgets need >= 2 (evplp_group_noise_fold)", name, (long long)c->noise_b); return EVPLP_ERR_INVALID; }
        if (c->noise_k != c->adapt_n) { g->set_error("%s: %lld of %lld samples are folded: fold first (evplp_group_noise_fold)", name, (long long)c->noise_k, (long long)c->adapt_n); return EVPLP_ERR_INVALID; }
    }
    // (every rank takes its own tiles from the caller's whole-image array, which is read before the call returns)
    return post_and_wait(g, command([=](Worker &w) { return evplp_adaptive_set_budgets(w.c, samples_per_image_tile, count); }));
}
// (host state of the contexts only: set on the caller's thread once the workers are idle, as evplp_group_path_trace_batch_scratch does)
extern "C" int evplp_group_adaptive_budget_window(evplp_group *g, int32_t window) {
    GRP_CHECK(g);
    const char *name = "evplp_group_adaptive_budget_window";
    int rc = adapt_group_ready(g, name);
    if (rc < 0) return rc;
    if (!g->adapt_gather_budget) { g->set_error("%s: gather budget mode is off (evplp_group_adaptive_enable(g, 2))", name); return EVPLP_ERR_INVALID; }
    if (window < 1 || window > evplp::kGatherBudgetMaxWindow) { g->set_error("%s: a window is 1 .. %d calls, not %d", name, evplp::kGatherBudgetMaxWindow, window); return EVPLP_ERR_INVALID; }
    for (evplp_context *c : g->ctx) { c->adapt_window = window; c->adapt_m = 0; }
    return EVPLP_OK;
}
extern "C" int evplp_group_adaptive_budgets(evplp_group *g, int32_t *out, int32_t capacity) {
    GRP_CHECK(g);
    const char *name = "evplp_group_adaptive_budgets";
    int rc = adapt_group_ready(g, name);
    if (rc < 0) return rc;
    if (!g->adapt_budget) { g->set_error("%s: budget mode is off (evplp_group_adaptive_enable(g, 2) / evplp_group_adaptive_enable_pt(g, 2))", name); return EVPLP_ERR_INVALID; }
    const int64_t n = group_image_tiles(g);
    if (!out || capacity < n) { g->set_error("%s: the image has %lld tiles, the output holds %d", name, (long long)n, capacity); return EVPLP_ERR_INVALID; }
    std::fill(out, out + n, 0);
    for (const evplp_context *c : g->ctx) evplp::adaptive_budgets_into(c, out);
    return (int)n;
}
extern "C" int evplp_group_adaptive_tile_noise(evplp_group *g, float scale, float ls, int32_t mask_emitter, double *rel_per_image_tile, int32_t capacity) {
    GRP_CHECK(g);
    const char *name = "evplp_group_adaptive_tile_noise";
    if (g->iterations) { g->set_error("%s: not under EVPLP_PARTITION_ITERATIONS (the ranks' decisions are not pooled)", name); return EVPLP_ERR_INVALID; }
    if (!g->adapt_on) { g->set_error("%s: adaptivity is off (evplp_group_adaptive_enable)", name); return EVPLP_ERR_INVALID; }
    const int64_t n = group_image_tiles(g);
    if (!rel_per_image_tile || capacity < n) { g->set_error("%s: the image has %lld tiles, the output holds %d", name, (long long)n, capacity); return EVPLP_ERR_INVALID; }
    int rc = noise_group_ready(g, name);
    if (rc < 0) return rc;
    std::fill(rel_per_image_tile, rel_per_image_tile + n, 0.0);
    // (every rank puts its own tiles into the caller's whole-image array, which outlives the drain)
    if ((rc = post_and_wait(g, command([=](Worker &w) { return evplp::adaptive_tile_noise_into(w.c, scale, ls, mask_emitter, rel_per_image_tile); }))) < 0) return rc;
    return (int)n;
}
