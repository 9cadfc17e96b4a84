// C ABI of libprisma_bands.so (include/prisma_bands.h): context lifetime, the band entry points and their host pipelines.
// The pb_op_* single-kernel entry points are in abi_ops.hip.
#include <dlfcn.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "abi_ctx.h"
#include "gmflow_engine.h"
#include "raft_engine.h"

static thread_local char g_err[1024] = "";

void pb_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// The caller's buffer is page-locked host memory (hipHostMalloc / hipHostRegister / torch pin_memory): the copy engines can address it
// directly, so the host-pointer entry points skip their own pinned staging copies (a 1080p clip of 32 frames is 199 MB each way: ~20 ms of
// one core per memcpy, which the pipeline can only hide while a LATER chunk computes)
static bool pb_is_pinned(const void *p, size_t bytes = 1) {
    if (!p) return false;
    // both ends of the range must be page-locked (a caller may hand a pointer into the middle of a registered region whose end lies before ours)
    for (const char *q : {(const char *)p, (const char *)p + (bytes ? bytes - 1 : 0)}) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

// Error exits of the host-pointer pipelines: with page-locked caller buffers the copy engines read and write CALLER memory asynchronously on the
// pipeline's two copy streams, so no path may return - with or without an error - while a copy or a kernel that feeds one is still in flight:
// the caller is free to release or reuse its buffers the moment the call returns.  Declared after the streams exist; its destructor drains them.
// A blocking call leaves it armed, so every exit drains; an asynchronous one disarms it once everything is enqueued, so only error exits do
// (the caller gets an error, not a half-enqueued call).
struct PipeDrain {
    hipStream_t a, b, c;
    bool armed = true;
    ~PipeDrain() {
        if (!armed) return;
        (void)hipStreamSynchronize(a);
        (void)hipStreamSynchronize(b);
        (void)hipStreamSynchronize(c);
    }
};

// One host-pointer call = several engine infer() calls (one per chunk): the per-launch timer is reset ONCE per API call and accumulates over the
// chunks, so pb_get_kernel_stats describes the whole call as it does for a device-pointer call (stage snapshots - pb_*_get_stage -
// still describe the last chunk).  Restores the caller's accumulate setting.
struct TimerSpan {
    KernelTimer &t;
    bool saved;
    explicit TimerSpan(KernelTimer &timer) : t(timer), saved(timer.accumulate) { t.reset(); t.accumulate = true; }
    ~TimerSpan() { t.accumulate = saved; }
};

// One array of a chunked host-pointer call.  Lane k of the table uses ChunkPipe::lane[k].
struct ChunkLane {
    void *host = nullptr;       // the caller's array (null: a small-result lane nobody asked for)
    size_t unit = 0;            // bytes per unit (a frame, a frame pair); 0: the lane is absent
    bool out = true;            // direction: result (D2H) or input (H2D)
    bool pinned = false;        // the caller's array is page-locked: the copy engines address it directly, no staging
    bool small = false;         // a few bytes per unit (min / max, max displacement): always staged by the blocking form, DMAed straight to the caller by submit
    void *host2 = nullptr;      // parts == 2: the second caller array
    int parts = 1;              // small lanes: 2 = the device slot holds two arrays [host | host2], units-per-chunk entries each (either caller pointer may be null)
};

// The host-pointer entry points of the depth and flow bands: a three-stage pipeline over chunks of `per` units.  Stage 1 copies the caller's
// frames into a pinned staging buffer and DMAs them to HBM on a copy stream, stage 2 is the band on the ctx stream (`compute(slot, first_unit,
// m)`, which reads and writes the slot's device buffers), stage 3 DMAs the results into pinned memory on a second copy stream and hands them to
// the caller's arrays.  Two slots per stage, ordered by events, so the PCIe traffic of chunks i + 1 and i - 1 overlaps the compute of chunk i.
// A chunk reads `extra_in` units beyond its own (the halo frame of a chunk of frame pairs).  Page-locked caller arrays are read and written by
// the copy engines directly (no staging memcpy on this thread).
// `submit`: the asynchronous form (pb_depth_submit_batch / pb_flow_submit_sequence) - every caller buffer is page-locked (the callers check),
// nothing in the loop waits on the host (slot reuse is ordered by events on the streams: the H2D into a slot waits for the compute that last
// read it, the compute into a slot for the D2H that last emptied it), the small results are DMAed straight into the caller's arrays, and the
// call returns after the enqueue with a completion event queued for pb_wait().  The blocking form keeps its host-side finish() for pageable
// buffers and drains on every exit.
template <class Compute>
static int run_chunks(pb_ctx *c, int units, int per, int extra_in, const ChunkLane *lanes, int n_lanes, bool submit, Compute compute) {
    ChunkPipe &p = c->pipe;
    PB_TRY(p.ensure_streams());
    PipeDrain drain{p.s_in, c->stream, p.s_out};
    for (int k = 0; k < n_lanes; ++k) {
        const ChunkLane &l = lanes[k];
        PB_TRY(p.grow(k, (size_t)(per + (l.out ? 0 : extra_in)) * l.unit * l.parts, l.small || !l.pinned));
    }
    const int chunks = (units + per - 1) / per;
    const unsigned base = p.seq;
    p.seq += (unsigned)chunks;
    auto finish = [&](int i) -> int {           // results of chunk i: pinned staging -> caller (page-locked caller arrays were written directly)
        const int slot = (int)((base + i) & 1), u0 = i * per, m = std::min(per, units - u0);
        PB_HIP(hipEventSynchronize(p.ev_d2h[slot]));
        for (int k = 0; k < n_lanes; ++k) {
            const ChunkLane &l = lanes[k];
            const char *h = (const char *)p.lane[k].h[slot];
            if (!l.out || !l.unit || (l.pinned && !l.small)) continue;
            if (l.host) memcpy((char *)l.host + u0 * l.unit, h, m * l.unit);
            if (l.host2) memcpy((char *)l.host2 + u0 * l.unit, h + per * l.unit, m * l.unit);
        }
        return 0;
    };
    for (int i = 0; i < chunks; ++i) {
        const int slot = (int)((base + i) & 1), u0 = i * per, m = std::min(per, units - u0);
        if (!submit && i >= 2) PB_TRY(finish(i - 2));       // frees this slot's staging and (through ev_d2h) its device buffers
        PB_HIP(hipStreamWaitEvent(p.s_in, p.ev_comp[slot], 0));        // the compute that last read this input slot: this call's chunk i - 2 or an earlier submission's (also in the blocking form: a submission may still be in flight)
        for (int k = 0; k < n_lanes; ++k) {
            const ChunkLane &l = lanes[k];
            if (l.out || !l.unit) continue;
            const size_t bytes = (size_t)(m + extra_in) * l.unit;
            const void *src = (const char *)l.host + u0 * l.unit;
            if (!l.pinned) { memcpy(p.lane[k].h[slot], src, bytes); src = p.lane[k].h[slot]; }
            PB_HIP(hipMemcpyAsync(p.lane[k].d[slot], src, bytes, hipMemcpyHostToDevice, p.s_in));
        }
        PB_HIP(hipEventRecord(p.ev_h2d[slot], p.s_in));
        PB_HIP(hipStreamWaitEvent(c->stream, p.ev_h2d[slot], 0));
        PB_HIP(hipStreamWaitEvent(c->stream, p.ev_d2h[slot], 0));      // the D2H that last emptied this output slot
        PB_TRY(compute(slot, u0, m));
        PB_HIP(hipEventRecord(p.ev_comp[slot], c->stream));
        PB_HIP(hipStreamWaitEvent(p.s_out, p.ev_comp[slot], 0));
        for (int k = 0; k < n_lanes; ++k) {
            const ChunkLane &l = lanes[k];
            const char *d = (const char *)p.lane[k].d[slot];
            if (!l.out || !l.unit) continue;
            if (!l.small) {
                PB_HIP(hipMemcpyAsync(l.pinned ? (char *)l.host + u0 * l.unit : p.lane[k].h[slot], d, m * l.unit, hipMemcpyDeviceToHost, p.s_out));
            } else if (submit) {
                if (l.host) PB_HIP(hipMemcpyAsync((char *)l.host + u0 * l.unit, d, m * l.unit, hipMemcpyDeviceToHost, p.s_out));
                if (l.host2) PB_HIP(hipMemcpyAsync((char *)l.host2 + u0 * l.unit, d + per * l.unit, m * l.unit, hipMemcpyDeviceToHost, p.s_out));
            } else {
                PB_HIP(hipMemcpyAsync(p.lane[k].h[slot], d, ((l.parts - 1) * per + m) * l.unit, hipMemcpyDeviceToHost, p.s_out));
            }
        }
        PB_HIP(hipEventRecord(p.ev_d2h[slot], p.s_out));
    }
    if (submit) {
        hipEvent_t done;
        PB_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        PB_HIP(hipEventRecord(done, p.s_out));                // s_out runs its copies in order: the last chunk's results are the last thing it does
        c->pending.push_back(done);
        drain.armed = false;
        return 0;
    }
    for (int i = std::max(0, chunks - 2); i < chunks; ++i) PB_TRY(finish(i));
    return 0;
}

extern "C" {

const char *pb_last_error(void) { return g_err; }
int pb_version(void) { return 100; }
int pb_abi_version(void) { return PB_ABI_VERSION; }
int pb_struct_size(int which) {
    switch (which) {
        case 0: return (int)sizeof(pb_tensor);
        case 1: return (int)sizeof(pb_depth_cfg);
        case 2: return (int)sizeof(pb_flow_cfg);
        case 3: return (int)sizeof(pb_mask_cfg);
        case 4: return (int)sizeof(pb_kernel_stat);
        case 5: return (int)sizeof(pb_comm_id);
        case 6: return (int)sizeof(pb_yuv_fmt);
        case 7: return (int)sizeof(pb_jpeg_cfg);
        default: return -1;
    }
}

int pb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pb_create(pb_ctx **out, int device_id, const char *band, const pb_tensor *weights, int n_weights, const void *cfg,
              size_t cfg_bytes) {
    PB_CHECK(out && band, PB_ERR_ARG, "pb_create: null argument");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    PB_CHECK(e == hipSuccess && ndev > 0, PB_ERR_DEVICE, "no HIP device available (%s); this library has no CPU path",
             e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    PB_CHECK(device_id >= 0 && device_id < ndev, PB_ERR_ARG, "device %d out of range (%d devices)", device_id, ndev);
    PB_HIP(hipSetDevice(device_id));
    pb_ctx *c = new pb_ctx();
    c->device = device_id;
    const CreateEnv env = create_env();         // the create-time switches, read once for this context
    if (!strcmp(band, "depth_anything")) {
        if (!cfg || cfg_bytes != sizeof(pb_depth_cfg) || !weights || n_weights <= 0) {
            delete c;
            PB_CHECK(false, PB_ERR_ARG, "depth_anything: needs a pb_depth_cfg (%zu bytes, got %zu) and weights",
                     sizeof(pb_depth_cfg), cfg_bytes);
        }
        c->depth = new DepthEngine(device_id, *(const pb_depth_cfg *)cfg, env);
        int r = c->depth->load(weights, n_weights);
        if (r) {
            delete c->depth;
            delete c;
            return r;
        }
        c->band = c->depth;
    } else if (!strcmp(band, "flow_raft") || !strcmp(band, "flow_gmflow")) {
        const bool gm = band[5] == 'g';
        if (!weights || n_weights <= 0 || (cfg && cfg_bytes != sizeof(pb_flow_cfg))) {
            delete c;
            PB_CHECK(false, PB_ERR_ARG, "%s: needs weights (and cfg = NULL or a pb_flow_cfg of %zu bytes, got %zu)", band, sizeof(pb_flow_cfg), cfg_bytes);
        }
        const int prec = cfg ? ((const pb_flow_cfg *)cfg)->precision : PB_PREC_F16;
        if (prec != PB_PREC_F16 && prec != PB_PREC_SPLIT) {
            delete c;
            PB_CHECK(false, PB_ERR_ARG, "%s: precision %d unknown", band, prec);
        }
        c->flow = gm ? (FlowEngine *)new GmflowEngine(device_id, env) : new RaftEngine(device_id, env);
        c->flow->split_w_ = prec == PB_PREC_SPLIT;
        c->flow->mx_ = !gm && c->flow->split_w_ && env.mx;
        int r = c->flow->load(weights, n_weights);
        if (r) {
            delete c->flow;
            delete c;
            return r;
        }
        c->band = c->flow;
    } else if (!strcmp(band, "mask_mmdet")) {
        if (!cfg || cfg_bytes != sizeof(pb_mask_cfg) || !weights || n_weights <= 0) {
            delete c;
            PB_CHECK(false, PB_ERR_ARG, "mask_mmdet: needs a pb_mask_cfg (%zu bytes, got %zu) and weights", sizeof(pb_mask_cfg),
                     cfg_bytes);
        }
        c->mask = new MaskEngine(device_id, *(const pb_mask_cfg *)cfg, env);
        int r = c->mask->load(weights, n_weights);
        if (r) {
            delete c->mask;
            delete c;
            return r;
        }
        c->band = c->mask;
    } else if (!strcmp(band, "ops")) {
        // kernel-level context for the parity tests: a stream and a zero page, no model
        hipError_t e1 = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        void *z = nullptr;
        hipError_t e2 = hipMalloc(&z, 4096);
        if (e1 != hipSuccess || e2 != hipSuccess) {
            delete c;
            PB_CHECK(false, PB_ERR_DEVICE, "ops context: stream/alloc failed");
        }
        hipMemset(z, 0, 4096);
        hipDeviceSynchronize();
        c->zero = (f16 *)z;
        c->own_stream = true;
    } else {
        delete c;
        PB_CHECK(false, PB_ERR_ARG, "unknown band '%s' (depth_anything | flow_raft | flow_gmflow | mask_mmdet | ops)", band);
    }
    if (c->band) {
        c->stream = c->band->stream;
        c->zero = (f16 *)c->band->zero_page();
    }
    *out = c;
    return 0;
}

// ---- RCCL (the per-frame scalar all-gather of SURVEY 8(e)) -------------------------------------------------
// librccl is opened lazily and privately (dlopen, RTLD_LOCAL): the library carries no link-time dependency on it and does
// not interpose the copy a host framework (torch.distributed's "nccl" backend) may have loaded.
namespace {
struct Rccl {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, pb_comm_id, int) = nullptr;      // ncclUniqueId is passed by value: 128 bytes
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool load() {
        if (h) return true;
        for (const char *n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return false;
        GetUniqueId = (decltype(GetUniqueId))dlsym(h, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(h, "ncclCommInitRank");
        AllGather = (decltype(AllGather))dlsym(h, "ncclAllGather");
        CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
        GetErrorString = (decltype(GetErrorString))dlsym(h, "ncclGetErrorString");
        return GetUniqueId && CommInitRank && AllGather && CommDestroy && GetErrorString;
    }
} g_rccl;
}  // namespace

int pb_comm_unique_id(pb_comm_id *id_out) {
    PB_CHECK(id_out, PB_ERR_ARG, "comm_unique_id: null");
    PB_CHECK(g_rccl.load(), PB_ERR_DEVICE, "librccl could not be loaded: %s", dlerror());
    const int rc = g_rccl.GetUniqueId(id_out);
    PB_CHECK(rc == 0, PB_ERR_DEVICE, "ncclGetUniqueId: %s", g_rccl.GetErrorString(rc));
    return 0;
}

int pb_comm_init(pb_ctx *c, const pb_comm_id *id, int rank, int world) {
    PB_CHECK(c && id && world >= 1 && rank >= 0 && rank < world, PB_ERR_ARG, "comm_init: bad arguments");
    PB_CHECK(!c->comm, PB_ERR_STATE, "comm_init: the ctx already has a communicator");
    PB_CHECK(g_rccl.load(), PB_ERR_DEVICE, "librccl could not be loaded: %s", dlerror());
    PB_HIP(hipSetDevice(c->device));
    const int rc = g_rccl.CommInitRank(&c->comm, world, *id, rank);
    PB_CHECK(rc == 0, PB_ERR_DEVICE, "ncclCommInitRank(rank %d of %d): %s", rank, world, g_rccl.GetErrorString(rc));
    c->comm_rank = rank; c->comm_world = world;
    return 0;
}

int pb_gather_scalars(pb_ctx *c, const float *local, int n_local, float *global) {
    PB_CHECK(c && c->comm && local && global && n_local > 0, PB_ERR_ARG, "gather_scalars: needs pb_comm_init and non-empty buffers");
    PB_HIP(hipSetDevice(c->device));
    const size_t need = (size_t)(c->comm_world + 1) * n_local;
    if (need > c->comm_cap) {
        if (c->comm_buf) PB_HIP(hipFree(c->comm_buf));
        c->comm_buf = nullptr; c->comm_cap = 0;
        PB_HIP(hipMalloc((void **)&c->comm_buf, need * 4));
        c->comm_cap = need;
    }
    float *send = c->comm_buf, *recv = c->comm_buf + n_local;
    PB_HIP(hipMemcpyAsync(send, local, (size_t)n_local * 4, hipMemcpyHostToDevice, c->stream));
    const int rc = g_rccl.AllGather(send, recv, (size_t)n_local, 7 /* ncclFloat32 */, c->comm, c->stream);
    PB_CHECK(rc == 0, PB_ERR_DEVICE, "ncclAllGather: %s", g_rccl.GetErrorString(rc));
    PB_HIP(hipMemcpyAsync(global, recv, (size_t)c->comm_world * n_local * 4, hipMemcpyDeviceToHost, c->stream));
    PB_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

void pb_destroy(pb_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->comm) { hipStreamSynchronize(c->stream); g_rccl.CommDestroy(c->comm); }
    if (c->comm_buf) hipFree(c->comm_buf);
    if (c->still_stream) { hipStreamSynchronize(c->still_stream); hipStreamDestroy(c->still_stream); }
    if (c->still_buf) hipFree(c->still_buf);
    if (c->pcl_mm) { hipStreamSynchronize(c->stream); hipFree(c->pcl_mm); }
    for (hipEvent_t e : c->pending) { hipEventSynchronize(e); hipEventDestroy(e); }
    c->pipe.release();
    c->mpipe.release();
    for (void *p : c->yuv) if (p) { hipStreamSynchronize(c->stream); hipFree(p); }
    if (c->jpeg.ws || c->jpeg.d_in[0]) { hipStreamSynchronize(c->stream); c->jpeg.release(); }
    // pb_host_alloc blocks: the submissions that wrote into them were waited for above and the copy streams are drained and gone
    for (void *p : c->host_blocks) hipHostFree(p);
    if (c->depth) delete c->depth;
    if (c->flow) delete c->flow;
    if (c->mask) delete c->mask;
    if (c->own_stream) {
        hipStreamSynchronize(c->stream);
        hipFree(c->zero);
        hipStreamDestroy(c->stream);
    }
    delete c;
}

int pb_sync(pb_ctx *c) {
    PB_CHECK(c, PB_ERR_ARG, "null ctx");
    PB_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int pb_depth_infer_batch_dev(pb_ctx *c, const uint8_t *frames, int n, int H, int W, float *depth_out, uint8_t *rgb_out,
                             float *min_out, float *max_out, int flip) {
    PB_CHECK(c && c->depth, PB_ERR_STATE, "ctx has no depth_anything band");
    return c->depth->infer(frames, n, H, W, depth_out, rgb_out, min_out, max_out, flip);
}

// Host-pointer variant: run_chunks over chunks of max_batch frames; `submit` is pb_depth_submit_batch.
static int depth_host_pipeline(pb_ctx *c, const uint8_t *frames, int n, int H, int W, float *depth_out, uint8_t *rgb_out, float *min_out,
                               float *max_out, int flip, bool submit) {
    PB_HIP(hipSetDevice(c->device));
    const size_t px = (size_t)H * W;
    // frames per chunk: pb_set_option("host_chunk"), else max_batch.  (Round 6 first cut calls of >= 16 frames in two so that one half's copies ran
    // under the other half's kernels: on the bench clip the 16-frame launches' longer tails cost more than the hidden copies gave -
    // profiles/r06j_pcie_entry_points.txt; copies are hidden ACROSS calls by the asynchronous form instead.)
    const int mb = c->depth->max_batch();
    const int cap = std::min(n, c->host_chunk > 0 ? std::min(c->host_chunk, mb) : mb);
    // pb_set_frame_format / pb_set_out_format: the lane carries planar YUV frames, converted on the ctx stream into / out of the RGB buffer the band works on
    const bool yin = c->frames_i420 != 0, yout = c->rgb_out_i420 != 0 && rgb_out;
    const size_t fin = yin ? (size_t)yuv_frame_bytes(c->frame_fmt, H, W) : px * 3, fout = yout ? (size_t)yuv_frame_bytes(c->out_fmt, H, W) : px * 3;
    const bool pin_in = pb_is_pinned(frames, (size_t)n * fin), pin_d = pb_is_pinned(depth_out, (size_t)n * px * 4),
               pin_r = pb_is_pinned(rgb_out, (size_t)n * fout);
    const bool pin_mm = (!min_out || pb_is_pinned(min_out, (size_t)n * 4)) && (!max_out || pb_is_pinned(max_out, (size_t)n * 4));
    if (submit) PB_CHECK(pin_in && (!depth_out || pin_d) && (!rgb_out || pin_r) && pin_mm, PB_ERR_ARG,
                         "depth submit: every buffer of an asynchronous call must be page-locked host memory (hipHostMalloc / hipHostRegister / torch pin_memory)");
    const ChunkLane lanes[4] = {{(void *)frames, fin, false, pin_in},
                                {depth_out, depth_out ? px * 4 : 0, true, pin_d},
                                {rgb_out, rgb_out ? fout : 0, true, pin_r},
                                {min_out, 4, true, pin_mm, true, max_out, 2}};
    if (yin) PB_TRY(c->yuv_grow(0, (size_t)cap * px * 3));
    if (yout) PB_TRY(c->yuv_grow(1, (size_t)cap * px * 3));
    TimerSpan span(c->depth->timer);
    const ChunkPipe::Lane *l = c->pipe.lane;
    return run_chunks(c, n, cap, 0, lanes, 4, submit, [&](int slot, int, int m) {
        float *mn = (float *)l[3].d[slot];
        const uint8_t *in = (const uint8_t *)l[0].d[slot];
        if (yin) {
            PB_TRY(launch_yuv_to_rgb(c->stream, c->frame_fmt, in, m, H, W, (uint8_t *)c->yuv[0]));
            in = (const uint8_t *)c->yuv[0];
        }
        uint8_t *enc = (uint8_t *)(rgb_out ? (yout ? c->yuv[1] : l[2].d[slot]) : nullptr);
        PB_TRY(c->depth->infer(in, m, H, W, (float *)(depth_out ? l[1].d[slot] : nullptr), enc, mn, mn + cap, flip));
        return yout ? launch_rgb_to_yuv(c->stream, c->out_fmt, enc, m, H, W, (uint8_t *)l[2].d[slot]) : 0;
    });
}

int pb_depth_infer_batch(pb_ctx *c, const uint8_t *frames, int n, int H, int W, float *depth_out, uint8_t *rgb_out,
                         float *min_out, float *max_out, int flip) {
    PB_CHECK(c && c->depth, PB_ERR_STATE, "ctx has no depth_anything band");
    PB_CHECK(frames && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "infer: bad arguments");
    return depth_host_pipeline(c, frames, n, H, W, depth_out, rgb_out, min_out, max_out, flip, false);
}

int pb_depth_submit_batch(pb_ctx *c, const uint8_t *frames, int n, int H, int W, float *depth_out, uint8_t *rgb_out,
                          float *min_out, float *max_out, int flip) {
    PB_CHECK(c && c->depth, PB_ERR_STATE, "ctx has no depth_anything band");
    PB_CHECK(frames && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "submit: bad arguments");
    return depth_host_pipeline(c, frames, n, H, W, depth_out, rgb_out, min_out, max_out, flip, true);
}

int pb_wait(pb_ctx *c) {
    PB_CHECK(c, PB_ERR_ARG, "null ctx");
    PB_CHECK(!c->pending.empty(), PB_ERR_STATE, "pb_wait: no submission is outstanding on this ctx");
    PB_HIP(hipSetDevice(c->device));
    hipEvent_t done = c->pending.front();
    c->pending.pop_front();
    const hipError_t e = hipEventSynchronize(done);
    (void)hipEventDestroy(done);
    PB_CHECK(e == hipSuccess, PB_ERR_DEVICE, "pb_wait: %s", hipGetErrorString(e));
    return 0;
}

// pb_depth_get_stage / pb_flow_get_stage / pb_mask_get_stage: `own` is the ctx's engine of the band the entry point belongs to (null: another band's ctx)
static int64_t band_stage(pb_ctx *c, const EngineBase *own, const char *what, const char *name, float *out, int64_t cap, int64_t shape_out[4]) {
    PB_CHECK(c && own && name && out && shape_out, PB_ERR_ARG, "%sget_stage: bad arguments", what);
    PB_HIP(hipSetDevice(c->device));
    return c->band->get_stage(name, out, cap, shape_out);
}

int64_t pb_depth_get_stage(pb_ctx *c, const char *name, float *out, int64_t cap, int64_t shape_out[4]) {
    return band_stage(c, c ? c->depth : nullptr, "", name, out, cap, shape_out);
}

int pb_set_profiling(pb_ctx *c, int enabled) {
    PB_CHECK(c && c->band, PB_ERR_STATE, "ctx has no band");
    KernelTimer &t = c->band->timer;
    t.enabled = (enabled & 1) != 0;
    t.accumulate = (enabled & 4) != 0;
    t.clear();
    c->band->debug = (enabled & 2) != 0;
    return 0;
}

int pb_flow_out_size(int H, int W, float scale, int *sh, int *sw) {
    PB_CHECK(H > 0 && W > 0 && scale > 0.f && sh && sw, PB_ERR_ARG, "flow_out_size: bad arguments");
    FlowEngine::out_size(H, W, scale, sh, sw);
    return 0;
}

int pb_flow_infer_sequence_dev(pb_ctx *c, const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward,
                               float *flow_out, uint8_t *rgb_out, float *maxdisp_out) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow_raft band");
    return c->flow->infer(frames, F, H, W, scale, iters, backward, flow_out, rgb_out, maxdisp_out);
}

// Host-pointer variants (reference loop bands/flow_raft.py:98-113: a decoded frame pair per iteration; :63-64 the consistency masks of --mask):
// run_chunks over chunks of PB_FLOW_HOST_PAIRS frame pairs.  A chunk carries one halo frame, so the frame it shares with its neighbour is
// encoded twice; every pair's flow (and mask: both directions of a pair are in the same chunk) is that of one whole-sequence call - pairs do
// not interact.  mask_out != NULL: both directions + the forward / backward consistency masks (pb_flow_infer_sequence_masks).
static int flow_host_pipeline(pb_ctx *c, const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward,
                              float *flow_out, uint8_t *rgb_out, float *maxdisp_out, uint8_t *mask_out, float alpha1, float alpha2, bool submit = false) {
    PB_HIP(hipSetDevice(c->device));
    int sh, sw;
    FlowEngine::out_size(H, W, scale, &sh, &sw);
    const int dirs = backward ? 2 : 1, pairs = F - 1;
    // (default 32 pairs since round 6 - was 16: a chunk's launches are the same kernels on fewer rows, and 16-pair chunks cost the bench clip more in
    // launch tails and re-encoded halo frames than their hidden copies gave; profiles/r06j_pcie_entry_points.txt)
    const int env_cp = launch_env().flow_host_pairs;
    int cp = c->host_chunk > 0 ? c->host_chunk : (env_cp > 0 ? env_cp : 32);
    if (pairs <= cp + cp / 4) cp = pairs;                       // a short tail is not worth a chunk of its own
    // ... and no chunk larger than one infer() call accepts at this size (flow_chunk.h: 4K frames); a single pair that does not fit goes
    // through as it is and the engine refuses it
    cp = std::max(1, c->flow->chunk_pairs(cp, H, W, scale, dirs));
    const size_t px = (size_t)sh * sw * dirs, np = (size_t)pairs;      // px: result pixels of a pair, all directions
    // pb_set_frame_format / pb_set_out_format: planar YUV frames in, ... of the output size out (dirs of them per pair), converted on the ctx stream
    // "rgb_out_full": ... of the clip's H x W, resized on the ctx stream from the sh x sw frames the band encodes (nothing to do at scale 1): I420
    // by the fused resize kernel, any other layout by a resize into ctx scratch and a conversion out of it
    const bool yin = c->frames_i420 != 0, yout = c->rgb_out_i420 != 0 && rgb_out, full = c->rgb_out_full != 0 && rgb_out && (sh != H || sw != W);
    const int rh = full ? H : sh, rw = full ? W : sw;                  // the size of an rgb_out frame
    const bool two = full && yout && !yuv_fmt_is_i420(c->out_fmt);
    const size_t fpx = yin ? (size_t)yuv_frame_bytes(c->frame_fmt, H, W) : (size_t)H * W * 3,
                 rpx = (yout ? (size_t)yuv_frame_bytes(c->out_fmt, rh, rw) : (size_t)rh * rw * 3) * dirs;
    const bool pin_in = pb_is_pinned(frames, (size_t)F * fpx), pin_f = pb_is_pinned(flow_out, np * px * 8), pin_r = pb_is_pinned(rgb_out, np * rpx),
               pin_k = pb_is_pinned(mask_out, np * px), pin_m = !maxdisp_out || pb_is_pinned(maxdisp_out, np * dirs * 4);
    if (submit) PB_CHECK(pin_in && (!flow_out || pin_f) && (!rgb_out || pin_r) && (!mask_out || pin_k) && pin_m, PB_ERR_ARG,
                         "flow submit: every buffer of an asynchronous call must be page-locked host memory (hipHostMalloc / hipHostRegister / torch pin_memory)");
    const ChunkLane lanes[5] = {{(void *)frames, fpx, false, pin_in},
                                {flow_out, flow_out ? px * 8 : 0, true, pin_f},
                                {rgb_out, rgb_out ? rpx : 0, true, pin_r},
                                {maxdisp_out, (size_t)dirs * 4, true, pin_m, true},
                                {mask_out, mask_out ? px : 0, true, pin_k}};
    if (yin) PB_TRY(c->yuv_grow(0, (size_t)(cp + 1) * H * W * 3));
    if (yout || full) PB_TRY(c->yuv_grow(1, (size_t)cp * px * 3));
    if (two) PB_TRY(c->yuv_grow(2, (size_t)cp * dirs * H * W * 3));
    TimerSpan span(c->flow->timer);
    const ChunkPipe::Lane *l = c->pipe.lane;
    return run_chunks(c, pairs, cp, 1, lanes, 5, submit, [&](int slot, int, int m) {
        const uint8_t *in = (const uint8_t *)l[0].d[slot];
        if (yin) {
            PB_TRY(launch_yuv_to_rgb(c->stream, c->frame_fmt, in, m + 1, H, W, (uint8_t *)c->yuv[0]));
            in = (const uint8_t *)c->yuv[0];
        }
        uint8_t *enc = (uint8_t *)(rgb_out ? (yout || full ? c->yuv[1] : l[2].d[slot]) : nullptr);
        PB_TRY(c->flow->infer(in, m + 1, H, W, scale, iters, backward, (float *)(flow_out ? l[1].d[slot] : nullptr), enc, (float *)l[3].d[slot],
                              (uint8_t *)(mask_out ? l[4].d[slot] : nullptr), alpha1, alpha2));
        if (two) {
            PB_TRY(launch_rgb_resize(c->stream, enc, m * dirs, sh, sw, H, W, (uint8_t *)c->yuv[2], false));
            return launch_rgb_to_yuv(c->stream, c->out_fmt, (const uint8_t *)c->yuv[2], m * dirs, H, W, (uint8_t *)l[2].d[slot]);
        }
        if (full) return launch_rgb_resize(c->stream, enc, m * dirs, sh, sw, H, W, (uint8_t *)l[2].d[slot], yout);
        return yout ? launch_rgb_to_yuv(c->stream, c->out_fmt, enc, m * dirs, sh, sw, (uint8_t *)l[2].d[slot]) : 0;
    });
}

int pb_flow_submit_sequence(pb_ctx *c, const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward,
                            float *flow_out, uint8_t *rgb_out, float *maxdisp_out) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow_raft band");
    PB_CHECK(frames && F >= 2 && H > 0 && W > 0, PB_ERR_ARG, "flow submit: bad arguments");
    return flow_host_pipeline(c, frames, F, H, W, scale, iters, backward, flow_out, rgb_out, maxdisp_out, nullptr, 0.05f, 0.5f, true);
}

int pb_flow_infer_sequence(pb_ctx *c, const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward,
                           float *flow_out, uint8_t *rgb_out, float *maxdisp_out) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow_raft band");
    PB_CHECK(frames && F >= 2 && H > 0 && W > 0, PB_ERR_ARG, "flow infer: bad arguments");
    return flow_host_pipeline(c, frames, F, H, W, scale, iters, backward, flow_out, rgb_out, maxdisp_out, nullptr, 0.05f, 0.5f);
}

int pb_flow_infer_sequence_masks_dev(pb_ctx *c, const uint8_t *frames, int F, int H, int W, float scale, int iters,
                                     float alpha1, float alpha2, float *flow_out, uint8_t *rgb_out, float *maxdisp_out,
                                     uint8_t *mask_out) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow_raft band");
    PB_CHECK(mask_out, PB_ERR_ARG, "flow masks: mask_out is NULL");
    return c->flow->infer(frames, F, H, W, scale, iters, 1, flow_out, rgb_out, maxdisp_out, mask_out, alpha1, alpha2);
}

int pb_flow_infer_sequence_masks(pb_ctx *c, const uint8_t *frames, int F, int H, int W, float scale, int iters, float alpha1,
                                 float alpha2, float *flow_out, uint8_t *rgb_out, float *maxdisp_out, uint8_t *mask_out) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow_raft band");
    PB_CHECK(frames && F >= 2 && H > 0 && W > 0 && mask_out, PB_ERR_ARG, "flow masks: bad arguments");
    return flow_host_pipeline(c, frames, F, H, W, scale, iters, 1, flow_out, rgb_out, maxdisp_out, mask_out, alpha1, alpha2);
}

int pb_flow_submit_sequence_masks(pb_ctx *c, const uint8_t *frames, int F, int H, int W, float scale, int iters, float alpha1,
                                  float alpha2, float *flow_out, uint8_t *rgb_out, float *maxdisp_out, uint8_t *mask_out) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow_raft band");
    PB_CHECK(frames && F >= 2 && H > 0 && W > 0 && mask_out, PB_ERR_ARG, "flow masks submit: bad arguments");
    return flow_host_pipeline(c, frames, F, H, W, scale, iters, 1, flow_out, rgb_out, maxdisp_out, mask_out, alpha1, alpha2, true);
}

int pb_flow_fwdbwd_mask(pb_ctx *c, const float *flows, int n, int sh, int sw, float alpha1, float alpha2, uint8_t *mask_out) {
    PB_CHECK(c && flows && mask_out && n > 0 && sh > 0 && sw > 0, PB_ERR_ARG, "fwdbwd_mask: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const size_t px = (size_t)n * 2 * sh * sw;
    DevMem dO, dK;
    PB_TRY(dO.alloc(px * 8));
    PB_TRY(dK.alloc(px));
    PB_HIP(hipMemcpy(dO.p, flows, px * 8, hipMemcpyHostToDevice));
    PB_TRY(launch_fwdbwd_mask(c->stream, dO.as<float>(), n, sh, sw, alpha1, alpha2, dK.as<uint8_t>()));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(mask_out, dK.p, px, hipMemcpyDeviceToHost));
    return 0;
}

int pb_mask_net_size(const pb_mask_cfg *cfg, int H, int W, int *nh, int *nw, int *Hp, int *Wp) {
    PB_CHECK(cfg && H > 0 && W > 0 && nh && nw && Hp && Wp, PB_ERR_ARG, "mask_net_size: bad arguments");
    MaskEngine::net_size(*cfg, H, W, nh, nw, Hp, Wp);
    return 0;
}

int pb_mask_infer_batch_dev(pb_ctx *c, const uint8_t *frames, int n, int H, int W, float confidence, const int32_t *keep,
                            int n_keep, uint8_t *mask_out) {
    PB_CHECK(c && c->mask, PB_ERR_STATE, "ctx has no mask_mmdet band");
    return c->mask->infer(frames, n, H, W, confidence, keep, n_keep, mask_out);
}

// Host-pointer variant (reference loop bands/mask_mmdet.py:131-154: a decoded frame per iteration): frames of every chunk go to HBM on a copy
// stream up front, chunk i's kernels wait for chunk i's copy, and its id images (with the --sdf channel when tables are set) return on a second
// copy stream while chunk i + 1 runs; device buffers, pinned staging and streams are kept on the ctx (rounds 1-5: two hipMalloc / hipFree pairs
// and two exposed whole-batch copies per call).  Page-locked caller buffers are used directly.
int pb_mask_infer_batch(pb_ctx *c, const uint8_t *frames, int n, int H, int W, float confidence, const int32_t *keep,
                        int n_keep, uint8_t *mask_out) {
    PB_CHECK(c && c->mask, PB_ERR_STATE, "ctx has no mask_mmdet band");
    PB_CHECK(frames && mask_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "mask infer: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const size_t fb = (size_t)H * W * 3, bytes = (size_t)n * fb;
    const int cf = c->mask->frames_per_chunk(), chunks = (n + cf - 1) / cf;
    // pb_set_frame_format / pb_set_out_format: the copies move planar YUV frames (fi / fo bytes each) into / out of whole-batch buffers (ctx yuv[0] / yuv[1]);
    // the chunk's frames are converted into d_in once its copy has arrived, its id images out of d_out before they leave - both on the ctx stream
    const bool yin = c->frames_i420 != 0, yout = c->rgb_out_i420 != 0;
    const size_t fi = yin ? (size_t)yuv_frame_bytes(c->frame_fmt, H, W) : fb, fo = yout ? (size_t)yuv_frame_bytes(c->out_fmt, H, W) : fb;
    const bool pin_in = pb_is_pinned(frames, n * fi), pin_out = pb_is_pinned(mask_out, n * fo);
    MaskPipe &mp = c->mpipe;
    PB_TRY(mp.ensure(bytes, n * fi, n * fo, !pin_in, !pin_out, chunks));        // h_in / h_out by the frames' own size: up to 6 bytes per pixel, not RGB's 3
    if (yin) PB_TRY(c->yuv_grow(0, n * fi));
    if (yout) PB_TRY(c->yuv_grow(1, n * fo));
    PipeDrain drain{mp.s_in, c->stream, mp.s_out};              // no exit, error or not, leaves a copy into caller memory in flight
    char *up = yin ? (char *)c->yuv[0] : (char *)mp.d_in, *down = yout ? (char *)c->yuv[1] : (char *)mp.d_out;
    for (int i = 0; i < chunks; ++i) {
        const size_t off = (size_t)i * cf * fi, len = (size_t)std::min(cf, n - i * cf) * fi;
        const void *src = frames + off;
        if (!pin_in) { memcpy((char *)mp.h_in + off, src, len); src = (char *)mp.h_in + off; }
        PB_HIP(hipMemcpyAsync(up + off, src, len, hipMemcpyHostToDevice, mp.s_in));
        PB_HIP(hipEventRecord(mp.ev_in[i], mp.s_in));
    }
    hipStream_t st = c->stream;
    char *dst = pin_out ? (char *)mask_out : (char *)mp.h_out;
    const pb_yuv_fmt ffmt = c->frame_fmt, ofmt = c->out_fmt;
    c->mask->chunk_begin = [&mp, st, cf, yin, up, fi, fb, H, W, ffmt](int first, int m) -> int {
        PB_HIP(hipStreamWaitEvent(st, mp.ev_in[first / cf], 0));
        if (yin) PB_TRY(launch_yuv_to_rgb(st, ffmt, (const uint8_t *)up + (size_t)first * fi, m, H, W, (uint8_t *)mp.d_in + (size_t)first * fb));
        return 0;
    };
    c->mask->chunk_end = [&mp, st, cf, fb, fo, dst, yout, down, H, W, ofmt](int first, int m) -> int {
        const size_t off = (size_t)first * fo;
        if (yout) PB_TRY(launch_rgb_to_yuv(st, ofmt, (const uint8_t *)mp.d_out + (size_t)first * fb, m, H, W, (uint8_t *)down + off));
        PB_HIP(hipEventRecord(mp.ev_done[first / cf], st));
        PB_HIP(hipStreamWaitEvent(mp.s_out, mp.ev_done[first / cf], 0));
        PB_HIP(hipMemcpyAsync(dst + off, down + off, (size_t)m * fo, hipMemcpyDeviceToHost, mp.s_out));
        return 0;
    };
    const int r = c->mask->infer((const uint8_t *)mp.d_in, n, H, W, confidence, keep, n_keep, (uint8_t *)mp.d_out);
    c->mask->chunk_begin = nullptr; c->mask->chunk_end = nullptr;     // (an argument error returns before infer() consumes them)
    if (r) return r;
    PB_HIP(hipStreamSynchronize(mp.s_out));
    if (!pin_out) memcpy(mask_out, mp.h_out, n * fo);
    return 0;
}

int pb_mask_set_sdf(pb_ctx *c, const uint8_t *tab_out, const uint8_t *tab_in, int n_tab) {
    PB_CHECK(c && c->mask, PB_ERR_STATE, "ctx has no mask_mmdet band");
    PB_CHECK(n_tab <= 0 || (tab_out && tab_in && n_tab >= 2 && n_tab <= 4226), PB_ERR_ARG, "mask set_sdf: bad tables (n_tab = %d)", n_tab);
    return c->mask->set_sdf(tab_out, tab_in, n_tab);
}

int pb_mask_sdf_green_dev(pb_ctx *c, uint8_t *masks, int n, int H, int W) {
    PB_CHECK(c && c->mask, PB_ERR_STATE, "ctx has no mask_mmdet band");
    return c->mask->sdf_green(masks, n, H, W);
}

int pb_mask_sdf_green(pb_ctx *c, uint8_t *masks, int n, int H, int W) {
    PB_CHECK(c && c->mask, PB_ERR_STATE, "ctx has no mask_mmdet band");
    PB_CHECK(masks && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "mask sdf: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)n * H * W * 3;
    DevMem d;
    PB_TRY(d.alloc(bytes));
    PB_HIP(hipMemcpy(d.p, masks, bytes, hipMemcpyHostToDevice));
    PB_TRY(c->mask->sdf_green(d.as<uint8_t>(), n, H, W));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(masks, d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int pb_mask_get_instances(pb_ctx *c, int frame, int cap, float *scores_out, int32_t *labels_out, uint8_t *masks_out,
                          int32_t *candidates_out) {
    PB_CHECK(c && c->mask, PB_ERR_STATE, "ctx has no mask_mmdet band");
    const auto &res = c->mask->results();
    PB_CHECK(frame >= 0 && frame < (int)res.size(), PB_ERR_ARG, "mask instances: frame %d of %zu", frame, res.size());
    const auto &r = res[frame];
    const int cnt = std::min<int>(cap, (int)r.scores.size());
    for (int i = 0; i < cnt; ++i) {
        if (scores_out) scores_out[i] = r.scores[i];
        if (labels_out) labels_out[i] = r.labels[i];
    }
    if (masks_out && cnt > 0) {
        PB_CHECK(!r.masks.empty(), PB_ERR_STATE, "instance masks are kept only with pb_set_profiling(ctx, 2)");
        memcpy(masks_out, r.masks.data(), r.masks.size() / r.scores.size() * cnt);
    }
    if (candidates_out) *candidates_out = r.candidates;
    return (int)r.scores.size();
}

int64_t pb_mask_get_stage(pb_ctx *c, const char *name, float *out, int64_t cap, int64_t shape_out[4]) {
    return band_stage(c, c ? c->mask : nullptr, "mask ", name, out, cap, shape_out);
}

int pb_flow_set_inference_size(pb_ctx *c, int h, int w) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow band");
    GmflowEngine *g = dynamic_cast<GmflowEngine *>(c->flow);
    PB_CHECK(g, PB_ERR_STATE, "--inference_size is a flow_gmflow option");
    return g->set_inference_size(h, w);
}

int pb_flow_set_matching(pb_ctx *c, int corr_radius, int prop_radius) {
    PB_CHECK(c && c->flow, PB_ERR_STATE, "ctx has no flow band");
    GmflowEngine *g = dynamic_cast<GmflowEngine *>(c->flow);
    PB_CHECK(g, PB_ERR_STATE, "--corr_radius_list / --prop_radius_list are flow_gmflow options");
    return g->set_matching(corr_radius, prop_radius);
}

int pb_flow_num_scales(pb_ctx *c) {
    PB_CHECK(c && c->flow, PB_ERR_ARG, "ctx has no flow band");
    GmflowEngine *g = dynamic_cast<GmflowEngine *>(c->flow);
    PB_CHECK(g, PB_ERR_ARG, "num_scales is a flow_gmflow property");
    return g->num_scales();
}

int pb_flow_set_alternate_corr(pb_ctx *c, int on) {
    PB_CHECK(c && c->flow, PB_ERR_ARG, "ctx has no flow band");
    RaftEngine *e = dynamic_cast<RaftEngine *>(c->flow);
    PB_CHECK(e, PB_ERR_ARG, "--alternate_corr is a flow_raft option");
    e->set_alternate_corr(on);
    return 0;
}

int64_t pb_flow_arena_bytes(pb_ctx *c) {
    PB_CHECK(c && c->flow, PB_ERR_ARG, "ctx has no flow band");
    return c->flow->plan_bytes();
}

int64_t pb_flow_get_stage(pb_ctx *c, const char *name, float *out, int64_t cap, int64_t shape_out[4]) {
    return band_stage(c, c ? c->flow : nullptr, "flow ", name, out, cap, shape_out);
}

int pb_set_option(pb_ctx *c, const char *key, int value) {
    PB_CHECK(c && key, PB_ERR_ARG, "set_option: bad arguments");
    if (!strcmp(key, "gemm_tile")) (c->band ? c->band->dense_tile : c->gemm_tile) = value;
    else if (!strcmp(key, "conv_tile")) (c->band ? c->band->conv_tile : c->conv_tile) = value;
    else if (!strcmp(key, "host_chunk")) c->host_chunk = value;
    else if (!strcmp(key, "op_splitk")) c->op_splitk = value;
    else if (!strcmp(key, "frames_i420") || !strcmp(key, "rgb_out_i420") || !strcmp(key, "rgb_out_full")) {
        PB_CHECK(value == 0 || value == 1, PB_ERR_ARG, "option '%s' is 0 or 1, not %d", key, value);
        PB_CHECK(c->pending.empty(), PB_ERR_STATE, "option '%s': a submission of this ctx is still outstanding (pb_wait first)", key);
        (key[0] == 'f' ? c->frames_i420 : key[8] == 'i' ? c->rgb_out_i420 : c->rgb_out_full) = value;
        if (key[0] == 'f') c->frame_fmt = pb_yuv_fmt{420, 8, 0, PB_YUV_BT601};      // pb_set_frame_format's special case
        else if (key[8] == 'i') c->out_fmt = pb_yuv_fmt{420, 8, 0, PB_YUV_BT601};   // pb_set_out_format's
    }
    else if (!strcmp(key, "corr_layout")) {        // corr_layout.h: 1 = source-blocked volume (default), 0 = row-major; the next flow_raft call re-plans
        PB_CHECK(value == 0 || value == 1, PB_ERR_ARG, "option '%s' is 0 or 1, not %d", key, value);
        PB_CHECK(c->pending.empty(), PB_ERR_STATE, "option '%s': a submission of this ctx is still outstanding (pb_wait first)", key);
        c->corr_layout = value;
        if (RaftEngine *e = dynamic_cast<RaftEngine *>(c->flow)) e->set_corr_layout(value);
    }
    else if (!strcmp(key, "tile_n96")) pb_gemm_set_n96(value);         // process-wide (gemm.h): A/B of the 128 x 96 tile inside one test process
    else PB_CHECK(false, PB_ERR_ARG, "unknown option '%s'", key);
    return 0;
}

int pb_get_kernel_stats(pb_ctx *c, pb_kernel_stat *out, int cap) {
    PB_CHECK(c && c->band && out, PB_ERR_STATE, "ctx has no band");
    return c->band->stats(out, cap);
}

int pb_dev_alloc(pb_ctx *c, void **ptr, size_t bytes) {
    PB_CHECK(c && ptr, PB_ERR_ARG, "dev_alloc: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    hipError_t e = hipMalloc(ptr, bytes);
    PB_CHECK(e == hipSuccess, PB_ERR_MEMORY, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return 0;
}
int pb_dev_free(pb_ctx *c, void *ptr) {
    PB_CHECK(c, PB_ERR_ARG, "null ctx");
    PB_HIP(hipSetDevice(c->device));
    PB_HIP(hipFree(ptr));
    return 0;
}
int pb_host_alloc(pb_ctx *c, void **ptr, size_t bytes) {
    PB_CHECK(c && ptr, PB_ERR_ARG, "host_alloc: bad arguments");
    *ptr = nullptr;
    PB_HIP(hipSetDevice(c->device));
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) (void)hipGetLastError();
    PB_CHECK(e == hipSuccess && p, PB_ERR_MEMORY, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    std::lock_guard<std::mutex> lock(c->host_mu);
    c->host_blocks.push_back(p);
    *ptr = p;
    return 0;
}
int pb_host_free(pb_ctx *c, void *ptr) {
    PB_CHECK(c, PB_ERR_ARG, "null ctx");
    {
        std::lock_guard<std::mutex> lock(c->host_mu);
        auto it = std::find(c->host_blocks.begin(), c->host_blocks.end(), ptr);
        PB_CHECK(ptr && it != c->host_blocks.end(), PB_ERR_ARG, "host_free: %p is not a block pb_host_alloc gave this ctx", ptr);
        c->host_blocks.erase(it);
    }
    PB_HIP(hipSetDevice(c->device));
    PB_HIP(hipHostFree(ptr));
    return 0;
}
int pb_memcpy_h2d(pb_ctx *c, void *dst, const void *src, size_t bytes) {
    PB_CHECK(c, PB_ERR_ARG, "null ctx");
    PB_HIP(hipSetDevice(c->device));
    PB_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
int pb_memcpy_d2h(pb_ctx *c, void *dst, const void *src, size_t bytes) {
    PB_CHECK(c, PB_ERR_ARG, "null ctx");
    PB_HIP(hipSetDevice(c->device));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int pb_depth_encode_still(pb_ctx *c, const float *depth, int H, int W, int flip, int encode_range, uint8_t *rgb_out, float *min_out,
                          float *max_out) {
    PB_CHECK(c && depth && rgb_out && H > 0 && W > 0, PB_ERR_ARG, "depth_encode_still: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lock(c->still_mu);
    const size_t px = (size_t)H * W;
    // [depth f32 | rgb u8 x 3 | quantised u8 | 64 bytes of min / max words], each part 256-byte aligned
    const size_t o_rgb = round_up(px * 4, 256), o_q = o_rgb + round_up(px * 3, 256), o_mm = o_q + round_up(px, 256), need = o_mm + 256;
    if (!c->still_stream) PB_HIP(hipStreamCreateWithFlags(&c->still_stream, hipStreamNonBlocking));
    if (need > c->still_cap) {
        if (c->still_buf) { PB_HIP(hipStreamSynchronize(c->still_stream)); PB_HIP(hipFree(c->still_buf)); c->still_buf = nullptr; c->still_cap = 0; }
        PB_HIP(hipMalloc((void **)&c->still_buf, need));
        c->still_cap = need;
    }
    hipStream_t st = c->still_stream;
    PB_HIP(hipMemsetAsync(c->still_buf + o_mm, 0, 256, st));
    PB_HIP(hipMemcpyAsync(c->still_buf, depth, px * 4, hipMemcpyHostToDevice, st));
    unsigned *mm = (unsigned *)(c->still_buf + o_mm);
    PB_TRY(launch_still_encode(st, (const float *)c->still_buf, H, W, mm, mm + 2, (uint8_t *)(c->still_buf + o_q), flip, encode_range,
                               (uint8_t *)(c->still_buf + o_rgb), (float *)(mm + 4)));
    float mnmx[2];
    PB_HIP(hipMemcpyAsync(rgb_out, c->still_buf + o_rgb, px * 3, hipMemcpyDeviceToHost, st));
    PB_HIP(hipMemcpyAsync(mnmx, mm + 4, 8, hipMemcpyDeviceToHost, st));
    PB_HIP(hipStreamSynchronize(st));
    if (min_out) *min_out = mnmx[0];
    if (max_out) *max_out = mnmx[1];
    return 0;
}

int pb_depth_point_cloud_dev(pb_ctx *c, const float *depth, const uint8_t *rgb, int n, int H, int W, int flip, float u0, float v0, float fx,
                             float fy, uint8_t *vertices_out) {
    PB_CHECK(c && depth && rgb && vertices_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "depth_point_cloud: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    if (flip && n > c->pcl_mm_cap) {
        if (c->pcl_mm) { PB_HIP(hipStreamSynchronize(c->stream)); PB_HIP(hipFree(c->pcl_mm)); c->pcl_mm = nullptr; c->pcl_mm_cap = 0; }
        PB_HIP(hipMalloc((void **)&c->pcl_mm, (size_t)n * 8));
        c->pcl_mm_cap = n;
    }
    // with a band on the ctx and pb_set_profiling on, the call is one record of pb_get_kernel_stats (22 algorithmic bytes per pixel)
    KernelTimer *t = c->band ? &c->band->timer : nullptr;
    if (t && !t->enabled) t = nullptr;
    if (t) {
        t->reset();
        t->recs.push_back(KernelTimer::Rec{0, t->get(), t->get(), 0.0, 22.0 * n * H * W, 0.0, "depth_point_cloud"});
        PB_HIP(hipEventRecord(t->recs.back().a, c->stream));
    }
    const int r = launch_point_cloud(c->stream, depth, rgb, n, H, W, flip, u0, v0, fx, fy, c->pcl_mm, vertices_out);
    if (t) PB_HIP(hipEventRecord(t->recs.back().b, c->stream));
    return r;
}

int pb_depth_point_cloud(pb_ctx *c, const float *depth, const uint8_t *rgb, int n, int H, int W, int flip, float u0, float v0, float fx,
                         float fy, uint8_t *vertices_out) {
    PB_CHECK(c && depth && rgb && vertices_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "depth_point_cloud: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lock(c->still_mu);
    const size_t px = (size_t)n * H * W;
    // [depth f32 | rgb u8 x 3 | vertices 15 bytes | min / max words], each part 256-byte aligned
    const size_t o_rgb = round_up(px * 4, 256), o_v = o_rgb + round_up(px * 3, 256), o_mm = o_v + round_up(px * 15, 256),
                 need = o_mm + round_up((size_t)n * 8, 256);
    if (!c->still_stream) PB_HIP(hipStreamCreateWithFlags(&c->still_stream, hipStreamNonBlocking));
    if (need > c->still_cap) {
        if (c->still_buf) { PB_HIP(hipStreamSynchronize(c->still_stream)); PB_HIP(hipFree(c->still_buf)); c->still_buf = nullptr; c->still_cap = 0; }
        PB_HIP(hipMalloc((void **)&c->still_buf, need));
        c->still_cap = need;
    }
    hipStream_t st = c->still_stream;
    PB_HIP(hipMemcpyAsync(c->still_buf, depth, px * 4, hipMemcpyHostToDevice, st));
    PB_HIP(hipMemcpyAsync(c->still_buf + o_rgb, rgb, px * 3, hipMemcpyHostToDevice, st));
    const int r = launch_point_cloud(st, (const float *)c->still_buf, (const uint8_t *)(c->still_buf + o_rgb), n, H, W, flip, u0, v0, fx, fy,
                                     (unsigned *)(c->still_buf + o_mm), (uint8_t *)(c->still_buf + o_v));
    if (!r) PB_HIP(hipMemcpyAsync(vertices_out, c->still_buf + o_v, px * 15, hipMemcpyDeviceToHost, st));
    PB_HIP(hipStreamSynchronize(st));
    return r;
}

// ---- rgba band: side-by-side RGB-D captures (bands/rgba.py:24-75) ------------------------------------------------------------
int pb_rgbd_boxes(int H, int W, int side, int rgb_box[4], int depth_box[4]) {
    PB_CHECK(rgb_box && depth_box, PB_ERR_ARG, "rgbd_boxes: null box");
    PB_CHECK(side >= 0 && side <= 3, PB_ERR_ARG, "rgbd_boxes: side %d unknown (0 left, 1 right, 2 top, 3 bottom: where the depth is)", side);
    PB_CHECK(H > 0 && W > 0 && (side < 2 ? W : H) >= 2, PB_ERR_ARG, "rgbd_boxes: a %d x %d frame has no %s half", H, W,
             side == 0 ? "left" : (side == 1 ? "right" : (side == 2 ? "top" : "bottom")));
    // int(width / 2), int(height / 2) of rgba.py:29-40 as the slice bounds of :58-59: the half that starts at the middle takes the odd column / row
    const int k = (side < 2 ? W : H) / 2;
    int first[4] = {0, H, 0, W}, second[4] = {0, H, 0, W};
    if (side < 2) { first[3] = k; second[2] = k; } else { first[1] = k; second[0] = k; }
    const bool depth_first = side == 0 || side == 2;
    for (int i = 0; i < 4; ++i) {
        depth_box[i] = depth_first ? first[i] : second[i];
        rgb_box[i] = depth_first ? second[i] : first[i];
    }
    return 0;
}

int pb_rgbd_depth_dev(pb_ctx *c, const uint8_t *frames, int n, int H, int W, int side, uint8_t *depth_out, float *heat_out) {
    PB_CHECK(c && frames && (depth_out || heat_out) && n > 0, PB_ERR_ARG, "rgbd_depth: bad arguments");
    int rb[4], db[4];
    PB_TRY(pb_rgbd_boxes(H, W, side, rb, db));
    PB_HIP(hipSetDevice(c->device));
    return launch_hue_heat(c->stream, frames, n, H, W, db[0], db[2], db[1] - db[0], db[3] - db[2], depth_out, heat_out);
}

// Host-pointer variant: run_chunks over chunks of "host_chunk" (default 8) frames; lanes: the frames in, the two results out.
int pb_rgbd_depth(pb_ctx *c, const uint8_t *frames, int n, int H, int W, int side, uint8_t *depth_out, float *heat_out) {
    PB_CHECK(c && frames && (depth_out || heat_out) && n > 0, PB_ERR_ARG, "rgbd_depth: bad arguments");
    int rb[4], db[4];
    PB_TRY(pb_rgbd_boxes(H, W, side, rb, db));
    PB_HIP(hipSetDevice(c->device));
    const int Hd = db[1] - db[0], Wd = db[3] - db[2];
    const size_t px = (size_t)H * W, pd = (size_t)Hd * Wd;
    const int cap = std::min(n, c->host_chunk > 0 ? c->host_chunk : 8);
    const ChunkLane lanes[3] = {{(void *)frames, px * 3, false, pb_is_pinned(frames, (size_t)n * px * 3)},
                                {depth_out, depth_out ? pd * 3 : 0, true, pb_is_pinned(depth_out, (size_t)n * pd * 3)},
                                {heat_out, heat_out ? pd * 4 : 0, true, pb_is_pinned(heat_out, (size_t)n * pd * 4)}};
    const ChunkPipe::Lane *l = c->pipe.lane;
    return run_chunks(c, n, cap, 0, lanes, 3, false, [&](int slot, int, int m) {
        return launch_hue_heat(c->stream, (const uint8_t *)l[0].d[slot], m, H, W, db[0], db[2], Hd, Wd,
                               (uint8_t *)(depth_out ? l[1].d[slot] : nullptr), (float *)(heat_out ? l[2].d[slot] : nullptr));
    });
}

// ---- I420 <-> RGB on their own (yuv.hip): .y4m frames for callers that hold them, the still dumps, the tests --------------------------------
int64_t pb_i420_bytes(int H, int W) { return i420_frame_bytes(H, W); }

int pb_i420_to_rgb_dev(pb_ctx *c, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out) {
    PB_CHECK(c && yuv && rgb_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "i420_to_rgb: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    return launch_i420_to_rgb(c->stream, yuv, n, H, W, rgb_out);
}

int pb_rgb_to_i420_dev(pb_ctx *c, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out) {
    PB_CHECK(c && rgb && yuv_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "rgb_to_i420: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    return launch_rgb_to_i420(c->stream, rgb, n, H, W, yuv_out);
}

// Host-pointer variants: run_chunks over chunks of "host_chunk" (default 8) frames; lanes: the frames in, the converted frames out.
static int yuv_host_pipeline(pb_ctx *c, const uint8_t *in, int n, int H, int W, uint8_t *out, bool to_rgb) {
    PB_CHECK(c && in && out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "%s: bad arguments", to_rgb ? "i420_to_rgb" : "rgb_to_i420");
    PB_CHECK(c->pending.empty(), PB_ERR_STATE, "%s: a submission of this ctx is still outstanding (pb_wait first)", to_rgb ? "i420_to_rgb" : "rgb_to_i420");
    PB_HIP(hipSetDevice(c->device));
    const size_t fy = (size_t)i420_frame_bytes(H, W), fr = (size_t)H * W * 3, fi = to_rgb ? fy : fr, fo = to_rgb ? fr : fy;
    const int cap = std::min(n, c->host_chunk > 0 ? c->host_chunk : 8);
    const ChunkLane lanes[2] = {{(void *)in, fi, false, pb_is_pinned(in, n * fi)}, {out, fo, true, pb_is_pinned(out, n * fo)}};
    const ChunkPipe::Lane *l = c->pipe.lane;
    return run_chunks(c, n, cap, 0, lanes, 2, false, [&](int slot, int, int m) {
        return to_rgb ? launch_i420_to_rgb(c->stream, (const uint8_t *)l[0].d[slot], m, H, W, (uint8_t *)l[1].d[slot])
                      : launch_rgb_to_i420(c->stream, (const uint8_t *)l[0].d[slot], m, H, W, (uint8_t *)l[1].d[slot]);
    });
}

int pb_i420_to_rgb(pb_ctx *c, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out) { return yuv_host_pipeline(c, yuv, n, H, W, rgb_out, true); }
int pb_rgb_to_i420(pb_ctx *c, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out) { return yuv_host_pipeline(c, rgb, n, H, W, yuv_out, false); }

// ---- any .y4m layout -> RGB (yuv_formats.hip): on its own, and as the frame format of a band ctx ------------------------------------------------
int64_t pb_yuv_bytes(const pb_yuv_fmt *fmt, int H, int W) { return fmt ? yuv_frame_bytes(*fmt, H, W) : 0; }

int pb_yuv_coeffs(const pb_yuv_fmt *fmt, int32_t out[7]) {
    PB_CHECK(fmt && out, PB_ERR_ARG, "yuv_coeffs: bad arguments");
    PB_CHECK(yuv_fmt_ok(*fmt), PB_ERR_ARG, "yuv_coeffs: no such format (chroma %d, depth %d, full_range %d, matrix %d)", fmt->chroma, fmt->depth,
             fmt->full_range, fmt->matrix);
    yuv_coeffs(*fmt, out);
    return 0;
}

int pb_yuv_to_rgb_dev(pb_ctx *c, const pb_yuv_fmt *fmt, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out) {
    PB_CHECK(c && fmt && yuv && rgb_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "yuv_to_rgb: bad arguments");
    PB_CHECK(yuv_fmt_ok(*fmt), PB_ERR_ARG, "yuv_to_rgb: no such format (chroma %d, depth %d, full_range %d, matrix %d)", fmt->chroma, fmt->depth,
             fmt->full_range, fmt->matrix);
    PB_HIP(hipSetDevice(c->device));
    return launch_yuv_to_rgb(c->stream, *fmt, yuv, n, H, W, rgb_out);
}

// Host-pointer variant: run_chunks over chunks of "host_chunk" (default 8) frames, as pb_i420_to_rgb.
int pb_yuv_to_rgb(pb_ctx *c, const pb_yuv_fmt *fmt, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out) {
    PB_CHECK(c && fmt && yuv && rgb_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "yuv_to_rgb: bad arguments");
    PB_CHECK(yuv_fmt_ok(*fmt), PB_ERR_ARG, "yuv_to_rgb: no such format (chroma %d, depth %d, full_range %d, matrix %d)", fmt->chroma, fmt->depth,
             fmt->full_range, fmt->matrix);
    PB_CHECK(c->pending.empty(), PB_ERR_STATE, "yuv_to_rgb: a submission of this ctx is still outstanding (pb_wait first)");
    PB_HIP(hipSetDevice(c->device));
    const pb_yuv_fmt f = *fmt;
    const size_t fi = (size_t)yuv_frame_bytes(f, H, W), fo = (size_t)H * W * 3;
    const int cap = std::min(n, c->host_chunk > 0 ? c->host_chunk : 8);
    const ChunkLane lanes[2] = {{(void *)yuv, fi, false, pb_is_pinned(yuv, n * fi)}, {rgb_out, fo, true, pb_is_pinned(rgb_out, n * fo)}};
    const ChunkPipe::Lane *l = c->pipe.lane;
    return run_chunks(c, n, cap, 0, lanes, 2, false, [&](int slot, int, int m) {
        return launch_yuv_to_rgb(c->stream, f, (const uint8_t *)l[0].d[slot], m, H, W, (uint8_t *)l[1].d[slot]);
    });
}

int pb_set_frame_format(pb_ctx *c, const pb_yuv_fmt *fmt) {
    PB_CHECK(c, PB_ERR_ARG, "set_frame_format: null ctx");
    PB_CHECK(!fmt || yuv_fmt_ok(*fmt), PB_ERR_ARG, "set_frame_format: no such format (chroma %d, depth %d, full_range %d, matrix %d)", fmt->chroma,
             fmt->depth, fmt->full_range, fmt->matrix);
    PB_CHECK(c->pending.empty(), PB_ERR_STATE, "set_frame_format: a submission of this ctx is still outstanding (pb_wait first)");
    c->frames_i420 = fmt != nullptr;
    if (fmt) c->frame_fmt = *fmt;
    return 0;
}

// ---- RGB -> any .y4m layout (yuv_out.hip): on its own, and as the format of a band ctx's rgb_out ----------------------------------------------------
#define PB_CHECK_FMT(what, fmt) \
    PB_CHECK(yuv_fmt_ok(*(fmt)), PB_ERR_ARG, what ": no such format (chroma %d, depth %d, full_range %d, matrix %d)", (fmt)->chroma, (fmt)->depth, \
             (fmt)->full_range, (fmt)->matrix)

int pb_yuv_fwd_coeffs(const pb_yuv_fmt *fmt, int32_t out[12]) {
    PB_CHECK(fmt && out, PB_ERR_ARG, "yuv_fwd_coeffs: bad arguments");
    PB_CHECK_FMT("yuv_fwd_coeffs", fmt);
    yuv_fwd_coeffs(*fmt, out);
    return 0;
}

int pb_rgb_to_yuv_dev(pb_ctx *c, const pb_yuv_fmt *fmt, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out) {
    PB_CHECK(c && fmt && rgb && yuv_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "rgb_to_yuv: bad arguments");
    PB_CHECK_FMT("rgb_to_yuv", fmt);
    PB_HIP(hipSetDevice(c->device));
    return launch_rgb_to_yuv(c->stream, *fmt, rgb, n, H, W, yuv_out);
}

// Host-pointer variant: run_chunks over chunks of "host_chunk" (default 8) frames, as pb_rgb_to_i420.
int pb_rgb_to_yuv(pb_ctx *c, const pb_yuv_fmt *fmt, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out) {
    PB_CHECK(c && fmt && rgb && yuv_out && n > 0 && H > 0 && W > 0, PB_ERR_ARG, "rgb_to_yuv: bad arguments");
    PB_CHECK_FMT("rgb_to_yuv", fmt);
    PB_CHECK(c->pending.empty(), PB_ERR_STATE, "rgb_to_yuv: a submission of this ctx is still outstanding (pb_wait first)");
    PB_HIP(hipSetDevice(c->device));
    const pb_yuv_fmt f = *fmt;
    const size_t fi = (size_t)H * W * 3, fo = (size_t)yuv_frame_bytes(f, H, W);
    const int cap = std::min(n, c->host_chunk > 0 ? c->host_chunk : 8);
    const ChunkLane lanes[2] = {{(void *)rgb, fi, false, pb_is_pinned(rgb, n * fi)}, {yuv_out, fo, true, pb_is_pinned(yuv_out, n * fo)}};
    const ChunkPipe::Lane *l = c->pipe.lane;
    return run_chunks(c, n, cap, 0, lanes, 2, false, [&](int slot, int, int m) {
        return launch_rgb_to_yuv(c->stream, f, (const uint8_t *)l[0].d[slot], m, H, W, (uint8_t *)l[1].d[slot]);
    });
}

int pb_set_out_format(pb_ctx *c, const pb_yuv_fmt *fmt) {
    PB_CHECK(c, PB_ERR_ARG, "set_out_format: null ctx");
    if (fmt) PB_CHECK_FMT("set_out_format", fmt);
    PB_CHECK(c->pending.empty(), PB_ERR_STATE, "set_out_format: a submission of this ctx is still outstanding (pb_wait first)");
    c->rgb_out_i420 = fmt != nullptr;
    if (fmt) c->out_fmt = *fmt;
    return 0;
}

// ---- bilinear RGB resize on its own (resize.hip): what "rgb_out_full" runs behind the flow bands, for callers that hold frames, and the tests ----
int pb_rgb_resize_dev(pb_ctx *c, const uint8_t *rgb, int n, int sh, int sw, int H, int W, uint8_t *out, int out_i420) {
    PB_CHECK(c && rgb && out && n > 0 && sh > 0 && sw > 0 && H > 0 && W > 0, PB_ERR_ARG, "rgb_resize: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    return launch_rgb_resize(c->stream, rgb, n, sh, sw, H, W, out, out_i420 != 0);
}

// Host-pointer variant: run_chunks over chunks of "host_chunk" (default 8) frames; lanes: the frames in, the resized frames out.
int pb_rgb_resize(pb_ctx *c, const uint8_t *rgb, int n, int sh, int sw, int H, int W, uint8_t *out, int out_i420) {
    PB_CHECK(c && rgb && out && n > 0 && sh > 0 && sw > 0 && H > 0 && W > 0, PB_ERR_ARG, "rgb_resize: bad arguments");
    PB_CHECK(c->pending.empty(), PB_ERR_STATE, "rgb_resize: a submission of this ctx is still outstanding (pb_wait first)");
    PB_HIP(hipSetDevice(c->device));
    const size_t fi = (size_t)sh * sw * 3, fo = out_i420 ? (size_t)i420_frame_bytes(H, W) : (size_t)H * W * 3;
    const int cap = std::min(n, c->host_chunk > 0 ? c->host_chunk : 8);
    const ChunkLane lanes[2] = {{(void *)rgb, fi, false, pb_is_pinned(rgb, n * fi)}, {out, fo, true, pb_is_pinned(out, n * fo)}};
    const ChunkPipe::Lane *l = c->pipe.lane;
    return run_chunks(c, n, cap, 0, lanes, 2, false, [&](int slot, int, int m) {
        return launch_rgb_resize(c->stream, (const uint8_t *)l[0].d[slot], m, sh, sw, H, W, (uint8_t *)l[1].d[slot], out_i420 != 0);
    });
}

// ---- baseline JPEG frames out of planar YUV (jpeg.hip) ---------------------------------------------------------------------------------------------
#define PB_CHECK_JPEG(what, cfg, H, W)                                                                                                              \
    do {                                                                                                                                            \
        PB_CHECK(jpeg_cfg_ok(*(cfg)), PB_ERR_ARG, what ": no such format (chroma %d: 444, 420 or 400; quality %d: 1 .. 100)", (cfg)->chroma,       \
                 (cfg)->quality);                                                                                                                   \
        PB_CHECK((H) >= 1 && (W) >= 1 && (H) <= 65535 && (W) <= 65535, PB_ERR_ARG, what ": a %d x %d frame (a side is 1 .. 65535)", (H), (W));      \
    } while (0)

int64_t pb_jpeg_bound(const pb_jpeg_cfg *cfg, int H, int W) { return cfg ? jpeg_frame_bound(*cfg, H, W) : 0; }

int pb_jpeg_encode_dev(pb_ctx *c, const pb_jpeg_cfg *cfg, const uint8_t *planes, int n, int H, int W, uint8_t *out, int64_t capacity,
                       int64_t *offsets) {
    PB_CHECK(c && cfg && planes && out && offsets && n > 0 && capacity >= 0, PB_ERR_ARG, "jpeg_encode: bad arguments");
    PB_CHECK_JPEG("jpeg_encode", cfg, H, W);
    PB_HIP(hipSetDevice(c->device));
    return jpeg_encode_dev(c->jpeg, c->stream, *cfg, planes, n, H, W, out, capacity, offsets);
}

// Host-pointer variant: chunks of "host_chunk" (default 8) frames through two slots.  A chunk's planes go up on the pipe's copy-in stream while
// the chunk before is encoded; its offsets come back first, and then exactly the bytes of the frames that fit, on the copy-out stream.  Page-locked
// caller arrays are addressed by the copy engines directly; pageable ones go through the runtime's own staging (the copy then blocks this thread).
int pb_jpeg_encode(pb_ctx *c, const pb_jpeg_cfg *cfg, const uint8_t *planes, int n, int H, int W, uint8_t *out, int64_t capacity, int64_t *offsets) {
    PB_CHECK(c && cfg && planes && offsets && n > 0 && capacity >= 0 && (out || capacity == 0), PB_ERR_ARG, "jpeg_encode: bad arguments");
    PB_CHECK_JPEG("jpeg_encode", cfg, H, W);
    PB_CHECK(c->pending.empty(), PB_ERR_STATE, "jpeg_encode: a submission of this ctx is still outstanding (pb_wait first)");
    PB_HIP(hipSetDevice(c->device));
    const pb_jpeg_cfg f = *cfg;
    const pb_yuv_fmt yf = {f.chroma, 8, 1, PB_YUV_BT601};
    const size_t fb = (size_t)yuv_frame_bytes(yf, H, W);
    const int64_t bound = jpeg_frame_bound(f, H, W);
    const int per = std::min(n, c->host_chunk > 0 ? c->host_chunk : 8);
    const int64_t dcap = std::max<int64_t>(std::min<int64_t>((int64_t)per * bound, capacity), 16);
    ChunkPipe &p = c->pipe;
    PB_TRY(p.ensure_streams());
    PB_HIP(hipStreamSynchronize(c->stream));        // the slots may grow: nothing of an earlier _dev call may be in flight
    JpegState &j = c->jpeg;
    PB_TRY(j.grow_host((size_t)per * fb, (size_t)dcap, per));
    PipeDrain drain{p.s_in, c->stream, p.s_out};
    const int chunks = (n + per - 1) / per;
    auto copy_in = [&](int i) -> int {
        const int slot = i & 1, u0 = i * per, m = std::min(per, n - u0);
        PB_HIP(hipStreamWaitEvent(p.s_in, p.ev_comp[slot], 0));        // the encode that last read this slot
        PB_HIP(hipMemcpyAsync(j.d_in[slot], planes + (size_t)u0 * fb, (size_t)m * fb, hipMemcpyHostToDevice, p.s_in));
        PB_HIP(hipEventRecord(p.ev_h2d[slot], p.s_in));
        return 0;
    };
    int64_t total = 0;
    offsets[0] = 0;
    PB_TRY(copy_in(0));
    for (int i = 0; i < chunks; ++i) {
        const int slot = i & 1, u0 = i * per, m = std::min(per, n - u0);
        const int64_t room = std::min<int64_t>(dcap, std::max<int64_t>(capacity - total, 0));
        PB_HIP(hipStreamWaitEvent(c->stream, p.ev_h2d[slot], 0));
        PB_HIP(hipStreamWaitEvent(c->stream, p.ev_d2h[slot], 0));      // the copy that last emptied this slot's stream buffer
        PB_TRY(jpeg_encode_dev(j, c->stream, f, (const uint8_t *)j.d_in[slot], m, H, W, (uint8_t *)j.d_out[slot], room, j.d_offs[slot]));
        PB_HIP(hipMemcpyAsync(j.h_offs[slot], j.d_offs[slot], (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        PB_HIP(hipEventRecord(p.ev_comp[slot], c->stream));
        if (i + 1 < chunks) PB_TRY(copy_in(i + 1));
        PB_HIP(hipEventSynchronize(p.ev_comp[slot]));
        int64_t fit = 0;        // bytes of the chunk's frames that end within the caller's capacity: a prefix, the positions only grow
        for (int k = 0; k < m; ++k) {
            offsets[u0 + k + 1] = total + j.h_offs[slot][k + 1];
            if (offsets[u0 + k + 1] <= capacity) fit = j.h_offs[slot][k + 1];
        }
        if (fit > 0) PB_HIP(hipMemcpyAsync(out + total, j.d_out[slot], (size_t)fit, hipMemcpyDeviceToHost, p.s_out));
        PB_HIP(hipEventRecord(p.ev_d2h[slot], p.s_out));
        total = offsets[u0 + m];
    }
    PB_HIP(hipStreamSynchronize(p.s_out));
    PB_CHECK(total <= capacity, PB_ERR_MEMORY, "jpeg_encode: %d frames of %d x %d need %lld bytes, the buffer holds %lld (offsets[n] has the need)", n, H,
             W, (long long)total, (long long)capacity);
    return 0;
}

}  // extern "C"
