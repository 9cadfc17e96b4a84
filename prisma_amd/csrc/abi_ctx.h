// The context behind the C ABI and the small helpers its two translation units share: abi.hip (context lifetime, band entry points, host
// pipelines) and abi_ops.hip (the pb_op_* single-kernel entry points of the op-level tests).  Private: nothing outside those two includes it.
#pragma once
#include <deque>
#include <mutex>
#include <vector>

#include "engine.h"
#include "mask_engine.h"
#include "flow_engine.h"
#include "jpeg.h"
#include "resize.h"
#include "yuv.h"

void pb_cubic_taps(int src, int dst, int *idx, float *wt);   // engine.hip
void pb_bilinear_ac_taps(int src, int dst, int *idx, float *wt);   // engine.hip: the metric band's align-corners table, 4 taps of which two weigh 0

void pb_flow_cubic_taps(int src, int dst, float scale, std::vector<int> &idx, std::vector<int> &co);   // flow_engine.hip: the flow bands' 8-bit cubic table

#define PB_TRY(expr) do { int _r = (expr); if (_r) return _r; } while (0)

// Streams, events and double-buffered slots of the chunked host-pointer entry points (pb_depth_infer_batch, pb_flow_infer_sequence and their
// submit forms; run_chunks in abi.hip is the schedule).  A lane is one array of the call - the frames in, each result out - with a device
// buffer per slot and, for callers whose own array is pageable, a pinned staging buffer per slot.
struct ChunkPipe {
    static constexpr int kLanes = 5;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_h2d[2] = {}, ev_comp[2] = {}, ev_d2h[2] = {};
    struct Lane { void *h[2] = {}, *d[2] = {}; size_t cap = 0; } lane[kLanes];
    unsigned seq = 0;               // chunks enqueued so far: chunk i of a call takes slot (seq + i) & 1, so consecutive one-chunk calls alternate slots
    // device slots always; the pinned staging halves only when asked for (`host`), and nothing at all for a lane of zero bytes (an absent output)
    int grow(int k, size_t need, bool host) {
        Lane &l = lane[k];
        if (need <= l.cap && (!host || l.h[0] || !need)) return 0;
        const size_t want = need > l.cap ? need : l.cap;
        for (int i = 0; i < 2; ++i) {
            if (need > l.cap) {
                if (l.h[i]) PB_HIP(hipHostFree(l.h[i]));
                if (l.d[i]) PB_HIP(hipFree(l.d[i]));
                l.h[i] = l.d[i] = nullptr;
                PB_HIP(hipMalloc(&l.d[i], want));
            }
            if (host && !l.h[i]) PB_HIP(hipHostMalloc(&l.h[i], want, hipHostMallocDefault));
        }
        l.cap = want;
        return 0;
    }
    int ensure_streams() {
        if (s_in) return 0;
        PB_HIP(hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
        PB_HIP(hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            PB_HIP(hipEventCreateWithFlags(&ev_h2d[i], hipEventDisableTiming));
            PB_HIP(hipEventCreateWithFlags(&ev_comp[i], hipEventDisableTiming));
            PB_HIP(hipEventCreateWithFlags(&ev_d2h[i], hipEventDisableTiming));
        }
        return 0;
    }
    void release() {
        if (s_in) { hipStreamSynchronize(s_in); hipStreamSynchronize(s_out); }
        for (Lane &l : lane)
            for (int i = 0; i < 2; ++i) {
                if (l.h[i]) hipHostFree(l.h[i]);
                if (l.d[i]) hipFree(l.d[i]);
            }
        for (int i = 0; i < 2; ++i) {
            if (ev_h2d[i]) hipEventDestroy(ev_h2d[i]);
            if (ev_comp[i]) hipEventDestroy(ev_comp[i]);
            if (ev_d2h[i]) hipEventDestroy(ev_d2h[i]);
        }
        if (s_in) { hipStreamDestroy(s_in); hipStreamDestroy(s_out); }
    }
};

// pb_mask_infer_batch: the engine walks the batch in chunks of max_batch frames itself and takes whole-batch device pointers, so the pipeline is
// whole-batch device buffers + one event per chunk: every chunk's H2D is enqueued up front on s_in, chunk i's kernels wait for event i, and its id
// images leave on s_out as soon as its last launch is enqueued (MaskEngine::chunk_begin / chunk_end).  Buffers and streams stay on the ctx.
struct MaskPipe {
    hipStream_t s_in = nullptr, s_out = nullptr;
    void *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
    size_t cap_d = 0, cap_hi = 0, cap_ho = 0;
    std::vector<hipEvent_t> ev_in, ev_done;
    // bytes: the batch as RGB (d_in, d_out); in_bytes / out_bytes: the batch as the caller hands it over (h_in) / takes it back (h_out) - planar
    // YUV frames may be larger than RGB
    int ensure(size_t bytes, size_t in_bytes, size_t out_bytes, bool host_in, bool host_out, int chunks) {
        if (!s_in) {
            PB_HIP(hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
            PB_HIP(hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
        }
        if (bytes > cap_d) {
            if (d_in) PB_HIP(hipFree(d_in));
            if (d_out) PB_HIP(hipFree(d_out));
            d_in = d_out = nullptr; cap_d = 0;
            PB_HIP(hipMalloc(&d_in, bytes));
            PB_HIP(hipMalloc(&d_out, bytes));
            cap_d = bytes;
        }
        if (host_in && in_bytes > cap_hi) {
            if (h_in) PB_HIP(hipHostFree(h_in));
            h_in = nullptr; cap_hi = 0;
            PB_HIP(hipHostMalloc(&h_in, in_bytes, hipHostMallocDefault));
            cap_hi = in_bytes;
        }
        if (host_out && out_bytes > cap_ho) {
            if (h_out) PB_HIP(hipHostFree(h_out));
            h_out = nullptr; cap_ho = 0;
            PB_HIP(hipHostMalloc(&h_out, out_bytes, hipHostMallocDefault));
            cap_ho = out_bytes;
        }
        while ((int)ev_in.size() < chunks) {
            hipEvent_t a, b;
            PB_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
            PB_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
            ev_in.push_back(a); ev_done.push_back(b);
        }
        return 0;
    }
    void release() {
        if (s_in) { hipStreamSynchronize(s_in); hipStreamSynchronize(s_out); }
        if (d_in) hipFree(d_in);
        if (d_out) hipFree(d_out);
        if (h_in) hipHostFree(h_in);
        if (h_out) hipHostFree(h_out);
        for (auto e : ev_in) hipEventDestroy(e);
        for (auto e : ev_done) hipEventDestroy(e);
        if (s_in) { hipStreamDestroy(s_in); hipStreamDestroy(s_out); }
    }
};

struct pb_ctx {
    int device = 0;
    DepthEngine *depth = nullptr;
    FlowEngine *flow = nullptr;
    MaskEngine *mask = nullptr;
    EngineBase *band = nullptr;     // whichever of the three was created: what every band has (timer, debug, tiles, stats)
    hipStream_t stream = nullptr;   // == depth->stream when a band is loaded
    f16 *zero = nullptr;
    bool own_stream = false;
    int gemm_tile = TILE_AUTO, conv_tile = TILE_AUTO;
    int op_splitk = 0;              // pb_set_option("op_splitk", 1): pb_op_gemm / pb_op_conv2d lend launch_gemm a split-K workspace (gemm.h splitk; op-level tests)
    int host_chunk = 0;             // pb_set_option("host_chunk"): frames (depth) / frame pairs (flow) per chunk of the host-pointer pipelines, 0 = default
    int corr_layout = 1;            // pb_set_option("corr_layout"): flow_raft's volume layout (corr_layout.h) - the band's engine and pb_op_raft_lookup follow it
    ChunkPipe pipe;                 // depth / flow bands (a ctx has one band)
    MaskPipe mpipe;
    std::deque<hipEvent_t> pending;     // completion events of pb_*_submit_* calls not yet waited for (pb_wait pops the oldest)
    std::vector<void *> host_blocks;    // pb_host_alloc: page-locked blocks the ctx owns (the band loops' rings); pb_destroy frees what pb_host_free did not
    std::mutex host_mu;
    // pb_comm_init: RCCL communicator of the ranks (one process per GPU) for pb_gather_scalars
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    float *comm_buf = nullptr;
    size_t comm_cap = 0;
    // pb_depth_encode_still: its own stream and buffers, kept for the life of the ctx (the band calls it from its sink thread for
    // every --subpath frame while the main thread's batches run on `stream`; a hipMalloc / hipFree pair per frame synchronised the device)
    hipStream_t still_stream = nullptr;
    char *still_buf = nullptr;
    size_t still_cap = 0;
    std::mutex still_mu;
    // pb_set_option("frames_i420" / "rgb_out_i420"): the host-pointer and submit entry points of the bands take their frames / give their rgb_out as
    // I420.  The conversions run on the ctx stream between the copies and the band, through one RGB buffer per direction (yuv[0]: the frames the
    // band reads - for the mask band the I420 frames instead, its pipeline keeps whole-batch RGB buffers of its own; yuv[1]: what it encodes).
    // Work on one stream runs in order, so chunks and submissions share them; they grow only while the stream is idle.
    // pb_set_option("rgb_out_full"): the flow bands' rgb_out holds frames of the clip's size, resized (resize.hip) out of yuv[1] as well.
    // pb_set_frame_format: frames_i420 != 0 says the frames are planar YUV, frame_fmt which ("frames_i420" sets {420, 8, limited, BT.601}).
    // pb_set_out_format: the same for rgb_out - rgb_out_i420 != 0 says it is planar YUV, out_fmt which ("rgb_out_i420" sets {420, 8, limited,
    // BT.601}).  yuv[2]: the resized RGB frames of "rgb_out_full" on their way to a layout that has no fused resize kernel.
    int frames_i420 = 0, rgb_out_i420 = 0, rgb_out_full = 0;
    pb_yuv_fmt frame_fmt = {420, 8, 0, PB_YUV_BT601}, out_fmt = {420, 8, 0, PB_YUV_BT601};
    void *yuv[3] = {};
    size_t yuv_cap[3] = {};
    int yuv_grow(int k, size_t need) {
        if (need <= yuv_cap[k]) return 0;
        PB_HIP(hipStreamSynchronize(stream));
        if (yuv[k]) PB_HIP(hipFree(yuv[k]));
        yuv[k] = nullptr; yuv_cap[k] = 0;
        PB_HIP(hipMalloc(&yuv[k], need));
        yuv_cap[k] = need;
        return 0;
    }
    // pb_depth_point_cloud_dev: the per-frame min / max words of the un-flip, on the ctx stream (the host variant keeps its own in still_buf)
    unsigned *pcl_mm = nullptr;
    int pcl_mm_cap = 0;
    // pb_jpeg_encode / pb_jpeg_encode_dev: the encoder's workspace and the slots of its host pipeline, on the ctx stream
    JpegState jpeg;
};
