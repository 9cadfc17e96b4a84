/*
 * prisma_bands.h - C ABI of libprisma_bands.so (MI355X / gfx950 "bands" engine).
 *
 * The reference (patriciogonzalezvivo/prisma) has no native boundary: a band is a Python
 * script exposing init_model()/infer() and a per-frame loop.  This header is the boundary a
 * maintainer would bind from those scripts (ctypes stub: INTEGRATION.md).  Each entry point
 * cites the reference code it replaces; paths are relative to the reference checkout.
 *
 * Conventions
 *   - every function returns 0 on success or a negative pb_status; pb_last_error() holds the
 *     message of the last failure on the calling thread.
 *   - the caller owns every host buffer (pb_host_alloc blocks excepted: page-locked memory the ctx
 *     lends and frees); the library owns device memory, streams and events
 *     inside pb_ctx.  One pb_ctx per GPU per process; a ctx is not re-entrant.
 *   - no CPU fallback: without a usable HIP device pb_create fails (PB_ERR_DEVICE).
 */
#ifndef PRISMA_BANDS_H
#define PRISMA_BANDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pb_ctx pb_ctx;

typedef enum {
    PB_OK = 0,
    PB_ERR_ARG = -1,      /* bad argument / shape / missing weight            */
    PB_ERR_DEVICE = -2,   /* no HIP device, HIP call failed                   */
    PB_ERR_MEMORY = -3,   /* device or host allocation failed                 */
    PB_ERR_STATE = -4     /* call sequence error (e.g. wrong band for ctx)    */
} pb_status;

typedef enum { PB_F32 = 0, PB_F16 = 1, PB_U8 = 2, PB_I32 = 3 } pb_dtype;

/* One named weight tensor, reference state_dict naming
 * (Depth-Anything: `pretrained.*`, `depth_head.*` - bands/d_anything/dpt.py:139-166;
 *  RAFT: `fnet.*`, `cnet.*`, `update_block.*` - bands/raft/raft.py:24-58, without the
 *  `module.` prefix that bands/flow_raft.py:42-44 strips).  data is host memory, float32,
 *  C-contiguous; it is consumed (packed + uploaded) during pb_create and not referenced after. */
typedef struct {
    const char *name;
    int32_t dtype;        /* pb_dtype, PB_F32 only today */
    int32_t ndim;
    int64_t shape[6];
    const void *data;
} pb_tensor;

/* Depth-Anything geometry (bands/depth_anything.py:257-264 `--encoder`; the HF config that
 * DepthAnything.from_pretrained reads: encoder / features / out_channels). */
typedef struct {
    int32_t embed_dim;        /* 384 / 768 / 1024                       */
    int32_t depth;            /* 12 / 12 / 24 transformer blocks        */
    int32_t heads;            /* 6 / 12 / 16 (head_dim is always 64)    */
    int32_t features;         /* DPT head width 64 / 128 / 256          */
    int32_t out_channels[4];  /* DPT reassemble widths                  */
    int32_t pos_grid;         /* 37 (pos_embed rows = 1 + 37*37)        */
    int32_t max_batch;        /* frames per launch the arena is sized for (>= 1) */
    int32_t metric;           /* 1: ZoeDepth metric head on top (`--metric indoor|outdoor`, ViT-L only): weights also
                               * carry conv2.*, seed_bin_regressor.*, seed_projector.*, projectors.*, attractors.*,
                               * conditional_log_binomial.mlp.* (ZoeDepth state dict, `core.core.` prefix stripped);
                               * the network input is 392 x 518, depth_out is metric depth, use flip = 0 */
    int32_t precision;        /* pb_precision: 0 = one fp16 MFMA pass per GEMM, 1 = split-fp16 (see pb_precision)        */
} pb_depth_cfg;

/* Arithmetic of the GEMMs / convolutions (everything else - LayerNorm, softmax, residual streams, GRU state, norms'
 * statistics - is fp32 in both modes).
 *   PB_PREC_F16   : operands rounded to fp16 once, fp32 accumulation.  Against the fp32 reference: relative L2 < 1e-3,
 *                   max-norm error up to 1.6e-3 of the output range on the 24-block ViT-L.
 *   PB_PREC_SPLIT : the operands the error budget is dominated by are kept as hi + lo fp16 pairs and the products
 *                   a_hi w_hi + a_lo w_hi + a_hi w_lo accumulate in the same fp32 MFMA accumulators (2-3 passes over K):
 *                   max-norm and L2 error < 1e-3 on every reference vector - the mode the parity tests assert 1e-3 in. */
typedef enum { PB_PREC_F16 = 0, PB_PREC_SPLIT = 1 } pb_precision;

/* flow_raft options (cfg of pb_create; NULL = all zero). */
typedef struct {
    int32_t precision;        /* pb_precision */
} pb_flow_cfg;

/* SOLOv2 geometry and test_cfg for band = "mask_mmdet" (the values live in the mmdet config the reference downloads,
 * models/solov2_r101_fpn_3x_coco.py -> _base_ solov2_r50_fpn_1x_coco.py; bands/mask_mmdet.py:26-27). */
typedef struct {
    int32_t blocks[4];           /* ResNet bottleneck counts: 3,4,23,3 (R-101) / 3,4,6,3 (R-50)                 */
    int32_t scale_long;          /* test pipeline img_scale = (1333, 800), keep_ratio                            */
    int32_t scale_short;
    int32_t num_classes;         /* 80                                                                            */
    int32_t feat_channels;       /* 512: kernel / class branch width                                              */
    int32_t stacked_convs;       /* 4                                                                             */
    int32_t num_grids[5];        /* 40, 36, 24, 16, 12                                                            */
    int32_t strides[5];          /* 8, 8, 16, 32, 32 (area filter: mask area > stride)                            */
    int32_t mask_feat_channels;  /* 128                                                                           */
    int32_t mask_out_channels;   /* 256 (= dynamic kernel length)                                                 */
    int32_t nms_pre;             /* 500                                                                           */
    int32_t max_per_img;         /* 100                                                                           */
    float score_thr;             /* 0.1                                                                           */
    float mask_thr;              /* 0.5                                                                           */
    float filter_thr;            /* 0.05                                                                          */
    float sigma;                 /* 2.0 (gaussian Matrix NMS)                                                     */
    int32_t max_batch;           /* frames per backbone launch the arena is sized for (>= 1)                      */
    int32_t precision;           /* pb_precision                                                                  */
} pb_mask_cfg;

const char *pb_last_error(void);
int pb_version(void);
/* ABI guard: bumped whenever a public struct's layout or an entry point's signature changes.  A binding compares
 * pb_abi_version() with the PB_ABI_VERSION it was written against and pb_struct_size(which) with its own sizeof before the first
 * call (prisma_amd/_lib.py load(); integration/depth_anything_stub.py) - a stale binding fails at load, not by reading shifted
 * fields.  which: 0 pb_tensor, 1 pb_depth_cfg, 2 pb_flow_cfg, 3 pb_mask_cfg, 4 pb_kernel_stat, 5 pb_comm_id, 6 pb_yuv_fmt, 7 pb_jpeg_cfg;
 * -1 for others. */
#define PB_ABI_VERSION 3
int pb_abi_version(void);
int pb_struct_size(int which);
/* Number of visible HIP devices (0 on a CPU-only box; never fails). */
int pb_device_count(void);

/* init_model(): bands/depth_anything.py:48-76 (+ bands/d_anything/dpt.py:139-171).
 * band = "depth_anything" | "flow_raft" | "flow_gmflow" | "mask_mmdet" (the sections below).  Packs weights to fp16 MFMA layouts
 * and uploads them. */
int pb_create(pb_ctx **out, int device_id, const char *band, const pb_tensor *weights,
              int n_weights, const void *cfg, size_t cfg_bytes);
void pb_destroy(pb_ctx *ctx);

/* infer() + the per-frame post-process of process_video():
 * bands/depth_anything.py:100-143 and :215-221 (min/max, normalise, flip, heat_to_rgb).
 *   frames   : n x H x W x 3 uint8 RGB (decoder layout)            [host]
 *   depth_out: n x H x W float32 relative depth, or NULL           [host]
 *   rgb_out  : n x H x W x 3 uint8 heat-encoded frame, or NULL     [host]
 *   min_out / max_out: n floats each, or NULL                      [host]
 *   flip     : 1 for the relative model (bands/depth_anything.py:188) */
int pb_depth_infer_batch(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W,
                         float *depth_out, uint8_t *rgb_out, float *min_out, float *max_out, int flip);

/* Same contract with every pointer in device memory of ctx's GPU (frames already resident
 * in HBM; used by bench.py and by pipelines that decode on the GPU).  Asynchronous on the
 * ctx stream; pb_sync() waits for it. */
int pb_depth_infer_batch_dev(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W,
                             float *depth_out, uint8_t *rgb_out, float *min_out, float *max_out, int flip);
int pb_sync(pb_ctx *ctx);
/* Asynchronous host-pointer calls (round 6).  pb_depth_submit_batch / pb_flow_submit_sequence take the arguments of pb_depth_infer_batch /
 * pb_flow_infer_sequence, enqueue the whole three-stage pipeline (H2D, band, D2H of every chunk) and return; pb_wait(ctx) blocks until the
 * OLDEST submission of the ctx not yet waited for has its results in host memory (PB_ERR_STATE when none is outstanding).  Every buffer
 * handed to a submit - frames and each non-NULL output, the per-frame scalars included - must be page-locked host memory and stay valid and
 * untouched until the matching pb_wait returns.  Two submissions of one ctx may be in flight: the second one's uploads run under the first
 * one's kernels, the first one's downloads under the second one's, so a caller that streams clips (bands/depth_anything.py:203-225,
 * bands/flow_raft.py:98-113: the reference's frame loops) hides every copy.  Results are those of the blocking calls, bit for bit. */
int pb_depth_submit_batch(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W,
                          float *depth_out, uint8_t *rgb_out, float *min_out, float *max_out, int flip);
int pb_flow_submit_sequence(pb_ctx *ctx, const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward,
                            float *flow_out, uint8_t *rgb_out, float *maxdisp_out);
int pb_wait(pb_ctx *ctx);
/* pb_flow_submit_sequence_masks: the asynchronous form of pb_flow_infer_sequence_masks (below) - its arguments and argument checks, the
 * rules of the two submit calls above (mask_out page-locked like every other buffer), on flow_raft and flow_gmflow contexts alike.
 * There is no submit form of pb_mask_infer_batch, on purpose: the SOLOv2 engine synchronises with the host many times per call (its
 * candidate counts depend on the data), so an "asynchronous" call would block its caller anyway; the blocking call already pipelines its
 * own chunks and already addresses page-locked caller arrays directly.  The mask band's loop therefore uses page-locked rings with the
 * blocking call (bands/common/loop.py). */
int pb_flow_submit_sequence_masks(pb_ctx *ctx, const uint8_t *frames, int F, int H, int W, float scale, int iters,
                                  float alpha1, float alpha2, float *flow_out, uint8_t *rgb_out, float *maxdisp_out,
                                  uint8_t *mask_out);
/* Page-locked host memory owned by the ctx, for callers that stream (the band loops' input and output rings: a Python host gets
 * what torch's pin_memory would give it without importing torch).  pb_host_alloc: *ptr = a block of `bytes` bytes every submit call
 * accepts and every blocking host-pointer call addresses without staging (PB_ERR_MEMORY when the allocation fails).  pb_host_free: the
 * caller has waited for every submission that reads or writes the block; a pointer this ctx does not own is PB_ERR_ARG and nothing is
 * freed.  pb_destroy waits for the outstanding submissions and then frees the blocks that are left: they die with the ctx. */
int pb_host_alloc(pb_ctx *ctx, void **ptr, size_t bytes);
int pb_host_free(pb_ctx *ctx, void *ptr);
/* Several bands at once: contexts share nothing, every *_dev entry point returns after the enqueue, so a caller enqueues on two or three
 * contexts and then pb_sync()s each (prisma_amd.engine.run_concurrently; replaces the reference's strictly sequential band order,
 * process.py:205-290, where the bands of one video are independent).  Results are those of running the bands one after the other. */

/* Multi-GPU: one process and one pb_ctx per GPU; frames shard by rank and never cross GPUs.  The only
 * exchange is the all-gather of the per-frame scalars the CSV files need in frame order - depth (min, max), flow max
 * displacement: 4-12 bytes per frame - over RCCL (xGMI inside a node).  Rank 0 calls pb_comm_unique_id and hands the 128
 * bytes to the other ranks by any host channel (a file, torch.distributed's store); every rank then calls pb_comm_init on
 * its ctx (collective), and pb_gather_scalars (collective): `local` n_local floats of this rank -> `global`
 * [world x n_local] on every rank, rank-major.  Ranks with fewer frames pad to a common n_local.  Replaces the implicit
 * single-process ordering of bands/depth_anything.py:215-238 and bands/flow_raft.py:138-141. */
typedef struct { char internal[128]; } pb_comm_id;       /* = ncclUniqueId */
int pb_comm_unique_id(pb_comm_id *id_out);
int pb_comm_init(pb_ctx *ctx, const pb_comm_id *id, int rank, int world);
int pb_gather_scalars(pb_ctx *ctx, const float *local, int n_local, float *global);

/* Still-image / `--subpath` post-process: write_depth(heatmap=True, encode_range) of bands/common/io.py:138-172 as called from
 * bands/depth_anything.py:176-180,221-225, with encode.py:73-95 (float_to_edge, saturation) and :141-146 (float_to_rgb) -
 * normalise by the map's own min / max, flip, heat ramp, Sobel-edge magnitude of the 8-bit map in the saturation, min / max packed
 * as 24-bit fixed point of [0, 1000] into pixels (0, 0) and (0, 1), uint8 truncation.  Bytes equal the reference's
 * (tests/golden/write_depth.npz; cv2.Sobel's ksize-1 taps restated).  Works on any ctx.
 *   depth   : H x W float32 [host]        rgb_out : H x W x 3 uint8 RGB (what the PNG holds) [host]
 *   min_out / max_out: the map's min / max, or NULL */
int pb_depth_encode_still(pb_ctx *ctx, const float *depth, int H, int W, int flip, int encode_range, uint8_t *rgb_out,
                          float *min_out, float *max_out);

/* Still-image `--ply` post-process: write_pcl of bands/common/io.py:201-211 as called from bands/depth_anything.py:170-171, with
 * create_point_cloud / save_point_cloud of bands/common/geom.py:5-47 - with `flip` the relative model's range is turned over in float32
 * (d = mn + (1 - (d - mn) / (mx - mn)) * (mx - mn) by the frame's own min / max, every operation separately rounded), then
 * cv2.medianBlur(d, 5), x = (col - u0) / fx, y = (row - v0) / fy, vertex = (m x, m (-y), m (-1)) and the source pixel's colour, one packed
 * 15-byte record <f4 x, f4 y, f4 z, u1 red, u1 green, u1 blue (little endian) per pixel in row-major order: the body of the binary PLY
 * the reference writes through plyfile.  cv2 and plyfile are absent where this library is built and tested, so medianBlur (the exact
 * median of the 5 x 5 window, border replicated, also on maps smaller than 5) and the record layout are pinned by restatement
 * (tests/pcl_ref.py), not against the real packages.  Contract: finite depth; NaN and -0.0 in the map are outside it.  A constant map
 * with `flip` gives NaN vertices, as in the reference.  Works on any ctx.
 *   depth : n x H x W float32     rgb : n x H x W x 3 uint8     vertices_out : n x H x W x 15 bytes (no alignment needed)
 * pb_depth_point_cloud: host pointers, blocking (its own stream and buffers, shared with pb_depth_encode_still: callable from another
 * thread while the ctx stream works).  pb_depth_point_cloud_dev: device pointers, asynchronous on the ctx stream; pb_sync() waits. */
int pb_depth_point_cloud(pb_ctx *ctx, const float *depth, const uint8_t *rgb, int n, int H, int W, int flip,
                         float u0, float v0, float fx, float fy, uint8_t *vertices_out);
int pb_depth_point_cloud_dev(pb_ctx *ctx, const float *depth, const uint8_t *rgb, int n, int H, int W, int flip,
                             float u0, float v0, float fx, float fy, uint8_t *vertices_out);

/* rgba band, side-by-side RGB-D captures (`--rgbd left|right|top|bottom`, Record3D): split() of bands/rgba.py:24-75.
 * pb_rgbd_boxes (no GPU needed): the two halves of an H x W frame as half-open boxes {y0, y1, x0, x1}.  `side` is where the DEPTH is:
 * 0 left, 1 right, 2 top, 3 bottom.  The reference slices with int() of width / 2 and height / 2 (rgba.py:29-40, 58-59), so with
 * k = W / 2 (integer division) left gives depth columns [0, k) and rgb [k, W), right rgb [0, k) and depth [k, W); top and bottom the same
 * on rows with H / 2: of an odd size the half that starts at the middle is one wider.  PB_ERR_ARG when a half is empty (W < 2 for left /
 * right, H < 2 for top / bottom) or `side` is unknown.  The colour half is a crop without arithmetic and stays with the caller.
 * pb_rgbd_depth: `--encoding_depth hue` of the depth half (rgba.py:61-63 with rgb_to_hsv / heat_to_rgb / hue_to_rgb of
 * bands/common/encode.py:13-58): d = clip(hue / 360, 0, 1) of every pixel, then heat_to_rgb(d) * 255 truncated to uint8 - float64 with
 * numpy's operation order, every operation separately rounded; the bytes equal the reference's on all 2^24 colours
 * (tests/golden/rgbd_hue.npz).  With `--encoding_depth none` the half is a crop too and needs no call.
 *   frames    : n x H x W x 3 uint8, the whole side-by-side frames
 *   depth_out : n x Hd x Wd x 3 uint8, the heat-encoded half (Hd x Wd = pb_rgbd_boxes' depth box), or NULL
 *   heat_out  : n x Hd x Wd float32, d itself rounded to float32 - what a viewer recovers from the video as min + heat (max - min),
 *               without the 8-bit round trip - or NULL (not both)
 * pb_rgbd_depth: host pointers, blocking, in chunks of "host_chunk" frames (pb_set_option; default 8) whose copies overlap the kernel;
 * page-locked caller arrays are addressed directly.  pb_rgbd_depth_dev: device pointers, asynchronous on the ctx stream; pb_sync() waits.
 * Works on any ctx: the rgba band has no model. */
int pb_rgbd_boxes(int H, int W, int side, int rgb_box[4], int depth_box[4]);
int pb_rgbd_depth(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W, int side, uint8_t *depth_out, float *heat_out);
int pb_rgbd_depth_dev(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W, int side, uint8_t *depth_out, float *heat_out);

/* I420 frames (YUV4MPEG2 `.y4m` clips; what decoders produce and encoders consume): 8 bit, 4:2:0, BT.601 limited range.  A frame is H W bytes
 * of Y, then ceil(H / 2) ceil(W / 2) bytes of Cb, then as many of Cr - pb_i420_bytes(H, W) in all, 1.5 per pixel where RGB takes 3; frames are
 * packed.  The arithmetic is the published 8-bit integer form, exact, `>>` an arithmetic shift, clip8 a clamp to 0 .. 255:
 *   RGB -> I420   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 per pixel; per 2 x 2 block, of R, G, B = (sum of the block's 4 samples + 2) >> 2 with
 *                 pixel indices clamped to the frame: Cb = ((-38 R - 74 G + 112 B + 128) >> 8) + 128, Cr = ((112 R - 94 G - 18 B + 128) >> 8) + 128
 *   I420 -> RGB   C = Y - 16, D = Cb - 128, E = Cr - 128 with the chroma sample plane[y >> 1][x >> 1]: R = clip8((298 C + 409 E + 128) >> 8),
 *                 G = clip8((298 C - 100 D - 208 E + 128) >> 8), B = clip8((298 C + 516 D + 128) >> 8)
 * It is not swscale's fixed-point code: against ffmpeg the bytes agree to an LSB or two (PARITY UNPINNED); tests/yuv_ref.py pins them by
 * restatement, on all 2^24 inputs of either direction.
 * pb_i420_to_rgb / pb_rgb_to_i420: host pointers, blocking, in chunks of "host_chunk" frames (default 8) whose copies overlap the kernel;
 * page-locked caller arrays are addressed directly.  The *_dev forms: device pointers, asynchronous on the ctx stream; pb_sync() waits.  No
 * alignment is needed (with W % 16 == 0 and 16-byte aligned device pointers the kernels move 16 bytes per access).  Work on any ctx.
 *   yuv : n x pb_i420_bytes(H, W) bytes      rgb : n x H x W x 3 uint8
 * Inside the bands: pb_set_option(ctx, "frames_i420", 1) makes the host-pointer and submit entry points of the ctx - pb_depth_infer_batch,
 * pb_depth_submit_batch, pb_flow_infer_sequence(_masks), pb_flow_submit_sequence(_masks), pb_mask_infer_batch - take `frames` as n (F) x
 * pb_i420_bytes(H, W) bytes; pb_set_option(ctx, "rgb_out_i420", 1) makes their rgb_out (the mask band's mask_out: its id image counts as one) hold
 * I420 frames of the output size - pb_i420_bytes(H, W) per frame for depth and mask, pb_i420_bytes(sh, sw) per pair and direction for flow.  The
 * I420 chunk crosses PCIe, the conversion runs on the ctx stream next to the band's kernels.  Every other output is untouched, and the *_dev band
 * entry points keep RGB (their callers hold device memory and can call the *_dev conversions themselves).  Both options are 0 by default and can
 * be set only while no submission is outstanding. */
int64_t pb_i420_bytes(int H, int W);
int pb_i420_to_rgb(pb_ctx *ctx, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out);
int pb_i420_to_rgb_dev(pb_ctx *ctx, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out);
int pb_rgb_to_i420(pb_ctx *ctx, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out);
int pb_rgb_to_i420_dev(pb_ctx *ctx, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out);

/* Every planar layout a `.y4m` clip can have, to RGB (the way in; pb_rgb_to_yuv below is the way out; chroma
 * siting is not acted on; the matrix is the caller's to name - it is not guessed from the frame size).  One rule, exact integers:
 *   chroma      400 (mono: no chroma planes), 420, 422 or 444;  (sx, sy) = (1, 1) for 420, (1, 0) for 422, (0, 0) for 444
 *   depth d     8 .. 16: one byte per sample at d = 8, else a 16-bit little-endian word, read whole and not masked
 *   full_range  0: limited (yoff = 16 << (d - 8)), 1: full (yoff = 0);  coff = half = 1 << (d - 1)
 *   matrix      PB_YUV_BT601: Kr = 299 / 1000, Kb = 114 / 1000;  PB_YUV_BT709: Kr = 2126 / 10000, Kb = 722 / 10000;  Kg = 1 - Kr - Kb
 * A frame is H x W samples of Y, then ceil(H / 2^sy) x ceil(W / 2^sx) of Cb, then as many of Cr; frames are packed.  Per pixel (x, y), with the
 * chroma samples plane[y >> sy][x >> sx] (nearest) and D = E = 0 for 400:
 *   C = Y - yoff, D = Cb - coff, E = Cr - coff
 *   R = clip8((cy C + crv E + half) >> d)     G = clip8((cy C - cgu D - cgv E + half) >> d)     B = clip8((cy C + cbu D + half) >> d)
 * `>>` an arithmetic shift on int32 (every intermediate is inside int32; below 2^27 for samples within d bits), clip8 a clamp to 0 .. 255.  The coefficients are exact rationals rounded
 * half up, rhu(p / q) = floor((2 p + q) / (2 q)), no floating point anywhere:
 *   limited: sy = 255 / (219 2^(d - 8)), sc = 255 / (224 2^(d - 8));   full: sy = sc = 255 / (2^d - 1)
 *   cy = rhu(2^d sy)   crv = rhu(2^d sc 2 (1 - Kr))   cgu = rhu(2^d sc 2 Kb (1 - Kb) / Kg)   cgv = rhu(2^d sc 2 Kr (1 - Kr) / Kg)   cbu = rhu(2^d sc 2 (1 - Kb))
 * - (298, 409, 100, 208, 516) for BT.601 limited at every d, so {420, 8, 0, PB_YUV_BT601} is pb_i420_to_rgb byte for byte (and runs its kernel);
 * (298, 459, 55, 136, 541) for BT.709 limited.  For samples within d bits the result is within 1.5 of the real-valued conversion: 0.5 for the final floor, and
 * 0.5 (|C| + |D| + |E|) / 2^d <= 1 for the rounding of the coefficients.
 * pb_yuv_bytes: bytes of one frame, 0 for a format outside the above or a size that is not positive; pb_yuv_coeffs: out = cy, crv, cgu, cgv, cbu,
 * yoff, coff.  Neither needs a GPU.  pb_yuv_to_rgb: host pointers, blocking, in chunks of "host_chunk" frames (default 8) as pb_i420_to_rgb;
 * pb_yuv_to_rgb_dev: device pointers, asynchronous on the ctx stream, pb_sync() waits.  No alignment is needed (with W % 16 == 0 and 16-byte
 * aligned device pointers a lane moves 16 bytes per access).  Work on any ctx.
 *   yuv : n x pb_yuv_bytes(fmt, H, W) bytes      rgb : n x H x W x 3 uint8
 * Inside the bands: pb_set_frame_format(ctx, fmt) makes the host-pointer and submit entry points of the ctx (those "frames_i420" names above) take
 * `frames` as n (F) x pb_yuv_bytes(fmt, H, W) bytes, converted on the ctx stream into the RGB buffer the band reads; page-locked caller buffers
 * stay directly addressed.  fmt = NULL: RGB again.  pb_set_option(ctx, "frames_i420", 1) is pb_set_frame_format with {420, 8, 0, PB_YUV_BT601},
 * 0 is NULL.  Refused while a submission is outstanding, and for a format outside the above - the ctx is then left as it was.  The *_dev band
 * entry points keep RGB. */
enum { PB_YUV_BT601 = 0, PB_YUV_BT709 = 1 };
typedef struct {
    int32_t chroma;           /* 400 / 420 / 422 / 444 */
    int32_t depth;            /* 8 .. 16 bits per sample */
    int32_t full_range;       /* 0 limited, 1 full */
    int32_t matrix;           /* PB_YUV_BT601 / PB_YUV_BT709 */
} pb_yuv_fmt;
int64_t pb_yuv_bytes(const pb_yuv_fmt *fmt, int H, int W);
int pb_yuv_coeffs(const pb_yuv_fmt *fmt, int32_t out[7]);
int pb_yuv_to_rgb(pb_ctx *ctx, const pb_yuv_fmt *fmt, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out);
int pb_yuv_to_rgb_dev(pb_ctx *ctx, const pb_yuv_fmt *fmt, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb_out);
int pb_set_frame_format(pb_ctx *ctx, const pb_yuv_fmt *fmt);

/* RGB to every one of those layouts, the way out: what a written `.y4m` holds.  A format is the pb_yuv_fmt above; plane order, plane sizes, sample
 * size (one byte at d = 8, else a 16-bit little-endian word), yoff and coff are those of the read direction.  One rule, exact integers, one table:
 *   limited: ys = 219 2^(d - 8) / 255, cs = 224 2^(d - 8) / 255;   full: ys = cs = (2^d - 1) / 255;   F = 24 - d fractional bits
 *   - the one exception: {d = 8, limited, BT.601} takes F = 8
 *   yr = rhu(2^F ys Kr)     yb = rhu(2^F ys Kb)     yg = rhu(2^F ys) - yr - yb
 *   h  = rhu(2^F cs / 2)    ur = rhu(2^F cs Kr / (2 (1 - Kb)))    ug = h - ur    vb = rhu(2^F cs Kb / (2 (1 - Kr)))    vg = h - vb
 *   Y  = clamp((( yr R + yg G + yb B + 2^(F - 1)) >> F) + yoff)      per pixel
 *   Cb = clamp(((-ur R - ug G + h  B + 2^(F - 1)) >> F) + coff)      per chroma sample
 *   Cr = clamp((( h  R - vg G - vb B + 2^(F - 1)) >> F) + coff)
 * rhu, Kr, Kb as above, `>>` an arithmetic shift on int32 (|coefficient| <= 2^24 / 255, so every intermediate is inside int32), clamp to
 * 0 .. 2^d - 1.  The R, G, B of a chroma sample are the rounded mean of the pixels it covers, indices clamped to the frame: (sum of 4 + 2) >> 2
 * for 420 (as pb_rgb_to_i420), (sum of 2 + 1) >> 1 for 422, the pixel itself for 444; 400 writes Y only.  The G coefficients are remainders, so a
 * grey pixel gives Cb = Cr = coff exactly and white gives the top code.  With F = 8 the construction yields the published integers 66, 129, 25 /
 * 38, 74, 112 / 112, 94, 18 of pb_rgb_to_i420 - which is why the exception is an F and not a second table: {420, 8, 0, PB_YUV_BT601} is
 * pb_rgb_to_i420 byte for byte (and runs its kernel), and the other 8-bit limited BT.601 layouts share its luma.
 * Outside the exception the result is within 0.5 + 510 / 2^F codes of the real-valued conversion of the same (block-mean) R, G, B: 0.5 for the
 * final floor, and coefficient rounding of at most 0.5, 1 and 0.5 per unit on inputs up to 255 - under 0.51 codes at d = 8, under 2.5 codes of
 * 65536 at d = 16.  Read back by the rule above (pb_yuv_to_rgb, same format): 444 at d = 12, 14, 16 returns every one of the 2^24 colours
 * exactly, in both ranges and matrices; at d = 10 up to 2.2 % of them are off by 1, at d = 8 75 - 84 % by up to 2; a grey value through
 * {400, 8, full} comes back exactly.
 * pb_yuv_fwd_coeffs: out = yr, yg, yb, ur, ug, h, vg, vb, F, yoff, coff, 2^d - 1; needs no GPU.  pb_rgb_to_yuv: host pointers, blocking, in
 * chunks of "host_chunk" frames (default 8) as pb_rgb_to_i420, page-locked arrays addressed directly; pb_rgb_to_yuv_dev: device pointers,
 * asynchronous on the ctx stream, pb_sync() waits.  No alignment is needed (with W % 16 == 0 and 16-byte aligned device pointers a lane moves 16
 * bytes per access).  Work on any ctx; a format outside the table or a size that is not positive is refused before any launch.
 *   rgb : n x H x W x 3 uint8      yuv : n x pb_yuv_bytes(fmt, H, W) bytes
 * Inside the bands: pb_set_out_format(ctx, fmt) makes the rgb_out of the host-pointer and submit entry points of the ctx (the mask band's
 * mask_out) hold pb_yuv_bytes(fmt, h, w) bytes per frame in that layout, converted on the ctx stream out of the RGB buffer the band encodes into.
 * fmt = NULL: RGB again.  pb_set_option(ctx, "rgb_out_i420", 1) is pb_set_out_format with {420, 8, 0, PB_YUV_BT601}, 0 is NULL.  With
 * "rgb_out_full" (below) that format keeps the fused resize kernels; any other resizes to RGB into ctx scratch and then converts - two launches,
 * the bytes of pb_rgb_to_yuv of pb_rgb_resize.  Refused while a submission is outstanding (PB_ERR_STATE), and for a format outside the table
 * (PB_ERR_ARG) - the ctx is then left as it was.  The *_dev band entry points keep RGB. */
int pb_yuv_fwd_coeffs(const pb_yuv_fmt *fmt, int32_t out[12]);
int pb_rgb_to_yuv(pb_ctx *ctx, const pb_yuv_fmt *fmt, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out);
int pb_rgb_to_yuv_dev(pb_ctx *ctx, const pb_yuv_fmt *fmt, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv_out);
int pb_set_out_format(pb_ctx *ctx, const pb_yuv_fmt *fmt);

/* Baseline JPEG frames - a Motion JPEG video is their concatenation (`.mjpeg`) or an AVI of them.  One rule, exact integers; tests/jpeg_ref.py
 * restates it and the kernels (jpeg.hip) give its bytes.
 *   input     a frame's planes as pb_rgb_to_yuv of {chroma, 8, full_range = 1, PB_YUV_BT601} lays them out - JFIF's colour space; chroma 444, 420 or
 *             400 (one component)
 *   padding   every plane to whole MCUs (8 x 8 samples; at 420 16 x 16 of Y, 8 x 8 of Cb and Cr) by repeating its last column and row; s = sample - 128
 *   DCT       F[v][u] = sum_y sum_x C[v][y] C[u][x] s[y][x],  C[u][x] = round(2^13 c(u) / 2 cos((2x + 1) u pi / 16)),  c(0) = 1 / sqrt 2, c(u) = 1
 *             (C[0][x] = 2896; the others +- 4017 3784 3406 2896 2276 1567 799); nothing is rounded between the passes, |F| < 2^37
 *   quantise  sign(F) ((|F| + D / 2) div D),  D = 2^26 Q: round half away from zero in one integer division
 *   tables    Q = clamp((base s + 50) div 100, 1, 255) with base ITU-T T.81 Annex K.1 (Y) / K.2 (Cb, Cr) and s = 5000 div quality below 50, else
 *             200 - 2 quality (the IJG scaling, quality 1 .. 100); Huffman tables Annex K.3 - K.6
 *   coding    zigzag, then T.81 F.1.2: the DC difference to the previous block of the component inside the restart interval (0 at its start),
 *             AC as (run, size) with ZRL and EOB; the blocks of an MCU in the order Y00 Y01 Y10 Y11 Cb Cr at 420
 *   stream    SOI, APP0 (JFIF 1.01, density 1 : 1), one DQT per table, SOF0 (8 bit; components 1 2 3; sampling 1x1, or 2x2 1x1 1x1), one DHT per table
 *             (DC, AC of table 0, then of table 1; 400 has table 0 only), DRI = the MCUs of one MCU row, SOS, the intervals with RST(m mod 8) after
 *             interval m except the last, each padded to a whole byte with 1-bits and a 0x00 after every 0xFF byte, EOI.  Every frame is a complete
 *             .jpg; a restart interval per MCU row is what makes the rows independent.
 * pb_jpeg_bound: the worst-case bytes of one frame - the header, every block at 20 + 63 x 26 bits (208 bytes), every byte stuffed, the markers;
 * 0 for a cfg outside the table or a side outside 1 .. 65535.  Needs no GPU.  Real frames are a small fraction of it: a caller may pass less and
 * grow on overflow.
 * pb_jpeg_encode: host pointers, blocking, in chunks of "host_chunk" frames (default 8) whose copies overlap the kernels; page-locked arrays are
 * addressed directly, and only the bytes produced are copied back.  planes: n x pb_yuv_bytes({chroma, 8, 1, BT601}, H, W) bytes; out: capacity
 * bytes, the frames back to back; offsets: n + 1 values, frame i is out[offsets[i] .. offsets[i + 1]).
 * Overflow: offsets[] always holds the positions the frames need, so offsets[n] is the capacity that would do; a frame is written whole if its end
 * lies within capacity and not at all otherwise (nothing past out[capacity - 1] is touched); the call then returns PB_ERR_MEMORY.
 * pb_jpeg_encode_dev: device pointers (offsets too), asynchronous on the ctx stream, pb_sync() waits; the same rule, the caller compares
 * offsets[n] with capacity.  No alignment is needed (with plane rows that are multiples of 16 bytes and a 16-byte aligned `planes` a lane loads 16
 * bytes per access).  Work on any ctx; a cfg outside the table or a side outside 1 .. 65535 is PB_ERR_ARG before any launch.  So is a call too large for the
 * encoder's 32-bit positions: a frame whose pb_jpeg_bound reaches 2^31 bytes (about 5.1 million blocks: 110 Mpixel at 4:4:4, 330 Mpixel mono) or
 * n frames of 2^25 blocks and more together (split the call).  The ctx keeps a
 * workspace of 353 bytes per 8 x 8 block (coefficients, offsets, the unstuffed stream) for the frames of one chunk (of the call, for _dev). */
typedef struct pb_jpeg_cfg {
    int32_t chroma;         /* 444, 420, 400 */
    int32_t quality;        /* 1 .. 100 */
} pb_jpeg_cfg;
int64_t pb_jpeg_bound(const pb_jpeg_cfg *cfg, int H, int W);
int pb_jpeg_encode(pb_ctx *ctx, const pb_jpeg_cfg *cfg, const uint8_t *planes, int n, int H, int W, uint8_t *out, int64_t capacity, int64_t *offsets);
int pb_jpeg_encode_dev(pb_ctx *ctx, const pb_jpeg_cfg *cfg, const uint8_t *planes, int n, int H, int W, uint8_t *out, int64_t capacity,
                       int64_t *offsets);

/* Bilinear resize of RGB frames, 8 bit, exact integers, half-pixel centres (the geometry of swscale's SWS_BILINEAR, which the reference's
 * VideoWriter applies to every frame that is not of the video's size).  Per axis, for output index x of n_out from n_in samples:
 *   num = (2 x + 1) n_in - n_out (may be negative);  i0 = floor(num / (2 n_out)), r = num - i0 * 2 n_out (0 <= r < 2 n_out);
 *   w = (256 r + n_out) / (2 n_out) (integer division, 0 .. 256);  taps clamp(i0, 0, n_in - 1) and clamp(i0 + 1, 0, n_in - 1)
 * and per channel, with the taps' four samples p00 p01 (row i0) p10 p11 (row i0 + 1):
 *   out = ((256 - wy) ((256 - wx) p00 + wx p01) + wy ((256 - wx) p10 + wx p11) + 32768) >> 16
 * Rounded once; an equal-size call is a byte copy.  The same two taps serve a shrink - swscale widens its filter there, this does not.  It is
 * not swscale's fixed-point code (PARITY UNPINNED: PyAV is not in the build image); tests/resize_ref.py pins the bytes by restatement and
 * Pillow's bilinear pins the geometry to one LSB on enlargements.  A side above 16384 is refused.
 * pb_rgb_resize: host pointers, blocking, in chunks of "host_chunk" frames (default 8); pb_rgb_resize_dev: device pointers, asynchronous on the
 * ctx stream.  out_i420 = 0: out is n x H x W x 3 uint8; 1: n x pb_i420_bytes(H, W) bytes, byte for byte pb_rgb_to_i420 of the resized frames,
 * which are never written to memory.  No alignment is needed (with W % 16 == 0 and a 16-byte aligned device `out` the kernels store 16 bytes
 * per access).  Work on any ctx.
 *   rgb : n x sh x sw x 3 uint8
 * Inside the flow bands: pb_set_option(ctx, "rgb_out_full", 1) makes the rgb_out of pb_flow_infer_sequence(_masks) and
 * pb_flow_submit_sequence(_masks) hold frames of the clip's H x W instead of the band's sh x sw (pb_flow_out_size) - H x W x 3 bytes per pair
 * and direction, or pb_i420_bytes(H, W) with "rgb_out_i420" - resized on the ctx stream from the sh x sw frame the band encodes: what a video
 * of the clip's size (the reference's VideoWriter) holds.  flow_out, mask_out and maxdisp_out stay at sh x sw, the *_dev entry points keep
 * sh x sw RGB, and where (sh, sw) == (H, W) the option changes no byte.  0 by default; set only while no submission is outstanding. */
int pb_rgb_resize(pb_ctx *ctx, const uint8_t *rgb, int n, int sh, int sw, int H, int W, uint8_t *out, int out_i420);
int pb_rgb_resize_dev(pb_ctx *ctx, const uint8_t *rgb, int n, int sh, int sw, int H, int W, uint8_t *out, int out_i420);

/* Network input size for an H x W frame: keep-aspect lower-bound resize to 518, each side a
 * multiple of 14 (bands/d_anything/util/transform.py:100-166). */
int pb_depth_net_size(int H, int W, int *net_h, int *net_w);

/* flow_raft band (band = "flow_raft", cfg = NULL; weights: fnet.*, cnet.*, update_block.*).
 * Replaces bands/flow_raft.py:98-113 (frame loop: cv2.resize(fx=fy=scale, INTER_CUBIC), [prev,curr] /
 * [curr,prev] batch), :51-62 infer (InputPadder, RAFT(iters, test_mode=True), unpad) and
 * bands/common/flow.py:64-88 write_flow -> encode.py:98-126 process_flow.
 *   frames     : F x H x W x 3 uint8 RGB, consecutive frames of one clip (F >= 2)
 *   outputs    : for pair i = (frame i, frame i+1) and direction d (0 = forward i -> i+1, 1 = backward when
 *                `backward` != 0), index i*dirs + d:
 *     flow_out   [F-1, dirs, sh, sw, 2] float32 (u, v) pixels at the scaled resolution, or NULL
 *     rgb_out    [F-1, dirs, sh, sw, 3] uint8 process_flow encoding, or NULL
 *     maxdisp_out[F-1, dirs] float32 max displacement (the band's CSV value), or NULL
 *   (sh, sw) = pb_flow_out_size(H, W, scale).
 *   scale      : the reference computes with Python's double; every call here takes the float's shortest round-trip decimal as that double
 *                (0.6f -> 0.6, not 0.60000002384), so sizes and resize taps are the reference's for any scale of up to 7 significant digits. */
int pb_flow_out_size(int H, int W, float scale, int *sh, int *sw);
int pb_flow_infer_sequence(pb_ctx *ctx, const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward,
                           float *flow_out, uint8_t *rgb_out, float *maxdisp_out);
int pb_flow_infer_sequence_dev(pb_ctx *ctx, const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward,
                               float *flow_out, uint8_t *rgb_out, float *maxdisp_out);
/* Forward/backward consistency masks.  Replaces bands/common/flow.py:19-40 compute_fwdbwd_mask as
 * called from bands/flow_raft.py:63-64: the opposite flow is sampled at p + f(p) with cv2.remap's INTER_LINEAR /
 * BORDER_CONSTANT arithmetic, and mask = |f + f'| < alpha1 (|f| + |f'|) + alpha2 (reference defaults 0.05, 0.5).
 *   pb_flow_infer_sequence_masks*: both directions are always computed (dirs = 2); flow_out / rgb_out / maxdisp_out
 *     as above (any may be NULL), mask_out [F-1, 2, sh, sw] bytes of 0 / 1 (index 0 = forward mask, 1 = backward).
 *   pb_flow_fwdbwd_mask: the mask step alone on host flows [n, 2, sh, sw, 2].
 * The host-pointer variant is the same chunked three-stage pipeline as pb_flow_infer_sequence (both directions of a pair are in one
 * chunk; page-locked caller buffers are used directly); every host-pointer pipeline drains its streams before it returns, error or not. */
int pb_flow_infer_sequence_masks(pb_ctx *ctx, const uint8_t *frames, int F, int H, int W, float scale, int iters,
                                 float alpha1, float alpha2, float *flow_out, uint8_t *rgb_out, float *maxdisp_out,
                                 uint8_t *mask_out);
int pb_flow_infer_sequence_masks_dev(pb_ctx *ctx, const uint8_t *frames, int F, int H, int W, float scale, int iters,
                                     float alpha1, float alpha2, float *flow_out, uint8_t *rgb_out, float *maxdisp_out,
                                     uint8_t *mask_out);
int pb_flow_fwdbwd_mask(pb_ctx *ctx, const float *flows, int n, int sh, int sw, float alpha1, float alpha2,
                        uint8_t *mask_out);
/* flow_gmflow band (band = "flow_gmflow", cfg = pb_flow_cfg or NULL; weights: backbone.*, transformer.*, feature_flow_attn.*,
 * upsampler.* of the GMFlow state dict).  Same entry points and output contract as flow_raft above (pb_flow_infer_sequence*,
 * pb_flow_out_size; `iters` is ignored): replaces bands/flow_gmflow.py:60-118 infer (cv2.resize by --scale, InputPadder(16),
 * GMFlow(attn_splits_list=[2], corr_radius_list=[-1], prop_radius_list=[-1], pred_bidir_flow per `backward`)) ->
 * bands/gmflow/gmflow.py:12-170 (shared instance-norm encoder, position encoding, 6 transformer blocks with 2 x 2 shifted windows,
 * global matching, self-attention propagation, convex upsampling) and the same write_flow / process_flow encode.
 * Two architectures are built (128 channels, 6 layers, 1 head, ffn x 4), and the WEIGHTS say which: the band's default (1 scale, attn_splits
 * 2, upsample_factor 8, InputPadder(16)), and GMFlow's refinement model (gmflow_with_refine: num_scales 2, upsample_factor 4,
 * padding_factor 32, attn_splits_list 2 8, corr_radius_list -1 R, prop_radius_list -1 r) when the state dict carries
 * backbone.trident_conv.weight [128, 128, 3, 3] and an upsampler.2.weight of 4 * 4 * 9 = 144 rows (576 rows and no trident weight: one
 * scale; anything else: PB_ERR_ARG naming the tensor).  The two-scale model runs the coarse scale at 1/8 exactly as the default model runs
 * (2 x 2 windows, global matching and propagation), enlarges its flow x 2, warps the target's 1/4 features by it, and runs the six blocks
 * again at 1/4 with 8 x 8 windows, local matching and local-window propagation, then convex upsampling by 4 (gmflow.py:112-165); frames are
 * padded to multiples of 32 and must reach 64 x 64.  Its backward direction is the forward direction of the swapped pair - what
 * pred_bidir_flow computes, every batch element of it being its own sample.  The band script rejects every other GMFlow flag set. */
/* 1 or 2: the architecture a flow_gmflow context was built with (see above); PB_ERR_ARG on other contexts. */
int pb_flow_num_scales(pb_ctx *ctx);
/* Stages of the last flow call: "fmap" [F,256,h/8,w/8], "flow_lo" [pairs*dirs, h/8*w/8, 2]; flow_gmflow (token-major fp32, shape
 * [n, tokens, channels, 1]): "feat" [F, h/8*w/8, 128] (encoder output), "block0" / "tfeat" [2 pairs, tokens, 128] (after the first / last
 * transformer block; both images of every pair), "flow_match" / "flow_prop" [pairs*dirs, tokens, 2].  On a two-scale context these names
 * mean the coarse scale, and the fine scale adds (B = pairs*dirs, P4 = h/4*w/4): "feat4" [F, P4, 128], "flow_up" [B, P4, 2] (the coarse flow
 * enlarged and doubled), "warp" [B, P4, 128] (the target's features warped by it), "block0_4" / "tfeat4" [2 B, P4, 128] (source and warped
 * target of every batch element), "flow_match4" [B, P4, 2] (flow_up + the matched residual), "flow_prop4" [B, P4, 2].  The fine scale re-uses
 * the token stream, so on a two-scale context the coarse "tfeat" and "block0" (like "block0" / "block0_4" everywhere) are copies made only
 * with pb_set_profiling's debug bit and are unknown stages without it.
 * One call on a two-scale context takes at most 511 (pair, direction) elements and 2^20 token rows (elements x 2 x P4): the host entry points
 * split a sequence into such chunks, the *_dev entry points refuse a larger F with PB_ERR_ARG. */
int64_t pb_flow_get_stage(pb_ctx *ctx, const char *name, float *out, int64_t cap, int64_t shape_out[4]);
/* flow_gmflow --inference_size (reference bands/flow_gmflow.py:76-100): with (h, w) > 0 - multiples of 16 - the network runs on
 * F.interpolate(bilinear, align_corners = True) of the (scaled) frame to h x w instead of on the frame padded to /16, and the flow is
 * resized back the same way with u * W' / w, v * H' / h.  (0, 0) turns it off.  flow_gmflow contexts only.  A two-scale context takes
 * multiples of 32, at least 64; a refused size leaves the context as it was. */
int pb_flow_set_inference_size(pb_ctx *ctx, int h, int w);
/* flow_gmflow --corr_radius_list R / --prop_radius_list r (reference bands/gmflow/gmflow.py:128-157, same checkpoint): -1 = global (the
 * default: nothing of the default path changes).  corr_radius 1 .. 4: local matching - the softmax runs over the (2 R + 1)^2 target tokens
 * around the source token, those outside the grid masked (matching.py:39-83).  prop_radius 1 .. 2: local-window propagation over
 * (2 r + 1)^2 zero-padded neighbours, pads counted in the softmax (transformer.py:376-409; its key is k_proj of the feature, where the
 * global form takes k_proj of the projected query).  Backward direction (`backward`, masks): with global matching it is the reference's
 * pred_bidir_flow; with a matching radius the reference's pred_bidir_flow raises (local_correlation_softmax returns B flows for 2 B
 * features), and the band defines it as the forward direction of the swapped pair - what pred_bidir_flow equals wherever the reference
 * can run it.  Other values are an error and leave the context as it was.  flow_gmflow contexts only.
 * On a two-scale context the two radii are the FINE scale's (the reference's -1 R / -1 r): R in 1 .. 4, r in 1 .. 2, default (4, 1); -1 is
 * refused there (global matching or propagation over the 1/4 grid is not built) and the coarse scale is always global. */
int pb_flow_set_matching(pb_ctx *ctx, int corr_radius, int prop_radius);
/* flow_raft --alternate_corr (reference bands/raft/raft.py:103-106 selects AlternateCorrBlock, bands/raft/corr.py:63-91, same checkpoint):
 * on != 0 - the 9 x 9 x 4 lookup of every GRU iteration computes its window entries from the feature maps (fp16 operands, fp32
 * accumulation, no fp16 rounding of an entry) instead of reading them from the all-pairs correlation volume, which is then neither
 * allocated nor computed: the arena loses pairs * dirs * P * sum_l ld_l * 2 bytes (P = 1/8-grid pixels).  0 (the default): nothing of the
 * default path changes.  Takes effect with the next call, which re-plans the arena.  flow_raft contexts only: on a flow_gmflow (or any
 * other) context it returns PB_ERR_ARG and leaves the context as it was. */
int pb_flow_set_alternate_corr(pb_ctx *ctx, int on);
/* Bytes of the arena the context's current plan committed (the last call's frame size, pair count and mode); 0 before the first call.
 * Flow contexts only. */
int64_t pb_flow_arena_bytes(pb_ctx *ctx);

/* mask_mmdet band (band = "mask_mmdet", cfg = pb_mask_cfg; weights: backbone.*, neck.*, mask_head.* in mmdet's
 * state_dict naming).  Replaces the per-frame body of bands/mask_mmdet.py:131-154: inference_detector
 * (mmdet/apis/inference.py:99-162: Resize keep_ratio (1333, 800) -> Normalize -> Pad 32 -> SOLOv2 forward ->
 * get_results / Matrix NMS -> format_results) and the accumulation of :43-61,139-147.
 *   frames      : n x H x W x 3 uint8 RGB (what decord hands the band; the reference swaps to BGR for mmdet and
 *                 Normalize(to_rgb) swaps back, so means / stds apply in RGB order)
 *   confidence  : --confidence; an instance is drawn when its class is kept and score > 0.5 and > confidence
 *   keep_classes: class ids (model.CLASSES order) the band keeps, mask_mmdet.py:30; NULL keeps every class
 *   mask_out    : n x H x W x 3 uint8: per pixel (255 * number of drawn instances covering it) mod 256 in all
 *                 three channels - `masks.astype(np.uint8)` of the reference's float64 sum.
 * pb_mask_get_instances: what format_results held for frame `frame` of the last call, score-descending: up to cap
 *   scores / labels; returns the count.  masks_out (optional, [count, H, W] bytes of 0 / 1) needs
 *   pb_set_profiling(ctx, 2) before the infer call.
 * pb_mask_net_size: resized (nh, nw) and padded (Hp, Wp) network input for an H x W frame.
 * The host-pointer variant (reference loop bands/mask_mmdet.py:131-154) pipelines over the engine's chunks of max_batch frames: every
 * chunk's frames go to the device up front on a copy stream, chunk i's id images return on a second one while chunk i + 1 runs. */
int pb_mask_infer_batch(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W, float confidence,
                        const int32_t *keep_classes, int n_keep, uint8_t *mask_out);
int pb_mask_infer_batch_dev(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W, float confidence,
                            const int32_t *keep_classes, int n_keep, uint8_t *mask_out);
int pb_mask_get_instances(pb_ctx *ctx, int frame, int cap, float *scores_out, int32_t *labels_out, uint8_t *masks_out,
                          int32_t *candidates_out);
int pb_mask_net_size(const pb_mask_cfg *cfg, int H, int W, int *nh, int *nw, int *Hp, int *Wp);
/* --sdf (process.py passes it on every run, /root/reference/process.py:46-48,207; bands/mask_mmdet.py:64-69 getSDF, :150-152): the
 * clamped signed distance field of the id image in its GREEN channel.  getSDF's byte is a function of the side of the mask a pixel is
 * on and of its (integer) squared Euclidean distance n to the other side; the host tabulates it with the reference's own float64
 * expression - tab_out[i] / tab_in[i] for n = i outside / inside the mask, the last entry (index n_tab - 1) for every n >= n_tab - 1
 * (the remap saturates at sdf >= 64.25 and <= -63.25, so n_tab = 4130 holds every distinct byte; n_tab <= 4226) - and the library
 * computes the exact n on the device (mask_kernels.hip sdf_*_kernel).
 *   pb_mask_set_sdf : n_tab > 0 turns the green channel on for every following pb_mask_infer_batch* call of the ctx, 0 turns it off
 *   pb_mask_sdf_green(_dev): the same pass on id images the caller holds ([n, H, W, 3] uint8, in place; host / device pointer) */
int pb_mask_set_sdf(pb_ctx *ctx, const uint8_t *tab_out, const uint8_t *tab_in, int n_tab);
int pb_mask_sdf_green(pb_ctx *ctx, uint8_t *masks, int n, int H, int W);
int pb_mask_sdf_green_dev(pb_ctx *ctx, uint8_t *masks, int n, int H, int W);
/* Stages of the last mask call as float32 NCHW: "input", "c2".."c5", "p2".."p6", "mask_feats",
 * "kernel_pred<l>", "cls_logit<l>" (l = 0..4). */
int64_t pb_mask_get_stage(pb_ctx *ctx, const char *name, float *out, int64_t cap, int64_t shape_out[4]);

/* Debug/parity: copy a named intermediate of the last pb_depth_infer_batch* call to the host
 * as float32 in the reference's layout ([n, C, h, w] for maps, [n, tokens, D] for tokens).
 * Names: "tokens", "block<i>", "feat<i>", "layer<i>_rn", "path<i>", "output_conv1", "net_depth".
 * shape_out receives up to 4 dims; returns the element count or a negative pb_status.  shape_out[0] is the number of frames the
 * stage holds: the whole call for the ViT's stages; for the DPT head's stages the LAST head chunk (the trailing shape_out[0] frames of
 * the call) when the call was large enough for the head to run in several chunks (split precision: more than 16 frames of 1080p). */
int64_t pb_depth_get_stage(pb_ctx *ctx, const char *name, float *out, int64_t cap, int64_t shape_out[4]);

/* Device memory helpers so a Python host without torch can keep frames resident. */
int pb_dev_alloc(pb_ctx *ctx, void **ptr, size_t bytes);
int pb_dev_free(pb_ctx *ctx, void *ptr);
int pb_memcpy_h2d(pb_ctx *ctx, void *dst, const void *src, size_t bytes);
int pb_memcpy_d2h(pb_ctx *ctx, void *dst, const void *src, size_t bytes);

/* Timing of the kernels launched by the last infer call, measured with HIP events on the ctx
 * stream: fills up to cap entries; returns the count.  name points into static storage. */
typedef struct {
    const char *name;     /* kernel family, e.g. "gemm_f16", "attention", "conv3x3"      */
    double ms;            /* summed event time of that family in the last call            */
    double flops;         /* algorithmic FLOPs those launches performed (2 M N K of the layers) */
    double exec_flops;    /* MFMA work actually issued, in fp16-pass equivalents: x1.5 ... x3 for the split layers (PB_PREC_SPLIT; an e4m3 pass counts 0.5) */
    double bytes;         /* algorithmic HBM bytes (compulsory traffic) of those launches */
    int32_t launches;
} pb_kernel_stat;
/* enabled: bit 0 = time every kernel launch with HIP events on the ctx stream, bit 1 = keep debug stages / instance
 * masks, bit 2 = accumulate the timings over successive infer calls (pb_get_kernel_stats then reports the sums since
 * this call) instead of restarting at every infer call. */
int pb_set_profiling(pb_ctx *ctx, int enabled);
/* Tuning / A-B switches: "gemm_tile", "conv_tile" = 0 auto, 1 128x128, 2 256x256 ping-pong, 3 256x32, 9 256x64,
 * 12 128x96 (convolutions with N <= 96) (prisma_amd/csrc/gemm.h; the other round-1 variants were measured slower and
 * removed); "tile_n96" (process-wide) = 0: convolutions with 64 < N <= 96 stay on the 128x128 tile, 1: auto gives them
 * the 128x96 tile (same bytes), 2 (default): ... and the packed-channel K axis where the weights carry one (RAFT encoder
 * stage 2: another summation order); "host_chunk", "op_splitk": see INTEGRATION.md; "frames_i420", "rgb_out_i420" (0 | 1): see pb_i420_bytes;
 * "rgb_out_full" (0 | 1): see pb_rgb_resize; "corr_layout" (0 | 1, flow_raft): 1 (default) = the correlation volume
 * source-blocked, read by corr_lookup_blocked_kernel, 0 = row-major and corr_lookup_kernel - same bytes out (prisma_amd/csrc/corr_layout.h). */
int pb_set_option(pb_ctx *ctx, const char *key, int value);
int pb_get_kernel_stats(pb_ctx *ctx, pb_kernel_stat *out, int cap);

/* ---- single-kernel entry points (host buffers) used by the -m gpu parity tests ---------- */
/* C[M,N] = act(A[M,K] @ W[N,K]^T + bias) with fp16 operands, fp32 accumulate (MFMA).       */
int pb_op_gemm(pb_ctx *ctx, const float *A, const float *W, const float *bias, float *C,
               int M, int N, int K, int act /*0 none,1 relu,2 gelu*/, int tile /*0 auto,1 128x128,2 256x256*/);
/* Kernel micro-benchmark on device-resident uniform[-1,1) fp16 data: mean ms per launch over iters.
 * epi: 0 fp16 store, 1 bias+GELU fp16 store, 2 LayerScale + fp32 residual read-modify-write. */
int pb_op_gemm_bench(pb_ctx *ctx, int M, int N, int K, int tile, int epi, int iters, double *ms_out);
/* The flow band's all-pairs correlation kernel on its own (bands/raft/corr.py:52-60, without the 1/sqrt(256) factor the band folds into the
 * features): out[m, n] = fp16(sum_k fp16(A[m, k]) fp16(W[n, k])), A [M, 256], W [N, 256] fp32 on the host, N % 8 == 0, ldo >= N.
 * `out` holds (M + guard_rows) x ldo floats; everything the kernel must not touch - columns N..ldo-1 and the guard rows - is preset to NaN. */
int pb_op_corr_volume(pb_ctx *ctx, const float *A, int M, const float *W, int N, int ldo, int guard_rows, float *out);
/* The same kernel storing flow_raft's source-blocked volume layout (prisma_amd/csrc/corr_layout.h; ldo % 64 == 0): `out` holds the raw halfs,
 * round_up(M, 8) rows of ldo entries and guard_halfs behind them, preset to 0x7e7e.  pb_op_corr_layout_index (no GPU needed): out[p * pld + c] =
 * the offset in halfs of entry c of source row p < P in layout 0 (row-major) / 1 (blocked) - corr_layout.h's function, the one the kernels use. */
int pb_op_corr_volume_blocked(pb_ctx *ctx, const float *A, int M, const float *W, int N, int ldo, int guard_halfs, void *out);
int pb_op_corr_layout_index(int layout, int P, int pld, int64_t *out);
/* LayerNorm over the last dim, eps 1e-6 (vision_transformer.py:95). */
/* times `iters` launches of the fused attention kernel on random Q, K, V (variant 0 = default); ms per launch */
int pb_op_attention_bench(pb_ctx *ctx, int B, int heads, int N, int variant, int iters, double *ms_out);
int pb_op_layernorm(pb_ctx *ctx, const float *x, const float *g, const float *b, float *y, int rows, int D);
/* softmax(q k^T * 64^-0.5) v per (batch, head); q,k,v,o: [B, heads, N, 64] float32
 * (dinov2/layers/attention.py:49-62). */
int pb_op_attention(pb_ctx *ctx, const float *q, const float *k, const float *v, float *o,
                    int B, int heads, int N);
/* NCHW float32 conv2d via NHWC fp16 implicit GEMM: x [B,Ci,H,W], w [Co,Ci,kh,kw]. */
/* single-head attention over 128-wide heads, q / k / v / o [B, L, 128]; region [B, L] or NULL: a key whose region id differs from the
 * query's gets -100 on its logit (bands/gmflow/transformer.py:8-15, 18-44, 47-101) - a building block of the flow_gmflow band */
int pb_op_attention128(pb_ctx *ctx, const float *q, const float *k, const float *v, const int8_t *region, float *o, int B, int L);
/* the same attention in the flow_gmflow band's split precision (q, k, v and the probabilities as hi + lo fp16 pairs: three MFMA passes
 * for the scores and for P V); v / o [B, L, vcols] with vcols 128 or 32 (coordinates / flow padded to 32 columns); region [nreg, L],
 * batch element b uses row b % nreg; keys and values of batch element b are those of b ^ kxor (cross attention between a pair's frames) */
int pb_op_attention128_split(pb_ctx *ctx, const float *q, const float *k, const float *v, const int8_t *region, int nreg, float *o,
                             int B, int L, int vcols, int kxor);
int pb_op_conv2d(pb_ctx *ctx, const float *x, const float *w, const float *bias, float *y,
                 int B, int Ci, int H, int W, int Co, int ksize, int stride, int pad, int relu_in, int relu_out);
/* One convolution / dense layer in the engines' split precision, through their own weight packers and launch code (EngineBase pack_conv / pack,
 * set_weights, conv() / dense()).  layout: 0 fp16, 1 split16 (fp16 residual parts; sa = 1: the map is [hi | lo], 0: [hi]), 2 mx3 (maps
 * [hi | hi8 | lo8] with e4m3 residual parts), 3 mx2 (maps [a16 | a8]: the layer reads channels [ci_off, ci_off + Ci) of a Ctot-channel map).
 * The map is built on the host from x (NHWC [B, H, W, Ci], or [B, H, W, Ctot] for mx2; dense: A [M, K]) the way the producing epilogues
 * write it.  w [Co, Ci, kh, kw] (dense: [N, K]), bias [Co]; skip (or NULL) [M, Co] is added in the output's layout.  tapin: slice-major K
 * order; tile: 0 = the engines' choice (the halo conv included), else a gemm.h TILE_*; split_out: the output is a split map (lo_off = its
 * channels padded to 64).  `out` receives the raw output buffer, rows_out x ldo halfs (rows_out >= M rounded up to 256), preset to 0xFF
 * bytes where the launch must not write; info[13] = {pw, map pa, mx3, mx2, sa, sw, tapin, packed K, packed-channel copy, Cseg, ldo, lo8,
 * lo8 pa}; kernel = the symbol that ran (pb_set_option "op_splitk" lends a split-K workspace). */
int pb_op_conv2d_split(pb_ctx *ctx, const float *x, const float *w, const float *bias, const float *skip, int B, int H, int W, int Ci, int Ctot,
                       int ci_off, int Co, int kh, int kw, int stride, int layout, int sa, int tapin, int tile, int split_out, int act,
                       int pre_relu, int rows_out, void *out, int *info, char *kernel, int kernel_cap);
int pb_op_dense_split(pb_ctx *ctx, const float *A, const float *w, const float *bias, const float *skip, int M, int K, int N, int layout,
                      int sa, int tile, int split_out, int act, int rows_out, void *out, int *info, char *kernel, int kernel_cap);
/* The GEMM's fused ViT epilogues one by one, launched as DepthEngine::vit launches them (tests/test_gpu_epilogue_ops.py).  layout: 0 fp16, 1
 * split16 (weights hi + lo fp16, activations [hi]), 3 mx2 (weights [w_hi | w_lo8], token rows [a16 | a8]); tile: a gemm.h TILE_* (1: 128 x 128, 2:
 * the 256 x 256 ping-pong kernel); info[8] = {pw, a8 / lo8 pa, mx2, sw, packed K, nk16, mx3, split-K factor of the launch}; kernel = the symbol that ran.  Output buffers are preset to
 * 0xFF bytes and carry guard_rows untouched rows behind the last one; pb_set_option "op_splitk" lends a split-K workspace.
 * resid: X [M, N] (fp32, copied into rows of ldr floats) += A [M, K] (gamma . w [N, K])^T + gamma . bias, LayerScale folded on the host as
 *   DepthEngine::load folds it and also passed as GemmArgs::gamma; out (M + guard) x ldr floats.
 * qkv: A [B ntp, D] x w [3 D, D]^T + bias -> q (x PB_QSCALE) and k, (B D/64 ntp + guard) x 64 halfs as [b, head, t, 64]; vt (B D/64 64 + guard) x ntp
 *   halfs as [b, head, 64, ntp].
 * patch: A [B P, 588] x w [D, 588]^T + bias + pos [1 + P, D] rows 1 .. P -> rows b ntp + 1 + patch of out, (B ntp + guard) x D floats.
 * conv_head: the DPT head's fused output_conv2 (EPI_HEAD): x NHWC [B, H, W, C], w [32, C, 3, 3], bias [32]; out[m] = relu(sum_n relu(conv + bias)[n]
 *   w2[n] + b2), (B H W + guard) floats.  Here layout 1 is split16 with a split map [hi | lo] and 2 is mx3 ([hi | hi8 | lo8]).
 * fc1: gelu(A [M, K] w [N, K]^T + bias) as the split ViT's fc1 runs (EPI_STD on the MX build with an all-fp16 K axis, nk16 = K / 64); out: (M + guard)
 *   rows of [fp16 (N) | e4m3 (N bytes) of the stored fp16 x 2^(a8 pa)].
 * pixshuf: the DPT head's transposed convolutions (kernel == stride == s) as a 1 x 1 GEMM with the pixel-shuffle epilogue (EPI_PIXSHUF): x [B h w, C],
 *   wt [C, C, s, s] (ConvTranspose2d), bias [C]; out: (B h s w s + guard) pixels of ldo = (layout ? 2 : 1) x (C padded to 64) halfs, layouts as
 *   conv_head's for the input map and the output alike. */
int pb_op_gemm_resid(pb_ctx *ctx, const float *A, const float *w, const float *bias, const float *gamma, const float *X, int M, int N, int K, int ldr,
                     int layout, int tile, int guard_rows, float *out, int *info, char *kernel, int kernel_cap);
int pb_op_gemm_qkv(pb_ctx *ctx, const float *A, const float *w, const float *bias, int B, int ntp, int D, int layout, int tile, int guard_rows, void *q,
                   void *k, void *vt, int *info, char *kernel, int kernel_cap);
int pb_op_gemm_patch(pb_ctx *ctx, const float *A, const float *w, const float *bias, const float *pos, int B, int P, int ntp, int D, int layout,
                     int guard_rows, float *out, int *info, char *kernel, int kernel_cap);
/* SepConvGRU's fused epilogues (ACT_GRU_ZR / ACT_GRU_Q) through EngineBase::conv with the ConvFuse RaftEngine::infer builds.  x [n, H, W, 384]: the
 * GRU input map, of which the kh x kw convolution reads the first gc (256 with the hoisted terms add1 / add2, else 384) channels; layout 0 fp16 or 3
 * mx2 (map [a16 (384) | a8 (384 bytes)], row stride 576 halfs, fp8 twins stored at byte 768).  zr: w [256, gc, kh, kw]; z = sigmoid -> zrb columns
 * [0, 128) ((rows + guard) x 256 halfs, the r half is not written), r h32 -> rh ((rows + guard) x 384 / 576 halfs).  q: w [128, gc, kh, kw], z
 * [rows, 256]; h32 = (1 - z) h32 + z tanh(.) in place ((rows + guard) x 128 floats, guard rows preset by the caller), its fp16 (and fp8) copy -> out
 * ((rows + guard) x 384 / 576 halfs).  add1 / add2: [rows, N] or NULL. */
int pb_op_raft_gru_zr(pb_ctx *ctx, const float *x, const float *w, const float *bias, const float *add1, const float *add2, float *h32, int n, int H, int W,
                      int gc, int kh, int kw, int layout, int tile, int guard_rows, void *zrb, void *rh, int *info, char *kernel, int kernel_cap);
int pb_op_raft_gru_q(pb_ctx *ctx, const float *x, const float *w, const float *bias, const float *add1, const float *add2, const float *z, float *h32, int n,
                     int H, int W, int gc, int kh, int kw, int layout, int tile, int guard_rows, void *out, int *info, char *kernel, int kernel_cap);
/* conv_pixshuf: the convolution form of EPI_PIXSHUF (RAFT's encoder stem): x [B, H, W, 64], w [256, 64, 3, 3] with output channel (dy 2 + dx) 64 + co,
 * bias [64], act 0 / 1 (ReLU); out: (B 2H 2W + guard) pixels of (layout ? 128 : 64) halfs, layouts as pb_op_gemm_pixshuf's. */
int pb_op_conv_pixshuf(pb_ctx *ctx, const float *x, const float *w, const float *bias, int B, int H, int W, int layout, int act, int guard_rows, void *out,
                       int *info, char *kernel, int kernel_cap);
int pb_op_gemm_fc1(pb_ctx *ctx, const float *A, const float *w, const float *bias, int M, int K, int N, int tile, int guard_rows, void *out, int *info,
                   char *kernel, int kernel_cap);
int pb_op_gemm_pixshuf(pb_ctx *ctx, const float *x, const float *wt, const float *bias, int B, int h, int w, int C, int s, int layout, int tile,
                       int guard_rows, void *out, int *info, char *kernel, int kernel_cap);
int pb_op_conv_head(pb_ctx *ctx, const float *x, const float *w, const float *bias, const float *w2, float b2, int B, int H, int W, int C, int layout,
                    int guard_rows, float *out, int *info, char *kernel, int kernel_cap);
/* The flow_raft band's own kernels one by one, through the launchers and arguments RaftEngine::infer uses (tests/test_gpu_raft_ops.py).  Raw
 * output buffers are preset to 0xFF bytes (NaN as fp16, fp32 and e4m3) and carry guard_rows untouched rows behind the last one.
 * pb_op_raft_geometry (no GPU needed): geo[l * 5 + {0..4}] = {h, w, padded w, padded h, volume row stride} of pyramid level l over an h8 x w8
 * grid - the function RaftEngine::prepare plans with.
 * lookup: avg-pool x3, tile x4, the all-pairs volume x4 per pair, then the 9 x 9 x 4 lookup.  fmap1 [n, h8 w8, 256], fmap2 [n, h8, w8, 256],
 *   flow [n h8 w8, 2]; out: (rows + guard) x (o8 ? 576 : 384) halfs (o8: the e4m3 copy at byte 768 of a row); levels (or NULL): the four volume
 *   levels de-tiled, [n h8 w8, h_l, w_l] floats one after the other.  The volume between the kernels is stored as the ctx's "corr_layout" option says.
 * convf1: flow [n, h8, w8, 2], w [128, 2, 7, 7], bias [128]; passes 1 / 2 (w_hi, + w_lo); out: (rows + guard) x (o8 ? 192 : 128) halfs (e4m3
 *   copy at byte 256); gemm_path: im2col + GEMM (PB_CONVF1_DIRECT=0) instead of the direct kernel.
 * flow_head2: x [n, H, W, 256], w [2, 256, 3, 3], bias [2]; flow [n H W + guard, 2] is read (rows < n H W) and written in place.
 * upsample: flow [n, h8 w8, 2], mask [n h8 w8, 576] -> up [n, sh, sw, 2] + guard floats, maxd [n] as the encode kernel decodes it.
 * instnorm: a (and b) [B, HW, C] -> stats [B, C, 2] = {mean, rstd} of a, out (B HW + guard) x ld halfs; layout 0 [C], 1 [hi | lo], 2 [hi | hi8 |
 *   lo8] (ld = 2 C); stats_lo: statistics of hi + lo; bmode 0 none / 1 raw / 2 normalised second operand; inplace: out is a's buffer.
 * state: init_state on ctx_rows [rows, 256] (flow0 = the flow it leaves, rows + guard), then put_flow of `flow` [rows, 2]; ld 384 / 576 (fp8
 *   copies at byte 768), inp_off 128 / 256; h32 (rows + guard) x 128 floats, hx / hx2 (rows + guard) x ld halfs. */
int pb_op_raft_geometry(int h8, int w8, int *geo);
int pb_op_raft_lookup(pb_ctx *ctx, const float *fmap1, const float *fmap2, const float *flow, int n, int h8, int w8, int o8, int guard_rows,
                      void *out, float *levels);
/* lookup_otf (--alternate_corr): the inputs, output convention and refusals of pb_op_raft_lookup; avg-pool x3, then corr_lookup_otf_kernel. */
int pb_op_raft_lookup_otf(pb_ctx *ctx, const float *fmap1, const float *fmap2, const float *flow, int n, int h8, int w8, int o8,
                          int guard_rows, void *out);
int pb_op_raft_convf1(pb_ctx *ctx, const float *flow, const float *w, const float *bias, int n, int h8, int w8, int passes, int o8,
                      int gemm_path, int guard_rows, void *out);
int pb_op_raft_flow_head2(pb_ctx *ctx, const float *x, const float *w, const float *bias, float *flow, int n, int H, int W, int split,
                          int guard_rows);
int pb_op_raft_upsample(pb_ctx *ctx, const float *flow, const float *mask, int n, int h8, int w8, int pad_l, int pad_t, int sh, int sw,
                        int guard, float *up, float *maxd);
int pb_op_raft_instnorm(pb_ctx *ctx, const float *a, const float *b, int B, int HW, int C, int layout, int stats_lo, int bmode, int inplace,
                        int guard_rows, float *stats, void *out);
int pb_op_raft_state(pb_ctx *ctx, const float *ctx_rows, const float *flow, int rows, int ld, int inp_off, int guard_rows, float *h32, void *hx,
                     void *hx2, float *flow0);
/* The flow bands' frame path outside the networks - the first kernel and the last kernels of every flow_raft / flow_gmflow call
 * (tests/test_gpu_flow_io_ops.py).  Outputs are preset to 0xFF bytes and carry a guard, as above.
 * pb_op_flow_geometry (no GPU needed): geo[0..8] = {sh, sw, Hp, Wp, pad_l, pad_t, h8, w8, P} of an H x W frame at `scale`, padded to a multiple
 *   of `factor` (8, 16 or 32) - the function the engines plan with.
 * pb_op_flow_taps (no GPU needed): the 8-bit cubic table of one axis the engines upload: idx, co [dst, 4] (co = coefficient x 2048).
 * flow_prep: n uint8 frames [n, H, W, 3] through ONE launch of the prep kernel with the engines' arguments.  norm_mode 0: RAFT's 2 x / 255 - 1,
 *   1: GMFlow's ImageNet mean / std.  isz_h, isz_w > 0: GMFlow's --inference_size (bilinear, align_corners, no padding; Hp x Wp = the
 *   inference size).  out: (n Hp / 4 Wp / 4 + guard_rows) rows of one 4 x 4 block each - layout 0: 64 halfs (((y & 3) 4 + (x & 3)) 4 + c,
 *   channel 3 zero), 1: [hi | lo] 128 halfs, 2: [hi (64 halfs) | hi8 (64 bytes) | lo8 (64 bytes)] with the e4m3 scales 2^*lo8_pa and
 *   2^(*lo8_pa + 12).  scaled: the scaled uint8 frames [n, sh, sw, 3] + guard bytes (left preset with an inference size).
 * flow_resize_back: in [n, ih, iw, 2] -> out [n, sh, sw, 2] + guard floats (bilinear, align_corners, u sw / iw, v sh / ih); maxd [n]: the
 *   per-frame maximum displacement as the encode kernel decodes it.
 * flow_encode: flow [n, sh, sw, 2] and the per-frame maximum maxd [n] -> rgb [n, sh, sw, 3] + guard bytes, max_out [n]. */
int pb_op_flow_geometry(int H, int W, float scale, int factor, int *geo);
int pb_op_flow_taps(int src, int dst, float scale, int *idx, int *co);
int pb_op_flow_prep(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W, float scale, int factor, int layout, int norm_mode, int isz_h,
                    int isz_w, int guard_rows, int guard, void *out, uint8_t *scaled, int *lo8_pa);
int pb_op_flow_resize_back(pb_ctx *ctx, const float *in, int n, int ih, int iw, int sh, int sw, int guard, float *out, float *maxd);
int pb_op_flow_encode(pb_ctx *ctx, const float *flow, const float *maxd, int n, int sh, int sw, int guard, uint8_t *rgb, float *max_out);
/* The flow_gmflow band's own kernels one by one, through the launchers and arguments GmflowEngine::infer uses (tests/test_gpu_gmflow_ops.py).
 * (h8, w8) is the 1/8-resolution token grid (both even, >= 4): P = h8 w8 tokens per image, 2 x 2 windows of Lw = P / 4 tokens, V^T row strides
 * ldv = Lw and ldvP = P rounded up to 32.  Raw buffers are preset to 0xFF bytes and carry guard_rows untouched rows, as above.
 * pb_op_gm_tables (no GPU needed): the two host tables of the engine's plan - pos [P, 128] (per-window sine embedding, tiled) and the
 *   shifted-window region ids [4, Lw] in window order.
 * tokens: feat [NP + 1, P, 128], pos [P, 128] -> X (2 NP P + guard) x 128 floats, Xs the same rows x 256 halfs [hi | lo].
 * split_rows: src [rows, ld] of which C columns -> (rows + guard) x 2 C halfs.   grid_vt: (64 + guard) x ldvP halfs.
 * pack: src [images P, ld]; job j takes columns cols[j] .. + 128 as kinds[j] 0: window rows (4 images Lw + guard) x 256 halfs, 1: V^T
 *   (4 images x 2 x 128 + guard) x ldv halfs; outs[j] receives job j's buffer.
 * ln: M [rows, 128], X (xrows + guard) x 128 floats read and returned whole; out (xrows + guard) x (mode ? 512 : 256) halfs.
 * match_flow: O [B, P, 32] -> flow (B P + guard) x 2 floats, vt (64 B + guard) x ldvP halfs, NOT zeroed first (the engine's arena is).
 * upsampler_in: O [B, P, 32], X [images, P, 128] (batch element b takes image b img_step) -> flow (B P + guard) x 2, map (B P + guard) x 384 halfs.
 * pb_op_attention128_cfg: attention128.hip's general form.  q, k [B, L, 128] as rows of ldq halfs ([hi] or [hi | lo]); strided 0: packed
 *   buffers; 1: ONE buffer of B images, Q = K, batch stride one image, kxor 1 (k unused); 2: ONE buffer [q_0, k_0, q_1, ..], stride two images,
 *   K = Q + one image.  v [v_shared ? 1 : B, L, vcols] as V^T [.., 2, vcols, ldv]; `fill` goes into columns [L, ldv) and into the lo rows
 *   wherever the kernel must not read them (split = 0 or pv_single).  region [nreg, L] or NULL.  o [B, L, vcols].
 * window_block: Y [images P, 384] = q | k | v in token order; pack, the window attention (pv_single, the production region table when
 *   shifted, kxor 4 when cross), then gm_ln (windowed, mode 0, gamma / beta [128]) on the attention output; X [images P, 128] in and out.
 * match: tokens [2 NP, P, 128]; split_rows, the global matching over the shared coordinate V^T, match_flow -> flow [NP dirs, P, 2].
 * propagate: q, k, X [2 NP, P, 128], flow_in [NP dirs, P, 2]; match_flow on flow_in + own coordinate (flow_match returns the fp32 flow it made
 *   of that), the propagation attention, upsampler_in -> flow_prop [NP dirs, P, 2], map (NP dirs P + guard) x 384 halfs.  Both flow chains
 *   zero the flow V^T first, as the engine's arena is zeroed.
 * local_match (gmflow_local.hip): tokens [2 NP, P, 128]; batch element (pair, direction) reads source image 2 pair + dir and the other image
 *   of the pair as target (dirs 1: the even images only) -> flow (NP dirs P + guard) x 2 floats; 1 <= radius <= 4.
 * local_propagate: q, k [B img_step, P, 128] (batch element b takes image b img_step), flow_in [B, P, 2] -> flow_out (B P + guard) x 32
 *   floats, the propagation output's layout: the kernel owns columns 0, 1 (where upsampler_in reads the flow); 1 <= radius <= 2.
 * The two-scale model's forms (tests/test_gpu_gmflow_scale2_ops.py).  `splits` is 2 (as above) or 8: the (h, w) grid - multiples of splits, at
 *   least two tokens per window and axis - is cut into splits x splits windows, window index wy splits + wx, region table [splits^2, Lw],
 *   and the cross attention pairs a window with the other image's same window.  tables_n / pack_n / ln_n / window_block_n are tables / pack /
 *   ln / window_block with that argument (pack: splits^2 images Lw window rows).  window_block_n also takes pv_single: 1 is window_block's
 *   attention (P and V single fp16, the one-scale model's), 0 the attention a two-scale context launches on both of its scales (P and V
 *   split into hi + lo, nreg = splits^2, kxor = splits^2 when cross).
 * tokens_warped: feat [B / dirs + 1, P, 128], warped [B, P, 128], pos [P, 128]: batch element b = pair dirs + d takes frame pair + d plus pos
 *   as image 2 b and warped[b] plus pos as image 2 b + 1 -> X (2 B P + guard) x 128 floats, Xs the same rows x 256 halfs.
 * warp: flow8 [B, h8 w8, 2], feat4 [B / dirs + 1, 4 h8 w8, 128] -> flow_up (4 B h8 w8 + guard) x 2 floats = 2 x the bilinear (align_corners)
 *   enlargement to (2 h8) x (2 w8), warped (4 B h8 w8 + guard) x 128 floats = the features of frame pair + 1 - d sampled at token + flow_up
 *   (bilinear, align_corners, zeros outside the grid).
 * upsample: pb_op_raft_upsample with the factor: 8, or 4 with mask rows of 4 * 4 * 9 = 144 floats on the (h, w) = 1/4 grid. */
int pb_op_gm_tables(int h8, int w8, float *pos, int8_t *region);
int pb_op_gm_tables_n(int h, int w, int splits, float *pos, int8_t *region);
int pb_op_gm_tokens_warped(pb_ctx *ctx, const float *feat, const float *warped, const float *pos, int B, int dirs, int P, int guard_rows, float *X,
                           void *Xs);
int pb_op_gm_warp(pb_ctx *ctx, const float *flow8, const float *feat4, int B, int dirs, int h8, int w8, int guard_rows, float *flow_up,
                  float *warped);
int pb_op_gm_upsample(pb_ctx *ctx, const float *flow, const float *mask, int n, int h, int w, int factor, int pad_l, int pad_t, int sh, int sw,
                      int guard, float *up, float *maxd);
int pb_op_gm_pack_n(pb_ctx *ctx, const float *src, int images, int h, int w, int splits, int ld, int njobs, const int *cols, const int *kinds,
                    int shifted, int guard_rows, void **outs);
int pb_op_gm_ln_n(pb_ctx *ctx, const float *M, const float *gamma, const float *beta, float *X, int rows, int xrows, int h, int w, int splits,
                  int windowed, int shifted, int mode, int guard_rows, void *out);
int pb_op_gm_window_block_n(pb_ctx *ctx, const float *Y, float *X, const float *gamma, const float *beta, int images, int h, int w, int splits,
                            int shifted, int cross, int split, int pv_single);
int pb_op_gm_tokens(pb_ctx *ctx, const float *feat, const float *pos, int NP, int P, int guard_rows, float *X, void *Xs);
int pb_op_gm_split_rows(pb_ctx *ctx, const float *src, int rows, int ld, int C, int guard_rows, void *out);
int pb_op_gm_grid_vt(pb_ctx *ctx, int h8, int w8, int guard_rows, void *out);
int pb_op_gm_pack(pb_ctx *ctx, const float *src, int images, int h8, int w8, int ld, int njobs, const int *cols, const int *kinds, int shifted,
                  int guard_rows, void **outs);
int pb_op_gm_ln(pb_ctx *ctx, const float *M, const float *gamma, const float *beta, float *X, int rows, int xrows, int h8, int w8, int windowed,
                int shifted, int mode, int guard_rows, void *out);
int pb_op_gm_match_flow(pb_ctx *ctx, const float *O, int B, int h8, int w8, int guard_rows, float *flow, void *vt);
int pb_op_gm_upsampler_in(pb_ctx *ctx, const float *O, const float *X, int B, int images, int P, int img_step, int guard_rows, float *flow,
                          void *map);
int pb_op_attention128_cfg(pb_ctx *ctx, const float *q, const float *k, const float *v, const int8_t *region, int nreg, float *o, int B, int L,
                           int split, int pv_single, int vcols, int v_shared, int kxor, int ldq, int strided, float fill);
int pb_op_gm_window_block(pb_ctx *ctx, const float *Y, float *X, const float *gamma, const float *beta, int images, int h8, int w8, int shifted,
                          int cross, int split);
int pb_op_gm_match(pb_ctx *ctx, const float *tokens, int NP, int h8, int w8, int dirs, int split, float *flow);
int pb_op_gm_propagate(pb_ctx *ctx, const float *q, const float *k, const float *flow_in, const float *X, int NP, int h8, int w8, int dirs,
                       int split, int guard_rows, float *flow_match, float *flow_prop, void *map);
int pb_op_gm_local_match(pb_ctx *ctx, const float *tokens, int NP, int h8, int w8, int dirs, int radius, int guard_rows, float *flow);
int pb_op_gm_local_propagate(pb_ctx *ctx, const float *q, const float *k, const float *flow_in, int B, int h8, int w8, int img_step, int radius,
                             int guard_rows, float *flow_out);
/* The mask_mmdet band's own kernels one by one, through the launchers of mask_kernels.h with MaskEngine's arguments (tests/test_gpu_mask_ops.py).
 * Maps are rows of fp16: C halfs, or [hi (C) | lo (C)] with split; row strides L(C) = C (1 + split) unless ldi / ldo say otherwise (then the
 * halfs a row does not define are NaNs on the way in).  Inputs are fp32 and are rounded to the layout on the host (hi = fp16(v),
 * lo = fp16(v - hi)).  Raw outputs are preset to 0xFF bytes and carry guard_rows untouched rows (guard: elements).
 * prep: frames uint8 [n, H, W, 3], xt [nw, 4] / yt [nh, 4] = {i0, i1, c0, c1} -> out (n Hp/4 Wp/4 + guard) x 64 (1 + split) halfs, chw 3 n Hp Wp + guard floats.
 * maxpool / subsample2 / nearest_add / coord_concat / bilinear: x [rows, C] NHWC.  nearest_add returns dst += src; bilinear accumulates into y0
 *   when it is given.  coord_concat writes C + 64 channels per part.
 * gn_relu: layout 0 fp16 -> fp16, 1 split -> split, 2 split -> [hi | hi | lo] rows of 3 C halfs; aff [n, C, 2] = the per-channel (rstd gamma, group mean).
 * cls_points_nms: logit [n, g g, C] -> score (n pts_total + guard) x C floats, this level's cells from row `off` of every frame.
 * gather_rows: src [src_rows, cols], idx [count] -> (rows_pad + guard) x cols (1 + split) halfs.
 * stats: logit [rows, ld] -> (rows + guard) x {area, soft sum}.
 * intersections: bitpack_rows of rows idx[0 .. n) of logit [src_rows, ld], then mask_intersections with ld 512: bits (n + guard) x HW / 64 words,
 *   inter [inter_rows, 512] floats returned whole.
 * matrix_nms: inter [n, 512], area / label / score [n] -> comp, out (n + guard) floats.
 * sigmoid_rows: -> (count + guard) x HW floats.
 * dynconv: post_chunk's dynamic convolution.  gather_rows builds A from kernels [src_rows, 256] and idx [row_off + M]; the launch reads its rows
 *   from row_off (a multiple of 8); feat [HW4, 256] is laid out as gn_relu's layout 0 / 2 output; out (M + guard) x HW4 floats.
 * band_accumulate: sig [k, fh, fw], use [k] -> out 3 H W + guard bytes, inst k H W + guard bytes (NULL: not computed). */
int pb_op_mask_prep(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W, int nh, int nw, int Hp, int Wp, const int *xt, const int *yt, int split,
                    int guard_rows, void *out, float *chw);
int pb_op_mask_maxpool(pb_ctx *ctx, const float *x, int n, int H, int W, int C, int split, int guard_rows, void *out);
int pb_op_mask_nearest_add(pb_ctx *ctx, const float *dst, const float *src, int n, int h, int w, int sh, int sw, int C, int split, int guard_rows,
                           void *out);
int pb_op_mask_subsample2(pb_ctx *ctx, const float *x, int n, int H, int W, int C, int split, int guard_rows, void *out);
int pb_op_mask_coord_concat(pb_ctx *ctx, const float *x, int n, int h, int w, int C, int ldi, int split, int guard_rows, void *out);
int pb_op_mask_bilinear(pb_ctx *ctx, const float *x, const float *y0, int n, int H, int W, int OH, int OW, int C, int ldi, int ldo, int split,
                        int guard_rows, void *out);
int pb_op_mask_gn_relu(pb_ctx *ctx, const float *x, const float *gamma, const float *beta, int n, int HW, int C, int layout, int guard_rows, void *out,
                       float *aff);
int pb_op_mask_cls_points_nms(pb_ctx *ctx, const float *logit, int n, int pts_total, int off, int g, int C, int guard_rows, float *score);
int pb_op_mask_gather_rows(pb_ctx *ctx, const float *src, int src_rows, const int *idx, int count, int rows_pad, int cols, int split, int guard_rows,
                           void *out);
int pb_op_mask_stats(pb_ctx *ctx, const float *logit, int rows, int HW, int ld, float thr, int guard_rows, float *out);
int pb_op_mask_intersections(pb_ctx *ctx, const float *logit, int src_rows, int ld, const int *idx, int n, int HW, float thr, int guard_rows,
                             void *bits, int inter_rows, float *inter);
int pb_op_mask_matrix_nms(pb_ctx *ctx, const float *inter, const float *area, const int *label, const float *score, int n, float sigma, int guard,
                          float *comp, float *out);
int pb_op_mask_sigmoid_rows(pb_ctx *ctx, const float *logit, int src_rows, int ld, const int *idx, int count, int HW, int guard_rows, float *sig);
int pb_op_mask_dynconv(pb_ctx *ctx, const float *kernels, int src_rows, const int *idx, int row_off, int M, const float *feat, int HW4, int split,
                       int guard_rows, float *out);
int pb_op_mask_band_accumulate(pb_ctx *ctx, const float *sig, const uint8_t *use, int k, int fh, int fw, int h, int w, int H, int W, float thr,
                               int guard, uint8_t *out, uint8_t *inst);
/* The depth bands' own kernels one by one (tests/test_gpu_depth_ops.py): the launchers of kernels.h / zoe_kernels.h with arguments the caller chooses,
 * in the modes DepthEngine uses.  Inputs are float32 host arrays staged into the engine's layouts; every `out` is the RAW buffer, preset to 0xFF bytes,
 * with guard rows (or guard elements) behind the last row.
 * depth_layernorm: x [B, ntp, D] -> rows of ldy halfs, (B ntp + guard) of them, or with drop_cls (B (ntok - 1) + guard): output row b (ntok - 1) + t - 1
 *   holds token t.  lo_off: the rounding residual at half lo_off (lo8 = 0) or the e4m3 parts at bytes 2 lo_off / 3 lo_off (lo8 = 1, scale 2^*lo8_pa,
 *   the engine's); o8_off: e4m3(hi o8_scale) at byte o8_off of the row.
 * depth_attention: q, k, v [B, heads, N, 64] -> (B ntp + guard) rows of ldo halfs, ntp = N rounded up to 16; variant 1: the 8-wave kernel, 2: the 4-wave one.
 * depth_preprocess: frames u8 [n, H, W, 3] -> one launch of the pre-process kernel for all n frames with both outputs: chw [n, 3, net_h, net_w] float32
 *   and patch_raw, the fused 14 x 14 im2col: round_up(n P, 256) + guard_rows rows of 640 halfs (P = net_h / 14 x net_w / 14), row (b, gy, gx), column
 *   c 196 + py 14 + px.  mode 0: the relative band (pb_depth_net_size, cubic taps); 1: the metric band (392 x 518, align-corners bilinear taps); the
 *   tables are built by the engine's own functions, net_h / net_w must be the mode's.
 * depth_cls_rows: -> the residual stream (B ntp + guard) x D floats, of which only row 0 of every image is written.
 * depth_dpt_tail: z [B, H, W, 288] in pixels of ldz halfs, layout 0 [hi], 1 [hi | lo], 2 [hi | hi8 | lo8] (parts 320 wide) -> B OH OW + guard floats.
 * depth_resize_minmax: net [B, nh, nw] -> out B H W + guard floats, mnmx [B, 2] the decoded per-frame min / max.
 * zoe_softplus: x is the whole buffer [(rows + guard), ld], in and out.  zoe_dot32_relu / zoe_bilerp_add / zoe_cat: fp16 inputs in rows of the given
 *   strides.  zoe_attractor: A [n H W, ldA], bprev [n, h, w, 64] -> (n H W + guard) x 64 floats.  zoe_logbinom_depth: pt [n H W, ld_pt], bins [n, h, w, 64]
 *   -> n H W + guard floats.  zoe_pil_resize: in [n, h, w] -> n H W + guard floats; the tap tables are built by the engine's own functions. */
int pb_op_depth_layernorm(pb_ctx *ctx, const float *x, const float *g, const float *b, int B, int ntp, int ntok, int D, int drop_cls, int ldy, int lo_off,
                          int o8_off, float o8_scale, int lo8, int guard_rows, void *out, int *lo8_pa);
int pb_op_depth_attention(pb_ctx *ctx, const float *q, const float *k, const float *v, int B, int heads, int N, int variant, int ldo, int o8_off,
                          float o8_scale, int guard_rows, void *out);
int pb_op_depth_preprocess(pb_ctx *ctx, const uint8_t *frames, int n, int H, int W, int mode, int net_h, int net_w, int guard_rows, float *chw,
                           void *patch_raw);
int pb_op_depth_cls_rows(pb_ctx *ctx, const float *cls, const float *pos, int B, int ntp, int D, int guard_rows, float *out);
int pb_op_depth_dpt_tail(pb_ctx *ctx, const float *z, const float *bias, const float *w2, float b2, int B, int H, int W, int OH, int OW, int layout,
                         int ldz, int guard, float *out, int *lo8_pa);
int pb_op_depth_resize_minmax(pb_ctx *ctx, const float *net, int B, int nh, int nw, int H, int W, int guard, float *out, float *mnmx);
int pb_op_zoe_softplus(pb_ctx *ctx, float *x, int rows, int cols, int ld, int guard_rows);
int pb_op_zoe_dot32_relu(pb_ctx *ctx, const float *act, int ld, const float *w2, float b2, int rows, int guard, float *out);
int pb_op_zoe_bilerp_add(pb_ctx *ctx, const float *a, const float *src, int n, int h, int w, int H, int W, int C, int lda, int lds, int ldo,
                         int guard_rows, void *out);
int pb_op_zoe_attractor(pb_ctx *ctx, const float *A, int ldA, int nA, const float *bprev, int n, int h, int w, int H, int W, float alpha,
                        int guard_rows, float *out);
int pb_op_zoe_cat(pb_ctx *ctx, const float *act, int ld_act, const float *rel, const float *emb, int ld_emb, int n, int h, int w, int H, int W,
                  int guard_rows, void *out);
int pb_op_zoe_logbinom_depth(pb_ctx *ctx, const float *pt, int ld_pt, const float *bins, int n, int h, int w, int H, int W, float min_temp,
                             float max_temp, int guard, float *out);
int pb_op_zoe_pil_resize(pb_ctx *ctx, const float *in, int n, int h, int w, int H, int W, int guard, float *out);
/* bilinear resize NCHW float32, align_corners 0/1 (torch F.interpolate semantics). */
int pb_op_bilinear(pb_ctx *ctx, const float *x, float *y, int B, int C, int H, int W, int OH, int OW,
                   int align_corners);
/* uint8 frame -> normalised network input [3, net_h, net_w] float32
 * (bands/depth_anything.py:122-126). */
int pb_op_preprocess(pb_ctx *ctx, const uint8_t *frame, int H, int W, float *out, int net_h, int net_w);
/* float32 depth [n,H,W] -> heat RGB + min/max (bands/depth_anything.py:215-221). */
int pb_op_encode_depth(pb_ctx *ctx, const float *depth, int n, int H, int W, int flip,
                       uint8_t *rgb, float *mn, float *mx);

#ifdef __cplusplus
}
#endif
#endif /* PRISMA_BANDS_H */
