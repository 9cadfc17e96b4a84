// Launchers of the flow_gmflow band's non-GEMM kernels (gmflow_kernels.hip).
#pragma once
#include "common.h"
#include "../../include/prisma_bands.h"

// token grid of one frame and its ns x ns attention windows: the 1/8 grid with attn_splits = 2 (bands/flow_gmflow.py:237), and for the
// two-scale model's fine scale the 1/4 grid with attn_splits = 8 (the fields keep the coarse grid's names)
struct GmGeom {
    int h8, w8, P;          // grid, tokens per frame
    int wh, ww, Lw;         // window size, tokens per window
    int ldv;                // row stride of a window's V^T (round_up(Lw, 32))
    int ns;                 // windows per axis (window index of an image = wy * ns + wx)
};
struct GmPackJob {
    const float *src;       // fp32 projection matrix [frames * P, ld]
    int ld, col;            // ... and the first of the 128 columns to take
    f16 *dst;               // rows: [Bw, Lw, 256] = [hi | lo];  vt: [Bw, 2, 128, ldv]
    int is_vt;
};
struct GmPackJobs { GmPackJob j[5]; int n; };

// X[(n, e)] = feature + pos.  warped == nullptr: frames n, n + 1 of feat [NP + 1, P, 128].  Else (the fine scale: batch element n = pair * dirs +
// direction): e = 0 is frame n / dirs + n % dirs of feat, e = 1 is warped [NP, P, 128] (launch_gm_warp).
int launch_gm_tokens(hipStream_t s, const float *feat, const float *pos, float *X, f16 *Xs, int NP, int P, const float *warped = nullptr, int dirs = 1);
int launch_gm_split_rows(hipStream_t s, const float *src, int ld, int C, f16 *dst, int64_t rows);
int launch_gm_pack(hipStream_t s, const GmPackJobs &jobs, const GmGeom &g, int Bw, int shifted);
int launch_gm_ln(hipStream_t s, const float *M, const float *gamma, const float *beta, float *X, f16 *out, int64_t rows, const GmGeom &g,
                 int windowed, int shifted, int mode);
int launch_gm_grid_vt(hipStream_t s, f16 *vt, int P, int w8, int ldv);
int launch_gm_match_flow(hipStream_t s, const float *O, float *flow, f16 *vt, int B, int P, int w8, int ldv);
int launch_gm_upsampler_in(hipStream_t s, const float *O, const float *X, float *flow, f16 *map, int B, int P, int img_step);
// The step between the scales (gmflow.py:121-126, geometry.py:41-72): flow8 [B, h8 * w8, 2] -> flow_up [B, 4 h8 w8, 2] = 2 x its bilinear
// (align_corners) enlargement to the (2 h8) x (2 w8) grid, and warped [B, 4 h8 w8, 128] = feat4 [frames, 4 h8 w8, 128] of the TARGET frame of
// batch element b (b = pair * dirs + d: frame pair + 1 - d) sampled bilinearly (align_corners, zeros outside) at token + flow_up
int launch_gm_warp(hipStream_t s, const float *flow8, const float *feat4, float *flow_up, float *warped, int B, int dirs, int h8, int w8);
// out = a + b over n flows of 2: the fine scale's flow = enlarged flow + matched residual (gmflow.py:145), the local propagation's input
int launch_gm_flow_add(hipStream_t s, const float *a, const float *b, float *out, int64_t n);

// gmflow_local.hip: the local forms of matching and propagation over fp32 token maps [images, P, 128]; batch element b reads image b * img_step.
// Matching (radius 1 .. 4): the target is the other image of the pair (index ^ 1); flow [B, P, 2], and with vt != nullptr the global
// propagation's V^T as launch_gm_match_flow writes it.  Propagation (radius 1 .. 2): writes columns 0, 1 of O [B, P, 32] (launch_gm_upsampler_in's input).
int launch_gm_local_match(hipStream_t s, const float *X, float *flow, f16 *vt, int B, int h8, int w8, int img_step, int radius, int ldv);
int launch_gm_local_prop(hipStream_t s, const float *q, const float *k, const float *flow_in, float *O, int B, int h8, int w8, int img_step,
                         int radius);
