// yuv.hip: I420 <-> RGB, 8 bit, BT.601 limited range, exact integers (the formulas are at the top of yuv.hip and in include/prisma_bands.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prisma_bands.h"

// bytes of one I420 frame: H W of Y + 2 ceil(H / 2) ceil(W / 2) of Cb and Cr (0 for a size that is not positive)
int64_t i420_frame_bytes(int H, int W);
// n packed I420 frames -> n packed [H, W, 3] RGB frames and back, on stream s.  No alignment is needed; with W % 16 == 0 and both pointers
// 16-byte aligned the kernels move 16 bytes per access.
int launch_i420_to_rgb(hipStream_t s, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb);
int launch_rgb_to_i420(hipStream_t s, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv);

// yuv_formats.hip: every planar layout of a .y4m to RGB - 4:0:0 / 4:2:0 / 4:2:2 / 4:4:4, 8 .. 16 bit, limited / full range, BT.601 / BT.709
// (include/prisma_bands.h pb_yuv_fmt has every formula).  {420, 8, limited, BT.601} runs launch_i420_to_rgb.
bool yuv_fmt_ok(const pb_yuv_fmt &f);
bool yuv_fmt_is_i420(const pb_yuv_fmt &f);
int64_t yuv_frame_bytes(const pb_yuv_fmt &f, int H, int W);       // 0 for a bad format or a size that is not positive
void yuv_coeffs(const pb_yuv_fmt &f, int32_t out[7]);             // cy, crv, cgu, cgv, cbu, yoff, coff of a good format
int launch_yuv_to_rgb(hipStream_t s, const pb_yuv_fmt &f, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb);

// yuv_out.hip: RGB to every one of those layouts, the way out (include/prisma_bands.h pb_rgb_to_yuv has the rule).  {420, 8, limited, BT.601} runs
// launch_rgb_to_i420.
void yuv_fwd_coeffs(const pb_yuv_fmt &f, int32_t out[12]);        // yr, yg, yb, ur, ug, h, vg, vb, F, yoff, coff, 2^d - 1 of a good format
int launch_rgb_to_yuv(hipStream_t s, const pb_yuv_fmt &f, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv);

// ---- what the kernels of yuv_formats.hip and yuv_out.hip share ------------------------------------------------------------------------------------
struct YuvLayout {  // plane geometry of one frame: samples of BPS bytes, chroma planes subsampled by 2^SX x 2^SY (none with MONO)
    int ch, cw;
    size_t luma, chroma, bytes;
    __host__ __device__ YuvLayout(int H, int W, int bps, int sx, int sy, bool mono)
        : ch((H + (1 << sy) - 1) >> sy), cw((W + (1 << sx) - 1) >> sx) {
        luma = (size_t)H * W * bps;
        chroma = mono ? 0 : (size_t)ch * cw * bps;
        bytes = luma + 2 * chroma;
    }
};

// ---- what the kernels of yuv.hip and resize.hip share -------------------------------------------------------------------------------------------
struct I420Frame {  // plane geometry of one I420 frame
    int H, W, ch, cw;
    size_t luma, chroma, bytes;
    __host__ __device__ I420Frame(int h, int w) : H(h), W(w), ch((h + 1) / 2), cw((w + 1) / 2) {
        luma = (size_t)H * W;
        chroma = (size_t)ch * cw;
        bytes = luma + 2 * chroma;
    }
};

// The empty asm keeps the `>> 8` of its argument and the clamp apart.  Left together, hipcc 7 fuses pairs of them into v_ashr_pk_u8_i32 (shift,
// saturate to u8, pack two) and ORs the result into the output word as if its bits 16 .. 31 were zero; on the MI355X they were not, and the two
// bytes above such a pair came out as 255 wherever one of the pair's values had been negative (tests/test_gpu_yuv.py, 16 x 64).
__device__ __forceinline__ unsigned clip8(int v) {
    asm volatile("" : "+v"(v));
    return (unsigned)min(max(v, 0), 255);
}

__device__ __forceinline__ unsigned luma_of(int r, int g, int b) { return (unsigned)(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16); }
__device__ __forceinline__ unsigned cb_of(int r, int g, int b) { return (unsigned)(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128); }
__device__ __forceinline__ unsigned cr_of(int r, int g, int b) { return (unsigned)(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128); }
