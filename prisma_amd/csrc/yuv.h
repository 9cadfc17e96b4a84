// yuv.hip: I420 <-> RGB, 8 bit, BT.601 limited range, exact integers (the formulas are at the top of yuv.hip and in include/prisma_bands.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// bytes of one I420 frame: H W of Y + 2 ceil(H / 2) ceil(W / 2) of Cb and Cr (0 for a size that is not positive)
int64_t i420_frame_bytes(int H, int W);
// n packed I420 frames -> n packed [H, W, 3] RGB frames and back, on stream s.  No alignment is needed; with W % 16 == 0 and both pointers
// 16-byte aligned the kernels move 16 bytes per access.
int launch_i420_to_rgb(hipStream_t s, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb);
int launch_rgb_to_i420(hipStream_t s, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv);
