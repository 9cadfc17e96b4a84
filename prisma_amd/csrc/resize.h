// resize.hip: bilinear resize of packed RGB frames, 8 bit, exact integers, optionally straight into I420 (the formulas are at the top of
// resize.hip and in include/prisma_bands.h, pb_rgb_resize).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// n packed [sh, sw, 3] RGB frames -> n packed [H, W, 3] RGB frames, or with out_i420 n packed I420 frames of H x W (i420_frame_bytes(H, W)
// each: the bytes of launch_rgb_to_i420 on the resized frames, which never exist in memory), on stream s.  No alignment is needed; with
// W % 16 == 0 and `out` 16-byte aligned the kernels store 16 bytes per access.  Refuses sizes whose tap arithmetic would leave int32.
int launch_rgb_resize(hipStream_t s, const uint8_t *rgb, int n, int sh, int sw, int H, int W, uint8_t *out, bool out_i420);
