// jpeg.hip: baseline JPEG frames (Motion JPEG) out of planar full-range BT.601 YUV, exact integers (include/prisma_bands.h pb_jpeg_encode has the
// rule; tests/jpeg_ref.py restates it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prisma_bands.h"

// device buffers of the encoder, kept for the life of a ctx: the kernels' workspace and the slots of the host-pointer pipeline
struct JpegState {
    void *ws = nullptr;                 // coefficients, bit offsets, the unstuffed stream, byte counts (jpeg_encode_dev carves it up)
    size_t ws_cap = 0;
    void *d_in[2] = {}, *d_out[2] = {}; // pb_jpeg_encode: the planes and the streams of a chunk, two slots
    size_t in_cap = 0, out_cap = 0;
    int64_t *d_offs[2] = {}, *h_offs[2] = {};   // a chunk's offsets on the device and in page-locked host memory
    int offs_cap = 0;
    int grow_host(size_t in_bytes, size_t out_bytes, int frames);
    void release();
};

bool jpeg_cfg_ok(const pb_jpeg_cfg &cfg);
// worst-case bytes of one frame, 0 for a size outside 1 .. 65535 or a bad cfg
int64_t jpeg_frame_bound(const pb_jpeg_cfg &cfg, int H, int W);
// n frames of planes -> their streams back to back in out[0 .. capacity), offsets[0 .. n] (device memory) their starts and the bytes needed; a frame
// whose end lies past capacity is not written.  Asynchronous on stream s; grows st.ws (synchronising s) when the call needs more than it holds.
int jpeg_encode_dev(JpegState &st, hipStream_t s, const pb_jpeg_cfg &cfg, const uint8_t *planes, int n, int H, int W, uint8_t *out, int64_t capacity,
                    int64_t *offsets);
