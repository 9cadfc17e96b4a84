// I420 <-> RGB, 8 bit, BT.601 limited range, exact integers (include/prisma_bands.h pb_i420_to_rgb / pb_rgb_to_i420; the host states the same
// arithmetic in bands/common/yuv.py and tests/yuv_ref.py pins both):
//   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 per pixel; Cb = ((-38 R - 74 G + 112 B + 128) >> 8) + 128 and Cr = ((112 R - 94 G - 18 B + 128) >> 8) + 128
//   per 2 x 2 block of the block's rounded mean colour ((sum of 4 + 2) >> 2, pixel indices clamped to the frame);
//   R = clip8((298 C + 409 E + 128) >> 8), G = clip8((298 C - 100 D - 208 E + 128) >> 8), B = clip8((298 C + 516 D + 128) >> 8) with C = Y - 16,
//   D = Cb - 128, E = Cr - 128 of the pixel's block (nearest).  `>>` on int is arithmetic on this target (floor).
// A frame is H W bytes of Y, ceil(H / 2) ceil(W / 2) of Cb, as many of Cr; frames are packed, as are the [H, W, 3] RGB frames.
// Both kernels are HBM-bound, 4.5 bytes per pixel.  A lane owns whole 2 x 2 blocks.  Where W % 16 == 0 and both arrays are 16-byte aligned (then
// every luma row, RGB row and 8-block chroma run of every frame is aligned too) a lane takes 8 blocks: 16 luma bytes of each of its two rows as one
// 16-byte access each, their 48 RGB bytes as three, their 8 + 8 chroma bytes as two 8-byte ones.  Every other width takes one block per lane with
// byte accesses and clamped indices.  No lane reads or writes outside the planes of its frame.
#include "common.h"
#include "yuv.h"

namespace {

// one pixel's three output bytes, each in a word of its own
__device__ __forceinline__ void rgb_of(unsigned y, unsigned cb, unsigned cr, unsigned &r, unsigned &g, unsigned &b) {
    const int c = 298 * ((int)y - 16) + 128, d = (int)cb - 128, e = (int)cr - 128;
    r = clip8((c + 409 * e) >> 8);
    g = clip8((c - 100 * d - 208 * e) >> 8);
    b = clip8((c + 516 * d) >> 8);
}

__device__ __forceinline__ unsigned byte_of(const unsigned *w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

using Frame = I420Frame;

// ---- 16-byte paths: W % 16 == 0, lane = (frame, block row by, group of 8 blocks gx) ------------------------------------------------------------
__global__ __launch_bounds__(256) void i420_to_rgb_kernel(const uint8_t *__restrict__ yuv, int H, int W, int64_t lanes, uint8_t *__restrict__ rgb) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Frame fr(H, W);
    const int groups = W / 16;
    const int gx = (int)(t % groups);
    const int64_t r = t / groups;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    const uint8_t *src = yuv + f * fr.bytes;
    const uint2 cb = *(const uint2 *)(src + fr.luma + (size_t)by * fr.cw + gx * 8);
    const uint2 cr = *(const uint2 *)(src + fr.luma + fr.chroma + (size_t)by * fr.cw + gx * 8);
    const unsigned cbw[2] = {cb.x, cb.y}, crw[2] = {cr.x, cr.y};
    const int rows = 2 * by + 1 < H ? 2 : 1;                // an odd H: the last block row is one pixel high
    for (int dy = 0; dy < rows; ++dy) {
        const size_t y = (size_t)2 * by + dy;
        const uint4 yv = *(const uint4 *)(src + y * W + gx * 16);
        const unsigned yw[4] = {yv.x, yv.y, yv.z, yv.w};
        unsigned o[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                        // four pixels = twelve bytes = three words, every byte placed once and whole
            unsigned r[4], g[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = 4 * q + k;
                rgb_of(byte_of(yw, p), byte_of(cbw, p >> 1), byte_of(crw, p >> 1), r[k], g[k], b[k]);
            }
            o[3 * q] = r[0] | g[0] << 8 | b[0] << 16 | r[1] << 24;
            o[3 * q + 1] = g[1] | b[1] << 8 | r[2] << 16 | g[2] << 24;
            o[3 * q + 2] = b[2] | r[3] << 8 | g[3] << 16 | b[3] << 24;
        }
        uint4 *dst = (uint4 *)(rgb + ((f * H + y) * W + (size_t)gx * 16) * 3);
        dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
        dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
        dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
    }
}

__global__ __launch_bounds__(256) void rgb_to_i420_kernel(const uint8_t *__restrict__ rgb, int H, int W, int64_t lanes, uint8_t *__restrict__ yuv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Frame fr(H, W);
    const int groups = W / 16;
    const int gx = (int)(t % groups);
    const int64_t r = t / groups;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    uint8_t *dst = yuv + f * fr.bytes;
    const int rows = 2 * by + 1 < H ? 2 : 1;
    int sum[8][3] = {};                                      // colour sums of the lane's 8 blocks
    for (int dy = 0; dy < 2; ++dy) {
        const size_t y = (size_t)2 * by + (dy < rows ? dy : 0);           // the clamped row of an odd H: the block's first row again
        const uint4 *src = (const uint4 *)(rgb + ((f * H + y) * W + (size_t)gx * 16) * 3);
        const uint4 a = src[0], b = src[1], c = src[2];
        const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        unsigned yo[4] = {};
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int rr = (int)byte_of(w, 3 * p), gg = (int)byte_of(w, 3 * p + 1), bb = (int)byte_of(w, 3 * p + 2);
            yo[p >> 2] |= luma_of(rr, gg, bb) << (8 * (p & 3));
            sum[p >> 1][0] += rr; sum[p >> 1][1] += gg; sum[p >> 1][2] += bb;
        }
        if (dy < rows) *(uint4 *)(dst + y * W + gx * 16) = make_uint4(yo[0], yo[1], yo[2], yo[3]);
    }
    unsigned cbo[2] = {}, cro[2] = {};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int rr = (sum[k][0] + 2) >> 2, gg = (sum[k][1] + 2) >> 2, bb = (sum[k][2] + 2) >> 2;
        cbo[k >> 2] |= cb_of(rr, gg, bb) << (8 * (k & 3));
        cro[k >> 2] |= cr_of(rr, gg, bb) << (8 * (k & 3));
    }
    *(uint2 *)(dst + fr.luma + (size_t)by * fr.cw + gx * 8) = make_uint2(cbo[0], cbo[1]);
    *(uint2 *)(dst + fr.luma + fr.chroma + (size_t)by * fr.cw + gx * 8) = make_uint2(cro[0], cro[1]);
}

// ---- byte paths: any size, lane = (frame, block row by, block column bx) --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void i420_to_rgb_block_kernel(const uint8_t *__restrict__ yuv, int H, int W, int64_t lanes, uint8_t *__restrict__ rgb) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Frame fr(H, W);
    const int bx = (int)(t % fr.cw);
    const int64_t r = t / fr.cw;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    const uint8_t *src = yuv + f * fr.bytes;
    const unsigned cb = src[fr.luma + (size_t)by * fr.cw + bx], cr = src[fr.luma + fr.chroma + (size_t)by * fr.cw + bx];
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int y = 2 * by + dy, x = 2 * bx + dx;
            if (y >= H || x >= W) continue;
            unsigned r8, g8, b8;
            rgb_of(src[(size_t)y * W + x], cb, cr, r8, g8, b8);
            uint8_t *o = rgb + ((f * H + y) * W + x) * 3;
            o[0] = (uint8_t)r8; o[1] = (uint8_t)g8; o[2] = (uint8_t)b8;
        }
}

__global__ __launch_bounds__(256) void rgb_to_i420_block_kernel(const uint8_t *__restrict__ rgb, int H, int W, int64_t lanes, uint8_t *__restrict__ yuv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Frame fr(H, W);
    const int bx = (int)(t % fr.cw);
    const int64_t r = t / fr.cw;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    uint8_t *dst = yuv + f * fr.bytes;
    int sr = 0, sg = 0, sb = 0;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int y = min(2 * by + dy, H - 1), x = min(2 * bx + dx, W - 1);         // clamped: the last row / column again
            const uint8_t *p = rgb + ((f * H + y) * W + x) * 3;
            const int rr = p[0], gg = p[1], bb = p[2];
            sr += rr; sg += gg; sb += bb;
            if (2 * by + dy < H && 2 * bx + dx < W) dst[(size_t)y * W + x] = (uint8_t)luma_of(rr, gg, bb);
        }
    sr = (sr + 2) >> 2; sg = (sg + 2) >> 2; sb = (sb + 2) >> 2;
    dst[fr.luma + (size_t)by * fr.cw + bx] = (uint8_t)cb_of(sr, sg, sb);
    dst[fr.luma + fr.chroma + (size_t)by * fr.cw + bx] = (uint8_t)cr_of(sr, sg, sb);
}

bool wide(int W, const void *a, const void *b) { return W % 16 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

template <class K>
int launch(K kernel, const char *what, hipStream_t s, const uint8_t *in, int n, int H, int W, int per_row, uint8_t *out) {
    PB_CHECK(in && out && n > 0 && H > 0 && W > 0, -1, "%s: bad arguments (n %d, %d x %d)", what, n, H, W);
    const int64_t lanes = (int64_t)n * ((H + 1) / 2) * per_row, blocks = (lanes + 255) / 256;
    PB_CHECK(blocks <= 0x7fffffff, -1, "%s: %d frames of %d x %d exceed the launch grid", what, n, H, W);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, H, W, lanes, out);
    PB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int64_t i420_frame_bytes(int H, int W) { return H > 0 && W > 0 ? (int64_t)Frame(H, W).bytes : 0; }

int launch_i420_to_rgb(hipStream_t s, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb) {
    if (wide(W, yuv, rgb)) return launch(i420_to_rgb_kernel, "i420_to_rgb", s, yuv, n, H, W, W / 16, rgb);
    return launch(i420_to_rgb_block_kernel, "i420_to_rgb", s, yuv, n, H, W, (W + 1) / 2, rgb);
}

int launch_rgb_to_i420(hipStream_t s, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv) {
    if (wide(W, rgb, yuv)) return launch(rgb_to_i420_kernel, "rgb_to_i420", s, rgb, n, H, W, W / 16, yuv);
    return launch(rgb_to_i420_block_kernel, "rgb_to_i420", s, rgb, n, H, W, (W + 1) / 2, yuv);
}
