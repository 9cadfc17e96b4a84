// RGB -> planar YUV of any .y4m layout, the way out: 4:0:0 / 4:2:0 / 4:2:2 / 4:4:4, 8 .. 16 bit, limited / full range, BT.601 / BT.709, exact integers
// (include/prisma_bands.h pb_rgb_to_yuv states the rule; bands/common/yuv.py rgb_to_yuv is the host's form of it and tests/yuv_out_ref.py pins both):
//   Y  = clamp((( yr R + yg G + yb B + rnd) >> F) + yoff) per pixel
//   Cb = clamp(((-ur R - ug G + h  B + rnd) >> F) + coff), Cr = clamp((( h R - vg G - vb B + rnd) >> F) + coff) per chroma sample, of the rounded mean
//   colour of the 2^sx x 2^sy pixels it covers ((sum + half the count) >> (sx + sy), pixel indices clamped to the frame); rnd = 2^(F - 1), clamp to 0 .. 2^d - 1.
// A sample is a byte at d = 8, else a 16-bit little-endian word.  The coefficients are rounded once on the host, from exact rationals in int64
// (coeffs_of); they, the offsets and F are kernel arguments: uniform, so they sit in SGPRs.  Every product sum stays inside int32.
// A frame is H W samples of Y, ceil(H / 2^sy) ceil(W / 2^sx) of Cb, as many of Cr; frames are packed, as are the [H, W, 3] RGB frames.
// The kernels are yuv_formats.hip's shape, mirrored.  HBM-bound: 3 bytes of RGB in per pixel for 1 (8-bit mono) to 6 (16-bit 4:4:4) out.  Where
// W % 16 == 0 and both arrays are 16-byte aligned - then every RGB row, luma row and chroma run of every frame is aligned to its access - a lane
// owns a run of 16 pixels over 2^sy rows: 48 RGB bytes per row as three 16-byte loads, the row's 16 luma samples packed in registers and stored
// as one 16-byte access (two for 16-bit samples - never a 2-byte store per lane), the colour sums of the 16 >> sx chroma samples under the run
// kept across the rows and each plane's samples stored as 16-byte accesses too (one 8-byte store per plane for 8-bit 4:2:0 / 4:2:2).  Every
// other width or alignment takes one chroma sample's 2^sx x 2^sy pixels per lane with byte accesses (a 16-bit sample as two: the array may start
// at an odd address).  No lane reads or writes outside the planes of its frame; all stores are plain vector stores.
// {4:2:0, 8 bit, limited, BT.601} is not served here: launch_rgb_to_yuv hands it to yuv.hip's rgb_to_i420 kernels, whose constants are literals.
#include "common.h"
#include "yuv.h"

namespace {

struct Fwd { int yr, yg, yb, ur, ug, h, vg, vb, F, yoff, coff, top; };

using Layout = YuvLayout;

__device__ __forceinline__ int clampd(int v, int top) { return min(max(v, 0), top); }
__device__ __forceinline__ int y_of(const Fwd &k, int r, int g, int b) {
    return clampd(((k.yr * r + k.yg * g + k.yb * b + (1 << (k.F - 1))) >> k.F) + k.yoff, k.top);
}
__device__ __forceinline__ int cb_of(const Fwd &k, int r, int g, int b) {
    return clampd(((k.h * b - k.ur * r - k.ug * g + (1 << (k.F - 1))) >> k.F) + k.coff, k.top);
}
__device__ __forceinline__ int cr_of(const Fwd &k, int r, int g, int b) {
    return clampd(((k.h * r - k.vg * g - k.vb * b + (1 << (k.F - 1))) >> k.F) + k.coff, k.top);
}

// sample v (within d bits) into place i of a run held in 32-bit words that start as zero
template <int BPS>
__device__ __forceinline__ void put_sample(unsigned *w, int i, int v) {
    if (BPS == 1) w[i >> 2] |= (unsigned)v << (8 * (i & 3));
    else w[i >> 1] |= (unsigned)v << (16 * (i & 1));
}

// sample v to place i of a plane, byte by byte
template <int BPS>
__device__ __forceinline__ void store_sample(uint8_t *p, size_t i, int v) {
    if (BPS == 1) p[i] = (uint8_t)v;
    else { p[2 * i] = (uint8_t)(v & 255); p[2 * i + 1] = (uint8_t)(v >> 8); }
}

// WORDS 32-bit words to an address aligned to 4 WORDS bytes (8 for two words, else 16)
template <int WORDS>
__device__ __forceinline__ void store_words(uint8_t *p, const unsigned *w) {
    if (WORDS == 2) {
        *(uint2 *)p = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
        for (int q = 0; q < WORDS / 4; ++q) ((uint4 *)p)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
}

__device__ __forceinline__ int byte_of(const unsigned *w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// ---- 16-byte path: W % 16 == 0, lane = (frame, chroma row by, group of 16 luma columns gx) ----------------------------------------------------
template <int BPS, int SX, int SY, bool MONO>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const uint8_t *__restrict__ rgb, int H, int W, int64_t lanes, Fwd k,
                                                         uint8_t *__restrict__ yuv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Layout fr(H, W, BPS, SX, SY, MONO);
    const int groups = W / 16;
    const int gx = (int)(t % groups);
    const int64_t r = t / groups;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    uint8_t *dst = yuv + f * fr.bytes;
    constexpr int NC = 16 >> SX, CWORDS = NC * BPS / 4;      // chroma samples per plane under the run, and their words
    const int rows = min(1 << SY, H - (by << SY));          // an odd H of a 4:2:0 frame: the last chroma row has one luma row
    int sum[MONO ? 1 : NC][3] = {};                          // colour sums of the pixels each chroma sample covers
    for (int dy = 0; dy < (1 << SY); ++dy) {
        const size_t y = ((size_t)by << SY) + (dy < rows ? dy : 0);      // the clamped row of an odd H: the block's first row again
        const uint4 *src = (const uint4 *)(rgb + ((f * H + y) * W + (size_t)gx * 16) * 3);
        const uint4 a = src[0], b = src[1], c = src[2];
        const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        unsigned yo[4 * BPS] = {};
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int rr = byte_of(w, 3 * p), gg = byte_of(w, 3 * p + 1), bb = byte_of(w, 3 * p + 2);
            put_sample<BPS>(yo, p, y_of(k, rr, gg, bb));
            if constexpr (!MONO) { sum[p >> SX][0] += rr; sum[p >> SX][1] += gg; sum[p >> SX][2] += bb; }
        }
        if (dy < rows) store_words<4 * BPS>(dst + (y * W + (size_t)gx * 16) * BPS, yo);
    }
    if constexpr (!MONO) {
        constexpr int SH = SX + SY, HALF = (1 << SH) >> 1;     // a sample covers 2^SH pixels; the mean rounds half up
        unsigned cbo[CWORDS] = {}, cro[CWORDS] = {};
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int rr = (sum[i][0] + HALF) >> SH, gg = (sum[i][1] + HALF) >> SH, bb = (sum[i][2] + HALF) >> SH;
            put_sample<BPS>(cbo, i, cb_of(k, rr, gg, bb));
            put_sample<BPS>(cro, i, cr_of(k, rr, gg, bb));
        }
        const size_t at = fr.luma + ((size_t)by * fr.cw + (size_t)gx * NC) * BPS;
        store_words<CWORDS>(dst + at, cbo);
        store_words<CWORDS>(dst + at + fr.chroma, cro);
    }
}

// ---- byte path: any size and alignment, lane = (frame, chroma row by, chroma column bx) -------------------------------------------------------
template <int BPS, int SX, int SY, bool MONO>
__global__ __launch_bounds__(256) void rgb_to_yuv_block_kernel(const uint8_t *__restrict__ rgb, int H, int W, int64_t lanes, Fwd k,
                                                               uint8_t *__restrict__ yuv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Layout fr(H, W, BPS, SX, SY, MONO);
    const int bx = (int)(t % fr.cw);
    const int64_t r = t / fr.cw;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    uint8_t *dst = yuv + f * fr.bytes;
    int sr = 0, sg = 0, sb = 0;
    for (int dy = 0; dy < (1 << SY); ++dy)
        for (int dx = 0; dx < (1 << SX); ++dx) {
            const int y = min((by << SY) + dy, H - 1), x = min((bx << SX) + dx, W - 1);          // clamped: the last row / column again
            const uint8_t *p = rgb + ((f * H + y) * W + x) * 3;
            const int rr = p[0], gg = p[1], bb = p[2];
            sr += rr; sg += gg; sb += bb;
            if ((by << SY) + dy < H && (bx << SX) + dx < W) store_sample<BPS>(dst, (size_t)y * W + x, y_of(k, rr, gg, bb));
        }
    if (MONO) return;
    constexpr int SH = SX + SY, HALF = (1 << SH) >> 1;
    sr = (sr + HALF) >> SH; sg = (sg + HALF) >> SH; sb = (sb + HALF) >> SH;
    const size_t at = (size_t)by * fr.cw + bx;
    store_sample<BPS>(dst + fr.luma, at, cb_of(k, sr, sg, sb));
    store_sample<BPS>(dst + fr.luma + fr.chroma, at, cr_of(k, sr, sg, sb));
}

template <int BPS, int SX, int SY, bool MONO>
int launch(hipStream_t s, const Fwd &k, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv) {
    const bool wide = W % 16 == 0 && (((uintptr_t)yuv | (uintptr_t)rgb) & 15) == 0;
    const Layout fr(H, W, BPS, SX, SY, MONO);
    const int64_t lanes = (int64_t)n * fr.ch * (wide ? W / 16 : fr.cw), blocks = (lanes + 255) / 256;
    PB_CHECK(blocks <= 0x7fffffff, -1, "rgb_to_yuv: %d frames of %d x %d exceed the launch grid", n, H, W);
    if (wide) hipLaunchKernelGGL((rgb_to_yuv_kernel<BPS, SX, SY, MONO>), dim3((unsigned)blocks), dim3(256), 0, s, rgb, H, W, lanes, k, yuv);
    else hipLaunchKernelGGL((rgb_to_yuv_block_kernel<BPS, SX, SY, MONO>), dim3((unsigned)blocks), dim3(256), 0, s, rgb, H, W, lanes, k, yuv);
    PB_HIP(hipGetLastError());
    return 0;
}

template <int BPS>
int launch_layout(int chroma, hipStream_t s, const Fwd &k, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv) {
    switch (chroma) {
        case 400: return launch<BPS, 0, 0, true>(s, k, rgb, n, H, W, yuv);
        case 420: return launch<BPS, 1, 1, false>(s, k, rgb, n, H, W, yuv);
        case 422: return launch<BPS, 1, 0, false>(s, k, rgb, n, H, W, yuv);
        default: return launch<BPS, 0, 0, false>(s, k, rgb, n, H, W, yuv);
    }
}

int64_t rhu(int64_t p, int64_t q) { return (2 * p + q) / (2 * q); }      // round half up of p / q, both positive

// the table of a good format, from exact rationals: Kr = kr / den ..., 2^F ys = yn / 255, 2^F cs = cn / 255 (the largest product is below 2^48)
Fwd coeffs_of(const pb_yuv_fmt &f) {
    const int d = f.depth;
    const int64_t den = f.matrix == PB_YUV_BT709 ? 10000 : 1000, kr = f.matrix == PB_YUV_BT709 ? 2126 : 299,
                  kb = f.matrix == PB_YUV_BT709 ? 722 : 114;
    const int F = d == 8 && !f.full_range && f.matrix == PB_YUV_BT601 ? 8 : 24 - d;      // the one exception: the published 8-bit integers
    const int64_t top = ((int64_t)1 << d) - 1;
    const int64_t yn = (f.full_range ? top : (int64_t)219 << (d - 8)) << F, cn = (f.full_range ? top : (int64_t)224 << (d - 8)) << F;
    Fwd k;
    k.yr = (int)rhu(yn * kr, 255 * den);
    k.yb = (int)rhu(yn * kb, 255 * den);
    k.yg = (int)rhu(yn, 255) - k.yr - k.yb;
    k.h = (int)rhu(cn, 255 * 2);
    k.ur = (int)rhu(cn * kr, 255 * 2 * (den - kb));
    k.ug = k.h - k.ur;
    k.vb = (int)rhu(cn * kb, 255 * 2 * (den - kr));
    k.vg = k.h - k.vb;
    k.F = F;
    k.yoff = f.full_range ? 0 : 16 << (d - 8);
    k.coff = 1 << (d - 1);
    k.top = (int)top;
    return k;
}

}  // namespace

void yuv_fwd_coeffs(const pb_yuv_fmt &f, int32_t out[12]) {
    const Fwd k = coeffs_of(f);
    const int32_t v[12] = {k.yr, k.yg, k.yb, k.ur, k.ug, k.h, k.vg, k.vb, k.F, k.yoff, k.coff, k.top};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}

int launch_rgb_to_yuv(hipStream_t s, const pb_yuv_fmt &f, const uint8_t *rgb, int n, int H, int W, uint8_t *yuv) {
    PB_CHECK(yuv_fmt_ok(f), -1, "rgb_to_yuv: no such format (chroma %d, depth %d, full_range %d, matrix %d)", f.chroma, f.depth, f.full_range, f.matrix);
    PB_CHECK(yuv && rgb && n > 0 && H > 0 && W > 0, -1, "rgb_to_yuv: bad arguments (n %d, %d x %d)", n, H, W);
    if (yuv_fmt_is_i420(f)) return launch_rgb_to_i420(s, rgb, n, H, W, yuv);
    const Fwd k = coeffs_of(f);
    return f.depth > 8 ? launch_layout<2>(f.chroma, s, k, rgb, n, H, W, yuv) : launch_layout<1>(f.chroma, s, k, rgb, n, H, W, yuv);
}
