// Planar YUV of any .y4m layout -> RGB: 4:0:0 / 4:2:0 / 4:2:2 / 4:4:4, 8 .. 16 bit, limited / full range, BT.601 / BT.709, exact integers
// (include/prisma_bands.h pb_yuv_fmt states the rule; bands/common/yuv.py is the host's form of it and tests/yuv_fmt_ref.py pins both):
//   C = Y - yoff, D = Cb - coff, E = Cr - coff with the chroma samples plane[y >> sy][x >> sx] (nearest; D = E = 0 for 4:0:0)
//   R = clip8((cy C + crv E + half) >> d), G = clip8((cy C - cgu D - cgv E + half) >> d), B = clip8((cy C + cbu D + half) >> d)
// A sample is a byte at d = 8, else a 16-bit little-endian word that is read whole.  The coefficients are rounded once on the host, from exact
// rationals in int64 (coeffs_of); they, the offsets and d are kernel arguments: uniform, so they sit in SGPRs.
// A frame is H W samples of Y, ceil(H / 2^sy) ceil(W / 2^sx) of Cb, as many of Cr; frames are packed, as are the [H, W, 3] RGB frames.
// The kernels are yuv.hip's shape.  HBM-bound: 3 bytes of RGB out per pixel for 1 (8-bit mono) to 6 (16-bit 4:4:4) in.  Where W % 16 == 0 and both
// arrays are 16-byte aligned - then every luma row, RGB row and chroma run of every frame is aligned to its access - a lane owns a run of 16
// luma samples over 2^sy rows and the 16 >> sx chroma samples of each plane under them: 16-byte loads (one 8-byte load per plane for 8-bit
// 4:2:0 / 4:2:2), the chroma terms of the three channels computed once and used by every pixel above them, 48 RGB bytes per row as three 16-byte
// stores.  Every other width or alignment takes one chroma sample's 2^sx x 2^sy pixels per lane with byte accesses (a 16-bit sample as two: the
// array may start at an odd address).  No lane reads or writes outside the planes of its frame; all stores are plain vector stores.
// {4:2:0, 8 bit, limited, BT.601} is not served here: launch_yuv_to_rgb hands it to yuv.hip's i420_to_rgb kernels, whose constants are literals.
#include "common.h"
#include "yuv.h"

namespace {

struct Coeffs { int cy, crv, cgu, cgv, cbu, yoff, coff, half, d; };

using Layout = YuvLayout;

// sample i of a run held in 32-bit words
template <int BPS>
__device__ __forceinline__ int sample_of(const unsigned *w, int i) {
    return BPS == 1 ? (int)((w[i >> 2] >> (8 * (i & 3))) & 255u) : (int)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
}

// sample i of a plane, byte by byte
template <int BPS>
__device__ __forceinline__ int sample_at(const uint8_t *p, size_t i) {
    return BPS == 1 ? (int)p[i] : (int)p[2 * i] | (int)p[2 * i + 1] << 8;
}

// WORDS 32-bit words from an address aligned to 4 WORDS bytes (8 for two words, else 16)
template <int WORDS>
__device__ __forceinline__ void load_words(const uint8_t *p, unsigned *w) {
    if (WORDS == 2) {
        const uint2 v = *(const uint2 *)p;
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int q = 0; q < WORDS / 4; ++q) {
            const uint4 v = ((const uint4 *)p)[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    }
}

// ---- 16-byte path: W % 16 == 0, lane = (frame, chroma row by, group of 16 luma columns gx) ----------------------------------------------------
template <int BPS, int SX, int SY, bool MONO>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const uint8_t *__restrict__ yuv, int H, int W, int64_t lanes, Coeffs k,
                                                         uint8_t *__restrict__ rgb) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Layout fr(H, W, BPS, SX, SY, MONO);
    const int groups = W / 16;
    const int gx = (int)(t % groups);
    const int64_t r = t / groups;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    const uint8_t *src = yuv + f * fr.bytes;
    constexpr int NC = 16 >> SX, CWORDS = NC * BPS / 4;      // chroma samples per plane under the run, and their words
    int rv[NC], gv[NC], bv[NC];                             // the chroma terms of R, G, B with the rounding half in them
    if (MONO) {
#pragma unroll
        for (int i = 0; i < NC; ++i) rv[i] = gv[i] = bv[i] = k.half;
    } else {
        unsigned cbw[CWORDS], crw[CWORDS];
        const size_t at = fr.luma + ((size_t)by * fr.cw + (size_t)gx * NC) * BPS;
        load_words<CWORDS>(src + at, cbw);
        load_words<CWORDS>(src + at + fr.chroma, crw);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int d = sample_of<BPS>(cbw, i) - k.coff, e = sample_of<BPS>(crw, i) - k.coff;
            rv[i] = k.crv * e + k.half;
            gv[i] = k.half - k.cgu * d - k.cgv * e;
            bv[i] = k.cbu * d + k.half;
        }
    }
    const int rows = min(1 << SY, H - (by << SY));          // an odd H of a 4:2:0 frame: the last chroma row has one luma row
    for (int dy = 0; dy < rows; ++dy) {
        const size_t y = ((size_t)by << SY) + dy;
        unsigned yw[4 * BPS];
        load_words<4 * BPS>(src + (y * W + (size_t)gx * 16) * BPS, yw);
        unsigned o[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                        // four pixels = twelve bytes = three words, every byte placed once and whole
            unsigned r8[4], g8[4], b8[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = 4 * q + j, c = k.cy * (sample_of<BPS>(yw, p) - k.yoff);
                r8[j] = clip8((c + rv[p >> SX]) >> k.d);
                g8[j] = clip8((c + gv[p >> SX]) >> k.d);
                b8[j] = clip8((c + bv[p >> SX]) >> k.d);
            }
            o[3 * q] = r8[0] | g8[0] << 8 | b8[0] << 16 | r8[1] << 24;
            o[3 * q + 1] = g8[1] | b8[1] << 8 | r8[2] << 16 | g8[2] << 24;
            o[3 * q + 2] = b8[2] | r8[3] << 8 | g8[3] << 16 | b8[3] << 24;
        }
        uint4 *dst = (uint4 *)(rgb + ((f * H + y) * W + (size_t)gx * 16) * 3);
        dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
        dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
        dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
    }
}

// ---- byte path: any size and alignment, lane = (frame, chroma row by, chroma column bx) -------------------------------------------------------
template <int BPS, int SX, int SY, bool MONO>
__global__ __launch_bounds__(256) void yuv_to_rgb_block_kernel(const uint8_t *__restrict__ yuv, int H, int W, int64_t lanes, Coeffs k,
                                                               uint8_t *__restrict__ rgb) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= lanes) return;
    const Layout fr(H, W, BPS, SX, SY, MONO);
    const int bx = (int)(t % fr.cw);
    const int64_t r = t / fr.cw;
    const int by = (int)(r % fr.ch);
    const size_t f = (size_t)(r / fr.ch);
    const uint8_t *src = yuv + f * fr.bytes;
    int d = 0, e = 0;
    if (!MONO) {
        const size_t at = (size_t)by * fr.cw + bx;
        d = sample_at<BPS>(src + fr.luma, at) - k.coff;
        e = sample_at<BPS>(src + fr.luma + fr.chroma, at) - k.coff;
    }
    const int rv = k.crv * e + k.half, gv = k.half - k.cgu * d - k.cgv * e, bv = k.cbu * d + k.half;
    for (int dy = 0; dy < (1 << SY); ++dy)
        for (int dx = 0; dx < (1 << SX); ++dx) {
            const int y = (by << SY) + dy, x = (bx << SX) + dx;
            if (y >= H || x >= W) continue;
            const int c = k.cy * (sample_at<BPS>(src, (size_t)y * W + x) - k.yoff);
            uint8_t *o = rgb + ((f * H + y) * W + x) * 3;
            o[0] = (uint8_t)clip8((c + rv) >> k.d);
            o[1] = (uint8_t)clip8((c + gv) >> k.d);
            o[2] = (uint8_t)clip8((c + bv) >> k.d);
        }
}

template <int BPS, int SX, int SY, bool MONO>
int launch(hipStream_t s, const Coeffs &k, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb) {
    const bool wide = W % 16 == 0 && (((uintptr_t)yuv | (uintptr_t)rgb) & 15) == 0;
    const Layout fr(H, W, BPS, SX, SY, MONO);
    const int64_t lanes = (int64_t)n * fr.ch * (wide ? W / 16 : fr.cw), blocks = (lanes + 255) / 256;
    PB_CHECK(blocks <= 0x7fffffff, -1, "yuv_to_rgb: %d frames of %d x %d exceed the launch grid", n, H, W);
    if (wide) hipLaunchKernelGGL((yuv_to_rgb_kernel<BPS, SX, SY, MONO>), dim3((unsigned)blocks), dim3(256), 0, s, yuv, H, W, lanes, k, rgb);
    else hipLaunchKernelGGL((yuv_to_rgb_block_kernel<BPS, SX, SY, MONO>), dim3((unsigned)blocks), dim3(256), 0, s, yuv, H, W, lanes, k, rgb);
    PB_HIP(hipGetLastError());
    return 0;
}

template <int BPS>
int launch_layout(int chroma, hipStream_t s, const Coeffs &k, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb) {
    switch (chroma) {
        case 400: return launch<BPS, 0, 0, true>(s, k, yuv, n, H, W, rgb);
        case 420: return launch<BPS, 1, 1, false>(s, k, yuv, n, H, W, rgb);
        case 422: return launch<BPS, 1, 0, false>(s, k, yuv, n, H, W, rgb);
        default: return launch<BPS, 0, 0, false>(s, k, yuv, n, H, W, rgb);
    }
}

int64_t rhu(int64_t p, int64_t q) { return (2 * p + q) / (2 * q); }      // round half up of p / q, both positive

// the table of a good format, from exact rationals: Kr = kr / den ..., 2^d sy = yn / yd, 2^d sc = cn / cd (the largest product is below 2^48)
Coeffs coeffs_of(const pb_yuv_fmt &f) {
    const int d = f.depth;
    const int64_t den = f.matrix == PB_YUV_BT709 ? 10000 : 1000, kr = f.matrix == PB_YUV_BT709 ? 2126 : 299,
                  kb = f.matrix == PB_YUV_BT709 ? 722 : 114, kg = den - kr - kb;
    const int64_t full = ((int64_t)1 << d) - 1;
    const int64_t yn = f.full_range ? 255 * (full + 1) : 255 * 256, yd = f.full_range ? full : 219, cn = yn, cd = f.full_range ? full : 224;
    Coeffs k;
    k.cy = (int)rhu(yn, yd);
    k.crv = (int)rhu(cn * 2 * (den - kr), cd * den);
    k.cgu = (int)rhu(cn * 2 * kb * (den - kb), cd * den * kg);
    k.cgv = (int)rhu(cn * 2 * kr * (den - kr), cd * den * kg);
    k.cbu = (int)rhu(cn * 2 * (den - kb), cd * den);
    k.yoff = f.full_range ? 0 : 16 << (d - 8);
    k.coff = k.half = 1 << (d - 1);
    k.d = d;
    return k;
}

}  // namespace

bool yuv_fmt_ok(const pb_yuv_fmt &f) {
    return (f.chroma == 400 || f.chroma == 420 || f.chroma == 422 || f.chroma == 444) && f.depth >= 8 && f.depth <= 16 &&
           (f.full_range == 0 || f.full_range == 1) && (f.matrix == PB_YUV_BT601 || f.matrix == PB_YUV_BT709);
}

bool yuv_fmt_is_i420(const pb_yuv_fmt &f) { return f.chroma == 420 && f.depth == 8 && f.full_range == 0 && f.matrix == PB_YUV_BT601; }

int64_t yuv_frame_bytes(const pb_yuv_fmt &f, int H, int W) {
    if (!yuv_fmt_ok(f) || H <= 0 || W <= 0) return 0;
    return (int64_t)Layout(H, W, f.depth > 8 ? 2 : 1, f.chroma == 420 || f.chroma == 422, f.chroma == 420, f.chroma == 400).bytes;
}

void yuv_coeffs(const pb_yuv_fmt &f, int32_t out[7]) {
    const Coeffs k = coeffs_of(f);
    const int32_t v[7] = {k.cy, k.crv, k.cgu, k.cgv, k.cbu, k.yoff, k.coff};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
}

int launch_yuv_to_rgb(hipStream_t s, const pb_yuv_fmt &f, const uint8_t *yuv, int n, int H, int W, uint8_t *rgb) {
    PB_CHECK(yuv_fmt_ok(f), -1, "yuv_to_rgb: no such format (chroma %d, depth %d, full_range %d, matrix %d)", f.chroma, f.depth, f.full_range, f.matrix);
    PB_CHECK(yuv && rgb && n > 0 && H > 0 && W > 0, -1, "yuv_to_rgb: bad arguments (n %d, %d x %d)", n, H, W);
    if (yuv_fmt_is_i420(f)) return launch_i420_to_rgb(s, yuv, n, H, W, rgb);
    const Coeffs k = coeffs_of(f);
    return f.depth > 8 ? launch_layout<2>(f.chroma, s, k, yuv, n, H, W, rgb) : launch_layout<1>(f.chroma, s, k, yuv, n, H, W, rgb);
}
