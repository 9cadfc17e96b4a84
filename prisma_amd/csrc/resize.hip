// Bilinear resize of packed 8-bit RGB frames, exact integers (include/prisma_bands.h pb_rgb_resize; the host states the same arithmetic in
// bands/common/resize.py and tests/resize_ref.py pins both).  Half-pixel centres, the geometry of swscale's SWS_BILINEAR; per axis, for output
// index x of n_out from n_in samples:
//   num = (2 x + 1) n_in - n_out (may be negative);  i0 = floor(num / (2 n_out)), r = num - i0 2 n_out;  w = (256 r + n_out) / (2 n_out), 0 .. 256
//   taps clamp(i0, 0, n_in - 1) and clamp(i0 + 1, 0, n_in - 1)
// and per channel, rounded once:
//   out = ((256 - wy) ((256 - wx) p00 + wx p01) + wy ((256 - wx) p10 + wx p11) + 32768) >> 16
// Everything fits in int32 (the launcher refuses a side above 16384), and an equal-size call is a byte copy (w = 0 everywhere).  The same two
// taps serve a shrink: swscale widens its filter there, this code does not.  It is not swscale's fixed-point code: PARITY UNPINNED (PyAV is not
// in the build image); tests/test_resize_ref_cpu.py pins the geometry against Pillow's bilinear to one LSB on enlargements.
// rgb_resize_i420_*: the same pixels straight into I420 - byte for byte launch_rgb_to_i420 of the resized frames (luma_of / cb_of / cr_of of yuv.h,
// chroma of the 2 x 2 block's rounded mean colour, pixel indices clamped to the frame), the resized RGB frame living in registers only.
//
// A lane owns whole 2 x 2 output blocks, as in yuv.hip, and the split is yuv.hip's: a 16-byte path where W % 16 == 0 and `out` is 16-byte aligned,
// a byte path for every other size.  The kernels are NOT bound by HBM: they wait for the loads of the taps and for the taps' arithmetic
// (EXPERIMENTS.md 6.22).  The first cut had yuv.hip's shape, 16 pixels of a row per lane and every tap a byte gather from global memory: a
// wavefront's gathers touched some twenty cache lines each, and that 16-byte path ran slower than the byte path (0.39 against 0.26 ms for 32
// frames of 810 x 1440 -> 1080 x 1920) - the measurement that moved the taps into LDS.  The 16-byte path now works in tiles of 256 blocks
// (512 pixels) of a block row per workgroup, which walks down kRows block rows: the four source rows a block row taps, cut to the tile's
// columns, come into LDS as aligned 32-bit words, all loads in flight together; every lane resizes its block from LDS with column taps it
// worked out once; luma / chroma (or the RGB bytes) go to LDS and leave as 16-byte stores (8-byte for the chroma runs): 0.16 ms for those 32
// frames into I420, 0.18 into RGB.  A size whose tiles' source columns do not fit an LDS row (a shrink to less than half) takes the byte path,
// one block (RGB: one pixel) per lane, gathers from global memory and byte stores.  Divisions are float estimates corrected to the exact
// quotient and products 24-bit multiplies: the 32-bit ones run at a quarter of the rate.  No lane reads outside its source frame or writes
// outside its output frame.
#include <algorithm>

#include "common.h"
#include "resize.h"
#include "yuv.h"

namespace {

constexpr int kTile = 256;          // blocks of a tile: one block row, 2 * kTile pixels wide
constexpr int kSpan = 3072;         // bytes of an LDS row: the source columns of a tile (up to 1022 pixels) from the 4-byte boundary below them
constexpr int kRows = 4;            // block rows a workgroup of the 16-byte path walks down: its column taps are worked out once

struct Tap { int a, b, w; };        // the two source indices of an output index and the weight of the second, 0 .. 256
struct Px { int r, g, b; };

// floor(num / d) and its remainder for num < 2^30, d < 2^16 and a quotient below 2^15: a float estimate with the reciprocal rd of d - off by one
// at most, the quotient's 15 bits against a 24-bit mantissa - and one correction either way.  (The compiler's 32-bit division and its 32-bit
// multiplies run at a quarter of the rate of the 24-bit ones; with them the kernels were bound by the taps' arithmetic, EXPERIMENTS.md 6.22.)
__device__ __forceinline__ unsigned div_floor(unsigned num, unsigned d, float rd, unsigned &rem) {
    unsigned q = (unsigned)((float)num * rd);
    int r = (int)(num - __umul24(q, d));
    if (r < 0) { --q; r += (int)d; }
    if (r >= (int)d) { ++q; r -= (int)d; }
    rem = (unsigned)r;
    return q;
}

__host__ __device__ __forceinline__ Tap tap_of(int o, int n_in, int n_out) {
    const unsigned d = 2u * (unsigned)n_out;
    Tap t;
#ifdef __HIP_DEVICE_COMPILE__
    const unsigned num = (unsigned)(__mul24(2 * o + 1, n_in) - n_out) + d;  // + d: never negative (output 0 has num = n_in - n_out > -d); i0 = q - 1
    const float rd = __builtin_amdgcn_rcpf((float)d);
    unsigned r, r2;
    const unsigned q = div_floor(num, d, rd, r);
    t.w = (int)div_floor((r << 8) + (unsigned)n_out, d, rd, r2);           // (256 r + n_out) < 513 n_out: exact in a float
#else
    const unsigned num = (unsigned)((2 * o + 1) * n_in - n_out) + d;
    const unsigned q = num / d;
    t.w = (int)((256u * (num - q * d) + (unsigned)n_out) / d);
#endif
    const int i0 = (int)q - 1, last = n_in - 1;
    t.a = i0 < 0 ? 0 : (i0 > last ? last : i0);
    t.b = i0 + 1 > last ? last : i0 + 1;
    return t;
}

// every product has factors below 2^24 (weights up to 256, sums up to 255 * 256): the 24-bit multiply is exact
__device__ __forceinline__ int lerp2(int p00, int p01, int p10, int p11, int wx, int wy) {
    const unsigned ux = (unsigned)wx, vx = 256u - ux, uy = (unsigned)wy, vy = 256u - uy;
    const unsigned top = __umul24(vx, (unsigned)p00) + __umul24(ux, (unsigned)p01), bot = __umul24(vx, (unsigned)p10) + __umul24(ux, (unsigned)p11);
    return (int)((__umul24(vy, top) + __umul24(uy, bot) + 32768u) >> 16);
}

// one output pixel from the two source rows r0, r1 of its vertical taps (global memory or LDS); tx indexes pixels of those rows
__device__ __forceinline__ Px sample(const uint8_t *r0, const uint8_t *r1, int wy, const Tap &tx) {
    const int a = __mul24(tx.a, 3), b = __mul24(tx.b, 3);
    const uint8_t *p00 = r0 + a, *p01 = r0 + b, *p10 = r1 + a, *p11 = r1 + b;
    Px o;
    o.r = lerp2(p00[0], p01[0], p10[0], p11[0], tx.w, wy);
    o.g = lerp2(p00[1], p01[1], p10[1], p11[1], tx.w, wy);
    o.b = lerp2(p00[2], p01[2], p10[2], p11[2], tx.w, wy);
    return o;
}

// ... from one source frame in global memory: a row's offset stays below 2^31 (sides up to 16384)
__device__ __forceinline__ Px sample(const uint8_t *__restrict__ src, int sw, const Tap &ty, const Tap &tx) {
    return sample(src + __mul24(ty.a, 3 * sw), src + __mul24(ty.b, 3 * sw), ty.w, tx);
}

// Every kernel: grid = (columns / 256, rows, frames) - blockIdx.z the frame, blockIdx.y the block row by (rgb_resize_px_kernel: the row y).

// ---- 16-byte paths: W % 16 == 0, `out` 16-byte aligned, every tile's source columns within kSpan bytes ---------------------------------------------
// workgroup = (frame, kRows block rows, tile of kTile blocks); lane = one block of the tile in each of the block rows.  I420: luma / Cb / Cr of the tile; else its RGB bytes.
template <bool I420>
__device__ __forceinline__ void resize_tile(const uint8_t *__restrict__ rgb, int sh, int sw, int H, int W, uint8_t *__restrict__ out) {
    __shared__ uint4 s_src[4][kSpan / 16];                   // source rows ty0.a, ty0.b, ty1.a, ty1.b from column c0 on
    __shared__ uint4 s_out[I420 ? 96 : 192];                 // I420: 512 + 512 luma bytes, 256 Cb, 256 Cr; RGB: 1536 bytes of each of the two rows
    const int lane = threadIdx.x, tile = blockIdx.x, cw = W / 2, ch = (H + 1) / 2;
    const size_t f = blockIdx.z;
    const uint8_t *src = rgb + f * sh * sw * 3;
    const int x0 = tile * 2 * kTile, x1 = min(W, x0 + 2 * kTile), px = x1 - x0;           // the tile's pixels [x0, x1): 16 .. 512, a multiple of 16
    const int c0 = tap_of(x0, sw, W).a, span = (tap_of(x1 - 1, sw, W).b - c0 + 1) * 3;      // its source columns from c0 on, `span` bytes a row
    const int bx = tile * kTile + lane;
    Tap tx[2] = {tap_of(min(2 * bx, W - 1), sw, W), tap_of(min(2 * bx + 1, W - 1), sw, W)};  // the block's columns, in the tile's LDS rows
    tx[0].a -= c0; tx[0].b -= c0; tx[1].a -= c0; tx[1].b -= c0;
    for (int by = blockIdx.y * kRows; by < min(ch, (int)(blockIdx.y + 1) * kRows); ++by) {
        const int rows = 2 * by + 1 < H ? 2 : 1;             // an odd H: the last block row is one pixel high, its row counts twice in the mean
        const Tap ty0 = tap_of(2 * by, sh, H), ty1 = rows == 2 ? tap_of(2 * by + 1, sh, H) : ty0;
        const int row[4] = {ty0.a, ty0.b, ty1.a, ty1.b};
        // The rows' bytes as aligned 32-bit words, all loads first, then the LDS stores: byte i of a row's columns lands at LDS byte mis + i.  Words
        // lo .. hi - 1 lie wholly inside the row's columns; the up to three bytes in front of them and behind them are copied by lanes 0 .. 7.
        unsigned v[4][3];
        int mis[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t *g = src + (row[k] * sw + c0) * 3;
            mis[k] = (int)((uintptr_t)g & 3);
            const int lo = (mis[k] + 3) >> 2, hi = (mis[k] + span) >> 2;     // hi <= kSpan / 4 (tiles_fit)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int w = min(max(lane + 256 * j, lo), hi - 1);          // a word of the row in any case, where it has one
                v[k][j] = hi > lo ? *(const unsigned *)(g - mis[k] + 4 * w) : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lo = (mis[k] + 3) >> 2, hi = (mis[k] + span) >> 2;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (lane + 256 * j >= lo && lane + 256 * j < hi) ((unsigned *)s_src[k])[lane + 256 * j] = v[k][j];
        }
        if (lane < 8) {
            const int k = lane >> 1;
            const uint8_t *g = src + ((k == 0 ? ty0.a : k == 1 ? ty0.b : k == 2 ? ty1.a : ty1.b) * sw + c0) * 3;
            const int m = (int)((uintptr_t)g & 3), lo = (m + 3) >> 2, hi = (m + span) >> 2;
            // in front of word lo: bytes [0, 4 lo - m); behind word hi - 1: bytes [4 hi - m, span) - or, with no whole word, all of them at once
            const int from = (lane & 1) ? max(4 * hi - m, hi > lo ? 0 : span) : 0, to = (lane & 1) ? span : (hi > lo ? 4 * lo - m : span);
            uint8_t *sb = (uint8_t *)s_src[0] + k * kSpan + m;
            for (int i = from; i < to; ++i) sb[i] = g[i];
        }
        __syncthreads();
        if (bx < cw) {
            Px p[2][2];
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                p[0][dx] = sample((const uint8_t *)s_src[0] + mis[0], (const uint8_t *)s_src[1] + mis[1], ty0.w, tx[dx]);
                p[1][dx] = sample((const uint8_t *)s_src[2] + mis[2], (const uint8_t *)s_src[3] + mis[3], ty1.w, tx[dx]);
            }
            if (I420) {
                unsigned short *y = (unsigned short *)s_out;
                uint8_t *c = (uint8_t *)s_out + 4 * kTile;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
                    y[dy * kTile + lane] = (unsigned short)(luma_of(p[dy][0].r, p[dy][0].g, p[dy][0].b) | luma_of(p[dy][1].r, p[dy][1].g, p[dy][1].b) << 8);
                const int rr = (p[0][0].r + p[0][1].r + p[1][0].r + p[1][1].r + 2) >> 2, gg = (p[0][0].g + p[0][1].g + p[1][0].g + p[1][1].g + 2) >> 2,
                          bb = (p[0][0].b + p[0][1].b + p[1][0].b + p[1][1].b + 2) >> 2;
                c[lane] = (uint8_t)cb_of(rr, gg, bb);
                c[kTile + lane] = (uint8_t)cr_of(rr, gg, bb);
            } else {
                unsigned short *o = (unsigned short *)s_out;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {             // six bytes = three 16-bit words, each whole
                    unsigned short *q = o + dy * 3 * kTile + 3 * lane;
                    q[0] = (unsigned short)(p[dy][0].r | p[dy][0].g << 8);
                    q[1] = (unsigned short)(p[dy][0].b | p[dy][1].r << 8);
                    q[2] = (unsigned short)(p[dy][1].g | p[dy][1].b << 8);
                }
            }
        }
        __syncthreads();
        // (the next block row's fills and LDS stores come after its own barrier: no lane overtakes these reads of s_out)
        if (I420) {
            const I420Frame fr(H, W);
            uint8_t *dst = out + f * fr.bytes;
            const int part = lane >> 5, i = lane & 31;       // lanes 0 .. 31: luma row 0, 32 .. 63: luma row 1, 64 .. 95: Cb, 96 .. 127: Cr
            if (part < 4 && 16 * i < px) {
                if (part < 2) {
                    if (part < rows) *(uint4 *)(dst + (size_t)(2 * by + part) * W + x0 + 16 * i) = s_out[32 * part + i];
                } else {
                    uint8_t *plane = dst + fr.luma + (part == 3 ? fr.chroma : 0);
                    *(uint2 *)(plane + (size_t)by * fr.cw + x0 / 2 + 8 * i) = ((const uint2 *)s_out)[128 + 32 * (part - 2) + i];
                }
            }
        } else {
            const int part = lane >= 96 ? 1 : 0, i = lane - 96 * part;   // lanes 0 .. 95: row 0, 96 .. 191: row 1
            if (lane < 192 && part < rows && 16 * i < 3 * px)
                *(uint4 *)(out + ((f * H + 2 * by + part) * W + x0) * 3 + 16 * i) = s_out[96 * part + i];
        }
    }
}

__global__ __launch_bounds__(256) void rgb_resize_kernel(const uint8_t *__restrict__ rgb, int sh, int sw, int H, int W, uint8_t *__restrict__ out) {
    resize_tile<false>(rgb, sh, sw, H, W, out);
}

__global__ __launch_bounds__(256) void rgb_resize_i420_kernel(const uint8_t *__restrict__ rgb, int sh, int sw, int H, int W, uint8_t *__restrict__ yuv) {
    resize_tile<true>(rgb, sh, sw, H, W, yuv);
}

// ---- byte paths: any size -----------------------------------------------------------------------------------------------------------------------------
// lane = (frame, row y, column x)
__global__ __launch_bounds__(256) void rgb_resize_px_kernel(const uint8_t *__restrict__ rgb, int sh, int sw, int H, int W, uint8_t *__restrict__ out) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t f = blockIdx.z;
    const Px p = sample(rgb + f * sh * sw * 3, sw, tap_of(y, sh, H), tap_of(x, sw, W));
    uint8_t *o = out + ((f * H + y) * W + x) * 3;
    o[0] = (uint8_t)p.r; o[1] = (uint8_t)p.g; o[2] = (uint8_t)p.b;
}

// lane = (frame, block row by, block column bx)
__global__ __launch_bounds__(256) void rgb_resize_i420_block_kernel(const uint8_t *__restrict__ rgb, int sh, int sw, int H, int W,
                                                                    uint8_t *__restrict__ yuv) {
    const I420Frame fr(H, W);
    const int bx = blockIdx.x * 256 + threadIdx.x, by = blockIdx.y;
    if (bx >= fr.cw) return;
    const size_t f = blockIdx.z;
    const uint8_t *src = rgb + f * sh * sw * 3;
    uint8_t *dst = yuv + f * fr.bytes;
    int sr = 0, sg = 0, sb = 0;
    for (int dy = 0; dy < 2; ++dy) {
        const int y = min(2 * by + dy, H - 1);               // clamped: the last row / column again
        const Tap ty = tap_of(y, sh, H);
        for (int dx = 0; dx < 2; ++dx) {
            const int x = min(2 * bx + dx, W - 1);
            const Px p = sample(src, sw, ty, tap_of(x, sw, W));
            sr += p.r; sg += p.g; sb += p.b;
            if (2 * by + dy < H && 2 * bx + dx < W) dst[(size_t)y * W + x] = (uint8_t)luma_of(p.r, p.g, p.b);
        }
    }
    sr = (sr + 2) >> 2; sg = (sg + 2) >> 2; sb = (sb + 2) >> 2;
    dst[fr.luma + (size_t)by * fr.cw + bx] = (uint8_t)cb_of(sr, sg, sb);
    dst[fr.luma + fr.chroma + (size_t)by * fr.cw + bx] = (uint8_t)cr_of(sr, sg, sb);
}

// the 16-byte path's condition on the sizes: every tile's source columns fit its LDS rows
bool tiles_fit(int sw, int W) {
    for (int x0 = 0; x0 < W; x0 += 2 * kTile) {
        const int x1 = W < x0 + 2 * kTile ? W : x0 + 2 * kTile;
        if ((tap_of(x1 - 1, sw, W).b - tap_of(x0, sw, W).a + 1) * 3 + 6 > kSpan) return false;      // + 6: the rows sit word-aligned in LDS
    }
    return true;
}

constexpr int kGridZ = 65535;       // frames of one launch (the grid's z limit); a longer call is cut

// `cols` lanes per row of the grid, `grid_rows` rows, one z slice per frame; in_frame / out_frame: bytes of a frame on either side
template <class K>
int launch(K kernel, hipStream_t s, const uint8_t *rgb, int n, int sh, int sw, int H, int W, int cols, int grid_rows, size_t out_frame, uint8_t *out) {
    const size_t in_frame = (size_t)sh * sw * 3;
    for (int f0 = 0; f0 < n; f0 += kGridZ) {
        const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)grid_rows, (unsigned)std::min(kGridZ, n - f0));
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, rgb + f0 * in_frame, sh, sw, H, W, out + f0 * out_frame);
        PB_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace

int launch_rgb_resize(hipStream_t s, const uint8_t *rgb, int n, int sh, int sw, int H, int W, uint8_t *out, bool out_i420) {
    PB_CHECK(rgb && out && n > 0 && sh > 0 && sw > 0 && H > 0 && W > 0, -1, "rgb_resize: bad arguments (n %d, %d x %d -> %d x %d)", n, sh, sw, H, W);
    // tap_of: (2 x + 1) n_in + n_out and 513 n_out stay inside 32 bits, quotients inside 15; a frame's offsets inside 31; rows inside the grid's y
    PB_CHECK(sh <= 16384 && sw <= 16384 && H <= 16384 && W <= 16384, -1, "rgb_resize: %d x %d -> %d x %d: a side above 16384", sh, sw, H, W);
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    const size_t out_frame = out_i420 ? (size_t)i420_frame_bytes(H, W) : (size_t)H * W * 3;
    // (the frames of a call are packed: with `out` aligned and W % 16 == 0 every frame, row and chroma run of the 16-byte path is aligned too)
    if (W % 16 == 0 && ((uintptr_t)out & 15) == 0 && tiles_fit(sw, W))
        return out_i420 ? launch(rgb_resize_i420_kernel, s, rgb, n, sh, sw, H, W, cw, (ch + kRows - 1) / kRows, out_frame, out)
                        : launch(rgb_resize_kernel, s, rgb, n, sh, sw, H, W, cw, (ch + kRows - 1) / kRows, out_frame, out);
    return out_i420 ? launch(rgb_resize_i420_block_kernel, s, rgb, n, sh, sw, H, W, cw, ch, out_frame, out)
                    : launch(rgb_resize_px_kernel, s, rgb, n, sh, sw, H, W, W, H, out_frame, out);
}
