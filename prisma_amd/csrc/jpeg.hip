// Baseline sequential JPEG (SOF0, 8 bit, JFIF) out of planar YUV {444 | 420 | 400, 8 bit, full range, BT.601}, one restart interval per MCU row, exact
// integers: include/prisma_bands.h pb_jpeg_encode states the rule and tests/jpeg_ref.py restates it; the bytes are the reference's.
//   coef    planes -> quantised coefficients, zigzagged int16, in coded order (frame, MCU row, MCU, block of the MCU).  A lane owns 16 x 8 samples
//           of one plane - two blocks -, read as eight 16-byte loads where the plane's rows are aligned (else bytes, clamped to the plane: the
//           padding).  F = C s C^T with C = round(2^13 c(u) / 2 cos((2x + 1) u pi / 16)) folded over its symmetry C[u][7 - x] = (-1)^u C[u][x]: the
//           same integers as the plain sums, half the products; the second pass accumulates in 64 bits.  Quantisation: sign(F) ((|F| + Q 2^25)
//           >> 26) div Q, which is (|F| + D / 2) div D for D = Q 2^26.
//   scan    one workgroup per interval: each block's code length (its DC difference is to the previous block of its component, read from the
//           coefficients, so blocks are independent) and the exclusive scan of the lengths: a block's bit offset in its interval.
//           The same workgroup then clears what the interval will use of its slot in the unstuffed stream (no memset of the worst case).
//   pack    one lane per block writes its codes at that offset into the interval's slot of an unstuffed stream (sized from the worst block,
//           20 + 63 x 26 bits): the word it shares with the block before and the one it shares with the block after by atomic OR, the words
//           between by plain stores.
//   count   one workgroup per interval: the 0xFF bytes of every 64-byte chunk of the interval (its last byte padded with 1-bits first) and
//           their exclusive scan; then one workgroup per frame scans the intervals' stuffed sizes, and one lane the frames' sizes: offsets[].
//   write   one lane per chunk copies it to its place in the caller's buffer, 0x00 after every 0xFF, the RSTm marker in front of an interval's first
//           chunk; one workgroup per frame writes the header segments and EOI.  Every position is checked against the capacity before the store, and
//           a frame whose end lies past the capacity is not written at all.
// No float anywhere; a frame's bytes do not depend on its place in the batch.  All stores are plain vector stores or vector atomics.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "jpeg.h"

namespace {

constexpr int kMaxBlockBytes = 208;      // ceil((20 + 63 * 26) / 8): DC 9 + 11 bits (11 + 11 chrominance, category <= 11), AC 16 + 10 bits each
constexpr int kChunk = 64;               // bytes of the unstuffed stream one lane counts and copies

// ---- tables of the standard (ITU-T T.81 Annex K), typed from it; tests/jpeg_ref.py holds the same and a test reads them back from Pillow's files
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kQ[2][64] = {{16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
                               {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// the codes of Annex C: entry = code << 8 | length, indexed by symbol (0 where the table has none); per table 16 DC entries, then 256 AC entries
constexpr int kHuffWords = 16 + 256;
struct HuffEnc { uint32_t e[2][kHuffWords]; };
constexpr HuffEnc make_huff() {
    HuffEnc h{};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kDcBits[t][len - 1]; ++i, ++k, ++code) h.e[t][k] = (code << 8) | (uint32_t)len;      // HUFFVAL of both DC tables is 0 .. 11
            code <<= 1;
        }
        code = 0; k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kAcBits[t][len - 1]; ++i, ++k, ++code) h.e[t][16 + kAcVals[t][k]] = (code << 8) | (uint32_t)len;
            code <<= 1;
        }
    }
    return h;
}
__constant__ HuffEnc g_huff = make_huff();

// the integer cosine matrix at 13 fractional bits: C[0][x] = 2896; C[u][x] = +- kCos[a] with a the angle (2x + 1) u folded into 0 .. 8 sixteenths of pi
constexpr int kCos[9] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0};
constexpr int cos_entry(int u, int x) {
    if (u == 0) return 2896;
    int a = ((2 * x + 1) * u) % 32;
    if (a > 16) a = 32 - a;
    return a > 8 ? -kCos[16 - a] : kCos[a];
}
constexpr int inv_zigzag(int natural) {
    for (int i = 0; i < 64; ++i)
        if (kZigzag[i] == natural) return i;
    return -1;
}

// ---- geometry of a call, by value to every kernel -------------------------------------------------------------------------------------------------
struct Geom {
    int n, H, W, ncomp, bpm;            // frames; components; blocks per MCU
    int R, MX, BI;                      // MCU rows = intervals per frame, MCUs per row, blocks per interval
    int hs[3], vs[3], koff[3], tab[3];  // per component: blocks per MCU across / down, first block of the MCU, table id
    int pw[3], ph[3], wide[3];          // plane size; rows are read by 16-byte loads
    int64_t poff[3], frame_bytes;       // plane offset in a frame
    int iv_stride, CI;                  // bytes of an interval's slot in the unstuffed stream, its chunks
    int hdr_len;
};
struct QTabs { uint16_t q[2][64]; };    // natural order
struct Header { uint8_t b[704]; };

struct Work {                           // the workspace, carved
    int16_t *coef;
    uint32_t *bitoff, *iv_bits, *chunk_pre, *iv_size, *iv_off;
    uint8_t *scratch;
    int64_t *frame_size;
};

bool make_geom(const pb_jpeg_cfg &cfg, int n, int H, int W, const uint8_t *planes, Geom &g) {
    if (!jpeg_cfg_ok(cfg) || H < 1 || W < 1 || H > 65535 || W > 65535) return false;
    memset(&g, 0, sizeof(g));
    g.n = n; g.H = H; g.W = W;
    const bool sub = cfg.chroma == 420;
    g.ncomp = cfg.chroma == 400 ? 1 : 3;
    g.bpm = cfg.chroma == 400 ? 1 : (sub ? 6 : 3);
    const int m = sub ? 16 : 8;
    g.R = (H + m - 1) / m;
    g.MX = (W + m - 1) / m;
    g.BI = g.MX * g.bpm;
    const int ch = sub ? (H + 1) / 2 : H, cw = sub ? (W + 1) / 2 : W;
    g.frame_bytes = (int64_t)H * W + (g.ncomp == 3 ? 2 * (int64_t)ch * cw : 0);
    for (int c = 0; c < g.ncomp; ++c) {
        g.hs[c] = g.vs[c] = (c == 0 && sub) ? 2 : 1;
        g.koff[c] = c == 0 ? 0 : (sub ? 3 + c : c);
        g.tab[c] = c ? 1 : 0;
        g.pw[c] = c ? cw : W;
        g.ph[c] = c ? ch : H;
        g.poff[c] = c == 0 ? 0 : (int64_t)H * W + (int64_t)(c - 1) * ch * cw;
        g.wide[c] = g.pw[c] % 16 == 0 && g.poff[c] % 16 == 0 && g.frame_bytes % 16 == 0 && ((uintptr_t)planes & 15) == 0;
    }
    g.iv_stride = (g.BI * kMaxBlockBytes + kChunk - 1) / kChunk * kChunk;
    g.CI = g.iv_stride / kChunk;
    return true;
}

void quant_tables(int quality, QTabs &t) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 64; ++i) t.q[k][i] = (uint16_t)std::min(std::max((kQ[k][i] * s + 50) / 100, 1), 255);
}

// every byte of a frame before its entropy-coded data: SOI, APP0, DQT per table, SOF0, DHT per table, DRI, SOS
int make_header(const pb_jpeg_cfg &cfg, const Geom &g, const QTabs &q, uint8_t *b) {
    int p = 0;
    auto put = [&](int v) { b[p++] = (uint8_t)v; };
    auto put2 = [&](int v) { put(v >> 8); put(v & 255); };
    auto seg = [&](int marker, int body) { put(0xFF); put(marker); put2(body + 2); };
    const int ntab = g.ncomp == 1 ? 1 : 2;
    put(0xFF); put(0xD8);
    seg(0xE0, 14);
    for (char ch : {'J', 'F', 'I', 'F', '\0'}) put(ch);
    put(1); put(1); put(0); put2(1); put2(1); put(0); put(0);
    for (int t = 0; t < ntab; ++t) {
        seg(0xDB, 65);
        put(t);
        for (int i = 0; i < 64; ++i) put(q.q[t][kZigzag[i]]);
    }
    seg(0xC0, 6 + 3 * g.ncomp);
    put(8); put2(g.H); put2(g.W); put(g.ncomp);
    for (int c = 0; c < g.ncomp; ++c) { put(c + 1); put((g.hs[c] << 4) | g.vs[c]); put(g.tab[c]); }
    for (int t = 0; t < ntab; ++t) {
        seg(0xC4, 17 + 12);
        put(t);
        for (int i = 0; i < 16; ++i) put(kDcBits[t][i]);
        for (int i = 0; i < 12; ++i) put(i);
        seg(0xC4, 17 + 162);
        put(0x10 | t);
        for (int i = 0; i < 16; ++i) put(kAcBits[t][i]);
        for (int i = 0; i < 162; ++i) put(kAcVals[t][i]);
    }
    seg(0xDD, 2);
    put2(g.MX);
    seg(0xDA, 4 + 2 * g.ncomp);
    put(g.ncomp);
    for (int c = 0; c < g.ncomp; ++c) { put(c + 1); put((g.tab[c] << 4) | g.tab[c]); }
    put(0); put(0x3F); put(0);
    return p;
}

int header_len(int ncomp) {
    const int ntab = ncomp == 1 ? 1 : 2;
    return 2 + 18 + ntab * 69 + (10 + 3 * ncomp) + ntab * (33 + 183) + 6 + (8 + 2 * ncomp);
}

// ---- (a) coefficients ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int byte_at(const unsigned *w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// one block: samples s[y][x] (already minus 128) -> quantised coefficients, packed two per word in zigzag order
__device__ __forceinline__ void dct_quant(const int (&s)[64], const QTabs &qt, int tab, unsigned (&out)[32]) {
    int t[64];      // t[y][u] = sum_x C[u][x] s[y][x]
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int e[4], o[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) { e[x] = s[8 * y + x] + s[8 * y + 7 - x]; o[x] = s[8 * y + x] - s[8 * y + 7 - x]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int a = 0;
#pragma unroll
            for (int x = 0; x < 4; ++x) a += cos_entry(u, x) * ((u & 1) ? o[x] : e[x]);
            t[8 * y + u] = a;
        }
    }
    short q[64];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int e[4], o[4];
#pragma unroll
        for (int y = 0; y < 4; ++y) { e[y] = t[8 * y + u] + t[8 * (7 - y) + u]; o[y] = t[8 * y + u] - t[8 * (7 - y) + u]; }
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            int64_t F = 0;
#pragma unroll
            for (int y = 0; y < 4; ++y) F += (int64_t)cos_entry(v, y) * (int64_t)((v & 1) ? o[y] : e[y]);
            const unsigned Q = qt.q[tab][8 * v + u];
            const uint64_t mag = (uint64_t)(F < 0 ? -F : F);
            const unsigned N = (unsigned)((mag + ((uint64_t)Q << 25)) >> 26);
            const int m = (int)(N / Q);
            q[inv_zigzag(8 * v + u)] = (short)(F < 0 ? -m : m);
        }
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) out[i] = (unsigned)(unsigned short)q[2 * i] | ((unsigned)(unsigned short)q[2 * i + 1] << 16);
}

// unit t of component c: 16 x 8 samples, two blocks
__device__ __forceinline__ void coef_unit(const uint8_t *__restrict__ planes, const Geom &g, const QTabs &qt, int16_t *__restrict__ coef, int c, int64_t t) {
    const int bw = g.MX * g.hs[c], bh = g.R * g.vs[c], upr = (bw + 1) / 2;
    if (t >= (int64_t)g.n * bh * upr) return;
    const int ux = (int)(t % upr);
    const int by = (int)((t / upr) % bh);
    const int64_t f = t / ((int64_t)upr * bh);
    const int pw = g.pw[c], ph = g.ph[c];
    const uint8_t *plane = planes + f * g.frame_bytes + g.poff[c];
    unsigned rows[8][4];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const uint8_t *row = plane + (size_t)min(by * 8 + y, ph - 1) * pw;      // past the plane: its last row again
        if (g.wide[c]) {
            const uint4 v = *(const uint4 *)(row + (size_t)ux * 16);
            rows[y][0] = v.x; rows[y][1] = v.y; rows[y][2] = v.z; rows[y][3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned w = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) w |= (unsigned)row[min(ux * 16 + 4 * k + j, pw - 1)] << (8 * j);      // past the plane: its last column again
                rows[y][k] = w;
            }
        }
    }
    const int tab = g.tab[c];
#pragma unroll 1
    for (int b = 0; b < 2; ++b) {
        const int bx = 2 * ux + b;
        if (bx >= bw) break;
        int s[64];
#pragma unroll
        for (int y = 0; y < 8; ++y)
#pragma unroll
            for (int x = 0; x < 8; ++x) s[8 * y + x] = (b ? byte_at(rows[y], 8 + x) : byte_at(rows[y], x)) - 128;
        unsigned out[32];
        dct_quant(s, qt, tab, out);
        // coded order: frame, MCU row, MCU, block of the MCU
        const int64_t blk = ((f * g.R + by / g.vs[c]) * g.MX + bx / g.hs[c]) * g.bpm + g.koff[c] + (by % g.vs[c]) * g.hs[c] + bx % g.hs[c];
        uint4 *dst = (uint4 *)(coef + blk * 64);
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
    }
}

__global__ __launch_bounds__(256) void jpeg_coef_kernel(const uint8_t *__restrict__ planes, Geom g, QTabs qt, int16_t *__restrict__ coef) {
    coef_unit(planes, g, qt, coef, (int)blockIdx.y, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// ---- the entropy coder of one block (F.1.2), over a sink that takes (bits, count) ----------------------------------------------------------------------
__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }                     // 0 for 0
__device__ __forceinline__ unsigned extra_bits(int v, int n) { return (unsigned)(v + (v >> 31)) & ((1u << n) - 1u); }      // v, or v - 1 below 0, in n bits

template <class Sink>
__device__ __forceinline__ void code_block(const unsigned (&w)[32], int pred, const uint32_t *tabs, Sink &sink) {
    const uint32_t *dc = tabs, *ac = tabs + 16;
    {
        const int d = (int)(short)(w[0] & 0xffffu) - pred;
        const int n = category(d);
        const uint32_t e = dc[n];
        sink.put(((e >> 8) << n) | extra_bits(d, n), (int)(e & 255u) + n);
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = (int)(short)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
        if (v == 0) {
            ++run;
        } else {
            while (run > 15) {
                const uint32_t z = ac[0xF0];
                sink.put(z >> 8, (int)(z & 255u));
                run -= 16;
            }
            const int n = category(v);
            const uint32_t e = ac[(run << 4) | n];
            sink.put(((e >> 8) << n) | extra_bits(v, n), (int)(e & 255u) + n);
            run = 0;
        }
    }
    if (run) {
        const uint32_t z = ac[0x00];
        sink.put(z >> 8, (int)(z & 255u));
    }
}

// block j of an interval: its component's table and the DC value it predicts from (0 at the interval's start)
__device__ __forceinline__ void block_context(const Geom &g, const int16_t *iv_coef, int j, int &tab, int &pred) {
    const int k = j % g.bpm, m = j / g.bpm;
    int prev;       // the previous block of the component in coded order, as an offset from j
    if (g.bpm == 6 && k < 4) { tab = 0; prev = k ? 1 : 3; }
    else { tab = k ? 1 : 0; prev = g.bpm; }
    const bool first = (g.bpm == 6 && k > 0 && k < 4) ? false : m == 0;
    pred = first ? 0 : (int)iv_coef[(int64_t)(j - prev) * 64];
}

__device__ __forceinline__ void load_block(const int16_t *p, unsigned (&w)[32]) {
    const uint4 *src = (const uint4 *)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = src[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
}

__device__ __forceinline__ void load_huff(uint32_t *lds) {
    for (int i = threadIdx.x; i < 2 * kHuffWords; i += blockDim.x) lds[i] = g_huff.e[i / kHuffWords][i % kHuffWords];
    __syncthreads();
}

// exclusive scan of v over the 256 lanes of a workgroup; total: the sum.  lds: 4 words
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *lds, unsigned &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();        // the lanes are done with what an earlier call left in lds
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < wv) before += lds[i];
        total += lds[i];
    }
    return before + inc - v;
}

struct LengthSink {
    unsigned bits = 0;
    __device__ __forceinline__ void put(unsigned, int n) { bits += (unsigned)n; }
};

// bits of block j of an interval
__device__ __forceinline__ unsigned block_length(const Geom &g, const int16_t *iv_coef, int j, const uint32_t *huff) {
    int tab, pred;
    block_context(g, iv_coef, j, tab, pred);
    unsigned w[32];
    load_block(iv_coef + (int64_t)j * 64, w);
    LengthSink sink;
    code_block(w, pred, huff + tab * kHuffWords, sink);
    return sink.bits;
}

// the part of an interval's slot that its `bits` bits reach, rounded up to 16 bytes, zeroed by lanes lane, lane + lanes, ...: the words the packing
// ORs into and the bytes the count reads.  The slot is sized from the worst block; a real interval uses a few per cent of it.
__device__ __forceinline__ void zero_interval(uint8_t *slot, unsigned bits, int stride, int lane, int lanes) {
    const unsigned units = min(((bits + 31) / 32 * 4 + 15) / 16, (unsigned)stride / 16);
    for (unsigned i = (unsigned)lane; i < units; i += (unsigned)lanes) ((uint4 *)slot)[i] = make_uint4(0, 0, 0, 0);
}

// ---- (b) + (c): code lengths and their exclusive scan, one workgroup per interval; it also clears what the interval will use of its slot ------------
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const int16_t *__restrict__ coef, Geom g, uint32_t *__restrict__ bitoff,
                                                        uint32_t *__restrict__ iv_bits, uint8_t *__restrict__ scratch) {
    __shared__ uint32_t huff[2 * kHuffWords];
    __shared__ unsigned part[4];
    load_huff(huff);
    const int64_t iv = blockIdx.x;
    const int16_t *iv_coef = coef + iv * g.BI * 64;
    unsigned carry = 0;
    for (int start = 0; start < g.BI; start += 256) {
        const int j = start + threadIdx.x;
        const unsigned bits = j < g.BI ? block_length(g, iv_coef, j, huff) : 0u;
        unsigned total;
        const unsigned ex = block_scan(bits, part, total);
        if (j < g.BI) bitoff[iv * g.BI + j] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) iv_bits[iv] = carry;
    zero_interval(scratch + iv * g.iv_stride, carry, g.iv_stride, (int)threadIdx.x, 256);       // carry is the same in every lane
}

// ---- (d) packing -------------------------------------------------------------------------------------------------------------------------------------
struct PackSink {
    uint32_t *words;        // the interval's slot, big-endian bit order: bit i of the stream is bit 7 - i % 8 of byte i / 8
    unsigned w, limit;      // next word, words of the slot
    uint64_t acc = 0;
    int nacc;               // bits of acc that belong below word w (the first word's leading bits are another block's: zeros here)
    bool first = true;
    __device__ __forceinline__ void emit(unsigned v) {
        if (w < limit) {
            if (first) atomicOr(&words[w], __builtin_bswap32(v));        // shared with the block before
            else words[w] = __builtin_bswap32(v);
        }
        first = false;
        ++w;
    }
    __device__ __forceinline__ void put(unsigned bits, int n) {         // n <= 26, nacc < 32
        acc = (acc << n) | bits;
        nacc += n;
        if (nacc >= 32) {
            nacc -= 32;
            emit((unsigned)(acc >> nacc));
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc > 0 && w < limit) atomicOr(&words[w], __builtin_bswap32((unsigned)(acc << (32 - nacc))));      // shared with the block after
    }
};

__device__ __forceinline__ void pack_block(const int16_t *__restrict__ coef, const Geom &g, const uint32_t *__restrict__ bitoff,
                                           uint8_t *__restrict__ scratch, const uint32_t *huff, int64_t blk) {
    if (blk >= (int64_t)g.n * g.R * g.BI) return;
    const int64_t iv = blk / g.BI;
    const int j = (int)(blk % g.BI);
    const int16_t *iv_coef = coef + iv * g.BI * 64;
    int tab, pred;
    block_context(g, iv_coef, j, tab, pred);
    unsigned w[32];
    load_block(iv_coef + (int64_t)j * 64, w);
    const unsigned o = bitoff[blk];
    PackSink sink;
    sink.words = (uint32_t *)(scratch + iv * g.iv_stride);
    sink.w = o >> 5;
    sink.limit = (unsigned)g.iv_stride / 4;
    sink.nacc = (int)(o & 31u);
    code_block(w, pred, huff + tab * kHuffWords, sink);
    sink.finish();
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int16_t *__restrict__ coef, Geom g, const uint32_t *__restrict__ bitoff,
                                                        uint8_t *__restrict__ scratch) {
    __shared__ uint32_t huff[2 * kHuffWords];
    load_huff(huff);
    pack_block(coef, g, bitoff, scratch, huff, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// ---- (e) stuffing and compaction -----------------------------------------------------------------------------------------------------------------------
// byte i of an interval of `bits` bits: its last byte padded with 1-bits
__device__ __forceinline__ unsigned stream_byte(const uint8_t *iv_bytes, unsigned i, unsigned bits) {
    unsigned b = iv_bytes[i];
    if (i == (bits - 1) >> 3 && (bits & 7u)) b |= 0xFFu >> (bits & 7u);
    return b;
}

// the 0xFF bytes of chunk ch of an interval
__device__ __forceinline__ unsigned count_chunk(const uint8_t *src, int ch, unsigned bits) {
    const unsigned nb = (bits + 7) >> 3, lo = (unsigned)ch * kChunk, hi = min(lo + (unsigned)kChunk, nb);
    unsigned cnt = 0;
    for (unsigned i = lo; i < hi; ++i) cnt += stream_byte(src, i, bits) == 0xFFu;
    return cnt;
}

__global__ __launch_bounds__(256) void jpeg_count_kernel(const uint8_t *__restrict__ scratch, Geom g, const uint32_t *__restrict__ iv_bits,
                                                         uint32_t *__restrict__ chunk_pre, uint32_t *__restrict__ iv_size) {
    __shared__ unsigned part[4];
    const int64_t iv = blockIdx.x;
    const unsigned bits = iv_bits[iv], nb = (bits + 7) >> 3;
    const uint8_t *src = scratch + iv * g.iv_stride;
    const int chunks = (int)((nb + kChunk - 1) / kChunk);
    unsigned carry = 0;
    for (int start = 0; start < chunks; start += 256) {
        const int ch = start + threadIdx.x;
        const unsigned cnt = ch < chunks && ch < g.CI ? count_chunk(src, ch, bits) : 0u;
        unsigned total;
        const unsigned ex = block_scan(cnt, part, total);
        if (ch < chunks && ch < g.CI) chunk_pre[iv * g.CI + ch] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) iv_size[iv] = nb + carry;
}

// one workgroup per frame: where each interval's data starts in the frame (its RSTm marker, if any, sits in the two bytes before) and the frame's size
__global__ __launch_bounds__(256) void jpeg_frame_kernel(Geom g, const uint32_t *__restrict__ iv_size, uint32_t *__restrict__ iv_off,
                                                         int64_t *__restrict__ frame_size) {
    __shared__ unsigned part[4];
    const int64_t f = blockIdx.x;
    unsigned carry = (unsigned)g.hdr_len;
    for (int start = 0; start < g.R; start += 256) {
        const int r = start + threadIdx.x;
        const unsigned v = r < g.R ? iv_size[f * g.R + r] + (r ? 2u : 0u) : 0u;
        unsigned total;
        const unsigned ex = block_scan(v, part, total);
        if (r < g.R) iv_off[f * g.R + r] = carry + ex + (r ? 2u : 0u);
        carry += total;
    }
    if (threadIdx.x == 0) frame_size[f] = (int64_t)carry + 2;
}

__global__ void jpeg_offsets_kernel(int n, const int64_t *__restrict__ frame_size, int64_t *__restrict__ offsets) {
    if (blockIdx.x || threadIdx.x) return;
    int64_t at = 0;
    offsets[0] = 0;
    for (int f = 0; f < n; ++f) {
        at += frame_size[f];
        offsets[f + 1] = at;
    }
}

__device__ __forceinline__ void store_checked(uint8_t *out, int64_t at, int64_t capacity, unsigned v) {
    if (at >= 0 && at < capacity) out[at] = (uint8_t)v;
}

__device__ __forceinline__ void write_chunk(const uint8_t *__restrict__ scratch, const Geom &g, const uint32_t *__restrict__ iv_bits,
                                            const uint32_t *__restrict__ chunk_pre, const uint32_t *__restrict__ iv_off,
                                            const int64_t *__restrict__ offsets, uint8_t *__restrict__ out, int64_t capacity, int64_t t) {
    if (t >= (int64_t)g.n * g.R * g.CI) return;
    const int64_t iv = t / g.CI;
    const int ch = (int)(t % g.CI);
    const unsigned bits = iv_bits[iv], nb = (bits + 7) >> 3;
    const unsigned lo = (unsigned)ch * kChunk, hi = min(lo + kChunk, nb);
    if (lo >= nb && ch) return;
    const int64_t f = iv / g.R;
    const int r = (int)(iv % g.R);
    if (offsets[f + 1] > capacity) return;       // the frame does not fit: none of it is written
    const int64_t base = offsets[f] + iv_off[iv];
    if (ch == 0 && r) {
        store_checked(out, base - 2, capacity, 0xFF);
        store_checked(out, base - 1, capacity, 0xD0 + ((r - 1) & 7));
    }
    if (lo >= nb) return;
    const uint8_t *src = scratch + iv * g.iv_stride;
    int64_t at = base + lo + chunk_pre[iv * g.CI + ch];
    for (unsigned i = lo; i < hi; ++i) {
        const unsigned b = stream_byte(src, i, bits);
        store_checked(out, at++, capacity, b);
        if (b == 0xFFu) store_checked(out, at++, capacity, 0);
    }
}

__global__ __launch_bounds__(256) void jpeg_write_kernel(const uint8_t *__restrict__ scratch, Geom g, const uint32_t *__restrict__ iv_bits,
                                                         const uint32_t *__restrict__ chunk_pre, const uint32_t *__restrict__ iv_off,
                                                         const int64_t *__restrict__ offsets, uint8_t *__restrict__ out, int64_t capacity) {
    write_chunk(scratch, g, iv_bits, chunk_pre, iv_off, offsets, out, capacity, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void jpeg_header_kernel(Geom g, Header hdr, const int64_t *__restrict__ offsets, uint8_t *__restrict__ out,
                                                          int64_t capacity) {
    const int64_t f = blockIdx.x;
    if (offsets[f + 1] > capacity) return;
    for (int i = threadIdx.x; i < g.hdr_len; i += 256) store_checked(out, offsets[f] + i, capacity, hdr.b[i]);
    if (threadIdx.x == 0) {
        store_checked(out, offsets[f + 1] - 2, capacity, 0xFF);
        store_checked(out, offsets[f + 1] - 1, capacity, 0xD9);
    }
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

bool jpeg_cfg_ok(const pb_jpeg_cfg &cfg) {
    return (cfg.chroma == 444 || cfg.chroma == 420 || cfg.chroma == 400) && cfg.quality >= 1 && cfg.quality <= 100;
}

int64_t jpeg_frame_bound(const pb_jpeg_cfg &cfg, int H, int W) {
    Geom g;
    if (!make_geom(cfg, 1, H, W, nullptr, g)) return 0;
    // every block at its longest, every byte of it stuffed; the markers between the intervals; EOI
    return header_len(g.ncomp) + (int64_t)g.R * (2 * (int64_t)g.BI * kMaxBlockBytes) + 2 * (int64_t)(g.R - 1) + 2;
}

int JpegState::grow_host(size_t in_bytes, size_t out_bytes, int frames) {
    for (int i = 0; i < 2; ++i) {
        if (in_bytes > in_cap) {
            if (d_in[i]) PB_HIP(hipFree(d_in[i]));
            d_in[i] = nullptr;
            PB_HIP(hipMalloc(&d_in[i], in_bytes));
        }
        if (out_bytes > out_cap) {
            if (d_out[i]) PB_HIP(hipFree(d_out[i]));
            d_out[i] = nullptr;
            PB_HIP(hipMalloc(&d_out[i], out_bytes));
        }
        if (frames + 1 > offs_cap) {
            if (d_offs[i]) PB_HIP(hipFree(d_offs[i]));
            if (h_offs[i]) PB_HIP(hipHostFree(h_offs[i]));
            d_offs[i] = h_offs[i] = nullptr;
            PB_HIP(hipMalloc((void **)&d_offs[i], (size_t)(frames + 1) * 8));
            PB_HIP(hipHostMalloc((void **)&h_offs[i], (size_t)(frames + 1) * 8, hipHostMallocDefault));
        }
    }
    in_cap = std::max(in_cap, in_bytes);
    out_cap = std::max(out_cap, out_bytes);
    offs_cap = std::max(offs_cap, frames + 1);
    return 0;
}

void JpegState::release() {
    if (ws) hipFree(ws);
    for (int i = 0; i < 2; ++i) {
        if (d_in[i]) hipFree(d_in[i]);
        if (d_out[i]) hipFree(d_out[i]);
        if (d_offs[i]) hipFree(d_offs[i]);
        if (h_offs[i]) hipHostFree(h_offs[i]);
    }
    *this = JpegState();
}

int jpeg_encode_dev(JpegState &st, hipStream_t s, const pb_jpeg_cfg &cfg, const uint8_t *planes, int n, int H, int W, uint8_t *out, int64_t capacity,
                    int64_t *offsets) {
    Geom g;
    PB_CHECK(jpeg_cfg_ok(cfg), -1, "jpeg_encode: no such format (chroma %d: 444, 420 or 400; quality %d: 1 .. 100)", cfg.chroma, cfg.quality);
    PB_CHECK(planes && out && offsets && n > 0 && capacity >= 0, -1, "jpeg_encode: bad arguments (n %d, capacity %lld)", n, (long long)capacity);
    PB_CHECK(make_geom(cfg, n, H, W, planes, g), -1, "jpeg_encode: a %d x %d frame (a side is 1 .. 65535)", H, W);
    g.hdr_len = header_len(g.ncomp);
    const int64_t ivs = (int64_t)n * g.R, blocks = ivs * g.BI, chunks = ivs * g.CI;
    PB_CHECK(jpeg_frame_bound(cfg, H, W) < ((int64_t)1 << 31) && blocks < ((int64_t)1 << 31) / 64 && (chunks + 255) / 256 <= 0x7fffffff, -1,
             "jpeg_encode: %d frames of %d x %d are more than one call takes", n, H, W);
    QTabs qt;
    quant_tables(cfg.quality, qt);
    Header hdr;
    memset(&hdr, 0, sizeof(hdr));
    PB_CHECK(g.hdr_len <= (int)sizeof(hdr.b) && make_header(cfg, g, qt, hdr.b) == g.hdr_len, -2, "jpeg_encode: header of %d bytes", g.hdr_len);

    // the workspace
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    const size_t o_coef = take((size_t)blocks * 128), o_bitoff = take((size_t)blocks * 4), o_ivbits = take((size_t)ivs * 4),
                 o_scratch = take((size_t)ivs * g.iv_stride), o_chunk = take((size_t)chunks * 4), o_ivsize = take((size_t)ivs * 4),
                 o_ivoff = take((size_t)ivs * 4), o_fsize = take((size_t)n * 8);
    if (at > st.ws_cap) {
        PB_HIP(hipStreamSynchronize(s));        // an earlier call may still use the block
        if (st.ws) PB_HIP(hipFree(st.ws));
        st.ws = nullptr; st.ws_cap = 0;
        PB_HIP(hipMalloc(&st.ws, at));
        st.ws_cap = at;
    }
    char *base = (char *)st.ws;
    Work k;
    k.coef = (int16_t *)(base + o_coef);
    k.bitoff = (uint32_t *)(base + o_bitoff);
    k.iv_bits = (uint32_t *)(base + o_ivbits);
    k.scratch = (uint8_t *)(base + o_scratch);
    k.chunk_pre = (uint32_t *)(base + o_chunk);
    k.iv_size = (uint32_t *)(base + o_ivsize);
    k.iv_off = (uint32_t *)(base + o_ivoff);
    k.frame_size = (int64_t *)(base + o_fsize);

    int64_t units = 0;
    for (int c = 0; c < g.ncomp; ++c) units = std::max(units, (int64_t)n * g.R * g.vs[c] * ((g.MX * g.hs[c] + 1) / 2));
    hipLaunchKernelGGL(jpeg_coef_kernel, dim3((unsigned)((units + 255) / 256), g.ncomp), dim3(256), 0, s, planes, g, qt, k.coef);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)ivs), dim3(256), 0, s, k.coef, g, k.bitoff, k.iv_bits, k.scratch);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, k.coef, g, k.bitoff, k.scratch);
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)ivs), dim3(256), 0, s, k.scratch, g, k.iv_bits, k.chunk_pre, k.iv_size);
    hipLaunchKernelGGL(jpeg_frame_kernel, dim3((unsigned)n), dim3(256), 0, s, g, k.iv_size, k.iv_off, k.frame_size);
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(64), 0, s, n, k.frame_size, offsets);
    hipLaunchKernelGGL(jpeg_write_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, k.scratch, g, k.iv_bits, k.chunk_pre, k.iv_off,
                       offsets, out, capacity);
    hipLaunchKernelGGL(jpeg_header_kernel, dim3((unsigned)n), dim3(256), 0, s, g, hdr, offsets, out, capacity);
    PB_HIP(hipGetLastError());
    return 0;
}
