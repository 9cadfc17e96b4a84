// flow_raft --alternate_corr: the 9 x 9 x 4 correlation lookup computed from the feature maps, without the all-pairs volume
// (reference: AlternateCorrBlock, bands/raft/corr.py:63-91, selected in raft.py:103-106).
//
// corr_lookup_kernel (raft_kernels.hip) reads the 10 x 10 integer-grid entries of a window from the stored volume; here they are
//     c_l(r, t) = (1/16) sum_k fmap1[r, k] fpool_l[target frame, t, k]          (level 0: fpool_0 = the feature map itself)
// computed when they are needed.  A per-row gather of 400 target rows of 512 bytes would move ~100x the bytes of the volume lookup, so the
// work is shared by the 64 source pixels of an 8 x 8 tile, whose windows overlap when the flow is coherent:
//   1. the tile's 64 source rows (64 x 256 fp16) are staged in the LDS once, for all four levels;
//   2. per level: the 9 + 9 sample coordinates of every row (the fp32 sequence of corr_lookup_kernel, restated below), and the bounding box of
//      the tile's windows clipped to the level - rows outside the level contribute nothing and no address is formed for them;
//   3. the box is walked in chunks of 32 targets, one chunk per wave at a time (the next one's loads in flight): a 64 x 32 x 256 GEMM on v_mfma_f32_32x32x16_f16 (A = the staged
//      source rows, B = the targets' features straight from global memory in fragment order, fp32 accumulators, K in ascending order), and
//      every accumulator element (row r, target t) that falls into r's own 11 x 11 window is written - times 1/16, exact - to the row's fp32
//      window in the LDS.  An entry has exactly one slot, so the waves never meet and the chunk loop has no barrier;
//   4. one thread per (row, window column) blends its 9 samples from the fp32 window with corr_lookup_kernel's expression and stores them.
// Numerics: fp16 operands, fp32 accumulation, the entry is NOT rounded to fp16 before the blend (there is no volume to store it in); the only
// fp16 rounding is the final store (tests/raft_otf_ref.py restates exactly this).  An entry's bits depend on its source row and its target
// alone (one accumulator element, fixed K order): not on the tile's other rows, the box, the chunk, or the number of pair-directions.
// Incoherent flow only makes the box larger - up to the whole level: slower, same result.
#include <limits.h>

#include "raft_kernels.h"

#define LAUNCH_CHECK() do { PB_HIP(hipGetLastError()); return 0; } while (0)

struct OtfArgs {
    const f16 *src;            // source features [frames, P, 256]
    const f16 *tgt[4];         // target features of level l [frames, h[l] * w[l], 256]
    int h[4], w[4];
    int dirs;                  // 0: row block n reads source frame n and target frame n (op-level entry point); 1 / 2: n = i * dirs + d reads
};                             // source frame i + d and target frame i + 1 - d (RaftEngine::infer's pair order)

constexpr int OTF_LDA = 264;                       // halfs per staged source row: 528 bytes, so 16-byte fragment reads of 16 rows hit 64 distinct banks
constexpr int OTF_WIN = 11;                        // window side: the 9 floors of a row spread over at most 10 targets, + 1 for the right / lower tap
constexpr int OTF_SMEM = 64 * OTF_LDA * 2 + 64 * OTF_WIN * OTF_WIN * 4 + 64 * 18 * 4 * 2 + 64 * 8 + 16;

__global__ __launch_bounds__(256, 2) void corr_lookup_otf_kernel(OtfArgs g, const float *__restrict__ flow, int P, int w8, f16 *__restrict__ out,
                                                                  int ldo, int o8_off, float o8_scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f16 *As = (f16 *)smem;
    float *win = (float *)(smem + 64 * OTF_LDA * 2);
    int *ci = (int *)(win + 64 * OTF_WIN * OTF_WIN);
    float *ca = (float *)(ci + 64 * 18);
    float *fl = ca + 64 * 18;                      // the 64 rows' flow
    int *box = (int *)(fl + 128);                  // x min, x max, y min, y max over the tile's windows
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
    const int h8 = g.h[0];
    const int tiles_x = (w8 + 7) >> 3;
    const int n = blockIdx.y, tx0 = (blockIdx.x % tiles_x) * 8, ty0 = (blockIdx.x / tiles_x) * 8;
    const int sf = g.dirs ? n / g.dirs + n % g.dirs : n, tf = g.dirs ? n / g.dirs + 1 - n % g.dirs : n;
    // row pr of the tile = pixel (ty0 + pr / 8, tx0 + pr % 8); rows outside the grid are staged as zeros, take no part in the box and store nothing
    {
        const f16 *sb = g.src + (int64_t)sf * P * 256;
        f16x8 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = t + 256 * u, pr = idx >> 5, c = idx & 31;
            const int py = ty0 + (pr >> 3), px = tx0 + (pr & 7);
            const bool ok = py < h8 && px < w8;
            const f16x8 z = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
            v[u] = ok ? *(const f16x8 *)(sb + ((int64_t)py * w8 + px) * 256 + c * 8) : z;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = t + 256 * u, pr = idx >> 5, c = idx & 31;
            *(f16x8 *)(As + pr * OTF_LDA + c * 8) = v[u];
        }
        if (t < 64) {
            const int py = ty0 + (t >> 3), px = tx0 + (t & 7);
            const bool ok = py < h8 && px < w8;
            const f32x2 z = {0.f, 0.f};
            const f32x2 f = ok ? *(const f32x2 *)(flow + ((int64_t)n * P + (int64_t)py * w8 + px) * 2) : z;
            fl[t * 2] = f[0]; fl[t * 2 + 1] = f[1];
        }
    }
    for (int l = 0; l < 4; ++l) {
        const int lw = g.w[l], lhh = g.h[l];
        if (t < 4) box[t] = (t & 1) ? INT_MIN : INT_MAX;
        __syncthreads();                               // the previous level's blend has read win / ci; As and fl are staged
        for (int i = t; i < 64 * OTF_WIN * OTF_WIN; i += 256) win[i] = 0.f;
        for (int idx = t; idx < 64 * 18; idx += 256) {
            const int k = idx % 18, pr = idx / 18;
            const int py = ty0 + (pr >> 3), px = tx0 + (pr & 7);
            const float inv = 1.f / (float)(1 << l);
            const bool isx = k < 9;
            // corr_lookup_kernel's coordinate sequence, operation for operation (raft_kernels.hip: grid_sample's normalise / un-normalise round
            // trip with align_corners=True, the floor clamped to +-65536 so that the integer arithmetic below cannot overflow)
            const float c = (float)(isx ? px : py) + (isx ? fl[pr * 2] : fl[pr * 2 + 1]);
            const int dim = isx ? lw : lhh;
            const float v = ((2.f * (c * inv + (float)(isx ? k - 4 : k - 13)) / (float)(dim - 1) - 1.f) + 1.f) * 0.5f * (float)(dim - 1);
            const float f = floorf(v);
            const int fi = (int)fminf(fmaxf(f, -65536.f), 65536.f);
            ci[idx] = fi;
            ca[idx] = v - f;
            if (py < h8 && px < w8) {                  // the floors ascend with k: the first one and the last one + 1 bound the window
                if (k == 0) atomicMin(&box[0], fi);
                if (k == 8) atomicMax(&box[1], fi + 1);
                if (k == 9) atomicMin(&box[2], fi);
                if (k == 17) atomicMax(&box[3], fi + 1);
            }
        }
        __syncthreads();
        const int bx0 = max(box[0], 0), bx1 = min(box[1], lw - 1), by0 = max(box[2], 0), by1 = min(box[3], lhh - 1);
        const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
        const int nt = bw > 0 && bh > 0 ? bw * bh : 0;     // a box wholly outside the level: no target is addressed, the windows stay zero
        const f16 *tb = g.tgt[l] + (int64_t)tf * lhh * lw * 256;
        // chunk c0 .. c0 + 31 of the box, target li of it: its position in the level and its fragment pointer
        auto target = [&](int c0, int &ty, int &tx) -> const f16 * {
            const int tt = c0 + li, ttc = tt < nt ? tt : nt - 1;      // the last chunk's spare lanes repeat the last target and write nothing
            ty = by0 + ttc / bw; tx = bx0 + ttc % bw;
            return tb + ((int64_t)ty * lw + tx) * 256 + lh * 8;
        };
        auto load_b = [&](f16x8 (&b)[16], const f16 *bp) {
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) b[ks] = *(const f16x8 *)(bp + ks * 16);
        };
        auto chunk = [&](const f16x8 (&b)[16], int c0, int ty, int tx) {
            f32x16 acc[2];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
            // (an opaque offset: otherwise the 32 loop-invariant A fragments are hoisted out of the chunk loop into 128 registers, and the
            // two B register sets spill)
            int aoff = li * OTF_LDA + lh * 8;
            asm volatile("" : "+v"(aoff));
            const f16 *ap = As + aoff;
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                const f16x8 a0 = *(const f16x8 *)(ap + ks * 16), a1 = *(const f16x8 *)(ap + 32 * OTF_LDA + ks * 16);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[ks], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b[ks], acc[1], 0, 0, 0);
            }
            // acc[m][r]: source row m * 32 + (r & 3) + 8 (r >> 2) + 4 lh of the tile, target li of the chunk
            if (c0 + li < nt) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int sr = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const int ox = tx - ci[sr * 18], oy = ty - ci[sr * 18 + 9];
                        if ((unsigned)ox < (unsigned)OTF_WIN && (unsigned)oy < (unsigned)OTF_WIN)
                            win[sr * (OTF_WIN * OTF_WIN) + oy * OTF_WIN + ox] = acc[m][r] * 0.0625f;      // corr.py:58's 1 / sqrt(256), exact
                    }
            }
        };
        // a wave takes every fourth chunk; the next chunk's 16 fragment loads are in flight while this one's 32 MFMAs run (two register sets)
        if (wave * 32 < nt) {
            f16x8 bA[16], bB[16];
            int c0 = wave * 32, tyA, txA, tyB = 0, txB = 0;
            load_b(bA, target(c0, tyA, txA));
            for (;;) {
                const int c1 = c0 + 128;
                if (c1 < nt) load_b(bB, target(c1, tyB, txB));
                chunk(bA, c0, tyA, txA);
                if (c1 >= nt) break;
                c0 = c1 + 128;
                if (c0 < nt) load_b(bA, target(c0, tyA, txA));
                chunk(bB, c1, tyB, txB);
                if (c0 >= nt) break;
            }
        }
        __syncthreads();
        for (int v = t; v < 64 * 9; v += 256) {
            const int pr = v / 9, wi = v - pr * 9;
            const int py = ty0 + (pr >> 3), px = tx0 + (pr & 7);
            if (py >= h8 || px >= w8) continue;
            const int cb = pr * 18;
            int xo = ci[cb + wi] - ci[cb];
            const float ax = ca[cb + wi];
            xo = xo < 0 ? 0 : (xo > OTF_WIN - 2 ? OTF_WIN - 2 : xo);      // always in range (spread of the 9 floors <= 9); defensive
            const float *wp = win + pr * (OTF_WIN * OTF_WIN) + xo;
            f16 *dst = out + ((int64_t)n * P + (int64_t)py * w8 + px) * ldo + l * 81 + wi * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                int yo = ci[cb + 9 + j] - ci[cb + 9];
                const float ay = ca[cb + 9 + j];
                yo = yo < 0 ? 0 : (yo > OTF_WIN - 2 ? OTF_WIN - 2 : yo);
                const float v00 = wp[yo * OTF_WIN], v01 = wp[yo * OTF_WIN + 1];
                const float v10 = wp[yo * OTF_WIN + OTF_WIN], v11 = wp[yo * OTF_WIN + OTF_WIN + 1];
                const f16 o = (f16)(v00 * (1.f - ax) * (1.f - ay) + v01 * ax * (1.f - ay) + v10 * (1.f - ax) * ay + v11 * ax * ay);
                dst[j] = o;
                if (o8_off)      // fp8 copy after the row's fp16 part: the A operand of convc1's MX segment (gemm.h nk16)
                    ((unsigned char *)dst)[o8_off - (l * 81 + wi * 9) + j] = (unsigned char)pb_fp8x2((float)o * o8_scale, 0.f);
            }
        }
    }
}

int launch_corr_lookup_otf(hipStream_t s, const f16 *fmap_src, const f16 *const fmap_tgt[4], const int h[4], const int w[4], const float *flow, int P,
                           int w8, f16 *out, int64_t rows, int ldo, int o8_off, float o8_scale, int dirs) {
    PB_CHECK(rows < (1LL << 31) && P == h[0] * w[0] && w8 == w[0] && rows % P == 0 && dirs >= 0 && dirs <= 2, -1, "corr_lookup_otf: %lld rows of a %d x %d grid",
             (long long)rows, h[0], w[0]);
    PB_CHECK(h[3] >= 2 && w[3] >= 2, -1, "corr_lookup_otf: a %d x %d grid is too small for four levels", h[0], w[0]);
    OtfArgs g;
    g.src = fmap_src; g.dirs = dirs;
    for (int l = 0; l < 4; ++l) { g.tgt[l] = fmap_tgt[l]; g.h[l] = h[l]; g.w[l] = w[l]; }
    static PbLdsLimit lds;
    if (int rc = pb_lds_limit(lds, (const void *)corr_lookup_otf_kernel, OTF_SMEM)) return rc;
    const int nd = (int)(rows / P);
    PB_CHECK(nd <= 65535, -1, "corr_lookup_otf: %d pair-directions", nd);
    hipLaunchKernelGGL(corr_lookup_otf_kernel, dim3((unsigned)(((w8 + 7) / 8) * ((h[0] + 7) / 8)), (unsigned)nd), dim3(256), OTF_SMEM, s, g, flow, P, w8, out,
                       ldo, o8_off, o8_scale);
    LAUNCH_CHECK();
}
