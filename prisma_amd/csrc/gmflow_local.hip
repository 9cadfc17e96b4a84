// Local matching and local flow propagation of the flow_gmflow band (--corr_radius_list R, --prop_radius_list r).
// Reference being replaced: bands/gmflow/matching.py:39-83 (local_correlation_softmax) and transformer.py:376-409
// (FeatureFlowAttention.forward_local_window_attn).  Both are a softmax over the (2R + 1)^2 tokens around each token of the fp32 token-major
// maps the engine holds ([images, P, 128]); the work is P x (2R + 1)^2 fp32 dot products, bound by the maps' bytes, so plain FMA, no MFMA.
//
// One block = an 8 x 8 tile of query tokens, 256 threads = 64 queries x 4 candidate groups (lane = query * 4 + group; candidate j of a query
// belongs to group j & 3, so a query's softmax closes with two lane shuffles).  The tile's keys with their halo, (8 + 2R)^2 tokens, pass
// through the LDS in four slices of 32 channels (rows of 36 floats: consecutive tokens fall on distinct 16-byte slots), so a key row is
// fetched once per tile, not (2R + 1)^2 times.  A score is ONE chain of 128 FMAs in channel order, then one multiply by 1 / sqrt(128);
// expf is the library's (1 ulp).  Keys outside the grid are staged as zeros: their dot product is exactly 0.
//   * matching: those candidates get -1e9 as in the reference (probability exactly 0); flow = sum p (dx, dy) - the OFFSETS, which in exact
//     arithmetic equal the reference's sum p (x + dx, y + dy) - (x, y) without its cancellation at x ~ 180.  The reference gathers the window
//     with grid_sample(align_corners = True) at coordinates that are integers up to fp32 round-off; a plain gather restates it.
//   * propagation: F.unfold zero-pads, so a candidate outside the grid has score 0 and flow 0 and STILL counts in the softmax's denominator.
#include "gmflow_kernels.h"

namespace {

constexpr int kTile = 8;            // queries per tile edge
constexpr int kSlice = 32;          // channels per LDS slice
constexpr int kRow = kSlice + 4;    // LDS row stride in floats

template <int R> struct LocalGeom {
    static constexpr int W = 2 * R + 1, NC = W * W, NCG = (NC + 3) / 4, HT = kTile + 2 * R;
};

// acc[i] = <q, k_j> of this lane's query and its candidates j = group + 4 i (0 for a j >= NC, never read): qimg / kimg are one image's
// [P, 128] maps.  Every thread of the block must call it (barriers); queries of a tile's tail outside the grid read zeros.
template <int R>
__device__ __forceinline__ void local_scores(const float *__restrict__ qimg, const float *__restrict__ kimg, int h8, int w8, int ty0, int tx0,
                                             float *ktile, float *qtile, float (&acc)[LocalGeom<R>::NCG]) {
    using G = LocalGeom<R>;
    const int tid = threadIdx.x, q = tid >> 2, grp = tid & 3, ly = q >> 3, lx = q & 7;
    int koff[G::NCG];
#pragma unroll
    for (int i = 0; i < G::NCG; ++i) {
        const int j = grp + 4 * i;
        koff[i] = j < G::NC ? ((ly + j / G::W) * G::HT + lx + j % G::W) * kRow : 0;
        acc[i] = 0.f;
    }
    for (int s = 0; s < 128 / kSlice; ++s) {
        __syncthreads();
        for (int i = tid; i < G::HT * G::HT * (kSlice / 4); i += 256) {
            const int tok = i >> 3, c4 = i & 7, hy = tok / G::HT, hx = tok - hy * G::HT;
            const int gy = ty0 - R + hy, gx = tx0 - R + hx;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < h8 && gx >= 0 && gx < w8) v = *(const f32x4 *)(kimg + ((int64_t)gy * w8 + gx) * 128 + s * kSlice + c4 * 4);
            *(f32x4 *)(ktile + tok * kRow + c4 * 4) = v;
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = tid + it * 256, tok = i >> 3, c4 = i & 7;
            const int gy = ty0 + (tok >> 3), gx = tx0 + (tok & 7);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gy < h8 && gx < w8) v = *(const f32x4 *)(qimg + ((int64_t)gy * w8 + gx) * 128 + s * kSlice + c4 * 4);
            *(f32x4 *)(qtile + tok * kRow + c4 * 4) = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int c4 = 0; c4 < kSlice / 4; ++c4) {
            const f32x4 qv = *(const f32x4 *)(qtile + q * kRow + c4 * 4);
#pragma unroll
            for (int i = 0; i < G::NCG; ++i) {
                const f32x4 kv = *(const f32x4 *)(ktile + koff[i] + c4 * 4);
                acc[i] = fmaf(qv[0], kv[0], acc[i]); acc[i] = fmaf(qv[1], kv[1], acc[i]);
                acc[i] = fmaf(qv[2], kv[2], acc[i]); acc[i] = fmaf(qv[3], kv[3], acc[i]);
            }
        }
    }
}

__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    return fmaxf(v, __shfl_xor(v, 2));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 1);
    return v + __shfl_xor(v, 2);
}

// Batch element b = blockIdx.z: source image b * img_step of X [images, P, 128], target the other image of its pair (index ^ 1).
// flow [B, P, 2]; vt (may be null) = the global propagation's V^T [B, 2, 32, ldv] rows 0, 1 (hi) and 32, 33 (lo), as gm_match_flow_kernel writes it
template <int R>
__global__ __launch_bounds__(256) void gm_local_match_kernel(const float *__restrict__ X, float *__restrict__ flow, f16 *__restrict__ vt, int h8,
                                                             int w8, int img_step, int ldv) {
    using G = LocalGeom<R>;
    __shared__ __attribute__((aligned(16))) float ktile[G::HT * G::HT * kRow];
    __shared__ __attribute__((aligned(16))) float qtile[kTile * kTile * kRow];
    const int P = h8 * w8, b = blockIdx.z, src = b * img_step, ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
    float acc[G::NCG];
    local_scores<R>(X + (int64_t)src * P * 128, X + (int64_t)(src ^ 1) * P * 128, h8, w8, ty0, tx0, ktile, qtile, acc);
    const int q = threadIdx.x >> 2, grp = threadIdx.x & 3, qy = ty0 + (q >> 3), qx = tx0 + (q & 7);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < G::NCG; ++i) {
        const int j = grp + 4 * i, x = qx + j % G::W - R, y = qy + j / G::W - R;
        acc[i] = j >= G::NC ? -INFINITY : (x >= 0 && x < w8 && y >= 0 && y < h8 ? acc[i] * 0.088388347648318441f : -1e9f);
        m = fmaxf(m, acc[i]);
    }
    m = group_max(m);
    float l = 0.f, u = 0.f, v = 0.f;
#pragma unroll
    for (int i = 0; i < G::NCG; ++i) {
        const int j = grp + 4 * i;
        const float p = expf(acc[i] - m);
        l += p;
        u = fmaf(p, (float)(j % G::W - R), u);
        v = fmaf(p, (float)(j / G::W - R), v);
    }
    l = group_sum(l); u = group_sum(u); v = group_sum(v);
    if (grp || qy >= h8 || qx >= w8) return;
    u /= l; v /= l;
    const int t = qy * w8 + qx;
    const int64_t i = (int64_t)b * P + t;
    flow[i * 2] = u; flow[i * 2 + 1] = v;
    if (!vt) return;
    f16 *d = vt + (int64_t)b * 64 * ldv + t;
    const f16 uh = (f16)u, vh = (f16)v;
    d[0] = uh; d[ldv] = vh;
    d[32 * (int64_t)ldv] = (f16)(u - (float)uh); d[33 * (int64_t)ldv] = (f16)(v - (float)vh);
}

// Batch element b: query / key image b * img_step of Q / K [images, P, 128], flow_in [B, P, 2]; writes columns 0, 1 of O [B, P, 32], where
// gm_upsampler_in_kernel reads the propagated flow
template <int R>
__global__ __launch_bounds__(256) void gm_local_prop_kernel(const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ flow_in,
                                                            float *__restrict__ O, int h8, int w8, int img_step) {
    using G = LocalGeom<R>;
    __shared__ __attribute__((aligned(16))) float ktile[G::HT * G::HT * kRow];
    __shared__ __attribute__((aligned(16))) float qtile[kTile * kTile * kRow];
    const int P = h8 * w8, b = blockIdx.z, ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
    const int64_t img = (int64_t)b * img_step * P * 128;
    float acc[G::NCG];
    local_scores<R>(Q + img, K + img, h8, w8, ty0, tx0, ktile, qtile, acc);
    const int q = threadIdx.x >> 2, grp = threadIdx.x & 3, qy = ty0 + (q >> 3), qx = tx0 + (q & 7);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < G::NCG; ++i) {
        acc[i] = grp + 4 * i >= G::NC ? -INFINITY : acc[i] * 0.088388347648318441f;          // a zero pad keeps its score of exactly 0
        m = fmaxf(m, acc[i]);
    }
    m = group_max(m);
    float l = 0.f, u = 0.f, v = 0.f;
#pragma unroll
    for (int i = 0; i < G::NCG; ++i) {
        const int j = grp + 4 * i, x = qx + j % G::W - R, y = qy + j / G::W - R;
        const float p = expf(acc[i] - m);
        l += p;
        if (j < G::NC && x >= 0 && x < w8 && y >= 0 && y < h8) {
            const f32x2 f = *(const f32x2 *)(flow_in + ((int64_t)b * P + y * w8 + x) * 2);
            u = fmaf(p, f[0], u);
            v = fmaf(p, f[1], v);
        }
    }
    l = group_sum(l); u = group_sum(u); v = group_sum(v);
    if (grp || qy >= h8 || qx >= w8) return;
    float *o = O + ((int64_t)b * P + qy * w8 + qx) * 32;
    o[0] = u / l; o[1] = v / l;
}

inline dim3 tile_grid(int B, int h8, int w8) { return dim3((w8 + kTile - 1) / kTile, (h8 + kTile - 1) / kTile, B); }

}  // namespace

int launch_gm_local_match(hipStream_t s, const float *X, float *flow, f16 *vt, int B, int h8, int w8, int img_step, int radius, int ldv) {
    PB_CHECK(B > 0 && B <= 65535 && h8 > 0 && w8 > 0 && (img_step == 1 || img_step == 2), PB_ERR_ARG, "gm_local_match: B = %d, grid %d x %d", B, h8, w8);
    const dim3 grid = tile_grid(B, h8, w8);
#define GM_LM(R) hipLaunchKernelGGL(gm_local_match_kernel<R>, grid, dim3(256), 0, s, X, flow, vt, h8, w8, img_step, ldv)
    switch (radius) {
        case 1: GM_LM(1); break;
        case 2: GM_LM(2); break;
        case 3: GM_LM(3); break;
        case 4: GM_LM(4); break;
        default: PB_CHECK(false, PB_ERR_ARG, "gm_local_match: radius %d (1 .. 4)", radius);
    }
#undef GM_LM
    PB_HIP(hipGetLastError());
    return 0;
}

int launch_gm_local_prop(hipStream_t s, const float *q, const float *k, const float *flow_in, float *O, int B, int h8, int w8, int img_step,
                         int radius) {
    PB_CHECK(B > 0 && B <= 65535 && h8 > 0 && w8 > 0 && (img_step == 1 || img_step == 2), PB_ERR_ARG, "gm_local_prop: B = %d, grid %d x %d", B, h8, w8);
    const dim3 grid = tile_grid(B, h8, w8);
    switch (radius) {
        case 1: hipLaunchKernelGGL(gm_local_prop_kernel<1>, grid, dim3(256), 0, s, q, k, flow_in, O, h8, w8, img_step); break;
        case 2: hipLaunchKernelGGL(gm_local_prop_kernel<2>, grid, dim3(256), 0, s, q, k, flow_in, O, h8, w8, img_step); break;
        default: PB_CHECK(false, PB_ERR_ARG, "gm_local_prop: radius %d (1 .. 2)", radius);
    }
    PB_HIP(hipGetLastError());
    return 0;
}
