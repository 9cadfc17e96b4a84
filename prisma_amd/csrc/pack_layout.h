// Host images of the packed GEMM weights (gemm.h W): the fp16, split-fp16, mx2 and mx3 layouts of a K axis, the e4m3 encoder of their residual
// parts and the slice-major K order.  Plain C++ without a HIP call - EngineBase::pack_spec (engine_base.hip) uploads what pack_rows builds,
// and tests/test_pack_layout_cpu.py compiles this very text on the host and holds every byte against a numpy restatement.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

typedef _Float16 f16;

struct PackedW {
    f16 *w = nullptr;        // [Npad, K] fp16, K % 64 == 0
    float *bias = nullptr;   // [Npad] fp32 (zero padded) or null
    int N = 0, K = 0, Kreal = 0;
    int Nreal = 0;           // output columns that are the layer's own when N holds padding rows (RAFT's motion conv: 126 of 128); 0 = N.  Only the FLOP / byte counters read it
    // split-fp16 packing (gemm.h kwrap): per tap the K axis holds the segments [w_hi | w_hi (if sa) | w_lo (if sw)] of Cseg
    // channels each; the activation operand must then be [hi | lo (if sa)] with Cseg channels per part
    int sa = 0, sw = 0, Cseg = 0;
    // MX-fp8 correction (gemm.h nk16): rows are [w_hi fp16 (Kin) | w_lo e4m3 (Kin bytes, scaled by 2^mx_pw)]; K counts 64-half units of the row.
    // nk16 on a weight that is neither mx2 nor mx3 (every K tile an fp16 tile) only selects the MX build of the kernel, for its fp8 output copy
    int nk16 = 0, mx_pw = 0;
    // mx3: weights AND activations split with e4m3 residual parts: per tap [w_hi fp16 (Cseg) | w_lo8 (Cseg bytes) | w_hi8 (Cseg bytes)]
    // = 2 Cseg halfs, meeting a split map's [hi | hi8 | lo8] pixel (gemm.h mx_period, lo8); K = taps x 2 Cseg
    int mx3 = 0;
    int mx2 = 0;             // weights-only split with the residual as e4m3: per tap [w_hi fp16 (Cseg) | w_lo8 (Cseg bytes)] = 1.5 Cseg halfs
    // conv weights in slice-major K order (gemm.h cTapInner): the (taps x K / (64 taps)) grid of 128-byte blocks of every row, transposed
    int tapin = 0, taps = 1;
    // packed-channel copy (gemm.h Wcw, conv_walk.h conv_cw3_word): mx3 convolution weights whose Cseg input channels hold cwC < Cseg real ones, with a K axis
    // that lists only those - read by the 128 x 96 tile's chunk walk (EngineBase::pack_conv builds it for 64 < N <= 96)
    f16 *wcw = nullptr;
    int Kcw = 0, nk16cw = 0, cwC = 0;
};

// What pack_rows lays out.  sa: the activation operand is a split map [hi | lo], so w_hi is stored twice; sw: the weights' fp16 rounding residual
// follows as a segment of its own; mx: with sa AND sw the residual parts are e4m3 (the mx3 layout); mx2: weights-only split with an e4m3 residual
// (needs sw, no sa, channels per tap % 128 == 0); tapin: convolution rows (taps > 1, channels per tap % 64 == 0) go slice-major
struct PackSpec {
    int sa = 0, sw = 0, mx = 0, mx2 = 0, tapin = 0;
};

// OCP e4m3fn, round to nearest even, saturating at +-448 (NaN -> 0x7F)
inline unsigned char pb_f32_to_e4m3(float x) {
    const unsigned char s = std::signbit(x) ? 0x80 : 0x00;       // (-0 keeps its sign, as the device's conversion and torch's cast do)
    const float a = fabsf(x);
    if (!(a == a)) return 0x7F;
    if (a >= 448.f) return s | 0x7E;
    int e;
    const float m = frexpf(a, &e);                  // a = m 2^e, m in [0.5, 1)
    int E = e - 1;                                  // a = (2 m) 2^E
    if (a == 0.f || E < -6) {                       // subnormal range: multiples of 2^-9
        const int q = (int)nearbyintf(a * 512.f);
        return s | (unsigned char)(q >= 8 ? 0x08 : q);
    }
    int q = (int)nearbyintf((2.f * m - 1.f) * 8.f);
    if (q == 8) { q = 0; ++E; }
    unsigned char code = (unsigned char)(((E + 7) << 3) | q);
    if (E > 8 || code > 0x7E) code = 0x7E;
    return s | code;
}

// slice-major K order of packed conv weights (gemm.h cTapInner): every row of `rowlen` halfs is a (taps x S) grid of 128-byte blocks; transposed in place
inline void pb_rows_slice_major(f16 *rows, int64_t nrows, int64_t rowlen, int taps) {
    const int64_t S = rowlen / (64 * (int64_t)taps);
    std::vector<f16> row((size_t)rowlen);
    for (int64_t n = 0; n < nrows; ++n) {
        f16 *r = rows + n * rowlen;
        for (int t = 0; t < taps; ++t)
            for (int64_t sidx = 0; sidx < S; ++sidx) std::copy_n(r + ((int64_t)t * S + sidx) * 64, 64, row.data() + (sidx * taps + t) * 64);
        std::copy_n(row.data(), (size_t)rowlen, r);
    }
}

// power-of-two storage scale of a weight's e4m3 parts: max |w - fp16(w)| 2^pw in [128, 256), and where w_hi is stored too (mx3, at 2^(pw - 12))
// max |w| 2^(pw - 12) < 256 as well; 0 for an all-zero residual
inline int pb_weight_pw(const float *w, int64_t n, bool with_hi) {
    float mlo = 0.f, mhi = 0.f;
    for (int64_t i = 0; i < n; ++i) {
        mhi = fmaxf(mhi, fabsf(w[i]));
        mlo = fmaxf(mlo, fabsf(w[i] - (float)(f16)w[i]));
    }
    int pw = 0, e = 0;
    if (mlo > 0.f) { frexpf(mlo, &e); pw = 8 - e; }
    if (with_hi && mhi > 0.f) { frexpf(mhi, &e); pw = std::min(pw, 20 - e); }
    return pw;
}

// the e4m3 parts of one weight at the scales of pb_weight_pw: its fp16 rounding residual, and its fp16 value (mx3)
inline unsigned char pb_w_lo8(float v, f16 hi, int pw) { return pb_f32_to_e4m3(ldexpf(v - (float)hi, pw)); }      // (v - hi is exact in fp32)
inline unsigned char pb_w_hi8(f16 hi, int pw) { return pb_f32_to_e4m3(ldexpf((float)hi, pw - 12)); }

// conv weight [co, ci, taps] (PyTorch's [co, ci, kh, kw]) -> GEMM rows [co][tap * cip + c], zero padded, optional per-output scale
inline std::vector<float> pb_conv_rows(const float *w, int co, int ci, int taps, int cip, const float *scale = nullptr) {
    std::vector<float> g((size_t)co * taps * cip, 0.f);
    for (int o = 0; o < co; ++o) {
        const float s = scale ? scale[o] : 1.f;
        for (int c = 0; c < ci; ++c)
            for (int t = 0; t < taps; ++t) g[((size_t)o * taps + t) * cip + c] = w[((size_t)o * ci + c) * taps + t] * s;
    }
    return g;
}

// LayerScale (layer_scale.py:27-28) folded into a linear layer: x + g (W y + b) = x + (g.W) y + g.b, so the GEMM can accumulate straight onto the
// residual stream (gemm.h EPI_RESID).  wt [N, K], bs / g [N] -> ws [N, K], bb [N]
inline void pb_fold_layerscale(const float *wt, const float *bs, const float *g, int N, int K, std::vector<float> &ws, std::vector<float> &bb) {
    ws.resize((size_t)N * K); bb.resize(N);
    for (int n = 0; n < N; ++n) {
        for (int k = 0; k < K; ++k) ws[(size_t)n * K + k] = wt[(size_t)n * K + k] * g[n];
        bb[n] = bs[n] * g[n];
    }
}

// src: host fp32 [N, K] in GEMM order, K = taps x channels -> rows [round_up(N, 256), out.K] fp16 and the metadata of `out` (every field but
// the device pointers).  Every tap is padded to Kpad / taps channels Cp and becomes, by layout,
//   fp16 / split-fp16   [w_hi | w_hi (sa) | w_lo (sw)]                      (1 + sa + sw) Cp halfs
//   mx2                 [w_hi | w_lo8 (Cp bytes)]                           1.5 Cp halfs
//   mx3                 [w_hi | w_lo8 (Cp bytes) | w_hi8 (Cp bytes)]        2 Cp halfs
// (a K that does not divide into taps is one tap, plain fp16 only).  An empty vector: the sizes do not fit the layout.
inline std::vector<f16> pack_rows(const float *src, int N, int K, int Kpad, int taps, const PackSpec &spec, PackedW &out) {
    const bool per_tap = taps > 0 && K % taps == 0 && Kpad % taps == 0;
    const int tp = per_tap ? taps : 1, Cin = K / tp, Cp = Kpad / tp;
    const int sa = spec.sa ? 1 : 0, sw = spec.sw ? 1 : 0;
    const bool mx3 = spec.mx && sa && sw, mx2 = spec.mx2 != 0, split = sa || sw;
    if (N <= 0 || Cp < Cin || (split && (!per_tap || Cp % 64)) || (mx2 && (sa || !sw || Cp % 128))) return {};
    const int tapin = spec.tapin && taps > 1 && Kpad % (64 * taps) == 0 ? 1 : 0;
    const int pw = mx3 || mx2 ? pb_weight_pw(src, (int64_t)N * K, mx3) : 0;
    const int64_t Np = (N + 255) / 256 * 256, tapw = mx3 ? 2 * Cp : (mx2 ? Cp + Cp / 2 : (1 + sa + sw) * Cp), Kt = tp * tapw;
    std::vector<f16> h((size_t)Np * Kt, (f16)0.f);
    for (int n = 0; n < N; ++n)
        for (int t = 0; t < tp; ++t) {
            const float *s = src + (int64_t)n * K + (int64_t)t * Cin;
            f16 *d = h.data() + n * Kt + t * tapw;
            unsigned char *d8 = (unsigned char *)(d + Cp);
            for (int k = 0; k < Cin; ++k) {
                const f16 hi = (f16)s[k];
                d[k] = hi;
                if (mx3 || mx2) {
                    d8[k] = pb_w_lo8(s[k], hi, pw);
                    if (mx3) d8[Cp + k] = pb_w_hi8(hi, pw);
                } else {
                    if (sa) d[Cp + k] = hi;
                    if (sw) d[(1 + sa) * Cp + k] = (f16)(s[k] - (float)hi);
                }
            }
        }
    if (tapin) pb_rows_slice_major(h.data(), Np, Kt, taps);
    out.N = N; out.K = (int)Kt; out.Kreal = K; out.Cseg = Cp; out.tapin = tapin; out.taps = taps;
    out.sa = mx2 ? 0 : sa; out.sw = sw; out.mx2 = mx2; out.mx3 = mx3; out.mx_pw = pw; out.nk16 = mx3 || mx2 ? Cp / 64 : 0;
    return h;
}
