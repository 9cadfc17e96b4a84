// FlowEngine: what the flow_raft and flow_gmflow bands share (flow_engine.h) - host code only, the kernels are raft_kernels.hip's.
#include "flow_engine.h"
#include "flow_chunk.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace {
void cubic_taps_u8(int src, int dst, double scale, std::vector<int> &idx, std::vector<int> &co) {
    // OpenCV 8-bit INTER_CUBIC: float32 coefficients (A = -0.75) -> saturate_cast<short>(c * 2048)
    idx.resize((size_t)dst * 4);
    co.resize((size_t)dst * 4);
    const double inv = 1.0 / scale;
    const float A = -0.75f;
    for (int d = 0; d < dst; ++d) {
        float fx = (float)((d + 0.5) * inv - 0.5);
        const int sx = (int)floorf(fx);
        fx -= (float)sx;
        float c[4];
        c[0] = ((A * (fx + 1.f) - 5.f * A) * (fx + 1.f) + 8.f * A) * (fx + 1.f) - 4.f * A;
        c[1] = ((A + 2.f) * fx - (A + 3.f)) * fx * fx + 1.f;
        c[2] = ((A + 2.f) * (1.f - fx) - (A + 3.f)) * (1.f - fx) * (1.f - fx) + 1.f;
        c[3] = 1.f - c[0] - c[1] - c[2];
        for (int t = 0; t < 4; ++t) {
            idx[(size_t)d * 4 + t] = std::min(std::max(sx - 1 + t, 0), src - 1);
            co[(size_t)d * 4 + t] = (int)nearbyint((double)c[t] * 2048.0);
        }
    }
}
}  // namespace

// The tap table of one axis as upload_resize_tables builds it, with external linkage (as pb_cubic_taps, engine.hip): pb_op_flow_prep and
// pb_op_flow_taps hand the tests the table the engines upload.  scale: the call's float, taken through flow_scale_exact (flow_chunk.h)
void pb_flow_cubic_taps(int src, int dst, float scale, std::vector<int> &idx, std::vector<int> &co) {
    cubic_taps_u8(src, dst, flow_scale_exact(scale), idx, co);
}

void FlowEngine::out_size(int H, int W, float scale, int *sh, int *sw) {
    const FlowGeometry g = flow_geometry(H, W, scale, 8);
    *sh = g.sh; *sw = g.sw;
}

void FlowEngine::geometry(int H, int W, float scale, int factor) {
    const FlowGeometry g = flow_geometry(H, W, scale, factor);
    sh_ = g.sh; sw_ = g.sw; Hp_ = g.Hp; Wp_ = g.Wp; padl_ = g.padl; padt_ = g.padt; h8_ = g.h8; w8_ = g.w8; P_ = g.P;
}

// BasicEncoder weights (extractor.py:118-192) up to the last residual block: stem, layer1-3, downsample paths.  bnf: eval BatchNorm folded
// into the convolutions (cnet); conv_bias: the 3x3 / 7x7 convolutions carry biases (RAFT yes, GMFlow's CNNEncoder no - its 1x1 downsample
// convolutions do, backbone.py:22-25)
int FlowEngine::pack_encoder(const std::string &en, bool bnf, bool conv_bias, Enc &E) {
    int r;
    const int dims[3] = {64, 96, 128};
    std::vector<float> sc, sf;
    {   // stem 7x7 / stride 2 (extractor.py:124,171): on the 4 x 4 space-to-depth image (64 channels = (dy, dx, c), raft_prep) it is a
        // 3x3 / stride 1 convolution whose 4 x 64 output channels are the 2 x 2 output pixels of a block - an implicit GEMM on the
        // ping-pong kernel with the pixel-shuffle epilogue instead of an im2col round trip (2.8 GB per 32 frames at 1080p x 0.75).
        // W2[(sy, sx, o)][(ty, tx)][(dy, dx, c)] = w[o][c][ky][kx],  ky = 4 (ty - 1) + dy - 2 sy + 3 (same in x), zero outside 0..6
        auto iw = tmap_.find(en + ".conv1.weight"), ib = tmap_.find(en + ".conv1.bias");
        PB_CHECK(iw != tmap_.end() && (ib != tmap_.end() || !conv_bias), PB_ERR_ARG, "missing %s.conv1", en.c_str());
        if (bnf && (r = fold_bn(en + ".norm1", 64, sc, sf))) return r;
        const float *wt = (const float *)iw->second->data, *bs = conv_bias ? (const float *)ib->second->data : nullptr;
        std::vector<float> g((size_t)256 * 576, 0.f), bb(256);
        for (int sy = 0; sy < 2; ++sy)
            for (int sx = 0; sx < 2; ++sx)
                for (int o = 0; o < 64; ++o) {
                    const float s = bnf ? sc[o] : 1.f;
                    const int n = (sy * 2 + sx) * 64 + o;
                    bb[n] = (bs ? bs[o] : 0.f) * s + (bnf ? sf[o] : 0.f);
                    for (int ty = 0; ty < 3; ++ty)
                        for (int tx = 0; tx < 3; ++tx)
                            for (int dy = 0; dy < 4; ++dy)
                                for (int dx = 0; dx < 4; ++dx) {
                                    const int ky = 4 * (ty - 1) + dy - 2 * sy + 3, kx = 4 * (tx - 1) + dx - 2 * sx + 3;
                                    if (ky < 0 || ky > 6 || kx < 0 || kx > 6) continue;
                                    for (int c = 0; c < 3; ++c)
                                        g[(size_t)n * 576 + (ty * 3 + tx) * 64 + (dy * 4 + dx) * 4 + c] = wt[((size_t)o * 3 + c) * 49 + ky * 7 + kx] * s;
                                }
                }
        if ((r = pack(g.data(), 256, 576, 576, E.stem, bb.data(), 9, 1))) return r;
        E.stem.Kreal = 147;
    }
    for (int li = 0; li < 3; ++li)
        for (int bi = 0; bi < 2; ++bi) {
            const std::string p = en + ".layer" + std::to_string(li + 1) + "." + std::to_string(bi);
            for (int c = 0; c < 2; ++c) {
                if (bnf && (r = fold_bn(p + ".norm" + std::to_string(c + 1), dims[li], sc, sf))) return r;
                if ((r = pack_conv(p + ".conv" + std::to_string(c + 1), conv_bias, bnf ? sc.data() : nullptr, bnf ? sf.data() : nullptr,
                                   E.l[li][bi][c], 1)))
                    return r;
            }
            if (bi == 0 && li > 0) {
                if (bnf && (r = fold_bn(p + ".norm3", dims[li], sc, sf))) return r;
                if ((r = pack_conv(p + ".downsample.0", true, bnf ? sc.data() : nullptr, bnf ? sf.data() : nullptr, E.ds[li], 1))) return r;
            }
        }
    return 0;
}

void FlowEngine::carve_encoder(int F) {
    const int h2 = Hp_ / 2, w2 = Wp_ / 2, h4 = Hp_ / 4, w4 = Wp_ / 4;
    xi_ = (int *)carve((size_t)sw_ * 16); xc_ = (int *)carve((size_t)sw_ * 16);
    yi_ = (int *)carve((size_t)sh_ * 16); yc_ = (int *)carve((size_t)sh_ * 16);
    // split-fp16 mode: the encoders' maps (image included) are [hi | lo] per pixel (es = 2)
    const size_t es = split_w_ ? 2 : 1;
    img_ = (f16 *)carve((size_t)F * Hp_ * Wp_ * 8 * es);
    for (auto &b : r1_) b = (f16 *)carve((size_t)round_up((int64_t)F * h2 * w2, 256) * 64 * 2 * es);
    for (auto &b : r2_) b = (f16 *)carve((size_t)round_up((int64_t)F * h4 * w4, 256) * 128 * 2 * es);
    for (auto &b : r3_) b = (f16 *)carve((size_t)round_up((int64_t)F * (enc_s3_ == 1 ? h4 * w4 : P_), 256) * 128 * 2 * es);
    for (auto &b : st_) b = (float *)carve((size_t)F * 256 * 2 * 4);
    stp_ = (float *)carve((size_t)in_stats_chunks(h2 * w2) * F * 256 * 2 * 4);     // per-chunk partial sums of the largest map
}

int FlowEngine::upload_resize_tables(int H, int W, float scale) {
    if (scale != 1.f) {
        std::vector<int> xi, xc, yi, yc;
        pb_flow_cubic_taps(W, sw_, scale, xi, xc);
        pb_flow_cubic_taps(H, sh_, scale, yi, yc);
        PB_HIP(hipMemcpyAsync(xi_, xi.data(), xi.size() * 4, hipMemcpyHostToDevice, stream));
        PB_HIP(hipMemcpyAsync(xc_, xc.data(), xc.size() * 4, hipMemcpyHostToDevice, stream));
        PB_HIP(hipMemcpyAsync(yi_, yi.data(), yi.size() * 4, hipMemcpyHostToDevice, stream));
        PB_HIP(hipMemcpyAsync(yc_, yc.data(), yc.size() * 4, hipMemcpyHostToDevice, stream));
    }
    PB_HIP(hipStreamSynchronize(stream));
    return 0;
}

int FlowEngine::prep_frames(const uint8_t *frames, int F, int H, int W, float scale, int lo8, int norm, int isz) {
    return timed(F_PP, 0, (double)F * H * W * 3, [&] {
        return launch_raft_prep(stream, frames, F, H, W, sh_, sw_, Hp_, Wp_, padl_, padt_, scale != 1.f, xi_, xc_, yi_, yc_, img_, nullptr, 1,
                                split_w_ ? 64 : 0, lo8, norm, isz);
    });
}

// BasicEncoder.forward (extractor.py:171-192) without its last 1x1 convolution, on the F prepared frames in img_: stem, three stages of two
// residual blocks.  inorm: InstanceNorm with run-time statistics (fnet; GMFlow's backbone) - otherwise the folded BatchNorm path (cnet).
// *x_out = the last block's output map [F, h8, w8, 128] (split-fp16 layout in PB_PREC_SPLIT); with enc_s3_ = 1 [F, Hp / 4, Wp / 4, 128].
int FlowEngine::run_encoder(const Enc &E, bool inorm, int F, const f16 **x_out) {
    int r = 0;
    const int h2 = Hp_ / 2, w2 = Wp_ / 2;
    const int es = split_w_ ? 2 : 1;                         // encoder maps are [hi | lo] in split-fp16 mode
    auto lo = [&](int c) { return split_w_ ? c : 0; };
    const int l8 = split_w_ && mx_ ? kLo8Pa : -1;            // the residual parts of the encoder maps are e4m3 ([hi | hi8 | lo8])
    auto norm_relu = [&](const f16 *t, float *st, f16 *y, int HW, int C, const f16 *b, const float *sb) -> int {
        return timed(F_ELT, 0, 0, [&] { return launch_in_apply(stream, t, st, b, sb, y, F, HW, C, es * C, lo(C), l8); });
    };
    // On the e4m3-residual maps (flow_raft) the instance-norm statistics are taken from the hi parts alone (PB_IN_STATS_LO=1: from hi + lo8
    // as before): the fp16 rounding residuals are symmetric around zero, so over a channel's pixels they move the mean by ~2^-12 / sqrt(n) of a
    // value, and a 64-channel pixel's hi part is one of its two 128-byte lines (the lo8 bytes sit in the other one): half the pass's traffic,
    // -1.2 ms per step, RAFT parity unchanged (worst 720p pair 6.0e-4 either way).  flow_gmflow (fp16 residual planes) keeps hi + lo: its
    // 216x300 vector moves from 2.2e-4 to 3.8e-4 without them.
    const bool stats_lo = launch_env().in_stats_lo || !mx_;
    auto stats = [&](const f16 *t, float *st, int HW, int C) -> int {
        return timed(F_ELT, 0, 0, [&] { return launch_in_stats(stream, t, F, HW, C, es * C, stp_, st, stats_lo ? lo(C) : 0, l8); });
    };
    // stem (BasicEncoder.forward, extractor.py:171-192)
    {
        GemmArgs a;
        a.A = img_; a.N = 256;
        a.cH = Hp_ / 4; a.cW = Wp_ / 4; a.cC = 64; a.cLd = es * 64; a.cKW = 3; a.cStride = 1; a.cPad = 1; a.cPadX = 1;
        set_weights(a, E.stem, true);
        a.cOH = a.cH; a.cOW = a.cW; a.M = F * a.cH * a.cW;
        a.out = r1_[5]; a.ldo = es * 64; a.lo_off = lo(64); a.act = inorm ? ACT_NONE : ACT_RELU;
        if (l8 >= 0) { a.lo8 = 1; a.lo8_pa = l8; }
        a.ps_h = a.cH; a.ps_w = a.cW; a.ps_s = 2; a.ps_co = 64;
        r = timed_gemm(F_CONV, 2.0 * F * h2 * w2 * 64.0 * 147, 0, [&] { return launch_gemm(stream, A_CONV, EPI_PIXSHUF, TILE_AUTO, a); },
                       E.stem.mx3 ? 2.0 : 1.0 + E.stem.sa + E.stem.sw);
        if (r) return r;
    }
    const f16 *x = r1_[5];
    if (inorm) {
        if ((r = stats(r1_[5], st_[0], h2 * w2, 64))) return r;
        if ((r = norm_relu(r1_[5], st_[0], r1_[6], h2 * w2, 64, nullptr, nullptr))) return r;
        x = r1_[6];
    }
    int H_ = h2, W_ = w2, C_ = 64;
    for (int li = 0; li < 3; ++li) {
        const int stride = li == 0 ? 1 : (li == 2 ? enc_s3_ : 2);
        const int Cn = li == 0 ? 64 : 128;               // 96 is carried as 128 (zero padded channels)
        f16 **R = li == 0 ? r1_ : (li == 1 ? r2_ : r3_);
        for (int bi = 0; bi < 2; ++bi) {                  // ResidualBlock.forward (extractor.py:46-56)
            const int s = bi == 0 ? stride : 1;
            const bool ds = bi == 0 && li > 0;            // the block changes stride or channel count: 1 x 1 convolution + norm on the skip path
            const int OH = (H_ - 1) / s + 1, OW = (W_ - 1) / s + 1;
            const int Cin = bi == 0 ? C_ : Cn;
            f16 *t1 = R[0], *t2 = R[1], *t3 = R[2], *outb = R[3 + bi];
            if (inorm) {
                if ((r = conv(x, Cin, es * Cin, F, H_, W_, 3, 3, s, E.l[li][bi][0], t1, es * Cn, ACT_NONE, 0, nullptr, nullptr, lo(Cn)))) return r;
                if ((r = stats(t1, st_[0], OH * OW, Cn))) return r;
                if ((r = norm_relu(t1, st_[0], t1, OH * OW, Cn, nullptr, nullptr))) return r;
                if ((r = conv(t1, Cn, es * Cn, F, OH, OW, 3, 3, 1, E.l[li][bi][1], t2, es * Cn, ACT_NONE, 0, nullptr, nullptr, lo(Cn)))) return r;
                if ((r = stats(t2, st_[1], OH * OW, Cn))) return r;
                if (ds) {
                    if ((r = conv(x, Cin, es * Cin, F, H_, W_, 1, 1, s, E.ds[li], t3, es * Cn, ACT_NONE, 0, nullptr, nullptr, lo(Cn)))) return r;
                    if ((r = stats(t3, st_[2], OH * OW, Cn))) return r;
                    if ((r = norm_relu(t2, st_[1], outb, OH * OW, Cn, t3, st_[2]))) return r;
                } else {
                    if ((r = norm_relu(t2, st_[1], outb, OH * OW, Cn, x, nullptr))) return r;
                }
            } else {
                if ((r = conv(x, Cin, es * Cin, F, H_, W_, 3, 3, s, E.l[li][bi][0], t1, es * Cn, ACT_RELU, 0, nullptr, nullptr, lo(Cn)))) return r;
                const f16 *xs = x;
                if (ds) {
                    if ((r = conv(x, Cin, es * Cin, F, H_, W_, 1, 1, s, E.ds[li], t3, es * Cn, ACT_NONE, 0, nullptr, nullptr, lo(Cn)))) return r;
                    xs = t3;
                }
                if ((r = conv(t1, Cn, es * Cn, F, OH, OW, 3, 3, 1, E.l[li][bi][1], outb, es * Cn, ACT_RELU, 1, xs, nullptr, lo(Cn)))) return r;
            }
            x = outb; H_ = OH; W_ = OW; C_ = Cn;
        }
    }
    *x_out = x;
    return 0;
}

int FlowEngine::flow_tail(const float *flow_lo, int N, int pairs, int hu, int wu, int factor, float *flow_out, uint8_t *rgb_out, float *maxdisp,
                          uint8_t *mask_out, float alpha1, float alpha2, float *upi) {
    float *up = flow_out ? flow_out : up_;
    int r = timed(F_PP, 0, (double)N * sh_ * sw_ * 8, [&] {
        if (!upi) return launch_upsample(stream, flow_lo, mask_, N, hu, wu, padl_, padt_, sh_, sw_, up, maxd_, factor);
        // convex upsampling at the inference size, then the bilinear resize back to the scaled frame
        const int rc = launch_upsample(stream, flow_lo, mask_, N, hu, wu, 0, 0, Hp_, Wp_, upi, maxd_, factor);
        return rc ? rc : launch_flow_resize_back(stream, upi, N, Hp_, Wp_, sh_, sw_, up, maxd_);
    });
    if (r) return r;
    r = timed(F_PP, 0, (double)N * sh_ * sw_ * 11, [&] { return launch_flow_encode(stream, up, N, sh_, sw_, maxd_, rgb_out, maxdisp); });
    if (r || !mask_out) return r;
    return timed(F_PP, 0, (double)N * sh_ * sw_ * 17, [&] { return launch_fwdbwd_mask(stream, up, pairs, sh_, sw_, alpha1, alpha2, mask_out); });
}
