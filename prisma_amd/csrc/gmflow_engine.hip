// GmflowEngine: the flow_gmflow band on one MI355X.
// Reference call stack being replaced: bands/flow_gmflow.py:134-157 (frame loop: cv2.resize(fx = fy = scale, INTER_CUBIC)) -> :66-118
// infer (InputPadder(padding_factor = 16), GMFlow(...), unpad) -> bands/gmflow/gmflow.py:95-170 -> backbone.py:56-117 (CNNEncoder),
// utils.py:53-86 (normalise, per-window sine positions), transformer.py:108-290 (6 x [self-attention, cross-attention + FFN] over
// 2 x 2 shifted windows), matching.py:7-42 (global correlation softmax), transformer.py:300-337 (flow propagation), gmflow.py:74-92
// (convex upsampling) -> bands/common/flow.py:64-88 + encode.py:98-126 (process_flow).
//
// Schedule, not arithmetic:
//   * every frame passes the backbone once per sequence (the reference encodes both frames of every pair);
//   * the token stream [pairs, 2 frames, P, 128] is fp32; what enters a block's cross attention as `target` is the OTHER frame's stream
//     as it entered the block (transformer.py:286-288), so all five projections that read the entering stream (q, k, v of the self
//     attention; k, v of the cross attention) are ONE GEMM with N = 640, and the cross attention reads the partner frame's windows
//     through the attention kernel's batch-index xor (attention128.hip kxor) - nothing is concatenated or swapped in memory;
//   * window split / roll / merge (transformer.py:47-101) are index maps inside the pack and LayerNorm kernels (gmflow_kernels.hip);
//   * global matching and propagation are the same flash-style attention with V = pixel coordinates / flow padded to 32 columns: the
//     P x P correlation volume (2.7 GB fp32 per pair at 1080p x 0.75) never exists;
//   * PB_PREC_SPLIT: every MFMA operand is a hi + lo fp16 pair (GEMMs: three K segments; attention: three passes for S and for P V) -
//     this network's two softmax stages amplify operand rounding several times more than RAFT does.
#include "gmflow_engine.h"
#include "flow_chunk.h"

#include <math.h>
#include <string.h>

#include <algorithm>

int GmflowEngine::upload(const std::string &name, int n, float **dst) {
    const pb_tensor *t = find(name);
    PB_CHECK(t && t->shape[0] == n, PB_ERR_ARG, "missing weight '%s' [%d]", name.c_str(), n);
    void *p = nullptr;
    PB_HIP(hipMalloc(&p, (size_t)n * 4));
    owned_.push_back(p);
    PB_HIP(hipMemcpy(p, t->data, (size_t)n * 4, hipMemcpyHostToDevice));
    *dst = (float *)p;
    return 0;
}

int GmflowEngine::load(const pb_tensor *w, int n) {
    int r = begin_load(w, n);
    if (r) return r;
    mx_ = 0;                                    // fp16 residual parts everywhere: activations AND weights split, three K segments
    pack_tapin_ = 0;
    {   // the architecture comes from the weights: the two-scale model (gmflow_with_refine: num_scales 2, upsample_factor 4) carries the
        // backbone's trident convolution and an upsampler of 4 * 4 * 9 logits, the one-scale model neither
        const pb_tensor *tri = find("backbone.trident_conv.weight"), *u2 = find("upsampler.2.weight");
        PB_CHECK(u2 && u2->ndim == 4, PB_ERR_ARG, "missing conv 'upsampler.2'");
        const int rows = (int)u2->shape[0];
        if (tri) {
            PB_CHECK(tri->ndim == 4 && tri->shape[0] == 128 && tri->shape[1] == 128 && tri->shape[2] == 3 && tri->shape[3] == 3, PB_ERR_ARG,
                     "flow_gmflow: 'backbone.trident_conv.weight' must be [128, 128, 3, 3] (the two-scale model's shared 3 x 3 convolution)");
            PB_CHECK(rows == 144, PB_ERR_ARG, "flow_gmflow: 'upsampler.2.weight' has %d rows; with 'backbone.trident_conv.weight' (two scales) it has 4 * 4 * 9 = 144", rows);
        } else {
            PB_CHECK(rows == 576, PB_ERR_ARG, "flow_gmflow: 'upsampler.2.weight' has %d rows; without 'backbone.trident_conv.weight' (one scale) it has 8 * 8 * 9 = 576", rows);
        }
        scales_ = tri ? 2 : 1;
        enc_s3_ = tri ? 1 : 2;
    }
    if ((r = pack_encoder("backbone", false, false, backbone_))) return r;
    if ((r = pack_conv("backbone.conv2", true, nullptr, nullptr, backbone_.out, 1))) return r;
    if (scales_ == 2 && (r = pack_conv("backbone.trident_conv", false, nullptr, nullptr, trident_, 1))) return r;
    auto lin = [&](const std::string &name, int N, int K, PackedW &out, bool bias) -> int {
        const pb_tensor *t = find(name + ".weight");
        PB_CHECK(t && t->ndim == 2 && t->shape[0] == N && t->shape[1] == K, PB_ERR_ARG, "missing linear '%s' [%d, %d]", name.c_str(), N, K);
        const float *b = nullptr;
        if (bias) {
            const pb_tensor *tb = find(name + ".bias");
            PB_CHECK(tb && tb->shape[0] == N, PB_ERR_ARG, "missing bias of '%s'", name.c_str());
            b = (const float *)tb->data;
        }
        return pack((const float *)t->data, N, K, K, out, b, 1, 1);
    };
    for (int i = 0; i < 6; ++i) {
        Layer &L = layers_[i];
        const std::string p = "transformer.layers." + std::to_string(i) + ".", s = p + "self_attn.", c = p + "cross_attn_ffn.";
        std::vector<float> w1((size_t)640 * 128);
        const char *parts[5] = {"q_proj", "k_proj", "v_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 5; ++j) {
            const std::string nm = (j < 3 ? s : c) + parts[j] + ".weight";
            const pb_tensor *t = find(nm);
            PB_CHECK(t && t->ndim == 2 && t->shape[0] == 128 && t->shape[1] == 128, PB_ERR_ARG, "missing linear '%s' [128, 128]", nm.c_str());
            memcpy(w1.data() + (size_t)j * 128 * 128, t->data, (size_t)128 * 128 * 4);
        }
        if ((r = pack(w1.data(), 640, 128, 128, L.w1, nullptr, 1, 1))) return r;
        if ((r = lin(s + "merge", 128, 128, L.merge_s, false))) return r;
        if ((r = lin(c + "q_proj", 128, 128, L.q_c, false))) return r;
        if ((r = lin(c + "merge", 128, 128, L.merge_c, false))) return r;
        if ((r = lin(c + "mlp.0", 1024, 256, L.mlp0, false))) return r;
        if ((r = lin(c + "mlp.2", 128, 1024, L.mlp2, false))) return r;
        if ((r = upload(s + "norm1.weight", 128, &L.ln1s_g)) || (r = upload(s + "norm1.bias", 128, &L.ln1s_b))) return r;
        if ((r = upload(c + "norm1.weight", 128, &L.ln1c_g)) || (r = upload(c + "norm1.bias", 128, &L.ln1c_b))) return r;
        if ((r = upload(c + "norm2.weight", 128, &L.ln2c_g)) || (r = upload(c + "norm2.bias", 128, &L.ln2c_b))) return r;
    }
    if ((r = lin("feature_flow_attn.q_proj", 128, 128, ffq_, true))) return r;
    if ((r = lin("feature_flow_attn.k_proj", 128, 128, ffk_, true))) return r;
    if ((r = pack_conv("upsampler.0", true, nullptr, nullptr, up0_, 1))) return r;
    if ((r = pack_conv("upsampler.2", true, nullptr, nullptr, up2_, 1))) return r;
    tmap_.clear();
    PB_HIP(hipDeviceSynchronize());
    return 0;
}

// PositionEmbeddingSine(num_pos_feats = 64, temperature 10000, normalize, scale 2 pi) of ONE wh x ww window (position.py:26-46), tiled over
// the splits x splits windows (utils.py:61-86), as a token-major table [h8 * w8, 128]: channels 0..63 from y, 64..127 from x, (sin, cos) interleaved
void sine_positions(int h8, int w8, std::vector<float> &pos, int splits) {
    const int wh = h8 / splits, ww = w8 / splits;
    const float eps = 1e-6f, scale = 6.283185307179586f;
    pos.assign((size_t)h8 * w8 * 128, 0.f);
    float dim_t[64];
    for (int i = 0; i < 64; ++i) dim_t[i] = powf(10000.f, 2.f * (float)(i / 2) / 64.f);
    for (int y = 0; y < h8; ++y)
        for (int x = 0; x < w8; ++x) {
            const float ye = (float)(y % wh + 1) / ((float)wh + eps) * scale, xe = (float)(x % ww + 1) / ((float)ww + eps) * scale;
            float *p = pos.data() + ((size_t)y * w8 + x) * 128;
            for (int i = 0; i < 64; ++i) {
                const float ay = ye / dim_t[i], ax = xe / dim_t[i];
                p[i] = (i & 1) ? cosf(ay) : sinf(ay);
                p[64 + i] = (i & 1) ? cosf(ax) : sinf(ax);
            }
        }
}

// region ids of generate_shift_window_attn_mask (transformer.py:18-44) in window order: [splits * splits windows][Lw]
void shift_regions(int h8, int w8, std::vector<int8_t> &reg, int splits) {
    const int wh = h8 / splits, ww = w8 / splits;
    reg.assign((size_t)splits * splits * wh * ww, 0);
    for (int win = 0; win < splits * splits; ++win)
        for (int ly = 0; ly < wh; ++ly)
            for (int lx = 0; lx < ww; ++lx) {
                const int ry = (win / splits) * wh + ly, rx = (win % splits) * ww + lx;
                const int cy = ry < h8 - wh ? 0 : (ry < h8 - wh / 2 ? 1 : 2), cx = rx < w8 - ww ? 0 : (rx < w8 - ww / 2 ? 1 : 2);
                reg[((size_t)win * wh + ly) * ww + lx] = (int8_t)(cy * 3 + cx);
            }
}

void gm_geometry(int h8, int w8, GmGeom &g, int &ldvP, int splits) {
    g.h8 = h8; g.w8 = w8; g.P = h8 * w8; g.wh = h8 / splits; g.ww = w8 / splits; g.Lw = g.wh * g.ww; g.ldv = (int)round_up(g.Lw, 32); g.ns = splits;
    ldvP = (int)round_up(g.P, 32);
}

int GmflowEngine::prepare_g(int F, int H, int W, float scale, int dirs) {
    if (plan_.covers(F, H, W, scale, dirs, options_)) return 0;
    PB_HIP(hipStreamSynchronize(stream));
    plan_.clear();
    geometry(H, W, scale, scales_ == 2 ? 32 : 16);        // InputPadder(padding_factor): 16 = 8 x the 2 x 2 split, 32 = 4 x the fine scale's 8 x 8 split
    if (isz_h_ > 0) {                 // --inference_size: the network's size is given, nothing is padded (sh_, sw_ stay the output size)
        padl_ = padt_ = 0;
        Hp_ = isz_h_; Wp_ = isz_w_;
        h8_ = Hp_ / 8; w8_ = Wp_ / 8; P_ = h8_ * w8_;
    }
    PB_CHECK(h8_ >= 4 && w8_ >= 4 && h8_ % 2 == 0 && w8_ % 2 == 0, PB_ERR_ARG, "flow_gmflow: %dx%d is too small", sh_, sw_);
    gm_geometry(h8_, w8_, g_, ldvP_);
    const int NP = F - 1;
    const int64_t B = (int64_t)NP * dirs;
    int64_t R = (int64_t)NP * 2 * P_, VtW = (int64_t)NP * 8 * g_.ldv, Pm = P_;       // token rows, window V^T rows of 2 x 128 halfs, tokens of an image
    h4_ = w4_ = P4_ = 0;
    if (scales_ == 2) {               // the fine scale: both frames of every (pair, direction) on the 1/4 grid, 8 x 8 windows; shares the coarse scale's buffers
        PB_CHECK(Hp_ >= 64 && Wp_ >= 64 && Hp_ % 32 == 0 && Wp_ % 32 == 0, PB_ERR_ARG, "flow_gmflow (two scales): %dx%d is too small (64 x 64 after padding to /32)", sh_, sw_);
        h4_ = Hp_ / 4; w4_ = Wp_ / 4; P4_ = h4_ * w4_;
        int ldvP4;
        gm_geometry(h4_, w4_, g4_, ldvP4, 8);
        // what chunk_pairs keeps the host pipeline inside; the device entry points (pb_flow_infer_sequence*_dev) come here with the caller's F
        PB_CHECK(B <= 511 && B * 2 * P4_ <= (INT64_C(1) << 20), PB_ERR_ARG,
                 "flow_gmflow (two scales): %lld (pair, direction) elements of 2 x %d tokens in one call; one call takes 511 elements and 2^20 token rows "
                 "(the host entry points split a sequence into such chunks; a device entry point takes one chunk)", (long long)B, P4_);
        R = std::max(R, B * 2 * P4_); VtW = std::max(VtW, B * 2 * 64 * g4_.ldv); Pm = P4_;
    }
    const size_t slack = 1 << 16;
    int r = plan_arena("flow_gmflow", [&]() -> int {
        carve_encoder(F);
        feat_ = (float *)carve((size_t)F * P_ * 128 * 4);
        pos_ = (float *)carve((size_t)P_ * 128 * 4);
        region_ = (int8_t *)carve((size_t)4 * g_.Lw);
        if (scales_ == 2) {
            c2_ = (f16 *)carve((size_t)round_up((int64_t)F * P4_, 256) * 256 * 2 + slack);
            feat4_ = (float *)carve((size_t)F * P4_ * 128 * 4);
            pos4_ = (float *)carve((size_t)P4_ * 128 * 4);
            region4_ = (int8_t *)carve((size_t)64 * g4_.Lw);
            warp_ = (float *)carve((size_t)B * P4_ * 128 * 4);
            flowu_ = (float *)carve((size_t)B * P4_ * 2 * 4); flowm4_ = (float *)carve((size_t)B * P4_ * 2 * 4);
            flowf_ = (float *)carve((size_t)B * P4_ * 2 * 4); flowp4_ = (float *)carve((size_t)B * P4_ * 2 * 4);
            // the fine scale re-uses the token stream's buffers: the coarse scale's "tfeat" / "block0" stages are kept as copies
            tfeat8_ = (float *)carve((size_t)NP * 2 * P_ * 128 * 4); blk08_ = (float *)carve((size_t)NP * 2 * P_ * 128 * 4);
        }
        X_ = (float *)carve((size_t)R * 128 * 4); blk0_ = (float *)carve((size_t)R * 128 * 4);
        Xs_ = (f16 *)carve((size_t)R * 256 * 2 + slack);
        Y1_ = (float *)carve((size_t)R * 640 * 4); Yq_ = (float *)carve((size_t)R * 128 * 4);
        Qw_ = (f16 *)carve((size_t)R * 256 * 2 + slack); Kw_ = (f16 *)carve((size_t)R * 256 * 2 + slack); Kcw_ = (f16 *)carve((size_t)R * 256 * 2 + slack);
        Vtw_ = (f16 *)carve((size_t)VtW * 2 * 128 * 2 + slack); Vtcw_ = (f16 *)carve((size_t)VtW * 2 * 128 * 2 + slack);
        Ow_ = (float *)carve((size_t)R * 128 * 4); Os_ = (f16 *)carve((size_t)R * 256 * 2 + slack);
        M_ = (float *)carve((size_t)R * 128 * 4);
        cat_ = (f16 *)carve((size_t)R * 512 * 2 + slack); Hs_ = (f16 *)carve((size_t)R * 2048 * 2 + slack);
        gridvt_ = (f16 *)carve((size_t)64 * ldvP_ * 2 + slack);
        Om_ = (float *)carve((size_t)B * Pm * 32 * 4);
        flowm_ = (float *)carve((size_t)B * P_ * 2 * 4); flowp_ = (float *)carve((size_t)B * P_ * 2 * 4);
        Vtf_ = (f16 *)carve((size_t)B * 64 * ldvP_ * 2 + slack);
        qs_ = (f16 *)carve((size_t)R * 256 * 2 + slack); ks_ = (f16 *)carve((size_t)R * 256 * 2 + slack);
        umap_ = (f16 *)carve((size_t)B * Pm * 384 * 2 + slack); u1_ = (f16 *)carve((size_t)round_up(B * Pm, 256) * 512 * 2 + slack);
        mask_ = (float *)carve((size_t)B * P_ * 576 * 4);                 // (two scales: P4 x 144 logits, the same bytes)
        up_ = (float *)carve((size_t)B * sh_ * sw_ * 2 * 4);
        upi_ = isz_h_ > 0 ? (float *)carve((size_t)B * Hp_ * Wp_ * 2 * 4) : nullptr;
        maxd_ = (unsigned *)carve((size_t)B * 4);
        return 0;
    });
    if (r) return r;
    std::vector<float> pos;
    std::vector<int8_t> reg;
    sine_positions(h8_, w8_, pos);
    shift_regions(h8_, w8_, reg);
    PB_HIP(hipMemcpyAsync(pos_, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, stream));
    PB_HIP(hipMemcpyAsync(region_, reg.data(), reg.size(), hipMemcpyHostToDevice, stream));
    std::vector<float> pos4;
    std::vector<int8_t> reg4;
    if (scales_ == 2) {
        sine_positions(h4_, w4_, pos4, 8);
        shift_regions(h4_, w4_, reg4, 8);
        PB_HIP(hipMemcpyAsync(pos4_, pos4.data(), pos4.size() * 4, hipMemcpyHostToDevice, stream));
        PB_HIP(hipMemcpyAsync(region4_, reg4.data(), reg4.size(), hipMemcpyHostToDevice, stream));
    }
    if ((r = launch_gm_grid_vt(stream, gridvt_, P_, w8_, ldvP_))) return r;
    if ((r = upload_resize_tables(H, W, scale))) return r;         // synchronises: the host vectors above stay alive until then
    plan_.set(F, H, W, scale, dirs, options_);
    return 0;
}

int GmflowEngine::gemm32(const f16 *A, int lda, int64_t M, const PackedW &w, float *out, int ldo) {
    GemmArgs a;
    a.A = A; a.lda = lda; a.N = w.N; a.M = (int)M;
    set_weights(a, w, false);
    a.out32 = out; a.ldo = ldo; a.scale = 1.f;
    return timed_gemm(F_GEMM, 2.0 * M * (double)w.N * w.Kreal, 2.0 * ((double)M * w.Kreal + (double)w.N * w.Kreal) + 4.0 * M * w.N, [&] { return launch_gemm(cur_, A_DENSE, EPI_F32, TILE_AUTO, a); },
                      1.0 + w.sa + w.sw);
}

int GmflowEngine::gemm16(const f16 *A, int lda, int64_t M, const PackedW &w, f16 *out, int ldo, int act, int lo_off) {
    GemmArgs a;
    a.A = A; a.lda = lda; a.N = w.N; a.M = (int)M;
    set_weights(a, w, false);
    a.out = out; a.ldo = ldo; a.act = act; a.lo_off = lo_off;
    return timed_gemm(F_GEMM, 2.0 * M * (double)w.N * w.Kreal, 2.0 * ((double)M * w.Kreal + (double)w.N * w.Kreal + (double)M * w.N), [&] { return launch_gemm(cur_, A_DENSE, EPI_STD, TILE_AUTO, a); },
                      1.0 + w.sa + w.sw);
}

// 3 x 3 convolution of a split map [n, H, W, 256] (128 channels) with fp32 output [n * OH * OW, 128]: the implicit GEMM with the fp32 epilogue
int GmflowEngine::conv32(const f16 *in, int n, int H, int W, int stride, const PackedW &w, float *out) {
    GemmArgs a;
    a.A = in; a.N = w.N;
    a.cH = H; a.cW = W; a.cC = 128; a.cLd = 256; a.cKW = 3; a.cStride = stride; a.cPad = 1; a.cPadX = 1;
    a.cOH = (H - 1) / stride + 1; a.cOW = (W - 1) / stride + 1;
    a.M = n * a.cOH * a.cOW;
    a.out32 = out; a.ldo = 128; a.scale = 1.f;
    PB_CHECK(!w.sw || w.Cseg == 128, PB_ERR_STATE, "conv32: weights packed for %d channels", w.Cseg);
    set_weights(a, w, true);
    PB_CHECK(w.K == 9 * a.cC, PB_ERR_STATE, "conv32: packed K %d != 9*%d", w.K, a.cC);
    return timed_gemm(F_CONV128, 2.0 * a.M * (double)a.N * w.Kreal, 2.0 * ((double)n * H * W * 128 + (double)a.N * w.Kreal) + 4.0 * a.M * a.N, [&] { return launch_gemm(cur_, A_CONV, EPI_F32, TILE_128, a); },
                      1.0 + w.sa + w.sw);
}

int GmflowEngine::attention(const Attn128Args &a, double keys_per_query) {
    // S and P V: 2 x 2 x (128 + vcols) flops per (query, key); three MFMA passes each in split mode
    const double qk = 2.0 * a.B * (double)a.L * keys_per_query * 128.0, pv = 2.0 * a.B * (double)a.L * keys_per_query * a.vcols;
    return timed(F_ATTN, qk + pv, 0, [&] { return launch_attention128x(cur_, a); }, nullptr, ((a.split ? 3.0 : 1.0) * qk + (a.split && !a.pv_single ? 3.0 : 1.0) * pv) / (qk + pv));
}

int GmflowEngine::set_inference_size(int h, int w) {
    if (scales_ == 2)
        PB_CHECK((h == 0 && w == 0) || (h >= 64 && w >= 64 && h % 32 == 0 && w % 32 == 0), PB_ERR_ARG,
                 "flow_gmflow (two scales): --inference_size %d %d must be multiples of 32, at least 64 (4 x the fine scale's 8 x 8 window split)", h, w);
    PB_CHECK((h == 0 && w == 0) || (h >= 32 && w >= 32 && h % 16 == 0 && w % 16 == 0), PB_ERR_ARG,
             "flow_gmflow: --inference_size %d %d must be multiples of 16 (8 x the 2 x 2 window split; the reference fails in its window split otherwise)", h, w);
    if (h != isz_h_ || w != isz_w_) { isz_h_ = h; isz_w_ = w; ++options_; }      // re-plan on the next call
    return 0;
}

int GmflowEngine::set_matching(int corr_radius, int prop_radius) {
    if (scales_ == 2) {               // the fine scale's radii; the coarse scale is always global
        PB_CHECK(corr_radius >= 1 && corr_radius <= 4, PB_ERR_ARG,
                 "flow_gmflow (two scales): --corr_radius_list -1 %d: the fine scale's matching radius must be 1 .. 4 (global matching over the 1/4 grid is not built)", corr_radius);
        PB_CHECK(prop_radius >= 1 && prop_radius <= 2, PB_ERR_ARG,
                 "flow_gmflow (two scales): --prop_radius_list -1 %d: the fine scale's propagation radius must be 1 .. 2 (global propagation over the 1/4 grid is not built)", prop_radius);
        corr_r4_ = corr_radius; prop_r4_ = prop_radius;          // kernel template arguments only: the plan does not depend on them
        return 0;
    }
    PB_CHECK(corr_radius == -1 || (corr_radius >= 1 && corr_radius <= 4), PB_ERR_ARG,
             "flow_gmflow: --corr_radius_list %d must be -1 (global matching) or 1 .. 4", corr_radius);
    PB_CHECK(prop_radius == -1 || (prop_radius >= 1 && prop_radius <= 2), PB_ERR_ARG,
             "flow_gmflow: --prop_radius_list %d must be -1 (global propagation) or 1 .. 2", prop_radius);
    if (corr_radius != corr_r_ || prop_radius != prop_r_) { corr_r_ = corr_radius; prop_r_ = prop_radius; ++options_; }      // re-plan on the next call
    return 0;
}

// two scales: a (pair, direction) carries 2 x P4 token rows of ~14 KB through the fine scale's blocks - chunks of at most 2^20 rows (~14 GB)
int GmflowEngine::chunk_pairs(int wanted, int H, int W, float scale, int dirs) const {
    if (scales_ != 2) return wanted;
    const FlowGeometry g = flow_geometry(H, W, scale, 32);
    const int64_t P4 = isz_h_ > 0 ? (int64_t)(isz_h_ / 4) * (isz_w_ / 4) : (int64_t)(g.Hp / 4) * (g.Wp / 4);
    const int64_t fit = std::min<int64_t>((INT64_C(1) << 20) / ((int64_t)dirs * 2 * P4), 511 / dirs);       // ... and of 511 batch elements (fine_scale)
    return (int)std::max<int64_t>(1, std::min<int64_t>(wanted, fit));
}

// The six transformer blocks (transformer.py:108-290) on the token stream X_ / Xs_ of NPs pairs over the grid and windows of g; `region`
// is g's shifted-window region table, blk0 the stage name of the stream after the first block (debug)
int GmflowEngine::blocks(const GmGeom &g, int NPs, const int8_t *region, const char *blk0) {
    int r;
    const int nw = g.ns * g.ns, Bw = NPs * 2 * nw, split = split_w_ ? 1 : 0;
    const int64_t R = (int64_t)NPs * 2 * g.P;
    for (int li = 0; li < 6; ++li) {
        const Layer &L = layers_[li];
        const int shifted = li & 1;
        if ((r = gemm32(Xs_, 256, R, L.w1, Y1_, 640))) return r;
        GmPackJobs jobs{};
        jobs.n = 5;
        jobs.j[0] = GmPackJob{Y1_, 640, 0, Qw_, 0};
        jobs.j[1] = GmPackJob{Y1_, 640, 128, Kw_, 0};
        jobs.j[2] = GmPackJob{Y1_, 640, 256, Vtw_, 1};
        jobs.j[3] = GmPackJob{Y1_, 640, 384, Kcw_, 0};
        jobs.j[4] = GmPackJob{Y1_, 640, 512, Vtcw_, 1};
        r = timed(F_ELT, 0, 0, [&] { return launch_gm_pack(stream, jobs, g, Bw, shifted); });
        if (r) return r;
        Attn128Args a;
        a.Q = Qw_; a.K = Kw_; a.Vt = Vtw_; a.region = shifted ? region : nullptr; a.nreg = nw; a.O = Ow_;
        a.B = Bw; a.L = g.Lw; a.ldv = g.ldv; a.split = split; a.vcols = 128; a.ldq = 256; a.v_bstride = (int64_t)2 * 128 * g.ldv;
        // window attention: q / k split; P and V as single fp16 in the one-scale model (2.6e-4 of its budget, attention128.hip).  The two-scale
        // model runs both scales with P and V split as well: its warp samples the target's 1/4 features at the coarse flow, and features that
        // change by their whole range from one token to the next turn a coarse-flow error of 3e-4 of range into 1e-3 .. 3e-3 of the warped
        // features (EXPERIMENTS.md 6.12), so the coarse scale has to be several times closer than the one-scale model needs to be.
        a.pv_single = scales_ == 2 ? 0 : 1;
        if ((r = attention(a, g.Lw))) return r;
        r = timed(F_ELT, 0, 0, [&] { return launch_gm_split_rows(stream, Ow_, 128, 128, Os_, R); });
        if (r) return r;
        if ((r = gemm32(Os_, 256, R, L.merge_s, M_, 128))) return r;
        r = timed(F_LN, 0, 0, [&] { return launch_gm_ln(stream, M_, L.ln1s_g, L.ln1s_b, X_, Xs_, R, g, 1, shifted, 0); });
        if (r) return r;
        // cross attention + FFN: queries from the updated stream, keys / values from the partner frame's ENTERING stream (Kcw_, Vtcw_)
        if ((r = gemm32(Xs_, 256, R, L.q_c, Yq_, 128))) return r;
        jobs.n = 1;
        jobs.j[0] = GmPackJob{Yq_, 128, 0, Qw_, 0};
        r = timed(F_ELT, 0, 0, [&] { return launch_gm_pack(stream, jobs, g, Bw, shifted); });
        if (r) return r;
        a.K = Kcw_; a.Vt = Vtcw_; a.kxor = nw;            // the same window of the pair's other frame
        if ((r = attention(a, g.Lw))) return r;
        r = timed(F_ELT, 0, 0, [&] { return launch_gm_split_rows(stream, Ow_, 128, 128, Os_, R); });
        if (r) return r;
        if ((r = gemm32(Os_, 256, R, L.merge_c, M_, 128))) return r;
        r = timed(F_LN, 0, 0, [&] { return launch_gm_ln(stream, M_, L.ln1c_g, L.ln1c_b, X_, cat_, R, g, 1, shifted, 1); });
        if (r) return r;
        if ((r = gemm16(cat_, 512, R, L.mlp0, Hs_, 2048, ACT_GELU, 1024))) return r;
        if ((r = gemm32(Hs_, 2048, R, L.mlp2, M_, 128))) return r;
        r = timed(F_LN, 0, 0, [&] { return launch_gm_ln(stream, M_, L.ln2c_g, L.ln2c_b, X_, Xs_, R, g, 0, 0, 0); });
        if (r) return r;
        if (debug && li == 0) {
            PB_HIP(hipMemcpyAsync(blk0_, X_, (size_t)R * 128 * 4, hipMemcpyDeviceToDevice, stream));
            stages_[blk0] = Stage::f32_rows(blk0_, (int64_t)NPs * 2, g.P, 128);
        }
    }
    return 0;
}

int GmflowEngine::infer(const uint8_t *frames, int F, int H, int W, float scale, int /*iters*/, int backward, float *flow_out,
                        uint8_t *rgb_out, float *maxdisp, uint8_t *mask_out, float alpha1, float alpha2) {
    PB_CHECK(frames && F >= 2 && H > 0 && W > 0 && scale > 0.f, PB_ERR_ARG, "flow_gmflow infer: bad arguments");
    PB_CHECK(!mask_out || backward, PB_ERR_ARG, "consistency masks need both directions (backward = 1)");
    PB_HIP(hipSetDevice(device));
    const int dirs = backward ? 2 : 1;
    int r = prepare_g(F, H, W, scale, dirs);
    if (r) return r;
    timer.reset();
    stages_.clear();
    const int NP = F - 1, B = NP * dirs, P = P_;
    const int64_t R = (int64_t)NP * 2 * P;
    const int split = split_w_ ? 1 : 0;
    const int es = split_w_ ? 2 : 1;
    const bool fine = scales_ == 2;
    const int corr_r = fine ? -1 : corr_r_, prop_r = fine ? -1 : prop_r_;       // two scales: the coarse scale is always global

    // ---- frame prep (resize, replicate pad to /16 - two scales: /32 -, ImageNet normalisation) and the backbone, once per frame ----
    if ((r = prep_frames(frames, F, H, W, scale, -1, 1, isz_h_ > 0))) return r;
    const f16 *x = nullptr;
    if ((r = run_encoder(backbone_, true, F, &x))) return r;
    if (!fine) {
        if ((r = gemm32(x, es * 128, (int64_t)F * P, backbone_.out, feat_, 128))) return r;
    } else {
        // the backbone ends at 1/4 (layer3 at stride 1, conv2 1 x 1) and ONE 3 x 3 weight gives both scales (trident_conv.py:64-72): stride 1
        // the 1/4 features, stride 2 the 1/8 features
        if ((r = gemm16(x, es * 128, (int64_t)F * P4_, backbone_.out, c2_, 256, ACT_NONE, split_w_ ? 128 : 0))) return r;
        if ((r = conv32(c2_, F, h4_, w4_, 1, trident_, feat4_))) return r;
        if ((r = conv32(c2_, F, h4_, w4_, 2, trident_, feat_))) return r;
        stages_["feat4"] = Stage::f32_rows(feat4_, F, P4_, 128);
    }
    stages_["feat"] = Stage::f32_rows(feat_, F, P, 128);

    // ---- tokens + per-window sine positions; the six transformer blocks ----
    r = timed(F_ELT, 0, 0, [&] { return launch_gm_tokens(stream, feat_, pos_, X_, Xs_, NP, P); });
    if (r) return r;
    if ((r = blocks(g_, NP, region_, "block0"))) return r;
    stages_["tfeat"] = Stage::f32_rows(X_, (int64_t)NP * 2, P, 128);
    if (fine) {                       // X_ and blk0_ are the fine scale's next: the coarse "tfeat" / "block0" stages exist as debug copies only
        stages_.erase("tfeat");
        if (debug) {
            PB_HIP(hipMemcpyAsync(tfeat8_, X_, (size_t)R * 128 * 4, hipMemcpyDeviceToDevice, stream));
            stages_["tfeat"] = Stage::f32_rows(tfeat8_, (int64_t)NP * 2, P, 128);
            PB_HIP(hipMemcpyAsync(blk08_, blk0_, (size_t)R * 128 * 4, hipMemcpyDeviceToDevice, stream));
            stages_["block0"] = Stage::f32_rows(blk08_, (int64_t)NP * 2, P, 128);
        }
    }

    // ---- matching: global (matching.py:7-42: softmax over ALL target tokens of the dot products, expectation of their coordinates) or, with a
    // radius, local (matching.py:39-83: over the (2R + 1)^2 target tokens around the source token; both directions = source and target swapped) ----
    const int64_t img = (int64_t)P * 256;                    // one frame's rows of a split token matrix
    const int img_step = dirs == 2 ? 1 : 2;
    if (corr_r < 0) {
        Attn128Args m;
        m.Q = Xs_; m.O = Om_; m.B = B; m.L = P; m.ldv = ldvP_; m.split = split; m.vcols = 32; m.ldq = 256;
        m.Vt = gridvt_; m.v_shared = 1;
        if (dirs == 2) { m.K = Xs_; m.q_bstride = m.k_bstride = img; m.kxor = 1; }
        else { m.K = Xs_ + img; m.q_bstride = m.k_bstride = 2 * img; }
        if ((r = attention(m, P))) return r;
        r = timed(F_ELT, 0, 0, [&] { return launch_gm_match_flow(stream, Om_, flowm_, Vtf_, B, P, w8_, ldvP_); });
        if (r) return r;
    } else {
        const double nc = (2.0 * corr_r + 1) * (2.0 * corr_r + 1);
        r = timed(F_ATTN, 2.0 * B * (double)P * nc * 128.0, 2.0 * (double)B * P * 128 * 4, [&] { return launch_gm_local_match(stream, X_, flowm_, prop_r < 0 ? Vtf_ : nullptr, B, h8_, w8_, img_step, corr_r, ldvP_); },
                  "gm_local_match_kernel");
        if (r) return r;
    }
    stages_["flow_match"] = Stage::f32_rows(flowm_, B, P, 2);

    // ---- flow propagation (transformer.py:316-337 global, :376-409 local window): self-similarity of the source frame's features spreads the
    // matched flow ----
    if ((r = gemm32(Xs_, 256, R, ffq_, Yq_, 128))) return r;
    if (prop_r < 0) {
        r = timed(F_ELT, 0, 0, [&] { return launch_gm_split_rows(stream, Yq_, 128, 128, qs_, R); });
        if (r) return r;
        if ((r = gemm32(qs_, 256, R, ffk_, M_, 128))) return r;         // the key is k_proj of the PROJECTED query, as in the reference (:363-364)
        r = timed(F_ELT, 0, 0, [&] { return launch_gm_split_rows(stream, M_, 128, 128, ks_, R); });
        if (r) return r;
        Attn128Args pa;
        pa.Q = qs_; pa.K = ks_; pa.O = Om_; pa.B = B; pa.L = P; pa.ldv = ldvP_; pa.split = split; pa.vcols = 32; pa.ldq = 256;
        pa.Vt = Vtf_; pa.v_bstride = (int64_t)64 * ldvP_;
        pa.q_bstride = pa.k_bstride = dirs == 2 ? img : 2 * img;
        if ((r = attention(pa, P))) return r;
    } else {
        if ((r = gemm32(Xs_, 256, R, ffk_, M_, 128))) return r;         // the local form projects the key from the feature itself (:389), not from the query
        const double nc = (2.0 * prop_r + 1) * (2.0 * prop_r + 1);
        r = timed(F_ATTN, 2.0 * B * (double)P * nc * 128.0, 2.0 * (double)B * P * 128 * 4, [&] { return launch_gm_local_prop(stream, Yq_, M_, flowm_, Om_, B, h8_, w8_, img_step, prop_r); },
                  "gm_local_prop_kernel");
        if (r) return r;
    }

    // ---- convex upsampling (gmflow.py:74-92), unpad, encode ----
    // (two scales: launched for the coarse flow it leaves in flowp_; the B P x 768 bytes of umap_ it also writes - 29 MB at 1080p x 0.75 with
    // both directions, microseconds - are overwritten by the fine scale's launch.  The kernel is the one-scale model's, left as it is.)
    r = timed(F_ELT, 0, 0, [&] { return launch_gm_upsampler_in(stream, Om_, X_, flowp_, umap_, B, P, img_step); });
    if (r) return r;
    stages_["flow_prop"] = Stage::f32_rows(flowp_, B, P, 2);
    int hu = h8_, wu = w8_, Pu = P, factor = 8;            // the grid the upsampler runs on
    const float *flow_lo = flowp_;
    if (fine) {
        if ((r = fine_scale(B, dirs))) return r;
        hu = h4_; wu = w4_; Pu = P4_; factor = 4; flow_lo = flowp4_;
    }
    if ((r = conv(umap_, 192, 384, B, hu, wu, 3, 3, 1, up0_, u1_, 512, ACT_RELU, 0, nullptr, nullptr, split_w_ ? 256 : 0))) return r;
    if ((r = gemm32(u1_, 512, (int64_t)B * Pu, up2_, mask_, 9 * factor * factor))) return r;
    return flow_tail(flow_lo, B, NP, hu, wu, factor, flow_out, rgb_out, maxdisp, mask_out, alpha1, alpha2, upi_);
}

// The fine scale of the two-scale model (gmflow.py:112-165, scale_idx = 1) from the coarse flow in flowp_ [B, P, 2] and the 1/4 features in
// feat4_: batch element b = (pair, direction) is its own sample - source frame pair + d, target frame pair + 1 - d - because instance norm and
// every attention are per sample, which is what pred_bidir_flow's concatenation computes.  Leaves the propagated flow in flowp4_ and the
// upsampler's input map in umap_.
int GmflowEngine::fine_scale(int B, int dirs) {
    int r;
    const int64_t R4 = (int64_t)B * 2 * P4_;
    PB_CHECK(B * 128 <= 65535, PB_ERR_ARG, "flow_gmflow (two scales): %d (pair, direction) elements in one call; the window kernels take 511 (128 windows each)", B);
    r = timed(F_ELT, 0, (double)B * P4_ * 128 * 8, [&] { return launch_gm_warp(stream, flowp_, feat4_, flowu_, warp_, B, dirs, h8_, w8_); }, "gm_warp_kernel");
    if (r) return r;
    stages_["flow_up"] = Stage::f32_rows(flowu_, B, P4_, 2);
    stages_["warp"] = Stage::f32_rows(warp_, B, P4_, 128);
    r = timed(F_ELT, 0, 0, [&] { return launch_gm_tokens(stream, feat4_, pos4_, X_, Xs_, B, P4_, warp_, dirs); });
    if (r) return r;
    if ((r = blocks(g4_, B, region4_, "block0_4"))) return r;
    stages_["tfeat4"] = Stage::f32_rows(X_, (int64_t)B * 2, P4_, 128);
    // local matching of (source, warped target): images 2 b and 2 b + 1 of the stream; the residual adds to the enlarged flow (:145)
    const double nc = (2.0 * corr_r4_ + 1) * (2.0 * corr_r4_ + 1);
    r = timed(F_ATTN, 2.0 * B * (double)P4_ * nc * 128.0, 2.0 * (double)B * P4_ * 128 * 4, [&] { return launch_gm_local_match(stream, X_, flowm4_, nullptr, B, h4_, w4_, 2, corr_r4_, 0); },
              "gm_local_match_kernel");
    if (r) return r;
    r = timed(F_ELT, 0, 0, [&] { return launch_gm_flow_add(stream, flowu_, flowm4_, flowf_, (int64_t)B * P4_); });
    if (r) return r;
    stages_["flow_match4"] = Stage::f32_rows(flowf_, B, P4_, 2);
    // the two projections run over the whole stream in one launch each, as at the coarse scale; gm_local_prop reads the source images only
    // (every other block of P4 rows, which one GEMM launch cannot address), so half of these 2 x 128 x 128 products per row - 0.5 % of the
    // six blocks' GEMM work on the same rows - go unread
    if ((r = gemm32(Xs_, 256, R4, ffq_, Yq_, 128))) return r;
    if ((r = gemm32(Xs_, 256, R4, ffk_, M_, 128))) return r;
    const double np = (2.0 * prop_r4_ + 1) * (2.0 * prop_r4_ + 1);
    r = timed(F_ATTN, 2.0 * B * (double)P4_ * np * 128.0, 2.0 * (double)B * P4_ * 128 * 4, [&] { return launch_gm_local_prop(stream, Yq_, M_, flowf_, Om_, B, h4_, w4_, 2, prop_r4_); },
              "gm_local_prop_kernel");
    if (r) return r;
    r = timed(F_ELT, 0, 0, [&] { return launch_gm_upsampler_in(stream, Om_, X_, flowp4_, umap_, B, P4_, 2); });
    if (r) return r;
    stages_["flow_prop4"] = Stage::f32_rows(flowp4_, B, P4_, 2);
    return 0;
}
