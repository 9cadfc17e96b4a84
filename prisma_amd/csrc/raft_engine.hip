// RaftEngine: the flow_raft band on one MI355X.
// Reference call stack being replaced: bands/flow_raft.py:98-113 (per-frame loop: resize, [prev,curr] /
// [curr,prev] batch, infer) -> :51-62 (pad, RAFT(test_mode), unpad) -> bands/raft/raft.py:87-146 ->
// extractor.py / corr.py / update.py -> bands/common/flow.py:64-88 + encode.py:98-126 (process_flow).
//
// Differences in schedule, not in arithmetic:
//   * every frame goes through fnet and cnet ONCE per sequence (the reference re-encodes both frames of
//     every pair, twice when it also computes the backward flow);
//   * the mask head (152.9 of 1559.6 GFLOP per pair at 720p) runs only after the last iteration - in
//     test_mode the reference computes it every iteration and discards all but the last (raft.py:136-144);
//   * cnet's eval-mode BatchNorm is folded into its convolutions at pack time; fnet's InstanceNorm uses
//     run-time statistics and stays a separate pass.
#include "raft_engine.h"
#include "flow_chunk.h"
#include "corr_layout.h"

#include <math.h>
#include <string.h>

#include <algorithm>

int RaftEngine::chunk_pairs(int wanted, int H, int W, float scale, int dirs) const {
    if (!hoist_) return wanted;
    return flow_chunk_pairs(wanted, dirs, flow_geometry(H, W, scale, 8).P, upd8_ ? 576 : 384);
}

int RaftEngine::load(const pb_tensor *w, int n) {
    int r0 = begin_load(w, n);
    if (r0) return r0;
    int r;
    pack_tapin_ = env.tapin == 2;
    for (int e = 0; e < 2; ++e) {
        const std::string en = e == 0 ? "fnet" : "cnet";
        Enc &E = e == 0 ? fnet_ : cnet_;
        if ((r = pack_encoder(en, e == 1, true, E))) return r;
        if ((r = pack_conv(en + ".conv2", true, nullptr, nullptr, E.out, 1))) return r;
    }
    const std::string u = "update_block.";
    // the update block's activations carry an fp8 copy ([a16 | a8] per pixel) and its weight residuals are e4m3 (PackedW::mx2): the residual
    // pass a8 x w_lo8 runs on the MX-scaled MFMA at half the matrix-pipe time of the second fp16 pass it replaces.  History: rounds 2-3 kept
    // this off (it bought 1 % of the band: the MX build of the 128 x 128 tile copied its accumulators through VGPRs every K tile, and the
    // variant excluded the context hoist below); round 4 fixed both - 31 pairs 1080p x 0.75: flow band 150.4 -> 142.2 ms on one box - and the
    // parity figures do not move (720p x 8 pairs 4.1e-4 ... 5.4e-4 max, 3.4e-4 ... 3.5e-4 L2 against 4.1e-4 ... 6.6e-4 / 3.4e-4 with two fp16
    // passes; heavy-tailed weights 5.8e-4 against 6.3e-4): the e4m3 rounding only ever enters a residual term.  PB_MX_UPD=0: two fp16 passes.
    pack_mx2_ = mx_ && env.mx_upd;
    upd8_ = pack_mx2_;
    // slice-major K order (gemm.h cTapInner) for the 3x3 / 1x5 / 5x1 convolutions over the 128 ... 384-channel maps of the update block:
    // tap-major order overflows the XCD L2 there.  PB_TAPIN=0 turns it off, 2 also applies it to the encoders (A/B runs).
    const int tapin_all = pack_tapin_;
    pack_tapin_ = env.tapin != 0;
    if ((r = pack_conv(u + "encoder.convc1", true, nullptr, nullptr, convc1_))) return r;
    if ((r = pack_conv(u + "encoder.convc2", true, nullptr, nullptr, convc2_))) return r;
    if ((r = pack_conv(u + "encoder.convf2", true, nullptr, nullptr, convf2_))) return r;
    if ((r = pack_conv(u + "encoder.conv", true, nullptr, nullptr, convm_))) return r;
    convm_.N = 128; convm_.Nreal = 126;                     // 126 real outputs + 2 zero rows (N must be a multiple of 8)
    {   // convf1 7x7 on the 2-channel flow: im2col order k = tap*2 + c, K 98 -> 128
        auto iw = tmap_.find(u + "encoder.convf1.weight"), ib = tmap_.find(u + "encoder.convf1.bias");
        PB_CHECK(iw != tmap_.end() && ib != tmap_.end(), PB_ERR_ARG, "missing convf1");
        const float *wt = (const float *)iw->second->data;
        std::vector<float> g((size_t)128 * 98);
        for (int o = 0; o < 128; ++o)
            for (int c = 0; c < 2; ++c)
                for (int tp = 0; tp < 49; ++tp) g[(size_t)o * 98 + tp * 2 + c] = wt[((size_t)o * 2 + c) * 49 + tp];
        if ((r = pack(g.data(), 128, 98, 128, convf1_, (const float *)ib->second->data))) return r;
        {
            f1_direct_ = env.convf1_direct;
            f1_passes_ = split_w_ ? 2 : 1;
            std::vector<f16> hw((size_t)convf1_packed_halfs(f1_passes_));
            convf1_pack(wt, f1_passes_, hw.data());
            void *pw = nullptr;
            PB_HIP(hipMalloc(&pw, hw.size() * 2));
            owned_.push_back(pw);
            PB_HIP(hipMemcpy(pw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
            f1w_ = (f16 *)pw;
        }
    }
    // Context hoist (default; PB_GRU_HOIST=0 turns it off): the GRU's input is cat(h, inp, motion) and `inp` - the context
    // features - does not change over the iterations (raft.py:112-115, update.py:131).  A convolution is linear in its input channels, so
    // the inp share of every gate's pre-activation is computed ONCE per call (bias-free, stored as an fp16 hi plane + an fp16 lo plane: ~22
    // bits) and the per-iteration convolutions run on [h | motion] alone (K = 5 x 256 instead of 5 x 384), adding the two planes as the
    // epilogue's skip tensors (add1, add2) before the gate's activation.  The buffers hold [h | motion | inp] so that the two varying
    // parts are adjacent.  (First version: fp32 share as the accumulators' starting value - its 256 KB per tile were a prologue burst that
    // ate half of what the smaller K saved; as an fp32 read in the GRU epilogues it cost every EPI_STD kernel its register allocation.)
    hoist_ = env.gru_hoist;
    for (int half = 0; half < 2; ++half) {
        // z and r gates share their input: one GEMM with N = 256 ([z | r]); q separately
        const std::string sfx = std::to_string(half + 1);
        auto get = [&](const std::string &nm) -> const pb_tensor * {
            auto it = tmap_.find(nm);
            return it == tmap_.end() ? nullptr : it->second;
        };
        const pb_tensor *wz = get(u + "gru.convz" + sfx + ".weight"), *wr = get(u + "gru.convr" + sfx + ".weight");
        const pb_tensor *bz = get(u + "gru.convz" + sfx + ".bias"), *br = get(u + "gru.convr" + sfx + ".bias");
        const pb_tensor *wq = get(u + "gru.convq" + sfx + ".weight"), *bq = get(u + "gru.convq" + sfx + ".bias");
        PB_CHECK(wz && wr && bz && br && wq && bq, PB_ERR_ARG, "missing gru weights");
        // rows [o][tap][c] over the channel range [c0, c0 + nc) of the reference's 384 input channels (h 0..127, inp 128..255, motion 256..383),
        // written at column offset `dst` of a [taps x width] row
        auto fill = [&](std::vector<float> &g, int row0, int width, int dst, const pb_tensor *w, int c0, int nc) {
            const float *wt = (const float *)w->data;
            for (int o = 0; o < 128; ++o)
                for (int c = 0; c < nc; ++c)
                    for (int tp = 0; tp < 5; ++tp) g[(size_t)(row0 + o) * 5 * width + tp * width + dst + c] = wt[((size_t)o * 384 + c0 + c) * 5 + tp];
        };
        std::vector<float> bb(256);
        for (int o = 0; o < 128; ++o) { bb[o] = ((const float *)bz->data)[o]; bb[128 + o] = ((const float *)br->data)[o]; }
        if (!hoist_) {
            const int K = 5 * 384;
            std::vector<float> g((size_t)256 * K, 0.f);
            fill(g, 0, 384, 0, wz, 0, 384);
            fill(g, 128, 384, 0, wr, 0, 384);
            if ((r = pack(g.data(), 256, K, K, zr_[half], bb.data(), 5))) return r;
            if ((r = pack_conv(u + "gru.convq" + sfx, true, nullptr, nullptr, q_[half]))) return r;
            continue;
        }
        {   // [h | motion] parts (with the biases) and the inp parts (bias-free: their result is the accumulators' starting value)
            std::vector<float> g((size_t)256 * 5 * 256, 0.f), gi((size_t)256 * 5 * 128, 0.f);
            fill(g, 0, 256, 0, wz, 0, 128);   fill(g, 0, 256, 128, wz, 256, 128);
            fill(g, 128, 256, 0, wr, 0, 128); fill(g, 128, 256, 128, wr, 256, 128);
            fill(gi, 0, 128, 0, wz, 128, 128);
            fill(gi, 128, 128, 0, wr, 128, 128);
            if ((r = pack(g.data(), 256, 5 * 256, 5 * 256, zr_[half], bb.data(), 5))) return r;
            pack_mx2_ = 0;                                  // the once-per-call share runs two fp16 passes into an fp16 hi + lo plane
            r = pack(gi.data(), 256, 5 * 128, 5 * 128, zr_in_[half], nullptr, 5);
            pack_mx2_ = upd8_;
            if (r) return r;
        }
        {
            std::vector<float> g((size_t)128 * 5 * 256, 0.f), gi((size_t)128 * 5 * 128, 0.f);
            fill(g, 0, 256, 0, wq, 0, 128); fill(g, 0, 256, 128, wq, 256, 128);
            fill(gi, 0, 128, 0, wq, 128, 128);
            if ((r = pack(g.data(), 128, 5 * 256, 5 * 256, q_[half], (const float *)bq->data, 5))) return r;
            pack_mx2_ = 0;
            r = pack(gi.data(), 128, 5 * 128, 5 * 128, q_in_[half], nullptr, 5);
            pack_mx2_ = upd8_;
            if (r) return r;
        }
    }
    if ((r = pack_conv(u + "flow_head.conv1", true, nullptr, nullptr, fh1_))) return r;
    pack_mx2_ = 0;                                          // flow_head2 is a direct kernel, mask.2 an fp32-output GEMM: fp16 residuals
    const int tapin_upd = pack_tapin_;
    pack_tapin_ = 0;                                        // ... that walks its weights tap-major
    if ((r = pack_conv(u + "flow_head.conv2", true, nullptr, nullptr, fh2_))) return r;
    fh2_.N = 8;                                             // 2 real outputs, rows 2..7 are zero
    pack_mx2_ = upd8_;
    pack_tapin_ = tapin_upd;
    if ((r = pack_conv(u + "mask.0", true, nullptr, nullptr, mk0_))) return r;
    pack_mx2_ = 0;
    pack_tapin_ = tapin_all;
    if ((r = pack_conv(u + "mask.2", true, nullptr, nullptr, mk2_))) return r;
    tmap_.clear();
    PB_HIP(hipDeviceSynchronize());
    return 0;
}

int RaftEngine::vol_layout() const { return corr_layout_ && !alt_corr_ && launch_env().volume ? CORR_BLOCKED : CORR_ROWMAJOR; }

int RaftEngine::prepare(int F, int H, int W, float scale, int dirs) {
    if (plan_.covers(F, H, W, scale, dirs, plan_word())) return 0;
    PB_HIP(hipStreamSynchronize(stream));
    plan_.clear();
    geometry(H, W, scale, 8);
    PB_CHECK(h8_ >= 16 && w8_ >= 16, PB_ERR_ARG, "flow_raft: %dx%d is too small (the 4-level pyramid needs >= 128 px)", sh_, sw_);
    {
        CorrGeo g;
        corr_pyramid_geometry(h8_, w8_, g);
        for (int l = 0; l < 4; ++l) { lh_[l] = g.h[l]; lw_[l] = g.w[l]; lwp_[l] = g.wp[l]; lhp_[l] = g.hp[l]; pld_[l] = g.ld[l]; }
    }
    const int64_t ND = (int64_t)(F - 1) * dirs;
    const size_t slack = 1 << 20;
    int r = plan_arena("flow", [&]() -> int {
        carve_encoder(F);
        fmap_ = (f16 *)carve((size_t)round_up((int64_t)F * P_, 256) * 256 * 2 + slack);
        ctx_ = (f16 *)carve((size_t)round_up((int64_t)F * P_, 256) * 256 * 2);
        for (int l = 0; l < 4; ++l) {
            // level l of the volume: fp16, one row per source pixel of pld_[l] entries (raft_kernels.hip corr_pyramid_geometry), a
            // pair-direction's rows rounded up to whole groups of 8 in the blocked layout (corr_layout.h).  alt_corr_: no volume and no tiled B
            // operand - corr_otf.hip reads fmap_ and the pooled maps
            pyr_[l] = alt_corr_ ? nullptr : (f16 *)carve((size_t)ND * corr_layout_rows(vol_layout(), P_) * pld_[l] * 2 + slack);
            fpool_[l] = l == 0 ? nullptr : (f16 *)carve((size_t)round_up((int64_t)F * lh_[l] * lw_[l], 256) * 256 * 2 + slack);
            ftile_[l] = alt_corr_ ? nullptr : (f16 *)carve((size_t)(F * (int64_t)pld_[l] + 256) * 256 * 2 + slack);
        }
        const int64_t rows = round_up(ND * P_, 256);
        h32_ = (float *)carve((size_t)rows * 128 * 4); flow_ = (float *)carve((size_t)rows * 2 * 4);
        mask_ = (float *)carve((size_t)rows * 576 * 4);
        const int Lq = upd8_ ? 576 : 384;
        const size_t u8 = upd8_ ? 3 : 2;                   // bytes per channel of an update-block map: fp16 (+ its fp8 copy after the pixel's fp16 part)
        hx_ = (f16 *)carve((size_t)rows * 384 * u8); hx2_ = (f16 *)carve((size_t)rows * 384 * u8);
        corr_ = (f16 *)carve((size_t)rows * 384 * u8); c1_ = (f16 *)carve((size_t)rows * 256 * u8);
        corflo_ = (f16 *)carve((size_t)rows * 256 * u8); fa_ = (f16 *)carve((size_t)rows * 128 * u8);
        f1_ = (f16 *)carve((size_t)rows * 128 * u8); zrb_ = (f16 *)carve((size_t)rows * 256 * 2);
        fh_ = (f16 *)carve((size_t)rows * 256 * 2);
        for (int half = 0; half < 2; ++half) {            // the context features' share of the GRU pre-activations (hoist_): hi plane, lo plane
            gz_[half] = hoist_ ? (f16 *)carve((size_t)rows * 256 * 2 * 2) : nullptr;           // row stride 256 = zrb_'s
            gq_[half] = hoist_ ? (f16 *)carve((size_t)rows * Lq * 2 * 2) : nullptr;            // row stride = hx_'s (the q convolution writes h there)
        }
        m0_ = (f16 *)carve((size_t)rows * 256 * 2);
        up_ = (float *)carve((size_t)ND * sh_ * sw_ * 2 * 4);
        maxd_ = (unsigned *)carve((size_t)ND * 4);
        return 0;
    });
    if (r || (r = upload_resize_tables(H, W, scale))) return r;
    plan_.set(F, H, W, scale, dirs, plan_word());
    return 0;
}

int RaftEngine::infer(const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward, float *flow_out,
                      uint8_t *rgb_out, float *maxdisp, uint8_t *mask_out, float alpha1, float alpha2) {
    PB_CHECK(frames && F >= 2 && H > 0 && W > 0 && iters >= 1 && scale > 0.f, PB_ERR_ARG, "flow infer: bad arguments");
    PB_CHECK(!mask_out || backward, PB_ERR_ARG, "consistency masks need both directions (backward = 1)");
    PB_HIP(hipSetDevice(device));
    const int dirs = backward ? 2 : 1;
    int r = prepare(F, H, W, scale, dirs);
    if (r) return r;
    timer.reset();
    stages_.clear();
    const int ND = (F - 1) * dirs;
    const int64_t rows = (int64_t)ND * P_;

    // ---- frame prep + stem im2col (shared by fnet and cnet) ----
    const int Lhx = upd8_ ? 576 : 384, L256 = upd8_ ? 384 : 256, L128 = upd8_ ? 192 : 128;    // pixel strides of the update block's maps
    const float s8 = (float)(1 << kMx2Pa);
    const int es = split_w_ ? 2 : 1;                         // encoder maps are [hi | lo] in split-fp16 mode
    // (the residual parts of the encoder maps are e4m3 where the mode has them: [hi | hi8 | lo8])
    if ((r = prep_frames(frames, F, H, W, scale, split_w_ && mx_ ? kLo8Pa : -1))) return r;

    // ---- the two encoders ----
    for (int e = 0; e < 2; ++e) {
        const Enc &E = e == 0 ? fnet_ : cnet_;
        const f16 *x = nullptr;
        // the context network runs on the SOURCE frame of every pair (raft.py:110-115): frames 0 .. F - 2 forward, 1 .. F - 1 backward - without the
        // backward direction the clip's last frame needs no context features (1 / F of cnet's work; per-frame results do not depend on the batch)
        const int Fe = e == 1 && dirs == 1 ? F - 1 : F;
        if ((r = run_encoder(E, e == 0, Fe, &x))) return r;
        if ((r = dense(x, es * 128, (int64_t)Fe * P_, E.out, e == 0 ? fmap_ : ctx_, 256, ACT_NONE))) return r;
    }
    stages_["fmap"] = Stage::f16_nhwc(fmap_, F, 256, h8_, w8_, 256);

    // ---- all-pairs correlation pyramid, recurrent state ----
    // corr.py:22-27 pools the volume over the target dims; pooling is linear, so level l is the correlation of fmap1 with the
    // l-times avg-pooled target features: three small pooling passes over [F, P, 256] instead of three over the 4 P^2-byte volume
    for (int l = 0; l < 4; ++l) {
        r = timed(F_ELT, 0, 0, [&] {
            int rc = l > 0 ? launch_avgpool2_nhwc(stream, l == 1 ? fmap_ : fpool_[l - 1], fpool_[l], F, lh_[l - 1], lw_[l - 1], 256) : 0;
            if (!rc && !alt_corr_) rc = launch_corr_tile(stream, l == 0 ? fmap_ : fpool_[l], ftile_[l], F, lh_[l], lw_[l], lwp_[l], pld_[l]);
            return rc;
        });
        if (r) return r;
    }
    const int layout = vol_layout();
    for (int i = 0; i < F - 1 && !alt_corr_; ++i)
        for (int d = 0; d < dirs; ++d) {
            const int n = i * dirs + d;
            for (int l = 0; l < 4; ++l) {
                GemmArgs a;
                a.A = fmap_ + (int64_t)(i + d) * P_ * 256; a.lda = 256; a.M = P_;
                a.W = ftile_[l] + (int64_t)(i + 1 - d) * pld_[l] * 256;
                a.K = 256; a.N = pld_[l];
                a.out = pyr_[l] + (int64_t)n * corr_layout_rows(layout, P_) * pld_[l]; a.ldo = pld_[l]; a.zero = zero_;
                // K = 256 against P x pld fp16 outputs: this launch is bound by writing the volume, not by the matrix pipe (bytes: A + W + out)
                const double flops = 2.0 * P_ * (double)lh_[l] * lw_[l] * 256, bytes = 2.0 * ((double)P_ * 256 + (double)pld_[l] * 256 + (double)P_ * pld_[l]);
                if (!launch_env().volume)          // PB_VOLUME=0, A/B: the generic GEMM kernels
                    r = timed_gemm(F_GEMM, flops, bytes, [&] { return launch_gemm(stream, A_DENSE, EPI_STD, TILE_AUTO, a); });
                else            // volume.hip: A-stationary, persistent along the targets; same accumulation order, same bits
                    r = timed(F_GEMM, flops, bytes, [&] { return launch_corr_volume(stream, a.A, a.M, a.W, a.N, a.N, a.out, a.ldo, layout); }, "corr_volume_kernel");
                if (r) return r;
            }
        }
    // the recurrent state of every pair-direction in one launch: pair-direction n = i * dirs + d starts from the context features of frame i + d
    r = timed(F_ELT, 0, 0, [&] { return launch_init_state(stream, ctx_, h32_, hx_, hx2_, flow_, rows, Lhx, upd8_ ? 768 : 0, s8, hoist_ ? 256 : 128, P_, dirs); });
    if (r) return r;

    if (debug && (r = snapshot("net0", h32_, (size_t)ND * P_ * 128 * 4, Stage::f32_rows(nullptr, ND, P_, 128)))) return r;

    // ---- the context features' share of the SepConvGRU gates, once per call (hoist_, see load()) ----
    const int mot = hoist_ ? 128 : 256;                     // channel offset of the motion features inside hx_ / hx2_
    if (hoist_) {
        PB_CHECK(rows * Lhx < (1LL << 31), PB_ERR_ARG, "flow_raft: %lld update-block rows exceed the 32-bit plane offset of the hoisted GRU share", (long long)rows);
        const int mx_saved = mx_;
        mx_ = 0;                                             // fp16 residual plane (these weights are packed without MX tiles)
        for (int half = 0; half < 2; ++half) {
            const int kh = half == 0 ? 1 : 5, kw = half == 0 ? 5 : 1;
            // [hi plane | lo plane]: lo_off = one whole plane, so both planes have the row stride of the tensor they are added to
            if ((r = conv(hx_ + 256, 128, Lhx, ND, h8_, w8_, kh, kw, 1, zr_in_[half], gz_[half], 256, ACT_NONE, 0, nullptr, nullptr, (int)(rows * 256)))) break;
            if ((r = conv(hx_ + 256, 128, Lhx, ND, h8_, w8_, kh, kw, 1, q_in_[half], gq_[half], Lhx, ACT_NONE, 0, nullptr, nullptr, (int)(rows * Lhx)))) break;
        }
        mx_ = mx_saved;
        if (r) return r;
    }

    // ---- GRU iterations (raft.py:124-144, update.py:122-136) ----
    for (int it = 0; it < iters; ++it) {
        if (alt_corr_) {       // --alternate_corr (corr.py:63-91): the window entries are computed from fmap_ and the pooled maps, 100 per row and level
            const f16 *const tg[4] = {fmap_, fpool_[1], fpool_[2], fpool_[3]};
            r = timed(F_GEMM, 2.0 * rows * 4.0 * 100.0 * 256.0, 0, [&] {
                return launch_corr_lookup_otf(stream, fmap_, tg, lh_, lw_, flow_, P_, w8_, corr_, rows, Lhx, upd8_ ? 768 : 0, s8, dirs);
            }, "corr_lookup_otf_kernel");
        } else {
            r = timed(F_ELT, 0, 0, [&] { return launch_corr_lookup(stream, pyr_, lh_, lw_, lwp_, lhp_, pld_, flow_, P_, w8_, corr_, rows, Lhx, upd8_ ? 768 : 0, s8, layout); });
        }
        if (r) return r;
        if (debug && it == 0 && (r = snapshot("corr0", corr_, (size_t)ND * P_ * Lhx * 2, Stage::f16_nhwc(nullptr, ND, 324, h8_, w8_, Lhx)))) return r;
        // BasicMotionEncoder.  With upd8_ every map is [a16 (C) | a8 (C bytes)] per pixel (pixel stride 1.5 C halfs): the conv epilogues
        // store the fp8 copy too (o8 = its byte offset from the output row: 2 Ctot - slice offset) and the MX segments read it
        if ((r = conv(corr_, 384, Lhx, ND, h8_, w8_, 1, 1, 1, convc1_, c1_, L256, ACT_RELU, 0, nullptr, nullptr, 0, 0, upd8_ ? 512 : 0))) return r;
        if ((r = conv(c1_, 256, L256, ND, h8_, w8_, 3, 3, 1, convc2_, corflo_, L256, ACT_RELU, 0, nullptr, nullptr, 0, 0, upd8_ ? 512 : 0))) return r;
        if (f1_direct_) {
            r = timed(F_CONV, 2.0 * rows * 128.0 * 98.0, 8.0 * rows + 256.0 * rows, [&] {
                return launch_convf1(stream, flow_, f1w_, convf1_.bias, f1_, rows, P_, h8_, w8_, L128, upd8_ ? 256 : 0, (float)(1 << kMx2Pa), f1_passes_);
            }, "convf1_kernel", (double)f1_passes_);
            if (r) return r;
        } else {
            r = timed(F_ELT, 0, 0, [&] { return launch_im2col7_flow(stream, flow_, ND, h8_, w8_, fa_, 128, L128, upd8_); });
            if (r) return r;
            if ((r = dense(fa_, L128, rows, convf1_, f1_, L128, ACT_RELU, nullptr, upd8_ ? 256 : 0, 0))) return r;     // flow is in pixels: its fp8 copy is unscaled
        }
        if ((r = conv(f1_, 128, L128, ND, h8_, w8_, 3, 3, 1, convf2_, corflo_ + 192, L256, ACT_RELU, 0, nullptr, nullptr, 0, 0, upd8_ ? 512 - 192 : 0))) return r;
        // HX = [h | inp | motion] feeds the z / r convs, HX2 = [r * h | inp | motion] the q conv: the motion features are
        // written to both by the producing conv (its ReLU'd second output), r * h and the state update by the GRU epilogues
        ConvFuse dup; dup.out2 = hx2_ + mot;
        if ((r = conv(corflo_, 256, L256, ND, h8_, w8_, 3, 3, 1, convm_, hx_ + mot, Lhx, ACT_RELU, 0, nullptr, &dup, 0, 0, upd8_ ? 768 - mot : 0))) return r;
        r = timed(F_ELT, 0, 0, [&] { return launch_put_flow(stream, flow_, hx_, hx2_, rows, Lhx, upd8_ ? 768 : 0, s8, mot + 126); });
        if (r) return r;
        // SepConvGRU: (1 x 5) then (5 x 1)
        for (int half = 0; half < 2; ++half) {
            const int kh = half == 0 ? 1 : 5, kw = half == 0 ? 5 : 1;
            const int gc = hoist_ ? 256 : 384;               // channels the per-iteration convolutions read: [h | motion] (+ inp without the hoist)
            ConvFuse fz; fz.gru_h = h32_; fz.gru_rh = hx2_; fz.gru_ld = Lhx; fz.add2 = hoist_ ? gz_[half] + rows * 256 : nullptr;
            // (upd8_: the fp8 copy of the [h | motion] slice starts 384 halfs after the pixel's first channel - conv()'s a8_rel - and the
            // epilogues store the new copies of r * h / h at byte 768 of the row)
            const int a8 = upd8_ && hoist_ ? 384 : 0;
            if ((r = conv(hx_, gc, Lhx, ND, h8_, w8_, kh, kw, 1, zr_[half], zrb_, 256, ACT_GRU_ZR, 0, hoist_ ? gz_[half] : nullptr, &fz, 0, a8, upd8_ ? 768 : 0))) return r;
            ConvFuse fq; fq.gru_h = h32_; fq.gru_z = zrb_; fq.add2 = hoist_ ? gq_[half] + rows * Lhx : nullptr;
            if ((r = conv(hx2_, gc, Lhx, ND, h8_, w8_, kh, kw, 1, q_[half], hx_, Lhx, ACT_GRU_Q, 0, hoist_ ? gq_[half] : nullptr, &fq, 0, a8, upd8_ ? 768 : 0))) return r;
        }
        // FlowHead -> delta_flow (fp32), coords1 += delta (the h slice's fp8 copy sits 384 halfs after it)
        if ((r = conv(hx_, 128, Lhx, ND, h8_, w8_, 3, 3, 1, fh1_, fh_, 256, ACT_RELU, 0, nullptr, nullptr, 0, upd8_ ? 384 : 0))) return r;
        r = timed(F_CONV, 2.0 * rows * 2.0 * fh2_.Kreal, 0, [&] { return launch_flow_head2(stream, fh_, fh2_.w, fh2_.bias, flow_, ND, h8_, w8_, fh2_.sw); },
                  fh2_.sw ? "flow_head2_kernel<true>" : "flow_head2_kernel<false>");
        if (r) return r;
        if (debug && it == 0 && (r = snapshot("flow_it0", flow_, (size_t)ND * P_ * 2 * 4, Stage::f32_rows(nullptr, ND, P_, 2)))) return r;
    }
    stages_["flow_lo"] = Stage::f32_rows(flow_, ND, P_, 2);

    // ---- mask head (last iteration only) + convex upsample + unpad + encode ----
    if ((r = conv(hx_, 128, Lhx, ND, h8_, w8_, 3, 3, 1, mk0_, m0_, 256, ACT_RELU, 0, nullptr, nullptr, 0, upd8_ ? 384 : 0))) return r;
    {
        GemmArgs a;
        a.A = m0_; a.lda = 256; a.N = 576; a.M = (int)rows;
        set_weights(a, mk2_, false);
        a.out32 = mask_; a.ldo = 576; a.scale = 0.25f;
        r = timed_gemm(F_GEMM, 2.0 * rows * 576.0 * 256, 0, [&] { return launch_gemm(stream, A_DENSE, EPI_F32, TILE_AUTO, a); }, 1.0 + mk2_.sw);
        if (r) return r;
    }
    return flow_tail(flow_, ND, F - 1, h8_, w8_, 8, flow_out, rgb_out, maxdisp, mask_out, alpha1, alpha2);
}
