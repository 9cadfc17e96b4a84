// The pb_op_* entry points of libprisma_bands.so (include/prisma_bands.h): single kernels and single layers for the op-level tests and the
// bench tools.  No band runs through this file; context lifetime and the band entry points are in abi.hip.
#include <string.h>

#include <algorithm>
#include <vector>

#include "abi_ctx.h"
#include "corr_layout.h"
#include "flow_chunk.h"
#include "gmflow_engine.h"
#include "mask_kernels.h"
#include "zoe_kernels.h"

namespace {
// ---- one layer through EngineBase's own packing and launch code (pb_op_conv2d_split / pb_op_dense_split) ------------------------------
// The maps are built on the host the way the producing epilogues write them (gemm_kernels.h lo8_store2 / direct epilogue); the weights go
// through begin_load / pack_conv / pack / set_weights / conv() / dense() untouched, so the host packers are under test with the kernels.
enum { SL_F16 = 0, SL_SPLIT16 = 1, SL_MX3 = 2, SL_MX2 = 3 };

class SplitOpEngine : public EngineBase {
  public:
    explicit SplitOpEngine(int device) : EngineBase(device) {}
    int setup(const pb_tensor *t, int n, int layout, int tapin) {
        PB_TRY(begin_load(t, n));
        split_w_ = layout != SL_F16; mx_ = layout >= SL_MX3; pack_mx2_ = layout == SL_MX2; pack_tapin_ = tapin;
        return 0;
    }
    int pack_layer(bool is_conv, int sa, int N, int K, PackedW &w) {
        if (is_conv) return pack_conv("l", true, nullptr, nullptr, w, sa);
        const pb_tensor *tw = find("l.weight"), *tb = find("l.bias");
        PB_CHECK(tw && tb, PB_ERR_ARG, "split op: no weights");
        return pack((const float *)tw->data, N, K, (int)round_up(K, 64), w, (const float *)tb->data, 1, sa);
    }
    // host map of P rows of C fp32 values: f16 [hi], split16 [hi | lo (sa)], mx3 [hi | hi8 | lo8], mx2 [a16 | a8] (a8 of the fp16 value)
    void build_map(const float *x, int64_t P, int C, int Cp, int layout, int sa, int64_t ld, std::vector<f16> &h) const {
        for (int64_t p = 0; p < P; ++p) {
            f16 *row = h.data() + p * ld;
            unsigned char *r8 = (unsigned char *)(row + Cp);
            for (int c = 0; c < C; ++c) {
                const float v = x[p * C + c];
                const f16 hi = (f16)v;
                row[c] = hi;
                if (layout == SL_SPLIT16 && sa) row[Cp + c] = (f16)(v - (float)hi);
                if (layout == SL_MX3) {
                    r8[c] = pb_f32_to_e4m3(ldexpf((float)hi, kLo8Pa));
                    r8[Cp + c] = pb_f32_to_e4m3(ldexpf(v - (float)hi, kLo8Pa + 12));
                }
                if (layout == SL_MX2) r8[c] = pb_f32_to_e4m3(ldexpf((float)hi, kMx2Pa));
            }
        }
    }
    // skip tensor in the output's layout: [hi], [hi | lo] (fp16 residual) or [hi | hi8 | lo8] (e4m3 residual), C = lo_off
    void build_skip(const float *s, int M, int N, int C, int lo_off, bool lo8, int64_t ldo, std::vector<f16> &h) const {
        for (int m = 0; m < M; ++m) {
            f16 *row = h.data() + (int64_t)m * ldo;
            unsigned char *r8 = (unsigned char *)(row + C);
            for (int n = 0; n < N; ++n) {
                const float v = s[(int64_t)m * N + n];
                const f16 hi = (f16)v;
                row[n] = hi;
                if (lo_off && lo8) {
                    r8[n] = pb_f32_to_e4m3(ldexpf((float)hi, kLo8Pa));
                    r8[C + n] = pb_f32_to_e4m3(ldexpf(v - (float)hi, kLo8Pa + 12));
                } else if (lo_off) {
                    row[C + n] = (f16)(v - (float)hi);
                }
            }
        }
    }
    int run(bool is_conv, const float *x, const float *skip, int B, int H, int W, int Ci, int Ctot, int ci_off, int Co, int kh, int kw, int stride,
            int layout, int sa, int tile, int splitk, int split_out, int act, int pre_relu, int rows_out, void *out, int *info, char *kname, int kcap) {
        PB_CHECK(layout >= SL_F16 && layout <= SL_MX2 && Co % 8 == 0 && Ci > 0 && ci_off >= 0 && ci_off + Ci <= Ctot, PB_ERR_ARG, "split op: bad arguments");
        if (layout != SL_SPLIT16) sa = layout == SL_MX3;
        PackedW w;
        const int K = is_conv ? 0 : Ci;
        PB_TRY(pack_layer(is_conv, sa, Co, K, w));
        const int Cp = (int)round_up(Ci, 64);
        // the map: mx2 carries Ctot channels per pixel [a16 (Ctot) | a8 (Ctot bytes)] and the layer reads the slice [ci_off, ci_off + Ci)
        const bool m2 = w.mx2 != 0;
        PB_CHECK(m2 || w.mx3 || (Ctot == Ci && ci_off == 0), PB_ERR_ARG, "split op: a channel slice needs the mx2 layout");
        PB_CHECK(!m2 || (Ctot % 128 == 0 && ci_off % 16 == 0), PB_ERR_ARG, "split op: mx2 map of %d channels, slice at %d", Ctot, ci_off);
        const int Cm = m2 ? Ctot : Cp;
        const int64_t ld = m2 ? Cm + Cm / 2 : (w.mx3 ? 2 * Cp : (w.sa ? 2 * Cp : Cp));
        const int64_t P = is_conv ? (int64_t)B * H * W : B;
        const int OH = is_conv ? (H + 2 * (kh / 2) - kh) / stride + 1 : 1, OW = is_conv ? (W + 2 * (kw / 2) - kw) / stride + 1 : 1;
        const int64_t M = is_conv ? (int64_t)B * OH * OW : B;
        const int C = (int)round_up(Co, 64), lo_off = split_out ? C : 0;
        const int64_t ldo = split_out ? 2 * C : C;
        const bool lo8 = split_out && mx_;
        PB_CHECK(rows_out >= round_up(M, 256), PB_ERR_ARG, "split op: the output holds %d rows, the launch writes %lld", rows_out, (long long)M);
        std::vector<f16> hx((size_t)round_up(P, 256) * ld, (f16)0.f);
        std::vector<float> xpad;
        const float *xs = x;
        if (Cm != (m2 ? Ctot : Ci)) {          // channels padded to 64 with zeros
            xpad.assign((size_t)P * Cm, 0.f);
            for (int64_t p = 0; p < P; ++p) memcpy(&xpad[(size_t)p * Cm], x + p * Ci, (size_t)Ci * 4);
            xs = xpad.data();
        }
        build_map(xs, P, Cm, m2 ? Cm : Cp, m2 ? SL_MX2 : (w.mx3 ? SL_MX3 : (w.sa ? SL_SPLIT16 : SL_F16)), w.sa, ld, hx);
        DevMem dx, dout, dskip, dsk;
        PB_TRY(dx.alloc(hx.size() * 2));
        PB_HIP(hipMemcpy(dx.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
        PB_TRY(dout.alloc((size_t)rows_out * ldo * 2));
        PB_HIP(hipMemset(dout.p, 0xFF, (size_t)rows_out * ldo * 2));            // 0xFFFF: an fp16 NaN, 0xFF: an e4m3 NaN
        if (skip) {
            std::vector<f16> hs((size_t)rows_out * ldo, (f16)0.f);
            build_skip(skip, (int)M, Co, C, lo_off, lo8, ldo, hs);
            PB_TRY(dskip.alloc(hs.size() * 2));
            PB_HIP(hipMemcpy(dskip.p, hs.data(), hs.size() * 2, hipMemcpyHostToDevice));
        }
        if (splitk) {
            PB_TRY(dsk.alloc((size_t)512 * 128 * 128 * 4));
            sk_ws_ = dsk.as<float>(); sk_cap_ = (int64_t)512 * 128 * 128;
        }
        PB_HIP(hipDeviceSynchronize());
        pb_gemm_set_last_kernel("");
        const f16 *in = dx.as<f16>() + (m2 ? ci_off : 0);
        int r;
        if (is_conv) {
            conv_tile = tile;
            r = conv(in, Cp, m2 ? (int)ld : 0, B, H, W, kh, kw, stride, w, dout.as<f16>(), (int)ldo, act, pre_relu, dskip.as<f16>(), nullptr, lo_off,
                     m2 ? Ctot - ci_off / 2 : 0);
        } else {
            dense_tile = tile;
            PB_CHECK(!pre_relu, PB_ERR_ARG, "split op: dense() has no pre_relu");
            r = dense(in, (int)ld, M, w, dout.as<f16>(), (int)ldo, act, dskip.as<f16>(), 0, -1, lo_off);
        }
        sk_ws_ = nullptr; sk_cap_ = 0;
        if (r) return r;
        PB_HIP(hipStreamSynchronize(stream));
        PB_HIP(hipMemcpy(out, dout.p, (size_t)rows_out * ldo * 2, hipMemcpyDeviceToHost));
        if (info) {
            const int v[13] = {w.mx_pw, m2 ? kMx2Pa : kLo8Pa, w.mx3, w.mx2, w.sa, w.sw, w.tapin, w.K, w.wcw != nullptr, w.Cseg, (int)ldo, lo8, kLo8Pa};
            memcpy(info, v, sizeof(v));
        }
        if (kname && kcap > 0) snprintf(kname, kcap, "%s", pb_gemm_last_kernel());
        return 0;
    }
};

// ---- the flow_raft band's own kernels one by one (pb_op_raft_*) -----------------------------------------------------------------------
// Every entry point calls the launcher RaftEngine::infer calls (FlowEngine's encoder and tail included), with the engine's arguments; host maps
// are built by build_map above, weights go through EngineBase::pack / pack_conv / convf1_pack.  Output buffers are preset to 0xFF bytes (an fp16 / fp32 / e4m3 NaN) with guard
// rows behind the last row, so a test can tell what the kernel did NOT write.
class RaftOpEngine : public SplitOpEngine {
  public:
    explicit RaftOpEngine(int device) : SplitOpEngine(device) {}
    static int up(DevMem &d, const void *src, size_t bytes) {
        PB_TRY(d.alloc(bytes));
        PB_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    static int preset(DevMem &d, size_t bytes) {
        PB_TRY(d.alloc(bytes));
        PB_HIP(hipMemset(d.p, 0xFF, bytes));
        PB_HIP(hipDeviceSynchronize());
        return 0;
    }
    int to_f16(DevMem &d, const float *x, int64_t rows, int C, size_t min_bytes = 0) {
        std::vector<f16> h((size_t)rows * C);
        build_map(x, rows, C, C, SL_F16, 0, C, h);
        PB_TRY(d.alloc(std::max(h.size() * 2, min_bytes)));
        PB_HIP(hipMemcpy(d.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        return 0;
    }
    int finish(void *out, const DevMem &d, size_t bytes) {
        PB_HIP(hipStreamSynchronize(stream));
        PB_HIP(hipMemcpy(out, d.p, bytes, hipMemcpyDeviceToHost));
        return 0;
    }

    // layout (corr_layout.h): how the volume between the two kernels is stored - the ctx's "corr_layout" option, as RaftEngine follows it
    int lookup(const float *fmap1, const float *fmap2, const float *flow, int n, int h8, int w8, int o8, int guard_rows, void *out, float *levels,
               int layout) {
        PB_CHECK(h8 >= 16 && w8 >= 16, PB_ERR_ARG, "op_raft_lookup: a %d x %d grid is too small (the 4-level pyramid needs >= 16 x 16)", h8, w8);
        CorrGeo g;
        corr_pyramid_geometry(h8, w8, g);
        const int P = h8 * w8;
        const int64_t rows = (int64_t)n * P, Pv = corr_layout_rows(layout, P);      // Pv: volume rows a pair-direction is carved for
        const size_t slack = 1 << 20;                       // what RaftEngine::prepare leaves behind fmap_ and every pyramid buffer
        const int ldo = o8 ? 576 : 384;
        DevMem f1, f2, dflow, dout, fpool[4], ftile[4], pyr[4];
        PB_TRY(to_f16(f1, fmap1, rows, 256, (size_t)round_up(rows, 256) * 256 * 2 + slack));
        PB_TRY(to_f16(f2, fmap2, rows, 256, (size_t)round_up(rows, 256) * 256 * 2 + slack));
        PB_TRY(up(dflow, flow, (size_t)rows * 8));
        PB_TRY(preset(dout, (size_t)(rows + guard_rows) * ldo * 2));
        const f16 *lv[4];
        for (int l = 0; l < 4; ++l) {
            PB_TRY(pyr[l].alloc((size_t)n * Pv * g.ld[l] * 2 + slack));
            if (l) PB_TRY(fpool[l].alloc((size_t)round_up((int64_t)n * g.h[l] * g.w[l], 256) * 256 * 2 + slack));
            PB_TRY(ftile[l].alloc((size_t)(n * (int64_t)g.ld[l] + 256) * 256 * 2 + slack));
            lv[l] = pyr[l].as<f16>();
        }
        for (int l = 0; l < 4; ++l) {
            if (l > 0) PB_TRY(launch_avgpool2_nhwc(stream, l == 1 ? f2.as<f16>() : fpool[l - 1].as<f16>(), fpool[l].as<f16>(), n, g.h[l - 1], g.w[l - 1], 256));
            PB_TRY(launch_corr_tile(stream, l == 0 ? f2.as<f16>() : fpool[l].as<f16>(), ftile[l].as<f16>(), n, g.h[l], g.w[l], g.wp[l], g.ld[l]));
        }
        for (int i = 0; i < n; ++i)
            for (int l = 0; l < 4; ++l)
                PB_TRY(launch_corr_volume(stream, f1.as<f16>() + (int64_t)i * P * 256, P, ftile[l].as<f16>() + (int64_t)i * g.ld[l] * 256, g.ld[l], g.ld[l],
                                          pyr[l].as<f16>() + (int64_t)i * Pv * g.ld[l], g.ld[l], layout));
        PB_TRY(launch_corr_lookup(stream, lv, g.h, g.w, g.wp, g.hp, g.ld, dflow.as<float>(), P, w8, dout.as<f16>(), rows, ldo, o8 ? 768 : 0,
                                  (float)(1 << kMx2Pa), layout));
        PB_TRY(finish(out, dout, (size_t)(rows + guard_rows) * ldo * 2));
        if (levels) {                                       // the four levels, de-blocked and de-tiled: [n P, h_l, w_l] one after the other
            float *dst = levels;
            for (int l = 0; l < 4; ++l) {
                std::vector<f16> h((size_t)n * Pv * g.ld[l]);
                PB_HIP(hipMemcpy(h.data(), pyr[l].p, h.size() * 2, hipMemcpyDeviceToHost));
                const int wt = g.wp[l] >> 3;
                for (int64_t r = 0; r < rows; ++r) {
                    const f16 *hn = h.data() + (size_t)(r / P) * Pv * g.ld[l];
                    const int p = (int)(r % P);
                    for (int y = 0; y < g.h[l]; ++y)
                        for (int x = 0; x < g.w[l]; ++x)
                            *dst++ = (float)hn[corr_layout_index(layout, p, ((y >> 3) * wt + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7), g.ld[l])];
                }
            }
        }
        return 0;
    }

    // --alternate_corr: RaftEngine::infer's sequence with alt_corr_ - three pooling passes, then the lookup straight from the feature maps
    int lookup_otf(const float *fmap1, const float *fmap2, const float *flow, int n, int h8, int w8, int o8, int guard_rows, void *out) {
        PB_CHECK(h8 >= 16 && w8 >= 16, PB_ERR_ARG, "op_raft_lookup_otf: a %d x %d grid is too small (the 4-level pyramid needs >= 16 x 16)", h8, w8);
        CorrGeo g;
        corr_pyramid_geometry(h8, w8, g);
        const int P = h8 * w8;
        const int64_t rows = (int64_t)n * P;
        const size_t slack = 1 << 20;
        const int ldo = o8 ? 576 : 384;
        DevMem f1, f2, dflow, dout, fpool[4];
        PB_TRY(to_f16(f1, fmap1, rows, 256, (size_t)round_up(rows, 256) * 256 * 2 + slack));
        PB_TRY(to_f16(f2, fmap2, rows, 256, (size_t)round_up(rows, 256) * 256 * 2 + slack));
        PB_TRY(up(dflow, flow, (size_t)rows * 8));
        PB_TRY(preset(dout, (size_t)(rows + guard_rows) * ldo * 2));
        for (int l = 1; l < 4; ++l) {
            PB_TRY(fpool[l].alloc((size_t)round_up((int64_t)n * g.h[l] * g.w[l], 256) * 256 * 2 + slack));
            PB_TRY(launch_avgpool2_nhwc(stream, l == 1 ? f2.as<f16>() : fpool[l - 1].as<f16>(), fpool[l].as<f16>(), n, g.h[l - 1], g.w[l - 1], 256));
        }
        const f16 *const tg[4] = {f2.as<f16>(), fpool[1].as<f16>(), fpool[2].as<f16>(), fpool[3].as<f16>()};
        PB_TRY(launch_corr_lookup_otf(stream, f1.as<f16>(), tg, g.h, g.w, dflow.as<float>(), P, w8, dout.as<f16>(), rows, ldo, o8 ? 768 : 0,
                                      (float)(1 << kMx2Pa), 0));
        return finish(out, dout, (size_t)(rows + guard_rows) * ldo * 2);
    }

    int convf1(const float *flow, const float *wt, const float *bias, int n, int h8, int w8, int passes, int o8, int gemm, int guard_rows, void *out) {
        const int P = h8 * w8, ldo = o8 ? 192 : 128;
        const int64_t rows = (int64_t)n * P, rows_buf = round_up(rows + guard_rows, 256);
        DevMem dflow, dout, dw, db, fa;
        PB_TRY(up(dflow, flow, (size_t)rows * 8));
        PB_TRY(preset(dout, (size_t)rows_buf * ldo * 2));
        if (!gemm) {
            std::vector<f16> hw((size_t)convf1_packed_halfs(passes));
            convf1_pack(wt, passes, hw.data());
            PB_TRY(up(dw, hw.data(), hw.size() * 2));
            PB_TRY(up(db, bias, 128 * 4));
            PB_TRY(launch_convf1(stream, dflow.as<float>(), dw.as<f16>(), db.as<float>(), dout.as<f16>(), rows, P, h8, w8, ldo, o8 ? 256 : 0,
                                 (float)(1 << kMx2Pa), passes));
        } else {        // PB_CONVF1_DIRECT=0: im2col order k = tap * 2 + c, K 98 -> 128, then the GEMM (RaftEngine::load / infer)
            PB_CHECK(passes == 2 || !o8, PB_ERR_ARG, "op_raft_convf1: the GEMM path reads fp8 copies only in the split mode");
            split_w_ = passes == 2; mx_ = o8; pack_mx2_ = o8; pack_tapin_ = 0;
            std::vector<float> g((size_t)128 * 98);
            for (int o = 0; o < 128; ++o)
                for (int c = 0; c < 2; ++c)
                    for (int tp = 0; tp < 49; ++tp) g[(size_t)o * 98 + tp * 2 + c] = wt[((size_t)o * 2 + c) * 49 + tp];
            PackedW w;
            PB_TRY(pack(g.data(), 128, 98, 128, w, bias));
            PB_TRY(fa.alloc((size_t)round_up(rows, 256) * ldo * 2));
            PB_TRY(launch_im2col7_flow(stream, dflow.as<float>(), n, h8, w8, fa.as<f16>(), 128, ldo, o8));
            PB_TRY(dense(fa.as<f16>(), ldo, rows, w, dout.as<f16>(), ldo, ACT_RELU, nullptr, o8 ? 256 : 0, 0));
        }
        return finish(out, dout, (size_t)(rows + guard_rows) * ldo * 2);
    }

    int flow_head2(const float *x, float *flow, int n, int H, int W, int split, int guard_rows) {
        // as RaftEngine::load packs flow_head.conv2: fp16 residuals (no mx2), tap-major, N = 8
        split_w_ = split; mx_ = split; pack_mx2_ = 0; pack_tapin_ = 0;
        PackedW w;
        PB_TRY(pack_conv("l", true, nullptr, nullptr, w));
        w.N = 8;
        const int64_t rows = (int64_t)n * H * W;
        DevMem dx, dflow;
        PB_TRY(to_f16(dx, x, rows, 256));
        PB_TRY(preset(dflow, (size_t)(rows + guard_rows) * 8));
        PB_HIP(hipMemcpy(dflow.p, flow, (size_t)rows * 8, hipMemcpyHostToDevice));
        PB_TRY(launch_flow_head2(stream, dx.as<f16>(), w.w, w.bias, dflow.as<float>(), n, H, W, w.sw));
        return finish(flow, dflow, (size_t)(rows + guard_rows) * 8);
    }

    int upsample(const float *flow, const float *mask, int n, int h8, int w8, int pad_l, int pad_t, int sh, int sw, int guard, float *upo, float *maxd,
                 int factor = 8) {
        const int64_t rows = (int64_t)n * h8 * w8, px = (int64_t)n * sh * sw;
        DevMem dflow, dmask, dup, dmax, dmx;
        PB_TRY(up(dflow, flow, (size_t)rows * 8));
        PB_TRY(up(dmask, mask, (size_t)rows * 9 * factor * factor * 4));
        PB_TRY(preset(dup, (size_t)(px * 2 + guard) * 4));
        PB_TRY(preset(dmax, (size_t)n * 4));
        PB_TRY(dmx.alloc((size_t)n * 4));
        PB_TRY(launch_upsample(stream, dflow.as<float>(), dmask.as<float>(), n, h8, w8, pad_l, pad_t, sh, sw, dup.as<float>(), dmax.as<unsigned>(),
                               factor));
        PB_TRY(launch_flow_encode(stream, dup.as<float>(), n, sh, sw, dmax.as<unsigned>(), nullptr, dmx.as<float>()));     // decodes maxd, no colours
        PB_TRY(finish(upo, dup, (size_t)(px * 2 + guard) * 4));
        PB_HIP(hipMemcpy(maxd, dmx.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return 0;
    }

    // The flow bands' frame path outside the networks (pb_op_flow_*).  flow_prep: ONE launch_raft_prep as FlowEngine::prep_frames issues it -
    // always space-to-depth, the geometry of flow_geometry (GmflowEngine::prepare_g's override with an inference size), the tap tables of
    // upload_resize_tables - plus the scaled uint8 frame the engines never ask for.  layout 0: 64 halfs per 4 x 4 block, 1: [hi | lo],
    // 2: [hi | hi8 | lo8] (128 halfs per block)
    int flow_prep(const uint8_t *frames, int n, int H, int W, float scale, int factor, int layout, int norm_mode, int isz_h, int isz_w,
                  int guard_rows, int guard, void *out, uint8_t *scaled, int *lo8_pa) {
        FlowGeometry g = flow_geometry(H, W, scale, factor);
        if (isz_h > 0) { g.padl = g.padt = 0; g.Hp = isz_h; g.Wp = isz_w; }
        PB_CHECK(g.sh > 0 && g.sw > 0 && g.Hp % 4 == 0 && g.Wp % 4 == 0, PB_ERR_ARG, "op_flow_prep: %d x %d scaled, %d x %d padded", g.sh, g.sw, g.Hp, g.Wp);
        const int resize = scale != 1.f;
        DevMem df, dxi, dxc, dyi, dyc, dout, dsc;
        if (resize) {
            std::vector<int> xi, xc, yi, yc;
            pb_flow_cubic_taps(W, g.sw, scale, xi, xc);
            pb_flow_cubic_taps(H, g.sh, scale, yi, yc);
            for (int v : xi) PB_CHECK(v >= 0 && v < W, PB_ERR_STATE, "op_flow_prep: x tap %d outside a row of %d pixels", v, W);
            for (int v : yi) PB_CHECK(v >= 0 && v < H, PB_ERR_STATE, "op_flow_prep: y tap %d outside %d rows", v, H);
            PB_TRY(up(dxi, xi.data(), xi.size() * 4)); PB_TRY(up(dxc, xc.data(), xc.size() * 4));
            PB_TRY(up(dyi, yi.data(), yi.size() * 4)); PB_TRY(up(dyc, yc.data(), yc.size() * 4));
        }
        const int lo_off = layout ? 64 : 0, ld = layout ? 128 : 64;
        const int64_t rows = (int64_t)n * (g.Hp / 4) * (g.Wp / 4);
        const size_t ob = (size_t)(rows + guard_rows) * ld * 2, sb = (size_t)n * g.sh * g.sw * 3 + guard;
        PB_TRY(up(df, frames, (size_t)n * H * W * 3));
        PB_TRY(preset(dout, ob)); PB_TRY(preset(dsc, sb));
        PB_TRY(launch_raft_prep(stream, df.as<uint8_t>(), n, H, W, g.sh, g.sw, g.Hp, g.Wp, g.padl, g.padt, resize, dxi.as<int>(), dxc.as<int>(), dyi.as<int>(),
                                dyc.as<int>(), dout.as<f16>(), dsc.as<uint8_t>(), 1, lo_off, layout == 2 ? kLo8Pa : -1, norm_mode, isz_h > 0));
        PB_TRY(finish(out, dout, ob));
        PB_HIP(hipMemcpy(scaled, dsc.p, sb, hipMemcpyDeviceToHost));
        if (lo8_pa) *lo8_pa = kLo8Pa;
        return 0;
    }

    // in [n, ih, iw, 2] -> out [n, sh, sw, 2] + guard floats, maxd [n] as the encode kernel decodes it (its words preset, not zeroed)
    int flow_resize_back(const float *in, int n, int ih, int iw, int sh, int sw, int guard, float *out, float *maxd) {
        const int64_t px = (int64_t)n * sh * sw;
        DevMem din, dout, dmax, dmx;
        PB_TRY(up(din, in, (size_t)n * ih * iw * 8));
        PB_TRY(preset(dout, (size_t)(px * 2 + guard) * 4));
        PB_TRY(preset(dmax, (size_t)n * 4));
        PB_TRY(dmx.alloc((size_t)n * 4));
        PB_TRY(launch_flow_resize_back(stream, din.as<float>(), n, ih, iw, sh, sw, dout.as<float>(), dmax.as<unsigned>()));
        PB_TRY(launch_flow_encode(stream, dout.as<float>(), n, sh, sw, dmax.as<unsigned>(), nullptr, dmx.as<float>()));
        PB_TRY(finish(out, dout, (size_t)(px * 2 + guard) * 4));
        PB_HIP(hipMemcpy(maxd, dmx.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return 0;
    }

    // flow [n, sh, sw, 2], maxd [n] (stored in the ordered-unsigned form of the kernels' atomicMax) -> rgb [n, sh, sw, 3] + guard bytes, max_out [n]
    int flow_encode(const float *flow, const float *maxd, int n, int sh, int sw, int guard, uint8_t *rgb, float *max_out) {
        const int64_t px = (int64_t)n * sh * sw;
        std::vector<unsigned> ord((size_t)n);
        for (int i = 0; i < n; ++i) {
            unsigned u;
            memcpy(&u, maxd + i, 4);
            ord[i] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        }
        DevMem dflow, drgb, dmax, dmx;
        PB_TRY(up(dflow, flow, (size_t)px * 8));
        PB_TRY(up(dmax, ord.data(), (size_t)n * 4));
        PB_TRY(preset(drgb, (size_t)px * 3 + guard));
        PB_TRY(preset(dmx, (size_t)n * 4));
        PB_TRY(launch_flow_encode(stream, dflow.as<float>(), n, sh, sw, dmax.as<unsigned>(), drgb.as<uint8_t>(), dmx.as<float>()));
        PB_TRY(finish(rgb, drgb, (size_t)px * 3 + guard));
        PB_HIP(hipMemcpy(max_out, dmx.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return 0;
    }

    // layout 0: [C] fp16, 1: [hi | lo], 2: [hi | hi8 | lo8]; bmode 0: no second operand, 1: raw, 2: normalised with its own statistics
    int instnorm(const float *a, const float *b, int B, int HW, int C, int layout, int stats_lo, int bmode, int inplace, int guard_rows,
                 float *stats_out, void *out) {
        const int ld = layout ? 2 * C : C, lo_off = layout ? C : 0, l8 = layout == 2 ? kLo8Pa : -1;
        const int sl = layout == 0 ? SL_F16 : (layout == 1 ? SL_SPLIT16 : SL_MX3);
        const int64_t rows = (int64_t)B * HW;
        std::vector<f16> ha((size_t)(rows + guard_rows) * ld), hb;
        memset(ha.data(), 0xFF, ha.size() * 2);
        build_map(a, rows, C, C, sl, 1, ld, ha);
        DevMem da, db, dout, part, st, st2;
        PB_TRY(up(da, ha.data(), ha.size() * 2));
        if (bmode) {
            hb.assign((size_t)rows * ld, (f16)0.f);
            build_map(b, rows, C, C, sl, 1, ld, hb);
            PB_TRY(up(db, hb.data(), hb.size() * 2));
        }
        if (!inplace) PB_TRY(preset(dout, (size_t)(rows + guard_rows) * ld * 2));
        PB_TRY(part.alloc((size_t)in_stats_chunks(HW) * B * 256 * 2 * 4));
        PB_TRY(st.alloc((size_t)B * 256 * 2 * 4)); PB_TRY(st2.alloc((size_t)B * 256 * 2 * 4));
        PB_TRY(launch_in_stats(stream, da.as<f16>(), B, HW, C, ld, part.as<float>(), st.as<float>(), stats_lo ? lo_off : 0, l8));
        if (bmode == 2) PB_TRY(launch_in_stats(stream, db.as<f16>(), B, HW, C, ld, part.as<float>(), st2.as<float>(), stats_lo ? lo_off : 0, l8));
        DevMem &o = inplace ? da : dout;
        PB_TRY(launch_in_apply(stream, da.as<f16>(), st.as<float>(), bmode ? db.as<f16>() : nullptr, bmode == 2 ? st2.as<float>() : nullptr, o.as<f16>(),
                               B, HW, C, ld, lo_off, l8));
        PB_TRY(finish(out, o, (size_t)(rows + guard_rows) * ld * 2));
        PB_HIP(hipMemcpy(stats_out, st.p, (size_t)B * C * 2 * 4, hipMemcpyDeviceToHost));
        return 0;
    }

    int state(const float *cx, const float *flow, int64_t rows, int ld, int inp_off, int guard_rows, float *h32, void *hx, void *hx2, float *flow0) {
        const int o8_off = ld == 576 ? 768 : 0, mot = inp_off == 256 ? 128 : 256;      // RaftEngine::infer: hoist_ ? [h | motion | inp] : [h | inp | motion]
        const float s8 = (float)(1 << kMx2Pa);
        DevMem dc, dh32, dhx, dhx2, dflow;
        PB_TRY(to_f16(dc, cx, rows, 256));
        PB_TRY(preset(dh32, (size_t)(rows + guard_rows) * 128 * 4));
        PB_TRY(preset(dhx, (size_t)(rows + guard_rows) * ld * 2)); PB_TRY(preset(dhx2, (size_t)(rows + guard_rows) * ld * 2));
        PB_TRY(preset(dflow, (size_t)(rows + guard_rows) * 8));
        PB_TRY(launch_init_state(stream, dc.as<f16>(), dh32.as<float>(), dhx.as<f16>(), dhx2.as<f16>(), dflow.as<float>(), rows, ld, o8_off, s8, inp_off));
        PB_TRY(finish(flow0, dflow, (size_t)(rows + guard_rows) * 8));
        PB_HIP(hipMemcpy(dflow.p, flow, (size_t)rows * 8, hipMemcpyHostToDevice));
        PB_TRY(launch_put_flow(stream, dflow.as<float>(), dhx.as<f16>(), dhx2.as<f16>(), rows, ld, o8_off, s8, mot + 126));
        PB_TRY(finish(h32, dh32, (size_t)(rows + guard_rows) * 128 * 4));
        PB_HIP(hipMemcpy(hx, dhx.p, (size_t)(rows + guard_rows) * ld * 2, hipMemcpyDeviceToHost));
        PB_HIP(hipMemcpy(hx2, dhx2.p, (size_t)(rows + guard_rows) * ld * 2, hipMemcpyDeviceToHost));
        return 0;
    }
};

// ---- the flow_gmflow band's own kernels one by one (pb_op_gm_*, pb_op_attention128_cfg) ------------------------------------------------
// Every entry point calls the launcher GmflowEngine::infer calls, with the arguments infer gives it; the window geometry comes from
// gm_geometry, the function prepare_g plans with.  Raw output buffers are preset to 0xFF bytes and carry guard rows, as the raft ops above.
class GmOpEngine : public RaftOpEngine {
  public:
    explicit GmOpEngine(int device) : RaftOpEngine(device) {}
    static constexpr size_t kSlack = 1 << 16;               // what prepare_g leaves behind every fp16 buffer
    GmGeom g{};
    int ldvP = 0;
    // splits 2: the 1/8 grid and its 2 x 2 windows; 8: the two-scale model's 1/4 grid and its 8 x 8 windows
    int geom(int h8, int w8, int splits = 2) {
        PB_CHECK((splits == 2 || splits == 8) && h8 >= 2 * splits && w8 >= 2 * splits && h8 % splits == 0 && w8 % splits == 0, PB_ERR_ARG,
                 "op_gm: a %d x %d token grid (multiples of the %d splits, at least two tokens per window and axis)", h8, w8, splits);
        gm_geometry(h8, w8, g, ldvP, splits);
        return 0;
    }
    int down(void *dst, const DevMem &d, size_t bytes) {
        PB_HIP(hipMemcpy(dst, d.p, bytes, hipMemcpyDeviceToHost));
        return 0;
    }

    int tokens(const float *feat, const float *pos, int NP, int P, int guard, float *X, void *Xs) {
        const int64_t R = (int64_t)NP * 2 * P;
        DevMem df, dp, dX, dXs;
        PB_TRY(up(df, feat, (size_t)(NP + 1) * P * 128 * 4)); PB_TRY(up(dp, pos, (size_t)P * 128 * 4));
        PB_TRY(preset(dX, (size_t)(R + guard) * 128 * 4)); PB_TRY(preset(dXs, (size_t)(R + guard) * 256 * 2));
        PB_TRY(launch_gm_tokens(stream, df.as<float>(), dp.as<float>(), dX.as<float>(), dXs.as<f16>(), NP, P));
        PB_TRY(finish(X, dX, (size_t)(R + guard) * 128 * 4));
        return down(Xs, dXs, (size_t)(R + guard) * 256 * 2);
    }

    // the fine scale's tokens: feat [frames, P, 128], warped [B, P, 128], batch element b = pair * dirs + d takes frame pair + d as its source
    int tokens_warped(const float *feat, const float *warped, const float *pos, int B, int dirs, int P, int guard, float *X, void *Xs) {
        const int64_t R = (int64_t)B * 2 * P;
        DevMem df, dw, dp, dX, dXs;
        PB_TRY(up(df, feat, (size_t)(B / dirs + 1) * P * 128 * 4)); PB_TRY(up(dw, warped, (size_t)B * P * 128 * 4)); PB_TRY(up(dp, pos, (size_t)P * 128 * 4));
        PB_TRY(preset(dX, (size_t)(R + guard) * 128 * 4)); PB_TRY(preset(dXs, (size_t)(R + guard) * 256 * 2));
        PB_TRY(launch_gm_tokens(stream, df.as<float>(), dp.as<float>(), dX.as<float>(), dXs.as<f16>(), B, P, dw.as<float>(), dirs));
        PB_TRY(finish(X, dX, (size_t)(R + guard) * 128 * 4));
        return down(Xs, dXs, (size_t)(R + guard) * 256 * 2);
    }

    // flow8 [B, h8 w8, 2], feat4 [B / dirs + 1, 4 h8 w8, 128] -> flow_up (4 B h8 w8 + guard) x 2, warped (4 B h8 w8 + guard) x 128 floats
    int warp(const float *flow8, const float *feat4, int B, int dirs, int h8, int w8, int guard, float *flow_up, float *warped) {
        const int64_t P8 = (int64_t)h8 * w8, n4 = (int64_t)B * 4 * P8;
        DevMem df, dx, du, dw;
        PB_TRY(up(df, flow8, (size_t)B * P8 * 2 * 4)); PB_TRY(up(dx, feat4, (size_t)(B / dirs + 1) * 4 * P8 * 128 * 4));
        PB_TRY(preset(du, (size_t)(n4 + guard) * 2 * 4)); PB_TRY(preset(dw, (size_t)(n4 + guard) * 128 * 4));
        PB_TRY(launch_gm_warp(stream, df.as<float>(), dx.as<float>(), du.as<float>(), dw.as<float>(), B, dirs, h8, w8));
        PB_TRY(finish(flow_up, du, (size_t)(n4 + guard) * 2 * 4));
        return down(warped, dw, (size_t)(n4 + guard) * 128 * 4);
    }

    int split_rows(const float *src, int64_t rows, int ld, int C, int guard, void *out) {
        DevMem ds, dd;
        PB_TRY(up(ds, src, (size_t)rows * ld * 4));
        PB_TRY(preset(dd, (size_t)(rows + guard) * 2 * C * 2));
        PB_TRY(launch_gm_split_rows(stream, ds.as<float>(), ld, C, dd.as<f16>(), rows));
        return finish(out, dd, (size_t)(rows + guard) * 2 * C * 2);
    }

    int grid_vt(int guard, void *out) {
        DevMem dv;
        PB_TRY(preset(dv, (size_t)(64 + guard) * ldvP * 2));
        PB_TRY(launch_gm_grid_vt(stream, dv.as<f16>(), g.P, g.w8, ldvP));
        return finish(out, dv, (size_t)(64 + guard) * ldvP * 2);
    }

    size_t pack_bytes(int Bw, int is_vt, int guard) const {
        return is_vt ? ((size_t)Bw * 2 * 128 + guard) * g.ldv * 2 : ((size_t)Bw * g.Lw + guard) * 256 * 2;
    }
    int pack(const float *src, int images, int ld, int njobs, const int *cols, const int *kinds, int shifted, int guard, void **outs) {
        const int Bw = images * g.ns * g.ns;
        DevMem ds, dd[5];
        PB_TRY(up(ds, src, (size_t)images * g.P * ld * 4));
        GmPackJobs jobs{};
        jobs.n = njobs;
        for (int j = 0; j < njobs; ++j) {
            PB_TRY(preset(dd[j], pack_bytes(Bw, kinds[j], guard)));
            jobs.j[j] = GmPackJob{ds.as<float>(), ld, cols[j], dd[j].as<f16>(), kinds[j]};
        }
        PB_TRY(launch_gm_pack(stream, jobs, g, Bw, shifted));
        PB_HIP(hipStreamSynchronize(stream));
        for (int j = 0; j < njobs; ++j) PB_TRY(down(outs[j], dd[j], pack_bytes(Bw, kinds[j], guard)));
        return 0;
    }

    // X arrives with its guard rows (the caller presets them) and is returned whole: mode 1 must leave every byte of it alone
    int ln(const float *M, const float *gamma, const float *beta, float *X, int64_t rows, int64_t xrows, int windowed, int shifted, int mode, int guard,
           void *out) {
        const int ldo = mode ? 512 : 256;
        DevMem dM, dg, db, dX, dout;
        PB_TRY(up(dM, M, (size_t)rows * 128 * 4)); PB_TRY(up(dg, gamma, 128 * 4)); PB_TRY(up(db, beta, 128 * 4));
        PB_TRY(up(dX, X, (size_t)(xrows + guard) * 128 * 4));
        PB_TRY(preset(dout, (size_t)(xrows + guard) * ldo * 2));
        PB_TRY(launch_gm_ln(stream, dM.as<float>(), dg.as<float>(), db.as<float>(), dX.as<float>(), dout.as<f16>(), rows, g, windowed, shifted, mode));
        PB_TRY(finish(X, dX, (size_t)(xrows + guard) * 128 * 4));
        return down(out, dout, (size_t)(xrows + guard) * ldo * 2);
    }

    // stand-alone: Vt is NOT zeroed first (0xFF preset), so the test sees exactly which halfs the kernel owns; the engine and the two flow
    // chains below rely on commit_arena's memset for rows 2..31, 34..63 and the pad columns
    int match_flow(const float *O, int B, int guard, float *flow, void *vt) {
        const int64_t n = (int64_t)B * g.P;
        DevMem dO, dflow, dvt;
        PB_TRY(up(dO, O, (size_t)n * 32 * 4));
        PB_TRY(preset(dflow, (size_t)(n + guard) * 2 * 4)); PB_TRY(preset(dvt, (size_t)(B * 64 + guard) * ldvP * 2));
        PB_TRY(launch_gm_match_flow(stream, dO.as<float>(), dflow.as<float>(), dvt.as<f16>(), B, g.P, g.w8, ldvP));
        PB_TRY(finish(flow, dflow, (size_t)(n + guard) * 2 * 4));
        return down(vt, dvt, (size_t)(B * 64 + guard) * ldvP * 2);
    }

    int upsampler_in(const float *O, const float *X, int B, int nimg, int P, int img_step, int guard, float *flow, void *map) {
        const int64_t n = (int64_t)B * P;
        DevMem dO, dX, dflow, dmap;
        PB_TRY(up(dO, O, (size_t)n * 32 * 4)); PB_TRY(up(dX, X, (size_t)nimg * P * 128 * 4));
        PB_TRY(preset(dflow, (size_t)(n + guard) * 2 * 4)); PB_TRY(preset(dmap, (size_t)(n + guard) * 384 * 2));
        PB_TRY(launch_gm_upsampler_in(stream, dO.as<float>(), dX.as<float>(), dflow.as<float>(), dmap.as<f16>(), B, P, img_step));
        PB_TRY(finish(flow, dflow, (size_t)(n + guard) * 2 * 4));
        return down(map, dmap, (size_t)(n + guard) * 384 * 2);
    }

    // rows of ldq halfs: [hi (128)] or [hi | lo]
    static void host_rows(f16 *dst, const float *src, int64_t rows, int ldq) {
        for (int64_t r = 0; r < rows; ++r)
            for (int d = 0; d < 128; ++d) {
                const float x = src[r * 128 + d];
                const f16 hi = (f16)x;
                dst[r * ldq + d] = hi;
                if (ldq == 256) dst[r * ldq + 128 + d] = (f16)(x - (float)hi);
            }
    }
    // strided 0: Q and K packed, one buffer each.  1: ONE buffer of B images, Q = K = its base, batch stride one image (the caller gives kxor = 1:
    // the matching in both directions; k is not read).  2: ONE buffer of 2 B images [q_0, k_0, q_1, k_1, ..], batch stride two images, K = Q + one
    // image (the matching in one direction).  Vt is [Bv, 2, vcols, ldv] with the batch stride given explicitly, as the engine does for its window
    // attention and its propagation: hi rows f16(v); lo rows f16(v - hi) where the kernel reads them (split without pv_single), else `fill`;
    // columns [L, ldv) of every row `fill`.
    int attention_cfg(const float *q, const float *k, const float *v, const int8_t *region, int nreg, float *o, int B, int L, int split, int pv_single,
                      int vcols, int v_shared, int kxor, int ldq, int strided, float fill) {
        const int64_t img = (int64_t)L * ldq;
        const int ldv = (int)round_up(L, 32), Bv = v_shared ? 1 : B, spv = split && !pv_single;
        std::vector<f16> hq, hk;
        if (strided == 2) {
            hq.resize((size_t)2 * B * img);
            for (int b = 0; b < B; ++b) {
                host_rows(hq.data() + (size_t)2 * b * img, q + (size_t)b * L * 128, L, ldq);
                host_rows(hq.data() + (size_t)(2 * b + 1) * img, k + (size_t)b * L * 128, L, ldq);
            }
        } else {
            hq.resize((size_t)B * img);
            host_rows(hq.data(), q, (int64_t)B * L, ldq);
            if (!strided) { hk.resize((size_t)B * img); host_rows(hk.data(), k, (int64_t)B * L, ldq); }
        }
        std::vector<f16> hv((size_t)Bv * 2 * vcols * ldv, (f16)fill);
        for (int b = 0; b < Bv; ++b)
            for (int t = 0; t < L; ++t)
                for (int d = 0; d < vcols; ++d) {
                    const float x = v[((size_t)b * L + t) * vcols + d];
                    const f16 hi = (f16)x;
                    hv[(((size_t)b * 2 + 0) * vcols + d) * ldv + t] = hi;
                    if (spv) hv[(((size_t)b * 2 + 1) * vcols + d) * ldv + t] = (f16)(x - (float)hi);
                }
        DevMem dq, dk, dv, dr, dout;
        PB_TRY(dq.alloc(hq.size() * 2 + kSlack));
        PB_HIP(hipMemcpy(dq.p, hq.data(), hq.size() * 2, hipMemcpyHostToDevice));
        if (!strided) {
            PB_TRY(dk.alloc(hk.size() * 2 + kSlack));
            PB_HIP(hipMemcpy(dk.p, hk.data(), hk.size() * 2, hipMemcpyHostToDevice));
        }
        PB_TRY(dv.alloc(hv.size() * 2 + kSlack));
        PB_HIP(hipMemcpy(dv.p, hv.data(), hv.size() * 2, hipMemcpyHostToDevice));
        if (region) PB_TRY(up(dr, region, (size_t)nreg * L));
        PB_TRY(preset(dout, (size_t)B * L * vcols * 4));
        Attn128Args a;
        a.Q = dq.as<f16>(); a.K = strided == 0 ? dk.as<f16>() : (strided == 1 ? dq.as<f16>() : dq.as<f16>() + img);
        a.Vt = dv.as<f16>(); a.region = region ? dr.as<int8_t>() : nullptr; a.nreg = nreg; a.O = dout.as<float>();
        a.B = B; a.L = L; a.ldv = ldv; a.split = split; a.vcols = vcols; a.v_shared = v_shared; a.kxor = kxor; a.pv_single = pv_single; a.ldq = ldq;
        a.v_bstride = (int64_t)2 * vcols * ldv;
        if (strided) a.q_bstride = a.k_bstride = strided == 1 ? img : 2 * img;
        PB_TRY(launch_attention128x(stream, a));
        return finish(o, dout, (size_t)B * L * vcols * 4);
    }

    // pack (q, k, v), the window attention as blocks() configures it - pv_single 1: the one-scale model's (P and V single fp16), 0: the
    // two-scale model's on both of its scales (P and V split) -, gm_ln (windowed, mode 0) straight on the attention output
    int window_block(const float *Y, float *X, const float *gamma, const float *beta, int images, int shifted, int cross, int split, int pv_single = 1) {
        const int64_t R = (int64_t)images * g.P;
        const int nw = g.ns * g.ns, Bw = images * nw;
        DevMem dY, dX, dg, db, dQ, dK, dVt, dO, dXs, dreg;
        PB_TRY(up(dY, Y, (size_t)R * 384 * 4)); PB_TRY(up(dX, X, (size_t)R * 128 * 4)); PB_TRY(up(dg, gamma, 128 * 4)); PB_TRY(up(db, beta, 128 * 4));
        PB_TRY(dQ.alloc((size_t)R * 256 * 2 + kSlack)); PB_TRY(dK.alloc((size_t)R * 256 * 2 + kSlack)); PB_TRY(dXs.alloc((size_t)R * 256 * 2 + kSlack));
        PB_TRY(dVt.alloc((size_t)Bw * 2 * 128 * g.ldv * 2 + kSlack)); PB_TRY(dO.alloc((size_t)R * 128 * 4));
        GmPackJobs jobs{};
        jobs.n = 3;
        jobs.j[0] = GmPackJob{dY.as<float>(), 384, 0, dQ.as<f16>(), 0};
        jobs.j[1] = GmPackJob{dY.as<float>(), 384, 128, dK.as<f16>(), 0};
        jobs.j[2] = GmPackJob{dY.as<float>(), 384, 256, dVt.as<f16>(), 1};
        PB_TRY(launch_gm_pack(stream, jobs, g, Bw, shifted));
        if (shifted) {
            std::vector<int8_t> reg;
            shift_regions(g.h8, g.w8, reg, g.ns);
            PB_TRY(up(dreg, reg.data(), reg.size()));
        }
        Attn128Args a;
        a.Q = dQ.as<f16>(); a.K = dK.as<f16>(); a.Vt = dVt.as<f16>(); a.region = shifted ? dreg.as<int8_t>() : nullptr; a.nreg = nw; a.O = dO.as<float>();
        a.B = Bw; a.L = g.Lw; a.ldv = g.ldv; a.split = split; a.vcols = 128; a.ldq = 256; a.v_bstride = (int64_t)2 * 128 * g.ldv;
        a.pv_single = pv_single;
        if (cross) a.kxor = nw;
        PB_TRY(launch_attention128x(stream, a));
        PB_TRY(launch_gm_ln(stream, dO.as<float>(), dg.as<float>(), db.as<float>(), dX.as<float>(), dXs.as<f16>(), R, g, 1, shifted, 0));
        return finish(X, dX, (size_t)R * 128 * 4);
    }

    // split_rows, the global matching with the shared coordinate V^T, match_flow.  DevMem::alloc zeroes Vtf as commit_arena zeroes the arena.
    int match(const float *tok, int NP, int dirs, int split, float *flow) {
        const int P = g.P, B = NP * dirs;
        const int64_t R = (int64_t)NP * 2 * P, img = (int64_t)P * 256;
        DevMem dT, dXs, dgrid, dOm, dflow, dVtf;
        PB_TRY(up(dT, tok, (size_t)R * 128 * 4));
        PB_TRY(dXs.alloc((size_t)R * 256 * 2 + kSlack)); PB_TRY(dgrid.alloc((size_t)64 * ldvP * 2 + kSlack));
        PB_TRY(dOm.alloc((size_t)B * P * 32 * 4)); PB_TRY(preset(dflow, (size_t)B * P * 2 * 4)); PB_TRY(dVtf.alloc((size_t)B * 64 * ldvP * 2 + kSlack));
        PB_TRY(launch_gm_split_rows(stream, dT.as<float>(), 128, 128, dXs.as<f16>(), R));
        PB_TRY(launch_gm_grid_vt(stream, dgrid.as<f16>(), P, g.w8, ldvP));
        Attn128Args m;
        m.Q = dXs.as<f16>(); m.O = dOm.as<float>(); m.B = B; m.L = P; m.ldv = ldvP; m.split = split; m.vcols = 32; m.ldq = 256;
        m.Vt = dgrid.as<f16>(); m.v_shared = 1;
        if (dirs == 2) { m.K = dXs.as<f16>(); m.q_bstride = m.k_bstride = img; m.kxor = 1; }
        else { m.K = dXs.as<f16>() + img; m.q_bstride = m.k_bstride = 2 * img; }
        PB_TRY(launch_attention128x(stream, m));
        PB_TRY(launch_gm_match_flow(stream, dOm.as<float>(), dflow.as<float>(), dVtf.as<f16>(), B, P, g.w8, ldvP));
        return finish(flow, dflow, (size_t)B * P * 2 * 4);
    }

    // match_flow on O = flow_in + own coordinate (fp32: flowm returns the flow the kernel made of it, the V of what follows), the propagation
    // attention over the zeroed Vtf, upsampler_in
    int propagate(const float *q, const float *k, const float *flow_in, const float *X, int NP, int dirs, int split, int guard, float *flowm, float *flowp,
                  void *map) {
        const int P = g.P, B = NP * dirs;
        const int64_t R = (int64_t)NP * 2 * P, img = (int64_t)P * 256, n = (int64_t)B * P;
        std::vector<float> hO((size_t)n * 32, 0.f);
        for (int64_t i = 0; i < n; ++i) {
            const int t = (int)(i % P);
            hO[i * 32] = flow_in[i * 2] + (float)(t % g.w8);
            hO[i * 32 + 1] = flow_in[i * 2 + 1] + (float)(t / g.w8);
        }
        DevMem dOm, dq, dk, dX, dqs, dks, dVtf, dfm, dfp, dmap;
        PB_TRY(up(dOm, hO.data(), hO.size() * 4)); PB_TRY(up(dq, q, (size_t)R * 128 * 4)); PB_TRY(up(dk, k, (size_t)R * 128 * 4));
        PB_TRY(up(dX, X, (size_t)R * 128 * 4));
        PB_TRY(dqs.alloc((size_t)R * 256 * 2 + kSlack)); PB_TRY(dks.alloc((size_t)R * 256 * 2 + kSlack)); PB_TRY(dVtf.alloc((size_t)B * 64 * ldvP * 2 + kSlack));
        PB_TRY(preset(dfm, (size_t)n * 2 * 4)); PB_TRY(preset(dfp, (size_t)n * 2 * 4)); PB_TRY(preset(dmap, (size_t)(n + guard) * 384 * 2));
        PB_TRY(launch_gm_match_flow(stream, dOm.as<float>(), dfm.as<float>(), dVtf.as<f16>(), B, P, g.w8, ldvP));
        PB_TRY(launch_gm_split_rows(stream, dq.as<float>(), 128, 128, dqs.as<f16>(), R));
        PB_TRY(launch_gm_split_rows(stream, dk.as<float>(), 128, 128, dks.as<f16>(), R));
        Attn128Args pa;
        pa.Q = dqs.as<f16>(); pa.K = dks.as<f16>(); pa.O = dOm.as<float>(); pa.B = B; pa.L = P; pa.ldv = ldvP; pa.split = split; pa.vcols = 32; pa.ldq = 256;
        pa.Vt = dVtf.as<f16>(); pa.v_bstride = (int64_t)64 * ldvP;
        pa.q_bstride = pa.k_bstride = dirs == 2 ? img : 2 * img;
        PB_TRY(launch_attention128x(stream, pa));
        PB_TRY(launch_gm_upsampler_in(stream, dOm.as<float>(), dX.as<float>(), dfp.as<float>(), dmap.as<f16>(), B, P, dirs == 2 ? 1 : 2));
        PB_TRY(finish(flowm, dfm, (size_t)n * 2 * 4));
        PB_TRY(down(flowp, dfp, (size_t)n * 2 * 4));
        return down(map, dmap, (size_t)(n + guard) * 384 * 2);
    }

    // the local matching alone, as infer launches it before a local propagation (no flow V^T)
    int local_match(const float *tok, int NP, int dirs, int radius, int guard, float *flow) {
        const int B = NP * dirs;
        const int64_t n = (int64_t)B * g.P;
        DevMem dT, dflow;
        PB_TRY(up(dT, tok, (size_t)NP * 2 * g.P * 128 * 4));
        PB_TRY(preset(dflow, (size_t)(n + guard) * 2 * 4));
        PB_TRY(launch_gm_local_match(stream, dT.as<float>(), dflow.as<float>(), nullptr, B, g.h8, g.w8, dirs == 2 ? 1 : 2, radius, ldvP));
        return finish(flow, dflow, (size_t)(n + guard) * 2 * 4);
    }

    int local_propagate(const float *q, const float *k, const float *flow_in, int B, int img_step, int radius, int guard, float *out) {
        const int64_t n = (int64_t)B * g.P;
        DevMem dq, dk, dfi, dO;
        PB_TRY(up(dq, q, (size_t)n * img_step * 128 * 4)); PB_TRY(up(dk, k, (size_t)n * img_step * 128 * 4)); PB_TRY(up(dfi, flow_in, (size_t)n * 2 * 4));
        PB_TRY(preset(dO, (size_t)(n + guard) * 32 * 4));
        PB_TRY(launch_gm_local_prop(stream, dq.as<float>(), dk.as<float>(), dfi.as<float>(), dO.as<float>(), B, g.h8, g.w8, img_step, radius));
        return finish(out, dO, (size_t)(n + guard) * 32 * 4);
    }
};

// ---- the mask_mmdet band's own kernels one by one (pb_op_mask_*) -----------------------------------------------------------------------
// Every entry point calls the launcher of mask_kernels.h with the arguments MaskEngine gives it: row strides L(C) = C (1 + split), residual
// offsets lo(C) = split ? C : 0, ld = 512 for the NMS matrices.  Input maps are rows of `ld` halfs, [hi (C) | lo (C)] when split, every half
// the map does not define 0xFFFF (a NaN: a kernel that reads a row tail shows it); outputs are preset to 0xFF bytes and carry guard rows.
class MaskOpEngine : public RaftOpEngine {
  public:
    explicit MaskOpEngine(int device) : RaftOpEngine(device) {}
    // x [rows, C] fp32 -> rows of ld halfs: hi at 0, the residual at lo_off (0 = none); `extra` more rows of 0xFF behind them
    int to_map(DevMem &d, const float *x, int64_t rows, int C, int ld, int lo_off, int64_t extra = 0) {
        std::vector<f16> h((size_t)(rows + extra) * ld);
        memset(h.data(), 0xFF, h.size() * 2);
        for (int64_t r = 0; r < rows; ++r)
            for (int c = 0; c < C; ++c) {
                const float v = x[r * C + c];
                const f16 hi = (f16)v;
                h[(size_t)r * ld + c] = hi;
                if (lo_off) h[(size_t)r * ld + lo_off + c] = (f16)(v - (float)hi);
            }
        return up(d, h.data(), h.size() * 2);
    }
    int down(void *dst, const DevMem &d, size_t bytes) {
        PB_HIP(hipMemcpy(dst, d.p, bytes, hipMemcpyDeviceToHost));
        return 0;
    }

    int prep(const uint8_t *frames, int n, int H, int W, int nh, int nw, int Hp, int Wp, const int *xt, const int *yt, int split, int guard, void *out,
             float *chw) {
        const int64_t blocks = (int64_t)n * (Hp / 4) * (Wp / 4), px = (int64_t)n * 3 * Hp * Wp;
        const int ld = split ? 128 : 64;
        DevMem df, dx, dy, dout, dchw;
        PB_TRY(up(df, frames, (size_t)n * H * W * 3)); PB_TRY(up(dx, xt, (size_t)nw * 16)); PB_TRY(up(dy, yt, (size_t)nh * 16));
        PB_TRY(preset(dout, (size_t)(blocks + guard) * ld * 2)); PB_TRY(preset(dchw, (size_t)(px + guard) * 4));
        PB_TRY(launch_mask_prep(stream, df.as<uint8_t>(), n, H, W, nh, nw, Hp, Wp, dx.as<int>(), dy.as<int>(), dout.as<f16>(), dchw.as<float>(), split));
        PB_TRY(finish(out, dout, (size_t)(blocks + guard) * ld * 2));
        return down(chw, dchw, (size_t)(px + guard) * 4);
    }
    int maxpool(const float *x, int n, int H, int W, int C, int split, int guard, void *out) {
        const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, ld = C * (1 + split);
        const int64_t orows = (int64_t)n * OH * OW;
        DevMem dx, dout;
        PB_TRY(to_map(dx, x, (int64_t)n * H * W, C, ld, split ? C : 0));
        PB_TRY(preset(dout, (size_t)(orows + guard) * ld * 2));
        PB_TRY(launch_maxpool3x3s2(stream, dx.as<f16>(), dout.as<f16>(), n, H, W, C, split));
        return finish(out, dout, (size_t)(orows + guard) * ld * 2);
    }
    int nearest_add(const float *dst, const float *src, int n, int h, int w, int sh, int sw, int C, int split, int guard, void *out) {
        const int ld = C * (1 + split);
        const int64_t rows = (int64_t)n * h * w;
        DevMem dd, ds;
        PB_TRY(to_map(dd, dst, rows, C, ld, split ? C : 0, guard)); PB_TRY(to_map(ds, src, (int64_t)n * sh * sw, C, ld, split ? C : 0));
        PB_TRY(launch_nearest_add(stream, dd.as<f16>(), ds.as<f16>(), n, h, w, sh, sw, C, split));
        return finish(out, dd, (size_t)(rows + guard) * ld * 2);
    }
    int subsample2(const float *x, int n, int H, int W, int C, int split, int guard, void *out) {
        const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, ld = C * (1 + split);
        const int64_t orows = (int64_t)n * OH * OW;
        DevMem dx, dout;
        PB_TRY(to_map(dx, x, (int64_t)n * H * W, C, ld, split ? C : 0));
        PB_TRY(preset(dout, (size_t)(orows + guard) * ld * 2));
        PB_TRY(launch_subsample2(stream, dx.as<f16>(), dout.as<f16>(), n, H, W, ld));         // whole rows: both parts of a split map
        return finish(out, dout, (size_t)(orows + guard) * ld * 2);
    }
    int coord_concat(const float *x, int n, int h, int w, int C, int ldi, int split, int guard, void *out) {
        const int64_t rows = (int64_t)n * h * w;
        const int ldo = (C + 64) * (1 + split);
        DevMem dx, dout;
        PB_TRY(to_map(dx, x, rows, C, ldi, split ? C : 0));
        PB_TRY(preset(dout, (size_t)(rows + guard) * ldo * 2));
        PB_TRY(launch_coord_concat(stream, dx.as<f16>(), dout.as<f16>(), n, h, w, C, ldi, split ? C : 0));
        return finish(out, dout, (size_t)(rows + guard) * ldo * 2);
    }
    int bilinear(const float *x, const float *y0, int n, int H, int W, int OH, int OW, int C, int ldi, int ldo, int split, int guard, void *out) {
        const int64_t orows = (int64_t)n * OH * OW;
        const int lo = split ? C : 0;
        DevMem dx, dout;
        PB_TRY(to_map(dx, x, (int64_t)n * H * W, C, ldi, lo));
        if (y0) PB_TRY(to_map(dout, y0, orows, C, ldo, lo, guard));
        else PB_TRY(preset(dout, (size_t)(orows + guard) * ldo * 2));
        PB_TRY(launch_bilinear(stream, dx.as<f16>(), dout.as<f16>(), n, H, W, OH, OW, C, ldi, ldo, y0 ? 1 : 0, lo, lo));
        return finish(out, dout, (size_t)(orows + guard) * ldo * 2);
    }
    // layout 0: fp16 -> fp16, 1: split -> split, 2: split -> [hi | hi | lo] (the B operand of the dynamic convolution)
    int gn_relu(const float *x, const float *gamma, const float *beta, int n, int HW, int C, int layout, int guard, void *out, float *aff) {
        const int sa = layout ? 1 : 0, ldc = C * (1 + sa), ldo = layout == 2 ? 3 * C : ldc;
        const int64_t rows = (int64_t)n * HW;
        DevMem dx, dg, db, dout, dst, daff;
        PB_TRY(to_map(dx, x, rows, C, ldc, sa ? C : 0));
        PB_TRY(up(dg, gamma, (size_t)C * 4)); PB_TRY(up(db, beta, (size_t)C * 4));
        PB_TRY(preset(dout, (size_t)(rows + guard) * ldo * 2));
        PB_TRY(preset(dst, (size_t)n * gn_chunks(HW) * C * 2 * 4)); PB_TRY(preset(daff, (size_t)n * C * 2 * 4));
        PB_TRY(launch_gn_relu(stream, dx.as<f16>(), dout.as<f16>(), n, HW, C, ldc, ldo, 32, dg.as<float>(), db.as<float>(), dst.as<float>(), daff.as<float>(),
                              sa ? C : 0, layout == 2 ? 2 * C : (sa ? C : 0), layout == 2 ? C : 0));
        PB_TRY(finish(out, dout, (size_t)(rows + guard) * ldo * 2));
        return down(aff, daff, (size_t)n * C * 2 * 4);
    }
    int cls_points_nms(const float *logit, int n, int pts_total, int off, int g, int C, int guard, float *score) {
        DevMem dl, ds;
        PB_TRY(up(dl, logit, (size_t)n * g * g * C * 4));
        PB_TRY(preset(ds, ((size_t)n * pts_total + guard) * C * 4));
        PB_TRY(launch_cls_points_nms(stream, dl.as<float>(), ds.as<float>(), n, pts_total, off, g, C));
        return finish(score, ds, ((size_t)n * pts_total + guard) * C * 4);
    }
    int gather_rows(const float *src, int src_rows, const int *idx, int count, int rows_pad, int cols, int split, int guard, void *out) {
        const int ld = cols * (1 + split);
        DevMem ds, di, dout;
        PB_TRY(up(ds, src, (size_t)src_rows * cols * 4)); PB_TRY(up(di, idx, (size_t)std::max(count, 1) * 4));
        PB_TRY(preset(dout, (size_t)(rows_pad + guard) * ld * 2));
        PB_TRY(launch_gather_rows_f16(stream, ds.as<float>(), di.as<int>(), dout.as<f16>(), count, rows_pad, cols, split));
        return finish(out, dout, (size_t)(rows_pad + guard) * ld * 2);
    }
    int mask_stats(const float *logit, int rows, int HW, int ld, float thr, int guard, float *out) {
        DevMem dl, dout;
        PB_TRY(up(dl, logit, (size_t)rows * ld * 4));
        PB_TRY(preset(dout, (size_t)(rows + guard) * 2 * 4));
        PB_TRY(launch_mask_stats(stream, dl.as<float>(), rows, HW, ld, thr, dout.as<float>()));
        return finish(out, dout, (size_t)(rows + guard) * 2 * 4);
    }
    // bitpack_rows then mask_intersections on its output; inter is [irows, 512] floats, returned whole
    int intersections(const float *logit, int src_rows, int ld, const int *idx, int n, int HW, float thr, int guard, void *bits, int irows, float *inter) {
        const int words = HW / 64;
        DevMem dl, di, dbits, dint;
        PB_TRY(up(dl, logit, (size_t)src_rows * ld * 4)); PB_TRY(up(di, idx, (size_t)n * 4));
        PB_TRY(preset(dbits, (size_t)(n + guard) * words * 8)); PB_TRY(preset(dint, (size_t)irows * 512 * 4));
        PB_TRY(launch_bitpack_rows(stream, dl.as<float>(), ld, di.as<int>(), n, HW, thr, dbits.as<unsigned long long>()));
        PB_TRY(launch_mask_intersections(stream, dbits.as<unsigned long long>(), n, words, dint.as<float>(), 512));
        PB_TRY(finish(bits, dbits, (size_t)(n + guard) * words * 8));
        return down(inter, dint, (size_t)irows * 512 * 4);
    }
    int matrix_nms(const float *inter, const float *area, const int *label, const float *score, int n, float sigma, int guard, float *comp, float *out) {
        DevMem di, da, dl, ds, dc, dout;
        PB_TRY(up(di, inter, (size_t)n * 512 * 4)); PB_TRY(up(da, area, (size_t)n * 4)); PB_TRY(up(dl, label, (size_t)n * 4)); PB_TRY(up(ds, score, (size_t)n * 4));
        PB_TRY(preset(dc, (size_t)(n + guard) * 4)); PB_TRY(preset(dout, (size_t)(n + guard) * 4));
        PB_TRY(launch_matrix_nms(stream, di.as<float>(), 512, da.as<float>(), dl.as<int>(), ds.as<float>(), n, sigma, dc.as<float>(), dout.as<float>()));
        PB_TRY(finish(comp, dc, (size_t)(n + guard) * 4));
        return down(out, dout, (size_t)(n + guard) * 4);
    }
    int sigmoid_rows(const float *logit, int src_rows, int ld, const int *idx, int count, int HW, int guard, float *sig) {
        DevMem dl, di, ds;
        PB_TRY(up(dl, logit, (size_t)src_rows * ld * 4)); PB_TRY(up(di, idx, (size_t)count * 4));
        PB_TRY(preset(ds, (size_t)(count + guard) * HW * 4));
        PB_TRY(launch_sigmoid_rows(stream, dl.as<float>(), ld, di.as<int>(), count, HW, ds.as<float>()));
        return finish(sig, ds, (size_t)(count + guard) * HW * 4);
    }
    // post_chunk's dynamic convolution: gather_rows_f16 builds A (row_off + M kernels, the launch reads rows [row_off, row_off + M)), B is the
    // mask-feature map in the layout gn_relu's dup output has ([hi | hi | lo] when split), EPI_F32 into [M, HW4]
    int dynconv(const float *kern, int src_rows, const int *idx, int row_off, int M, const float *feat, int HW4, int split, int guard, float *out) {
        const int total = row_off + M, lda = 256 * (1 + split), ldb = split ? 768 : 256;
        const int64_t arows = round_up(total, 256) + 256, brows = round_up(HW4, 256);
        std::vector<f16> hb((size_t)brows * ldb, (f16)0.f);
        for (int64_t p = 0; p < HW4; ++p)
            for (int c = 0; c < 256; ++c) {
                const float v = feat[p * 256 + c];
                const f16 hi = (f16)v;
                hb[(size_t)p * ldb + c] = hi;
                if (split) { hb[(size_t)p * ldb + 256 + c] = hi; hb[(size_t)p * ldb + 512 + c] = (f16)(v - (float)hi); }
            }
        DevMem dk, di, da, dB, dout;
        PB_TRY(up(dk, kern, (size_t)src_rows * 256 * 4)); PB_TRY(up(di, idx, (size_t)total * 4)); PB_TRY(up(dB, hb.data(), hb.size() * 2));
        PB_TRY(da.alloc((size_t)arows * lda * 2));
        PB_TRY(preset(dout, (size_t)(M + guard) * HW4 * 4));
        PB_TRY(launch_gather_rows_f16(stream, dk.as<float>(), di.as<int>(), da.as<f16>(), total, total, 256, split));
        GemmArgs a;
        a.A = da.as<f16>() + (int64_t)row_off * lda; a.lda = lda; a.M = M; a.W = dB.as<f16>(); a.K = ldb; a.N = HW4;
        if (split) a.kwrap = 8;
        a.out32 = dout.as<float>(); a.ldo = HW4; a.scale = 1.f; a.zero = zero_;
        PB_TRY(launch_gemm(stream, A_DENSE, EPI_F32, TILE_AUTO, a));
        return finish(out, dout, (size_t)(M + guard) * HW4 * 4);
    }
    int band_accumulate(const float *sig, const uint8_t *use, int k, int fh, int fw, int h, int w, int H, int W, float thr, int guard, uint8_t *out,
                        uint8_t *inst) {
        const int64_t px = (int64_t)H * W;
        DevMem ds, du, dout, dinst;
        PB_TRY(up(ds, sig, (size_t)k * fh * fw * 4)); PB_TRY(up(du, use, (size_t)k));
        PB_TRY(preset(dout, (size_t)px * 3 + guard));
        if (inst) PB_TRY(preset(dinst, (size_t)k * px + guard));
        PB_TRY(launch_band_accumulate(stream, ds.as<float>(), k, fh, fw, h, w, H, W, thr, du.as<uint8_t>(), dout.as<uint8_t>(),
                                      inst ? dinst.as<uint8_t>() : nullptr));
        PB_TRY(finish(out, dout, (size_t)px * 3 + guard));
        return inst ? down(inst, dinst, (size_t)k * px + guard) : 0;
    }
};

// the "l.weight" [n, k] or [n, k, kh, kw] / "l.bias" [n] pair of one layer, as begin_load() takes it
struct LayerTensors {
    pb_tensor t[2] = {};
    LayerTensors(const float *w, const float *bias, int n, int k, int kh = 0, int kw = 0) {
        t[0].name = "l.weight"; t[0].dtype = PB_F32; t[0].ndim = kh ? 4 : 2; t[0].data = (void *)w;
        t[0].shape[0] = n; t[0].shape[1] = k; t[0].shape[2] = kh; t[0].shape[3] = kw;
        t[1].name = "l.bias"; t[1].dtype = PB_F32; t[1].ndim = 1; t[1].shape[0] = n; t[1].data = (void *)bias;
    }
};

// pb_set_option("op_splitk", 1): lends one launch_gemm a split-K workspace that lives as long as `ws`
int lend_splitk(const pb_ctx *c, DevMem &ws, GemmArgs &g) {
    if (!c->op_splitk) return 0;
    PB_TRY(ws.alloc((size_t)512 * 128 * 128 * 4));
    g.sk_ws = ws.as<float>(); g.sk_cap = (int64_t)512 * 128 * 128;
    return 0;
}

// mean milliseconds of `iters` launches on stream s (the callers warm up first)
template <class Launch>
int time_launches(hipStream_t s, int iters, double *ms_out, Launch launch) {
    hipEvent_t e0, e1;
    PB_HIP(hipEventCreate(&e0)); PB_HIP(hipEventCreate(&e1));
    PB_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) PB_TRY(launch());
    PB_HIP(hipEventRecord(e1, s));
    PB_HIP(hipStreamSynchronize(s));
    float ms = 0;
    PB_HIP(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    *ms_out = ms / iters;
    return 0;
}

// ---- the depth bands' own kernels one by one (pb_op_depth_*, pb_op_zoe_*) ---------------------------------------------------------------
// Every entry point calls the launcher DepthEngine calls (kernels.h, zoe_kernels.h) with arguments the test chooses, in the modes the engine
// uses: token rows wider than the payload with an fp8 copy behind it, the compacted class-token-free tap maps, the three pixel layouts of
// the DPT tail.  Inputs are staged as above (build_map / to_map: 0xFFFF wherever a map defines nothing), outputs are preset to 0xFF bytes
// and carry guard rows.
class DepthOpEngine : public MaskOpEngine {
  public:
    explicit DepthOpEngine(int device) : MaskOpEngine(device) {}
    int lo8_pa() const { return kLo8Pa; }

    int layernorm(const float *x, const float *g, const float *b, int B, int ntp, int ntok, int D, int drop_cls, int ldy, int lo_off, int o8_off,
                  float o8_scale, int lo8, int guard, void *out) {
        const int64_t rows = drop_cls ? (int64_t)B * (ntok - 1) : (int64_t)B * ntp;
        DevMem dx, dg, db, dout;
        PB_TRY(up(dx, x, (size_t)B * ntp * D * 4)); PB_TRY(up(dg, g, (size_t)D * 4)); PB_TRY(up(db, b, (size_t)D * 4));
        PB_TRY(preset(dout, (size_t)(rows + guard) * ldy * 2));
        PB_TRY(launch_layernorm(stream, dx.as<float>(), dg.as<float>(), db.as<float>(), dout.as<f16>(), B, ntp, ntok, D, 1e-6f, drop_cls, ldy, lo_off, o8_off,
                                o8_scale, lo8 ? kLo8Pa : -1));
        return finish(out, dout, (size_t)(rows + guard) * ldy * 2);
    }

    // q, k, v [B, heads, N, 64] -> the engine's Q (pre-scaled by PB_QSCALE as the qkv epilogue does) / K [B heads, ntp, 64] and Vt [B heads, 64, ntp],
    // pad tokens zero; the output rows [B ntp, ldo] raw
    int attention(const float *q, const float *k, const float *v, int B, int heads, int N, int variant, int ldo, int o8_off, float o8_scale, int guard,
                  void *out) {
        const int ntp = (int)round_up(N, 16);
        const size_t bh = (size_t)B * heads;
        std::vector<f16> hq(bh * ntp * 64, (f16)0.f), hk(bh * ntp * 64, (f16)0.f), hv(bh * 64 * ntp, (f16)0.f);
        for (size_t i = 0; i < bh; ++i)
            for (int t = 0; t < N; ++t)
                for (int d = 0; d < 64; ++d) {
                    const size_t s = (i * N + t) * 64 + d;
                    hq[(i * ntp + t) * 64 + d] = (f16)(q[s] * PB_QSCALE);
                    hk[(i * ntp + t) * 64 + d] = (f16)k[s];
                    hv[(i * 64 + d) * ntp + t] = (f16)v[s];
                }
        DevMem dq, dk, dv, dout;
        const size_t slack = 32768;
        PB_TRY(dq.alloc(hq.size() * 2 + slack)); PB_TRY(dk.alloc(hk.size() * 2 + slack)); PB_TRY(dv.alloc(hv.size() * 2 + slack));
        PB_HIP(hipMemcpy(dq.p, hq.data(), hq.size() * 2, hipMemcpyHostToDevice));
        PB_HIP(hipMemcpy(dk.p, hk.data(), hk.size() * 2, hipMemcpyHostToDevice));
        PB_HIP(hipMemcpy(dv.p, hv.data(), hv.size() * 2, hipMemcpyHostToDevice));
        const size_t bytes = ((size_t)B * ntp + guard) * ldo * 2;
        PB_TRY(preset(dout, bytes));
        PB_TRY(launch_attention(stream, dq.as<f16>(), dk.as<f16>(), dv.as<f16>(), dout.as<f16>(), B, heads, ntp, N, ldo, variant, o8_off, o8_scale));
        return finish(out, dout, bytes);
    }

    // launch_preprocess as DepthEngine::run_chunk issues it - one launch for all n frames, the tap tables of DepthEngine::prepare (mode 0:
    // pb_cubic_taps, mode 1: pb_bilinear_ac_taps) - with BOTH outputs: chw [n, 3, nh, nw] and the im2col rows of patchA_, 640 halfs wide,
    // round_up(n P, 256) + guard of them, raw
    int preprocess(const uint8_t *frames, int n, int H, int W, int mode, int nh, int nw, int guard, float *chw, void *patch) {
        std::vector<int> xi((size_t)nw * 4), yi((size_t)nh * 4);
        std::vector<float> xw((size_t)nw * 4), yw((size_t)nh * 4);
        if (mode) { pb_bilinear_ac_taps(W, nw, xi.data(), xw.data()); pb_bilinear_ac_taps(H, nh, yi.data(), yw.data()); }
        else { pb_cubic_taps(W, nw, xi.data(), xw.data()); pb_cubic_taps(H, nh, yi.data(), yw.data()); }
        for (int v : xi) PB_CHECK(v >= 0 && v < W, PB_ERR_STATE, "op_depth_preprocess: x tap %d outside a row of %d pixels", v, W);
        for (int v : yi) PB_CHECK(v >= 0 && v < H, PB_ERR_STATE, "op_depth_preprocess: y tap %d outside %d rows", v, H);
        const int Kp = 640;
        const int64_t P = (int64_t)(nh / 14) * (nw / 14), rows = round_up((int64_t)n * P, 256) + guard;
        const size_t cb = (size_t)n * 3 * nh * nw * 4, pbytes = (size_t)rows * Kp * 2;
        DevMem df, dxi, dxw, dyi, dyw, dchw, dpatch;
        PB_TRY(up(df, frames, (size_t)n * H * W * 3));
        PB_TRY(up(dxi, xi.data(), xi.size() * 4)); PB_TRY(up(dxw, xw.data(), xw.size() * 4));
        PB_TRY(up(dyi, yi.data(), yi.size() * 4)); PB_TRY(up(dyw, yw.data(), yw.size() * 4));
        PB_TRY(preset(dchw, cb)); PB_TRY(preset(dpatch, pbytes));
        PB_TRY(launch_preprocess(stream, df.as<uint8_t>(), n, H, W, nh, nw, dxi.as<int>(), dxw.as<float>(), dyi.as<int>(), dyw.as<float>(), dpatch.as<f16>(), Kp,
                                 dchw.as<float>()));
        PB_TRY(finish(chw, dchw, cb));
        return down(patch, dpatch, pbytes);
    }

    int cls_rows(const float *cls, const float *pos, int B, int ntp, int D, int guard, float *out) {
        DevMem dc, dp, dr;
        PB_TRY(up(dc, cls, (size_t)D * 4)); PB_TRY(up(dp, pos, (size_t)D * 4));
        PB_TRY(preset(dr, ((size_t)B * ntp + guard) * D * 4));
        PB_TRY(launch_cls_rows(stream, dr.as<float>(), dc.as<float>(), dp.as<float>(), B, ntp, D));
        return finish(out, dr, ((size_t)B * ntp + guard) * D * 4);
    }

    // layout 0: [hi], 1: [hi | lo], 2: [hi | hi8 | lo8]; 288 channels in the engine's 320-wide parts, pixels ldz halfs apart
    int dpt_tail(const float *z, const float *bias, const float *w2, float b2, int B, int H, int W, int OH, int OW, int layout, int ldz, int guard,
                 float *out) {
        const int Zp = 320, lo_off = layout ? Zp : 0;
        const int64_t P = (int64_t)B * H * W, px = (int64_t)B * OH * OW;
        std::vector<float> zp((size_t)P * Zp, 0.f);
        for (int64_t p = 0; p < P; ++p) memcpy(&zp[(size_t)p * Zp], z + p * 288, 288 * 4);
        std::vector<f16> hz((size_t)P * ldz);
        memset(hz.data(), 0xFF, hz.size() * 2);
        build_map(zp.data(), P, Zp, Zp, layout == 0 ? SL_F16 : (layout == 1 ? SL_SPLIT16 : SL_MX3), 1, ldz, hz);
        DevMem dz, dbias, dw2, dout;
        PB_TRY(up(dz, hz.data(), hz.size() * 2)); PB_TRY(up(dbias, bias, 32 * 4)); PB_TRY(up(dw2, w2, 32 * 4));
        PB_TRY(preset(dout, (size_t)(px + guard) * 4));
        PB_TRY(launch_dpt_tail(stream, dz.as<f16>(), B, H, W, ldz, lo_off, layout == 2 ? kLo8Pa : -1, dbias.as<float>(), dw2.as<float>(), b2, dout.as<float>(),
                               OH, OW));
        return finish(out, dout, (size_t)(px + guard) * 4);
    }

    int resize_minmax(const float *net, int B, int nh, int nw, int H, int W, int guard, float *out, float *mnmx) {
        const int64_t px = (int64_t)B * H * W;
        DevMem dn, dout, dmm;
        PB_TRY(up(dn, net, (size_t)B * nh * nw * 4));
        PB_TRY(preset(dout, (size_t)(px + guard) * 4));
        PB_TRY(dmm.alloc((size_t)B * 2 * 4));
        PB_TRY(launch_init_minmax(stream, dmm.as<unsigned>(), B));
        PB_TRY(launch_depth_resize_minmax(stream, dn.as<float>(), B, nh, nw, dout.as<float>(), H, W, dmm.as<unsigned>()));
        PB_TRY(finish(out, dout, (size_t)(px + guard) * 4));
        std::vector<unsigned> mm((size_t)B * 2);
        PB_TRY(down(mm.data(), dmm, mm.size() * 4));
        for (size_t i = 0; i < mm.size(); ++i) {            // the ordered-uint encoding of elementwise.hip f2ord, undone
            const unsigned u = (mm[i] & 0x80000000u) ? (mm[i] & 0x7fffffffu) : ~mm[i];
            memcpy(mnmx + i, &u, 4);
        }
        return 0;
    }

    // x arrives as the whole buffer [rows + guard, ld] (the caller presets what the kernel does not own) and is returned whole
    int softplus(float *x, int64_t rows, int cols, int ld, int guard) {
        DevMem dx;
        PB_TRY(up(dx, x, (size_t)(rows + guard) * ld * 4));
        PB_TRY(launch_softplus(stream, dx.as<float>(), rows, cols, ld));
        return finish(x, dx, (size_t)(rows + guard) * ld * 4);
    }
    int dot32_relu(const float *act, int ld, const float *w2, float b2, int64_t rows, int guard, float *out) {
        DevMem da, dw, dout;
        PB_TRY(to_map(da, act, rows, 32, ld, 0)); PB_TRY(up(dw, w2, 32 * 4));
        PB_TRY(preset(dout, (size_t)(rows + guard) * 4));
        PB_TRY(launch_dot32_relu(stream, da.as<f16>(), ld, dw.as<float>(), b2, dout.as<float>(), rows));
        return finish(out, dout, (size_t)(rows + guard) * 4);
    }
    int bilerp_add(const float *a, const float *src, int n, int h, int w, int H, int W, int C, int lda, int lds, int ldo, int guard, void *out) {
        const int64_t rows = (int64_t)n * H * W;
        DevMem da, ds, dout;
        PB_TRY(to_map(da, a, rows, C, lda, 0)); PB_TRY(to_map(ds, src, (int64_t)n * h * w, C, lds, 0));
        PB_TRY(preset(dout, (size_t)(rows + guard) * ldo * 2));
        PB_TRY(launch_bilerp_add(stream, da.as<f16>(), ds.as<f16>(), dout.as<f16>(), n, h, w, H, W, C, lda, lds, ldo));
        return finish(out, dout, (size_t)(rows + guard) * ldo * 2);
    }
    int attractor(const float *A, int ldA, int nA, const float *bprev, int n, int h, int w, int H, int W, float alpha, int guard, float *out) {
        const int64_t rows = (int64_t)n * H * W;
        DevMem dA, db, dout;
        PB_TRY(up(dA, A, (size_t)rows * ldA * 4)); PB_TRY(up(db, bprev, (size_t)n * h * w * 64 * 4));
        PB_TRY(preset(dout, (size_t)(rows + guard) * 64 * 4));
        PB_TRY(launch_attractor(stream, dA.as<float>(), ldA, nA, db.as<float>(), h, w, dout.as<float>(), n, H, W, alpha));
        return finish(out, dout, (size_t)(rows + guard) * 64 * 4);
    }
    int cat(const float *act, int ld_act, const float *rel, const float *emb, int ld_emb, int n, int h, int w, int H, int W, int guard, void *out) {
        const int64_t rows = (int64_t)n * H * W;
        DevMem da, dr, de, dout;
        PB_TRY(to_map(da, act, rows, 32, ld_act, 0)); PB_TRY(up(dr, rel, (size_t)rows * 4)); PB_TRY(to_map(de, emb, (int64_t)n * h * w, 128, ld_emb, 0));
        PB_TRY(preset(dout, (size_t)(rows + guard) * 192 * 2));
        PB_TRY(launch_zoe_cat(stream, da.as<f16>(), ld_act, dr.as<float>(), de.as<f16>(), ld_emb, h, w, dout.as<f16>(), n, H, W));
        return finish(out, dout, (size_t)(rows + guard) * 192 * 2);
    }
    int logbinom(const float *pt, int ld_pt, const float *bins, int n, int h, int w, int H, int W, float min_temp, float max_temp, int guard, float *out) {
        const int64_t rows = (int64_t)n * H * W;
        DevMem dp, db, dout;
        PB_TRY(up(dp, pt, (size_t)rows * ld_pt * 4)); PB_TRY(up(db, bins, (size_t)n * h * w * 64 * 4));
        PB_TRY(preset(dout, (size_t)(rows + guard) * 4));
        PB_TRY(launch_logbinom_depth(stream, dp.as<float>(), ld_pt, db.as<float>(), h, w, dout.as<float>(), n, H, W, min_temp, max_temp));
        return finish(out, dout, (size_t)(rows + guard) * 4);
    }
    // the tables come from pil_coeffs / pil_ksize, the functions DepthEngine::metric_tables builds them with
    int pil_resize(const float *in, int n, int h, int w, int H, int W, int guard, float *out) {
        std::vector<int> xb, yb;
        std::vector<double> xk, yk;
        pil_coeffs(w, W, xb, xk); pil_coeffs(h, H, yb, yk);
        const int64_t px = (int64_t)n * H * W;
        DevMem di, dt, dout, dxb, dyb, dxk, dyk;
        PB_TRY(up(di, in, (size_t)n * h * w * 4));
        PB_TRY(preset(dt, (size_t)n * h * W * 4)); PB_TRY(preset(dout, (size_t)(px + guard) * 4));
        PB_TRY(up(dxb, xb.data(), xb.size() * 4)); PB_TRY(up(dyb, yb.data(), yb.size() * 4));
        PB_TRY(up(dxk, xk.data(), xk.size() * 8)); PB_TRY(up(dyk, yk.data(), yk.size() * 8));
        PB_TRY(launch_pil_resize(stream, di.as<float>(), dt.as<float>(), dout.as<float>(), n, h, w, H, W, dxb.as<int>(), dxk.as<double>(), pil_ksize(w, W),
                                 dyb.as<int>(), dyk.as<double>(), pil_ksize(h, H)));
        return finish(out, dout, (size_t)(px + guard) * 4);
    }
};

// ---- the GEMM's fused epilogues one by one (pb_op_gemm_resid / _qkv / _patch / _pixshuf / _fc1, pb_op_conv_head) -----------------------------------------------------------
// The ViT linears as DepthEngine::vit launches them: weights through pack_spec with the PackSpec DepthEngine::pack_vit fills (one fp16 pass,
// hi + lo fp16 weights, or mx2 [w_hi | w_lo8] against token rows [a16 | a8]), LayerScale folded by pb_fold_layerscale, the GemmArgs of
// engine.hip vit() and launch_gemm with the tile the test asks for.  Outputs are preset to 0xFF bytes and carry guard rows.
class EpiOpEngine : public DepthOpEngine {
  public:
    explicit EpiOpEngine(int device) : DepthOpEngine(device) {}

    static int vit_spec(int layout, PackSpec &s) {
        PB_CHECK(layout == SL_F16 || layout == SL_SPLIT16 || layout == SL_MX2, PB_ERR_ARG, "epilogue op: a ViT linear is f16 (0), split16 (1) or mx2 (3), not %d", layout);
        s = PackSpec();
        s.sw = layout != SL_F16; s.mx2 = layout == SL_MX2;
        return 0;
    }
    // A [M, K] -> token rows [a16 (Kp)] or, for mx2 weights, [a16 (Kp) | a8 (Kp bytes)]; the rows up to the next multiple of 256 are zero
    int vit_rows(DevMem &d, const float *A, int64_t M, int K, int Kp, bool m2, int &lda) const {
        lda = m2 ? Kp + Kp / 2 : Kp;
        std::vector<f16> h((size_t)round_up(M, 256) * lda, (f16)0.f);
        build_map(A, M, K, Kp, m2 ? SL_MX2 : SL_F16, 0, lda, h);
        return up(d, h.data(), h.size() * 2);
    }
    int launch(const pb_ctx *c, int epi, int tile, GemmArgs &a, const PackedW &w, int *info, char *kname, int kcap, int amode = A_DENSE) {
        a.N = w.N;
        set_weights(a, w, amode == A_CONV);
        DevMem dsk;
        PB_TRY(lend_splitk(c, dsk, a));
        PB_HIP(hipDeviceSynchronize());
        pb_gemm_set_last_kernel("");
        PB_TRY(launch_gemm(stream, amode, epi, tile, a));
        PB_HIP(hipStreamSynchronize(stream));
        if (info) {
            const int v[8] = {w.mx_pw, w.mx3 ? kLo8Pa : kMx2Pa, w.mx2, w.sw, w.K, w.nk16, w.mx3, pb_gemm_last_splitk()};
            memcpy(info, v, sizeof(v));
        }
        if (kname && kcap > 0) snprintf(kname, kcap, "%s", pb_gemm_last_kernel());
        return 0;
    }

    int resid(const pb_ctx *c, const float *A, const float *W, const float *bias, const float *gamma, const float *X, int M, int N, int K, int ldr,
              int layout, int tile, int guard, float *out, int *info, char *kname, int kcap) {
        PackSpec s;
        PB_TRY(vit_spec(layout, s));
        std::vector<float> ws, bb;
        pb_fold_layerscale(W, bias, gamma, N, K, ws, bb);
        PackedW w;
        PB_TRY(pack_spec(ws.data(), N, K, K, w, bb.data(), 1, s));
        DevMem da, dg, dx;
        int lda = 0;
        PB_TRY(vit_rows(da, A, M, K, K, w.mx2 != 0, lda));
        PB_TRY(up(dg, gamma, (size_t)N * 4));
        std::vector<float> hx((size_t)(M + guard) * ldr);
        memset(hx.data(), 0xFF, hx.size() * 4);
        for (int64_t m = 0; m < M; ++m) memcpy(&hx[(size_t)m * ldr], X + m * N, (size_t)N * 4);
        PB_TRY(up(dx, hx.data(), hx.size() * 4));
        GemmArgs a;
        a.A = da.as<f16>(); a.lda = lda; a.M = M; a.resid = dx.as<float>(); a.ldr = ldr; a.gamma = dg.as<float>();
        PB_TRY(launch(c, EPI_RESID, tile, a, w, info, kname, kcap));
        return down(out, dx, hx.size() * 4);
    }

    // q, k: (B heads ntp + guard) rows of 64 halfs; vt: (B heads 64 + guard) rows of ntp halfs
    int qkv(const pb_ctx *c, const float *A, const float *W, const float *bias, int B, int ntp, int D, int layout, int tile, int guard, void *q, void *k,
            void *vt, int *info, char *kname, int kcap) {
        PackSpec s;
        PB_TRY(vit_spec(layout, s));
        PackedW w;
        PB_TRY(pack_spec(W, 3 * D, D, D, w, bias, 1, s));
        const int heads = D / 64;
        const int64_t M = (int64_t)B * ntp;
        DevMem da, dq, dk, dv;
        int lda = 0;
        PB_TRY(vit_rows(da, A, M, D, D, w.mx2 != 0, lda));
        const size_t qb = ((size_t)B * heads * ntp + guard) * 64 * 2, vb = ((size_t)B * heads * 64 + guard) * ntp * 2;
        PB_TRY(preset(dq, qb)); PB_TRY(preset(dk, qb)); PB_TRY(preset(dv, vb));
        GemmArgs a;
        a.A = da.as<f16>(); a.lda = lda; a.M = (int)M;
        a.q = dq.as<f16>(); a.k = dk.as<f16>(); a.vt = dv.as<f16>(); a.ntp = ntp; a.heads = heads; a.D = D; a.qscale = PB_QSCALE;
        PB_TRY(launch(c, EPI_QKV, tile, a, w, info, kname, kcap));
        PB_TRY(down(q, dq, qb)); PB_TRY(down(k, dk, qb));
        return down(vt, dv, vb);
    }

    // the 14 x 14 x 3 patch embedding: K = 588 carried as 640; rows (b, patch) land on rows b ntp + 1 + patch of the residual stream
    int patch(const pb_ctx *c, const float *A, const float *W, const float *bias, const float *pos, int B, int P, int ntp, int D, int layout, int guard,
              float *out, int *info, char *kname, int kcap) {
        PackSpec s;
        PB_TRY(vit_spec(layout, s));
        PB_CHECK(!s.mx2, PB_ERR_ARG, "op_gemm_patch: the patch embedding is f16 (0) or split16 (1)");
        PackedW w;
        PB_TRY(pack_spec(W, D, 588, 640, w, bias, 1, s));
        DevMem da, dp, dx;
        int lda = 0;
        PB_TRY(vit_rows(da, A, (int64_t)B * P, 588, 640, false, lda));
        PB_TRY(up(dp, pos, (size_t)(1 + P) * D * 4));
        const size_t xb = ((size_t)B * ntp + guard) * D * 4;
        PB_TRY(preset(dx, xb));
        GemmArgs a;
        a.A = da.as<f16>(); a.lda = lda; a.M = B * P;
        a.resid = dx.as<float>(); a.ldr = D; a.pos = dp.as<float>(); a.ppi = P; a.ntp = ntp; a.D = D;
        PB_TRY(launch(c, EPI_PATCH, TILE_128, a, w, info, kname, kcap));
        return down(out, dx, xb);
    }

    // output_conv2 as DepthEngine::head fuses it: 3 x 3 over C channels -> 32, ReLU, dot with w2, + b2, ReLU -> one float per pixel.  The map is
    // [hi], [hi | lo] or [hi | hi8 | lo8] (layout 0 / 1 / 2), the weights slice-major as the head packs them
    int head(const pb_ctx *c, const float *x, const float *W, const float *bias, const float *w2, float b2, int B, int H, int Wd, int C, int layout,
             int guard, float *out, int *info, char *kname, int kcap) {
        PB_CHECK(layout == SL_F16 || layout == SL_SPLIT16 || layout == SL_MX3, PB_ERR_ARG, "op_conv_head: layout %d (0 f16, 1 split16, 2 mx3)", layout);
        PackSpec s;
        s.sa = s.sw = layout != SL_F16; s.mx = layout == SL_MX3; s.tapin = 1;
        const int Cp = (int)round_up(C, 64), K = 9 * Cp;
        PackedW w;
        PB_TRY(pack_spec(pb_conv_rows(W, 32, C, 9, Cp).data(), 32, K, K, w, bias, 9, s));
        w.Kreal = 9 * C;
        const int64_t P = (int64_t)B * H * Wd;
        const int ld = layout == SL_F16 ? Cp : 2 * Cp;
        std::vector<float> xp((size_t)P * Cp, 0.f);
        for (int64_t p = 0; p < P; ++p) memcpy(&xp[(size_t)p * Cp], x + p * C, (size_t)C * 4);
        std::vector<f16> hx((size_t)round_up(P, 256) * ld, (f16)0.f);
        build_map(xp.data(), P, Cp, Cp, layout, 1, ld, hx);
        DevMem dx, dw2, dout;
        PB_TRY(up(dx, hx.data(), hx.size() * 2)); PB_TRY(up(dw2, w2, 32 * 4));
        PB_TRY(preset(dout, (size_t)(P + guard) * 4));
        GemmArgs a;
        a.A = dx.as<f16>();
        a.cH = H; a.cW = Wd; a.cC = Cp; a.cKW = 3; a.cStride = 1; a.cPad = 1; a.cOH = H; a.cOW = Wd;
        a.M = (int)P; a.w2 = dw2.as<float>(); a.b2 = b2; a.depth = dout.as<float>();
        PB_CHECK(a.cC == w.Cseg, PB_ERR_STATE, "op_conv_head: %d channels per part, weights packed for %d", a.cC, w.Cseg);
        PB_TRY(launch(c, EPI_HEAD, TILE_AUTO, a, w, info, kname, kcap, A_CONV));
        return down(out, dout, (size_t)(P + guard) * 4);
    }

    // the convolution form of the pixel shuffle (RAFT's encoder stem, raft_engine.hip encoder): a 3 x 3 convolution over 64 channels to 4 x 64 columns
    // (dy, dx, co), s = 2, weights through EngineBase::pack with nine taps and sa = 1 as the stem's; bias [64]; maps and output as pixshuf's
    int pixshuf_conv(const pb_ctx *c, const float *x, const float *W, const float *bias, int B, int H, int Wd, int layout, int act, int guard, void *out,
                     int *info, char *kname, int kcap) {
        PB_CHECK(layout == SL_F16 || layout == SL_SPLIT16 || layout == SL_MX3, PB_ERR_ARG, "op_conv_pixshuf: layout %d (0 f16, 1 split16, 2 mx3)", layout);
        split_w_ = layout != SL_F16; mx_ = layout == SL_MX3; pack_mx2_ = 0; pack_tapin_ = 0;
        std::vector<float> bb(256);
        for (int n = 0; n < 256; ++n) bb[n] = bias[n % 64];
        PackedW w;
        PB_TRY(pack(pb_conv_rows(W, 256, 64, 9, 64).data(), 256, 576, 576, w, bb.data(), 9, 1));
        const int es = layout == SL_F16 ? 1 : 2, ld = es * 64;
        const int64_t M = (int64_t)B * H * Wd, px = M * 4;
        std::vector<f16> hx((size_t)round_up(M, 256) * ld, (f16)0.f);
        build_map(x, M, 64, 64, layout, 1, ld, hx);
        DevMem dx, dout;
        PB_TRY(up(dx, hx.data(), hx.size() * 2));
        const size_t ob = (size_t)(px + guard) * ld * 2;
        PB_TRY(preset(dout, ob));
        GemmArgs a;
        a.A = dx.as<f16>(); a.N = 256;
        a.cH = H; a.cW = Wd; a.cC = 64; a.cLd = ld; a.cKW = 3; a.cStride = 1; a.cPad = 1; a.cPadX = 1;
        set_weights(a, w, true);
        a.cOH = H; a.cOW = Wd; a.M = (int)M;
        a.out = dout.as<f16>(); a.ldo = ld; a.lo_off = layout == SL_F16 ? 0 : 64; a.act = act;
        if (layout == SL_MX3) { a.lo8 = 1; a.lo8_pa = kLo8Pa; }
        a.ps_h = H; a.ps_w = Wd; a.ps_s = 2; a.ps_co = 64;
        PB_HIP(hipDeviceSynchronize());
        pb_gemm_set_last_kernel("");
        PB_TRY(launch_gemm(stream, A_CONV, EPI_PIXSHUF, TILE_AUTO, a));
        PB_HIP(hipStreamSynchronize(stream));
        if (info) {
            const int v[8] = {w.mx_pw, kLo8Pa, w.mx2, w.sw, w.K, w.nk16, w.mx3, pb_gemm_last_splitk()};
            memcpy(info, v, sizeof(v));
        }
        if (kname && kcap > 0) snprintf(kname, kcap, "%s", pb_gemm_last_kernel());
        return down(out, dout, ob);
    }

    // SepConvGRU's fused epilogues (raft_engine.hip infer: ACT_GRU_ZR / ACT_GRU_Q through EngineBase::conv with a ConvFuse).  x [n, H, W, 384] is the
    // GRU input map ([h | inp | motion] for ZR, [r h | inp | motion] for Q) of which the convolution reads the first gc channels; mx2 (layout 3): the
    // map is [a16 (384) | a8 (384 bytes)] per pixel (576 halfs) and the epilogues store fp8 twins at byte 768.  add1 / add2 (or NULL): the hoisted
    // terms, fp16 rows of the output's stride.  which 0: ZR - w [256, gc, kh, kw]; outA = zrb (rows + guard) x 256 halfs, outB = the r h buffer
    // (rows + guard) x ld halfs.  which 1: Q - w [128, gc, kh, kw], z [rows, 256] (the z half is read); outA = the new map rows (rows + guard) x ld
    // halfs, h32 [rows + guard, 128] floats is read and written in place (the caller presets the guard rows).
    int gru(const pb_ctx *c, int which, const float *x, const float *W, const float *bias, const float *add1, const float *add2, const float *z, float *h32,
            int n, int H, int Wd, int gc, int kh, int kw, int layout, int tile, int guard, void *outA, void *outB, int *info, char *kname, int kcap) {
        PB_CHECK(layout == SL_F16 || layout == SL_MX2, PB_ERR_ARG, "op_raft_gru: layout %d (0 f16, 3 mx2)", layout);
        const bool m2 = layout == SL_MX2;
        const int N = which ? 128 : 256, ld = m2 ? 576 : 384, ldo = which ? ld : 256;
        const int64_t rows = (int64_t)n * H * Wd;
        LayerTensors l(W, bias, N, gc, kh, kw);
        PB_TRY(begin_load(l.t, 2));
        split_w_ = m2; mx_ = m2; pack_mx2_ = m2; pack_tapin_ = 0;
        PackedW w;
        PB_TRY(pack_conv("l", true, nullptr, nullptr, w, 0));
        PB_CHECK((w.mx2 != 0) == m2, PB_ERR_STATE, "op_raft_gru: the weights did not take the layout");
        std::vector<f16> hx((size_t)round_up(rows, 256) * ld, (f16)0.f);
        build_map(x, rows, 384, 384, m2 ? SL_MX2 : SL_F16, 0, ld, hx);
        DevMem dx, dh, da1, da2, dz, doA, doB;
        PB_TRY(up(dx, hx.data(), hx.size() * 2));
        PB_TRY(up(dh, h32, (size_t)(rows + guard) * 128 * 4));
        auto skip = [&](DevMem &d, const float *a) -> int {        // fp16 rows of the output's stride, the layer's N columns
            std::vector<f16> h((size_t)round_up(rows, 256) * ldo, (f16)0.f);
            for (int64_t m = 0; m < rows; ++m)
                for (int j = 0; j < N; ++j) h[(size_t)m * ldo + j] = (f16)a[m * N + j];
            return up(d, h.data(), h.size() * 2);
        };
        if (add1) { PB_TRY(skip(da1, add1)); }
        if (add2) { PB_TRY(skip(da2, add2)); }
        const size_t ab = (size_t)(rows + guard) * ldo * 2, bb = (size_t)(rows + guard) * ld * 2;
        PB_TRY(preset(doA, ab));
        ConvFuse f;
        f.gru_h = dh.as<float>(); f.add2 = da2.as<f16>();
        if (which) {
            std::vector<f16> hz((size_t)round_up(rows, 256) * 256, (f16)0.f);
            for (int64_t m = 0; m < rows; ++m)
                for (int j = 0; j < 256; ++j) hz[(size_t)m * 256 + j] = (f16)z[m * 256 + j];
            PB_TRY(up(dz, hz.data(), hz.size() * 2));
            f.gru_z = dz.as<f16>();
        } else {
            PB_TRY(preset(doB, bb));
            f.gru_rh = doB.as<f16>(); f.gru_ld = ld;
        }
        DevMem dsk;
        if (c->op_splitk) {
            PB_TRY(dsk.alloc((size_t)512 * 128 * 128 * 4));
            sk_ws_ = dsk.as<float>(); sk_cap_ = (int64_t)512 * 128 * 128;
        }
        PB_HIP(hipDeviceSynchronize());
        pb_gemm_set_last_kernel("");
        conv_tile = tile;
        const int r = conv(dx.as<f16>(), gc, ld, n, H, Wd, kh, kw, 1, w, doA.as<f16>(), ldo, which ? ACT_GRU_Q : ACT_GRU_ZR, 0, da1.as<f16>(), &f, 0,
                           m2 && gc != 384 ? 384 : 0, m2 ? 768 : 0);
        sk_ws_ = nullptr; sk_cap_ = 0;
        if (r) return r;
        PB_HIP(hipStreamSynchronize(stream));
        if (info) {
            const int v[8] = {w.mx_pw, kMx2Pa, w.mx2, w.sw, w.K, w.nk16, w.mx3, pb_gemm_last_splitk()};
            memcpy(info, v, sizeof(v));
        }
        if (kname && kcap > 0) snprintf(kname, kcap, "%s", pb_gemm_last_kernel());
        PB_TRY(down(outA, doA, ab));
        if (!which) { PB_TRY(down(outB, doB, bb)); }
        return down(h32, dh, (size_t)(rows + guard) * 128 * 4);
    }

    // fc1 as the split ViT runs it with fc2 on mx2 weights (engine.hip load / vit): plain fp16 weights on the MX build of the kernel (nk16 = K / 64,
    // every K tile an fp16 tile), GELU, and the e4m3 copy fc2 reads behind the row's fp16 part; out: (M + guard) rows of [fp16 (N) | e4m3 (N bytes)]
    int fc1(const pb_ctx *c, const float *A, const float *W, const float *bias, int M, int K, int N, int tile, int guard, void *out, int *info, char *kname,
            int kcap) {
        PackedW w;
        PB_TRY(pack_spec(W, N, K, K, w, bias, 1, PackSpec()));
        w.nk16 = K / 64;
        DevMem da, dout;
        int lda = 0;
        PB_TRY(vit_rows(da, A, M, K, K, false, lda));
        const int ldo = N + N / 2;
        const size_t ob = (size_t)(M + guard) * ldo * 2;
        PB_TRY(preset(dout, ob));
        GemmArgs a;
        a.A = da.as<f16>(); a.lda = lda; a.M = M; a.out = dout.as<f16>(); a.ldo = ldo; a.act = ACT_GELU;
        a.o8_off = N * 2; a.o8_scale = (float)(1 << kMx2Pa);
        PB_TRY(launch(c, EPI_STD, tile, a, w, info, kname, kcap));
        return down(out, dout, ob);
    }

    // a transposed convolution with kernel == stride == s as a 1 x 1 GEMM whose epilogue scatters column (dy, dx, co) of row (b, y, x) to pixel
    // (b, y s + dy, x s + dx) (DepthEngine::head, resize_layers.0 / .1): x [B h w, C] and the output in the head's map layout (0 [hi], 1 [hi | lo],
    // 2 [hi | hi8 | lo8]); Wt is ConvTranspose2d's [C, C, s, s], reordered as DepthEngine::load's pack_convT reorders it, bias [C] unpadded
    int pixshuf(const pb_ctx *c, const float *x, const float *Wt, const float *bias, int B, int h, int wd, int C, int s, int layout, int tile, int guard,
                void *out, int *info, char *kname, int kcap) {
        PB_CHECK(layout == SL_F16 || layout == SL_SPLIT16 || layout == SL_MX3, PB_ERR_ARG, "op_gemm_pixshuf: layout %d (0 f16, 1 split16, 2 mx3)", layout);
        PackSpec sp;
        sp.sa = sp.sw = layout != SL_F16; sp.mx = layout == SL_MX3; sp.tapin = 1;
        const int Cp = (int)round_up(C, 64), N = s * s * C;
        std::vector<float> g((size_t)N * Cp, 0.f);
        for (int ci = 0; ci < C; ++ci)
            for (int o = 0; o < C; ++o)
                for (int t = 0; t < s * s; ++t) g[((size_t)t * C + o) * Cp + ci] = Wt[((size_t)ci * C + o) * s * s + t];
        PackedW w;
        PB_TRY(pack_spec(g.data(), N, Cp, Cp, w, nullptr, 1, sp));
        w.Kreal = C;
        PB_TRY(upload_f32(bias, C, &w.bias));
        const int64_t M = (int64_t)B * h * wd, px = M * s * s;
        const int ld = layout == SL_F16 ? Cp : 2 * Cp;
        std::vector<float> xp((size_t)M * Cp, 0.f);
        for (int64_t m = 0; m < M; ++m) memcpy(&xp[(size_t)m * Cp], x + m * C, (size_t)C * 4);
        std::vector<f16> hx((size_t)round_up(M, 256) * ld, (f16)0.f);
        build_map(xp.data(), M, Cp, Cp, layout, 1, ld, hx);
        DevMem dx, dout;
        PB_TRY(up(dx, hx.data(), hx.size() * 2));
        const size_t ob = (size_t)(px + guard) * ld * 2;
        PB_TRY(preset(dout, ob));
        GemmArgs a;
        a.A = dx.as<f16>(); a.lda = ld; a.M = (int)M;
        a.out = dout.as<f16>(); a.ldo = ld; a.lo_off = layout == SL_F16 ? 0 : Cp; a.ps_s = s; a.ps_h = h; a.ps_w = wd; a.ps_co = C;
        if (layout == SL_MX3) { a.lo8 = 1; a.lo8_pa = kLo8Pa; }
        PB_TRY(launch(c, EPI_PIXSHUF, tile, a, w, info, kname, kcap));
        return down(out, dout, ob);
    }
};
}  // namespace

extern "C" {

// ---- single-kernel entry points ---------------------------------------------------------------
int pb_op_gemm(pb_ctx *c, const float *A, const float *W, const float *bias, float *C, int M, int N, int K, int act,
               int tile) {
    PB_CHECK(c && A && W && C && M > 0 && N > 0 && K > 0 && N % 8 == 0, PB_ERR_ARG, "op_gemm: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int Kp = (int)round_up(K, 64), Np = (int)round_up(N, 256);
    const int64_t Mp = round_up(M, 256);
    DevMem a32, w32, b32, a16, w16, c16, c32;
    PB_TRY(a32.alloc((size_t)M * K * 4)); PB_TRY(w32.alloc((size_t)N * K * 4));
    PB_TRY(a16.alloc((size_t)Mp * Kp * 2)); PB_TRY(w16.alloc((size_t)Np * Kp * 2));
    PB_TRY(c16.alloc((size_t)Mp * N * 2)); PB_TRY(c32.alloc((size_t)M * N * 4));
    PB_HIP(hipMemcpy(a32.p, A, (size_t)M * K * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(w32.p, W, (size_t)N * K * 4, hipMemcpyHostToDevice));
    if (bias) {
        PB_TRY(b32.alloc((size_t)N * 4));
        PB_HIP(hipMemcpy(b32.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    PB_TRY(launch_f32_to_f16(c->stream, a32.as<float>(), a16.as<f16>(), M, K, Kp));
    PB_TRY(launch_f32_to_f16(c->stream, w32.as<float>(), w16.as<f16>(), N, K, Kp));
    GemmArgs g;
    g.A = a16.as<f16>(); g.lda = Kp; g.W = w16.as<f16>(); g.K = Kp; g.M = M; g.N = N;
    g.bias = b32.as<float>(); g.out = c16.as<f16>(); g.ldo = N; g.act = act; g.zero = c->zero;
    DevMem skw;
    PB_TRY(lend_splitk(c, skw, g));
    PB_TRY(launch_gemm(c->stream, A_DENSE, EPI_STD, tile, g));
    PB_TRY(launch_f16_to_f32(c->stream, c16.as<f16>(), c32.as<float>(), M, N, N));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(C, c32.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_corr_volume(pb_ctx *c, const float *A, int M, const float *W, int N, int ldo, int guard_rows, float *out) {
    PB_CHECK(c && A && W && out && M > 0 && N > 0 && N % 8 == 0 && ldo >= N && guard_rows >= 0, PB_ERR_ARG, "op_corr_volume: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int64_t rows = (int64_t)M + guard_rows, Np = round_up(N, 64);
    DevMem a32, w32, a16, w16, o16, o32;
    PB_TRY(a32.alloc((size_t)M * 256 * 4)); PB_TRY(w32.alloc((size_t)N * 256 * 4));
    PB_TRY(a16.alloc((size_t)M * 256 * 2)); PB_TRY(w16.alloc((size_t)Np * 256 * 2));
    PB_TRY(o16.alloc((size_t)rows * ldo * 2)); PB_TRY(o32.alloc((size_t)rows * ldo * 4));
    PB_HIP(hipMemcpy(a32.p, A, (size_t)M * 256 * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(w32.p, W, (size_t)N * 256 * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemsetAsync(w16.p, 0, (size_t)Np * 256 * 2, c->stream));
    PB_HIP(hipMemsetAsync(o16.p, 0x7e, (size_t)rows * ldo * 2, c->stream));          // 0x7e7e: a NaN in fp16
    PB_TRY(launch_f32_to_f16(c->stream, a32.as<float>(), a16.as<f16>(), M, 256, 256));
    PB_TRY(launch_f32_to_f16(c->stream, w32.as<float>(), w16.as<f16>(), N, 256, 256));
    PB_TRY(launch_corr_volume(c->stream, a16.as<f16>(), M, w16.as<f16>(), N, (int)Np, o16.as<f16>(), ldo));
    PB_TRY(launch_f16_to_f32(c->stream, o16.as<f16>(), o32.as<float>(), rows, ldo, ldo));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(out, o32.p, (size_t)rows * ldo * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the kernel storing the blocked layout (corr_layout.h): raw halfs of round_up(M, 8) rows of ldo entries + guard_halfs behind them, preset to 0x7e7e
int pb_op_corr_volume_blocked(pb_ctx *c, const float *A, int M, const float *W, int N, int ldo, int guard_halfs, void *out) {
    PB_CHECK(c && A && W && out && M > 0 && N > 0 && N % 8 == 0 && ldo >= N && ldo % 64 == 0 && guard_halfs >= 0, PB_ERR_ARG, "op_corr_volume_blocked: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int64_t Np = round_up(N, 64);
    const size_t halfs = (size_t)corr_layout_rows(CORR_BLOCKED, M) * ldo + guard_halfs;
    DevMem a32, w32, a16, w16, o16;
    PB_TRY(a32.alloc((size_t)M * 256 * 4)); PB_TRY(w32.alloc((size_t)N * 256 * 4));
    PB_TRY(a16.alloc((size_t)M * 256 * 2)); PB_TRY(w16.alloc((size_t)Np * 256 * 2));
    PB_TRY(o16.alloc(halfs * 2));
    PB_HIP(hipMemcpy(a32.p, A, (size_t)M * 256 * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(w32.p, W, (size_t)N * 256 * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemsetAsync(w16.p, 0, (size_t)Np * 256 * 2, c->stream));
    PB_HIP(hipMemsetAsync(o16.p, 0x7e, halfs * 2, c->stream));
    PB_TRY(launch_f32_to_f16(c->stream, a32.as<float>(), a16.as<f16>(), M, 256, 256));
    PB_TRY(launch_f32_to_f16(c->stream, w32.as<float>(), w16.as<f16>(), N, 256, 256));
    PB_TRY(launch_corr_volume(c->stream, a16.as<f16>(), M, w16.as<f16>(), N, (int)Np, o16.as<f16>(), ldo, CORR_BLOCKED));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(out, o16.p, halfs * 2, hipMemcpyDeviceToHost));
    return 0;
}
// corr_layout.h's index function for the tests (needs no GPU): out[p * pld + c] = where entry c of source row p sits, p < P
int pb_op_corr_layout_index(int layout, int P, int pld, int64_t *out) {
    PB_CHECK(out && P > 0 && pld > 0 && pld % 64 == 0 && (layout == CORR_ROWMAJOR || layout == CORR_BLOCKED), PB_ERR_ARG, "op_corr_layout_index: bad arguments");
    for (int p = 0; p < P; ++p)
        for (int cc = 0; cc < pld; ++cc) out[(size_t)p * pld + cc] = corr_layout_index(layout, p, cc, pld);
    return 0;
}

int pb_op_gemm_bench(pb_ctx *c, int M, int N, int K, int tile, int epi, int iters, double *ms_out) {
    PB_CHECK(c && M > 0 && N > 0 && K > 0 && K % 64 == 0 && N % 8 == 0 && iters > 0 && ms_out, PB_ERR_ARG, "gemm_bench: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    DevMem a, w, o, r, b;
    const int64_t Mp = round_up(M, 256), Np = round_up(N, 256);
    PB_TRY(a.alloc((size_t)Mp * K * 2)); PB_TRY(w.alloc((size_t)Np * K * 2)); PB_TRY(o.alloc((size_t)Mp * N * 2));
    PB_TRY(r.alloc((size_t)Mp * N * 4)); PB_TRY(b.alloc((size_t)Np * 4));
    PB_TRY(launch_fill_random_f16(c->stream, a.as<f16>(), (int64_t)M * K, 1u, 1.f));
    PB_TRY(launch_fill_random_f16(c->stream, w.as<f16>(), (int64_t)N * K, 2u, 0.05f));
    GemmArgs g;
    g.A = a.as<f16>(); g.lda = K; g.W = w.as<f16>(); g.K = K; g.M = M; g.N = N; g.zero = c->zero; g.bias = b.as<float>();
    int e = EPI_STD, amode = A_DENSE;
    if (epi == 2) { e = EPI_RESID; g.resid = r.as<float>(); g.ldr = N; g.gamma = b.as<float>(); }
    else { g.out = o.as<f16>(); g.ldo = N; g.act = epi == 1 ? ACT_GELU : ACT_NONE; }
    if (epi >= 10) {                    // implicit-GEMM convolution over a [M / 18360, 102, 180, C] map (the RAFT update block's grid at 1080p x 0.75):
        const int taps = epi == 12 ? 5 : 9;         // 10: 3 x 3 tap-major, 11: 3 x 3 slice-major, 12: 1 x 5 tap-major; K = taps * C
        PB_CHECK(M % 18360 == 0 && K % (taps * 64) == 0, PB_ERR_ARG, "gemm_bench: conv modes need M = B * 102 * 180 and K = taps * C");
        amode = A_CONV;
        g.cH = g.cOH = 102; g.cW = g.cOW = 180; g.cC = K / taps; g.cStride = 1;
        if (epi == 12) { g.cKW = 5; g.cPad = 0; g.cPadX = 2; g.cKH = 1; }
        else { g.cKW = 3; g.cPad = 1; g.cKH = 3; g.cTapInner = epi == 11; }
    }
    const BenchEnv benv = bench_env();
    g.ablate = benv.gemm_abl;                      // PB_GEMM_ABL: timing-only epilogue ablations (wrong results): this tool op only, never an engine launch
    for (int i = 0; i < 2; ++i) PB_TRY(launch_gemm(c->stream, amode, e, tile, g));
    if (!benv.gemm_dbg.empty()) {                        // PB_GEMM_DBG=<file>: per-block stamps of one launch -> binary file
        const int nblk = (int)((Mp / 256) * (Np / 256));
        DevMem d;
        PB_TRY(d.alloc((size_t)nblk * 64));
        g.dbg = d.as<long long>();
        PB_TRY(launch_gemm(c->stream, amode, e, tile, g));
        PB_HIP(hipStreamSynchronize(c->stream));
        std::vector<long long> h((size_t)nblk * 8);
        PB_HIP(hipMemcpy(h.data(), d.p, h.size() * 8, hipMemcpyDeviceToHost));
        if (FILE *f = fopen(benv.gemm_dbg.c_str(), "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
        g.dbg = nullptr;
    }
    return time_launches(c->stream, iters, ms_out, [&] { return launch_gemm(c->stream, amode, e, tile, g); });
}

int pb_op_attention_bench(pb_ctx *c, int B, int heads, int N, int variant, int iters, double *ms_out) {
    PB_CHECK(c && B > 0 && heads > 0 && N > 0 && iters > 0 && ms_out, PB_ERR_ARG, "attention_bench: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int ntp = (int)round_up(N, 16), D = heads * 64;
    const size_t n = (size_t)B * heads * ntp * 64;
    DevMem dq, dk, dv, dout;
    PB_TRY(dq.alloc(n * 2 + 32768)); PB_TRY(dk.alloc(n * 2 + 32768)); PB_TRY(dv.alloc(n * 2 + 32768));
    PB_TRY(dout.alloc((size_t)B * ntp * D * 2));
    PB_TRY(launch_fill_random_f16(c->stream, dq.as<f16>(), (int64_t)n, 11u, 3.f * PB_QSCALE));
    PB_TRY(launch_fill_random_f16(c->stream, dk.as<f16>(), (int64_t)n, 12u, 3.f));
    PB_TRY(launch_fill_random_f16(c->stream, dv.as<f16>(), (int64_t)n, 13u, 1.f));
    auto launch = [&] { return launch_attention(c->stream, dq.as<f16>(), dk.as<f16>(), dv.as<f16>(), dout.as<f16>(), B, heads, ntp, N, D, variant); };
    for (int i = 0; i < 2; ++i) PB_TRY(launch());
    return time_launches(c->stream, iters, ms_out, launch);
}

int pb_op_layernorm(pb_ctx *c, const float *x, const float *g, const float *b, float *y, int rows, int D) {
    PB_CHECK(c && x && g && b && y && rows > 0, PB_ERR_ARG, "op_layernorm: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    DevMem dx, dg, db, dy, dy32;
    PB_TRY(dx.alloc((size_t)rows * D * 4)); PB_TRY(dg.alloc((size_t)D * 4)); PB_TRY(db.alloc((size_t)D * 4));
    PB_TRY(dy.alloc((size_t)rows * D * 2)); PB_TRY(dy32.alloc((size_t)rows * D * 4));
    PB_HIP(hipMemcpy(dx.p, x, (size_t)rows * D * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dg.p, g, (size_t)D * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(db.p, b, (size_t)D * 4, hipMemcpyHostToDevice));
    PB_TRY(launch_layernorm(c->stream, dx.as<float>(), dg.as<float>(), db.as<float>(), dy.as<f16>(), 1, rows, rows, D,
                            1e-6f, 0));
    PB_TRY(launch_f16_to_f32(c->stream, dy.as<f16>(), dy32.as<float>(), rows, D, D));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(y, dy32.p, (size_t)rows * D * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_attention(pb_ctx *c, const float *q, const float *k, const float *v, float *o, int B, int heads, int N) {
    PB_CHECK(c && q && k && v && o && B > 0 && heads > 0 && N > 0, PB_ERR_ARG, "op_attention: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int ntp = (int)round_up(N, 16), D = heads * 64;
    const size_t bh = (size_t)B * heads;
    // host-side relayout to the engine's Q / K / Vt buffers (q pre-scaled by 64^-0.5 like the qkv epilogue)
    std::vector<f16> hq(bh * ntp * 64, (f16)0.f), hk(bh * ntp * 64, (f16)0.f), hv(bh * 64 * ntp, (f16)0.f);
    for (size_t i = 0; i < bh; ++i)
        for (int t = 0; t < N; ++t)
            for (int d = 0; d < 64; ++d) {
                const size_t s = (i * N + t) * 64 + d;
                hq[(i * ntp + t) * 64 + d] = (f16)(q[s] * PB_QSCALE);
                hk[(i * ntp + t) * 64 + d] = (f16)k[s];
                hv[(i * 64 + d) * ntp + t] = (f16)v[s];
            }
    DevMem dq, dk, dv, dout, dout32;
    const size_t slack = 32768;
    PB_TRY(dq.alloc(hq.size() * 2 + slack)); PB_TRY(dk.alloc(hk.size() * 2 + slack)); PB_TRY(dv.alloc(hv.size() * 2 + slack));
    PB_TRY(dout.alloc((size_t)B * ntp * D * 2)); PB_TRY(dout32.alloc((size_t)B * ntp * D * 4));
    PB_HIP(hipMemcpy(dq.p, hq.data(), hq.size() * 2, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dk.p, hk.data(), hk.size() * 2, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dv.p, hv.data(), hv.size() * 2, hipMemcpyHostToDevice));
    PB_TRY(launch_attention(c->stream, dq.as<f16>(), dk.as<f16>(), dv.as<f16>(), dout.as<f16>(), B, heads, ntp, N, D));
    PB_TRY(launch_f16_to_f32(c->stream, dout.as<f16>(), dout32.as<float>(), (int64_t)B * ntp, D, D));
    PB_HIP(hipStreamSynchronize(c->stream));
    std::vector<float> ho((size_t)B * ntp * D);
    PB_HIP(hipMemcpy(ho.data(), dout32.p, ho.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
        for (int h = 0; h < heads; ++h)
            for (int t = 0; t < N; ++t)
                for (int d = 0; d < 64; ++d)
                    o[(((size_t)b * heads + h) * N + t) * 64 + d] = ho[((size_t)b * ntp + t) * D + h * 64 + d];
    return 0;
}

int pb_op_attention128(pb_ctx *c, const float *q, const float *k, const float *v, const int8_t *region, float *o, int B, int L) {
    PB_CHECK(c && q && k && v && o && B > 0 && L > 0, PB_ERR_ARG, "op_attention128: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int ldv = (int)round_up(L, 32);
    const size_t n = (size_t)B * L * 128;
    std::vector<f16> hq(n), hk(n), hv((size_t)B * 128 * ldv, (f16)0.f);
    for (size_t i = 0; i < n; ++i) { hq[i] = (f16)q[i]; hk[i] = (f16)k[i]; }
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < L; ++t)
            for (int d = 0; d < 128; ++d) hv[((size_t)b * 128 + d) * ldv + t] = (f16)v[((size_t)b * L + t) * 128 + d];
    DevMem dq, dk, dv, dr, dout;
    PB_TRY(dq.alloc(n * 2)); PB_TRY(dk.alloc(n * 2)); PB_TRY(dv.alloc(hv.size() * 2)); PB_TRY(dout.alloc(n * 4));
    PB_HIP(hipMemcpy(dq.p, hq.data(), n * 2, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dk.p, hk.data(), n * 2, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dv.p, hv.data(), hv.size() * 2, hipMemcpyHostToDevice));
    if (region) {
        PB_TRY(dr.alloc((size_t)B * L));
        PB_HIP(hipMemcpy(dr.p, region, (size_t)B * L, hipMemcpyHostToDevice));
    }
    PB_TRY(launch_attention128(c->stream, dq.as<f16>(), dk.as<f16>(), dv.as<f16>(), region ? dr.as<int8_t>() : nullptr, dout.as<float>(), B, L, ldv));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(o, dout.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_attention128_split(pb_ctx *c, const float *q, const float *k, const float *v, const int8_t *region, int nreg, float *o, int B, int L,
                             int vcols, int kxor) {
    PB_CHECK(c && q && k && v && o && B > 0 && L > 0 && (vcols == 128 || vcols == 32), PB_ERR_ARG, "op_attention128_split: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int ldv = (int)round_up(L, 32);
    const size_t n = (size_t)B * L * 128;
    std::vector<f16> hq(2 * n), hk(2 * n), hv((size_t)B * 2 * vcols * ldv, (f16)0.f);
    auto split = [](float x, f16 &hi, f16 &lo) { hi = (f16)x; lo = (f16)(x - (float)hi); };
    for (size_t r = 0; r < (size_t)B * L; ++r)
        for (int d = 0; d < 128; ++d) {
            split(q[r * 128 + d], hq[r * 256 + d], hq[r * 256 + 128 + d]);
            split(k[r * 128 + d], hk[r * 256 + d], hk[r * 256 + 128 + d]);
        }
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < L; ++t)
            for (int d = 0; d < vcols; ++d)
                split(v[((size_t)b * L + t) * vcols + d], hv[(((size_t)b * 2 + 0) * vcols + d) * ldv + t], hv[(((size_t)b * 2 + 1) * vcols + d) * ldv + t]);
    DevMem dq, dk, dv, dr, dout;
    PB_TRY(dq.alloc(2 * n * 2)); PB_TRY(dk.alloc(2 * n * 2)); PB_TRY(dv.alloc(hv.size() * 2)); PB_TRY(dout.alloc((size_t)B * L * vcols * 4));
    PB_HIP(hipMemcpy(dq.p, hq.data(), 2 * n * 2, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dk.p, hk.data(), 2 * n * 2, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dv.p, hv.data(), hv.size() * 2, hipMemcpyHostToDevice));
    if (region) {
        PB_TRY(dr.alloc((size_t)nreg * L));
        PB_HIP(hipMemcpy(dr.p, region, (size_t)nreg * L, hipMemcpyHostToDevice));
    }
    Attn128Args a;
    a.Q = dq.as<f16>(); a.K = dk.as<f16>(); a.Vt = dv.as<f16>(); a.region = region ? dr.as<int8_t>() : nullptr; a.nreg = nreg;
    a.O = dout.as<float>(); a.B = B; a.L = L; a.ldv = ldv; a.split = 1; a.vcols = vcols; a.kxor = kxor;
    PB_TRY(launch_attention128x(c->stream, a));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(o, dout.p, (size_t)B * L * vcols * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_conv2d(pb_ctx *c, const float *x, const float *w, const float *bias, float *y, int B, int Ci, int H, int W,
                 int Co, int ks, int stride, int pad, int relu_in, int relu_out) {
    PB_CHECK(c && x && w && y && Co % 8 == 0 && (ks == 1 || ks == 3), PB_ERR_ARG, "op_conv2d: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const int cip = (int)round_up(Ci, 64), cop = (int)round_up(Co, 64), K = ks * ks * cip;
    const int OH = (H + 2 * pad - ks) / stride + 1, OW = (W + 2 * pad - ks) / stride + 1;
    std::vector<f16> hw((size_t)round_up(Co, 256) * K, (f16)0.f);
    for (int o = 0; o < Co; ++o)
        for (int ci = 0; ci < Ci; ++ci)
            for (int t = 0; t < ks * ks; ++t)
                hw[(size_t)o * K + t * cip + ci] = (f16)w[((size_t)o * Ci + ci) * ks * ks + t];
    DevMem dx32, dx, dw, db, dy, dy32;
    PB_TRY(dx32.alloc((size_t)B * Ci * H * W * 4)); PB_TRY(dx.alloc((size_t)round_up((int64_t)B * H * W, 256) * cip * 2));
    PB_TRY(dw.alloc(hw.size() * 2)); PB_TRY(dy.alloc((size_t)round_up((int64_t)B * OH * OW, 256) * cop * 2));
    PB_TRY(dy32.alloc((size_t)B * Co * OH * OW * 4));
    PB_HIP(hipMemcpy(dx32.p, x, (size_t)B * Ci * H * W * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dw.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    if (bias) {
        PB_TRY(db.alloc((size_t)Co * 4));
        PB_HIP(hipMemcpy(db.p, bias, (size_t)Co * 4, hipMemcpyHostToDevice));
    }
    PB_TRY(launch_nchw_f32_to_nhwc_f16(c->stream, dx32.as<float>(), dx.as<f16>(), B, Ci, H, W, cip, relu_in));
    GemmArgs g;
    g.A = dx.as<f16>(); g.W = dw.as<f16>(); g.K = K; g.M = B * OH * OW; g.N = Co;
    g.cH = H; g.cW = W; g.cC = cip; g.cOH = OH; g.cOW = OW; g.cKW = ks; g.cStride = stride; g.cPad = pad;
    g.zero = c->zero; g.bias = db.as<float>(); g.out = dy.as<f16>(); g.ldo = cop; g.act = relu_out ? ACT_RELU : ACT_NONE;
    DevMem skw;
    PB_TRY(lend_splitk(c, skw, g));
    PB_TRY(launch_gemm(c->stream, A_CONV, EPI_STD, c->conv_tile ? c->conv_tile : TILE_128, g));
    PB_TRY(launch_nhwc_f16_to_nchw_f32(c->stream, dy.as<f16>(), dy32.as<float>(), B, Co, OH, OW, cop));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(y, dy32.p, (size_t)B * Co * OH * OW * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_bilinear(pb_ctx *c, const float *x, float *y, int B, int C, int H, int W, int OH, int OW, int align) {
    PB_CHECK(c && x && y && C % 8 == 0, PB_ERR_ARG, "op_bilinear: bad arguments (C %% 8)");
    PB_HIP(hipSetDevice(c->device));
    DevMem dx32, dx, dy, dy32;
    PB_TRY(dx32.alloc((size_t)B * C * H * W * 4)); PB_TRY(dx.alloc((size_t)B * C * H * W * 2));
    PB_TRY(dy.alloc((size_t)B * C * OH * OW * 2)); PB_TRY(dy32.alloc((size_t)B * C * OH * OW * 4));
    PB_HIP(hipMemcpy(dx32.p, x, (size_t)B * C * H * W * 4, hipMemcpyHostToDevice));
    PB_TRY(launch_nchw_f32_to_nhwc_f16(c->stream, dx32.as<float>(), dx.as<f16>(), B, C, H, W, C, 0));
    PB_TRY(launch_bilinear_nhwc(c->stream, dx.as<f16>(), dy.as<f16>(), B, H, W, OH, OW, C, C, align));
    PB_TRY(launch_nhwc_f16_to_nchw_f32(c->stream, dy.as<f16>(), dy32.as<float>(), B, C, OH, OW, C));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(y, dy32.p, (size_t)B * C * OH * OW * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_preprocess(pb_ctx *c, const uint8_t *frame, int H, int W, float *out, int net_h, int net_w) {
    PB_CHECK(c && frame && out, PB_ERR_ARG, "op_preprocess: bad arguments");
    int nh, nw;
    PB_TRY(pb_depth_net_size(H, W, &nh, &nw));
    PB_CHECK(nh == net_h && nw == net_w, PB_ERR_ARG, "op_preprocess: net size is %dx%d, caller passed %dx%d", nh, nw,
             net_h, net_w);
    PB_HIP(hipSetDevice(c->device));
    std::vector<int> xi((size_t)nw * 4), yi((size_t)nh * 4);
    std::vector<float> xw((size_t)nw * 4), yw((size_t)nh * 4);
    pb_cubic_taps(W, nw, xi.data(), xw.data());
    pb_cubic_taps(H, nh, yi.data(), yw.data());
    DevMem df, dxi, dxw, dyi, dyw, dout;
    PB_TRY(df.alloc((size_t)H * W * 3)); PB_TRY(dxi.alloc(xi.size() * 4)); PB_TRY(dxw.alloc(xw.size() * 4));
    PB_TRY(dyi.alloc(yi.size() * 4)); PB_TRY(dyw.alloc(yw.size() * 4)); PB_TRY(dout.alloc((size_t)3 * nh * nw * 4));
    PB_HIP(hipMemcpy(df.p, frame, (size_t)H * W * 3, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dxi.p, xi.data(), xi.size() * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dxw.p, xw.data(), xw.size() * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dyi.p, yi.data(), yi.size() * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(dyw.p, yw.data(), yw.size() * 4, hipMemcpyHostToDevice));
    PB_TRY(launch_preprocess(c->stream, df.as<uint8_t>(), 1, H, W, nh, nw, dxi.as<int>(), dxw.as<float>(), dyi.as<int>(),
                             dyw.as<float>(), nullptr, 640, dout.as<float>()));
    PB_HIP(hipStreamSynchronize(c->stream));
    PB_HIP(hipMemcpy(out, dout.p, (size_t)3 * nh * nw * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_encode_depth(pb_ctx *c, const float *depth, int n, int H, int W, int flip, uint8_t *rgb, float *mn, float *mx) {
    PB_CHECK(c && depth && n > 0, PB_ERR_ARG, "op_encode_depth: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    const size_t px = (size_t)H * W;
    DevMem dd, dr, dm, dmn;
    PB_TRY(dd.alloc(n * px * 4)); PB_TRY(dr.alloc(n * px * 3)); PB_TRY(dm.alloc((size_t)n * 8)); PB_TRY(dmn.alloc((size_t)n * 8));
    PB_HIP(hipMemcpy(dd.p, depth, n * px * 4, hipMemcpyHostToDevice));
    PB_TRY(launch_init_minmax(c->stream, dm.as<unsigned>(), n));
    PB_TRY(launch_minmax_only(c->stream, dd.as<float>(), n, (int64_t)px, dm.as<unsigned>()));
    PB_TRY(launch_heat_encode(c->stream, dd.as<float>(), n, H, W, dm.as<unsigned>(), flip, dr.as<uint8_t>(),
                              dmn.as<float>(), dmn.as<float>() + n));
    PB_HIP(hipStreamSynchronize(c->stream));
    if (rgb) PB_HIP(hipMemcpy(rgb, dr.p, n * px * 3, hipMemcpyDeviceToHost));
    if (mn) PB_HIP(hipMemcpy(mn, dmn.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (mx) PB_HIP(hipMemcpy(mx, dmn.as<float>() + n, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pb_op_conv2d_split(pb_ctx *c, const float *x, const float *w, const float *bias, const float *skip, int B, int H, int W, int Ci, int Ctot,
                       int ci_off, int Co, int kh, int kw, int stride, int layout, int sa, int tapin, int tile, int split_out, int act, int pre_relu,
                       int rows_out, void *out, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && x && w && bias && out && B > 0 && H > 0 && W > 0 && kh >= 1 && kw >= 1 && (stride == 1 || stride == 2), PB_ERR_ARG,
             "op_conv2d_split: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    LayerTensors l(w, bias, Co, Ci, kh, kw);
    SplitOpEngine e(c->device);
    PB_TRY(e.setup(l.t, 2, layout, tapin));
    return e.run(true, x, skip, B, H, W, Ci, Ctot ? Ctot : Ci, ci_off, Co, kh, kw, stride, layout, sa, tile, c->op_splitk, split_out, act, pre_relu,
                 rows_out, out, info, kernel, kernel_cap);
}

int pb_op_dense_split(pb_ctx *c, const float *A, const float *w, const float *bias, const float *skip, int M, int K, int N, int layout, int sa,
                      int tile, int split_out, int act, int rows_out, void *out, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && A && w && bias && out && M > 0 && K > 0, PB_ERR_ARG, "op_dense_split: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    LayerTensors l(w, bias, N, K);
    SplitOpEngine e(c->device);
    PB_TRY(e.setup(l.t, 2, layout, 0));
    return e.run(false, A, skip, M, 1, 1, K, K, 0, N, 1, 1, 1, layout, sa, tile, c->op_splitk, split_out, act, 0, rows_out, out, info, kernel,
                 kernel_cap);
}

// ---- the GEMM's fused epilogues one by one (EpiOpEngine above) ----
#define EPI_OP_ENGINE(e) PB_HIP(hipSetDevice(c->device)); EpiOpEngine e(c->device); PB_TRY(e.setup(nullptr, 0, SL_F16, 0))
int pb_op_gemm_resid(pb_ctx *c, const float *A, const float *w, const float *bias, const float *gamma, const float *X, int M, int N, int K, int ldr,
                     int layout, int tile, int guard_rows, float *out, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && A && w && bias && gamma && X && out && M > 0 && N > 0 && N % 8 == 0 && K > 0 && K % 64 == 0 && ldr >= N && ldr % 4 == 0 && guard_rows >= 0,
             PB_ERR_ARG, "op_gemm_resid: bad arguments");
    EPI_OP_ENGINE(e);
    return e.resid(c, A, w, bias, gamma, X, M, N, K, ldr, layout, tile, guard_rows, out, info, kernel, kernel_cap);
}
int pb_op_gemm_qkv(pb_ctx *c, const float *A, const float *w, const float *bias, int B, int ntp, int D, int layout, int tile, int guard_rows, void *q,
                   void *k, void *vt, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && A && w && bias && q && k && vt && B > 0 && ntp > 0 && ntp % 16 == 0 && D > 0 && D % 128 == 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_gemm_qkv: bad arguments");
    EPI_OP_ENGINE(e);
    return e.qkv(c, A, w, bias, B, ntp, D, layout, tile, guard_rows, q, k, vt, info, kernel, kernel_cap);
}
int pb_op_gemm_patch(pb_ctx *c, const float *A, const float *w, const float *bias, const float *pos, int B, int P, int ntp, int D, int layout,
                     int guard_rows, float *out, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && A && w && bias && pos && out && B > 0 && P > 0 && ntp >= P + 1 && D > 0 && D % 128 == 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_gemm_patch: bad arguments");
    EPI_OP_ENGINE(e);
    return e.patch(c, A, w, bias, pos, B, P, ntp, D, layout, guard_rows, out, info, kernel, kernel_cap);
}
int pb_op_conv_head(pb_ctx *c, const float *x, const float *w, const float *bias, const float *w2, float b2, int B, int H, int W, int C, int layout,
                    int guard_rows, float *out, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && x && w && bias && w2 && out && B > 0 && H > 0 && W > 0 && C > 0 && guard_rows >= 0, PB_ERR_ARG, "op_conv_head: bad arguments");
    EPI_OP_ENGINE(e);
    return e.head(c, x, w, bias, w2, b2, B, H, W, C, layout, guard_rows, out, info, kernel, kernel_cap);
}
int pb_op_conv_pixshuf(pb_ctx *c, const float *x, const float *w, const float *bias, int B, int H, int W, int layout, int act, int guard_rows, void *out,
                       int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && x && w && bias && out && B > 0 && H > 0 && W > 0 && (act == ACT_NONE || act == ACT_RELU) && guard_rows >= 0, PB_ERR_ARG,
             "op_conv_pixshuf: bad arguments");
    EPI_OP_ENGINE(e);
    return e.pixshuf_conv(c, x, w, bias, B, H, W, layout, act, guard_rows, out, info, kernel, kernel_cap);
}
int pb_op_raft_gru_zr(pb_ctx *c, const float *x, const float *w, const float *bias, const float *add1, const float *add2, float *h32, int n, int H, int W,
                      int gc, int kh, int kw, int layout, int tile, int guard_rows, void *zrb, void *rh, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && x && w && bias && h32 && zrb && rh && n > 0 && H > 0 && W > 0 && (gc == 256 || gc == 384) && kh >= 1 && kw >= 1 && guard_rows >= 0,
             PB_ERR_ARG, "op_raft_gru_zr: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    EpiOpEngine e(c->device);
    return e.gru(c, 0, x, w, bias, add1, add2, nullptr, h32, n, H, W, gc, kh, kw, layout, tile, guard_rows, zrb, rh, info, kernel, kernel_cap);
}
int pb_op_raft_gru_q(pb_ctx *c, const float *x, const float *w, const float *bias, const float *add1, const float *add2, const float *z, float *h32, int n,
                     int H, int W, int gc, int kh, int kw, int layout, int tile, int guard_rows, void *out, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && x && w && bias && z && h32 && out && n > 0 && H > 0 && W > 0 && (gc == 256 || gc == 384) && kh >= 1 && kw >= 1 && guard_rows >= 0,
             PB_ERR_ARG, "op_raft_gru_q: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    EpiOpEngine e(c->device);
    return e.gru(c, 1, x, w, bias, add1, add2, z, h32, n, H, W, gc, kh, kw, layout, tile, guard_rows, out, nullptr, info, kernel, kernel_cap);
}
int pb_op_gemm_fc1(pb_ctx *c, const float *A, const float *w, const float *bias, int M, int K, int N, int tile, int guard_rows, void *out, int *info,
                   char *kernel, int kernel_cap) {
    PB_CHECK(c && A && w && bias && out && M > 0 && K > 0 && K % 64 == 0 && N > 0 && N % 64 == 0 && guard_rows >= 0, PB_ERR_ARG, "op_gemm_fc1: bad arguments");
    EPI_OP_ENGINE(e);
    return e.fc1(c, A, w, bias, M, K, N, tile, guard_rows, out, info, kernel, kernel_cap);
}
int pb_op_gemm_pixshuf(pb_ctx *c, const float *x, const float *wt, const float *bias, int B, int h, int w, int C, int s, int layout, int tile,
                       int guard_rows, void *out, int *info, char *kernel, int kernel_cap) {
    PB_CHECK(c && x && wt && bias && out && B > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0 && s >= 1 && s <= 4 && guard_rows >= 0, PB_ERR_ARG,
             "op_gemm_pixshuf: bad arguments");
    EPI_OP_ENGINE(e);
    return e.pixshuf(c, x, wt, bias, B, h, w, C, s, layout, tile, guard_rows, out, info, kernel, kernel_cap);
}

// ---- the flow_raft band's kernels one by one (RaftOpEngine above) ----
int pb_op_raft_geometry(int h8, int w8, int *geo) {
    PB_CHECK(geo && h8 >= 1 && w8 >= 1, PB_ERR_ARG, "op_raft_geometry: bad arguments");
    CorrGeo g;
    corr_pyramid_geometry(h8, w8, g);
    for (int l = 0; l < 4; ++l) { geo[l * 5] = g.h[l]; geo[l * 5 + 1] = g.w[l]; geo[l * 5 + 2] = g.wp[l]; geo[l * 5 + 3] = g.hp[l]; geo[l * 5 + 4] = g.ld[l]; }
    return 0;
}
#define RAFT_OP_ENGINE(e) PB_HIP(hipSetDevice(c->device)); RaftOpEngine e(c->device); PB_TRY(e.setup(nullptr, 0, SL_F16, 0))
int pb_op_raft_lookup(pb_ctx *c, const float *fmap1, const float *fmap2, const float *flow, int n, int h8, int w8, int o8, int guard_rows, void *out,
                      float *levels) {
    PB_CHECK(c && fmap1 && fmap2 && flow && out && n > 0 && guard_rows >= 0, PB_ERR_ARG, "op_raft_lookup: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.lookup(fmap1, fmap2, flow, n, h8, w8, o8, guard_rows, out, levels, launch_env().volume ? c->corr_layout : CORR_ROWMAJOR);
}
int pb_op_raft_lookup_otf(pb_ctx *c, const float *fmap1, const float *fmap2, const float *flow, int n, int h8, int w8, int o8, int guard_rows, void *out) {
    PB_CHECK(c && fmap1 && fmap2 && flow && out && n > 0 && guard_rows >= 0, PB_ERR_ARG, "op_raft_lookup_otf: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.lookup_otf(fmap1, fmap2, flow, n, h8, w8, o8, guard_rows, out);
}
int pb_op_raft_convf1(pb_ctx *c, const float *flow, const float *w, const float *bias, int n, int h8, int w8, int passes, int o8, int gemm_path,
                      int guard_rows, void *out) {
    PB_CHECK(c && flow && w && bias && out && n > 0 && h8 > 0 && w8 > 0 && (passes == 1 || passes == 2) && guard_rows >= 0, PB_ERR_ARG,
             "op_raft_convf1: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.convf1(flow, w, bias, n, h8, w8, passes, o8, gemm_path, guard_rows, out);
}
int pb_op_raft_flow_head2(pb_ctx *c, const float *x, const float *w, const float *bias, float *flow, int n, int H, int W, int split, int guard_rows) {
    PB_CHECK(c && x && w && bias && flow && n > 0 && H > 0 && W > 0 && guard_rows >= 0, PB_ERR_ARG, "op_raft_flow_head2: bad arguments");
    PB_HIP(hipSetDevice(c->device));
    LayerTensors l(w, bias, 2, 256, 3, 3);
    RaftOpEngine e(c->device);
    PB_TRY(e.setup(l.t, 2, SL_F16, 0));
    return e.flow_head2(x, flow, n, H, W, split, guard_rows);
}
int pb_op_raft_upsample(pb_ctx *c, const float *flow, const float *mask, int n, int h8, int w8, int pad_l, int pad_t, int sh, int sw, int guard,
                        float *up, float *maxd) {
    PB_CHECK(c && flow && mask && up && maxd && n > 0 && h8 > 0 && w8 > 0 && sh > 0 && sw > 0 && pad_l >= 0 && pad_t >= 0 && guard >= 0 &&
             pad_t + sh <= 8 * h8 && pad_l + sw <= 8 * w8, PB_ERR_ARG, "op_raft_upsample: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.upsample(flow, mask, n, h8, w8, pad_l, pad_t, sh, sw, guard, up, maxd);
}
int pb_op_raft_instnorm(pb_ctx *c, const float *a, const float *b, int B, int HW, int C, int layout, int stats_lo, int bmode, int inplace,
                        int guard_rows, float *stats, void *out) {
    PB_CHECK(c && a && stats && out && B > 0 && HW > 0 && C > 0 && layout >= 0 && layout <= 2 && bmode >= 0 && bmode <= 2 && (b || !bmode) &&
             guard_rows >= 0, PB_ERR_ARG, "op_raft_instnorm: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.instnorm(a, b, B, HW, C, layout, stats_lo, bmode, inplace, guard_rows, stats, out);
}
int pb_op_raft_state(pb_ctx *c, const float *ctx_rows, const float *flow, int rows, int ld, int inp_off, int guard_rows, float *h32, void *hx,
                     void *hx2, float *flow0) {
    PB_CHECK(c && ctx_rows && flow && h32 && hx && hx2 && flow0 && rows > 0 && (ld == 384 || ld == 576) && (inp_off == 128 || inp_off == 256) &&
             guard_rows >= 0, PB_ERR_ARG, "op_raft_state: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.state(ctx_rows, flow, rows, ld, inp_off, guard_rows, h32, hx, hx2, flow0);
}

// ---- the flow bands' frame prep and flow tail (RaftOpEngine above); geometry and taps need no GPU ----
int pb_op_flow_geometry(int H, int W, float scale, int factor, int *geo) {
    PB_CHECK(geo && H > 0 && W > 0 && scale > 0.f && (factor == 8 || factor == 16 || factor == 32), PB_ERR_ARG, "op_flow_geometry: bad arguments");
    const FlowGeometry g = flow_geometry(H, W, scale, factor);
    const int v[9] = {g.sh, g.sw, g.Hp, g.Wp, g.padl, g.padt, g.h8, g.w8, g.P};
    memcpy(geo, v, sizeof(v));
    return 0;
}
int pb_op_flow_taps(int src, int dst, float scale, int *idx, int *co) {
    PB_CHECK(idx && co && src > 0 && dst > 0 && scale > 0.f, PB_ERR_ARG, "op_flow_taps: bad arguments");
    std::vector<int> i, c;
    pb_flow_cubic_taps(src, dst, scale, i, c);
    memcpy(idx, i.data(), i.size() * 4);
    memcpy(co, c.data(), c.size() * 4);
    return 0;
}
int pb_op_flow_prep(pb_ctx *c, const uint8_t *frames, int n, int H, int W, float scale, int factor, int layout, int norm_mode, int isz_h, int isz_w,
                    int guard_rows, int guard, void *out, uint8_t *scaled, int *lo8_pa) {
    PB_CHECK(c && frames && out && scaled && n > 0 && H > 0 && W > 0 && scale > 0.f && (factor == 8 || factor == 16 || factor == 32) && layout >= 0 &&
             layout <= 2 && (norm_mode == 0 || norm_mode == 1) && isz_h >= 0 && (isz_h > 0) == (isz_w > 0) && guard_rows >= 0 && guard >= 0, PB_ERR_ARG,
             "op_flow_prep: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.flow_prep(frames, n, H, W, scale, factor, layout, norm_mode, isz_h, isz_w, guard_rows, guard, out, scaled, lo8_pa);
}
int pb_op_flow_resize_back(pb_ctx *c, const float *in, int n, int ih, int iw, int sh, int sw, int guard, float *out, float *maxd) {
    PB_CHECK(c && in && out && maxd && n > 0 && ih > 0 && iw > 0 && sh > 0 && sw > 0 && guard >= 0, PB_ERR_ARG, "op_flow_resize_back: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.flow_resize_back(in, n, ih, iw, sh, sw, guard, out, maxd);
}
int pb_op_flow_encode(pb_ctx *c, const float *flow, const float *maxd, int n, int sh, int sw, int guard, uint8_t *rgb, float *max_out) {
    PB_CHECK(c && flow && maxd && rgb && max_out && n > 0 && sh > 0 && sw > 0 && guard >= 0, PB_ERR_ARG, "op_flow_encode: bad arguments");
    RAFT_OP_ENGINE(e);
    return e.flow_encode(flow, maxd, n, sh, sw, guard, rgb, max_out);
}

// ---- the flow_gmflow band's kernels one by one (GmOpEngine above) ----
int pb_op_gm_tables(int h8, int w8, float *pos, int8_t *region) {
    PB_CHECK(pos && region && h8 >= 4 && w8 >= 4 && h8 % 2 == 0 && w8 % 2 == 0, PB_ERR_ARG, "op_gm_tables: bad arguments");
    std::vector<float> p;
    std::vector<int8_t> r;
    sine_positions(h8, w8, p);
    shift_regions(h8, w8, r);
    memcpy(pos, p.data(), p.size() * 4);
    memcpy(region, r.data(), r.size());
    return 0;
}
int pb_op_gm_tables_n(int h, int w, int splits, float *pos, int8_t *region) {
    PB_CHECK(pos && region && (splits == 2 || splits == 8) && h >= 2 * splits && w >= 2 * splits && h % splits == 0 && w % splits == 0, PB_ERR_ARG,
             "op_gm_tables_n: bad arguments");
    std::vector<float> p;
    std::vector<int8_t> r;
    sine_positions(h, w, p, splits);
    shift_regions(h, w, r, splits);
    memcpy(pos, p.data(), p.size() * 4);
    memcpy(region, r.data(), r.size());
    return 0;
}
#define GM_OP_ENGINE(e) PB_HIP(hipSetDevice(c->device)); GmOpEngine e(c->device); PB_TRY(e.setup(nullptr, 0, SL_F16, 0))
int pb_op_gm_tokens_warped(pb_ctx *c, const float *feat, const float *warped, const float *pos, int B, int dirs, int P, int guard_rows, float *X,
                           void *Xs) {
    PB_CHECK(c && feat && warped && pos && X && Xs && B > 0 && (dirs == 1 || dirs == 2) && B % dirs == 0 && P > 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_gm_tokens_warped: bad arguments");
    GM_OP_ENGINE(e);
    return e.tokens_warped(feat, warped, pos, B, dirs, P, guard_rows, X, Xs);
}
int pb_op_gm_warp(pb_ctx *c, const float *flow8, const float *feat4, int B, int dirs, int h8, int w8, int guard_rows, float *flow_up, float *warped) {
    PB_CHECK(c && flow8 && feat4 && flow_up && warped && B > 0 && (dirs == 1 || dirs == 2) && B % dirs == 0 && h8 >= 2 && w8 >= 2 && guard_rows >= 0,
             PB_ERR_ARG, "op_gm_warp: bad arguments");
    GM_OP_ENGINE(e);
    return e.warp(flow8, feat4, B, dirs, h8, w8, guard_rows, flow_up, warped);
}
int pb_op_gm_upsample(pb_ctx *c, const float *flow, const float *mask, int n, int h, int w, int factor, int pad_l, int pad_t, int sh, int sw, int guard,
                      float *up, float *maxd) {
    PB_CHECK(c && flow && mask && up && maxd && n > 0 && h > 0 && w > 0 && (factor == 4 || factor == 8) && sh > 0 && sw > 0 && pad_l >= 0 &&
             pad_t >= 0 && guard >= 0 && pad_t + sh <= factor * h && pad_l + sw <= factor * w, PB_ERR_ARG, "op_gm_upsample: bad arguments");
    GM_OP_ENGINE(e);
    return e.upsample(flow, mask, n, h, w, pad_l, pad_t, sh, sw, guard, up, maxd, factor);
}
int pb_op_gm_pack_n(pb_ctx *c, const float *src, int images, int h, int w, int splits, int ld, int njobs, const int *cols, const int *kinds, int shifted,
                    int guard_rows, void **outs) {
    PB_CHECK(c && src && cols && kinds && outs && images > 0 && njobs >= 1 && njobs <= 5 && ld % 4 == 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_gm_pack_n: bad arguments");
    for (int j = 0; j < njobs; ++j)
        PB_CHECK(outs[j] && cols[j] >= 0 && cols[j] % 8 == 0 && cols[j] + 128 <= ld, PB_ERR_ARG, "op_gm_pack_n: job %d takes columns %d.. of %d", j, cols[j], ld);
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h, w, splits));
    return e.pack(src, images, ld, njobs, cols, kinds, shifted, guard_rows, outs);
}
int pb_op_gm_ln_n(pb_ctx *c, const float *M, const float *gamma, const float *beta, float *X, int rows, int xrows, int h, int w, int splits, int windowed,
                  int shifted, int mode, int guard_rows, void *out) {
    PB_CHECK(c && M && gamma && beta && X && out && rows > 0 && rows <= xrows && (mode == 0 || mode == 1) && guard_rows >= 0, PB_ERR_ARG,
             "op_gm_ln_n: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h, w, splits));
    PB_CHECK(!windowed || xrows % e.g.P == 0, PB_ERR_ARG, "op_gm_ln_n: windowed rows address whole images of %d tokens, X has %d rows", e.g.P, xrows);
    return e.ln(M, gamma, beta, X, rows, xrows, windowed, shifted, mode, guard_rows, out);
}
int pb_op_gm_window_block_n(pb_ctx *c, const float *Y, float *X, const float *gamma, const float *beta, int images, int h, int w, int splits,
                            int shifted, int cross, int split, int pv_single) {
    PB_CHECK(c && Y && X && gamma && beta && images > 0 && (!cross || images % 2 == 0) && (pv_single == 0 || pv_single == 1), PB_ERR_ARG,
             "op_gm_window_block_n: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h, w, splits));
    return e.window_block(Y, X, gamma, beta, images, shifted, cross, split, pv_single);
}
int pb_op_gm_tokens(pb_ctx *c, const float *feat, const float *pos, int NP, int P, int guard_rows, float *X, void *Xs) {
    PB_CHECK(c && feat && pos && X && Xs && NP > 0 && P > 0 && guard_rows >= 0, PB_ERR_ARG, "op_gm_tokens: bad arguments");
    GM_OP_ENGINE(e);
    return e.tokens(feat, pos, NP, P, guard_rows, X, Xs);
}
int pb_op_gm_split_rows(pb_ctx *c, const float *src, int rows, int ld, int C, int guard_rows, void *out) {
    PB_CHECK(c && src && out && rows > 0 && C > 0 && ld >= C && guard_rows >= 0, PB_ERR_ARG, "op_gm_split_rows: bad arguments");
    GM_OP_ENGINE(e);
    return e.split_rows(src, rows, ld, C, guard_rows, out);
}
int pb_op_gm_grid_vt(pb_ctx *c, int h8, int w8, int guard_rows, void *out) {
    PB_CHECK(c && out && guard_rows >= 0, PB_ERR_ARG, "op_gm_grid_vt: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.grid_vt(guard_rows, out);
}
int pb_op_gm_pack(pb_ctx *c, const float *src, int images, int h8, int w8, int ld, int njobs, const int *cols, const int *kinds, int shifted,
                  int guard_rows, void **outs) {
    PB_CHECK(c && src && cols && kinds && outs && images > 0 && njobs >= 1 && njobs <= 5 && ld % 4 == 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_gm_pack: bad arguments");
    for (int j = 0; j < njobs; ++j)
        PB_CHECK(outs[j] && cols[j] >= 0 && cols[j] % 8 == 0 && cols[j] + 128 <= ld, PB_ERR_ARG, "op_gm_pack: job %d takes columns %d.. of %d", j, cols[j], ld);
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.pack(src, images, ld, njobs, cols, kinds, shifted, guard_rows, outs);
}
int pb_op_gm_ln(pb_ctx *c, const float *M, const float *gamma, const float *beta, float *X, int rows, int xrows, int h8, int w8, int windowed,
                int shifted, int mode, int guard_rows, void *out) {
    PB_CHECK(c && M && gamma && beta && X && out && rows > 0 && rows <= xrows && (mode == 0 || mode == 1) && guard_rows >= 0, PB_ERR_ARG,
             "op_gm_ln: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    PB_CHECK(!windowed || xrows % e.g.P == 0, PB_ERR_ARG, "op_gm_ln: windowed rows address whole images of %d tokens, X has %d rows", e.g.P, xrows);
    return e.ln(M, gamma, beta, X, rows, xrows, windowed, shifted, mode, guard_rows, out);
}
int pb_op_gm_match_flow(pb_ctx *c, const float *O, int B, int h8, int w8, int guard_rows, float *flow, void *vt) {
    PB_CHECK(c && O && flow && vt && B > 0 && guard_rows >= 0, PB_ERR_ARG, "op_gm_match_flow: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.match_flow(O, B, guard_rows, flow, vt);
}
int pb_op_gm_upsampler_in(pb_ctx *c, const float *O, const float *X, int B, int images, int P, int img_step, int guard_rows, float *flow, void *map) {
    PB_CHECK(c && O && X && flow && map && B > 0 && P > 0 && (img_step == 1 || img_step == 2) && (B - 1) * img_step < images && guard_rows >= 0,
             PB_ERR_ARG, "op_gm_upsampler_in: bad arguments");
    GM_OP_ENGINE(e);
    return e.upsampler_in(O, X, B, images, P, img_step, guard_rows, flow, map);
}
int pb_op_attention128_cfg(pb_ctx *c, const float *q, const float *k, const float *v, const int8_t *region, int nreg, float *o, int B, int L,
                           int split, int pv_single, int vcols, int v_shared, int kxor, int ldq, int strided, float fill) {
    PB_CHECK(c && q && v && o && B > 0 && L > 0 && (vcols == 128 || vcols == 32) && (ldq == 256 || (ldq == 128 && !split)) && strided >= 0 &&
                 strided <= 2 && (k || strided == 1) && (strided != 1 || (kxor == 1 && B % 2 == 0)) && (!region || nreg > 0),
             PB_ERR_ARG, "op_attention128_cfg: bad arguments");
    GM_OP_ENGINE(e);
    return e.attention_cfg(q, k, v, region, nreg, o, B, L, split, pv_single, vcols, v_shared, kxor, ldq, strided, fill);
}
int pb_op_gm_window_block(pb_ctx *c, const float *Y, float *X, const float *gamma, const float *beta, int images, int h8, int w8, int shifted,
                          int cross, int split) {
    PB_CHECK(c && Y && X && gamma && beta && images > 0 && (!cross || images % 2 == 0), PB_ERR_ARG, "op_gm_window_block: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.window_block(Y, X, gamma, beta, images, shifted, cross, split);
}
int pb_op_gm_match(pb_ctx *c, const float *tokens, int NP, int h8, int w8, int dirs, int split, float *flow) {
    PB_CHECK(c && tokens && flow && NP > 0 && (dirs == 1 || dirs == 2), PB_ERR_ARG, "op_gm_match: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.match(tokens, NP, dirs, split, flow);
}
int pb_op_gm_propagate(pb_ctx *c, const float *q, const float *k, const float *flow_in, const float *X, int NP, int h8, int w8, int dirs, int split,
                       int guard_rows, float *flow_match, float *flow_prop, void *map) {
    PB_CHECK(c && q && k && flow_in && X && flow_match && flow_prop && map && NP > 0 && (dirs == 1 || dirs == 2) && guard_rows >= 0, PB_ERR_ARG,
             "op_gm_propagate: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.propagate(q, k, flow_in, X, NP, dirs, split, guard_rows, flow_match, flow_prop, map);
}
int pb_op_gm_local_match(pb_ctx *c, const float *tokens, int NP, int h8, int w8, int dirs, int radius, int guard_rows, float *flow) {
    PB_CHECK(c && tokens && flow && NP > 0 && (dirs == 1 || dirs == 2) && guard_rows >= 0, PB_ERR_ARG, "op_gm_local_match: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.local_match(tokens, NP, dirs, radius, guard_rows, flow);
}
int pb_op_gm_local_propagate(pb_ctx *c, const float *q, const float *k, const float *flow_in, int B, int h8, int w8, int img_step, int radius,
                             int guard_rows, float *flow_out) {
    PB_CHECK(c && q && k && flow_in && flow_out && B > 0 && (img_step == 1 || img_step == 2) && guard_rows >= 0, PB_ERR_ARG,
             "op_gm_local_propagate: bad arguments");
    GM_OP_ENGINE(e);
    PB_TRY(e.geom(h8, w8));
    return e.local_propagate(q, k, flow_in, B, img_step, radius, guard_rows, flow_out);
}

// ---- the mask_mmdet band's kernels one by one (MaskOpEngine above) ----
#define MASK_OP_ENGINE(e) PB_HIP(hipSetDevice(c->device)); MaskOpEngine e(c->device); PB_TRY(e.setup(nullptr, 0, SL_F16, 0))
int pb_op_mask_prep(pb_ctx *c, const uint8_t *frames, int n, int H, int W, int nh, int nw, int Hp, int Wp, const int *xt, const int *yt, int split,
                    int guard_rows, void *out, float *chw) {
    PB_CHECK(c && frames && xt && yt && out && chw && n > 0 && H > 0 && W > 0 && nh > 0 && nw > 0 && nh <= Hp && nw <= Wp && Hp % 4 == 0 && Wp % 4 == 0 &&
                 guard_rows >= 0, PB_ERR_ARG, "op_mask_prep: bad arguments");
    for (int i = 0; i < nw; ++i) PB_CHECK(xt[i * 4] >= 0 && xt[i * 4] < W && xt[i * 4 + 1] >= 0 && xt[i * 4 + 1] < W, PB_ERR_ARG, "op_mask_prep: column table entry %d outside the frame", i);
    for (int i = 0; i < nh; ++i) PB_CHECK(yt[i * 4] >= 0 && yt[i * 4] < H && yt[i * 4 + 1] >= 0 && yt[i * 4 + 1] < H, PB_ERR_ARG, "op_mask_prep: row table entry %d outside the frame", i);
    MASK_OP_ENGINE(e);
    return e.prep(frames, n, H, W, nh, nw, Hp, Wp, xt, yt, split, guard_rows, out, chw);
}
int pb_op_mask_maxpool(pb_ctx *c, const float *x, int n, int H, int W, int C, int split, int guard_rows, void *out) {
    PB_CHECK(c && x && out && n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && guard_rows >= 0, PB_ERR_ARG, "op_mask_maxpool: bad arguments");
    MASK_OP_ENGINE(e);
    return e.maxpool(x, n, H, W, C, split, guard_rows, out);
}
int pb_op_mask_nearest_add(pb_ctx *c, const float *dst, const float *src, int n, int h, int w, int sh, int sw, int C, int split, int guard_rows, void *out) {
    PB_CHECK(c && dst && src && out && n > 0 && h > 0 && w > 0 && sh > 0 && sw > 0 && C > 0 && C % 8 == 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_mask_nearest_add: bad arguments");
    MASK_OP_ENGINE(e);
    return e.nearest_add(dst, src, n, h, w, sh, sw, C, split, guard_rows, out);
}
int pb_op_mask_subsample2(pb_ctx *c, const float *x, int n, int H, int W, int C, int split, int guard_rows, void *out) {
    PB_CHECK(c && x && out && n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && guard_rows >= 0, PB_ERR_ARG, "op_mask_subsample2: bad arguments");
    MASK_OP_ENGINE(e);
    return e.subsample2(x, n, H, W, C, split, guard_rows, out);
}
int pb_op_mask_coord_concat(pb_ctx *c, const float *x, int n, int h, int w, int C, int ldi, int split, int guard_rows, void *out) {
    PB_CHECK(c && x && out && n > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0 && ldi % 8 == 0 && ldi >= C * (1 + (split ? 1 : 0)) && guard_rows >= 0, PB_ERR_ARG,
             "op_mask_coord_concat: bad arguments");
    MASK_OP_ENGINE(e);
    return e.coord_concat(x, n, h, w, C, ldi, split, guard_rows, out);
}
int pb_op_mask_bilinear(pb_ctx *c, const float *x, const float *y0, int n, int H, int W, int OH, int OW, int C, int ldi, int ldo, int split, int guard_rows,
                        void *out) {
    PB_CHECK(c && x && out && n > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && C > 0 && C % 8 == 0 && ldi % 8 == 0 && ldo % 8 == 0 &&
                 ldi >= C * (1 + (split ? 1 : 0)) && ldo >= C * (1 + (split ? 1 : 0)) && guard_rows >= 0, PB_ERR_ARG, "op_mask_bilinear: bad arguments");
    MASK_OP_ENGINE(e);
    return e.bilinear(x, y0, n, H, W, OH, OW, C, ldi, ldo, split, guard_rows, out);
}
int pb_op_mask_gn_relu(pb_ctx *c, const float *x, const float *gamma, const float *beta, int n, int HW, int C, int layout, int guard_rows, void *out,
                       float *aff) {
    PB_CHECK(c && x && gamma && beta && out && aff && n > 0 && HW > 0 && C > 0 && C % 32 == 0 && layout >= 0 && layout <= 2 && guard_rows >= 0, PB_ERR_ARG,
             "op_mask_gn_relu: bad arguments");
    MASK_OP_ENGINE(e);
    return e.gn_relu(x, gamma, beta, n, HW, C, layout, guard_rows, out, aff);
}
int pb_op_mask_cls_points_nms(pb_ctx *c, const float *logit, int n, int pts_total, int off, int g, int C, int guard_rows, float *score) {
    PB_CHECK(c && logit && score && n > 0 && g > 0 && C > 0 && off >= 0 && off + g * g <= pts_total && guard_rows >= 0, PB_ERR_ARG,
             "op_mask_cls_points_nms: bad arguments");
    MASK_OP_ENGINE(e);
    return e.cls_points_nms(logit, n, pts_total, off, g, C, guard_rows, score);
}
int pb_op_mask_gather_rows(pb_ctx *c, const float *src, int src_rows, const int *idx, int count, int rows_pad, int cols, int split, int guard_rows,
                           void *out) {
    PB_CHECK(c && src && idx && out && src_rows > 0 && count >= 0 && count <= rows_pad && cols > 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_mask_gather_rows: bad arguments");
    for (int i = 0; i < count; ++i) PB_CHECK(idx[i] >= 0 && idx[i] < src_rows, PB_ERR_ARG, "op_mask_gather_rows: idx[%d] = %d of %d rows", i, idx[i], src_rows);
    MASK_OP_ENGINE(e);
    return e.gather_rows(src, src_rows, idx, count, rows_pad, cols, split, guard_rows, out);
}
int pb_op_mask_stats(pb_ctx *c, const float *logit, int rows, int HW, int ld, float thr, int guard_rows, float *out) {
    PB_CHECK(c && logit && out && rows > 0 && HW > 0 && ld >= HW && guard_rows >= 0, PB_ERR_ARG, "op_mask_stats: bad arguments");
    MASK_OP_ENGINE(e);
    return e.mask_stats(logit, rows, HW, ld, thr, guard_rows, out);
}
int pb_op_mask_intersections(pb_ctx *c, const float *logit, int src_rows, int ld, const int *idx, int n, int HW, float thr, int guard_rows, void *bits,
                             int inter_rows, float *inter) {
    PB_CHECK(c && logit && idx && bits && inter && src_rows > 0 && n > 0 && n <= 512 && HW > 0 && HW % 64 == 0 && ld >= HW && inter_rows >= n &&
                 guard_rows >= 0, PB_ERR_ARG, "op_mask_intersections: bad arguments");
    for (int i = 0; i < n; ++i) PB_CHECK(idx[i] >= 0 && idx[i] < src_rows, PB_ERR_ARG, "op_mask_intersections: idx[%d] = %d of %d rows", i, idx[i], src_rows);
    MASK_OP_ENGINE(e);
    return e.intersections(logit, src_rows, ld, idx, n, HW, thr, guard_rows, bits, inter_rows, inter);
}
int pb_op_mask_matrix_nms(pb_ctx *c, const float *inter, const float *area, const int *label, const float *score, int n, float sigma, int guard,
                          float *comp, float *out) {
    PB_CHECK(c && inter && area && label && score && comp && out && n > 0 && n <= 512 && guard >= 0, PB_ERR_ARG, "op_mask_matrix_nms: bad arguments");
    MASK_OP_ENGINE(e);
    return e.matrix_nms(inter, area, label, score, n, sigma, guard, comp, out);
}
int pb_op_mask_sigmoid_rows(pb_ctx *c, const float *logit, int src_rows, int ld, const int *idx, int count, int HW, int guard_rows, float *sig) {
    PB_CHECK(c && logit && idx && sig && src_rows > 0 && count > 0 && HW > 0 && HW % 4 == 0 && ld % 4 == 0 && ld >= HW && guard_rows >= 0, PB_ERR_ARG,
             "op_mask_sigmoid_rows: bad arguments");
    for (int i = 0; i < count; ++i) PB_CHECK(idx[i] >= 0 && idx[i] < src_rows, PB_ERR_ARG, "op_mask_sigmoid_rows: idx[%d] = %d of %d rows", i, idx[i], src_rows);
    MASK_OP_ENGINE(e);
    return e.sigmoid_rows(logit, src_rows, ld, idx, count, HW, guard_rows, sig);
}
int pb_op_mask_dynconv(pb_ctx *c, const float *kernels, int src_rows, const int *idx, int row_off, int M, const float *feat, int HW4, int split,
                       int guard_rows, float *out) {
    PB_CHECK(c && kernels && idx && feat && out && src_rows > 0 && row_off >= 0 && row_off % 8 == 0 && M > 0 && HW4 > 0 && HW4 % 8 == 0 && guard_rows >= 0,
             PB_ERR_ARG, "op_mask_dynconv: bad arguments");
    for (int i = 0; i < row_off + M; ++i) PB_CHECK(idx[i] >= 0 && idx[i] < src_rows, PB_ERR_ARG, "op_mask_dynconv: idx[%d] = %d of %d rows", i, idx[i], src_rows);
    MASK_OP_ENGINE(e);
    return e.dynconv(kernels, src_rows, idx, row_off, M, feat, HW4, split, guard_rows, out);
}
int pb_op_mask_band_accumulate(pb_ctx *c, const float *sig, const uint8_t *use, int k, int fh, int fw, int h, int w, int H, int W, float thr, int guard,
                               uint8_t *out, uint8_t *inst) {
    PB_CHECK(c && sig && use && out && k > 0 && fh > 0 && fw > 0 && h > 0 && w > 0 && h <= 4 * fh && w <= 4 * fw && H > 0 && W > 0 && guard >= 0, PB_ERR_ARG,
             "op_mask_band_accumulate: bad arguments");
    MASK_OP_ENGINE(e);
    return e.band_accumulate(sig, use, k, fh, fw, h, w, H, W, thr, guard, out, inst);
}

// ---- the depth bands' kernels one by one (DepthOpEngine above) ----
#define DEPTH_OP_ENGINE(e) PB_HIP(hipSetDevice(c->device)); DepthOpEngine e(c->device); PB_TRY(e.setup(nullptr, 0, SL_F16, 0))
int pb_op_depth_layernorm(pb_ctx *c, const float *x, const float *g, const float *b, int B, int ntp, int ntok, int D, int drop_cls, int ldy, int lo_off,
                          int o8_off, float o8_scale, int lo8, int guard_rows, void *out, int *lo8_pa) {
    PB_CHECK(c && x && g && b && out && B > 0 && ntok > (drop_cls ? 1 : 0) && ntok <= ntp && D > 0 && D % 4 == 0 && D <= 1024 && ldy >= D && ldy % 4 == 0 &&
                 guard_rows >= 0, PB_ERR_ARG, "op_depth_layernorm: bad arguments");
    // every part of a row the kernel stores must lie inside the row: lo at half lo_off, hi8 / lo8 at bytes 2 lo_off / 3 lo_off, the fp8 copy at byte o8_off
    PB_CHECK(lo_off == 0 || (lo_off >= D && lo_off % 4 == 0 && (lo8 ? 3 * lo_off + D <= 2 * ldy : lo_off + D <= ldy)), PB_ERR_ARG,
             "op_depth_layernorm: residual part at %d outside a row of %d halfs", lo_off, ldy);
    PB_CHECK(!lo8 || lo_off, PB_ERR_ARG, "op_depth_layernorm: e4m3 residual parts need lo_off");
    PB_CHECK(o8_off == 0 || (o8_off >= 2 * D && o8_off % 4 == 0 && o8_off + D <= 2 * ldy && !lo_off), PB_ERR_ARG,
             "op_depth_layernorm: fp8 copy at byte %d outside a row of %d halfs", o8_off, ldy);
    DEPTH_OP_ENGINE(e);
    if (lo8_pa) *lo8_pa = e.lo8_pa();
    return e.layernorm(x, g, b, B, ntp, ntok, D, drop_cls, ldy, lo_off, o8_off, o8_scale, lo8, guard_rows, out);
}
int pb_op_depth_attention(pb_ctx *c, const float *q, const float *k, const float *v, int B, int heads, int N, int variant, int ldo, int o8_off,
                          float o8_scale, int guard_rows, void *out) {
    PB_CHECK(c && q && k && v && out && B > 0 && heads > 0 && N > 0 && (variant == 1 || variant == 2) && ldo >= heads * 64 && ldo % 8 == 0 && guard_rows >= 0,
             PB_ERR_ARG, "op_depth_attention: bad arguments (variant 1: 8 waves, 2: 4 waves)");
    PB_CHECK(o8_off == 0 || (o8_off >= heads * 128 && o8_off % 4 == 0 && o8_off + heads * 64 <= 2 * ldo), PB_ERR_ARG,
             "op_depth_attention: fp8 copy at byte %d outside a row of %d halfs", o8_off, ldo);
    DEPTH_OP_ENGINE(e);
    return e.attention(q, k, v, B, heads, N, variant, ldo, o8_off, o8_scale, guard_rows, out);
}
int pb_op_depth_preprocess(pb_ctx *c, const uint8_t *frames, int n, int H, int W, int mode, int net_h, int net_w, int guard_rows, float *chw, void *patch_raw) {
    PB_CHECK(c && frames && chw && patch_raw && n > 0 && H > 0 && W > 0 && (mode == 0 || mode == 1) && guard_rows >= 0, PB_ERR_ARG,
             "op_depth_preprocess: bad arguments (mode 0: the relative band's cubic table, 1: the metric band's align-corners table)");
    int nh = 392, nw = 518;
    if (mode == 0) PB_TRY(pb_depth_net_size(H, W, &nh, &nw));
    PB_CHECK(nh == net_h && nw == net_w, PB_ERR_ARG, "op_depth_preprocess: net size is %dx%d, caller passed %dx%d", nh, nw, net_h, net_w);
    PB_CHECK((int64_t)n * H * W * 3 < (1LL << 31) && (int64_t)n * 3 * nh * nw < (1LL << 31), PB_ERR_ARG, "op_depth_preprocess: %d frames of %dx%d are too many for one launch",
             n, H, W);
    DEPTH_OP_ENGINE(e);
    return e.preprocess(frames, n, H, W, mode, nh, nw, guard_rows, chw, patch_raw);
}
int pb_op_depth_cls_rows(pb_ctx *c, const float *cls, const float *pos, int B, int ntp, int D, int guard_rows, float *out) {
    PB_CHECK(c && cls && pos && out && B > 0 && ntp > 0 && D > 0 && guard_rows >= 0, PB_ERR_ARG, "op_depth_cls_rows: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.cls_rows(cls, pos, B, ntp, D, guard_rows, out);
}
int pb_op_depth_dpt_tail(pb_ctx *c, const float *z, const float *bias, const float *w2, float b2, int B, int H, int W, int OH, int OW, int layout,
                         int ldz, int guard, float *out, int *lo8_pa) {
    PB_CHECK(c && z && bias && w2 && out && B > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && layout >= 0 && layout <= 2 && ldz % 8 == 0 &&
                 ldz >= (layout ? 640 : 320) && guard >= 0, PB_ERR_ARG, "op_depth_dpt_tail: bad arguments (a pixel is 320 halfs per part)");
    DEPTH_OP_ENGINE(e);
    if (lo8_pa) *lo8_pa = e.lo8_pa();
    return e.dpt_tail(z, bias, w2, b2, B, H, W, OH, OW, layout, ldz, guard, out);
}
int pb_op_depth_resize_minmax(pb_ctx *c, const float *net, int B, int nh, int nw, int H, int W, int guard, float *out, float *mnmx) {
    PB_CHECK(c && net && out && mnmx && B > 0 && nh > 0 && nw > 0 && H > 0 && W > 0 && guard >= 0, PB_ERR_ARG, "op_depth_resize_minmax: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.resize_minmax(net, B, nh, nw, H, W, guard, out, mnmx);
}
int pb_op_zoe_softplus(pb_ctx *c, float *x, int rows, int cols, int ld, int guard_rows) {
    PB_CHECK(c && x && rows > 0 && cols > 0 && ld >= cols && guard_rows >= 0, PB_ERR_ARG, "op_zoe_softplus: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.softplus(x, rows, cols, ld, guard_rows);
}
int pb_op_zoe_dot32_relu(pb_ctx *c, const float *act, int ld, const float *w2, float b2, int rows, int guard, float *out) {
    PB_CHECK(c && act && w2 && out && rows > 0 && ld >= 32 && ld % 8 == 0 && guard >= 0, PB_ERR_ARG, "op_zoe_dot32_relu: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.dot32_relu(act, ld, w2, b2, rows, guard, out);
}
int pb_op_zoe_bilerp_add(pb_ctx *c, const float *a, const float *src, int n, int h, int w, int H, int W, int C, int lda, int lds, int ldo, int guard_rows,
                         void *out) {
    PB_CHECK(c && a && src && out && n > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && lda >= C && lds >= C && ldo >= C && lda % 8 == 0 &&
                 lds % 8 == 0 && ldo % 8 == 0 && guard_rows >= 0, PB_ERR_ARG, "op_zoe_bilerp_add: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.bilerp_add(a, src, n, h, w, H, W, C, lda, lds, ldo, guard_rows, out);
}
int pb_op_zoe_attractor(pb_ctx *c, const float *A, int ldA, int nA, const float *bprev, int n, int h, int w, int H, int W, float alpha, int guard_rows,
                        float *out) {
    PB_CHECK(c && A && bprev && out && nA > 0 && nA <= ldA && n > 0 && h > 0 && w > 0 && H > 0 && W > 0 && guard_rows >= 0, PB_ERR_ARG,
             "op_zoe_attractor: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.attractor(A, ldA, nA, bprev, n, h, w, H, W, alpha, guard_rows, out);
}
int pb_op_zoe_cat(pb_ctx *c, const float *act, int ld_act, const float *rel, const float *emb, int ld_emb, int n, int h, int w, int H, int W, int guard_rows,
                  void *out) {
    PB_CHECK(c && act && rel && emb && out && ld_act >= 32 && ld_act % 8 == 0 && ld_emb >= 128 && n > 0 && h > 0 && w > 0 && H > 0 && W > 0 && guard_rows >= 0,
             PB_ERR_ARG, "op_zoe_cat: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.cat(act, ld_act, rel, emb, ld_emb, n, h, w, H, W, guard_rows, out);
}
int pb_op_zoe_logbinom_depth(pb_ctx *c, const float *pt, int ld_pt, const float *bins, int n, int h, int w, int H, int W, float min_temp, float max_temp,
                             int guard, float *out) {
    PB_CHECK(c && pt && bins && out && ld_pt >= 4 && n > 0 && h > 0 && w > 0 && H > 0 && W > 0 && guard >= 0, PB_ERR_ARG, "op_zoe_logbinom_depth: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.logbinom(pt, ld_pt, bins, n, h, w, H, W, min_temp, max_temp, guard, out);
}
int pb_op_zoe_pil_resize(pb_ctx *c, const float *in, int n, int h, int w, int H, int W, int guard, float *out) {
    PB_CHECK(c && in && out && n > 0 && h > 0 && w > 0 && H > 0 && W > 0 && guard >= 0, PB_ERR_ARG, "op_zoe_pil_resize: bad arguments");
    DEPTH_OP_ENGINE(e);
    return e.pil_resize(in, n, h, w, H, W, guard, out);
}

}  // extern "C"
