#include "engine_base.h"
#include "conv_walk.h"      // cw3_tiles16 / cw3_tiles8: the packed-channel K axis the kernels walk

#include <math.h>
#include <string.h>

#include <algorithm>

namespace {
const char *const kFam[] = {"gemm_f16", "conv_igemm_f16", "attention", "layernorm", "elementwise", "prepost", "conv_igemm_f16_tile128",
                      "conv_igemm_f16_tile256x64"};
inline int cp64(int c) { return (int)round_up(c, 64); }
}  // namespace

hipEvent_t KernelTimer::get() {
    if (used == pool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        pool.push_back(e);
    }
    return pool[used++];
}
KernelTimer::~KernelTimer() {
    for (auto e : pool) hipEventDestroy(e);
}

int KernelTimer::collect(const char *const *fam_names, int nfam, pb_kernel_stat *out, int cap) {
    std::vector<pb_kernel_stat> acc;
    auto slot = [&](const char *name) -> pb_kernel_stat & {
        for (auto &a : acc)
            if (a.name == name || !strcmp(a.name, name)) return a;
        acc.push_back(pb_kernel_stat{name, 0, 0, 0, 0, 0});
        return acc.back();
    };
    for (auto &r : recs) {
        float ms = 0;
        hipEventElapsedTime(&ms, r.a, r.b);
        pb_kernel_stat &a = slot(r.name && r.name[0] ? r.name : fam_names[r.fam < nfam ? r.fam : 0]);
        a.ms += ms; a.flops += r.flops; a.exec_flops += r.exec; a.bytes += r.bytes; a.launches++;
    }
    int n = 0;
    for (auto &a : acc)
        if (n < cap) out[n++] = a;
    return n;
}

EngineBase::EngineBase(int device, const CreateEnv &env, const char *const *fam_names) : env(env), device(device), fam_names_(fam_names ? fam_names : kFam) {}

EngineBase::~EngineBase() {
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    snaps_.clear();
    for (auto p : owned_) hipFree(p);
    if (arena_) hipFree(arena_);
    if (stream) hipStreamDestroy(stream);
}

size_t EngineBase::tic(int fam, double flops, double bytes, double passes) {
    KernelTimer::Rec r{fam, timer.get(), timer.get(), flops, bytes, flops * passes, nullptr};
    hipEventRecord(r.a, cur_);
    timer.recs.push_back(r);
    return timer.recs.size() - 1;
}
void EngineBase::toc(size_t rec) { hipEventRecord(timer.recs[rec].b, cur_); }

int EngineBase::stats(pb_kernel_stat *out, int cap) {
    if (hipStreamSynchronize(stream) != hipSuccess) return -2;
    return timer.collect(fam_names_, F_COUNT, out, cap);
}

int EngineBase::snapshot(const std::string &name, const void *src, size_t bytes, Stage as) {
    DevMem &buf = snaps_[name];
    int r = buf.reserve(bytes);
    if (r) return r;
    PB_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyDeviceToDevice, stream));
    as.ptr = buf.p;
    stages_[name] = as;
    return 0;
}

int64_t EngineBase::get_stage(const char *name, float *out, int64_t cap, int64_t shape[4]) {
    auto it = stages_.find(name);
    PB_CHECK(it != stages_.end(), PB_ERR_ARG, "unknown stage '%s'", name);
    const Stage &s = it->second;
    const bool rows = s.kind == Stage::F32_ROWS || s.kind == Stage::F16_ROWS;
    const int64_t plane = s.h * s.w, total = s.n * s.c * plane;
    shape[0] = s.n; shape[1] = rows ? s.h : s.c; shape[2] = rows ? s.w : s.h; shape[3] = rows ? 1 : s.w;
    PB_CHECK(total <= cap, PB_ERR_ARG, "stage buffer too small (%lld > %lld)", (long long)total, (long long)cap);
    PB_HIP(hipStreamSynchronize(stream));
    DevMem tmp;                         // fp32 copy of an fp16 stage
    int r;
    auto fetch = [&](float *dst) -> int {
        PB_HIP(hipStreamSynchronize(stream));
        PB_HIP(hipMemcpy(dst, tmp.p, (size_t)total * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    switch (s.kind) {
    case Stage::F32_ROWS:
        if (s.bstride == plane) {
            PB_HIP(hipMemcpy(out, s.ptr, (size_t)total * 4, hipMemcpyDeviceToHost));
        } else {
            for (int64_t b = 0; b < s.n; ++b)
                PB_HIP(hipMemcpy(out + b * plane, (const float *)s.ptr + b * s.bstride, (size_t)plane * 4, hipMemcpyDeviceToHost));
        }
        break;
    case Stage::F32_NCHW:
        PB_HIP(hipMemcpy(out, s.ptr, (size_t)total * 4, hipMemcpyDeviceToHost));
        break;
    case Stage::F16_ROWS:
        if ((r = tmp.reserve((size_t)total * 4))) return r;
        if ((r = launch_f16_to_f32(stream, (const f16 *)s.ptr, tmp.as<float>(), s.n * s.h, (int)s.w, (int)s.ld))) return r;
        if ((r = fetch(out))) return r;
        break;
    case Stage::F16_NHWC:
        if ((r = tmp.reserve((size_t)total * 4))) return r;
        if ((r = launch_nhwc_f16_to_nchw_f32(stream, (const f16 *)s.ptr, tmp.as<float>(), (int)s.n, (int)s.c, (int)s.h, (int)s.w, (int)s.ld))) return r;
        if ((r = fetch(out))) return r;
        if (s.lo_off) {                 // split map: hi + lo in fp32
            std::vector<float> lo_part((size_t)total);
            if ((r = launch_nhwc_f16_to_nchw_f32(stream, (const f16 *)s.ptr + s.lo_off, tmp.as<float>(), (int)s.n, (int)s.c, (int)s.h, (int)s.w, (int)s.ld))) return r;
            if ((r = fetch(lo_part.data()))) return r;
            for (int64_t i = 0; i < total; ++i) out[i] += lo_part[(size_t)i];
        }
        break;
    case Stage::F32_NHWC: {
        std::vector<float> px((size_t)(s.n * plane * s.ld));
        PB_HIP(hipMemcpy(px.data(), s.ptr, px.size() * 4, hipMemcpyDeviceToHost));
        for (int64_t b = 0; b < s.n; ++b)
            for (int64_t c = 0; c < s.c; ++c)
                for (int64_t p = 0; p < plane; ++p) out[(b * s.c + c) * plane + p] = px[(size_t)((b * plane + p) * s.ld + c)];
        break;
    }
    }
    return total;
}

int EngineBase::begin_load(const pb_tensor *w, int n, bool depth_stream) {
    PB_HIP(hipSetDevice(device));
    PB_HIP(pb_create_stream(&stream, depth_stream ? env.stream_depth : env.stream_flow));
    cur_ = stream;
    for (int i = 0; i < n; ++i) {
        PB_CHECK(w[i].data && w[i].name, PB_ERR_ARG, "weight %d: null", i);
        if (w[i].dtype == PB_F32) tmap_[w[i].name] = &w[i];      // integer buffers (num_batches_tracked) are not needed
    }
    void *z = nullptr;
    PB_HIP(hipMalloc(&z, 4096));
    PB_HIP(hipMemset(z, 0, 4096));
    owned_.push_back(z);
    zero_ = (f16 *)z;
    return 0;
}

const pb_tensor *EngineBase::find(const std::string &name) const {
    auto it = tmap_.find(name);
    return it == tmap_.end() ? nullptr : it->second;
}

int EngineBase::upload_f32(const float *src, size_t n, float **dst) {
    void *p = nullptr;
    PB_HIP(hipMalloc(&p, std::max<size_t>(n * 4, 256)));
    owned_.push_back(p);
    PB_HIP(hipMemcpy(p, src, n * 4, hipMemcpyHostToDevice));
    *dst = (float *)p;
    return 0;
}

int EngineBase::upload_rows(const std::vector<f16> &rows, f16 **dst) {
    void *p = nullptr;
    PB_HIP(hipMalloc(&p, rows.size() * 2));
    owned_.push_back(p);
    PB_HIP(hipMemcpy(p, rows.data(), rows.size() * 2, hipMemcpyHostToDevice));
    *dst = (f16 *)p;
    return 0;
}

int EngineBase::pack_spec(const float *src, int N, int K, int Kpad, PackedW &out, const float *bias, int taps, const PackSpec &spec) {
    const std::vector<f16> rows = pack_rows(src, N, K, Kpad, taps, spec, out);
    PB_CHECK(!rows.empty(), PB_ERR_ARG, "pack: N %d / K %d / Kpad %d / taps %d do not fit the layout (sa %d, sw %d, mx2 %d)", N, K, Kpad, taps, spec.sa,
             spec.sw, spec.mx2);
    int r = upload_rows(rows, &out.w);
    if (r) return r;
    out.bias = nullptr;
    if (bias) {
        const size_t Np = (size_t)round_up(N, 256);
        void *b = nullptr;
        PB_HIP(hipMalloc(&b, std::max<size_t>(Np * 4, 256)));
        owned_.push_back(b);
        PB_HIP(hipMemset(b, 0, Np * 4));
        PB_HIP(hipMemcpy(b, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        out.bias = (float *)b;
    }
    return 0;
}

int EngineBase::pack(const float *src, int N, int K, int Kpad, PackedW &out, const float *bias, int taps, int sa_req) {
    PackSpec s;
    // split_w_ (PB_PREC_SPLIT): every tap's channels are followed by the rounding residuals of the same weights, and the GEMM reads the
    // activations twice (gemm.h kwrap): a w_hi + a w_lo in one accumulator
    s.sw = split_w_ && Kpad % (64 * taps) == 0 && K % taps == 0;
    s.sa = s.sw && sa_req;
    s.mx = mx_;
    s.mx2 = !s.sa && s.sw && mx_ && pack_mx2_ && Kpad / taps % 128 == 0;
    s.tapin = pack_tapin_;
    return pack_spec(src, N, K, Kpad, out, bias, taps, s);
}

int EngineBase::fold_bn(const std::string &bn, int C, std::vector<float> &scale, std::vector<float> &shift) {
    const char *sfx[4] = {".weight", ".bias", ".running_mean", ".running_var"};
    const float *t[4];
    for (int i = 0; i < 4; ++i) {
        const pb_tensor *x = find(bn + sfx[i]);
        PB_CHECK(x && x->shape[0] == C, PB_ERR_ARG, "missing weight '%s%s' [%d]", bn.c_str(), sfx[i], C);
        t[i] = (const float *)x->data;
    }
    scale.resize(C); shift.resize(C);
    for (int c = 0; c < C; ++c) {
        const float s = t[0][c] / sqrtf(t[3][c] + 1e-5f);       // nn.BatchNorm2d eval, eps 1e-5
        scale[c] = s;
        shift[c] = t[1][c] - t[2][c] * s;
    }
    return 0;
}

int EngineBase::pack_conv(const std::string &name, bool has_bias, const float *scale, const float *shift, PackedW &out, int sa, int ci_pad) {
    const pb_tensor *t = find(name + ".weight");
    PB_CHECK(t && t->ndim == 4, PB_ERR_ARG, "missing conv '%s'", name.c_str());
    const float *b = nullptr;
    if (has_bias) {
        const pb_tensor *tb = find(name + ".bias");
        PB_CHECK(tb, PB_ERR_ARG, "missing bias of '%s'", name.c_str());
        b = (const float *)tb->data;
    }
    const int co = (int)t->shape[0], ci = (int)t->shape[1], kh = (int)t->shape[2], kw = (int)t->shape[3];
    const float *w = (const float *)t->data;
    const int cip = ci_pad ? ci_pad : cp64(ci), K = kh * kw * cip;
    PB_CHECK(cip >= ci && cip % 64 == 0, PB_ERR_ARG, "pack_conv '%s': %d input channels padded to %d", name.c_str(), ci, cip);
    const std::vector<float> g = pb_conv_rows(w, co, ci, kh * kw, cip, scale);
    std::vector<float> bb(co);
    for (int o = 0; o < co; ++o) bb[o] = (b ? b[o] : 0.f) * (scale ? scale[o] : 1.f) + (shift ? shift[o] : 0.f);
    int r = pack(g.data(), co, K, K, out, bb.data(), kh * kw, sa);
    out.Kreal = kh * kw * ci;
    if (r) return r;
    // RAFT's encoder stage 2: 96 -> 96 channels carried as 128.  The per-tap layout walks 9 x (2 + 2) K tiles of which a quarter multiply padding
    // channels; the packed-channel copy (conv_walk.h conv_cw3_word: 14 + 14 tiles) is what the 128 x 96 tile reads (PB_CW3=0: not built)
    if (launch_env().cw3 && out.mx3 && !out.tapin && kh * kw > 1 && ci % 16 == 0 && ci < cip && co > 64 && co <= 96) {
        const int taps = kh * kw, nk16 = cw3_tiles16(taps, ci), nk8 = cw3_tiles8(taps, ci), pw = out.mx_pw;
        const int64_t Kc = (int64_t)(nk16 + nk8) * 64, Np = round_up(co, 256);
        std::vector<f16> h((size_t)Np * Kc, (f16)0.f);
        for (int o = 0; o < co; ++o) {
            f16 *row = h.data() + (size_t)o * Kc;
            unsigned char *row8 = (unsigned char *)(row + (size_t)nk16 * 64);
            for (int tp = 0; tp < taps; ++tp)
                for (int c = 0; c < ci; ++c) {
                    const float v = g[(size_t)o * K + tp * cip + c];
                    const f16 hi = (f16)v;
                    row[tp * ci + c] = hi;                                      // fp16 chunks: tap-major, ci / 8 per tap
                    row8[(tp * 2 + 0) * ci + c] = pb_w_lo8(v, hi, pw);          // meets the map's hi8 chunks
                    row8[(tp * 2 + 1) * ci + c] = pb_w_hi8(hi, pw);             // ... and its lo8 chunks
                }
        }
        if ((r = upload_rows(h, &out.wcw))) return r;
        out.Kcw = (int)Kc; out.nk16cw = nk16; out.cwC = ci;
    }
    return 0;
}

void EngineBase::set_weights(GemmArgs &a, const PackedW &w, bool is_conv) const {
    a.W = w.w; a.K = w.K; a.bias = w.bias; a.zero = zero_;
    const bool tapin = is_conv && w.tapin;
    if (tapin) { a.cTapInner = 1; a.cKH = w.taps / a.cKW; }
    if (w.mx2) {                 // [a16 | a8] maps x [w_hi | w_lo8] weights: per tap Cseg / 64 fp16 tiles then Cseg / 128 fp8 tiles
        a.nk16 = w.nk16; a.mx_scale_a = 127 - kMx2Pa; a.mx_scale_b = 127 - w.mx_pw;
        if (is_conv) {
            const int c = a.cC;                   // channels of the slice; the caller set cLd and (conv()) a8_rel via kshift
            a.cC = c + c / 2;
            a.mx_period = a.cC / 64;
            if (tapin) { a.mx_period = 0; a.nk16 = w.nk16 * w.taps; }      // slice-major: every fp16 slice of all taps, then the fp8 slices
        }
        return;
    }
    if (w.mx3) {                 // [hi | hi8 | lo8] maps: per tap fp16 tiles then fp8 tiles (gemm.h mx_period)
        a.nk16 = w.nk16; a.mx_scale_a = 127 - kLo8Pa; a.mx_scale_b = 127 - w.mx_pw;
        if (is_conv) {
            if (!a.cLd) a.cLd = 2 * a.cC;
            a.cC = 2 * w.Cseg;
            a.mx_period = 2 * w.Cseg / 64;
            if (tapin) { a.mx_period = 0; a.nk16 = w.nk16 * w.taps; }
            if (w.wcw) { a.Wcw = w.wcw; a.Kcw = w.Kcw; a.nk16cw = w.nk16cw; a.cwC = w.cwC; a.cwPad = w.Cseg; a.cwTaps = w.taps; }
        }
        return;
    }
    // an fp16 weight with nk16 (every K tile an fp16 tile): the MX build of the kernel, for the fp8 copy its epilogue stores (PackedW::nk16)
    if (w.nk16) { a.nk16 = w.nk16; a.mx_scale_a = 127 - kMx2Pa; a.mx_scale_b = 127 - w.mx_pw; }
    if (!w.sa && !w.sw) return;
    // per tap [w_hi | w_hi (if sa) | w_lo (if sw)]: after the activation's parts the channel cursor wraps back onto the pixel's hi part
    if (is_conv) {
        if (!a.cLd) a.cLd = (1 + w.sa) * a.cC;
        a.kwrap = w.sw ? (1 + w.sa) * a.cC : 0;
        a.kshift = -a.kwrap;
        a.cC = (1 + w.sa + w.sw) * a.cC;
    } else {
        a.kwrap = w.sw ? (1 + w.sa) * w.Cseg / 64 : 0;
    }
}

void *EngineBase::carve(size_t bytes) {
    const size_t off = arena_off_;
    arena_off_ += round_up((int64_t)bytes, 256);
    return planning_ ? nullptr : (void *)(arena_ + off);
}

int EngineBase::plan_arena(const char *what, const std::function<int()> &carves) {
    for (int pass = 0; pass < 2; ++pass) {
        planning_ = pass == 0;
        arena_off_ = 0;
        int r = carves();
        if (!r && pass == 0) r = commit_arena(what);
        if (r) return r;
    }
    return 0;
}

int EngineBase::commit_arena(const char *what) {
    plan_bytes_ = arena_off_;
    if (arena_off_ > arena_bytes_) {
        if (arena_) PB_HIP(hipFree(arena_));
        arena_ = nullptr; arena_bytes_ = 0;
        hipError_t e = hipMalloc((void **)&arena_, arena_off_);
        PB_CHECK(e == hipSuccess, PB_ERR_MEMORY, "%s arena of %zu bytes: %s", what, arena_off_, hipGetErrorString(e));
        arena_bytes_ = arena_off_;
    }
    // stale bit patterns must never be read as fp16 NaN / Inf by padded tiles
    PB_HIP(hipMemsetAsync(arena_, 0, arena_bytes_, stream));
    return 0;
}

int EngineBase::conv(const f16 *in, int cC, int cLd, int n, int H, int W, int kh, int kw, int stride, const PackedW &w, f16 *out,
                     int ldo, int act, int pre_relu, const f16 *add1, const ConvFuse *fuse, int lo_off, int a8_rel, int o8_off) {
    GemmArgs a;
    a.A = in; a.N = w.N;
    a.cH = H; a.cW = W; a.cC = cC; a.cLd = cLd; a.cKW = kw; a.cStride = stride; a.cPad = kh / 2; a.cPadX = kw / 2;
    a.cOH = (H + 2 * (kh / 2) - kh) / stride + 1; a.cOW = (W + 2 * (kw / 2) - kw) / stride + 1;
    a.M = n * a.cOH * a.cOW;
    a.out = out; a.ldo = ldo; a.act = act; a.pre_relu = pre_relu; a.add1 = add1; a.lo_off = lo_off;
    if (lo_off && mx_) { a.lo8 = 1; a.lo8_pa = kLo8Pa; }
    if (fuse) { a.out2 = fuse->out2; a.gru_h = fuse->gru_h; a.gru_z = fuse->gru_z; a.gru_rh = fuse->gru_rh; a.gru_ld = fuse->gru_ld; a.add2 = fuse->add2; }
    if (w.mx2 && a8_rel && a8_rel != cC) { a.kwrap = cC; a.kshift = a8_rel - cC; }      // the fp8 copy of a channel slice is not adjacent
    if (o8_off) { a.o8_off = o8_off; a.o8_scale = (float)(1 << kMx2Pa); }
    a.sk_ws = sk_ws_; a.sk_cap = sk_cap_;
    PB_CHECK(!w.sw || w.Cseg == cC, PB_ERR_STATE, "split conv: %d channels, weights packed for %d", cC, w.Cseg);
    set_weights(a, w, true);
    PB_CHECK(w.K == kh * kw * a.cC, PB_ERR_STATE, "conv: packed K %d != %d*%d*%d", w.K, kh, kw, a.cC);
    // same predicate as launch_gemm's TILE_AUTO: the 256 x 256 ping-pong kernel needs N % 256 == 0 and >= 256 tiles
    const bool wide = conv_tile == TILE_256 || (conv_tile == TILE_AUTO && a.N % 256 == 0 && (int64_t)(a.M / 256) * (a.N / 256) >= 256);
    // algorithmic bytes: the input map once, the weights once, the output once (fp16)
    // one family per kernel symbol launch_gemm picks: 256 x 256 ping-pong, 256 x 64 (N <= 64), 128 x 128
    const double nr = w.Nreal ? w.Nreal : a.N;       // (padding rows of the weights are not the layer's work)
    return timed_gemm(wide ? F_CONV : (conv_tile == TILE_AUTO && a.N <= 64 ? F_CONV64 : F_CONV128), 2.0 * a.M * nr * w.Kreal,
                      2.0 * ((double)n * H * W * cC + nr * w.Kreal + (double)a.M * nr), [&] {
        // 64 -> 64 channels at half resolution: the halo-tiled direct kernel (halo_conv.hip) instead of the implicit GEMM
        return kh == 3 && kw == 3 && conv_tile == TILE_AUTO && conv3x3_c64_supported(a) ? launch_conv3x3_c64(cur_, a) : launch_gemm(cur_, A_CONV, EPI_STD, conv_tile, a);
    }, w.mx3 ? 2.0 : (w.mx2 ? 1.5 : 1.0 + w.sa + w.sw));
}

int EngineBase::dense(const f16 *A, int lda, int64_t M, const PackedW &w, f16 *out, int ldo, int act, const f16 *add1, int o8_off, int a_pa,
                      int lo_off) {
    GemmArgs a;
    a.A = A; a.lda = lda; a.N = w.N; a.M = (int)M;
    set_weights(a, w, false);
    a.out = out; a.ldo = ldo; a.act = act; a.add1 = add1; a.lo_off = lo_off;
    if (lo_off && mx_) { a.lo8 = 1; a.lo8_pa = kLo8Pa; }
    if (o8_off) { a.o8_off = o8_off; a.o8_scale = (float)(1 << kMx2Pa); }
    if (w.mx2 && a_pa >= 0) a.mx_scale_a = 127 - a_pa;
    a.sk_ws = sk_ws_; a.sk_cap = sk_cap_;
    return timed_gemm(F_GEMM, 2.0 * M * (double)a.N * w.Kreal, 2.0 * ((double)M * w.Kreal + (double)a.N * w.Kreal + (double)M * a.N),
                      [&] { return launch_gemm(cur_, A_DENSE, EPI_STD, dense_tile, a); }, w.mx3 ? 2.0 : (w.mx2 ? 1.5 : 1.0 + w.sa + w.sw));
}
