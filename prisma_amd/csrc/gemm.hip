// fp16 MFMA GEMM / implicit-GEMM convolution: argument checks, tile choice and dispatch to the kernel instantiations
// (gemm_kernels.h holds the kernels; gemm_i*.hip instantiate them, one group per translation unit).
#include "gemm.h"

#include <algorithm>

#include "launch_env.h"

int pb_gemm_dense_std_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_std_mx(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_resid_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_resid_mx(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_qkv_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_qkv_mx(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_pixshuf_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_pixshuf_mx(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_patch_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_dense_f32_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_conv_f32_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_conv_std_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_conv_std_mx(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_conv_pixshuf_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_conv_pixshuf_mx(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_conv_head_f16(hipStream_t s, int tile, const GemmArgs &a);
int pb_gemm_conv_head_mx(hipStream_t s, int tile, const GemmArgs &a);

static int clamp_n96(int mode) { return mode < 0 ? 0 : (mode > 2 ? 2 : mode); }
static std::atomic<int> &n96_mode() {            // starts from PB_TILE_N96 (default 2: gemm.h pb_gemm_set_n96)
    static std::atomic<int> v{clamp_n96(launch_env().tile_n96)};
    return v;
}
void pb_gemm_set_n96(int mode) { n96_mode().store(clamp_n96(mode), std::memory_order_relaxed); }
static thread_local const char *g_last_kernel = "";
const char *pb_gemm_last_kernel() { return g_last_kernel; }
void pb_gemm_set_last_kernel(const char *name) { g_last_kernel = name; }
static thread_local int g_last_splitk = 1;
int pb_gemm_last_splitk() { return g_last_splitk; }

static int cus_of(int dev) {
    static std::atomic<int> cus[64];              // 0: not asked yet
    if (dev < 0 || dev >= 64) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n <= 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

int pb_device_cus() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? cus_of(dev) : 256;
}

int pb_lds_limit(PbLdsLimit &done, const void *kernel, int bytes, int *cus) {
    int dev = 0;
    PB_HIP(hipGetDevice(&dev));
    if (cus) *cus = cus_of(dev);
    const uint64_t bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;            // a device id past 63 sets the attribute at every launch
    if (done.devices.load(std::memory_order_acquire) & bit) return 0;
    PB_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.devices.fetch_or(bit, std::memory_order_release);
    return 0;
}

int launch_gemm(hipStream_t stream, int amode, int epi, int tile, const GemmArgs &a_in) {
    GemmArgs a = a_in;
    const LaunchEnv &env = launch_env();
    const int n96 = n96_mode().load(std::memory_order_relaxed);
    PB_CHECK(a.K > 0 && a.K % 64 == 0, -1, "gemm: K=%d must be a positive multiple of 64", a.K);
    PB_CHECK(a.M > 0 && a.N > 0 && a.N % 8 == 0, -1, "gemm: bad M=%d N=%d", a.M, a.N);
    if (amode == A_CONV) PB_CHECK(a.cC % 64 == 0 && a.cLd % 8 == 0 && a.zero, -1, "conv: channels %d (x64) / pixel stride %d (x8)", a.cC, a.cLd);
    // gemm_kernel tests a tap against an 8 + 8 bit mask of the pixel (gemm_kernels.h tap_mask)
    if (amode == A_CONV) PB_CHECK(a.K / 64 <= 512 && a.kshift % 8 == 0 && (int64_t)8 * a.cW * (a.cLd ? a.cLd : a.cC) * 2 < (1LL << 30), -1,
                                  "conv: K walk table (K = %d, kshift = %d, row of %d pixels)", a.K, a.kshift, a.cW);
    if (amode == A_CONV) PB_CHECK(a.cKW >= 1 && a.cKW <= 8 && a.K / (a.cKW * a.cC) <= 8, -1, "conv: kernel %d x %d (up to 8 x 8)", a.K / (a.cKW * a.cC), a.cKW);
    {   // experiment switch: PB_GEMM_STAGGER=<percent> de-phases the CUs by that share of 1/8 tile period per step
        const int nk = a.K / 64;
        const int est = (3200 * nk + 24000) / 8 / 64;
        a.stagger = env.gemm_stagger > 0 ? est * env.gemm_stagger / 100 : 0;   // measured: no gain (0.97-1.0x), so off unless requested
    }
    if (epi == EPI_PIXSHUF) {
        // buffer-addressed pixel-shuffle epilogue (gemm_kernels.h pixshuf_epilogue_buf): at most TM <= 4 grid rows per wave tile, and the
        // window a wave addresses (128 rows x s pixels + 4 wraps of s (s - 1) ps_w pixels) well inside the 2 GB a resource spans
        const int64_t pbytes = a.ldo * 2, window = (int64_t)(128 * a.ps_s + 4 * a.ps_s * (a.ps_s - 1) * (int64_t)a.ps_w) * pbytes;
        a.ps_buf = env.pixshuf_buf && a.ps_w >= 32 && a.ps_co % 64 == 0 && window < (1LL << 30) ? 1 : 0;
    }
    if (tile == TILE_AUTO) {
        // 256x256 needs wide N and enough tiles to fill 256 CUs; the q/k/v split needs D % BN == 0
        // wide_need: the fewest 256 x 256 tiles a launch must have to take the ping-pong kernel, 256 = one per CU.  A one-frame
        // context (the caller lent a split-K workspace: gemm.h sk_ws) takes it from 128 tiles on: fc1 of a 720p frame (144 tiles) and the head's
        // full-resolution convolutions run one round of 256 x 256 tiles faster than 1.25 rounds of 128 x 128 ones (7.11 -> 6.93 ms per frame,
        // profiles/r06p_latency_knobs.txt; 100 - qkv as well - is slower again).  Same bits either way: every tile shape walks K in one order.
        const int wide_need = a.sk_ws ? 128 : 256;
        const bool wide = a.N % 256 == 0 && (int64_t)(a.M / 256) * (a.N / 256) >= wide_need;
        tile = wide && (epi != EPI_QKV || a.D % 256 == 0) ? TILE_256 : TILE_128;
        // N = 192 (RAFT's convc2): two 128-wide tiles of which the second is half empty, or one 256-wide tile that is a quarter empty - the
        // ping-pong kernel's K loop runs ~2460 cycles per 256 x 256 x 64 against the generic tile's ~1000 per 128 x 128 x 64.  Measured (r04p, one box):
        // flow band 147.4 -> 145.3 ms with N = 192 on the wide tile, 157.8 with N = 128 on it too.  PB_TILE_WIDE=<min columns of the last tile>, 0 = off
        const int wide_min = env.tile_wide;
        if (tile == TILE_128 && epi == EPI_STD && wide_min > 0 && a.N % 256 >= wide_min && (int64_t)(a.M / 256) * ((a.N + 255) / 256) >= 256) tile = TILE_256;
        // N <= 64 (RAFT / ResNet stems and first stages): a 128-wide tile spends half its MFMAs and B loads on padding columns
        if (tile == TILE_128 && epi == EPI_STD && a.N <= 64) tile = TILE_256x64;
        // (round 5 built a 384 x 128 ping-pong kernel for 64 < N <= 128 - K loop at 70 % of the matrix pipe against this tile's ~45 % - whose one
        // workgroup per CU exposed its set-up and epilogue: 35.5 against 34.6 ms on the bands' launches; under two-band overlap, round 6, +0.2 ... 0.8 %
        // of a step (profiles/r06b_overlap_n128.txt, r06c_bench_n128_line.json).  Not a gain worth 1300 lines and two translation units: removed.)
        // 64 < N <= 96 (RAFT / GMFlow encoder stage 2 carries 96 channels): the 128 x 96 tile - a quarter fewer MFMAs, B rows and fragment reads than
        // the 128-wide tile spends on 32 padding columns; its third column block has a plain single-column epilogue (gemm_kernels.h single_col_epilogue)
        // ... only when its chunk table holds the launch's K tiles (counted on the packed-channel K axis where that copy applies below): a deeper
        // layer (3 x 3 over 512 mx3 / 1024 fp16 channels: 144 K tiles) stays on the 128 x 128 tile instead of failing the check further down
        const int k96 = (a.Wcw && n96 >= 2 && !a.cTapInner ? a.Kcw : a.K) / 64;
        if (tile == TILE_128 && n96 && amode == A_CONV && epi == EPI_STD && a.N > 64 && a.N <= 96 && (a.act == ACT_NONE || a.act == ACT_RELU) && !a.out2 && !a.o8_off &&
            k96 <= 128)
            tile = TILE_128x96;
    }
    // split-K (gemm.h splitk): only the generic 128 x 128 tile, only when the caller lent a workspace, only launches that leave CUs idle
    a.splitk = 1;
    if (tile == TILE_128 && a.sk_ws && (epi == EPI_STD || epi == EPI_RESID)) {
        const int sk_max = env.splitk, ncu = pb_device_cus();          // largest factor; 0 / 1 = off
        const int64_t tiles = (int64_t)((a.M + 127) / 128) * ((a.N + 127) / 128);
        const int nk = a.K / 64;
        if (sk_max > 1 && tiles < ncu) {
            int S = (int)std::min<int64_t>(sk_max, 2 * (int64_t)ncu / tiles);      // two workgroups of this tile fit a CU
            S = std::min(S, nk / 8);                                              // a slice keeps >= 8 K tiles: its prologue / reduction must stay small beside it
            while (S > 1 && (int64_t)S * tiles * 128 * 128 > a.sk_cap) --S;
            if (S > 1) a.splitk = S;
        }
    }
    g_last_splitk = a.splitk;
    if (tile == TILE_128x96 && a.Wcw && n96 >= 2 && !a.cTapInner) {        // packed-channel K axis (gemm.h Wcw)
        a.W = a.Wcw; a.K = a.Kcw; a.nk16 = a.nk16cw; a.mx_period = 0; a.kwrap = 0; a.kshift = 0; a.cwalk = 1;
    }
    if (tile == TILE_128x96) PB_CHECK(a.K / 64 <= 128, -1, "conv: the 128 x 96 tile's chunk table holds 128 K tiles (K = %d)", a.K);
    if (tile == TILE_128x96)
        PB_CHECK(amode == A_CONV && epi == EPI_STD && a.N <= 96 && (a.act == ACT_NONE || a.act == ACT_RELU) && !a.out2 && !a.o8_off, -1,
                 "gemm: the 128 x 96 tile serves convolutions with N <= 96, a linear / ReLU output and no copies (N = %d, act %d)", a.N, a.act);
    if (epi == EPI_RESID) PB_CHECK(a.resid && (int64_t)a.M * a.ldr * 4 < (1LL << 32) - (1 << 20), -1, "residual epilogue: the stream (%d rows) must fit a 32-bit buffer resource", a.M);
    if (epi == EPI_QKV) PB_CHECK(a.D % (tile == TILE_128 ? 128 : 256) == 0 && a.ntp % 8 == 0, -1, "qkv epilogue: D=%d ntp=%d", a.D, a.ntp);
    {   // PB_EPI_REPORT=1 (diagnostic): EPI_STD launches whose activation / skip / copy combination is not one of the
        // straight-line epilogue copies (gemm_kernels.h direct_epilogue_any PB_FAST_CASE list; tests/test_build_checks_cpu.py holds the two
        // lists against each other) take the run-time switched pass loop at ~2x the epilogue cost: name them, once per combination
        if (env.epi_report && epi == EPI_STD) {
            static const int fast_keys[] = {ACT_NONE, ACT_RELU, ACT_GELU, ACT_GRU_ZR, ACT_GRU_Q, ACT_NONE | 64, ACT_NONE | 16, ACT_NONE | 16 | 32 | 64,
                                            ACT_GRU_ZR | 16 | 32, ACT_GRU_Q | 16 | 32, ACT_RELU | 16 | 128, ACT_RELU | 64, ACT_RELU | 16};
            const int key = a.act | (a.add1 ? 16 : 0) | (a.add2 ? 32 : 0) | (a.out2 ? 64 : 0) | (a.pre_relu ? 128 : 0);
            bool hit = false;
            for (int k : fast_keys) hit |= k == key;
            static std::atomic<unsigned long long> seen[8];
            // fetch_or: of the threads that meet at a combination's first launch, the one that sets the bit reports it
            if (!hit && !(seen[key >> 6 & 7].fetch_or(1ull << (key & 63), std::memory_order_relaxed) >> (key & 63) & 1)) {
                fprintf(stderr, "[pb_epi_report] EPI_STD launch outside the fast-epilogue list: key %d (act %d%s%s%s%s), first seen at M = %d, N = %d, K = %d, %s\n", key,
                        a.act, a.add1 ? " + add1" : "", a.add2 ? " + add2" : "", a.out2 ? " + out2" : "", a.pre_relu ? " + pre_relu" : "", a.M, a.N, a.K,
                        amode == A_CONV ? "conv" : "dense");
            }
        }
    }
    const bool mx = a.nk16 > 0;
    // MX builds write / read split maps with e4m3 residual parts, fp16-only builds with fp16 residual parts
    PB_CHECK(!a.lo_off || (a.lo8 != 0) == mx, -1, "gemm: split-map format (lo8 = %d) does not match the weights' (nk16 = %d)", a.lo8, a.nk16);
    PB_CHECK(!a.o8_off || mx, -1, "gemm: an fp8 output copy needs an MX build");
    if (amode == A_DENSE && epi == EPI_STD) return mx ? pb_gemm_dense_std_mx(stream, tile, a) : pb_gemm_dense_std_f16(stream, tile, a);
    if (amode == A_DENSE && epi == EPI_RESID) return mx ? pb_gemm_dense_resid_mx(stream, tile, a) : pb_gemm_dense_resid_f16(stream, tile, a);
    if (amode == A_DENSE && epi == EPI_QKV) return mx ? pb_gemm_dense_qkv_mx(stream, tile, a) : pb_gemm_dense_qkv_f16(stream, tile, a);
    if (amode == A_DENSE && epi == EPI_PIXSHUF) return mx ? pb_gemm_dense_pixshuf_mx(stream, tile, a) : pb_gemm_dense_pixshuf_f16(stream, tile, a);
    if (amode == A_DENSE && epi == EPI_PATCH) { PB_CHECK(!mx, -1, "gemm: no MX build of epilogue %d", epi); return pb_gemm_dense_patch_f16(stream, tile, a); }
    if (amode == A_DENSE && epi == EPI_F32) { PB_CHECK(!mx, -1, "gemm: no MX build of epilogue %d", epi); return pb_gemm_dense_f32_f16(stream, tile, a); }
    if (amode == A_CONV && epi == EPI_F32) { PB_CHECK(!mx, -1, "gemm: no MX build of epilogue %d", epi); return pb_gemm_conv_f32_f16(stream, tile, a); }
    if (amode == A_CONV && epi == EPI_STD) return mx ? pb_gemm_conv_std_mx(stream, tile, a) : pb_gemm_conv_std_f16(stream, tile, a);
    if (amode == A_CONV && epi == EPI_PIXSHUF) return mx ? pb_gemm_conv_pixshuf_mx(stream, tile, a) : pb_gemm_conv_pixshuf_f16(stream, tile, a);
    if (amode == A_CONV && epi == EPI_HEAD) return mx ? pb_gemm_conv_head_mx(stream, tile, a) : pb_gemm_conv_head_f16(stream, tile, a);
    PB_CHECK(false, -1, "gemm: unsupported amode/epilogue %d/%d", amode, epi);
}
