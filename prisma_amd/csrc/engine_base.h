// Shared plumbing of the band engines (depth_anything, flow_raft, flow_gmflow, mask_mmdet): the ctx stream, the named-weight map, the upload
// of packed GEMM weights (pack_layout.h has the layouts) with folded BatchNorm, the two-pass arena planner (plan_arena), the timed launch
// (timed / timed_gemm: per-family and per-kernel timing around a launch), the implicit-GEMM / dense GEMM launch helpers, and the debug-stage
// registry behind pb_*_get_stage.  The two flow bands share more than this: flow_engine.h.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/prisma_bands.h"
#include "common.h"
#include "gemm.h"
#include "kernels.h"
#include "launch_env.h"
#include "pack_layout.h"

// The ctx stream of a band engine.  `se.cu_mask` (PB_CU_MASK_DEPTH / PB_CU_MASK_FLOW, launch_env.h) is a CU mask as comma-separated 32-bit hex
// words (bit i of the concatenation = CU i of the queue's mask; on gfx950 the driver deals the bits round-robin over the 8 XCDs, so 0f0f0f0f,...
// keeps XCDs 0-3): an experiment switch for running two bands on disjoint parts of the chip (tools/overlap_bench.py --cu-masks).  Empty = the whole device.
static inline hipError_t pb_create_stream(hipStream_t *s, const StreamEnv &se) {
    if (!se.cu_mask.empty()) {
        uint32_t words[8];
        int n = 0;
        for (const char *p = se.cu_mask.c_str(); *p && n < 8;) {
            char *end = nullptr;
            words[n++] = (uint32_t)strtoul(p, &end, 16);
            if (!end || end == p) break;
            p = *end == ',' ? end + 1 : end;
        }
        if (n > 0) return hipExtStreamCreateWithCUMask(s, (uint32_t)n, words);
    }
    // se.prio (<mask>_PRIO) = -1 / 1: a higher- / lower-priority queue (hipStreamCreateWithPriority; 0 = default).  Experiment switch: with two
    // bands at once the band with the large persistent GEMMs gets more than half of the chip (tools/overlap_bench.py 2way-fprio / 2way-dprio)
    if (se.prio != 0) {
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) return hipStreamCreateWithPriority(s, hipStreamNonBlocking, se.prio < 0 ? hi : lo);
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

// A device allocation freed when it goes out of scope.  alloc: a zeroed buffer (the op-level entry points); reserve: at least `bytes` of
// undefined contents, grown by free + malloc and never shrunk (debug snapshots, get_stage temporaries)
struct DevMem {
    void *p = nullptr;
    size_t cap = 0;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { if (p) hipFree(p); }
    int alloc(size_t bytes) {
        PB_HIP(hipMalloc(&p, bytes < 256 ? 256 : bytes));
        PB_HIP(hipMemset(p, 0, bytes < 256 ? 256 : bytes));
        PB_HIP(hipDeviceSynchronize());     // memset runs on the null stream; kernels use the ctx stream
        return 0;
    }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) PB_HIP(hipFree(p));
        p = nullptr; cap = 0;
        PB_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return 0;
    }
    template <class T> T *as() { return (T *)p; }
};

// A debug stage (pb_*_get_stage): a device buffer of the last infer call and how EngineBase::get_stage turns it into the caller's fp32
// array.  One kind = one source layout and one shape_out in every band; `n` (frames, pairs x directions, ... - prisma_bands.h says which per
// stage) is what the buffer held when the stage was registered.
struct Stage {
    enum Kind {
        F32_ROWS,            // fp32 [n, rows, cols], batch elements bstride floats apart            -> [n, rows, cols, 1]
        F16_ROWS,            // fp16 [n * rows, ld], the first cols of every row                     -> [n, rows, cols, 1]
        F16_NHWC,            // fp16 [n, h, w, ld], the first c of every pixel; lo_off != 0: a split map, the residual parts lo_off halfs
                             // further on are added in fp32 on the host                             -> [n, c, h, w]
        F32_NCHW,            // fp32 [n, c, h, w], contiguous                                        -> [n, c, h, w]
        F32_NHWC,            // fp32 [n, h, w, ld], the first c of every pixel                       -> [n, c, h, w]
    };
    Kind kind;
    const void *ptr;
    int64_t n, c, h, w;      // the row kinds keep rows in h and cols in w (c = 1)
    int64_t ld, bstride, lo_off;
    static Stage f32_rows(const void *p, int64_t n, int64_t rows, int64_t cols, int64_t bstride = 0) {
        return Stage{F32_ROWS, p, n, 1, rows, cols, cols, bstride ? bstride : rows * cols, 0};
    }
    static Stage f16_rows(const void *p, int64_t n, int64_t rows, int64_t cols, int64_t ld) { return Stage{F16_ROWS, p, n, 1, rows, cols, ld, 0, 0}; }
    static Stage f16_nhwc(const void *p, int64_t n, int64_t c, int64_t h, int64_t w, int64_t ld, int64_t lo_off = 0) {
        return Stage{F16_NHWC, p, n, c, h, w, ld, 0, lo_off};
    }
    static Stage f32_nchw(const void *p, int64_t n, int64_t c, int64_t h, int64_t w) { return Stage{F32_NCHW, p, n, c, h, w, 0, 0, 0}; }
    static Stage f32_nhwc(const void *p, int64_t n, int64_t c, int64_t h, int64_t w, int64_t ld) { return Stage{F32_NHWC, p, n, c, h, w, ld, 0, 0}; }
};

struct KernelTimer {
    struct Rec { int fam; hipEvent_t a, b; double flops, bytes, exec; const char *name; };   // name: GEMM launches, the kernel symbol (gemm.h)
    // per family (non-GEMM kernels) / per GEMM kernel symbol sums of the records
    int collect(const char *const *fam_names, int nfam, pb_kernel_stat *out, int cap);
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    bool enabled = false;
    bool accumulate = false;      // keep the records of earlier infer calls (one query after a timed loop)
    hipEvent_t get();
    void reset() { if (accumulate) return; recs.clear(); used = 0; }
    void clear() { recs.clear(); used = 0; }
    ~KernelTimer();
};

class EngineBase {
  public:
    // env: the create-time switches (launch_env.h) - pb_create reads them once per context, the op-level helpers at every call;
    // fam_names: the F_COUNT family names stats() reports (default: the convolutional bands' table, engine_base.hip)
    explicit EngineBase(int device, const CreateEnv &env = create_env(), const char *const *fam_names = nullptr);
    virtual ~EngineBase();
    int stats(pb_kernel_stat *out, int cap);
    // the stage `name` of the last infer call as fp32 in out[cap] (floats): returns the element count and the dimensions in shape, or a
    // negative pb error ("unknown stage", "stage buffer too small") that leaves the registry as it was
    int64_t get_stage(const char *name, float *out, int64_t cap, int64_t shape[4]);

    const CreateEnv env;
    hipStream_t stream = nullptr;
    int device = 0;
    bool debug = false;
    KernelTimer timer;
    int conv_tile = TILE_AUTO;
    int dense_tile = TILE_AUTO;  // tile of the dense GEMMs (pb_set_option "gemm_tile"; the split-precision op entry points force one)
    float *sk_ws_ = nullptr;     // split-K workspace the launches lend launch_gemm (gemm.h sk_ws; null in the convolutional engines)
    int64_t sk_cap_ = 0;
    int split_w_ = 0;            // PB_PREC_SPLIT: weights packed as hi + lo fp16, two passes over K (set before load)
    int mx_ = 0;                 // ... and where activations are split too (sa) the residual parts are e4m3: maps [hi | hi8 | lo8],
                                 // weights [w_hi | w_lo8 | w_hi8] per tap, fp8 tiles through the MX-scaled MFMA (PackedW::mx3)
    // power-of-two storage scales of the e4m3 copies.  hi8 = e4m3(x 2^kLo8Pa), lo8 = e4m3((x - fp16(x)) 2^(kLo8Pa + 12)); e4m3 saturates at
    // 448, so the copy of |x| > 448 / 2^kLo8Pa clamps and that element's correction term degrades to the single-pass error.  Round 3:
    // 2^0 (saturation at 448; was 2^3 = 56) - a correction term needs a few significant bits of a NORMAL e4m3 (|x| >= 2^-6) and what
    // lies below contributes |x| 2^-12 |w| at most (tools/precision_budget.py --scales; tests/test_gpu_outliers.py)
    const int kLo8Pa = env.lo8_pow;               // PB_LO8_POW
    int pack_mx2_ = 0;           // while set, pack() lays weights out as [w_hi fp16 | w_lo e4m3] per tap (PackedW::mx2): the layer's input
                                 // map carries an fp8 copy after its fp16 part ([a16 (Ctot) | a8 (Ctot bytes)], scaled by 2^kMx2Pa)
    const int kMx2Pa = env.a8_pow;      // PB_A8_POW.  [a16 | a8] maps: a8 = e4m3(a 2^kMx2Pa); 2^0 since round 3 (was 2^4: |a| > 28 clamped)
    int pack_tapin_ = 0;         // while set, pack() stores convolution weights (taps > 1) in slice-major K order (gemm.h cTapInner)
    const f16 *zero_page() const { return zero_; }

  protected:
    // kernel families of the per-launch timer; convolutions are split by the GEMM kernel that runs them (launch_gemm's choice).  Indices 6
    // and 7 are the band's own: the depth band counts its residual / qkv GEMMs there (engine.hip)
    enum { F_GEMM = 0, F_CONV = 1, F_ATTN = 2, F_LN = 3, F_ELT = 4, F_PP = 5, F_CONV128 = 6, F_CONV64 = 7, F_COUNT = 8 };

    // create the ctx stream (pb_create_stream; depth_stream: env.stream_depth instead of env.stream_flow), index the float32 tensors by name,
    // allocate the zero page
    int begin_load(const pb_tensor *w, int n, bool depth_stream = false);
    const pb_tensor *find(const std::string &name) const;
    int upload_f32(const float *src, size_t n, float **dst);
    // src: host fp32 [N, K] in GEMM order -> device fp16 [round_up(N, 256), out.K] in the layout `spec` asks for (pack_layout.h pack_rows)
    // and a zero-padded fp32 bias of round_up(N, 256)
    int pack_spec(const float *src, int N, int K, int Kpad, PackedW &out, const float *bias, int taps, const PackSpec &spec);
    // the same with the layout derived from the engine's flags (split_w_, mx_, pack_mx2_, pack_tapin_): weights are split where the sizes
    // allow it, and sa (the activation operand is a split map [hi | lo]) only counts with split weights
    int pack(const float *src, int N, int K, int Kpad, PackedW &out, const float *bias, int taps = 1, int sa = 0);
    // eval-mode BatchNorm2d (eps 1e-5) as a per-channel (scale, shift)
    int fold_bn(const std::string &bn, int C, std::vector<float> &scale, std::vector<float> &shift);
    // conv weight [co, ci, kh, kw] (+ bias) -> rows [co][(ky * kw + kx) * round_up(ci, 64) + c], optional per-output affine
    // ci_pad: input channels the rows are padded to (default round_up(ci, 64))
    int pack_conv(const std::string &name, bool has_bias, const float *scale, const float *shift, PackedW &out, int sa = 0, int ci_pad = 0);

    // direct launch_gemm callers: W, K, bias, the zero page, and with split weights the K wrap / channel / MX bookkeeping of gemm.h.
    // Convolutions set a.cC (and a.cLd, unless the map is exactly its parts) of ONE part before the call, and check a.cC == w.Cseg
    void set_weights(GemmArgs &a, const PackedW &w, bool is_conv) const;

    // The two-pass arena of a prepare(): `carves` assigns every buffer of the plan with carve() and returns 0 or a pb error.  It runs twice -
    // first planning (carve returns null and only adds up the sizes), then, with the arena grown to the planned size and zeroed, for real -
    // so a buffer's offset is decided by the order and the sizes of the carve calls alone.  `what` names the arena in the allocation error.
    int plan_arena(const char *what, const std::function<int()> &carves);
    void *carve(size_t bytes);

    // One timed launch: `launch` issues the kernel(s) of one timer record and returns their status; with the timer on, the record opens on
    // cur_ before the call and closes on cur_ after it (cur_: the ctx stream unless a derived engine forks work onto side streams), counted
    // in family `fam` with the algorithmic flops / bytes and `passes` MFMA passes over the flops.  `name`: the kernel symbol stats() reports
    // instead of the family's name.  A failed launch leaves its record without a name.
    template <class Launch> int timed(int fam, double flops, double bytes, Launch &&launch, const char *name = nullptr, double passes = 1.0) {
        if (!timer.enabled) return launch();
        const size_t rec = tic(fam, flops, bytes, passes);
        const int r = launch();
        if (!r) timer.recs[rec].name = name;
        toc(rec);
        return r;
    }
    // ... of launch_gemm (or a launcher that records its choice the same way): named by the kernel symbol the launch picked (gemm.h)
    template <class Launch> int timed_gemm(int fam, double flops, double bytes, Launch &&launch, double passes = 1.0) {
        if (!timer.enabled) return launch();
        const size_t rec = tic(fam, flops, bytes, passes);
        const int r = launch();
        if (!r) timer.recs[rec].name = pb_gemm_last_kernel();
        toc(rec);
        return r;
    }
    // fusion hooks of one conv() call: a second (ReLU'd) copy of the output, and the SepConvGRU epilogues (gemm.h ACT_GRU_*)
    struct ConvFuse { f16 *out2 = nullptr; float *gru_h = nullptr; const f16 *gru_z = nullptr; f16 *gru_rh = nullptr; int gru_ld = 384;
                      const f16 *add2 = nullptr; };       // add2: a second skip tensor (same row stride as the output), added next to add1
    // lo_off != 0: out (and add1) are split-fp16 maps, the rounding residual of every output goes to +lo_off (gemm.h)
    int conv(const f16 *in, int cC, int cLd, int n, int H, int W, int kh, int kw, int stride, const PackedW &w, f16 *out, int ldo,
             int act, int pre_relu = 0, const f16 *add1 = nullptr, const ConvFuse *fuse = nullptr, int lo_off = 0, int a8_rel = 0,
             int o8_off = 0);
    // a8_rel (mx2 weights): half-offset from `in` to the fp8 copy of its channels (0 = right after the cC channels); o8_off: byte
    // offset, from the output row, of the fp8 copy the epilogue also stores (0 = none)
    int dense(const f16 *A, int lda, int64_t M, const PackedW &w, f16 *out, int ldo, int act, const f16 *add1 = nullptr, int o8_off = 0,
              int a_pa = -1, int lo_off = 0);          // a_pa: power-of-two scale the A operand's fp8 copy was stored with (default kMx2Pa)

    // The debug-stage registry: infer() clears stages_ and registers views of arena buffers as it goes (`as.ptr` of a snapshot is ignored).
    // snapshot() registers a copy instead - of a buffer that later launches overwrite - made on `stream` into a buffer kept under `name`,
    // which grows when a call needs more; engines call it only while `debug` is set.
    int snapshot(const std::string &name, const void *src, size_t bytes, Stage as);
    std::map<std::string, Stage> stages_;

    const char *const *fam_names_;
    std::map<std::string, const pb_tensor *> tmap_;
    std::vector<void *> owned_;                 // permanent device allocations (weights), freed by the destructor
    f16 *zero_ = nullptr;
    size_t plan_bytes_ = 0;                     // what the last plan_arena carved (the arena itself never shrinks)
    hipStream_t cur_ = nullptr;

  private:
    // grow the arena to the planned size (after the planning pass) and zero it
    int commit_arena(const char *what);
    char *arena_ = nullptr;
    size_t arena_bytes_ = 0, arena_off_ = 0;
    bool planning_{false};
    size_t tic(int fam, double flops, double bytes, double passes);     // opens a record on cur_, returns its index
    void toc(size_t rec);
    int upload_rows(const std::vector<f16> &rows, f16 **dst);
    std::map<std::string, DevMem> snaps_;
};
