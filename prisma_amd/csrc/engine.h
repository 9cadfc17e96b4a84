// Depth-Anything band engine: weight loading, arena planning and the per-batch launch sequence.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "engine_base.h"
#include "zoe_kernels.h"

class DepthEngine : public EngineBase {
  public:
    DepthEngine(int device, const pb_depth_cfg &cfg, const CreateEnv &env = create_env());
    int load(const pb_tensor *w, int n);
    int infer(const uint8_t *frames_dev, int n, int H, int W, float *depth_out, uint8_t *rgb_out, float *mn,
              float *mx, int flip);
    int max_batch() const { return cfg_.max_batch > 0 ? cfg_.max_batch : 1; }

  private:
    int prepare(int B, int H, int W);
    int run_chunk(const uint8_t *frames, int n, float *depth_out, uint8_t *rgb_out, float *mn, float *mx, int flip);
    int vit(int n);
    int head(int f0, int n);
    int tail(int n, float *depth_out, uint8_t *rgb_out, float *mn, float *mx, int flip);
    // ZoeDepth metric head (engine_zoe.hip)
    int load_metric();
    int plan_metric(int B, int H, int W);
    int metric_tables(int H, int W);
    int metric_head(int n);
    int gemm(int amode, int epi, GemmArgs &a, const PackedW &w, int tile = TILE_AUTO);
    int conv3(const f16 *in, int inC, int n, int H, int W, const PackedW &w, f16 *out, f16 *out2, const f16 *add1,
              const f16 *add2, int act, int stride, int outC);
    // the layout of one weight (pack_layout.h): sa / sw / mx2 as given, e4m3 residual parts and slice-major rows as the head runs them
    PackSpec spec(int sa, int sw, int mx2 = 0) const;
    int pack_vit(const float *wt, int N, int K, PackedW &out, const float *bias, bool keep_res);
    int snapshot_tokens(const std::string &name, int n);      // debug copy of the residual stream X_ as stage `name`

    pb_depth_cfg cfg_;
    // PB_PREC_SPLIT (tools/precision_budget.py): ViT linears and the metric head keep their weights as hi + lo (2 passes);
    // the DPT head keeps weights AND feature maps as hi + lo (3 passes; maps are [hi | lo] per pixel, hs_ = 2)
    int head_tapin_ = 1;         // the head's 3x3 convolutions walk K slice-major (gemm.h cTapInner; PB_TAPIN=0 turns it off)
    int vit_sw_ = 0, head_sa_ = 0, head_sw_ = 0, hs_ = 1;
    // vit_mx_: the ViT linears' weight residual runs as an MX-fp8 segment (half the matrix-pipe time of an fp16 pass); their A
    // operands (LayerNorm out, attention out, GELU out) then carry an fp8 copy after the fp16 part of each row (row stride 1.5 K)
    int vit_res_ = 15;           // which ViT linears keep their weight residual: bit 0 qkv, 1 proj, 2 fc1, 3 fc2 (engine.hip load())
    int vit_mx_ = 0, head_mx_ = 0;              // head_mx_: the DPT head's maps / weights carry e4m3 residual parts (PackedW::mx3)
    // storage scales of the e4m3 copies (engine_base.h): head maps hi8 = e4m3(x 2^kLo8Pa), lo8 = e4m3(lo 2^(kLo8Pa + 12)); ViT token rows
    // a8 = e4m3(a 2^kMx2Pa)
    int batch_cap(int H, int W) const;          // frames per chunk the 32-bit tensor offsets allow for this frame size
    // weights
    PackedW patch_;
    float *cls_ = nullptr;
    std::vector<float> pos_host_;               // [1 + g*g, D]
    struct Block { float *ln1g, *ln1b, *ln2g, *ln2b, *ls1, *ls2; PackedW qkv, proj, fc1, fc2; };
    std::vector<Block> blocks_;
    float *normg_ = nullptr, *normb_ = nullptr;
    PackedW proj_[4], rs0_, rs1_, rs3_, rn_[4], outc_[4], rcu_[4][2][2], oc1_, oc2_;
    // output_conv2's 3 x 3 weights as a 1 x 1 GEMM [9 x 32, F / 2] over output_conv1's LOW-resolution map: row t * 32 + c = tap t of output channel c
    // (the convolution commutes with the bilinear resize in front of it; elementwise.hip dpt_tail_kernel sums the resized tap products).  PB_HEAD_TAIL=0:
    // the round-1..5 formulation (resize to the network size, implicit GEMM with the fused 1 x 1 there); the metric head keeps that one (it needs the
    // 32-channel activation at the network resolution)
    PackedW wz_;
    int head_tail_ = 1;
    f16 *z_ = nullptr;
    float *w2_ = nullptr;
    float b2_ = 0.f;
    // split-K workspace (engine_base.h sk_ws_, gemm.h splitk): lent to every launch of a context created with max_batch = 1 - one frame per call is the latency
    // configuration (BASELINE.json configs[1]), its residual GEMMs and low-resolution head convolutions have 20-160 tiles for 256 CUs.
    // Contexts with max_batch > 1 never split, so a frame's bits do not depend on the size of the batch it arrives in; they do differ (within
    // the parity tolerance) between a max_batch = 1 context and the others.  PB_SPLITK=0 turns it off, PB_SPLITK_ALWAYS=1 lends it to every ctx.
    static constexpr int64_t kSkFloats = (int64_t)512 * 128 * 128;      // 512 slices of a 128 x 128 fp32 tile: 32 MB

    // plan
    int pB_ = 0, pH_ = 0, pW_ = 0;
    int hB_ = 1;                                // frames per DPT-head chunk (<= batch_cap: 32-bit offsets of the high-resolution split maps)
    int nh_ = 0, nw_ = 0, gh_ = 0, gw_ = 0, ntok_ = 0, ntp_ = 0, P_ = 0;
    int lh_[4] = {0, 0, 0, 0}, lw_[4] = {0, 0, 0, 0};      // DPT level sizes (level 0 = finest)
    // arena buffers
    int *xi_ = nullptr, *yi_ = nullptr;
    float *xw_ = nullptr, *yw_ = nullptr, *pos_ = nullptr;
    f16 *patchA_ = nullptr, *Y_ = nullptr, *Q_ = nullptr, *K_ = nullptr, *Vt_ = nullptr, *AO_ = nullptr, *Hd_ = nullptr;
    float *X_ = nullptr;
    f16 *feat_[4] = {nullptr, nullptr, nullptr, nullptr};
    f16 *pj_[4] = {}, *lay_[4] = {}, *rnraw_[4] = {}, *rnrelu_[4] = {}, *tmp_[4] = {}, *sraw_[4] = {}, *srelu_[4] = {},
        *yb_[4] = {}, *ocb_[4] = {}, *path_[4] = {};
    f16 *o1_ = nullptr, *up_ = nullptr;
    float *netd_ = nullptr, *full_ = nullptr;
    unsigned *mm_ = nullptr;
    // metric head: weights, buffers (arena), Pillow resize tables
    struct Mlp2 { PackedW a, b; };
    PackedW zconv2_;
    Mlp2 zseed_, zsproj_, zproj_[4], zattr_[4], zclb_;
    f16 *act32_ = nullptr, *zx0_ = nullptr, *zh_ = nullptr, *zemb_[2] = {}, *zxa_ = nullptr, *zcat_ = nullptr, *zmid_ = nullptr;
    float *zA_ = nullptr, *zbins_[2] = {}, *zpt_ = nullptr, *md_ = nullptr, *ptmp_ = nullptr;
    int *pxb_ = nullptr, *pyb_ = nullptr;
    double *pxk_ = nullptr, *pyk_ = nullptr;
    int pxks_ = 0, pyks_ = 0;
};
