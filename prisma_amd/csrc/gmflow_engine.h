// flow_gmflow band engine: GMFlow at the band's defaults (bands/flow_gmflow.py:223-255: feature_channels 128, 1 scale,
// 1 head, swin attention with 2 x 2 windows, global matching, global propagation, 6 transformer blocks, ffn x 4, padding_factor 16), and
// with set_matching the two inference-time radii of the same checkpoint (local matching, local-window propagation: gmflow_local.hip).
// Frame prep, the instance-norm encoder and the tail of a call (convex upsampling, flow encode, consistency masks) are FlowEngine's.
#pragma once
#include <vector>

#include "flow_engine.h"
#include "gmflow_kernels.h"

// Host tables of prepare_g (gmflow_engine.hip; pb_op_gm_tables hands the same two functions to the tests): the per-window sine position
// embedding tiled over the 2 x 2 windows, token-major [h8 * w8, 128], and the shifted-window region ids in window order [4][Lw]
// (splits = 8 on the 1/4 grid: the two-scale model's fine scale, [64][Lw] regions)
void sine_positions(int h8, int w8, std::vector<float> &pos, int splits = 2);
void shift_regions(int h8, int w8, std::vector<int8_t> &reg, int splits = 2);
// the window geometry of an h8 x w8 token grid (multiples of splits, at least 2 x splits) and ldvP, the row stride of the matching /
// propagation V^T (round_up(P, 32))
void gm_geometry(int h8, int w8, GmGeom &g, int &ldvP, int splits = 2);

class GmflowEngine : public FlowEngine {
  public:
    explicit GmflowEngine(int device, const CreateEnv &env = create_env()) : FlowEngine(device, env) {}
    int load(const pb_tensor *w, int n) override;
    // `iters` is ignored (GMFlow is not iterative)
    int infer(const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward, float *flow_out, uint8_t *rgb_out,
              float *maxdisp, uint8_t *mask_out = nullptr, float alpha1 = 0.05f, float alpha2 = 0.5f) override;
    // It registers its own stages only, all fp32 rows [n, rows, cols]: "feat" [F, P, 128], "block0" / "tfeat" [2 pairs, P, 128] (token stream after
    // the first / last transformer block), "flow_match" / "flow_prop" [pairs * dirs, P, 2] - with two scales these are the coarse scale's, and
    // the fine scale adds (B = pairs * dirs, P4 = 4 P): "feat4" [F, P4, 128], "flow_up" [B, P4, 2], "warp" [B, P4, 128], "block0_4" / "tfeat4"
    // [2 B, P4, 128], "flow_match4" (enlarged flow + matched residual) / "flow_prop4" [B, P4, 2]

    // --inference_size of the band (reference flow_gmflow.py:76-100): the network runs on a bilinear (align_corners) resize of the scaled frame to
    // (h, w) - multiples of 16, no padding - and the flow is resized back and rescaled; (0, 0) = off (InputPadder(16), the default)
    int set_inference_size(int h, int w);
    // --corr_radius_list / --prop_radius_list of the band (reference gmflow.py:128-157): -1 = global (the default), else local matching
    // over (2 R + 1)^2 target tokens, 1 <= R <= 4, and local-window propagation, 1 <= r <= 2.  With local matching the backward direction
    // is the forward direction of the swapped pair - what pred_bidir_flow equals wherever the reference can run it (with a matching
    // radius its pred_bidir_flow raises: local_correlation_softmax returns B flows for 2 B features).
    // On a two-scale context these are the FINE scale's radii (reference flags -1 R / -1 r): 1 <= R <= 4, 1 <= r <= 2, default (4, 1); -1 is
    // refused (global matching over the 1/4 grid is not built) and the coarse scale is always global.
    int set_matching(int corr_radius, int prop_radius);
    // 1, or 2 for the refinement model (gmflow_with_refine: num_scales 2, upsample_factor 4, padding_factor 32, attn_splits_list 2 8) - decided
    // by the weights in load(): 'backbone.trident_conv.weight' and an 'upsampler.2.weight' of 144 rows
    int num_scales() const { return scales_; }
    // two scales: the fine scale's token rows and batch elements bound the pairs of a call
    int chunk_pairs(int wanted, int H, int W, float scale, int dirs) const override;

  private:
    struct Layer {
        PackedW w1;                 // [q_s; k_s; v_s; k_c; v_c] x 128: every projection of the token stream as it enters the block
        PackedW merge_s, q_c, merge_c, mlp0, mlp2;
        float *ln1s_g, *ln1s_b, *ln1c_g, *ln1c_b, *ln2c_g, *ln2c_b;
    };
    int prepare_g(int F, int H, int W, float scale, int dirs);
    int upload(const std::string &name, int n, float **dst);
    int gemm32(const f16 *A, int lda, int64_t M, const PackedW &w, float *out, int ldo);
    int gemm16(const f16 *A, int lda, int64_t M, const PackedW &w, f16 *out, int ldo, int act, int lo_off);
    int attention(const Attn128Args &a, double keys_per_query);
    int conv32(const f16 *in, int n, int H, int W, int stride, const PackedW &w, float *out);
    int blocks(const GmGeom &g, int NPs, const int8_t *region, const char *blk0);
    int fine_scale(int B, int dirs);

    Enc backbone_;                  // CNNEncoder: FlowEngine's encoder without conv biases
    Layer layers_[6];
    PackedW ffq_, ffk_, up0_, up2_;
    GmGeom g_{};
    // two scales: the trident convolution, the 1/4 grid and its 8 x 8 windows, the fine scale's radii and buffers (stages of the same names)
    int scales_ = 1;
    PackedW trident_;
    GmGeom g4_{};
    int h4_ = 0, w4_ = 0, P4_ = 0;
    int corr_r4_ = 4, prop_r4_ = 1;
    f16 *c2_ = nullptr;               // conv2's output at 1/4 as a split map, the trident convolution's input
    float *feat4_ = nullptr, *pos4_ = nullptr, *warp_ = nullptr, *flowu_ = nullptr, *flowm4_ = nullptr, *flowf_ = nullptr, *flowp4_ = nullptr,
          *tfeat8_ = nullptr, *blk08_ = nullptr;
    int8_t *region4_ = nullptr;
    int isz_h_ = 0, isz_w_ = 0;
    int corr_r_ = -1, prop_r_ = -1;
    int options_ = 0;                 // the plan key's word: counts the changes set_inference_size / set_matching made, so the next call re-plans
    float *upi_ = nullptr;            // flow at the inference size, before the resize back
    int ldvP_ = 0;
    float *feat_ = nullptr, *pos_ = nullptr, *X_ = nullptr, *Y1_ = nullptr, *Yq_ = nullptr, *Ow_ = nullptr, *M_ = nullptr, *Om_ = nullptr,
          *flowm_ = nullptr, *flowp_ = nullptr, *blk0_ = nullptr;
    f16 *Xs_ = nullptr, *Qw_ = nullptr, *Kw_ = nullptr, *Kcw_ = nullptr, *Vtw_ = nullptr, *Vtcw_ = nullptr, *Os_ = nullptr, *cat_ = nullptr,
        *Hs_ = nullptr, *gridvt_ = nullptr, *Vtf_ = nullptr, *qs_ = nullptr, *ks_ = nullptr, *umap_ = nullptr, *u1_ = nullptr;
    int8_t *region_ = nullptr;
};
