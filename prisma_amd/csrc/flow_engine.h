// What the two flow bands (flow_raft: raft_engine.h, flow_gmflow: gmflow_engine.h) share: frame prep, the residual encoder (RAFT's BasicEncoder;
// GMFlow's CNNEncoder is the same encoder without conv biases), the padded geometry and the resize tables, the plan key, and the tail of a call -
// convex upsampling, flow encode, consistency masks.
#pragma once
#include <string>

#include "engine_base.h"
#include "raft_kernels.h"

class FlowEngine : public EngineBase {
  public:
    explicit FlowEngine(int device, const CreateEnv &env) : EngineBase(device, env) {}
    virtual int load(const pb_tensor *w, int n) = 0;
    // frames: device uint8 [F, H, W, 3].  Outputs are device pointers (any may be null):
    //   flow_out [F-1, dirs, sh, sw, 2] fp32, rgb_out [F-1, dirs, sh, sw, 3] u8, maxdisp [F-1, dirs]; mask_out (needs backward): the forward /
    //   backward consistency masks of pb_flow_infer_sequence_masks (prisma_bands.h)
    virtual int infer(const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward, float *flow_out,
                      uint8_t *rgb_out, float *maxdisp, uint8_t *mask_out = nullptr, float alpha1 = 0.05f,
                      float alpha2 = 0.5f) = 0;
    // largest chunk of pairs <= wanted that one infer() call accepts at this frame size; 0: not even one pair
    virtual int chunk_pairs(int wanted, int H, int W, float scale, int dirs) const { return wanted; }
    int64_t plan_bytes() const { return (int64_t)plan_bytes_; }
    static void out_size(int H, int W, float scale, int *sh, int *sw);

  protected:
    struct Enc {                    // BasicEncoder weights (BN folded for RAFT's cnet)
        PackedW stem, l[3][2][2], ds[3], out;
    };
    int pack_encoder(const std::string &en, bool bnf, bool conv_bias, Enc &E);
    int run_encoder(const Enc &E, bool inorm, int F, const f16 **x_out);
    // arena buffers of frame prep and run_encoder: the first carves of a prepare's plan
    void carve_encoder(int F);
    int enc_s3_ = 2;            // stride of the encoder's third stage: 1 = its output stays at 1/4 (the two-scale GMFlow backbone, backbone.py:58-62)

    // The key of the plan the arena holds, as the last successful prepare left it: a call of at most F frames and `dirs` directions at the same
    // frame size and scale, with the same `word`, runs on it without re-planning.  word: what else a derived engine's plan depends on.
    // A prepare that re-plans calls clear() BEFORE it rewrites the geometry and the buffers and set() after its last step that can fail: a
    // failure in between (a frame too small, an allocation) must not leave the OLD plan's key behind, or the next call with the old size
    // would skip prepare and run on the half-written geometry (found by tests/test_gpu_raft.py::
    // test_pipeline_error_exit_leaves_no_copy_in_flight - wrong flows after a refused 40 x 40 call).
    struct PlanKey {
        int F = 0, H = 0, W = 0, dirs = 0, word = 0;
        float scale = 0.f;
        bool covers(int f, int h, int w, float s, int d, int wd) const { return f <= F && h == H && w == W && s == scale && d <= dirs && wd == word; }
        void clear() { F = 0; H = 0; W = 0; dirs = 0; }
        void set(int f, int h, int w, float s, int d, int wd) { F = f; H = h; W = w; scale = s; dirs = d; word = wd; }
    };
    PlanKey plan_;

    // flow_geometry (flow_chunk.h) into the members below
    void geometry(int H, int W, float scale, int factor);
    int upload_resize_tables(int H, int W, float scale);
    int sh_ = 0, sw_ = 0, Hp_ = 0, Wp_ = 0, padl_ = 0, padt_ = 0, h8_ = 0, w8_ = 0, P_ = 0;
    int *xi_ = nullptr, *xc_ = nullptr, *yi_ = nullptr, *yc_ = nullptr;
    f16 *img_ = nullptr;                              // padded frames, 4 x 4 space-to-depth: [F, Hp / 4, Wp / 4, 64] fp16
    f16 *r1_[7] = {}, *r2_[7] = {}, *r3_[7] = {};     // scratch maps at 1/2, 1/4, 1/8 resolution: t1 t2 t3 outA outB stem stem_n
    float *st_[3] = {};                               // instance-norm statistics {mean, rstd} per (frame, channel)
    float *stp_ = nullptr;                            // ... and their per-chunk partial sums

    // frames -> img_: cubic resize to the scaled size, replicate padding, 4 x 4 space-to-depth.  lo8: power-of-two scale of the e4m3 residual
    // parts of a split map, -1 = fp16 residuals; norm: ImageNet mean / std (GMFlow); isz: (Hp_, Wp_) is GMFlow's --inference_size
    int prep_frames(const uint8_t *frames, int F, int H, int W, float scale, int lo8, int norm = 0, int isz = 0);

    // The tail of a call: convex upsampling of the N = pairs * dirs flow fields flow_lo [N, hu * wu, 2] on the 1 / factor grid with the logits in
    // mask_, unpadding to [N, sh_, sw_, 2] (in flow_out, or up_ when the caller wants no flow), flow encode, and with mask_out the forward /
    // backward consistency masks.  upi (GMFlow's --inference_size): upsample at the network size Hp_ x Wp_ into upi, then resize back.
    int flow_tail(const float *flow_lo, int N, int pairs, int hu, int wu, int factor, float *flow_out, uint8_t *rgb_out, float *maxdisp,
                  uint8_t *mask_out, float alpha1, float alpha2, float *upi = nullptr);
    float *mask_ = nullptr;           // convex-upsampling logits [N * hu * wu, 9 * factor^2]
    float *up_ = nullptr;             // full-size flow of a call without flow_out
    unsigned *maxd_ = nullptr;        // per (pair, direction) max displacement, as float bits
};
