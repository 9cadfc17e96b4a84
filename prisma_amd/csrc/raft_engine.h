// flow_raft band engine: weight packing (BatchNorm folded), arena planning, launch sequence.  Frame prep, the encoder and the tail of a call are
// FlowEngine's (flow_engine.h); the two encoders' weights, the correlation pyramid, the update block and the context hoist are this class's.
#pragma once
#include "flow_engine.h"

class RaftEngine : public FlowEngine {
  public:
    explicit RaftEngine(int device, const CreateEnv &env = create_env()) : FlowEngine(device, env) {}
    int load(const pb_tensor *w, int n) override;
    int infer(const uint8_t *frames, int F, int H, int W, float scale, int iters, int backward, float *flow_out, uint8_t *rgb_out,
              float *maxdisp, uint8_t *mask_out = nullptr, float alpha1 = 0.05f, float alpha2 = 0.5f) override;
    // --alternate_corr (raft.py:103-106): the lookup computes its window entries from the feature maps (corr_otf.hip) and prepare() carves no
    // correlation volume.  The plan key's word: the next call re-plans.
    void set_alternate_corr(int on) { alt_corr_ = on ? 1 : 0; }
    // pb_set_option "corr_layout" (corr_layout.h): 1 = the volume source-blocked and corr_lookup_blocked_kernel (default), 0 = row-major and
    // corr_lookup_kernel.  Same bytes out either way; part of the plan key's word (a blocked level holds round_up(P, 8) rows per pair-direction).
    void set_corr_layout(int blocked) { corr_layout_ = blocked ? 1 : 0; }
    // the hoisted GRU share's 32-bit plane offset bounds the pairs of a call (flow_chunk.h)
    int chunk_pairs(int wanted, int H, int W, float scale, int dirs) const override;

  private:
    int prepare(int F, int H, int W, float scale, int dirs);
    Enc fnet_, cnet_;
    PackedW convc1_, convc2_, convf1_, convf2_, convm_, zr_[2], q_[2], fh1_, fh2_, mk0_, mk2_;
    // convf1 as a direct kernel on the fp32 flow field (raft_kernels.hip convf1_kernel; PB_CONVF1_DIRECT=0: im2col + GEMM as in rounds 1-3)
    f16 *f1w_ = nullptr;
    int f1_passes_ = 1;
    bool f1_direct_ = true;
    // context hoist (raft_engine.hip load()): zr_ / q_ then cover [h | motion] only, zr_in_ / q_in_ the context features' 128 channels
    PackedW zr_in_[2], q_in_[2];
    int hoist_ = 0;
    f16 *gz_[2] = {}, *gq_[2] = {};             // hoisted shares: [hi plane | lo plane], rows x 256 (z | r) and rows x Lhx (q)

    // plan
    int alt_corr_ = 0;
    int corr_layout_ = 1;
    // the layout the volume is stored in: blocked only where volume.hip writes it (PB_VOLUME=0's generic GEMM writes row-major)
    int vol_layout() const;
    int plan_word() const { return alt_corr_ | (vol_layout() << 1); }
    int lh_[4] = {0, 0, 0, 0}, lw_[4] = {0, 0, 0, 0};
    f16 *fmap_ = nullptr, *ctx_ = nullptr;
    f16 *pyr_[4] = {};                                // correlation volume levels: fp16 [pairs][corr_layout_rows(P)][pld_] in 8 x 8 target tiles (corr_layout.h)
    f16 *ftile_[4] = {};                              // target features / 16 in tile order (B operand of the volume GEMM)
    int lwp_[4] = {}, lhp_[4] = {};                   // padded width / height of a level's tiled layout (multiples of 8)
    f16 *fpool_[4] = {};                              // avg-pooled target features of levels 1..3
    int pld_[4] = {};
    float *h32_ = nullptr, *flow_ = nullptr;
    f16 *hx_ = nullptr, *hx2_ = nullptr, *corr_ = nullptr, *c1_ = nullptr, *corflo_ = nullptr, *fa_ = nullptr, *f1_ = nullptr,
        *zrb_ = nullptr, *fh_ = nullptr, *m0_ = nullptr;
    int upd8_ = 0;               // the update block's maps carry fp8 copies and its weights e4m3 residuals (MX segments; raft_engine.hip load)
    // (debug snapshots - EngineBase::snapshot, pb_set_profiling bit 2 - keep what later iterations overwrite: the initial hidden state, the
    // first lookup's output and the flow after the first iteration, the intermediates the reference goldens hold: tests/golden/raft_*.npz)
};
