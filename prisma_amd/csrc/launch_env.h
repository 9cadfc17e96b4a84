// Every PB_* environment switch the library honours, read in launch_env.cpp and nowhere else (host only, no HIP headers; DESIGN.md has the
// table of names, defaults and users).  Three lifetimes:
//   launch_env()  read once per process, at the first call from any thread; an A/B run of one needs a fresh process
//   create_env()  read at the moment of the call: pb_create takes one and hands it to the engine it constructs
//   bench_env()   read per call by the pb_op_gemm_bench tool op
#pragma once
#include <string>

struct LaunchEnv {
    int gemm_stagger;       // PB_GEMM_STAGGER=<percent>: > 0 de-phases the CUs by that share of 1/8 tile period per step
    int pixshuf_buf;        // PB_PIXSHUF_BUF: 0 = flat-addressed pixel-shuffle epilogue
    int tile_wide;          // PB_TILE_WIDE=<min columns of the last 256-wide tile>, 0 = off
    int tile_n96;           // PB_TILE_N96: initial value of pb_set_option("tile_n96") (gemm.h pb_gemm_set_n96)
    int splitk;             // PB_SPLITK: largest split-K factor; 0 / 1 = off
    int epi_report;         // PB_EPI_REPORT=1 names EPI_STD launches outside the fast-epilogue list
    int gemm_persist;       // PB_GEMM_PERSIST=0: one workgroup per 256 x 256 tile
    int gemm_prefetch;      // PB_GEMM_PREFETCH=0: a persistent workgroup issues a tile's prologue after the previous epilogue
    int resid_atomic;       // PB_RESID_ATOMIC=1: the residual epilogue adds with atomics
    int gemm_buffer;        // PB_GEMM_BUFFER=0: flat-addressed GEMM kernels only
    int halo;               // PB_HALO=0: the 64 -> 64 encoder convolutions run on the implicit GEMM
    int halo_dbg;           // PB_HALO_DBG=<n>: phase cycle stamps of n halo-conv launches
    int attn_variant;       // PB_ATTN_VARIANT: attention kernel variant where the caller asks for none
    int vol_abl;            // PB_VOL_ABL: ablations of the correlation-volume kernel (-DPB_DIAG builds only; wrong results)
    int cw3;                // PB_CW3=0: no packed-channel copy of 96-channel 3 x 3 weights
    int flow_host_pairs;    // PB_FLOW_HOST_PAIRS: pairs per chunk of a host-pointer flow call
    bool in_stats_lo;       // PB_IN_STATS_LO=1: instance-norm statistics include the residual part
    bool volume;            // PB_VOLUME=0: the correlation volume runs on the generic GEMM kernels
};
const LaunchEnv &launch_env();

struct StreamEnv {
    std::string cu_mask;    // comma-separated 32-bit hex words, empty = the whole device (engine_base.h pb_create_stream)
    int prio;               // -1 / 1: a higher- / lower-priority queue, 0 = default
};
struct CreateEnv {
    bool mx, mx_head;               // PB_MX: first digit 0 = no MX anywhere, second digit 0 = MX in the ViT only
    bool split_vit_w, split_head_a, split_head_w;      // PB_SPLIT=<vit_w><head_a><head_w>, three digits
    int tapin;                      // PB_TAPIN: -1 unset, 0 off, 2 also the encoders, 1 anything else
    int vit_res;                    // PB_VIT_RES: which ViT linears keep their weight residual (bit 0 qkv, 1 proj, 2 fc1, 3 fc2)
    int splitk_always;              // PB_SPLITK_ALWAYS=1: a split-K workspace for max_batch > 1 too
    int head_tail;                  // PB_HEAD_TAIL=0: the DPT head's last convolutions as separate launches
    int mask_sa;                    // PB_MASK_SA=0: mask band without split activations
    bool mx_upd;                    // PB_MX_UPD=0: RAFT update block on two fp16 passes
    bool convf1_direct;             // PB_CONVF1_DIRECT=0: convf1 through im2col + GEMM
    bool gru_hoist;                 // PB_GRU_HOIST=0: no context hoist
    int lo8_pow, a8_pow;            // PB_LO8_POW, PB_A8_POW: power-of-two storage scales of the e4m3 copies
    StreamEnv stream_depth, stream_flow;        // PB_CU_MASK_DEPTH / PB_CU_MASK_FLOW and their _PRIO
};
CreateEnv create_env();

struct BenchEnv {
    int gemm_abl;                   // PB_GEMM_ABL: timing-only epilogue ablations (wrong results)
    std::string gemm_dbg;           // PB_GEMM_DBG=<file>: per-block stamps of one launch, empty = none
};
BenchEnv bench_env();
