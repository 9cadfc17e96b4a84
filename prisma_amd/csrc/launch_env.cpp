// The one place that reads the environment (launch_env.h).  A switch keeps the parsing it had where it was first read, so two helpers:
// env_int treats an empty value as unset, env_atoi as 0.
#include "launch_env.h"

#include <stdlib.h>
#include <string.h>

namespace {

int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}
int env_atoi(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
bool env_first_is(const char *name, char c) {
    const char *e = getenv(name);
    return e && e[0] == c;
}
StreamEnv stream_env(const char *mask, const char *prio) {
    const char *e = getenv(mask);
    return StreamEnv{e ? e : "", env_int(prio, 0)};
}

LaunchEnv read_launch_env() {
    LaunchEnv v;
    v.gemm_stagger = env_atoi("PB_GEMM_STAGGER", -1);
    v.pixshuf_buf = env_int("PB_PIXSHUF_BUF", 1);
    v.tile_wide = env_atoi("PB_TILE_WIDE", 192);
    v.tile_n96 = env_int("PB_TILE_N96", 2);
    v.splitk = env_int("PB_SPLITK", 8);
    v.epi_report = env_int("PB_EPI_REPORT", 0);
    v.gemm_persist = env_int("PB_GEMM_PERSIST", 1);
    v.gemm_prefetch = env_int("PB_GEMM_PREFETCH", 1);
    v.resid_atomic = env_int("PB_RESID_ATOMIC", 0);
    v.gemm_buffer = env_atoi("PB_GEMM_BUFFER", 1);
    v.halo = env_atoi("PB_HALO", 1);
    v.halo_dbg = env_atoi("PB_HALO_DBG", 0);
    v.attn_variant = env_atoi("PB_ATTN_VARIANT", 0);
    v.vol_abl = env_int("PB_VOL_ABL", 0);
    v.cw3 = env_int("PB_CW3", 1);
    v.flow_host_pairs = env_int("PB_FLOW_HOST_PAIRS", 32);
    v.in_stats_lo = env_first_is("PB_IN_STATS_LO", '1');
    v.volume = !env_first_is("PB_VOLUME", '0');
    return v;
}

}  // namespace

const LaunchEnv &launch_env() {
    static const LaunchEnv v = read_launch_env();       // C++11: initialised once, by one thread, while the others wait
    return v;
}

CreateEnv create_env() {
    CreateEnv v;
    const char *mx = getenv("PB_MX");
    v.mx = !(mx && mx[0] == '0');
    v.mx_head = !(mx && (mx[0] == '0' || mx[1] == '0'));
    v.split_vit_w = v.split_head_a = v.split_head_w = true;
    const char *sp = getenv("PB_SPLIT");
    if (sp && strlen(sp) == 3) { v.split_vit_w = sp[0] == '1'; v.split_head_a = sp[1] == '1'; v.split_head_w = sp[2] == '1'; }
    const char *tin = getenv("PB_TAPIN");
    v.tapin = !tin ? -1 : tin[0] == '0' ? 0 : tin[0] == '2' ? 2 : 1;
    v.vit_res = env_int("PB_VIT_RES", 10);
    v.splitk_always = env_int("PB_SPLITK_ALWAYS", 0);
    v.head_tail = env_int("PB_HEAD_TAIL", 1);
    v.mask_sa = env_int("PB_MASK_SA", 1);
    v.mx_upd = !env_first_is("PB_MX_UPD", '0');
    v.convf1_direct = !env_first_is("PB_CONVF1_DIRECT", '0');
    v.gru_hoist = !env_first_is("PB_GRU_HOIST", '0');
    v.lo8_pow = env_int("PB_LO8_POW", 0);
    v.a8_pow = env_int("PB_A8_POW", 0);
    v.stream_depth = stream_env("PB_CU_MASK_DEPTH", "PB_CU_MASK_DEPTH_PRIO");
    v.stream_flow = stream_env("PB_CU_MASK_FLOW", "PB_CU_MASK_FLOW_PRIO");
    return v;
}

BenchEnv bench_env() {
    const char *dbg = getenv("PB_GEMM_DBG");
    return BenchEnv{env_int("PB_GEMM_ABL", 0), dbg ? dbg : ""};
}
