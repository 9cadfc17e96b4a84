"""CPU: the environment switches of the library (prisma_amd/csrc/launch_env.{h,cpp} - the text the library links) built with g++ behind a
small main and run as a child: defaults and parsing against the table of DESIGN.md section 12, the lifetimes (launch_env() once per process,
create_env() at every call), first calls of launch_env() from eight threads, and that no other file of csrc reads the environment."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prisma_amd", "csrc")

# one line per switch, keyed by its name, in a spelling that can be fed back as the variable's value ("unset" / "empty" where there is none)
SRC = r"""
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "launch_env.h"
static const char *str(const std::string &s) { return s.empty() ? "empty" : s.c_str(); }
static void print_launch(const LaunchEnv &e) {
    printf("PB_GEMM_STAGGER=%d\nPB_PIXSHUF_BUF=%d\nPB_TILE_WIDE=%d\nPB_TILE_N96=%d\nPB_SPLITK=%d\nPB_EPI_REPORT=%d\n", e.gemm_stagger, e.pixshuf_buf,
           e.tile_wide, e.tile_n96, e.splitk, e.epi_report);
    printf("PB_GEMM_PERSIST=%d\nPB_GEMM_PREFETCH=%d\nPB_RESID_ATOMIC=%d\nPB_GEMM_BUFFER=%d\nPB_HALO=%d\nPB_HALO_DBG=%d\n", e.gemm_persist,
           e.gemm_prefetch, e.resid_atomic, e.gemm_buffer, e.halo, e.halo_dbg);
    printf("PB_ATTN_VARIANT=%d\nPB_VOL_ABL=%d\nPB_CW3=%d\nPB_FLOW_HOST_PAIRS=%d\nPB_IN_STATS_LO=%d\nPB_VOLUME=%d\n", e.attn_variant, e.vol_abl, e.cw3,
           e.flow_host_pairs, (int)e.in_stats_lo, (int)e.volume);
}
static void print_create(const CreateEnv &e) {
    printf("PB_MX=%d%d\nPB_SPLIT=%d%d%d\n", (int)e.mx, (int)e.mx_head, (int)e.split_vit_w, (int)e.split_head_a, (int)e.split_head_w);
    if (e.tapin < 0) printf("PB_TAPIN=unset\n");
    else printf("PB_TAPIN=%d\n", e.tapin);
    printf("PB_VIT_RES=%d\nPB_SPLITK_ALWAYS=%d\nPB_HEAD_TAIL=%d\nPB_MASK_SA=%d\nPB_MX_UPD=%d\nPB_CONVF1_DIRECT=%d\nPB_GRU_HOIST=%d\n", e.vit_res,
           e.splitk_always, e.head_tail, e.mask_sa, (int)e.mx_upd, (int)e.convf1_direct, (int)e.gru_hoist);
    printf("PB_LO8_POW=%d\nPB_A8_POW=%d\n", e.lo8_pow, e.a8_pow);
    printf("PB_CU_MASK_DEPTH=%s\nPB_CU_MASK_DEPTH_PRIO=%d\nPB_CU_MASK_FLOW=%s\nPB_CU_MASK_FLOW_PRIO=%d\n", str(e.stream_depth.cu_mask), e.stream_depth.prio,
           str(e.stream_flow.cu_mask), e.stream_flow.prio);
}
int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "print";
    if (!strcmp(mode, "print")) {
        print_launch(launch_env());
        print_create(create_env());
        const BenchEnv b = bench_env();
        printf("PB_GEMM_ABL=%d\nPB_GEMM_DBG=%s\n", b.gemm_abl, str(b.gemm_dbg));
    } else if (!strcmp(mode, "setenv")) {
        const LaunchEnv *a0 = &launch_env();
        const CreateEnv c0 = create_env();
        printf("before: splitk %d mx_upd %d a8_pow %d\n", a0->splitk, (int)c0.mx_upd, c0.a8_pow);
        setenv("PB_SPLITK", "3", 1); setenv("PB_MX_UPD", "0", 1); setenv("PB_A8_POW", "4", 1);
        const LaunchEnv *a1 = &launch_env();
        const CreateEnv c1 = create_env();
        printf("after: splitk %d mx_upd %d a8_pow %d same %d\n", a1->splitk, (int)c1.mx_upd, c1.a8_pow, (int)(a0 == a1));
    } else {                    // "threads": eight first calls released together
        const int n = 8;
        std::atomic<int> ready{0};
        std::atomic<bool> go{false};
        std::vector<const LaunchEnv *> addr(n);
        std::vector<LaunchEnv> val(n);
        std::vector<std::thread> th;
        for (int i = 0; i < n; ++i)
            th.emplace_back([&, i] {
                ready.fetch_add(1);
                while (!go.load()) {}
                addr[i] = &launch_env();
                val[i] = *addr[i];
            });
        while (ready.load() < n) {}
        go.store(true);
        for (auto &t : th) t.join();
        int same_addr = 0, same_val = 0;
        for (int i = 0; i < n; ++i) {
            same_addr += addr[i] == addr[0];
            same_val += val[i].splitk == val[0].splitk && val[i].tile_wide == val[0].tile_wide && val[i].volume == val[0].volume &&
                        val[i].gemm_stagger == val[0].gemm_stagger && val[i].flow_host_pairs == val[0].flow_host_pairs;
        }
        printf("threads %d same_addr %d same_val %d splitk %d tile_wide %d\n", n, same_addr, same_val, val[0].splitk, val[0].tile_wide);
    }
    return 0;
}
"""

# every switch at a value that is not its default and that the program prints back as given
NON_DEFAULT = {
    "PB_GEMM_STAGGER": "25", "PB_PIXSHUF_BUF": "0", "PB_TILE_WIDE": "0", "PB_TILE_N96": "1", "PB_SPLITK": "4", "PB_EPI_REPORT": "1",
    "PB_GEMM_PERSIST": "0", "PB_GEMM_PREFETCH": "0", "PB_RESID_ATOMIC": "1", "PB_GEMM_BUFFER": "0", "PB_HALO": "0", "PB_HALO_DBG": "2",
    "PB_ATTN_VARIANT": "2", "PB_VOL_ABL": "5", "PB_CW3": "0", "PB_FLOW_HOST_PAIRS": "16", "PB_IN_STATS_LO": "1", "PB_VOLUME": "0",
    "PB_MX": "10", "PB_SPLIT": "010", "PB_TAPIN": "2", "PB_VIT_RES": "15", "PB_SPLITK_ALWAYS": "1", "PB_HEAD_TAIL": "0", "PB_MASK_SA": "0",
    "PB_MX_UPD": "0", "PB_CONVF1_DIRECT": "0", "PB_GRU_HOIST": "0", "PB_LO8_POW": "3", "PB_A8_POW": "4",
    "PB_CU_MASK_DEPTH": "0f0f0f0f,0f0f0f0f", "PB_CU_MASK_DEPTH_PRIO": "-1", "PB_CU_MASK_FLOW": "f0f0f0f0", "PB_CU_MASK_FLOW_PRIO": "1",
    "PB_GEMM_ABL": "2", "PB_GEMM_DBG": "stamps.out",
}


def design_table():
    """{name: (default, lifetime)} from the rows `| \\`PB_X\\` | \\`default\\` | lifetime | ...` of DESIGN.md"""
    rows = {}
    for line in open(os.path.join(ROOT, "DESIGN.md")):
        m = re.match(r"\| `(PB_[A-Z0-9_]+)` \| `([^`]*)` \| (launch|create|per call) \|", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_env")
    src = d / "main.cpp"
    src.write_text(SRC)
    out = d / "launch_env"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", CSRC, str(src), os.path.join(CSRC, "launch_env.cpp"), "-o", str(out)],
                   check=True)
    return str(out)


def run(exe, mode, env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PB_")}
    clean.update(env)
    return subprocess.run([exe, mode], check=True, capture_output=True, text=True, env=clean).stdout


def printed(out):
    return dict(line.split("=", 1) for line in out.splitlines())


def test_defaults_are_the_design_table(exe):
    table = design_table()
    got = printed(run(exe, "print", {}))
    assert set(got) == set(table)
    for name, (default, _) in table.items():
        assert got[name] == default, (name, got[name], default)


def test_every_switch_is_read(exe):
    table = design_table()
    assert set(NON_DEFAULT) == set(table)
    for name, v in NON_DEFAULT.items():
        assert v != table[name][0], name
    got = printed(run(exe, "print", NON_DEFAULT))
    assert got == NON_DEFAULT
    # the parsing the launchers had: an empty value is 0 for the switches once read with atoi, the default for the others
    got = printed(run(exe, "print", {"PB_GEMM_BUFFER": "", "PB_SPLITK": "", "PB_TAPIN": "0", "PB_MX": "0", "PB_SPLIT": "01"}))
    assert (got["PB_GEMM_BUFFER"], got["PB_SPLITK"], got["PB_TAPIN"], got["PB_MX"], got["PB_SPLIT"]) == ("0", "8", "0", "00", "111")


def test_create_env_follows_setenv_launch_env_does_not(exe):
    out = run(exe, "setenv", {}).splitlines()
    assert out == ["before: splitk 8 mx_upd 1 a8_pow 0", "after: splitk 8 mx_upd 0 a8_pow 4 same 1"]


def test_first_calls_from_eight_threads_agree(exe):
    assert run(exe, "threads", {"PB_SPLITK": "5", "PB_TILE_WIDE": "128"}).strip() == "threads 8 same_addr 8 same_val 8 splitk 5 tile_wide 128"


def test_only_the_module_reads_the_environment():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, f)
        if not os.path.isfile(path):
            continue
        text = open(path, errors="replace").read()
        if f == "launch_env.cpp":
            names = set(re.findall(r'"(PB_[A-Z0-9_]+)"', text))
            continue
        assert "getenv(" not in text and "pb_env_int(" not in text, f
    assert names == set(design_table())
