"""CPU: the index arithmetic of flow_raft's correlation-volume layouts (prisma_amd/csrc/corr_layout.h - the very text volume.hip's stores,
corr_lookup_blocked_kernel's loads and the host de-blocking compile) built with g++: the blocked layout is a bijection of the P8 x pld entries
of a level (P8 = P rounded up to 8 rows) onto [0, P8 * pld), a group's eight copies of a target tile are 1 KB contiguous in source-row order,
and the row-major layout is the plain p * pld + c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "corr_layout.h"
int main(int argc, char **argv) {       // P pld: prints "ok" or the first violation
    const int P = atoi(argv[1]), pld = atoi(argv[2]), T = pld / 64;
    const long long P8 = corr_layout_rows(CORR_BLOCKED, P), total = P8 * pld;
    if (P8 % 8 || P8 < P || P8 >= P + 8 || corr_layout_rows(CORR_ROWMAJOR, P) != P) { printf("rows %lld of %d\n", P8, P); return 0; }
    std::vector<unsigned char> seen((size_t)total, 0);
    for (int p = 0; p < (int)P8; ++p)
        for (int c = 0; c < pld; ++c) {
            const long long i = corr_layout_index(CORR_BLOCKED, p, c, pld);
            if (i < 0 || i >= total || seen[(size_t)i]) { printf("entry (%d, %d) -> %lld: outside or taken\n", p, c, i); return 0; }
            seen[(size_t)i] = 1;
            if (corr_layout_index(CORR_ROWMAJOR, p, c, pld) != (long long)p * pld + c) { printf("row-major (%d, %d)\n", p, c); return 0; }
            // the issue's formula, and the run: entry e of tile j of rows 8 b .. 8 b + 7 at tile start + (p & 7) * 64 + e
            if (i != ((long long)(p >> 3) * T + (c >> 6)) * 512 + (p & 7) * 64 + (c & 63)) { printf("formula (%d, %d) -> %lld\n", p, c, i); return 0; }
            if (i != corr_blocked_tile(p >> 3, c >> 6, T) + (p & 7) * 64 + (c & 63)) { printf("tile start (%d, %d)\n", p, c); return 0; }
        }
    for (int b = 0; b < (int)(P8 / 8); ++b)
        for (int j = 0; j < T; ++j) {
            const long long t0 = corr_blocked_tile(b, j, T);
            if (t0 % 512) { printf("tile (%d, %d) starts at %lld: not 1 KB aligned\n", b, j, t0); return 0; }
            for (int q = 0; q < 8; ++q)
                for (int e = 0; e < 64; ++e)
                    if (corr_layout_index(CORR_BLOCKED, b * 8 + q, j * 64 + e, pld) != t0 + q * 64 + e) { printf("run (%d, %d, %d, %d)\n", b, j, q, e); return 0; }
        }
    printf("ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("corr_layout")
    src = d / "layout.cpp"
    src.write_text(SRC)
    out = d / "layout"
    subprocess.run(["g++", "-O1", "-I", os.path.join(ROOT, "prisma_amd", "csrc"), str(src), "-o", str(out)], check=True)
    return str(out)


# P = 256: whole groups; 391 = 17 x 23: a partial last group; 18360 = 102 x 180 (1080p x 0.75).  pld: one tile, the 17 x 23 grid's levels 0 and 1
# (448, 192), an odd number of tiles; the 18360-row level is checked at a short row (its 19200-entry one is 350 M entries - the arithmetic
# is linear in T)
@pytest.mark.parametrize("P,pld", [(256, 256), (256, 64), (391, 448), (391, 192), (391, 64), (18360, 192), (18360, 320), (1, 64), (8, 128), (9, 128)])
def test_blocked_index_is_a_bijection_with_contiguous_tile_copies(exe, P, pld):
    r = subprocess.run([exe, str(P), str(pld)], capture_output=True, text=True, check=True)
    assert r.stdout.strip() == "ok", (P, pld, r.stdout)
