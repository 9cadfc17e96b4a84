"""CPU: the host-compilable pieces of the flow engines (prisma_amd/csrc/flow_chunk.h - the text the engines and abi.hip compile) built with g++:
how many pairs a host-pointer flow call hands to one FlowEngine::infer, held against a brute-force loop over cp, and the padded geometry of a
call, held against a brute-force padder; and the flow_raft band's --alternate_corr plumbing with a recording stand-in for the engine."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "flow_chunk.h"
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "geo")) {          // geo H W scale factor ...: one line of sh sw Hp Wp padl padt h8 w8 P per case
        for (int i = 2; i + 3 < argc; i += 4) {
            const FlowGeometry g = flow_geometry(atoi(argv[i]), atoi(argv[i + 1]), (float)atof(argv[i + 2]), atoi(argv[i + 3]));
            printf("%d %d %d %d %d %d %d %d %d\n", g.sh, g.sw, g.Hp, g.Wp, g.padl, g.padt, g.h8, g.w8, g.P);
        }
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "exact")) {        // exact scale ...: flow_scale_exact of every scale, narrowed to float as the C ABI carries it
        for (int i = 2; i < argc; ++i) printf("%.17g\n", flow_scale_exact((float)atof(argv[i])));
        return 0;
    }
    for (int i = 1; i + 3 < argc; i += 4)
        printf("%d\n", flow_chunk_pairs(atoi(argv[i]), atoi(argv[i + 1]), atoll(argv[i + 2]), atoll(argv[i + 3])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("flow_chunk")
    src = d / "chunk.cpp"
    src.write_text(SRC)
    out = d / "chunk"
    subprocess.run(["g++", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "prisma_amd", "csrc"), str(src), "-o", str(out)], check=True)
    return str(out)


def brute(wanted, dirs, P, Lhx):
    best = 0
    for cp in range(1, wanted + 1):
        if cp * dirs * P * Lhx < 2 ** 31:
            best = cp
    return best


GEO = ("sh", "sw", "Hp", "Wp", "padl", "padt", "h8", "w8", "P")


def geometry(exe, cases):
    """flow_geometry of every (H, W, scale, factor), as dicts over GEO"""
    out = subprocess.run([exe, "geo"] + [repr(v) for c in cases for v in c], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    return [dict(zip(GEO, map(int, line.split()))) for line in out]


def grid(exe, h, w, scale):
    """tokens of RAFT's 1/8 grid (padding factor 8) as the compiled flow_geometry gives them"""
    return geometry(exe, [(h, w, scale, 8)])[0]["P"]


def pad_brute(size, factor):
    """InputPadder: the smallest multiple of factor that is at least size; the smaller half of the padding goes left / top"""
    m = size
    while m % factor:
        m += 1
    return m, (m - size) // 2


# (H, W, scale, factor) and the scaled size it gives: the two ragged sizes of the GPU tests at RAFT's factor, the bench's 810 x 1440 at every
# factor, and a size that is a multiple of 32 already (plain and through a scale)
GEO_CASES = [((125, 157, 1.0, 8), (125, 157)), ((131, 181, 1.0, 8), (131, 181)), ((1080, 1920, 0.75, 8), (810, 1440)),
             ((1080, 1920, 0.75, 16), (810, 1440)), ((1080, 1920, 0.75, 32), (810, 1440)), ((96, 128, 1.0, 8), (96, 128)),
             ((96, 128, 1.0, 16), (96, 128)), ((96, 128, 1.0, 32), (96, 128)), ((192, 256, 0.5, 32), (96, 128))]


def test_flow_geometry_against_brute_force_padder(exe):
    got = geometry(exe, [c for c, _ in GEO_CASES])
    for (case, (sh, sw)), g in zip(GEO_CASES, got):
        factor = case[3]
        Hp, padt = pad_brute(sh, factor)
        Wp, padl = pad_brute(sw, factor)
        want = dict(sh=sh, sw=sw, Hp=Hp, Wp=Wp, padl=padl, padt=padt, h8=Hp // 8, w8=Wp // 8, P=(Hp // 8) * (Wp // 8))
        assert g == want, (case, g, want)
    # the ragged grids the GPU tests run on, and no padding where the size is a multiple of the factor already
    assert (got[0]["h8"], got[0]["w8"]) == (16, 20) and (got[1]["h8"], got[1]["w8"]) == (17, 23)
    assert all(g["Hp"] == 96 and g["Wp"] == 128 and g["padl"] == 0 and g["padt"] == 0 for g in got[5:])


def test_scale_exact_is_the_double_the_caller_typed(exe):
    """the C ABI carries --scale as a float, the reference computes with Python's double: flow_scale_exact gives that double back - for every
    scale of EXPERIMENTS 6.30's table, for two- to seven-digit literals, and unchanged where the float is the number itself (dyadic scales)"""
    scales = [0.75, 0.5, 0.25, 0.4, 0.8, 1.25, 1.5, 0.6, 0.3, 0.9, 0.7, 0.35, 1.0, 2.0, 0.1, 0.05, 0.333, 0.6667, 1.23456, 0.1234567, 3.0, 0.0625]
    out = subprocess.run([exe, "exact"] + [repr(s) for s in scales], check=True, capture_output=True, text=True).stdout.split()
    assert [float(o) for o in out] == scales
    # plain arithmetic (no text, no locale): held against numpy's shortest round-trip decimal of the float on 4000 literals of 1 - 7 digits
    # between 1e-3 and 1e3, and against the widened float where the helper steps aside
    import numpy as np
    g = np.random.default_rng(3)
    lits = [float("%.*e" % (int(d), v)) for d, v in zip(g.integers(0, 7, 4000), 10.0 ** g.uniform(-3, 3, 4000))]
    out = subprocess.run([exe, "exact"] + [repr(v) for v in lits], check=True, capture_output=True, text=True).stdout.split()
    want = [float(np.format_float_positional(np.float32(v), unique=True)) for v in lits]
    assert [float(o) for o in out] == want == lits
    out = subprocess.run([exe, "exact", "1e-20", "3e15"], check=True, capture_output=True, text=True).stdout.split()
    assert [float(o) for o in out] == [float(np.float32(1e-20)), float(np.float32(3e15))]
    import struct
    widened = lambda s: struct.unpack("f", struct.pack("f", s))[0]
    assert all(widened(s) == s for s in (0.75, 0.5, 1.0)) and all(widened(s) != s for s in (0.6, 0.3, 0.9, 0.7, 0.35))
    # sizes the widened float gets wrong - the double's products are half-even ties (4.5, 10.5, 3.5, 17.5), the widened float's fall beside
    # them - and a tie of a dyadic scale
    got = geometry(exe, [(15, 35, 0.3, 8), (5, 25, 0.7, 8), (2, 6, 0.75, 8)])
    assert [(g["sh"], g["sw"]) for g in got] == [(4, 10), (4, 18), (2, 4)]
    assert [(round(15 * widened(0.3)), round(35 * widened(0.3))), (round(5 * widened(0.7)), round(25 * widened(0.7)))] == [(5, 11), (3, 17)]


def test_chunk_pairs_against_brute_force(exe):
    cases = []
    for wanted in (1, 2, 7, 16, 31, 32, 40):
        for dirs in (1, 2):
            for P in (16 * 16, 16 * 20, 102 * 180, 135 * 240, 270 * 480, 271 * 481, 2 ** 20, 2 ** 22, 3728270, 3728271):
                for Lhx in (384, 576):
                    cases.append((wanted, dirs, P, Lhx))
    out = subprocess.run([exe] + [str(v) for c in cases for v in c], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(cases)
    for c, o in zip(cases, out):
        assert int(o) == brute(*c), (c, o)


def test_chunk_pairs_named_cases(exe):
    run = lambda *a: int(subprocess.run([exe] + [str(v) for v in a], check=True, capture_output=True, text=True).stdout)
    # a chunk that fits is left alone: the band's 16 pairs (and the pipeline's 32) at 1080p x 0.75, both directions
    P = grid(exe, 1080, 1920, 0.75)
    assert P == 102 * 180
    assert run(16, 2, P, 576) == 16 and run(32, 2, P, 576) == 32 and run(31, 1, P, 576) == 31
    # 2160p x 1.0, both directions: 2 x 129600 x 576 halfs per pair -> 14 pairs at most (15 would be 2.24e9 >= 2^31)
    P4 = grid(exe, 2160, 3840, 1.0)
    assert P4 == 270 * 480
    assert run(16, 2, P4, 576) == 14 and run(32, 2, P4, 576) == 14 and run(32, 1, P4, 576) == 28 and run(8, 2, P4, 576) == 8
    assert 14 * 2 * P4 * 576 < 2 ** 31 <= 15 * 2 * P4 * 576
    # a single pair that is too large has no chunk: 0, and the engine refuses the call itself
    assert run(16, 2, 2 ** 21, 576) == 0 and run(1, 1, 3728271, 576) == 0 and run(1, 1, 3728270, 576) == 1
    assert run(0, 2, P, 576) == 0


class FakeRaft:
    calls = []

    def __init__(self, weights, device=0, precision=None):
        FakeRaft.calls.append(("init", device))

    def set_alternate_corr(self, on=True):
        FakeRaft.calls.append(("set_alternate_corr", on))


@pytest.mark.parametrize("flag", [True, False])
def test_band_alternate_corr_reaches_the_engine(monkeypatch, tmp_path, capsys, flag):
    sys.path.insert(0, os.path.join(ROOT, "bands"))
    import flow_raft as band
    from prisma_amd import engine
    FakeRaft.calls = []
    monkeypatch.setattr(engine, "FlowRaft", FakeRaft)
    monkeypatch.setattr(band, "load_weights", lambda path: {})
    monkeypatch.setattr(band, "process_video", lambda args: None)
    monkeypatch.setattr(band, "model", None)
    monkeypatch.setenv("PRISMA_OVERWRITE", "1")
    clip = tmp_path / "clip.mp4"
    clip.write_bytes(b"")
    band.main(["-i", str(clip), "-o", str(tmp_path / "out.mp4")] + (["--alternate_corr"] if flag else []))
    err = capsys.readouterr().err
    if flag:
        assert FakeRaft.calls == [("init", 0), ("set_alternate_corr", True)]
        assert "--alternate_corr" in err and "ignored" not in err
    else:
        assert FakeRaft.calls == [("init", 0)]
        assert "alternate_corr" not in err
    assert isinstance(band.model, FakeRaft)
