"""CPU: how many pairs a host-pointer flow call hands to one RaftEngine::infer (prisma_amd/csrc/flow_chunk.h - the text abi.hip compiles) built
with g++ and held against a brute-force loop over cp; and the flow_raft band's --alternate_corr plumbing with a recording stand-in for the
engine."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "flow_chunk.h"
int main(int argc, char **argv) {
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


def grid(h, w, scale):
    sh, sw = round(h * scale), round(w * scale)
    return -(-sh // 8) * -(-sw // 8)


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
    P = grid(1080, 1920, 0.75)
    assert P == 102 * 180
    assert run(16, 2, P, 576) == 16 and run(32, 2, P, 576) == 32 and run(31, 1, P, 576) == 31
    # 2160p x 1.0, both directions: 2 x 129600 x 576 halfs per pair -> 14 pairs at most (15 would be 2.24e9 >= 2^31)
    P4 = grid(2160, 3840, 1.0)
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
