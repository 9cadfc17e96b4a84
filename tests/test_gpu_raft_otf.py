"""GPU: the flow_raft band with set_alternate_corr(True) - the lookup computed from the feature maps (csrc/corr_otf.hip), no all-pairs volume -
held to the bars of the default path (conftest.TOL[1] against the committed reference vectors), plus what a mode switch must guarantee:
results independent of the batch, the default path's bytes back after switching off, the arena smaller by the volume, flow_gmflow untouched."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import TOL
from prisma_amd import engine, synth

pytestmark = pytest.mark.gpu
TOL_RANGE, TOL_L2 = TOL[1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rell2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.fixture(scope="module")
def weights():
    return synth.raft_weights(seed=4321)


@pytest.fixture(scope="module")
def alt(weights):
    n = engine.FlowRaft(weights, device=0, precision=1)
    n.set_alternate_corr(True)
    yield n
    n.close()


@pytest.mark.parametrize("name", ["raft_125x157.npz", "raft_131x181.npz"])
def test_alternate_against_reference_vectors(alt, golden_dir, name):
    """fwd / bwd at the default path's tolerance; on 125x157 also the first lookup's output (corr0, every third channel).
    measured (relmax / relL2): 125x157 corr0 3.17e-4 / 2.10e-4, fwd 2.21e-4 / 1.78e-4, bwd 2.26e-4 / 1.67e-4; 131x181 fwd 2.33e-4 / 1.81e-4,
    bwd 3.13e-4 / 2.08e-4."""
    z = np.load(os.path.join(golden_dir, name))
    h, w = [int(v) for v in z["hw"]]
    fr = synth.frame_pair_sequence(2, h, w, seed=int(z["frame_seed"]))
    alt.set_profiling(timing=False, debug_stages=True)
    flow, _, _ = alt.infer_sequence(fr, scale=1.0, iters=int(z["iters"]), backward=True)
    alt.set_profiling(timing=False, debug_stages=False)
    if name == "raft_125x157.npz":
        corr0 = alt.stage("corr0")[:, ::3]
        print("\n  corr0/golden relmax %.3e relL2 %.3e" % (relmax(corr0, z["corr0"]), rell2(corr0, z["corr0"])), end="")
        assert relmax(corr0, z["corr0"]) < TOL_RANGE and rell2(corr0, z["corr0"]) < TOL_L2
    for k, got, ref in (("fwd", flow[0, 0], z["fwd"]), ("bwd", flow[0, 1], z["bwd"])):
        print("\n  %s %s/golden relmax %.3e relL2 %.3e" % (name, k, relmax(got, ref), rell2(got, ref)), end="")
        assert relmax(got, ref) < TOL_RANGE and rell2(got, ref) < TOL_L2, (name, k)


def test_alternate_batch_independence(alt):
    """a pair's flow does not depend on the pairs it shares a call with: 3 frames, both directions, against the two pairs on their own"""
    fr = synth.frame_pair_sequence(3, 128, 160, seed=11)
    both, _, _ = alt.infer_sequence(fr, scale=1.0, iters=4, backward=True, want_rgb=False)
    for i in range(2):
        one, _, _ = alt.infer_sequence(fr[i:i + 2], scale=1.0, iters=4, backward=True, want_rgb=False)
        assert np.array_equal(one[0].view(np.uint32), both[i].view(np.uint32)), "pair %d differs between a 2-pair and a 1-pair call" % i


def test_switch_hygiene_and_arena(weights):
    """off again = a fresh default context, byte for byte; with the mode on the arena is smaller by at least the volume:
    ND P sum_l ld_l 2 bytes (125x157, both directions: 2 x 409 600).
    measured: default 59 926 528 bytes, alternate 49 539 072 (the volume 819 200, the tiled B operands and their slack the rest)."""
    z_h, z_w = 125, 157
    fr = synth.frame_pair_sequence(2, z_h, z_w, seed=5)
    dflt = engine.FlowRaft(weights, device=0, precision=1)
    ctx = engine.FlowRaft(weights, device=0, precision=1)
    try:
        assert dflt.arena_bytes() == 0 and ctx.arena_bytes() == 0
        want, _, _ = dflt.infer_sequence(fr, scale=1.0, iters=3, backward=True, want_rgb=False)
        ctx.set_alternate_corr(True)
        on, _, _ = ctx.infer_sequence(fr, scale=1.0, iters=3, backward=True, want_rgb=False)
        bytes_on = ctx.arena_bytes()
        geo = engine.raft_geometry(16, 20)
        volume = 2 * (16 * 20) * sum(g["ld"] for g in geo) * 2
        assert volume == 2 * 409600
        print("\n  arena: default %d, alternate %d, volume %d" % (dflt.arena_bytes(), bytes_on, volume), end="")
        assert 0 < bytes_on <= dflt.arena_bytes() - volume
        assert relmax(on, want) < TOL_RANGE          # another rounding of the window entries, the same flow
        ctx.set_alternate_corr(False)
        off, _, _ = ctx.infer_sequence(fr, scale=1.0, iters=3, backward=True, want_rgb=False)
        assert np.array_equal(off.view(np.uint32), want.view(np.uint32))
        assert ctx.arena_bytes() == dflt.arena_bytes()
    finally:
        dflt.close()
        ctx.close()


def test_gmflow_context_refuses_and_is_unchanged():
    g = engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0, precision=1)
    try:
        fr = synth.frame_pair_sequence(2, 128, 160, seed=3)
        before, _, _ = g.infer_sequence(fr, scale=1.0, backward=True, want_rgb=False)
        with pytest.raises(Exception, match="flow_raft"):
            g.set_alternate_corr(True)
        after, _, _ = g.infer_sequence(fr, scale=1.0, backward=True, want_rgb=False)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    finally:
        g.close()


def test_band_cli_alternate_corr(tmp_path):
    """bands/flow_raft.py --alternate_corr -b --mask on the clip of tests/test_band_cli.py::test_flow_cli_video: the same files, shapes, CSV and
    metadata, and a smaller arena than a default run of the same command"""
    sys.path.insert(0, os.path.join(ROOT, "bands"))
    import flow_raft as band
    frames = synth.frame_pair_sequence(4, 176, 256, seed=6)
    os.environ["PRISMA_OVERWRITE"] = "1"
    arena = {}
    for mode, extra in (("alt", ["--alternate_corr"]), ("default", [])):
        folder = tmp_path / mode
        folder.mkdir()
        np.save(folder / "rgba.npy", frames)
        (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba.npy"}}}))
        band.model = None
        band.main(["-i", str(folder), "--iterations", "4", "--scale", "1.0", "-b", "--mask"] + extra)
        out = np.load(folder / "flow_raft.npy")
        assert out.shape == (4, 176, 256, 3) and out.dtype == np.uint8 and not out[-1].any() and out[0].any()
        assert np.load(folder / "flow_raft_bwd.npy").shape == out.shape
        m = np.load(folder / "flow_raft_mask.npy")
        assert m.shape == (4, 176, 256, 3) and set(np.unique(m)) <= {0, 255} and not m[-1].any()
        assert np.load(folder / "flow_raft_mask_bwd.npy").shape == m.shape
        dist = [float(x) for x in open(folder / "flow_raft.csv")]
        assert len(dist) == 4 and dist[-1] == 0.0 and all(d > 0 for d in dist[:-1])
        md = json.load(open(folder / "metadata.json"))
        assert md["bands"]["flow_raft"]["values"]["dist"] == {"type": "float", "url": "flow_raft.csv"}
        assert md["bands"]["flow_raft_bwd"]["url"] == "flow_raft_bwd.npy"
        assert md["bands"]["flow_raft_mask"]["url"] == "flow_raft_mask.npy"
        arena[mode] = band.model.arena_bytes()
        band.model.close()
        band.model = None
    assert 0 < arena["alt"] < arena["default"], arena
