"""GPU: the debug-stage registry every band shares (EngineBase::stages_ / snapshot / get_stage behind pb_*_get_stage and engine.*.stage()).
What a stage holds is the stagewise parity tests' business; these check the registry itself: snapshot buffers follow a plan that grows,
frame counts are those of the call (or chunk) that registered the stage, debug-only names vanish with the debug bit, and a refused query
leaves the context as it was.  Every comparison with a fresh context is bit for bit on what stage() returns."""
import numpy as np
import pytest

from prisma_amd import engine, synth
from prisma_amd._lib import PrismaBandsError

pytestmark = pytest.mark.gpu

DEPTH_CFG = synth.DEPTH_CFGS["vits"]
DEPTH_STAGES = ("tokens", "block0", f"block{DEPTH_CFG.depth - 1}", "feat3", "path4", "net_depth")
RAFT_STAGES = ("fmap", "net0", "corr0", "flow_it0", "flow_lo")
MASK_CFG = synth.MASK_CFGS["tiny"]


@pytest.fixture(scope="module")
def depth_w():
    return synth.depth_anything_weights(DEPTH_CFG, seed=1234)


@pytest.fixture(scope="module")
def raft_w():
    return synth.raft_weights(seed=4321)


@pytest.fixture(scope="module")
def mask_w():
    return synth.solov2_weights(MASK_CFG)


def depth_ctx(w, debug=True):
    net = engine.DepthAnything(w, DEPTH_CFG, device=0, max_batch=2)
    net.set_profiling(timing=False, debug_stages=debug)
    return net


def raft_ctx(w, debug=True):
    net = engine.FlowRaft(w, device=0, precision=1)
    net.set_profiling(timing=False, debug_stages=debug)
    return net


def raft_call(net, frames):
    return net.infer_sequence(frames, scale=1.0, iters=2, backward=True)


def unknown(net, name):
    with pytest.raises(PrismaBandsError, match="unknown stage"):
        net.stage(name)


def test_depth_snapshots_follow_the_plan(depth_w):
    """One context, three calls with a growing plan: more tokens per frame (90 x 160 after 128 x 128), then a larger batch.  The token
    snapshots ("tokens", "block<i>") are copies kept across calls, so each call needs the buffers at its own size."""
    calls = [synth.frames(1, 128, 128, seed=21), synth.frames(1, 90, 160, seed=22), synth.frames(2, 90, 160, seed=23)]
    net = depth_ctx(depth_w)
    for frames in calls:
        net.infer_batch(frames)
        got = {s: net.stage(s) for s in DEPTH_STAGES}
        fresh = depth_ctx(depth_w)
        fresh.infer_batch(frames)
        for s in DEPTH_STAGES:
            assert got[s].shape[0] == len(frames), (s, got[s].shape)
            assert np.array_equal(got[s], fresh.stage(s)), (s, len(frames), frames.shape)
        fresh.close()
    net.close()


def test_raft_snapshots_follow_the_plan(raft_w):
    small, large = synth.frame_pair_sequence(2, 128, 160, seed=31), synth.frame_pair_sequence(3, 136, 184, seed=32)
    net = raft_ctx(raft_w)
    raft_call(net, small)
    raft_call(net, large)
    got = {s: net.stage(s) for s in RAFT_STAGES}
    fresh = raft_ctx(raft_w)
    raft_call(fresh, large)
    for s in RAFT_STAGES:
        assert np.array_equal(got[s], fresh.stage(s)), s
    assert got["fmap"].shape[0] == 3                                          # frames
    assert got["net0"].shape[0] == 4 and got["flow_lo"].shape[0] == 4          # pairs x directions
    fresh.close()
    net.close()


def test_debug_only_stages_disappear_without_the_debug_bit(depth_w, raft_w):
    """A call with the debug bit registers the snapshots; the next call without it must not serve them (nor anything stale), while the
    stages that are views of the call's own buffers stay."""
    net = depth_ctx(depth_w)
    frames = synth.frames(1, 128, 128, seed=21)
    net.infer_batch(frames)
    assert net.stage("tokens").shape[0] == 1
    net.set_profiling(timing=False, debug_stages=False)
    net.infer_batch(frames)
    for s in ("tokens", "block0", "net0"):
        unknown(net, s)
    assert net.stage("net_depth").shape[0] == 1
    net.close()

    net = raft_ctx(raft_w)
    fr = synth.frame_pair_sequence(2, 128, 160, seed=31)
    raft_call(net, fr)
    assert net.stage("net0").shape[0] == 2
    net.set_profiling(timing=False, debug_stages=False)
    raft_call(net, fr)
    for s in ("net0", "corr0", "flow_it0", "tokens", "block0"):
        unknown(net, s)
    assert net.stage("flow_lo").shape[0] == 2
    net.close()

    # flow_gmflow shares EngineBase's registry and registers its own names only
    net = engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0, precision=1)
    net.set_profiling(timing=False, debug_stages=True)
    fr = synth.frame_pair_sequence(2, 120, 168, seed=33)
    net.infer_sequence(fr, scale=1.0, backward=True)
    assert net.stage("block0").shape[0] == 2
    net.set_profiling(timing=False, debug_stages=False)
    net.infer_sequence(fr, scale=1.0, backward=True)
    for s in ("block0", "tokens", "net0", "fmap", "flow_lo"):
        unknown(net, s)
    assert net.stage("flow_prop").shape[0] == 2
    net.close()


def _depth(w):
    net = depth_ctx(w)
    net.infer_batch(synth.frames(1, 96, 128, seed=41))
    return net, "feat3"                 # fp16 rows: converted through a device temporary


def _raft(w):
    net = raft_ctx(w)
    raft_call(net, synth.frame_pair_sequence(2, 128, 160, seed=42))
    return net, "fmap"                  # fp16 NHWC map


def _gmflow(_):
    net = engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0, precision=1)
    net.set_profiling(timing=False, debug_stages=True)
    net.infer_sequence(synth.frame_pair_sequence(2, 120, 168, seed=43), scale=1.0, backward=False)
    return net, "flow_prop"             # fp32 rows


def _mask(w):
    net = engine.MaskMMDet(w, MASK_CFG, max_batch=2)
    net.set_profiling(timing=False, debug_stages=True)
    net.infer_batch(synth.frames(1, 180, 300, seed=44))
    return net, "mask_feats"            # split fp16 map: hi + lo


SETUPS = {"depth": (_depth, "depth_w"), "raft": (_raft, "raft_w"), "gmflow": (_gmflow, None), "mask": (_mask, "mask_w")}


@pytest.mark.parametrize("band", list(SETUPS))
def test_refusals_leave_the_context_usable(band, request):
    make, weights = SETUPS[band]
    net, name = make(request.getfixturevalue(weights) if weights else None)
    before = net.stage(name)
    assert before.size > 16
    unknown(net, "no_such_stage")
    with pytest.raises(PrismaBandsError, match="stage buffer too small"):
        net.stage(name, cap=16)
    assert np.array_equal(net.stage(name), before)
    net.close()


def test_mask_stages_describe_the_last_chunk(mask_w):
    frames = synth.frames(3, 180, 300, seed=51)
    net = engine.MaskMMDet(mask_w, MASK_CFG, max_batch=2)            # 3 frames: chunks of 2 and 1
    net.set_profiling(timing=False, debug_stages=True)
    net.infer_batch(frames)
    got = {s: net.stage(s) for s in ("input", "c2", "p6", "mask_feats", "kernel_pred0", "cls_logit4")}
    for s, a in got.items():
        assert a.ndim == 4 and a.shape[0] == 1, (s, a.shape)
    one = engine.MaskMMDet(mask_w, MASK_CFG, max_batch=2)
    one.set_profiling(timing=False, debug_stages=True)
    one.infer_batch(frames[2:3])
    assert np.array_equal(got["input"][0], one.stage("input")[0])
    one.close()
    net.close()
