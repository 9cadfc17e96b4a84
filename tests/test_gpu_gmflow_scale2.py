"""GPU: the two-scale GMFlow (num_scales 2: the refinement model) through the C ABI - (a) every stage and the final flow, both directions,
against the vectors the REAL reference produced (tests/golden/gmflow_scale2_*.npz, tools/make_gmflow_scale2_golden.py), asserted at
conftest.TOL[1] (1e-3 of range, 1e-3 L2), the figure this band's other configurations are held to; (b) a pair's bytes do not depend on its
position in a sequence or on `backward`; masks and encode come through the unchanged tail; (c) refused radii / sizes leave the context
usable, pb_flow_num_scales, and a one-scale context after a two-scale one equals a fresh one.  3-frame sequences (frame 0 twice around
frame 1: pair 0 is the fixture's pair, pair 1 its reverse) where pairs are compared.

measured (MI355X), relmax of the worst stage / of the final flow fwd, bwd against the reference vectors at (4, 1):
  64x96   1.06e-4 (flow_match4) / 1.03e-4, 6.9e-5;  (2, 2): 9.3e-5 (flow_match4) / 6.1e-5
  96x160  8.2e-5 (flow_prop4) / 4.6e-5, 1.23e-4
  100x150 1.84e-4 (flow_prop4) / 1.93e-4, 1.75e-4
the whole table: EXPERIMENTS.md 6.12.  With the window attention's P and V as single fp16 (the one-scale model's setting) 64x96 measured
warp 2.5e-3, flow_match4 4.3e-3, bwd 3.9e-3: the warp turns the coarse flow's 5e-4 into several times that, so the two-scale model runs
its window attention with P and V split (gmflow_engine.hip blocks).
"""
import os

import numpy as np
import pytest

import gm_scale2_ref as S
from conftest import TOL
from prisma_amd import engine, synth

pytestmark = pytest.mark.gpu


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rell2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.fixture(scope="module")
def weights2():
    return synth.gmflow_weights(seed=2468, num_scales=2)


@pytest.fixture(scope="module")
def net(weights2):
    n = engine.FlowGMFlow(weights2, device=0, precision=1)
    yield n
    n.close()


def fixture_frames(z):
    h, w = [int(v) for v in z["hw"]]
    return synth.frame_pair_sequence(2, h, w, seed=int(z["frame_seed"]), shift=tuple(float(v) for v in z["frame_shift"]))


@pytest.mark.parametrize("hw", S.SIZES, ids=lambda v: "%dx%d" % v)
def test_stages_and_flow(net, golden_dir, hw):
    """every stage the engine names and the final flow of both directions at (4, 1) - and the forward flow with its fine-scale stages at
    (2, 2) where the fixture holds it - against the real model.  The engine's 128-channel stages are compared on the fixture's token subset.
    measured: worst stage 1.84e-4 (100x150 flow_prop4), worst final flow 1.93e-4 (100x150 fwd); bound 1e-3."""
    z = np.load(os.path.join(golden_dir, S.golden_name(hw)))
    fr = fixture_frames(z)
    h, w = hw
    Hp, Wp = S.padded(hw)
    P8, P4 = (Hp // 8) * (Wp // 8), (Hp // 4) * (Wp // 4)
    assert net.num_scales == 2
    net.set_matching(4, 1)
    net.set_profiling(timing=False, debug_stages=True)
    flow, rgb, mx = net.infer_sequence(fr, scale=1.0, backward=True)
    net.set_profiling(timing=False, debug_stages=False)
    assert flow.shape == (1, 2, h, w, 2) and rgb.shape == (1, 2, h, w, 3)
    shapes = dict(feat=(2, P8, 128), feat4=(2, P4, 128), tfeat=(2, P8, 128), flow_prop=(2, P8, 2), flow_up=(2, P4, 2), warp=(2, P4, 128),
                  block0_4=(4, P4, 128), tfeat4=(4, P4, 128), flow_match4=(2, P4, 2), flow_prop4=(2, P4, 2))
    print()
    errs = {}
    for name in S.STAGES:
        got, ref = net.stage(name), z[name + "_c4p1"]
        assert got.shape == shapes[name], (name, got.shape)
        if got.shape[-1] == 128:
            got = got[:, z["sub8" if got.shape[1] == P8 else "sub4"]]
        errs[name] = (relmax(got, ref), rell2(got, ref), float(np.abs(ref).max()))
    errs["fwd"] = (relmax(flow[0, 0], z["fwd_c4p1"]), rell2(flow[0, 0], z["fwd_c4p1"]), float(np.abs(z["fwd_c4p1"]).max()))
    errs["bwd"] = (relmax(flow[0, 1], z["bwd_c4p1"]), rell2(flow[0, 1], z["bwd_c4p1"]), float(np.abs(z["bwd_c4p1"]).max()))
    for cfg in S.CONFIGS[hw]:
        if cfg != (4, 1):
            tag = "_c%dp%d" % cfg
            net.set_matching(*cfg)
            f2, _, _ = net.infer_sequence(fr, scale=1.0, backward=False)
            for name, got in (("flow_match4", net.stage("flow_match4")), ("flow_prop4", net.stage("flow_prop4")), ("fwd", f2[0, 0])):
                ref = z[name + tag]
                errs[name + tag] = (relmax(got, ref), rell2(got, ref), float(np.abs(ref).max()))
            net.set_matching(4, 1)
    for k, (em, el, rg) in errs.items():
        print("  %dx%d %-16s relmax %.3e relL2 %.3e (range %.2f)" % (h, w, k, em, el, rg))
    bad = {k: v for k, v in errs.items() if v[0] > TOL[1][0] or v[1] > TOL[1][1]}
    assert not bad, bad
    ref = z["fwd_c4p1"]
    assert abs(float(mx[0, 0]) - float(np.sqrt((ref ** 2).sum(-1)).max())) < TOL[1][0] * float(np.abs(ref).max()) + 1e-4


def test_sequence_batching_directions_masks_and_encode(net, golden_dir):
    """a 3-frame sequence [a, c, a]: pair 0 is the 100 x 150 fixture's pair and pair 1 its reverse.  A pair's bytes do not depend on the
    sequence it is computed in nor on `backward`; pair 1's forward flow is pair 0's backward flow up to the encoder's batch order; the masks
    and the colour encode are those of the unchanged tail (the stand-alone consistency check on the same flows gives the same masks)."""
    z = np.load(os.path.join(golden_dir, S.golden_name((100, 150))))
    fr2 = fixture_frames(z)
    fr = np.stack([fr2[0], fr2[1], fr2[0]])
    net.set_matching(4, 1)
    f_all, rgb_all, m_all, mask_all = net.infer_sequence_masks(fr, scale=1.0)
    f_both, _, m_both = net.infer_sequence(fr, scale=1.0, backward=True)
    f_fwd, _, m_fwd = net.infer_sequence(fr, scale=1.0, backward=False)
    assert f_all.shape == (2, 2, 100, 150, 2) and f_fwd.shape == (2, 1, 100, 150, 2) and mask_all.shape[:2] == (2, 2)
    assert np.array_equal(f_all, f_both) and np.array_equal(m_all, m_both)
    for i in range(2):
        one, rgb1, m1 = net.infer_sequence(fr[i:i + 2], scale=1.0, backward=True)
        assert np.array_equal(one[0], f_all[i]) and np.array_equal(m1[0], m_all[i]) and np.array_equal(rgb1[0], rgb_all[i])
        assert np.array_equal(f_fwd[i, 0], f_all[i, 0]) and m_fwd[i, 0] == m_all[i, 0]
    assert relmax(f_all[1, 0], f_all[0, 1]) < 1e-5 and relmax(f_all[0, 0], z["fwd_c4p1"]) <= TOL[1][0]
    assert np.array_equal(np.asarray(mask_all).astype(bool), np.asarray(net.fwdbwd_mask(f_all)).astype(bool))
    assert rgb_all.dtype == np.uint8 and rgb_all[0, 0].any() and mask_all.any() and not mask_all.all()


def test_refusals_leave_the_context_usable_and_num_scales(net, weights2):
    fr = synth.frame_pair_sequence(3, 72, 104, seed=12, shift=(3.0, 2.0))
    net.set_matching(4, 1)
    net.set_inference_size(None)
    want = net.infer_sequence(fr, scale=1.0, backward=True)
    for bad in ((-1, 1), (4, -1), (-1, -1), (5, 1), (0, 1), (4, 3)):
        with pytest.raises(engine._lib.PrismaBandsError, match="radius_list"):
            net.set_matching(*bad)
    for bad in ((48, 64), (64, 80), (32, 64), (64, 100)):
        with pytest.raises(engine._lib.PrismaBandsError, match="multiples of 32"):
            net.set_inference_size(bad)
    again = net.infer_sequence(fr, scale=1.0, backward=True)
    for a, b in zip(again, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    net.set_inference_size((64, 96))                                            # a good size works, and going back gives the same bytes
    sized = net.infer_sequence(fr, scale=1.0, backward=True)
    assert sized[0].shape == want[0].shape and np.isfinite(sized[0]).all() and not np.array_equal(sized[0], want[0])
    net.set_inference_size(None)
    net.set_matching(2, 2)
    other = net.infer_sequence(fr, scale=1.0, backward=True)
    assert not np.array_equal(other[0], want[0])
    net.set_matching(4, 1)
    for a, b in zip(net.infer_sequence(fr, scale=1.0, backward=True), want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    with pytest.raises(engine._lib.PrismaBandsError, match="too small"):
        net.infer_sequence(synth.frame_pair_sequence(2, 32, 96, seed=3), scale=1.0, backward=False)
    # pb_flow_num_scales: 2, 1, and an error on another band
    assert net.num_scales == 2
    one = engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0, precision=1)
    assert one.num_scales == 1
    one.close()
    raft = engine.FlowRaft(synth.raft_weights(seed=4321), device=0)
    with pytest.raises(engine._lib.PrismaBandsError, match="flow_gmflow"):
        engine.check(raft.lib.pb_flow_num_scales(raft.ctx))
    raft.close()
    # a state dict that is neither model names the tensor
    mixed = dict(weights2)
    mixed["upsampler.2.weight"] = synth.gmflow_weights(seed=2468)["upsampler.2.weight"]
    mixed["upsampler.2.bias"] = synth.gmflow_weights(seed=2468)["upsampler.2.bias"]
    with pytest.raises(engine._lib.PrismaBandsError, match="upsampler.2.weight"):
        engine.FlowGMFlow(mixed, device=0, precision=1)
    mixed = dict(weights2)
    del mixed["backbone.trident_conv.weight"]
    with pytest.raises(engine._lib.PrismaBandsError, match="upsampler.2.weight"):
        engine.FlowGMFlow(mixed, device=0, precision=1)


def test_one_scale_context_after_a_two_scale_one_equals_a_fresh_one(net, golden_dir):
    """two one-scale contexts, each created and run after the two-scale one has run in the same process (same streams and allocator
    history), give the same bytes as each other (array_equal; global and (4, 1) radii), and the first of them is within the band's bound
    of the real one-scale model's flow on the one-scale fixture's pair (tests/golden/gmflow_125x157.npz, both directions).  That the
    one-scale bytes equal the previous commit's is a measurement of two builds (EXPERIMENTS.md 6.12), not something one build can assert."""
    z = np.load(os.path.join(golden_dir, "gmflow_125x157.npz"))
    h, w = [int(v) for v in z["hw"]]
    fr1 = synth.frame_pair_sequence(2, h, w, seed=int(z["frame_seed"]))
    fr = synth.frame_pair_sequence(3, 120, 168, seed=9)
    net.set_matching(4, 1)
    net.infer_sequence(fr, scale=1.0, backward=True)
    w1 = synth.gmflow_weights(seed=2468)
    outs = []
    for _ in range(2):
        one = engine.FlowGMFlow(w1, device=0, precision=1)
        if not outs:
            flow = one.infer_sequence(fr1, scale=1.0, backward=True)[0]
            for k, got in (("fwd", flow[0, 0]), ("bwd", flow[0, 1])):
                print("\n  one-scale after two-scale %s relmax %.3e relL2 %.3e" % (k, relmax(got, z[k]), rell2(got, z[k])), end="")
                assert relmax(got, z[k]) < TOL[1][0] and rell2(got, z[k]) < TOL[1][1], k
        outs.append(one.infer_sequence(fr, scale=1.0, backward=True))
        one.set_matching(4, 1)
        outs.append(one.infer_sequence(fr, scale=1.0, backward=True))
        one.close()
        net.infer_sequence(fr[:2], scale=1.0, backward=False)               # the two-scale context runs in between
    for a, b in zip(outs[0] + outs[1], outs[2] + outs[3]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert not np.array_equal(outs[0][0], outs[1][0])
