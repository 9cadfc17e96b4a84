"""CPU: the float64 restatements of the two-scale GMFlow's new steps (tests/gm_scale2_ref.py) against the REAL reference's vectors
(tests/golden/gmflow_scale2_*.npz, tools/make_gmflow_scale2_golden.py) to 1e-4 of every tensor's range - a tenth of the band's 1e-3, so the
yardstick cannot eat the budget -, every planted fault seen by a wide margin, the conditions that keep the fixture from passing with the
fine scale idle, and the synthetic weights of the two models."""
import os

import numpy as np
import pytest

import gm_ref as R
import gm_scale2_ref as S
from prisma_amd import synth

YARD = 1e-4
FAULT = 1e-2          # a planted fault moves its stage by at least 100 x the yardstick


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def ops(golden_dir):
    return np.load(os.path.join(golden_dir, "gmflow_scale2_ops.npz"))


@pytest.fixture(scope="module")
def weights2():
    return synth.gmflow_weights(seed=2468, num_scales=2)


_RUNS = {}


def reference_run(golden_dir, weights2, hw, cfg=(4, 1), swapped=False, bug=None):
    """forward() of one fixture's pair, computed once per (size, radii, direction, fault) and shared between the tests"""
    key = (tuple(hw), cfg, swapped, bug)
    if key not in _RUNS:
        z = np.load(os.path.join(golden_dir, S.golden_name(hw)))
        fr = synth.frame_pair_sequence(2, hw[0], hw[1], seed=int(z["frame_seed"]), shift=tuple(float(v) for v in z["frame_shift"]))
        a, c, pad = S.pad_pair(fr)
        up, st = S.forward(weights2, c if swapped else a, a if swapped else c, cfg[0], cfg[1], bug=bug)
        _RUNS[key] = (S.unpad(up, pad), st, z)
    return _RUNS[key]


def stage_of(z, name, st, b):
    """(the fixture's tensor of batch element b, the same tokens of a forward() stage of ONE direction)"""
    ref = z[name + "_c4p1"]
    got = st[name]
    per = got.shape[0]                                   # images of one direction: 2 for the streams, 1 for the flows and the warp
    if name in ("feat", "feat4", "tfeat"):               # frames (the coarse scale runs one sample for both directions), not batch elements
        ref = ref[::-1] if b else ref
    else:
        ref = ref[b * per:(b + 1) * per]
    if got.shape[-1] == 128:
        got = got[:, z["sub8" if name in ("feat", "tfeat") else "sub4"]]
    return ref, got


def test_op_restatements_equal_the_reference_functions(ops):
    print()
    worst = 0.0
    for h4, w4 in ops["grids"]:
        tag = "%dx%d" % (h4, w4)
        up = S.enlarge2_restated(ops["flow8_" + tag], h4 // 2, w4 // 2)["o"]
        wp = S.warp_restated(ops["feat_" + tag], ops["up_" + tag], h4, w4)
        pos = S.positions_n(h4, w4, 8)[0]
        mask = R.region_mask(S.regions_n(h4, w4, 8))
        assert wp["outside"].any(), "no sample outside the grid: the zero padding is not exercised"
        errs = dict(up=relmax(up, ops["up_" + tag]), warp=relmax(wp["o"], ops["warp_" + tag]), pos=relmax(pos, ops["pos_" + tag]))
        print("  %-6s " % tag + " ".join("%s %.2e" % kv for kv in errs.items()))
        assert max(errs.values()) <= YARD, (tag, errs)
        assert np.array_equal(mask, ops["mask_" + tag].astype(np.float64)), tag
        assert np.array_equal(S.win_rows_n(h4, w4, 8, 2, True), S.win_rows_oracle_n(h4, w4, 8, 2, True)), tag
        assert np.array_equal(S.win_rows_n(h4, w4, 8, 2, False), S.win_rows_oracle_n(h4, w4, 8, 2, False)), tag
        worst = max(worst, *errs.values())
    h4, w4 = ops["grids"][0]
    e = relmax(S.upsample_restated(ops["flow4"], ops["logits"], h4, w4, 4)["o"], ops["ups"])
    print("  upsample x 4 %.2e; worst of all %.2e" % (e, max(worst, e)))
    assert e <= YARD


def test_op_yardstick_sees_the_planted_faults(ops):
    h4, w4 = ops["grids"][1]
    tag = "%dx%d" % (h4, w4)
    for bug in ("not_doubled", "align_false"):
        assert relmax(S.enlarge2_restated(ops["flow8_" + tag], h4 // 2, w4 // 2, bug=bug)["o"], ops["up_" + tag]) > FAULT, bug
    assert relmax(S.warp_restated(ops["feat_" + tag], ops["up_" + tag], h4, w4, bug="border")["o"], ops["warp_" + tag]) > FAULT
    assert relmax(S.positions_n(h4, w4, 2)[0], ops["pos_" + tag]) > FAULT                       # the 2-split table at the fine scale
    assert not np.array_equal(R.region_mask(S.regions_n(h4, w4, 8, bug="region_edge")), ops["mask_" + tag].astype(np.float64))
    assert not np.array_equal(S.win_rows_n(h4, w4, 8, 2, True, bug="wywx"), S.win_rows_oracle_n(h4, w4, 8, 2, True))
    h4, w4 = ops["grids"][0]
    assert relmax(S.upsample_restated(ops["flow4"], ops["logits"], h4, w4, 4, bug="times8")["o"], ops["ups"]) > FAULT


def test_window_restatement_with_8_splits_equals_the_reference_route():
    """gather / region mask / partner window with 64 windows per image = the reference's roll + split + mask + merge, float64"""
    for (h4, w4), shifted, cross in (((16, 24), True, True), ((24, 40), True, False), ((24, 40), False, True)):
        Y = R.window_data(5, 2, h4, w4)[0]
        t = S.window_restated_n(Y, h4, w4, 8, 2, shifted, cross)["o"].reshape(2, h4 * w4, 128)
        assert np.abs(t - S.window_truth_n(Y, h4, w4, 8, 2, shifted, cross)).max() < 1e-12
        for bug in (("no_partner",) if cross else ()) + (("region_edge",) if shifted else ()):
            b = S.window_restated_n(Y, h4, w4, 8, 2, shifted, cross, bug=bug)["o"].reshape(2, h4 * w4, 128)
            assert relmax(b, t) > FAULT, bug


@pytest.mark.parametrize("hw", S.SIZES)
def test_restatement_equals_every_stage_and_flow_of_the_real_model(golden_dir, weights2, hw):
    """both directions (the backward one is the swapped pair) at (4, 1), the forward one at (2, 2) where the fixture holds it; and the two
    conditions on the inputs.  measured worst case over all sizes: 1.5e-5 of range (flow_match4 at 100 x 150), EXPERIMENTS.md"""
    print()
    worst = 0.0
    for b, swapped in enumerate((False, True)):
        up, st, z = reference_run(golden_dir, weights2, hw, swapped=swapped)
        errs = {"flow": relmax(up, z["bwd_c4p1" if b else "fwd_c4p1"])}
        for name in S.STAGES:
            ref, got = stage_of(z, name, st, b)
            assert ref.shape == got.shape, (name, ref.shape, got.shape)
            errs[name] = relmax(got, ref)
        print("  %dx%d %s " % (hw[0], hw[1], "bwd" if b else "fwd") + " ".join("%s %.1e" % kv for kv in errs.items()))
        assert max(errs.values()) <= YARD, errs
        worst = max(worst, *errs.values())
        residual = np.abs(z["flow_match4_c4p1"][b] - z["flow_up_c4p1"][b]).max()
        wp = S.warp_restated(np.zeros((1, st["flow_up"].shape[1], 1)), z["flow_up_c4p1"][b:b + 1], *[v // 4 for v in S.padded(hw)])
        assert residual > 0.25, "the fine scale's matching is idle on this fixture (residual %.3f px)" % residual
        assert wp["outside"].any(), "no warped token takes a zero from outside the grid"
    for cfg in S.CONFIGS[hw]:
        if cfg != (4, 1):
            up, st, z = reference_run(golden_dir, weights2, hw, cfg=cfg)
            tag = "_c%dp%d" % cfg
            errs = {"flow": relmax(up, z["fwd" + tag]), "flow_match4": relmax(st["flow_match4"], z["flow_match4" + tag]),
                    "flow_prop4": relmax(st["flow_prop4"], z["flow_prop4" + tag])}
            print("  %dx%d %s " % (hw[0], hw[1], cfg) + " ".join("%s %.1e" % kv for kv in errs.items()))
            assert max(errs.values()) <= YARD, errs
            worst = max(worst, *errs.values())
    print("  worst %.2e of range" % worst)


# the planted faults of the whole model and the first stage each must move
FAULTS = [("not_doubled", "flow_up"), ("align_false", "flow_up"), ("border", "warp"), ("warp_feature0", "warp"), ("coarse_windows", "block0_4"),
          ("coarse_positions", "block0_4"), ("no_residual", "flow_match4"), ("times8", "flow"), ("trident_swapped", "feat4")]


@pytest.mark.parametrize("bug,stage", FAULTS)
def test_yardstick_sees_every_planted_fault(golden_dir, weights2, bug, stage):
    """on the 96 x 160 fixture (3 x 5 windows, shifts 1 and 2): the named stage and the final flow both leave the reference by > 100 x 1e-4"""
    hw = (96, 160)
    up, st, z = reference_run(golden_dir, weights2, hw, bug=bug)
    e_flow = relmax(up, z["fwd_c4p1"])
    e_stage = e_flow if stage == "flow" else relmax(*stage_of(z, stage, st, 0)[::-1])
    print("\n  %-16s %s %.2e, final flow %.2e" % (bug, stage, e_stage, e_flow))
    assert e_stage > FAULT and e_flow > FAULT, (bug, e_stage, e_flow)


def test_wrong_pad_is_seen(golden_dir, weights2):
    """100 x 150 pads to 128 x 160 under /32; the /16 pad (112 x 160) is what the reference refuses - a restatement fed the /16 pad cannot
    even be cut into 8 x 8 windows of whole tokens"""
    z = np.load(os.path.join(golden_dir, S.golden_name((100, 150))))
    assert S.padded((100, 150)) == (128, 160) and S.padded((100, 150), 16) == (112, 160)
    assert z["fwd_c4p1"].shape == (100, 150, 2) and (112 // 4) % 8 != 0


# recorded from synth.gmflow_weights(seed=2468) of the commit before the two-scale model: sha256 over every tensor in order (name, dtype,
# shape, bytes), the number of tensors, and the first three values of four named tensors as float32 hex literals
ONE_SCALE_SHA256 = "eb3d7f6fe8495c9144673e1fe0c046fc2d80dc6f274de07e859289cee2fe2456"
ONE_SCALE_COUNT = 123
ONE_SCALE_VALUES = {"upsampler.2.weight": ("-0x1.762828p-10", "0x1.671080p-5", "0x1.0b35acp-2"),
                    "upsampler.2.bias": ("0x1.154c74p-4", "0x1.166508p-4", "-0x1.9805ecp-5"),
                    "backbone.conv1.weight": ("-0x1.7a3510p-5", "0x1.f75062p-3", "0x1.38a092p-3"),
                    "transformer.layers.3.cross_attn_ffn.norm2.weight": ("0x1.048e66p-2", "0x1.1d1ac0p-2", "0x1.7e4808p-2")}


def weights_digest(w):
    import hashlib
    h = hashlib.sha256()
    for k, v in w.items():
        for part in (k.encode(), str(v.dtype).encode(), str(v.shape).encode(), np.ascontiguousarray(v).tobytes()):
            h.update(part)
    return h.hexdigest()


def test_one_scale_weights_are_unchanged_and_shared_tensors_identical(weights2):
    """gmflow_weights(num_scales=1) is the dict of the commit before this model bit for bit: a few exact values of named tensors
    (upsampler.2 among them) and the sha256 of the whole dict, both recorded from that commit, are pinned above; and every tensor the two
    models share is identical, the two-scale dict adding one name and re-drawing only upsampler.2"""
    w1 = synth.gmflow_weights(seed=2468)
    for w in (w1, synth.gmflow_weights(seed=2468, num_scales=1)):
        assert len(w) == ONE_SCALE_COUNT
        for k, vals in ONE_SCALE_VALUES.items():
            assert w[k].dtype == np.float32 and [float(x) for x in w[k].ravel()[:3]] == [float.fromhex(v) for v in vals], k
        assert weights_digest(w) == ONE_SCALE_SHA256
    assert [n for n, _ in synth.gmflow_param_shapes()] == list(w1) and "backbone.trident_conv.weight" not in w1
    assert w1["upsampler.2.weight"].shape == (576, 256, 1, 1) and weights2["upsampler.2.weight"].shape == (144, 256, 1, 1)
    assert weights2["backbone.trident_conv.weight"].shape == (128, 128, 3, 3)
    extra = set(weights2) - set(w1)
    assert extra == {"backbone.trident_conv.weight"}
    for k, v in w1.items():
        if not k.startswith("upsampler.2"):
            assert np.array_equal(v, weights2[k]) and v.dtype == weights2[k].dtype, k
    assert synth.gmflow_param_shapes(num_scales=1) == synth.gmflow_param_shapes()


def test_two_scale_names_and_shapes_are_the_real_models(golden_dir, weights2):
    """the generator loaded these tensors into the real GMFlow(num_scales=2, upsample_factor=4) with strict=True and stored the list"""
    z = np.load(os.path.join(golden_dir, S.golden_name(S.SIZES[0])))
    assert [str(n) for n in z["names"]] == list(weights2)
    assert [str(s) for s in z["shapes"]] == [",".join(str(d) for d in v.shape) for v in weights2.values()]
    assert [(n, tuple(v.shape)) for n, v in weights2.items()] == [(n, tuple(s)) for n, s in synth.gmflow_param_shapes(num_scales=2)]
