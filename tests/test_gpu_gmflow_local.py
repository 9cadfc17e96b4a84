"""GPU: the flow_gmflow band with a local matching radius and / or a local-window propagation radius (FlowGMFlow.set_matching) through the
C ABI - (a) the engine's flow_match / flow_prop stages against the float64 restatements (tests/gm_local_ref.py) applied to the engine's OWN
tfeat stage, inside the tolerance derived from the kernels' arithmetic; (b) end to end against the vectors the REAL reference produced
(tests/golden/gmflow_local_*.npz, tools/make_gmflow_local_golden.py); (c) a pair's bytes do not depend on its sequence or on the backward
direction; (d) the default comes back bit for bit, bad radii and other bands' contexts are errors.

measured (MI355X), (b) relmax / relL2 of the final flow against the reference vectors (range = max |ref|, px):
                125x157 fwd            125x157 bwd            90x150 fwd             90x150 bwd
  (4, -1)  1.90e-4 / 8.9e-5 (11.3)        -              2.11e-4 / 1.61e-4 (9.4)        -
  (-1, 1)  1.14e-4 / 4.7e-5 (117.3)  1.00e-4 / 4.2e-5   1.73e-4 / 9.7e-5 (94.2)   1.85e-4 / 4.9e-5
  (4, 1)   3.27e-4 / 6.9e-5 (31.0)   1.85e-4 / 1.11e-4  2.43e-4 / 8.5e-5 (25.4)   1.85e-4 / 9.8e-5
  (1, 2)   2.17e-4 / 1.17e-4 (7.1)        -              1.69e-4 / 1.18e-4 (7.4)        -
(a) worst error / derived tolerance: flow_match 0.024 .. 0.060, flow_prop 0.001 .. 0.021.
The bound is conftest.TOL[1] (1e-3 / 1e-3) wherever the measured value is at or below it; where a configuration measures above it, its entry
in BOUNDS is 1.5 x the measured value rounded up to one digit (a reordering of K redraws about a third of a margin, EXPERIMENTS.md 6.6),
with (a) still held to its derived tolerance.  Every configuration measures below 1e-3, so BOUNDS is empty and all are asserted at 1e-3.
"""
import os

import numpy as np
import pytest

import gm_local_ref as L
from conftest import TOL
from gm_ref import check
from prisma_amd import engine, synth

pytestmark = pytest.mark.gpu

# (file, configuration, output) -> (relmax, relL2) bound where the measured value is above conftest.TOL[1]
BOUNDS = {}


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rell2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.fixture(scope="module")
def weights():
    return synth.gmflow_weights(seed=2468)


@pytest.fixture(scope="module")
def net(weights):
    n = engine.FlowGMFlow(weights, device=0, precision=1)
    yield n
    n.set_matching(-1, -1)
    n.close()


@pytest.mark.parametrize("cfg,corr,prop", L.CONFIGS)
@pytest.mark.parametrize("name", L.SIZES)
def test_stages_and_flow(net, weights, golden_dir, name, cfg, corr, prop):
    """(a) and (b) of the module docstring for one size and configuration; both directions where the golden holds a backward flow.
    measured (a): worst err / tol 0.060 (125x157 (1, 2) flow_match); (b): worst relmax 3.27e-4 (125x157 (4, 1) fwd), table in the module docstring."""
    z = np.load(os.path.join(golden_dir, name))
    h, w = [int(v) for v in z["hw"]]
    fr = synth.frame_pair_sequence(2, h, w, seed=int(z["frame_seed"]))
    bidir = ("bwd_" + cfg) in z.files
    dirs = 2 if bidir else 1
    net.set_matching(corr, prop)
    net.set_profiling(timing=False, debug_stages=True)
    flow, rgb, mx = net.infer_sequence(fr, scale=1.0, backward=bidir)
    net.set_profiling(timing=False, debug_stages=False)
    assert flow.shape == (1, dirs, h, w, 2) and rgb.shape == (1, dirs, h, w, 3)
    h8, w8 = (h + 15) // 16 * 2, (w + 15) // 16 * 2
    tfeat, fm, fp = net.stage("tfeat"), net.stage("flow_match"), net.stage("flow_prop")
    assert tfeat.shape == (2, h8 * w8, 128) and fm.shape == (dirs, h8 * w8, 2) and fp.shape == fm.shape
    # (a) the two kernels in place, each against float64 on the very input the engine gave it
    if corr > 0:
        t = L.local_match_restated(tfeat, h8, w8, dirs, corr)
        check("%s %s flow_match" % (name, cfg), fm, t["o"], L.local_tolerance(t, corr))
    if prop > 0:
        wts = [weights["feature_flow_attn." + n] for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias")]
        q, k = L.prop_qk(tfeat[:dirs], *wts)
        t = L.local_prop_restated(q, k, fm, h8, w8, prop)
        check("%s %s flow_prop" % (name, cfg), fp, t["o"], L.local_tolerance(t, prop, L.projection_score_error(tfeat[:dirs], *wts, h8, w8, prop)))
    # (b) end to end against the reference
    print()
    outs = [("fwd", flow[0, 0], z["fwd_" + cfg])] + ([("bwd", flow[0, 1], z["bwd_" + cfg])] if bidir else [])
    for k_, g, ref in (("flow_match", fm[0], z["flow_match_" + cfg][0]), ("flow_prop", fp[0], z["flow_prop_" + cfg][0])):
        print("  %s %-5s %-10s relmax %.3e relL2 %.3e (range %.2f)" % (name, cfg, k_, relmax(g, ref), rell2(g, ref), float(np.abs(ref).max())))
    for k_, g, ref in outs:
        print("  %s %-5s %-10s relmax %.3e relL2 %.3e (range %.2f)" % (name, cfg, k_, relmax(g, ref), rell2(g, ref), float(np.abs(ref).max())))
    for k_, g, ref in outs:
        bm, bl = BOUNDS.get((name, cfg, k_), TOL[1])
        assert relmax(g, ref) <= bm and rell2(g, ref) <= bl, (name, cfg, k_)
    bm = BOUNDS.get((name, cfg, "fwd"), TOL[1])[0]
    ref = z["fwd_" + cfg]
    assert abs(float(mx[0, 0]) - float(np.sqrt((ref ** 2).sum(-1)).max())) < bm * float(np.abs(ref).max()) + 1e-4


def test_sequence_batching_and_directions_agree(net):
    """With (4, 1) a frame pair's bytes do not depend on the sequence it is computed in, and the forward bytes do not depend on whether the
    backward direction was asked for: past the transformer (which always runs both frames of a pair) every batch element of the local
    kernels, the upsampler and the encode is computed alone."""
    net.set_matching(4, 1)
    fr = synth.frame_pair_sequence(4, 120, 168, seed=8)
    f_all, _, m_all = net.infer_sequence(fr, scale=1.0, backward=True)
    f_fwd, _, m_fwd = net.infer_sequence(fr, scale=1.0, backward=False)
    assert f_all.shape == (3, 2, 120, 168, 2) and f_fwd.shape == (3, 1, 120, 168, 2)
    for i in range(3):
        one, _, m1 = net.infer_sequence(fr[i:i + 2], scale=1.0, backward=True)
        assert np.array_equal(one[0], f_all[i]) and np.array_equal(m1[0], m_all[i])
        assert np.array_equal(f_fwd[i, 0], f_all[i, 0]) and m_fwd[i, 0] == m_all[i, 0]
    # the backward direction is the forward direction of the swapped pair (the frames pass the encoder in another order: same arithmetic)
    back, _, _ = net.infer_sequence(fr[1::-1], scale=1.0, backward=False)
    assert relmax(back[0, 0], f_all[0, 1]) < 1e-5


def test_default_comes_back_and_errors_leave_the_context_usable(net, weights):
    fr = synth.frame_pair_sequence(2, 120, 168, seed=9)
    fresh = engine.FlowGMFlow(weights, device=0, precision=1)
    want = fresh.infer_sequence(fr, scale=1.0, backward=True)
    fresh.close()
    net.set_matching(4, 1)
    local = net.infer_sequence(fr, scale=1.0, backward=True)
    assert relmax(local[0], want[0]) > 1e-2                                  # another algorithm, not the default's flow
    net.set_matching(-1, -1)
    got = net.infer_sequence(fr, scale=1.0, backward=True)
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for bad in ((5, -1), (0, -1), (-2, 1), (4, 3), (-1, 0)):
        with pytest.raises(engine._lib.PrismaBandsError, match="radius_list"):
            net.set_matching(*bad)
    again = net.infer_sequence(fr, scale=1.0, backward=True)                  # still the default, still usable
    for a, b in zip(again, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    raft = engine.FlowRaft(synth.raft_weights(seed=4321), device=0)
    with pytest.raises(engine._lib.PrismaBandsError, match="flow_gmflow"):
        engine.check(raft.lib.pb_flow_set_matching(raft.ctx, 4, 1))
    small = synth.frame_pair_sequence(2, 128, 160, seed=4)                   # flow_raft's 4-level pyramid needs >= 128 px
    f, _, _ = raft.infer_sequence(small, scale=1.0, iters=2, backward=False)
    raft.close()
    assert f.shape == (1, 1, 128, 160, 2) and np.isfinite(f).all()
