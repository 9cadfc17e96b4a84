"""GPU: the flow bands' frame path outside the networks, kernel by kernel (pb_op_flow_*: the launchers of raft_kernels.h with the arguments
FlowEngine::prep_frames and FlowEngine::flow_tail pass) against tests/flow_io_ref.py - raft_prep_kernel in its three output layouts, both
normalisations and the --inference_size mode; flow_resize_back_kernel; flow_encode_kernel; fwdbwd_mask_kernel.  Bytes where the reference
is integer arithmetic or a defined sequence of IEEE operations, float64 truth with a tolerance derived from the float32 operation count
elsewhere; everything a kernel does not own must still be 0xFF.  The checks live in flow_io_ref.*_verify; tests/test_flow_io_ref_cpu.py
runs the same checks on the restatements, with and without planted faults.

measured (MI355X; worst error / tolerance per op): see the "measured:" line of every test.
"""
import numpy as np
import pytest

import flow_io_ref as R
from conftest import TOL
from prisma_amd import engine, synth

pytestmark = pytest.mark.gpu

PREP_RUNS = [(c, norm, layout) for c in R.PREP_CASES for norm, layout in R.prep_modes(c[3])]
ISZ_RUNS = [(c, norm, layout) for c in R.PREP_ISZ_CASES for norm, layout in R.prep_modes(16)]


def run_id(r):
    return "%s-n%d-l%d" % (R.case_id(r[0]), r[1], r[2])


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


# ---- raft_prep_kernel ----
@pytest.mark.parametrize("run", PREP_RUNS, ids=run_id)
def test_prep_direct(ops, run):
    """one launch_raft_prep over three frames (noise, a 0 / 255 checker, a ramp) per (H, W, scale, factor) of the issue's table, in the
    layouts and the normalisation the factor's band uses: 8 RAFT, fp16 and [hi | hi8 | lo8]; 16 / 32 GMFlow, fp16 and [hi | lo].  The plan
    equals the oracle's (scaled_size, pad_amounts); the scaled uint8 frame - which the engines never ask for - equals cv_resize_cubic_u8
    byte for byte; hi is the fp16 of the float64 truth bit for bit; hi + lo within 2 (RAFT) / 3 (GMFlow) float32 roundings plus lo's fp16
    half-step; hi8 the e4m3 bytes of the kernel's own hi, lo8 within one e4m3 step; channel 3 zero; guard rows and bytes still 0xFF.
    measured: scaled frames and hi equal in all 20 launches; hi + lo err / tol <= 0.867, lo8 err / tol <= 0.519."""
    (H, W, s, factor), norm, layout = run
    fr = R.prep_frames(H, W)
    geo, raw, sc, sg, pa = ops.flow_prep(fr, s, factor, layout, norm, None, R.GUARD_ROWS, R.GUARD)
    m = R.prep_verify("prep " + run_id(run), fr, s, factor, layout, norm, pa, geo, raw, sc, sg)
    print("\n  prep %s: err / tol %s" % (run_id(run), m))


@pytest.mark.parametrize("run", ISZ_RUNS, ids=run_id)
def test_prep_inference_size(ops, run):
    """flow_gmflow --inference_size: the scaled frame blended (bilinear, align_corners) to the given size, no padding, GMFlow's normalisation,
    fp16 and [hi | lo]; 34 x 58 to 32 x 64 and to 64 x 32, and 48 x 80 onto itself, where every weight is 0.  hi lies between the fp16
    roundings of truth -+ 7 float32 roundings (the coordinates are torch's float32 ones, so none of a coordinate's rounding is in the
    tolerance; under 1e-3 of the elements have two admissible fp16 values: test_flow_io_ref_cpu); hi + lo within the tolerance plus lo's
    half-step; scaled_out is left alone.
    measured: hi + lo err / tol <= 0.849; tie share 6.5e-4, 8.7e-4, 0."""
    (H, W, s, isz), norm, layout = run
    fr = R.prep_frames(H, W, True)
    geo, raw, sc, sg, pa = ops.flow_prep(fr, s, 16, layout, norm, isz, R.GUARD_ROWS, R.GUARD)
    m = R.prep_verify("prep " + run_id(run), fr, s, 16, layout, norm, pa, geo, raw, sc, sg, isz)
    print("\n  prep %s: err / tol %s" % (run_id(run), m))


@pytest.mark.parametrize("mode", R.prep_modes(16), ids=lambda m: "n%d-l%d" % m)
def test_prep_inference_size_full_range(ops, mode):
    """the first inference-size case on full-range frames: the blend at full magnitude, the 0 / 255 checker clamping the cubic resize at
    both ends before it.  The same checks; about 1e-2 of the elements admit two fp16 values here (reported by test_flow_io_ref_cpu).
    measured: hi + lo err / tol <= 0.743; tie share 1.0e-2."""
    H, W, s, isz = R.PREP_ISZ_FULL
    norm, layout = mode
    fr = R.prep_frames(H, W)
    geo, raw, sc, sg, pa = ops.flow_prep(fr, s, 16, layout, norm, isz, R.GUARD_ROWS, R.GUARD)
    m = R.prep_verify("prep full range %s" % (mode,), fr, s, 16, layout, norm, pa, geo, raw, sc, sg, isz)
    print("\n  prep full range %s: err / tol %s" % (mode, m))


# ---- flow_resize_back_kernel ----
@pytest.mark.parametrize("case", R.BACK_CASES, ids=["%dx%d-%dx%d" % (a + b) for a, b in R.BACK_CASES])
def test_resize_back(ops, case):
    """launch_flow_resize_back on three flows with differing maxima: values against float64 at torch's float32 coordinates within 6 float32
    roundings; maxd bit-equal to the float32 maximum of sqrt(u u + v v) over the kernel's own output; a second call with flows a
    hundredth the size returns its own, smaller maxima (the maximum's words are preset to 0xFF by the op, so a launch that does not reset
    them returns NaN).  96 x 160 -> 300 x 450 is 135000 pixels: the 512-block grid strides twice.
    measured: value err / tol <= 0.689; maxd equal in all 6 cases."""
    (ih, iw), (sh, sw) = case
    fl = R.back_data(ih, iw)
    out, guard, mx = ops.flow_resize_back(fl, sh, sw, R.GUARD)
    m = R.back_verify("resize_back %s" % (case,), fl, sh, sw, out, guard, mx)
    small = R.back_data(ih, iw, 0.01)
    out2, guard2, mx2 = ops.flow_resize_back(small, sh, sw, R.GUARD)
    m2 = R.back_verify("resize_back small %s" % (case,), small, sh, sw, out2, guard2, mx2)
    assert (mx2 < mx).all() and len(set(mx.tolist())) == 3
    print("\n  resize_back %s: err / tol %.3f, %.3f" % (case, m["value"], m2["value"]))


# ---- flow_encode_kernel ----
@pytest.mark.parametrize("name", ["adversarial", "1x1", "random"])
def test_encode(ops, name):
    """launch_flow_encode with the per-frame maximum given: bytes equal to process_flow(exact_atan2=True) on the axes in both signs with
    either zero in the other component, the diagonals, min / max ratios at and one ulp either side of every switch of atan2_rn's k,
    signed zeros, denormals, a frame whose maximum is 0 (0 / 0: NaN colours are written as 0) and a 1 x 1 frame; and on 520 x 520 noise at
    three scales, 270400 pixels against the 1024-block cap.  max_out returns the maximum given, bit for bit.
    measured: equal in all three cases."""
    fl = R.encode_cases()[name]
    _, mx = R.encode_truth(fl)
    rgb, guard, mo = ops.flow_encode(fl, mx, R.GUARD)
    R.encode_verify("encode " + name, fl, rgb, guard, mo, mx)


# ---- fwdbwd_mask_kernel ----
@pytest.mark.parametrize("name", ["ties", "neg_x", "neg_y", "neg_xy", "h1", "w1"])
def test_fwdbwd_mask_delicate_integers(ops, name):
    """pb_flow_fwdbwd_mask against compute_fwdbwd_mask, bit for bit, where the kernel's integer arithmetic is delicate: targets exactly on
    the half-even ties of the 1/32-pixel quantisation (inside and outside the frame); targets left of, above, and left of and above the
    frame by fractions, with backward flows that close the round trip through the one tap inside the frame, so that >> 5 and & 31 of
    negative integers decide the bits (a truncating division or |q| & 31 flips a quarter of them: test_flow_io_ref_cpu); one-pixel axes.
    measured: equal in all six cases."""
    fl = R.mask_cases()[name]
    got = ops.flow_fwdbwd_mask(fl)
    want = R.mask_truth(fl)
    assert got.shape == want.shape
    bad = got != want
    assert not bad.any(), "mask %s: %d of %d differ, first %s" % (name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


# ---- the engine at a non-dyadic scale ----
def test_raft_sequence_at_scale_0_6_matches_oracle():
    """FlowRaft.infer_sequence(scale=0.6, iters=2) on three 216 x 288 frames -> 130 x 173 (padded to 136 x 176) against the oracle at the
    same scale: a check that the band runs a non-dyadic scale end to end, NOT a witness of the scale fix - the size is 130 x 173 with the
    widened float as well, and the 382 of 202410 bytes it would change by one level are far below 1e-3 of the flow's range (what sees the
    fix: test_prep_direct at 15 x 35 x 0.3 and the table test of test_flow_io_ref_cpu).  flow_raft's 4-level pyramid needs a 16 x 16 grid,
    128 pixels a side after scaling, hence this frame size.
    measured: relmax 4.0e-4 / 3.6e-4, relL2 2.9e-4 / 2.9e-4 (bounds 1e-3)."""
    from oracle import raft_oracle as O
    fr = synth.frame_pair_sequence(3, 216, 288, seed=6)
    w = synth.raft_weights(seed=4321)
    net = engine.FlowRaft(w, device=0, precision=1)
    try:
        flow, rgb, mx = net.infer_sequence(fr, scale=0.6, iters=2, backward=False)
    finally:
        net.close()
    for i in range(2):
        fwd, _ = O.infer_pair(w, fr[i], fr[i + 1], scale=0.6, iters=2, backward=False)
        assert flow[i, 0].shape == fwd.shape == (130, 173, 2)
        d, ref = flow[i, 0].astype(np.float64) - fwd, fwd.astype(np.float64)
        relmax, rell2 = np.abs(d).max() / np.abs(ref).max(), np.linalg.norm(d) / np.linalg.norm(ref)
        print("\n  scale 0.6 pair %d relmax %.3e relL2 %.3e" % (i, relmax, rell2))
        assert relmax < TOL[1][0] and rell2 < TOL[1][1]
