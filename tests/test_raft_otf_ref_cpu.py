"""CPU: the restatement and the tolerance tests/test_gpu_raft_otf_ops.py holds corr_lookup_otf_kernel to (tests/raft_otf_ref.py).
(1) the restatement alone sits inside the float64-truth budget on the seeded cases, (2) the tight tolerance sees every planted fault of
raft_ref's lookup, (3) it sees levels rounded to fp16 - what the volume path does and the on-the-fly kernel must not."""
import numpy as np
import pytest

import raft_otf_ref as O
import raft_ref as R
from split_ref import f16

CPU_GRIDS = [g for g in R.LOOKUP_GRIDS if g[0] in ("16x16", "17x23", "24x40")]


def _case(grid):
    name, n, h8, w8, sub, brd = grid
    P = h8 * w8
    f1, f2 = R.lookup_features(1000 + P, n, h8, w8)
    return name, n, h8, w8, P, f1, f2, O.otf_flows(2000 + P, n, h8, w8, sub, brd)


@pytest.mark.parametrize("grid", CPU_GRIDS, ids=lambda g: g[0])
def test_restatement_inside_truth_budget(grid):
    """measured: worst |restatement - truth| / budget 0.064 over the three grids and all flow families"""
    name, n, h8, w8, P, f1, f2, flows = _case(grid)
    lo, mo = O.pyramid_otf(f1, f2)
    lt, mt = R.pyramid_truth(f1, f2)
    assert set(flows) == {"zero", "eighths", "subpixel", "border", "far", "smooth"}
    worst = 0.0
    for fam, fl in flows.items():
        r, tol = O.lookup_otf_restated(lo, mo, fl, P, w8)
        t = R.lookup_truth(lt, fl, P, w8)
        bud = O.truth_budget(mt, fl, P, w8) + tol
        ratio = np.abs(r - t) / np.maximum(bud, 1e-300)
        ratio[(bud == 0) & (r == t)] = 0
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (name, fam, float(ratio.max()))
    print("\n  %s: restatement vs truth, worst share of the budget %.3f" % (name, worst), end="")
    assert worst <= 0.25          # the restatement itself must leave the kernel most of the budget


def test_smooth_family_is_coherent_with_fractions():
    fl = O.smooth_flow(1, 17, 23).astype(np.float64)
    assert (np.abs(fl - np.round(fl)) > 1e-3).mean() > 0.9
    f = fl.reshape(17, 23, 2)
    assert np.abs(np.diff(f, axis=0)).max() < 0.05 and np.abs(np.diff(f, axis=1)).max() < 0.05


@pytest.mark.parametrize("bug", ["swap_ij", "level_scale", "border_clamp", "align_false", "third_segment"])
def test_tight_tolerance_sees_planted_faults(bug):
    """a kernel with the fault = the restatement with bug=...; it must leave the tolerance of the correct restatement on 17x23"""
    name, n, h8, w8, P, f1, f2, flows = _case(R.LOOKUP_GRIDS[1])
    lo, mo = O.pyramid_otf(f1, f2)
    outside = 0
    for fam, fl in flows.items():
        r, tol = O.lookup_otf_restated(lo, mo, fl, P, w8)
        faulty = R.lookup_restated(lo, fl, P, w8, bug=bug)[0]
        outside += int((np.abs(f16(faulty).astype(np.float64) - r) > tol).sum())
    print("\n  %s: %d elements outside" % (bug, outside), end="")
    assert outside >= 100, (bug, outside)


def test_tight_tolerance_sees_fp16_levels():
    """levels rounded to fp16 before the blend (the volume path's rounding): 2.0 .. 3.1 tolerances on 17x23"""
    name, n, h8, w8, P, f1, f2, flows = _case(R.LOOKUP_GRIDS[1])
    lo, mo = O.pyramid_otf(f1, f2)
    l16 = [f16(l).astype(np.float64) for l in lo]
    for fam in ("subpixel", "smooth", "eighths"):
        fl = flows[fam]
        r, tol = O.lookup_otf_restated(lo, mo, fl, P, w8)
        r16 = R.lookup_restated(l16, fl, P, w8)[0]
        worst = float((np.abs(f16(r16).astype(np.float64) - r) / tol).max())
        print("\n  %s: fp16 levels are %.2f tolerances off" % (fam, worst), end="")
        assert worst > 1.5, (fam, worst)
