"""GPU: corr_lookup_otf_kernel (flow_raft --alternate_corr, csrc/corr_otf.hip) through pb_op_raft_lookup_otf - the pooling launches and the
lookup with the arguments RaftEngine::infer uses - against tests/raft_otf_ref.py: (1) element-wise against the restatement (fp16 operands,
entries NOT rounded to fp16) inside half an fp16 step + the coordinate round trip + the blend's and the accumulation's fp32 roundings,
(2) against float64 truth inside the fp16-operand budget, (3) bytes: the e4m3 copy exact, everything the kernel does not own still preset.
tests/test_raft_otf_ref_cpu.py holds the CPU side: the tolerance sees the planted faults and a kernel that rounds its entries to fp16.

measured (MI355X; worst error / tolerance): see the "measured:" line of every test."""
import functools

import numpy as np
import pytest

import raft_otf_ref as O
import raft_ref as R
from gm_ref import check, preset
from prisma_amd import engine
from split_ref import e4m3_bytes

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


def lookup_rows(raw, rows, o8):
    """tests/test_gpu_raft_ops.py lookup_rows restated: raw [rows + GUARD, ldo * 2] bytes -> the 324 values of every row; halfs 324..383 and
    the guard rows still preset, the e4m3 copy (byte 768) equal to e4m3(fp16 value), the bytes behind the copy preset"""
    h = raw.view(np.float16)
    preset("lookup_otf halfs 324..383", raw[:rows, 648:768])
    preset("lookup_otf guard rows", raw[rows:])
    if o8:
        want = e4m3_bytes(h[:rows, :324].astype(np.float32))
        got8 = raw[:rows, 768:768 + 324]
        bad = got8 != want
        assert not bad.any(), "lookup_otf e4m3 copy: element %s is 0x%02x, e4m3 of the fp16 value is 0x%02x" % (
            tuple(np.argwhere(bad)[0]), got8[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])
        preset("lookup_otf bytes behind the e4m3 copy", raw[:rows, 768 + 324:])
    else:
        assert raw.shape[1] == 768
    return h[:rows, :324].astype(np.float64)


@functools.lru_cache(maxsize=1)
def reference(name):
    """features, flows, restated and truth levels of one grid: computed once, read-only"""
    grid = next(g for g in R.LOOKUP_GRIDS if g[0] == name)
    _, n, h8, w8, sub, brd = grid
    P = h8 * w8
    f1, f2 = R.lookup_features(1000 + P, n, h8, w8)
    flows = O.otf_flows(2000 + P, n, h8, w8, sub, brd)
    if name.startswith("129x17"):
        flows["down"] = R.downward_flows(2100, n, h8, w8)
    return f1, f2, flows, O.pyramid_otf(f1, f2), R.pyramid_truth(f1, f2)


@pytest.mark.parametrize("grid", R.LOOKUP_GRIDS, ids=lambda g: g[0])
def test_lookup_otf(ops, grid):
    """every flow family (zero, eighths, sub-pixel, across every border, +-1e4 / +-1e6, affine; 129x17 also flows past the last padded row),
    the e4m3 copy on every second one.  Tiles: 16x16 four full ones, 17x23 and 129x17 partial tiles on both edges, 46x62x3 three
    pair-directions of 48 tiles; a `far` row makes its tile's box the whole level.
    measured: worst err / tol vs restatement | vs truth: 16x16 0.841 | 0.103, 17x23 0.887 | 0.117, 46x62x3 0.870 | 0.144, 129x17x2 0.843 |
    0.146, 24x40 0.845 | 0.146.  (Figures near 1 against the restatement are fp16 stores next to a rounding tie, as in test_gpu_raft_ops.)"""
    name, n, h8, w8, sub, brd = grid
    P, rows = h8 * w8, n * h8 * w8
    f1, f2, flows, (lo, mo), (lt, mt) = reference(name)
    for k, (fam, fl) in enumerate(flows.items()):
        o8 = k % 2 == 1
        raw = ops.raft_lookup_otf(f1, f2, fl, o8=o8, guard_rows=GUARD)
        got = lookup_rows(raw, rows, o8)
        r, tol = O.lookup_otf_restated(lo, mo, fl, P, w8)
        check("%s %s vs restatement" % (name, fam), got, r, tol)
        t = R.lookup_truth(lt, fl, P, w8)
        check("%s %s vs truth" % (name, fam), got, t, O.truth_budget(mt, fl, P, w8) + tol)
        if fam == "border":
            sh = R.window_shares(fl, P, w8, h8, w8, rows)
            assert sh["straddle"] >= 0.10 and sh["outside"] >= 0.02


@pytest.mark.parametrize("grid", [R.LOOKUP_GRIDS[1], R.LOOKUP_GRIDS[3]], ids=lambda g: g[0])
def test_lookup_otf_layout_detector(ops, grid):
    """fmap1 rows are 16 e_c one-hots, fmap2 holds multiples of 64: every product, every pooled feature and every window entry is exact, so
    the kernel must sit inside lookup_restated's tolerance on the TRUTH levels, and a wrong target address, frame, level or window slot is
    an O(100) error.
    measured: err / tol 0.973 (17x23), 0.955 (129x17x2)."""
    name, n, h8, w8, sub, brd = grid
    P, rows = h8 * w8, n * h8 * w8
    f1, f2 = R.lookup_features(3000 + P, n, h8, w8, detector=True)
    fl = R.downward_flows(2100, n, h8, w8) if name.startswith("129x17") else R.lookup_flows(2000 + P, n, h8, w8, sub, brd)["subpixel"]
    lt, _ = R.pyramid_truth(f1, f2)
    raw = ops.raft_lookup_otf(f1, f2, fl, o8=True, guard_rows=GUARD)
    got = lookup_rows(raw, rows, True)
    r, tol = R.lookup_restated(lt, fl, P, w8)
    assert np.abs(r).max() > 100
    check("%s detector lookup_otf vs restatement on truth levels" % name, got, r, tol)


def test_lookup_otf_large_grid(ops):
    """102 x 180 (1080p x 0.75): 13 x 23 = 299 tiles in one launch, the last tile row 6 pixels high, levels of 51 x 90, 25 x 45, 12 x 22
    (odd sizes, floor pooling); restatement and truth for a seeded subset of 600 rows plus the first and last 64.
    measured: err / tol <= 0.806 vs restatement, <= 0.095 vs truth."""
    name, n, h8, w8, sub, brd = R.LARGE_GRID
    P, rows = h8 * w8, n * h8 * w8
    f1, f2 = R.lookup_features(1000 + P, n, h8, w8)
    flows = O.otf_flows(2000 + P, n, h8, w8, sub, brd)
    sel = np.unique(np.concatenate([np.arange(64), np.arange(rows - 64, rows), R.rng(9).choice(rows, 600, replace=False)]))
    lo, mo = O.pyramid_otf(f1, f2, sel)
    lt, mt = R.pyramid_truth(f1, f2, sel)
    for fam in ("subpixel", "border", "far", "smooth"):
        fl = flows[fam]
        raw = ops.raft_lookup_otf(f1, f2, fl, o8=True, guard_rows=GUARD)
        got = lookup_rows(raw, rows, True)[sel]
        r, tol = O.lookup_otf_restated(lo, mo, fl[sel], P, w8, sel)
        check("%s %s vs restatement" % (name, fam), got, r, tol)
        t = R.lookup_truth(lt, fl[sel], P, w8, sel)
        check("%s %s vs truth" % (name, fam), got, t, O.truth_budget(mt, fl[sel], P, w8, sel) + tol)


def test_lookup_otf_refuses_what_the_engine_refuses(ops):
    f1, f2 = R.lookup_features(1, 1, 15, 16)
    with pytest.raises(Exception, match="too small"):
        ops.raft_lookup_otf(f1, f2, np.zeros((15 * 16, 2), np.float32))
