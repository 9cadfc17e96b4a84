"""CPU: the float64 truth / restatements of tests/raft_ref.py against each other, on the data tests/test_gpu_raft_ops.py runs on a card.

* restatement vs truth inside each op's budget;
* the tolerances see the bugs: every planted fault moves some element by at least 4x the kernel-vs-restatement tolerance;
* the lookup kernel's integer index arithmetic restated and asserted in bounds for every input the GPU test uses (far flows included), and
  the conditions that keep a lookup test from passing on emptiness (zero / inside / outside shares, third-segment share).
"""
import numpy as np
import pytest

import raft_ref as R
from split_ref import BUDGET, F16, MX2, SPLIT16

SEE = 4.0         # a planted bug must move an element by this many tolerances


def worst(err, tol):
    i = np.unravel_index(np.argmax(err / tol), err.shape)
    return float((err / tol)[i]), i


# ---------------------------------------------------------------------------------------------------------------------
# lookup
# ---------------------------------------------------------------------------------------------------------------------
def lookup_case(name, n, h8, w8, sub, brd, max_rows=1200):
    f1, f2 = R.lookup_features(1000 + h8 * w8, n, h8, w8)
    flows = R.lookup_flows(2000 + h8 * w8, n, h8, w8, sub, brd)
    R_ = n * h8 * w8
    rows = np.arange(R_) if R_ <= max_rows else np.unique(np.concatenate([np.arange(64), np.arange(R_ - 64, R_),
                                                                            R.rng(7).choice(R_, max_rows, replace=False)]))
    return f1, f2, flows, rows


@pytest.mark.parametrize("grid", R.LOOKUP_GRIDS + [R.LARGE_GRID], ids=lambda g: g[0])
def test_lookup_index_arithmetic_in_bounds_and_inputs_not_empty(grid):
    """before anything runs on a card: every tile address the kernel forms for the GPU test's flows is inside the level's row, the window
    offsets stay inside the LDS copy, and the sub-pixel / border families are not degenerate"""
    name, n, h8, w8, sub, brd = grid
    geo = R.geometry(h8, w8)
    P = h8 * w8
    flows = R.lookup_flows(2000 + P, n, h8, w8, sub, brd)
    if name.startswith("129x17"):
        flows["down"] = R.downward_flows(2100, n, h8, w8)
    for fam, fl in flows.items():
        assert np.isfinite(fl).all()
        st = R.lookup_index_check(fl, P, w8, geo, n * P)
        sh = R.window_shares(fl, P, w8, h8, w8, n * P)
        print("\n  %-9s %-8s third-segment %.3f  inside %.2f straddle %.2f outside %.2f  rows beyond hp (old bound) %d"
              % (name, fam, st["third"] / st["windows"], sh["inside"], sh["straddle"], sh["outside"], st["beyond_hp"]), end="")
        if fam == "subpixel":
            assert st["third"] * 16 >= st["windows"] and sh["inside"] >= 0.25
        if fam == "border":
            assert sh["straddle"] >= 0.10 and sh["outside"] >= 0.02
        if fam == "down":
            assert st["beyond_hp"] >= 100


def test_geometry_restated_is_the_library_s():
    """corr_pyramid_geometry (the function RaftEngine::prepare plans with; it needs no GPU) against its restatement"""
    import __graft_entry__ as entry
    from prisma_amd import engine
    entry.build()
    for h8 in list(range(16, 140, 3)) + [129, 258, 299]:
        for w8 in list(range(16, 200, 7)) + [17, 34, 184, 519]:
            assert engine.raft_geometry(h8, w8) == R.geometry(h8, w8), (h8, w8)


def test_geometry_takes_both_stride_branches():
    took = {R.geometry(h, w)[0]["ld"] != R.geometry(h, w)[0]["hp"] * R.geometry(h, w)[0]["wp"] for _, _, h, w, _, _ in R.LOOKUP_GRIDS + [R.LARGE_GRID]}
    assert took == {True, False}
    g = R.geometry(129, 17)[0]
    assert (g["hp"], g["wp"], g["ld"], g["ld"] // g["wp"]) == (136, 24, 3328, 138)
    g = R.geometry(56, 184)[0]
    assert (g["hp"], g["ld"], g["ld"] // g["wp"]) == (56, 10496, 57)


@pytest.mark.parametrize("grid", R.LOOKUP_GRIDS[:3], ids=lambda g: g[0])
def test_lookup_restatement_vs_truth(grid):
    name, n, h8, w8, sub, brd = grid
    f1, f2, flows, rows = lookup_case(*grid)
    P = h8 * w8
    lt, mt = R.pyramid_truth(f1, f2, rows)
    lr, mr = R.pyramid_restated(f1, f2, rows)
    for l in range(4):
        # a level entry: pooled features rounded l times, the entry once: (l + 1) 2^-11 of sum |a||b| at worst, 2^-10 for l <= 1; held to 2^-10
        e, _ = worst(np.abs(lr[l] - lt[l]), BUDGET[F16] * mt[l] + 2.0 ** -24)
        print("\n  %s level %d restated vs truth: worst err / (2^-10 mag) %.3f" % (name, l, e), end="")
        assert e < 1
    for fam, fl in flows.items():
        t = R.lookup_truth(lt, fl[rows], P, w8, rows)
        mag = R.lookup_truth(mt, fl[rows], P, w8, rows)
        r, tol = R.lookup_restated(lr, fl[rows], P, w8, rows)
        e, i = worst(np.abs(r - t), BUDGET[F16] * mag + tol)
        z = float((t[:, :81] == 0).mean())
        print("\n  %s %-8s chain restated vs truth %.3f of budget; level-0 outputs exactly zero %.2f" % (name, fam, e, z), end="")
        assert e < 1, (fam, i)
        if fam == "subpixel":
            assert z <= 0.5
        # the restatement on the TRUTH's levels differs from truth by the coordinate round trip alone: inside its own tolerance
        r2, tol2 = R.lookup_restated(lt, fl[rows], P, w8, rows)
        e2, i2 = worst(np.abs(r2 - t), tol2)
        assert e2 < 1, (fam, i2, e2)


LOOKUP_BUGS = ["swap_ij", "level_scale", "align_false", "border_clamp", "third_segment", "pool_ceil"]


def test_lookup_tolerance_sees_the_bugs():
    name, n, h8, w8, sub, brd = R.LOOKUP_GRIDS[1]           # 17 x 23: odd sizes, so floor and ceil pooling differ
    f1, f2, flows, rows = lookup_case(name, n, h8, w8, sub, brd)
    P = h8 * w8
    lr, _ = R.pyramid_restated(f1, f2, rows)
    for bug in LOOKUP_BUGS:
        seen = 0.0
        for fam in ("subpixel", "border"):
            fl = flows[fam][rows]
            r, tol = R.lookup_restated(lr, fl, P, w8, rows)
            if bug == "pool_ceil":      # another pyramid (levels of 9 x 12, 5 x 6, 3 x 3 instead of 8 x 11, 4 x 5, 2 x 2) under the same lookup
                lt, _ = R.pyramid_truth(f1, f2, rows)
                lb, _ = R.pyramid_truth(f1, f2, rows, bug=bug)
                r, tol = R.lookup_restated(lt, fl, P, w8, rows)
                b, _ = R.lookup_restated(lb, fl, P, w8, rows)
                seen = max(seen, worst(np.abs(b - r), tol)[0])
                continue
            b, _ = R.lookup_restated(lr, fl, P, w8, rows, bug=bug)
            seen = max(seen, worst(np.abs(b - r), tol)[0])
        print("\n  lookup bug %-14s moves an element by %.3g tolerances" % (bug, seen), end="")
        assert seen >= SEE, bug


# ---------------------------------------------------------------------------------------------------------------------
# convf1 / flow_head2
# ---------------------------------------------------------------------------------------------------------------------
def test_convf1_restatement_vs_truth_and_bugs():
    flow, w, b = R.convf1_data(31 + 17, 3, 17, 23)          # the GPU test's (3, 17, 23) data
    t, mag = R.convf1_truth(flow, w, b)
    assert (t > 0).mean() >= 0.30
    for passes, mx2, budget in ((1, False, BUDGET[F16]), (2, False, BUDGET[SPLIT16]), (2, True, BUDGET[MX2])):
        r, tol = R.convf1_restated(flow, w, b, passes, mx2)
        e, i = worst(np.abs(r - t), budget * mag + tol)
        print("\n  convf1 passes %d mx2 %d restated vs truth: %.3f of budget" % (passes, mx2, e), end="")
        assert e < 1, i
    r, tol = R.convf1_restated(flow, w, b, 2)
    for bug in ("residual_dropped", "tap_transposed", "channels_swapped", "next_image"):
        bad, _ = R.convf1_restated(flow, w, b, 2, bug=bug)
        s = worst(np.abs(bad - r), tol)[0]
        print("\n  convf1 bug %-17s moves an element by %.3g tolerances" % (bug, s), end="")
        assert s >= SEE, bug
    # unrounded flows: the kernel rounds them to fp16 by design - inside the fp16-operand budget of the truth on the unrounded field
    flow_u, w, b = R.convf1_data(31 + 16, 1, 16, 16, rounded=False)
    t, mag = R.convf1_truth(flow_u, w, b)
    r, tol = R.convf1_restated(flow_u, w, b, 2)
    assert worst(np.abs(r - t), BUDGET[F16] * mag + tol)[0] < 1


def test_flow_head2_restatement_vs_truth_and_bugs():
    x, w, b, flow = R.flow_head2_data(41 + 23, 3, 17, 23)       # the GPU test's n 3, H 17, W 23 data
    t, mag = R.flow_head2_truth(x, w, b, flow)
    for split, budget in ((False, BUDGET[F16]), (True, BUDGET[SPLIT16])):
        r, tol = R.flow_head2_restated(x, w, b, flow, split)
        e, i = worst(np.abs(r - t), budget * mag + tol)
        print("\n  flow_head2 split %d restated vs truth: %.3f of budget" % (split, e), end="")
        assert e < 1, i
    r, tol = R.flow_head2_restated(x, w, b, flow, True)
    for bug in ("w_lo_dropped", "bias_twice", "old_flow_dropped"):
        bad, _ = R.flow_head2_restated(x, w, b, flow, True, bug=bug)
        s = worst(np.abs(bad - r), tol)[0]
        print("\n  flow_head2 bug %-17s moves an element by %.3g tolerances" % (bug, s), end="")
        assert s >= SEE, bug


# ---------------------------------------------------------------------------------------------------------------------
# upsample
# ---------------------------------------------------------------------------------------------------------------------
def test_upsample_truth_matches_the_oracle_formula_and_sees_the_bugs():
    import torch
    from oracle import raft_oracle as O
    pad_l, pad_t, h8, w8 = R.pad_geometry(131, 181)
    assert (pad_l, pad_t, h8, w8) == (1, 2, 17, 23)
    flow, mask = R.upsample_data(51 + h8, 2, h8, w8)             # the GPU test's 17x23_crop data
    up, mag, maxd = R.upsample_truth(flow, mask, h8, w8, pad_l, pad_t, 131, 181)
    # the oracle's upsample_flow (unfold / softmax / permute as the reference writes it) in float64 on the same data
    fl = torch.from_numpy(flow.astype(np.float64)).reshape(2, h8, w8, 2).permute(0, 3, 1, 2)
    mk = torch.from_numpy(mask.astype(np.float64)).reshape(2, h8, w8, 576).permute(0, 3, 1, 2)
    ref = O.upsample_flow(fl, mk).permute(0, 2, 3, 1).numpy()[:, pad_t:pad_t + 131, pad_l:pad_l + 181]
    assert np.abs(up - ref).max() < 1e-12
    tol = R.upsample_tolerance(mag)
    for bug in ("softmax_axis", "no_8x", "crop_off_by_one"):
        bad, _, _ = R.upsample_truth(flow, mask, h8, w8, pad_l, pad_t, 131, 181, bug=bug)
        s = worst(np.abs(bad - up), tol)[0]
        print("\n  upsample bug %-16s moves an element by %.3g tolerances" % (bug, s), end="")
        assert s >= SEE, bug
    # maxd is compared bit for bit: any other value is seen.  Make the largest displacement fall into the cropped-away margin.
    flow2, mask2 = R.upsample_margin_case(flow, mask, w8)
    _, _, m_ok = R.upsample_truth(flow2, mask2, h8, w8, pad_l, pad_t, 131, 181)
    _, _, m_bad = R.upsample_truth(flow2, mask2, h8, w8, pad_l, pad_t, 131, 181, bug="maxd_uncropped")
    print("\n  upsample maxd over the uncropped map: %s instead of %s" % (m_bad, m_ok), end="")
    assert np.all(m_bad > 10 * m_ok)


# ---------------------------------------------------------------------------------------------------------------------
# instance norm
# ---------------------------------------------------------------------------------------------------------------------
def test_instnorm_tolerance_sees_the_bugs():
    for ratio in (0.0, 2.0):
        a = R.instnorm_data(61, 3, 2049, 64, ratio)
        b = R.instnorm_data(62, 3, 2049, 64, 0.0)
        av, bv = R.map_value(a, 0), R.map_value(b, 0)
        v, mean, rstd, var = R.instnorm_truth(av, bv, True)
        tol, _, trstd, kappa = R.instnorm_tolerance(av, av, mean, rstd, var, 64, v, False)
        print("\n  instance norm ratio %g: kappa up to %.1f" % (ratio, kappa.max()), end="")
        for bug in ("unbiased", "eps", "batch_shared", "second_relu"):
            bad, _, brstd, _ = R.instnorm_truth(av, bv, True, bug=bug)
            # the op returns {mean, rstd} beside the map: a fault in the statistics is judged on whichever shows it more
            s = max(worst(np.abs(bad - v), tol)[0], worst(np.abs(brstd - rstd), trstd)[0])
            print("\n  instance norm bug %-12s (mean / std %g) moves an element by %.3g tolerances" % (bug, ratio, s), end="")
            assert s >= SEE, bug
