"""CPU: the float64 truth / restatements of tests/gm_ref.py against the reference's own steps (oracle/gmflow_oracle.py) and against each
other, on the data tests/test_gpu_gmflow_ops.py runs on a card.

* the two host tables the engine plans with (pb_op_gm_tables needs no GPU): region ids vs shift_mask, positions vs float64;
* the restated index maps vs torch.roll + split_feature, the restated chains vs the oracle's functions;
* the tolerances see the bugs: every planted fault moves some element by at least SEE tolerances of the GPU test that would meet it
  (a byte-exact test's tolerance is zero: there the fault has to change the bytes);
* the conditions that keep a GPU test from passing on emptiness.
"""
import numpy as np
import pytest

import gm_ref as R

SEE = 4.0         # a planted bug must move an element by this many tolerances, as in test_raft_ref_cpu.py
ALL_GRIDS = R.GRIDS + [(16, 20), R.LARGE]


def worst(err, tol):
    r = err / np.broadcast_to(tol, err.shape)
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), i


@pytest.fixture(scope="module")
def tables():
    import __graft_entry__ as entry
    from prisma_amd import engine
    entry.build()
    return {g: engine.gm_tables(*g) for g in ALL_GRIDS}


@pytest.mark.parametrize("grid", ALL_GRIDS, ids=lambda g: "%dx%d" % g)
def test_region_table_gives_the_reference_mask(tables, grid):
    """shift_regions (the function prepare_g uploads from) -> exactly generate_shift_window_attn_mask's 0 / -100 pattern"""
    h8, w8 = grid
    reg = tables[grid][1]
    want = R.G.shift_mask(h8, w8, h8 // 2, w8 // 2).numpy()
    assert np.array_equal(R.region_mask(reg), want)
    assert np.array_equal(reg, R.regions_restated(h8, w8))
    if h8 * w8 <= 2048:
        assert not np.array_equal(R.region_mask(R.regions_restated(h8, w8, "region_edge")), want)


@pytest.mark.parametrize("grid", ALL_GRIDS, ids=lambda g: "%dx%d" % g)
def test_position_table_vs_float64(tables, grid):
    """sine_positions (fp32 on the host) within 3 2^-24 |arg| + 2^-22 of float64"""
    pos = tables[grid][0]
    truth, arg = R.positions_truth(*grid)
    assert arg.max() <= 2 * np.pi
    w, i = worst(np.abs(pos.astype(np.float64) - truth), R.positions_tolerance(arg))
    print("\n  %dx%d position table: worst err / tol %.3f at %s, max |err| %.2e" % (grid + (w, i, np.abs(pos - truth).max())), end="")
    assert w <= 1
    # ... and it is the reference's own table to fp32 noise (its position_sine runs in float32)
    h8, w8 = grid
    ref = R.G.position_sine(h8 // 2, w8 // 2).repeat(1, 2, 2).permute(1, 2, 0).reshape(h8 * w8, 128).numpy()
    assert np.abs(ref - truth).max() < 4e-6


@pytest.mark.parametrize("grid", R.GRIDS + [(4, 6)], ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("shifted", [0, 1])
def test_win_rows_is_roll_plus_split(grid, shifted):
    h8, w8 = grid
    want = R.win_rows_oracle(h8, w8, 3, bool(shifted))
    assert np.array_equal(R.win_rows(h8, w8, 3, bool(shifted)), want)
    for bug in ("wywx",) + (("shift_up", "roll_dir") if shifted else ()):
        if bug == "shift_up" and (h8 // 2) % 2 == 0 and (w8 // 2) % 2 == 0:
            continue                                        # even windows: rounding up changes nothing
        if bug == "roll_dir" and h8 == 4 and w8 == 4:
            continue                                        # a roll by half the map is its own inverse
        if bug == "wywx" and h8 == w8:
            assert not np.array_equal(R.win_rows(h8, w8, 3, bool(shifted), bug), want)
            continue
        assert not np.array_equal(R.win_rows(h8, w8, 3, bool(shifted), bug), want), bug


# ---------------------------------------------------------------------------------------------------------------------
# window block chain
# ---------------------------------------------------------------------------------------------------------------------
WINDOW_GRIDS = [(6, 10), (18, 26)]          # (28, 38) runs on the card; here it would only repeat the same code on more data


@pytest.mark.parametrize("grid", WINDOW_GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("shifted,cross", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_window_block_restated_vs_oracle_and_bugs(grid, shifted, cross):
    h8, w8 = grid
    images = 4
    Y, X, gamma, beta = R.window_data(100 + h8, images, h8, w8)
    truth = R.window_truth(Y, h8, w8, images, shifted, cross).reshape(-1, 128)
    t = R.window_restated(Y, h8, w8, images, shifted, cross)
    assert np.abs(t["o"] - truth).max() < 1e-12
    if shifted:
        # windows 1..3 of a shifted map mix regions: a test that ignored the mask would not pass
        print("\n  %dx%d masked (query, key) share per window %s" % (h8, w8, np.round(t["masked_share"], 2)), end="")
        assert (t["masked_share"][1:] >= 0.40).all() and t["masked_share"][0] == 0
    ref = R.window_block_truth(t["o"], X, gamma, beta)
    tol = R.window_block_tolerance(t, X, gamma, beta)
    # (wy / wx swapped in the gather AND the scatter only renames windows 1 and 2: it shows where the region table's rows are per window,
    # and in the byte-exact pack test)
    bugs = (["wywx", "roll_dir", "region_edge"] if shifted else []) + (["no_partner"] if cross else [])
    if shifted and ((h8 // 2) % 2 or (w8 // 2) % 2):
        bugs.append("shift_up")
    for bug in bugs:
        b = R.window_restated(Y, h8, w8, images, shifted, cross, bug)
        w, i = worst(np.abs(R.window_block_truth(b["o"], X, gamma, beta) - ref), tol)
        print("\n  %dx%d shifted %d cross %d bug %-11s moves element %s by %.0f tolerances" % (h8, w8, shifted, cross, bug, i, w), end="")
        assert w >= SEE, bug


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def test_ln_tolerance_sees_the_bugs_and_the_data_is_hard():
    M, gamma, beta = R.ln_data(7, 1003)
    y, mean, se = R.ln_truth(M, gamma, beta)
    ratio = np.abs(mean[:, 0]) / np.sqrt(se[:, 0] ** 2 - R.EPS_LN)
    assert (ratio >= 100).sum() >= 100 and (ratio >= 2500).sum() >= 50
    assert (se[:, 0] ** 2 < 3 * R.EPS_LN).sum() >= 50          # rows where eps is a third of the denominator or more
    tol = R.ln_tolerance(M, gamma, beta)
    w, i = worst(np.abs(R.ln_restated(M, gamma, beta) - y), tol)
    print("\n  ln restated (numpy fp32) vs float64: worst err / tol %.3f at %s" % (w, i), end="")
    assert w <= 1
    for bug in ("one_pass", "no_eps", "var127"):
        w, i = worst(np.abs(R.ln_restated(M, gamma, beta, bug) - y), tol)
        print("\n  ln bug %-8s moves element %s by %.0f tolerances" % (bug, i, w), end="")
        assert w >= SEE, bug


def test_cat_row_swap_changes_bytes():
    M, gamma, beta = R.ln_data(8, 64)
    y16 = R.split16(R.ln_restated(M, gamma, beta))
    a, b = R.cat_rows_restated(M, y16), R.cat_rows_restated(M, y16, "cat_swap")
    assert a.shape == (64, 512) and not np.array_equal(a.view(np.uint16), b.view(np.uint16))


# ---------------------------------------------------------------------------------------------------------------------
# matching, propagation
# ---------------------------------------------------------------------------------------------------------------------
MATCH_GRIDS = [(4, 6), (18, 26)]


@pytest.mark.parametrize("grid", MATCH_GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("dirs", [1, 2])
def test_match_restated_vs_oracle_and_bugs(grid, dirs):
    h8, w8 = grid
    tok = R.match_tokens(300 + h8, 2, h8, w8)
    flow, t = R.match_restated(tok, h8, w8, dirs)
    assert np.abs(flow - R.match_truth_oracle(tok, h8, w8, dirs)).max() < 1e-10
    big = max(h8, w8) - 1
    rng_flow = np.abs(flow).max()
    print("\n  %dx%d dirs %d: flow range %.2f px under coordinates up to %d" % (h8, w8, dirs, rng_flow, big), end="")
    assert rng_flow >= 1.0                      # not a zero flow ...
    if big >= 10:
        assert rng_flow <= big / 10.0           # ... and small against the coordinates it is the difference of (a 4 x 6 grid has none that large)
    tol = R.match_tolerance(t, h8, w8)
    for bug in ("own_xy",):
        w, i = worst(np.abs(R.match_restated(tok, h8, w8, dirs, bug)[0] - flow), tol)
        print("\n  %dx%d dirs %d bug %-7s moves element %s by %.0f tolerances" % (h8, w8, dirs, bug, i, w), end="")
        assert w >= SEE, bug
    # the byte-exact match_flow test meets the swap too
    O = np.zeros((1, h8 * w8, 32), np.float32)
    assert not np.array_equal(R.match_flow_restated(O, w8), R.match_flow_restated(O, w8, "own_xy"))


def test_propagate_truth_is_the_oracle_s_flow_attention():
    """gm_ref.propagate_truth against oracle flow_attention with identity projections"""
    import torch
    h8, w8 = 6, 10
    q, k, X, flow = R.propagate_data(5, 1, h8, w8)
    t = R.propagate_truth(q, k, flow, 2)
    # flow_attention projects q and k itself; with k given, its arithmetic is softmax(q k^T / sqrt(c)) v
    tq, tk, tv = (torch.from_numpy(a.astype(np.float64)) for a in (q, k, flow))
    ref = torch.matmul(torch.softmax(torch.matmul(tq, tk.permute(0, 2, 1)) / 128 ** 0.5, dim=-1), tv).numpy()
    assert np.abs(t["o"] - ref).max() < 1e-12
    assert (t["pd"] > 0.1).mean() > 0.5           # the rows are real averages, not one-hot picks


def test_attention_tolerance_sees_a_dropped_q_lo():
    """q rounded to fp16 (its lo part dropped) against the split-precision tolerance, on the data of the (split, split P V, 32 columns) GPU case"""
    q, k, v = R.attention_data(117 + 32, 4, 117, 32)
    t = R.attention_truth(q, k, v)
    b = R.attention_truth(q.astype(np.float16), k, v)
    w, i = worst(np.abs(b["o"] - t["o"]), R.attention_tolerance(t, True, True))
    print("\n  q lo dropped moves element %s by %.0f tolerances" % (i, w), end="")
    assert w >= SEE


def test_spiked_rows_pick_one_key():
    q, k, v = R.attention_data(11, 2, 117, 128)
    q, j = R.spiked(q, k)
    t = R.attention_truth(q, k, v)
    assert t["gap"].min() >= 50
    assert np.abs(t["o"] - v[:, j]).max() < 1e-15
