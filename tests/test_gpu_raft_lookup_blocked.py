"""GPU: flow_raft's source-blocked correlation volume (csrc/corr_layout.h; pb_set_option "corr_layout" 1, the default) against the row-major
one (0).  The layout changes where the volume's bytes sit and how the lookup fetches them, nothing else, so every comparison here is
array_equal: the lookup's raw output rows (fp16 part, e4m3 copy, the untouched halfs 324..383 and the guard rows), the volume kernel's entries
de-blocked with the header's own index function, and the band's flow / RGB / max displacement."""
import os

import numpy as np
import pytest

import raft_ref as R
from prisma_amd import engine, synth
from prisma_amd._lib import PrismaBandsError

pytestmark = pytest.mark.gpu
GUARD = 8
GRIDS = [g for g in R.LOOKUP_GRIDS if g[0] in ("16x16", "17x23", "129x17x2")]
assert len(GRIDS) == 3


def flow_families(seed, n, h8, w8):
    """{family: [n P, 2] float32}"""
    g = np.random.default_rng(seed)
    P = h8 * w8
    rows = n * P
    p = np.arange(rows) % P
    px, py = (p % w8).astype(np.float64), (p // w8).astype(np.float64)
    fam = {"zero": np.zeros((rows, 2))}
    fam["translation"] = np.tile(np.array([[0.37, -1.61]]), (rows, 1))           # coherent: the 8 pixels of a group want the same tiles
    fam["random"] = g.standard_normal((rows, 2)) * 20.0                           # several tiles' amplitude: every pixel its own tiles
    # level 0: the window's first column is floor(px + fx) - 4 and its first row floor(py + fy) - 4; put both at offsets 6 / 7 of a tile, which
    # makes the window reach a third tile column / row.  (x + 4) & 7 in {6, 7} <=> x & 7 in {2, 3}
    want = g.integers(2, 4, (rows, 2)).astype(np.float64)
    base = np.stack([px, py], 1)
    fam["third_tile"] = ((want - base) % 8.0) + g.uniform(0.05, 0.95, (rows, 2)) - 8.0 * g.integers(0, 2, (rows, 2))
    x0 = np.floor(base + fam["third_tile"]) - 4
    assert (np.mod(x0, 8) >= 6).all()
    fam["far"] = np.where(g.random((rows, 2)) < 0.5, -1.0, 1.0) * g.uniform(3e3, 5e4, (rows, 2))      # outside every level: all zeros
    if h8 == 129:
        fam["down"] = R.downward_flows(2100, n, h8, w8)       # windows reach the padded rows 136, 137 behind the level's last one
    return {k: np.ascontiguousarray(v, np.float32) for k, v in fam.items()}


@pytest.fixture(scope="module")
def ops():
    a, b = engine.Ops(0), engine.Ops(0)
    a.set_option("corr_layout", 0)
    yield a, b                                               # (row-major, default = blocked)
    a.close()
    b.close()


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: g[0])
def test_lookup_rows_equal_in_both_layouts(ops, grid):
    """16x16: P = 256, whole groups of 8; 17x23: P = 391, a partial last group, no level a multiple of 8; 129x17x2: two pair-directions
    (a group must not straddle them), windows past the last padded row."""
    rowmajor, blocked = ops
    name, n, h8, w8, _, _ = grid
    rows = n * h8 * w8
    f1, f2 = R.lookup_features(1000 + h8 * w8, n, h8, w8)
    for k, (fam, fl) in enumerate(flow_families(77 + h8, n, h8, w8).items()):
        o8 = k % 2 == 0
        a, la = rowmajor.raft_lookup(f1, f2, fl, o8=o8, guard_rows=GUARD, want_levels=k == 0)
        b, lb = blocked.raft_lookup(f1, f2, fl, o8=o8, guard_rows=GUARD, want_levels=k == 0)
        assert np.array_equal(a, b), "%s %s: raw rows differ, first at %s" % (name, fam, tuple(np.argwhere(a != b)[0]))
        assert (a[rows:] == 0xFF).all() and (a[:rows, 648:768] == 0xFF).all()
        vals = a.view(np.float16)[:rows, :324]
        if fam == "far":
            assert not vals.view(np.uint16).any(), "%s far: a window outside every level must be all zeros" % name
        elif fam != "down":
            assert np.abs(vals.astype(np.float32)).max() > 0.1, "%s %s: the lookup returned (almost) nothing" % (name, fam)
        if k == 0:      # the de-blocked levels are the row-major kernel's, bit for bit
            for l in range(4):
                assert np.array_equal(la[l].view(np.uint32), lb[l].view(np.uint32)), "%s level %d" % (name, l)


@pytest.mark.parametrize("N", [64, 192, 448])
def test_volume_blocked_equals_rowmajor(ops, N):
    """M = 391 (a partial last group of 8, a partial last 32-row wave); the entries de-blocked on the host with corr_layout.h's index function;
    row 391 of the last group (which does not exist) and everything behind it keep their preset"""
    o = ops[1]
    M, guard = 391, 4096
    g = np.random.default_rng(N)
    A = g.standard_normal((M, 256)).astype(np.float32)
    W = g.standard_normal((N, 256)).astype(np.float32)
    want = o.corr_volume(A, W, ldo=N, guard_rows=0)
    raw = o.corr_volume_blocked(A, W, ldo=N, guard_halfs=guard)
    idx = engine.corr_layout_index(1, M, N)
    assert raw.size == 392 * N + guard and idx.max() < 392 * N
    got = raw[idx].astype(np.float32)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want), "first at %s" % (tuple(np.argwhere(got != want)[0]),)
    rest = np.ones(raw.size, bool)
    rest[idx.ravel()] = False
    assert rest.sum() == N + guard and (raw.view(np.uint16)[rest] == 0x7E7E).all(), "the kernel wrote behind row %d" % (M - 1)


@pytest.fixture(scope="module")
def weights():
    return synth.raft_weights(seed=4321)


def run(net, fr, iters):
    flow, rgb, mx = net.infer_sequence(fr, scale=1.0, iters=iters, backward=True)
    return flow.view(np.uint32).copy(), np.array(rgb, copy=True), np.asarray(mx, np.float32).view(np.uint32).copy()


def same(a, b, what):
    for x, y, k in zip(a, b, ("flow", "rgb", "max displacement")):
        assert np.array_equal(x, y), "%s: %s differs" % (what, k)


def test_band_equal_in_both_layouts_and_switch_replans(weights, golden_dir):
    """the 125 x 157 golden pair (P = 320) and a 3-frame call, both directions: a "corr_layout" 0 context against a default one; then the
    option switched on the live contexts, which must re-plan and give the other context's bytes"""
    z = np.load(os.path.join(golden_dir, "raft_125x157.npz"))
    h, w = [int(v) for v in z["hw"]]
    pair = synth.frame_pair_sequence(2, h, w, seed=int(z["frame_seed"]))
    three = synth.frame_pair_sequence(3, 136, 168, seed=12)                   # 17 x 21: P = 357, a partial last group per pair-direction
    row = engine.FlowRaft(weights, device=0, precision=1)
    blk = engine.FlowRaft(weights, device=0, precision=1)
    try:
        row.set_option("corr_layout", 0)
        for fr, iters, what in ((pair, int(z["iters"]), "125x157"), (three, 4, "3 frames")):
            a, b = run(row, fr, iters), run(blk, fr, iters)
            same(a, b, what)
            assert a[0].any()
        want = run(blk, three, 4)
        row.set_option("corr_layout", 1)
        same(run(row, three, 4), want, "row-major context switched to blocked")
        assert row.arena_bytes() == blk.arena_bytes()
        blk.set_option("corr_layout", 0)
        same(run(blk, three, 4), want, "blocked context switched to row-major")
        with pytest.raises(PrismaBandsError, match="option 'corr_layout' is 0 or 1, not 2"):
            blk.set_option("corr_layout", 2)
    finally:
        row.close()
        blk.close()
