"""GPU: the flow_gmflow band's local matching and local-window propagation kernels (gmflow_local.hip) through their op entry points -
the engine's launchers with the engine's arguments - against the float64 restatements of tests/gm_local_ref.py (pinned to the real
reference by tests/test_gm_local_ref_cpu.py), inside the tolerance derived there from the kernels' arithmetic.  Grids: the window larger
than the image, odd windows, a grid that is no multiple of the 8 x 8 query tile, several tiles with a tail.  The inputs sit on large
common offsets (tokens mostly offset, 40 px of common motion), so an accumulation that cancels would show.  Raw buffers arrive preset to
0xFF: the guard rows, and for the propagation columns 2 .. 31 of every row, must still be.

measured (MI355X; worst error / tolerance per case): see the "measured:" line of every test.  The kernels' own source text built for the
host (one thread per lane, barriers and shuffles emulated, address and undefined-behaviour sanitizers on) gave 0.001 .. 0.016 (matching)
and 0.011 .. 0.18 (propagation) on the same cases, nothing outside the rows and columns the kernels own.
"""
import numpy as np
import pytest

import gm_local_ref as L
import gm_ref as R
from gm_ref import check, preset
from prisma_amd import engine

pytestmark = pytest.mark.gpu
GUARD = 8
NP = 2


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


def gid(g):
    return "%dx%d" % g if isinstance(g, tuple) else str(g)


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("radius", [1, 4])
@pytest.mark.parametrize("grid", R.GRIDS, ids=gid)
def test_local_match(ops, grid, radius, dirs):
    """gm_local_match_kernel, two pairs: batch element (pair, dir) matches image 2 pair + dir against the other image of its pair.
    measured: worst err / tol 0.001 .. 0.007 over the 16 cases (worst 28x38 R 4 dirs 2)."""
    h8, w8 = grid
    tok = L.match_tokens(h8 * 100 + w8, NP, h8, w8)
    raw = ops.gm_local_match(tok, h8, w8, dirs, radius, GUARD)
    n = NP * dirs * h8 * w8
    t = L.local_match_restated(tok, h8, w8, dirs, radius)
    check("local_match %s R %d dirs %d" % (gid(grid), radius, dirs), raw[:n].reshape(NP * dirs, h8 * w8, 2), t["o"], L.local_tolerance(t, radius))
    preset("local_match guard rows", raw[n:])


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("grid", R.GRIDS, ids=gid)
def test_local_propagate(ops, grid, radius, dirs):
    """gm_local_prop_kernel as the engine launches it: batch element b reads image b (both directions) or 2 b (forward only) of q and k.
    measured: worst err / tol 0.011 .. 0.180 over the 16 cases (worst 18x26 r 1 dirs 2)."""
    h8, w8 = grid
    B, step = NP * dirs, 1 if dirs == 2 else 2
    q, k, flow = L.prop_data(h8 * 100 + w8 + 7, B * step, h8, w8, B)
    raw = ops.gm_local_propagate(q, k, flow, h8, w8, step, radius, GUARD)
    n = B * h8 * w8
    t = L.local_prop_restated(q[::step], k[::step], flow, h8, w8, radius)
    check("local_propagate %s r %d dirs %d" % (gid(grid), radius, dirs), raw[:n, :2].reshape(B, h8 * w8, 2), t["o"], L.local_tolerance(t, radius))
    preset("local_propagate columns 2 .. 31", raw[:n, 2:])
    preset("local_propagate guard rows", raw[n:])


def test_radii_outside_the_kernels_are_errors(ops):
    tok = L.match_tokens(1, 1, 4, 4)
    q, k, flow = L.prop_data(2, 1, 4, 4, 1)
    for r in (0, 5):
        with pytest.raises(engine._lib.PrismaBandsError, match="radius"):
            ops.gm_local_match(tok, 4, 4, 1, r, GUARD)
    for r in (0, 3):
        with pytest.raises(engine._lib.PrismaBandsError, match="radius"):
            ops.gm_local_propagate(q, k, flow, 4, 4, 1, r, GUARD)
