"""GPU: the kernels and launch forms the two-scale GMFlow adds to the flow_gmflow band, one by one (pb_op_gm_warp, pb_op_gm_upsample,
pb_op_gm_tokens_warped and the split-count forms pb_op_gm_tables_n / pack_n / ln_n / window_block_n: the engine's launchers with the engine's
arguments) against the float64 restatements of tests/gm_scale2_ref.py.  Element-wise forms byte for byte; the warp, the factor-4 convex
upsampling and the window block inside tolerances derived from their arithmetic (gm_scale2_ref module docstring: both new kernels are
fp32 FMA chains of a handful of terms - an error term for the weights times the spread of the values, a term for the accumulation;
gm_ref.window_block_tolerance for the chain).  Guard rows and pad columns stay untouched; the region table is exact.

measured (MI355X; worst error / tolerance): see the "measured:" line of every test.
"""
import numpy as np
import pytest

import gm_ref as R
import gm_scale2_ref as S
from gm_ref import check, preset, same_bytes
from prisma_amd import engine
from raft_ref import U24

pytestmark = pytest.mark.gpu
GUARD = 8
GRIDS4 = [(16, 24), (24, 40)]           # 8 x 8 windows of 2 x 3 tokens (Lw 6, the smallest) and of 3 x 5 (Lw 15: odd, shifts 1 and 2)
ENGINE_JOBS = [(0, 0), (128, 0), (256, 1), (384, 0), (512, 1)]


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


def gid(g):
    return "%dx%d" % g if isinstance(g, tuple) else str(g)


def halfs(raw):
    return np.ascontiguousarray(raw).view(np.float16)


@pytest.mark.parametrize("grid", GRIDS4 + [(208, 360)], ids=gid)
def test_tables_with_8_splits(grid):
    """the host tables of the fine scale: region ids equal generate_shift_window_attn_mask's regions exactly ([64, Lw], window order), the
    position table is one window's embedding tiled bit for bit and within the fp32 evaluation's error of float64.  (208, 360): 1080p x 0.75.
    measured: regions equal; positions <= 0.504 of the tolerance (208 x 360)."""
    h4, w4 = grid
    pos, reg = engine.gm_tables_n(h4, w4, 8)
    assert reg.shape == (64, (h4 // 8) * (w4 // 8)) and np.array_equal(reg, S.regions_n(h4, w4, 8))
    truth, arg = S.positions_n(h4, w4, 8)
    check("positions %s" % gid(grid), pos, truth, R.positions_tolerance(arg))
    p = pos.reshape(8, h4 // 8, 8, w4 // 8, 128)
    assert np.array_equal(p, np.broadcast_to(p[:1, :, :1], p.shape))
    two = engine.gm_tables_n(h4, w4, 2)
    same = engine.gm_tables(h4, w4)
    assert np.array_equal(two[0], same[0]) and np.array_equal(two[1], same[1])          # splits = 2 is the existing entry point's table


@pytest.mark.parametrize("grid", GRIDS4, ids=gid)
@pytest.mark.parametrize("dirs", [1, 2])
def test_warp_against_float64(ops, grid, dirs):
    """gm_warp on 2 pairs x dirs batch elements: flow_up = 2 x the align_corners enlargement, warped = the TARGET frame's features (frame
    pair + 1 - d) sampled at token + flow_up with zeros outside; the coarse flow is ~4 tokens + noise, so samples fall outside on every side.
    The warp is judged at the kernel's OWN flow_up (its error against float64 is the first assertion), so dflow = 0 plus the coordinate's
    rounding.  Guard rows untouched.
    measured: flow_up <= 0.028, warped <= 0.876."""
    h4, w4 = grid
    h8, w8 = h4 // 2, w4 // 2
    B = 2 * dirs
    g = R.rng(h4 + dirs)
    flow8 = (np.array([4.0, -3.0]) * np.where(np.arange(B) % 2, -1, 1)[:, None, None] + 2.0 * g.standard_normal((B, h8 * w8, 2))).astype(np.float32)
    feat4 = (g.standard_normal((3, h4 * w4, 128)) * 2).astype(np.float32)
    up, wp = ops.gm_warp(flow8, feat4, h8, w8, dirs, GUARD)
    n = B * h4 * w4
    preset("warp flow_up guard rows", up[n:])
    preset("warp warped guard rows", wp[n:])
    up, wp = up[:n].reshape(B, h4 * w4, 2), wp[:n].reshape(B, h4 * w4, 128)
    t = S.enlarge2_restated(flow8, h8, w8)
    check("flow_up %s dirs %d" % (gid(grid), dirs), up, t["o"], S.enlarge2_tolerance(t, h8, w8))
    tgt = np.array([b // dirs + 1 - b % dirs for b in range(B)])
    tw = S.warp_restated(feat4[tgt], up, h4, w4)
    assert tw["outside"].mean() > 0.05
    check("warped %s dirs %d" % (gid(grid), dirs), wp, tw["o"], S.warp_tolerance(tw, 0.0))
    wrong = S.warp_restated(feat4[tgt[::-1]], up, h4, w4)["o"] if dirs == 2 else S.warp_restated(feat4[tgt - 1], up, h4, w4)["o"]
    assert (np.abs(wp - wrong) > 100 * S.warp_tolerance(tw, 0.0)).any()                 # the source frame, or the other direction's, would show


def test_warp_far_outside_and_large_grid(ops):
    """flows of +-1e6, 1e30 and NaN keep every tap outside (zeros, no read); a 104 x 180 -> 208 x 360 grid (1080p x 0.75) runs more blocks
    than one wave of CUs.  measured: zeros; large grid 0.914."""
    h8, w8 = 8, 12
    flow8 = np.zeros((4, h8 * w8, 2), np.float32)
    flow8[0], flow8[1], flow8[2, :, 0], flow8[3, :, 1] = 1e6, -1e6, 1e30, np.nan
    feat4 = np.ones((5, 4 * h8 * w8, 128), np.float32)
    up, wp = ops.gm_warp(flow8, feat4, h8, w8, 1, GUARD)
    assert not wp[:4 * 4 * h8 * w8].any()
    preset("warp guard rows", wp[4 * 4 * h8 * w8:])
    h8, w8 = 104, 180
    g = R.rng(7)
    flow8 = (3.0 * g.standard_normal((1, h8 * w8, 2))).astype(np.float32)
    feat4 = g.standard_normal((2, 4 * h8 * w8, 128)).astype(np.float32)
    up, wp = ops.gm_warp(flow8, feat4, h8, w8, 1, GUARD)
    n = 4 * h8 * w8
    tw = S.warp_restated(feat4[1:], up[:n][None], 2 * h8, 2 * w8)
    check("warped 208x360", wp[:n][None], tw["o"], S.warp_tolerance(tw, 0.0))
    preset("warp guard rows", wp[n:])


@pytest.mark.parametrize("grid,pads", [((16, 24), (0, 0, 64, 96)), ((24, 40), (3, 5, 90, 150)), ((7, 9), (1, 2, 25, 31))], ids=str)
def test_upsample_factor_4_against_float64(ops, grid, pads):
    """upsample_kernel<4>: four 1/4-grid pixels per wave, mask rows of 144; with the unpad window (pad_l, pad_t, sh, sw), an odd grid whose
    pixel count is no multiple of 4, and the maximum displacement.  Guard floats untouched.
    measured: <= 0.349; the maximum displacement within 4 x 2^-24 of the float64 norm's maximum."""
    h, w = grid
    pad_l, pad_t, sh, sw = pads
    g = R.rng(h * w)
    n = 3
    flow = (np.array([-6.0, 9.0]) + 3.0 * g.standard_normal((n, h * w, 2))).astype(np.float32)
    logits = (2.5 * g.standard_normal((n, h * w, 144))).astype(np.float32)
    up, mx = ops.gm_upsample(flow, logits, h, w, 4, pad_l, pad_t, sh, sw, 16)
    preset("upsample guard", up[n * sh * sw * 2:])
    up = up[:n * sh * sw * 2].reshape(n, sh, sw, 2)
    t = S.upsample_restated(flow, logits, h, w, 4)
    cut = lambda a: a[:, pad_t:pad_t + sh, pad_l:pad_l + sw]
    check("upsample x4 %s" % gid(grid), up, cut(t["o"]), cut(S.upsample_tolerance(t)))
    norm = np.sqrt((up.astype(np.float64) ** 2).sum(-1)).reshape(n, -1).max(1)
    assert np.abs(mx - norm).max() <= 4 * U24 * norm.max()
    assert (np.abs(up - cut(S.upsample_restated(flow, logits, h, w, 4, bug="times8")["o"])) > 100 * cut(S.upsample_tolerance(t))).any()


def test_upsample_factor_8_form_is_the_existing_kernel(ops):
    """pb_op_gm_upsample with factor 8 and pb_op_raft_upsample give the same bytes (one template, K = 8)"""
    h, w = 6, 10
    g = R.rng(3)
    flow = g.standard_normal((2, h * w, 2)).astype(np.float32) * 4
    mask = g.standard_normal((2, h * w, 576)).astype(np.float32)
    up, mx = ops.gm_upsample(flow, mask, h, w, 8, 2, 1, 44, 75, 16)
    up8, mx8 = np.empty_like(up), np.empty_like(mx)
    engine.check(ops.lib.pb_op_raft_upsample(ops.ctx, engine._ptr(flow), engine._ptr(mask), 2, h, w, 2, 1, 44, 75, 16, engine._ptr(up8), engine._ptr(mx8)))
    assert np.array_equal(up.view(np.uint32), up8.view(np.uint32)) and np.array_equal(mx, mx8)


@pytest.mark.parametrize("dirs", [1, 2])
def test_tokens_warped_bytes(ops, dirs):
    """gm_tokens' fine-scale form: image 2 b = frame b // dirs + b % dirs + pos, image 2 b + 1 = warped[b] + pos, X and its split copy byte
    for byte.  measured: equal."""
    h4, w4 = 16, 24
    P, B = h4 * w4, 2 * dirs
    g = R.rng(dirs)
    feat = g.standard_normal((3, P, 128)).astype(np.float32) * 3
    warped = g.standard_normal((B, P, 128)).astype(np.float32) * 3
    pos = engine.gm_tables_n(h4, w4, 8)[0]
    X, Xs = ops.gm_tokens_warped(feat, warped, pos, dirs, GUARD)
    src = np.stack([feat[[b // dirs + b % dirs for b in range(B)]], warped], 1).reshape(2 * B, P, 128)
    want = (src + pos[None]).astype(np.float32).reshape(-1, 128)
    rows = 2 * B * P
    same_bytes("tokens_warped X", X[:rows], want)
    same_bytes("tokens_warped Xs", halfs(Xs[:rows]), R.split_rows(want))
    preset("tokens_warped guard rows", X[rows:])
    preset("tokens_warped Xs guard rows", Xs[rows:])


@pytest.mark.parametrize("grid", GRIDS4, ids=gid)
@pytest.mark.parametrize("shifted", [0, 1])
def test_pack_and_ln_bytes_with_8_splits(ops, grid, shifted):
    """gm_pack's five engine jobs and gm_ln's windowed forms over 64 windows per image (2 images: Bw = 128): window rows, V^T (pad columns
    [Lw, 32) zero) byte for byte against gm_ref's restatements on the 8-split row map; the LayerNorm's scatter against float64 inside
    gm_ref.ln_tolerance and its split copy byte for byte; guard rows untouched.
    measured: pack equal; ln <= 0.358."""
    h4, w4 = grid
    g = engine.gm_geometry(h4, w4, 8)
    images = 2
    src = R.rng(g["P"] + shifted).standard_normal((images * g["P"], 640)).astype(np.float32) * 2
    rows = S.win_rows_n(h4, w4, 8, images, bool(shifted))
    outs = ops.gm_pack_n(src, h4, w4, 8, ENGINE_JOBS, bool(shifted), GUARD)
    for (col, vt), raw in zip(ENGINE_JOBS, outs):
        what = "pack_n %s shifted %d column %d %s" % (gid(grid), shifted, col, "vt" if vt else "rows")
        n = images * 64 * (256 if vt else g["Lw"])
        want = R.pack_vt_restated(src, col, rows, g["ldv"]) if vt else R.pack_rows_restated(src, col, rows)
        same_bytes(what, halfs(raw[:n]), want)
        if vt:
            assert not halfs(raw[:n]).reshape(-1, g["ldv"])[:, g["Lw"]:].any(), what + ": pad columns"
        preset(what + " guard rows", raw[n:])
    # gm_ln, windowed, mode 0: row r of M is window-order row r, added to token row rows[r] of X (tolerance and byte checks of
    # tests/test_gpu_gmflow_ops.py test_ln)
    n = images * g["P"]
    M, gamma, beta = R.ln_data(40 + h4, n)
    X = R.rng(50 + shifted).standard_normal((n, 128)).astype(np.float32)
    Xa, raw = ops.gm_ln_n(M, gamma, beta, X, h4, w4, 8, True, bool(shifted), 0, GUARD)
    gr = rows.reshape(-1)
    assert np.array_equal(np.sort(gr), np.arange(n))
    ref = X[gr].astype(np.float64) + R.ln_truth(M, gamma, beta)[0]
    what = "ln_n %s shifted %d" % (gid(grid), shifted)
    check(what + " X vs float64", Xa[gr], ref, R.ln_tolerance(M, gamma, beta) + U24 * np.abs(ref))
    same_bytes(what + ": split copy of its own X", halfs(raw)[gr], R.split_rows(Xa[gr]))
    preset(what + " X guard rows", Xa[n:])
    preset(what + " out guard rows", raw[n:])


@pytest.mark.parametrize("grid", GRIDS4, ids=gid)
@pytest.mark.parametrize("shifted,cross", [(1, 0), (0, 1), (1, 1)])
def test_window_block_with_8_splits(ops, grid, shifted, cross):
    """pack -> window attention (64 windows per image, region table [64, Lw], kxor 64 when cross) -> gm_ln on 4 images (Bw = 256), against
    the reference's single_head_split_window_attention with num_splits 8 on float64 tensors + float64 LayerNorm + X.  The attention is the
    one a two-scale context launches with 8 splits: q / k AND P / V split (pv_single 0), judged inside the tolerance of that form
    (gm_scale2_ref.window_block_tolerance_n, pv_split: the P V term is BUDGET[SPLIT16], not the fp16 one of the one-scale model's window
    attention).  16 x 24: Lw = 6; 24 x 40: Lw = 15.
    measured: <= 0.055 (with pv_single 1 and the fp16 form's tolerance the same cases gave <= 0.249)."""
    h4, w4 = grid
    images = 4
    Y, X, gamma, beta = R.window_data(200 + h4, images, h4, w4)
    got = ops.gm_window_block_n(Y, X, gamma, beta, h4, w4, 8, bool(shifted), bool(cross), pv_single=False)
    t = S.window_restated_n(Y, h4, w4, 8, images, shifted, cross)
    o = S.window_truth_n(Y, h4, w4, 8, images, shifted, cross).reshape(-1, 128)
    assert np.abs(t["o"] - o).max() < 1e-12
    check("window_block_n %s shifted %d cross %d vs float64" % (gid(grid), shifted, cross), got, R.window_block_truth(o, X, gamma, beta),
          S.window_block_tolerance_n(t, X, gamma, beta, True))


def test_window_block_n_with_2_splits_is_the_existing_op(ops):
    """splits 2 and pv_single 1 is pb_op_gm_window_block (the one-scale model's block), byte for byte; pv_single 0 on the same data is the
    coarse scale of a two-scale context, inside the pv-split tolerance.  measured: equal; 0.028."""
    h8, w8 = 12, 20
    images = 2
    Y, X, gamma, beta = R.window_data(77, images, h8, w8)
    one = ops.gm_window_block(Y, X, gamma, beta, h8, w8, True, True)
    same_bytes("window_block_n splits 2 pv_single 1", ops.gm_window_block_n(Y, X, gamma, beta, h8, w8, 2, True, True, pv_single=True), one)
    t = S.window_restated_n(Y, h8, w8, 2, images, True, True)
    check("window_block_n 12x20 splits 2 pv split vs float64", ops.gm_window_block_n(Y, X, gamma, beta, h8, w8, 2, True, True, pv_single=False),
          R.window_block_truth(t["o"], X, gamma, beta), S.window_block_tolerance_n(t, X, gamma, beta, True))
