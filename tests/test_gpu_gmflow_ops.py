"""GPU: the flow_gmflow band's own kernels one by one (pb_op_gm_*, pb_op_attention128_cfg: the engine's launchers with the engine's
arguments) against tests/gm_ref.py - (1) bytes: what an element-wise kernel owns equals a restatement that rounds where the kernel rounds,
what it does not own is still preset; (2) gm_ln and attention128.hip, as GmflowEngine::infer configures it, against float64 inside
tolerances derived from the arithmetic; (3) the engine's three launch chains with the GEMMs left out against the reference's own functions
(oracle/gmflow_oracle.py on float64 tensors).  A failure names the op, the case and the element.  tests/test_gm_ref_cpu.py holds the CPU
side: the host tables, the index maps against torch.roll + split_feature, and that the tolerances see the planted bugs.

measured (MI355X; worst error / tolerance per op): see the "measured:" line of every test.
"""
import numpy as np
import pytest

import gm_ref as R
from gm_ref import check, preset, same_bytes
from prisma_amd import engine

pytestmark = pytest.mark.gpu
GUARD = 8
ENGINE_JOBS = [(0, 0), (128, 0), (256, 1), (384, 0), (512, 1)]          # GmflowEngine::infer: q, k, v^T of the self attention, k, v^T of the cross attention


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


def gid(g):
    return "%dx%d" % g if isinstance(g, tuple) else str(g)


def halfs(raw):
    return np.ascontiguousarray(raw).view(np.float16)


# ---------------------------------------------------------------------------------------------------------------------
# bytes: tokens, split_rows, pack, grid_vt, match_flow, upsampler_in
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(4, 4), (28, 38), R.LARGE], ids=gid)
def test_tokens_bytes(ops, grid):
    """gm_tokens on a 3-frame feature stack: pair n holds frames n and n + 1 plus the production position table; X and its split copy byte
    for byte, guard rows untouched.
    measured: equal on all three grids."""
    h8, w8 = grid
    P = h8 * w8
    feat = R.rng(P).standard_normal((3, P, 128)).astype(np.float32) * 3
    pos = engine.gm_tables(h8, w8)[0]
    X, Xs = ops.gm_tokens(feat, pos, GUARD)
    rows = 4 * P
    want = R.tokens_restated(feat, pos)
    same_bytes("tokens %s X" % gid(grid), X[:rows], want)
    same_bytes("tokens %s Xs" % gid(grid), halfs(Xs[:rows]), R.split_rows(want))
    preset("tokens X guard rows", X[rows:])
    preset("tokens Xs guard rows", Xs[rows:])


@pytest.mark.parametrize("ld", [128, 160])
def test_split_rows_bytes(ops, ld):
    """gm_split_rows, 1003 rows of 128 columns out of ld (the engine's ld = C and a wider source): [hi | lo] byte for byte.  The values span
    fp16's range: subnormal his (|v| < 6e-5), los that underflow to zero.
    measured: equal."""
    g = R.rng(ld)
    src = (g.standard_normal((1003, ld)) * 10.0 ** g.uniform(-7, 3, (1003, ld))).astype(np.float32)
    raw = ops.gm_split_rows(src, 128, GUARD)
    same_bytes("split_rows ld %d" % ld, halfs(raw[:1003]), R.split_rows(src[:, :128]))
    preset("split_rows guard rows", raw[1003:])


@pytest.mark.parametrize("grid", [(4, 4), (6, 10), (28, 38)], ids=gid)
@pytest.mark.parametrize("shifted", [0, 1])
def test_pack_bytes(ops, grid, shifted):
    """gm_pack: the engine's five jobs on an ld = 640 matrix of 2 pairs (Bw = 16) in ONE launch, then its one-job launch on an ld = 128
    matrix.  Window rows and V^T byte for byte (the V^T columns [Lw, ldv) zero), guard rows untouched.
    measured: equal for every grid and both shift states."""
    h8, w8 = grid
    g = R.geom(h8, w8)
    images = 4
    src = R.rng(g["P"] + shifted).standard_normal((images * g["P"], 640)).astype(np.float32) * 2
    rows = R.win_rows(h8, w8, images, bool(shifted))
    outs = ops.gm_pack(src, h8, w8, ENGINE_JOBS, bool(shifted), GUARD)
    for (col, vt), raw in zip(ENGINE_JOBS, outs):
        what = "pack %s shifted %d column %d %s" % (gid(grid), shifted, col, "vt" if vt else "rows")
        n = images * 4 * (256 if vt else g["Lw"])
        want = R.pack_vt_restated(src, col, rows, g["ldv"]) if vt else R.pack_rows_restated(src, col, rows)
        same_bytes(what, halfs(raw[:n]), want)
        if vt:
            assert not halfs(raw[:n]).reshape(-1, g["ldv"])[:, g["Lw"]:].any(), what + ": pad columns"
        preset(what + " guard rows", raw[n:])
    one = ops.gm_pack(src[:, 256:384].copy(), h8, w8, [(0, 0)], bool(shifted), GUARD)[0]
    same_bytes("pack %s one job" % gid(grid), halfs(one[:images * 4 * g["Lw"]]), R.pack_rows_restated(src, 256, rows))
    preset("pack one job guard rows", one[images * 4 * g["Lw"]:])


@pytest.mark.parametrize("grid", R.GRIDS + [R.LARGE], ids=gid)
def test_grid_vt_bytes(ops, grid):
    """gm_grid_vt owns rows 0 and 1, columns < P, of the [64, ldvP] block: x and y of every token; everything else (the lo rows included:
    the engine's arena is zeroed once) still preset.
    measured: equal."""
    raw = ops.gm_grid_vt(grid[0], grid[1], GUARD)
    same_bytes("grid_vt %s" % gid(grid), halfs(raw), R.grid_vt_restated(grid[0], grid[1], GUARD))


@pytest.mark.parametrize("grid", [(4, 4), (28, 38), R.LARGE], ids=gid)
def test_match_flow_bytes(ops, grid):
    """gm_match_flow: flow = O[:, :2] - own coordinate in fp32, and its hi / lo rows 0, 1 / 32, 33 of the propagation's V^T; rows 2..31,
    34..63, the pad columns [P, ldvP) and the guard rows still preset (the stand-alone op does not zero the buffer).
    measured: equal."""
    h8, w8 = grid
    g = R.geom(h8, w8)
    B = 3
    r = R.rng(g["P"])
    O = r.standard_normal((B, g["P"], 32)).astype(np.float32)
    O[..., :2] = (R.coords(h8, w8)[None] + 1.5 * r.standard_normal((B, g["P"], 2))).astype(np.float32)
    flow, vt = ops.gm_match_flow(O, h8, w8, GUARD)
    want = R.match_flow_restated(O, w8)
    same_bytes("match_flow %s flow" % gid(grid), flow[:B * g["P"]].reshape(B, g["P"], 2), want)
    preset("match_flow flow guard rows", flow[B * g["P"]:])
    same_bytes("match_flow %s vt" % gid(grid), halfs(vt), R.flow_vt_restated(want, g["ldvP"], GUARD))


@pytest.mark.parametrize("grid", [(6, 10), R.LARGE], ids=gid)
@pytest.mark.parametrize("img_step", [1, 2])
def test_upsampler_in_bytes(ops, grid, img_step):
    """gm_upsampler_in: flow = O[:, :2]; the map [hi (192) | lo (192)] of cat(flow, feature of image b * img_step, zeros): channels 130..191
    zero in hi and lo, guard rows untouched.
    measured: equal."""
    h8, w8 = grid
    P, B = h8 * w8, 2
    r = R.rng(P + img_step)
    O = (r.standard_normal((B, P, 32)) * 5).astype(np.float32)
    X = r.standard_normal((B * img_step, P, 128)).astype(np.float32)
    flow, mp = ops.gm_upsampler_in(O, X, img_step, GUARD)
    same_bytes("upsampler_in flow", flow[:B * P].reshape(B, P, 2), O[..., :2])
    m = halfs(mp[:B * P])
    same_bytes("upsampler_in %s step %d map" % (gid(grid), img_step), m, R.upsampler_map_restated(O[..., :2], X, img_step))
    assert not m[:, 130:192].any() and not m[:, 322:384].any()
    preset("upsampler_in guard rows", mp[B * P:])
    preset("upsampler_in flow guard rows", flow[B * P:])


# ---------------------------------------------------------------------------------------------------------------------
# gm_ln
# ---------------------------------------------------------------------------------------------------------------------
def lo_half_step(y):
    """half a step of the lo part of a split pair holding y (|lo| <= half a step of the hi part)"""
    return 0.5 * R.f16_step(0.5 * R.f16_step(y))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("windowed,shifted", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_ln(ops, windowed, shifted, mode):
    """gm_ln on rows with |mean| / std up to 3000 and rows whose variance is near eps (gm_ref.ln_data), row counts that are no multiple of 4
    (a partial last block): 1003 rows as they come, or 239 of the 240 window-order rows of 4 images of a 6 x 10 grid.
    vs float64: |gamma| c 2^-24 (|mean| + |v|) / s + 2^-22 |y| with c = 8 + 18 z from the wave sum's depth (gm_ref.ln_tolerance), plus the
    fp32 add's rounding in mode 0 and half an fp16-lo step where y is read back from a split pair (mode 1).
    bytes: mode 0 - the split copy of the kernel's own X; mode 1 - X untouched, [hi X | . | lo X | .] the split of X; rows the launch does not
    address (the last window-order row, the guard rows) untouched in X and still preset in the output.
    measured: vs float64 <= 0.298 (mode 0), <= 0.195 (mode 1); bytes equal."""
    h8, w8 = 6, 10
    if windowed:
        xrows = 4 * h8 * w8
        rows = xrows - 1
        gr = R.win_rows(h8, w8, 4, bool(shifted)).reshape(-1)[:rows]
    else:
        xrows = rows = 1003
        gr = np.arange(rows)
    M, gamma, beta = R.ln_data(20 + windowed, rows)
    X = R.rng(30 + shifted).standard_normal((xrows, 128)).astype(np.float32)
    Xa, raw = ops.gm_ln(M, gamma, beta, X, h8, w8, bool(windowed), bool(shifted), mode, GUARD)
    what = "ln windowed %d shifted %d mode %d" % (windowed, shifted, mode)
    y = R.ln_truth(M, gamma, beta)[0]
    tol = R.ln_tolerance(M, gamma, beta)
    rest = np.setdiff1d(np.arange(xrows + GUARD), gr)
    same_bytes(what + ": X rows the launch does not address", Xa[rest][:len(rest) - GUARD], X[rest[:len(rest) - GUARD]])
    preset(what + ": X guard rows", Xa[xrows:])
    preset(what + ": output rows the launch does not address", raw[rest])
    out = halfs(raw)
    if mode == 0:
        ref = X[gr].astype(np.float64) + y
        check(what + " X vs float64", Xa[gr], ref, tol + R.U24 * np.abs(ref))
        same_bytes(what + ": split copy of its own X", out[gr], R.split_rows(Xa[gr]))
    else:
        same_bytes(what + ": X must stay", Xa[:xrows], X)
        xh, xl = R.split16(X[gr])
        same_bytes(what + ": hi X", out[gr][:, :128], xh)
        same_bytes(what + ": lo X", out[gr][:, 256:384], xl)
        yh, yl = out[gr][:, 128:256], out[gr][:, 384:]
        got = yh.astype(np.float64) + yl.astype(np.float64)
        check(what + " y (hi + lo) vs float64", got, y, tol + lo_half_step(y))
        bad = np.abs(yl.astype(np.float64)) > 0.5 * R.f16_step(yh)
        assert not bad.any(), "%s: y is no split pair at %s: lo %r is more than half a step of hi %r" % (
            what, tuple(np.argwhere(bad)[0]), yl[tuple(np.argwhere(bad)[0])], yh[tuple(np.argwhere(bad)[0])])


# ---------------------------------------------------------------------------------------------------------------------
# attention128.hip as the engine configures it
# ---------------------------------------------------------------------------------------------------------------------
def run_cfg(ops, what, q, k, v, **kw):
    """two launches that differ only in what the V^T pad columns and the unread lo rows hold; they must agree bit for bit"""
    a = ops.attention128_cfg(q, k, v, fill=0.0, **kw)
    b = ops.attention128_cfg(q, k, v, fill=60000.0, **kw)
    same_bytes(what + ": result with 60000 in the V^T pad columns / unread lo rows vs with 0", b, a)
    return a


@pytest.mark.parametrize("grid", [(6, 10), (18, 26), (28, 38)], ids=gid)
@pytest.mark.parametrize("kxor", [0, 4])
def test_attention_window_config(ops, grid, kxor):
    """the window attention's instantiation <SPLIT, !SPV, 4>: split q / k, P and V single fp16 (pv_single), V^T batch stride 2 x 128 x ldv
    with the lo rows never read, the production region table (nreg 4), kxor 4 = the partner image's windows.  L = Lw of the grid: 15, 117,
    266 (three query blocks, key tail 10).  vs float64 torch on unrounded operands: BUDGET[F16] sum p |v| + 2 ds sum p |v - o|, ds = 2^-21 of
    sum |q||k| / sqrt(128).
    measured: <= 0.669 (what is used is P and V as single fp16 against BUDGET[F16]); fill 60000 vs 0 bit-identical."""
    h8, w8 = grid
    L, B = (h8 // 2) * (w8 // 2), 8
    q, k, v = R.attention_data(L + kxor, B, L, 128)
    reg = engine.gm_tables(h8, w8)[1]
    what = "attention window %s kxor %d" % (gid(grid), kxor)
    got = run_cfg(ops, what, q, k, v, region=reg, split=1, pv_single=1, kxor=kxor)
    idx = np.arange(B) ^ kxor
    t = R.attention_truth(q, k[idx], v[idx], R.region_mask(reg)[np.arange(B) % 4])
    check(what + " vs float64", got, t["o"], R.attention_tolerance(t, True, False))


@pytest.mark.parametrize("grid", [(4, 6), (18, 26), (28, 38)], ids=gid)
@pytest.mark.parametrize("strided", [1, 2])
def test_attention_matching_config(ops, grid, strided):
    """the matching's instantiation <SPLIT, SPV, 1>: 32-column V^T shared by the batch (v_shared), Q and K in ONE buffer - both directions
    (batch stride one image, kxor 1) and one direction (stride two images, K = Q + one image).  L = P of the grid: 24, 468, 1064.
    vs float64: BUDGET[SPLIT16] sum p |v| + the score term.
    measured: <= 0.111 (before the probabilities were carried 2^14 higher in attention128.hip: <= 0.280); fill bit-identical."""
    h8, w8 = grid
    L, B = h8 * w8, 2
    q, k, v = R.attention_data(L + strided, B, L, 32)
    v = v[:1]
    what = "attention matching %s strided %d" % (gid(grid), strided)
    if strided == 1:
        got = run_cfg(ops, what, q, None, v, split=1, v_shared=True, kxor=1, strided=1)
        k = q[np.arange(B) ^ 1]
    else:
        got = run_cfg(ops, what, q, k, v, split=1, v_shared=True, strided=2)
    t = R.attention_truth(q, k, np.broadcast_to(v, (B,) + v.shape[1:]))
    check(what + " vs float64", got, t["o"], R.attention_tolerance(t, True, True))


@pytest.mark.parametrize("L,vcols", [(117, 128), (266, 128), (468, 32)])
def test_attention_fast_mode_on_split_rows(ops, L, vcols):
    """precision 0: the non-split kernel reads the hi half of split rows (ldq = 256) and the hi rows of a [2, vcols, ldv] V^T.
    vs float64: BUDGET[F16] sum p |v| + the score term with ds = 2^-10 of sum |q||k| / sqrt(128).
    measured: <= 0.163; fill bit-identical."""
    q, k, v = R.attention_data(L, 4, L, vcols)
    what = "attention fast mode L %d vcols %d" % (L, vcols)
    got = run_cfg(ops, what, q, k, v, split=0, ldq=256)
    t = R.attention_truth(q, k, v)
    check(what + " vs float64", got, t["o"], R.attention_tolerance(t, False, False))


@pytest.mark.parametrize("split,pv_single,vcols", [(1, 1, 128), (1, 0, 32), (0, 0, 128)])
def test_attention_spiked(ops, split, pv_single, vcols):
    """every query's logit for one key is ~60 above the rest (exp(-60) of the mass elsewhere): the row is that key's V.  |v| >= 4: a row
    that is ONE key's V has no average to hide in, and below |v| = 2^-3 the lo half of a split pair is an fp16 subnormal (absolute step
    2^-24), so the pair is no longer good to 2^-22 of v - with V ~ 40 N(0, 1) as it came, an element 0.00107 was off by 1.96e-8, 19
    tolerances, which is that floor and not the kernel.
    measured: the row equals V to <= 0.497 of the tolerance (single fp16 V), 0.125 (split V)."""
    L = 117
    q, k, v = R.attention_data(5, 2, L, vcols)
    v = v + np.copysign(np.float32(4.0), v)
    q, j = R.spiked(q, k)
    t = R.attention_truth(q, k, v)
    assert t["gap"].min() >= 50 and np.abs(t["o"] - v[:, j]).max() < 1e-15
    got = run_cfg(ops, "attention spiked", q, k, v, split=split, pv_single=pv_single, ldq=256)
    check("attention spiked split %d pv_single %d vcols %d vs the key's V" % (split, pv_single, vcols), got, v[:, j],
          R.attention_tolerance(t, bool(split), bool(split and not pv_single)))


# ---------------------------------------------------------------------------------------------------------------------
# the engine's launch chains with the GEMMs left out
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(6, 10), (18, 26), (28, 38)], ids=gid)
@pytest.mark.parametrize("shifted,cross", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_window_block_chain(ops, grid, shifted, cross):
    """pack (q, k, v) -> window attention (pv_single, production regions when shifted, kxor 4 when cross) -> gm_ln (windowed, mode 0) on
    4 images (Bw = 16), against the reference's single_head_split_window_attention on float64 tensors + float64 LayerNorm + X.  The tolerance
    is the attention's pushed through the LayerNorm's derivative, plus gm_ln's own (gm_ref.window_block_tolerance).
    measured: <= 0.210."""
    h8, w8 = grid
    images = 4
    Y, X, gamma, beta = R.window_data(100 + h8, images, h8, w8)
    got = ops.gm_window_block(Y, X, gamma, beta, h8, w8, bool(shifted), bool(cross))
    t = R.window_restated(Y, h8, w8, images, shifted, cross)
    o = R.window_truth(Y, h8, w8, images, shifted, cross).reshape(-1, 128)
    assert np.abs(t["o"] - o).max() < 1e-12
    check("window_block %s shifted %d cross %d vs float64" % (gid(grid), shifted, cross), got, R.window_block_truth(o, X, gamma, beta),
          R.window_block_tolerance(t, X, gamma, beta))


@pytest.mark.parametrize("grid", [(4, 6), (18, 26), (28, 38)], ids=gid)
@pytest.mark.parametrize("dirs", [1, 2])
def test_match_chain(ops, grid, dirs):
    """split_rows -> the global matching over the shared coordinate V^T (both stride modes of the one Xs buffer) -> match_flow, 2 pairs,
    against the reference's global_correlation_softmax on float64 maps.  The flows are about a pixel, the coordinates they are the
    difference of up to 37: the error is judged against 2^-20 of the largest COORDINATE plus the score term - 2e-5 of the flow's range.
    This test failed on 28 x 38 before attention128.hip was changed: token 33 of pair 0, kernel -1.28623772, float64 -1.28616844, 1.67
    tolerances, 4 elements outside (dirs 1; 9 with dirs 2); 18 x 26 stood at 0.818.  Two causes, both in the <SPLIT, SPV, 1> kernel: a
    probability below 2^-3 of the row's largest had an fp16-subnormal lo half (2^-25 absolute, every key but the matched one), and the six
    P V MFMAs of a tile were chained through the running accumulator, rounding at the coordinate's magnitude each time.  With the
    probabilities carried 2^14 higher and a per-tile accumulator joined by one fma:
    measured: <= 0.660 (28 x 38), 0.532 (18 x 26), 0.327 (4 x 6)."""
    h8, w8 = grid
    tok = R.match_tokens(300 + h8, 2, h8, w8)
    got = ops.gm_match(tok, h8, w8, dirs)
    flow, t = R.match_restated(tok, h8, w8, dirs)
    truth = R.match_truth_oracle(tok, h8, w8, dirs)
    assert np.abs(flow - truth).max() < 1e-10 and np.abs(truth).max() >= 1.0
    check("match %s dirs %d vs float64" % (gid(grid), dirs), got, truth, R.match_tolerance(t, h8, w8))


@pytest.mark.parametrize("grid", [(4, 6), (28, 38)], ids=gid)
@pytest.mark.parametrize("dirs", [1, 2])
def test_propagate_chain(ops, grid, dirs):
    """match_flow (the V^T of a given flow; the buffer zeroed first as the engine's arena is) -> the propagation attention (separate q / k
    buffers, batch stride one or two images) -> upsampler_in, 2 pairs.  The matched flow and the upsampler map byte for byte; the propagated
    flow against softmax(q k^T / sqrt(128)) flow in float64: BUDGET[SPLIT16] sum p |v| + the score term.
    Failed before the same change (the subnormal lo halves of P): 4 x 6 1.036, 28 x 38 dirs 2 1.149 tolerances (kernel -0.238276094,
    float64 -0.238273067).
    measured: <= 0.375; bytes equal."""
    h8, w8 = grid
    P, NP = h8 * w8, 2
    q, k, X, flow = R.propagate_data(400 + h8, NP, h8, w8)
    flow = flow[:NP * dirs]
    fm, fp, mp = ops.gm_propagate(q, k, flow, X, h8, w8, dirs, guard_rows=GUARD)
    what = "propagate %s dirs %d" % (gid(grid), dirs)
    O = np.zeros((NP * dirs, P, 32), np.float32)
    O[..., :2] = flow + R.coords(h8, w8).astype(np.float32)[None]
    same_bytes(what + ": matched flow", fm, R.match_flow_restated(O, w8))
    t = R.propagate_truth(q, k, fm, dirs)
    check(what + " vs float64", fp, t["o"], R.attention_tolerance(t, True, True))
    same_bytes(what + ": upsampler map", halfs(mp[:NP * dirs * P]), R.upsampler_map_restated(fp, X, 1 if dirs == 2 else 2))
    preset(what + ": map guard rows", mp[NP * dirs * P:])
