"""GPU: the mask_mmdet band's own kernels one by one (pb_op_mask_*: the launchers of mask_kernels.h with MaskEngine's arguments) against
tests/mask_ref.py - bytes where a kernel only moves or selects representable values, a restatement that rounds where the kernel rounds
otherwise, and float64 truth inside the layout's budget.  Everywhere the bytes a kernel does not own (row tails, guard rows) must still be
0xFF.  A failure names the op, the case and the element.  tests/test_mask_ref_cpu.py holds the CPU side: the tolerances see the planted
faults and the inputs meet the conditions the checks rely on.

measured (MI355X; worst error / tolerance per op): see the "measured:" line of every test.
"""
import numpy as np
import pytest

import mask_ref as R
from mask_ref import check, preset, same_bytes
from prisma_amd import engine
from split_ref import BUDGET

pytestmark = pytest.mark.gpu
GUARD = 8
SPLITS = [0, 1]


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


def halfs(raw, rows):
    """raw uint8 [rows + GUARD, bytes] -> float16 [rows, ld]; the guard rows must still be preset"""
    preset("guard rows", raw[rows:])
    return raw[:rows].view(np.float16)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", R.PREP_CASES, ids=lambda c: c[0])
def test_mask_prep(ops, case, split):
    """chw bit-exact with the oracle's fixed-point resize + normalise; the 4 x 4 space-to-depth map - what the network reads - equal to f16(v)
    (and f16(v - hi)) at channel ((y & 3) 4 + (x & 3)) 4 + c, channel 3 and the pad region zero.
    measured: bytes equal in all six cases."""
    name, H, W, nh, nw, Hp, Wp = case
    n = 2
    frames = R.prep_frames(10 + H, n, H, W)
    xt, yt = R.prep_tables(H, W, nh, nw)
    raw, chw = ops.mask_prep(frames, nh, nw, Hp, Wp, xt, yt, bool(split), GUARD)
    want_chw, s2d = R.prep_restated(frames, nh, nw, Hp, Wp)
    px = n * 3 * Hp * Wp
    preset(name + " chw guard", chw[px:])
    same_bytes(name + " chw", chw[:px].reshape(n, 3, Hp, Wp), want_chw)
    blocks = n * (Hp // 4) * (Wp // 4)
    same_bytes(name + " space-to-depth", halfs(raw, blocks), R.rows16(s2d.reshape(blocks, 64), split))
    v = s2d.reshape(n, Hp // 4, Wp // 4, 16, 4)
    assert not v[..., 3].any() and not want_chw[:, :, nh:].any() and not want_chw[:, :, :, nw:].any()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("size", R.POOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_maxpool3x3s2(ops, size, split):
    """max_pool2d(3, 2, 1) selects one input: bytes.  The all-negative map catches a maximum that starts at 0.
    measured: bytes equal."""
    H, W = size
    for neg in (False, True):
        x = R.map_data(20 + H + neg, (2, H, W, 64), split, negative=neg)
        raw = ops.mask_maxpool(x, bool(split), GUARD)
        y = R.maxpool_restated(x).astype(np.float32)
        rows = y.shape[0] * y.shape[1] * y.shape[2]
        same_bytes("maxpool %dx%d neg %d" % (H, W, neg), halfs(raw, rows), R.rows16(y.reshape(rows, 64), split))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("size", R.POOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_subsample2(ops, size, split):
    """max_pool2d(1, stride 2) = x[::2, ::2] on whole rows of L(64) halfs: bytes.
    measured: bytes equal."""
    H, W = size
    x = R.map_data(30 + H, (2, H, W, 64), split)
    raw = ops.mask_subsample2(x, bool(split), GUARD)
    y = x[:, ::2, ::2]
    rows = y.shape[0] * y.shape[1] * y.shape[2]
    same_bytes("subsample2 %dx%d" % size, halfs(raw, rows), R.rows16(y.reshape(rows, 64), split))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", R.NEAREST_CASES, ids=lambda c: "%dx%d" % c[0])
def test_nearest_add(ops, case, split):
    """dst += src at torch's 'nearest' source pixel, within one output rounding of the restatement (which equals float64 truth).
    measured: err / tol <= 0.500 (fp16: a rounding tie), <= 0.154 (split)."""
    (h, w), (sh, sw) = case
    dst = R.map_data(40 + h, (2, h, w, 64), split)
    src = R.map_data(41 + h, (2, sh, sw, 64), split)
    raw = ops.mask_nearest_add(dst, src, bool(split), GUARD)
    ref = R.nearest_add_restated(dst, src)
    assert np.array_equal(ref, R.nearest_add_truth(dst, src))
    rows = 2 * h * w
    got = R.decode("nearest_add", raw, rows, 64, split)
    check("nearest_add %dx%d <- %dx%d split %d" % (h, w, sh, sw, split), got, ref.reshape(rows, 64), R.store_tol(ref.reshape(rows, 64), split))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("size", R.COORD_SIZES, ids=lambda s: "%dx%d" % s)
def test_coord_concat(ops, size, split):
    """copied channels exact, channels C / C + 1 = torch.linspace(-1, 1, steps) in float32 rounded the same way, C + 2 .. C + 63 zero;
    1 x 5 and 5 x 1 take the steps <= 1 branch.  Input rows are wider than the map (ldi > L(C)).
    measured: bytes equal."""
    h, w = size
    C = 16
    x = R.map_data(50 + h, (2, h, w, C), split)
    raw = ops.mask_coord_concat(x, (C + 8) * (1 + split), bool(split), GUARD)
    want = R.coord_restated(x)
    rows = 2 * h * w
    same_bytes("coord_concat %dx%d" % size, halfs(raw, rows), R.rows16(want.reshape(rows, C + 64), split))
    assert not want[..., C + 2:].any()


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_bilinear(ops, case, split, acc):
    """against the restatement (float32 indices and weights as torch computes them, float64 values) at the output layout's budget times the
    largest tap magnitude, and against F.interpolate on float64 with that plus the coordinate round trip (mask_ref.bilinear_coord_tolerance).
    Rows are wider than the map on both sides.
    measured: vs restatement <= 0.978 (fp16: with accumulate |out| reaches twice the largest tap, half an fp16 step of that is the whole
    tolerance), <= 0.592 (split); vs float64 truth <= 0.970 / <= 0.178."""
    (H, W), (OH, OW) = case
    C, n = 16, 2
    ldi, ldo = (C + 8) * (1 + split), (C + 16) * (1 + split)
    x = R.map_data(60 + H + OW, (n, H, W, C), split)
    y0 = R.map_data(61 + H + OW, (n, OH, OW, C), split) if acc else None
    raw = ops.mask_bilinear(x, OH, OW, ldi, ldo, bool(split), y0, GUARD)
    rows = n * OH * OW
    got = R.decode("bilinear", raw, rows, C, split, ldo, C if split else 0).reshape(n, OH, OW, C)
    ref, mag = R.bilinear_restated(x, OH, OW, y0)
    tol = BUDGET[R.layout_of(split)] * mag + 2.0 ** -25
    name = "bilinear %dx%d -> %dx%d split %d acc %d" % (H, W, OH, OW, split, acc)
    check(name + " vs restatement", got, ref, tol)
    check(name + " vs float64", got, R.bilinear_truth(x, OH, OW, y0), tol + R.bilinear_coord_tolerance(x, OH, OW))


@pytest.mark.parametrize("ratio", R.GN_RATIOS)
@pytest.mark.parametrize("shape", R.GN_SHAPES, ids=lambda s: "C%d_HW%d" % s)
def test_gn_relu(ops, shape, ratio):
    """GroupNorm(32) + ReLU of three samples with their own offset and scale against float64, within BUDGET[layout] x max |ref| of the
    sample, in the three layouts the engine uses (fp16 -> fp16, split -> split, split -> [hi | hi | lo]); group mean / std 0, 3, 10.  The
    shapes cover cpg 1 / 4 / 16, 64 / 16 / 4 pixel lanes per channel group and fewer and more than 64 (chunk, channel) items per wave.
    Sample 1 run alone must give the same bytes.
    With the variance taken as E[x^2] - mean^2 from plain float32 sums the split layouts fail at mean / std 10 and 3 (EXPERIMENTS.md has the
    figures); with per-chunk centred sums they pass.
    measured: err / tol at mean / std 0, 3, 10: fp16 <= 0.391, 0.435, 0.414; split and dup <= 0.266, 0.256, 0.372.  The previous kernels, same
    cases, split: 53 (C 32, HW 1) and <= 0.24 elsewhere at 0; 369 and 0.93 .. 3.07 at 3; 426 and 9.8 .. 21.6 at 10."""
    C, HW = shape
    n = 3
    for layout in (0, 1, 2):
        split = layout > 0
        x, gamma, beta = R.gn_data(70 + C + HW + ratio, C, HW, ratio, split)
        raw, aff = ops.mask_gn_relu(x, gamma, beta, layout, GUARD)
        ref, aff_ref = R.gn_truth(x, gamma, beta)
        rows = n * HW
        ldo = C * (1, 2, 3)[layout]
        got = R.decode("gn_relu", raw, rows, C, split, ldo, (0, C, 2 * C)[layout] if split else 0) if layout < 2 else None
        if layout == 2:
            h = halfs(raw, rows)
            assert np.array_equal(h[:, :C].view(np.uint16), h[:, C:2 * C].view(np.uint16)), "gn_relu dup: the two hi copies differ"
            got = h[:, :C].astype(np.float64) + h[:, 2 * C:].astype(np.float64)
        tol = BUDGET[R.layout_of(split)] * np.abs(ref).max((1, 2), keepdims=True) + 2.0 ** -25
        name = "gn_relu C %d HW %d mean/std %d layout %d" % (C, HW, ratio, layout)
        check(name, got.reshape(n, HW, C), ref, np.broadcast_to(tol, ref.shape))
        scale = np.abs(aff_ref).max((1,), keepdims=True)
        print("\n  %-58s aff worst |err| / max|aff| %.3e" % (name, float((np.abs(aff - aff_ref) / scale).max())), end="")
        raw1, aff1 = ops.mask_gn_relu(x[1:2], gamma, beta, layout, GUARD)
        assert np.array_equal(raw1[:HW], raw[HW:2 * HW]) and np.array_equal(aff1[0].view(np.uint32), aff[1].view(np.uint32)), \
            name + ": sample 1 depends on the batch"


@pytest.mark.parametrize("g", R.NMS_GRIDS)
def test_cls_points_nms(ops, g):
    """sigmoid + points NMS into this level's rows of the frames' concatenated score table (pts_total > g^2, off != 0).  The kept / zeroed
    pattern is exact (ties keep: the planted plateau, the saturated 20 | 21 pair); kept values within 2^-21 of float64 sigmoid (four float32
    roundings, doubled); rows of other levels still preset.
    measured: pattern equal; err / tol <= 0.148."""
    n, C, off = 2, 80, 5
    pts = g * g + 11
    x = R.cls_logits(80 + g, n, g, C)
    raw = ops.mask_cls_points_nms(x, pts, off, GUARD)
    tab = raw[:n * pts].reshape(n, pts, C)
    preset("cls_points_nms rows before the level", tab[:, :off])
    preset("cls_points_nms rows behind the level", tab[:, off + g * g:])
    preset("cls_points_nms guard rows", raw[n * pts:])
    got = tab[:, off:off + g * g]
    kept, sig = R.cls_truth(x)
    bad = (got != 0) != kept
    assert not bad.any(), "cls_points_nms g %d: cell %s kept %r, truth %r (%d cells differ)" % (
        g, tuple(np.argwhere(bad)[0]), bool(got[tuple(np.argwhere(bad)[0])] != 0), bool(kept[tuple(np.argwhere(bad)[0])]), int(bad.sum()))
    check("cls_points_nms g %d kept values" % g, got[kept], sig[kept], 2.0 ** -21)
    if g >= 4:
        assert kept[:, (g - 1) * g, 7].all() and kept[:, (g - 1) * g + 1, 7].all() and (got[:, (g - 1) * g:(g - 1) * g + 2, 7] == 1).all()


@pytest.mark.parametrize("split", SPLITS)
def test_gather_rows_f16(ops, split):
    """dst[k] = f16 (and residual) of src[idx[k]], repeated and unsorted indices, rows count .. rows_pad zero: bytes.
    measured: bytes equal."""
    src = (R.rng(90).standard_normal((40, 256)) * 3).astype(np.float32)
    idx = np.array([7, 3, 3, 39, 0, 12, 7, 21, 38, 1, 30], np.int32)
    rows_pad = 16
    raw = ops.mask_gather_rows(src, idx, rows_pad, bool(split), GUARD)
    want = np.zeros((rows_pad, 256), np.float32)
    want[:len(idx)] = src[idx]
    same_bytes("gather_rows_f16 split %d" % split, halfs(raw, rows_pad), R.rows16(want, split))


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("HW", [64, 2368, 4096])
def test_mask_stats(ops, HW, pad):
    """area = #(sigmoid > thr) exact, the soft sum within 2^-20 relative (at most 16 roundings), row K still preset; 2368 is no multiple of
    the 1024-element stride, ld = HW and HW + 64.
    measured: areas equal; soft sum err / tol <= 0.082."""
    K = 5
    x = np.full((K, HW + pad), 9.0, np.float32)          # the columns behind HW would all count
    x[:, :HW] = R.mask_logits(100 + HW, K, HW // 16 if HW > 64 else 4, 16).reshape(K, HW)
    raw = ops.mask_stats(x, HW, R.THR, 1)
    preset("mask_stats row K", raw[K:])
    area, soft = R.stats_truth(x, HW)
    assert np.array_equal(raw[:K, 0].astype(np.float64), area), (raw[:K, 0], area)
    assert area.min() > 0 and area.max() < HW
    check("mask_stats HW %d ld %d soft sum" % (HW, HW + pad), raw[:K, 1], soft, 2.0 ** -20 * soft)


@pytest.mark.parametrize("case", [(1, 1), (16, 37), (17, 64), (33, 65), (33, 1), (1, 65)], ids=lambda c: "n%d_w%d" % c)
def test_bitpack_and_intersections(ops, case):
    """bit rows = np.packbits(little) of the float64 decision for rows picked by a non-identity idx; |mask_i & mask_j| exact for i <= j in a
    matrix of row stride 512; nothing written outside rows and columns [0, n).
    measured: bits and counts equal."""
    n, words = case
    HW = 64 * words
    src_rows = n + 3
    x = R.mask_logits(110 + n + words, src_rows, words, 64, amp=4.0).reshape(src_rows, HW)
    idx = (np.arange(n) * 5 + 2) % src_rows
    irows = -(-n // 16) * 16 + 16
    bits, inter = ops.mask_intersections(x, idx, HW, R.THR, irows, 2)
    want, on = R.bits_truth(x, idx, HW)
    preset("bitpack guard rows", bits[n:])
    assert np.array_equal(bits[:n], want), "bitpack n %d words %d: row %d differs" % (n, words, int(np.argwhere((bits[:n] != want).any(1))[0]))
    assert 0.05 < on.mean() < 0.95
    cnt = on.astype(np.float64) @ on.astype(np.float64).T
    iu = np.triu_indices(n)
    assert np.array_equal(inter[:n, :n][iu].astype(np.float64), cnt[iu]), "mask_intersections n %d words %d" % (n, words)
    preset("mask_intersections columns >= n", inter[:, n:])
    preset("mask_intersections rows >= n", inter[n:])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_matrix_nms(ops, n):
    """compensation and decayed score within 2^-20 relative of the float64 restatement; intersections and areas come from real bit masks; the
    lower triangle of the matrix handed to the kernel is NaN (the engine never writes it).
    measured: comp err / tol <= 0.059, score err / tol <= 0.169."""
    inter, area, label, score = R.nms_data(120 + n, n)
    comp_ref, out_ref = R.nms_restated(inter, area, label, score, 2.0)
    m = np.full((n, 512), np.nan, np.float32)
    iu = np.triu_indices(n)
    m[:, :n][iu] = inter[iu]
    comp, out = ops.mask_matrix_nms(m, area, label, score, 2.0, 4)
    preset("matrix_nms comp guard", comp[n:])
    preset("matrix_nms out guard", out[n:])
    assert (label == 3).sum() == 1 and (n < 63 or (comp_ref > 0).mean() > 0.3)
    check("matrix_nms n %d comp" % n, comp[:n], comp_ref, 2.0 ** -20 * comp_ref + 2.0 ** -126)
    check("matrix_nms n %d score" % n, out[:n], out_ref, 2.0 ** -20 * out_ref)


@pytest.mark.parametrize("HW", [64, 2368])
def test_sigmoid_rows(ops, HW):
    """sigmoid of the rows idx picks (with repeats), within 2^-22 of float64; row `count` still preset.
    measured: err / tol <= 0.364."""
    x = R.mask_logits(130 + HW, 6, HW // 16 if HW > 64 else 4, 16, amp=10.0).reshape(6, HW)
    idx = np.array([4, 1, 1, 5, 0], np.int32)
    raw = ops.mask_sigmoid_rows(x, idx, HW, 1)
    preset("sigmoid_rows row count", raw[len(idx):])
    check("sigmoid_rows HW %d" % HW, raw[:len(idx)], R.sigmoid(x[idx]), 2.0 ** -22)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("HW4", [384, 2368])
@pytest.mark.parametrize("M", [1, 7, 130])
def test_dynamic_convolution(ops, M, HW4, split):
    """post_chunk's GEMM: A = gather_rows_f16's output read from row 8, B = the mask features in the layout gn_relu's dup output has, K = 768
    with kwrap 8 when split, EPI_F32, TILE_AUTO; against float64 k . f within BUDGET[layout] x sum |k||f| per element.
    measured: err / tol < 0.0005 (fp16: the products of representable inputs are exact, only the fp32 accumulation rounds), <= 0.521 (split)."""
    off = 8
    kern, feat = R.dynconv_data(140 + M + HW4, 150, HW4, split)
    idx = np.concatenate([np.arange(off), (np.arange(M) * 37 + 11) % 150]).astype(np.int32)
    raw = ops.mask_dynconv(kern, idx, off, feat, bool(split), 2)
    preset("dynamic convolution guard rows", raw[M:])
    k64, f64 = kern[idx[off:]].astype(np.float64), feat.astype(np.float64)
    check("dynamic convolution M %d HW4 %d split %d" % (M, HW4, split), raw[:M], k64 @ f64.T, BUDGET[R.layout_of(split)] * (np.abs(k64) @ np.abs(f64).T))


@pytest.mark.parametrize("case", R.ACC_CASES, ids=lambda c: "%dx%d_%dx%d_%dx%d_k%d" % c)
def test_band_accumulate(ops, case):
    """the two bilinear resizes, the threshold and the accumulation per output pixel: inst and out against the restatement; a pixel may differ
    only where the restatement's value lies within 2^-19 of thr, and at most 1e-4 of a case's pixels may be excused that way.
    measured: 0 pixels differ, 0 excused, in all four cases."""
    fh, fw, h, w, H, W, k = case
    sig, use = R.acc_data(150 + H + k, fh, fw, k)
    raw_out, raw_inst = ops.mask_band_accumulate(sig, use, h, w, H, W, R.THR, 64)
    preset("band_accumulate out guard", raw_out[3 * H * W:])
    preset("band_accumulate inst guard", raw_inst[k * H * W:])
    soft = R.acc_restated(sig, h, w, H, W)
    on = soft > R.THR
    inst = raw_inst[:k * H * W].reshape(k, H, W)
    assert np.isin(inst, (0, 1)).all()
    diff = (inst != 0) != on
    excused = diff & (np.abs(soft - R.THR) < R.ACC_MARGIN)
    print("\n  band_accumulate %s: %d pixels differ, %d excused" % (case, int(diff.sum()), int(excused.sum())), end="")
    assert not (diff & ~excused).any(), "band_accumulate %s: instance pixel %s differs, restatement value %.9g" % (
        case, tuple(np.argwhere(diff & ~excused)[0]), soft[tuple(np.argwhere(diff & ~excused)[0])])
    assert excused.sum() <= 1e-4 * k * H * W
    out = raw_out[:3 * H * W].reshape(H, W, 3)
    want = R.acc_image(inst != 0, use)
    assert np.array_equal(out, want), "band_accumulate %s: out differs from the accumulation of the kernel's own masks at %s" % (
        case, tuple(np.argwhere(out != want)[0]))
    want_r = R.acc_image(on, use)
    assert not ((out != want_r).any(-1) & ~excused.any(0)).any()
    if use[0] and use[1]:
        assert (want_r == 254).any(), "no pixel with two overlapping kept instances"
