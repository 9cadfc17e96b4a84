"""CPU: tests/mask_ref.py itself - every restatement agrees with float64 truth inside the budget the GPU tests use, every planted fault moves
some element by at least 4 tolerances (or flips a byte where the GPU check is exact), and the shipped inputs meet the conditions the GPU
checks rely on (threshold margins, non-degenerate masks).  Same role as tests/test_raft_ref_cpu.py for the flow_raft band.
"""
import numpy as np
import pytest
import torch

import mask_ref as R
from oracle import solov2_oracle as S
from split_ref import BUDGET, F16, SPLIT16


def worst(got, ref, tol):
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.broadcast_to(tol, np.shape(ref))).max())


def test_representable_inputs():
    x = R.rng(1).standard_normal(4096) * 37
    for split in (0, 1):
        v = R.rep(x, split)
        hi, lo = R.split16(v)
        back = hi.astype(np.float64) + (lo.astype(np.float64) if split else 0)
        assert np.array_equal(back, v.astype(np.float64))
    rows = R.rows16(R.rep(x, 1)[None], 1)
    assert not np.array_equal(rows.view(np.uint16), R.rows16(R.rep(x, 1)[None], 1, bug="swap").view(np.uint16))


@pytest.mark.parametrize("case", R.PREP_CASES, ids=lambda c: c[0])
def test_prep(case):
    name, H, W, nh, nw, Hp, Wp = case
    frames = R.prep_frames(10 + H, 2, H, W)
    chw, s2d = R.prep_restated(frames, nh, nw, Hp, Wp)
    y, x, c = 5, 6, 2
    assert s2d[1, y >> 2, x >> 2, ((y & 3) * 4 + (x & 3)) * 4 + c] == chw[1, c, y, x]
    assert nw % 4 != 0 or name != "up"
    _, bad = R.prep_restated(frames, nh, nw, Hp, Wp, bug="s2d_xy")
    assert not np.array_equal(R.rows16(s2d.reshape(-1, 64), 1).view(np.uint16), R.rows16(bad.reshape(-1, 64), 1).view(np.uint16))
    xt, yt = R.prep_tables(H, W, nh, nw)
    assert xt[:, :2].max() < W and yt[:, :2].max() < H and xt.min() >= 0 and yt.min() >= 0


def test_maxpool_and_max0():
    for H, W in R.POOL_SIZES:
        x = R.map_data(21 + H, (2, H, W, 64), 1, negative=True)
        good, bad = R.maxpool_restated(x), R.maxpool_restated(x, "max0")
        assert (good < 0).all() and not np.array_equal(good, bad)          # exact check: any differing byte is seen


@pytest.mark.parametrize("case", R.NEAREST_CASES, ids=lambda c: "%dx%d" % c[0])
def test_nearest(case):
    (h, w), (sh, sw) = case
    for split in (0, 1):
        dst, src = R.map_data(40 + h, (2, h, w, 64), split), R.map_data(41 + h, (2, sh, sw, 64), split)
        ref = R.nearest_add_restated(dst, src)
        assert np.array_equal(ref, R.nearest_add_truth(dst, src))
        assert worst(R.nearest_add_restated(dst, src, "row_off"), ref, R.store_tol(ref, split)) >= 4


@pytest.mark.parametrize("size", R.COORD_SIZES, ids=lambda s: "%dx%d" % s)
def test_coord(size):
    h, w = size
    x = R.map_data(50 + h, (2, h, w, 16), 1)
    out = R.coord_restated(x)
    assert np.array_equal(out[0, :, :, 16], np.broadcast_to(torch.linspace(-1, 1, w).numpy(), (h, w)))
    assert np.array_equal(out[0, :, :, 17], np.broadcast_to(torch.linspace(-1, 1, h).numpy()[:, None], (h, w)))
    if h != w:
        assert not np.array_equal(out, R.coord_restated(x, "xy"))
    assert not out[..., 18:].any()


@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_bilinear(case):
    (H, W), (OH, OW) = case
    for split in (0, 1):
        x = R.map_data(60 + H + OW, (2, H, W, 16), split)
        y0 = R.map_data(61 + H + OW, (2, OH, OW, 16), split)
        for acc in (None, y0):
            ref, mag = R.bilinear_restated(x, OH, OW, acc)
            tol = BUDGET[R.layout_of(split)] * mag + 2.0 ** -25
            assert worst(ref, R.bilinear_truth(x, OH, OW, acc), tol + R.bilinear_coord_tolerance(x, OH, OW)) <= 1
            if split and H > 1:
                # a missing -0.5 shows where the sizes differ, a missing clamp where the last rows blend past the end (upscaling)
                for bug in ["row_off"] + (["no_half"] if OH != H else []) + (["no_clamp"] if OH > H else []):
                    w = worst(R.bilinear_restated(x, OH, OW, acc, bug=bug)[0], ref, tol)
                    assert w >= 4, (bug, w)


@pytest.mark.parametrize("shape", R.GN_SHAPES[:5], ids=lambda s: "C%d_HW%d" % s)
def test_group_norm(shape):
    """the centred statistics stay inside the split budget at every mean / std; the uncentred ones miss it by more than 4 tolerances at 10"""
    C, HW = shape
    for ratio in R.GN_RATIOS:
        x, gamma, beta = R.gn_data(70 + C + HW + ratio, C, HW, ratio, 1)
        ref, aff_ref = R.gn_truth(x, gamma, beta)
        tol = BUDGET[SPLIT16] * np.abs(ref).max((1, 2), keepdims=True) + 2.0 ** -25
        y, aff = R.gn_restated(x, gamma, beta)
        assert worst(y, ref, tol) <= 1, (ratio, worst(y, ref, tol))
        if ratio == 10 and HW > 1:
            w = worst(R.gn_restated(x, gamma, beta, "uncentred")[0], ref, tol)
            assert w >= 4, w


def test_group_norm_single_pixel():
    x, gamma, beta = R.gn_data(1, 32, 1, 10, 1)
    ref, _ = R.gn_truth(x, gamma, beta)
    assert np.allclose(ref, np.maximum(beta, 0)[None, None], atol=1e-6)


@pytest.mark.parametrize("g", R.NMS_GRIDS)
def test_cls_points_nms(g):
    x = R.cls_logits(80 + g, 2, g)
    kept, sig = R.cls_truth(x)
    s = R.cls_restated(x)
    assert np.array_equal(s != 0, kept)
    assert np.abs(s[kept] - sig[kept]).max() <= 2.0 ** -21
    if g >= 4:
        assert kept[:, 0 * g + 1:0 * g + 4, 5].all() and kept[:, (g - 1) * g:(g - 1) * g + 2, 7].all()          # plateau's first row, the saturated pair
        assert s[0, (g - 1) * g, 7] == 1 and s[0, (g - 1) * g + 1, 7] == 1
        assert not np.array_equal(R.cls_restated(x, "window") != 0, kept)
    d = np.diff(np.unique(R.sigmoid(np.arange(-48, 33) / 8.0)))
    assert d.min() > 1000 * 2.0 ** -24


def test_mask_inputs():
    """threshold ops: no sigmoid within 2^-20 of thr, masks neither empty nor full"""
    for HW in (64, 2368, 4096):
        x = R.mask_logits(100 + HW, 5, HW // 16 if HW > 64 else 4, 16)
        s = R.sigmoid(x)
        assert np.abs(s - R.THR).min() > 2.0 ** -20
        assert np.abs(R.sigmoid(x.astype(np.float32)).astype(np.float32).astype(np.float64) - R.THR).min() > 2.0 ** -20
        on = (s > R.THR).reshape(5, -1).mean(1)
        assert (on > 0.02).all() and (on < 0.98).all(), on
    for n, words in [(1, 1), (16, 37), (17, 64), (33, 65), (33, 1), (1, 65)]:
        x = R.mask_logits(110 + n + words, n + 3, words, 64, amp=4.0)
        assert np.abs(R.sigmoid(x) - R.THR).min() > 2.0 ** -20
        idx = (np.arange(n) * 5 + 2) % (n + 3)
        assert n == 1 or not np.array_equal(idx, np.arange(n))
        bits, on = R.bits_truth(x.reshape(n + 3, -1), idx, 64 * words)
        assert bits.shape == (n, words) and 0.05 < on.mean() < 0.95
        assert int(bits[0, 0]) & 1 == int(on[0, 0])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_matrix_nms(n):
    inter, area, label, score = R.nms_data(120 + n, n)
    assert (inter <= np.minimum(area[:, None], area[None, :])).all()
    up = np.triu(inter)
    comp, out = R.nms_restated(up, area, label, score)
    cfg = type("C", (), dict(nms_pre=10 ** 6, sigma=2.0, filter_thr=0.0, max_per_img=10 ** 6))
    if n > 1:           # the oracle's matrix_nms on the masks themselves, float32
        masks = R.nms_masks(120 + n, n)[0]
        s, lab, keep = S.matrix_nms(torch.from_numpy(masks), torch.from_numpy(label.astype(np.int64)), torch.from_numpy(score),
                                    torch.from_numpy(area), cfg)
        mine = np.sort(out)[::-1]
        assert np.allclose(s.numpy(), mine, rtol=2e-5, atol=1e-7)
        tol = 2.0 ** -20 * out
        assert worst(R.nms_restated(up, area, label, score, bug="lower")[1], out, tol) >= 4
        assert worst(R.nms_restated(up, area, label, score, bug="comp_j")[1], out, tol) >= 4
    else:
        assert comp[0] == 0 and out[0] == np.float64(score[0])


@pytest.mark.parametrize("case", R.ACC_CASES, ids=lambda c: "%dx%d_%dx%d_%dx%d_k%d" % c)
def test_band_accumulate(case):
    """the conditions the GPU check relies on, for the inputs actually shipped: no pixel within 4e-7 of the threshold, at most 1e-4 of the
    pixels within 1e-5 (the excusable share is bounded by that), no float32-coordinate / float64-coordinate decision flip"""
    fh, fw, h, w, H, W, k = case
    sig, use = R.acc_data(150 + H + k, fh, fw, k)
    soft = R.acc_restated(sig, h, w, H, W)
    truth = R.acc_truth(sig, h, w, H, W)
    margin = np.abs(soft - R.THR)
    assert margin.min() > 4e-7, margin.min()
    assert (margin < 1e-5).mean() <= 1e-4 and (margin < R.ACC_MARGIN).mean() <= 1e-4
    assert np.array_equal(soft > R.THR, truth > R.THR)
    assert np.abs(soft - truth).max() < 1e-5
    on = soft > R.THR
    share = on.reshape(k, -1).mean(1)
    assert (share > 0.02).all() and (share < 0.98).all(), share
    assert use.min() == 0 and use.max() == 1
    img = R.acc_image(on, use)
    if use[0] and use[1]:
        assert (img == 254).any()
    # (rows of the second resize: a missing -0.5 shows where the sizes differ, a missing clamp where it upscales)
    for bug in ["row_off"] + (["no_half"] if H != h else []) + (["no_clamp"] if H > h else []):
        bad = R.acc_restated(sig, h, w, H, W, bug=bug) > R.THR
        flips = bad != on
        assert (flips & (margin >= R.ACC_MARGIN)).sum() > 1e-4 * on.size, bug


def test_stats_and_dynconv_budgets():
    x = R.mask_logits(100 + 2368, 5, 148, 16).reshape(5, -1)
    area, soft = R.stats_truth(x, 2368)
    s32 = R.sigmoid(x).astype(np.float32)
    assert np.abs((s32 * (s32 > 0.5)).sum(1, dtype=np.float32) - soft).max() <= (2.0 ** -20 * soft).min()
    for split in (0, 1):
        kern, feat = R.dynconv_data(140, 16, 384, split)
        k64, f64 = kern.astype(np.float64), feat.astype(np.float64)
        hi_k, hi_f = R.split16(kern)[0].astype(np.float64), R.split16(feat)[0].astype(np.float64)
        tol = BUDGET[R.layout_of(split)] * (np.abs(k64) @ np.abs(f64).T)
        if split:           # dropping the residual parts (a swapped / missing lo) is seen
            assert worst(hi_k @ hi_f.T, k64 @ f64.T, tol) >= 4
    assert BUDGET[F16] == 2.0 ** -10 and BUDGET[SPLIT16] == 2.0 ** -20
