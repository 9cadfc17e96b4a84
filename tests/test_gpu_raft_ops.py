"""GPU: the flow_raft band's own kernels one by one (pb_op_raft_*: the engine's launchers with the engine's arguments) against
tests/raft_ref.py - (1) element-wise against a restatement that rounds where the kernel rounds, inside a tolerance derived from the
arithmetic, (2) against float64 truth inside the op's budget, (3) bytes: e4m3 copies exact, everything the kernel does not own still preset.
A failure names the op, the case and the element.  tests/test_raft_ref_cpu.py holds the CPU side: the tolerances see the planted bugs, and
the lookup's index arithmetic is in bounds for every flow used here (it runs first; the far flows depend on it).

measured (MI355X; worst error / tolerance per op): see the "measured:" line of every test.  Figures near 1 against a restatement are fp16
stores: the tolerance of an fp16 result is half its step, and among 10^5 .. 10^7 outputs some land within a percent of a rounding tie.
"""
import numpy as np
import pytest

import raft_ref as R
from gm_ref import check, preset          # the assert helpers the op-level GPU tests share
from prisma_amd import engine
from split_ref import BUDGET, F16, MX2, SPLIT16, e4m3_bytes, e4m3_decode, e4m3_step

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


# ---------------------------------------------------------------------------------------------------------------------
# lookup chain: avgpool2_nhwc x3, corr_tile x4, corr_volume x4 per pair, corr_lookup
# ---------------------------------------------------------------------------------------------------------------------
def lookup_rows(raw, rows, o8):
    """raw [rows + GUARD, ldo * 2] bytes -> the 324 values of every row; asserts the bytes: halfs 324..383 and the guard rows still preset, the
    e4m3 copy (byte 768, scale 2^0) equal to e4m3(fp16 value), the bytes behind the copy preset"""
    h = raw.view(np.float16)
    preset("lookup halfs 324..383", raw[:rows, 648:768])
    preset("lookup guard rows", raw[rows:])
    if o8:
        want = e4m3_bytes(h[:rows, :324].astype(np.float32))
        bad = raw[:rows, 768:768 + 324] != want
        assert not bad.any(), "lookup e4m3 copy: element %s is 0x%02x, e4m3 of the fp16 value is 0x%02x" % (
            tuple(np.argwhere(bad)[0]), raw[:rows, 768:768 + 324][tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])
        preset("lookup bytes behind the e4m3 copy", raw[:rows, 768 + 324:])
    return h[:rows, :324].astype(np.float64)


@pytest.mark.parametrize("grid", R.LOOKUP_GRIDS, ids=lambda g: g[0])
def test_lookup_chain(ops, grid):
    """pyramid vs restatement and truth, the lookup on the kernel's OWN levels vs its restatement (tight: half an fp16 step + the coordinate
    round trip + 4 blend roundings, raft_ref.lookup_restated), the chain vs float64 truth (2^-10 of the blended sum |f1||f2| / 16).
    129x17x2 is the grid on which a row bound derived from the 256-rounded stride (3328 / 24 = 138 > 136 padded rows) admits two rows that
    do not exist.  With that bound (launch_corr_lookup's `hp8 = ld / wp`) this case failed: `eighths` on own levels, row 4376 channel 53:
    kernel 2.586, float64 0, 6935 tolerances, 195 elements outside (the detector case: 941 instead of 0).  With the padded height handed to
    the kernel it passes.
    measured: own levels vs restatement <= 0.985, chain vs truth <= 0.16, pyramid vs restatement <= 0.96 (a volume entry one fp16 step off:
    its fp32 accumulation order is not restated), pyramid vs truth <= 0.14.  Level-0 truth exactly zero / windows inside / outside:
    sub-pixel 16x16 0.27 / 0.29 / 0.00, 17x23 0.22 / 0.38 / 0.00, 46x62 0.12 / 0.72 / 0.02, 129x17 0.14 / 0.55 / 0.00; border family
    0.42 .. 0.59 zero, 0.18 .. 0.26 fully outside.  Levels 2, 3 of the small grids are 0.66 .. 0.89 zero (a 2 x 2 level under a 9 x 9 window)."""
    name, n, h8, w8, sub, brd = grid
    P, rows = h8 * w8, n * h8 * w8
    geo = engine.raft_geometry(h8, w8)
    assert geo == R.geometry(h8, w8)
    f1, f2 = R.lookup_features(1000 + P, n, h8, w8)
    flows = R.lookup_flows(2000 + P, n, h8, w8, sub, brd)
    if name.startswith("129x17"):
        flows["down"] = R.downward_flows(2100, n, h8, w8)
        st = R.lookup_index_check(flows["down"], P, w8, geo, rows)
        assert st["beyond_hp"] >= 100, st           # window rows hp <= y < ld / wp with tx >= 1: what the stride-derived bound let through
    lt, mt = R.pyramid_truth(f1, f2)
    lr, mr = R.pyramid_restated(f1, f2)
    levels = None
    for k, (fam, fl) in enumerate(flows.items()):
        R.lookup_index_check(fl, P, w8, geo, rows)
        o8 = k % 2 == 1
        raw, lv = ops.raft_lookup(f1, f2, fl, o8=o8, guard_rows=GUARD, want_levels=levels is None)
        got = lookup_rows(raw, rows, o8)
        if levels is None:
            levels = [np.asarray(x, np.float64) for x in lv]
            for l in range(4):
                vt = R.volume_tolerance(lr[l], mr[l])
                check("%s pyramid level %d vs restatement" % (name, l), levels[l], lr[l], vt)
                check("%s pyramid level %d vs truth" % (name, l), levels[l], lt[l], BUDGET[F16] * mt[l] + vt)
        r, tol = R.lookup_restated(levels, fl, P, w8)
        check("%s %s on own levels vs restatement" % (name, fam), got, r, tol)
        t = R.lookup_truth(lt, fl, P, w8)
        mag = R.lookup_truth(mt, fl, P, w8)
        vtw = R.lookup_truth([R.volume_tolerance(lr[l], mr[l]) for l in range(4)], fl, P, w8)
        check("%s %s chain vs truth" % (name, fam), got, t, BUDGET[F16] * mag + vtw + tol)
        sh = R.window_shares(fl, P, w8, h8, w8, rows)
        z = float((t[:, :81] == 0).mean())
        print("\n  %s %s: level-0 truth exactly zero %.2f, windows inside %.2f straddling %.2f outside %.2f; levels 1..3 zero %.2f %.2f %.2f"
              % (name, fam, z, sh["inside"], sh["straddle"], sh["outside"], *[float((t[:, 81 * l:81 * l + 81] == 0).mean()) for l in (1, 2, 3)]), end="")
        if fam == "subpixel":
            assert z <= 0.5 and sh["inside"] >= 0.25
        if fam == "border":
            assert sh["straddle"] >= 0.10 and sh["outside"] >= 0.02


@pytest.mark.parametrize("grid", [R.LOOKUP_GRIDS[1], R.LOOKUP_GRIDS[3]], ids=lambda g: g[0])
def test_lookup_layout_detector(ops, grid):
    """fmap1 rows are 16 e_c one-hots and fmap2 holds multiples of 64 in [-960, 960]: every pooled feature and every volume entry is exact
    in fp16, so the kernel's levels must EQUAL float64 truth, and a wrong tile address, level or window index is an O(100) error.
    measured: levels equal; lookup err / tol <= 0.973."""
    name, n, h8, w8, sub, brd = grid
    P, rows = h8 * w8, n * h8 * w8
    f1, f2 = R.lookup_features(3000 + P, n, h8, w8, detector=True)
    fl = R.downward_flows(2100, n, h8, w8) if name.startswith("129x17") else R.lookup_flows(2000 + P, n, h8, w8, sub, brd)["subpixel"]
    R.lookup_index_check(fl, P, w8, engine.raft_geometry(h8, w8), rows)
    lt, _ = R.pyramid_truth(f1, f2)
    raw, lv = ops.raft_lookup(f1, f2, fl, o8=True, guard_rows=GUARD, want_levels=True)
    got = lookup_rows(raw, rows, True)
    for l in range(4):
        bad = np.asarray(lv[l], np.float64) != lt[l]
        assert not bad.any(), "%s detector: level %d entry %s is %r, truth %r" % (name, l, tuple(np.argwhere(bad)[0]), lv[l][tuple(np.argwhere(bad)[0])],
                                                                                   lt[l][tuple(np.argwhere(bad)[0])])
    r, tol = R.lookup_restated(lt, fl, P, w8)
    assert np.abs(r).max() > 100
    check("%s detector lookup vs restatement" % name, got, r, tol)


def test_lookup_large_grid(ops):
    """102 x 180 (1080p x 0.75): 18360 source rows against a 19200-entry level 0 (the 256-rounded stride); truth for a seeded subset of 600
    rows plus the first and last 64.  Without the kernel's own levels the restated ones are used, and the tolerance carries what a volume
    entry may differ by (raft_ref.volume_tolerance) blended over the window.
    measured: err / tol <= 0.754 vs restatement, <= 0.12 vs truth."""
    name, n, h8, w8, sub, brd = R.LARGE_GRID
    P, rows = h8 * w8, n * h8 * w8
    geo = engine.raft_geometry(h8, w8)
    assert geo[0]["ld"] == 19200 and geo[0]["hp"] * geo[0]["wp"] == 19136
    f1, f2 = R.lookup_features(1000 + P, n, h8, w8)
    flows = R.lookup_flows(2000 + P, n, h8, w8, sub, brd)
    sel = np.unique(np.concatenate([np.arange(64), np.arange(rows - 64, rows), R.rng(9).choice(rows, 600, replace=False)]))
    lt, mt = R.pyramid_truth(f1, f2, sel)
    lr, mr = R.pyramid_restated(f1, f2, sel)
    vt = [R.volume_tolerance(lr[l], mr[l]) for l in range(4)]
    for fam in ("subpixel", "border", "far"):
        fl = flows[fam]
        R.lookup_index_check(fl, P, w8, geo, rows)
        raw, _ = ops.raft_lookup(f1, f2, fl, o8=True, guard_rows=GUARD)
        got = lookup_rows(raw, rows, True)[sel]
        r, tol = R.lookup_restated(lr, fl[sel], P, w8, sel)
        vtw = R.lookup_truth(vt, fl[sel], P, w8, sel)
        check("%s %s vs restatement (restated levels)" % (name, fam), got, r, tol + vtw)
        t = R.lookup_truth(lt, fl[sel], P, w8, sel)
        check("%s %s chain vs truth" % (name, fam), got, t, BUDGET[F16] * R.lookup_truth(mt, fl[sel], P, w8, sel) + vtw + tol)


def test_lookup_refuses_what_the_engine_refuses(ops):
    f1, f2 = R.lookup_features(1, 1, 15, 16)
    with pytest.raises(Exception, match="too small"):
        ops.raft_lookup(f1, f2, np.zeros((15 * 16, 2), np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# convf1
# ---------------------------------------------------------------------------------------------------------------------
CONVF1_CASES = [       # (n, h8, w8, passes, e4m3 copy, im2col + GEMM path, fp16-representable flows)
    (3, 17, 23, 2, True, False, True),          # P = 391: 32-pixel tiles straddle images
    (3, 17, 23, 1, False, False, True),
    (3, 17, 23, 2, False, False, True),
    (3, 17, 23, 2, True, True, True),           # the GEMM path on [a16 | a8] rows with e4m3 weight residuals
    (1, 16, 16, 2, True, False, True),
    (1, 16, 16, 1, True, False, True),
    (1, 16, 16, 2, False, True, True),          # the GEMM path, two fp16 passes
    (1, 16, 16, 2, True, False, False),         # unrounded flows: the kernel rounds the flow to fp16 BY DESIGN (it is the A operand of an fp16
                                                # MFMA, as the im2col operand was) - held to the fp16-operand budget against truth on the raw field
    (4, 102, 180, 2, True, False, True),        # 73440 rows = 2295 tiles > 512 blocks x 4 waves: the grid-stride loop
    (4, 102, 180, 1, False, False, True),
]


@pytest.mark.parametrize("case", CONVF1_CASES, ids=lambda c: "%dx%dx%d_p%d_o8%d_gemm%d_r%d" % tuple(int(v) for v in c))
def test_convf1(ops, case):
    """measured: err / tol <= 0.978 vs restatement (direct and GEMM path; fp16 ties among 9.4 M outputs), <= 0.953 vs truth; the GEMM path's e4m3
    copy 0.998 of its bound."""
    n, h8, w8, passes, o8, gemm, rounded = case
    rows = n * h8 * w8
    flow, w, b = R.convf1_data(31 + h8, n, h8, w8, rounded=rounded)
    raw = ops.raft_convf1(flow, w, b, passes=passes, o8=o8, gemm_path=gemm, guard_rows=GUARD)
    h = raw.view(np.float16)
    got = h[:rows, :128].astype(np.float64)
    what = "convf1 %s" % (case,)
    mx2 = bool(gemm and o8)
    r, tol = R.convf1_restated(flow, w, b, passes, mx2)
    check(what + " vs restatement", got, r, tol)
    t, mag = R.convf1_truth(flow, w, b)
    assert (t > 0).mean() >= 0.30
    budget = BUDGET[F16] if (passes == 1 or not rounded) else (BUDGET[MX2] if mx2 else BUDGET[SPLIT16])
    check(what + " vs truth", got, t, budget * mag + tol)
    preset(what + " guard rows", raw[rows:])
    if o8 and not gemm:
        want = e4m3_bytes(h[:rows, :128].astype(np.float32))
        bad = raw[:rows, 256:384] != want
        assert not bad.any(), "%s e4m3 copy: element %s" % (what, tuple(np.argwhere(bad)[0]))
    elif o8:
        # the GEMM epilogue encodes its fp32 value, not the fp16 one it stores beside it: the copy is within half an e4m3 step of a value that
        # lies within half an fp16 step of the fp16 output
        v16 = h[:rows, :128].astype(np.float64)
        check(what + " e4m3 copy (of the fp32 value)", e4m3_decode(raw[:rows, 256:384]), v16, 0.5 * e4m3_step(v16) + 0.5 * R.f16_step(v16))


# ---------------------------------------------------------------------------------------------------------------------
# flow_head2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", [16, 17])
def test_flow_head2(ops, H, n, split):
    """rows whose last run is shorter than 16 pixels (W = 17, 23, 31, 33), odd run counts (idle upper half wave), non-zero incoming flow.
    The tolerance counts the roundings of a lane's own chain (raft_ref.flow_head2_restated), which is what lets it see a dropped w_lo.
    measured: err / tol <= 0.010 vs restatement; vs truth <= 0.015 (split), <= 0.30 (fp16 weights).  With w_lo dropped from
    flow_head2_kernel<true> in a scratch build the four split cases fail (n 1 H 16 W 16: row 56, 9.4e-3 off, 33 tolerances) while every
    whole-network comparison of tests/test_gpu_raft.py still passes."""
    for W in (16, 17, 23, 31, 33):
        rows = n * H * W
        x, w, b, flow = R.flow_head2_data(41 + W, n, H, W)
        out = ops.raft_flow_head2(x, w, b, flow, split=bool(split), guard_rows=GUARD)
        what = "flow_head2 n %d H %d W %d split %d" % (n, H, W, split)
        r, tol = R.flow_head2_restated(x, w, b, flow, bool(split))
        check(what + " vs restatement", out[:rows], r, tol)
        t, mag = R.flow_head2_truth(x, w, b, flow)
        check(what + " vs truth", out[:rows], t, (BUDGET[SPLIT16] if split else BUDGET[F16]) * mag + tol)
        preset(what + " guard rows", out[rows:])


# ---------------------------------------------------------------------------------------------------------------------
# upsample
# ---------------------------------------------------------------------------------------------------------------------
UPSAMPLE_CASES = [     # (name, n, frame h, frame w, logit std, +-80 logits, margin case)
    ("16x16", 1, 128, 128, 3.0, False, False),
    ("17x23_crop", 2, 131, 181, 3.0, False, False),      # pads (1, 2): odd crops as geometry() gives for 131 x 181
    ("17x23_pm80", 1, 131, 181, 3.0, True, False),
    ("17x23_margin", 2, 131, 181, 3.0, False, True),     # the largest displacement lies in the cropped-away margin
    ("46x62x3", 3, 365, 493, 3.0, False, False),         # 2852 low-res pixels > 256 blocks x 4 waves: the grid-stride loop
]


@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=lambda c: c[0])
def test_upsample(ops, case):
    """output against float64 (tolerance: twice the fast exp's measured error + 22 fp32 roundings, all relative to sum_k softmax_k |8 f_k|);
    maxd bit for bit the float32 maximum of sqrt(u u + v v) over the kernel's own cropped output.
    measured: err / tol <= 0.151."""
    name, n, fh, fw, std, extreme, margin = case
    pad_l, pad_t, h8, w8 = R.pad_geometry(fh, fw)
    flow, mask = R.upsample_data(51 + h8, n, h8, w8, std, extreme)
    if margin:
        flow, mask = R.upsample_margin_case(flow, mask, w8)
        assert pad_l > 0 and pad_t > 0
    up, guard, maxd = ops.raft_upsample(flow, mask, h8, w8, pad_l, pad_t, fh, fw)
    t, mag, _ = R.upsample_truth(flow, mask, h8, w8, pad_l, pad_t, fh, fw)
    check("upsample %s vs truth" % name, up, t, R.upsample_tolerance(mag))
    preset("upsample %s guard" % name, guard)
    want = R.maxd_of(up)
    assert np.array_equal(maxd.view(np.uint32), want.view(np.uint32)), "upsample %s: maxd %r, float32 max over the cropped output %r" % (name, maxd, want)


# ---------------------------------------------------------------------------------------------------------------------
# instance norm
# ---------------------------------------------------------------------------------------------------------------------
def decode_map(raw, rows, C, layout):
    h = raw.view(np.float16)
    hi = h[:rows, :C].astype(np.float64)
    if layout == 0:
        return hi, hi
    if layout == 1:
        return hi + h[:rows, C:2 * C].astype(np.float64), hi
    return hi + np.ldexp(e4m3_decode(raw[:rows, 3 * C:4 * C]), -12), hi


@pytest.mark.parametrize("layout,stats_lo", [(0, 1), (1, 1), (2, 1), (2, 0)])
def test_instnorm(ops, layout, stats_lo):
    """in_stats / in_finalize / in_apply on HW = 1, 2047, 2048, 2049, 5 x 2048 + 37 pixels, C = 64 and 128 (channels 96.. zero), B = 1, 3,
    second operand none / raw / normalised, in place where run_encoder runs it in place; per-channel mean / std 0, 2, 30.  The bound carries
    kappa = 1 + mean^2 / var (raft_ref.instnorm_tolerance): the kernel forms E[x^2] - mean^2 in fp32.  Printed beside it, not asserted: the
    distance of {mean, rstd} from float64 and torch float32 F.instance_norm's on the same data.
    measured: err / tol <= 0.997 (map: fp16 ties), <= 0.27 (mean), <= 0.36 (rstd).  max |normalised - float64| with the kernel's statistics
    against torch float32's, HW 2047 .. 10277: mean / std 2: 0.93e-6 .. 1.6e-6 against 4.2e-7 .. 5.1e-7 (1.9x .. 3.7x); 30: 1.2e-6 ..
    3.2e-6 against 1.2e-6 .. 2.8e-6.  Before the statistics were shifted by a pivot (in_stats_kernel) the same figures were 4.2e-6 .. 5.2e-6
    (10x torch) at 2 and 0.8e-3 .. 1.1e-3 (400x) at 30."""
    import torch
    import torch.nn.functional as F
    k = 0
    for HW in (1, 2047, 2048, 2049, 5 * 2048 + 37):
        for C in (64, 128):
            for B in (1, 3):
                for bmode in (0, 1, 2):
                    ratio = (0.0, 2.0, 30.0)[(k // 3) % 3]
                    k += 1
                    rows = B * HW
                    a = R.instnorm_data(61 + k, B, HW, C, ratio, 96 if C == 128 else 0)
                    b = None if bmode == 0 else R.instnorm_data(600 + k, B, HW, C, 0.0, 96 if C == 128 else 0)
                    inplace = bmode == 0 and k % 2 == 0
                    st, raw = ops.raft_instnorm(a, b, layout=layout, stats_lo=bool(stats_lo), normalise_b=bmode == 2, inplace=inplace, guard_rows=GUARD)
                    av = R.map_value(a, layout)
                    xs = R.map_value(a, layout, with_lo=bool(stats_lo))
                    bv = None if b is None else R.map_value(b, layout)
                    bs = None if b is None else R.map_value(b, layout, with_lo=bool(stats_lo))
                    v, mean, rstd, var = R.instnorm_truth(av, bv, bmode == 2, stats_of=xs, stats_of_b=bs)
                    tol, tmean, trstd, kappa = R.instnorm_tolerance(xs, av, mean, rstd, var, C, v, layout != 0)
                    if bmode == 2:      # the second operand's own statistics carry the same bound
                        _, mb, rb, vb = R.instnorm_truth(bv, stats_of=bs)
                        tol = tol + R.instnorm_tolerance(bs, bv, mb, rb, vb, C, v, layout != 0)[0]
                    what = "instnorm layout %d stats_lo %d HW %d C %d B %d b %d ratio %g" % (layout, stats_lo, HW, C, B, bmode, ratio)
                    got, hi = decode_map(raw, rows, C, layout)
                    check(what + " mean", st[:, :, 0], mean[:, 0], tmean[:, 0] + 2.0 ** -126)
                    check(what + " rstd", st[:, :, 1], rstd[:, 0], trstd[:, 0])
                    check(what + " map", got.reshape(B, HW, C), v, tol)
                    preset(what + " guard rows", raw[rows:])
                    if layout == 2:
                        assert np.array_equal(raw[:rows, 2 * C:3 * C], e4m3_bytes(hi.astype(np.float32))), what + ": hi8 copy"
                    if HW > 1 and bmode == 0 and C == 64:
                        x32 = torch.from_numpy(xs.astype(np.float32)).permute(0, 2, 1)[..., None]
                        ref32 = F.instance_norm(x32, eps=1e-5)[..., 0].permute(0, 2, 1).numpy().astype(np.float64)
                        pre = (xs - mean) * rstd
                        mine = (xs - st[:, None, :, 0].astype(np.float64)) * st[:, None, :, 1].astype(np.float64)
                        print("\n    %s: |normalised - float64| max: kernel statistics %.2e, torch float32 %.2e (kappa <= %.0f)"
                              % (what, np.abs(mine - pre).max(), np.abs(ref32 - pre).max(), kappa.max()), end="")


# ---------------------------------------------------------------------------------------------------------------------
# init_state + put_flow
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,inp_off", [(384, 128), (384, 256), (576, 128), (576, 256)])
def test_state(ops, ld, inp_off):
    """h = tanh(c[:128]) (fp32 master + fp16 copy at 0), inp = relu(c[128:]) at inp_off of hx and hx2, flow == 0 after init; put_flow writes the
    two flow channels at the engine's flow_off (motion offset + 126) of both maps; fp8 copies at byte 768 with ld 576; nothing else written.
    measured: tanh err <= 0.26 of 4 fp32 ulps."""
    rows = 1000
    g = R.rng(71)
    c = R.f16(g.standard_normal((rows, 256)) * 2)
    flow = (g.standard_normal((rows, 2)) * 20).astype(np.float32)
    h32, hx, hx2, f0 = ops.raft_state(c, flow, ld=ld, inp_off=inp_off, guard_rows=GUARD)
    th, inp = R.state_truth(c)
    what = "state ld %d inp_off %d" % (ld, inp_off)
    check(what + " h32", h32[:rows], th, 4 * 2.0 ** -23 * np.maximum(np.abs(th), 2.0 ** -126) + 2.0 ** -140)      # tanhf: 4 ulps allowed (OCML: 2)
    assert np.all(f0[:rows] == 0), what + ": flow after init_state"
    preset(what + " guard", np.concatenate([h32[rows:].view(np.uint8).ravel(), f0[rows:].view(np.uint8).ravel(), hx[rows:].ravel(), hx2[rows:].ravel()]))
    mot = 128 if inp_off == 256 else 256
    fo = mot + 126
    for nm, m in (("hx", hx), ("hx2", hx2)):
        h = m.view(np.float16)
        own = np.zeros(m.shape, bool)
        if nm == "hx":
            assert np.array_equal(h[:rows, :128], h32[:rows].astype(np.float16)), what + ": hx h copy is fp16(h32)"
            own[:rows, :256] = True
        assert np.array_equal(h[:rows, inp_off:inp_off + 128].astype(np.float64), inp), what + " %s: context features" % nm
        own[:rows, 2 * inp_off:2 * inp_off + 256] = True
        assert np.array_equal(h[:rows, fo:fo + 2], flow.astype(np.float16)), what + " %s: flow channels" % nm
        own[:rows, 2 * fo:2 * fo + 4] = True
        if ld == 576:
            for off, cnt in ((0, 128 if nm == "hx" else 0), (inp_off, 128), (fo, 2)):
                if cnt:
                    assert np.array_equal(m[:rows, 768 + off:768 + off + cnt], e4m3_bytes(h[:rows, off:off + cnt].astype(np.float32))), \
                        what + " %s: e4m3 copy at channel %d" % (nm, off)
                    own[:rows, 768 + off:768 + off + cnt] = True
        preset(what + " %s outside the written channels" % nm, m[~own])
