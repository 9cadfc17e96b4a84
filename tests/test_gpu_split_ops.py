"""GPU: single convolution / dense layers in the engines' split precision, through their own packers and launch code
(pb_op_conv2d_split / pb_op_dense_split), against the exact restatement of each layout (tests/split_ref.py) and float64 truth.

Every case runs three checks: (1) element-wise |kernel - restatement| within the fp32-accumulation and output-storage bounds; (2) the kernel
within its layout's budget of float64 truth; (3) the output's bytes - the e4m3 hi8 copy equal to e4m3(hi 2^pa) byte for byte, lo8 within one
e4m3 step of (restatement - hi), and every byte outside rows [0, M) x columns [0, N) of each part left as preset."""
import numpy as np
import pytest

import split_ref as R
from prisma_amd import _lib, engine

pytestmark = pytest.mark.gpu

F16, SPLIT16, MX3, MX2 = R.F16, R.SPLIT16, R.MX3, R.MX2
T_AUTO, T_128, T_256, T_256x64, T_128x96 = 0, 1, 2, 9, 12
KERNEL = {"halo": "conv3x3_c64", "wide": "gemm8_kernel<", "128x128": "gemm_kernel<128, 128,", "128x96": "gemm_kernel<128, 96,",
          "256x64": "gemm_kernel<256, 64,"}


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


def packed_layout(info) -> int:
    return MX3 if info["mx3"] else MX2 if info["mx2"] else SPLIT16 if info["sw"] else F16


def check(raw, info, kname, x, w, b, *, conv=True, stride=1, split_out=True, act=0, pre_relu=False, skip=None, layout=None, kernel=None,
          truth_rows=None, budget=None):
    """the three checks; x is what the layer reads (for a channel slice: the slice); returns (kernel vs restatement / tolerance, kernel vs truth
    / sum |x||w|) for the record"""
    N = w.shape[0]
    lay = packed_layout(info)
    if layout is not None:
        assert lay == layout, (info, layout)
    if kernel is not None:
        assert kname.startswith(KERNEL[kernel]), (kname, kernel)
    # (3a) nothing written outside [M, N] of each part; no NaN / Inf inside
    keep = ~R.written_mask(raw, info, N, split_out)
    assert (raw[keep] == 0xFF).all(), f"bytes outside [M, N] written: {np.argwhere(keep & (raw != 0xFF))[:8].tolist()}"
    val, hi, lo, lo8, hi8 = R.decode_output(raw, info, N, split_out)
    assert np.isfinite(val).all()
    # (1) kernel vs the exact restatement
    acc, mag = R.restate(lay, x, w, info["pa"], info["pw"], sa=info["sa"], conv=conv, stride=stride)
    sk = None if skip is None else R.skip_value(skip, split_out, info["lo8"], info["lo8_pa"])
    ref = R.epilogue(acc, b, sk, pre_relu, act)
    n = R.n_products(lay, int(np.prod(w.shape[1:])), info["sa"])
    tol = R.tolerance(mag, ref, n, split_out, bias=b, skip=sk) + (2.0 ** -20 if act in (R.ACT_SIGMOID, R.ACT_TANH) else 0.0)
    r1 = np.abs(val - ref) / tol
    assert r1.max() <= 1, f"kernel vs restatement: {r1.max():.2f} x tolerance at {np.unravel_index(r1.argmax(), r1.shape)} ({kname})"
    # (2) kernel vs float64 truth
    t, tmag = R.truth(lay, x, w, conv=conv, stride=stride, sa=info["sa"])
    tref = R.epilogue(t, b, sk, pre_relu, act)
    rows = slice(None) if truth_rows is None else truth_rows
    d2 = np.abs(val - tref)[rows]
    lim = (R.BUDGET[lay] if budget is None else budget) * tmag[rows] + tol[rows]
    assert (d2 <= lim).all(), f"kernel vs float64: {(d2 / lim).max():.2f} x budget ({kname})"
    # (3b) the split output's parts
    if lo8 is not None:
        pa = info["lo8_pa"]
        assert np.array_equal(hi8, R.e4m3_bytes(np.ldexp(hi.astype(np.float32), pa))), "hi8 != e4m3(hi 2^pa)"
        r = np.ldexp(ref - hi, pa + 12)
        assert (np.abs(np.ldexp(lo, pa + 12) - r) <= R.e4m3_step(r) + np.ldexp(tol, pa + 12)).all(), "lo8 off by more than one e4m3 step"
    if split_out:
        assert (np.abs(hi - ref) <= np.abs(ref) * 2.0 ** -10 + 2.0 ** -24 + tol).all(), "hi is not fp16(v)"
    return float(r1.max()), float((np.abs(val - tref) / np.maximum(tmag, 1e-30)).max())


def conv_case(ops, lay, xs, ws, *, seed, stride=1, cancel=False, x=None, w=None, ci_off=0, skip=False, **kw):
    if x is None:
        cx = xs[-1]
        x, w, b = R.case_data(seed, xs, ws, cancel=cancel)
        if cx != ws[1]:         # an mx2 map wider than the layer: the layer reads channels [ci_off, ci_off + Ci)
            _, w, b = R.case_data(seed + 1, xs[:-1] + (ws[1],), ws)
    else:
        b = R.case_data(seed, xs, ws)[2]
    opts = {k: kw.pop(k) for k in ("sa", "tapin", "tile", "split_out", "act", "pre_relu") if k in kw}
    B, H, W, _ = x.shape
    kh, kwd = w.shape[2], w.shape[3]
    M = B * ((H + 2 * (kh // 2) - kh) // stride + 1) * ((W + 2 * (kwd // 2) - kwd) // stride + 1)
    s = (np.random.default_rng(seed + 7).standard_normal((M, w.shape[0])) * 0.5).astype(np.float32) if skip else None
    raw, info, kname = ops.conv2d_split(x, w, b, skip=s, stride=stride, layout=lay, ci_off=ci_off, **opts)
    xr = x[..., ci_off:ci_off + w.shape[1]]
    return check(raw, info, kname, xr, w, b, stride=stride, skip=s, split_out=opts.get("split_out", True), act=opts.get("act", 0),
                 pre_relu=opts.get("pre_relu", False), layout=kw.pop("layout", lay), kernel=kw.pop("kernel", None), **kw)


# ---- the halo-tiled 64 -> 64 mx3 conv (halo_conv.hip) and the same layers on the 128 x 128 implicit GEMM --------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (7, 15), (8, 16), (63, 79), (51, 90)])
def test_halo_conv(ops, H, W):
    conv_case(ops, MX3, (3, H, W, 64), (64, 64, 3, 3), seed=H * 100 + W, kernel="halo")


@pytest.mark.parametrize("H,W", [(7, 15), (51, 90)])
def test_halo_shape_on_128_tile(ops, H, W):
    conv_case(ops, MX3, (3, H, W, 64), (64, 64, 3, 3), seed=H * 100 + W, tile=T_128, kernel="128x128")


@pytest.mark.parametrize("act,pre_relu,skip", [(1, False, False), (0, True, True), (1, True, True)])
def test_halo_conv_epilogue(ops, act, pre_relu, skip):
    conv_case(ops, MX3, (3, 9, 21, 64), (64, 64, 3, 3), seed=77, act=act, pre_relu=pre_relu, skip=skip, kernel="halo")
    conv_case(ops, MX3, (3, 9, 21, 64), (64, 64, 3, 3), seed=77, act=act, pre_relu=pre_relu, skip=skip, tile=T_128, kernel="128x128")


# ---- tile choice, K layouts and shapes of the implicit-GEMM convolution -------------------------------------------------------------------------
CONV_CASES = [
    # name, layout, x NHWC, w, stride, options
    ("mx3_3x3_48to72_cw", MX3, (2, 11, 13, 48), (72, 48, 3, 3), 1, dict(kernel="128x96")),
    ("mx3_3x3_96to96_cw", MX3, (2, 10, 17, 96), (96, 96, 3, 3), 1, dict(kernel="128x96")),
    ("mx3_3x3_128to88_s2", MX3, (2, 15, 14, 128), (88, 128, 3, 3), 2, dict(kernel="128x96")),
    ("mx3_1x1_128to32", MX3, (1, 13, 21, 128), (32, 128, 1, 1), 1, dict(kernel="256x64")),
    ("mx3_3x3_64to128_tapmajor", MX3, (2, 9, 12, 64), (128, 64, 3, 3), 1, dict(kernel="128x128")),
    ("mx3_3x3_128to128_slicemajor", MX3, (2, 9, 12, 128), (128, 128, 3, 3), 1, dict(tapin=1, kernel="128x128")),
    ("mx3_3x3_128to64_slicemajor", MX3, (2, 9, 12, 128), (64, 128, 3, 3), 1, dict(tapin=1, kernel="256x64")),
    ("mx3_5x1_128to256_s2", MX3, (1, 17, 9, 128), (256, 128, 5, 1), 2, dict(kernel="128x128")),
    ("mx3_1x5_128to192", MX3, (1, 9, 17, 128), (192, 128, 1, 5), 1, dict(kernel="128x128")),
    ("mx3_3x3_512to96_k144", MX3, (1, 6, 7, 512), (96, 512, 3, 3), 1, dict(kernel="128x128")),       # failed the 128 x 96 check
    ("f16_3x3_1024to96_k144", F16, (1, 5, 6, 1024), (96, 1024, 3, 3), 1, dict(split_out=False, kernel="128x128")),
    ("f16_3x3_96to96_split_out", F16, (1, 6, 9, 96), (96, 96, 3, 3), 1, dict(kernel="128x96")),
    ("mx2_1x5_128to128_tapmajor", MX2, (1, 9, 17, 128), (128, 128, 1, 5), 1, dict(kernel="128x128")),
    ("mx2_5x1_128to128_slicemajor", MX2, (1, 9, 17, 128), (128, 128, 5, 1), 1, dict(tapin=1, kernel="128x128")),
    ("mx2_3x3_256to96_s2", MX2, (2, 10, 9, 256), (96, 256, 3, 3), 2, dict(kernel="128x96")),
    ("split16_sa1_3x3_64to64_s2", SPLIT16, (2, 12, 10, 64), (64, 64, 3, 3), 2, dict(sa=1, kernel="256x64")),
    ("split16_sa0_1x1_96to128", SPLIT16, (1, 11, 13, 96), (128, 96, 1, 1), 1, dict(sa=0, kernel="128x128")),
    ("split16_sa1_1x5_128to96", SPLIT16, (1, 8, 21, 128), (96, 128, 1, 5), 1, dict(sa=1, kernel="128x96")),
    ("f16_3x3_sigmoid", F16, (1, 7, 9, 64), (64, 64, 3, 3), 1, dict(split_out=False, act=3)),
    ("f16_3x3_tanh", F16, (1, 7, 9, 64), (128, 64, 3, 3), 1, dict(split_out=False, act=4)),
    ("mx3_3x3_relu_skip", MX3, (2, 7, 9, 128), (128, 128, 3, 3), 1, dict(act=1, pre_relu=True, skip=True)),
    ("split16_3x3_skip", SPLIT16, (2, 7, 9, 64), (96, 64, 3, 3), 1, dict(skip=True, kernel="128x96")),
    ("mx2_1x1_skip_relu", MX2, (1, 9, 9, 128), (64, 128, 1, 1), 1, dict(act=1, skip=True, kernel="256x64")),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_split(ops, case):
    name, lay, xs, ws, stride, opt = case
    conv_case(ops, lay, xs, ws, seed=sum(map(ord, name)), stride=stride, **dict(opt))


@pytest.mark.parametrize("ci_off", [0, 128])
def test_mx2_channel_slice(ops, ci_off):
    # the layer reads 256 of a 384-channel [a16 | a8] map: the fp8 copy of its slice is not adjacent (a8_rel != Ci)
    conv_case(ops, MX2, (1, 9, 13, 384), (128, 256, 1, 5), seed=31 + ci_off, ci_off=ci_off, tapin=1)
    conv_case(ops, MX2, (1, 9, 13, 384), (96, 256, 3, 3), seed=37 + ci_off, ci_off=ci_off)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tile_n96_modes(ops, mode):
    # 128 x 128 (0), 128 x 96 on the per-tap K axis (1), 128 x 96 on the packed-channel K axis (2, the default)
    try:
        ops.set_option("tile_n96", mode)
        conv_case(ops, MX3, (2, 10, 17, 96), (96, 96, 3, 3), seed=5, kernel="128x96" if mode else "128x128")
    finally:
        ops.set_option("tile_n96", 2)


FORCED = [
    ("wide_N192", MX3, (1, 13, 21, 128), (192, 128, 3, 3), T_256, "wide"),
    ("wide_N256", MX3, (2, 9, 15, 64), (256, 64, 1, 1), T_256, "wide"),
    ("256x64_N64", SPLIT16, (1, 13, 21, 64), (64, 64, 3, 3), T_256x64, "256x64"),
    ("128x96_N96", MX3, (1, 13, 21, 128), (96, 128, 3, 3), T_128x96, "128x96"),
    ("128_N96", MX3, (1, 13, 21, 96), (96, 96, 3, 3), T_128, "128x128"),
]


@pytest.mark.parametrize("case", FORCED, ids=[c[0] for c in FORCED])
def test_forced_tiles(ops, case):
    name, lay, xs, ws, tile, kern = case
    conv_case(ops, lay, xs, ws, seed=sum(map(ord, name)), tile=tile, kernel=kern)


def test_auto_wide_tile_N192(ops):
    # TILE_AUTO puts N = 192 on the 256 x 256 tile from 256 row tiles on (gemm.hip PB_TILE_WIDE)
    conv_case(ops, MX3, (1, 256, 256, 64), (192, 64, 1, 1), seed=9, kernel="wide")


def test_split_k_128(ops):
    try:
        ops.set_option("op_splitk", 1)
        conv_case(ops, MX3, (1, 9, 11, 256), (128, 256, 3, 3), seed=13, tile=T_128, kernel="128x128")
        conv_case(ops, SPLIT16, (1, 9, 11, 256), (128, 256, 3, 3), seed=14, tile=T_128, kernel="128x128")
    finally:
        ops.set_option("op_splitk", 0)


def test_explicit_128x96_keeps_its_k_check(ops):
    # the tile choice no longer gives a 144-K-tile layer the 128 x 96 tile; asking for it explicitly still fails loudly
    x, w, b = R.case_data(3, (1, 6, 7, 512), (96, 512, 3, 3))
    with pytest.raises(_lib.PrismaBandsError, match="128 K tiles"):
        ops.conv2d_split(x, w, b, layout=MX3, tile=T_128x96)


# ---- the seeded data of the CPU sensitivity test (tests/test_split_ref_cpu.py test_tolerance_sees_the_bugs) ------------------------------------
@pytest.mark.parametrize("case", R.SENS_CASES, ids=[c[0] for c in R.SENS_CASES])
def test_sensitivity_cases_on_gpu(ops, case):
    name, lay, xs, ws, stride, seed, cancel = case
    x, w, b = R.case_data(seed, xs, ws, cancel=cancel)
    conv_case(ops, lay, xs, ws, seed=seed, x=x, w=w, stride=stride, sa=1)


# ---- dense layers ---------------------------------------------------------------------------------------------------------------------------------
DENSE = [
    ("mx2_tokens_128", MX2, 1000, 384, 128, T_AUTO, {}, "128x128"),
    ("mx2_tokens_256", MX2, 1000, 384, 256, T_256, {}, "wide"),
    ("mx2_K192_falls_back_to_split16", SPLIT16, 333, 192, 128, T_AUTO, dict(split_out=False), "128x128"),
    ("split16_sa0_K192", SPLIT16, 333, 192, 128, T_AUTO, dict(sa=0), "128x128"),
    ("split16_sa1_K192", SPLIT16, 333, 192, 128, T_AUTO, dict(sa=1), "128x128"),
    ("split16_sa1_K320_N64", SPLIT16, 517, 320, 64, T_AUTO, dict(sa=1), "256x64"),
    ("mx3_K256_N96", MX3, 300, 256, 96, T_AUTO, {}, "128x128"),
    ("f16_K192_tanh", F16, 200, 192, 128, T_AUTO, dict(split_out=False, act=4), "128x128"),
]


@pytest.mark.parametrize("case", DENSE, ids=[c[0] for c in DENSE])
def test_dense_split(ops, case):
    name, lay, M, K, N, tile, opt, kern = case
    x, w, b = R.case_data(sum(map(ord, name)), (M, K), (N, K))
    req = MX2 if name.startswith("mx2") else lay
    raw, info, kname = ops.dense_split(x, w, b, layout=req, tile=tile, **opt)
    check(raw, info, kname, x, w, b, conv=False, split_out=opt.get("split_out", True), act=opt.get("act", 0), layout=lay, kernel=kern)


def test_dense_skip(ops):
    x, w, b = R.case_data(21, (300, 256), (128, 256))
    s = np.random.default_rng(22).standard_normal((300, 128)).astype(np.float32)
    raw, info, kname = ops.dense_split(x, w, b, skip=s, layout=MX2)
    check(raw, info, kname, x, w, b, conv=False, skip=s, layout=MX2)


# ---- outliers ---------------------------------------------------------------------------------------------------------------------------------------
def test_activations_above_448(ops):
    # hi8 clamps at 448: that pixel's hi8 . w_lo8 correction degrades to the single-pass error, nothing else moves and nothing is NaN / Inf
    x, w, b = R.case_data(41, (1, 9, 14, 128), (128, 128, 1, 1))
    hot = [(0, 2, 3, 5), (0, 7, 11, 100), (0, 4, 0, 64)]
    for i, (bb, yy, xx, cc) in enumerate(hot):
        x[bb, yy, xx, cc] = (600.0, -1000.0, 460.0)[i]
    rows = np.ones(9 * 14, bool)
    for bb, yy, xx, _ in hot:
        rows[yy * 14 + xx] = False
    raw, info, kname = ops.conv2d_split(x, w, b, layout=MX3)
    check(raw, info, kname, x, w, b, layout=MX3, truth_rows=rows)
    val = R.decode_output(raw, info, 128, True)[0]
    t, tmag = R.truth(MX3, x, w)
    bad = np.abs(val - R.epilogue(t, b))[~rows] / tmag[~rows]
    assert bad.max() < 2.0 ** -11          # degraded to about the fp16-only error, not worse


def test_wide_dynamic_range_weights(ops):
    # small activations keep every output below 224: above it a split output's lo8 (residual 2^12, up to 2^-11 |v|) saturates at 448 by design
    x, w, b = R.case_data(43, (1, 8, 9, 128), (96, 128, 3, 3), x_scale=0.02)
    w[3, 5, 1, 1] = 3000.0                 # w_hi 2^(pw - 12) would pass 448 without the 20 - e(max |w|) cap
    w[7, 9, 0, 2] = 1e-6
    raw, info, kname = ops.conv2d_split(x, w, b, layout=MX3)
    assert info["pw"] == R.weight_pw(w, True) == 20 - 12
    # the cap costs the other weights their w_lo8 bits (the residuals of |w| ~ 0.1 land in e4m3's subnormals at 2^8): the kernel still meets
    # the restatement exactly, and float64 within the fp16-only budget
    check(raw, info, kname, x, w, b, layout=MX3, budget=R.BUDGET[F16])


def test_zero_weights(ops):
    x, _, b = R.case_data(45, (1, 8, 9, 128), (96, 128, 3, 3))
    w = np.zeros((96, 128, 3, 3), np.float32)
    raw, info, kname = ops.conv2d_split(x, w, b, layout=MX3)
    assert info["pw"] == 0
    check(raw, info, kname, x, w, b, layout=MX3)
    val = R.decode_output(raw, info, 96, True)[0]
    assert np.array_equal(val, np.broadcast_to(R.skip_value(b, True, True), val.shape))
