"""GPU: the GEMM's fused epilogues one by one (pb_op_gemm_resid / _qkv / _patch / _pixshuf / _fc1, pb_op_conv_head: EPI_RESID, EPI_QKV, EPI_PATCH,
EPI_PIXSHUF, EPI_HEAD and fc1's GELU + fp8 mode of gemm_kernels.h, launched as DepthEngine::vit / head launch them) against tests/epi_ref.py: every value within the accumulation bound of the layout's exact restatement and
within the layout's budget of float64 truth, every byte the epilogue does not own still 0xFF, and the kernel symbol that ran.

The `measured:` lines give (kernel vs restatement / tolerance, kernel vs float64 / limit), the worst over the test's cases, on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import epi_ref as R
import split_ref as S
from prisma_amd import engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"f16": R.F16, "split16": R.SPLIT16, "mx2": R.MX2}
EPI_RESID, EPI_QKV, EPI_PATCH = 1, 2, 4


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


@pytest.fixture(scope="module")
def cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ran(kname: str, tile: str, epi: int, info: dict, layout: int, pw_of=None):
    assert kname.startswith(R.kernel_prefix(tile, epi)), (kname, tile, epi)
    assert (info["mx2"], info["sw"]) == (int(layout == R.MX2), int(layout != R.F16)), info
    assert info["pa"] == 0 and (pw_of is None or info["pw"] == (S.weight_pw(pw_of, False) if layout == R.MX2 else 0)), info


def record(r):
    print("measured: %.3f / %.3f" % r)
    return r


# ---- EPI_RESID ----------------------------------------------------------------------------------------------------------------------------
def resid_case(ops, shape, layout, tile, seed=None, ldr=0, splitk=False):
    M, N, K = shape
    d = R.resid_data(M + N + K if seed is None else seed, M, N, K)
    raw, info, kname = ops.gemm_resid(*d, layout=layout, tile=R.T_256 if tile == "wide" else R.T_128, ldr=ldr)
    ran(kname, tile, EPI_RESID, info, layout, R.fold(d[1], d[2], d[3])[0])
    assert (info["splitk"] > 1) == bool(splitk), info
    return record(R.resid_verify("resid %s" % (shape,), raw, *d, layout)), raw


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", R.RESID_128, ids=lambda s: "%dx%dx%d" % s)
def test_resid_128_tile(ops, shape, layout):
    """partial row tiles on every shape, three column tiles on the second.  measured: 0.347 / 0.243"""
    resid_case(ops, shape, LAYOUTS[layout], "128")


def test_resid_row_stride_wider_than_the_layer(ops):
    """ldr = N + 8: the tails of the rows stay preset.  measured: 0.258 / 0.080"""
    resid_case(ops, (300, 384, 256), R.MX2, "128", ldr=392)
    resid_case(ops, (300, 256, 128), R.MX2, "wide", ldr=264)


def test_resid_split_k(ops):
    """the two-launch split-K reduction on top of the residual rows (the launch reports its factor), byte-identical across two calls.  measured: 0.025 / 0.023"""
    try:
        ops.set_option("op_splitk", 1)
        _, a = resid_case(ops, R.RESID_SPLITK, R.MX2, "128", splitk=True)
        _, b = resid_case(ops, R.RESID_SPLITK, R.MX2, "128", splitk=True)
    finally:
        ops.set_option("op_splitk", 0)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", R.RESID_WIDE, ids=lambda s: "%dx%dx%d" % s)
def test_resid_wide_tile_one_workgroup_per_tile(ops, cu, shape, layout):
    """a partial row tile, and on N = 384 a partial column tile.  measured: 0.416 / 0.299"""
    assert -(-shape[0] // 256) * -(-shape[1] // 256) <= cu
    resid_case(ops, shape, LAYOUTS[layout], "wide")


@pytest.fixture(scope="module")
def persistent(cu):
    shape = R.resid_persistent_shape(cu)
    assert -(-shape[0] // 256) * -(-shape[1] // 256) > cu
    d = R.resid_data(cu, *shape)
    return shape, d, R.resid_reference(*d, R.MX2)


def test_resid_wide_tile_persistent(ops, persistent):
    """more tiles than CUs: interior tiles (resid_swap) and edge tiles in one launch, byte-identical across two calls.  measured: 0.345 / 0.117"""
    shape, d, ref = persistent
    raws = []
    for _ in range(2):
        raw, info, kname = ops.gemm_resid(*d, layout=R.MX2, tile=R.T_256)
        ran(kname, "wide", EPI_RESID, info, R.MX2)
        raws.append(raw)
    record(R.resid_verify("resid persistent %s" % (shape,), raws[0], *d, R.MX2, ref=ref))
    assert np.array_equal(raws[0], raws[1])


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import epi_ref as R
from prisma_amd import engine
cu = torch.cuda.get_device_properties(0).multi_processor_count
ops = engine.Ops(0)
raw, info, kname = ops.gemm_resid(*R.resid_data(cu, *R.resid_persistent_shape(cu)), layout=R.MX2, tile=R.T_256)
ops.close()
assert kname.startswith(R.kernel_prefix("wide", 1)), kname
np.save(%r, raw)
"""


@pytest.mark.parametrize("switch", ["PB_RESID_ATOMIC=1", "PB_GEMM_PERSIST=0", "PB_GEMM_PREFETCH=0"])
def test_resid_switches(persistent, switch, tmp_path):
    """the launcher reads its switches once per process: a fresh child runs the persistent shape and the parent verifies its buffer.
    measured: 0.334 / 0.111 (PB_RESID_ATOMIC=1), 0.345 / 0.117 (the other two)"""
    shape, d, ref = persistent
    out = str(tmp_path / "raw.npy")
    key, value = switch.split("=")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), out)], env=dict(os.environ, **{key: value}), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    record(R.resid_verify("resid %s" % switch, np.load(out), *d, R.MX2, ref=ref))


# ---- EPI_QKV ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", R.QKV_CASES, ids=lambda c: c[0])
def test_qkv(ops, case, layout):
    """Q (pre-scaled) and K as [b, head, t, 64], V through the LDS transpose as [b, head, 64, ntp]; M = 144 puts two batch boundaries inside
    one wave's rows.  measured: 0.155 / 0.175"""
    name, tile, D, B, ntp = case
    lay = LAYOUTS[layout]
    A, w, b = R.qkv_data(sum(map(ord, name)), D, B, ntp)
    q, k, vt, info, kname = ops.gemm_qkv(A, w, b, B, ntp, layout=lay, tile=tile)
    ran(kname, "wide" if tile == R.T_256 else "128", EPI_QKV, info, lay, w)
    record(R.qkv_verify(name, q, k, vt, A, w, b, B, ntp, lay))


# ---- EPI_PATCH ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["f16", "split16"])
@pytest.mark.parametrize("case", R.PATCH_CASES, ids=lambda c: c[0])
def test_patch(ops, case, layout):
    """rows (b, patch) land on rows b ntp + 1 + patch with pos[1 + patch]; class, pad and guard rows stay preset.  measured: 0.334 / 0.143"""
    name, D, B, P, ntp = case
    lay = LAYOUTS[layout]
    A, w, b, pos = R.patch_data(D + P, D, B, P)
    raw, info, kname = ops.gemm_patch(A, w, b, pos, B, ntp, layout=lay)
    ran(kname, "128", EPI_PATCH, info, lay)
    record(R.patch_verify(name, raw, A, w, b, pos, B, ntp, lay))


# ---- EPI_HEAD -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=lambda c: "%dx%dx%d_C%d_%s" % (*c[0], c[1], c[2]))
def test_head(ops, case):
    """3 x 3 convolution to 32 channels, ReLU, dot with w2, + b2, ReLU on the 256 x 32 tile; a third of the pixels clamp.  measured: 0.022 / 0.014"""
    (B, H, W), C, layout = case
    lay = {"f16": R.F16, "split16": R.SPLIT16, "mx3": R.MX3}[layout]
    x, w, b, w2, b2 = R.head_data(B * H * W + C, B, H, W, C)
    raw, info, kname = ops.conv_head(x, w, b, w2, b2, layout=lay)
    assert kname.startswith(R.HEAD_KERNEL), kname
    assert (info["mx3"], info["sw"]) == (int(lay == R.MX3), int(lay != R.F16)) and info["pw"] == (S.weight_pw(w, True) if lay == R.MX3 else 0), info
    record(R.head_verify("head %s" % (case,), raw, x, w, b, w2, b2, lay))


# ---- EPI_PIXSHUF (dense) ------------------------------------------------------------------------------------------------------------------
PIXSHUF_KERNEL = {R.T_128: "gemm_kernel<128, 128, 2, 2, 0, 3,", R.T_256: "gemm8_kernel<0, 3,"}
PIXSHUF_GPU = [(c, g, R.T_128) for c in R.PIXSHUF_CASES for g in R.PIXSHUF_GRIDS] + [(R.PIXSHUF_CASES[0], R.PIXSHUF_GRIDS[0], R.T_256)]


@pytest.mark.parametrize("layout", ["f16", "split16", "mx3"])
@pytest.mark.parametrize("case,grid,tile", PIXSHUF_GPU, ids=["%s_%dx%d_t%d" % (c[0], *g, t) for c, g, t in PIXSHUF_GPU])
def test_pixshuf_dense(ops, case, grid, tile, layout):
    """the transposed convolutions of the DPT head as 1 x 1 GEMMs: 33 columns take the buffer-addressed stores (a wave's 128 rows wrap the grid),
    7 columns the flat ones, 96 channels the LDS path; outputs [hi], [hi | lo] and [hi | hi8 | lo8].  measured: 0.208 / 0.229"""
    name, s, C = case
    lay = {"f16": R.F16, "split16": R.SPLIT16, "mx3": R.MX3}[layout]
    x, wt, b = R.pixshuf_data(s * C + grid[0], *grid, C, s)
    raw, info, kname = ops.gemm_pixshuf(x, wt, b, s, layout=lay, tile=tile)
    assert kname.startswith(PIXSHUF_KERNEL[tile]), kname
    assert (info["mx3"], info["sw"]) == (int(lay == R.MX3), int(lay != R.F16)), info
    assert info["pw"] == (S.weight_pw(R.pixshuf_rows(wt, s), True) if lay == R.MX3 else 0), info
    record(R.pixshuf_verify("%s %s" % (name, grid), raw, x, wt, b, s, lay))


# ---- fc1 as the split ViT runs it ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FC1_CASES, ids=lambda c: "%dx%dx%d_t%d" % c)
def test_fc1_gelu_with_fp8_copy(ops, case):
    """fp16 weights on the MX build of the kernel (nk16 = K / 64), GELU (tolerance: twice the 6.39e-7 absolute that tools/probe/gelu_probe.hip measured
    for fast_gelu2 against float64 erf-GELU on [-8, 8], epi_ref.GELU_ABS_MEASURED), the e4m3 copy of the stored fp16 byte for byte.  measured: 0.101 / 0.153"""
    M, K, N, tile = case
    A, w, b = R.fc1_data(M + K, M, K, N)
    raw, info, kname = ops.gemm_fc1(A, w, b, tile=tile)
    assert kname.startswith(R.FC1_KERNEL[tile]) and kname.rstrip(">").endswith("true"), kname          # the MX build
    assert (info["nk16"], info["K"], info["mx2"], info["sw"], info["pa"]) == (K // 64, K, 0, 0, 0), info
    record(R.fc1_verify("fc1 %s" % (case,), raw, A, w, b))


# ---- ACT_GRU_ZR / ACT_GRU_Q ---------------------------------------------------------------------------------------------------------------
GRU_GPU = [(g, m, o) for g in R.GRU_GRIDS for m in R.GRU_MODES for o in ((1, 5), (5, 1))]


def gru_ran(kname, info, tile, lay):
    assert kname.startswith(R.GRU_KERNEL[tile]) and kname.rstrip(">").endswith("true" if lay == R.MX2 else "false"), kname
    assert (info["mx2"], info["sw"], info["pa"]) == (int(lay == R.MX2), int(lay == R.MX2), 0), info


@pytest.mark.parametrize("tile", [R.T_128, R.T_256])
@pytest.mark.parametrize("grid,mode,orient", GRU_GPU, ids=["%dx%d_%s_%dx%d" % (*g, m[0], *o) for g, m, o in GRU_GPU])
def test_gru_zr(ops, grid, mode, orient, tile):
    """sigmoid; z to zrb's first half (the r half stays preset), r h32 and its fp8 twin to the next convolution's input map at its own stride.
    measured: 0.039 / 0.038"""
    name, gc, hoist, lay = mode
    d = R.gru_data(len(name) + orient[0] + grid[0], "zr", *grid, gc, *orient, hoist)
    zrb, rh, info, kname = ops.raft_gru("zr", d["x"], d["w"], d["b"], d["h32"], add1=d["add1"], add2=d["add2"], layout=lay, tile=tile)
    gru_ran(kname, info, tile, lay)
    record(R.gru_zr_verify("zr %s %s" % (name, grid), zrb, rh, d, lay))


@pytest.mark.parametrize("grid,mode,orient", GRU_GPU, ids=["%dx%d_%s_%dx%d" % (*g, m[0], *o) for g, m, o in GRU_GPU])
def test_gru_q(ops, grid, mode, orient):
    """fast tanh, h = (1 - z) h + z q in place in fp32, its fp16 copy (and fp8 twin) to the map.  measured: 0.535 / 0.247"""
    name, gc, hoist, lay = mode
    d = R.gru_data(len(name) + orient[0] + grid[0], "q", *grid, gc, *orient, hoist)
    out, hraw, info, kname = ops.raft_gru("q", d["x"], d["w"], d["b"], d["h32"], z=d["z"], add1=d["add1"], add2=d["add2"], layout=lay, tile=R.T_128)
    gru_ran(kname, info, R.T_128, lay)
    record(R.gru_q_verify("q %s %s" % (name, grid), out, hraw, d, lay))


@pytest.mark.parametrize("lay", [R.F16, R.MX2], ids=["f16", "mx2"])
def test_gru_chain(ops, lay):
    """ZR (1 x 5), Q, ZR (5 x 1), Q with the op outputs fed forward: every step is verified on the inputs it was given (its own tolerance), and the
    final state against the float64 chain run from the start at the summed tolerance of the four steps.  measured: steps 0.258 / 0.258; final state 4.89e-4 against 1.59e-2 (f16) / 8.46e-3 (mx2)"""
    h8, w8 = R.GRU_GRIDS[0]
    rows = R.GRU_N * h8 * w8
    base = R.gru_data(77, "zr", h8, w8, 384, 1, 5, False)
    x, h32 = base["x"].copy(), base["h32"].copy()
    x64, h64, bound = x.astype(np.float64), h32.astype(np.float64), 0.0
    for step, (kh, kw) in enumerate(((1, 5), (5, 1))):
        wz = R.gru_data(80 + step, "zr", h8, w8, 384, kh, kw, False)
        wq = R.gru_data(90 + step, "q", h8, w8, 384, kh, kw, False)
        for dd in (wz, wq):                                             # rows of l1 norm <= 1 / 2: a step amplifies an incoming error by at most 1.5
            dd["w"] = (dd["w"] * (0.5 / np.abs(dd["w"]).sum(axis=(1, 2, 3)).max())).astype(np.float32)
        dz = dict(wz, x=x, h32=h32)
        zrb, rh, info, kname = ops.raft_gru("zr", x, dz["w"], dz["b"], h32, layout=lay)
        gru_ran(kname, info, R.T_128, lay)
        r = R.gru_zr_verify("chain zr %d" % step, zrb, rh, dz, lay)
        z = zrb[:rows].copy().view(np.float16).astype(np.float32)
        z[:, 128:] = 0                                                  # (the preset r half is not read)
        x2 = x.copy()
        x2.reshape(rows, 384)[:, :128] = rh[:rows, :256].copy().view(np.float16).astype(np.float32)
        dq = dict(wq, x=x2, h32=h32, z=z)
        out, hraw, info, kname = ops.raft_gru("q", x2, dq["w"], dq["b"], h32, z=z, layout=lay)
        gru_ran(kname, info, R.T_128, lay)
        r = max(max(r), *R.gru_q_verify("chain q %d" % step, out, hraw, dq, lay))
        record((r, r))
        # the float64 chain: the same step on its own state, Lipschitz-propagating what the earlier steps were allowed
        def conv64(xx, w, b):
            return S.conv_nhwc(xx, w, 1) + b.astype(np.float64)
        v = conv64(x64, dz["w"], dz["b"])
        z64, r64 = 1 / (1 + np.exp(-v[:, :128])), 1 / (1 + np.exp(-v[:, 128:]))
        x64b = x64.copy()
        x64b.reshape(rows, 384)[:, :128] = r64 * h64
        h64 = (1 - z64) * h64 + z64 * np.tanh(conv64(x64b, dq["w"], dq["b"]))
        x64 = x64.copy()
        x64.reshape(rows, 384)[:, :128] = h64
        h32 = hraw[:rows].copy().view(np.float32)
        x = x.copy()
        x.reshape(rows, 384)[:, :128] = out[:rows, :256].copy().view(np.float16).astype(np.float32)
    # summed tolerance: per step the fp16 rounding of the carried maps (2^-11 of values up to 1.2), the layout's budget on sums of l1 norm 1 / 2
    # and the activations' 2^-20, amplified by the later convolutions' gain (rows of l1 norm 1 / 2, activation slopes <= 1: at most 1.5 a step)
    gain = 0.5
    per_step = 1.2 * 2.0 ** -11 + S.BUDGET[lay] * gain * 1.2 + 2.0 ** -18
    tol = per_step * (1 + gain) ** 3 * 4
    err = float(np.abs(h32.astype(np.float64) - h64).max())
    print("measured: chain err %.3e, summed tolerance %.3e" % (err, tol))
    assert err <= tol, (err, tol)


# ---- EPI_PIXSHUF (convolution) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("layout", ["f16", "split16", "mx3"])
@pytest.mark.parametrize("grid", R.PIXSHUF_CONV_GRIDS, ids=lambda g: "%dx%d" % g)
def test_pixshuf_conv(ops, grid, layout, relu):
    """RAFT's stem form: a 3 x 3 convolution over 64 channels to 4 x 64 columns, s = 2; 46 columns take the buffer-addressed stores, 11 the flat
    ones.  measured: 0.082 / 0.101"""
    lay = {"f16": R.F16, "split16": R.SPLIT16, "mx3": R.MX3}[layout]
    x, wt, b = R.pixshuf_conv_data(grid[0], *grid)
    raw, info, kname = ops.conv_pixshuf(x, wt, b, layout=lay, act=int(relu))
    assert kname.startswith("gemm_kernel<128, 128, 2, 2, 1, 3,"), kname
    assert (info["mx3"], info["sw"]) == (int(lay == R.MX3), int(lay != R.F16)) and info["pw"] == (S.weight_pw(wt, True) if lay == R.MX3 else 0), info
    record(R.pixshuf_verify("stem %s" % (grid,), raw, x, wt, b, 2, lay, conv=True, relu=relu))
