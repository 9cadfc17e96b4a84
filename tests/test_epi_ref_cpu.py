"""CPU: the checks of tests/test_gpu_epilogue_ops.py, run on float32 restatements of the kernels instead of the kernels' buffers.  A
restatement - the layout's operands as split_ref builds them, products summed in float32 sixteen at a time onto the accumulator the kernel
starts from, the epilogue's own float32 / fp16 roundings, the output in the kernel's layout inside a buffer preset to 0xFF - must pass
every verifier of tests/epi_ref.py at half its tolerance or less, and with one planted fault it must fail."""
import numpy as np
import pytest

import epi_ref as R
import split_ref as S

F32 = np.float32
GUARD = 4
LAYOUTS = {"f16": R.F16, "split16": R.SPLIT16, "mx2": R.MX2}


def caught(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


def gemm32(acc0, layout, A, w, pw, drop_w_lo=False):
    """float32 accumulators starting from acc0 [M, N]; every segment of the layout's K axis added sixteen products at a time"""
    segs = S.operand_pairs(layout, A, w, 0, pw, 0)
    if drop_w_lo:
        assert len(segs) == 2
        segs = segs[:1]
    acc = np.broadcast_to(np.asarray(acc0, F32), (A.shape[0], w.shape[0])).copy()
    for _, a, b in segs:
        a, b = a.astype(F32), b.astype(F32)                   # fp16 / scaled e4m3 values: exact in float32
        for k0 in range(0, a.shape[1], 16):
            acc = acc + a[:, k0:k0 + 16] @ b[:, k0:k0 + 16].T
    return acc


def preset(rows: int, row_bytes: int) -> np.ndarray:
    return np.full((rows, row_bytes), 0xFF, np.uint8)


# ---- EPI_RESID ----------------------------------------------------------------------------------------------------------------------------
def resid_restated(A, w, b, gamma, X, layout, ldr, bug=None):
    M, N = X.shape
    wf, bf = R.fold(w, b, gamma)
    if bug == "layerscale_missing":
        wf, bf = w, b
    pw = S.weight_pw(wf, False) if layout == R.MX2 else 0
    acc0 = X + bf
    if bug == "residual_not_added":
        acc0 = bf
    if bug == "bias_dropped":
        acc0 = X
    v = gemm32(acc0, layout, A, wf, pw, drop_w_lo=bug == "w_lo_dropped")
    if bug == "layerscale_twice":                          # gamma multiplied in the epilogue onto weights that carry it already
        v = X + gamma * gemm32(bf, layout, A, wf, pw)
    raw = preset(M + GUARD, ldr * 4)
    raw[:M, :4 * N] = v.astype(F32).view(np.uint8)
    if bug == "tail_written":
        raw[M - 1, 4 * N:] = 0
    if bug == "guard_written":
        raw[M, :8] = 0
    return raw


RESID_CPU = [(s, l) for s in R.RESID_128 + R.RESID_WIDE for l in LAYOUTS]


@pytest.mark.parametrize("shape,layout", RESID_CPU, ids=["%dx%dx%d_%s" % (*s, l) for s, l in RESID_CPU])
def test_resid_restatement_passes(shape, layout):
    M, N, K = shape
    lay = LAYOUTS[layout]
    d = R.resid_data(M + N + K, M, N, K)
    r1, r2 = R.resid_verify("resid", resid_restated(*d, lay, N + 8), *d, lay)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)


@pytest.mark.parametrize("bug", ["layerscale_twice", "layerscale_missing", "residual_not_added", "bias_dropped", "tail_written", "guard_written"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_resid_faults_are_seen(bug, layout):
    lay = LAYOUTS[layout]
    d = R.resid_data(7, 144, 128, 128)
    assert caught(lambda: R.resid_verify("resid", resid_restated(*d, lay, 136, bug=bug), *d, lay)), bug


@pytest.mark.parametrize("layout", ["split16", "mx2"])
@pytest.mark.parametrize("shape", R.RESID_128)
def test_resid_dropped_weight_residual_is_seen(shape, layout):
    lay = LAYOUTS[layout]
    d = R.resid_data(11, *shape, signed=True)
    r1, r2 = R.resid_verify("resid", resid_restated(*d, lay, shape[1]), *d, lay)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)
    assert caught(lambda: R.resid_verify("resid", resid_restated(*d, lay, shape[1], bug="w_lo_dropped"), *d, lay))


def test_resid_data():
    A, w, b, gamma, X = R.resid_data(1, 144, 128, 128)
    assert gamma.min() >= 0.05 and gamma.max() <= 2 and (X == 0).all(axis=1).sum() == 1
    _, w, _, gamma, _ = R.resid_data(1, 144, 128, 128, signed=True)
    wf, _ = R.fold(w, b, gamma)
    assert (wf.astype(np.float64) - S.f16(wf) > 0).mean() > 0.99         # the fold keeps the residuals' sign (but for fp16 subnormals)


# ---- EPI_QKV ------------------------------------------------------------------------------------------------------------------------------
def qkv_restated(A, w, b, B, ntp, layout, bug=None):
    M, D = A.shape
    heads = D // 64
    pw = S.weight_pw(w, False) if layout == R.MX2 else 0
    acc = gemm32(F32(0), layout, A, w, pw, drop_w_lo=bug == "w_lo_dropped")
    s = R.qkv_scale(D).astype(F32)
    if bug == "q_unscaled":
        s[:] = 1
    v = (((acc + (0 if bug == "bias_dropped" else b)).astype(F32)) * s).astype(np.float16)
    parts = [v[:, :D], v[:, D:2 * D], v[:, 2 * D:]]
    if bug == "kv_swapped":
        parts[1], parts[2] = parts[2], parts[1]
    m = np.arange(M)[:, None]
    hn = np.arange(D)[None, :]
    head, dd = hn >> 6, hn & 63
    if bug == "head_d_swapped":
        head, dd = hn % heads, hn // heads
    bb, t = m // ntp, m % ntp
    stride = ntp - 3 if bug == "batch_stride_ntok" else ntp
    qk_idx = ((bb * heads + head) * stride + t) * 64 + dd
    vt_idx = qk_idx if bug == "v_not_transposed" else ((bb * heads + head) * 64 + dd) * stride + t
    out = []
    for part, idx, rows, cols in ((parts[0], qk_idx, B * heads * ntp, 64), (parts[1], qk_idx, B * heads * ntp, 64), (parts[2], vt_idx, B * heads * 64, ntp)):
        flat = np.full((rows + GUARD) * cols, 0xFFFF, np.uint16)
        flat[idx.reshape(-1)] = part.reshape(-1).view(np.uint16)
        out.append(flat.view(np.uint8).reshape(rows + GUARD, cols * 2))
    if bug == "guard_written":
        out[2][B * heads * 64, 0] = 0
    return out


QKV_CPU = [(c, l) for c in R.QKV_CASES for l in LAYOUTS]


@pytest.mark.parametrize("case,layout", QKV_CPU, ids=["%s_%s" % (c[0], l) for c, l in QKV_CPU])
def test_qkv_restatement_passes(case, layout):
    name, _, D, B, ntp = case
    lay = LAYOUTS[layout]
    A, w, b = R.qkv_data(sum(map(ord, name)), D, B, ntp)
    r1, r2 = R.qkv_verify(name, *qkv_restated(A, w, b, B, ntp, lay), A, w, b, B, ntp, lay)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)


@pytest.mark.parametrize("bug", ["q_unscaled", "kv_swapped", "v_not_transposed", "head_d_swapped", "batch_stride_ntok", "bias_dropped", "guard_written"])
def test_qkv_faults_are_seen(bug):
    name, _, D, B, ntp = R.QKV_CASES[0]
    A, w, b = R.qkv_data(5, D, B, ntp)
    for lay in LAYOUTS.values():
        assert caught(lambda: R.qkv_verify(name, *qkv_restated(A, w, b, B, ntp, lay, bug=bug), A, w, b, B, ntp, lay)), bug


@pytest.mark.parametrize("layout", ["split16", "mx2"])
def test_qkv_dropped_weight_residual_is_seen(layout):
    name, _, D, B, ntp = R.QKV_CASES[1]
    lay = LAYOUTS[layout]
    A, w, b = R.qkv_data(6, D, B, ntp, signed=True)
    r1, r2 = R.qkv_verify(name, *qkv_restated(A, w, b, B, ntp, lay), A, w, b, B, ntp, lay)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)
    assert caught(lambda: R.qkv_verify(name, *qkv_restated(A, w, b, B, ntp, lay, bug="w_lo_dropped"), A, w, b, B, ntp, lay))


# ---- EPI_PATCH ----------------------------------------------------------------------------------------------------------------------------
def patch_restated(A, w, b, pos, B, ntp, layout, bug=None):
    D = w.shape[0]
    P = A.shape[0] // B
    acc = gemm32(F32(0), layout, A, w, 0, drop_w_lo=bug == "w_lo_dropped")
    pe = np.tile(pos[:P] if bug == "pos_unshifted" else pos[1:], (B, 1))
    v = ((acc + (0 if bug == "bias_dropped" else b)).astype(F32) + pe).astype(F32)
    bi, pi = np.divmod(np.arange(B * P), P)
    rows = bi * (P + 1 if bug == "batch_stride_ntok" else ntp) + pi + (0 if bug == "row_without_plus_1" else 1)
    raw = preset(B * ntp + GUARD, D * 4)
    raw[rows] = v.view(np.uint8)
    if bug == "class_row_overwritten":
        raw[ntp] = 0
    if bug == "pad_row_written":
        raw[1 + P, :32] = 0
    return raw


PATCH_CPU = [(c, l) for c in R.PATCH_CASES for l in ("f16", "split16")]


@pytest.mark.parametrize("case,layout", PATCH_CPU, ids=["%s_%s" % (c[0], l) for c, l in PATCH_CPU])
def test_patch_restatement_passes(case, layout):
    name, D, B, P, ntp = case
    lay = LAYOUTS[layout]
    A, w, b, pos = R.patch_data(D + P, D, B, P)
    r1, r2 = R.patch_verify(name, patch_restated(A, w, b, pos, B, ntp, lay), A, w, b, pos, B, ntp, lay)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)


@pytest.mark.parametrize("bug", ["row_without_plus_1", "pos_unshifted", "class_row_overwritten", "pad_row_written", "batch_stride_ntok", "bias_dropped"])
def test_patch_faults_are_seen(bug):
    name, D, B, P, ntp = R.PATCH_CASES[0]
    A, w, b, pos = R.patch_data(9, D, B, P)
    for lay in (R.F16, R.SPLIT16):
        assert caught(lambda: R.patch_verify(name, patch_restated(A, w, b, pos, B, ntp, lay, bug=bug), A, w, b, pos, B, ntp, lay)), bug


def test_patch_dropped_weight_residual_is_seen():
    name, D, B, P, ntp = R.PATCH_CASES[0]
    A, w, b, pos = R.patch_data(10, D, B, P, signed=True)
    r1, r2 = R.patch_verify(name, patch_restated(A, w, b, pos, B, ntp, R.SPLIT16), A, w, b, pos, B, ntp, R.SPLIT16)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)
    assert caught(lambda: R.patch_verify(name, patch_restated(A, w, b, pos, B, ntp, R.SPLIT16, bug="w_lo_dropped"), A, w, b, pos, B, ntp, R.SPLIT16))


# ---- EPI_HEAD -----------------------------------------------------------------------------------------------------------------------------
HEAD_LAYOUTS = {"f16": R.F16, "split16": R.SPLIT16, "mx3": R.MX3}


def head_restated(x, w, b, w2, b2, layout, bug=None):
    """float32: the layout's products tap by tap and sixteen channels at a time, + bias, ReLU, the 32-term dot in float32, + b2, ReLU"""
    B, H, W, C = x.shape
    pw = S.weight_pw(w, True) if layout == R.MX3 else 0
    xp = [np.pad(a.astype(F32), ((0, 0), (1, 1), (1, 1), (0, 0))) for _, a, _ in S.operand_pairs(layout, x, w, 0, pw, 1)]
    ws = [ww.astype(F32) for _, _, ww in S.operand_pairs(layout, x, w, 0, pw, 1)]
    acc = np.zeros((B * H * W, 32), F32)
    for a, ww in zip(xp, ws):
        for ky in range(3):
            for kx in range(3):
                tap = a[:, ky:ky + H, kx:kx + W].reshape(-1, C)
                for c0 in range(0, C, 16):
                    acc = acc + tap[:, c0:c0 + 16] @ ww[:, c0:c0 + 16, ky, kx].T
    act = acc + b
    if bug != "no_inner_relu":
        act = np.maximum(act, 0)
    s = np.zeros(B * H * W, F32)
    for j in range(32):
        s = s + act[:, j] * w2[j]
    v = s + F32(b2)
    raw = np.frombuffer(preset(B * H * W + GUARD, 4).tobytes(), F32).copy()
    raw[:B * H * W] = v if bug == "no_outer_relu" else np.maximum(v, 0)
    if bug == "guard_written":
        raw[B * H * W] = 0
    return raw


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=lambda c: "%dx%dx%d_C%d_%s" % (*c[0], c[1], c[2]))
def test_head_restatement_passes(case):
    (B, H, W), C, layout = case
    lay = HEAD_LAYOUTS[layout]
    d = R.head_data(B * H * W + C, B, H, W, C)
    r1, r2 = R.head_verify("head", head_restated(*d, lay), *d, lay)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)


@pytest.mark.parametrize("bug", ["no_inner_relu", "no_outer_relu", "guard_written"])
def test_head_faults_are_seen(bug):
    d = R.head_data(3, 1, 7, 9, 64)
    for lay in HEAD_LAYOUTS.values():
        assert caught(lambda: R.head_verify("head", head_restated(*d, lay, bug=bug), *d, lay)), bug


def test_head_data_clamps_a_third():
    for (B, H, W), C, _ in R.HEAD_CASES[::3]:
        x, w, b, w2, b2 = R.head_data(B * H * W + C, B, H, W, C)
        s = np.maximum(S.conv_nhwc(x, w, 1) + b, 0) @ w2.astype(np.float64) + b2
        assert 0.25 < (s <= 0).mean() < 0.42 and (w2 > 0).any() and (w2 < 0).any()


# ---- EPI_PIXSHUF --------------------------------------------------------------------------------------------------------------------------
def pixshuf_restated(x, wt, b, s, layout, bug=None):
    B, h, w, C = x.shape
    Cp = -(-C // 64) * 64
    g = R.pixshuf_rows(wt, s)
    pw = S.weight_pw(g, True) if layout == R.MX3 else 0
    acc = F32(0)
    for _, a, ww in S.operand_pairs(layout, x.reshape(-1, C), g, 0, pw, 1):
        a, ww = a.astype(F32), ww.astype(F32)
        for k0 in range(0, C, 16):
            acc = acc + a[:, k0:k0 + 16] @ ww[:, k0:k0 + 16].T
    n = np.arange(s * s * C)
    co = n % (Cp if bug == "co_modulo_padded" else C)
    v = (acc + b[np.minimum(co, C - 1)]).astype(F32)
    if bug == "dy_dx_swapped":
        v = v.reshape(-1, s, s, C).transpose(0, 2, 1, 3).reshape(-1, s * s * C)
    if bug == "co_modulo_padded":                           # column n lands on tap n / Cp, channel n % Cp
        keep = (n // Cp < s * s) & (co < C)
        moved = np.zeros_like(v)
        moved[:, (n // Cp)[keep] * C + co[keep]] = v[:, keep]
        v = moved
    v = R.pixshuf_arrange(v, B, h, w, C, s)
    px = v.shape[0]
    raw = preset(px + GUARD, (1 if layout == R.F16 else 2) * Cp * 2)
    hi = v.astype(np.float16)
    raw[:px, :2 * C] = hi.view(np.uint8)
    if layout == R.SPLIT16:
        raw[:px, 2 * Cp:2 * Cp + 2 * C] = (v - hi.astype(F32)).astype(np.float16).view(np.uint8)
    if layout == R.MX3:
        raw[:px, 2 * Cp:2 * Cp + C] = S.e4m3_bytes(hi.astype(F32))
        raw[:px, 3 * Cp:3 * Cp + C] = S.e4m3_bytes(np.ldexp(v - hi.astype(F32), 12))
    if bug == "pad_channel_written":
        raw[0, 2 * C:2 * C + 2] = 0
    return raw


PIXSHUF_CPU = [(c, g, l) for c in R.PIXSHUF_CASES for g in R.PIXSHUF_GRIDS[1:] for l in HEAD_LAYOUTS] + [(R.PIXSHUF_CASES[2], R.PIXSHUF_GRIDS[0], "mx3")]


@pytest.mark.parametrize("case,grid,layout", PIXSHUF_CPU, ids=["%s_%dx%d_%s" % (c[0], *g, l) for c, g, l in PIXSHUF_CPU])
def test_pixshuf_restatement_passes(case, grid, layout):
    name, s, C = case
    lay = HEAD_LAYOUTS[layout]
    x, wt, b = R.pixshuf_data(s * C + grid[0], *grid, C, s)
    r1, r2 = R.pixshuf_verify(name, pixshuf_restated(x, wt, b, s, lay), x, wt, b, s, lay)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)


@pytest.mark.parametrize("bug", ["dy_dx_swapped", "co_modulo_padded", "pad_channel_written"])
def test_pixshuf_faults_are_seen(bug):
    name, s, C = R.PIXSHUF_CASES[2]                          # 96 channels carried as 128
    x, wt, b = R.pixshuf_data(4, 5, 7, C, s)
    for lay in HEAD_LAYOUTS.values():
        assert caught(lambda: R.pixshuf_verify(name, pixshuf_restated(x, wt, b, s, lay, bug=bug), x, wt, b, s, lay)), bug


# ---- fc1 mode -----------------------------------------------------------------------------------------------------------------------------
def fc1_restated(A, w, b, bug=None):
    M, N = A.shape[0], w.shape[0]
    v = (gemm32(F32(0), R.F16, A, w, 0) + b).astype(F32)
    g = np.maximum(v, 0) if bug == "relu_for_gelu" else R.gelu64(v).astype(F32)
    h = g.astype(np.float16)
    raw = preset(M + GUARD, 3 * N)
    raw[:M, :2 * N] = h.view(np.uint8)
    raw[:M, 2 * N:] = S.e4m3_bytes(g if bug == "fp8_of_the_fp32_value" else h.astype(F32))
    if bug == "fp8_shifted":
        raw[:M, 2 * N + 1:] = raw[:M, 2 * N:-1].copy()
    return raw


@pytest.mark.parametrize("case", R.FC1_CASES[:2], ids=lambda c: "%dx%dx%d" % c[:3])
def test_fc1_restatement_passes(case):
    M, K, N, _ = case
    A, w, b = R.fc1_data(M + K, M, K, N)
    r1, r2 = R.fc1_verify("fc1", fc1_restated(A, w, b), A, w, b)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)
    v = A.astype(np.float64) @ w.astype(np.float64).T + b
    assert v.min() < -6 and v.max() > 6 and (np.abs(v + 0.75) < 0.05).any()          # both tails and the minimum of the GELU


@pytest.mark.parametrize("bug", ["relu_for_gelu", "fp8_of_the_fp32_value", "fp8_shifted"])
def test_fc1_faults_are_seen(bug):
    M, K, N, _ = R.FC1_CASES[0]
    A, w, b = R.fc1_data(M + K, M, K, N)
    assert caught(lambda: R.fc1_verify("fc1", fc1_restated(A, w, b, bug=bug), A, w, b)), bug


# ---- ACT_GRU_ZR / ACT_GRU_Q ---------------------------------------------------------------------------------------------------------------
def gru_pre32(d, layout):
    """float32 pre-activation: the layout's products tap by tap, sixteen channels at a time, + bias + the hoisted terms"""
    x, w = d["x"], d["w"]
    N, gc, kh, kw = w.shape
    n, H, W, _ = x.shape
    pw = S.weight_pw(w, False) if layout == R.MX2 else 0
    acc = np.zeros((n * H * W, N), F32)
    for _, a, ww in S.operand_pairs(layout, x[..., :gc], w, 0, pw, 0):
        a = np.pad(a.astype(F32), ((0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2), (0, 0)))
        ww = ww.astype(F32)
        for ky in range(kh):
            for kx in range(kw):
                tap = a[:, ky:ky + H, kx:kx + W].reshape(-1, gc)
                for c0 in range(0, gc, 16):
                    acc = acc + tap[:, c0:c0 + 16] @ ww[:, c0:c0 + 16, ky, kx].T
    v = acc + d["b"]
    if d["add1"] is not None:
        v = v + d["add1"] + d["add2"]
    return v.astype(F32)


def gru_zr_restated(d, layout, bug=None):
    rows = d["h32"].shape[0]
    ld = 576 if layout == R.MX2 else 384
    s = (1 / (1 + np.exp(-gru_pre32(d, layout).astype(np.float64)))).astype(F32)
    zc, rc = (s[:, 128:], s[:, :128]) if bug == "z_r_swapped" else (s[:, :128], s[:, 128:])
    h = S.f16(d["h32"]) if bug == "rh_from_fp16_h" else d["h32"]
    rh32 = (rc * h).astype(F32)
    rh16 = rh32.astype(np.float16)
    zrb, rh = preset(rows + GUARD, 512), preset(rows + GUARD, ld * 2)
    zrb[:rows, :256] = zc.astype(np.float16).view(np.uint8)
    if bug == "r_half_written":
        zrb[:rows, 256:] = rc.astype(np.float16).view(np.uint8)
    rh[:rows, :256] = rh16.view(np.uint8)
    if layout == R.MX2:
        rh[:rows, 768:896] = S.e4m3_bytes(rh32 if bug == "fp8_of_the_fp32_value" else rh16.astype(F32))
    return zrb, rh


def gru_q_restated(d, layout, bug=None):
    rows = d["h32"].shape[0]
    ld = 576 if layout == R.MX2 else 384
    q = np.tanh(gru_pre32(d, layout).astype(np.float64)).astype(F32)
    z, h = d["z"][:, :128], d["h32"]
    hn = (z * h + (1 - z) * q if bug == "z_blend_swapped" else (1 - z) * h + z * q).astype(F32)
    out, hraw = preset(rows + GUARD, ld * 2), preset(rows + GUARD, 512)
    hraw[:rows] = (h if bug == "h32_not_updated" else hn).view(np.uint8)
    o16 = hn.astype(np.float16)
    out[:rows, :256] = o16.view(np.uint8)
    if layout == R.MX2:
        out[:rows, 768:896] = S.e4m3_bytes(hn if bug == "fp8_of_the_fp32_value" else o16.astype(F32))
    return out, hraw


GRU_CPU = [(m, o) for m in R.GRU_MODES for o in ((1, 5), (5, 1))]


@pytest.fixture(scope="module")
def gru_inputs():
    return {(which, m[0], o): R.gru_data(len(m[0]) + o[0], which, *R.GRU_GRIDS[0], m[1], *o, m[2]) for which in ("zr", "q") for m, o in GRU_CPU}


@pytest.mark.parametrize("mode,orient", GRU_CPU, ids=["%s_%dx%d" % (m[0], *o) for m, o in GRU_CPU])
def test_gru_restatements_pass(gru_inputs, mode, orient):
    d = gru_inputs[("zr", mode[0], orient)]
    r = R.gru_zr_verify("zr", *gru_zr_restated(d, mode[3]), d, mode[3])
    assert max(r) <= 0.5, r
    d = gru_inputs[("q", mode[0], orient)]
    r = R.gru_q_verify("q", *gru_q_restated(d, mode[3]), d, mode[3])
    assert max(r) <= 0.5, r


@pytest.mark.parametrize("bug", ["z_r_swapped", "rh_from_fp16_h", "r_half_written", "fp8_of_the_fp32_value"])
def test_gru_zr_faults_are_seen(gru_inputs, bug):
    mode = R.GRU_MODES[1]
    d = gru_inputs[("zr", mode[0], (1, 5))]
    assert caught(lambda: R.gru_zr_verify("zr", *gru_zr_restated(d, mode[3], bug=bug), d, mode[3])), bug


@pytest.mark.parametrize("bug", ["z_blend_swapped", "h32_not_updated", "fp8_of_the_fp32_value"])
def test_gru_q_faults_are_seen(gru_inputs, bug):
    mode = R.GRU_MODES[1]
    d = gru_inputs[("q", mode[0], (5, 1))]
    assert caught(lambda: R.gru_q_verify("q", *gru_q_restated(d, mode[3], bug=bug), d, mode[3])), bug


def test_gru_data_saturates():
    d = R.gru_data(3, "zr", 9, 13, 384, 1, 5, False)
    v = S.conv_nhwc(d["x"], d["w"], 1) + d["b"]
    assert v.min() < -12 and v.max() > 12 and np.abs(d["h32"]).max() > 1


def pixshuf_conv_restated(x, wt, b, layout, relu, bug=None):
    B, h, w, Ci = x.shape
    pw = S.weight_pw(wt, True) if layout == R.MX3 else 0
    acc = np.zeros((B * h * w, 256), F32)
    for _, a, ww in S.operand_pairs(layout, x, wt, 0, pw, 1):
        a, ww = np.pad(a.astype(F32), ((0, 0), (1, 1), (1, 1), (0, 0))), ww.astype(F32)
        for ky in range(3):
            for kx in range(3):
                tap = a[:, ky:ky + h, kx:kx + w].reshape(-1, Ci)
                for c0 in range(0, Ci, 16):
                    acc = acc + tap[:, c0:c0 + 16] @ ww[:, c0:c0 + 16, ky, kx].T
    v = (acc + np.tile(b, 4)).astype(F32)
    if relu:
        v = np.maximum(v, 0)
    if bug == "dy_dx_swapped":
        v = v.reshape(-1, 2, 2, 64).transpose(0, 2, 1, 3).reshape(-1, 256)
    v = R.pixshuf_arrange(v, B, h, w, 64, 2)
    px = v.shape[0]
    raw = preset(px + GUARD, (1 if layout == R.F16 else 2) * 128)
    hi = v.astype(np.float16)
    raw[:px, :128] = hi.view(np.uint8)
    if layout == R.SPLIT16:
        raw[:px, 128:256] = (v - hi.astype(F32)).astype(np.float16).view(np.uint8)
    if layout == R.MX3:
        raw[:px, 128:192] = S.e4m3_bytes(hi.astype(F32))
        raw[:px, 192:256] = S.e4m3_bytes(np.ldexp(v - hi.astype(F32), 12))
    return raw


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("layout", list(HEAD_LAYOUTS))
def test_pixshuf_conv_restatement_passes(layout, relu):
    lay = HEAD_LAYOUTS[layout]
    x, wt, b = R.pixshuf_conv_data(21, *R.PIXSHUF_CONV_GRIDS[1])
    r = R.pixshuf_verify("stem", pixshuf_conv_restated(x, wt, b, lay, relu), x, wt, b, 2, lay, conv=True, relu=relu)
    assert max(r) <= 0.5, r
    assert caught(lambda: R.pixshuf_verify("stem", pixshuf_conv_restated(x, wt, b, lay, relu, bug="dy_dx_swapped"), x, wt, b, 2, lay, conv=True, relu=relu))
