"""Float64 references of the GEMM's fused epilogues (CPU only; a helper module of the tests, not a conftest): EPI_RESID, EPI_QKV and EPI_PATCH
of csrc/gemm_kernels.h as DepthEngine::vit launches them, EPI_PIXSHUF (dense) and EPI_HEAD as DepthEngine::head does, behind pb_op_gemm_resid /
_qkv / _patch / _pixshuf / _fc1 and pb_op_conv_head.

Per op: a seeded data builder, the float64 truth, and one *_verify(name, raw, ...) that decodes the op's raw buffer, holds every value to
two levels - the exact restatement of the layout's products (split_ref.restate) within the accumulation and storage bounds, and float64
truth within the layout's budget (split_ref.BUDGET) of sum |x||w| - and asserts that every byte the epilogue does not own is still the
0xFF it was preset to.  tests/test_epi_ref_cpu.py runs the verifiers on float32 restatements of the kernels, clean and with planted
faults; tests/test_gpu_epilogue_ops.py runs them on the kernels' buffers.

Tolerances on top of split_ref.tolerance (products accumulated in fp32), each from the number formats:
  fp32 stream outputs   2^-24 (|x| + |v|) per fp32 addition that touches the stream value.  EPI_RESID starts the accumulators from x + b'
                        and every MFMA adds onto them: 1 + n / 16 additions for n products (an fp16 MFMA sums 16 products per accumulator
                        update, an fp8 one 64), each rounding at most 2^-24 of |x| + |b'| + the products so far - the products' own share is
                        split_ref.tolerance's.  EPI_PATCH adds bias and pos-embed to a finished accumulator: 2 additions.
  LayerScale fold       w' = fl32(g w), b' = fl32(g b) on the host: 2^-24 of g (sum |a||w| + |b|) against the unfolded float64 truth.
  EPI_QKV               one fp16 rounding of (v + b) qscale: half an fp16 step of the value, granted in full (worst()); the float32 bias add
                        and scaling are split_ref.tolerance's 2^-22 (|b| + |v|).  The transposed V is held to the same untransposed formula
                        as K.
  EPI_PIXSHUF           split_ref.tolerance as tests/test_gpu_split_ops.py applies it to EPI_STD, the storage rounding granted in full.
  fc1 (GELU + fp8)      twice the measured absolute error of fast_gelu2 (GELU_ABS_MEASURED), the pre-activation's bound times the GELU's largest
                        slope; the e4m3 copy is compared byte for byte with e4m3(stored fp16 x scale).
  EPI_HEAD              33 float32 roundings of the dot product's magnitudes (depth_ref.dot_verify) on top of the 32 activations' own bounds.
"""
from __future__ import annotations

import numpy as np

import split_ref as S
from raft_ref import f16_step

F16, SPLIT16, MX2 = S.F16, S.SPLIT16, S.MX2
U24 = 2.0 ** -24
QSCALE = np.float32(0.125) * np.float32(1.4426950408889634)        # common.h PB_QSCALE: softmax scale 1 / 8 times log2(e)
T_128, T_256 = 1, 2
KERNEL = {"128": "gemm_kernel<128, 128, 2, 2, 0, %d,", "wide": "gemm8_kernel<0, %d,"}


def kernel_prefix(tile: str, epi: int) -> str:
    return KERNEL[tile] % epi


def untouched(name: str, raw: np.ndarray, owned: np.ndarray):
    """every byte outside `owned` (bool, raw's shape) is still 0xFF"""
    bad = ~owned & (raw != 0xFF)
    assert not bad.any(), f"{name}: bytes the epilogue does not own were written, first at {np.argwhere(bad)[:8].tolist()}"


def worst(name: str, what: str, err: np.ndarray, tol: np.ndarray, rounding=0.0) -> float:
    """asserts err <= rounding + tol element by element; returns the worst (err - rounding) / tol.  `rounding` is the half step of an output
    stored as fp16: a correct kernel reaches it on every near-tie, so it is granted in full and the ratio measures what is left"""
    r = np.maximum(err - rounding, 0) / tol
    i = np.unravel_index(np.nanargmax(r), r.shape)
    assert np.isfinite(err).all() and r[i] <= 1, f"{name}: {what} {r[i]:.2f} x tolerance at element {tuple(int(x) for x in i)}"
    return float(r[i])


def one_signed(w) -> np.ndarray:
    """weights whose fp16 rounding residuals all have one sign (0.4 of an fp16 step above w_hi, tests/raft_ref.py flow_head2_data): on
    non-negative activations the w_lo products add up, and a kernel that drops the weight-residual segment loses ~2^-12 of sum |x||w|"""
    h = S.f16(w)
    return (h.astype(np.float64) + 0.4 * f16_step(h)).astype(np.float32)


# =====================================================================================================================
# EPI_RESID: X += A (g W)^T + g b
# =====================================================================================================================
def resid_data(seed: int, M: int, N: int, K: int, signed: bool = False):
    """A [M, K], w [N, K], bias, gamma in [0.05, 2], X [M, N] with one all-zero row.  signed: non-negative activations, one-signed weight
    residuals and power-of-two gammas (the fold keeps the residuals' sign).

    The weights are N(0, 1/2) against activations of N(0, 1/K): a split16 weight keeps its residual as fp16, whose subnormal step of 2^-24
    is 2^-20 of a FOLDED weight g w of 2^-4 - with weights of N(0, 1/K) and g = 0.05 the float32 restatement itself sat at 0.7 of the
    split16 budget (the mx2 residual carries its own power-of-two scale and does not care)."""
    g = np.random.default_rng(seed)
    A, w, b = S.case_data(seed, (M, K), (N, K), x_scale=K ** -0.5, w_scale=0.5)
    gamma = g.uniform(0.05, 2.0, N).astype(np.float32)
    if signed:
        A = np.abs(A)
        w = one_signed(w)
        gamma = np.ldexp(1.0, g.integers(-2, 2, N)).astype(np.float32)
    X = (g.standard_normal((M, N)) * 2).astype(np.float32)
    X[M // 3] = 0
    return A, w, b, gamma, X


def fold(w, b, gamma):
    """pack_layout.h pb_fold_layerscale: fp32 products"""
    gamma = np.asarray(gamma, np.float32)
    return (np.asarray(w, np.float32) * gamma[:, None]).astype(np.float32), (np.asarray(b, np.float32) * gamma).astype(np.float32)


def resid_truth(A, w, b, gamma, X, layout: int):
    """(X + g (A W^T + b), g sum |a||w|) in float64 from the UNFOLDED weights"""
    t, tmag = S.truth(layout, A, w, conv=False, sa=0)
    g = np.asarray(gamma, np.float64)
    return np.asarray(X, np.float64) + g * (t + np.asarray(b, np.float64)), np.abs(g) * tmag


def resid_expected(A, w, b, gamma, X, layout: int, pa: int = 0, pw=None):
    """(restated value, tolerance of kernel vs restatement, pw) of the folded layer"""
    wf, bf = fold(w, b, gamma)
    if pw is None:
        pw = S.weight_pw(wf, False) if layout == MX2 else 0
    acc, mag = S.restate(layout, A, wf, pa, pw, sa=0, conv=False)
    x64 = np.asarray(X, np.float64)
    v = x64 + bf.astype(np.float64) + acc
    n = S.n_products(layout, A.shape[1], 0)
    tol = S.tolerance(mag, 0.0, n, False) + (1 + n / 16) * U24 * (np.abs(x64) + np.abs(bf.astype(np.float64)) + np.abs(v))
    return v, tol, pw


def resid_reference(A, w, b, gamma, X, layout: int, pa: int = 0, pw=None):
    """(restated value, its tolerance, float64 truth, its limit): computed once per case and shared by the runs that verify against it"""
    v, tol, _ = resid_expected(A, w, b, gamma, X, layout, pa, pw)
    t, tmag = resid_truth(A, w, b, gamma, X, layout)
    g = np.abs(np.asarray(gamma, np.float64))
    return v, tol, t, S.BUDGET[layout] * tmag + tol + U24 * (tmag + g * np.abs(np.asarray(b, np.float64)))


def resid_verify(name: str, raw: np.ndarray, A, w, b, gamma, X, layout: int, pa: int = 0, pw=None, ref=None):
    """raw: uint8 [M + guard, ldr * 4].  Returns (kernel vs restatement / tolerance, kernel vs float64 / limit)"""
    M, N = X.shape
    owned = np.zeros(raw.shape, bool)
    owned[:M, :4 * N] = True
    untouched(name, raw, owned)
    val = raw[:M, :4 * N].copy().view(np.float32).astype(np.float64)
    v, tol, t, lim = ref if ref is not None else resid_reference(A, w, b, gamma, X, layout, pa, pw)
    r1 = worst(name, "kernel vs restatement", np.abs(val - v), tol)
    r2 = worst(name, "kernel vs float64", np.abs(val - t), lim)
    return r1, r2


# (M, N, K): the 128 x 128 tile's shapes; the wide tile's one-workgroup-per-tile shapes; the split-K shape
RESID_128 = [(144, 128, 128), (300, 384, 256), (517, 256, 1024)]
RESID_WIDE = [(300, 256, 128), (513, 384, 128)]
RESID_SPLITK = (300, 384, 1536)


def resid_persistent_shape(cu: int):
    """more 256 x 256 tiles than the chip has CUs, the last row tile and the second column tile partial"""
    return 256 * -(-(cu + 4) // 2) - 199, 384, 128


# =====================================================================================================================
# EPI_QKV: Q (x qscale), K -> [b, head, t, 64]; V -> [b, head, 64, ntp]
# =====================================================================================================================
QKV_CASES = [("D128_B3_ntp48", T_128, 128, 3, 48), ("D384_B2_ntp272", T_128, 384, 2, 272),
             ("D256_B2_ntp272", T_256, 256, 2, 272), ("D512_B1_ntp304", T_256, 512, 1, 304)]


def qkv_data(seed: int, D: int, B: int, ntp: int, signed: bool = False):
    A, w, b = S.case_data(seed, (B * ntp, D), (3 * D, D))
    b = (b * 5).astype(np.float32)
    if signed:
        A, w = np.abs(A), one_signed(w)
    return A, w, b


def qkv_decode(q, k, vt, B: int, ntp: int, D: int):
    """raw q, k [B heads ntp + guard, 128] / vt [B heads 64 + guard, ntp * 2] bytes -> [B ntp, 3 D] float64 in the GEMM's column order"""
    heads = D // 64
    out = []
    for raw in (q, k):
        h = raw[:B * heads * ntp].copy().view(np.float16).reshape(B, heads, ntp, 64)
        out.append(h.transpose(0, 2, 1, 3).reshape(B * ntp, D))
    h = vt[:B * heads * 64].copy().view(np.float16).reshape(B, heads, 64, ntp)
    out.append(h.transpose(0, 3, 1, 2).reshape(B * ntp, D))
    return np.concatenate(out, axis=1).astype(np.float64)


def qkv_scale(D: int) -> np.ndarray:
    s = np.ones(3 * D)
    s[:D] = float(QSCALE)
    return s


def qkv_verify(name: str, q, k, vt, A, w, b, B: int, ntp: int, layout: int, pa: int = 0, pw=None):
    D = A.shape[1]
    heads = D // 64
    for what, raw, rows in (("q", q, B * heads * ntp), ("k", k, B * heads * ntp), ("vt", vt, B * heads * 64)):
        owned = np.zeros(raw.shape, bool)
        owned[:rows] = True
        untouched(f"{name} {what}", raw, owned)
    val = qkv_decode(q, k, vt, B, ntp, D)
    if pw is None:
        pw = S.weight_pw(w, False) if layout == MX2 else 0
    s = qkv_scale(D)
    acc, mag = S.restate(layout, A, w, pa, pw, sa=0, conv=False)
    v = (acc + np.asarray(b, np.float64)) * s
    n = S.n_products(layout, D, 0)
    # split_ref.tolerance's accumulation part on the scaled sums; its fp16 storage part is replaced by the exact half step of the stored value
    tol = S.tolerance(mag * s, 0.0, n, False) + 2.0 ** -22 * (np.abs(np.asarray(b, np.float64)) * s + np.abs(v))
    half = 0.5 * f16_step(v)
    r1 = worst(name, "kernel vs restatement", np.abs(val - v), tol, half)
    t, tmag = S.truth(layout, A, w, conv=False, sa=0)
    r2 = worst(name, "kernel vs float64", np.abs(val - (t + np.asarray(b, np.float64)) * s), S.BUDGET[layout] * tmag * s + tol, half)
    return r1, r2


# =====================================================================================================================
# EPI_PATCH: rows (b, patch) -> resid[b ntp + 1 + patch] = v + bias + pos[1 + patch]
# =====================================================================================================================
PATCH_CASES = [("D128", 128, 2, 77, 80), ("D384", 384, 3, 130, 144)]
PATCH_K = 588


def patch_data(seed: int, D: int, B: int, P: int, signed: bool = False):
    A, w, b = S.case_data(seed, (B * P, PATCH_K), (D, PATCH_K))
    if signed:
        A, w = np.abs(A), one_signed(w)
    pos = (np.random.default_rng(seed + 1).standard_normal((1 + P, D)) * 0.5).astype(np.float32)
    return A, w, b, pos


def patch_verify(name: str, raw: np.ndarray, A, w, b, pos, B: int, ntp: int, layout: int):
    """raw: uint8 [B ntp + guard, D * 4]: the class row, the pad rows behind the patches and the guard rows stay preset"""
    D = w.shape[0]
    P = A.shape[0] // B
    rows = (np.arange(B)[:, None] * ntp + 1 + np.arange(P)[None, :]).reshape(-1)
    owned = np.zeros(raw.shape, bool)
    owned[rows] = True
    untouched(name, raw, owned)
    val = raw[rows].copy().view(np.float32).astype(np.float64)
    acc, mag = S.restate(layout, A, w, 0, 0, sa=0, conv=False)
    pe = np.tile(np.asarray(pos, np.float64)[1:], (B, 1))
    b64 = np.asarray(b, np.float64)
    v = acc + b64 + pe
    n = S.n_products(layout, 640, 0)
    tol = S.tolerance(mag, 0.0, n, False) + 2 * U24 * (np.abs(acc) + np.abs(b64) + np.abs(pe) + np.abs(v))
    r1 = worst(name, "kernel vs restatement", np.abs(val - v), tol)
    t, tmag = S.truth(layout, A, w, conv=False, sa=0)
    r2 = worst(name, "kernel vs float64", np.abs(val - (t + b64 + pe)), S.BUDGET[layout] * tmag + tol)
    return r1, r2


# =====================================================================================================================
# EPI_HEAD: depth[m] = relu(sum_n relu(conv3x3 + bias)[n] w2[n] + b2), N = 32
# =====================================================================================================================
MX3 = S.MX3
HEAD_MAPS = [(1, 7, 9), (2, 13, 21), (1, 17, 16)]
HEAD_CASES = [(m, C, lay) for m in HEAD_MAPS for C in (64, 128) for lay in ("f16", "split16", "mx3")]
HEAD_KERNEL = "gemm_kernel<256, 32, 4, 1, 1, 5,"


def head_data(seed: int, B: int, H: int, W: int, C: int):
    """x NHWC, w [32, C, 3, 3], bias, w2 of both signs, and b2 placed so that a third of the pixels clamp at 0"""
    x, w, b = S.case_data(seed, (B, H, W, C), (32, C, 3, 3))
    w2 = (np.random.default_rng(seed + 1).standard_normal(32) / 4).astype(np.float32)
    s = np.maximum(S.conv_nhwc(x, w, 1) + b.astype(np.float64), 0) @ w2.astype(np.float64)
    return x, w, b, w2, float(np.float32(-np.quantile(s, 1 / 3)))


def head_verify(name: str, raw: np.ndarray, x, w, b, w2, b2: float, layout: int, pa: int = 0, pw=None):
    """raw: float32 [B H W + guard].  The 32 activations carry split_ref.tolerance's accumulation bound and the float32 bias add; the dot
    product adds 33 float32 roundings of the magnitudes (depth_ref.dot_verify); ReLU does not grow an error"""
    M = int(np.prod(x.shape[:3]))
    bytes_ = raw.view(np.uint8)
    owned = np.zeros(bytes_.shape, bool)
    owned[:4 * M] = True
    untouched(name, bytes_, owned)
    val = raw[:M].astype(np.float64)
    if pw is None:
        pw = S.weight_pw(w, True) if layout == MX3 else 0
    b64, w64 = np.asarray(b, np.float64), np.asarray(w2, np.float64)
    acc, mag = S.restate(layout, x, w, pa, pw, sa=1, conv=True, stride=1)
    act = np.maximum(acc + b64, 0)
    n = S.n_products(layout, 9 * x.shape[3], 1)
    tol_act = S.tolerance(mag, 0.0, n, False) + U24 * (np.abs(acc) + np.abs(b64))
    v = np.maximum(act @ w64 + np.float64(np.float32(b2)), 0)
    tol = tol_act @ np.abs(w64) + 33 * U24 * (act @ np.abs(w64) + abs(b2)) + 2.0 ** -149
    r1 = worst(name, "kernel vs restatement", np.abs(val - v), tol)
    t, tmag = S.truth(layout, x, w, conv=True, stride=1, sa=1)
    tv = np.maximum(np.maximum(t + b64, 0) @ w64 + np.float64(np.float32(b2)), 0)
    r2 = worst(name, "kernel vs float64", np.abs(val - tv), S.BUDGET[layout] * (tmag @ np.abs(w64)) + tol)
    return r1, r2


# =====================================================================================================================
# EPI_PIXSHUF (dense): row (b, y, x), column (dy, dx, co) -> pixel (b, y s + dy, x s + dx), channel co
# =====================================================================================================================
# (name, s, C): the buffer-addressed / flat store paths (C % 64 == 0; the grid's width decides) and the LDS path (C % 64 != 0)
PIXSHUF_CASES = [("s4_c256", 4, 256), ("s2_c512", 2, 512), ("s4_c96", 4, 96)]
PIXSHUF_GRIDS = [(19, 33), (5, 7)]
PIXSHUF_B = 2
PIXSHUF_CONV_GRIDS = [(23, 46), (9, 11)]          # the stem's form: 64 -> 4 x 64, s = 2; 46 columns take the buffer-addressed stores, 11 the flat ones


def pixshuf_conv_data(seed: int, h: int, w: int):
    x, wt, _ = S.case_data(seed, (PIXSHUF_B, h, w, 64), (256, 64, 3, 3))
    return x, wt, (np.random.default_rng(seed + 1).standard_normal(64) * 0.3).astype(np.float32)


def pixshuf_data(seed: int, h: int, w: int, C: int, s: int):
    g = np.random.default_rng(seed)
    x = g.standard_normal((PIXSHUF_B, h, w, C)).astype(np.float32)
    wt = (g.standard_normal((C, C, s, s)) * C ** -0.5).astype(np.float32)
    return x, wt, (g.standard_normal(C) * 0.1).astype(np.float32)


def pixshuf_rows(wt, s: int) -> np.ndarray:
    """ConvTranspose2d weight [ci, co, dy, dx] -> GEMM rows n = (dy s + dx) C + co, k = ci (DepthEngine::load pack_convT)"""
    C = wt.shape[0]
    return np.ascontiguousarray(np.asarray(wt, np.float32).transpose(2, 3, 1, 0).reshape(s * s * C, C))


def pixshuf_arrange(v, B: int, h: int, w: int, C: int, s: int):
    """[B h w, s s C] in the GEMM's order -> [B (h s) (w s), C] in the output's"""
    return v.reshape(B, h, w, s, s, C).transpose(0, 1, 3, 2, 4, 5).reshape(B * h * s * w * s, C)


def pixshuf_verify(name: str, raw: np.ndarray, x, wt, b, s: int, layout: int, pa: int = 0, pw=None, conv: bool = False, relu: bool = False):
    """raw: uint8 [B h s w s + guard, ldo * 2] in the head's map layout ([hi], [hi | lo] or [hi | hi8 | lo8]).  The storage rounding of the
    output's format (half an fp16 step; split_ref.tolerance's 2^-15 |v| of a split output) is granted in full (worst()).  conv: wt is a
    convolution weight [s s C, Ci, 3, 3] whose output channel is (dy s + dx) C + co (RAFT's stem), x [B, h, w, Ci]"""
    B, h, w, Ci = x.shape
    C = wt.shape[0] // (s * s) if conv else Ci
    px = B * h * s * w * s
    split_out = layout != F16
    info = dict(M=px, ldo=raw.shape[1] // 2, lo8=layout == MX3, lo8_pa=pa)
    untouched(name, raw, S.written_mask(raw, info, C, split_out))
    val, hi, lo, lo8, hi8 = S.decode_output(raw, info, C, split_out)
    g = np.asarray(wt, np.float32) if conv else pixshuf_rows(wt, s)
    if pw is None:
        pw = S.weight_pw(g, True) if layout == MX3 else 0
    x2 = np.asarray(x, np.float32) if conv else np.asarray(x, np.float32).reshape(-1, Ci)
    arr = lambda v: pixshuf_arrange(v, B, h, w, C, s)
    acc, mag = S.restate(layout, x2, g, pa, pw, sa=1, conv=conv, stride=1)
    bias = np.tile(np.asarray(b, np.float64), s * s)
    act = (lambda v: np.maximum(v, 0)) if relu else (lambda v: v)
    v, mag = arr(act(acc + bias)), arr(mag)
    n = S.n_products(layout, int(np.prod(g.shape[1:])), 1)
    tol = S.tolerance(mag, 0.0, n, False) + 2.0 ** -22 * (np.abs(np.asarray(b, np.float64)) + np.abs(v))
    store = S.tolerance(0.0, v, 0, True) - 2.0 ** -22 * np.abs(v) if split_out else 0.5 * f16_step(v)
    r1 = worst(name, "kernel vs restatement", np.abs(val - v), tol, store)
    t, tmag = S.truth(layout, x2, g, conv=conv, stride=1, sa=1)
    r2 = worst(name, "kernel vs float64", np.abs(val - arr(act(t + bias))), S.BUDGET[layout] * arr(tmag) + tol, store)
    if split_out:
        assert (np.abs(hi - v) <= np.abs(v) * 2.0 ** -10 + 2.0 ** -24 + tol).all(), f"{name}: hi is not fp16(v)"
    if lo8 is not None:                                     # (tests/test_gpu_split_ops.py check (3b))
        assert np.array_equal(hi8, S.e4m3_bytes(np.ldexp(hi.astype(np.float32), pa))), f"{name}: hi8 != e4m3(hi 2^pa)"
        r = np.ldexp(v - hi, pa + 12)
        assert (np.abs(np.ldexp(lo, pa + 12) - r) <= S.e4m3_step(r) + np.ldexp(tol, pa + 12)).all(), f"{name}: lo8 off by more than one e4m3 step"
    return r1, r2


# =====================================================================================================================
# fc1 as the split ViT runs it: EPI_STD on the MX build with an all-fp16 K axis (nk16 = K / 64), GELU, an e4m3 copy of the stored fp16
# =====================================================================================================================
# fast_gelu2 (gemm_kernels.h: a degree-5 fit of log2 Q(|x|), one exp2) against the float64 erf form: tools/probe/gelu_probe.hip measures it
# on [-8, 8] (nothing to do with the GEMM under test); the constant allows twice the figure.
# measured on an MI355X, 4 194 304 points: max absolute error 6.3915e-7 = 2^-20.58 (at x = 4.0003); relative to |gelu| it reaches 3.9e-2 in the
# negative tail (x = -5.08, gelu = -5e-7), so the allowance is absolute
GELU_ABS_MEASURED = 6.3915e-7
FC1_CASES = [(300, 128, 512, T_128), (517, 384, 1536, T_128), (517, 384, 1536, T_256)]
FC1_KERNEL = {T_128: "gemm_kernel<128, 128, 2, 2, 0, 0,", T_256: "gemm8_kernel<0, 0,"}
GELU_SLOPE = 1.13                                          # max |d gelu / dx| (1.1290 at x = 1.41)


def gelu64(v):
    import torch
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1 + torch.erf(torch.from_numpy(v / np.sqrt(2.0))).numpy())


def fc1_data(seed: int, M: int, K: int, N: int):
    """pre-activations of N(0, ~3): both tails of the GELU and its minimum are hit"""
    return S.case_data(seed, (M, K), (N, K), w_scale=3 * K ** -0.5)


def fc1_verify(name: str, raw: np.ndarray, A, w, b, o8_scale: float = 1.0):
    """raw: uint8 [M + guard, 3 N]: N halfs of gelu(A w^T + b), then N e4m3 bytes of the stored fp16 times o8_scale (compared exactly)"""
    M, N = A.shape[0], w.shape[0]
    owned = np.zeros(raw.shape, bool)
    owned[:M] = True
    untouched(name, raw, owned)
    h = raw[:M, :2 * N].copy().view(np.float16)
    assert np.array_equal(raw[:M, 2 * N:], S.e4m3_bytes(h.astype(np.float32) * np.float32(o8_scale))), f"{name}: the fp8 copy is not e4m3(stored fp16 x scale)"
    val = h.astype(np.float64)
    b64 = np.asarray(b, np.float64)
    acc, mag = S.restate(F16, A, w, 0, 0, sa=0, conv=False)
    v = gelu64(acc + b64)
    n = S.n_products(F16, A.shape[1], 0)
    tol = GELU_SLOPE * (S.tolerance(mag, 0.0, n, False) + 2.0 ** -22 * (np.abs(b64) + np.abs(acc + b64))) + 2 * GELU_ABS_MEASURED
    half = 0.5 * f16_step(v)
    r1 = worst(name, "kernel vs restatement", np.abs(val - v), tol, half)
    t, tmag = S.truth(F16, A, w, conv=False, sa=0)
    r2 = worst(name, "kernel vs float64", np.abs(val - gelu64(t + b64)), GELU_SLOPE * S.BUDGET[F16] * tmag + tol, half)
    return r1, r2


# =====================================================================================================================
# ACT_GRU_ZR / ACT_GRU_Q (SepConvGRU, RAFT update.py:55-76) through EngineBase::conv
# =====================================================================================================================
# sigmoid as __frcp_rn(1 + __expf(-v)) and fast_tanh: the project's allowance of 2^-20 absolute (tests/test_gpu_split_ops.py check)
ACT_ABS = 2.0 ** -20
GRU_GRIDS = [(9, 13), (17, 23)]
GRU_N = 2
# (name, gc, hoisted add1 / add2, layout)
GRU_MODES = [("gc384_f16", 384, False, F16), ("gc384_mx2", 384, False, MX2), ("gc256_hoist_f16", 256, True, F16), ("gc256_hoist_mx2", 256, True, MX2)]
GRU_KERNEL = {T_128: "gemm_kernel<128, 128, 2, 2, 1, 0,", T_256: "gemm8_kernel<1, 0,"}


def gru_data(seed: int, which: str, h8: int, w8: int, gc: int, kh: int, kw: int, hoist: bool):
    """x [n, h8, w8, 384] fp16-representable with its first 128 channels = fp16(h) for "zr"; weights scaled so that the pre-activations cover
    [-12, 12] (both saturations of sigmoid and tanh); h32 up to about +-1; z in [0, 1] as fp16; the hoisted terms as fp16"""
    g = np.random.default_rng(seed)
    N = 256 if which == "zr" else 128
    rows = GRU_N * h8 * w8
    h32 = np.clip(g.standard_normal((rows, 128)) * 0.45, -1.2, 1.2).astype(np.float32)
    x = S.f16(g.standard_normal((GRU_N, h8, w8, 384)) * 0.7)
    if which == "zr":
        x.reshape(rows, 384)[:, :128] = S.f16(h32)
    fan = gc * kh * kw
    w = (g.standard_normal((N, gc, kh, kw)) * 6 * fan ** -0.5).astype(np.float32)
    b = g.standard_normal(N).astype(np.float32)
    add1 = S.f16(g.standard_normal((rows, N))) if hoist else None
    add2 = S.f16(g.standard_normal((rows, N)) * 0.5) if hoist else None
    z = S.f16(g.uniform(0, 1, (rows, 256)))
    z[:, :8] = (0.0, 1.0) * 4                                # exact 0 and 1: h kept / replaced
    return dict(x=x, w=w, b=b, h32=h32, add1=add1, add2=add2, z=z)


def _gru_pre(d, layout: int, pa: int, pw):
    """(restated pre-activation, its tolerance, float64 truth, budget x magnitude)"""
    w = d["w"]
    gc = w.shape[1]
    xs = d["x"][..., :gc]
    if pw is None:
        pw = S.weight_pw(w, False) if layout == MX2 else 0
    acc, mag = S.restate(layout, xs, w, pa, pw, sa=0, conv=True, stride=1)
    sk = 0.0 if d["add1"] is None else d["add1"].astype(np.float64) + d["add2"].astype(np.float64)
    b64 = d["b"].astype(np.float64)
    v = acc + b64 + sk
    n = S.n_products(layout, gc * w.shape[2] * w.shape[3], 0)
    tol = S.tolerance(mag, 0.0, n, False) + 2.0 ** -22 * (np.abs(b64) + np.abs(sk) + np.abs(v))
    t, tmag = S.truth(layout, xs, w, conv=True, stride=1, sa=0)
    return v, tol, t + b64 + sk, S.BUDGET[layout] * tmag


def _sig(v):
    return 1 / (1 + np.exp(-v))


def gru_zr_verify(name: str, zrb: np.ndarray, rh: np.ndarray, d, layout: int, pa: int = 0, pw=None):
    """zrb uint8 [rows + guard, 512]: z in halfs [0, 128), the r half untouched; rh uint8 [rows + guard, ld * 2]: fp16(r h32) in halfs [0, 128)
    and, mx2, its e4m3 twin at bytes [768, 896); everything else untouched"""
    rows = d["h32"].shape[0]
    owned = np.zeros(zrb.shape, bool)
    owned[:rows, :256] = True
    untouched(name + " zrb", zrb, owned)
    owned = np.zeros(rh.shape, bool)
    owned[:rows, :256] = True
    if layout == MX2:
        owned[:rows, 768:896] = True
    untouched(name + " rh", rh, owned)
    zv = zrb[:rows, :256].copy().view(np.float16)
    rv = rh[:rows, :256].copy().view(np.float16)
    if layout == MX2:
        assert np.array_equal(rh[:rows, 768:896], S.e4m3_bytes(rv.astype(np.float32))), f"{name}: the fp8 twin of r h is not e4m3(stored fp16)"
    v, tol, t, bud = _gru_pre(d, layout, pa, pw)
    h = d["h32"].astype(np.float64)
    ref = np.concatenate([_sig(v[:, :128]), _sig(v[:, 128:]) * h], axis=1)
    tref = np.concatenate([_sig(t[:, :128]), _sig(t[:, 128:]) * h], axis=1)
    scale = np.concatenate([np.ones_like(h), np.abs(h)], axis=1)
    tl = scale * (tol / 4 + ACT_ABS) + U24 * np.abs(ref)          # sigmoid's slope is at most 1 / 4; r h: one more float32 rounding
    val = np.concatenate([zv, rv], axis=1).astype(np.float64)
    half = 0.5 * f16_step(ref)
    r1 = worst(name, "kernel vs restatement", np.abs(val - ref), tl, half)
    r2 = worst(name, "kernel vs float64", np.abs(val - tref), scale * bud / 4 + tl, half)
    return r1, r2


def gru_q_verify(name: str, out: np.ndarray, h32raw: np.ndarray, d, layout: int, pa: int = 0, pw=None):
    """out uint8 [rows + guard, ld * 2]: fp16(new h) in halfs [0, 128) (and, mx2, its e4m3 twin at bytes [768, 896)); h32raw uint8
    [rows + guard, 512]: the updated fp32 state.  tolerance: z (tol_v + 2^-20) + 2^-23 (|h| + |q|), z as the fp16 the kernel reads"""
    rows = d["h32"].shape[0]
    owned = np.zeros(out.shape, bool)
    owned[:rows, :256] = True
    if layout == MX2:
        owned[:rows, 768:896] = True
    untouched(name + " out", out, owned)
    owned = np.zeros(h32raw.shape, bool)
    owned[:rows] = True
    untouched(name + " h32", h32raw, owned)
    hn = h32raw[:rows].copy().view(np.float32)
    ov = out[:rows, :256].copy().view(np.float16)
    assert np.array_equal(ov, hn.astype(np.float16)), f"{name}: the fp16 copy is not fp16(h32)"
    if layout == MX2:
        assert np.array_equal(out[:rows, 768:896], S.e4m3_bytes(ov.astype(np.float32))), f"{name}: the fp8 twin is not e4m3(stored fp16)"
    v, tol, t, bud = _gru_pre(d, layout, pa, pw)
    h, z = d["h32"].astype(np.float64), d["z"][:, :128].astype(np.float64)
    q = np.tanh(v)
    ref = (1 - z) * h + z * q
    tl = z * (tol + ACT_ABS) + 2.0 ** -23 * (np.abs(h) + np.abs(q)) + 2.0 ** -149
    r1 = worst(name, "kernel vs restatement", np.abs(hn.astype(np.float64) - ref), tl)
    r2 = worst(name, "kernel vs float64", np.abs(hn.astype(np.float64) - ((1 - z) * h + z * np.tanh(t))), z * bud + tl)
    return r1, r2
