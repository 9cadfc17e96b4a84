"""Exact restatement of the split-precision GEMM / convolution layouts (CPU only; a helper module of the tests, not a conftest).

From fp32 operands and a layout this builds the operands the kernels actually multiply - the fp16 hi / lo parts, the e4m3 copies with
EngineBase::pack's power-of-two weight scale and the maps' activation scale - and sums exactly that set of products in float64:

  f16       a_hi w_hi
  split16   a_hi w_hi + a_lo w_hi + a_hi w_lo        (sa = 1: the map is [hi | lo]; sa = 0: [hi], the a_lo w_hi segment is absent)
  mx3       a_hi w_hi + a_hi8 w_lo8 + a_lo8 w_hi8    (maps [hi | hi8 | lo8], weights [w_hi | w_lo8 | w_hi8] per tap)
  mx2       a16 w_hi + a8 w_lo8                      (maps [a16 | a8]: the activation is its fp16 value, a8 = e4m3(a16 2^pa))

with hi = fp16(x), lo = fp16(x - hi), hi8 = e4m3(hi 2^pa) 2^-pa, lo8 = e4m3((x - hi) 2^(pa + 12)) 2^-(pa + 12) (gemm_kernels.h lo8_store2),
w_lo8 = e4m3((w - w_hi) 2^pw) 2^-pw, w_hi8 = e4m3(w_hi 2^(pw - 12)) 2^(12 - pw).  e4m3 is OCP e4m3fn with round to nearest even, clamped to
+-448 first as the device encoder (common.h pb_fp8x2) and the host one (pb_f32_to_e4m3) do: torch's own cast of 465 gives 0x7F, a NaN.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

F16, SPLIT16, MX3, MX2 = 0, 1, 2, 3
LAYOUTS = {"f16": F16, "split16": SPLIT16, "mx3": MX3, "mx2": MX2}
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 3, 4


def f16(x) -> np.ndarray:
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def e4m3_bytes(x) -> np.ndarray:
    t = torch.from_numpy(np.clip(np.asarray(x, np.float32), -448.0, 448.0))
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def e4m3_decode(b) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(b, np.uint8)).view(torch.float8_e4m3fn).to(torch.float64).numpy()


def e4m3_q(x, p: int) -> np.ndarray:
    """the value an e4m3 copy stored with scale 2^p decodes to (float64)"""
    return np.ldexp(e4m3_decode(e4m3_bytes(np.ldexp(np.asarray(x, np.float32), p))), -p)


def e4m3_step(v) -> np.ndarray:
    """spacing of e4m3 values at |v| (subnormal spacing 2^-9 below 2^-6)"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))
    return np.ldexp(1.0, (e - 3).astype(int))


def _exp(v: float) -> int:
    return int(np.frexp(np.float32(v))[1])


def weight_pw(w, mx3: bool) -> int:
    """EngineBase::pack: pw = 8 - e(max |w - fp16(w)|), for mx3 capped by 20 - e(max |w|) (frexp exponents)"""
    w = np.asarray(w, np.float32)
    mlo = float(np.abs(w - f16(w)).max()) if w.size else 0.0
    mhi = float(np.abs(w).max()) if w.size else 0.0
    pw = 8 - _exp(mlo) if mlo > 0 else 0
    if mx3 and mhi > 0:
        pw = min(pw, 20 - _exp(mhi))
    return pw


def operand_pairs(layout: int, x, w, pa: int, pw: int, sa: int = 1):
    """[(name, A part, W part)] in float64, the segments of the layout's K axis"""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    a_hi, w_hi = f16(x), f16(w)
    a_r, w_r = x - a_hi, w - w_hi                       # exact in fp32
    d = np.float64
    if layout == F16:
        return [("hi.hi", a_hi.astype(d), w_hi.astype(d))]
    if layout == SPLIT16:
        segs = [("hi.hi", a_hi.astype(d), w_hi.astype(d))]
        if sa:
            segs.append(("lo.hi", f16(a_r).astype(d), w_hi.astype(d)))
        segs.append(("hi.lo", a_hi.astype(d), f16(w_r).astype(d)))
        return segs
    if layout == MX3:
        return [("hi.hi", a_hi.astype(d), w_hi.astype(d)),
                ("hi8.lo8", e4m3_q(a_hi, pa), e4m3_q(w_r, pw)),
                ("lo8.hi8", e4m3_q(a_r, pa + 12), e4m3_q(w_hi, pw - 12))]
    if layout == MX2:
        return [("hi.hi", a_hi.astype(d), w_hi.astype(d)),
                ("a8.lo8", e4m3_q(a_hi, pa), e4m3_q(w_r, pw))]
    raise ValueError(layout)


def truth_input(layout: int, x, sa: int = 1) -> np.ndarray:
    """the activation the float64 truth multiplies: mx2 maps and split16 maps without a lo part (sa = 0) carry only its fp16 value"""
    return (f16(x) if layout == MX2 or (layout == SPLIT16 and not sa) else np.asarray(x, np.float32)).astype(np.float64)


def conv_nhwc(x, w, stride: int) -> np.ndarray:
    """float64 convolution, x NHWC [B, H, W, C], w [Co, C, kh, kw], zero padding (kh // 2, kw // 2) -> rows (b, oy, ox) x Co"""
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w, np.float64))
    y = F.conv2d(xt, wt, stride=stride, padding=(wt.shape[2] // 2, wt.shape[3] // 2))
    return y.permute(0, 2, 3, 1).reshape(-1, wt.shape[0]).numpy()


def dense(x, w) -> np.ndarray:
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64).T


def _mm(conv: bool, stride: int):
    return (lambda a, b: conv_nhwc(a, b, stride)) if conv else dense


def skip_value(s, split_out: bool, lo8: bool, lo8_pa: int = 0) -> np.ndarray:
    """the skip tensor as the epilogue reads it: hi, hi + lo (fp16) or hi + lo8"""
    s = np.asarray(s, np.float32)
    hi = f16(s)
    v = hi.astype(np.float64)
    if split_out and lo8:
        v = v + e4m3_q(s - hi, lo8_pa + 12)
    elif split_out:
        v = v + f16(s - hi).astype(np.float64)
    return v


def epilogue(acc, bias, skip=None, pre_relu: bool = False, act: int = ACT_NONE) -> np.ndarray:
    v = acc + np.asarray(bias, np.float64)
    if pre_relu:
        v = np.maximum(v, 0)
    if skip is not None:
        v = v + skip
    if act == ACT_RELU:
        v = np.maximum(v, 0)
    elif act == ACT_SIGMOID:
        v = 1 / (1 + np.exp(-v))
    elif act == ACT_TANH:
        v = np.tanh(v)
    return v


def restate(layout: int, x, w, pa: int, pw: int, sa: int = 1, conv: bool = True, stride: int = 1, perturb=None):
    """(accumulator of the layout's products, sum of |A||W| over the same products) in float64.  perturb = (segment index, factor on its
    A part): factor 0 drops the segment, 2 doubles its scale, 4096 reads lo8 without its 2^-12."""
    mm = _mm(conv, stride)
    acc = 0.0
    mag = 0.0
    for i, (_, a, b) in enumerate(operand_pairs(layout, x, w, pa, pw, sa)):
        f = perturb[1] if perturb is not None and perturb[0] == i else 1.0
        acc = acc + mm(a * f, b)
        mag = mag + mm(np.abs(a), np.abs(b))
    return acc, mag


def truth(layout: int, x, w, conv: bool = True, stride: int = 1, sa: int = 1):
    """(float64 x w, sum of |x||w|)"""
    mm = _mm(conv, stride)
    xt, wt = truth_input(layout, x, sa), np.asarray(w, np.float64)
    return mm(xt, wt), mm(np.abs(xt), np.abs(wt))


# kernel vs restatement: fp32 accumulation (MFMA products are exact; the sums are fp32) and the output's storage.  The accumulation bound is
# 2^-26 sqrt(n) of the sum of |products| over the n products of an output (~2^-24 per accumulator rounding, n / 16 roundings of partial sums
# of ~sqrt(n) typical products, with a factor 4 of room); the storage bound is 2^-15 |v| for a split output (lo8 keeps 3 mantissa bits of a
# residual below 2^-11 |v|; fp16 residuals far more) and 2^-11 |v| for an fp16 one, plus the subnormal floors of both parts
def tolerance(mag, v, n: int, split_out: bool, bias=None, skip=None) -> np.ndarray:
    extra = 0.0 if bias is None else np.abs(np.asarray(bias, np.float64))
    if skip is not None:
        extra = extra + np.abs(skip)
    t = 2.0 ** -26 * np.sqrt(n) * mag + 2.0 ** -22 * (extra + np.abs(v))
    # (floors: half the subnormal step of lo8, 2^-10 2^-(pa + 12) with pa = 0, and of fp16)
    store = (2.0 ** -15 if split_out else 2.0 ** -11) * np.abs(v) + (2.0 ** -22 if split_out else 2.0 ** -25)
    return t + store


def n_products(layout: int, k: int, sa: int = 1) -> int:
    """products per output element: k (= taps x channels) per segment"""
    return k * {F16: 1, SPLIT16: 2 + sa, MX3: 3, MX2: 2}[layout]


# budgets of the layouts against float64 truth, as a fraction of sum |x||w| per output element: the worst case of each product's rounding.
# fp16 parts round to 2^-11 relative; an e4m3 copy of a residual (itself <= 2^-11 of its value) to 2^-4 relative:
#   f16      2 x 2^-11                      = 2^-10
#   split16  2 x 2^-11 x 2^-11 + lo . lo    < 2^-20
#   mx3/mx2  2 x 2^-4 x 2^-11 (+ lo . lo)   ~ 2^-14
# Measured (tests/test_split_ref_cpu.py, 2 x 9 x 11 x 128 -> 96 3 x 3 and 300 x 256 -> 128 dense, plain / cancelling channels): f16 2^-12.7 .. -14.3,
# split16 2^-22.8 .. -23.5, mx3 2^-17.8 .. -19.0, mx2 2^-18.2 .. -19.6; the kernels on the GPU cases stay within the same figures (a 1 x 1 layer
# over 64 channels on 12.6 M outputs reaches about 2^-16.3).  The GPU tests hold the kernels to these budgets plus the accumulation / storage bounds.
BUDGET = {F16: 2.0 ** -10, SPLIT16: 2.0 ** -20, MX3: 2.0 ** -14, MX2: 2.0 ** -14}


def decode_output(raw: np.ndarray, info: dict, N: int, split_out: bool):
    """raw output buffer [rows, ldo * 2] bytes -> (value, hi, lo part (float64, decoded), lo8 bytes or None, hi8 bytes or None) of rows [0, M)"""
    M, ldo = info["M"], info["ldo"]
    C = ldo // 2 if split_out else ldo
    h = raw[:M].view(np.float16)
    hi = h[:, :N].astype(np.float64)
    if not split_out:
        return hi, hi, np.zeros_like(hi), None, None
    if info["lo8"]:
        hi8 = raw[:M, 2 * C:2 * C + N]
        lo8 = raw[:M, 3 * C:3 * C + N]
        lo = np.ldexp(e4m3_decode(lo8), -(info["lo8_pa"] + 12))
        return hi + lo, hi, lo, lo8, hi8
    lo = h[:, C:C + N].astype(np.float64)
    return hi + lo, hi, lo, None, None


def written_mask(raw: np.ndarray, info: dict, N: int, split_out: bool) -> np.ndarray:
    """bytes of the raw buffer the launch may write: rows [0, M), columns [0, N) of every part"""
    M, ldo = info["M"], info["ldo"]
    C = ldo // 2 if split_out else ldo
    m = np.zeros(raw.shape, bool)
    m[:M, :2 * N] = True
    if split_out and info["lo8"]:
        m[:M, 2 * C:2 * C + N] = True
        m[:M, 3 * C:3 * C + N] = True
    elif split_out:
        m[:M, 2 * C:2 * C + 2 * N] = True
    return m


def case_data(seed: int, x_shape, w_shape, cancel: bool = False, x_scale: float = 1.0, w_scale=None):
    """seeded operands of one case: x ~ N(0, x_scale), w ~ N(0, 1 / fan-in), bias, and a skip source.  cancel: channels are paired so that
    the fp16 products cancel - channel c + C/2 carries fp16(x_c) with weight -fp16(w_c) - and the output is made of correction terms"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(x_shape) * x_scale).astype(np.float32)
    fan = int(np.prod(w_shape[1:]))
    w = (g.standard_normal(w_shape) * (w_scale if w_scale is not None else fan ** -0.5)).astype(np.float32)
    if cancel:
        c = x_shape[-1] // 2
        x[..., c:2 * c] = f16(x[..., :c])
        w[:, c:2 * c] = -f16(w[:, :c])
    b = (g.standard_normal(w_shape[0]) * 0.1).astype(np.float32)
    return x, w, b


# cases the GPU tests run (tests/test_gpu_split_ops.py test_sensitivity_cases_on_gpu) and the CPU sensitivity test perturbs: (name, layout,
# x shape NHWC, w shape, stride, seed, cancel)
SENS_CASES = [
    ("mx3_3x3", MX3, (2, 9, 13, 64), (64, 64, 3, 3), 1, 101, False),
    ("mx3_3x3_cancel", MX3, (2, 9, 13, 128), (72, 128, 3, 3), 1, 102, True),
    ("mx2_1x5", MX2, (1, 7, 19, 128), (96, 128, 1, 5), 1, 103, False),
    ("mx2_1x1_cancel", MX2, (1, 11, 9, 256), (128, 256, 1, 1), 1, 104, True),
    ("split16_3x3_s2", SPLIT16, (2, 12, 10, 64), (64, 64, 3, 3), 2, 105, False),
    ("split16_5x1_cancel", SPLIT16, (1, 13, 8, 128), (128, 128, 5, 1), 1, 106, True),
]


def perturbations(layout: int):
    """(name, segment, factor) of the bugs the tolerances exist for: a dropped correction segment, an E8M0 scale off by 2, lo8 read without
    its 2^12"""
    segs = {SPLIT16: 3, MX3: 3, MX2: 2}[layout]
    out = [(f"drop_seg{i}", i, 0.0) for i in range(1, segs)]
    if layout in (MX3, MX2):
        out += [(f"scale2_seg{i}", i, 2.0) for i in range(1, segs)]
    if layout == MX3:
        out.append(("lo8_without_2^12", 2, 4096.0))
    return out
