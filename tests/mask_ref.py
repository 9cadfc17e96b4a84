"""float64 truth and restatements of the mask_mmdet band's own kernels (CPU only; a helper module of the tests, not a conftest).

Truth is torch / numpy on float64 tensors and, where it already restates the reference, oracle/solov2_oracle.py (cv_resize_linear_u8,
linear_taps_u8, points_nms_scores, matrix_nms, coord_feat).  A restatement rounds where the kernel rounds: source-pixel indices and blend
weights are part of the specification (they decide which taps are read), so they are computed in float32 exactly as torch does -
max(scale * (d + 0.5) - 0.5, 0), floor(d * scale) for nearest, scale the float32 quotient - and the values are then carried in float64.
Every restatement takes a `bug=` name that plants one fault; tests/test_mask_ref_cpu.py asserts the tolerances see each of them.
The generators are shared by the CPU and the GPU tests: inputs are exactly representable in the layout under test (fp16 values for plain
rows, fp16 hi + fp16 lo pairs for split rows), so the upload adds no rounding.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from gm_ref import check, preset, same_bytes, split16          # noqa: F401  (the assert helpers the op-level GPU tests share)
from oracle import solov2_oracle as S
from raft_ref import U24, rng
from split_ref import BUDGET, F16, SPLIT16

THR = 0.5                   # MaskCfg.mask_thr
F32 = np.float32


def layout_of(split) -> int:
    return SPLIT16 if split else F16


def rep(x, split) -> np.ndarray:
    """float32 values the layout holds exactly: fp16(x), or hi + lo with hi = fp16(x), lo = fp16(x - hi) (the sum is exact in fp32: lo's
    last bit is no lower than x's)"""
    x = np.asarray(x, F32)
    hi, lo = split16(x)
    return hi.astype(F32) + lo.astype(F32) if split else hi.astype(F32)


def store_tol(ref, split):
    """one output rounding: the layout's budget of |value| plus half the fp16 subnormal step of the part that rounds"""
    return BUDGET[layout_of(split)] * np.abs(ref) + 2.0 ** -25


def rows16(v, split, dup: bool = False, bug=None) -> np.ndarray:
    """[rows, C] float32 -> the float16 row a kernel stores: [hi], [hi | lo] or [hi | hi | lo].  bug 'swap': [lo | hi]"""
    hi, lo = split16(v)
    if not split:
        return hi
    parts = [lo, hi] if bug == "swap" else [hi, lo]
    if dup:
        parts = [parts[0]] + parts
    return np.concatenate(parts, -1)


def decode(what, raw, rows: int, C: int, split, ld: int = 0, lo_off: int = 0):
    """raw uint8 [rows + guard, 2 ld] -> float64 [rows, C] = hi + lo; asserts that the row tails and the guard rows are still 0xFF"""
    ld = ld or C * (2 if split else 1)
    lo_off = lo_off or (C if split else 0)
    h = raw.view(np.float16).reshape(-1, ld)
    own = np.zeros(ld, bool)
    own[:C] = True
    if split:
        own[lo_off:lo_off + C] = True
    preset(what + ": row tails", h[:rows][:, ~own])
    preset(what + ": guard rows", h[rows:])
    v = h[:rows, :C].astype(np.float64)
    return v + h[:rows, lo_off:lo_off + C].astype(np.float64) if split else v


def box(a, r: int = 2):
    """box filter of radius r over the last two axes (edge padding): the smooth logit fields of the mask inputs"""
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], mode="edge")
    out = np.zeros_like(a)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += p[..., dy:dy + a.shape[-2], dx:dx + a.shape[-1]]
    return out / (2 * r + 1) ** 2


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


# =====================================================================================================================
# mask_prep
# =====================================================================================================================
PREP_CASES = [          # (name, H, W, nh, nw, Hp, Wp)
    ("down", 100, 150, 40, 60, 64, 64),
    ("up", 37, 53, 85, 122, 96, 128),         # nw % 4 = 2, the pad is more than one 4 x 4 block wide
    ("identity", 32, 64, 32, 64, 32, 64),
]


def prep_frames(seed: int, n: int, H: int, W: int):
    g = rng(seed)
    f = g.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    f[:, :2, :3] = 255
    f[:, -2:, -3:] = 0
    return f


def prep_tables(H, W, nh, nw):
    return (np.stack(S.linear_taps_u8(W, nw), 1).astype(np.int32), np.stack(S.linear_taps_u8_rows(H, nh), 1).astype(np.int32))


def prep_restated(frames, nh, nw, Hp, Wp, bug=None):
    """(chw float32 [n, 3, Hp, Wp], s2d float32 [n, Hp / 4, Wp / 4, 64]).  bugs: 's2d_xy' (dy, dx swapped in the channel index)"""
    n = frames.shape[0]
    mean = np.asarray(S.MEAN, np.float64).astype(F32)
    stdinv = (1.0 / np.asarray(S.STD, np.float64)).astype(F32)
    chw = np.zeros((n, 3, Hp, Wp), F32)
    for i in range(n):
        img = S.cv_resize_linear_u8(frames[i], nh, nw).astype(F32)
        chw[i, :, :nh, :nw] = ((img - mean) * stdinv).transpose(2, 0, 1)
    b = chw.reshape(n, 3, Hp // 4, 4, Wp // 4, 4)                      # [n, c, by, dy, bx, dx]
    order = (0, 2, 4, 5, 3, 1) if bug == "s2d_xy" else (0, 2, 4, 3, 5, 1)
    s = np.zeros((n, Hp // 4, Wp // 4, 4, 4, 4), F32)
    s[..., :3] = b.transpose(order)
    return chw, s.reshape(n, Hp // 4, Wp // 4, 64)


# =====================================================================================================================
# maxpool3x3s2, subsample2, nearest_add, coord_concat
# =====================================================================================================================
POOL_SIZES = [(7, 9), (8, 10), (1, 1)]


def map_data(seed: int, shape, split, negative: bool = False, scale: float = 1.0):
    x = rng(seed).standard_normal(shape) * scale
    if negative:
        x = -np.abs(x) - 0.25
    return rep(x, split)


def maxpool_restated(x, bug=None):
    """x [n, H, W, C] -> float64 [n, OH, OW, C].  bug 'max0': the running maximum starts at 0"""
    t = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    y = F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).numpy()
    return np.maximum(y, 0.0) if bug == "max0" else y


NEAREST_CASES = [((7, 11), (4, 6)), ((13, 21), (7, 11)), ((12, 20), (6, 10))]


def nearest_index(dst: int, src: int, bug=None):
    """torch 'nearest': min(floor(d * scale), src - 1) with scale = float32(src) / float32(dst), the product in float32"""
    scale = F32(src) / F32(dst)
    i = np.floor(np.arange(dst, dtype=F32) * scale).astype(np.int64)
    if bug == "row_off":
        i = i + 1
    return np.minimum(i, src - 1)


def nearest_add_restated(dst, src, bug=None):
    """bug 'row_off': the source row one too far down"""
    h, w = dst.shape[1:3]
    sy = nearest_index(h, src.shape[1], bug)
    sx = nearest_index(w, src.shape[2])
    return np.asarray(dst, np.float64) + np.asarray(src, np.float64)[:, sy][:, :, sx]


def nearest_add_truth(dst, src):
    t = torch.from_numpy(np.asarray(src, np.float64)).permute(0, 3, 1, 2)
    return np.asarray(dst, np.float64) + F.interpolate(t, size=dst.shape[1:3], mode="nearest").permute(0, 2, 3, 1).numpy()


COORD_SIZES = [(1, 5), (5, 1), (6, 4), (7, 9)]


def coord_restated(x, bug=None):
    """x [n, h, w, C] float32 -> float32 [n, h, w, C + 64]: x, then torch.linspace(-1, 1, w)[px], linspace(-1, 1, h)[py], zeros.
    bug 'xy': the two coordinate channels swapped"""
    n, h, w, C = x.shape
    out = np.zeros((n, h, w, C + 64), F32)
    out[..., :C] = x
    cf = S.coord_feat(n, h, w).numpy()                          # [n, 2, h, w]: channel 0 = x
    out[..., C] = cf[:, 1 if bug == "xy" else 0]
    out[..., C + 1] = cf[:, 0 if bug == "xy" else 1]
    return out


# =====================================================================================================================
# bilinear (align_corners False)
# =====================================================================================================================
BILINEAR_CASES = [((5, 7), (10, 14)), ((12, 20), (10, 10)), ((5, 7), (12, 12)), ((12, 12), (12, 12)), ((1, 1), (4, 4))]


def lerp_taps(dst: int, src: int, scale=None, bug=None):
    """(i0, i1, l1 float64 of the float32 weight) per destination index, every operation rounded to float32 as torch's
    area_pixel_compute_source_index does.  bugs: 'no_half' (src = scale d), 'row_off' (i0 + 1), 'no_clamp' (i1 = i0 + 1 past the end)"""
    scale = F32(src) / F32(dst) if scale is None else F32(scale)
    d = np.arange(dst, dtype=F32)
    s = scale * d if bug == "no_half" else np.maximum(scale * (d + F32(0.5)) - F32(0.5), F32(0))
    s = s.astype(F32)
    i0 = np.minimum(s.astype(np.int64), src - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    if bug == "row_off":
        i0 = np.minimum(i0 + 1, src - 1)
    i1 = i0 + 1 if bug == "no_clamp" else i0 + (i0 < src - 1)
    return i0, i1, l1.astype(np.float64)


def bilinear_restated(x, OH, OW, y0=None, bug=None, sy=None, sx=None):
    """x [n, H, W, C] -> (float64 [n, OH, OW, C], largest tap magnitude of every output).  The blend is the kernel's expression
    hy (hx v00 + lx v01) + ly (hx v10 + lx v11) in float64 with the float32 weights; bugs of lerp_taps apply to the rows.  A tap past the
    last row ('no_clamp') reads what follows in memory: the next sample's first row (the first sample's after the last)"""
    x = np.asarray(x, np.float64)
    n, H, W, C = x.shape
    y0_, y1_, ly = lerp_taps(OH, H, sy, bug)
    x0_, x1_, lx = lerp_taps(OW, W, sx)
    flat = x.reshape(n * H, W, C)
    base = (np.arange(n) * H)[:, None]
    r0 = flat[(base + y0_[None]) % (n * H)]                       # [n, OH, W, C]
    r1 = flat[(base + y1_[None]) % (n * H)]
    hy = (F32(1) - ly.astype(F32)).astype(np.float64)
    hx = (F32(1) - lx.astype(F32)).astype(np.float64)
    LY, HY = ly[None, :, None, None], hy[None, :, None, None]
    LX, HX = lx[None, None, :, None], hx[None, None, :, None]
    v00, v01, v10, v11 = r0[:, :, x0_], r0[:, :, x1_], r1[:, :, x0_], r1[:, :, x1_]
    out = HY * (HX * v00 + LX * v01) + LY * (HX * v10 + LX * v11)
    mag = np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11)))
    if y0 is not None:
        out = out + np.asarray(y0, np.float64)
        mag = np.maximum(mag, np.abs(y0))
    return out, mag


def bilinear_truth(x, OH, OW, y0=None):
    """F.interpolate on float64 (float64 coordinates)"""
    t = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    y = F.interpolate(t, size=(OH, OW), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    return y if y0 is None else y + np.asarray(y0, np.float64)


def bilinear_coord_tolerance(x, OH, OW):
    """kernel (float32 coordinates) vs float64 coordinates: the source position carries three float32 roundings (the scale quotient, the
    product, the subtraction), each at most 2^-24 of a value no larger than the input size, so it is off by at most 3 2^-24 (size + 1) per
    axis; a bilinear surface's slope along an axis never exceeds the largest difference of adjacent entries, and the surface is continuous
    where the integer part changes -> [n, 1, 1, C]"""
    x = np.asarray(x, np.float64)
    n, H, W, C = x.shape
    ay = np.abs(np.diff(x, axis=1)).max((1, 2)) if H > 1 else np.zeros((n, C))
    ax = np.abs(np.diff(x, axis=2)).max((1, 2)) if W > 1 else np.zeros((n, C))
    return (3 * U24 * ((H + 1) * ay + (W + 1) * ax))[:, None, None, :]


# =====================================================================================================================
# GroupNorm(32) + ReLU
# =====================================================================================================================
GN_SHAPES = [(32, 1), (32, 257), (128, 255), (128, 256), (128, 700), (512, 5000)]
GN_RATIOS = [0, 3, 10]
GN_CHUNK = 256


def gn_data(seed: int, C: int, HW: int, ratio: float, split, n: int = 3):
    """x [n, HW, C]: sample b is N(0, 1) scaled by (0.5, 1, 4)[b] around a group mean of ratio std whose sign alternates over the groups and
    flips with the sample; gamma in +-[0.5, 1.5], beta N(0, 0.3)"""
    g = rng(seed)
    x = g.standard_normal((n, HW, C))
    sign = np.where(np.arange(C) // (C // 32) % 2 == 0, 1.0, -1.0)
    for b in range(n):
        x[b] = (x[b] + ratio * sign * (1 if b % 2 == 0 else -1)) * (0.5, 1.0, 4.0)[b % 3]
    gamma = (0.5 + g.random(C)) * np.where(g.random(C) < 0.5, -1, 1)
    beta = 0.3 * g.standard_normal(C)
    return rep(x, split), gamma.astype(F32), beta.astype(F32)


def gn_truth(x, gamma, beta):
    """float64 GroupNorm(32, eps 1e-5) + ReLU of x [n, HW, C] -> (y, aff [n, C, 2] = (rstd gamma, mean))"""
    x = np.asarray(x, np.float64)
    n, HW, C = x.shape
    xg = x.reshape(n, HW, 32, C // 32)
    mean = xg.mean((1, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(xg.var((1, 3), keepdims=True) + 1e-5)
    y = ((xg - mean) * rstd).reshape(n, HW, C) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    r = np.broadcast_to(rstd, (n, 1, 32, C // 32)).reshape(n, C) * np.asarray(gamma, np.float64)
    return np.maximum(y, 0.0), np.stack([r, np.broadcast_to(mean, (n, 1, 32, C // 32)).reshape(n, C)], -1)


def _seq_sum32(a, axis):
    """float32 sum along an axis in index order (np.cumsum accumulates sequentially), as a kernel's running sum does"""
    return np.take(np.cumsum(a.astype(F32), axis=axis, dtype=F32), -1, axis=axis)


def gn_restated(x, gamma, beta, bug=None):
    """the kernels' arithmetic in numpy float32: per (chunk of 256 pixels, channel) the mean from sums shifted by the chunk's first pixel and
    M2 = sum (v - mean)^2, combined over a group's (chunk, channel) items with the parallel-variance formula; y = max((v - mean) r + beta, 0).
    bug 'uncentred': the variance as E[x^2] - mean^2 from plain float32 sums and y = max(v r + (beta - mean r), 0) (what the kernels did before)"""
    x = np.asarray(x, F32)
    n, HW, C = x.shape
    cpg = C // 32
    nch = -(-HW // GN_CHUNK)
    inv_cnt = F32(1.0) / (F32(HW) * F32(cpg))
    aff = np.zeros((n, C, 2), F32)
    if bug == "uncentred":
        s = np.zeros((n, nch, C), F32)
        q = np.zeros((n, nch, C), F32)
        for ch in range(nch):
            c = x[:, ch * GN_CHUNK:(ch + 1) * GN_CHUNK]
            s[:, ch] = _seq_sum32(c, 1)
            q[:, ch] = _seq_sum32(c * c, 1)
        sg = _seq_sum32(s.reshape(n, nch, 32, cpg).transpose(0, 2, 1, 3).reshape(n, 32, -1), 2)
        qg = _seq_sum32(q.reshape(n, nch, 32, cpg).transpose(0, 2, 1, 3).reshape(n, 32, -1), 2)
        mean = sg * inv_cnt
        var = np.maximum(qg * inv_cnt - mean * mean, F32(0))
    else:
        m = np.zeros((n, nch, C), F32)
        M2 = np.zeros((n, nch, C), F32)
        cnt = np.zeros(nch, F32)
        for ch in range(nch):
            c = x[:, ch * GN_CHUNK:(ch + 1) * GN_CHUNK]
            cnt[ch] = c.shape[1]
            k = c[:, :1]
            m[:, ch] = k[:, 0] + _seq_sum32(c - k, 1) * (F32(1) / F32(c.shape[1]))
            d = c - m[:, ch][:, None]
            M2[:, ch] = _seq_sum32(d * d, 1)
        mg = m.reshape(n, nch, 32, cpg).transpose(0, 2, 1, 3)                # [n, 32, nch, cpg]
        Mg = M2.reshape(n, nch, 32, cpg).transpose(0, 2, 1, 3)
        w = cnt[None, None, :, None]
        k = mg[:, :, :1, :1]
        mean = (k[..., 0, 0] + _seq_sum32((w * (mg - k)).reshape(n, 32, -1), 2) * inv_cnt).astype(F32)
        d = mg - mean[..., None, None]
        var = _seq_sum32((Mg + w * (d * d)).reshape(n, 32, -1), 2) * inv_cnt
    rs = (F32(1) / np.sqrt(var + F32(1e-5), dtype=F32)).astype(F32)
    r = np.repeat(rs, cpg, 1) * np.asarray(gamma, F32)
    aff[..., 0] = r
    mc = np.repeat(mean, cpg, 1).astype(F32)
    if bug == "uncentred":
        aff[..., 1] = np.asarray(beta, F32) - mc * r
        y = np.maximum(x * aff[:, None, :, 0] + aff[:, None, :, 1], F32(0))
    else:
        aff[..., 1] = mc
        y = np.maximum((x - mc[:, None]) * r[:, None] + np.asarray(beta, F32), F32(0))
    return y.astype(np.float64), aff


# =====================================================================================================================
# cls_points_nms
# =====================================================================================================================
NMS_GRIDS = [1, 4, 12]
SAT = 17.5          # 1 - sigmoid(x) < 2^-25 from x = 17.33: the float32 sigmoid is exactly 1


def cls_logits(seed: int, n: int, g: int, C: int = 80):
    """[n, g, g, C] multiples of 1/8 in [-6, 4]; on grids that have room a 3 x 3 plateau of equal values and a horizontal pair 20 | 21, both
    of which saturate to 1.0f (the reference compares float32 sigmoids and keeps both)"""
    gg = rng(seed)
    x = gg.integers(-48, 33, (n, g, g, C)).astype(F32) / F32(8)
    if g >= 4:
        x[:, 0:3, 1:4, 5] = 3.5
        x[:, g - 1, 0, 7] = 20.0
        x[:, g - 1, 1, 7] = 21.0
    return x


def cls_truth(logit):
    """float64: (kept [n, g g, C] bool, sigmoid [n, g g, C]).  A cell is kept when no cell of the 2 x 2 window whose lower-right corner it
    is has a larger float32 sigmoid: logits decide, with everything from SAT up equal"""
    x = np.minimum(np.asarray(logit, np.float64), SAT)
    n, g, _, C = x.shape
    p = np.pad(x, ((0, 0), (1, 0), (1, 0), (0, 0)), constant_values=-np.inf)
    m = np.maximum(np.maximum(p[:, 1:, 1:], p[:, :-1, 1:]), np.maximum(p[:, 1:, :-1], p[:, :-1, :-1]))
    return (x >= m).reshape(n, g * g, C), sigmoid(logit).reshape(n, g * g, C)


def cls_restated(logit, bug=None):
    """the oracle's points_nms_scores on float32 tensors -> [n, g g, C].  bug 'window': the window on the lower-right side instead"""
    t = torch.from_numpy(np.asarray(logit, F32)).permute(0, 3, 1, 2)
    if bug == "window":
        t = t.flip(2, 3)
        return S.points_nms_scores(t).reshape(t.shape[0], t.shape[2], t.shape[3], -1).flip(1, 2).reshape(t.shape[0], -1, t.shape[1]).numpy()
    return S.points_nms_scores(t).numpy()


# =====================================================================================================================
# mask logits: stats, bit masks, intersections, sigmoid rows, final masks
# =====================================================================================================================
def mask_logits(seed: int, rows: int, fh: int, fw: int, amp: float = 6.0):
    """[rows, fh, fw] float32: box-smoothed noise (blobs of both signs) with no value whose sigmoid lies within 2^-20 of THR"""
    g = rng(seed)
    x = box(g.standard_normal((rows, fh, fw)), 2) * amp + 0.3 * g.standard_normal((rows, 1, 1))
    x = x.astype(F32)
    near = np.abs(x) < 1e-4             # d sigmoid / dx = 1 / 4 at 0
    x[near] = np.where(x[near] < 0, F32(-1e-3), F32(1e-3))
    return x


def stats_truth(logit, HW: int):
    """logit [rows, ld] -> (area, soft sum) float64 over the first HW columns"""
    s = sigmoid(np.asarray(logit)[:, :HW])
    on = s > THR
    return on.sum(1).astype(np.float64), (s * on).sum(1)


def bits_truth(logit, idx, HW: int):
    """-> (uint64 [n, HW / 64] little-endian bit rows, masks bool [n, HW])"""
    on = sigmoid(np.asarray(logit)[np.asarray(idx), :HW]) > THR
    return np.packbits(on, axis=1, bitorder="little").view(np.uint64), on


def nms_masks(seed: int, n: int, side: int = 32):
    """n rectangles on a side x side grid around a few centres, so IoUs of every size occur -> (masks bool [n, side, side], generator)"""
    g = rng(seed)
    m = np.zeros((n, side, side), bool)
    for i in range(n):
        cy, cx = g.integers(4, side - 4, 2) if i % 3 == 0 else (8 + 8 * (i % 2), 8 + 8 * (i % 4 // 2))
        hy, hx = g.integers(2, 9, 2)
        m[i, max(cy - hy, 0):cy + hy, max(cx - hx, 0):cx + hx] = True
    return m, g


def nms_data(seed: int, n: int):
    """n score-sorted instances: intersections and areas of real masks (so every IoU is <= 1), four labels of which label 3 is carried by
    one instance -> (inter [n, n], area [n], label [n], score [n])"""
    m, g = nms_masks(seed, n)
    flat = m.reshape(n, -1).astype(np.float64)
    inter = flat @ flat.T
    label = g.integers(0, 3, n)
    label[n // 2] = 3
    score = np.sort(0.1 + 0.9 * g.random(n))[::-1]
    return inter.astype(F32), np.diag(inter).astype(F32), label.astype(np.int32), score.astype(F32)


def nms_restated(inter, area, label, score, sigma: float = 2.0, bug=None):
    """mask_matrix_nms's gaussian decay in float64 on score-sorted inputs -> (comp [n], decayed score [n]).
    bugs: 'lower' (the lower triangle of the IoU matrix), 'comp_j' (the compensation of the column instead of the row)"""
    inter, area = np.asarray(inter, np.float64), np.asarray(area, np.float64)
    n = len(area)
    iou = inter / (area[:, None] + area[None, :] - inter)
    tri = np.tril(np.ones((n, n), bool), -1) if bug == "lower" else np.triu(np.ones((n, n), bool), 1)
    d = iou * tri * (np.asarray(label)[:, None] == np.asarray(label)[None, :])
    if bug == "lower":
        d = d.T
    comp = d.max(0) if n > 1 else np.zeros(1)
    cm = np.broadcast_to(comp[None, :] if bug == "comp_j" else comp[:, None], (n, n))
    coeff = (np.exp(-sigma * d ** 2) / np.exp(-sigma * cm ** 2)).min(0)
    return comp, np.asarray(score, np.float64) * coeff


ACC_CASES = [           # (fh, fw, h, w, H, W, k)
    (12, 20, 45, 77, 37, 61, 9),
    (12, 20, 45, 77, 180, 300, 9),
    (16, 24, 64, 96, 64, 96, 5),
    (8, 8, 29, 30, 97, 33, 3),
]


def acc_data(seed: int, fh, fw, k):
    """sig [k, fh, fw] float32 = sigmoid of box-smoothed logits; instance 1 is instance 0 plus a little noise, so the two overlap; use [k]
    with zeros (instances 0 and 1 are both used in the even cases: their common pixels read 254)"""
    g = rng(seed)
    x = box(g.standard_normal((k, fh, fw)), 1) * 8.0
    x[1] = x[0] + 0.5 * g.standard_normal((fh, fw))
    use = np.ones(k, np.uint8)
    use[2::3] = 0
    if seed % 2:
        use[1] = 0
    return sigmoid(x).astype(F32), use


def acc_restated(sig, h, w, H, W, bug=None):
    """the band's two resizes per output pixel: F.interpolate(x4)[:h, :w] then F.interpolate(size = (H, W)), float32 indices and weights,
    float64 values -> soft [k, H, W].  bugs of lerp_taps apply to the rows of the second resize"""
    sig = np.asarray(sig, np.float64)
    k, fh, fw = sig.shape
    up, _ = bilinear_restated(sig[..., None], 4 * fh, 4 * fw, sy=0.25, sx=0.25)
    out, _ = bilinear_restated(up[:, :h, :w], H, W, bug=bug)
    return out[..., 0]


def acc_truth(sig, h, w, H, W):
    t = torch.from_numpy(np.asarray(sig, np.float64))[None]
    up = F.interpolate(t, size=(4 * t.shape[2], 4 * t.shape[3]), mode="bilinear", align_corners=False)[:, :, :h, :w]
    return F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()


def acc_image(on, use):
    """on [k, H, W] bool -> uint8 [H, W, 3]: (255 count) mod 256 of the used instances"""
    cnt = (on & (np.asarray(use) != 0)[:, None, None]).sum(0)
    return np.repeat(((255 * cnt) & 255).astype(np.uint8)[..., None], 3, -1)


ACC_MARGIN = 2.0 ** -19         # 16 float32 roundings on values in [0, 1], doubled


# =====================================================================================================================
# dynamic convolution
# =====================================================================================================================
def dynconv_data(seed: int, rows: int, HW4: int, split):
    g = rng(seed)
    return rep(g.standard_normal((rows, 256)) * 0.3, split), rep(np.maximum(g.standard_normal((HW4, 256)), 0), split)
