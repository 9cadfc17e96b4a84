"""float64 truth and exact restatements of the flow_gmflow band's own kernels (CPU only; a helper module of the tests, not a conftest).

Truth is oracle/gmflow_oracle.py (pinned to the real reference by the goldens) fed float64 tensors: window_attention, shift_mask, split_windows,
global_correlation_softmax, and the flow_attention arithmetic; position_sine is float32 inside, so it is restated here in float64.  A
restatement rounds where the kernels round - numpy float32 adds, hi = f16(v), lo = f16(v - hi) - and takes a `bug=` name that plants one
fault (tests/test_gm_ref_cpu.py asserts the tolerances see each of them).  `check` / `preset` are the assert helpers of the op-level GPU
tests (tests/test_gpu_raft_ops.py imports them from here).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import gmflow_oracle as G
from raft_ref import U24, f16_step, rng
from split_ref import BUDGET, F16, SPLIT16

# (h8, w8): each the smallest grid that hits its edge
GRIDS = [(4, 4),            # engine minimum: Lw 4, ldv 32, one partial key tile
         (6, 10),           # odd windows 3 x 5: wh / 2 floors
         (18, 26),          # Lw 117 < 128 queries, key tail 21
         (28, 38)]          # Lw 266: three query blocks, key tail 10; P 1064, P % 32 = 8
LARGE = (102, 180)          # 1080p x 0.75: element-wise kernels only
EPS_LN = 1e-5


# =====================================================================================================================
# assert helpers of the op-level GPU tests
# =====================================================================================================================
def check(what, got, ref, tol):
    """asserts |got - ref| <= tol element-wise; the message names the worst element.  Returns worst error / tolerance."""
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(ref))
    bad = ~np.isfinite(got)
    assert not bad.any(), "%s: element %s is %r" % (what, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])])
    r = np.abs(got - ref) / tol
    i = np.unravel_index(np.argmax(r), r.shape)
    print("\n  %-58s worst err / tol %.3f at %s" % (what, r[i], i), end="")
    assert r[i] <= 1, "%s: element %s: kernel %.9g reference %.9g |err| %.3e tolerance %.3e (%d elements outside)" % (
        what, i, got[i], ref[i], abs(got[i] - ref[i]), tol[i], int((r > 1).sum()))
    return float(r[i])


def preset(what, raw):
    raw = np.ascontiguousarray(raw).view(np.uint8)
    bad = raw != 0xFF
    assert not bad.any(), "%s: %d bytes written outside what the kernel owns, first at %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))


def same_bytes(what, got, want):
    """got, want: arrays of one dtype and shape that must agree bit for bit (a -0.0 is not a +0.0)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = got.view(u) != want.view(u)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: element %s is %r (0x%x), the restatement gives %r (0x%x); %d elements differ" % (
            what, i, got[i], got.view(u)[i], want[i], want.view(u)[i], int(bad.sum())))


# =====================================================================================================================
# geometry, the two host tables
# =====================================================================================================================
def geom(h8: int, w8: int) -> dict:
    P, wh, ww = h8 * w8, h8 // 2, w8 // 2
    return dict(h8=h8, w8=w8, P=P, wh=wh, ww=ww, Lw=wh * ww, ldv=-(-(wh * ww) // 32) * 32, ldvP=-(-P // 32) * 32)


def positions_truth(h8: int, w8: int):
    """PositionEmbeddingSine(64, temperature 10000, normalize, scale 2 pi) of ONE wh x ww window tiled over the 2 x 2 windows, float64:
    (pos [P, 128], the sin / cos arguments [P, 128]); channels 0..63 from y, 64..127 from x, (sin, cos) interleaved"""
    wh, ww = h8 // 2, w8 // 2
    i = np.arange(64)
    dim_t = 10000.0 ** (2.0 * (i // 2) / 64.0)
    ye = ((np.arange(h8) % wh + 1) / (wh + 1e-6) * 2 * np.pi)[:, None, None] / dim_t
    xe = ((np.arange(w8) % ww + 1) / (ww + 1e-6) * 2 * np.pi)[None, :, None] / dim_t
    arg = np.concatenate([np.broadcast_to(ye, (h8, w8, 64)), np.broadcast_to(xe, (h8, w8, 64))], 2).reshape(h8 * w8, 128)
    odd = (np.arange(128) & 1).astype(bool)
    return np.where(odd, np.cos(arg), np.sin(arg)), arg


def positions_tolerance(arg):
    """three fp32 roundings precede the sin / cos (the normalised coordinate, the scale, the division by dim_t; arg <= 2 pi), then the
    function's own rounding"""
    return 3 * U24 * np.abs(arg) + 2.0 ** -22


def region_mask(reg):
    """region ids [4, Lw] -> the additive mask [4, Lw (query), Lw (key)] the attention kernel applies: -100 where the ids differ"""
    reg = np.asarray(reg)
    return np.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0)


def regions_restated(h8: int, w8: int, bug=None):
    """shift_regions restated (ids in window order).  bug 'region_edge': a boundary one row / column late"""
    wh, ww = h8 // 2, w8 // 2
    o = 1 if bug == "region_edge" else 0
    ry, rx = np.arange(h8), np.arange(w8)
    cy = np.where(ry < h8 - wh, 0, np.where(ry < h8 - wh // 2 + o, 1, 2))
    cx = np.where(rx < w8 - ww, 0, np.where(rx < w8 - ww // 2 + o, 1, 2))
    img = (cy[:, None] * 3 + cx[None, :]).reshape(2, wh, 2, ww).transpose(0, 2, 1, 3)
    return img.reshape(4, wh * ww).astype(np.int8)


def win_rows(h8: int, w8: int, images: int, shifted: bool, bug=None):
    """the kernels' win_row: [images * 4, Lw] -> row of the [images * P] token matrix.  Window bw = image * 4 + wy * 2 + wx, position
    ly * ww + lx; the windows are cut from the map rolled by (-wh / 2, -ww / 2).  bugs: 'shift_up', 'roll_dir', 'wywx'"""
    wh, ww, P = h8 // 2, w8 // 2, h8 * w8
    sy, sx = (wh // 2, ww // 2) if shifted else (0, 0)
    if shifted and bug == "shift_up":
        sy, sx = (wh + 1) // 2, (ww + 1) // 2
    if bug == "roll_dir":
        sy, sx = -sy, -sx
    bw = np.arange(images * 4)
    img, wy, wx = bw >> 2, (bw >> 1) & 1, bw & 1
    if bug == "wywx":
        wy, wx = wx, wy
    ly, lx = np.divmod(np.arange(wh * ww), ww)
    gy = (wy[:, None] * wh + ly[None, :] + sy) % h8
    gx = (wx[:, None] * ww + lx[None, :] + sx) % w8
    return img[:, None] * P + gy * w8 + gx


def win_rows_oracle(h8: int, w8: int, images: int, shifted: bool):
    """the same map from the reference's own steps: torch.roll + split_feature on a map of row numbers"""
    wh, ww = h8 // 2, w8 // 2
    t = torch.arange(images * h8 * w8).view(images, h8, w8, 1)
    if shifted:
        t = torch.roll(t, shifts=(-(wh // 2), -(ww // 2)), dims=(1, 2))
    return G.split_windows(t, 2).reshape(images * 4, wh * ww).numpy()


# =====================================================================================================================
# element-wise kernels restated (bytes)
# =====================================================================================================================
def split16(v):
    """(hi, lo) float16: hi = f16(v), lo = f16(v - hi) with the subtraction in fp32 (gmflow_kernels.hip split8)"""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def split_rows(v):
    """[rows, C] -> float16 [rows, 2 C] = [hi | lo]"""
    return np.concatenate(split16(v), axis=-1)


def tokens_restated(feat, pos):
    """feat [NP + 1, P, 128], pos [P, 128] -> X float32 [NP * 2 * P, 128]: pair n holds frames n and n + 1"""
    feat, pos = np.asarray(feat, np.float32), np.asarray(pos, np.float32)
    NP = feat.shape[0] - 1
    X = np.stack([feat[n + e] + pos for n in range(NP) for e in (0, 1)])
    return X.reshape(-1, 128)


def pack_rows_restated(src, col, rows):
    """window rows job: float16 [Bw * Lw, 256]"""
    return split_rows(np.asarray(src, np.float32)[rows.reshape(-1), col:col + 128])


def pack_vt_restated(src, col, rows, ldv):
    """V^T job: float16 [Bw * 2 * 128, ldv]: hi rows then lo rows of every window, keys along the row, columns [Lw, ldv) zero"""
    Bw, Lw = rows.shape
    hi, lo = split16(np.asarray(src, np.float32)[rows, col:col + 128])                # [Bw, Lw, 128]
    out = np.zeros((Bw, 2, 128, ldv), np.float16)
    out[:, 0, :, :Lw] = hi.transpose(0, 2, 1)
    out[:, 1, :, :Lw] = lo.transpose(0, 2, 1)
    return out.reshape(Bw * 256, ldv)


def cat_rows_restated(X, y16, bug=None):
    """mode 1 of gm_ln: [hi X | hi y | lo X | lo y] (512 halfs); y16 = (hi, lo) of y.  bug 'cat_swap': [hi X | lo X | hi y | lo y]"""
    xh, xl = split16(X)
    parts = [xh, xl, y16[0], y16[1]] if bug == "cat_swap" else [xh, y16[0], xl, y16[1]]
    return np.concatenate(parts, axis=-1)


def match_flow_restated(O, w8, bug=None):
    """O [B, P, 32] -> flow float32 [B, P, 2] = O[.., :2] - own (x, y) in fp32.  bug 'own_xy': the own coordinate swapped"""
    O = np.asarray(O, np.float32)
    t = np.arange(O.shape[1])
    x, y = (t % w8).astype(np.float32), (t // w8).astype(np.float32)
    if bug == "own_xy":
        x, y = y, x
    return np.stack([O[..., 0] - x, O[..., 1] - y], -1)


def flow_vt_restated(flow, ldvP, guard):
    """the halfs gm_match_flow owns in a 0xFF-preset [B * 64 + guard, ldvP] buffer: rows 0, 1 (hi) and 32, 33 (lo), columns < P"""
    B, P, _ = flow.shape
    out = np.full((B * 64 + guard, ldvP), 0xFFFF, np.uint16).view(np.float16)
    hi, lo = split16(flow)
    v = out[:B * 64].reshape(B, 64, ldvP)
    v[:, 0:2, :P] = hi.transpose(0, 2, 1)
    v[:, 32:34, :P] = lo.transpose(0, 2, 1)
    return out


def grid_vt_restated(h8, w8, guard):
    g = geom(h8, w8)
    out = np.full((64 + guard, g["ldvP"]), 0xFFFF, np.uint16).view(np.float16)
    t = np.arange(g["P"])
    out[0, :g["P"]] = (t % w8).astype(np.float16)
    out[1, :g["P"]] = (t // w8).astype(np.float16)
    return out


def upsampler_map_restated(flow, X, img_step):
    """flow [B, P, 2], X [images, P, 128] -> float16 [B * P, 384] = [hi (flow 2, feature 128, zeros 62) | lo (192)]"""
    B, P, _ = flow.shape
    v = np.zeros((B, P, 192), np.float32)
    v[..., :2] = flow
    v[..., 2:130] = np.asarray(X, np.float32)[np.arange(B) * img_step]
    return split_rows(v.reshape(B * P, 192))


# =====================================================================================================================
# LayerNorm (gm_ln_kernel: one wave per row, two passes, biased variance, eps 1e-5, fp32)
# =====================================================================================================================
def ln_truth(M, gamma, beta):
    """float64: (y, mean, sqrt(var + eps)) of rows M [rows, 128]"""
    M = np.asarray(M, np.float64)
    mean = M.mean(-1, keepdims=True)
    se = np.sqrt(((M - mean) ** 2).mean(-1, keepdims=True) + EPS_LN)
    return (M - mean) / se * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64), mean, se


LN_SUM = 7          # roundings in a wave_sum of 128 values: the lane's own pair add, then the 6 levels of the 64-lane butterfly


def ln_tolerance(M, gamma, beta):
    """|kernel y - float64 y| per element, from the kernel's arithmetic (2^-24 = one fp32 rounding, relative):
      mean      LN_SUM roundings of partial sums no larger than 128 max|v|           -> |dmean| <= 7 2^-24 max|v|
      d = v - mean  one rounding more; |d| <= |mean| + max|v|                        -> |dd| <= 8 2^-24 (|mean| + max|v|)
      var       d^2 and the same sum: 9 2^-24 var + 2 mean|d| |dd|; rs = 1 / sqrt(var + eps) adds 3 (sqrt, divide)
                                                                                    -> |drs| / rs <= (8 (|mean| + max|v|) / s + 7.5) 2^-24
      y = d rs gamma + beta   two multiplies, one add                               -> 2 z 2^-24 |gamma|, 2^-24 |y| twice (+ margin: 2^-22 |y|)
    with s = sqrt(var + eps) and z = |d| / s.  As (|mean| + max|v|) / s >= 1 this is |gamma| c 2^-24 (|mean| + |v|) / s + 2^-22 |y| with
    c = 8 + 17.5 z rounded up to 8 + 18 z and |v| the row's largest magnitude."""
    y, mean, se = ln_truth(M, gamma, beta)
    M = np.asarray(M, np.float64)
    z = np.abs(M - mean) / se
    c = (LN_SUM + 1) + 18 * z
    return np.abs(np.asarray(gamma, np.float64)) * c * U24 * (np.abs(mean) + np.abs(M).max(-1, keepdims=True)) / se + 2.0 ** -22 * np.abs(y)


def ln_restated(M, gamma, beta, bug=None):
    """the kernel's steps in numpy float32 (numpy's pairwise sum stands in for the butterfly).  bugs: 'one_pass' (var = E v^2 - mean^2),
    'no_eps', 'var127'"""
    M, gamma, beta = np.asarray(M, np.float32), np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    inv = np.float32(1.0 / 128.0)
    mean = (M.sum(-1, keepdims=True, dtype=np.float32) * inv).astype(np.float32)
    d = M - mean
    if bug == "one_pass":
        var = (M * M).sum(-1, keepdims=True, dtype=np.float32) * inv - mean * mean
        var = np.maximum(var, np.float32(0))
    else:
        var = (d * d).sum(-1, keepdims=True, dtype=np.float32) * (np.float32(1.0 / 127.0) if bug == "var127" else inv)
    rs = np.float32(1.0) / np.sqrt(var + (np.float32(0) if bug == "no_eps" else np.float32(EPS_LN)), dtype=np.float32)
    return (d * rs * gamma + beta).astype(np.float32)


def ln_data(seed: int, rows: int):
    """rows of 128 values: plain (mean 0, std 1), offset rows with |mean| / std in {100, 300, 1000, 3000} (one-pass variance cancels there), rows
    whose variance is near eps (std 1e-3 .. 1e-2: eps matters); gamma in +-[0.5, 1.5], beta N(0, 0.3)"""
    g = rng(seed)
    M = g.standard_normal((rows, 128))
    kind = np.arange(rows) % 8
    ratio = np.select([kind == 1, kind == 2, kind == 3, kind == 4], [100.0, 300.0, 1000.0, 3000.0], 0.0)
    M = M + (ratio * np.where(g.random(rows) < 0.5, -1, 1))[:, None]
    small = (kind == 5) | (kind == 6)
    M[small] *= np.where(kind[small] == 5, 1e-3, 1e-2)[:, None]
    gamma = (0.5 + g.random(128)) * np.where(g.random(128) < 0.5, -1, 1)
    beta = 0.3 * g.standard_normal(128)
    return M.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32)


# =====================================================================================================================
# attention (attention128.hip) in float64, with the magnitudes the tolerances need
# =====================================================================================================================
def attention_truth(q, k, v, mask=None):
    """q [B, Lq, 128], k [B, Lk, 128], v [B, Lk, C] float64, mask [B or 1, Lq, Lk] additive -> dict(o, pv = sum p |v|, pd = sum p |v - o|,
    qk = max over keys of sum |q||k| / sqrt(128), gap = best logit - second best)"""
    q, k, v = (torch.from_numpy(np.ascontiguousarray(t, np.float64)) for t in (q, k, v))
    s = q @ k.transpose(1, 2) / 128 ** 0.5
    if mask is not None:
        s = s + torch.from_numpy(np.ascontiguousarray(mask, np.float64))
    p = torch.softmax(s, -1)
    o = p @ v
    pv = p @ v.abs()
    pd = torch.zeros_like(o)
    for b in range(q.shape[0]):                              # one [Lq, Lk] temporary per column, not [Lq, Lk, C]
        for c in range(v.shape[2]):
            pd[b, :, c] = (p[b] * (v[b, :, c][None, :] - o[b, :, c][:, None]).abs()).sum(1)
    qk = (q.abs() @ k.abs().transpose(1, 2)).amax(-1, keepdim=True) / 128 ** 0.5
    top = torch.topk(s, 2, -1).values if s.shape[-1] > 1 else None
    return dict(o=o.numpy(), pv=pv.numpy(), pd=pd.numpy(), qk=qk.numpy(), gap=None if top is None else (top[..., 0] - top[..., 1]).numpy())


def attention_tolerance(t, split: bool, pv_split: bool):
    """P V: BUDGET[SPLIT16] sum p |v| where P and V are hi + lo pairs, BUDGET[F16] sum p |v| where they are single fp16; scores: a logit is off
    by at most ds = 2^-21 (split q, k) or 2^-10 (fp16 q, k) of sum |q||k| / sqrt(128), which moves the row by at most 2 ds sum p |v - o|"""
    ds = (2.0 ** -21 if split else 2.0 ** -10) * t["qk"]
    return BUDGET[SPLIT16 if pv_split else F16] * t["pv"] + 2 * ds * t["pd"]


def attention_data(seed: int, B: int, L: int, vcols: int):
    g = rng(seed)
    q = (g.standard_normal((B, L, 128)) * 1.5).astype(np.float32)
    k = (g.standard_normal((B, L, 128)) * 1.5).astype(np.float32)
    v = (g.standard_normal((B, L, vcols)) * (40.0 if vcols == 32 else 1.0)).astype(np.float32)
    return q, k, v


def spiked(q, k, gap: float = 80.0):
    """every query i of every batch element is made a multiple of key (7 i + 3) % L, its logit `gap`: the other keys stay ~60 below"""
    q = q.copy()
    L = q.shape[1]
    j = (7 * np.arange(L) + 3) % L
    kk = k[:, j].astype(np.float64)
    q[:] = (kk * (gap * 128 ** 0.5 / (kk * kk).sum(-1, keepdims=True))).astype(np.float32)
    return q, j


# =====================================================================================================================
# chains
# =====================================================================================================================
def window_data(seed: int, images: int, h8: int, w8: int):
    """Y [images P, 384] = q | k | v (q, k N(0, 1.5): logits of a few units, so masked and partner keys matter), X, gamma, beta"""
    g = rng(seed)
    R = images * h8 * w8
    Y = g.standard_normal((R, 384)) * np.r_[np.full(256, 1.5), np.full(128, 1.0)]
    X = g.standard_normal((R, 128))
    gamma = (0.5 + g.random(128)) * np.where(g.random(128) < 0.5, -1, 1)
    beta = 0.3 * g.standard_normal(128)
    return Y.astype(np.float32), X.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32)


def window_truth(Y, h8, w8, images, shifted, cross):
    """the reference's single_head_split_window_attention on float64 tensors: [images, P, 128] in token order"""
    P = h8 * w8
    y = torch.from_numpy(np.asarray(Y, np.float64)).view(images, P, 384)
    q, k, v = y[..., :128], y[..., 128:256], y[..., 256:]
    if cross:
        idx = torch.arange(images) ^ 1
        k, v = k[idx], v[idx]
    mask = G.shift_mask(h8, w8, h8 // 2, w8 // 2).double() if shifted else None
    return G.window_attention(q.contiguous(), k.contiguous(), v.contiguous(), 2, bool(shifted), h8, w8, mask).numpy()


def window_restated(Y, h8, w8, images, shifted, cross, bug=None):
    """the kernels' own route in float64: gather window rows (win_rows), region ids -> mask, partner window bw ^ 4, scatter back.
    Returns (o [images P, 128] in token order, the attention magnitudes gathered the same way).  bugs: win_rows' and regions_restated's,
    'no_partner' (cross attention reads its own image)"""
    Y = np.asarray(Y, np.float64)
    rows = win_rows(h8, w8, images, shifted, bug)
    q, k, v = Y[rows, :128], Y[rows, 128:256], Y[rows, 256:]
    if cross and bug != "no_partner":
        idx = np.arange(images * 4) ^ 4
        k, v = k[idx], v[idx]
    mask = np.tile(region_mask(regions_restated(h8, w8, bug)), (images, 1, 1)) if shifted else None
    t = attention_truth(q, k, v, mask)
    out = {}
    for name in ("o", "pv", "pd", "qk"):
        a = np.broadcast_to(t[name], t["o"].shape)
        tok = np.empty((images * h8 * w8, 128))
        tok[rows.reshape(-1)] = a.reshape(-1, 128)
        out[name] = tok
    out["masked_share"] = None if mask is None else (mask[:4] != 0).mean((1, 2))
    return out


def window_block_truth(o, X, gamma, beta):
    return np.asarray(X, np.float64) + ln_truth(o, gamma, beta)[0]


def window_block_tolerance(t, X, gamma, beta, split: bool = True):
    """the attention's tolerance (pv_single: P and V single fp16) pushed through the LayerNorm's derivative
    dy = gamma / s (do - mean(do) - d (d . do) / (128 s^2)): |dy| <= |gamma| / s (|do| + (1 + z) max_row |do|); plus gm_ln's own error on its
    input and the fp32 add X + y"""
    to = attention_tolerance(t, split, False)
    y, mean, se = ln_truth(t["o"], gamma, beta)
    z = np.abs(t["o"] - mean) / se
    through = np.abs(np.asarray(gamma, np.float64)) / se * (to + (1 + z) * to.max(-1, keepdims=True))
    return through + ln_tolerance(t["o"], gamma, beta) + U24 * np.abs(np.asarray(X, np.float64) + y)


def match_tokens(seed: int, NP: int, h8: int, w8: int, scale: float = 1.0):
    """tokens [2 NP, P, 128]: frame 1 of a pair holds frame 0's tokens with neighbours swapped (x <-> x ^ 1 in even pairs, y <-> y ^ 1 in
    odd ones: every token has its match, one pixel away) plus noise, so the softmax peaks one pixel away (p ~ 0.98 at scale 1) and the
    rest of the mass pulls towards the centre: flows of about a pixel under coordinates of tens"""
    g = rng(seed)
    P = h8 * w8
    y, x = np.divmod(np.arange(P), w8)
    out = np.empty((2 * NP, P, 128), np.float32)
    for n in range(NP):
        f0 = g.standard_normal((P, 128))
        f0 *= scale * 128 ** 0.5 / np.linalg.norm(f0, axis=1, keepdims=True)        # one norm: every token's own logit is 11.3 scale^2
        src = (y ^ 1) * w8 + x if n & 1 else y * w8 + (x ^ 1)
        out[2 * n] = f0
        out[2 * n + 1] = f0[src] + 0.1 * scale * g.standard_normal((P, 128))
    return out


def batch_images(NP: int, dirs: int):
    """(query image, key image) of every batch element of the matching as the engine orders them"""
    if dirs == 2:
        b = np.arange(2 * NP)
        return b, b ^ 1
    return np.arange(NP) * 2, np.arange(NP) * 2 + 1


def coords(h8, w8):
    t = np.arange(h8 * w8)
    return np.stack([t % w8, t // w8], -1).astype(np.float64)


def match_truth_oracle(tok, h8, w8, dirs):
    """the reference's global_correlation_softmax on float64 maps, re-ordered to the engine's batch order (pair-major): [B, P, 2]"""
    NP, P = tok.shape[0] // 2, h8 * w8
    t = torch.from_numpy(np.asarray(tok, np.float64)).view(NP, 2, h8, w8, 128).permute(0, 1, 4, 2, 3)
    grid32 = G.coords_grid
    G.coords_grid = lambda b, h, w: grid32(b, h, w).double()       # (its .float() grid would not multiply a float64 softmax)
    try:
        f = G.global_correlation_softmax(t[:, 0].contiguous(), t[:, 1].contiguous(), dirs == 2)        # [dirs NP (direction-major), 2, h, w]
    finally:
        G.coords_grid = grid32
    f = f.view(dirs, NP, 2, P).permute(1, 0, 3, 2).reshape(NP * dirs, P, 2)
    return f.numpy()


def match_restated(tok, h8, w8, dirs, bug=None):
    """the engine's route in float64: batch element b reads queries of image qi[b], keys of image ki[b], V = coordinates, then the own
    coordinate comes off.  Returns (flow [B, P, 2], attention magnitudes).  bug 'own_xy': the own coordinate swapped"""
    tok = np.asarray(tok, np.float64)
    qi, ki = batch_images(tok.shape[0] // 2, dirs)
    c = coords(h8, w8)
    t = attention_truth(tok[qi], tok[ki], np.broadcast_to(c, (len(qi),) + c.shape))
    own = c[:, ::-1] if bug == "own_xy" else c
    return t["o"] - own[None], t


def match_tolerance(t, h8, w8, split: bool = True):
    """the expected coordinate is good to 2^-20 of the largest coordinate (split P V and the fp32 result), plus the score term; the own
    coordinate that comes off is an integer - the error stays what it was while the value shrinks to the flow"""
    ds = (2.0 ** -21 if split else 2.0 ** -10) * t["qk"]
    return 2.0 ** -20 * max(h8 - 1, w8 - 1) + 2 * ds * t["pd"]


def propagate_data(seed: int, NP: int, h8: int, w8: int):
    """q, k, X [2 NP, P, 128] (k close to q: a token attends to itself and a few others), flow [.., P, 2] of a few pixels"""
    g = rng(seed)
    P = h8 * w8
    q = g.standard_normal((2 * NP, P, 128))
    k = 0.6 * q + 0.8 * g.standard_normal((2 * NP, P, 128))
    X = g.standard_normal((2 * NP, P, 128))
    flow = 3.0 * g.standard_normal((2 * NP, P, 2))
    return q.astype(np.float32), k.astype(np.float32), X.astype(np.float32), flow.astype(np.float32)


def propagate_truth(q, k, flow, dirs):
    """FeatureFlowAttention's arithmetic, softmax(q k^T / sqrt(128)) flow, on float64: batch element b is image b (dirs 2) or 2 b (dirs 1)"""
    NP = q.shape[0] // 2
    im = np.arange(2 * NP) if dirs == 2 else np.arange(NP) * 2
    return attention_truth(np.asarray(q, np.float64)[im], np.asarray(k, np.float64)[im], np.asarray(flow, np.float64))
