"""float64 restatements of the steps the two-scale GMFlow (num_scales 2, upsample_factor 4) adds to the flow_gmflow band (CPU only; a helper
module of the tests), built on tests/gm_ref.py and tests/gm_local_ref.py.

Reference: bands/gmflow/gmflow.py:112-165 (the scale loop), backbone.py:58-64, 101-117 + trident_conv.py:64-72 (one 3 x 3 weight, stride 1
-> 1/4 features, stride 2 -> 1/8 features), gmflow.py:121-126 + geometry.py:41-72 (flow x 2, flow_warp), utils.py:66-86 and
transformer.py:19-101 with 8 splits, gmflow.py:74-90 with upsample_factor 4.  Pinned by tests/golden/gmflow_scale2_*.npz - the real
functions' and the real model's outputs (tools/make_gmflow_scale2_golden.py).

  enlarge2     F.interpolate(scale_factor = 2, bilinear, align_corners = True) * 2: output row y reads source row y (h - 1) / (2 h - 1)
  warp         grid_sample(bilinear, zeros, align_corners = True) at token + flow: the reference normalises the coordinate to [-1, 1] and
               grid_sample maps it back, an identity up to fp32 round-off of the coordinate; a tap outside the grid contributes zero
  upsample     softmax over the 9 logits of every sub-pixel, weights on factor * flow's zero-padded 3 x 3 neighbourhood
  positions_n / regions_n / win_rows_n / window_restated_n: gm_ref's tables and window route with the split count as an argument
  forward      the whole two-scale model from oracle/gmflow_oracle.py's stages (fp32 torch, already pinned to the real one-scale model)
               around the restatements
Each takes a `bug=` name that plants one fault; tests/test_gm_scale2_ref_cpu.py asserts the yardstick sees every one of them.

Tolerances of the two new kernels (gm_warp_kernel, upsample_kernel<4>), from their arithmetic, in the two-term form of
gm_local_ref.local_tolerance: a term for the error of the WEIGHTS times the spread of the values, a term for the accumulation.
  warp_tolerance      flow_up is a chain of 3 lerps (weights 1 - l, l with l = f - floor(f) of a coordinate f = scale * y <= h, rounded
                      twice: 4 2^-24 h absolute on l), two products and an add each, then the doubling: (8 + 2) 2^-24 |v|max of the four
                      taps for the arithmetic and 2 * 4 2^-24 (h + w) * spread of the four taps for the weights.
                      The sample position g = x + u carries the flow's error du and one rounding 2^-24 |g|; the fractions a = g - floor(g)
                      are exact after that (Sterbenz), the four weights are products of two such terms (3 roundings: 3 2^-24), the
                      accumulation is 4 FMAs (4 2^-24 sum w |v|): the value error is (du_x + du_y + 2^-24 (|gx| + |gy|)) * (the local
                      Lipschitz bound of the bilinear surface: the largest difference between the taps, zeros included) +
                      7 2^-24 sum w |v|.
  upsample_tolerance  the 9 logits are fp32 inputs; e = __expf(l - max) is good to 2 ulp of the result plus the argument's rounding
                      2^-24 |l - max| <= 2^-24 spread(l): EXP = 2^-22 + 2^-24 spread(l) relative on every weight, the denominator a chain
                      of 9 adds, each weight one divide; the value a chain of 9 FMAs of w * (factor * f) with factor * f exact (a power
                      of two): |d| <= 2 EXP sum p |v - o| + (9 + 9 + 2) 2^-24 sum p |v|.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import gm_local_ref as L
import gm_ref as R
from oracle import gmflow_oracle as G
from raft_ref import U24

# (H, W) of the end-to-end goldens and the fine scale's radii they hold
SIZES = [(64, 96), (96, 160), (100, 150)]
CONFIGS = {(64, 96): [(4, 1), (2, 2)], (96, 160): [(4, 1)], (100, 150): [(4, 1)]}
STAGES = ["feat", "feat4", "tfeat", "flow_prop", "flow_up", "warp", "block0_4", "tfeat4", "flow_match4", "flow_prop4"]
# stage tensors on the 1/4 grid with 128 channels are stored on this many seeded tokens per image (the fixtures stay below 1 MB)
SUBSET = 64


def golden_name(hw):
    return "gmflow_scale2_%dx%d.npz" % tuple(hw)


def padded(hw, factor=32):
    return tuple(-(-v // factor) * factor for v in hw)


def token_subset(P4: int, seed: int = 2024):
    """the seeded, sorted token subset the fixtures keep of a [.., P4, 128] stage"""
    return np.sort(np.random.default_rng(seed).choice(P4, size=min(SUBSET, P4), replace=False))


# =====================================================================================================================
# the step between the scales
# =====================================================================================================================
def enlarge2_restated(flow8, h8, w8, bug=None):
    """flow8 [B, h8 w8, 2] -> dict(o [B, 4 h8 w8, 2], vmax, spread [B, 4 h8 w8, 1]).  bugs: 'not_doubled', 'align_false'"""
    f = np.asarray(flow8, np.float64).reshape(-1, h8, w8, 2)
    h4, w4 = 2 * h8, 2 * w8

    def src(n_in, n_out):
        o = np.arange(n_out, dtype=np.float64)
        s = np.maximum((o + 0.5) * n_in / n_out - 0.5, 0.0) if bug == "align_false" else o * (n_in - 1) / (n_out - 1)
        i0 = np.minimum(np.floor(s).astype(int), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0
    y0, y1, ly = src(h8, h4)
    x0, x1, lx = src(w8, w4)
    taps = [f[:, y0][:, :, x0], f[:, y0][:, :, x1], f[:, y1][:, :, x0], f[:, y1][:, :, x1]]
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    o = (1 - ly) * ((1 - lx) * taps[0] + lx * taps[1]) + ly * ((1 - lx) * taps[2] + lx * taps[3])
    o = o * (1.0 if bug == "not_doubled" else 2.0)
    st = np.stack(taps)
    B = f.shape[0]
    return dict(o=o.reshape(B, h4 * w4, 2), vmax=np.abs(st).max((0, -1)).reshape(B, h4 * w4, 1),
                spread=(st.max(0) - st.min(0)).max(-1).reshape(B, h4 * w4, 1))


def enlarge2_tolerance(t, h8, w8):
    return 10 * U24 * 2 * t["vmax"] + 2 * 4 * U24 * (2 * h8 + 2 * w8) * 2 * t["spread"] + 1e-30


def warp_restated(feat, flow, h4, w4, bug=None):
    """feat [B, h4 w4, C] (the target's features), flow [B, h4 w4, 2] -> dict(o [B, h4 w4, C], wv = sum w |v|, lip = the largest difference
    between two of the four taps (zeros included) per channel, g = |gx| + |gy|, outside = a tap of the token fell outside the grid).
    bug 'border': taps clamped to the grid instead of zeros"""
    feat, flow = np.asarray(feat, np.float64), np.asarray(flow, np.float64)
    B, P, C = feat.shape
    y, x = np.divmod(np.arange(P), w4)
    gx, gy = x[None] + flow[..., 0], y[None] + flow[..., 1]
    if bug == "border":
        gx, gy = np.clip(gx, 0, w4 - 1), np.clip(gy, 0, h4 - 1)
    fx, fy = np.floor(gx), np.floor(gy)
    ax, ay = gx - fx, gy - fy
    o, wv = np.zeros((B, P, C)), np.zeros((B, P, C))
    lo, hi = np.full((B, P, C), np.inf), np.full((B, P, C), -np.inf)
    outside = np.zeros((B, P), bool)
    bi = np.arange(B)[:, None]
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = (fy + dy).astype(np.int64), (fx + dx).astype(np.int64)
            ok = (yy >= 0) & (yy < h4) & (xx >= 0) & (xx < w4)
            wgt = (ay if dy else 1 - ay) * (ax if dx else 1 - ax)
            v = np.where(ok[..., None], feat[bi, np.clip(yy, 0, h4 - 1) * w4 + np.clip(xx, 0, w4 - 1)], 0.0)
            o += wgt[..., None] * v
            wv += wgt[..., None] * np.abs(v)
            lo, hi = np.minimum(lo, v), np.maximum(hi, v)
            outside |= ~ok
    return dict(o=o, wv=wv, lip=hi - lo, g=(np.abs(gx) + np.abs(gy))[..., None], outside=outside)


def warp_tolerance(t, dflow):
    """dflow: the absolute error of the flow the kernel sampled at, per token [B, P, 1] or a scalar (module docstring)"""
    return (2 * np.asarray(dflow) + U24 * t["g"]) * t["lip"] + 7 * U24 * t["wv"] + 1e-30


def between_scales(flow8, feat4_target, h8, w8, bug=None):
    """(flow_up, warped) of gmflow.py:121-126 for flow8 [B, h8 w8, 2] and the target's 1/4 features [B, 4 h8 w8, 128]"""
    up = enlarge2_restated(flow8, h8, w8, bug)
    return up, warp_restated(feat4_target, up["o"], 2 * h8, 2 * w8, bug)


# =====================================================================================================================
# convex upsampling with the factor
# =====================================================================================================================
def upsample_restated(flow, logits, h, w, factor, bug=None):
    """flow [n, h w, 2], logits [n, h w, 9 factor^2] (channel = k factor^2 + sy factor + sx) -> dict(o [n, factor h, factor w, 2], pv, pd, spread
    [same, 1]).  bug 'times8': the neighbourhood scaled by 8 whatever the factor"""
    flow, logits = np.asarray(flow, np.float64), np.asarray(logits, np.float64)
    n = flow.shape[0]
    f = factor
    l = logits.reshape(n, h, w, 9, f, f)
    p = np.exp(l - l.max(3, keepdims=True))
    p /= p.sum(3, keepdims=True)
    pad = np.zeros((n, h + 2, w + 2, 2))
    pad[:, 1:-1, 1:-1] = flow.reshape(n, h, w, 2) * (8.0 if bug == "times8" else f)
    v = np.stack([pad[:, k // 3:k // 3 + h, k % 3:k % 3 + w] for k in range(9)], 3)            # [n, h, w, 9, 2]
    o = np.einsum("nhwkab,nhwkc->nhwabc", p, v)                                                 # [n, h, w, sy, sx, 2]
    pv = np.einsum("nhwkab,nhwkc->nhwabc", p, np.abs(v))
    pd = np.einsum("nhwkabc->nhwabc", p[..., None] * np.abs(v[:, :, :, :, None, None] - o[:, :, :, None]))
    sp = (l.max(3) - l.min(3))[..., None]
    fold = lambda a: a.transpose(0, 1, 3, 2, 4, 5).reshape(n, f * h, f * w, a.shape[-1])
    return dict(o=fold(o), pv=fold(pv), pd=fold(pd), spread=fold(sp))


def upsample_tolerance(t):
    return 2 * (2.0 ** -22 + U24 * t["spread"]) * t["pd"] + 20 * U24 * t["pv"] + 1e-30


# =====================================================================================================================
# the host tables and the window route with the split count
# =====================================================================================================================
def positions_n(h, w, splits):
    """gm_ref.positions_truth for splits x splits windows: (pos [P, 128] float64, the sin / cos arguments)"""
    wh, ww = h // splits, w // splits
    i = np.arange(64)
    dim_t = 10000.0 ** (2.0 * (i // 2) / 64.0)
    ye = ((np.arange(h) % wh + 1) / (wh + 1e-6) * 2 * np.pi)[:, None, None] / dim_t
    xe = ((np.arange(w) % ww + 1) / (ww + 1e-6) * 2 * np.pi)[None, :, None] / dim_t
    arg = np.concatenate([np.broadcast_to(ye, (h, w, 64)), np.broadcast_to(xe, (h, w, 64))], 2).reshape(h * w, 128)
    odd = (np.arange(128) & 1).astype(bool)
    return np.where(odd, np.cos(arg), np.sin(arg)), arg


def regions_n(h, w, splits, bug=None):
    """shift_regions restated for splits x splits windows: ids [splits^2, Lw] int8 in window order.  bug 'region_edge': a boundary one late"""
    wh, ww = h // splits, w // splits
    o = 1 if bug == "region_edge" else 0
    ry, rx = np.arange(h), np.arange(w)
    cy = np.where(ry < h - wh, 0, np.where(ry < h - wh // 2 + o, 1, 2))
    cx = np.where(rx < w - ww, 0, np.where(rx < w - ww // 2 + o, 1, 2))
    img = (cy[:, None] * 3 + cx[None, :]).reshape(splits, wh, splits, ww).transpose(0, 2, 1, 3)
    return img.reshape(splits * splits, wh * ww).astype(np.int8)


def win_rows_n(h, w, splits, images, shifted, bug=None):
    """the kernels' win_row for splits x splits windows: [images splits^2, Lw] -> row of the [images P] token matrix.  bug 'wywx'"""
    wh, ww, P, nw = h // splits, w // splits, h * w, splits * splits
    sy, sx = (wh // 2, ww // 2) if shifted else (0, 0)
    bw = np.arange(images * nw)
    img, wy, wx = bw // nw, (bw % nw) // splits, bw % splits
    if bug == "wywx":
        wy, wx = wx, wy
    ly, lx = np.divmod(np.arange(wh * ww), ww)
    gy = (wy[:, None] * wh + ly[None, :] + sy) % h
    gx = (wx[:, None] * ww + lx[None, :] + sx) % w
    return img[:, None] * P + gy * w + gx


def win_rows_oracle_n(h, w, splits, images, shifted):
    wh, ww = h // splits, w // splits
    t = torch.arange(images * h * w).view(images, h, w, 1)
    if shifted:
        t = torch.roll(t, shifts=(-(wh // 2), -(ww // 2)), dims=(1, 2))
    return G.split_windows(t, splits).reshape(images * splits * splits, wh * ww).numpy()


def window_truth_n(Y, h, w, splits, images, shifted, cross):
    """the reference's single_head_split_window_attention on float64 tensors with `splits`: [images, P, 128] in token order"""
    P = h * w
    y = torch.from_numpy(np.asarray(Y, np.float64)).view(images, P, 384)
    q, k, v = y[..., :128], y[..., 128:256], y[..., 256:]
    if cross:
        idx = torch.arange(images) ^ 1
        k, v = k[idx], v[idx]
    mask = G.shift_mask(h, w, h // splits, w // splits).double() if shifted else None
    return G.window_attention(q.contiguous(), k.contiguous(), v.contiguous(), splits, bool(shifted), h, w, mask).numpy()


def window_restated_n(Y, h, w, splits, images, shifted, cross, bug=None):
    """gm_ref.window_restated with the split count: gather window rows, region ids -> mask, partner window bw ^ splits^2, scatter back"""
    Y = np.asarray(Y, np.float64)
    nw = splits * splits
    rows = win_rows_n(h, w, splits, images, shifted, bug)
    q, k, v = Y[rows, :128], Y[rows, 128:256], Y[rows, 256:]
    if cross and bug != "no_partner":
        idx = np.arange(images * nw) ^ nw
        k, v = k[idx], v[idx]
    mask = np.tile(R.region_mask(regions_n(h, w, splits, bug)), (images, 1, 1)) if shifted else None
    t = R.attention_truth(q, k, v, mask)
    out = {}
    for name in ("o", "pv", "pd", "qk"):
        a = np.broadcast_to(t[name], t["o"].shape)
        tok = np.empty((images * h * w, 128))
        tok[rows.reshape(-1)] = a.reshape(-1, 128)
        out[name] = tok
    return out


def window_block_tolerance_n(t, X, gamma, beta, pv_split: bool):
    """gm_ref.window_block_tolerance with the attention's P V term as the kernel is launched: pv_split True is the two-scale model's window
    attention (P and V as hi + lo pairs: BUDGET[SPLIT16] sum p |v| instead of BUDGET[F16] sum p |v|, gm_ref.attention_tolerance), pushed
    through the LayerNorm's derivative the same way, plus gm_ln's own error and the fp32 add"""
    to = R.attention_tolerance(t, True, pv_split)
    y, mean, se = R.ln_truth(t["o"], gamma, beta)
    z = np.abs(t["o"] - mean) / se
    through = np.abs(np.asarray(gamma, np.float64)) / se * (to + (1 + z) * to.max(-1, keepdims=True))
    return through + R.ln_tolerance(t["o"], gamma, beta) + U24 * np.abs(np.asarray(X, np.float64) + y)


# =====================================================================================================================
# the whole two-scale model on the CPU: oracle.gmflow_oracle's stages around the restatements
# =====================================================================================================================
def backbone2(w, x, bug=None):
    """CNNEncoder.forward with num_output_scales = 2 (backbone.py:101-117): layer3 at stride 1, conv2, and the one trident weight at stride 1
    (1/4) and 2 (1/8).  Returns (feat8, feat4).  bug 'trident_swapped': the two strides' outputs taken for each other's scale (each
    resampled to the other's grid so the shapes still fit)"""
    x = torch.relu(G._inorm(F.conv2d(x, G._t(w, "backbone.conv1.weight"), None, 2, 3)))
    for li, stride in ((1, 1), (2, 2), (3, 1)):
        x = G.residual_block(w, f"backbone.layer{li}.0.", x, stride)
        x = G.residual_block(w, f"backbone.layer{li}.1.", x, 1)
    x = F.conv2d(x, G._t(w, "backbone.conv2.weight"), G._t(w, "backbone.conv2.bias"))
    tw = G._t(w, "backbone.trident_conv.weight")
    f4, f8 = F.conv2d(x, tw, None, 1, 1), F.conv2d(x, tw, None, 2, 1)
    if bug == "trident_swapped":
        f4, f8 = F.interpolate(f8, scale_factor=2, mode="nearest"), f4[:, :, ::2, ::2].contiguous()
    return f8, f4


def _tok(t):
    return t.flatten(-2).permute(0, 2, 1).numpy()


def _map(a, h, w):
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(a).permute(0, 2, 1).reshape(a.shape[0], a.shape[2], h, w).contiguous()


def forward(w, img0, img1, corr: int, prop: int, bug=None):
    """GMFlow(num_scales=2, upsample_factor=4).forward(attn_splits_list=[2, 8], corr_radius_list=[-1, corr], prop_radius_list=[-1, prop]) for
    one pair (gmflow.py:92-170); img [1, 3, H, W] float 0..255, H and W multiples of 32.  Returns (up [2, H, W] float32, stages as the engine
    names them, token-major float32: feat / feat4 [2, P, 128], tfeat [2, P8, 128], flow_prop [1, P8, 2], flow_up, flow_match4, flow_prop4
    [1, P4, 2], warp [1, P4, 128], block0_4 / tfeat4 [2, P4, 128]).
    bugs: enlarge2's, warp's, 'warp_feature0', 'coarse_windows' (splits 2 at the fine scale), 'coarse_positions' (the 2-split position
    table at the fine scale), 'no_residual', 'times8', 'trident_swapped'"""
    st = {}
    with torch.no_grad():
        mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        i0 = (torch.from_numpy(np.ascontiguousarray(img0)).float() / 255.0 - mean) / std
        i1 = (torch.from_numpy(np.ascontiguousarray(img1)).float() / 255.0 - mean) / std
        f8, f4 = backbone2(w, torch.cat((i0, i1), 0), bug)
        st["feat"], st["feat4"] = _tok(f8), _tok(f4)
        _, c, h8, w8 = f8.shape
        h4, w4 = 2 * h8, 2 * w8
        # coarse scale: the one-scale model's own stages
        a, b = f8.chunk(2, 0)
        a, b = G.add_position(a, b, 2)
        a, b = G.feature_transformer(w, a, b, 2)
        st["tfeat"] = _tok(torch.cat((a, b), 0))
        flow = G.flow_attention(w, a, G.global_correlation_softmax(a, b, False))
        st["flow_prop"] = _tok(flow)
        # between the scales
        s4, t4 = f4.chunk(2, 0)
        up, wp = between_scales(st["flow_prop"], _tok(s4 if bug == "warp_feature0" else t4), h8, w8, bug)
        st["flow_up"], st["warp"] = up["o"].astype(np.float32), wp["o"].astype(np.float32)
        # fine scale
        a, b = s4, _map(st["warp"], h4, w4)
        a, b = G.add_position(a, b, 2 if bug == "coarse_positions" else 8)
        stages = {}
        a, b = G.feature_transformer(w, a, b, 2 if bug == "coarse_windows" else 8, stages=stages)
        st["block0_4"] = stages["block0"].numpy()
        tok = _tok(torch.cat((a, b), 0))
        st["tfeat4"] = tok
        res = L.local_match_restated(tok, h4, w4, 1, corr)["o"]
        fm = st["flow_up"].astype(np.float64) + (0.0 if bug == "no_residual" else res)
        st["flow_match4"] = fm.astype(np.float32)
        q, k = L.prop_qk(tok[:1], w["feature_flow_attn.q_proj.weight"], w["feature_flow_attn.q_proj.bias"], w["feature_flow_attn.k_proj.weight"],
                         w["feature_flow_attn.k_proj.bias"])
        fp = L.local_prop_restated(q, k, st["flow_match4"], h4, w4, prop)["o"]
        st["flow_prop4"] = fp.astype(np.float32)
        # convex upsampling by 4: the upsampler's two convolutions from the oracle's arithmetic, the combination restated
        x = torch.relu(F.conv2d(torch.cat((_map(st["flow_prop4"], h4, w4), a), 1), G._t(w, "upsampler.0.weight"), G._t(w, "upsampler.0.bias"), 1, 1))
        logits = _tok(F.conv2d(x, G._t(w, "upsampler.2.weight"), G._t(w, "upsampler.2.bias")))
        out = upsample_restated(st["flow_prop4"], logits, h4, w4, 4, bug)["o"][0]
    return np.ascontiguousarray(out.transpose(2, 0, 1), np.float32), st


def pad_pair(fr, factor=32):
    """frames [2, H, W, 3] uint8 -> (img0, img1 [1, 3, Hp, Wp] float32 replicate-padded as InputPadder(factor) does, pad [l, r, t, b])"""
    pad = G.pad_amounts(fr.shape[1], fr.shape[2], factor)
    t = torch.from_numpy(np.ascontiguousarray(fr)).permute(0, 3, 1, 2).float()
    t = F.pad(t, pad, mode="replicate")
    return t[:1].numpy(), t[1:].numpy(), pad


def unpad(up, pad):
    """[2, Hp, Wp] -> [H, W, 2]"""
    ht, wd = up.shape[-2:]
    return np.ascontiguousarray(up[:, pad[2]:ht - pad[3], pad[0]:wd - pad[1]].transpose(1, 2, 0))
