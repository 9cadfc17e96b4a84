"""float64 restatements of the flow_gmflow band's local matching and local-window propagation (CPU only; a helper module of the tests).

Reference: bands/gmflow/matching.py:39-83 (local_correlation_softmax) and transformer.py:376-409 (forward_local_window_attn), pinned by
tests/golden/gmflow_local_ops.npz (the real functions' outputs, tools/make_gmflow_local_golden.py).  The restatements are plain gathers:
  matching     candidate j of token (x, y) is target token (x + dx, y + dy), dx = j % (2R + 1) - R the fast index; candidates outside the grid
               get -1e9 (probability exactly 0); flow = sum p (dx, dy).  The reference samples with grid_sample(align_corners=True) at
               coordinates that are integers up to fp32 round-off (a neighbour's weight <= 2^-22): the gather differs by that much.
  propagation  F.unfold zero-pads: a padded candidate has key 0 -> score exactly 0, flow 0, and it COUNTS in the softmax's denominator.
               q = q_proj(feature), k = k_proj(feature): the local form projects the key from the feature itself (transformer.py:389),
               unlike the global form's k_proj(q_proj(feature)) (:363-364).
Each takes a `bug=` name that plants one fault; tests/test_gm_local_ref_cpu.py asserts the tolerance sees every one of them.

Tolerance (local_tolerance), from the kernels' arithmetic (gmflow_local.hip), in the two-term form of gm_ref.attention_tolerance:
  score   one chain of 128 fp32 FMAs and the multiply by 1 / sqrt(128) (itself rounded): |ds| <= (128 + 2) 2^-24 sum |q||k| / sqrt(128);
          the exponential: expf is good to 1 ulp (2^-23 relative on p) and its argument s - max is rounded once, |s - max| <= 2 max_j
          sum |q||k_j| / sqrt(128), so EXP = 2^-23 + 2 2^-24 max sum |q||k| / sqrt(128).  Relative errors of at most ds on every p move
          o = sum p v / sum p by at most 2 ds sum p |v - o|.
  value   numerator and denominator are each a chain of at most (window + 3) / 4 + 2 adds (a lane's candidates, then two shuffles), the
          products are fused, one divide: (2 ((window + 3) / 4 + 2) + 1) 2^-24 sum p |v| <= (window + 2) 2^-24 sum p |v| for every window
          the kernels take (9, 25, 49, 81).
"""
from __future__ import annotations

import numpy as np

from gm_ref import batch_images
from raft_ref import U24, rng

# (name, corr_radius, prop_radius) of the end-to-end goldens
CONFIGS = [("c4", 4, -1), ("p1", -1, 1), ("c4p1", 4, 1), ("c1p2", 1, 2)]
SIZES = ["gmflow_local_125x157.npz", "gmflow_local_90x150.npz"]


def window(radius: int):
    """(dx, dy) of candidate j: generate_window_grid's order, x fast"""
    W = 2 * radius + 1
    dy, dx = np.divmod(np.arange(W * W), W)
    return dx - radius, dy - radius


def _gather(m, h8, w8, radius):
    """m [B, P, C] -> [B, P, window, C]: the (2 radius + 1)^2 neighbours of every token, zeros outside the grid; and valid [P, window]"""
    B, P, C = m.shape
    pad = np.zeros((B, h8 + 2 * radius, w8 + 2 * radius, C), m.dtype)
    pad[:, radius:radius + h8, radius:radius + w8] = m.reshape(B, h8, w8, C)
    dx, dy = window(radius)
    out = np.stack([pad[:, radius + b:radius + b + h8, radius + a:radius + a + w8].reshape(B, P, C) for a, b in zip(dx, dy)], 2)
    y, x = np.divmod(np.arange(P), w8)
    valid = (x[:, None] + dx >= 0) & (x[:, None] + dx < w8) & (y[:, None] + dy >= 0) & (y[:, None] + dy < h8)
    return out, valid


def _softmax_stats(s, v, qk):
    """s [B, P, n] scores, v [B, P, n, 2] values -> dict(o, pv = sum p |v|, pd = sum p |v - o|, qk)"""
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = (p[..., None] * v).sum(2)
    return dict(o=o, pv=(p[..., None] * np.abs(v)).sum(2), pd=(p[..., None] * np.abs(v - o[:, :, None])).sum(2), qk=qk)


def local_match_restated(tok, h8, w8, dirs, radius, bug=None):
    """tok [2 NP, P, 128] -> dict(o = flow [NP dirs, P, 2], pv, pd, qk): batch element (pair, dir) reads source image 2 pair + dir and the
    other image of the pair.  bugs: 'dxdy' (offsets swapped), 'no_mask', 'dir_swap' (dir 1 reads source and target swapped), 'no_scale'"""
    tok = np.asarray(tok, np.float64)
    qi, ki = batch_images(tok.shape[0] // 2, dirs)
    if bug == "dir_swap":
        odd = (qi & 1).astype(bool)
        qi, ki = np.where(odd, ki, qi), np.where(odd, qi, ki)
    q = tok[qi]
    kw, valid = _gather(tok[ki], h8, w8, radius)
    scale = 1.0 if bug == "no_scale" else 128 ** -0.5
    s = np.einsum("bpc,bpjc->bpj", q, kw) * scale
    qk = (np.einsum("bpc,bpjc->bpj", np.abs(q), np.abs(kw)) * 128 ** -0.5).max(-1)[..., None]
    if bug != "no_mask":
        s = np.where(valid[None], s, -1e9)
    dx, dy = window(radius)
    if bug == "dxdy":
        dx, dy = dy, dx
    v = np.broadcast_to(np.stack([dx, dy], -1).astype(np.float64), s.shape + (2,))
    return _softmax_stats(s, v, qk)


def local_prop_restated(q, k, flow, h8, w8, radius, bug=None):
    """q, k [B, P, 128], flow [B, P, 2] -> dict(o = propagated flow [B, P, 2], pv, pd, qk).  bugs: 'drop_pads' (zero pads left out of the
    softmax), 'dxdy' (the window transposed), 'no_scale'"""
    q, k, flow = (np.asarray(t, np.float64) for t in (q, k, flow))
    kw, valid = _gather(k, h8, w8, radius)
    fw, _ = _gather(flow, h8, w8, radius)
    if bug == "dxdy":
        W = 2 * radius + 1
        t = np.arange(W * W).reshape(W, W).T.reshape(-1)
        fw = fw[:, :, t]
    scale = 1.0 if bug == "no_scale" else 128 ** -0.5
    s = np.einsum("bpc,bpjc->bpj", q, kw) * scale
    qk = (np.einsum("bpc,bpjc->bpj", np.abs(q), np.abs(kw)) * 128 ** -0.5).max(-1)[..., None]
    if bug == "drop_pads":
        s = np.where(valid[None], s, -np.inf)
    return _softmax_stats(s, fw, qk)


def prop_qk(feat, wq, bq, wk, bk, bug=None):
    """feature [B, P, 128] -> (q, k) float64 of the local-window propagation: q = q_proj(feature), k = k_proj(feature).
    bug 'key_of_q': k = k_proj(q), the GLOBAL form's key carried over"""
    feat, wq, bq, wk, bk = (np.asarray(t, np.float64) for t in (feat, wq, bq, wk, bk))
    q = feat @ wq.T + bq
    return q, (q if bug == "key_of_q" else feat) @ wk.T + bk


def local_tolerance(t, radius: int, ds_inputs=0.0):
    """|kernel - float64| per element of the flow (module docstring); ds_inputs: what the operands' own error adds to a score"""
    n = (2 * radius + 1) ** 2
    ds = (128 + 2) * U24 * t["qk"] + 2.0 ** -23 + 2 * U24 * t["qk"] + ds_inputs
    return 2 * ds * t["pd"] + (n + 2) * U24 * t["pv"] + 1e-30


def projection_score_error(feat, wq, bq, wk, bk, h8, w8, radius):
    """the engine's q and k are split-fp16 GEMMs of the fp32 feature (three K segments, fp32 accumulation and store): an element is off
    by at most 2^-19 (sum |x||w| + |b|) - split_ref.BUDGET's 2^-20 of the products plus 2^-26 sqrt(384) for the accumulation and 2^-24
    for the store, rounded up.  Returns what that adds to a score: max over the window of (sum dq |k| + |q| dk) / sqrt(128), [B, P, 1]"""
    feat, wq, bq, wk, bk = (np.asarray(t, np.float64) for t in (feat, wq, bq, wk, bk))
    q, k = prop_qk(feat, wq, bq, wk, bk)
    dq = 2.0 ** -19 * (np.abs(feat) @ np.abs(wq).T + np.abs(bq))
    dk = 2.0 ** -19 * (np.abs(feat) @ np.abs(wk).T + np.abs(bk))
    kw, _ = _gather(np.abs(k), h8, w8, radius)
    dkw, _ = _gather(dk, h8, w8, radius)
    e = np.einsum("bpc,bpjc->bpj", dq, kw) + np.einsum("bpc,bpjc->bpj", np.abs(q), dkw)
    return (e * 128 ** -0.5).max(-1)[..., None]


# ---- data of the op-level tests: large common offsets, so that a cancellation shows ----
def match_tokens(seed: int, NP: int, h8: int, w8: int):
    """tokens [2 NP, P, 128]: random features on an offset of 1.5 per channel, negated on the odd channels of every second frame - each
    operand is mostly offset, while the common logit is ~0, so a candidate outside the grid (dot product exactly 0) would weigh in if it
    were not masked; frame 1 = frame 0 shifted by (+2, -1) tokens (wrapping) plus noise: the mass sits off-centre, and on the grid's
    border part of the window is masked"""
    g = rng(seed)
    P = h8 * w8
    sign = np.where(np.arange(128) & 1, -1.0, 1.0)
    out = np.empty((2 * NP, P, 128), np.float32)
    for n in range(NP):
        f0 = g.standard_normal((h8, w8, 128)) * 0.6
        f1 = np.roll(f0, (-1, 2), (0, 1)) + 0.3 * g.standard_normal((h8, w8, 128))
        out[2 * n], out[2 * n + 1] = (f0 + 1.5).reshape(P, 128), (f1 + 1.5 * sign).reshape(P, 128)
    return out


def prop_data(seed: int, images: int, h8: int, w8: int, B: int):
    """q, k [images, P, 128] (k close to q, both on a common offset: the zero pads' score of 0 then lies ~25 BELOW the real ones, where
    dropping them from the denominator would not show - so half the channels carry the offset negated and the common logit is ~0),
    flow_in [B, P, 2] = 40 px common motion + a few pixels"""
    g = rng(seed)
    P = h8 * w8
    sign = np.where(np.arange(128) & 1, -1.0, 1.0)
    q = g.standard_normal((images, P, 128)) * 0.8
    k = 0.5 * q + 0.6 * g.standard_normal((images, P, 128))
    q, k = q + 1.5, k + 1.5 * sign
    flow = np.array([40.0, -25.0]) + 3.0 * g.standard_normal((B, P, 2))
    return q.astype(np.float32), k.astype(np.float32), flow.astype(np.float32)


# ---- end to end on the CPU: oracle.gmflow_oracle's stages around the restatements ----
def gmflow_local_forward(w, img0, img1, corr: int, prop: int, bidir: bool = False):
    """GMFlow.forward with one scale and the two radii (gmflow.py:95-170) from oracle/gmflow_oracle.py's stages; img [1, 3, H, W] float
    0..255.  Local matching in both directions = source and target swapped (the reference's pred_bidir_flow raises there).
    Returns (up [dirs, 2, H, W], dict(tfeat [2, P, 128], flow_match, flow_prop [dirs, P, 2])) float32"""
    import torch
    from oracle import gmflow_oracle as G
    with torch.no_grad():
        mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        i0 = (torch.from_numpy(np.ascontiguousarray(img0)).float() / 255.0 - mean) / std
        i1 = (torch.from_numpy(np.ascontiguousarray(img1)).float() / 255.0 - mean) / std
        f0, f1 = G.backbone(w, torch.cat((i0, i1), 0)).chunk(2, 0)
        f0, f1 = G.add_position(f0, f1, 2)
        f0, f1 = G.feature_transformer(w, f0, f1, 2)
        _, c, h8, w8 = f0.shape
        dirs = 2 if bidir else 1
        tok = torch.cat((f0, f1), 0).flatten(-2).permute(0, 2, 1).numpy()                    # [2, P, 128]
        if corr < 0:
            fm = G.global_correlation_softmax(f0, f1, bidir).flatten(-2).permute(0, 2, 1).numpy()
        else:
            fm = local_match_restated(tok, h8, w8, dirs, corr)["o"]
        src = tok[:dirs]
        if prop < 0:
            fmap = torch.from_numpy(np.ascontiguousarray(fm, np.float32)).permute(0, 2, 1).reshape(dirs, 2, h8, w8)
            fp = G.flow_attention(w, torch.cat((f0, f1), 0)[:dirs], fmap).flatten(-2).permute(0, 2, 1).numpy()
        else:
            q, k = prop_qk(src, w["feature_flow_attn.q_proj.weight"], w["feature_flow_attn.q_proj.bias"], w["feature_flow_attn.k_proj.weight"],
                           w["feature_flow_attn.k_proj.bias"])
            fp = local_prop_restated(q, k, fm, h8, w8, prop)["o"]
        fpt = torch.from_numpy(np.ascontiguousarray(fp, np.float32)).permute(0, 2, 1).reshape(dirs, 2, h8, w8)
        up = G.upsample_flow(w, fpt, torch.cat((f0, f1), 0)[:dirs])
    return up.numpy(), dict(tfeat=tok, flow_match=np.asarray(fm, np.float32), flow_prop=np.asarray(fp, np.float32))
