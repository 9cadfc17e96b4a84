#!/usr/bin/env python3
"""Write tests/golden/gmflow_scale2_*.npz from the REAL reference (build machine only: needs /root/reference, read-only).

  gmflow_scale2_ops.npz       small seeded inputs with the outputs of the real flow_warp (bands/gmflow/geometry.py:65-72), the x 2 enlargement
                              of gmflow.py:122, feature_add_position with 8 splits (utils.py:66-86, on a zero feature: the table itself),
                              generate_shift_window_attn_mask for 8 x 8 windows (transformer.py:19-44) and GMFlow.upsample_flow with
                              upsample_factor 4 (gmflow.py:74-90; its upsampler's logits are stored next to its output).  The flows are large
                              enough that some samples fall outside the grid.
  gmflow_scale2_<H>x<W>.npz   the real GMFlow(num_scales=2, upsample_factor=4) + InputPadder(32) on a seeded frame pair, called as
                              bands/flow_gmflow.py:84-89 calls it with --attn_splits_list 2 8 --corr_radius_list -1 R --prop_radius_list -1 r
                              and pred_bidir_flow: the final flow in both directions at (4, 1), the stages of tests/gm_scale2_ref.py STAGES in
                              the engine's layout and order (128-channel stages on a seeded token subset), on one size the forward flow at
                              (2, 2) as well, and the (name, shape) list of the state dict the synthetic weights were loaded into with
                              load_state_dict(strict=True).
Two conditions on the inputs are printed here and asserted by tests/test_gm_scale2_ref_cpu.py: the fine scale's matched residual exceeds
0.25 px of the 1/4 grid somewhere, and at least one warped token takes a zero from outside the grid.
Data only, float32 / int8.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "bands"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
from common.flow import InputPadder  # noqa: E402
from gmflow import gmflow as GM  # noqa: E402
from gmflow.geometry import flow_warp  # noqa: E402
from gmflow.transformer import generate_shift_window_attn_mask  # noqa: E402
from gmflow.utils import feature_add_position  # noqa: E402

import gm_scale2_ref as S  # noqa: E402
from prisma_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
GRIDS4 = [(16, 24), (24, 40)]          # 1/4 grids: 8 x 8 windows of 2 x 3 (the smallest) and 3 x 5 (odd, shifts 1 and 2) tokens
# (seed, shift per frame in px) of the frame pairs: chosen so that the reference meets the two conditions of the module docstring
PAIRS = {(64, 96): (71, (6.0, -4.0)), (96, 160): (72, (-7.0, 5.0)), (100, 150): (73, (5.0, 6.0))}


def tok(t):
    return t.flatten(-2).permute(0, 2, 1).numpy().astype(np.float32)


def model():
    w = synth.gmflow_weights(seed=2468, num_scales=2)
    m = GM.GMFlow(feature_channels=128, num_scales=2, upsample_factor=4, num_head=1, attention_type="swin", ffn_dim_expansion=4,
                  num_transformer_layers=6).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return m, w


def ops(m):
    keep = {}
    g = np.random.default_rng(311)
    for h4, w4 in GRIDS4:
        tag = "%dx%d" % (h4, w4)
        h8, w8 = h4 // 2, w4 // 2
        feat = g.standard_normal((2, 8, h4, w4)).astype(np.float32)                  # (8 channels: the warp treats every channel alike)
        flow8 = (np.array([3.0, -2.0])[None, :, None, None] + 2.5 * g.standard_normal((2, 2, h8, w8))).astype(np.float32)
        with torch.no_grad():
            up = F.interpolate(torch.from_numpy(flow8), scale_factor=2, mode="bilinear", align_corners=True) * 2
            wp = flow_warp(torch.from_numpy(feat), up)
            z = torch.zeros(1, 128, h4, w4)
            pos = feature_add_position(z, z, 8, 128)[0]
            mask = generate_shift_window_attn_mask((h4, w4), h4 // 8, w4 // 8, h4 // 8 // 2, w4 // 8 // 2, device=torch.device("cpu"))
        gx = np.arange(w4)[None, None] + up[:, 0].numpy()
        gy = np.arange(h4)[None, :, None] + up[:, 1].numpy()
        n_out = int(((gx < 0) | (gx > w4 - 1) | (gy < 0) | (gy > h4 - 1)).sum())
        print("[gmflow_scale2_ops %s] %d of %d samples outside the grid" % (tag, n_out, gx.size))
        assert n_out > 0
        keep.update({"feat_" + tag: tok(torch.from_numpy(feat)), "flow8_" + tag: tok(torch.from_numpy(flow8)), "up_" + tag: tok(up),
                     "warp_" + tag: tok(wp), "pos_" + tag: tok(pos)[0], "mask_" + tag: mask.numpy().astype(np.int8)})
    # the factor-4 convex upsampling on the small grid, one sample (144 logits per token)
    h4, w4 = GRIDS4[0]
    flow4 = (np.array([-6.0, 9.0])[None, :, None, None] + 3.0 * g.standard_normal((1, 2, h4, w4))).astype(np.float32)
    f4 = g.standard_normal((1, 128, h4, w4)).astype(np.float32)
    with torch.no_grad():
        logits = m.upsampler(torch.cat((torch.from_numpy(flow4), torch.from_numpy(f4)), 1))
        out = m.upsample_flow(torch.from_numpy(flow4), torch.from_numpy(f4))
    keep.update({"flow4": tok(torch.from_numpy(flow4)), "logits": tok(logits), "ups": out.permute(0, 2, 3, 1).numpy().astype(np.float32)})
    keep["grids"] = np.array(GRIDS4)
    out = os.path.join(GOLD, "gmflow_scale2_ops.npz")
    np.savez_compressed(out, **keep)
    print("[gmflow_scale2_ops] %d bytes" % os.path.getsize(out))
    assert os.path.getsize(out) < 1000000


def run(m, a, c, corr, prop, bidir):
    """the real two-scale GMFlow on a padded pair -> (flow_up [B, 2, H, W], stages in the engine's layout) with the stages caught where
    forward makes them.  Fine-scale batches come as [fwd, bwd]; streams of both frames are re-ordered to (b, source / target)."""
    st = {}
    real_warp, real_local = GM.flow_warp, GM.local_correlation_softmax
    calls = {"tr": 0, "ffa": 0, "blk": 0}

    def warp(feature, flow, *args, **kw):
        out = real_warp(feature, flow, *args, **kw)
        st["flow_up"], st["warp"] = tok(flow), tok(out)
        return out

    def local(*args, **kw):
        out = real_local(*args, **kw)
        st["residual"] = tok(out[0])
        return out

    def inter(a0, a1):
        """[B .. of frame 0], [B .. of frame 1] -> [(b, e)]"""
        return np.stack([a0, a1], 1).reshape((-1,) + a0.shape[1:])

    def on_backbone(mod, i, o):          # high to low resolution, both frames
        st["feat4"], st["feat"] = tok(o[0]), tok(o[1])

    def on_transformer(mod, i, o):
        st["tfeat" if calls["tr"] == 0 else "tfeat4"] = inter(tok(o[0]), tok(o[1]))
        calls["tr"] += 1

    def on_block0(mod, i, o):            # [2 B, L, C] = [frame 0 of every b, frame 1 of every b]
        if calls["blk"] == 1:
            x = o.numpy().astype(np.float32)
            st["block0_4"] = inter(x[:x.shape[0] // 2], x[x.shape[0] // 2:])
        calls["blk"] += 1

    def on_ffa(mod, i, o):
        st["flow_prop" if calls["ffa"] == 0 else "flow_prop4"] = tok(o)
        calls["ffa"] += 1

    hooks = [m.backbone.register_forward_hook(on_backbone), m.transformer.register_forward_hook(on_transformer),
             m.transformer.layers[0].register_forward_hook(on_block0), m.feature_flow_attn.register_forward_hook(on_ffa)]
    GM.flow_warp, GM.local_correlation_softmax = warp, local
    try:
        with torch.no_grad():
            up = m(a, c, attn_splits_list=[2, 8], corr_radius_list=[-1, corr], prop_radius_list=[-1, prop], pred_bidir_flow=bidir)["flow_preds"][-1]
    finally:
        for h in hooks:
            h.remove()
        GM.flow_warp, GM.local_correlation_softmax = real_warp, real_local
    st["flow_match4"] = st["flow_up"] + st["residual"]
    return up, st


def pair(m, w, hgt, wid):
    seed, shift = PAIRS[(hgt, wid)]
    fr = synth.frame_pair_sequence(2, hgt, wid, seed=seed, shift=shift)
    a = torch.from_numpy(fr[0]).permute(2, 0, 1).float()[None]
    c = torch.from_numpy(fr[1]).permute(2, 0, 1).float()[None]
    padder = InputPadder(a.shape, padding_factor=32)
    pa, pc = padder.pad(a, c)
    Hp, Wp = pa.shape[-2:]
    assert (Hp, Wp) == S.padded((hgt, wid))
    unpad = lambda t: padder.unpad(t).permute(1, 2, 0).numpy().astype(np.float32)
    keep = dict(frame_seed=np.array(seed), frame_shift=np.array(shift), hw=np.array([hgt, wid]),
                names=np.array([k for k in w]), shapes=np.array([",".join(str(d) for d in w[k].shape) for k in w]))
    P4 = (Hp // 4) * (Wp // 4)
    sub8, sub4 = S.token_subset(P4 // 4), S.token_subset(P4)
    keep["sub8"], keep["sub4"] = sub8, sub4
    up, st = run(m, pa, pc, 4, 1, True)
    keep["fwd_c4p1"], keep["bwd_c4p1"] = unpad(up[0]), unpad(up[1])
    for name in S.STAGES:
        v = st[name]
        if v.shape[-1] == 128:
            v = v[:, sub8 if v.shape[1] == P4 // 4 else sub4]
        keep[name + "_c4p1"] = np.ascontiguousarray(v, np.float32)
    res = float(np.abs(st["residual"]).max())
    # a warped token takes a zero from outside the grid: its sample position has a tap outside
    h4, w4 = Hp // 4, Wp // 4
    fu = st["flow_up"].reshape(-1, h4, w4, 2)
    gx, gy = np.arange(w4)[None, None] + fu[..., 0], np.arange(h4)[None, :, None] + fu[..., 1]
    n_out = int(((np.floor(gx) < 0) | (np.floor(gx) + 1 > w4 - 1) | (np.floor(gy) < 0) | (np.floor(gy) + 1 > h4 - 1)).sum())
    print("[gmflow_scale2 %dx%d] padded %dx%d; |flow| max %.2f px; fine residual max %.3f px of the 1/4 grid; %d warped tokens with a tap outside" % (
        hgt, wid, Hp, Wp, float(np.abs(keep["fwd_c4p1"]).max()), res, n_out))
    assert res > 0.25 and n_out > 0
    # pred_bidir_flow's backward is the forward of the swapped pair (every batch element is its own sample)
    swapped = unpad(run(m, pc, pa, 4, 1, False)[0][0])
    print("[gmflow_scale2 %dx%d] pred_bidir_flow's backward vs the swapped pair's forward: max abs diff %.3g" % (
        hgt, wid, float(np.abs(swapped - keep["bwd_c4p1"]).max())))
    for R, r in S.CONFIGS[(hgt, wid)]:
        if (R, r) == (4, 1):
            continue
        up, st = run(m, pa, pc, R, r, False)
        tag = "_c%dp%d" % (R, r)
        keep["fwd" + tag] = unpad(up[0])
        keep["flow_match4" + tag], keep["flow_prop4" + tag] = st["flow_match4"], st["flow_prop4"]
    out = os.path.join(GOLD, S.golden_name((hgt, wid)))
    np.savez_compressed(out, **keep)
    print("[gmflow_scale2 %dx%d] %d bytes" % (hgt, wid, os.path.getsize(out)))
    assert os.path.getsize(out) < 1000000


def refused(m):
    """the reference refuses 112 x 160 (a multiple of 16, not of 32) in its window split: what a /16 pad of 100 x 150 would give it"""
    z = torch.zeros(1, 3, 112, 160)
    try:
        with torch.no_grad():
            m(z, z, attn_splits_list=[2, 8], corr_radius_list=[-1, 4], prop_radius_list=[-1, 1])
        raise SystemExit("the reference was expected to refuse 112 x 160")
    except AssertionError:
        print("[gmflow_scale2] the reference refuses 112 x 160 (assertion in its window split)")


if __name__ == "__main__":
    net, wts = model()
    ops(net)
    refused(net)
    for hw in S.SIZES:
        pair(net, wts, *hw)
