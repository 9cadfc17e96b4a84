#!/usr/bin/env python3
"""Write tests/golden/gmflow_local_*.npz from the REAL reference (build machine only: needs /root/reference, read-only).

  gmflow_local_ops.npz       seeded tokens / feature / flow inputs on small grids with the outputs of the real local_correlation_softmax
                             (bands/gmflow/matching.py:39-83) and FeatureFlowAttention.forward_local_window_attn (transformer.py:376-409),
                             and that module's seeded q_proj / k_proj
  gmflow_local_125x157.npz   the real GMFlow + InputPadder(16) on a seeded frame pair (grid 16 x 20), called as bands/flow_gmflow.py:84-89
  gmflow_local_90x150.npz    calls it with one radius each: per configuration of tests/gm_local_ref.py CONFIGS the final flow `fwd` and the
                             stages `flow_match` / `flow_prop`; `bwd` from pred_bidir_flow for (-1, 1) and from the swapped pair for (4, 1)
                             (pred_bidir_flow raises with a matching radius: local_correlation_softmax returns B flows for 2 B features)
Data only, float32.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "bands"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
from common.flow import InputPadder  # noqa: E402
from gmflow import gmflow as GM  # noqa: E402
from gmflow.matching import local_correlation_softmax  # noqa: E402
from gmflow.transformer import FeatureFlowAttention  # noqa: E402

import gm_local_ref as L  # noqa: E402
from prisma_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OPS = [(4, 4, 4, 2), (6, 10, 1, 1), (6, 10, 4, 2), (12, 14, 2, 1)]          # (h8, w8, R, r): window larger than the grid, odd, interior


def ops():
    torch.manual_seed(97)
    att = FeatureFlowAttention(128)
    with torch.no_grad():
        att.q_proj.bias.normal_(0, 0.2)
        att.k_proj.bias.normal_(0, 0.2)
    keep = {k: v.detach().numpy().copy() for k, v in att.state_dict().items()}
    for h8, w8, R, r in OPS:
        tag = "%dx%d_R%d_r%d" % (h8, w8, R, r)
        tok = L.match_tokens(500 + h8, 1, h8, w8)                                          # [2, P, 128]
        maps = torch.from_numpy(tok).view(2, h8, w8, 128).permute(0, 3, 1, 2).contiguous()
        feat = (np.random.default_rng(600 + h8).standard_normal((2, h8 * w8, 128)) * 1.2).astype(np.float32)
        flow = L.prop_data(700 + h8, 2, h8, w8, 2)[2]
        with torch.no_grad():
            fm = local_correlation_softmax(maps[:1], maps[1:], R)[0]                       # [1, 2, h8, w8]
            fp = att.forward_local_window_attn(torch.from_numpy(feat).permute(0, 2, 1).reshape(2, 128, h8, w8).contiguous(),
                                               torch.from_numpy(flow).permute(0, 2, 1).reshape(2, 2, h8, w8).contiguous(), local_window_radius=r)
        keep.update({"tok_" + tag: tok, "feat_" + tag: feat, "flow_" + tag: flow, "match_" + tag: fm.flatten(-2).permute(0, 2, 1).numpy(),
                     "prop_" + tag: fp.flatten(-2).permute(0, 2, 1).numpy()})
    keep["cases"] = np.array(OPS)
    out = os.path.join(GOLD, "gmflow_local_ops.npz")
    np.savez_compressed(out, **keep)
    print("[gmflow_local_ops] %d cases, %d bytes" % (len(OPS), os.path.getsize(out)))


def run(m, a, c, corr, prop, bidir):
    """the real GMFlow on a padded pair -> (flow_up [B, 2, H, W], flow_match, flow_prop [B, P, 2]) with the stages caught where forward makes them"""
    st = {}
    real = {n: getattr(GM, n) for n in ("global_correlation_softmax", "local_correlation_softmax")}

    def catch(fn):
        def f(*args, **kw):
            out = fn(*args, **kw)
            st["flow_match"] = out[0].flatten(-2).permute(0, 2, 1).numpy().copy()
            return out
        return f
    hook = m.feature_flow_attn.register_forward_hook(lambda mod, i, o: st.__setitem__("flow_prop", o.flatten(-2).permute(0, 2, 1).numpy().copy()))
    for n, fn in real.items():
        setattr(GM, n, catch(fn))
    try:
        with torch.no_grad():
            up = m(a, c, attn_splits_list=[2], corr_radius_list=[corr], prop_radius_list=[prop], pred_bidir_flow=bidir)["flow_preds"][-1]
    finally:
        hook.remove()
        for n, fn in real.items():
            setattr(GM, n, fn)
    return up, st["flow_match"], st["flow_prop"]


def pair(hgt, wid, seed):
    w = synth.gmflow_weights(seed=2468)
    m = GM.GMFlow(feature_channels=128, num_scales=1, upsample_factor=8, num_head=1, attention_type="swin", ffn_dim_expansion=4,
                  num_transformer_layers=6).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    fr = synth.frame_pair_sequence(2, hgt, wid, seed=seed)
    a = torch.from_numpy(fr[0]).permute(2, 0, 1).float()[None]
    c = torch.from_numpy(fr[1]).permute(2, 0, 1).float()[None]
    padder = InputPadder(a.shape, padding_factor=16)
    pa, pc = padder.pad(a, c)
    unpad = lambda t: padder.unpad(t).permute(1, 2, 0).numpy().astype(np.float32)
    keep = dict(frame_seed=np.array(seed), hw=np.array([hgt, wid]))
    for name, corr, prop in L.CONFIGS:
        up, fm, fp = run(m, pa, pc, corr, prop, False)
        keep.update({"fwd_" + name: unpad(up[0]), "flow_match_" + name: fm.astype(np.float32), "flow_prop_" + name: fp.astype(np.float32)})
        print("[gmflow_local %dx%d %s] |flow| max %.2f px" % (hgt, wid, name, float(np.abs(keep["fwd_" + name]).max())))
    up = run(m, pa, pc, -1, 1, True)[0]
    assert np.array_equal(unpad(up[0]), keep["fwd_p1"])
    keep["bwd_p1"] = unpad(up[1])
    swapped = unpad(run(m, pc, pa, -1, 1, False)[0][0])
    print("[gmflow_local %dx%d p1] pred_bidir_flow's backward vs the swapped pair's forward: max abs diff %.3g" % (
        hgt, wid, float(np.abs(swapped - keep["bwd_p1"]).max())))
    keep["bwd_c4p1"] = unpad(run(m, pc, pa, 4, 1, False)[0][0])
    try:
        run(m, pa, pc, 4, 1, True)
        raise AssertionError("pred_bidir_flow with a matching radius was expected to raise")
    except RuntimeError as e:
        print("[gmflow_local %dx%d c4p1] pred_bidir_flow raises: %s" % (hgt, wid, str(e).splitlines()[0]))
    out = os.path.join(GOLD, "gmflow_local_%dx%d.npz" % (hgt, wid))
    np.savez_compressed(out, **keep)
    print("[gmflow_local %dx%d] %d bytes" % (hgt, wid, os.path.getsize(out)))
    assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    ops()
    pair(125, 157, 51)
    pair(90, 150, 54)
