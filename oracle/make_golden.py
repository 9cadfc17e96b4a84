"""Generate tests/golden/*.npz by running the REAL reference modules in the build container.

Run from the repo root:  python oracle/make_golden.py
Needs /root/reference (read-only).  It never runs on the GPU box; only the vectors
(inputs + expected outputs) are committed.  The same run asserts that the oracle
restatement (oracle/depth_oracle.py) reproduces the reference to fp32 round-off,
which is what "pinned" means in the oracle header.

Reference entry points exercised
  d_anything.dpt.DPT_DINOv2              bands/d_anything/dpt.py:139-166
  vision_transformer.vit_large(depth=4)  .../facebookresearch_dinov2_main/vision_transformer.py:367-378
  d_anything.dpt.DPTHead                 bands/d_anything/dpt.py:22-136
  common.encode.heat_to_rgb/process_flow bands/common/encode.py:13-33,113-126
  gmflow.gmflow.GMFlow                   bands/gmflow/gmflow.py:12-170 (case `gmflow`)
"""
import os
import sys
import types
import warnings

import numpy as np

warnings.filterwarnings("ignore")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "bands"))
sys.path.insert(0, os.path.join(REF, "bands/d_anything/torchhub/facebookresearch_dinov2_main"))
os.chdir(REF)                                   # dpt.py:147 uses a cwd-relative hub path

import torch  # noqa: E402

from oracle import depth_oracle as O  # noqa: E402
from prisma_amd import synth  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
torch.manual_seed(0)
torch.set_num_threads(8)


def load_into(module, weights, prefix=""):
    sd = {k[len(prefix):]: torch.from_numpy(v) for k, v in weights.items() if k.startswith(prefix)}
    missing, unexpected = module.load_state_dict(sd, strict=True)
    assert not missing and not unexpected


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def hook_stages(model):
    """Forward hooks that record the stages the oracle also reports."""
    st = {}

    def rec(name):
        def f(_m, _i, o):
            st[name] = (o[0] if isinstance(o, (tuple, list)) else o).detach().numpy().copy()
        return f

    vit, head = model.pretrained, model.depth_head
    vit.patch_embed.register_forward_hook(rec("patch_embed"))
    for i, b in enumerate(vit.blocks):
        b.register_forward_hook(rec(f"block{i}"))
    for i in range(4):
        getattr(head.scratch, f"layer{i + 1}_rn").register_forward_hook(rec(f"layer{i + 1}_rn"))
        getattr(head.scratch, f"refinenet{i + 1}").register_forward_hook(rec(f"path{i + 1}"))
    head.scratch.output_conv1.register_forward_hook(rec("output_conv1"))
    head.scratch.output_conv2[1].register_forward_hook(rec("output_conv2_0"))
    head.scratch.output_conv2[2].register_forward_hook(rec("pre_relu"))
    return st


class RefAssembled(torch.nn.Module):
    """Reference classes assembled by hand so depth != 24 is possible (DPT_DINOv2 hard-wires hub models)."""

    def __init__(self, cfg):
        super().__init__()
        import vision_transformer as vits
        from d_anything.dpt import DPTHead
        from dinov2.layers import MemEffAttention, NestedTensorBlock
        from functools import partial
        self.pretrained = vits.DinoVisionTransformer(
            img_size=518, patch_size=14, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.heads,
            mlp_ratio=4, init_values=1.0, ffn_layer="mlp", block_chunks=0,
            block_fn=partial(NestedTensorBlock, attn_class=MemEffAttention),
            num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1)
        self.depth_head = DPTHead(1, cfg.embed_dim, cfg.features, False, out_channels=list(cfg.out_channels),
                                  use_clstoken=False)

    def forward(self, x):
        from d_anything.dpt import DPT_DINOv2
        return DPT_DINOv2.forward(self, x)


def build_ref(cfg_name):
    from d_anything.dpt import DPT_DINOv2
    cfg = synth.DEPTH_CFGS[cfg_name]
    w = synth.depth_anything_weights(cfg, seed=1234)
    if cfg_name in ("vits", "vitb", "vitl"):
        m = DPT_DINOv2(encoder=cfg_name, features=cfg.features, out_channels=list(cfg.out_channels))
    else:
        m = RefAssembled(cfg)
    load_into(m, w)
    return cfg, w, m.eval()


def small_case(cfg_name, hgt, wid, seed):
    """A small synthetic frame through pre-process (oracle) -> REFERENCE model -> band resize."""
    cfg, w, m = build_ref(cfg_name)
    st_ref = hook_stages(m)
    frame = synth.frames(1, hgt, wid, seed=seed)[0]
    x = O.preprocess(frame)[None]
    with torch.no_grad():
        d_net = m(torch.from_numpy(x))
        d_ref = torch.nn.functional.interpolate(d_net[None], (hgt, wid), mode="bilinear",
                                                align_corners=False)[0, 0].numpy()
        d_net = d_net.numpy()
    d_or, st_or = O.model_forward(w, x, cfg.depth, cfg.heads, return_stages=True)
    worst = max(relerr(d_or, d_net), relerr(O.infer(w, frame, cfg.depth, cfg.heads), d_ref))
    for k in st_ref:
        if k in st_or:
            worst = max(worst, relerr(st_or[k], st_ref[k]))
    print(f"[{cfg_name} {hgt}x{wid} -> net {x.shape[2]}x{x.shape[3]}] oracle vs reference worst rel err "
          f"{worst:.2e}; depth range {d_ref.min():.4f}..{d_ref.max():.4f}")
    assert worst < 2e-5, worst
    keep = ["patch_embed", "block0", f"block{cfg.depth - 1}", "layer1_rn", "layer4_rn", "path4", "path1",
            "output_conv1", "pre_relu"]
    out = {"frame_seed": np.array(seed), "frame_hw": np.array([hgt, wid]), "depth": d_ref,
           "net_depth_s4": d_net[0, ::4, ::4].copy()}
    for k in keep:
        v = st_ref[k]
        out["sum_" + k] = np.array([v.astype(np.float64).sum(), np.abs(v.astype(np.float64)).sum()])
        if v.size > 40000:                      # keep fixtures small: strided sample + full-tensor moments
            v = v.reshape(-1)[:: max(1, v.size // 20000)]
        out["st_" + k] = v
    np.savez_compressed(os.path.join(GOLD, f"depth_{cfg_name}_{hgt}x{wid}.npz"), **out)


def full_case():
    """ViT-L at the 518x924 network size both BASELINE resolutions map to, from a 720p frame."""
    cfg, w, m = build_ref("vitl")
    frame = synth.frames(1, 720, 1280, seed=0)[0]
    x = O.preprocess(frame)[None]
    assert x.shape == (1, 3, 518, 924)
    with torch.no_grad():
        d_net = m(torch.from_numpy(x))
        d_ref = torch.nn.functional.interpolate(d_net[None], (720, 1280), mode="bilinear",
                                                align_corners=False)[0, 0].numpy()
    d_or = O.infer(w, frame, cfg.depth, cfg.heads)
    e = relerr(d_or, d_ref)
    print(f"[vitl 720p] oracle vs reference rel err {e:.2e}; depth {d_ref.min():.4f}..{d_ref.max():.4f} "
          f"mean {d_ref.mean():.4f}")
    assert e < 5e-5, e
    rgb, dmin, dmax = O.encode_depth_video(d_ref, flip=True)
    np.savez_compressed(
        os.path.join(GOLD, "depth_vitl_720p.npz"),
        frame_seed=np.array(0), depth_s8=d_ref[::8, ::8].copy(), net_s8=d_net[0].numpy()[::8, ::8].copy(),
        depth_sum=np.array([d_ref.astype(np.float64).sum(), np.abs(d_ref.astype(np.float64)).sum()]),
        minmax=np.array([dmin, dmax]), rgb_s8=rgb[::8, ::8].copy())


def heavy_case():
    """Round 3: the same reference models on HEAVY-TAILED weights (prisma_amd/synth.py *_heavy: outlier LayerNorm / BatchNorm channels
    x 30-50 with partly compensated consumers), so that activations reach tens to hundreds where the engine's split-precision copies
    live.  ViT-L from a 720p frame (strided samples, like depth_vitl_720p) and RAFT on a 184 x 256 pair, 12 iterations."""
    from d_anything.dpt import DPT_DINOv2
    cfg = synth.DEPTH_CFGS["vitl"]
    w = synth.depth_anything_weights_heavy(cfg, seed=1234)
    m = DPT_DINOv2(encoder="vitl", features=cfg.features, out_channels=list(cfg.out_channels))
    load_into(m, w)
    m = m.eval()
    st = hook_stages(m)
    frame = synth.frames(1, 720, 1280, seed=3)[0]
    x = O.preprocess(frame)[None]
    with torch.no_grad():
        d_net = m(torch.from_numpy(x))
        d_ref = torch.nn.functional.interpolate(d_net[None], (720, 1280), mode="bilinear", align_corners=False)[0, 0].numpy()
    d_or = O.infer(w, frame, cfg.depth, cfg.heads)
    e = relerr(d_or, d_ref)
    amax = {k: float(np.abs(v).max()) for k, v in st.items()}
    print(f"[vitl heavy 720p] oracle vs reference rel err {e:.2e}; depth {d_ref.min():.4f}..{d_ref.max():.4f} mean {d_ref.mean():.4f}; "
          f"max |activation|: block0 {amax.get('block0', 0):.1f}, block23 {amax.get('block23', 0):.1f}, layer1_rn {amax.get('layer1_rn', 0):.1f}, "
          f"path1 {amax.get('path1', 0):.1f}, output_conv1 {amax.get('output_conv1', 0):.1f}")
    assert e < 5e-5 and np.isfinite(d_ref).all() and d_ref.max() > d_ref.min() >= 0 and (d_ref > 0).mean() > 0.8, e
    np.savez_compressed(os.path.join(GOLD, "depth_vitl_heavy_720p.npz"), frame_seed=np.array(3), depth_s8=d_ref[::8, ::8].copy(),
                        net_s8=d_net[0].numpy()[::8, ::8].copy(),
                        depth_sum=np.array([d_ref.astype(np.float64).sum(), np.abs(d_ref.astype(np.float64)).sum()]))
    import argparse
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from raft.raft import RAFT
    from common.flow import InputPadder
    from oracle import raft_oracle as R
    rw = synth.raft_weights_heavy(seed=4321)
    rm = RAFT(argparse.Namespace()).eval()
    rm.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.items()}, strict=True)
    hgt, wid, iters = 184, 256, 12
    fr = synth.frame_pair_sequence(2, hgt, wid, seed=23)
    a = torch.from_numpy(fr[0]).permute(2, 0, 1).float()[None]
    c = torch.from_numpy(fr[1]).permute(2, 0, 1).float()[None]
    i1, i2 = torch.cat([a, c], 0), torch.cat([c, a], 0)
    padder = InputPadder(i1.shape)
    p1, p2 = padder.pad(i1, i2)
    with torch.no_grad():
        lo, up = rm(p1, p2, iters=iters, test_mode=True)
        fwd = padder.unpad(up[0]).permute(1, 2, 0).numpy()
        bwd = padder.unpad(up[1]).permute(1, 2, 0).numpy()
    f_o, b_o = R.infer_pair(rw, fr[0], fr[1], scale=1.0, iters=iters)
    e = max(relerr(f_o, fwd), relerr(b_o, bwd))
    print(f"[raft heavy {hgt}x{wid}] oracle vs reference rel err {e:.2e}; |flow| max {np.abs(fwd).max():.2f} px")
    assert e < 2e-4 and np.isfinite(fwd).all(), e
    np.savez_compressed(os.path.join(GOLD, "raft_heavy_184x256.npz"), frame_seed=np.array(23), hw=np.array([hgt, wid]), iters=np.array(iters),
                        fwd=fwd, bwd=bwd)


def heavy_1080p_case():
    """the heavy-tailed ViT-L weights on the frame the bench-shaped parity test reports (frame 13 of the 32-frame
    1080p clip of seed 77), through the REAL reference model - so that the margin the per-layer residual assignment left (qkv and fc1
    run one fp16 pass) is asserted at the timed size on outlier activations too."""
    from d_anything.dpt import DPT_DINOv2
    cfg = synth.DEPTH_CFGS["vitl"]
    w = synth.depth_anything_weights_heavy(cfg, seed=1234)
    m = DPT_DINOv2(encoder="vitl", features=cfg.features, out_channels=list(cfg.out_channels))
    load_into(m, w)
    m = m.eval()
    frame = synth.frames(32, 1080, 1920, seed=77)[13]
    x = O.preprocess(frame)[None]
    with torch.no_grad():
        d_net = m(torch.from_numpy(x))
        d_ref = torch.nn.functional.interpolate(d_net[None], (1080, 1920), mode="bilinear", align_corners=False)[0, 0].numpy()
    d_or = O.infer(w, frame, cfg.depth, cfg.heads)
    e = relerr(d_or, d_ref)
    print(f"[vitl heavy 1080p] oracle vs reference rel err {e:.2e}; depth {d_ref.min():.4f}..{d_ref.max():.4f} mean {d_ref.mean():.4f}")
    assert e < 5e-5 and np.isfinite(d_ref).all() and d_ref.max() > d_ref.min() >= 0, e
    np.savez_compressed(os.path.join(GOLD, "depth_vitl_heavy_1080p.npz"), frame_seed=np.array(77), frame_index=np.array(13),
                        depth_s8=d_ref[::8, ::8].copy(),
                        depth_sum=np.array([d_ref.astype(np.float64).sum(), np.abs(d_ref.astype(np.float64)).sum()]))


def encode_case():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))   # common/encode.py:10 imports cv2 for Sobel only
    from common import encode as E
    ramp = np.linspace(0.0, 1.0, 4096).reshape(64, 64)
    heat = (E.heat_to_rgb(ramp) * 255).astype(np.uint8)
    g = np.random.default_rng(7)
    pred = (g.standard_normal((45, 80)).astype(np.float32) * 3 + 10).astype(np.float32)
    dmin, dmax = pred.min(), pred.max()
    d = 1.0 - (pred - dmin) / (dmax - dmin)
    vid = (E.heat_to_rgb(d.astype(np.float64)) * 255).astype(np.uint8)
    mine, a, b = O.encode_depth_video(pred, flip=True)
    assert np.array_equal(mine, vid) and a == float(dmin) and b == float(dmax)
    assert np.array_equal((O.heat_to_rgb(ramp) * 255).astype(np.uint8), heat)
    flow = g.standard_normal((40, 64, 2)).astype(np.float32) * 5
    frgb, fmax = E.process_flow(flow.copy())
    with np.errstate(all="ignore"):
        zrgb, zmax = E.process_flow(np.zeros((8, 8, 2), np.float32))
    np.savez_compressed(os.path.join(GOLD, "encode.npz"), ramp=ramp, heat=heat, pred=pred, vid=vid,
                        flow=flow, flow_rgb=frgb, flow_max=np.array(fmax), zero_rgb=zrgb, zero_max=np.array(zmax),
                        float_to_rgb=np.array(E.float_to_rgb(12.5, 0.0, 1000.0)))
    print("[encode] oracle == reference (bit exact)")


def write_depth_case(seed=9):
    """The REAL reference write_depth (bands/common/io.py:138-172) + float_to_edge / saturation / float_to_rgb (encode.py:73-95,
    141-146) on a seeded float32 depth map, in the three ways the band scripts call it (relative: flip, metric: no flip, 16-bit).
    cv2 is absent, so the reference runs on a stand-in module: imwrite records the array, cvtColor swaps channels, and Sobel is
    the restatement this repo uses (bands/common/io.py _sobel_mag_u8: [-1, 0, 1] central differences, BORDER_REFLECT_101) -
    the golden pins every byte of the PNG except the Sobel taps themselves (opencv-python 4.8.1.78, third party, unpinned)."""
    written = {}
    cv2 = types.ModuleType("cv2")
    cv2.CV_64F, cv2.COLOR_RGB2BGR, cv2.INTER_AREA = 6, 4, 3

    def sobel(img, ddepth, dx, dy, ksize=1):
        assert ddepth == 6 and ksize == 1
        p = np.pad(img.astype(np.float64), 1, mode="reflect")
        return p[1:-1, 2:] - p[1:-1, :-2] if dx == 1 else p[2:, 1:-1] - p[:-2, 1:-1]
    cv2.Sobel = sobel
    cv2.cvtColor = lambda a, code: a[..., ::-1]
    cv2.imwrite = lambda path, a: written.__setitem__(path, np.array(a))
    for k in [k for k in sys.modules if k == "cv2" or k.startswith("common")]:
        del sys.modules[k]
    sys.modules["cv2"] = cv2
    for name in ("decord", "av", "plyfile"):        # imported at module level by common/io.py and common/geom.py, unused here
        m = sys.modules.setdefault(name, types.ModuleType(name))
        if name == "plyfile":
            m.PlyData = m.PlyElement = object
    from common import io as RIO
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:60, 0:96].astype(np.float32)
    depth = (3.0 + 2.0 * np.sin(xx / 11.0) * np.cos(yy / 7.0) + 0.05 * g.standard_normal((60, 96))).astype(np.float32)
    depth[20:40, 30:60] += 4.0                                        # a step edge: saturation drops along it
    RIO.write_depth("rel", depth.copy(), normalize=True, flip=True, heatmap=True, encode_range=True)
    RIO.write_depth("met", depth.copy(), normalize=True, flip=False, heatmap=True, encode_range=True)
    RIO.write_depth("u16", depth.copy(), normalize=True, flip=False, heatmap=False)
    np.savez_compressed(os.path.join(GOLD, "write_depth.npz"), depth=depth, rel_rgb=written["rel"][..., ::-1].copy(),
                        met_rgb=written["met"][..., ::-1].copy(), u16=written["u16"])
    print("[write_depth] reference io.write_depth on a stand-in cv2: 3 images recorded; pixel (0,0)/(0,1) =", written["rel"][0, 0, ::-1], written["rel"][0, 1, ::-1])


def raft_case(hgt=125, wid=157, seed=21, iters=12):
    """Reference RAFT (bands/raft/raft.py) + InputPadder (bands/common/flow.py) on a seeded frame pair,
    fwd and bwd in one batch exactly like bands/flow_raft.py:105-107 (scale = 1: cv2 is absent here)."""
    import argparse
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from raft.raft import RAFT
    from common.flow import InputPadder
    from oracle import raft_oracle as R
    w = synth.raft_weights(seed=4321)
    m = RAFT(argparse.Namespace()).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    fr = synth.frame_pair_sequence(2, hgt, wid, seed=seed)
    a = torch.from_numpy(fr[0]).permute(2, 0, 1).float()[None]
    c = torch.from_numpy(fr[1]).permute(2, 0, 1).float()[None]
    i1, i2 = torch.cat([a, c], 0), torch.cat([c, a], 0)
    padder = InputPadder(i1.shape)
    p1, p2 = padder.pad(i1, i2)
    assert list(padder._pad) == R.pad_amounts(hgt, wid)
    with torch.no_grad():
        lo, up = m(p1, p2, iters=iters, test_mode=True)
        fwd = padder.unpad(up[0]).permute(1, 2, 0).numpy()
        bwd = padder.unpad(up[1]).permute(1, 2, 0).numpy()
    lo_o, up_o, st = R.raft_forward(w, p1.numpy(), p2.numpy(), iters, return_stages=True)
    f_o, b_o = R.infer_pair(w, fr[0], fr[1], scale=1.0, iters=iters)
    e = max(relerr(lo_o, lo.numpy()), relerr(up_o, up.numpy()), relerr(f_o, fwd), relerr(b_o, bwd))
    print(f"[raft {hgt}x{wid} pad {padder._pad}] oracle vs reference rel err {e:.2e}; |flow| max {np.abs(fwd).max():.2f} px, "
          f"mean fwd {fwd.reshape(-1, 2).mean(0)}")
    assert e < 2e-4, e
    sys.path.insert(0, os.path.join(REF, "bands"))
    from common import encode as E
    rgb, mx = E.process_flow(fwd.copy())
    rgb_o, mx_o = R.process_flow(fwd)
    assert np.array_equal(rgb, rgb_o) and mx == mx_o
    np.savez_compressed(os.path.join(GOLD, f"raft_{hgt}x{wid}.npz"), frame_seed=np.array(seed), hw=np.array([hgt, wid]),
                        iters=np.array(iters), flow_lo=lo.numpy(), fwd=fwd, bwd=bwd, fwd_rgb=rgb, fwd_max=np.array(mx),
                        fmap1=st["fmap1"][:, ::4].copy(), net0=st["net0"][:, ::4].copy(), corr0=st["corr0"][:, ::3].copy(),
                        flow_it0=st["flow_it0"])


def gmflow_case(hgt=125, wid=157, seed=51, bidir=True, tag=None):
    """Reference GMFlow (bands/gmflow/gmflow.py) + InputPadder(padding_factor=16) on a seeded frame pair, called the way
    bands/flow_gmflow.py:66-118 calls it (attn_splits_list [2], corr_radius_list [-1], prop_radius_list [-1], pred_bidir_flow when
    backward flow / masks are wanted; scale = 1: cv2 is absent here)."""
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from gmflow.gmflow import GMFlow
    from common.flow import InputPadder
    from oracle import gmflow_oracle as G
    w = synth.gmflow_weights(seed=2468)
    m = GMFlow(feature_channels=128, num_scales=1, upsample_factor=8, num_head=1, attention_type="swin", ffn_dim_expansion=4,
               num_transformer_layers=6)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    fr = synth.frame_pair_sequence(2, hgt, wid, seed=seed)
    a = torch.from_numpy(fr[0]).permute(2, 0, 1).float()[None]
    c = torch.from_numpy(fr[1]).permute(2, 0, 1).float()[None]
    padder = InputPadder(a.shape, padding_factor=16)
    p1, p2 = padder.pad(a, c)
    assert list(padder._pad) == G.pad_amounts(hgt, wid)
    # the reference builds its shifted-window mask on device 'cuda' by default argument only; FeatureTransformer passes feature0.device
    with torch.no_grad():
        out = m(p1, p2, attn_splits_list=[2], corr_radius_list=[-1], prop_radius_list=[-1], pred_bidir_flow=bidir)["flow_preds"][-1]
        fwd = padder.unpad(out[0]).permute(1, 2, 0).numpy()
        bwd = padder.unpad(out[1]).permute(1, 2, 0).numpy() if bidir else None
    up_o, st = G.gmflow_forward(w, p1.numpy(), p2.numpy(), bidir=bidir, return_stages=True)
    f_o, b_o = G.infer_pair(w, fr[0], fr[1], scale=1.0, backward=bidir)
    e = max(relerr(up_o, out.numpy()), relerr(f_o, fwd), relerr(b_o, bwd) if bidir else 0.0)
    print(f"[gmflow {hgt}x{wid} pad {padder._pad} bidir {bidir}] oracle vs reference rel err {e:.2e}; |flow| max {np.abs(fwd).max():.2f} px, "
          f"mean fwd {fwd.reshape(-1, 2).mean(0)}, match-stage |flow| max {np.abs(st['flow_match']).max():.2f}")
    assert e < 2e-4, e
    keep = dict(frame_seed=np.array(seed), hw=np.array([hgt, wid]), fwd=fwd, feat0=st["feat0"][:, ::4].copy(),
                block0=st["block0"][:, :, ::4].copy(), tfeat0=st["tfeat0"][:, ::4].copy(), flow_match=st["flow_match"], flow_prop=st["flow_prop"])
    if bidir:
        keep["bwd"] = bwd
    np.savez_compressed(os.path.join(GOLD, f"gmflow_{tag or (str(hgt) + 'x' + str(wid))}.npz"), **keep)


def gmflow_isz_case(hgt=150, wid=210, seed=53, isz=(96, 160)):
    """flow_gmflow --inference_size (bands/flow_gmflow.py:76-100): the REAL GMFlow wrapped exactly as the band's infer() wraps it - no
    padder, F.interpolate(bilinear, align_corners=True) of the float frames to inference_size, the model, the flow resized back and
    rescaled per axis - both directions; the oracle's infer_pair(inference_size=...) must return the same."""
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import torch.nn.functional as Fn
    from gmflow.gmflow import GMFlow
    from oracle import gmflow_oracle as G
    w = synth.gmflow_weights(seed=2468)
    m = GMFlow(feature_channels=128, num_scales=1, upsample_factor=8, num_head=1, attention_type="swin", ffn_dim_expansion=4,
               num_transformer_layers=6)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    fr = synth.frame_pair_sequence(2, hgt, wid, seed=seed)
    image1 = torch.from_numpy(fr[0]).permute(2, 0, 1).float()[None]
    image2 = torch.from_numpy(fr[1]).permute(2, 0, 1).float()[None]
    ori_size = image1.shape[-2:]
    with torch.no_grad():
        i1 = Fn.interpolate(image1, size=list(isz), mode="bilinear", align_corners=True)
        i2 = Fn.interpolate(image2, size=list(isz), mode="bilinear", align_corners=True)
        flow_pr = m(i1, i2, attn_splits_list=[2], corr_radius_list=[-1], prop_radius_list=[-1], pred_bidir_flow=True)["flow_preds"][-1]
        flow_pr = Fn.interpolate(flow_pr, size=ori_size, mode="bilinear", align_corners=True)
        flow_pr[:, 0] = flow_pr[:, 0] * ori_size[-1] / isz[-1]
        flow_pr[:, 1] = flow_pr[:, 1] * ori_size[-2] / isz[-2]
    fwd, bwd = flow_pr[0].permute(1, 2, 0).numpy(), flow_pr[1].permute(1, 2, 0).numpy()
    f_o, b_o = G.infer_pair(w, fr[0], fr[1], scale=1.0, backward=True, inference_size=isz)
    e = max(relerr(f_o, fwd), relerr(b_o, bwd))
    print(f"[gmflow {hgt}x{wid} inference_size {isz}] oracle vs reference rel err {e:.2e}; |flow| max {np.abs(fwd).max():.2f} px")
    assert e < 2e-4, e
    np.savez_compressed(os.path.join(GOLD, "gmflow_isz_150x210.npz"), frame_seed=np.array(seed), hw=np.array([hgt, wid]), isz=np.array(isz),
                        fwd=fwd, bwd=bwd)


def gmflow_full_case(seed=61):
    """flow_gmflow at the size the bench times it: one 1920x1080 pair at the band's default --scale 0.75
    (810x1440 -> InputPadder(16) -> 816x1440: a 102 x 180 grid, 18 360 tokens, 18 360^2 global matching) through the REAL reference
    GMFlow, forward direction, committed as 1/8-strided samples + float64 sums (as raft_full).  cv2 is absent here, so the reference
    network is fed the oracle's 8-bit cubic resize (unpinned; GPU == oracle bit for bit: tests/test_gpu_flow_io_ops.py::test_prep_direct) - the golden pins the network at that size."""
    import time
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from gmflow.gmflow import GMFlow
    from common.flow import InputPadder
    from oracle import raft_oracle as R
    w = synth.gmflow_weights(seed=2468)
    m = GMFlow(feature_channels=128, num_scales=1, upsample_factor=8, num_head=1, attention_type="swin", ffn_dim_expansion=4,
               num_transformer_layers=6)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    big = synth.frame_pair_sequence(2, 1080, 1920, seed=seed)
    a_u8, c_u8 = R.cv_resize_cubic_u8(big[0], 0.75), R.cv_resize_cubic_u8(big[1], 0.75)
    assert a_u8.shape == (810, 1440, 3)
    a = torch.from_numpy(np.ascontiguousarray(a_u8)).permute(2, 0, 1).float()[None]
    c = torch.from_numpy(np.ascontiguousarray(c_u8)).permute(2, 0, 1).float()[None]
    padder = InputPadder(a.shape, padding_factor=16)
    p1, p2 = padder.pad(a, c)
    assert tuple(p1.shape[-2:]) == (816, 1440)
    t0 = time.time()
    with torch.no_grad():
        out = m(p1, p2, attn_splits_list=[2], corr_radius_list=[-1], prop_radius_list=[-1], pred_bidir_flow=False)["flow_preds"][-1]
    f = padder.unpad(out[0]).permute(1, 2, 0).numpy()
    print(f"[gmflow 1080p x0.75] reference forward {time.time() - t0:.1f} s, |flow| max {np.abs(f).max():.2f}, mean {f.reshape(-1, 2).mean(0)}", flush=True)
    np.savez_compressed(os.path.join(GOLD, "gmflow_full.npz"), frame_seed=np.array(seed), fwd1080_s8=f[::8, ::8].copy(),
                        sums1080=np.array([f[..., 0].astype(np.float64).sum(), f[..., 1].astype(np.float64).sum(),
                                           np.abs(f.astype(np.float64)).sum()]),
                        absmax=np.array(np.abs(f).max()))


def raft_full_case(seed=41, iters=12):
    """BASELINE configs[2] / [4] at full size: the REAL reference RAFT + InputPadder on (a) 8 consecutive-frame pairs of a 9-frame
    1280x720 sequence, forward direction, 12 iterations (configs[2]: batch of 8 pairs, no --scale), committed as 1/8-strided
    samples + float64 sums per pair; (b) one 1920x1080 pair at the band's default --scale 0.75 (810x1440 -> pad 816x1440,
    configs[4]); cv2 is absent here, so the reference network is fed the oracle's 8-bit cubic resize (unpinned, GPU == oracle bit
    for bit) - the golden pins the network at that size.  The reference runs one pair per call (batch 1), like its band script."""
    import argparse
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from raft.raft import RAFT
    from common.flow import InputPadder
    from oracle import raft_oracle as R
    w = synth.raft_weights(seed=4321)
    m = RAFT(argparse.Namespace()).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)

    def ref_pair(a_u8, c_u8):
        a = torch.from_numpy(np.ascontiguousarray(a_u8)).permute(2, 0, 1).float()[None]
        c = torch.from_numpy(np.ascontiguousarray(c_u8)).permute(2, 0, 1).float()[None]
        padder = InputPadder(a.shape)
        p1, p2 = padder.pad(a, c)
        with torch.no_grad():
            _, up = m(p1, p2, iters=iters, test_mode=True)
        return padder.unpad(up[0]).permute(1, 2, 0).numpy()

    import time
    fr = synth.frame_pair_sequence(9, 720, 1280, seed=seed)
    s8, sums = [], []
    for i in range(8):
        t0 = time.time()
        f = ref_pair(fr[i], fr[i + 1])
        s8.append(f[::8, ::8].copy())
        sums.append([f[..., 0].astype(np.float64).sum(), f[..., 1].astype(np.float64).sum(), np.abs(f.astype(np.float64)).sum()])
        if i == 0:
            f_o, _ = R.infer_pair(w, fr[0], fr[1], scale=1.0, iters=iters)
            e = relerr(f_o, f)
            assert e < 2e-4, e
            print(f"[raft 720p] oracle vs reference rel err {e:.2e}")
        print(f"[raft 720p] pair {i}: {time.time() - t0:.1f} s, |flow| max {np.abs(f).max():.2f}, mean {f.reshape(-1, 2).mean(0)}", flush=True)
    big = synth.frame_pair_sequence(2, 1080, 1920, seed=seed + 1)
    a, c = R.cv_resize_cubic_u8(big[0], 0.75), R.cv_resize_cubic_u8(big[1], 0.75)
    assert a.shape == (810, 1440, 3)
    f1080 = ref_pair(a, c)
    print(f"[raft 1080p x0.75] |flow| max {np.abs(f1080).max():.2f}, mean {f1080.reshape(-1, 2).mean(0)}")
    np.savez_compressed(os.path.join(GOLD, "raft_full.npz"), frame_seed=np.array(seed), iters=np.array(iters),
                        fwd720_s8=np.stack(s8), sums720=np.array(sums), fwd1080_s8=f1080[::8, ::8].copy(),
                        sums1080=np.array([f1080[..., 0].astype(np.float64).sum(), f1080[..., 1].astype(np.float64).sum(),
                                           np.abs(f1080.astype(np.float64)).sum()]))


def mask_case(seed=5):
    """Self-vector of oracle/solov2_oracle.py (the mask band's reference cannot be imported: mmcv is absent)."""
    from oracle import solov2_oracle as SO
    cfg = synth.MASK_CFGS["tiny"]
    w = synth.solov2_weights(cfg)
    fr = synth.frames(1, 180, 300, seed=seed)[0]
    x, meta = SO.preprocess(fr, cfg)
    kps, cps, mf = SO.network(w, cfg, x)
    sc, lb, mk = SO.get_results(cfg, kps, cps, mf, meta["img_shape"], meta["ori_shape"])
    img = SO.band_mask(sc, lb, mk, synth.COCO_CLASSES, synth.BAND_CLASSES, 0.5, meta["ori_shape"])
    print(f"[solov2 tiny] {len(sc)} instances, {int((sc > 0.5).sum())} over 0.5, image values {np.unique(img)}")
    np.savez_compressed(os.path.join(GOLD, "solov2_tiny_180x300.npz"), frame_seed=np.array(seed), cls_logit4=cps[4].numpy(),
                        mask_feats_sub=mf.numpy()[0, ::16, ::4, ::4].copy(), scores=sc.numpy(), labels=lb.numpy(), mask_image=img)



def matrix_nms_case(seed=3):
    """mask_matrix_nms of the REAL reference file (bands/mmdet/core/post_processing/matrix_nms.py:5-121 imports only torch, so
    it loads without mmcv): inputs + outputs committed, and the oracle's restatement asserted equal - the one piece of the
    mask band that can be pinned in this container."""
    import importlib.util
    from oracle import solov2_oracle as SO
    spec = importlib.util.spec_from_file_location("ref_matrix_nms", os.path.join(REF, "bands/mmdet/core/post_processing/matrix_nms.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for case, (n, h, w, ncls, nms_pre, max_num) in enumerate([(40, 24, 32, 3, 500, 100), (90, 40, 56, 5, 60, 25), (12, 16, 16, 1, 500, 100)]):
        rng = np.random.default_rng(seed + case)
        yy, xx = np.mgrid[0:h, 0:w]
        masks = np.stack([((yy - rng.uniform(4, h - 4)) ** 2 + (xx - rng.uniform(4, w - 4)) ** 2) < rng.uniform(9, 60) for _ in range(n)])
        labels = rng.integers(0, ncls, n)
        scores = rng.uniform(0.06, 0.9, n).astype(np.float32)
        areas = masks.reshape(n, -1).sum(1).astype(np.float32)
        import dataclasses
        cfg = dataclasses.replace(synth.MASK_CFGS["tiny"], nms_pre=nms_pre, max_per_img=max_num)
        tm, tl, ts, ta = torch.from_numpy(masks), torch.from_numpy(labels), torch.from_numpy(scores), torch.from_numpy(areas)
        r_sc, r_lb, r_mk, r_keep = ref.mask_matrix_nms(tm, tl, ts, filter_thr=cfg.filter_thr, nms_pre=cfg.nms_pre, max_num=cfg.max_per_img,
                                                       kernel="gaussian", sigma=cfg.sigma, mask_area=ta)
        o_sc, o_lb, o_keep = SO.matrix_nms(tm, tl, ts, ta, cfg)
        assert torch.equal(r_sc, o_sc) and torch.equal(r_lb, o_lb) and torch.equal(r_keep, o_keep) and torch.equal(r_mk, tm[o_keep])
        out.update({f"masks{case}": np.packbits(masks, axis=-1), f"shape{case}": np.array([n, h, w]), f"labels{case}": labels,
                    f"scores{case}": scores, f"areas{case}": areas, f"cfg{case}": np.array([nms_pre, max_num, cfg.filter_thr, cfg.sigma]),
                    f"out_scores{case}": r_sc.numpy(), f"out_labels{case}": r_lb.numpy(), f"out_keep{case}": r_keep.numpy()})
        print(f"[matrix nms] case {case}: {n} candidates -> {len(r_sc)} kept: oracle == reference (exact)")
    np.savez_compressed(os.path.join(GOLD, "matrix_nms.npz"), **out)


def zoe_layers_case(seed=31):
    """The metric head's layers against the reference's own modules (they import torch only), same seeded weights."""
    import importlib.util
    from oracle import zoe_oracle as Z

    def load(name):
        path = os.path.join(REF, "bands", "patchfusion", "zoedepth", "models", "layers", name + ".py")
        spec = importlib.util.spec_from_file_location("ref_zoe_" + name, path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    att, dist, loc = load("attractor"), load("dist_layers"), load("localbins_layers")
    w = {k: v for k, v in synth.zoe_weights().items() if not k.startswith("core.")}
    tw = lambda pre: {k[len(pre):]: torch.from_numpy(v) for k, v in w.items() if k.startswith(pre)}
    g = np.random.default_rng(seed)
    rnd = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    out = {}
    with torch.no_grad():
        x = rnd(1, 256, 5, 6)
        seed_m = loc.SeedBinRegressorUnnormed(256, n_bins=64)
        seed_m.load_state_dict(tw("seed_bin_regressor."))
        b0 = seed_m(x)[1]
        assert torch.equal(b0, Z.seed_bin_regressor(w, x))
        pr = loc.Projector(256, 128)
        pr.load_state_dict(tw("seed_projector."))
        e0 = pr(x)
        assert torch.equal(e0, Z.projector(w, "seed_projector", x))
        xb = rnd(1, 128, 10, 12)
        a0 = att.AttractorLayerUnnormed(128, 64, n_attractors=16, alpha=1000, gamma=2, kind="mean", attractor_type="inv")
        a0.load_state_dict(tw("attractors.0."))
        bn, bc = a0(xb, b0, e0, interpolate=True)
        mine = Z.attractor(w, "attractors.0", xb, b0, e0)
        assert torch.equal(bn, mine) and torch.equal(bc, mine)
        a3 = att.AttractorLayerUnnormed(128, 64, n_attractors=1, alpha=1000, gamma=2, kind="mean", attractor_type="inv")
        a3.load_state_dict(tw("attractors.3."))
        xb3 = rnd(1, 128, 12, 14)
        b3 = a3(xb3, bn, xb, interpolate=True)[0]
        assert torch.equal(b3, Z.attractor(w, "attractors.3", xb3, bn, xb))
        clb = dist.ConditionalLogBinomial(33, 128, n_classes=64, min_temp=0.0212, max_temp=50.0)
        clb.load_state_dict({**tw("conditional_log_binomial."), "log_binomial_transform.k_idx": torch.arange(0, 64).view(1, -1, 1, 1),
                             "log_binomial_transform.K_minus_1": torch.Tensor([63]).view(1, -1, 1, 1)})
        last, cond = rnd(1, 33, 12, 14).abs(), rnd(1, 128, 12, 14)
        pz = clb(last, cond)
        mine = Z.conditional_log_binomial(w, last, cond)
        assert torch.equal(pz, mine), (pz - mine).abs().max()
        out.update(x=x.numpy(), seed_bins=b0.numpy(), seed_emb=e0.numpy(), xb=xb.numpy(), bins0=bn.numpy(), xb3=xb3.numpy(),
                   bins3=b3.numpy(), last=last.numpy(), cond=cond.numpy(), prob=pz.numpy())
    print("[zoe layers] SeedBinRegressorUnnormed, Projector, AttractorLayerUnnormed x2, ConditionalLogBinomial: oracle == reference (exact)")
    np.savez_compressed(os.path.join(GOLD, "zoe_layers.npz"), **out)


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    which = sys.argv[1:] or ["encode", "vits", "vitl_d4", "full", "raft", "mask", "nms", "zoe", "write_depth"]
    if "mask" in which:
        mask_case()
    if "nms" in which:
        matrix_nms_case()
    if "zoe" in which:
        zoe_layers_case()
    if "encode" in which:
        encode_case()
    if "write_depth" in which:
        write_depth_case()
    if "vits" in which:
        small_case("vits", 96, 128, 11)
    if "vitl_d4" in which:
        small_case("vitl_d4", 90, 120, 12)
    if "full" in which:
        full_case()
    if "heavy" in which:
        heavy_case()
    if "heavy_1080p" in which:
        heavy_1080p_case()
    if "gmflow" in which:
        gmflow_case()
        gmflow_case(216, 300, 52, False)   # pads to 224x304: a 28 x 38 grid, 14 x 19 windows, forward only
    if "gmflow_isz" in which:
        gmflow_isz_case()
    if "gmflow_full" in which:
        gmflow_full_case()
    if "raft_full" in which:
        raft_full_case()
    if "raft" in which:
        raft_case()
        raft_case(131, 181, 33, 8)      # pads to 136x184: 17 x 23 = 391 feature pixels, not a multiple of 8
