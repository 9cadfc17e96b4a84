#!/usr/bin/env python3
"""flow_gmflow band - drop-in for /root/reference/bands/flow_gmflow.py on MI355X (prisma's DEFAULT flow band, process.py:23).

Same CLI (reference :223-255; the GMFlow architecture flags are accepted and must equal the band's defaults, which is the model the
engine builds, or the one flag set of GMFlow's refinement model, REFINE below; the two inference-time radii are honoured: --corr_radius_list R, 1 .. 4, selects local matching over (2 R + 1)^2 target
tokens and --prop_radius_list r, 1 .. 2, local-window flow propagation, -1 = global, reference bands/gmflow/gmflow.py:128-157), same outputs
(<BAND>.mp4, <BAND>.csv with the per-frame max displacement, optional <BAND>_bwd / _mask / _mask_bwd
videos, .flo / 16-bit PNG dumps, metadata entries :195-218), same module API (BAND, init_model(), infer()).  The frame loop, the file
writers and the multi-rank relay are the ones flow_raft uses (bands/common/flow.py process_video: the two reference scripts share them line
for line, flow_gmflow.py:121-218 vs flow_raft.py:69-166); the model is libprisma_bands.so's GmflowEngine through prisma_amd.engine.FlowGMFlow.

--backwards / --mask with a matching radius: the reference raises there (pred_bidir_flow: local_correlation_softmax returns B flows while
the features were concatenated to 2 B, gmflow.py:142,153-157).  This band computes the backward direction as the forward direction of the
swapped pair, which is what pred_bidir_flow equals wherever the reference can run it (global matching, either propagation).

--num_scales 2 is GMFlow's two-scale refinement model (gmflow_with_refine_*), with exactly the reference's flag set for it:
  --num_scales 2 --upsample_factor 4 --padding_factor 32 --attn_splits_list 2 8 --corr_radius_list -1 R --prop_radius_list -1 r
(R in 1 .. 4, r in 1 .. 2: the fine scale's radii; the coarse scale is global) and a checkpoint - or --synthetic weights - that is two-scale.
The engine reads the architecture from the weights; a mismatch between the flags and the checkpoint is refused before anything runs.
--num_scales 2 on its own, other split counts and other flag mixes stay refused.
"""
import argparse
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from common import flow  # noqa: E402
from common.ckpt import load_checkpoint  # noqa: E402
from common.cli import begin, end, synthetic_or_exit  # noqa: E402
from prisma_amd import engine, shard, synth  # noqa: E402

BAND = "flow_gmflow"
MODEL = "models/gmflow_sintel-0c07dcb3.pth"      # reference :35
CHUNK = int(os.environ.get("PRISMA_BATCH", "16"))
STREAM_MIN_CHUNKS = 16      # PRISMA_STREAM unset: the streamed loop for shards of at least this many chunks (EXPERIMENTS.md 6.19: slower on 6, faster on 16)
# the model flags of reference :239-249 and the only values the engine implements (the band's defaults); corr_radius_list and
# prop_radius_list are also taken as one radius each (RADII: the largest the engine's kernels are built for)
ARCH = {"feature_channels": 128, "num_scales": 1, "upsample_factor": 8, "num_head": 1, "attention_type": "swin", "ffn_dim_expansion": 4,
        "num_transformer_layers": 6, "attn_splits_list": [2], "corr_radius_list": [-1], "prop_radius_list": [-1], "padding_factor": 16}

RADII = {"corr_radius_list": 4, "prop_radius_list": 2}
# the refinement model's flag set (reference :46-53, 84-89 with gmflow_with_refine_*): the second entry of the two radius lists is the fine
# scale's radius, 1 .. RADII
REFINE = {"num_scales": 2, "upsample_factor": 4, "padding_factor": 32, "attn_splits_list": [2, 8]}

model = None
data = None
ranks = None
_SYNTH = [False]
_SCALES = [1]               # what the flags ask for: the synthetic weights are made to match


def load_weights(path):
    """reference :57-61: torch.load(checkpoint)['model'] if present, else the dict itself."""
    if path and os.path.exists(path):
        return load_checkpoint(path, wrappers=("model",))
    synthetic_or_exit(BAND, f"checkpoint {path!r} not found", "--model", _SYNTH[0])
    return synth.gmflow_weights(seed=2468, num_scales=_SCALES[0])


def radius(args, key):
    """the one radius of a --corr_radius_list / --prop_radius_list (-1 = global); with two scales the fine scale's (the list's second entry)"""
    v = getattr(args, key, None) if args is not None else None
    return int(v[-1]) if v else -1


def two_scale(args):
    """the flags are the refinement model's set (REFINE and two radius lists [-1, radius])"""
    if args is None or any(getattr(args, k, None) != v for k, v in REFINE.items()):
        return False
    return all((lambda v: v is not None and len(v) == 2 and v[0] == -1 and 1 <= v[1] <= top)(getattr(args, k, None)) for k, top in RADII.items())


def weights_scales(w):
    """1 or 2: what the engine will read from these weights (upsampler.2 of 4 * 4 * 9 rows and the backbone's trident convolution)"""
    return 2 if "backbone.trident_conv.weight" in w and np.asarray(w["upsampler.2.weight"]).shape[0] == 144 else 1


def check_arch(args):
    isz = getattr(args, "inference_size", None)
    if two_scale(args):
        bad = {k: getattr(args, k) for k, v in ARCH.items() if hasattr(args, k) and getattr(args, k) != v and k not in RADII and k not in REFINE}
        if bad:                                          # the refinement model shares every other architecture flag with the default one
            raise SystemExit(f"[{BAND}] only the band's default GMFlow is built ({ARCH}), or its refinement flag set ({REFINE}); got {bad}")
        if isz and (len(isz) != 2 or any(v < 64 or v % 32 for v in isz)):
            raise SystemExit(f"[{BAND}] --inference_size takes H W, multiples of 32 with --num_scales 2 (4 x the fine scale's 8 x 8 window split); got {isz}")
        return
    if getattr(args, "num_scales", 1) == 2:              # the refinement model's flag set, or nothing of it
        raise SystemExit(f"[{BAND}] --num_scales 2 takes exactly --upsample_factor 4 --padding_factor 32 --attn_splits_list 2 8 --corr_radius_list -1 R "
                         f"(R in 1 .. {RADII['corr_radius_list']}) --prop_radius_list -1 r (r in 1 .. {RADII['prop_radius_list']}); besides it "
                         f"only the band's default GMFlow is built ({ARCH}); got "
                         f"{ {k: getattr(args, k) for k in list(REFINE) + list(RADII) if hasattr(args, k)} }")
    bad = {k: getattr(args, k) for k, v in ARCH.items() if hasattr(args, k) and getattr(args, k) != v and k not in RADII}
    for k, top in RADII.items():
        v = getattr(args, k, None)
        if v is not None and (len(v) != 1 or not (v[0] == -1 or 1 <= v[0] <= top)):
            raise SystemExit(f"[{BAND}] --{k} takes one radius (one scale): -1 (global) or 1 .. {top}; got {v}")
    if bad:
        raise SystemExit(f"[{BAND}] only the band's default GMFlow is built ({ARCH}); got {bad}")
    if isz and (len(isz) != 2 or any(v < 32 or v % 16 for v in isz)):
        raise SystemExit(f"[{BAND}] --inference_size takes H W, multiples of 16 (the reference's 2 x 2 window split of the 1/8 grid fails otherwise); got {isz}")


def init_model(args=None, device=0):
    global model
    if args is not None:
        check_arch(args)
        _SYNTH[0] = bool(getattr(args, "synthetic", False))
    _SCALES[0] = 2 if two_scale(args) else 1
    weights = load_weights(getattr(args, "model", MODEL) if args else MODEL)
    if weights_scales(weights) != _SCALES[0]:             # before anything runs: the engine would build what the weights say, not what the flags say
        raise SystemExit(f"[{BAND}] the flags ask for the {_SCALES[0]}-scale model but the checkpoint is a {weights_scales(weights)}-scale one "
                         f"(backbone.trident_conv.weight and an upsampler.2.weight of 144 rows make a two-scale checkpoint; --num_scales 2 takes "
                         f"--upsample_factor 4 --padding_factor 32 --attn_splits_list 2 8 --corr_radius_list -1 R --prop_radius_list -1 r)")
    model = engine.FlowGMFlow(weights, device=device)
    assert model.num_scales == _SCALES[0]
    model.set_inference_size(getattr(args, "inference_size", None) if args is not None else None)      # reference :76-100
    model.set_matching(radius(args, "corr_radius_list"), radius(args, "prop_radius_list"))              # reference :84-89
    return model


def infer(args, image1, image2):
    """Reference signature (:66-118): image1 = prev, image2 = curr as float CHW 0..255 tensors (already scaled).
    Returns (fwd, bwd | None, fwd_mask | None, bwd_mask | None), flows as float32 [H', W', 2]."""
    if model is None:
        init_model(args)
    a = np.ascontiguousarray(np.asarray(image1).transpose(1, 2, 0)).astype(np.uint8)
    b = np.ascontiguousarray(np.asarray(image2).transpose(1, 2, 0)).astype(np.uint8)
    want_mask = bool(getattr(args, "output_mask", "") or getattr(args, "subpath_mask", ""))
    if want_mask:
        flow, _, _, mask = model.infer_sequence_masks(np.stack([a, b]), scale=1.0, want_rgb=False)
        return flow[0, 0], flow[0, 1], mask[0, 0], mask[0, 1]
    both = bool(getattr(args, "backwards", False))
    flow, _, _ = model.infer_sequence(np.stack([a, b]), scale=1.0, backward=both, want_rgb=False)
    return flow[0, 0], (flow[0, 1] if both else None), None, None


def process_video(args):
    """The flow bands' loop (common/flow.py) with this band's name, model, metadata and ranks as they are now.  The backward flow is predicted
    only when it is asked for; GMFlow is not iterative: the engine ignores the count the loop passes through."""
    rk = ranks or shard.Ranks()
    if model is None:
        init_model(args, device=rk.device)
    flow.process_video(args, BAND, model, data, rk, CHUNK, subpath_needs_both=False, iterations=1, stream_min_chunks=STREAM_MIN_CHUNKS)


def main(argv=None):
    global data, ranks
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", "-i", help="input", type=str, required=True)
    ap.add_argument("--output", "-o", help="output", type=str, default="")
    ap.add_argument("--subpath", help="path to flo files", type=str, default="")
    ap.add_argument("--backwards", "-b", help="Backward video", action="store_true")
    ap.add_argument("--mask", action="store_true", help="Compute mask as well")
    ap.add_argument("--output_mask", help="output dense", type=str, default="")
    ap.add_argument("--subpath_mask", help="path to flo files", type=str, default="")
    ap.add_argument("--scale", type=float, default=0.75)
    ap.add_argument("--model", "-m", help="model path", type=str, default=MODEL)
    ap.add_argument("--feature_channels", default=128, type=int)
    ap.add_argument("--num_scales", default=1, type=int)
    ap.add_argument("--upsample_factor", default=8, type=int)
    ap.add_argument("--num_head", default=1, type=int)
    ap.add_argument("--attention_type", default="swin", type=str)
    ap.add_argument("--ffn_dim_expansion", default=4, type=int)
    ap.add_argument("--num_transformer_layers", default=6, type=int)
    ap.add_argument("--attn_splits_list", default=[2], type=int, nargs="+")
    ap.add_argument("--corr_radius_list", default=[-1], type=int, nargs="+")
    ap.add_argument("--prop_radius_list", default=[-1], type=int, nargs="+")
    ap.add_argument("--strict_resume", action="store_true")
    ap.add_argument("--inference_size", default=None, type=int, nargs="+")
    ap.add_argument("--padding_factor", default=16, type=int)
    ap.add_argument("--local_rank", default=0, type=int)
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights when the checkpoint is missing (tests / benchmarks)")
    args = ap.parse_args(argv)
    check_arch(args)
    data, loaded, meta_path, ranks = begin(args, BAND, flow=True)
    init_model(args, device=ranks.device)
    process_video(args)
    end(ranks, meta_path, data, loaded)


if __name__ == "__main__":
    main()
