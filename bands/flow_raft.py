#!/usr/bin/env python3
"""flow_raft band - drop-in for /root/reference/bands/flow_raft.py on MI355X.

Same CLI (reference :169-225), same outputs (<BAND>.mp4, <BAND>.csv with the per-frame max
displacement, optional <BAND>_bwd.mp4, metadata entries :143-166), same module API (BAND, init_model(),
infer()).  Frames are pushed to libprisma_bands.so in overlapping chunks; every frame is encoded by
fnet / cnet once instead of twice per pair.
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

BAND = "flow_raft"
MODEL = "models/raft-sintel.pth"            # reference :31
ITERATIONS = 20
CHUNK = int(os.environ.get("PRISMA_BATCH", "16"))
STREAM_MIN_CHUNKS = 16      # PRISMA_STREAM unset: the streamed loop for shards of at least this many chunks (EXPERIMENTS.md 6.19: slower on 6, faster on 16)

model = None
data = None
_SYNTH = [False]      # --synthetic
ranks = None          # shard.Ranks(): one process per GPU under torchrun, world 1 otherwise


def load_weights(path):
    """Checkpoint keys carry a `module.` prefix from DataParallel (reference :42-44): strip it."""
    if path and os.path.exists(path):
        return load_checkpoint(path, strip_prefix="module.")
    synthetic_or_exit(BAND, f"checkpoint {path!r} not found", "--model", _SYNTH[0])
    return synth.raft_weights(seed=4321)


def init_model(args=None, device=0):
    global model
    if args is not None and getattr(args, "small", False):
        # reference raft.py:28-53: both `if args.small:` branches sit inside string literals (dead code) - RAFT(args) builds BasicEncoder /
        # BasicUpdateBlock (hidden 128, corr radius 4, 5.26 M parameters) whatever the flag says, and loads args.model into it.  Drop-in
        # behaviour is therefore: accept the flag, run the basic model (round 4 refused it as "another network"; it never was one here)
        print(f"[{BAND}] --small: the reference builds the basic RAFT regardless (bands/raft/raft.py:28-53, the small branches are commented out); flag ignored", file=sys.stderr)
    if args is not None and getattr(args, "mixed_precision", False):
        print(f"[{BAND}] --mixed_precision: the engine's precision is set by PRISMA_PRECISION (split-fp16 by default); flag ignored", file=sys.stderr)
    _SYNTH[0] = bool(getattr(args, "synthetic", False))
    model = engine.FlowRaft(load_weights(getattr(args, "model", MODEL) if args else MODEL), device=device)
    if args is not None and getattr(args, "alternate_corr", False):
        # reference raft.py:103-106, corr.py:63-91 (AlternateCorrBlock): the correlations of every lookup window are computed from the feature
        # maps when they are needed, and the all-pairs volume - 4 P^2 / 3 fp16 entries per pair and direction, 45 GB for a 2160p frame - is
        # never built.  Same flows within the band's tolerance (a window entry is not rounded to fp16 on the way)
        model.set_alternate_corr(True)
        print(f"[{BAND}] --alternate_corr: correlation windows computed on the fly, no all-pairs volume in memory", file=sys.stderr)
    return model


def infer(args, image1, image2):
    """Reference signature (:51-66): image1 = [prev, curr], image2 = [curr, prev] as float CHW 0..255 (already
    scaled).  Returns (fwd, bwd, None, None) with flows as float32 [H', W', 2]."""
    if model is None:
        init_model(args)
    a = np.ascontiguousarray(np.asarray(image1)[0].transpose(1, 2, 0)).astype(np.uint8)
    b = np.ascontiguousarray(np.asarray(image2)[0].transpose(1, 2, 0)).astype(np.uint8)
    if getattr(args, "output_mask", "") or getattr(args, "subpath_mask", ""):
        flow, _, _, mask = model.infer_sequence_masks(np.stack([a, b]), scale=1.0, iters=args.iterations, want_rgb=False)
        return flow[0, 0], flow[0, 1], mask[0, 0], mask[0, 1]
    flow, _, _ = model.infer_sequence(np.stack([a, b]), scale=1.0, iters=args.iterations, backward=True, want_rgb=False)
    return flow[0, 0], flow[0, 1], None, None


def process_video(args):
    """The flow bands' loop (common/flow.py) with this band's name, model, metadata and ranks as they are now.  RAFT always predicts both
    directions for the --subpath dumps; the iterations are the command line's."""
    rk = ranks or shard.Ranks()
    if model is None:
        init_model(args, device=rk.device)
    flow.process_video(args, BAND, model, data, rk, CHUNK, subpath_needs_both=True, iterations=args.iterations, stream_min_chunks=STREAM_MIN_CHUNKS)


def main(argv=None):
    global data, ranks
    ap = argparse.ArgumentParser()
    ap.add_argument("-input", "-i", "--input", dest="input", help="input", type=str, required=True)
    ap.add_argument("-output", "-o", "--output", dest="output", help="output", type=str, default="")
    ap.add_argument("--subpath", "-d", help="Subpath to frames", type=str, default="")
    ap.add_argument("--backwards", "-b", help="Backward video", action="store_true")
    ap.add_argument("--mask", help="Compute consistency mask", action="store_true")
    ap.add_argument("--output_mask", help="Mask video", type=str, default="")
    ap.add_argument("--subpath_mask", help="Subpath to mask frames", type=str, default="")
    ap.add_argument("--iterations", help="number of iterations", type=int, default=ITERATIONS)
    ap.add_argument("--model", "-m", help="model path", type=str, default=MODEL)
    ap.add_argument("--scale", type=float, default=0.75, help="scale factor")
    # reference :184: parsed and never read (init_model loads args.model, :40) - accepted so a reference command line runs unchanged
    ap.add_argument("--raft_model", default="models/raft-things.pth", help="[RAFT] restore checkpoint (unused by the reference as well)")
    ap.add_argument("--small", action="store_true", help="use small model")
    ap.add_argument("--mixed_precision", action="store_true", help="use mixed precision")
    ap.add_argument("--alternate_corr", action="store_true", help="use efficent correlation implementation")
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights when the checkpoint is missing (tests / benchmarks)")
    args = ap.parse_args(argv)
    data, loaded, meta_path, ranks = begin(args, BAND, flow=True)
    init_model(args, device=ranks.device)
    process_video(args)
    end(ranks, meta_path, data, loaded)


if __name__ == "__main__":
    main()
