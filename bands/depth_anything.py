#!/usr/bin/env python3
"""depth_anything band - drop-in for /root/reference/bands/depth_anything.py on MI355X.

Same CLI (reference :254-292), same outputs (<BAND>.mp4|png, <BAND>_min.csv, <BAND>_max.csv,
metadata.json entries, :157-166, :232-251), same module-level API (BAND, init_model(), infer()).
The PyTorch model and the numpy post-process are replaced by libprisma_bands.so through
prisma_amd.engine (C ABI, include/prisma_bands.h); frames are pushed in batches instead of one by one.
"""
import argparse
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from common.io import FrameReader, VideoWriter, create_folder, is_planar, open_rgb, planar_out, write_ply, write_rgb  # noqa: E402
from common.ckpt import load_checkpoint  # noqa: E402
from common.cli import begin, end, synthetic_or_exit  # noqa: E402
from common.loop import Stream, frame_formats, run_sharded, stream_enabled  # noqa: E402
from common.yuv import yuv_bytes  # noqa: E402
from common.meta import is_video  # noqa: E402
from prisma_amd import engine, shard, synth  # noqa: E402

BAND = "depth_anything"
BATCH = int(os.environ.get("PRISMA_BATCH", "32"))
STREAM_MIN_CHUNKS = 16      # PRISMA_STREAM unset: the streamed loop for shards of at least this many chunks (EXPERIMENTS.md 6.19: slower on 6, faster on 16)

model = None
data = None
args = None
ranks = None          # shard.Ranks(): one process per GPU under torchrun, world 1 otherwise
_still = None         # engine.Ops ctx of the still-image encodes (write_depth_png)


def heat_to_rgb(heat):
    """bands/common/encode.py:13-33 on the host: the ramp common.io.write_depth takes as an argument (tests compare the GPU encodes
    with it; both the video path and the still-image path encode on the GPU)."""
    hue = (1.0 - np.asarray(heat, np.float64)) * 0.65
    rgb = np.stack([hue * 6.0, hue * 6.0 + 4.0, hue * 6.0 + 2.0], axis=-1)
    return np.clip(np.abs(np.mod(rgb, 6.0) - 3.0) - 1.0, 0.0, 1.0)


def load_weights(encoder, path=""):
    """{reference state_dict name: float32 ndarray}.  The reference pulls LiheYoung/depth_anything_*14
    from the HF hub (:60); offline we read models/depth_anything_<enc>14.{npz,pth} if present and fall
    back to the seeded synthetic weights ONLY with --synthetic / PRISMA_SYNTH=1 (tests, benchmarks); otherwise a missing
    checkpoint is an error."""
    cands = [path] if path else [os.path.join("models", f"depth_anything_{encoder}14.npz"),
                                 os.path.join("models", f"depth_anything_{encoder}14.pth")]
    for c in cands:
        if c and os.path.exists(c):
            return load_checkpoint(c)
    synthetic_or_exit(BAND, f"no checkpoint found ({cands})", "--weights", getattr(args, "synthetic", False))
    return synth.depth_anything_weights(encoder, seed=1234)


def init_model(encoder=None, weights="", device=0, max_batch=BATCH):
    global model
    encoder = encoder or (args.encoder if args else "vitl")
    metric = getattr(args, "metric", "none") if args is not None else "none"
    if metric != "none":
        # reference :52-57: ZoeDepth (eval config) over the ViT-L core, checkpoints models/depth_anything_metric_depth_{indoor,outdoor}.pt
        path = weights or os.path.join("models", f"depth_anything_metric_depth_{metric}.pt")
        model = engine.DepthAnything(load_metric_weights(path), "vitl", device=device, max_batch=max_batch, metric=True)
    else:
        model = engine.DepthAnything(load_weights(encoder, weights), encoder, device=device, max_batch=max_batch)
    return model


def load_metric_weights(path):
    """ZoeDepth state dict (`core.core.*` + the metric head); `model_io.load_state_from_resource` keeps it under 'model'."""
    if path and os.path.exists(path):
        return load_checkpoint(path, wrappers=("model",))
    synthetic_or_exit(BAND, f"metric checkpoint {path!r} not found", "--weights", getattr(args, "synthetic", False), what="")
    return synth.zoe_weights()


def _flip():
    """The relative model encodes near = hot (flip), the metric models do not (reference :150,188)."""
    return getattr(args, "metric", "none") == "none" if args is not None else True


def infer(img, normalize=False):
    """uint8 RGB HxWx3 -> float32 HxW relative depth (reference :100-143)."""
    if model is None:
        init_model()
    return model.infer(img, normalize=normalize)


def write_depth_png(path, depth):
    """write_depth(path, depth, normalize=True, flip, heatmap=True, encode_range=True) (reference :176-180, :221-225;
    bands/common/io.py:138-172) with the encode on the GPU (pb_depth_encode_still): bytes equal common.io.write_depth's."""
    rgb, _, _ = _still_ctx().encode_still(depth, flip=_flip(), encode_range=True)
    write_rgb(path, rgb)


def _still_ctx():
    global _still
    if _still is None:      # its own ctx and stream: the --subpath dumps run on the sink thread while the band's ctx computes the next chunk
        _still = engine.Ops(device=ranks.device if ranks else 0)
    return _still


def write_depth_ply(path, depth, img):
    """write_pcl(path, depth, img, flip) (reference :170-171; bands/common/io.py:201-211, bands/common/geom.py:5-47: u0 = W / 2, v0 = H / 2,
    fx = fy = 1000) with the un-flip, the 5 x 5 median and the back-projection on the GPU (pb_depth_point_cloud) and the binary PLY
    written here (common.io.write_ply).  cv2.medianBlur and plyfile's header are pinned by restatement (tests/pcl_ref.py): neither
    package is installed where this is tested."""
    h, w = depth.shape
    write_ply(path, _still_ctx().point_cloud(depth, img, flip=_flip(), u0=w / 2, v0=h / 2, fx=1000.0, fy=1000.0))


def process_image(a):
    img = open_rgb(a.input)
    out_folder = os.path.dirname(a.output)
    pred = infer(img)
    if data:
        data["bands"][BAND]["values"] = {"min": {"value": float(pred.min()), "type": "float"},
                                         "max": {"value": float(pred.max()), "type": "float"}}
    if a.npy:
        np.save(os.path.join(out_folder, BAND + ".npy"), pred)
    if getattr(a, "ply", False):
        write_depth_ply(os.path.join(out_folder, BAND + ".ply"), pred, img)
    write_depth_png(a.output, pred)


def process_video(a):
    """Frames shard by rank: every rank encodes its contiguous block on its own GPU.  Rank 0 writes its own
    chunks to the video as they finish and then muxes the other ranks' chunks in frame order (shard.Relay: one chunk in
    memory at a time, nothing gathered); only the per-frame (min, max) scalars go through a collective."""
    rk = ranks or shard.Ranks()
    if getattr(a, "ply", False):
        print(f"[{BAND}] --ply only applies to still images (reference :168-174); ignored for video", file=sys.stderr)
    src = FrameReader(a.input)
    n = len(src)
    h, w = src[0].shape[:2]
    # a .y4m on either side, an .avi / .mjpeg out: its planes go to / come from the engine as they are
    yin, yout = src.i420, is_planar(a.output)
    ofmt = planar_out(a.output, getattr(src, "format", None))      # the layout written: PRISMA_Y4M_OUT's (I420 when unset), or the JPEG's planes
    out = VideoWriter(width=w, height=h, frame_rate=src.rate, filename=a.output, fmt=ofmt, device=rk.device) if rk.main else None
    out_bytes = yuv_bytes(ofmt, h, w) if yout else h * w * 3
    out_folder = os.path.dirname(a.output)
    if a.subpath:
        if data:
            data["bands"][BAND]["folder"] = a.subpath
        a.subpath = os.path.join(out_folder, a.subpath)
        create_folder(a.subpath)
    if model is None:
        init_model(device=rk.device)
    first, last = rk.frames(n)
    want_depth = bool(a.npy or a.subpath)
    fmt = frame_formats(model, yin, yout, h, w, getattr(src, "format", None), ofmt)
    frame = ((src.frame_bytes,), np.uint8) if yin else (src[0].shape, np.uint8)       # a .y4m's planes, in the clip's own layout

    def step(_s, frames):
        depth, rgb, mn, mx = model.infer_batch(frames, want_depth=want_depth, want_rgb=True, flip=_flip(), **fmt)
        return {"rgb": rgb}, depth, np.stack([mn, mx], 1)

    # the streamed loop (common/loop.py): the same call as submit_batch / wait on the loop's page-locked rings - one array per result asked for
    results = {"rgb": ((out_bytes,) if yout else (h, w, 3), np.uint8), "mn": ((), np.float32), "mx": ((), np.float32)}
    if want_depth:
        results["depth"] = ((h, w), np.float32)

    def submit(_s, frames, res):
        model.submit_batch(frames, out_rgb=res["rgb"], out_depth=res.get("depth"), out_min=res["mn"], out_max=res["mx"], flip=_flip(), **fmt)

    def collect(_s, res):
        return {"rgb": res["rgb"]}, res.get("depth"), np.stack([res["mn"], res["mx"]], 1)

    def write_chunk(_s, c):          # rank 0 only: the video frames, chunk after chunk in order
        for f in c["rgb"]:
            out.write_planes(f, h, w) if yout else out.write(f)

    def dump(s, depth):              # sink thread: .npy / .png dumps (reference :215-225); nothing of `depth` is kept past the return
        for j in range(len(depth)):
            if a.npy:
                np.save(os.path.join(a.subpath, "{:05d}.npy".format(s + j)), depth[j])
            write_depth_png(os.path.join(a.subpath, "{:05d}.png".format(s + j)), depth[j])

    stream = Stream(model, frame, results, submit, collect, i420=yin) if stream_enabled(STREAM_MIN_CHUNKS, -(-(last - first) // BATCH)) else None
    mm = run_sharded(rk, src, n, BATCH, 0, a.output, (n - (last - first)) * out_bytes, step, write_chunk,
                     dump if a.subpath else None, n_scalars=2, ctx=model, stream=stream, i420=yin)
    if not rk.main:
        return
    lo, hi = [float(v) for v in mm[:, 0]], [float(v) for v in mm[:, 1]]
    out.close()
    with open(os.path.join(out_folder, BAND + "_min.csv"), "w") as f:
        f.writelines("{}\n".format(v) for v in lo)
    with open(os.path.join(out_folder, BAND + "_max.csv"), "w") as f:
        f.writelines("{}\n".format(v) for v in hi)
    if data:
        data["bands"][BAND]["values"] = {"min": {"type": "float", "url": BAND + "_min.csv"},
                                         "max": {"type": "float", "url": BAND + "_max.csv"}}


def main(argv=None):
    global args, data, ranks
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", "-i", help="Input image/video", type=str, required=True)
    ap.add_argument("--output", "-o", help="Output image/video", type=str, default="")
    ap.add_argument("--npy", "-n", help="Save numpy data", action="store_true")
    ap.add_argument("--ply", "-p", help="Create point cloud PLY", action="store_true")
    ap.add_argument("--subpath", "-d", help="subpath to frames", type=str, default="")
    ap.add_argument("--encoder", type=str, default="vitl", choices=["vits", "vitb", "vitl"])
    ap.add_argument("--metric", help="Use a metric model", type=str, default="none", choices=["none", "indoor", "outdoor"])
    ap.add_argument("--weights", help="checkpoint (.npz / .pth state dict); default models/depth_anything_<encoder>14.*", default="")
    ap.add_argument("--synthetic", help="seeded synthetic weights when no checkpoint is found (tests / benchmarks)", action="store_true")
    args = ap.parse_args(argv)
    data, loaded, meta_path, ranks = begin(args, BAND)
    init_model(args.encoder, args.weights, device=ranks.device)
    if is_video(args.output):
        process_video(args)
    elif ranks.main:
        process_image(args)
    end(ranks, meta_path, data, loaded)


if __name__ == "__main__":
    main()
