#!/usr/bin/env python3
"""mask (mmdet / SOLOv2) band - drop-in for /root/reference/bands/mask_mmdet.py on MI355X.

Same CLI (reference :164-199), same outputs (mask.png | mask.mp4 with the accumulated instance masks of the 11
animate COCO classes, optional COLMAP black/white frames in --subpath, optional SDF in the green channel,
metadata entry `bands.mask = {url, ids}` :113-115,158-161), same module-level names (BAND, CLASSES, init_model()).
mmdet's init_detector / inference_detector are replaced by libprisma_bands.so through prisma_amd.engine; frames
are pushed in batches instead of one by one.
"""
import argparse
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from common.io import FrameReader, VideoWriter, create_folder, is_planar, open_rgb, planar_out, write_rgb  # noqa: E402
from common.ckpt import load_checkpoint  # noqa: E402
from common.cli import begin, end, synthetic_or_exit  # noqa: E402
from common.loop import Stream, frame_formats, run_sharded, stream_enabled  # noqa: E402
from common.yuv import yuv_bytes  # noqa: E402
from common.meta import is_video  # noqa: E402
from prisma_amd import engine, shard, synth  # noqa: E402

BAND = "mask"
MODEL = "models/solov2_r101_fpn_3x_coco_20220511_095119-c559a076.pth"
CLASSES = list(synth.BAND_CLASSES)
CONFIDENCE_THRESHOLD = 0.5
BATCH = int(os.environ.get("PRISMA_BATCH", "32"))
STREAM_MIN_CHUNKS = 16      # PRISMA_STREAM unset: the streamed loop for shards of at least this many chunks (EXPERIMENTS.md 6.19: slower on 6, faster on 16)

model = None
data = None
_SYNTH = [False]      # --synthetic
ranks = None          # shard.Ranks(): one process per GPU under torchrun, world 1 otherwise


def load_weights(path, cfg):
    """mmdet checkpoints keep the tensors under 'state_dict'."""
    if path and os.path.exists(path):
        return load_checkpoint(path, wrappers=("state_dict",))
    synthetic_or_exit(BAND, f"checkpoint {path!r} not found", "--weights", _SYNTH[0])
    return synth.solov2_weights(cfg)


def init_model(arch="r101", weights=MODEL, device=0, max_batch=BATCH):
    global model
    cfg = synth.MASK_CFGS[arch]
    model = engine.MaskMMDet(load_weights(weights, cfg), cfg, device=device, max_batch=max_batch)
    model.CLASSES = synth.COCO_CLASSES
    return model


def keep_ids():
    return [synth.COCO_CLASSES.index(c) for c in CLASSES]


def set_sdf(on):
    """--sdf (reference :64-69,150-152; process.py passes it on every run): the engine writes the clamped signed distance field of
    each id image into its green channel on the GPU (engine.MaskMMDet.set_sdf; the host restatement the tests compare it with is
    oracle/solov2_oracle.py band_sdf)."""
    model.set_sdf(bool(on))


def _colmap(masks_u8):
    """COLMAP wants black objects on white (reference :149-150 writes 255 - masks BEFORE the SDF goes into G): the id image has the
    same byte in all three channels, so the pre-SDF image is its red channel three times."""
    return 255 - np.repeat(masks_u8[..., :1], 3, axis=-1)


def process_image(args):
    img = open_rgb(args.input)
    set_sdf(args.sdf)
    masks = model.infer_batch(img[None], args.confidence, keep_ids())[0]
    write_rgb(args.output, masks)
    data["bands"][BAND] = {"url": os.path.basename(args.output), "ids": CLASSES}


def process_video(args):
    """Frames shard by rank (no cross-frame state, reference :131-154).  Rank 0 writes its own chunks to the video as they
    finish (sink thread) and then muxes the other ranks' chunks in frame order through shard.Relay; nothing is gathered
    and no list holds the whole video."""
    rk = ranks or shard.Ranks()
    src = FrameReader(args.input)
    n = len(src)
    h, w = src[0].shape[:2]
    if args.subpath:
        args.subpath = os.path.join(os.path.dirname(args.output), args.subpath)
        create_folder(args.subpath)
    first, last = rk.frames(n)
    ofmt = planar_out(args.output, getattr(src, "format", None))      # the layout written: PRISMA_Y4M_OUT's (I420 when unset), or an .avi / .mjpeg's JPEG planes
    out = VideoWriter(width=w, height=h, frame_rate=src.rate, filename=args.output, fmt=ofmt, device=rk.device) if rk.main else None
    set_sdf(args.sdf)
    # a .y4m on either side: its planes go to / come from the engine as they are - but the COLMAP dump needs the id images' red channel, so
    # with --subpath they come back as RGB and the video's frames are converted on the host
    yin, yout = src.i420, is_planar(args.output) and not args.subpath
    fmt = frame_formats(model, yin, yout, h, w, getattr(src, "format", None), ofmt)
    out_bytes = yuv_bytes(ofmt, h, w) if yout else h * w * 3
    frame = ((src.frame_bytes,), np.uint8) if yin else (src[0].shape, np.uint8)       # a .y4m's planes, in the clip's own layout

    def step(_s, frames):            # the SDF, if asked for, is already in G: set_sdf
        masks = model.infer_batch(frames, args.confidence, keep_ids(), **fmt)
        return {"mask": masks}, masks, None

    # the streamed loop (common/loop.py).  There is no asynchronous mask call (include/prisma_bands.h: SOLOv2 synchronises with the host many
    # times per call, its candidate counts depend on the data): "submit" is the blocking call, which pipelines its own chunks and addresses the
    # page-locked ring slots directly - no staging copy in, none out - and "wait" has nothing left to wait for
    def submit(_s, frames, res):
        model.infer_batch(frames, args.confidence, keep_ids(), out=res["mask"], **fmt)

    def collect(_s, res):
        return {"mask": res["mask"]}, res["mask"], None

    def write_chunk(_s, c):          # rank 0 only: the video frames, chunk after chunk in order
        for f in c["mask"]:
            out.write_planes(f, h, w) if yout else out.write(f)

    def dump(s, masks):              # sink thread: the COLMAP frames
        for j in range(len(masks)):
            write_rgb(os.path.join(args.subpath, "{:05d}.png".format(s + j)), _colmap(masks[j]))

    stream = Stream(model, frame, {"mask": ((out_bytes,) if yout else (h, w, 3), np.uint8)}, submit, collect, wait=lambda: None, i420=yin) if stream_enabled(STREAM_MIN_CHUNKS, -(-(last - first) // BATCH)) else None
    run_sharded(rk, src, n, BATCH, 0, args.output, (n - (last - first)) * out_bytes, step, write_chunk, dump if args.subpath else None,
                stream=stream, i420=yin)
    if not rk.main:
        return
    out.close()
    # the reference replaces the whole entry here, which also drops the `folder` key it set earlier (:127-129,158-161)
    data["bands"][BAND] = {"url": os.path.basename(args.output), "ids": CLASSES}


def main(argv=None):
    global data, ranks
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", "-i", help="input", type=str, required=True)
    ap.add_argument("--output", "-o", help="output", type=str, default="")
    ap.add_argument("--confidence", "-c", help="confidence threshold", type=float, default=CONFIDENCE_THRESHOLD)
    ap.add_argument("--sdf", "-s", help="Encode SDF on GREEN channel", action="store_true")
    ap.add_argument("--subpath", help="Mask Subpath to frames", type=str, default="")
    ap.add_argument("--arch", help="backbone / geometry preset (prisma_amd.synth.MASK_CFGS)", default="r101")
    ap.add_argument("--weights", help="mmdet checkpoint (.pth) or .npz state dict", default=MODEL)
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights when the checkpoint is missing (tests / benchmarks)")
    args = ap.parse_args(argv)
    _SYNTH[0] = args.synthetic
    data, loaded, meta_path, ranks = begin(args, BAND)
    if not data:
        data = {"bands": {}}
    init_model(args.arch, args.weights, device=ranks.device)
    if is_video(args.output):
        process_video(args)
    elif ranks.main:
        process_image(args)
    end(ranks, meta_path, data, loaded)


if __name__ == "__main__":
    main()
