#!/usr/bin/env python3
"""rgba band: bring the input into the prisma folder as rgba.png / rgba.mp4 (what every other band reads).

Re-statement of /root/reference/bands/rgba.py, same flags.  Plain path (process_image :104-110: open_float_rgb -> write_rgb as PNG;
process_video -> prune :77-101): frame pass-through that drops audio, optional --subpath frame dump `255 - frame`.  No model, no GPU.

RGB-D path (--rgbd left|right|top|bottom: where the depth is; split :24-75, process_video :112-128): side-by-side captures - Record3D's
iPhone LiDAR videos in particular - are cut in two.  The colour half goes to --output (rgba.<ext>), the other half to
<folder of --output>/<--output_depth>.<ext> (:173) and into metadata.json as band `depth`.  With --encoding_depth hue the depth half is
hue-coded: it is decoded and re-encoded in prisma's heat ramp (:61-63) on the GPU (engine.rgbd_depth, hue_heat_kernel; bytes equal the
reference's float64 numpy on every colour) in chunks whose decode, kernel and file writes overlap (common/pipe.py); with `none` it is a
crop like the colour half and no GPU is touched.  As in the reference the frame rate is truncated to an integer on this path only
(:113, 127), .mp4 writers get the halves' sizes as W / 2 and H / 2 (:54-55), and --rgbd is ignored for still images (process_image).
--subpath / --subpath_depth dump `255 - frame` PNGs of their half (the reference forgets to hand subpath_depth to split(); it is
honoured here).
"""
import argparse
import copy
import os
import shutil
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common.io import FrameReader, VideoWriter, check_overwrite, create_folder, open_rgb, write_rgb  # noqa: E402
from common.meta import add_band, get_target, is_video, load_metadata, merge_metadata  # noqa: E402
from common.loop import chunks  # noqa: E402
from common.pipe import AsyncSink  # noqa: E402

BAND = "rgba"
CHUNK = int(os.environ.get("PRISMA_BATCH", "32"))      # frames per engine call, like the other bands' loops


def split(src, args, ext):
    """split() of the reference (:24-75): colour half -> args.output, depth half -> args.output_depth; returns the depth file's name"""
    h, w = src[0].shape[:2]
    ctx = None
    if args.encoding_depth == "hue":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if root not in sys.path:
            sys.path.insert(0, root)
        from prisma_amd import engine
        ctx = engine.Ops()                      # no model: any context decodes (raises without a HIP device; there is no CPU path)
        rb, db = engine.rgbd_boxes(h, w, args.rgbd)
    else:
        k = (w if args.rgbd in ("left", "right") else h) // 2                   # int(width / 2), int(height / 2) of :29-40 as slice bounds
        if k < 1:
            raise SystemExit("rgba: a %d x %d frame has no %s half" % (h, w, args.rgbd))
        first, second = ((0, h, 0, k), (0, h, k, w)) if args.rgbd in ("left", "right") else ((0, k, 0, w), (k, h, 0, w))
        rb, db = (second, first) if args.rgbd in ("left", "top") else (first, second)
    folder = os.path.dirname(args.output)
    depth_file = os.path.join(folder, args.output_depth + "." + ext)
    check_overwrite(depth_file)
    subs = []
    for sub in (args.subpath, args.subpath_depth):
        subs.append(os.path.join(folder, sub) if sub else None)
        if sub:
            create_folder(subs[-1])
    fps = int(args.fps)                                                            # :113
    half = (w / 2, h) if args.rgbd in ("left", "right") else (w, h / 2)             # :30-40: the sizes both writers get
    outs = [VideoWriter(width=half[0], height=half[1], frame_rate=fps, filename=f) for f in (args.output, depth_file)]

    def emit(s, rgb, dep):
        # sink thread, chunk after chunk in order: both videos and the frame dumps (:65-72)
        for j in range(len(rgb)):
            for out, sub, frame in zip(outs, subs, (rgb[j], dep[j])):
                if sub:
                    write_rgb(os.path.join(sub, str(s + j).zfill(6) + ".png"), (255 - frame).astype(np.uint8))
                out.write(frame)

    sink = AsyncSink(depth=2)
    try:
        for s, frames in chunks(src, 0, len(src), CHUNK):
            dep = ctx.rgbd_depth(frames, args.rgbd) if ctx else frames[:, db[0]:db[1], db[2]:db[3]]
            sink.submit(emit, s, frames[:, rb[0]:rb[1], rb[2]:rb[3]], dep)
        sink.close()
    finally:
        if ctx:
            ctx.close()
    for out in outs:
        out.close()
    return depth_file


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--input", "-i", type=str, required=True)
    p.add_argument("--tmp", "-t", type=str, default="tmp")
    p.add_argument("--fps", "-r", type=float, default=24)
    p.add_argument("--output", "-o", type=str, default="")
    p.add_argument("--subpath", type=str, default=None)
    p.add_argument("--rgbd", choices=["none", "left", "right", "top", "bottom"], default="none")
    p.add_argument("--encoding_depth", choices=["none", "hue"], default="none")
    p.add_argument("--output_depth", type=str, default="depth")
    p.add_argument("--subpath_depth", type=str, default=None)
    args = p.parse_args(argv)
    ext = args.input.rsplit(".", 1)[1]
    if not is_video(args.input):
        ext = "png"
    if args.output == "" or os.path.isdir(args.output):
        folder = args.output if args.output else os.path.dirname(args.input)
        args.output = os.path.join(folder, BAND + "." + ext)
    check_overwrite(args.output)
    depth_file = None
    if is_video(args.input) and args.rgbd != "none":
        depth_file = split(FrameReader(args.input), args, ext)
    elif is_video(args.input):
        src = FrameReader(args.input)
        sub = None
        if args.subpath:
            sub = os.path.join(os.path.dirname(args.output), args.subpath)
            create_folder(sub)
        if src.i420:            # a .y4m carries no audio to drop and its frames are what the bands read: the file is copied, rate and all
            shutil.copyfile(args.input, args.output)
            for i in range(len(src) if sub else 0):
                write_rgb(os.path.join(sub, str(i).zfill(6) + ".png"), (255 - src[i]).astype(np.uint8))
        else:
            h, w = src[0].shape[:2]
            out = VideoWriter(width=w, height=h, frame_rate=args.fps, filename=args.output)
            for i in range(len(src)):
                f = src[i]
                if sub:
                    write_rgb(os.path.join(sub, str(i).zfill(6) + ".png"), (255 - f).astype(np.uint8))     # rgba.py:96
                out.write(f)
            out.close()
    else:
        if args.rgbd != "none":
            print("rgba: --rgbd %s is ignored for a still image, as in the reference (process_image): the whole image is the rgba band" % args.rgbd,
                  file=sys.stderr)
        write_rgb(args.output, open_rgb(args.input))
    data = load_metadata(os.path.dirname(args.output))
    loaded = copy.deepcopy(data)
    if data is not None:
        get_target(args.output, data, band=BAND, target=args.output)
        if depth_file:
            add_band(data, "depth", url=os.path.basename(depth_file))
        merge_metadata(os.path.dirname(args.output), data, loaded)


if __name__ == "__main__":
    main()
