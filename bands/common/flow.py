"""The flow bands' video loop (flow_raft, flow_gmflow: the two reference scripts share theirs line for line, flow_raft.py:69-166 and
flow_gmflow.py:121-218): videos, .flo / 16-bit PNG dumps, the max-displacement CSV and the metadata entries, on common/loop.py."""
import os

import numpy as np

from prisma_amd import engine

from .io import FrameReader, VideoWriter, is_planar, planar_out, write_flo, write_flow_png
from .loop import Stream, frame_formats, run_sharded, stream_enabled
from .yuv import yuv_bytes


def _mask_rgb(mask):
    """reference bands/common/flow.py:75-78: True -> 255, three equal channels."""
    return np.repeat((mask.astype(np.uint8) * 255)[..., None], 3, axis=-1)


def process_video(args, band, model, data, rk, chunk, subpath_needs_both, iterations, stream_min_chunks=0):
    """Pairs (i, i+1) shard by rank in contiguous blocks with a one-frame halo.  Every chunk is written as soon
    as it is done: rank 0 feeds its own chunks to the VideoWriters from a sink thread (the next chunk is already on the
    GPU) and then muxes the other ranks' chunks in frame order through shard.Relay; only the per-pair max displacements
    (4 bytes each) go through a collective.  No list or tensor ever holds the whole video."""
    src = FrameReader(args.input)
    n = len(src)
    h, w = src[0].shape[:2]
    base, ext = args.output.rsplit(".", 1)
    want_mask = bool(args.output_mask or args.subpath_mask)
    # flow_gmflow predicts the backward flow only for --backwards / masks (reference flow_gmflow.py:86); with --subpath alone (what
    # process.py passes) a second global matching would be computed and thrown away
    both = args.backwards or want_mask or (subpath_needs_both and bool(args.subpath))
    want_flow = bool(args.subpath or args.subpath_mask)
    sh, sw = engine.flow_out_size(h, w, args.scale)
    first, last = rk.frames(n - 1)                       # pair indices owned by this rank
    dirs = ("f", "b") if args.backwards else ("f",)
    # the videos, in the order a pair's frames go out; the key names the array of a chunk (rgb / mask) and its direction
    files = {"rgb_" + d: (args.output if d == "f" else base + "_bwd." + ext) for d in dirs}
    if args.output_mask:
        mbase, mext = args.output_mask.rsplit(".", 1)
        files.update({"mask_" + d: (args.output_mask if d == "f" else mbase + "_bwd." + mext) for d in dirs})
    # rescale: a .y4m has the clip's w x h like the reference's videos (its VideoWriter rescales every frame, io.py:297), not the band's sw x sh;
    # a .npy stack has no declared size and keeps the band's, an .mp4 is rescaled by PyAV as ever
    # the layout of every .y4m written: PRISMA_Y4M_OUT's (io.y4m_out), I420 when unset
    # (an .avi / .mjpeg: the JPEG's planes, PRISMA_VIDEO_OUT's subsampling)
    ofmt = planar_out(args.output, getattr(src, "format", None))
    videos = ({k: VideoWriter(width=w, height=h, frame_rate=src.rate, filename=f, rescale=True, fmt=ofmt, device=rk.device) for k, f in files.items()}
              if rk.main else {})
    # a .y4m on either side: its planes go to / come from the engine as they are - at --scale != 1 resized to the clip's size on the GPU, next
    # to the conversion (engine rgb_full).  The mask videos and the trailing zero frame are small and rare: they are converted, and
    # resized, on the host (VideoWriter.write)
    yin, yout = src.i420, is_planar(args.output)
    fmt = frame_formats(model, yin, yout, h, w, getattr(src, "format", None), ofmt)
    model.rgb_full = yout and (sh, sw) != (h, w)
    rh, rw = (h, w) if model.rgb_full else (sh, sw)      # the size of the engine's rgb frames
    frame = ((src.frame_bytes,), np.uint8) if yin else (src[0].shape, np.uint8)       # a .y4m's planes, in the clip's own layout

    def step(_s, frames):
        mask = None
        if want_mask:
            flow, rgb, mx, mask = model.infer_sequence_masks(frames, scale=args.scale, iters=iterations, want_flow=want_flow, want_rgb=True, **fmt)
        else:
            flow, rgb, mx = model.infer_sequence(frames, scale=args.scale, iters=iterations, backward=both, want_flow=want_flow, want_rgb=True, **fmt)
        return by_file(rgb, mask), (flow, mask), mx[:, :1]

    def by_file(rgb, mask):          # a chunk's video arrays: the key's array (rgb / mask) and direction
        return {k: (rgb if k.startswith("rgb") else mask)[:, "fb".index(k[-1])] for k in files}

    # the streamed loop (common/loop.py): the same calls as submit_sequence(_masks) / wait on the loop's page-locked rings - one array per result
    # asked for, [directions, ...] per pair
    nd = 2 if both else 1
    results = {"rgb": ((nd, yuv_bytes(ofmt, rh, rw)) if yout else (nd, sh, sw, 3), np.uint8), "mx": ((nd,), np.float32)}
    if want_flow:
        results["flow"] = ((nd, sh, sw, 2), np.float32)
    if want_mask:
        results["mask"] = ((2, sh, sw), np.uint8)

    def submit(_s, frames, res):
        if want_mask:
            model.submit_sequence_masks(frames, scale=args.scale, iters=iterations, out_flow=res.get("flow"), out_rgb=res["rgb"], out_max=res["mx"],
                                        out_mask=res["mask"], **fmt)
        else:
            model.submit_sequence(frames, scale=args.scale, iters=iterations, backward=both, out_flow=res.get("flow"), out_rgb=res["rgb"], out_max=res["mx"],
                                  **fmt)

    def collect(_s, res):
        mask = res["mask"].view(np.bool_) if want_mask else None
        return by_file(res["rgb"], mask), (res.get("flow"), mask), res["mx"][:, :1]

    def write_chunk(_s, c):          # rank 0 only: one chunk of encoded pairs into every open video, in order
        for j in range(len(c["rgb_f"])):
            for k, v in videos.items():
                if k.startswith("rgb") and yout:
                    v.write_planes(c[k][j], rh, rw)
                else:
                    v.write(c[k][j] if k.startswith("rgb") else _mask_rgb(c[k][j]))

    def dump(s, payload):
        flow, mask = payload
        for j in range(len(flow)):
            if args.subpath:    # the reference crashes here (common/flow.py:91 shadows io.write_flow); write the .flo it meant to
                write_flo(os.path.join(args.subpath + "_fwd", "%04d.flo" % (s + j)), flow[j, 0])
                if args.backwards:
                    write_flo(os.path.join(args.subpath + "_bwd", "%04d.flo" % (s + j)), flow[j, 1])
            if args.subpath_mask:
                write_flow_png(os.path.join(args.subpath_mask + "_fwd", "%04d.png" % (s + j)), flow[j, 0], mask[j, 0])
                if args.backwards:
                    write_flow_png(os.path.join(args.subpath_mask + "_bwd", "%04d.png" % (s + j)), flow[j, 1], mask[j, 1])

    stream = Stream(model, frame, results, submit, collect, i420=yin) if stream_enabled(stream_min_chunks, -(-(last - first) // chunk)) else None
    # what the other ranks' pairs park in the relay's spool: per video an encoded frame (planes of the clip's size, or RGB) or a mask's bytes
    pair_bytes = sum((yuv_bytes(ofmt, rh, rw) if yout else sh * sw * 3) if k.startswith("rgb") else sh * sw for k in files)
    mx_all = run_sharded(rk, src, n - 1, chunk, 1, args.output, ((n - 1) - (last - first)) * pair_bytes,
                         step, write_chunk, dump if want_flow else None, n_scalars=1, ctx=model, stream=stream, i420=yin)
    if not rk.main:
        return
    # last frame: zero flow -> 0/0 -> NaN -> uint8 0, max displacement 0.0, all-False masks (reference :116-131)
    for v in videos.values():
        v.write(np.zeros((sh, sw, 3), np.uint8))
    # the reference appends np.float32 scalars and formats them with "{}" (:138-141): '12.148', not the float64 repr
    max_disps = [np.float32(v) for v in mx_all.reshape(-1)] + [np.float32(0.0)]
    if want_flow:
        dump(n - 1, (np.zeros((1, 2, sh, sw, 2), np.float32), np.zeros((1, 2, sh, sw), bool)))
    for v in videos.values():
        v.close()
    with open(base + ".csv", "w") as f:
        f.writelines("{}\n".format(e) for e in max_disps)
    if data:
        data["bands"][band] = {"url": band + "." + ext, "values": {"dist": {"type": "float", "url": band + ".csv"}}}
        if args.subpath:
            data["bands"][band]["folder"] = args.subpath
        if args.backwards:
            data["bands"][band + "_bwd"] = {"url": band + "_bwd." + ext}
            if args.subpath:
                data["bands"][band + "_bwd"]["folder"] = args.subpath + "_bwd"
        if args.output_mask:
            data["bands"][band + "_mask"] = {"url": band + "_mask." + ext}
            if args.backwards:
                data["bands"][band + "_mask_bwd"] = {"url": band + "_mask_bwd." + ext}
