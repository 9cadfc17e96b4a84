"""What the sharded band scripts' main() do around their argparse block and their model: the PRISMA folder / metadata preamble, the ranks, the
last metadata write - and the one answer to a missing checkpoint."""
import copy
import os
import sys

from prisma_amd import shard

from .io import check_overwrite
from .meta import band_video_ext, get_target, get_url, is_video, load_metadata, merge_metadata, video_out


def begin(args, band, flow=False):
    """args.input is a PRISMA folder (metadata.json: input = its rgba band, output = <band>.<ext> in it) or a file (output next to it unless given).
    depth and mask write a PNG for a still image and say that they found the metadata; the flow bands (flow=True) take videos only, resolve --mask
    to args.output_mask and make their --subpath / --subpath_mask dump folders absolute.  Returns (data, loaded, meta_path, ranks): the metadata, a
    deep copy of it as loaded (merge_metadata's base), where it lives, and shard.Ranks() after rank 0's check_overwrite."""
    try:
        video_out()         # a PRISMA_VIDEO_OUT nobody can write is refused here, before a model loads
    except RuntimeError as e:
        raise SystemExit(f"[{band}] {e}")
    meta_path = args.input
    data = load_metadata(meta_path)
    loaded = copy.deepcopy(data)
    if data:
        if not flow:
            print("PRISMA metadata found and loaded")
        args.input = get_url(meta_path, data, "rgba")
        args.output = get_target(args.input, data, band=band, target=args.output, force_extension=None if flow else "png")
        if flow and args.mask:
            args.output_mask = get_target(args.input, data, band=band + "_mask")
    elif not args.output:
        ext = band_video_ext(args.input)       # the clip's own, or PRISMA_VIDEO_OUT's
        args.output = os.path.join(os.path.dirname(args.input), band + "." + (ext if flow or is_video(args.input) else "png"))
    if flow and not is_video(args.output):
        raise SystemExit(f"[{band}] needs a video input")
    ranks = shard.Ranks()
    if ranks.main:
        check_overwrite(args.output)
    if flow:
        input_folder = os.path.dirname(args.input)
        for attr in ("subpath", "subpath_mask"):
            if getattr(args, attr):
                setattr(args, attr, os.path.join(input_folder, getattr(args, attr)))
                os.makedirs(getattr(args, attr) + "_fwd", exist_ok=True)
                if args.backwards:
                    os.makedirs(getattr(args, attr) + "_bwd", exist_ok=True)
    return data, loaded, meta_path, ranks


def end(ranks, meta_path, data, loaded):
    if ranks.main:
        merge_metadata(meta_path, data, loaded)
    ranks.close()


def synthetic_or_exit(band, missing, flag, synthetic, what=" for seeded synthetic weights"):
    """A checkpoint is missing (`missing` says which): an error that names the flag to pass, unless seeded synthetic weights were asked for
    (--synthetic / PRISMA_SYNTH=1: tests, benchmarks) - then a note on stderr, and the caller makes them."""
    if not shard.synthetic_allowed(synthetic):
        raise SystemExit(f"[{band}] {missing}; pass {flag}, or --synthetic / PRISMA_SYNTH=1{what}")
    print(f"[{band}] {missing}; using seeded synthetic weights (--synthetic)", file=sys.stderr)
