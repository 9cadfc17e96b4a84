#!/usr/bin/env python3
"""process.py - prisma's L5 orchestrator over this repo's band scripts.

Re-statement of /root/reference/process.py: same flags (:76-99), same folder / metadata.json contract (:101-189: folder next to
the input, rgba band first, width / height / fps / frames / duration, principal_point, focal_length = sqrt(W H),
field_of_view), same band order (mask -> depth -> flow -> camera, :205-290), same per-band extra arguments (:47-58:
`--sdf` for mask_mmdet, `--metric outdoor` for depth_anything, `--ply` / `--npy` / `--subpath` from `--extra`), same
default-band aliases (`depth`, `flow`, `flow_bwd`, `flow_mask`, `flow_mask_bwd`, :243-287).  It shells out to
`bands/<band>.py` exactly like the reference's run() (:60-73), with `sys.executable` instead of a bare `python3`.

Side-by-side RGB-D captures (:124-166, 243): `--rgbd left|right|top|bottom` (where the depth is) is handed to the rgba band, which
writes the colour half as rgba.<ext> and the other half as band `depth`; every other band then runs on the colour half, and the
`depth` alias is NOT pointed at the estimated depth band.  `--record3d` is `--rgbd right` with `--encoding_depth hue`, plus the
capture's own camera: focal_length = max(fx, fy), principal_point = [cx, cy], field_of_view from the input's full height, and the
metric range of the `depth` band (values.min / max) from Record3D's tag - read from `<input>.record3d.json` beside the input, or
through pymediainfo where it is installed (bands/common/meta.py get_record3d_data).

Bands this repo builds: rgba, depth_anything, flow_raft, flow_gmflow (the reference's default flow band, :23 -
and this script's), mask_mmdet.  The reference's default for still images (depth_patchfusion) and camera_colmap are out of scope
(SURVEY section 2): a request for a band that is not built is reported and skipped; a default that is not built falls back to the
built band of the same kind.

Beyond the reference: `--jobs N` runs the bands of one input side by side, N at a time (they only read the rgba band; each ends with a
locked merge into metadata.json, bands/common/meta.py merge_metadata), and `--gpus G` launches every video band that shards its frames
under `torch.distributed.run` with G ranks on this node.  Both default to 1, which is the reference's shape: one band after the other,
each a plain process.  The folder a parallel run leaves is byte-identical to the serial run's.
"""
import argparse
import os
import queue
import shlex
import socket
import subprocess
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from bands.common.io import get_image_size, get_video_data, y4m_out  # noqa: E402
from bands.common.meta import (add_band, create_metadata, get_record3d_data, is_video, load_metadata,  # noqa: E402
                               set_default_band, update_metadata, video_out, write_metadata)

# Default BANDS & MODELS (reference :17-30; defaults narrowed to what is built here)
BUILT = ("rgba", "depth_anything", "flow_raft", "flow_gmflow", "mask_mmdet")
DEPTH_VIDEO_DEFAULT = "depth_anything"
DEPTH_IMAGE_DEFAULT = "depth_anything"          # reference: depth_patchfusion (not built)
DEPTH_BANDS = ["depth_midas", "depth_marigold", "depth_zoedepth", "depth_patchfusion", "depth_anything"]
DEPTH_OPTIONS = DEPTH_BANDS + ["all"]
FLOW_DEFAULT = "flow_gmflow"                    # reference :23
FLOW_BANDS = ["flow_gmflow", "flow_raft"]
FLOW_OPTIONS = FLOW_BANDS + ["all"]
MASK_DEFAULT = "mask_mmdet"

SUBFOLDERS = {"rgba": "images", "mask_mmdet": "mask", "flow_raft": "flow_raft", "flow_gmflow": "flow_gmflow",
              "depth_zoedepth": "depth_zoedepth", "depth_midas": "depth_midas", "depth_marigold": "depth_marigold",
              "depth_patchfusion": "depth_patchfusion", "depth_anything": "depth_anything", "camera_colmap": "sparse"}
EXTRA_ARGS = {"rgba": "", "mask_mmdet": "--sdf ", "depth_midas": " ", "depth_marigold": "", "depth_zoedepth": "",
              "depth_patchfusion": "", "depth_anything": "--metric outdoor ", "flow_raft": "", "flow_gmflow": ""}

COMMANDS = []        # every command run() issued, in order (tests read it)
RESULTS = []         # (band, return code) of every BUILT band run() launched; unbuilt bands are "skipped", not failures


SHARDED = ("depth_anything", "flow_raft", "flow_gmflow", "mask_mmdet")     # bands whose video loop shards frames by rank (prisma_amd/shard.py)
MAX_GPU_PROCESSES = 16           # a shared box allows this many processes holding a GPU at once: bands in flight x ranks per band
DEVICE_TROUBLE = (124, 134, 137, 139)     # time limit, abort, kill, segmentation fault: with --jobs > 1 no further band starts after one
_PORTS = set()                   # rendezvous ports handed out by this process: a fresh one per band


def plan_width(jobs, gpus):
    """Bands in flight at once: --jobs, cut so that bands x ranks stays within MAX_GPU_PROCESSES (--gpus 8 --jobs 3: two at a time)."""
    return min(jobs, max(1, MAX_GPU_PROCESSES // gpus))


def free_port():
    """A free TCP port for one band's rendezvous: bind port 0 and read back what the kernel gave, never the same one twice."""
    while True:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        if port not in _PORTS:
            _PORTS.add(port)
            return port


def build_command(band, input_folder, output_file="", subpath=False, extra_args="", gpus=1):
    """The argv of reference run() (:60-73): bands/<band>.py -i <input> [--output <file>] <extra> [--subpath <SUBFOLDERS[band]>].
    gpus > 1 puts a sharding band under `torch.distributed.run` with that many ranks on this node; the band's own arguments stay."""
    cmd = [sys.executable]
    if gpus > 1 and band in SHARDED:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % gpus, "--master-addr", "127.0.0.1",
                "--master-port", str(free_port())]
    cmd += [os.path.join(ROOT, "bands", band + ".py"), "-i", input_folder]
    if output_file != "":
        cmd += ["--output", output_file]
    if extra_args != "":
        cmd += shlex.split(extra_args)
    if subpath:
        cmd += ["--subpath", SUBFOLDERS[band]]
    return cmd


def run(band, input_folder, output_file="", subpath=False, extra_args="", gpus=1):
    print("\n# ", band.upper())
    if band not in BUILT:
        print(f"band '{band}' is not built in this repo (out of scope, SURVEY section 2): skipped")
        return 1
    cmd = build_command(band, input_folder, output_file, subpath, extra_args, gpus)
    COMMANDS.append(cmd)
    print(" ".join(shlex.quote(c) for c in cmd), "\n")
    rc = subprocess.run(cmd, cwd=ROOT).returncode
    RESULTS.append((band, rc))
    return rc


_PRINT = threading.Lock()


def _relay(stream, band, out):
    """One child stream, line by line, each line prefixed with its band; whole lines only, so bands never mix within one."""
    for line in iter(stream.readline, ""):
        with _PRINT:
            out.write("[%s] %s" % (band, line if line.endswith("\n") else line + "\n"))
            out.flush()
    stream.close()


def run_jobs(jobs, width):
    """Run `jobs`, dicts of {band, kwargs of run(), after: callables}, at most `width` at a time, started in list order.  A job's
    `after` steps run here, in the parent, as soon as that job ends.  A band that exits non-zero is recorded and the others go on;
    one that is killed by a signal or exits with a DEVICE_TROUBLE code stops further starts, the running ones finish."""
    done = queue.Queue()
    pending = list(jobs)
    running = {}
    stop = False

    def wait(job, proc, readers):
        for t in readers:
            t.join()
        done.put((job, proc.wait()))

    try:
        while pending or running:
            while pending and not stop and len(running) < width:
                job = pending.pop(0)
                band = job["band"]
                cmd = build_command(band, **job["kwargs"])
                COMMANDS.append(cmd)
                with _PRINT:
                    print("\n# ", band.upper())
                    print(" ".join(shlex.quote(c) for c in cmd), "\n", flush=True)
                proc = subprocess.Popen(cmd, cwd=ROOT, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                        text=True, errors="replace", bufsize=1)
                readers = [threading.Thread(target=_relay, args=(proc.stdout, band, sys.stdout), daemon=True),
                           threading.Thread(target=_relay, args=(proc.stderr, band, sys.stderr), daemon=True)]
                for t in readers:
                    t.start()
                running[id(job)] = proc
                threading.Thread(target=wait, args=(job, proc, readers), daemon=True).start()
            if not running:          # stopped with bands still pending: they are not started
                break
            job, rc = done.get()
            del running[id(job)]
            job["rc"] = rc
            if rc < 0 or rc in DEVICE_TROUBLE:
                stop = True
                with _PRINT:
                    print("process.py: %s ended with %d: no further band is started" % (job["band"], rc), file=sys.stderr, flush=True)
            for step in job["after"]:
                step()
    except KeyboardInterrupt:
        for proc in running.values():
            proc.terminate()
        for proc in running.values():
            proc.wait()
        raise
    finally:
        RESULTS.extend((j["band"], j["rc"]) for j in jobs if "rc" in j)
    if pending:
        with _PRINT:
            print("process.py: not started: %s" % ", ".join(j["band"] for j in pending), file=sys.stderr, flush=True)
    return [j["band"] for j in pending]


def order_bands(folder, first, steps):
    """Rewrite metadata.json once, under the lock, with the keys of `bands` in the order a serial run inserts them: the keys in
    `first` (what the folder held before the band jobs) where they are, then by owning step in `steps` - the band names in serial
    order with "=alias" entries where set_default_band follows.  `mask` belongs to mask_mmdet; otherwise the owner is the longest
    band name that prefixes the key, and an alias belongs to the step that sets it.  Keys nobody owns go last.  The sort is stable,
    so a band's own keys keep the order the band gave them."""
    def rank(key):
        if key in first:
            return -1
        if "=" + key in steps:
            return steps.index("=" + key)
        if key == "mask" and "mask_mmdet" in steps:
            return steps.index("mask_mmdet")
        owners = [s for s in steps if not s.startswith("=") and key.startswith(s)]
        return steps.index(max(owners, key=len)) if owners else len(steps)

    def reorder(data):
        bands = data.get("bands", {})
        data["bands"] = {k: bands[k] for k in sorted(bands, key=rank)}
    update_metadata(folder, reorder)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--input", "-i", help="input file", type=str, required=True)
    parser.add_argument("--output", help="folder name", type=str, default="")
    parser.add_argument("--record3d", help="Record3D video", action="store_true")
    parser.add_argument("--fps", "-r", help="fix framerate", type=float, default=24)
    parser.add_argument("--extra", "-e", help="Save extra data [>0 frames|PLYs; >1 FLOs; >2 NPY]", type=int, default=0)
    parser.add_argument("--rgbd", help="Where the depth is", type=str, default=None)
    parser.add_argument("--depth", "-d", help="Depth bands", type=str, default=None, choices=DEPTH_OPTIONS)
    parser.add_argument("--ply", "-p", help="Save ply for images", action="store_true")
    parser.add_argument("--npy", "-n", help="Save npy version of files", action="store_true")
    parser.add_argument("--flow", "-f", help="Flow bands", type=str, default=None, choices=FLOW_OPTIONS)
    parser.add_argument("--flo", help="Save flo files for raft", action="store_true")
    parser.add_argument("--flow_backwards", "-b", help="Save backwards video", action="store_true")
    parser.add_argument("--flow_mask", "-m", help="Save mask of videos", action="store_true")
    parser.add_argument("--jobs", "-j", help="Bands of one input run side by side, this many at a time", type=int, default=1)
    parser.add_argument("--gpus", "-g", help="GPUs of this node every video band shards its frames across (default $PRISMA_GPUS, else 1)",
                        type=int, default=int(os.environ.get("PRISMA_GPUS") or 1))
    parser.add_argument("--y4m_out", help="Layout of the .y4m videos the bands write: a C tag, then ,full and / or ,bt709 (C444p12,full is lossless, "
                        "Cmono,full for grey bands), or `source`; default 8-bit 4:2:0 limited BT.601 (sets PRISMA_Y4M_OUT for the bands)",
                        type=str, default=None, metavar="FORMAT")
    parser.add_argument("--video_out", help="Container of the video bands derived from a clip: avi or mjpeg (Motion JPEG, encoded on the GPU), then "
                        "optionally ,q=NN (quality, default 90) and one of ,444 ,420 ,mono (default 444); default the clip's own container "
                        "(sets PRISMA_VIDEO_OUT for the bands; rgba keeps the clip's)", type=str, default=None, metavar="FORMAT")
    args = parser.parse_args(argv)
    if args.jobs < 1 or args.gpus < 1:
        parser.error("--jobs and --gpus must be at least 1")
    before = os.environ.get("PRISMA_VIDEO_OUT")
    if args.video_out is not None:
        os.environ["PRISMA_VIDEO_OUT"] = args.video_out      # the band subprocesses inherit it
    try:
        video_out()         # from the option or the environment: refused here, before any band starts
    except RuntimeError as e:
        if args.video_out is not None:
            os.environ.pop("PRISMA_VIDEO_OUT")
            if before is not None:
                os.environ["PRISMA_VIDEO_OUT"] = before
        parser.error("--video_out: %s" % e)
    if args.y4m_out is not None:
        before = os.environ.get("PRISMA_Y4M_OUT")
        os.environ["PRISMA_Y4M_OUT"] = args.y4m_out        # the band subprocesses inherit it; the rgba band still copies a .y4m input as it is
        try:
            y4m_out()
        except RuntimeError as e:
            os.environ.pop("PRISMA_Y4M_OUT")
            if before is not None:
                os.environ["PRISMA_Y4M_OUT"] = before
            parser.error("--y4m_out: %s" % e)
    del COMMANDS[:]
    del RESULTS[:]

    # 1. input parameters, 2. folder + metadata (reference :101-117)
    input_path = args.input
    input_folder = os.path.dirname(input_path)
    input_basename = os.path.basename(input_path).rsplit(".", 1)[0]
    folder_name = args.output if args.output else os.path.join(input_folder, input_basename)
    data = create_metadata(folder_name)
    video = is_video(input_path)
    extension = input_path.rsplit(".", 1)[1] if video else "png"        # "mp4" in the reference; .npy frame stacks offline
    name_rgba = "rgba." + extension
    path_rgba = os.path.join(folder_name, name_rgba)

    # Record3D capture (reference :124-160): depth on the right, hue-coded; intrinsics and the depth range from the video's own tag
    extra_rgba_args = EXTRA_ARGS["rgba"]
    if args.record3d:
        args.rgbd = "right"
        height = get_video_data(input_path)[1] if video else get_image_size(input_path)[1]       # the INPUT's full height (:128-131)
        try:
            record3d_info = get_record3d_data(input_path)
        except RuntimeError as e:
            raise SystemExit("process.py: --record3d: %s" % e)
        print(record3d_info)
        camera = record3d_info["intrinsicMatrix"]
        fx, fy, cx, cy = camera[0], camera[4], camera[6], camera[7]
        depth_range = record3d_info["rangeOfEncodedDepth"]
        data["focal_length"] = max(fx, fy)
        data["principal_point"] = [cx, cy]
        data["field_of_view"] = float(2 * np.arctan(0.5 * height / data["focal_length"]) * 180 / np.pi)
        extra_rgba_args += "--encoding_depth hue "
        add_band(data, "depth", url="depth." + extension)
        data["bands"]["depth"]["values"] = {"min": {"type": "float", "value": depth_range[0]},
                                            "max": {"type": "float", "value": depth_range[1]}}

    # 3. extract RGBA (reference :160-171)
    add_band(data, "rgba", url=name_rgba)
    if args.rgbd:
        extra_rgba_args += "--rgbd " + args.rgbd
    if video:
        extra_rgba_args += " --fps " + str(args.fps)
    write_metadata(folder_name, data)
    run("rgba", input_path, path_rgba, subpath=True, extra_args=extra_rgba_args)
    data = load_metadata(folder_name)

    # 4. metadata: sizes and reconstructed intrinsics (reference :174-191)
    if video:
        data["width"], data["height"], data["fps"], data["frames"] = get_video_data(path_rgba)
        data["duration"] = float(data["frames"]) / float(data["fps"])
    else:
        data["width"], data["height"] = get_image_size(path_rgba)
    if "principal_point" not in data:
        data["principal_point"] = [float(data["width"] / 2), float(data["height"] / 2)]
    if "focal_length" not in data:
        data["focal_length"] = float(data["height"] * data["width"]) ** 0.5
    if "field_of_view" not in data:
        data["field_of_view"] = float(2 * np.arctan(0.5 * data["height"] / data["focal_length"]) * 180 / np.pi)
    write_metadata(folder_name, data)

    # 5. bands (reference :196-290)
    if args.extra > 0:
        args.ply = True
    if args.extra > 1:
        args.flo = True
    if args.extra > 2:
        args.npy = True

    # the plan, in serial order: ("band", name, arguments of run()) and ("alias", name, band it points at, band whose end it follows)
    gpus = args.gpus if video else 1             # a still image never shards
    plan = [("band", "mask_mmdet", dict(subpath=True, extra_args=EXTRA_ARGS["mask_mmdet"]))]

    depth_args = ""
    if args.ply:
        depth_args = "--ply "
    if args.npy:
        depth_args += "--npy "
    if args.depth is None:
        args.depth = DEPTH_VIDEO_DEFAULT if video else DEPTH_IMAGE_DEFAULT
    for band in (DEPTH_BANDS if args.depth == "all" else [args.depth]):
        extra_args = depth_args + EXTRA_ARGS.get(band, "")
        if band == "depth_patchfusion" and video:
            extra_args += "--mode=p49 "
        plan.append(("band", band, dict(subpath=args.extra, extra_args=extra_args)))
    if args.rgbd is None:           # reference :243: a measured depth half keeps the `depth` name; the estimated band stays under its own
        ddef = (DEPTH_VIDEO_DEFAULT if video else DEPTH_IMAGE_DEFAULT) if args.depth == "all" else args.depth
        plan.append(("alias", "depth", ddef, ddef))

    if video:
        if args.flow is None:
            args.flow = FLOW_DEFAULT
        flow_args = ""
        if args.flow_backwards:
            flow_args += "--backwards "
        if args.flow_mask:
            flow_args += "--mask "
        for band in (FLOW_BANDS if args.flow == "all" else [args.flow]):
            plan.append(("band", band, dict(subpath=args.flo, extra_args=flow_args + EXTRA_ARGS.get(band, ""))))
        fdef = FLOW_DEFAULT if args.flow == "all" else args.flow
        plan += [("alias", "flow" + suffix, fdef + suffix, fdef) for suffix in ("", "_bwd", "_mask", "_mask_bwd")]

    if args.jobs == 1:              # one band after the other, each alias where the reference sets it
        for step in plan:
            if step[0] == "band":
                run(step[1], folder_name, gpus=gpus, **step[2])
            else:
                set_default_band(folder_name, step[1], step[2])
    else:                           # side by side: an alias is set as soon as the band it points at has finished
        first = list(load_metadata(folder_name)["bands"])
        jobs, late = {}, []
        for step in plan:
            if step[0] == "band" and step[1] in BUILT:
                jobs[step[1]] = {"band": step[1], "kwargs": dict(step[2], input_folder=folder_name, gpus=gpus), "after": []}
            elif step[0] == "band":
                run(step[1], folder_name)       # reports the unbuilt band and skips it
            else:
                (jobs[step[3]]["after"] if step[3] in jobs else late).append(
                    lambda name=step[1], target=step[2]: set_default_band(folder_name, name, target))
        run_jobs(list(jobs.values()), plan_width(args.jobs, gpus))
        for step in late:
            step()
        order_bands(folder_name, first, [s[1] if s[0] == "band" else "=" + s[1] for s in plan])
    if video:
        run("camera_colmap", folder_name, subpath=True)
    # a band that failed (missing checkpoint, bad input ...) leaves a PRISMA folder without its entries: say so and fail the run
    # (the reference's os.system() ignores band failures; a drop-in that now refuses to run without weights must not exit 0 on them)
    failed = [(b, rc) for b, rc in RESULTS if rc != 0]
    if failed:
        print("\nprocess.py: %d band(s) FAILED: %s - %s is incomplete" % (len(failed), ", ".join("%s (exit %d)" % f for f in failed), folder_name),
              file=sys.stderr)
        raise SystemExit(1)
    return folder_name


if __name__ == "__main__":
    main()
