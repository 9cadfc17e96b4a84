#!/usr/bin/env python3
"""What .y4m flow videos of the clip's size cost, measured in one visit (EXPERIMENTS.md 6.22).  The flow bands encode sh x sw frames (--scale
0.75 of a 1920 x 1080 clip: 810 x 1440) and the video has the clip's size, so every frame is resized on the way out.

 (a) the resize kernels alone (prisma_amd/csrc/resize.hip, 32 device-resident frames, 810 x 1440 -> 1080 x 1920): ms per launch between two
     stream synchronisations, and GB/s of the bytes each must move (the source once, the output once) - RGB out, I420 out (fused: the resized
     RGB frame is never written), and next to the fused kernel the two launches it replaces on the GPU (resize to RGB, then rgb_to_i420).
     One fused frame is checked against the host arithmetic at the timed size before anything is timed;
 (b) the host side (bands/common/resize.py + bands/common/yuv.py, numpy on one core): frames per second - what the band loop's sink thread
     would deliver if the resize stayed on the host, as it does for the mask videos and the trailing frame;
 (c) the flow_gmflow band loop on a .y4m clip at --scale 0.75, blocking loop: wall time of run_sharded inside process_video (not the model
     load), this tree against --parent (a checkout of the parent commit, built: it writes the 810 x 1440 video), each tree in processes of
     its own that alternate, one untimed run first in each.  The difference is the price of the larger device-to-host copy and file.

  python tools/resize_bench.py --parent <checkout of the parent commit> --out profiles/resize_bench.json > profiles/resize_bench.txt

No threshold is set: nobody had measured any of the three."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(call, sync, iters):
    for _ in range(3):
        call()
    sync()
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        sync()
        runs.append((time.perf_counter() - t0) / iters * 1e3)
    return sorted(runs)[len(runs) // 2], runs


def kernels(np, engine, resize, yuv, n, sh, sw, H, W, iters):
    ops = engine.Ops()
    src_b, rgb_b, yuv_b = n * sh * sw * 3, n * H * W * 3, n * engine.i420_bytes(H, W)
    d_src, d_rgb, d_yuv = ops.dev_alloc(src_b), ops.dev_alloc(rgb_b), ops.dev_alloc(yuv_b)
    out = {}
    try:
        src = np.random.default_rng(0).integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
        ops.h2d(d_src, src)
        ops.rgb_resize_dev(d_src, n, sh, sw, H, W, d_yuv, i420=True)
        ops.sync()
        got = np.empty(engine.i420_bytes(H, W), np.uint8)
        ops.d2h(got, d_yuv)
        assert np.array_equal(got, yuv.rgb_to_i420(resize.resize_rgb(src[0], H, W))), "the fused kernel and the host arithmetic differ"
        arms = (("rgb_resize", lambda: ops.rgb_resize_dev(d_src, n, sh, sw, H, W, d_rgb), src_b + rgb_b),
                ("rgb_resize_i420", lambda: ops.rgb_resize_dev(d_src, n, sh, sw, H, W, d_yuv, i420=True), src_b + yuv_b),
                ("resize + rgb_to_i420", lambda: (ops.rgb_resize_dev(d_src, n, sh, sw, H, W, d_rgb), ops.rgb_to_i420_dev(d_rgb, n, H, W, d_yuv)),
                 src_b + 2 * rgb_b + yuv_b),
                ("rgb_to_i420 at sh x sw", lambda: ops.rgb_to_i420_dev(d_src, n, sh, sw, d_yuv), src_b + n * engine.i420_bytes(sh, sw)))
        for name, call, nbytes in arms:
            ms, runs = timed(call, ops.sync, iters)
            out[name] = {"ms_per_launch": ms, "runs_ms": runs, "bytes": nbytes, "GBps": nbytes / (ms * 1e-3) / 1e9}
    finally:
        for p in (d_src, d_rgb, d_yuv):
            ops.dev_free(p)
        ops.close()
    return out


def host(np, resize, yuv, sh, sw, H, W, frames=4):
    rgb = np.random.default_rng(1).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    out = {}
    for name, call in (("resize_rgb", lambda: resize.resize_rgb(rgb, H, W)), ("resize_rgb + rgb_to_i420", lambda: yuv.rgb_to_i420(resize.resize_rgb(rgb, H, W)))):
        call()
        t0 = time.perf_counter()
        for _ in range(frames):
            call()
        out[name] = {"fps": frames / (time.perf_counter() - t0)}
    return out


def loop_child(a):
    """--loop-child: the band loop of the tree in --tree, one untimed run and --rounds timed ones -> one JSON line on stdout"""
    import importlib
    for p in (os.path.join(a.tree, "bands"), a.tree):
        sys.path.insert(0, p)
    os.environ.update(PRISMA_SYNTH="1", PRISMA_OVERWRITE="1", PRISMA_STREAM="0")
    os.environ.pop("PRISMA_BATCH", None)
    from common import flow as flowmod
    mod = importlib.import_module(a.band)
    times, orig = [], flowmod.run_sharded

    def clocked(*args, **kw):
        t0 = time.perf_counter()
        r = orig(*args, **kw)
        times.append(time.perf_counter() - t0)
        return r
    flowmod.run_sharded = clocked
    ns = argparse.Namespace(subpath="", synthetic=True, backwards=False, mask=False, output_mask="", subpath_mask="", scale=a.scale, model="",
                            iterations=getattr(mod, "ITERATIONS", 1), small=False, mixed_precision=False, alternate_corr=False)
    mod.init_model(ns, device=0)
    out = os.path.join(os.path.dirname(a.clip), "%s_%d.y4m" % (a.band, os.getpid()))
    try:
        for _ in range(a.rounds + 1):
            mod.process_video(argparse.Namespace(input=a.clip, output=out, **vars(ns)))
        head = open(out, "rb").readline().decode().split()
        size = os.path.getsize(out)
    finally:
        mod.model.close()
        for p in (out, out[:-4] + ".csv"):
            if os.path.exists(p):
                os.remove(p)
    assert len(times) == a.rounds + 1
    print(json.dumps({"loop_s": times[1:], "video": head[1] + " " + head[2], "video_bytes": size}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--scale", type=float, default=0.75)
    ap.add_argument("--band", default="flow_gmflow")
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: the other arm of (c); without it (c) times this tree alone")
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per process of (c); one untimed run goes first")
    ap.add_argument("--visits", type=int, default=2, help="processes per tree in (c), the trees alternating")
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window of (a)")
    ap.add_argument("--out", default="")
    ap.add_argument("--loop-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--clip", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop_child:
        return loop_child(a)
    os.environ["OMP_NUM_THREADS"] = os.environ["OPENBLAS_NUM_THREADS"] = "1"         # (b) is one core's figure
    for p in (os.path.join(HERE, "bands"), HERE):
        sys.path.insert(0, p)
    import numpy as np
    from prisma_amd import engine, synth
    from common import io as iomod
    from common import resize, yuv

    n, H, W = a.frames, a.height, a.width
    sh, sw = engine.flow_out_size(H, W, a.scale)
    report = {"frames": n, "frame": [H, W], "band_frame": [sh, sw], "kernels": kernels(np, engine, resize, yuv, n, sh, sw, H, W, a.iters),
              "host": host(np, resize, yuv, sh, sw, H, W), "loop": {}}
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > (4 << 30) else None
    work = tempfile.mkdtemp(prefix="resize_bench.", dir=base)
    try:
        clip = os.path.join(work, "clip.y4m")
        w = iomod.VideoWriter(W, H, 24, clip)
        for f in synth.frame_pair_sequence(n, H, W, seed=7):
            w.write(f)
        w.close()
        trees = [("this tree", HERE)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
        runs = {name: {"loop_s": []} for name, _ in trees}
        for visit in range(a.visits):
            for name, tree in (trees if visit % 2 == 0 else trees[::-1]):
                env = dict(os.environ)
                env.pop("PRISMA_BANDS_LIB", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-child", "--tree", tree, "--clip", clip, "--band", a.band, "--scale", str(a.scale),
                                    "--rounds", str(a.rounds)], env=env, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise SystemExit("(c) %s: exit %d\n%s" % (name, r.returncode, r.stderr[-3000:]))
                got = json.loads(r.stdout.strip().splitlines()[-1])
                runs[name]["loop_s"] += got["loop_s"]
                runs[name].update(video=got["video"], video_bytes=got["video_bytes"])
                print("[%s] %-9s visit %d: %s s" % (a.band, name, visit, " / ".join("%.3f" % t for t in got["loop_s"])), file=sys.stderr, flush=True)
        for v in runs.values():
            v["median_s"], v["spread_s"] = float(np.median(v["loop_s"])), float(max(v["loop_s"]) - min(v["loop_s"]))
            v["pairs_per_s"] = (n - 1) / v["median_s"]
        report["loop"] = runs
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    print("%d frames, %d x %d -> %d x %d" % (n, sw, sh, W, H))
    print("(a) kernels alone, device-resident frames: ms per launch of %d frames, GB/s of the bytes the arm must move" % n)
    for k, v in report["kernels"].items():
        print("    %-24s %7.3f ms  %7.1f MB  %7.1f GB/s   (runs: %s)" % (k, v["ms_per_launch"], v["bytes"] / 1e6, v["GBps"], " / ".join("%.3f" % r for r in v["runs_ms"])))
    print("(b) host arithmetic, numpy, one core")
    for k, v in report["host"].items():
        print("    %-24s %7.2f frames per second" % (k, v["fps"]))
    print("(c) %s band loop on the .y4m clip, --scale %.2f, blocking: seconds per clip (%d pairs)" % (a.band, a.scale, n - 1))
    for name, v in report["loop"].items():
        print("    %-9s video %-12s %6.1f MB  runs %s  median %.3f  spread %.3f  %6.1f pairs/s" %
              (name, v["video"], v["video_bytes"] / 1e6, " / ".join("%.3f" % t for t in v["loop_s"]), v["median_s"], v["spread_s"], v["pairs_per_s"]))
    if "parent" in report["loop"]:
        print("    this tree / parent = %.3f" % (report["loop"]["this tree"]["median_s"] / report["loop"]["parent"]["median_s"]))


if __name__ == "__main__":
    main()
