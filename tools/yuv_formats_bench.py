#!/usr/bin/env python3
"""What the other .y4m layouts cost, measured in one visit on 32 frames of 1920 x 1080 (EXPERIMENTS.md 6.26):

 (a) every layout's conversion kernel alone (prisma_amd/csrc/yuv_formats.hip, device-resident frames, the 16-byte path): ms per launch of all
     32 frames between two stream synchronisations and GB/s of the bytes it must move (the planes once, 3 bytes of RGB per pixel once;
     launches run back to back on a 300 - 600 MB working set, so these are effective rates with cache hits in them, not HBM rates), next
     to i420_to_rgb_kernel (yuv.hip) in the same process - 8-bit 4:2:0 with another matrix runs the new kernel on the same bytes, so that
     pair is the cost of coefficients in registers instead of literals;
 (b) the depth band loop on a 10-bit clip (C420p10: 3 bytes per pixel through PCIe and the rings) against the same picture as the usual
     8-bit C420jpeg clip (1.5), blocking and streamed: wall time of the loop (run_sharded inside process_video: not the model load), runs
     interleaved, the first of each arm untimed.  Files live in a tmpfs folder.

  python tools/yuv_formats_bench.py > profiles/yuv_formats_bench.txt

No threshold is set: the parent commit refuses every one of these clips."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(ops, call, iters):
    for _ in range(3):
        call()
    ops.sync()
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        ops.sync()
        runs.append((time.perf_counter() - t0) / iters * 1e3)
    return sorted(runs)[len(runs) // 2], runs


def kernels(np, engine, n, H, W, iters):
    ops = engine.Ops()
    rgb_b = n * H * W * 3
    formats = [engine.YuvFormat(c, d, False, "bt709") for d in (8, 10) for c in (400, 420, 422, 444)] + [engine.YuvFormat(444, 16, True, "bt601")]
    biggest = max(engine.yuv_bytes(f, H, W) for f in formats) * n
    d_rgb, d_yuv = ops.dev_alloc(rgb_b), ops.dev_alloc(biggest)
    out = []
    try:
        ops.h2d(d_yuv, np.random.default_rng(0).integers(0, 256, biggest, dtype=np.uint8))
        calls = [("i420_to_rgb (yuv.hip)", n * engine.i420_bytes(H, W), lambda: ops.i420_to_rgb_dev(d_yuv, n, H, W, d_rgb))]
        calls += [("%d %2d bit %s %s" % (f.chroma, f.depth, "full" if f.full_range else "limited", f.matrix), n * engine.yuv_bytes(f, H, W),
                   lambda f=f: ops.yuv_to_rgb_dev(f, d_yuv, n, H, W, d_rgb)) for f in formats]
        for name, yuv_b, call in calls:
            ms, runs = timed(ops, call, iters)
            out.append({"kernel": name, "ms_per_launch": ms, "runs_ms": runs, "bytes": yuv_b + rgb_b, "GBps": (yuv_b + rgb_b) / (ms * 1e-3) / 1e9})
    finally:
        ops.dev_free(d_rgb)
        ops.dev_free(d_yuv)
        ops.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per arm, interleaved; one untimed run of each arm goes first")
    ap.add_argument("--encoder", default="vitl")
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window of (a)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["PRISMA_SYNTH"] = "1"
    os.environ["PRISMA_OVERWRITE"] = "1"
    os.environ.pop("PRISMA_BATCH", None)
    os.environ.pop("PRISMA_Y4M_MATRIX", None)
    for p in (os.path.join(HERE, "bands"), HERE):
        sys.path.insert(0, p)
    import numpy as np
    from prisma_amd import engine, synth
    import depth_anything as mod
    from common import loop as loopmod
    from common import yuv

    n, H, W = a.frames, a.height, a.width
    report = {"frames": n, "frame": [H, W], "kernels": kernels(np, engine, n, H, W, a.iters), "depth_loop": {}}
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > (4 << 30) else None
    work = tempfile.mkdtemp(prefix="yuv_formats_bench.", dir=base)
    try:
        # one picture, two clips: its 8-bit 4:2:0 planes, and the same samples shifted up to 10 bit
        clips = {"C420jpeg": os.path.join(work, "in8.y4m"), "C420p10": os.path.join(work, "in10.y4m")}
        files = {k: open(p, "wb") for k, p in clips.items()}
        for k, f in files.items():
            f.write(("YUV4MPEG2 W%d H%d F24:1 Ip A1:1 %s XCOLORRANGE=LIMITED\n" % (W, H, k)).encode())
        for fr in synth.frames(n, H, W, seed=7):
            planes = yuv.rgb_to_i420(fr)
            files["C420jpeg"].write(b"FRAME\n" + planes.tobytes())
            files["C420p10"].write(b"FRAME\n" + (planes.astype("<u2") << 2).tobytes())
        for f in files.values():
            f.close()
        ns = dict(subpath="", npy=False, ply=False, metric="none", encoder=a.encoder, weights="", synthetic=True)
        times = []
        orig = mod.run_sharded

        def wrapped(*args, **kw):
            t0 = time.perf_counter()
            r = orig(*args, **kw)
            times.append(time.perf_counter() - t0)
            return r
        mod.run_sharded = wrapped
        mod.args = argparse.Namespace(**ns)
        mod.init_model(a.encoder, "", device=0)
        arms = [(tag, loop) for loop in ("blocking", "streamed") for tag in clips]
        runs = {"%s %s" % arm: [] for arm in arms}
        rings = {}
        try:
            for rnd in range(a.rounds + 1):                 # round 0 is the untimed one
                for tag, loop in arms:
                    os.environ["PRISMA_STREAM"] = "1" if loop == "streamed" else "0"
                    del times[:]
                    mod.process_video(argparse.Namespace(input=clips[tag], output=os.path.join(work, "depth_%s.y4m" % tag), **ns))
                    assert len(times) == 1
                    if rnd:
                        runs["%s %s" % (tag, loop)].append(times[0])
                    elif loop == "streamed":
                        rings[tag] = dict(loopmod.last_stream).get("ring_bytes", 0)
                    print("[depth_anything] %-9s %-9s round %d: %.3f s" % (tag, loop, rnd, times[0]), file=sys.stderr, flush=True)
        finally:
            mod.run_sharded = orig
            mod.model.close()
            mod.model = None
        med = {k: float(np.median(v)) for k, v in runs.items()}
        report["depth_loop"] = {"encoder": a.encoder, "loop_s": runs, "median_s": med, "ring_bytes": rings,
                                "p10_over_8bit": {loop: med["C420p10 " + loop] / med["C420jpeg " + loop] for loop in ("blocking", "streamed")}}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    print("%d frames of %d x %d" % (n, W, H))
    print("(a) kernels alone, device-resident frames, 16-byte path")
    for v in report["kernels"]:
        print("    %-28s %7.3f ms  %7.1f MB  %7.1f GB/s   (runs: %s)" % (v["kernel"], v["ms_per_launch"], v["bytes"] / 1e6, v["GBps"], " / ".join("%.3f" % r for r in v["runs_ms"])))
    d = report["depth_loop"]
    print("(b) depth_anything %s loop: seconds per clip (runs), median" % d["encoder"])
    for key, v in d["loop_s"].items():
        print("    %-20s %-26s %7.3f" % (key, " / ".join("%.3f" % x for x in v), d["median_s"][key]))
    print("    C420p10 / C420jpeg: blocking %.3f, streamed %.3f; streamed rings %s MB" % (
        d["p10_over_8bit"]["blocking"], d["p10_over_8bit"]["streamed"], " / ".join("%s %.1f" % (k, v / 1e6) for k, v in d["ring_bytes"].items())))


if __name__ == "__main__":
    main()
