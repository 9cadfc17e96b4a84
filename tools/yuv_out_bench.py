#!/usr/bin/env python3
"""What writing the other .y4m layouts costs, measured in one visit on 32 frames of 1920 x 1080 (EXPERIMENTS.md 6.27; the twin of
tools/yuv_formats_bench.py, which measures the way in):

 (a) every layout's conversion kernel alone (prisma_amd/csrc/yuv_out.hip, device-resident frames, the 16-byte path): ms per launch of all 32
     frames between two stream synchronisations and GB/s of the bytes it must move (3 bytes of RGB per pixel once, the planes once;
     launches run back to back on a 300 - 600 MB working set, so these are effective rates with cache hits in them, not HBM rates), next
     to rgb_to_i420_kernel (yuv.hip) in the same process - 8-bit 4:2:0 with another matrix runs the new kernel on the same bytes, so that
     pair is the cost of coefficients in registers instead of literals;
 (b) the flow bands' way out at --scale 0.75 (810 x 1440 -> 1080 x 1920): the fused resize + I420 kernel (resize.hip) next to the two launches
     every other layout takes - resize to RGB, then convert - for I420 itself (the cost of not fusing) and for C444p12;
 (c) the depth band loop on a .y4m clip writing C444p12,full (6 bytes per pixel leave the GPU and cross the rings and the file) against the
     default (1.5), blocking and streamed: wall time of the loop (run_sharded inside process_video: not the model load), runs interleaved, the
     first of each arm untimed.  Files live in a tmpfs folder.

  python tools/yuv_out_bench.py > profiles/yuv_out_bench.txt

No threshold is set: the parent commit writes one layout only."""
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
    formats = [engine.YuvFormat(c, d, False, "bt709") for d in (8, 10) for c in (400, 420, 422, 444)]
    formats += [engine.YuvFormat(400, 8, True, "bt601"), engine.YuvFormat(444, 12, True, "bt601"), engine.YuvFormat(444, 16, True, "bt601")]
    biggest = max(engine.yuv_bytes(f, H, W) for f in formats) * n
    sh, sw = engine.flow_out_size(H, W, 0.75)
    f12 = engine.YuvFormat(444, 12, True, "bt601")
    d_rgb, d_yuv, d_small = ops.dev_alloc(rgb_b), ops.dev_alloc(biggest), ops.dev_alloc(n * sh * sw * 3)
    out, pair = [], []
    try:
        ops.h2d(d_rgb, np.random.default_rng(0).integers(0, 256, rgb_b, dtype=np.uint8))
        ops.h2d(d_small, np.random.default_rng(1).integers(0, 256, n * sh * sw * 3, dtype=np.uint8))
        calls = [("rgb_to_i420 (yuv.hip)", n * engine.i420_bytes(H, W), lambda: ops.rgb_to_i420_dev(d_rgb, n, H, W, d_yuv))]
        calls += [("%d %2d bit %s %s" % (f.chroma, f.depth, "full" if f.full_range else "limited", f.matrix), n * engine.yuv_bytes(f, H, W),
                   lambda f=f: ops.rgb_to_yuv_dev(f, d_rgb, n, H, W, d_yuv)) for f in formats]
        for name, yuv_b, call in calls:
            ms, runs = timed(ops, call, iters)
            out.append({"kernel": name, "ms_per_launch": ms, "runs_ms": runs, "bytes": yuv_b + rgb_b, "GBps": (yuv_b + rgb_b) / (ms * 1e-3) / 1e9})
        small_b = n * sh * sw * 3
        ways = [("fused resize + I420 (resize.hip)", small_b + n * engine.i420_bytes(H, W), lambda: ops.rgb_resize_dev(d_small, n, sh, sw, H, W, d_yuv, i420=True)),
                ("resize, then rgb_to_i420", small_b + 2 * rgb_b + n * engine.i420_bytes(H, W),
                 lambda: (ops.rgb_resize_dev(d_small, n, sh, sw, H, W, d_rgb), ops.rgb_to_i420_dev(d_rgb, n, H, W, d_yuv))),
                ("resize, then 444 12 bit full", small_b + 2 * rgb_b + n * engine.yuv_bytes(f12, H, W),
                 lambda: (ops.rgb_resize_dev(d_small, n, sh, sw, H, W, d_rgb), ops.rgb_to_yuv_dev(f12, d_rgb, n, H, W, d_yuv))),
                ("resize to RGB alone", small_b + rgb_b, lambda: ops.rgb_resize_dev(d_small, n, sh, sw, H, W, d_rgb))]
        for name, moved, call in ways:
            ms, runs = timed(ops, call, iters)
            pair.append({"way": name, "ms": ms, "runs_ms": runs, "bytes": moved})
    finally:
        for p in (d_rgb, d_yuv, d_small):
            ops.dev_free(p)
        ops.close()
    return out, pair, (sh, sw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per arm, interleaved; one untimed run of each arm goes first")
    ap.add_argument("--encoder", default="vitl")
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window of (a) and (b)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["PRISMA_SYNTH"] = "1"
    os.environ["PRISMA_OVERWRITE"] = "1"
    for k in ("PRISMA_BATCH", "PRISMA_Y4M_MATRIX", "PRISMA_Y4M_OUT"):
        os.environ.pop(k, None)
    for p in (os.path.join(HERE, "bands"), HERE):
        sys.path.insert(0, p)
    import numpy as np
    from prisma_amd import engine, synth
    import depth_anything as mod
    from common import loop as loopmod
    from common import yuv

    n, H, W = a.frames, a.height, a.width
    ks, pair, small = kernels(np, engine, n, H, W, a.iters)
    report = {"frames": n, "frame": [H, W], "kernels": ks, "resize": {"from": list(small), "ways": pair}, "depth_loop": {}}
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > (4 << 30) else None
    work = tempfile.mkdtemp(prefix="yuv_out_bench.", dir=base)
    try:
        clip = os.path.join(work, "in.y4m")
        with open(clip, "wb") as f:
            f.write(("YUV4MPEG2 W%d H%d F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (W, H)).encode())
            for fr in synth.frames(n, H, W, seed=7):
                f.write(b"FRAME\n" + yuv.rgb_to_i420(fr).tobytes())
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
        outs = {"default": "", "C444p12,full": "C444p12,full"}
        arms = [(tag, loop) for loop in ("blocking", "streamed") for tag in outs]
        runs = {"%s %s" % arm: [] for arm in arms}
        rings, sizes = {}, {}
        try:
            for rnd in range(a.rounds + 1):                 # round 0 is the untimed one
                for tag, loop in arms:
                    os.environ["PRISMA_STREAM"] = "1" if loop == "streamed" else "0"
                    os.environ["PRISMA_Y4M_OUT"] = outs[tag]
                    del times[:]
                    dst = os.path.join(work, "depth_%d.y4m" % list(outs).index(tag))
                    mod.process_video(argparse.Namespace(input=clip, output=dst, **ns))
                    assert len(times) == 1
                    sizes[tag] = os.path.getsize(dst)
                    if rnd:
                        runs["%s %s" % (tag, loop)].append(times[0])
                    elif loop == "streamed":
                        rings[tag] = dict(loopmod.last_stream).get("ring_bytes", 0)
                    print("[depth_anything] %-13s %-9s round %d: %.3f s" % (tag, loop, rnd, times[0]), file=sys.stderr, flush=True)
        finally:
            mod.run_sharded = orig
            mod.model.close()
            mod.model = None
            os.environ.pop("PRISMA_Y4M_OUT", None)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        report["depth_loop"] = {"encoder": a.encoder, "loop_s": runs, "median_s": med, "ring_bytes": rings, "file_bytes": sizes,
                                "lossless_over_default": {loop: med["C444p12,full " + loop] / med["default " + loop] for loop in ("blocking", "streamed")}}
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
    print("(b) %d x %d -> %d x %d, resized on the way out" % (small[1], small[0], W, H))
    for v in pair:
        print("    %-34s %7.3f ms  %7.1f MB   (runs: %s)" % (v["way"], v["ms"], v["bytes"] / 1e6, " / ".join("%.3f" % r for r in v["runs_ms"])))
    d = report["depth_loop"]
    print("(c) depth_anything %s loop on a .y4m clip: seconds per clip (runs), median" % d["encoder"])
    for key, v in d["loop_s"].items():
        print("    %-24s %-26s %7.3f" % (key, " / ".join("%.3f" % x for x in v), d["median_s"][key]))
    print("    C444p12,full / default: blocking %.3f, streamed %.3f; files %s MB; streamed rings %s MB" % (
        d["lossless_over_default"]["blocking"], d["lossless_over_default"]["streamed"],
        " / ".join("%s %.1f" % (k, v / 1e6) for k, v in d["file_bytes"].items()), " / ".join("%s %.1f" % (k, v / 1e6) for k, v in d["ring_bytes"].items())))


if __name__ == "__main__":
    main()
