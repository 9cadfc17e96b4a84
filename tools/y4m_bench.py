#!/usr/bin/env python3
"""What .y4m clips cost and save, measured in one visit on 32 frames of 1920 x 1080 (EXPERIMENTS.md 6.21):

 (a) the two conversion kernels alone (prisma_amd/csrc/yuv.hip, device-resident frames): ms per launch of all 32 frames between two stream
     synchronisations, and GB/s of the 4.5 bytes per pixel each moves - to be read next to the effective HBM rate DESIGN.md section 5 gives
     for the project's other one-pass kernels;
 (b) the host restatement (bands/common/yuv.py, numpy on one core): frames per second in either direction - what a band loop's one decode
     thread would deliver if the conversion stayed on the host;
 (c) the depth and flow band loops on the clip as a .y4m (I420 in, I420 out) against the same frames as an .npy stack, each with the blocking
     and with the streamed loop: wall time of the loop (run_sharded inside process_video: not the model load) and the page-locked bytes - the
     streamed loop's rings as the loop reports them, the blocking loop's staging inside the library computed from the chunk's shapes (two slots
     per array).  The .npy run is the baseline: the only clip the parent commit can run.  Files live in a tmpfs folder.

  python tools/y4m_bench.py --out profiles/y4m_bench.json > profiles/y4m_bench.txt

No threshold is set: nobody had measured any of the three."""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(np, engine, n, H, W, iters):
    ops = engine.Ops()
    fb = engine.i420_bytes(H, W)
    rgb_b, yuv_b = n * H * W * 3, n * fb
    d_rgb, d_yuv = ops.dev_alloc(rgb_b), ops.dev_alloc(yuv_b)
    out = {}
    try:
        rng = np.random.default_rng(0)
        ops.h2d(d_rgb, rng.integers(0, 256, rgb_b, dtype=np.uint8))
        ops.h2d(d_yuv, rng.integers(0, 256, yuv_b, dtype=np.uint8))
        for name, call in (("rgb_to_i420", lambda: ops.rgb_to_i420_dev(d_rgb, n, H, W, d_yuv)), ("i420_to_rgb", lambda: ops.i420_to_rgb_dev(d_yuv, n, H, W, d_rgb))):
            for _ in range(3):
                call()
            ops.sync()
            runs = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(iters):
                    call()
                ops.sync()
                runs.append((time.perf_counter() - t0) / iters)
            ms = sorted(runs)[len(runs) // 2] * 1e3
            out[name] = {"ms_per_launch": ms, "runs_ms": [r * 1e3 for r in runs], "bytes": rgb_b + yuv_b, "GBps": (rgb_b + yuv_b) / (ms * 1e-3) / 1e9}
    finally:
        ops.dev_free(d_rgb)
        ops.dev_free(d_yuv)
        ops.close()
    return out


def host(np, yuv, H, W, frames=6):
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    planes = yuv.rgb_to_i420(rgb)
    out = {}
    for name, call in (("rgb_to_i420", lambda: yuv.rgb_to_i420(rgb)), ("i420_to_rgb", lambda: yuv.i420_to_rgb(planes, H, W))):
        call()
        t0 = time.perf_counter()
        for _ in range(frames):
            call()
        out[name] = {"fps": frames / (time.perf_counter() - t0)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--bands", default="depth_anything,flow_raft,flow_gmflow")
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per arm, interleaved; one untimed run of each arm goes first")
    ap.add_argument("--encoder", default="vitl")
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window of (a)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["PRISMA_SYNTH"] = "1"
    os.environ["PRISMA_OVERWRITE"] = "1"
    os.environ.pop("PRISMA_BATCH", None)
    os.environ["OMP_NUM_THREADS"] = os.environ["OPENBLAS_NUM_THREADS"] = "1"         # (b) is one core's figure
    for p in (os.path.join(HERE, "bands"), HERE):
        sys.path.insert(0, p)
    import numpy as np
    from prisma_amd import engine, synth
    from common import flow as flowmod
    from common import io as iomod
    from common import loop as loopmod
    from common import yuv

    n, H, W = a.frames, a.height, a.width
    report = {"frames": n, "frame": [H, W], "kernels": kernels(np, engine, n, H, W, a.iters), "host": host(np, yuv, H, W), "bands": {}}
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > (4 << 30) else None
    work = tempfile.mkdtemp(prefix="y4m_bench.", dir=base)
    try:
        for name in [b for b in a.bands.split(",") if b]:
            mod = importlib.import_module(name)
            flow = name.startswith("flow")
            chunk = mod.CHUNK if flow else mod.BATCH
            rgb = synth.frame_pair_sequence(n, H, W, seed=7) if flow else synth.frames(n, H, W, seed=7)
            # the clip twice: the .y4m, and the .npy stack of the frames a host-side reader decodes from it - the two runs see the same pixels
            clips = {"y4m": os.path.join(work, name + "_in.y4m"), "npy": os.path.join(work, name + "_in.npy")}
            w = iomod.VideoWriter(W, H, 24, clips["y4m"])
            for f in rgb:
                w.write(f)
            w.close()
            src = iomod.FrameReader(clips["y4m"])
            np.save(clips["npy"], np.stack([src[i] for i in range(n)]))
            del rgb, src
            ns = argparse.Namespace(subpath="", npy=False, ply=False, metric="none", encoder=a.encoder, weights="", synthetic=True, backwards=False, mask=False,
                                    output_mask="", subpath_mask="", scale=0.75, model="", iterations=getattr(mod, "ITERATIONS", 1), small=False,
                                    mixed_precision=False, alternate_corr=False)
            holder, times = (flowmod if flow else mod), []
            orig = holder.run_sharded

            def timed(*args, _orig=orig, **kw):
                t0 = time.perf_counter()
                r = _orig(*args, **kw)
                times.append(time.perf_counter() - t0)
                return r
            holder.run_sharded = timed
            if name == "depth_anything":
                mod.args = ns
                mod.init_model(a.encoder, "", device=0)
            else:
                mod.init_model(ns, device=0)
            arms = [(ext, loop) for loop in ("blocking", "streamed") for ext in ("npy", "y4m")]
            runs = {"%s %s" % arm: [] for arm in arms}
            pinned = {}
            try:
                for rnd in range(a.rounds + 1):             # round 0 is the untimed one
                    for ext, loop in arms:
                        os.environ["PRISMA_STREAM"] = "1" if loop == "streamed" else "0"
                        del times[:]
                        mod.process_video(argparse.Namespace(input=clips[ext], output=os.path.join(work, name + "." + ext), **vars(ns)))
                        assert len(times) == 1
                        key = "%s %s" % (ext, loop)
                        if rnd:
                            runs[key].append(times[0])
                        elif loop == "streamed":
                            pinned[key] = dict(loopmod.last_stream).get("ring_bytes", 0)
                        else:   # the library's staging for pageable arrays: two slots of a chunk's frames (+ the halo frame of pairs) in, of its encoded frames and scalars out
                            units = min(chunk, n - 1 if flow else n)
                            sh, sw = engine.flow_out_size(H, W, ns.scale) if flow else (H, W)
                            fin = engine.i420_bytes(H, W) if ext == "y4m" else H * W * 3
                            fout = engine.i420_bytes(sh, sw) if ext == "y4m" else sh * sw * 3
                            pinned[key] = 2 * ((units + (1 if flow else 0)) * fin + units * (fout + (4 if flow else 8)))
                        print("[%s] %-12s round %d: %.3f s" % (name, key, rnd, times[0]), file=sys.stderr, flush=True)
            finally:
                holder.run_sharded = orig
                mod.model.close()
                mod.model = None
            med = {k: float(np.median(v)) for k, v in runs.items()}
            report["bands"][name] = {"chunk_units": chunk, "loop_s": runs, "median_s": med, "spread_s": {k: float(max(v) - min(v)) for k, v in runs.items()},
                                     "pinned_bytes": pinned, "y4m_over_npy": {loop: med["y4m " + loop] / med["npy " + loop] for loop in ("blocking", "streamed")}}
            for p in os.listdir(work):
                os.remove(os.path.join(work, p))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    print("%d frames of %d x %d" % (n, W, H))
    print("(a) kernels alone, device-resident frames, 4.5 bytes per pixel")
    for k, v in report["kernels"].items():
        print("    %-12s %7.3f ms per launch of %d frames  %7.1f GB/s   (runs: %s)" % (k, v["ms_per_launch"], n, v["GBps"], " / ".join("%.3f" % r for r in v["runs_ms"])))
    print("(b) host restatement, numpy, one core")
    for k, v in report["host"].items():
        print("    %-12s %7.2f frames per second" % (k, v["fps"]))
    print("(c) band loops: seconds per clip (runs), median, page-locked MB")
    for name, b in report["bands"].items():
        for key, v in b["loop_s"].items():
            print("    %-15s %-13s %-26s %7.3f  %8.1f MB" % (name, key, " / ".join("%.3f" % x for x in v), b["median_s"][key], b["pinned_bytes"][key] / 1e6))
        print("    %-15s y4m / npy: blocking %.3f, streamed %.3f" % (name, b["y4m_over_npy"]["blocking"], b["y4m_over_npy"]["streamed"]))


if __name__ == "__main__":
    main()
