#!/usr/bin/env python3
"""What Motion JPEG output costs and loses, measured in one visit (EXPERIMENTS.md 6.29):

 (a) the encoder on 32 frames of 1920 x 1080 of band-like content - a depth heat ramp, a flow colour wheel, grey mask ids; synthetic pictures
     with the bands' statistics (smooth ramps, flat regions, hard edges), not network output - at quality 90 in 4:4:4 and 4:2:0: ms per call of
     pb_jpeg_encode_dev (device-resident planes, the window ends in a stream synchronisation) and of pb_jpeg_encode (page-locked host arrays,
     copies included), bytes per frame, and beside them Pillow's save(format="JPEG") of the same frames on one host thread and on 16: the
     yardstick.  Arms alternate inside one process; the first call of each is untimed.
 (b) the depth band loop on a .y4m clip writing .avi (PRISMA_VIDEO_OUT=avi: quality 90, 4:4:4) against the same loop writing the default
     .y4m: seconds per clip of run_sharded (not the model load), blocking and streamed, runs interleaved, files in a tmpfs folder, their sizes.
 (c) what the depth band's value loses through encode + Pillow's decode at qualities 75, 90, 95, 100 in 4:4:4 and 4:2:0: the hue decode of
     tests/rgbd_ref.py on the frame before and after, max and mean of the difference in heat units (hue fraction / 0.65).
 (d) with --parent (a built checkout of the parent commit): the depth loop writing the default .y4m in this tree against the same loop in the
     parent's, each tree in processes of its own, the trees alternating - the arm of (b) this change must not have slowed.

  python tools/jpeg_bench.py --parent <checkout of the parent commit> > profiles/jpeg_bench.txt"""
import argparse
import io as _io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def band_frames(np, kind, n, H, W):
    """uint8 [n, H, W, 3]: synthetic frames with the statistics of a band's video"""
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    out = np.empty((n, H, W, 3), np.uint8)
    rng = np.random.default_rng(3)
    for t in range(n):
        if kind == "depth":       # a smooth depth field with a few hard object edges, through the band's hue ramp
            d = 0.5 + 0.3 * np.sin(xx / 310 + t / 9) * np.cos(yy / 270) + 0.15 * (((xx // 480 + yy // 360 + t // 8) % 2) - 0.5)
            d += rng.normal(0, 0.002, d.shape).astype(np.float32)
            hue = (1.0 - np.clip(d, 0, 1)) * 0.65
            rgb = np.stack([hue * 6.0, hue * 6.0 + 4.0, hue * 6.0 + 2.0], -1)
            out[t] = (np.clip(np.abs(np.mod(rgb, 6.0) - 3.0) - 1.0, 0.0, 1.0) * 255).astype(np.uint8)
        elif kind == "flow":      # direction as hue, length as saturation
            u, v = np.sin(xx / 400 + t / 7) + 0.3 * np.sin(yy / 90), np.cos(yy / 350 - t / 11)
            ang = (np.arctan2(v, u) / (2 * np.pi)) % 1.0
            sat = np.clip(np.sqrt(u * u + v * v) / 1.5, 0, 1)
            k = np.stack([ang * 6.0, ang * 6.0 + 4.0, ang * 6.0 + 2.0], -1)
            wheel = np.clip(np.abs(np.mod(k, 6.0) - 3.0) - 1.0, 0.0, 1.0)
            out[t] = ((1.0 - sat[..., None] * (1.0 - wheel)) * 255).astype(np.uint8)
        else:                     # grey ids in flat regions with hard edges
            ids = ((xx + 40 * np.sin(yy / 60 + t / 5)) // 240 + 7 * (yy // 180)) % 21
            out[t] = np.repeat((ids * 12).astype(np.uint8)[..., None], 3, -1)
    return out


def encoder_arms(np, engine, n, H, W, rounds):
    from PIL import Image
    ops = engine.Ops()
    rows = []
    try:
        for kind in ("depth", "flow", "mask"):
            rgb = band_frames(np, kind, n, H, W)
            for chroma in (444, 420):
                fmt = engine.jpeg_format(chroma)
                fb = engine.yuv_bytes(fmt, H, W)
                planes = ops.host_empty((n, fb), np.uint8)
                ops.rgb_to_yuv(fmt, rgb, out=planes)
                cap = n * fb
                out = ops.host_empty(cap, np.uint8)
                d_in, d_out, d_off = ops.dev_alloc(n * fb), ops.dev_alloc(cap), ops.dev_alloc(8 * (n + 1))
                ops.h2d(d_in, planes)
                sub = {444: 0, 420: 2}[chroma]

                def dev():
                    ops.jpeg_encode_dev(d_in, n, H, W, chroma, 90, d_out, cap, d_off)
                    ops.sync()

                def host():
                    return ops.jpeg_encode(planes, H, W, chroma, 90, out=out)

                def save(f):
                    b = _io.BytesIO()
                    Image.fromarray(f).save(b, format="JPEG", quality=90, subsampling=sub)
                    return b.tell()

                def pil1():
                    return sum(save(f) for f in rgb)

                pool = ThreadPoolExecutor(16)

                def pil16():
                    return sum(pool.map(save, rgb))

                arms = {"pb_jpeg_encode_dev": dev, "pb_jpeg_encode": host, "Pillow 1 thread": pil1, "Pillow 16 threads": pil16}
                runs = {k: [] for k in arms}
                for rnd in range(rounds + 1):               # round 0 is the untimed one
                    for k, call in arms.items():
                        t0 = time.perf_counter()
                        call()
                        if rnd:
                            runs[k].append((time.perf_counter() - t0) * 1e3)
                pool.shutdown()
                _, offs = host()
                rows.append({"content": kind, "chroma": chroma, "bytes_per_frame": int(offs[n]) // n, "pillow_bytes_per_frame": pil1() // n,
                             "ms_per_call": {k: float(np.median(v)) for k, v in runs.items()}, "runs_ms": runs})
                print("[encoder] %s %d done" % (kind, chroma), file=sys.stderr, flush=True)
                for p in (d_in, d_out, d_off):
                    ops.dev_free(p)
                ops.host_free(planes)
                ops.host_free(out)
    finally:
        ops.close()
    return rows


def loss_table(np, engine, H, W):
    from PIL import Image
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import rgbd_ref
    ops = engine.Ops()
    rgb = band_frames(np, "depth", 2, H, W)
    before, _ = rgbd_ref.hue_heat(rgb)
    rows = []
    try:
        for chroma in (444, 420):
            planes = ops.rgb_to_yuv(engine.jpeg_format(chroma), rgb)
            for q in (75, 90, 95, 100):
                out, offs = ops.jpeg_encode(planes, H, W, chroma, q)
                back = np.stack([np.asarray(Image.open(_io.BytesIO(bytes(out[offs[i]:offs[i + 1]]))).convert("RGB")) for i in range(len(rgb))])
                after, _ = rgbd_ref.hue_heat(back)
                err = np.abs(after - before) / 0.65
                rows.append({"chroma": chroma, "quality": q, "max": float(err.max()), "mean": float(err.mean()), "p999": float(np.quantile(err, 0.999)),
                             "bytes_per_frame": int(offs[len(rgb)]) // len(rgb)})
    finally:
        ops.close()
    return rows


def loop_child(a):
    """--loop-child: the depth loop of the tree in --tree writing the default .y4m, blocking and streamed, one untimed run and --rounds timed
    ones of each -> one JSON line on stdout"""
    for p in (os.path.join(a.tree, "bands"), a.tree):
        sys.path.insert(0, p)
    os.environ.update(PRISMA_SYNTH="1", PRISMA_OVERWRITE="1")
    for k in ("PRISMA_BATCH", "PRISMA_Y4M_MATRIX", "PRISMA_Y4M_OUT", "PRISMA_VIDEO_OUT"):
        os.environ.pop(k, None)
    import depth_anything as mod
    ns = dict(subpath="", npy=False, ply=False, metric="none", encoder=a.encoder, weights="", synthetic=True)
    mod.args = argparse.Namespace(**ns)
    mod.init_model(a.encoder, "", device=0)
    out = os.path.join(os.path.dirname(a.clip), "depth_%d.y4m" % os.getpid())
    runs = {"blocking": [], "streamed": []}
    try:
        for rnd in range(a.rounds + 1):
            for loop in runs:
                os.environ["PRISMA_STREAM"] = "1" if loop == "streamed" else "0"
                t0 = time.perf_counter()
                mod.process_video(argparse.Namespace(input=a.clip, output=out, **ns))
                if rnd:
                    runs[loop].append(time.perf_counter() - t0)
        size = os.path.getsize(out)
    finally:
        mod.model.close()
        for p in (out, out[:-4] + "_min.csv", out[:-4] + "_max.csv"):
            if os.path.exists(p):
                os.remove(p)
    print(json.dumps({"clip_s": runs, "file_bytes": size}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per arm, interleaved; one untimed run of each arm goes first")
    ap.add_argument("--encoder", default="vitl")
    ap.add_argument("--out", default="")
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: the other arm of (d); without it (d) is left out")
    ap.add_argument("--visits", type=int, default=2, help="processes per tree in (d), the trees alternating")
    ap.add_argument("--loop-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--clip", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop_child:
        return loop_child(a)
    os.environ["PRISMA_SYNTH"] = "1"
    os.environ["PRISMA_OVERWRITE"] = "1"
    for k in ("PRISMA_BATCH", "PRISMA_Y4M_MATRIX", "PRISMA_Y4M_OUT", "PRISMA_VIDEO_OUT"):
        os.environ.pop(k, None)
    for p in (os.path.join(HERE, "bands"), HERE):
        sys.path.insert(0, p)
    import numpy as np
    from prisma_amd import engine, synth
    import depth_anything as mod
    from common import yuv

    n, H, W = a.frames, a.height, a.width
    report = {"frames": n, "frame": [H, W], "encoder": encoder_arms(np, engine, n, H, W, a.rounds), "loss": loss_table(np, engine, H, W)}
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > (4 << 30) else None
    work = tempfile.mkdtemp(prefix="jpeg_bench.", dir=base)
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
        outs = {"y4m (default)": ("", "y4m"), "avi q=90 444": ("avi", "avi")}
        arms = [(tag, loop) for loop in ("blocking", "streamed") for tag in outs]
        runs = {"%s %s" % arm: [] for arm in arms}
        sizes = {}
        try:
            for rnd in range(a.rounds + 1):                 # round 0 is the untimed one
                for tag, loop in arms:
                    os.environ["PRISMA_STREAM"] = "1" if loop == "streamed" else "0"
                    os.environ["PRISMA_VIDEO_OUT"] = outs[tag][0]
                    del times[:]
                    dst = os.path.join(work, "depth." + outs[tag][1])
                    t0 = time.perf_counter()
                    mod.process_video(argparse.Namespace(input=clip, output=dst, **ns))
                    whole = time.perf_counter() - t0        # with the writer's close(): the last group is encoded there
                    assert len(times) == 1
                    sizes[tag] = os.path.getsize(dst)
                    if rnd:
                        runs["%s %s" % (tag, loop)].append(whole)
                    print("[depth_anything] %-14s %-9s round %d: loop %.3f s, with close %.3f s" % (tag, loop, rnd, times[0], whole), file=sys.stderr, flush=True)
        finally:
            mod.run_sharded = orig
            mod.model.close()
            mod.model = None
            os.environ.pop("PRISMA_VIDEO_OUT", None)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        report["depth_loop"] = {"encoder": a.encoder, "clip_s": runs, "median_s": med, "fps": {k: n / v for k, v in med.items()}, "file_bytes": sizes}
        if a.parent:
            trees = [("this tree", HERE), ("parent", os.path.abspath(a.parent))]
            both = {name: {"blocking": [], "streamed": []} for name, _ in trees}
            for visit in range(a.visits):
                for name, tree in (trees if visit % 2 == 0 else trees[::-1]):
                    env = dict(os.environ)
                    env.pop("PRISMA_BANDS_LIB", None)
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-child", "--tree", tree, "--clip", clip, "--encoder", a.encoder,
                                        "--rounds", str(a.rounds)], env=env, capture_output=True, text=True, timeout=600)
                    if r.returncode != 0:
                        raise SystemExit("(d) %s: exit %d\n%s" % (name, r.returncode, r.stderr[-3000:]))
                    got = json.loads(r.stdout.strip().splitlines()[-1])
                    for loop, v in got["clip_s"].items():
                        both[name][loop] += v
                    both[name]["file_bytes"] = got["file_bytes"]
                    print("[depth_anything] %-9s visit %d: %s" % (name, visit, got["clip_s"]), file=sys.stderr, flush=True)
            report["y4m_against_parent"] = {name: {"clip_s": {k: v[k] for k in ("blocking", "streamed")}, "file_bytes": v["file_bytes"],
                                                   "median_s": {k: float(np.median(v[k])) for k in ("blocking", "streamed")}} for name, v in both.items()}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    print("%d frames of %d x %d, quality 90" % (n, W, H))
    print("(a) ms per call of all %d frames (median of %d; Pillow: the yardstick), bytes per frame" % (n, a.rounds))
    for r in report["encoder"]:
        m = r["ms_per_call"]
        best = min(m["Pillow 1 thread"], m["Pillow 16 threads"])
        print("    %-5s %d  dev %8.2f  host %8.2f  Pillow x1 %8.1f  x16 %8.1f   %8d B/frame (Pillow %8d)   host / best Pillow %.2f - the GPU path %s"
              % (r["content"], r["chroma"], m["pb_jpeg_encode_dev"], m["pb_jpeg_encode"], m["Pillow 1 thread"], m["Pillow 16 threads"], r["bytes_per_frame"],
                 r["pillow_bytes_per_frame"], m["pb_jpeg_encode"] / best, "beats it" if m["pb_jpeg_encode"] < best else "does NOT beat it"))
    d = report["depth_loop"]
    print("(b) depth_anything %s on a .y4m clip, process_video without the model load: seconds per clip (runs), median, frames / s, file" % d["encoder"])
    for key, v in d["clip_s"].items():
        print("    %-26s %-26s %7.3f  %7.1f fps  %8.1f MB" % (key, " / ".join("%.3f" % x for x in v), d["median_s"][key], d["fps"][key],
                                                               d["file_bytes"][key.rsplit(" ", 1)[0]] / 1e6))
    if "y4m_against_parent" in report:
        print("(d) the same loop writing the default .y4m, this tree against the parent commit, a process per visit: seconds per clip (runs), median, frames / s")
        yp = report["y4m_against_parent"]
        for name, v in yp.items():
            for loop in ("blocking", "streamed"):
                print("    %-9s %-9s %-50s %7.3f  %7.1f fps  %8.1f MB" % (name, loop, " / ".join("%.3f" % x for x in v["clip_s"][loop]), v["median_s"][loop],
                                                                       n / v["median_s"][loop], v["file_bytes"] / 1e6))
        print("    this tree / parent: blocking %.3f, streamed %.3f" % tuple(yp["this tree"]["median_s"][k] / yp["parent"]["median_s"][k] for k in ("blocking", "streamed")))
    print("(c) heat lost by depth frames through encode + Pillow decode (hue decode of tests/rgbd_ref.py, heat units)")
    for r in report["loss"]:
        print("    %d q=%-3d  max %.5f  p99.9 %.5f  mean %.6f   %8d B/frame" % (r["chroma"], r["quality"], r["max"], r["p999"], r["mean"], r["bytes_per_frame"]))


if __name__ == "__main__":
    main()
