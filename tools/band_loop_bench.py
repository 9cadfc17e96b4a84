#!/usr/bin/env python3
"""A/B of the band scripts' two chunk loops (bands/common/loop.py): PRISMA_STREAM=0, one blocking engine call per chunk on pageable arrays,
against PRISMA_STREAM=1, submit / wait on page-locked rings - each band's own process_video on a seeded clip that lives in memory (.npy in a
tmpfs folder in, .npy out: decode and encode are memcpys), the model loaded once, the arms interleaved A/B/A/B in one process.

What is timed is the call of run_sharded inside process_video (the loop; not the model load, not the final np.save of the output video).
Shapes: chunks of the script's own default size (PRISMA_BATCH unset: 32 frames for depth_anything and mask_mmdet, 16 pairs for the flow bands;
--flow-chunk 32 for the bench clip's 32) at 1920 x 1080, flow at --scale 0.75, default presets (ViT-L; RAFT 20 iterations; GMFlow; SOLOv2 R-101).

  python tools/band_loop_bench.py --out profiles/band_loop_ab.json
  python tools/band_loop_bench.py --tree <checkout of another commit> --arms blocking --out parent.json      # that commit's loop, this build's library

The default of a band follows from the table (EXPERIMENTS.md 6.19): streamed only if its median lies inside the blocking arm's min - max of the
visit (its run-to-run spread), or below it."""
import argparse
import hashlib
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", default="depth_anything,flow_raft,flow_gmflow,mask_mmdet")
    ap.add_argument("--arms", default="blocking,streamed")
    ap.add_argument("--chunks", type=int, default=6, help="chunks per clip")
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per arm, interleaved; one untimed run of each arm goes first")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--encoder", default="vitl")
    ap.add_argument("--arch", default="r101")
    ap.add_argument("--flow-chunk", type=int, default=0, help="pairs per chunk of the flow bands (0: the scripts' default)")
    ap.add_argument("--tree", default="", help="take bands/ and prisma_amd/*.py from this checkout (another commit's loop) with this tree's library")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    root = os.path.abspath(a.tree) if a.tree else HERE
    if a.tree:
        os.environ.setdefault("PRISMA_BANDS_LIB", os.path.join(HERE, "prisma_amd", "libprisma_bands.so"))
    os.environ["PRISMA_SYNTH"] = "1"
    os.environ.pop("PRISMA_BATCH", None)
    for p in (os.path.join(root, "bands"), root):
        sys.path.insert(0, p)
    import numpy as np
    from prisma_amd import synth
    from common import loop as loopmod
    from common import flow as flowmod

    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > (8 << 30) else None
    work = tempfile.mkdtemp(prefix="band_loop_bench.", dir=base)
    arms = a.arms.split(",")
    report = {"tree": root, "tmp": work, "frame": [a.height, a.width], "chunks": a.chunks, "rounds": a.rounds, "bands": {}}
    try:
        for name in a.bands.split(","):
            mod = importlib.import_module(name)
            flow = name.startswith("flow")
            if flow and a.flow_chunk:
                mod.CHUNK = a.flow_chunk
            chunk = mod.CHUNK if flow else mod.BATCH
            n = a.chunks * chunk + (1 if flow else 0)
            # the clip: one seeded chunk, repeated with a horizontal roll per chunk (the engines' work does not depend on the content)
            seed_frames = synth.frame_pair_sequence(chunk, a.height, a.width, seed=7) if flow else synth.frames(chunk, a.height, a.width, seed=7)
            clip_path = os.path.join(work, name + "_in.npy")
            clip = np.lib.format.open_memmap(clip_path, mode="w+", dtype=np.uint8, shape=(n, a.height, a.width, 3))
            for k in range(a.chunks):
                clip[k * chunk:(k + 1) * chunk] = np.roll(seed_frames, 16 * k, axis=2)
            if flow:
                clip[-1] = np.roll(seed_frames[0], 16 * a.chunks, axis=1)
            clip.flush()
            del clip, seed_frames
            out_path = os.path.join(work, name + ".npy")
            ns = argparse.Namespace(input=clip_path, output=out_path, subpath="", npy=False, ply=False, metric="none", encoder=a.encoder, weights="",
                                    synthetic=True, backwards=False, mask=False, output_mask="", subpath_mask="", scale=0.75, model="", iterations=getattr(mod, "ITERATIONS", 1),
                                    small=False, mixed_precision=False, alternate_corr=False, confidence=0.5, sdf=True, arch=a.arch)
            holder = flowmod if flow else mod           # the module whose run_sharded name the band's process_video calls
            times = []
            orig = holder.run_sharded

            def timed(*args, _orig=orig, **kw):
                t0 = time.perf_counter()
                r = _orig(*args, **kw)
                times.append(time.perf_counter() - t0)
                return r
            holder.run_sharded = timed
            t0 = time.perf_counter()
            if name == "depth_anything":
                mod.args = ns
                mod.init_model(a.encoder, "", device=0)
            elif name == "mask_mmdet":
                mod._SYNTH[0] = True
                mod.data = {"bands": {}}
                mod.init_model(a.arch, "", device=0)
            else:
                mod.init_model(ns, device=0)
            t_init = time.perf_counter() - t0
            runs = {arm: [] for arm in arms}
            sha, ring, stats = {}, 0, []
            try:
                for rnd in range(a.rounds + 1):         # round 0 is the untimed one
                    for arm in arms:
                        os.environ["PRISMA_STREAM"] = "1" if arm == "streamed" else "0"
                        if os.path.exists(out_path):
                            os.remove(out_path)
                        del times[:]
                        mod.process_video(argparse.Namespace(**vars(ns)))
                        assert len(times) == 1
                        if rnd == 0:
                            sha[arm] = hashlib.sha256(open(out_path, "rb").read()).hexdigest()
                            if arm == "streamed":
                                ring = dict(getattr(loopmod, "last_stream", {})).get("ring_bytes", 0)
                        else:
                            runs[arm].append(1e3 * times[0] / a.chunks)
                            if arm == "streamed":       # what the rings cost this run: slots locked, seconds locking (decode, main thread) and freeing
                                ls = dict(getattr(loopmod, "last_stream", {}))
                                stats.append({"used": ls.get("used"), "ring_bytes": ls.get("ring_bytes"), "lock_s": [round(x, 4) for x in ls.get("lock_s", ())],
                                              "free_s": round(ls.get("free_s", 0.0), 4)})
                        print("[%s] %-8s round %d: %.1f ms / chunk" % (name, arm, rnd, 1e3 * times[0] / a.chunks), file=sys.stderr, flush=True)
            finally:
                holder.run_sharded = orig
                mod.model.close()
                mod.model = None
            b = {"chunk_units": chunk, "units": "pairs" if flow else "frames", "frames": n, "init_s": round(t_init, 2), "ms_per_chunk": runs,
                 "median": {k: float(np.median(v)) for k, v in runs.items()}, "spread": {k: float(max(v) - min(v)) for k, v in runs.items()},
                 "sha256": sha, "ring_bytes": ring, "rings": stats}
            if len(arms) == 2:
                m = b["median"]
                b["ratio"] = m[arms[1]] / m[arms[0]]
                b["identical_output"] = sha[arms[0]] == sha[arms[1]]
                # the criterion, set before the numbers: the streamed median inside the blocking arm's min - max of this visit, or below it
                b["streamed_default"] = bool(m["streamed"] <= max(runs["blocking"])) if set(arms) == {"blocking", "streamed"} else None
            report["bands"][name] = b
            for p in (clip_path, out_path):
                if os.path.exists(p):
                    os.remove(p)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print("band        chunk      arm        ms / chunk (runs)            median   spread   ring MB")
    for name, b in report["bands"].items():
        for arm, v in b["ms_per_chunk"].items():
            print("%-11s %3d %-6s %-10s %-28s %7.1f  %7.1f  %8.1f" % (name, b["chunk_units"], b["units"], arm, " / ".join("%.1f" % x for x in v), b["median"][arm],
                                                                    b["spread"][arm], b["ring_bytes"] / 1e6 if arm == "streamed" else 0.0))
        if "ratio" in b:
            print("%-11s streamed / blocking = %.3f, outputs identical: %s, streamed by default: %s" % (name, b["ratio"], b["identical_output"], b["streamed_default"]))
        for r in b.get("rings", []):
            print("%-11s   rings: slots used %s, %.1f MB, page-locking %s s (decode thread, main thread), freeing %.3f s" % (name, r["used"], (r["ring_bytes"] or 0) / 1e6, r["lock_s"], r["free_s"]))


if __name__ == "__main__":
    main()
