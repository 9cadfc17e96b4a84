#!/usr/bin/env python3
"""Wall time of `process.py --jobs 1` against `--jobs N` on one clip: the measurement of EXPERIMENTS.md "process.py --jobs".

    python tools/process_jobs_ab.py [--frames 32] [--height 1080] [--width 1920] [--jobs 3] [--gpus 1] [--runs 3] [--limit 600]

Builds a synthetic .npy clip in a temporary folder, then runs process.py on it with the default bands and the real presets
(PRISMA_SYNTH=1: seeded weights), `--runs` times each way, interleaved (1, N, 1, N, ...), every run into a fresh output folder and
under a time limit of its own.  Prints every wall time and the ratio of the medians; stops at the first run that fails.  This
process never opens the GPU: only the band children do."""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=600, help="seconds one process.py run may take")
    args = ap.parse_args()
    import numpy as np
    from prisma_amd import synth
    tmp = tempfile.mkdtemp(prefix="process_jobs_ab_")
    try:
        clip = os.path.join(tmp, "clip.npy")
        np.save(clip, synth.frames(args.frames, args.height, args.width, seed=7))
        env = dict(os.environ, PRISMA_SYNTH="1", PRISMA_OVERWRITE="1")
        times = {1: [], args.jobs: []}
        for run in range(args.runs):
            for jobs in (1, args.jobs):
                out = os.path.join(tmp, "out_%d_%d" % (jobs, run))
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, os.path.join(ROOT, "process.py"), "-i", clip, "--output", out, "--jobs", str(jobs),
                                    "--gpus", str(args.gpus)], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                                   timeout=args.limit)
                dt = time.perf_counter() - t0
                if r.returncode != 0:
                    raise SystemExit("run %d --jobs %d failed (exit %d) after %.1f s:\n%s" % (run, jobs, r.returncode, dt, r.stderr[-3000:]))
                times[jobs].append(dt)
                print("run %d  --jobs %d --gpus %d  %7.2f s" % (run, jobs, args.gpus, dt), flush=True)
                shutil.rmtree(out)
        m1, mn = statistics.median(times[1]), statistics.median(times[args.jobs])
        print("%d frames %dx%d: median --jobs 1 %.2f s, --jobs %d %.2f s, ratio serial / parallel %.3f"
              % (args.frames, args.width, args.height, m1, args.jobs, mn, m1 / mn))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
