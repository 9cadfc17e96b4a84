#!/usr/bin/env python3
"""Time pb_depth_point_cloud_dev (the depth band's --ply kernel) on one frame: per-call device time from pb_set_profiling /
pb_get_kernel_stats (HIP events around the call on the ctx stream), its 22 algorithmic bytes per pixel (4 depth + 3 colour in, 15 vertex
out) over that time, and the float32 numpy restatement (tests/pcl_ref.py) on this host.  EXPERIMENTS.md keeps the figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcl_ref as R  # noqa: E402
from prisma_amd import engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    H, W = a.height, a.width
    depth, rgb = R.make_case(H, W)
    # kernel statistics live on a band's timer: the smallest depth model carries the ctx
    net = engine.DepthAnything(synth.depth_anything_weights(synth.DEPTH_CFGS["vits"], seed=1234), "vits", device=0, max_batch=1)
    pd, pc, po = net.dev_alloc(depth.nbytes), net.dev_alloc(rgb.nbytes), net.dev_alloc(H * W * 15)
    net.h2d(pd, depth)
    net.h2d(pc, rgb)
    got = None
    for flip in (0, 1):
        for _ in range(5):
            net.point_cloud_dev(pd, pc, 1, H, W, po, flip=bool(flip))
        net.sync()
        net.set_profiling(timing=True, accumulate=True)
        for _ in range(a.iters):
            net.point_cloud_dev(pd, pc, 1, H, W, po, flip=bool(flip))
        st = [s for s in net.kernel_stats() if s["name"] == "depth_point_cloud"]
        net.set_profiling(timing=False)
        assert len(st) == 1 and st[0]["launches"] == a.iters, st
        ms = st[0]["ms"] / a.iters
        what = "min / max reduction + point_cloud_kernel" if flip else "point_cloud_kernel alone"
        print("%dx%d flip %d (%s): %.4f ms per call over %d calls; 22 B/px = %.1f MB -> %.0f GB/s" % (
            H, W, flip, what, ms, a.iters, 22e-6 * H * W, st[0]["bytes"] / a.iters / (ms * 1e-3) / 1e9))
        got = np.empty(H * W * 15, np.uint8)
        net.d2h(got, po)
    t0 = time.perf_counter()
    want = R.cloud_restated(depth, rgb, 1, W / 2, H / 2)
    host = time.perf_counter() - t0
    print("host float32 numpy restatement, one frame: %.3f s; GPU bytes equal: %s" % (host, np.array_equal(got, R.raw(want).reshape(-1))))
    for p in (pd, pc, po):
        net.dev_free(p)
    net.close()


if __name__ == "__main__":
    main()
