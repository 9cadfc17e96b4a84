#!/usr/bin/env python3
"""Time the rgba band's hue decode (pb_rgbd_depth / pb_rgbd_depth_dev, hue_heat_kernel) on 32 side-by-side frames of 1920 x 1080, depth on
the right:
  * hue_heat_kernel per frame - back-to-back pb_rgbd_depth_dev calls on resident frames between two device synchronisations - and its
    achieved bytes per second: 3 bytes read and 3 (bytes) + 4 (heat) written per pixel of the depth half;
  * frames per second of the blocking host-pointer call (pageable and page-locked caller arrays);
  * seconds per frame of the float64 numpy restatement (tests/rgbd_ref.py) on this host - the arithmetic the reference runs per frame.
EXPERIMENTS.md keeps the figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rgbd_ref as R  # noqa: E402
from prisma_amd import engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--side", default="right", choices=R.SIDES)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=2, help="frames the numpy restatement is timed on")
    a = ap.parse_args()
    n, H, W = a.frames, a.height, a.width
    fr = np.random.default_rng(0).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    _, db = engine.rgbd_boxes(H, W, a.side)
    px = (db[1] - db[0]) * (db[3] - db[2])
    ops = engine.Ops()
    pf, po, ph = ops.dev_alloc(fr.nbytes), ops.dev_alloc(n * px * 3), ops.dev_alloc(n * px * 4)
    ops.h2d(pf, fr)
    for what, dp, hp, bpp in (("bytes + heat", po, ph, 10), ("bytes alone", po, 0, 6), ("heat alone", 0, ph, 7)):
        for _ in range(3):
            ops.rgbd_depth_dev(pf, n, H, W, a.side, depth_ptr=dp, heat_ptr=hp)
        ops.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            ops.rgbd_depth_dev(pf, n, H, W, a.side, depth_ptr=dp, heat_ptr=hp)
        ops.sync()
        dt = (time.perf_counter() - t0) / a.iters
        print("hue_heat_kernel, %s: %d frames of %dx%d (%s half %dx%d): %.4f ms per call, %.2f us per frame; %d B/px = %.1f MB -> %.0f GB/s" % (
            what, n, W, H, a.side, db[3] - db[2], db[1] - db[0], dt * 1e3, dt / n * 1e6, bpp, bpp * n * px / 1e6, bpp * n * px / dt / 1e9))
    got = np.empty((n, db[1] - db[0], db[3] - db[2], 3), np.uint8)
    ops.d2h(got, po)
    for p in (pf, po, ph):
        ops.dev_free(p)

    import torch
    pin = [torch.empty(s, dtype=t).pin_memory().numpy() for s, t in ((fr.shape, torch.uint8), (got.shape, torch.uint8), (got.shape[:3], torch.float32))]
    pin[0][...] = fr
    for what, f, kw in (("pageable arrays", fr, {}), ("page-locked arrays", pin[0], dict(out_rgb=pin[1], out_heat=pin[2]))):
        ops.rgbd_depth(f, a.side, want_heat=True, **kw)
        t0 = time.perf_counter()
        for _ in range(5):
            rgb, heat = ops.rgbd_depth(f, a.side, want_heat=True, **kw)
        dt = (time.perf_counter() - t0) / 5
        print("pb_rgbd_depth (blocking, host pointers, bytes + heat), %s: %.2f ms per call of %d frames = %.0f frames/s" % (what, dt * 1e3, n, n / dt))
    ops.close()

    k = min(n, a.host_frames)
    t0 = time.perf_counter()
    _, want, hw = R.split_restated(fr[:k], a.side)
    host = (time.perf_counter() - t0) / k
    print("host float64 numpy restatement: %.3f s per frame; GPU bytes equal: %s, heat equal: %s" % (
        host, np.array_equal(got[:k], want), np.array_equal(heat[:k], hw.astype(np.float32))))


if __name__ == "__main__":
    main()
