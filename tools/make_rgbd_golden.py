#!/usr/bin/env python3
"""Write tests/golden/rgbd_hue.npz from the REAL reference functions (build machine only: needs /root/reference, read-only).

The rgba band's RGB-D split re-encodes the hue-coded depth half as (rgba.py:61-63)
    heat = np.clip(rgb_to_hsv(crop)[..., 0] / 360.0, 0.0, 1.0);  frame = heat_to_rgb(heat) * 255.0  -> uint8 in the video writer
with rgb_to_hsv / heat_to_rgb of bands/common/encode.py:13-58.  The input is three bytes, so the fixture covers the whole domain:
  sha256        SHA-256 of the 2^24 x 3 output bytes, colours in (r, g, b) order with r slowest
  colours       a sample - the 256 greys, the 1536 fully saturated ring colours, 4096 seeded random colours (tests/rgbd_ref.py
                sample_colours) - with the reference's `rgb` bytes and float64 `heat`
Data only.  cv2 (imported by encode.py for Sobel alone) is stubbed, as oracle/make_golden.py does.
"""
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "bands"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
from common import encode as E  # noqa: E402

import rgbd_ref as R  # noqa: E402


def reference(colours):
    """colours [N, 3] uint8 (N a multiple of 1024) -> (heat float64 [N], rgb uint8 [N, 3]) through the reference's own functions"""
    crop = colours.reshape(-1, 1024, 3)
    heat = np.clip(E.rgb_to_hsv(crop)[..., 0] / 360.0, 0.0, 1.0)
    rgb = (E.heat_to_rgb(heat) * 255.0).astype(np.uint8)        # VideoWriter.write: astype(np.uint8)
    return heat.reshape(-1), rgb.reshape(-1, 3)


def main():
    h = hashlib.sha256()
    for lo in range(0, 1 << 24, 1 << 20):
        h.update(reference(R.all_colours(lo, lo + (1 << 20)))[1].tobytes())
    s = R.sample_colours()
    pad = (-len(s)) % 1024
    heat, rgb = reference(np.concatenate([s, np.zeros((pad, 3), np.uint8)]))
    out = os.path.join(ROOT, "tests", "golden", "rgbd_hue.npz")
    np.savez_compressed(out, sha256=np.array(h.hexdigest()), colours=s, rgb=rgb[:len(s)], heat=heat[:len(s)])
    print("[rgbd_hue] sha256 of the 2^24 x 3 table %s; %d sample colours; %d bytes" % (h.hexdigest(), len(s), os.path.getsize(out)))


if __name__ == "__main__":
    main()
