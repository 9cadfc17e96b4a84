"""float32 restatement of the reference's still-image point cloud (CPU only; a helper module of the tests, not a conftest).

write_pcl (bands/common/io.py:201-211) with create_point_cloud / save_point_cloud (bands/common/geom.py:5-47), as the depth_anything band calls it
for `--ply`: un-flip the relative model's range, cv2.medianBlur(depth, 5), pinhole back-projection, one packed (x, y, z, red, green, blue)
record per pixel.  Every step is numpy float32 arithmetic, one rounding per operation, in the reference's order.

cv2 and plyfile are not installed where these tests run, so two steps are restated rather than called:
  * cv2.medianBlur(float32, 5) is the exact median of the 5 x 5 window with the border replicated (also on maps smaller than 5): np.pad(mode="edge"),
    sliding_window_view, np.partition(..., 12).  tests/test_pcl_ref_cpu.py holds it to scipy.ndimage.median_filter(size=5, mode="nearest").
  * plyfile's vertex element for save_point_cloud's dtype is 15 packed bytes per record, VERTEX below.

`bug=` plants one of the mistakes the kernel can make (BUGS); tests/test_pcl_ref_cpu.py asserts that the cases of the GPU test see each of them.
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
TILE = (16, 64)                 # rows x columns one block of point_cloud_kernel owns (elementwise.hip PC_TH, PC_TW)

BUGS = ("fma",                  # mn + d * (mx - mn) contracted into one fused multiply-add
        "rcp",                  # (col - u0) * (1 / fx) instead of the division
        "border_zero",          # the median's border padded with zeros ...
        "border_reflect",       # ... or reflected, instead of replicated
        "pos_zero",             # y negated after the product (0 - m y): +0.0 where row == v0
        "median_first")         # write_pcl's un-flip run on the blurred map, so with the blurred map's min / max.  (With the raw map's
                                # min / max the order would not show: every step of the un-flip is monotone, also after rounding, and the
                                # median of an odd count commutes with a monotone map.)

# single frames of the GPU test: name -> (H, W, ties).  `ties`: depth quantised to quarter units, so windows hold equal values
SHAPES = {"2x3": (2, 3, False), "4x4": (4, 4, False), "5x7": (5, 7, False), "18x70": (18, 70, True), "67x131": (67, 131, False),
          # three tiles and a remainder in both directions (TILE = 16 x 64): rows 16 + 16 + 5, columns 64 + 64 + 22
          "37x150": (37, 150, False)}

# non-default intrinsics on a 6 x 9 map (odd W: u0 = W / 2 is fractional): (u0, v0, fx, fy)
INTRINSICS = [(9 / 2, 6 / 2, 731.5, 1210.25),       # the reference's centre, fx != fy: row H / 2 = 3 stores y = -0.0
              (2.25, 4.0, 1210.25, 731.5)]          # off-centre both ways; v0 is row 4


def make_case(H: int, W: int, ties: bool = False, seed: int = 0, lo: float = 0.5, span: float = 20.0):
    """(depth [H, W] float32, strictly positive and finite; rgb [H, W, 3] uint8)"""
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    depth = (rng.random((H, W)) * span + lo).astype(np.float32)
    if ties:
        depth = (np.round(depth * 4) / 4).astype(np.float32)
    return depth, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def median5(d: np.ndarray, border: str = "edge") -> np.ndarray:
    p = np.pad(d, 2, mode=border)
    win = sliding_window_view(p, (5, 5)).reshape(d.shape + (25,))
    return np.partition(win, 12, axis=-1)[..., 12]


def _unflip(d: np.ndarray, mn, mx, fma: bool) -> np.ndarray:
    t = (d - mn) / (mx - mn)
    t = np.float32(1.0) - t
    if fma:                     # the product of two float32 is exact in float64: one rounding of product + mn (up to a double rounding)
        return (np.float64(mn) + t.astype(np.float64) * np.float64(mx - mn)).astype(np.float32)
    return mn + t * (mx - mn)


def cloud_restated(depth, rgb, flip, u0, v0, fx=1000.0, fy=1000.0, bug: str | None = None) -> np.ndarray:
    """depth [H, W] or [n, H, W] float32, rgb [..., H, W, 3] uint8 -> VERTEX records of depth's shape"""
    assert bug is None or bug in BUGS, bug
    depth = np.ascontiguousarray(depth, np.float32)
    rgb = np.ascontiguousarray(rgb, np.uint8)
    assert rgb.shape == depth.shape + (3,)
    if depth.ndim == 3:
        return np.stack([cloud_restated(d, c, flip, u0, v0, fx, fy, bug) for d, c in zip(depth, rgb)])
    H, W = depth.shape
    border = {"border_zero": "constant", "border_reflect": "symmetric"}.get(bug, "edge")
    mn, mx = depth.min(), depth.max()
    if bug == "median_first":
        m = median5(depth, border)
        if flip:
            m = _unflip(m, m.min(), m.max(), False)
    else:
        m = median5(_unflip(depth, mn, mx, bug == "fma") if flip else depth, border)
    u0, v0, fx, fy = np.float32(u0), np.float32(v0), np.float32(fx), np.float32(fy)
    u = np.arange(W).astype(np.float32) - u0
    v = np.arange(H).astype(np.float32) - v0
    x = u * (np.float32(1.0) / fx) if bug == "rcp" else u / fx
    y = v / fy
    out = np.empty((H, W), VERTEX)
    out["x"] = m * x[None, :]
    out["y"] = np.float32(0.0) - m * y[:, None] if bug == "pos_zero" else m * (-y)[:, None]
    out["z"] = m * np.float32(-1.0)
    out["red"], out["green"], out["blue"] = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return out


def raw(vertices: np.ndarray) -> np.ndarray:
    """the records' bytes: uint8 [..., 15]"""
    v = np.ascontiguousarray(vertices)
    return v.view(np.uint8).reshape(v.shape + (VERTEX.itemsize,))
