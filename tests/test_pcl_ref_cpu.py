"""CPU: the point-cloud restatement (tests/pcl_ref.py) the GPU test compares pb_depth_point_cloud with, and the PLY writer.

cv2.medianBlur and plyfile are pinned by restatement only (neither package is installed here): the median is held to scipy's, the header to
the bytes plyfile writes for save_point_cloud's dtype as the PLY format states them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bands"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcl_ref as R  # noqa: E402
from common.io import write_ply  # noqa: E402


def test_median_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for H, W, ties in [(1, 1, False), (2, 3, False), (4, 4, False), (5, 7, False), (18, 70, True), (67, 131, False)]:
        d, _ = R.make_case(H, W, ties)
        want = ndi.median_filter(d, size=5, mode="nearest")
        got = R.median5(d)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (H, W)
    d, _ = R.make_case(18, 70, True)
    assert len(np.unique(d)) < d.size // 4          # the quantised case does hold ties


def gpu_cases():
    """(depth, rgb, flip, u0, v0, fx, fy) of tests/test_gpu_point_cloud.py's single-frame and intrinsics cases"""
    for H, W, ties in R.SHAPES.values():
        d, c = R.make_case(H, W, ties)
        for flip in (0, 1):
            yield d, c, flip, W / 2, H / 2, 1000.0, 1000.0
    d, c = R.make_case(1, 1)
    yield d, c, 0, 0.5, 0.5, 1000.0, 1000.0
    d, c = R.make_case(6, 9)
    for k in R.INTRINSICS:
        yield (d, c, 1) + k


@pytest.mark.parametrize("bug", R.BUGS)
def test_cases_see_each_planted_bug(bug):
    seen = 0
    for d, c, flip, u0, v0, fx, fy in gpu_cases():
        good = R.cloud_restated(d, c, flip, u0, v0, fx, fy)
        seen += not np.array_equal(R.raw(good), R.raw(R.cloud_restated(d, c, flip, u0, v0, fx, fy, bug=bug)))
    assert seen, "no case of the GPU test distinguishes bug=%r" % bug


def test_restatement_properties():
    d, c = R.make_case(6, 9)
    v = R.cloud_restated(d, c, 0, 4.5, 3.0, 1000.0, 1000.0)
    assert v.dtype.itemsize == 15 and v.shape == (6, 9)
    assert R.raw(v)[3, :, 4:8].tolist() == [[0x00, 0x00, 0x00, 0x80]] * 9          # y of the centre row is -0.0
    assert np.array_equal(v["z"], -R.median5(d)) and np.array_equal(v["blue"], c[..., 2])
    # un-flip: min and max change places, so the flipped cloud of a two-valued map is the unflipped cloud of the swapped map
    two = np.where(d > 10, np.float32(12), np.float32(3)).astype(np.float32)
    swapped = np.where(d > 10, np.float32(3), np.float32(12)).astype(np.float32)
    assert np.array_equal(R.raw(R.cloud_restated(two, c, 1, 4.5, 3.0)), R.raw(R.cloud_restated(swapped, c, 0, 4.5, 3.0)))
    # a batch is its frames
    d3 = np.stack([d, d * 2 + 1, d[::-1]])
    c3 = np.stack([c, c[::-1], c])
    b = R.cloud_restated(d3, c3, 1, 4.5, 3.0)
    assert all(np.array_equal(R.raw(b[i]), R.raw(R.cloud_restated(d3[i], c3[i], 1, 4.5, 3.0))) for i in range(3))


def test_write_ply_bytes(tmp_path):
    d, c = R.make_case(5, 7)
    v = R.cloud_restated(d, c, 1, 3.5, 2.5)
    path = str(tmp_path / "cloud.ply")
    write_ply(path, v)
    blob = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 35\nproperty float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert blob[:len(header)] == header
    assert len(blob) == len(header) + 15 * 35
    back = np.frombuffer(blob[len(header):], R.VERTEX).reshape(5, 7)
    assert np.array_equal(R.raw(back), R.raw(v))
