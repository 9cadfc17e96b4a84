"""CPU: the float64 restatement of the rgba band's hue decode / heat encode (tests/rgbd_ref.py) that the GPU test compares pb_rgbd_depth with,
against the reference's own bytes (tests/golden/rgbd_hue.npz, written by tools/make_rgbd_golden.py from the reference's rgb_to_hsv /
heat_to_rgb), and pb_rgbd_boxes - which needs no GPU - against the reference's slicing."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rgbd_ref as R  # noqa: E402


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgbd_hue.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def true_table():
    """the restatement's full table, computed once: (rgb uint8 [2^24, 3], heat float32 [2^24])"""
    rgb, heat = np.empty((1 << 24, 3), np.uint8), np.empty(1 << 24, np.float32)
    for lo, d, o in R.table():
        rgb[lo:lo + len(o)], heat[lo:lo + len(d)] = o, d
    rgb.setflags(write=False)
    heat.setflags(write=False)
    return rgb, heat


def test_sample_equals_the_reference():
    g = golden()
    assert np.array_equal(g["colours"], R.sample_colours()) and len(g["colours"]) == 256 + 1536 + 4096
    heat, rgb = R.hue_heat(g["colours"])
    assert heat.dtype == np.float64 and g["heat"].dtype == np.float64
    assert np.array_equal(rgb, g["rgb"])
    assert np.array_equal(heat, g["heat"])                       # float64, exactly
    assert (heat[:256] == 0).all()                               # greys: hue 0, no NaN
    assert heat.min() == 0.0 and heat.max() <= 1.0


def test_every_colour_hash_equals_the_reference():
    import hashlib
    rgb, heat = true_table()
    assert hashlib.sha256(rgb.tobytes()).hexdigest() == str(golden()["sha256"])
    assert np.isfinite(heat).all()


@pytest.mark.parametrize("fault", list(R.FAULTS))
def test_planted_fault_shows_on_the_full_table(fault):
    """each mistake changes the table the GPU test walks through, on exactly as many colours as it does in the reference's arithmetic"""
    rgb, heat = true_table()
    n_bytes = n_heat = 0
    for lo, d, o in R.table(fault):
        n_bytes += int((o != rgb[lo:lo + len(o)]).any(axis=-1).sum())
        n_heat += int((d.astype(np.float32) != heat[lo:lo + len(d)]).sum())
    print("%s: %d colours change a byte, %d a float32 heat value" % (fault, n_bytes, n_heat))
    assert n_bytes > 0 or n_heat > 0
    assert n_bytes == R.FAULTS[fault]


def reference_slices(H, W, side):
    """the reference's crops (bands/rgba.py:29-40) as [x, y, width, height] and its slice bounds (:58-59), restated literally"""
    width, height = W, H
    rgb_crop, depth_crop = {"left": ([width / 2, 0, width / 2, height], [0, 0, width / 2, height]),
                            "right": ([0, 0, width / 2, height], [width / 2, 0, width / 2, height]),
                            "top": ([0, height / 2, width, height / 2], [0, 0, width, height / 2]),
                            "bottom": ([0, 0, width, height / 2], [0, height / 2, width, height / 2])}[side]
    return [(slice(int(c[1]), int(c[1] + c[3])), slice(int(c[0]), int(c[0] + c[2]))) for c in (rgb_crop, depth_crop)]


SIZES = [(7, 5), (8, 5), (2, 1), (1, 2)]


def has_halves(H, W, side):
    return (W if side in ("left", "right") else H) >= 2


@pytest.mark.parametrize("side", R.SIDES)
@pytest.mark.parametrize("H,W", SIZES)
def test_boxes_equal_the_reference_slicing(H, W, side):
    img = np.arange(H * W).reshape(H, W)
    if not has_halves(H, W, side):
        with pytest.raises(ValueError):
            R.boxes(H, W, side)
        return
    rb, db = R.boxes(H, W, side)
    for box, sl in zip((rb, db), reference_slices(H, W, side)):
        assert np.array_equal(img[box[0]:box[1], box[2]:box[3]], img[sl]), (box, sl)
        assert box[1] > box[0] and box[3] > box[2]
    assert R.boxes(H, W, R.SIDES.index(side)) == (rb, db)


def test_boxes_reject_bad_sides():
    for bad in ("middle", 4, -1, None):
        with pytest.raises(ValueError):
            R.boxes(4, 4, bad)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from prisma_amd import _lib
    entry.build()
    return _lib.load()


@pytest.mark.parametrize("side", range(4))
@pytest.mark.parametrize("H,W", SIZES + [(1080, 1920), (37, 150)])
def test_pb_rgbd_boxes(lib, H, W, side):
    rb, db = (C.c_int * 4)(), (C.c_int * 4)()
    rc = lib.pb_rgbd_boxes(H, W, side, rb, db)
    if not has_halves(H, W, R.SIDES[side]):
        assert rc == -1 and b"half" in lib.pb_last_error()
        return
    assert rc == 0
    assert (tuple(rb), tuple(db)) == R.boxes(H, W, side)


def test_pb_rgbd_boxes_bad_arguments(lib):
    rb, db = (C.c_int * 4)(), (C.c_int * 4)()
    assert lib.pb_rgbd_boxes(4, 4, 4, rb, db) == -1 and b"side" in lib.pb_last_error()
    assert lib.pb_rgbd_boxes(4, 4, -1, rb, db) == -1
    assert lib.pb_rgbd_boxes(0, 4, 0, rb, db) == -1
    assert lib.pb_rgbd_boxes(4, 4, 0, None, db) == -1
    from prisma_amd import engine
    assert engine.rgbd_boxes(5, 7, "left") == R.boxes(5, 7, "left") == ((0, 5, 3, 7), (0, 5, 0, 3))
    with pytest.raises(ValueError):
        engine.rgbd_boxes(5, 7, "middle")
