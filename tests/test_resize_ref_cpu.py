"""CPU: the restatement of the bilinear resize (tests/resize_ref.py) is what include/prisma_bands.h says - identity, constants, a case worked
by hand, every weight - its deliberate bugs are all visible on the shapes the GPU tests use, the host side (bands/common/resize.py) is byte
equal to it, and Pillow's bilinear pins its geometry on enlargements."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_ref as R  # noqa: E402

# (sh, sw, H, W) of tests/test_gpu_resize.py
GPU_SHAPES = [(132, 192, 176, 256), (45, 77, 60, 103), (1, 1, 5, 7), (2, 2, 512, 512), (60, 103, 45, 77), (16, 32, 16, 32), (9, 20, 7, 32),
              (6, 804, 7, 1072), (40, 1300, 20, 656), (4, 2100, 4, 528)]
# enlargements only: Pillow widens its filter on a shrink
PIL_PAIRS = [(810, 1440, 1080, 1920), (132, 192, 176, 256), (45, 77, 60, 103), (7, 5, 10, 7), (90, 150, 120, 200), (13, 21, 17, 28)]
CHECKER = np.array([[0, 255], [255, 0]], np.uint8)[..., None].repeat(3, axis=-1)


def frames(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (5, 7), (45, 77), (16, 64)])
def test_equal_size_is_identity(h, w):
    rgb = frames((2, h, w, 3), 1)
    assert np.array_equal(R.resize(rgb, h, w), rgb)
    assert np.array_equal(R.resize_i420(rgb, h, w), R.yuv_ref.rgb_to_i420(rgb))


@pytest.mark.parametrize("sh,sw,H,W", GPU_SHAPES)
def test_constant_frame_stays_constant(sh, sw, H, W):
    for v in (0, 1, 77, 254, 255):
        out = R.resize(np.full((sh, sw, 3), v, np.uint8), H, W)
        assert out.shape == (H, W, 3) and (out == v).all()


def test_one_by_two_to_one_by_four_by_hand():
    # n_in 2, n_out 4: num = -2, 2, 6, 10 over 8 -> i0 = -1, 0, 0, 1 with r = 6, 2, 6, 2 -> w = 192, 64, 192, 64; the outer taps clamp to one
    # sample.  x = 1: (256 (192 p0 + 64 p1) + 32768) >> 16, x = 2: (256 (64 p0 + 192 p1) + 32768) >> 16
    assert R.axis(2, 4) == ([0, 0, 0, 1], [0, 1, 1, 1], [192, 64, 192, 64])
    assert R.axis(1, 1) == ([0], [0], [0])
    src = np.array([[[0, 10, 255], [255, 200, 0]]], np.uint8)
    want = np.array([[[0, 10, 255], [64, 58, 191], [191, 153, 64], [255, 200, 0]]], np.uint8)
    assert np.array_equal(R.resize(src, 1, 4), want)


def test_weight_sweep_reaches_every_weight_and_is_monotone():
    a, b, w = R.axis(2, 512)
    # between the two samples every weight 1 .. 256; outside them both taps are the same sample: the pure taps, weights 0 and 256 in effect
    eff = {(0 if t0 == 0 else 256) if t0 == t1 else wt for t0, t1, wt in zip(a, b, w)}
    assert eff == set(range(257))
    out = R.resize(CHECKER, 512, 512)
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
    g = out[..., 0].astype(int)
    assert np.array_equal(g, g.T)                               # both axes carry the same weights
    assert g[0, 0] == 0 and g[0, -1] == 255 and g[-1, 0] == 255 and g[-1, -1] == 0
    assert (np.diff(g[0]) >= 0).all() and (np.diff(g[-1]) <= 0).all() and (np.diff(g[:, 0]) >= 0).all() and (np.diff(g[:, -1]) <= 0).all()
    assert set(np.unique(g[0])) == set(range(256))              # a ramp over the whole byte range
    # along every row the value moves one way only: the weights are monotone between the taps
    d = np.diff(g, axis=1)
    assert ((d >= 0).all(axis=1) | (d <= 0).all(axis=1)).all()


@pytest.mark.parametrize("bug", R.BUGS)
def test_every_bug_shows_on_a_gpu_shape(bug):
    fn = R.resize_i420 if bug == "chroma_first" else R.resize
    hit = []
    for sh, sw, H, W in GPU_SHAPES:
        src = CHECKER if (sh, sw) == (2, 2) else frames((sh, sw, 3), 5)
        if not np.array_equal(fn(src, H, W), fn(src, H, W, bug=bug)):
            hit.append((sh, sw, H, W))
    assert hit, bug
    if bug != "chroma_first":                                   # the I420 form carries the same bugs
        assert any(not np.array_equal(R.resize_i420(frames((sh, sw, 3), 5), H, W), R.resize_i420(frames((sh, sw, 3), 5), H, W, bug=bug))
                   for sh, sw, H, W in hit if (sh, sw) != (2, 2)), bug


@pytest.mark.parametrize("sh,sw,H,W", GPU_SHAPES + [(7, 5, 10, 7), (9, 4, 3, 11)])
def test_host_resize_is_byte_equal(sh, sw, H, W):
    from bands.common.resize import resize_rgb
    src = CHECKER if (sh, sw) == (2, 2) else frames((sh, sw, 3), 9)
    got = resize_rgb(src, H, W)
    assert got.dtype == np.uint8 and np.array_equal(got, R.resize(src, H, W))


@pytest.mark.parametrize("sh,sw,H,W", PIL_PAIRS)
def test_pillow_bilinear_pins_the_geometry(sh, sw, H, W):
    from PIL import Image
    src = np.random.default_rng(0).integers(0, 256, (sh, sw, 3)).astype(np.uint8)
    pil = np.asarray(Image.fromarray(src).resize((W, H), Image.BILINEAR))
    worst = int(np.abs(pil.astype(int) - R.resize(src, H, W).astype(int)).max())
    print("pillow %d x %d -> %d x %d: max |difference| %d" % (sh, sw, H, W, worst))
    assert worst <= 1
