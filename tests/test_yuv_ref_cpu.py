"""tests/yuv_ref.py, the restatement that pins the I420 <-> RGB kernels (prisma_amd/csrc/yuv.hip) and the host side of the .y4m files
(bands/common/yuv.py): known colours, plane shapes and clamped block means at odd sizes against a plain double loop, the grey round trip."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bands"))
import yuv_ref as R  # noqa: E402
from common import yuv as host  # noqa: E402

SIZES = [(1, 1), (3, 5), (5, 2), (2, 2), (4, 6), (17, 67)]


def _loop_rgb_to_i420(rgb):
    """the formulas with Python integers, pixel by pixel and block by block"""
    H, W = rgb.shape[:2]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    px = [[tuple(int(v) for v in rgb[y, x]) for x in range(W)] for y in range(H)]
    y_plane = [((66 * r + 129 * g + 25 * b + 128) >> 8) + 16 for row in px for r, g, b in row]
    cb_plane, cr_plane = [], []
    for by in range(ch):
        for bx in range(cw):
            four = [px[min(2 * by + dy, H - 1)][min(2 * bx + dx, W - 1)] for dy in (0, 1) for dx in (0, 1)]
            r, g, b = [(sum(p[k] for p in four) + 2) >> 2 for k in range(3)]
            cb_plane.append(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128)
            cr_plane.append(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128)
    return np.array(y_plane + cb_plane + cr_plane, np.uint8)


def _loop_i420_to_rgb(yuv, H, W):
    ch, cw = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((H, W, 3), np.uint8)
    clip8 = lambda v: max(0, min(255, v))      # noqa: E731
    for y in range(H):
        for x in range(W):
            c = int(yuv[y * W + x]) - 16
            d = int(yuv[H * W + (y >> 1) * cw + (x >> 1)]) - 128
            e = int(yuv[H * W + ch * cw + (y >> 1) * cw + (x >> 1)]) - 128
            out[y, x] = (clip8((298 * c + 409 * e + 128) >> 8), clip8((298 * c - 100 * d - 208 * e + 128) >> 8), clip8((298 * c + 516 * d + 128) >> 8))
    return out


def test_known_colours():
    for rgb, yuv in (((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((255, 0, 0), (82, 90, 240))):
        frame = np.broadcast_to(np.array(rgb, np.uint8), (2, 2, 3))
        out = R.rgb_to_i420(frame)
        assert out.tolist() == [yuv[0]] * 4 + [yuv[1], yuv[2]], (rgb, out)
    # and back: the three legal extremes decode to themselves
    for yuv, rgb in (((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255))):
        frame = np.array([yuv[0]] * 4 + [yuv[1], yuv[2]], np.uint8)
        assert (R.i420_to_rgb(frame, 2, 2) == np.array(rgb, np.uint8)).all()
    # out-of-range codes saturate instead of wrapping
    assert (R.i420_to_rgb(np.array([255] * 4 + [255, 255], np.uint8), 2, 2) == [255, 125, 255]).all()
    assert (R.i420_to_rgb(np.array([0] * 4 + [0, 0], np.uint8), 2, 2) == [0, 135, 0]).all()


@pytest.mark.parametrize("H,W", SIZES)
def test_shapes_and_clamped_blocks_against_a_double_loop(H, W):
    rng = np.random.default_rng(H * 100 + W)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yuv = R.rgb_to_i420(rgb)
    ch, cw = R.chroma_size(H, W)
    assert (ch, cw) == (-(-H // 2), -(-W // 2)) and yuv.shape == (R.i420_bytes(H, W),) == (H * W + 2 * ch * cw,)
    y, cb, cr = R.planes(yuv, H, W)
    assert y.shape == (H, W) and cb.shape == cr.shape == (ch, cw)
    assert (yuv == _loop_rgb_to_i420(rgb)).all()
    any_yuv = rng.integers(0, 256, R.i420_bytes(H, W), dtype=np.uint8)
    back = R.i420_to_rgb(any_yuv, H, W)
    assert back.shape == (H, W, 3) and (back == _loop_i420_to_rgb(any_yuv, H, W)).all()
    # leading axes are batch axes
    both = np.stack([rgb, 255 - rgb])
    assert (R.rgb_to_i420(both) == np.stack([R.rgb_to_i420(rgb), R.rgb_to_i420(255 - rgb)])).all()
    assert (R.i420_to_rgb(R.rgb_to_i420(both), H, W) == np.stack([R.i420_to_rgb(R.rgb_to_i420(f), H, W) for f in both])).all()


def test_grey_ramp_round_trip():
    """A grey v gives Y = ((220 v + 128) >> 8) + 16 and neutral chroma; decoding gives (298 (Y - 16) + 128) >> 8.  220 / 256 x 298 / 256 is
    just above 1, so the round trip is exact wherever the two floors lose less than one code together - which the formulas decide, not this test:
    the expectation below is their composition in Python integers."""
    v = np.arange(256)
    ramp = np.repeat(np.repeat(v.astype(np.uint8)[None, :, None], 2, axis=0), 3, axis=2)      # 2 x 256 x 3
    yuv = R.rgb_to_i420(ramp)
    y, cb, cr = R.planes(yuv, 2, 256)
    assert (cb == 128).all() and (cr == 128).all()
    assert y[0].tolist() == [((220 * int(g) + 128) >> 8) + 16 for g in v]
    back = R.i420_to_rgb(yuv, 2, 256)
    expect = [min(255, max(0, (298 * (((220 * int(g) + 128) >> 8)) + 128) >> 8)) for g in v]
    assert (back[..., 0] == back[..., 1]).all() and (back[..., 1] == back[..., 2]).all() and back[0, :, 0].tolist() == expect
    # 256 greys share the 220 luma codes 16 .. 235, so some neighbours collide; each floor rounds by at most half a step (1 and 298 / 256 codes),
    # so no grey moves by more than one code, and black and white survive
    assert len(set(y[0].tolist())) == 220 and expect[0] == 0 and expect[255] == 255 and max(abs(expect[g] - g) for g in v) == 1


@pytest.mark.parametrize("H,W", SIZES)
def test_host_side_equals_the_restatement(H, W):
    rng = np.random.default_rng(7 * H + W)
    for rgb in (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255):
        assert host.i420_bytes(H, W) == R.i420_bytes(H, W)
        assert (host.rgb_to_i420(rgb) == R.rgb_to_i420(rgb)).all()
    for yuv in (rng.integers(0, 256, R.i420_bytes(H, W), dtype=np.uint8), rng.integers(0, 2, R.i420_bytes(H, W), dtype=np.uint8) * 255):
        assert (host.i420_to_rgb(yuv, H, W) == R.i420_to_rgb(yuv, H, W)).all()
