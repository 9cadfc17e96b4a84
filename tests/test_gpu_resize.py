"""GPU: pb_rgb_resize / pb_rgb_resize_dev (prisma_amd/csrc/resize.hip), RGB and straight-to-I420, against the integer restatement
tests/resize_ref.py, byte for byte: the 16-byte path and the same frames off it (device pointers one byte into their allocations), odd sizes
with a one-pixel last block row and column, a single source pixel, every weight, a shrink, equal sizes, several frames of their own content,
and guard bytes round every device output."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_ref as R  # noqa: E402
import yuv_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3
GUARD = 64
# (sh, sw, H, W): 132 x 192 -> 176 x 256 the flow bands' --scale 0.75 on the suite's clip, W % 16 == 0: the 16-byte path; 45 x 77 -> 60 x 103 odd
# everywhere, H = 60 rows of 52 blocks with a one-pixel last block column, and the reverse a shrink with a one-pixel last block row as well;
# 1 x 1: every tap clamped; 2 x 2 -> 512 x 512: every weight on both axes, on the 16-byte path; 16 x 32 and 5 x 7 onto themselves: a byte copy
# 9 x 20 -> 7 x 32: the 16-byte path with a last block row one pixel high.  The 16-byte path works in tiles of 512 pixels whose source columns sit
# in LDS: 6 x 804 -> 7 x 1072 has three tiles in a row, the last of 48 pixels; 40 x 1300 -> 20 x 656 is a shrink whose tiles just fit
# (1015 of 1024 source pixels); the tiles of 4 x 2100 -> 4 x 528 do not fit, which sends an aligned multiple of 16 down the byte path
SHAPES = [(132, 192, 176, 256), (45, 77, 60, 103), (1, 1, 5, 7), (2, 2, 512, 512), (60, 103, 45, 77), (16, 32, 16, 32), (5, 7, 5, 7), (9, 20, 7, 32),
          (6, 804, 7, 1072), (40, 1300, 20, 656), (4, 2100, 4, 528)]


@pytest.fixture(scope="module")
def ops():
    from prisma_amd import engine
    o = engine.Ops()
    yield o
    o.close()


@functools.lru_cache(maxsize=None)
def case(sh, sw, H, W):
    """(N source frames of differing content, their restated resize, its restated I420): computed once, read-only"""
    rng = np.random.default_rng(1000 * sh + sw)
    src = rng.integers(0, 256, (N, sh, sw, 3), dtype=np.uint8)
    if (sh, sw) == (2, 2):
        src[0] = np.array([[0, 255], [255, 0]], np.uint8)[..., None]           # the weight sweep
    want = R.resize(src, H, W)
    out = (src, want, yuv_ref.rgb_to_i420(want))
    assert np.array_equal(out[2], R.resize_i420(src, H, W))
    assert len({f.tobytes() for f in want}) == N                              # a wrong frame stride cannot hide
    for a in out:
        a.setflags(write=False)
    return out


def same(what, got, want):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d bytes differ, first at %s: kernel %d, restatement %d" % (what, len(bad), want.size, i, got[i], want[i]))


def on_device(ops, src, dims, out_bytes, i420, skew):
    """one _dev call on device buffers: the output preset to 0xFF with `skew` bytes in front of it and GUARD bytes behind -> the output bytes.
    skew = 1: both arrays start one byte into their allocations, which takes a W % 16 == 0 frame off the 16-byte path"""
    d_in, d_out = ops.dev_alloc(src.nbytes + skew), ops.dev_alloc(skew + out_bytes + GUARD)
    try:
        ops.h2d(d_in + skew, src)
        ops.h2d(d_out, np.full(skew + out_bytes + GUARD, 0xFF, np.uint8))
        ops.rgb_resize_dev(d_in + skew, *dims, d_out + skew, i420=i420)
        ops.sync()
        got = np.empty(skew + out_bytes + GUARD, np.uint8)
        ops.d2h(got, d_out)
    finally:
        ops.dev_free(d_in)
        ops.dev_free(d_out)
    assert (got[:skew] == 0xFF).all() and (got[skew + out_bytes:] == 0xFF).all(), "a write outside the output"
    return got[skew:skew + out_bytes]


@pytest.mark.parametrize("i420", [False, True], ids=["rgb", "i420"])
@pytest.mark.parametrize("sh,sw,H,W", SHAPES)
def test_host_and_dev_forms_against_the_restatement(ops, sh, sw, H, W, i420):
    src, want_rgb, want_yuv = case(sh, sw, H, W)
    want = want_yuv if i420 else want_rgb
    got = ops.rgb_resize(src, H, W, i420=i420)
    same("host pointers", got, want)
    if (sh, sw) == (H, W) and not i420:
        assert got.tobytes() == src.tobytes()                                 # an equal-size call is a byte copy
    for skew in (0, 1):                                                       # the 16-byte path where the width allows it, and the byte path
        dev = on_device(ops, src, (N, sh, sw, H, W), want.nbytes, i420, skew)
        same("device pointers, skew %d" % skew, dev.reshape(want.shape), want)
        assert dev.tobytes() == got.tobytes()                                 # the two forms agree
    same("one frame", ops.rgb_resize(src[1], H, W, i420=i420), want[1])


def test_caller_owned_output_and_chunks(ops):
    """more frames than a host chunk (8), into the caller's array"""
    sh, sw, H, W = 9, 20, 7, 32
    src = np.random.default_rng(4).integers(0, 256, (19, sh, sw, 3), dtype=np.uint8)
    out = np.zeros((19, yuv_ref.i420_bytes(H, W)), np.uint8)
    assert ops.rgb_resize(src, H, W, i420=True, out=out) is out
    same("19 frames", out, R.resize_i420(src, H, W))


def test_refused_sizes(ops):
    from prisma_amd import _lib
    with pytest.raises(_lib.PrismaBandsError, match="16384"):              # the tap arithmetic would leave int32
        ops.rgb_resize(np.zeros((1, 2, 3), np.uint8), 2, 16385)
    ops.rgb_resize(np.zeros((1, 2, 3), np.uint8), 2, 3)                       # the ctx still works
