"""GPU: pb_i420_to_rgb / pb_rgb_to_i420 and their _dev twins (prisma_amd/csrc/yuv.hip) against the integer restatement tests/yuv_ref.py, byte
for byte: every size at which a kernel takes another path (one block, odd edges, the 16-byte path and its odd last block row, the byte path
over several workgroups), random and saturating data, every input value of either direction, and guard bytes behind every output."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import yuv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3
# 16 x 64 and 3 x 32: the 16-byte path (W % 16 == 0), the second with a last block row one pixel high; 17 x 67: the byte path with both odd edges,
# more than one workgroup; 2 x 4 and below: fewer blocks than a wavefront
SIZES = [(1, 1), (2, 2), (2, 4), (3, 5), (16, 64), (17, 67), (3, 32)]
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    from prisma_amd import engine
    o = engine.Ops()
    yield o
    o.close()


@functools.lru_cache(maxsize=None)
def case(H, W, kind):
    """(rgb frames, their restated I420, I420 frames, their restated RGB): random bytes, or only 0 and 255 so that every clip8 saturates"""
    rng = np.random.default_rng(1000 * H + W + (0 if kind == "random" else 7))
    draw = (lambda shape: rng.integers(0, 256, shape, dtype=np.uint8)) if kind == "random" else (lambda shape: rng.integers(0, 2, shape, dtype=np.uint8) * 255)
    rgb, yuv = draw((N, H, W, 3)), draw((N, R.i420_bytes(H, W)))
    out = (rgb, R.rgb_to_i420(rgb), yuv, R.i420_to_rgb(yuv, H, W))
    for a in out:
        a.setflags(write=False)
    return out


def same(what, got, want):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d bytes differ, first at %s: kernel %d, restatement %d" % (what, len(bad), want.size, i, got[i], want[i]))


def guarded(nbytes):
    buf = np.full(nbytes + GUARD, 0xFF, np.uint8)
    return buf, buf[:nbytes]


def on_device(ops, fn, src, out_bytes, *dims, skew=0):
    """one _dev call on device buffers: the output preset to 0xFF with GUARD bytes behind it -> (output bytes, guard bytes).  skew = 1: both
    arrays start one byte into their allocations, which takes a W % 16 == 0 frame off the 16-byte path (the byte in front is checked too)"""
    d_in, d_out = ops.dev_alloc(src.nbytes + skew), ops.dev_alloc(skew + out_bytes + GUARD)
    try:
        ops.h2d(d_in + skew, src)
        ops.h2d(d_out, np.full(skew + out_bytes + GUARD, 0xFF, np.uint8))
        fn(d_in + skew, *dims, d_out + skew)
        ops.sync()
        got = np.empty(skew + out_bytes + GUARD, np.uint8)
        ops.d2h(got, d_out)
    finally:
        ops.dev_free(d_in)
        ops.dev_free(d_out)
    assert (got[:skew] == 0xFF).all()
    return got[skew:skew + out_bytes], got[skew + out_bytes:]


@pytest.mark.parametrize("kind", ["random", "saturating"])
@pytest.mark.parametrize("H,W", SIZES)
def test_both_directions_host_and_dev(ops, H, W, kind):
    from prisma_amd import engine
    rgb, want_yuv, yuv, want_rgb = case(H, W, kind)
    fb = R.i420_bytes(H, W)
    assert engine.i420_bytes(H, W) == fb
    # host pointers, into the caller's arrays: nothing behind them is touched
    buf, out = guarded(N * fb)
    ops.rgb_to_i420(rgb, out=out.reshape(N, fb))
    same("rgb_to_i420 %dx%d %s" % (H, W, kind), out.reshape(N, fb), want_yuv)
    assert (buf[N * fb:] == 0xFF).all()
    buf, out = guarded(N * H * W * 3)
    ops.i420_to_rgb(yuv, H, W, out=out.reshape(N, H, W, 3))
    same("i420_to_rgb %dx%d %s" % (H, W, kind), out.reshape(N, H, W, 3), want_rgb)
    assert (buf[N * H * W * 3:] == 0xFF).all()
    # one frame without the batch axis
    same("one frame", ops.rgb_to_i420(rgb[1]), want_yuv[1])
    same("one frame", ops.i420_to_rgb(yuv[1], H, W), want_rgb[1])
    # device pointers
    got, guard = on_device(ops, ops.rgb_to_i420_dev, rgb, N * fb, N, H, W)
    same("rgb_to_i420_dev %dx%d %s" % (H, W, kind), got.reshape(N, fb), want_yuv)
    assert (guard == 0xFF).all()
    got, guard = on_device(ops, ops.i420_to_rgb_dev, yuv, N * H * W * 3, N, H, W)
    same("i420_to_rgb_dev %dx%d %s" % (H, W, kind), got.reshape(N, H, W, 3), want_rgb)
    assert (guard == 0xFF).all()


def test_chunked_host_call_and_any_context(ops):
    """more frames than a chunk ("host_chunk" 2: chunks of 2, 2, 1 through both device slots), and a misaligned device pointer on the 16-byte size"""
    H, W = 16, 64
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    ops.set_option("host_chunk", 2)
    try:
        yuv = ops.rgb_to_i420(rgb)
        same("chunked rgb_to_i420", yuv, R.rgb_to_i420(rgb))
        same("chunked i420_to_rgb", ops.i420_to_rgb(yuv, H, W), R.i420_to_rgb(yuv, H, W))
    finally:
        ops.set_option("host_chunk", 0)
    fb = R.i420_bytes(H, W)
    d_in, d_out = ops.dev_alloc(rgb.nbytes + 1), ops.dev_alloc(5 * fb + 1 + GUARD)
    try:
        ops.h2d(d_in + 1, rgb)
        ops.h2d(d_out, np.full(5 * fb + 1 + GUARD, 0xFF, np.uint8))
        ops.rgb_to_i420_dev(d_in + 1, 5, H, W, d_out + 1)           # not 16-byte aligned: the byte path, same bytes
        ops.sync()
        got = np.empty(5 * fb + 1 + GUARD, np.uint8)
        ops.d2h(got, d_out)
    finally:
        ops.dev_free(d_in)
        ops.dev_free(d_out)
    same("misaligned rgb_to_i420_dev", got[1:1 + 5 * fb].reshape(5, fb), R.rgb_to_i420(rgb))
    assert got[0] == 0xFF and (got[1 + 5 * fb:] == 0xFF).all()
    for bad in (lambda: ops.i420_to_rgb_dev(0, 1, H, W, 0), lambda: ops.set_option("frames_i420", 2)):        # refused before any launch
        with pytest.raises(RuntimeError):
            bad()


def test_every_colour_to_i420(ops):
    """all 2^24 colours, each a constant 2 x 2 block of one 8192 x 8192 frame (16-byte path): the block's mean is the colour itself, so Y (four
    times) and (Cb, Cr) are the restatement's values of the colour"""
    c = np.arange(1 << 24, dtype=np.uint32)
    colours = np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    frame = np.repeat(np.repeat(colours, 2, axis=0), 2, axis=1)
    H = W = 8192
    v = colours.reshape(-1, 3).astype(np.int64)
    y = R.luma(v[:, 0], v[:, 1], v[:, 2]).astype(np.uint8).reshape(4096, 4096)
    cb, cr = R.chroma(v[:, 0], v[:, 1], v[:, 2])
    for skew, path in ((0, "16-byte path"), (1, "byte path")):
        got, guard = on_device(ops, ops.rgb_to_i420_dev, frame, R.i420_bytes(H, W), 1, H, W, skew=skew)
        assert (guard == 0xFF).all()
        gy, gcb, gcr = R.planes(got, H, W)
        for dy in (0, 1):
            for dx in (0, 1):
                same("Y of every colour, " + path, np.ascontiguousarray(gy[dy::2, dx::2]), y)
        same("Cb of every colour, " + path, gcb, cb.astype(np.uint8).reshape(4096, 4096))
        same("Cr of every colour, " + path, gcr, cr.astype(np.uint8).reshape(4096, 4096))


def test_every_triple_to_rgb(ops):
    """all 2^24 (Y, Cb, Cr): one 4096 x 4096 frame whose block b carries (Cb, Cr) = the low 16 bits of b and the four luma values 4 (b >> 16) + 0 .. 3"""
    H = W = 4096
    b = np.arange(1 << 22, dtype=np.uint32).reshape(2048, 2048)
    cb, cr = (b & 255).astype(np.uint8), ((b >> 8) & 255).astype(np.uint8)
    y = np.empty((H, W), np.uint8)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        y[dy::2, dx::2] = 4 * (b >> 16) + k
    yuv = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    triples = np.stack([y.reshape(-1), np.repeat(np.repeat(cb, 2, 0), 2, 1).reshape(-1), np.repeat(np.repeat(cr, 2, 0), 2, 1).reshape(-1)], axis=-1)
    assert len(np.unique(triples.astype(np.uint32) @ np.array([1 << 16, 1 << 8, 1], np.uint32))) == 1 << 24          # every triple, once
    t = triples.astype(np.int64)
    want = np.stack(R.colour(t[:, 0], t[:, 1], t[:, 2]), axis=-1).reshape(H, W, 3)
    for skew, path in ((0, "16-byte path"), (1, "byte path")):
        got, guard = on_device(ops, ops.i420_to_rgb_dev, yuv, H * W * 3, 1, H, W, skew=skew)
        assert (guard == 0xFF).all()
        same("RGB of every (Y, Cb, Cr), " + path, got.reshape(H, W, 3), want)
    same("restatement of the whole frame", want, R.i420_to_rgb(yuv, H, W))
