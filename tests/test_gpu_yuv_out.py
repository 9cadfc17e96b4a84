"""GPU: pb_rgb_to_yuv / pb_rgb_to_yuv_dev (prisma_amd/csrc/yuv_out.hip) and pb_set_out_format against the restatement tests/yuv_out_ref.py, byte
for byte: every layout x depth x range x matrix at every size at which a kernel takes another path (one lane, odd edges with their clamped
chroma blocks, the 16-byte path and its odd last chroma row, the byte path over several workgroups and on a misaligned pointer), every RGB
colour, and guard bytes around every output."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import yuv_fmt_ref as F  # noqa: E402
import yuv_out_ref as O  # noqa: E402
import yuv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3                   # frames per call: a wrong frame stride shows
# 16 x 64 and 3 x 32: the 16-byte path (W % 16 == 0), the second with a last 4:2:0 chroma row one pixel high; 17 x 67: the byte path with both odd
# edges and more than one workgroup; 2 x 4 and below: fewer lanes than a wavefront
SIZES = [(1, 1), (2, 4), (3, 5), (3, 32), (16, 64), (17, 67)]
DEPTHS = (8, 10, 12, 16)
GUARD = 64
I420 = (420, 8, False, "bt601")


@pytest.fixture(scope="module")
def ops():
    from prisma_amd import engine
    o = engine.Ops()
    yield o
    o.close()


def same(what, got, want):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d bytes differ, first at %s: kernel %d, restatement %d" % (what, len(bad), want.size, i, got[i], want[i]))


@functools.lru_cache(maxsize=None)
def frames(H, W, n=N):
    """random RGB frames with the eight corners of the colour cube in the first pixels they fit in (every clamp's extreme)"""
    rgb = np.random.default_rng(1000 * H + W + n).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    corners = np.array(list(itertools.product((0, 255), repeat=3)), np.uint8)
    flat = rgb.reshape(n, -1, 3)
    flat[-1, :min(8, H * W)] = corners[:min(8, H * W)]
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def case(fmt, H, W, n=N):
    want = O.rgb_to_yuv(fmt, frames(H, W, n))
    want.setflags(write=False)
    return frames(H, W, n), want


def on_device(ops, fmt, rgb, skew=0):
    """one _dev call on device buffers: the output preset to 0xA5 with GUARD bytes behind it -> the output bytes.  skew = 1: both arrays start
    one byte into their allocations, which takes a W % 16 == 0 frame off the 16-byte path (the byte in front is checked too)"""
    from prisma_amd import engine
    n, H, W = rgb.shape[:3]
    out_bytes = n * engine.yuv_bytes(fmt, H, W)
    d_in, d_out = ops.dev_alloc(rgb.nbytes + skew), ops.dev_alloc(skew + out_bytes + GUARD)
    try:
        ops.h2d(d_in + skew, rgb)
        ops.h2d(d_out, np.full(skew + out_bytes + GUARD, 0xA5, np.uint8))
        ops.rgb_to_yuv_dev(fmt, d_in + skew, n, H, W, d_out + skew)
        ops.sync()
        got = np.empty(skew + out_bytes + GUARD, np.uint8)
        ops.d2h(got, d_out)
    finally:
        ops.dev_free(d_in)
        ops.dev_free(d_out)
    assert (got[:skew] == 0xA5).all() and (got[skew + out_bytes:] == 0xA5).all(), "bytes outside the output were written"
    return got[skew:skew + out_bytes].reshape(n, -1)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("chroma", F.CHROMAS)
def test_every_format_host_and_dev(ops, chroma, depth, H, W):
    from prisma_amd import engine
    for full, matrix in itertools.product((False, True), F.MATRICES):
        fmt = (chroma, depth, full, matrix)
        rgb, want = case(fmt, H, W)
        what = "%r %dx%d" % (fmt, H, W)
        assert engine.yuv_bytes(fmt, H, W) == want.shape[1]
        # host pointers, into the caller's array: nothing behind it is touched
        buf = np.full(want.size + GUARD, 0xA5, np.uint8)
        ops.rgb_to_yuv(fmt, rgb, out=buf[:want.size].reshape(want.shape))
        same("rgb_to_yuv " + what, buf[:want.size].reshape(want.shape), want)
        assert (buf[want.size:] == 0xA5).all()
        # device pointers, aligned (the 16-byte path where W allows it) and deliberately one byte off (the byte path, the same bytes)
        for skew in ((0, 1) if W % 16 == 0 else (0,)):
            same("rgb_to_yuv_dev skew %d %s" % (skew, what), on_device(ops, fmt, rgb, skew=skew), want)
    same("one frame", ops.rgb_to_yuv(fmt, rgb[1]), want[1])


@functools.lru_cache(maxsize=None)
def every_colour():
    g = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([g & 255, (g >> 8) & 255, g >> 16], axis=-1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    rgb.setflags(write=False)
    return rgb


def restated_in_slabs(fmt, rgb, rows=512):
    """the restatement of one 4:4:4 frame, slab by slab (a pixel stands alone; int64 temporaries of 2^24 pixels are large)"""
    parts = [O.samples(fmt, rgb[s:s + rows]) for s in range(0, rgb.shape[0], rows)]
    return F.pack(fmt, *(np.concatenate([p[i] for p in parts]) for i in range(3)))


@pytest.mark.parametrize("fmt", [(444, 12, True, "bt601"), (444, 8, False, "bt709")], ids=str)
def test_every_colour(ops, fmt):
    rgb = every_colour()
    got = on_device(ops, fmt, rgb)
    same("YUV of every colour, %r" % (fmt,), got[0], restated_in_slabs(fmt, rgb[0]))
    if fmt[1] == 12:        # the lossless choice: read back by the library's own rule, every colour is what went in
        same("round trip of every colour", ops.yuv_to_rgb(fmt, got, 4096, 4096), rgb)


@pytest.mark.parametrize("H,W", [(5, 18), (6, 32)])
def test_i420_format_is_the_existing_kernel(ops, H, W):
    rgb, want = case(I420, H, W)
    same("restatements agree", want, np.stack([R.rgb_to_i420(f) for f in rgb]))
    same("rgb_to_yuv at I420", ops.rgb_to_yuv(I420, rgb), ops.rgb_to_i420(rgb))
    same("rgb_to_yuv at I420 against the restatement", ops.rgb_to_yuv(I420, rgb), want)
    same("rgb_to_yuv_dev at I420", on_device(ops, I420, rgb), want)


@pytest.mark.parametrize("fmt", [(422, 10, True, "bt709"), (400, 16, False, "bt601")], ids=str)
def test_chunked_host_call(ops, fmt):
    """more frames than a chunk ("host_chunk" 2: chunks of 2, 2, 1 through both device slots), from pageable and from page-locked memory"""
    H, W = 16, 64
    rgb, want = case(fmt, H, W, n=5)
    ops.set_option("host_chunk", 2)
    pin_in, pin_out = ops.host_empty(rgb.shape, np.uint8), ops.host_empty(want.shape, np.uint8)
    try:
        same("chunked rgb_to_yuv %r, pageable" % (fmt,), ops.rgb_to_yuv(fmt, rgb), want)
        pin_in[:] = rgb
        pin_out[:] = 0xA5
        assert ops.rgb_to_yuv(fmt, pin_in, out=pin_out) is pin_out
        same("chunked rgb_to_yuv %r, page-locked" % (fmt,), np.array(pin_out), want)
    finally:
        ops.set_option("host_chunk", 0)
        ops.host_free(pin_in)
        ops.host_free(pin_out)


def test_bad_arguments_are_refused_before_any_launch(ops):
    for bad in (lambda: ops.rgb_to_yuv_dev((411, 8, False, "bt601"), 1, 1, 4, 4, 1), lambda: ops.rgb_to_yuv_dev((420, 17, False, "bt601"), 1, 1, 4, 4, 1),
                lambda: ops.rgb_to_yuv_dev((420, 7, False, "bt601"), 1, 1, 4, 4, 1), lambda: ops.rgb_to_yuv_dev((420, 8, False, "bt2020"), 1, 1, 4, 4, 1),
                lambda: ops.rgb_to_yuv_dev(I420, 0, 1, 4, 4, 1), lambda: ops.rgb_to_yuv_dev(I420, 1, 1, 4, 4, 0),
                lambda: ops.rgb_to_yuv_dev(I420, 1, 0, 4, 4, 1), lambda: ops.rgb_to_yuv_dev(I420, 1, 1, 0, 4, 1),
                lambda: ops.rgb_to_yuv_dev(I420, 1, 1, 4, -1, 1)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError):
        ops.rgb_to_yuv((411, 8, False, "bt601"), np.zeros((4, 4, 3), np.uint8))


def test_set_out_format_on_a_band_context():
    """a depth context: the format decides what its rgb result is; a refusal - an unknown format, a submission outstanding - leaves the context
    as it was and working; "rgb_out_i420" still toggles"""
    from prisma_amd import engine, synth
    H, W = 42, 64
    fmt = engine.YuvFormat(444, 12, True, "bt601")
    rgb = frames(H, W, 2)
    net = engine.DepthAnything(synth.depth_anything_weights("vits", seed=1234), "vits", device=0, max_batch=2)
    try:
        plain = net.infer_batch(rgb)
        want = O.rgb_to_yuv(tuple(fmt), plain[1])
        net.rgb_format = fmt
        assert net.rgb_format == fmt and net.rgb_shape(H, W) == (engine.yuv_bytes(fmt, H, W),)
        got = net.infer_batch(rgb)
        same("rgb result in %r" % (fmt,), got[1], want)
        assert got[0].tobytes() == plain[0].tobytes()
        for bad in ((411, 8, False, "bt601"), (420, 7, False, "bt601"), (420, 8, False, "bt2020")):
            with pytest.raises(RuntimeError):
                net.rgb_format = bad
            assert net.rgb_format == fmt
            same("after a refusal", net.infer_batch(rgb)[1], want)
        net.rgb_format = "i420"                                       # pb_set_option "rgb_out_i420", 1
        want420 = np.stack([R.rgb_to_i420(f) for f in plain[1]])
        same("i420", net.infer_batch(rgb)[1], want420)
        net.rgb_format = engine.YuvFormat(*I420)                      # the same through pb_set_out_format
        same("I420 as a format", net.infer_batch(rgb)[1], want420)
        net.rgb_format = "rgb"
        same("rgb again", net.infer_batch(rgb)[1], plain[1])
        # refused while a submission is outstanding
        fin, out, mm = net.host_empty(rgb.shape, np.uint8), net.host_empty(rgb.shape, np.uint8), net.host_empty((2, 2), np.float32)
        try:
            fin[:] = rgb
            net.submit_batch(fin, out_rgb=out, out_min=mm[0], out_max=mm[1])
            with pytest.raises(RuntimeError):
                net.rgb_format = fmt
            net.wait()
            assert net.rgb_format == "rgb" and out.tobytes() == plain[1].tobytes()
        finally:
            for a in (fin, out, mm):
                net.host_free(a)
        net.rgb_format = fmt                                          # and the context still works afterwards
        same("after the refused call", net.infer_batch(rgb)[1], want)
    finally:
        net.close()
