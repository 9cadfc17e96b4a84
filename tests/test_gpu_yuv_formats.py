"""GPU: pb_yuv_to_rgb / pb_yuv_to_rgb_dev (prisma_amd/csrc/yuv_formats.hip) and pb_set_frame_format against the restatement tests/yuv_fmt_ref.py,
byte for byte: every layout x depth x range x matrix at every size at which a kernel takes another path (one lane, odd edges, the 16-byte path
and its odd last chroma row, the byte path over several workgroups), random and saturating samples, every input value of 8-bit 4:4:4, value
lattices of the deeper formats, and guard bytes behind every output."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import yuv_fmt_ref as F  # noqa: E402
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
def case(fmt, H, W, kind, n=N):
    """(packed frames, their restated RGB): random bytes (a 16-bit word then uses all its bits, whatever the depth), or only 0x00 and 0xFF bytes
    - 0 and all-ones samples (and 0x00FF / 0xFF00 words), so that every clip8 saturates"""
    rng = np.random.default_rng(1000 * H + W + fmt[0] + fmt[1] + (0 if kind == "random" else 7))
    shape = (n, F.frame_bytes(fmt, H, W))
    yuv = rng.integers(0, 256, shape, dtype=np.uint8) if kind == "random" else rng.integers(0, 2, shape, dtype=np.uint8) * 255
    if kind != "random" and fmt[1] > 8:         # whole words: 0 or 0xFFFF
        yuv = np.repeat(yuv[:, ::2], 2, axis=1)
    want = F.to_rgb(fmt, yuv, H, W)
    yuv.setflags(write=False)
    want.setflags(write=False)
    return yuv, want


def on_device(ops, fmt, src, n, H, W, skew=0):
    """one _dev call on device buffers: the output preset to 0xFF with GUARD bytes behind it -> (output bytes, guard bytes).  skew = 1: both
    arrays start one byte into their allocations, which takes a W % 16 == 0 frame off the 16-byte path (the byte in front is checked too)"""
    out_bytes = n * H * W * 3
    d_in, d_out = ops.dev_alloc(src.nbytes + skew), ops.dev_alloc(skew + out_bytes + GUARD)
    try:
        ops.h2d(d_in + skew, src)
        ops.h2d(d_out, np.full(skew + out_bytes + GUARD, 0xFF, np.uint8))
        ops.yuv_to_rgb_dev(fmt, d_in + skew, n, H, W, d_out + skew)
        ops.sync()
        got = np.empty(skew + out_bytes + GUARD, np.uint8)
        ops.d2h(got, d_out)
    finally:
        ops.dev_free(d_in)
        ops.dev_free(d_out)
    assert (got[:skew] == 0xFF).all() and (got[skew + out_bytes:] == 0xFF).all(), "bytes outside the output were written"
    return got[skew:skew + out_bytes].reshape(n, H, W, 3)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("chroma", F.CHROMAS)
def test_every_format_host_and_dev(ops, chroma, depth, H, W):
    from prisma_amd import engine
    for full, matrix, kind in itertools.product((False, True), F.MATRICES, ("random", "saturating")):
        fmt = (chroma, depth, full, matrix)
        yuv, want = case(fmt, H, W, kind)
        what = "%r %dx%d %s" % (fmt, H, W, kind)
        assert engine.yuv_bytes(fmt, H, W) == yuv.shape[1]
        # host pointers, into the caller's array: nothing behind it is touched
        buf = np.full(want.size + GUARD, 0xFF, np.uint8)
        ops.yuv_to_rgb(fmt, yuv, H, W, out=buf[:want.size].reshape(want.shape))
        same("yuv_to_rgb " + what, buf[:want.size].reshape(want.shape), want)
        assert (buf[want.size:] == 0xFF).all()
        # device pointers, aligned (the 16-byte path where W allows it) and one byte off (the byte path, the same bytes)
        for skew in ((0, 1) if W % 16 == 0 else (0,)):
            same("yuv_to_rgb_dev skew %d %s" % (skew, what), on_device(ops, fmt, yuv, N, H, W, skew=skew), want)
    same("one frame", ops.yuv_to_rgb(fmt, yuv[1], H, W), want[1])


@pytest.mark.parametrize("fmt", [(422, 10, True, "bt709"), (444, 8, False, "bt709"), (400, 12, False, "bt601"), (420, 16, True, "bt601")], ids=str)
def test_chunked_host_call(ops, fmt):
    """more frames than a chunk ("host_chunk" 2: chunks of 2, 2, 1 through both device slots)"""
    H, W = 16, 64
    yuv, want = case(fmt, H, W, "random", n=5)
    ops.set_option("host_chunk", 2)
    try:
        same("chunked yuv_to_rgb %r" % (fmt,), ops.yuv_to_rgb(fmt, yuv, H, W), want)
    finally:
        ops.set_option("host_chunk", 0)


def both_paths(ops, fmt, yuv, H, W, want, what):
    for skew, path in ((0, "16-byte path"), (1, "byte path")):
        same("%s, %r, %s" % (what, fmt, path), on_device(ops, fmt, yuv, 1, H, W, skew=skew)[0], want)


@functools.lru_cache(maxsize=None)
def every_triple():
    """all 2^24 (Y, Cb, Cr) as one 4096 x 4096 8-bit 4:4:4 frame: Y = the pixel index >> 16, Cb = its bits 8 .. 15, Cr = its low byte"""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    y, cb, cr = (i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)
    yuv = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    yuv.setflags(write=False)
    return yuv, y.astype(np.int64), cb.astype(np.int64), cr.astype(np.int64)


@pytest.mark.parametrize("matrix", F.MATRICES)
@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
def test_every_triple_of_8_bit_444(ops, full, matrix):
    fmt = (444, 8, full, matrix)
    yuv, y, cb, cr = every_triple()
    want = np.stack(F.colour(fmt, y, cb, cr), axis=-1).astype(np.uint8)
    both_paths(ops, fmt, yuv, 4096, 4096, want, "RGB of every (Y, Cb, Cr)")


@pytest.mark.parametrize("depth,ystep", [(10, 1), (12, 4), (12, 64), (16, 4), (16, 64)])
def test_deep_444_lattices(ops, depth, ystep):
    """one 1024 x 4096 4:4:4 frame: a 64 x 64 chroma lattice (0, coff and its neighbours, the nominal limits, 2^d - 1, 0xFFFF, an even spread)
    crossed with 1024 luma values - every value at 10 bit; at 12 and 16 bit every 4th from 0 and every 64th over the whole 16-bit word"""
    H, W = 1024, 4096
    top = 2 ** depth - 1
    coff = 2 ** (depth - 1)
    special = [0, 1, coff - 1, coff, coff + 1, 16 << (depth - 8), 240 << (depth - 8), (240 << (depth - 8)) + 1, top - 1, top, 0xFFFF, 0xFFFE]
    special = sorted({min(v, 0xFFFF) for v in special})
    fill = [v for v in np.linspace(0, 0xFFFF, 80).astype(np.int64).tolist() if v not in special]
    cl = np.array(sorted(special + fill[:64 - len(special)]), np.int64)
    assert len(cl) == 64 and {0, coff, top, 0xFFFF} <= set(cl.tolist())
    yv = (np.arange(1024, dtype=np.int64) * ystep) & 0xFFFF
    y = np.repeat(yv[:, None], W, axis=1)
    cb = np.broadcast_to(np.repeat(cl, 64)[None, :], (H, W))
    cr = np.broadcast_to(np.tile(cl, 64)[None, :], (H, W))
    for full, matrix in itertools.product((False, True), F.MATRICES):
        fmt = (444, depth, full, matrix)
        yuv = F.pack(fmt, y, cb, cr)
        want = np.stack(F.colour(fmt, y, cb, cr), axis=-1).astype(np.uint8)
        both_paths(ops, fmt, yuv, H, W, want, "lattice, luma step %d" % ystep)


@pytest.mark.parametrize("H,W", [(5, 18), (6, 32)])
def test_i420_format_is_the_existing_kernel(ops, H, W):
    yuv, want = case(I420, H, W, "random")
    same("restatements agree", want, R.i420_to_rgb(yuv, H, W))
    same("yuv_to_rgb at I420", ops.yuv_to_rgb(I420, yuv, H, W), ops.i420_to_rgb(yuv, H, W))
    same("yuv_to_rgb at I420 against the restatement", ops.yuv_to_rgb(I420, yuv, H, W), want)
    same("yuv_to_rgb_dev at I420", on_device(ops, I420, yuv, N, H, W), want)


def test_bad_arguments_are_refused_before_any_launch(ops):
    for bad in (lambda: ops.yuv_to_rgb_dev((411, 8, False, "bt601"), 1, 1, 4, 4, 1), lambda: ops.yuv_to_rgb_dev((420, 17, False, "bt601"), 1, 1, 4, 4, 1),
                lambda: ops.yuv_to_rgb_dev((420, 8, False, "bt2020"), 1, 1, 4, 4, 1), lambda: ops.yuv_to_rgb_dev(I420, 0, 1, 4, 4, 0),
                lambda: ops.yuv_to_rgb_dev(I420, 1, 0, 4, 4, 1)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError):
        ops.yuv_to_rgb((411, 8, False, "bt601"), np.zeros(24, np.uint8), 4, 4)


def test_set_frame_format_on_a_band_context():
    """a depth context: the format decides what `frames` is; a refusal leaves the context as it was; "frames_i420" still toggles"""
    from prisma_amd import engine, synth
    H, W = 42, 64
    fmt = engine.YuvFormat(422, 10, True, "bt709")
    yuv, rgb = case(tuple(fmt), H, W, "random", n=2)
    i420, rgb420 = case(I420, H, W, "random", n=2)
    net = engine.DepthAnything(synth.depth_anything_weights("vits", seed=1234), "vits", device=0, max_batch=2)
    try:
        plain = net.infer_batch(rgb)
        net.frame_format = fmt
        assert net.frame_format == fmt
        got = net.infer_batch(yuv, size=(H, W))
        for x, y in zip(got, plain):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        for bad in ((411, 8, False, "bt601"), (420, 7, False, "bt601"), (420, 8, False, "bt2020")):
            with pytest.raises(RuntimeError):
                net.frame_format = bad
            assert net.frame_format == fmt
            again = net.infer_batch(yuv, size=(H, W))                 # the context still takes the format it had
            assert again[1].tobytes() == plain[1].tobytes()
        with pytest.raises(AssertionError):
            net.infer_batch(rgb)                                      # RGB frames on a YUV context: refused by the shape check
        net.frame_format = "i420"                                     # pb_set_option "frames_i420", 1
        want420 = net.infer_batch(i420, size=(H, W))
        net.frame_format = engine.YuvFormat(*I420)                    # the same through pb_set_frame_format
        assert net.infer_batch(i420, size=(H, W))[1].tobytes() == want420[1].tobytes()
        net.frame_format = "rgb"                                      # "frames_i420", 0 after a format: RGB again
        assert net.infer_batch(rgb420)[1].tobytes() == want420[1].tobytes()
        off = net.infer_batch(rgb)
        for x, y in zip(off, plain):
            assert x.tobytes() == y.tobytes()
        # refused while a submission is outstanding
        frames, out, mm = net.host_empty(rgb.shape, np.uint8), net.host_empty(rgb.shape, np.uint8), net.host_empty((2, 2), np.float32)
        try:
            frames[:] = rgb
            net.submit_batch(frames, out_rgb=out, out_min=mm[0], out_max=mm[1])
            with pytest.raises(RuntimeError):
                net.frame_format = fmt
            net.wait()
            assert net.frame_format == "rgb" and out.tobytes() == plain[1].tobytes()
        finally:
            for a in (frames, out, mm):
                net.host_free(a)
    finally:
        net.close()


@pytest.mark.parametrize("fmt", [(422, 10, False, "bt709"), (444, 16, True, "bt601")], ids=str)
def test_mask_context_takes_frames_larger_than_rgb_from_pageable_memory(fmt):
    """the mask band's pipeline stages a pageable `frames` array in page-locked memory of its own: 4 and 6 bytes per pixel here, more than the
    3 of the RGB frames that staging was once sized for.  Three frames at max_batch 2: two chunks.  The id images are those of the RGB run."""
    from prisma_amd import engine, synth
    H, W = 180, 300
    yuv, rgb = case(fmt, H, W, "random")
    assert yuv.shape[1] > H * W * 3 and not yuv.flags.writeable          # plain numpy memory, larger than RGB
    cfg = synth.MASK_CFGS["tiny"]
    net = engine.MaskMMDet(synth.solov2_weights(cfg), cfg, max_batch=2)
    try:
        plain = net.infer_batch(rgb, 0.5, None)
        net.frame_format = engine.YuvFormat(*fmt)
        got = net.infer_batch(yuv, 0.5, None, size=(H, W))
        assert got.dtype == plain.dtype and got.shape == plain.shape and got.tobytes() == plain.tobytes()
        again = net.infer_batch(yuv[:2], 0.5, None, size=(H, W))          # the kept staging buffer, a smaller call
        assert again.tobytes() == plain[:2].tobytes()
        net.frame_format = "rgb"
        assert net.infer_batch(rgb, 0.5, None).tobytes() == plain.tobytes()
    finally:
        net.close()
