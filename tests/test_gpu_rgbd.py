"""GPU: pb_rgbd_depth / pb_rgbd_depth_dev (the rgba band's `--rgbd ... --encoding_depth hue`) against the float64 restatement of the reference's
hue decode and heat encode (tests/rgbd_ref.py): the bytes and the float32 heat value equal, on every colour and on every geometry at which
hue_heat_kernel takes another path.  The restatement itself is held to the reference's bytes by tests/test_rgbd_ref_cpu.py."""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rgbd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from prisma_amd import engine
    o = engine.Ops()
    yield o
    o.close()


@functools.lru_cache(maxsize=None)
def case(n, H, W, side):
    """(frames, restated bytes, restated float32 heat), computed once and read-only"""
    fr = R.make_frames(n, H, W, side, seed=n)
    _, rgb, heat = R.split_restated(fr, side)
    out = (fr, np.ascontiguousarray(rgb), heat.astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def same(what, got_rgb, got_heat, want_rgb, want_heat):
    if got_rgb is not None:
        assert got_rgb.dtype == np.uint8 and got_rgb.shape == want_rgb.shape, (what, got_rgb.shape, want_rgb.shape)
        if not np.array_equal(got_rgb, want_rgb):
            bad = np.argwhere((got_rgb != want_rgb).any(axis=-1))
            i = tuple(bad[0])
            raise AssertionError("%s: %d of %d pixels differ, first at %s: kernel %s, restatement %s" % (
                what, len(bad), want_rgb[..., 0].size, i, got_rgb[i], want_rgb[i]))
    if got_heat is not None:
        assert got_heat.dtype == np.float32 and got_heat.shape == want_heat.shape, (what, got_heat.shape, want_heat.shape)
        if not np.array_equal(got_heat, want_heat):
            bad = np.argwhere(got_heat != want_heat)
            i = tuple(bad[0])
            raise AssertionError("%s: %d of %d heat values differ, first at %s: kernel %r, restatement %r" % (
                what, len(bad), want_heat.size, i, got_heat[i], want_heat[i]))


def test_every_colour(ops):
    """all 2^24 colours in order as the right halves of 16 frames of 1024 x 2048 (the colour halves random), one host-pointer call"""
    fr = np.random.default_rng(1).integers(0, 256, (16, 1024, 2048, 3), dtype=np.uint8)
    fr[:, :, 1024:] = R.all_colours().reshape(16, 1024, 1024, 3)
    rgb, heat = ops.rgbd_depth(fr, "right", want_heat=True)
    del fr
    assert rgb.shape == (16, 1024, 1024, 3) and heat.shape == (16, 1024, 1024)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgbd_hue.npz"))
    assert hashlib.sha256(rgb.tobytes()).hexdigest() == str(z["sha256"])
    rgb, heat = rgb.reshape(-1, 3), heat.reshape(-1)
    for lo, d, o in R.table():
        same("colours %d .." % lo, rgb[lo:lo + len(o)], heat[lo:lo + len(d)], o, d.astype(np.float32))


GEOMETRY = [(1, 2), (2, 1), (2, 2), (5, 7), (7, 5), (9, 301), (37, 150)]


@pytest.mark.parametrize("side", R.SIDES)
@pytest.mark.parametrize("H,W", GEOMETRY)
def test_geometry(ops, H, W, side):
    """odd sizes: box rows and frames start at every byte alignment, half widths are no multiple of the four pixels a lane owns (groups straddle
    row ends, the stream ends in a partial group); 37 x 150 spans several workgroups with a remainder"""
    if (W if side in ("left", "right") else H) < 2:
        with pytest.raises(Exception, match="half"):
            ops.rgbd_depth(np.zeros((1, H, W, 3), np.uint8), side)
        return
    if (H, W) == (37, 150):
        rb, db = R.boxes(H, W, side)
        px = (db[1] - db[0]) * (db[3] - db[2])
        assert px > 2 * 256 * R.PX_PER_LANE and px % (256 * R.PX_PER_LANE)
    if (H, W) == (9, 301) and side in ("left", "right"):
        assert (W // 2) % R.PX_PER_LANE and (W - W // 2) % R.PX_PER_LANE
    fr, want_rgb, want_heat = case(1, H, W, side)
    rgb, heat = ops.rgbd_depth(fr, side, want_heat=True)
    same("%dx%d %s" % (H, W, side), rgb, heat, want_rgb, want_heat)


@pytest.mark.parametrize("side", R.SIDES)
def test_three_frames(ops, side):
    """n = 3 frames of 5 x 7: frames 1 and 2 start at bytes 105 and 210, no dword multiples"""
    fr, want_rgb, want_heat = case(3, 5, 7, side)
    rgb, heat = ops.rgbd_depth(fr, side, want_heat=True)
    same("3 x 5x7 %s" % side, rgb, heat, want_rgb, want_heat)
    for i in range(3):
        one = ops.rgbd_depth(fr[i:i + 1], side)
        assert np.array_equal(one[0], rgb[i])


@pytest.mark.parametrize("H,W,side", [(9, 301, "right"), (37, 150, "bottom"), (5, 7, "left")])
def test_output_combinations(ops, H, W, side):
    fr, want_rgb, want_heat = case(1, H, W, side)
    both = ops.rgbd_depth(fr, side, want_heat=True)
    same("both", both[0], both[1], want_rgb, want_heat)
    same("bytes alone", ops.rgbd_depth(fr, side), None, want_rgb, want_heat)
    same("heat alone", None, ops.rgbd_depth(fr, side, want_heat=True, want_rgb=False), want_rgb, want_heat)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_entry_point(ops, shift):
    """pb_rgbd_depth_dev + pb_sync: the host entry point's values; the outputs sit between 0xA5 guard bytes that stay untouched, also when
    depth_out starts off a dword boundary (shift) and the frames do too; what lies outside the depth box never reaches the result (it is
    overwritten with another pattern before the call, and the result stays the same)"""
    for n, H, W, side in ((3, 5, 7, "right"), (1, 37, 150, "left"), (2, 9, 301, "bottom")):
        fr, want_rgb, want_heat = case(n, H, W, side)
        rb, db = R.boxes(H, W, side)
        poisoned = np.full_like(fr, 0x5A)
        poisoned[:, db[0]:db[1], db[2]:db[3]] = fr[:, db[0]:db[1], db[2]:db[3]]
        nb, nh = want_rgb.size, want_heat.size * 4
        pf, po, ph = ops.dev_alloc(64 + fr.nbytes + 64), ops.dev_alloc(64 + nb + 64), ops.dev_alloc(64 + nh + 64)
        try:
            ops.h2d(pf, np.concatenate([np.full(64, 0x5A, np.uint8), poisoned.reshape(-1), np.full(64, 0x5A, np.uint8)]))
            ops.h2d(po, np.full(64 + nb + 64, 0xA5, np.uint8))
            ops.h2d(ph, np.full(64 + nh + 64, 0xA5, np.uint8))
            # frames at 64 - shift: their start moves through the four byte alignments with the output's
            ops.h2d(pf + 64 - shift, poisoned)
            ops.rgbd_depth_dev(pf + 64 - shift, n, H, W, side, depth_ptr=po + 64 + shift, heat_ptr=ph + 64)
            ops.sync()
            back, backh = np.empty(64 + nb + 64, np.uint8), np.empty(64 + nh + 64, np.uint8)
            ops.d2h(back, po)
            ops.d2h(backh, ph)
        finally:
            for p in (pf, po, ph):
                ops.dev_free(p)
        what = "device entry point %dx%dx%d %s shift %d" % (n, H, W, side, shift)
        same(what, back[64 + shift:64 + shift + nb].reshape(want_rgb.shape), backh[64:64 + nh].view(np.float32).reshape(want_heat.shape),
             want_rgb, want_heat)
        assert (back[:64 + shift] == 0xA5).all() and (back[64 + shift + nb:] == 0xA5).all(), what + ": bytes outside depth_out were written"
        assert (backh[:64] == 0xA5).all() and (backh[64 + nh:] == 0xA5).all(), what + ": bytes outside heat_out were written"


def test_chunks_and_page_locked_arrays(ops):
    """n = 5 with host_chunk = 2 (three chunks, the last of one frame) equals one chunk; page-locked caller arrays equal pageable ones"""
    import torch
    fr, want_rgb, want_heat = case(5, 37, 150, "right")
    try:
        ops.set_option("host_chunk", 2)
        rgb, heat = ops.rgbd_depth(fr, "right", want_heat=True)
        same("host_chunk 2", rgb, heat, want_rgb, want_heat)
        pin = [torch.empty(a.shape, dtype=t).pin_memory().numpy() for a, t in ((fr, torch.uint8), (want_rgb, torch.uint8), (want_heat, torch.float32))]
        pin[0][...] = fr
        pin[1][...] = 0
        pin[2][...] = -1
        ops.rgbd_depth(pin[0], "right", want_heat=True, out_rgb=pin[1], out_heat=pin[2])
        same("page-locked, host_chunk 2", pin[1], pin[2], want_rgb, want_heat)
    finally:
        ops.set_option("host_chunk", 0)
    pin[1][...] = 0
    pin[2][...] = -1
    ops.rgbd_depth(pin[0], "right", want_heat=True, out_rgb=pin[1], out_heat=pin[2])
    same("page-locked, one chunk", pin[1], pin[2], want_rgb, want_heat)
    rgb, heat = ops.rgbd_depth(fr, "right", want_heat=True)
    same("one chunk", rgb, heat, want_rgb, want_heat)


def test_bad_arguments(ops):
    """an empty half or an unknown side is PB_ERR_ARG before anything is launched: the outputs keep their bytes"""
    from prisma_amd import _lib
    fr = np.zeros((1, 2, 1, 3), np.uint8)
    out, heat = np.full(64, 0xA5, np.uint8), np.full(16, -3.0, np.float32)
    P = lambda a: a.ctypes.data  # noqa: E731
    pd = ops.dev_alloc(256)
    try:
        for fn, f, o, h in ((ops.lib.pb_rgbd_depth, P(fr), P(out), P(heat)), (ops.lib.pb_rgbd_depth_dev, pd, pd + 64, pd + 128)):
            assert fn(ops.ctx, f, 1, 2, 1, 0, o, h) == -1 and b"half" in _lib.load().pb_last_error()       # 2 x 1 has no left half
            assert fn(ops.ctx, f, 1, 2, 1, 1, o, h) == -1
            assert fn(ops.ctx, f, 1, 1, 2, 2, o, h) == -1                                                  # 1 x 2 has no top half
            assert fn(ops.ctx, f, 1, 2, 2, 4, o, h) == -1 and b"side" in _lib.load().pb_last_error()
            assert fn(ops.ctx, f, 1, 2, 2, -1, o, h) == -1
            assert fn(ops.ctx, None, 1, 2, 2, 0, o, h) == -1
            assert fn(ops.ctx, f, 0, 2, 2, 0, o, h) == -1
            assert fn(ops.ctx, f, 1, 2, 2, 0, None, None) == -1
        ops.sync()
    finally:
        ops.dev_free(pd)
    assert (out == 0xA5).all() and (heat == -3.0).all()
