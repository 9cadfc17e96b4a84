"""GPU: pb_jpeg_encode / pb_jpeg_encode_dev (prisma_amd/csrc/jpeg.hip) against the restatement tests/jpeg_ref.py, byte for byte: all three layouts at
qualities 1, 50 and 100 over the sizes and contents at which the encoder takes another path, several frames in one call, the device-pointer form,
and the overflow rule with guard bytes behind the capacity."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jpeg_ref as J  # noqa: E402
import yuv_out_ref as O  # noqa: E402

pytestmark = pytest.mark.gpu

QUALITIES = (1, 50, 100)
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    from prisma_amd import engine
    o = engine.Ops()
    yield o
    o.close()


def fmt_of(chroma):
    return (chroma, 8, True, "bt601")


def noise(H, W, seed=0):
    return np.random.default_rng(7919 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def planes_of_rgb(chroma, rgb):
    return O.rgb_to_yuv(fmt_of(chroma), rgb)


def last_coefficient_planes(chroma, H, W):
    """every plane tiled with the (7, 7) basis function: its blocks quantise to the one coefficient at the end of the zigzag, 62 zeros before it"""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = np.clip(np.rint(128 + 120 * np.outer(c, c)), 0, 255).astype(np.uint8)
    out = []
    shapes = [(H, W)] + ([] if chroma == 400 else [((H + 1) // 2, (W + 1) // 2) if chroma == 420 else (H, W)] * 2)
    for h, w in shapes:
        out.append(np.tile(tile, ((h + 7) // 8, (w + 7) // 8))[:h, :w].reshape(-1))
    return np.concatenate(out)


# name -> (H, W, planes of a layout)
CASES = {
    "8x8": (8, 8, lambda ch: planes_of_rgb(ch, noise(8, 8))),
    "16x16": (16, 16, lambda ch: planes_of_rgb(ch, noise(16, 16))),                     # one MCU of 4:2:0
    "17x23": (17, 23, lambda ch: planes_of_rgb(ch, noise(17, 23))),                     # padding in both directions, an odd chroma size
    "80x16": (80, 16, lambda ch: planes_of_rgb(ch, noise(80, 16))),                     # 10 intervals at 444: the RST index wraps
    "24x136": (24, 136, lambda ch: planes_of_rgb(ch, noise(24, 136))),                  # three intervals of 17 MCUs
    "16x2064": (16, 2064, lambda ch: planes_of_rgb(ch, noise(16, 2064))),               # an interval longer than a wave's and a workgroup's blocks (774 at 444): the scans carry
    "flat": (24, 40, lambda ch: planes_of_rgb(ch, np.full((24, 40, 3), 128, np.uint8))),                     # EOB only
    "checker": (24, 40, lambda ch: planes_of_rgb(ch, np.repeat(((np.add.outer(np.arange(24), np.arange(40)) & 1) * 255).astype(np.uint8)[..., None], 3, -1))),
    "noise": (83, 101, lambda ch: planes_of_rgb(ch, noise(83, 101))),                   # long codes, many stuffed bytes
    "last": (16, 32, lambda ch: last_coefficient_planes(ch, 16, 32)),                   # ZRL runs; aligned rows: the 16-byte loads
}


@functools.lru_cache(maxsize=None)
def case(name, chroma):
    H, W, make = CASES[name]
    p = np.ascontiguousarray(make(chroma), np.uint8).reshape(-1)
    p.setflags(write=False)
    return H, W, p


@functools.lru_cache(maxsize=None)
def want(name, chroma, q):
    H, W, p = case(name, chroma)
    return J.encode(p, H, W, chroma, q)


def same(what, got, ref):
    got = bytes(got)
    if got != ref:
        k = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
        raise AssertionError("%s: %d bytes against the reference's %d, first difference at byte %d" % (what, len(got), len(ref), k))


def test_cases_are_what_they_claim():
    """the properties the cases are chosen for, read off the reference"""
    z = J.coefficients(case("last", 400)[2], 16, 32, 400, 50)[0].reshape(-1, 64)
    assert ((z[:, 63] != 0) & (np.abs(z[:, :63]).sum(axis=1) == 0)).any()
    z = J.coefficients(case("flat", 444)[2], 24, 40, 444, 50)
    assert all((c[..., 1:] == 0).all() for c in z)
    z = J.coefficients(case("checker", 400)[2], 24, 40, 400, 100)[0]
    assert np.abs(z).max() >= 512                     # category 10 and above
    assert J.mcu_grid(444, 80, 16)[0] == 10 and J.mcu_grid(444, 16, 2064)[1] * 3 > 256 and J.mcu_grid(400, 16, 2064)[1] > 256
    b = want("noise", 444, 100)
    assert b.count(b"\xff\x00") > 100                 # stuffed bytes


@pytest.mark.parametrize("chroma", J.CHROMAS)
@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_reference(ops, name, chroma):
    H, W, p = case(name, chroma)
    for q in QUALITIES:
        out, offs = ops.jpeg_encode(p, H, W, chroma, q)
        assert offs[0] == 0
        same("%s %d q%d" % (name, chroma, q), out[:offs[1]], want(name, chroma, q))


@pytest.mark.parametrize("chroma", J.CHROMAS)
def test_misaligned_planes(ops, chroma):
    """the byte path of the coefficient kernel on a size whose rows would take the 16-byte loads: device planes that start at an odd address (the
    host form copies into its own aligned slot, so only the device-pointer form can hand the kernel such a pointer); and a host array at an odd
    address through the host form"""
    H, W, p = case("last", chroma)
    ref = want("last", chroma, 50)
    buf = np.zeros(p.size + 1, np.uint8)
    buf[1:] = p
    out, offs = ops.jpeg_encode(buf[1:], H, W, chroma, 50)
    same("misaligned host %d" % chroma, out[:offs[1]], ref)
    cap = len(ref)
    d_in, d_out, d_off = ops.dev_alloc(p.size + 16), ops.dev_alloc(cap + GUARD), ops.dev_alloc(16)
    try:
        assert d_in % 16 == 0
        ops.h2d(d_in + 1, p)
        ops.h2d(d_out, np.full(cap + GUARD, 0xA5, np.uint8))
        ops.jpeg_encode_dev(d_in + 1, 1, H, W, chroma, 50, d_out, cap, d_off)
        ops.sync()
        got, goff = np.empty(cap + GUARD, np.uint8), np.empty(2, np.int64)
        ops.d2h(got, d_out)
        ops.d2h(goff, d_off)
    finally:
        for q in (d_in, d_out, d_off):
            ops.dev_free(q)
    assert list(goff) == [0, cap]
    same("misaligned device %d" % chroma, got[:cap], ref)
    assert (got[cap:] == 0xA5).all()


@pytest.mark.parametrize("chroma", J.CHROMAS)
def test_three_frames_equal_three_calls(ops, chroma):
    H, W = 17, 23
    frames = np.stack([planes_of_rgb(chroma, noise(H, W, seed)) for seed in (1, 2, 3)])
    out, offs = ops.jpeg_encode(frames, H, W, chroma, 90)
    assert offs[0] == 0 and (np.diff(offs) > 0).all()
    for i in range(3):
        one, o1 = ops.jpeg_encode(frames[i], H, W, chroma, 90)
        assert bytes(out[offs[i]:offs[i + 1]]) == bytes(one[:o1[1]])
        same("frame %d" % i, one[:o1[1]], J.encode(frames[i], H, W, chroma, 90))


def test_more_frames_than_a_chunk(ops):
    """five frames in chunks of two: the offsets run on over the chunks"""
    H, W = 9, 17
    frames = np.stack([planes_of_rgb(420, noise(H, W, seed)) for seed in range(5)])
    ops.set_option("host_chunk", 2)
    try:
        out, offs = ops.jpeg_encode(frames, H, W, 420, 75)
    finally:
        ops.set_option("host_chunk", 0)
    for i in range(5):
        same("frame %d" % i, out[offs[i]:offs[i + 1]], J.encode(frames[i], H, W, 420, 75))


@pytest.mark.parametrize("chroma", J.CHROMAS)
def test_dev_equals_host(ops, chroma):
    from prisma_amd import engine
    H, W, q, n = 24, 136, 75, 2
    frames = np.stack([planes_of_rgb(chroma, noise(H, W, seed)) for seed in (4, 5)])
    out, offs = ops.jpeg_encode(frames, H, W, chroma, q)
    cap = int(offs[n])
    d_in, d_out, d_off = ops.dev_alloc(frames.nbytes), ops.dev_alloc(cap + GUARD), ops.dev_alloc(8 * (n + 1))
    try:
        ops.h2d(d_in, frames)
        ops.h2d(d_out, np.full(cap + GUARD, 0xA5, np.uint8))
        ops.jpeg_encode_dev(d_in, n, H, W, chroma, q, d_out, cap, d_off)
        ops.sync()
        got, goff = np.empty(cap + GUARD, np.uint8), np.empty(n + 1, np.int64)
        ops.d2h(got, d_out)
        ops.d2h(goff, d_off)
    finally:
        for p in (d_in, d_out, d_off):
            ops.dev_free(p)
    assert np.array_equal(goff, offs)
    assert bytes(got[:cap]) == bytes(out[:cap])
    assert (got[cap:] == 0xA5).all()
    assert cap <= n * engine.jpeg_bound(chroma, q, H, W)


@pytest.mark.parametrize("chunk", (0, 2))
def test_overflow(ops, chunk):
    """a capacity one byte short: the error, the need in offsets[n], the frames that fit intact, nothing written behind them"""
    from prisma_amd import engine
    H, W, q, n = 17, 23, 100, 3
    frames = np.stack([planes_of_rgb(444, noise(H, W, seed)) for seed in (6, 7, 8)])
    refs = [J.encode(f, H, W, 444, q) for f in frames]
    need = sum(len(r) for r in refs)
    buf = np.full(need + GUARD, 0xA5, np.uint8)
    ops.set_option("host_chunk", chunk)
    try:
        with pytest.raises(engine.JpegOverflow) as e:
            ops.jpeg_encode(frames, H, W, 444, q, out=buf, capacity=need - 1)
    finally:
        ops.set_option("host_chunk", 0)
    assert e.value.needed == need
    assert list(e.value.offsets) == [0, len(refs[0]), len(refs[0]) + len(refs[1]), need]
    assert bytes(buf[:len(refs[0]) + len(refs[1])]) == refs[0] + refs[1]
    assert (buf[len(refs[0]) + len(refs[1]):] == 0xA5).all()
    # and the status is the one the header names
    offs = np.zeros(n + 1, np.int64)
    from prisma_amd import _lib
    rc = ops.lib.pb_jpeg_encode(ops.ctx, C.byref(_lib.pb_jpeg_cfg(444, q)), frames.ctypes.data_as(C.c_void_p), n, H, W,
                                buf.ctypes.data_as(C.c_void_p), need - 1, offs.ctypes.data_as(C.c_void_p))
    assert rc == -3 and offs[n] == need
    out, offs = ops.jpeg_encode(frames, H, W, 444, q, out=buf, capacity=need)
    assert bytes(buf[:need]) == b"".join(refs) and (buf[need:] == 0xA5).all()


@pytest.mark.parametrize("chroma,quality,H,W", [(422, 90, 8, 8), (444, 0, 8, 8), (444, 101, 8, 8), (420, 90, 0, 8), (400, 90, 8, 65536)])
def test_refusals(ops, chroma, quality, H, W):
    from prisma_amd import _lib, engine
    assert engine.jpeg_bound(chroma, quality, H, W) == 0
    a, offs = np.zeros(1 << 16, np.uint8), np.zeros(2, np.int64)
    rc = ops.lib.pb_jpeg_encode(ops.ctx, C.byref(_lib.pb_jpeg_cfg(chroma, quality)), a.ctypes.data_as(C.c_void_p), 1, H, W,
                                a.ctypes.data_as(C.c_void_p), a.size, offs.ctypes.data_as(C.c_void_p))
    assert rc == -1, ops.lib.pb_last_error()
