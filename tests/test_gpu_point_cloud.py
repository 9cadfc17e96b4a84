"""GPU: pb_depth_point_cloud / pb_depth_point_cloud_dev (the depth band's `--ply`) against the float32 restatement of the reference's
write_pcl (tests/pcl_ref.py), byte for byte.  cv2.medianBlur and plyfile's record layout are pinned by that restatement, not by the
packages (tests/test_pcl_ref_cpu.py)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bands"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcl_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from prisma_amd import engine
    o = engine.Ops()
    yield o
    o.close()


@functools.lru_cache(maxsize=None)
def case(name):
    H, W, ties = R.SHAPES[name]
    d, c = R.make_case(H, W, ties)
    d.setflags(write=False)
    c.setflags(write=False)
    return d, c


@functools.lru_cache(maxsize=None)
def batch():
    """three 5 x 7 frames (H W odd: frames 1 and 2 start at byte offsets 525 and 1050) with different ranges"""
    fr = [R.make_case(5, 7, seed=s, lo=lo, span=span) for s, (lo, span) in enumerate([(0.5, 20.0), (3.0, 2.0), (40.0, 100.0)])]
    return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])


def same(what, got, want):
    assert got.dtype == R.VERTEX and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    g, w = R.raw(got), R.raw(want)
    if not np.array_equal(g, w):
        bad = np.argwhere((g != w).any(axis=-1))
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d records differ, first at %s: kernel %s (%s), restatement %s (%s)" % (
            what, len(bad), g[..., 0].size, i, got[i], g[i].tobytes().hex(), want[i], w[i].tobytes().hex()))


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_single_frame(ops, name, flip):
    """2 x 3 .. 67 x 131: smaller than the window, ties, odd sizes; 37 x 150 spans three 16 x 64 tiles and a remainder both ways"""
    d, c = case(name)
    H, W = d.shape
    if name == "37x150":
        assert H > 2 * R.TILE[0] and H % R.TILE[0] and W > 2 * R.TILE[1] and W % R.TILE[1]
    same("%s flip %d" % (name, flip), ops.point_cloud(d, c, flip=bool(flip)), R.cloud_restated(d, c, flip, W / 2, H / 2))


def test_one_pixel(ops):
    d, c = R.make_case(1, 1)
    same("1x1", ops.point_cloud(d, c, flip=False), R.cloud_restated(d, c, 0, 0.5, 0.5))


@pytest.mark.parametrize("k", range(len(R.INTRINSICS)))
def test_intrinsics(ops, k):
    u0, v0, fx, fy = R.INTRINSICS[k]
    d, c = R.make_case(6, 9)
    got = ops.point_cloud(d, c, flip=True, u0=u0, v0=v0, fx=fx, fy=fy)
    same("intrinsics %r" % (R.INTRINSICS[k],), got, R.cloud_restated(d, c, 1, u0, v0, fx, fy))
    assert float(v0) == int(v0)
    assert R.raw(got)[int(v0), :, 4:8].tolist() == [[0x00, 0x00, 0x00, 0x80]] * 9, "y of row v0 must be -0.0"


def test_batch(ops):
    d, c = batch()
    got = ops.point_cloud(d, c, flip=True)
    assert got.shape == (3, 5, 7)
    same("batch of 3", got, R.cloud_restated(d, c, 1, 3.5, 2.5))
    for i in range(3):
        same("batch frame %d vs its own call" % i, got[i], ops.point_cloud(d[i], c[i], flip=True))
    assert not np.array_equal(R.raw(got[1]), R.raw(R.cloud_restated(d, c, 0, 3.5, 2.5)[1]))


@pytest.mark.parametrize("shift", [0, 1])
def test_device_entry_point(ops, shift):
    """pb_depth_point_cloud_dev + pb_sync = the host entry point's bytes; nothing is written outside the output (0xA5 guards), also when the
    output itself starts off a dword boundary (shift)"""
    for d, c in (batch(), tuple(a[None] for a in case("37x150"))):
        n, H, W = d.shape
        nb = n * H * W * 15
        want = ops.point_cloud(d, c, flip=True)
        pd, pc, po = ops.dev_alloc(d.nbytes), ops.dev_alloc(c.nbytes), ops.dev_alloc(64 + nb + 64)
        try:
            ops.h2d(pd, d)
            ops.h2d(pc, c)
            ops.h2d(po, np.full(64 + nb + 64, 0xA5, np.uint8))
            ops.point_cloud_dev(pd, pc, n, H, W, po + 64 + shift, flip=True)
            ops.sync()
            back = np.empty(64 + nb + 64, np.uint8)
            ops.d2h(back, po)
        finally:
            for p in (pd, pc, po):
                ops.dev_free(p)
        body = back[64 + shift:64 + shift + nb]
        same("device entry point %dx%dx%d shift %d" % (n, H, W, shift), body.view(R.VERTEX).reshape(n, H, W), want)
        assert (back[:64 + shift] == 0xA5).all() and (back[64 + shift + nb:] == 0xA5).all(), "bytes outside the output were written"


def test_bad_arguments(ops):
    from prisma_amd import _lib
    d, c = R.make_case(2, 3)
    out = np.empty(2 * 3 * 15, np.uint8)
    P = lambda a: a.ctypes.data  # noqa: E731
    for fn in (ops.lib.pb_depth_point_cloud, ops.lib.pb_depth_point_cloud_dev):
        assert fn(ops.ctx, None, P(c), 1, 2, 3, 1, 1.5, 1.0, 1000.0, 1000.0, P(out)) == -1
        assert fn(ops.ctx, P(d), P(c), 0, 2, 3, 1, 1.5, 1.0, 1000.0, 1000.0, P(out)) == -1
        assert fn(ops.ctx, P(d), P(c), 1, 2, -3, 1, 1.5, 1.0, 1000.0, 1000.0, P(out)) == -1
    assert b"point_cloud" in _lib.load().pb_last_error()


def test_band_writes_the_ply(tmp_path, capsys):
    """depth_anything.main(-i img.png --ply --npy): depth_anything.ply beside the PNG = write_pcl of the prediction the band saved"""
    import depth_anything as band
    from PIL import Image
    from prisma_amd import synth
    img = synth.frames(1, 70, 90, seed=5)[0]
    Image.fromarray(img).save(tmp_path / "img.png")
    os.environ["PRISMA_OVERWRITE"] = "1"
    band.model = None
    try:
        band.main(["-i", str(tmp_path / "img.png"), "--encoder", "vits", "--ply", "--npy"])
    finally:
        if band.model is not None:
            band.model.close()
        band.model = None
    assert "not built" not in capsys.readouterr().err
    blob = open(tmp_path / "depth_anything.ply", "rb").read()
    head, body = blob[:blob.index(b"end_header\n") + 11], blob[blob.index(b"end_header\n") + 11:]
    assert b"\nelement vertex %d\n" % (70 * 90) in head and head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    pred = np.load(tmp_path / "depth_anything.npy")
    assert pred.shape == (70, 90) and pred.dtype == np.float32
    want = R.cloud_restated(pred, img, True, 90 / 2, 70 / 2, 1000, 1000)
    assert len(body) == 15 * 70 * 90
    same("band ply", np.frombuffer(body, R.VERTEX).reshape(70, 90), want)
    assert np.asarray(Image.open(tmp_path / "depth_anything.png")).shape == (70, 90, 3)
