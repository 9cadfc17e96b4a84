"""GPU: `depth_anything --metric` (ZoeDepth head over the ViT-L core) through the C ABI vs oracle/zoe_oracle.py.
Tolerance: north_star's 1e-3 relative on the band's output (metric depth, at network and at frame resolution), asserted in the
default precision (PB_PREC_SPLIT); intermediate stages (relative depth of the core, bin centres) are printed and bounded at 2e-3.

The band's own tail - metric_head's ping-pong buffers, the Pillow resize whose tap count follows the frame size, the per-frame range, the
heat encode that is not flipped - is checked on ONE living context (max_batch 2, stages on) without another oracle forward: the network
size is fixed at 392 x 518, so for any frame size the frame-resolution depth must be the bytes of PIL.Image.resize of that call's own
`metric_net` stage, min / max those of the depth, the rgb the bytes of the oracle's encode of the depth.  Batch slots, chunking,
want_depth=False and re-planning are checked as bit equalities between calls."""
import numpy as np
import pytest

from oracle import depth_oracle as O
from oracle import zoe_oracle as Z
from prisma_amd import engine, synth

pytestmark = pytest.mark.gpu
TOL_RANGE, TOL_L2 = 1e-3, 1e-3
STAGE_RANGE, STAGE_L2 = 2e-3, 1e-3


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rell2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def same(what, got, want):
    """bit equality of two arrays (float32 compared as words: a NaN equals itself, -0 is not +0)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {1: np.uint8, 4: np.uint32}[got.dtype.itemsize]
    bad = got.view(u) != want.view(u)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


@pytest.fixture(scope="module")
def weights():
    return synth.zoe_weights()


@pytest.fixture(scope="module")
def net(weights):
    """the one ViT-L metric context of this module: max_batch 2, debug stages on"""
    n = engine.DepthAnything(weights, "vitl", max_batch=2, metric=True)
    n.set_profiling(True, True)
    yield n
    n.close()


SMALL = (97, 131)           # odd, not the network's aspect ratio, both axes upscaled to 392 x 518 and back


@pytest.fixture(scope="module")
def three(net):
    """three frames in one call: chunks of 2 + 1 -> (frames, depth, rgb, min, max).  Computed once; the tests below compare other calls
    of the same context with these bytes"""
    frames = synth.frames(3, *SMALL, seed=21)
    return (frames,) + tuple(net.infer_batch(frames, want_depth=True, want_rgb=True, flip=False))


def test_metric_depth_matches_oracle(net, weights):
    w = weights
    frames = synth.frames(2, 360, 640, seed=3)
    depth, rgb, mn, mx = net.infer_batch(frames, want_depth=True, want_rgb=True, flip=False)
    assert depth.shape == (2, 360, 640) and rgb.shape == (2, 360, 640, 3)
    ref_net, st = Z.forward(w, Z.preprocess(frames[1]), return_stages=True)
    for name, key in (("net_depth", "rel_depth"), ("seed_bins", "seed_bins"), ("bins0", "bins0"), ("bins3", "bins3"), ("metric_net", None)):
        got = net.stage(name)[1]
        ref = ref_net[0] if key is None else np.asarray(st[key])[0]
        if name.startswith("bins") or name == "seed_bins":
            ref = ref.reshape(64, -1).T                      # oracle NCHW -> engine [pixels, 64]
        a, b = relmax(got, ref), rell2(got, ref)
        print("  %-10s relmax %.3e relL2 %.3e" % (name, a, b))
        if name == "metric_net":
            assert a < TOL_RANGE and b < TOL_L2, name
        else:
            assert a < STAGE_RANGE and b < STAGE_L2, name
    # the Pillow resize of the engine's own network output is exact (double accumulation, float32 passes)
    from PIL import Image
    pil = np.asarray(Image.fromarray(net.stage("metric_net")[1]).resize((640, 360)))
    assert np.array_equal(depth[1], pil)
    ref = Z.pil_resize_f32(ref_net[0], 360, 640)
    print("  final      relmax %.3e relL2 %.3e  range %.2f .. %.2f m" % (relmax(depth[1], ref), rell2(depth[1], ref), ref.min(), ref.max()))
    assert relmax(depth[1], ref) < TOL_RANGE and rell2(depth[1], ref) < TOL_L2
    assert abs(mn[1] - depth[1].min()) < 1e-6 and abs(mx[1] - depth[1].max()) < 1e-6
    # not flipped: the farthest pixel is hot (heat 1 -> red), bands/depth_anything.py:150,188
    far = np.unravel_index(depth[1].argmax(), depth[1].shape)
    assert tuple(rgb[1][far]) == (255, 0, 0)


def test_metric_batch_slots_equal_single_frames(net, three):
    """three frames through a max_batch 2 context (chunks 2 + 1), then each alone: depth, rgb, min and max bit-equal - a frame's result
    depends neither on its batch slot nor on what the short chunk left behind.  With the oracle check of one batched frame above this
    covers every slot"""
    frames, d3, rgb3, mn3, mx3 = three
    assert np.isfinite(d3).all() and not np.array_equal(d3[0], d3[1]) and not np.array_equal(d3[1], d3[2])
    for i in range(3):
        d1, rgb1, mn1, mx1 = net.infer_batch(frames[i:i + 1], want_depth=True, want_rgb=True, flip=False)
        same("frame %d alone vs in the batch: depth" % i, d1[0], d3[i])
        same("frame %d alone vs in the batch: rgb" % i, rgb1[0], rgb3[i])
        same("frame %d alone vs in the batch: min / max" % i, np.stack([mn1[0], mx1[0]]), np.stack([mn3[i], mx3[i]]))


# in this order on the living context: the plan and the Pillow tap tables are rebuilt at every change of size.  1 x 1: one output pixel
# gathers the whole network map (pil_ksize(392, 1) = 1569 and pil_ksize(518, 1) = 2073 taps); 392 x 518: Pillow skips both passes
TOUR = [(360, 640), (1, 1), (7, 13), (392, 518), (1080, 1920), (600, 333), (2160, 3840), (360, 640)]


@pytest.fixture(scope="module")
def first_visit():
    return {}


def tour_call(net, H, W):
    frames = synth.frames(1 if (H, W) == (2160, 3840) else 2, H, W, seed=31)
    return frames, net.infer_batch(frames, want_depth=True, want_rgb=True, flip=False)


@pytest.mark.parametrize("step", range(len(TOUR)), ids=["%d-%dx%d" % ((i,) + s) for i, s in enumerate(TOUR)])
def test_metric_frame_sizes(net, first_visit, step):
    """per size: depth is the bytes of PIL.Image.resize (bicubic) of this call's own metric_net stage; min / max are exactly the depth's;
    rgb is the bytes of the oracle's encode of the depth, not flipped and - a second call - flipped.  The last step returns to the first
    size and must return the first visit's bytes: no plan or table carries history"""
    from PIL import Image
    H, W = TOUR[step]
    if step == len(TOUR) - 1 and not first_visit:            # (run on its own: make the first visit now)
        first_visit["out"] = tour_call(net, H, W)[1]
    frames, (depth, rgb, mn, mx) = tour_call(net, H, W)
    n = frames.shape[0]
    md = net.stage("metric_net")
    assert md.shape == (n, Z.NET_H, Z.NET_W) and np.isfinite(md).all()
    flipped = net.infer_batch(frames, want_depth=False, want_rgb=True, flip=True)[1]
    for b in range(n):
        what = "%dx%d frame %d" % (H, W, b)
        pil = np.asarray(Image.fromarray(md[b]).resize((W, H), Image.BICUBIC))
        same(what + ": depth vs PIL.Image.resize of the call's metric_net", depth[b], pil)
        same(what + ": min / max", np.stack([mn[b], mx[b]]), np.stack([depth[b].min(), depth[b].max()]))
        same(what + ": rgb vs the oracle's encode, not flipped", rgb[b], O.encode_depth_video(depth[b], flip=False)[0])
        same(what + ": rgb vs the oracle's encode, flipped", flipped[b], O.encode_depth_video(depth[b], flip=True)[0])
    if step == 0:
        first_visit["out"] = (depth, rgb, mn, mx)
    elif step == len(TOUR) - 1:
        for name, got, want in zip(("depth", "rgb", "min", "max"), (depth, rgb, mn, mx), first_visit["out"]):
            same("360x640 revisited: " + name, got, want)


def test_metric_without_depth_output(net, three):
    """want_depth=False: the frame-resolution depth lives in the engine's own scratch (full_) - the same rgb, min and max"""
    frames, d3, rgb3, mn3, mx3 = three
    depth, rgb, mn, mx = net.infer_batch(frames, want_depth=False, want_rgb=True, flip=False)
    assert depth is None
    same("want_depth=False: rgb", rgb, rgb3)
    same("want_depth=False: min", mn, mn3)
    same("want_depth=False: max", mx, mx3)


def test_metric_refusals_leave_the_context_usable(net, three):
    """a ViT-S state dict is no core for the metric head; an empty batch is refused; the living context then still gives its bytes"""
    with pytest.raises(engine._lib.PrismaBandsError, match="ViT-L core only"):
        engine.DepthAnything(synth.depth_anything_weights("vits", seed=1234), "vits", max_batch=1, metric=True)
    with pytest.raises(engine._lib.PrismaBandsError, match="bad arguments"):
        net.infer_batch(np.zeros((0,) + SMALL + (3,), np.uint8))
    frames, d3, rgb3, mn3, mx3 = three
    depth, rgb, mn, mx = net.infer_batch(frames, want_depth=True, want_rgb=True, flip=False)
    for name, got, want in zip(("depth", "rgb", "min", "max"), (depth, rgb, mn, mx), (d3, rgb3, mn3, mx3)):
        same("after the refusals: " + name, got, want)
