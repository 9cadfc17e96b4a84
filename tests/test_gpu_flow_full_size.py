"""GPU: the flow bands at --scale 0.75 write .y4m videos of the clip's size.  The engines' rgb_full option ("rgb_out_full": the encoded frames
resized on the GPU to the clip's H x W, RGB or straight to I420) must give, byte for byte, the restated resize (tests/resize_ref.py) of the
sh x sw frames the same call gives without it - blocking, with masks, and through submit / wait - and change nothing at --scale 1.0.  The band
scripts on a .y4m clip must leave videos with the clip's size in their headers whose frames are that restatement of the frames their .npy run
leaves, with the blocking and with the streamed loop, and process.py's folder must hold no video of another size than metadata.json records."""
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref  # noqa: E402
import yuv_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N, H, W = 4, 176, 256                   # PRISMA_BATCH=2: chunks of 2 and 1 pairs
SH, SW = 132, 192                       # the bands' size at --scale 0.75
SCALE, ITERS = 0.75, 3
RATE = (30000, 1001)


def _head(h, w):
    return b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % ((w, h) + RATE)


@functools.lru_cache(maxsize=None)
def _source():
    """(the clip's .y4m bytes, the RGB frames a host-side reader decodes from it)"""
    from prisma_amd import synth
    rgb = synth.frame_pair_sequence(N, H, W, seed=6)
    data = _head(H, W) + b"".join(b"FRAME\n" + yuv_ref.rgb_to_i420(f).tobytes() for f in rgb)
    decoded = np.stack([yuv_ref.i420_to_rgb(yuv_ref.rgb_to_i420(f), H, W) for f in rgb])
    decoded.setflags(write=False)
    return data, decoded


def _make(band):
    from prisma_amd import engine, synth
    if band == "flow_raft":
        return engine.FlowRaft(synth.raft_weights(seed=4321), device=0)
    return engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0)


def _same(what, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s" % (what, len(bad), want.size, tuple(bad[0])))


@pytest.mark.parametrize("band", ["flow_raft", "flow_gmflow"])
def test_rgb_full_is_the_resize_of_the_bands_own_frames(band):
    from prisma_amd import engine
    frames = _source()[1]
    assert engine.flow_out_size(H, W, SCALE) == (SH, SW)
    net = _make(band)
    try:
        assert net.rgb_full is False
        flow, rgb, mx = net.infer_sequence(frames, scale=SCALE, iters=ITERS, backward=True)
        mflow, mrgb, mmx, mask = net.infer_sequence_masks(frames, scale=SCALE, iters=ITERS)
        assert rgb.shape == (N - 1, 2, SH, SW, 3) and rgb.any() and len({p.tobytes() for p in rgb.reshape(-1, SH * SW * 3)}) > 1
        want_rgb, want_yuv = resize_ref.resize(rgb, H, W), resize_ref.resize_i420(rgb, H, W)
        want_mrgb, want_myuv = resize_ref.resize(mrgb, H, W), resize_ref.resize_i420(mrgb, H, W)
        net.rgb_full = True
        assert net.rgb_full is True
        for fmt, want, mwant in (("rgb", want_rgb, want_mrgb), ("i420", want_yuv, want_myuv)):
            net.rgb_format = fmt
            f2, r2, m2 = net.infer_sequence(frames, scale=SCALE, iters=ITERS, backward=True)
            _same(fmt + " frames", r2, want)
            _same("flow", f2, flow)                              # every other output stays at sh x sw, untouched
            _same("max displacement", m2, mx)
            f3, r3, m3, k3 = net.infer_sequence_masks(frames, scale=SCALE, iters=ITERS)
            _same(fmt + " frames, masks call", r3, mwant)
            _same("flow, masks call", f3, mflow)
            _same("max displacement, masks call", m3, mmx)
            _same("masks", k3, mask)
            # forward only: one direction per pair
            _, r4, _ = net.infer_sequence(frames, scale=SCALE, iters=ITERS, backward=False, want_flow=False)
            _same(fmt + " frames, forward only", r4, want[:, :1])
            # submit / wait on page-locked arrays: the bytes of the blocking call
            fr = net.host_empty(frames.shape, np.uint8)
            fr[...] = frames
            out = {"rgb": net.host_empty(want.shape, np.uint8), "flow": net.host_empty(flow.shape, np.float32), "mx": net.host_empty(mx.shape, np.float32),
                   "mask": net.host_empty(mask.shape, np.uint8)}
            net.submit_sequence(fr, scale=SCALE, iters=ITERS, backward=True, out_flow=out["flow"], out_rgb=out["rgb"], out_max=out["mx"])
            f5, r5, m5 = net.wait()
            _same(fmt + " frames, submit", r5, want)
            _same("flow, submit", f5, flow)
            net.submit_sequence_masks(fr, scale=SCALE, iters=ITERS, out_flow=out["flow"], out_rgb=out["rgb"], out_max=out["mx"], out_mask=out["mask"])
            f6, r6, m6, k6 = net.wait()
            _same(fmt + " frames, masks submit", r6, mwant)
            _same("masks, submit", k6, mask)
            with pytest.raises(AssertionError):                   # an array of the band's size is refused by the shape check
                net.infer_sequence(frames, scale=SCALE, iters=ITERS, backward=True, out_rgb=np.empty(rgb.shape, np.uint8))
            for a in [fr] + list(out.values()):
                net.host_free(a)
        # off again: the call of a context that never saw the option
        net.rgb_full, net.rgb_format = False, "rgb"
        _, r7, _ = net.infer_sequence(frames, scale=SCALE, iters=ITERS, backward=True, want_flow=False)
        _same("option off again", r7, rgb)
    finally:
        net.close()


@pytest.mark.parametrize("band", ["flow_raft", "flow_gmflow"])
def test_rgb_full_changes_nothing_at_scale_one(band):
    frames = _source()[1]
    net = _make(band)
    try:
        plain = net.infer_sequence_masks(frames, scale=1.0, iters=ITERS)
        assert plain[1].shape == (N - 1, 2, H, W, 3)
        net.rgb_full = True
        full = net.infer_sequence_masks(frames, scale=1.0, iters=ITERS)
        for x, y in zip(full, plain):
            _same("scale 1.0", x, y)
        net.rgb_format = "i420"
        _same("scale 1.0, I420", net.infer_sequence_masks(frames, scale=1.0, iters=ITERS)[1], yuv_ref.rgb_to_i420(plain[1]))
    finally:
        net.close()


# ---- the band scripts ----------------------------------------------------------------------------------------------------------------------
def _clip(folder, ext):
    folder.mkdir()
    data, decoded = _source()
    if ext == "y4m":
        (folder / "rgba.y4m").write_bytes(data)
    else:
        np.save(folder / "rgba.npy", decoded)
    (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba." + ext}}}))
    return folder


def _run(script, args, stream, timeout=240):
    env = dict(os.environ, PRISMA_SYNTH="1", PRISMA_OVERWRITE="1", PRISMA_BATCH="2", PRISMA_RING_SLOTS="2", PRISMA_STREAM=str(stream), PRISMA_STREAM_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bands", script)] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stderr


BANDS = {"flow_raft": ("flow_raft.py", ["--iterations", str(ITERS), "-b", "--mask", "--subpath", "flow"]),
         "flow_gmflow": ("flow_gmflow.py", ["-b", "--mask", "--subpath", "flow"])}
VIDEOS = ("", "_bwd", "_mask", "_mask_bwd")
_baseline = {}


def _npy_frames(tmp_path_factory, band):
    """the sh x sw frames of the band's four videos and its other files: the script on the .npy stack of the decoded frames, default --scale,
    once per band (a .npy stack keeps the band's own size)"""
    if band not in _baseline:
        script, extra = BANDS[band]
        folder = _clip(tmp_path_factory.mktemp("npy_" + band) / "clip", "npy")
        _run(script, ["-i", str(folder)] + extra, 0)
        videos = {v: np.load(str(folder / (band + v + ".npy"))) for v in VIDEOS}
        for v in videos.values():
            assert v.shape == (N, SH, SW, 3), v.shape
        others = {name: (folder / name).read_bytes() for name in (band + ".csv", "flow_fwd/0000.flo", "flow_bwd/0002.flo", "flow_fwd/0003.flo")}
        _baseline[band] = (videos, others)
    return _baseline[band]


@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("band", list(BANDS))
def test_band_writes_videos_of_the_clips_size(tmp_path, tmp_path_factory, band, stream):
    script, extra = BANDS[band]
    videos, others = _npy_frames(tmp_path_factory, band)
    folder = _clip(tmp_path / "clip", "y4m")
    err = _run(script, ["-i", str(folder)] + extra, stream)
    assert ("[loop] streamed: " in err) == bool(stream), err[-2000:]
    fb = yuv_ref.i420_bytes(H, W)
    black = np.concatenate([np.full(H * W, 16, np.uint8), np.full(fb - H * W, 128, np.uint8)]).tobytes()
    for v in VIDEOS:
        data = (folder / (band + v + ".y4m")).read_bytes()
        assert data.startswith(_head(H, W)), (v, data[:80])                  # W256 H176, the clip's
        body = data[len(_head(H, W)):]
        assert len(body) == N * (6 + fb), (v, len(body))                     # the clip's frame count
        for i in range(N):
            rec = body[i * (6 + fb):(i + 1) * (6 + fb)]
            assert rec[:6] == b"FRAME\n"
            assert rec[6:] == resize_ref.resize_i420(videos[v][i], H, W).tobytes(), (v, i)
        assert body[-fb:] == black, v                                        # the trailing zero-flow frame
        assert len({body[i * (6 + fb):(i + 1) * (6 + fb)] for i in range(N - 1)}) > (1 if "mask" not in v else 0)
    for name, want in others.items():                                        # dumps and the CSV do not change: the band's own size
        assert (folder / name).read_bytes() == want, name
    flo = (folder / "flow_fwd/0000.flo").read_bytes()
    assert np.frombuffer(flo[4:12], np.int32).tolist() == [SW, SH] and len(flo) == 12 + SH * SW * 8


DRIVER = """
import sys
sys.path.insert(0, %r)
import process
process.EXTRA_ARGS.update({"mask_mmdet": "--sdf --arch tiny ", "depth_anything": "--encoder vits "})
process.main(sys.argv[1:])
""" % ROOT


def test_process_folder_holds_videos_of_one_size(tmp_path):
    """process.py on a .y4m clip, the flow band at its default --scale 0.75: every video of the folder has the size metadata.json records"""
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(_source()[0])
    out = str(tmp_path / "out")
    env = dict(os.environ, PRISMA_SYNTH="1", PRISMA_OVERWRITE="1", PRISMA_BATCH="2")
    env.pop("PRISMA_GPUS", None)
    r = subprocess.run([sys.executable, "-c", DRIVER, "-i", str(clip), "-b", "--output", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    md = json.load(open(os.path.join(out, "metadata.json")))
    assert (md["width"], md["height"], md["frames"]) == (W, H, N)
    found = sorted(glob.glob(os.path.join(out, "*.y4m")))
    names = [os.path.basename(p) for p in found]
    for name in ("rgba.y4m", "mask.y4m", "depth_anything.y4m", "flow_gmflow.y4m", "flow_gmflow_bwd.y4m"):
        assert name in names, (name, names)
    for p in found:
        head = open(p, "rb").readline().split()
        assert (head[1], head[2]) == (b"W%d" % md["width"], b"H%d" % md["height"]), (p, head)
        assert os.path.getsize(p) == len(b" ".join(head)) + 1 + md["frames"] * (6 + yuv_ref.i420_bytes(H, W)), p
