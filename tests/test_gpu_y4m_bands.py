"""GPU: .y4m clips through the band scripts and process.py.  A band run on a .y4m (I420 frames into the engine, I420 frames out of it, the
conversions in HIP) must leave what the same script leaves for the .npy stack of the host-converted frames, once this test has converted that
run's videos with the restatement (tests/yuv_ref.py): videos, CSVs, metadata (apart from the extension) and --subpath dumps, byte for byte,
with the blocking and with the streamed loop.  And with the two options off a context returns the bytes of a context that never saw them."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4                                   # PRISMA_BATCH=2: two chunks of frames, chunks of 2 and 1 pairs
RATE = (30000, 1001)


def _head(h, w):
    return b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % ((w, h) + RATE)


def _y4m_bytes(rgb):
    """the .y4m the writer leaves for RGB frames [n, h, w, 3]: the restatement's planes behind the header"""
    return _head(*rgb.shape[1:3]) + b"".join(b"FRAME\n" + R.rgb_to_i420(f).tobytes() for f in rgb)


@functools.lru_cache(maxsize=None)
def _source(kind):
    """(the clip's .y4m bytes, the RGB frames a host-side reader decodes from it): synthetic frames at the smallest sizes the band tests use,
    the depth clip odd in both directions (byte-path kernels, clamped chroma), the others on the 16-byte path (256) and off it (300)"""
    from prisma_amd import synth
    rgb = {"depth": lambda: synth.frames(N, 179, 301, seed=5), "flow": lambda: synth.frame_pair_sequence(N, 176, 256, seed=6),
           "mask": lambda: synth.frames(N, 180, 300, seed=5)}[kind]()
    data = _y4m_bytes(rgb)
    h, w = rgb.shape[1:3]
    decoded = np.stack([R.i420_to_rgb(R.rgb_to_i420(f), h, w) for f in rgb])
    return data, decoded


def _clip(folder, ext, kind):
    folder.mkdir()
    data, decoded = _source(kind)
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


def _tree(folder):
    out = {}
    for base, _, files in os.walk(folder):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    out["metadata.json"] = out["metadata.json"].replace(str(folder).encode(), b"<clip>")
    return out


def _as_y4m(tree, folder):
    """the tree of an .npy run as the .y4m run must have left it: every video (a top-level .npy) converted with the restatement - the source
    clip is the .y4m it was decoded from - and the extension in metadata.json"""
    out = {}
    for name, data in tree.items():
        if name == "rgba.npy":
            continue
        if name.endswith(".npy") and os.sep not in name:
            out[name[:-4] + ".y4m"] = _y4m_bytes(np.load(os.path.join(folder, name)))
        else:
            out[name] = data
    out["metadata.json"] = out["metadata.json"].replace(b".npy", b".y4m")
    return out


BANDS = {
    "depth": ("depth_anything.py", ["--encoder", "vits", "--npy", "--subpath", "depth_frames"],
              ["depth_anything.y4m", "depth_anything_min.csv", "depth_anything_max.csv", "depth_frames/00003.npy", "depth_frames/00000.png"]),
    "flow_raft": ("flow_raft.py", ["--iterations", "3", "--scale", "1.0", "-b", "--mask", "--subpath_mask", "flow_mask", "--subpath", "flow"],
                  ["flow_raft.y4m", "flow_raft_bwd.y4m", "flow_raft_mask.y4m", "flow_raft_mask_bwd.y4m", "flow_raft.csv", "flow_fwd/0002.flo",
                   "flow_mask_bwd/0003.png"]),
    "flow_gmflow": ("flow_gmflow.py", ["--scale", "1.0", "-b", "--subpath", "flow"], ["flow_gmflow.y4m", "flow_gmflow_bwd.y4m", "flow_gmflow.csv", "flow_bwd/0000.flo"]),
    "mask": ("mask_mmdet.py", ["--arch", "tiny", "--sdf"], ["mask.y4m"]),                                    # id images leave the engine as I420
    "mask_colmap": ("mask_mmdet.py", ["--arch", "tiny", "--subpath", "colmap"], ["mask.y4m", "colmap/00003.png"]),   # ... as RGB: the dump needs them
}
_baseline = {}


def _npy_baseline(tmp_path_factory, band):
    """the script's folder for the .npy stack of the host-converted frames, converted: computed once per band (blocking loop; that the streamed
    loop leaves the same .npy folder is tests/test_gpu_stream_bands.py's)"""
    if band not in _baseline:
        script, extra, _ = BANDS[band]
        folder = _clip(tmp_path_factory.mktemp("npy_" + band) / "clip", "npy", band.split("_")[0])
        _run(script, ["-i", str(folder)] + extra, 0)
        _baseline[band] = _as_y4m(_tree(folder), folder)
    return _baseline[band]


@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("band", list(BANDS))
def test_band_on_y4m_equals_band_on_npy(tmp_path, tmp_path_factory, band, stream):
    script, extra, expect = BANDS[band]
    want = _npy_baseline(tmp_path_factory, band)
    folder = _clip(tmp_path / "clip", "y4m", band.split("_")[0])
    err = _run(script, ["-i", str(folder)] + extra, stream)
    assert ("[loop] streamed: " in err) == bool(stream), err[-2000:]
    got = _tree(folder)
    assert got.pop("rgba.y4m") == _source(band.split("_")[0])[0]
    assert sorted(got) == sorted(want)
    missing = [e for e in expect + ["metadata.json"] if e not in got]
    assert not missing, (missing, sorted(got)[:40])
    for name in sorted(got):
        assert got[name] == want[name], name
    video = got[expect[0]]
    assert video.count(b"FRAME\n") >= N
    if not band.startswith("mask"):         # (an id image may well be empty on synthetic weights)
        assert len(set(video.split(b"FRAME\n")[1:N])) > 1          # frames of their own, not one buffer N times


DRIVER = """
import sys
sys.path.insert(0, %r)
import process
process.EXTRA_ARGS.update({"mask_mmdet": "--sdf --arch tiny ", "depth_anything": "--encoder vits ", "flow_gmflow": "--scale 1.0 "})
process.main(sys.argv[1:])
""" % ROOT


def test_process_jobs_3_equals_jobs_1_on_a_y4m(tmp_path):
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(_source("flow")[0])
    out, trees = str(tmp_path / "out"), []
    for jobs in ("1", "3"):
        env = dict(os.environ, PRISMA_SYNTH="1", PRISMA_OVERWRITE="1", PRISMA_BATCH="2")
        env.pop("PRISMA_GPUS", None)
        r = subprocess.run([sys.executable, "-c", DRIVER, "-i", str(clip), "-b", "--output", out, "--jobs", jobs], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
        trees.append(_tree(out))
        os.rename(out, str(tmp_path / ("jobs" + jobs)))
    a, b = trees
    for name in ("metadata.json", "rgba.y4m", "mask.y4m", "depth_anything.y4m", "depth_anything_min.csv", "flow_gmflow.y4m", "flow_gmflow_bwd.y4m",
                 "flow_gmflow.csv", "images/000003.png"):
        assert name in a, (name, sorted(a))
    assert sorted(a) == sorted(b)
    for name in sorted(a):
        assert a[name] == b[name], name
    md = json.loads(a["metadata.json"])
    assert (md["width"], md["height"], md["frames"], md["fps"]) == (256, 176, N, RATE[0] / RATE[1])
    assert md["bands"]["flow"]["url"] == "flow_gmflow.y4m" and md["bands"]["depth"]["url"] == "depth_anything.y4m"
    assert a["rgba.y4m"] == _source("flow")[0]


# ---- the options themselves, in process: on a context, then off again, against a context that never had them -------------------------------
def _make(band):
    from prisma_amd import engine, synth
    if band == "depth":
        return engine.DepthAnything(synth.depth_anything_weights("vits", seed=1234), "vits", device=0, max_batch=2)
    if band == "flow_raft":
        return engine.FlowRaft(synth.raft_weights(seed=4321), device=0)
    if band == "flow_gmflow":
        return engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0)
    cfg = synth.MASK_CFGS["tiny"]
    return engine.MaskMMDet(synth.solov2_weights(cfg), cfg, max_batch=2)


def _call(band, net, frames, size=None):
    """one existing-style call -> the list of its result arrays, the encoded frames first"""
    if band == "depth":
        depth, rgb, mn, mx = net.infer_batch(frames, size=size)
        return [rgb, depth, mn, mx]
    if band == "mask":
        return [net.infer_batch(frames, 0.5, None, size=size)]
    flow, rgb, mx, mask = net.infer_sequence_masks(frames, scale=1.0, iters=3, size=size)
    return [rgb, flow, mx, mask]


@pytest.mark.parametrize("band", ["depth", "flow_raft", "flow_gmflow", "mask"])
def test_options_on_then_off_against_a_second_context(band):
    data, decoded = _source(band.split("_")[0])
    h, w = decoded.shape[1:3]
    yuv = np.frombuffer(data, np.uint8)[len(_head(h, w)):].reshape(N, 6 + R.i420_bytes(h, w))[:, 6:].copy()     # the clip's own planes
    a, b = _make(band), _make(band)
    try:
        plain = _call(band, b, decoded)                              # the second context: never saw an option
        a.frame_format, a.rgb_format = "i420", "i420"
        both = _call(band, a, yuv, size=(h, w))
        assert both[0].shape[-1] == R.i420_bytes(*plain[0].shape[-3:-1]) and both[0].ndim == plain[0].ndim - 2
        assert both[0].tobytes() == R.rgb_to_i420(plain[0]).tobytes(), "rgb_out_i420"
        for x, y in zip(both[1:], plain[1:]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        with pytest.raises(AssertionError):
            _call(band, a, decoded)                                   # RGB frames on an I420 context: refused by the shape check
        a.rgb_format = "rgb"
        one = _call(band, a, yuv, size=(h, w))                        # each side by its own option
        for x, y in zip(one, plain):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        a.frame_format = "rgb"
        assert (a.frame_format, a.rgb_format) == ("rgb", "rgb")
        off = _call(band, a, decoded)
        for x, y in zip(off, plain):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        if band != "mask":                  # (an id image may well be empty on synthetic weights)
            assert plain[0].any() and len(np.unique(plain[0].reshape(len(plain[0]), -1), axis=0)) > 1
    finally:
        a.close()
        b.close()
