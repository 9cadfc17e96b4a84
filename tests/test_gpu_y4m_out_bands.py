"""GPU: the band scripts writing .y4m videos in another layout than 8-bit 4:2:0 (PRISMA_Y4M_OUT; the pattern of tests/test_gpu_y4m_formats_bands.py).
A band run on a .y4m clip leaves videos whose header names the layout and whose frames are, byte for byte, the restatement's conversion
(tests/yuv_out_ref.py) of the RGB frames the same script leaves as a .npy stack for the .npy stack of the clip's decoded frames - for the flow
bands at --scale 0.75 of those frames resized to the clip's size (tests/resize_ref.py).  Read back through FrameReader a C444p12,full video
returns those RGB frames exactly, and so does a Cmono,full video of the mask band's grey id images."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))
import resize_ref as Z  # noqa: E402
import yuv_fmt_ref as F  # noqa: E402
import yuv_out_ref as O  # noqa: E402
import yuv_ref as R  # noqa: E402
from common import io  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4                                   # PRISMA_BATCH=2: two chunks of frames, chunks of 2 and 1 pairs
RATE = (30000, 1001)

# band -> (script, its arguments, the clip: kind and the smallest size of the band tests, the videos it writes)
BANDS = {
    "depth": ("depth_anything.py", ["--encoder", "vits"], ("frames", 179, 301), ["depth_anything"]),
    "flow_raft": ("flow_raft.py", ["--iterations", "3", "--scale", "0.75", "-b"], ("pairs", 176, 256), ["flow_raft", "flow_raft_bwd"]),
    "flow_gmflow": ("flow_gmflow.py", ["--scale", "0.75", "-b"], ("pairs", 176, 256), ["flow_gmflow", "flow_gmflow_bwd"]),
    "mask": ("mask_mmdet.py", ["--arch", "tiny"], ("frames", 180, 300), ["mask"]),
}
# (band, PRISMA_Y4M_OUT, the format it names, the header's tokens)
LOSSLESS = ("C444p12,full", (444, 12, True, "bt601"), b"C444p12 XCOLORRANGE=FULL")
GREY = ("Cmono,full", (400, 8, True, "bt601"), b"Cmono XCOLORRANGE=FULL")
CASES = [(b,) + LOSSLESS for b in BANDS] + [("mask",) + GREY]


@functools.lru_cache(maxsize=None)
def _source(band):
    """(the clip's .y4m bytes - plain 8-bit 4:2:0 -, the RGB frames a reader decodes from it)"""
    from prisma_amd import synth
    kind, h, w = BANDS[band][2]
    rgb = synth.frame_pair_sequence(N, h, w, seed=6) if kind == "pairs" else synth.frames(N, h, w, seed=5)
    head = b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % ((w, h) + RATE)
    planes = [R.rgb_to_i420(f) for f in rgb]
    return head + b"".join(b"FRAME\n" + p.tobytes() for p in planes), np.stack([R.i420_to_rgb(p, h, w) for p in planes])


def _clip(folder, ext, band):
    folder.mkdir()
    data, decoded = _source(band)
    if ext == "y4m":
        (folder / "rgba.y4m").write_bytes(data)
    else:
        np.save(folder / "rgba.npy", decoded)
    (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba." + ext}}}))
    return folder


def _run(script, args, stream, y4m_out, timeout=240):
    env = dict(os.environ, PRISMA_SYNTH="1", PRISMA_OVERWRITE="1", PRISMA_BATCH="2", PRISMA_RING_SLOTS="2", PRISMA_STREAM=str(stream), PRISMA_STREAM_LOG="1")
    env.pop("PRISMA_Y4M_MATRIX", None)
    env.pop("PRISMA_Y4M_OUT", None)
    if y4m_out:
        env["PRISMA_Y4M_OUT"] = y4m_out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bands", script)] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stderr


_baseline = {}


def _npy_frames(tmp_path_factory, band):
    """{video: the RGB frames [n, h, w, 3] the script leaves for the .npy stack of the clip's frames, at the clip's size}: once per band"""
    if band not in _baseline:
        script, extra, (_, h, w), videos = BANDS[band]
        folder = _clip(tmp_path_factory.mktemp("npy_" + band) / "clip", "npy", band)
        _run(script, ["-i", str(folder)] + extra, 0, None)
        out = {}
        for v in videos:
            rgb = np.load(os.path.join(folder, v + ".npy"))
            assert rgb.dtype == np.uint8 and rgb.shape[0] == N and rgb.shape[3] == 3
            if band.startswith("flow"):
                assert rgb.shape[1:3] != (h, w)                           # --scale 0.75: the band's frames are smaller than the clip's
                rgb = Z.resize(rgb, h, w)                                 # ... and a video of the clip's size holds them resized
            out[v] = rgb
        _baseline[band] = out
    return _baseline[band]


def _frames_of(data, head, fb):
    assert data.startswith(head), data[:100]
    body = data[len(head):]
    assert len(body) == N * (6 + fb), (len(body), fb)
    recs = [body[i * (6 + fb):(i + 1) * (6 + fb)] for i in range(N)]
    assert all(r.startswith(b"FRAME\n") for r in recs)
    return np.stack([np.frombuffer(r[6:], np.uint8) for r in recs])


@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("band,y4m_out,fmt,tokens", CASES, ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_band_writes_the_named_layout(tmp_path, tmp_path_factory, monkeypatch, band, y4m_out, fmt, tokens, stream):
    script, extra, (_, h, w), videos = BANDS[band]
    want = _npy_frames(tmp_path_factory, band)
    folder = _clip(tmp_path / "clip", "y4m", band)
    err = _run(script, ["-i", str(folder)] + extra, stream, y4m_out)
    assert ("[loop] streamed: " in err) == bool(stream), err[-2000:]
    head = b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 " % ((w, h) + RATE) + tokens + b"\n"
    monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    for v in videos:
        rgb = want[v]
        path = os.path.join(folder, v + ".y4m")
        got = _frames_of(open(path, "rb").read(), head, F.frame_bytes(fmt, h, w))
        ref = O.rgb_to_yuv(fmt, rgb)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), (v, int((got != ref).sum()))
        reader = io.FrameReader(path)
        assert tuple(reader.format) == fmt and len(reader) == N
        back = np.stack([reader[i] for i in range(N)])
        assert np.array_equal(back, rgb), v                               # lossless: what the band produced, byte for byte
    if band != "mask":                      # (an id image may well be empty on synthetic weights)
        assert len(np.unique(want[videos[0]][:N - 1].reshape(N - 1, -1), axis=0)) > 1


def test_mask_id_images_are_grey(tmp_path_factory):
    """what makes Cmono,full lossless for the mask band: the same byte in all three channels"""
    rgb = _npy_frames(tmp_path_factory, "mask")["mask"]
    assert (rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 0] == rgb[..., 2]).all()


def test_nothing_set_writes_what_it_always_wrote(tmp_path, tmp_path_factory):
    """the default's guard: with PRISMA_Y4M_OUT unset the file is the I420 writer's, byte for byte (tests/yuv_ref.py)"""
    script, extra, (_, h, w), videos = BANDS["depth"]
    want = _npy_frames(tmp_path_factory, "depth")
    folder = _clip(tmp_path / "clip", "y4m", "depth")
    _run(script, ["-i", str(folder)] + extra, 0, None)
    head = b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % ((w, h) + RATE)
    data = open(os.path.join(folder, videos[0] + ".y4m"), "rb").read()
    assert data == head + b"".join(b"FRAME\n" + R.rgb_to_i420(f).tobytes() for f in want[videos[0]])
