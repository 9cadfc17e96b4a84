"""GPU: .y4m clips of other layouts than 8-bit 4:2:0 through the band scripts (the pattern of tests/test_gpu_y4m_bands.py).  A band run on the
.y4m - the clip's planes into the engine as they are in the file, converted in HIP (pb_set_frame_format) - must leave, byte for byte, what the
same script leaves for the .npy stack of the frames the restatement (tests/yuv_fmt_ref.py) decodes from that clip, once this test has converted
that run's videos to .y4m with tests/yuv_ref.py: videos, CSVs and metadata (apart from the extension)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_fmt_ref as F  # noqa: E402
import yuv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4                                   # PRISMA_BATCH=2: two chunks of frames, chunks of 2 and 1 pairs
RATE = (30000, 1001)

# band -> (script, its arguments, the clip's header tokens, its format, the environment's matrix, the smallest size of the band tests, the loops)
CASES = {
    "depth": ("depth_anything.py", ["--encoder", "vits"], "C422p10 XCOLORRANGE=FULL", (422, 10, True, "bt709"), "bt709", (179, 301), (0, 1)),
    "flow": ("flow_gmflow.py", ["--scale", "1.0", "-b"], "C444", (444, 8, False, "bt601"), None, (176, 256), (0,)),
    "mask": ("mask_mmdet.py", ["--arch", "tiny"], "Cmono12", (400, 12, False, "bt601"), None, (180, 300), (0,)),
}
EXPECT = {"depth": ["depth_anything.y4m", "depth_anything_min.csv", "depth_anything_max.csv"], "flow": ["flow_gmflow.y4m", "flow_gmflow_bwd.y4m", "flow_gmflow.csv"],
          "mask": ["mask.y4m"]}


def _out_head(h, w):
    return b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % ((w, h) + RATE)


def _as_planes(fmt, rgb):
    """planes of layout `fmt` that look like the RGB frames [n, h, w, 3]: a plain real-valued forward conversion, chroma of the block's first
    pixel - any planes are a valid clip, these only keep the picture a picture"""
    chroma, d, full, m = fmt
    kr, kb = (float(k) for k in F.K[m])
    v = rgb.astype(np.float64) / 255.0
    y = kr * v[..., 0] + (1 - kr - kb) * v[..., 1] + kb * v[..., 2]
    cb, cr = (v[..., 2] - y) / (2 * (1 - kb)), (v[..., 0] - y) / (2 * (1 - kr))
    top = 2 ** d - 1
    if full:
        q = [y * top, cb * top + 2 ** (d - 1), cr * top + 2 ** (d - 1)]
    else:
        q = [(16 + 219 * y) * 2 ** (d - 8), (128 + 224 * cb) * 2 ** (d - 8), (128 + 224 * cr) * 2 ** (d - 8)]
    q = [np.clip(np.rint(p), 0, top).astype(np.int64) for p in q]
    if chroma == 400:
        return F.pack(fmt, q[0])
    sx, sy = F.SUB[chroma]
    return F.pack(fmt, q[0], q[1][:, ::2 ** sy, ::2 ** sx], q[2][:, ::2 ** sy, ::2 ** sx])


@functools.lru_cache(maxsize=None)
def _source(band):
    """(the clip's .y4m bytes, the RGB frames the restatement decodes from it)"""
    from prisma_amd import synth
    _, _, tokens, fmt, _, (h, w), _ = CASES[band]
    rgb = synth.frame_pair_sequence(N, h, w, seed=6) if band == "flow" else synth.frames(N, h, w, seed=5)
    planes = _as_planes(fmt, rgb)
    assert planes.shape == (N, F.frame_bytes(fmt, h, w))
    data = (b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 " % ((w, h) + RATE)) + tokens.encode() + b"\n" + b"".join(b"FRAME\n" + p.tobytes() for p in planes)
    decoded = F.to_rgb(fmt, planes, h, w)
    assert len(np.unique(decoded.reshape(N, -1), axis=0)) == N          # frames of their own
    return data, decoded


def _clip(folder, ext, band):
    folder.mkdir()
    data, decoded = _source(band)
    if ext == "y4m":
        (folder / "rgba.y4m").write_bytes(data)
    else:
        np.save(folder / "rgba.npy", decoded)
    (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba." + ext}}}))
    return folder


def _run(script, args, stream, matrix, timeout=240):
    env = dict(os.environ, PRISMA_SYNTH="1", PRISMA_OVERWRITE="1", PRISMA_BATCH="2", PRISMA_RING_SLOTS="2", PRISMA_STREAM=str(stream), PRISMA_STREAM_LOG="1")
    env.pop("PRISMA_Y4M_MATRIX", None)
    if matrix:
        env["PRISMA_Y4M_MATRIX"] = matrix
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
    """the tree of an .npy run as the .y4m run must have left it: every video (a top-level .npy) as the writer writes it, and the extension"""
    out = {}
    for name, data in tree.items():
        if name == "rgba.npy":
            continue
        if name.endswith(".npy") and os.sep not in name:
            rgb = np.load(os.path.join(folder, name))
            out[name[:-4] + ".y4m"] = _out_head(*rgb.shape[1:3]) + b"".join(b"FRAME\n" + R.rgb_to_i420(f).tobytes() for f in rgb)
        else:
            out[name] = data
    out["metadata.json"] = out["metadata.json"].replace(b".npy", b".y4m")
    return out


_baseline = {}


def _npy_baseline(tmp_path_factory, band):
    if band not in _baseline:
        script, extra = CASES[band][:2]
        folder = _clip(tmp_path_factory.mktemp("npy_" + band) / "clip", "npy", band)
        _run(script, ["-i", str(folder)] + extra, 0, None)
        _baseline[band] = _as_y4m(_tree(folder), folder)
    return _baseline[band]


@pytest.mark.parametrize("band,stream", [(b, s) for b in CASES for s in CASES[b][6]])
def test_band_on_a_y4m_of_another_layout_equals_band_on_npy(tmp_path, tmp_path_factory, band, stream):
    script, extra, _, _, matrix, _, _ = CASES[band]
    want = _npy_baseline(tmp_path_factory, band)
    folder = _clip(tmp_path / "clip", "y4m", band)
    err = _run(script, ["-i", str(folder)] + extra, stream, matrix)
    assert ("[loop] streamed: " in err) == bool(stream), err[-2000:]
    got = _tree(folder)
    assert got.pop("rgba.y4m") == _source(band)[0]
    assert sorted(got) == sorted(want)
    missing = [e for e in EXPECT[band] + ["metadata.json"] if e not in got]
    assert not missing, (missing, sorted(got)[:40])
    for name in sorted(got):
        assert got[name] == want[name], name
    video = got[EXPECT[band][0]]
    assert video.count(b"FRAME\n") >= N - (band == "flow")
    if band != "mask":                      # (an id image may well be empty on synthetic weights)
        assert len(set(video.split(b"FRAME\n")[1:N])) > 1
