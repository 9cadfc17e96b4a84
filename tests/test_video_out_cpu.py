"""CPU: PRISMA_VIDEO_OUT / process.py --video_out - its grammar and refusals, the file names the bands resolve with and without it, the band
preamble's refusal before a model loads, the layout the engines are asked for, and process.py's command lines, which do not change."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import process  # noqa: E402
import yuv_ref as R  # noqa: E402
from bands.common import cli, io as cio, loop, meta  # noqa: E402

H, W, N = 34, 50, 3


@pytest.fixture(autouse=True)
def _unset(monkeypatch):
    for k in ("PRISMA_VIDEO_OUT", "PRISMA_Y4M_OUT"):
        monkeypatch.setenv(k, "")       # recorded, so that what process.main(--video_out) leaves in os.environ is undone after the test
        monkeypatch.delenv(k)


@pytest.mark.parametrize("value,want", [
    ("avi", ("avi", 90, 444)), ("mjpeg", ("mjpeg", 90, 444)), ("avi,q=75", ("avi", 75, 444)), ("mjpeg,420", ("mjpeg", 90, 420)),
    ("avi,mono,q=100", ("avi", 100, 400)), ("avi,q=1,444", ("avi", 1, 444))])
def test_grammar(monkeypatch, value, want):
    monkeypatch.setenv("PRISMA_VIDEO_OUT", value)
    assert tuple(meta.video_out()) == want
    assert cio.planar_out("x." + want[0]) == (want[2], 8, True, "bt601")


def test_unset_is_none(monkeypatch):
    assert meta.video_out() is None
    monkeypatch.setenv("PRISMA_VIDEO_OUT", "")
    assert meta.video_out() is None
    assert cio.planar_out("x.avi") == (444, 8, True, "bt601") and cio.planar_out("x.npy") is None and cio.planar_out("x.y4m") == (420, 8, False, "bt601")


@pytest.mark.parametrize("value", ["mp4", "AVI", "avi,", "avi,q=0", "avi,q=101", "avi,q=", "avi,q=9x", "avi,422", "avi,444,420", "avi,q=50,q=60",
                                   "y4m", ",avi", "avi;q=50"])
def test_refusals(monkeypatch, value):
    monkeypatch.setenv("PRISMA_VIDEO_OUT", value)
    with pytest.raises(RuntimeError, match="PRISMA_VIDEO_OUT"):
        meta.video_out()
    # the band preamble refuses it before anything else happens - no model is loaded, no rank is set up
    args = types.SimpleNamespace(input="/nowhere/clip.npy", output="")
    with pytest.raises(SystemExit, match="PRISMA_VIDEO_OUT"):
        cli.begin(args, "depth_anything")
    with pytest.raises(SystemExit):
        process.main(["-i", "/nowhere/clip.npy"])
    monkeypatch.delenv("PRISMA_VIDEO_OUT")
    with pytest.raises(SystemExit):
        process.main(["-i", "/nowhere/clip.npy", "--video_out", value])
    assert "PRISMA_VIDEO_OUT" not in os.environ             # a refused option leaves the environment as it was


def test_is_video_knows_both():
    assert meta.is_video("a/depth.avi") and meta.is_video("a/depth.mjpeg") and meta.is_video("a.y4m") and not meta.is_video("a.png")
    assert cio.is_mjpeg("x.avi") and cio.is_mjpeg("x.mjpeg") and not cio.is_mjpeg("x.y4m") and cio.is_planar("x.y4m") and not cio.is_planar("x.npy")


DERIVED = ("mask", "depth_anything", "depth_zoedepth", "flow_raft", "flow_raft_mask", "flow_gmflow", "flow_gmflow_mask")


@pytest.mark.parametrize("clip_ext", ("y4m", "npy", "mp4"))
def test_get_target_names(monkeypatch, tmp_path, clip_ext):
    clip = str(tmp_path / ("rgba." + clip_ext))
    for band in DERIVED:        # unset: what it is today
        assert meta.get_target(clip, None, band=band, force_extension="png") == str(tmp_path / (band + "." + clip_ext))
    for value, ext in (("avi", "avi"), ("mjpeg,q=80,420", "mjpeg")):
        monkeypatch.setenv("PRISMA_VIDEO_OUT", value)
        data = {"bands": {}}
        for band in DERIVED:
            assert meta.get_target(clip, data, band=band, force_extension="png") == str(tmp_path / (band + "." + ext))
            assert data["bands"][band]["url"] == band + "." + ext           # metadata.json names the new file
        assert meta.get_target(clip, data, band="rgba") == clip               # rgba keeps the clip's container
        assert meta.get_target(clip, None, band="depth_anything", force_extension="csv").endswith("depth_anything.csv")
        # a still image is not a video band
        assert meta.get_target(str(tmp_path / "rgba.png"), None, band="mask", force_extension="png") == str(tmp_path / "mask.png")
        assert meta.band_video_ext(clip) == ext and meta.band_video_ext("x.png") == "png"


def test_begin_names_the_outputs(monkeypatch, tmp_path):
    """the band preamble on a bare file and on a PRISMA folder: <band>.avi beside the clip, and the flow bands' mask file"""
    monkeypatch.setenv("PRISMA_VIDEO_OUT", "avi")
    monkeypatch.setenv("PRISMA_OVERWRITE", "1")
    clip = tmp_path / "clip.npy"
    np.save(clip, np.zeros((2, 8, 8, 3), np.uint8))
    args = types.SimpleNamespace(input=str(clip), output="")
    cli.begin(args, "depth_anything")[3].close()
    assert args.output == str(tmp_path / "depth_anything.avi") and args.input == str(clip)
    folder = tmp_path / "f"
    folder.mkdir()
    json.dump({"bands": {"rgba": {"url": "rgba.npy"}}}, open(folder / "metadata.json", "w"))
    args = types.SimpleNamespace(input=str(folder), output="", mask=True, subpath="", subpath_mask="", backwards=True)
    data, _, _, rk = cli.begin(args, "flow_raft", flow=True)
    rk.close()
    assert args.output == str(folder / "flow_raft.avi") and args.output_mask == str(folder / "flow_raft_mask.avi")
    assert args.input == str(folder / "rgba.npy")
    assert data["bands"]["flow_raft"]["url"] == "flow_raft.avi"


def test_frame_formats_asks_for_the_jpegs_planes(monkeypatch):
    """common/loop.py hands the JPEG's layout to the engine through rgb_format, as it does a .y4m's"""
    monkeypatch.setenv("PRISMA_VIDEO_OUT", "mjpeg,420")
    m = types.SimpleNamespace(frame_format="rgb", rgb_format="rgb")
    kw = loop.frame_formats(m, False, cio.is_planar("depth.mjpeg"), 8, 10, None, cio.planar_out("depth.mjpeg"))
    assert kw == {"size": (8, 10)} and m.frame_format == "rgb" and m.rgb_format == (420, 8, True, "bt601")
    m = types.SimpleNamespace(frame_format="rgb", rgb_format="rgb")
    assert loop.frame_formats(m, False, cio.is_planar("depth.npy"), 8, 10, None, cio.planar_out("depth.npy")) == {} and m.rgb_format == "rgb"


def _clip(tmp_path):
    rgb = np.random.default_rng(5).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    p = tmp_path / "clip.y4m"
    with open(p, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (W, H))
        for fr in rgb:
            f.write(b"FRAME\n" + R.rgb_to_i420(fr).tobytes())
    return p


def _run_process(monkeypatch, tmp_path, sub, extra):
    real = subprocess.run
    seen = []

    def fake(cmd, **kw):
        seen.append(os.environ.get("PRISMA_VIDEO_OUT"))
        if os.path.basename(cmd[1]) == "rgba.py":
            return real(cmd, **kw)
        return subprocess.CompletedProcess(cmd, 0)
    monkeypatch.setattr(process.subprocess, "run", fake)
    d = tmp_path / sub
    d.mkdir()
    clip = _clip(d)
    folder = process.main(["-i", str(clip), "-b", "-m"] + extra)
    rel = lambda c: [a.replace(str(d), "<d>") for a in c[1:]]      # noqa: E731
    return folder, [rel(c) for c in process.COMMANDS], seen


def test_process_commands_do_not_change(monkeypatch, tmp_path):
    """process.py builds the argv it builds today - unset, and set too: the selection travels in the environment"""
    folder, plain, seen = _run_process(monkeypatch, tmp_path, "a", [])
    assert seen and all(v is None for v in seen)
    assert [os.path.basename(c[0]) for c in plain] == ["rgba.py", "mask_mmdet.py", "depth_anything.py", "flow_gmflow.py"]
    assert plain[0][1:] == ["-i", "<d>/clip.y4m", "--output", "<d>/clip/rgba.y4m", "--fps", "24", "--subpath", "images"]
    assert plain[1][1:] == ["-i", "<d>/clip", "--sdf", "--subpath", "mask"] and plain[2][1:] == ["-i", "<d>/clip", "--metric", "outdoor"]
    assert plain[3][1:] == ["-i", "<d>/clip", "--backwards", "--mask"]
    folder2, with_avi, seen2 = _run_process(monkeypatch, tmp_path, "b", ["--video_out", "avi,q=85"])
    assert with_avi == plain and all(v == "avi,q=85" for v in seen2)
    md = json.load(open(os.path.join(folder2, "metadata.json")))
    assert md["bands"]["rgba"]["url"] == "rgba.y4m" and os.path.exists(os.path.join(folder2, "rgba.y4m"))
    src = meta.get_url(folder2, md, "rgba")
    assert meta.get_target(src, md, band="depth_anything", force_extension="png") == os.path.join(folder2, "depth_anything.avi")


def test_writer_takes_quality_and_layout_from_the_selection(monkeypatch, tmp_path):
    monkeypatch.setenv("PRISMA_VIDEO_OUT", "mjpeg,q=77,420")
    w = cio.VideoWriter(8, 8, 24, str(tmp_path / "v.mjpeg"), encoder=lambda p, *a: [b"\xff\xd8\xff\xd9"] * len(p))
    assert (w.quality, tuple(w.format)) == (77, (420, 8, True, "bt601"))
    w.close()
    w = cio.VideoWriter(8, 8, 24, str(tmp_path / "v.avi"), quality=60, fmt=cio.jpeg_format(400), encoder=lambda p, *a: [b"\xff\xd8\xff\xd9"] * len(p))
    assert (w.quality, tuple(w.format)) == (60, (400, 8, True, "bt601"))      # what the caller names wins
    w.close()
