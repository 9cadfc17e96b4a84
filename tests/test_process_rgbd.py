"""process.py --record3d / --rgbd (reference process.py:124-172, 243): the rgba band's arguments, the capture's intrinsics and depth range in
metadata.json, and the `depth` alias that must stay with the measured half.  CPU: the band subprocesses are replaced by a recorder that
writes rgba.npy / depth.npy stand-ins.  GPU: the same run with the real rgba band."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import process  # noqa: E402

import rgbd_ref as R  # noqa: E402

# Record3D's `movie_more` tag: the intrinsic matrix is column major, so fx = m[0], fy = m[4], cx = m[6], cy = m[7]
SIDECAR = {"intrinsicMatrix": [590.5, 0.0, 0.0, 0.0, 592.25, 0.0, 3.25, 4.5, 1.0], "rangeOfEncodedDepth": [0.25, 3.0]}
H, W = 8, 12


def capture(tmp_path, sidecar=True):
    fr = R.make_frames(3, H, W, "right", seed=9)
    np.save(tmp_path / "cap.npy", fr)
    if sidecar:
        (tmp_path / "cap.record3d.json").write_text(json.dumps(SIDECAR))
    return fr, str(tmp_path / "cap.npy")


def recorder(monkeypatch, fr, real_rgba=False):
    """band subprocesses -> a recorder: rgba writes stand-ins of its two files (and registers `depth` like the band), depth_anything
    registers its own band the way the real one does"""
    real = subprocess.run

    def fake(cmd, **kw):
        name = os.path.basename(cmd[1])
        if name == "rgba.py" and real_rgba:
            return real(cmd, **kw)
        if name == "rgba.py":
            out = cmd[cmd.index("--output") + 1]
            side = cmd[cmd.index("--rgbd") + 1]
            rgb, dep, _ = R.split_restated(fr, side, "none")
            np.save(out, rgb)
            np.save(os.path.join(os.path.dirname(out), "depth.npy"), dep)
            md = json.load(open(os.path.join(os.path.dirname(out), "metadata.json")))
            md["bands"].setdefault("depth", {})["url"] = "depth.npy"
            json.dump(md, open(os.path.join(os.path.dirname(out), "metadata.json"), "w"))
        if name == "depth_anything.py":
            folder = cmd[cmd.index("-i") + 1]
            md = json.load(open(os.path.join(folder, "metadata.json")))
            md["bands"]["depth_anything"] = {"url": "depth_anything.npy"}
            json.dump(md, open(os.path.join(folder, "metadata.json"), "w"))
        return subprocess.CompletedProcess(cmd, 0)
    monkeypatch.setattr(process.subprocess, "run", fake)


def check_record3d_folder(folder, src):
    md = json.load(open(os.path.join(folder, "metadata.json")))
    rgba = process.COMMANDS[0]
    assert os.path.basename(rgba[1]) == "rgba.py"
    assert rgba[2:] == ["-i", src, "--output", os.path.join(folder, "rgba.npy"), "--encoding_depth", "hue", "--rgbd", "right", "--fps", "24.0",
                        "--subpath", "images"]
    assert md["focal_length"] == 592.25                                         # max(fx, fy)
    assert md["principal_point"] == [3.25, 4.5]
    assert md["field_of_view"] == float(2 * np.arctan(0.5 * H / 592.25) * 180 / np.pi)      # the INPUT's full height, not the half's
    assert md["bands"]["depth"]["url"] == "depth.npy"
    assert md["bands"]["depth"]["values"] == {"min": {"type": "float", "value": 0.25}, "max": {"type": "float", "value": 3.0}}
    assert md["bands"]["rgba"]["url"] == "rgba.npy"
    assert (md["width"], md["height"], md["frames"]) == (W // 2, H, 3)          # every other band runs on the colour half
    return md


def test_record3d_arguments_and_metadata(tmp_path, monkeypatch):
    fr, src = capture(tmp_path)
    recorder(monkeypatch, fr)
    folder = process.main(["-i", src, "--record3d", "--fps", "24"])
    md = check_record3d_folder(folder, src)
    # the estimated depth band still runs, and the `depth` alias is NOT pointed at it (reference :243)
    assert [os.path.basename(c[1]) for c in process.COMMANDS][:3] == ["rgba.py", "mask_mmdet.py", "depth_anything.py"]
    assert md["bands"]["depth_anything"] == {"url": "depth_anything.npy"} and md["bands"]["depth"] != md["bands"]["depth_anything"]


def test_rgbd_alone_keeps_default_intrinsics(tmp_path, monkeypatch):
    fr, src = capture(tmp_path, sidecar=False)
    recorder(monkeypatch, fr)
    folder = process.main(["-i", src, "--rgbd", "left"])
    rgba = process.COMMANDS[0]
    assert rgba[2:] == ["-i", src, "--output", os.path.join(folder, "rgba.npy"), "--rgbd", "left", "--fps", "24", "--subpath", "images"]       # the default rate, as argparse holds it
    md = json.load(open(os.path.join(folder, "metadata.json")))
    w, h = W - W // 2, H
    assert (md["width"], md["height"]) == (w, h)
    assert md["principal_point"] == [w / 2, h / 2] and md["focal_length"] == float(h * w) ** 0.5
    assert md["field_of_view"] == float(2 * np.arctan(0.5 * h / md["focal_length"]) * 180 / np.pi)
    assert md["bands"]["depth"] == {"url": "depth.npy"} and "values" not in md["bands"]["depth"]
    assert md["bands"]["depth_anything"] == {"url": "depth_anything.npy"}


def test_without_rgbd_the_alias_still_points_at_the_estimate(tmp_path, monkeypatch):
    fr, src = capture(tmp_path, sidecar=False)
    recorder(monkeypatch, fr, real_rgba=True)
    folder = process.main(["-i", src])
    md = json.load(open(os.path.join(folder, "metadata.json")))
    assert "--rgbd" not in process.COMMANDS[0] and md["bands"]["depth"] == md["bands"]["depth_anything"]


def test_record3d_without_its_data_names_both_sources(tmp_path, monkeypatch):
    fr, src = capture(tmp_path, sidecar=False)
    recorder(monkeypatch, fr)
    monkeypatch.setitem(sys.modules, "pymediainfo", None)           # import pymediainfo -> ImportError, also where it is installed
    with pytest.raises(SystemExit) as e:
        process.main(["-i", src, "--record3d"])
    assert "cap.record3d.json" in str(e.value) and "pymediainfo" in str(e.value)
    assert process.COMMANDS == []


@pytest.mark.gpu
def test_record3d_with_the_real_rgba_band(tmp_path, monkeypatch):
    fr, src = capture(tmp_path)
    recorder(monkeypatch, fr, real_rgba=True)
    monkeypatch.setenv("PRISMA_OVERWRITE", "1")
    folder = process.main(["-i", src, "--record3d", "--fps", "24"])
    check_record3d_folder(folder, src)
    want_rgb, want_dep, _ = R.split_restated(fr, "right")
    assert np.array_equal(np.load(os.path.join(folder, "rgba.npy")), want_rgb)
    assert np.array_equal(np.load(os.path.join(folder, "depth.npy")), want_dep)
    assert sorted(os.listdir(os.path.join(folder, "images"))) == ["000000.png", "000001.png", "000002.png"]
