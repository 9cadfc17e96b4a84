"""bands/rgba.py --rgbd: the split() path of the reference (bands/rgba.py:24-75, 112-128) - colour half to rgba.<ext>, depth half to
depth.<ext>, hue decode on the GPU - on a 6-frame 6 x 10 .npy stack, against tests/rgbd_ref.py.  Without a GPU the path fails loudly and the
plain path is untouched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bands"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import rgbd_ref as R  # noqa: E402

BAND = os.path.join(ROOT, "bands", "rgba.py")


def clip(tmp_path, n=6, H=6, W=10, side="right"):
    fr = R.make_frames(n, H, W, side, seed=3)
    np.save(tmp_path / "clip.npy", fr)
    return fr, str(tmp_path / "clip.npy")


def run(*argv):
    env = dict(os.environ, PRISMA_OVERWRITE="1")
    return subprocess.run([sys.executable, BAND] + list(argv), env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_hue_split_writes_both_halves(tmp_path):
    fr, src = clip(tmp_path)
    folder = tmp_path / "out"
    folder.mkdir()
    (folder / "metadata.json").write_text(json.dumps({"bands": {"depth": {"values": {"min": {"type": "float", "value": 0.5}}}}}))
    r = run("-i", src, "--output", str(folder / "rgba.npy"), "--rgbd", "right", "--encoding_depth", "hue", "--fps", "29.97",
            "--subpath", "images", "--subpath_depth", "depth_frames")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    want_rgb, want_dep, _ = R.split_restated(fr, "right")
    assert np.array_equal(np.load(folder / "rgba.npy"), fr[:, :, :5]) and np.array_equal(want_rgb, fr[:, :, :5])
    assert np.array_equal(np.load(folder / "depth.npy"), want_dep)
    # --subpath / --subpath_depth: `255 - frame` PNGs of their half, one per frame
    from PIL import Image
    for i in range(6):
        name = str(i).zfill(6) + ".png"
        assert np.array_equal(np.asarray(Image.open(folder / "images" / name)), 255 - want_rgb[i])
        assert np.array_equal(np.asarray(Image.open(folder / "depth_frames" / name)), 255 - want_dep[i])
    # metadata.json gets `depth` beside `rgba`; what the orchestrator put there stays
    md = json.load(open(folder / "metadata.json"))
    assert md["bands"]["rgba"]["url"] == "rgba.npy" and md["bands"]["depth"]["url"] == "depth.npy"
    assert md["bands"]["depth"]["values"]["min"]["value"] == 0.5


@pytest.mark.gpu
def test_plain_split_writes_two_crops(tmp_path):
    fr, src = clip(tmp_path, side="top")
    r = run("-i", src, "--output", str(tmp_path / "rgba.npy"), "--rgbd", "top", "--encoding_depth", "none", "--output_depth", "lidar")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert np.array_equal(np.load(tmp_path / "rgba.npy"), fr[:, 3:])
    assert np.array_equal(np.load(tmp_path / "lidar.npy"), fr[:, :3])


@pytest.mark.gpu
def test_subpaths_hold_the_right_halves(tmp_path):
    fr, src = clip(tmp_path, n=2, H=5, W=7, side="left")
    r = run("-i", src, "--output", str(tmp_path / "rgba.npy"), "--rgbd", "left", "--encoding_depth", "hue", "--subpath", "a", "--subpath_depth", "b")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    want_rgb, want_dep, _ = R.split_restated(fr, "left")
    assert want_rgb.shape == (2, 5, 4, 3) and want_dep.shape == (2, 5, 3, 3)          # odd width: the half that starts at the middle is wider
    from PIL import Image
    for i in range(2):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "a" / (str(i).zfill(6) + ".png"))), 255 - want_rgb[i])
        assert np.array_equal(np.asarray(Image.open(tmp_path / "b" / (str(i).zfill(6) + ".png"))), 255 - want_dep[i])
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["000000.png", "000001.png"]


def test_without_a_gpu_the_split_fails_loudly_and_the_plain_path_runs(tmp_path):
    import __graft_entry__ as entry
    from prisma_amd import _lib
    entry.build()
    fr, src = clip(tmp_path)
    plain = run("-i", src, "--output", str(tmp_path / "plain.npy"))
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert np.array_equal(np.load(tmp_path / "plain.npy"), fr)
    if _lib.load().pb_device_count() > 0:
        return                                  # the GPU tests above cover the split where a device is visible
    r = run("-i", src, "--output", str(tmp_path / "rgba.npy"), "--rgbd", "right", "--encoding_depth", "hue")
    assert r.returncode != 0 and "no HIP device" in r.stderr, r.stderr[-3000:]
    assert not os.path.exists(tmp_path / "depth.npy")


def test_rgbd_is_ignored_for_a_still_image(tmp_path):
    from PIL import Image
    img = R.make_frames(1, 6, 10, "right")[0]
    Image.fromarray(img).save(tmp_path / "img.png")
    r = run("-i", str(tmp_path / "img.png"), "--output", str(tmp_path / "rgba.png"), "--rgbd", "right", "--encoding_depth", "hue")
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ignored for a still image" in r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "rgba.png")), img) and not os.path.exists(tmp_path / "depth.png")
