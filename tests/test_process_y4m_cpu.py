"""process.py on a .y4m clip, plumbing only (the GPU bands are replaced by a recorder, rgba runs for real, as in tests/test_process_cli.py):
the metadata an .mp4 would give, every band command gets the folder, outputs are named .y4m, the rgba band is a copy of the input."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import process  # noqa: E402
import yuv_ref as R  # noqa: E402
from bands.common.meta import get_target, get_url, load_metadata  # noqa: E402

H, W, N = 34, 50, 3


def _clip(tmp_path):
    rgb = np.random.default_rng(5).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    p = tmp_path / "clip.y4m"
    with open(p, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (W, H))
        for fr in rgb:
            f.write(b"FRAME\n" + R.rgb_to_i420(fr).tobytes())
    return p, rgb


def _fake_bands(monkeypatch):
    real = subprocess.run

    def fake(cmd, **kw):
        if os.path.basename(cmd[1]) == "rgba.py":
            return real(cmd, **kw)
        return subprocess.CompletedProcess(cmd, 0)
    monkeypatch.setattr(process.subprocess, "run", fake)


def test_y4m_plumbing_metadata_commands_and_names(tmp_path, monkeypatch):
    _fake_bands(monkeypatch)
    clip, rgb = _clip(tmp_path)
    folder = process.main(["-i", str(clip), "-b", "-m"])
    assert folder == str(tmp_path / "clip")
    md = json.load(open(os.path.join(folder, "metadata.json")))
    assert (md["width"], md["height"], md["frames"]) == (W, H, N)
    assert md["fps"] == 30000 / 1001 and md["duration"] == N / (30000 / 1001)
    assert md["principal_point"] == [W / 2, H / 2] and abs(md["focal_length"] - (W * H) ** 0.5) < 1e-9
    assert md["bands"]["rgba"]["url"] == "rgba.y4m"
    # the rgba band is the input, byte for byte; --subpath images dumps 255 - frame of the host-converted RGB
    assert open(os.path.join(folder, "rgba.y4m"), "rb").read() == open(clip, "rb").read()
    from PIL import Image
    for i in range(N):
        dump = np.asarray(Image.open(os.path.join(folder, "images", "%06d.png" % i)))
        assert (dump == 255 - R.i420_to_rgb(R.rgb_to_i420(rgb[i]), H, W)).all()
    names = [os.path.basename(c[1]) for c in process.COMMANDS]
    assert names == ["rgba.py", "mask_mmdet.py", "depth_anything.py", "flow_gmflow.py"]
    rgba, mask, depth, flow = process.COMMANDS
    assert rgba[2:] == ["-i", str(clip), "--output", os.path.join(folder, "rgba.y4m"), "--fps", "24", "--subpath", "images"]
    assert mask[2:] == ["-i", folder, "--sdf", "--subpath", "mask"]
    assert depth[2:] == ["-i", folder, "--metric", "outdoor"]
    assert flow[2:] == ["-i", folder, "--backwards", "--mask"]
    # what a band started on the folder resolves: its input is the rgba .y4m, its outputs are .y4m files beside it
    data = load_metadata(folder)
    src = get_url(folder, data, "rgba")
    assert src == os.path.join(folder, "rgba.y4m")
    for band in ("mask", "depth_anything", "flow_gmflow", "flow_gmflow_mask", "flow_raft"):
        assert get_target(src, data, band=band, target="", force_extension="png") == os.path.join(folder, band + ".y4m")
    assert data["bands"]["depth_anything"]["url"] == "depth_anything.y4m" and data["bands"]["flow_gmflow"]["url"] == "flow_gmflow.y4m"


def test_rgbd_split_of_a_y4m_reads_rgb_and_keeps_the_container(tmp_path, monkeypatch):
    _fake_bands(monkeypatch)
    clip, rgb = _clip(tmp_path)
    folder = process.main(["-i", str(clip), "--rgbd", "right", "--fps", "30"])
    sys.path.insert(0, os.path.join(ROOT, "bands"))
    from common.io import FrameReader
    back = np.stack([R.i420_to_rgb(R.rgb_to_i420(f), H, W) for f in rgb])
    colour, depth = FrameReader(os.path.join(folder, "rgba.y4m")), FrameReader(os.path.join(folder, "depth.y4m"))
    assert len(colour) == len(depth) == N and colour.rate == depth.rate == Fraction(30)
    k = W // 2
    for i in range(N):       # each half: the host-converted RGB, cropped, and through the writer's conversion once more
        assert (colour[i] == R.i420_to_rgb(R.rgb_to_i420(back[i][:, :k]), H, k)).all()
        assert (depth[i] == R.i420_to_rgb(R.rgb_to_i420(back[i][:, k:]), H, W - k)).all()
    md = json.load(open(os.path.join(folder, "metadata.json")))
    assert (md["width"], md["height"], md["frames"]) == (k, H, N) and md["bands"]["depth"]["url"] == "depth.y4m"
