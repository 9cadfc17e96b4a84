"""GPU, end to end: the depth band on seeded ViT-S weights writing Motion JPEG (PRISMA_VIDEO_OUT=avi).  Every frame of the .avi holds exactly what
the rule (tests/jpeg_ref.py) makes of that frame's C444,full planes - which the same band run writes with PRISMA_Y4M_OUT=C444,full - in the
blocking loop and in the streamed one; the file reads back through FrameReader and metadata.json names it."""
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
import jpeg_ref as J  # noqa: E402
import yuv_ref as R  # noqa: E402
from common import io  # noqa: E402

pytestmark = pytest.mark.gpu

N, H, W = 6, 98, 154                    # PRISMA_BATCH=4: chunks of 4 and 2 frames; neither side a multiple of 8
RATE = (30000, 1001)
FMT = (444, 8, True, "bt601")


@functools.lru_cache(maxsize=None)
def _source():
    from prisma_amd import synth
    rgb = synth.frames(N, H, W, seed=5)
    head = b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % ((W, H) + RATE)
    return head + b"".join(b"FRAME\n" + R.rgb_to_i420(f).tobytes() for f in rgb)


def _run(folder, stream, **env_more):
    folder.mkdir()
    (folder / "rgba.y4m").write_bytes(_source())
    (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba.y4m"}}}))
    env = dict(os.environ, PRISMA_SYNTH="1", PRISMA_OVERWRITE="1", PRISMA_BATCH="4", PRISMA_RING_SLOTS="2", PRISMA_STREAM=str(stream), PRISMA_STREAM_LOG="1")
    for k in ("PRISMA_Y4M_MATRIX", "PRISMA_Y4M_OUT", "PRISMA_VIDEO_OUT"):
        env.pop(k, None)
    env.update(env_more)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bands", "depth_anything.py"), "-i", str(folder), "--encoder", "vits"], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert ("[loop] streamed: " in r.stderr) == bool(stream), r.stderr[-2000:]
    return folder


@pytest.mark.parametrize("stream", [0, 1])
def test_depth_band_avi_holds_the_rule_of_its_planes(tmp_path, stream):
    planes_run = _run(tmp_path / "planes", stream, PRISMA_Y4M_OUT="C444,full")
    y4m = io.Y4MFile(str(planes_run / "depth_anything.y4m"))
    assert tuple(y4m.format) == FMT and len(y4m) == N and (y4m.width, y4m.height) == (W, H)
    planes = [y4m.read_i420(i, np.empty(y4m.frame_bytes, np.uint8)) for i in range(N)]
    assert len({p.tobytes() for p in planes}) > 1                           # the frames differ: an order mix-up would show
    avi_run = _run(tmp_path / "avi", stream, PRISMA_VIDEO_OUT="avi")
    assert not os.path.exists(avi_run / "depth_anything.y4m")
    reader = io.FrameReader(str(avi_run / "depth_anything.avi"))
    assert len(reader) == N and reader.rate.numerator == RATE[0] and reader.rate.denominator == RATE[1]
    for i in range(N):
        want = J.encode(planes[i], H, W, 444, 90)                           # the defaults: quality 90, 4:4:4
        got = reader._mj.frame(i)
        assert got == want, "frame %d: %d bytes against the rule's %d" % (i, len(got), len(want))
        assert reader[i].shape == (H, W, 3)
    md = json.load(open(avi_run / "metadata.json"))
    assert md["bands"]["depth_anything"]["url"] == "depth_anything.avi" and md["bands"]["rgba"]["url"] == "rgba.y4m"
    # the scalars beside the video do not depend on the container
    for name in ("depth_anything_min.csv", "depth_anything_max.csv"):
        assert open(avi_run / name).read() == open(planes_run / name).read()
