"""CPU: the Motion JPEG containers of bands/common/io.py - VideoWriter for .avi (AVI 1.0: hdrl, movi, idx1) and .mjpeg (the bare stream) with the
reference encoder in place of the GPU's, FrameReader back, the structure of the file asserted from its bytes, the 2 GiB guard, and the refusals."""
import io
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "bands"))

import jpeg_ref as J  # noqa: E402
from common import io as cio  # noqa: E402
from common.yuv import Format, rgb_to_yuv  # noqa: E402

H, W, N = 18, 27, 5
RATE = Fraction(30000, 1001)


def frames_rgb():
    return np.random.default_rng(11).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def write(path, chroma=444, quality=75, planes=True, group=2):
    fmt = cio.jpeg_format(chroma)
    w = cio.VideoWriter(W, H, RATE, str(path), fmt=fmt, quality=quality, encoder=J.encode_frames, group=group)
    want = []
    for f in frames_rgb():
        p = rgb_to_yuv(fmt, f)
        want.append(J.encode(p, H, W, chroma, quality))
        w.write_planes(p, H, W) if planes else w.write(f)
    w.close()
    return want


def pillow(b):
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


@pytest.mark.parametrize("planes", (True, False))
@pytest.mark.parametrize("chroma", (444, 420, 400))
@pytest.mark.parametrize("ext", ("avi", "mjpeg"))
def test_round_trip(tmp_path, ext, chroma, planes):
    path = tmp_path / ("v." + ext)
    want = write(path, chroma, planes=planes)
    r = cio.FrameReader(str(path))
    assert len(r) == N and not r.i420
    for i in range(N):
        assert r._mj.frame(i) == want[i]
        assert np.array_equal(r[i], pillow(want[i]))
    assert r[0].shape == (H, W, 3)
    if ext == "avi":
        assert r.rate == RATE and abs(r.fps - 29.97) < 0.001 and (r._mj.width, r._mj.height) == (W, H)
    else:
        assert open(path, "rb").read() == b"".join(want)        # the bare concatenation
        assert (r._mj.width, r._mj.height) == (W, H)
    w, h, fps, n = cio.get_video_data(str(path))
    assert (w, h, n) == (W, H, N)


def test_avi_structure(tmp_path):
    """header counts, idx1 offsets and even padding, read from the file"""
    path = tmp_path / "v.avi"
    want = write(path, 444, quality=100, group=3)
    assert any(len(f) & 1 for f in want) and any(not len(f) & 1 for f in want)      # both paddings occur
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and struct.unpack("<I", b[4:8])[0] == len(b) - 8 and b[8:12] == b"AVI "
    assert b[12:16] == b"LIST" and b[20:24] == b"hdrl" and b[24:28] == b"avih" and struct.unpack("<I", b[28:32])[0] == 56
    usec, _, _, flags, total, _, streams, sugg, width, height = struct.unpack("<10I", b[32:72])
    assert (usec, flags, total, streams, width, height) == (33367, 0x10, N, 1, W, H) and sugg == max(map(len, want))
    assert b[88:92] == b"LIST" and b[96:100] == b"strl" and b[100:104] == b"strh" and b[108:116] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack("<4I", b[128:144])
    assert (scale, rate, start, length) == (1001, 30000, 0, N)
    assert b[164:168] == b"strf"
    size, bw, bh, planes, bits, comp = struct.unpack("<IiiHH4s", b[172:192])
    assert (size, bw, bh, planes, bits, comp) == (40, W, H, 1, 24, b"MJPG")
    assert b[212:216] == b"LIST" and b[220:224] == b"movi" == b[cio.AVI_MOVI:cio.AVI_MOVI + 4]
    movi_size = struct.unpack("<I", b[216:220])[0]
    pos, spans = 224, []
    for f in want:
        assert b[pos:pos + 4] == b"00dc" and struct.unpack("<I", b[pos + 4:pos + 8])[0] == len(f) and b[pos + 8:pos + 8 + len(f)] == f
        spans.append((pos - 220, len(f)))
        pos += 8 + len(f)
        if len(f) & 1:
            assert b[pos] == 0
            pos += 1
        assert pos % 2 == 0
    assert pos == 220 + movi_size
    assert b[pos:pos + 4] == b"idx1" and struct.unpack("<I", b[pos + 4:pos + 8])[0] == 16 * N and pos + 8 + 16 * N == len(b)
    for k, (off, ln) in enumerate(spans):
        assert struct.unpack("<4sIII", b[pos + 8 + 16 * k:pos + 24 + 16 * k]) == (b"00dc", 0x10, off, ln)


def test_frames_are_encoded_in_groups(tmp_path):
    calls = []

    def enc(planes, h, w, chroma, quality):
        calls.append(len(planes))
        return J.encode_frames(planes, h, w, chroma, quality)

    w = cio.VideoWriter(W, H, 24, str(tmp_path / "v.mjpeg"), fmt=cio.jpeg_format(400), quality=50, encoder=enc, group=2)
    for f in frames_rgb():
        w.write(f)
    assert calls == [2, 2]
    w.close()
    assert calls == [2, 2, 1] and len(cio.FrameReader(str(tmp_path / "v.mjpeg"))) == N


def test_avi_two_gib_guard(tmp_path):
    """a stub encoder and a mocked file position: the frame that would end the file past 2 GiB raises, naming the ways out"""
    path = tmp_path / "v.avi"
    w = cio.VideoWriter(8, 8, 24, str(path), fmt=cio.jpeg_format(400), quality=50, encoder=lambda p, *a: [b"\xff\xd8" + bytes(996) + b"\xff\xd9"] * len(p),
                        group=1)
    w.write_planes(np.zeros(64, np.uint8), 8, 8)
    real = w._tell
    n = 8 + 1000 + 8 + 16 * 2                   # the chunk, the index with both entries and its header
    w._tell = lambda: cio.AVI_MAX - n           # ends exactly at the limit: fits
    w.write_planes(np.zeros(64, np.uint8), 8, 8)
    w._tell = lambda: cio.AVI_MAX - n - 16 + 1  # one byte too many with the third entry
    with pytest.raises(RuntimeError, match=r"2 GiB.*\.mjpeg.*quality"):
        w.write_planes(np.zeros(64, np.uint8), 8, 8)
    w._tell = real
    w._index = w._index[:16]                    # the mocked entry points nowhere
    w._count = 1
    w.close()
    assert len(cio.FrameReader(str(path))) == 1
    # the bare stream has no such limit
    m = cio.VideoWriter(8, 8, 24, str(tmp_path / "v.mjpeg"), fmt=cio.jpeg_format(400), quality=50, encoder=lambda p, *a: [b"\xff\xd8\xff\xd9"] * len(p), group=1)
    m._tell = lambda: 2 ** 40
    m.write_planes(np.zeros(64, np.uint8), 8, 8)
    m.close()


def test_writer_refusals(tmp_path):
    for fmt in (Format(444, 8, False, "bt601"), Format(444, 10, True, "bt601"), Format(422, 8, True, "bt601"), Format(444, 8, True, "bt709")):
        with pytest.raises(ValueError, match="JPEG"):
            cio.VideoWriter(8, 8, 24, str(tmp_path / "x.avi"), fmt=fmt, encoder=J.encode_frames)
    with pytest.raises(ValueError, match="quality"):
        cio.VideoWriter(8, 8, 24, str(tmp_path / "x.avi"), quality=0, encoder=J.encode_frames)
    w = cio.VideoWriter(8, 8, 24, str(tmp_path / "y.mjpeg"), encoder=J.encode_frames)
    assert w.format == Format(444, 8, True, "bt601") and w.quality == 90         # the defaults
    with pytest.raises(ValueError, match="frame"):
        w.write_planes(np.zeros(10, np.uint8), 8, 8)
    w.close()


def test_reader_refusals(tmp_path):
    p = tmp_path / "not.avi"
    p.write_bytes(b"RIFF\x04\0\0\0WAVE")
    with pytest.raises(RuntimeError, match="not an AVI"):
        cio.FrameReader(str(p))
    # another codec, by name
    good = tmp_path / "v.avi"
    write(good, 400)
    b = bytearray(open(good, "rb").read())
    b[188:192] = b"H264"
    p = tmp_path / "h264.avi"
    p.write_bytes(bytes(b))
    with pytest.raises(RuntimeError, match="H264.*Motion JPEG"):
        cio.FrameReader(str(p))
    # no index
    b = bytearray(open(good, "rb").read())
    at = bytes(b).rindex(b"idx1")
    b[at:at + 4] = b"JUNK"
    p = tmp_path / "noidx.avi"
    p.write_bytes(bytes(b))
    with pytest.raises(RuntimeError, match="idx1"):
        cio.FrameReader(str(p))
    p = tmp_path / "broken.mjpeg"
    p.write_bytes(b"\xff\xd8\xff\xe0\x00\x04ab\xff\xda\x00\x02\x12\x34")
    with pytest.raises(RuntimeError, match="frame 0"):
        cio.FrameReader(str(p))


def test_bare_stream_scan_skips_markers_inside_segments(tmp_path):
    """SOI / EOI byte pairs in a segment's payload are not frame boundaries"""
    f = J.encode(rgb_to_yuv(cio.jpeg_format(400), frames_rgb()[0]), H, W, 400, 50)
    tricky = f[:2] + b"\xff\xfe\x00\x06\xff\xd9\xff\xd8" + f[2:]        # a COM segment that holds EOI SOI
    p = tmp_path / "v.mjpeg"
    p.write_bytes(tricky + f)
    r = cio.FrameReader(str(p))
    assert len(r) == 2 and r._mj.frame(0) == tricky and r._mj.frame(1) == f
    assert np.array_equal(r[0], r[1])
