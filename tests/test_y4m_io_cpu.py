""".y4m (YUV4MPEG2) clips in bands/common/io.py: header parsing and the refused tokens, bare and parameterised FRAME lines, a truncated file,
len() from the file size, [i] and read_i420 against tests/yuv_ref.py and the file's own bytes, and the streaming writer."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))
import yuv_ref as R  # noqa: E402
from common import io  # noqa: E402
from common.meta import get_target, is_video  # noqa: E402


def _frames(n, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, R.i420_bytes(H, W)), dtype=np.uint8)


def _write(path, header, frames, line=b"FRAME\n"):
    with open(path, "wb") as f:
        f.write(header)
        for i, fr in enumerate(frames):
            f.write(line(i) if callable(line) else line)
            f.write(fr.tobytes())
    return str(path)


def test_header_round_trip(tmp_path):
    H, W = 6, 10
    fr = _frames(3, H, W)
    for tokens, rate in (("F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED", Fraction(30000, 1001)), ("F25:1", Fraction(25)),
                         ("F24:1 C420mpeg2 A0:0", Fraction(24)), ("F60:1 C420paldv Ip", Fraction(60)), ("F12:1 C420", Fraction(12))):
        p = _write(tmp_path / "a.y4m", ("YUV4MPEG2 W%d H%d %s\n" % (W, H, tokens)).encode(), fr)
        v = io.FrameReader(p)
        assert (v.width, v.height, len(v), v.i420) == (W, H, 3, True)
        assert v.rate == rate and v.fps == rate.numerator / rate.denominator
        assert io.get_video_data(p) == (W, H, v.fps, 3)
    # what the writer writes is what the reader reads, 30000:1001 exactly - from the source's Fraction and from a float
    for given in (Fraction(30000, 1001), 30000 / 1001, 29.97, 24, 23.976):
        p = str(tmp_path / "w.y4m")
        w = io.VideoWriter(W, H, given, p)
        w.write_i420(fr[0], H, W)
        w.close()
        head = open(p, "rb").readline()
        want = given if isinstance(given, Fraction) else Fraction(given).limit_denominator(1001000)
        assert head == b"YUV4MPEG2 W10 H6 F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (want.numerator, want.denominator)
        assert io.FrameReader(p).rate == want
    assert Fraction(30000 / 1001).limit_denominator(1001000) == Fraction(30000, 1001)
    assert is_video("clip.y4m") and get_target("/x/rgba.y4m", None, band="depth_anything", force_extension="png") == "/x/depth_anything.y4m"


@pytest.mark.parametrize("token,word", [("It", "interlaced"), ("Ib", "interlaced"), ("Im", "interlaced"), ("C422", "4:2:0"), ("C444", "4:2:0"),
                                        ("Cmono", "4:2:0"), ("C420p10", "4:2:0"), ("C444p16", "4:2:0"), ("XCOLORRANGE=FULL", "limited range")])
def test_refused_tokens_are_named(tmp_path, token, word):
    p = _write(tmp_path / "bad.y4m", ("YUV4MPEG2 W4 H4 F25:1 %s\n" % token).encode(), _frames(1, 4, 4))
    with pytest.raises(RuntimeError) as e:
        io.FrameReader(p)
    assert token in str(e.value) and word in str(e.value)


def test_not_a_y4m_and_missing_size(tmp_path):
    with pytest.raises(RuntimeError, match="not a YUV4MPEG2"):
        io.FrameReader(_write(tmp_path / "a.y4m", b"RIFF W4 H4\n", []))
    with pytest.raises(RuntimeError, match="W / H"):
        io.FrameReader(_write(tmp_path / "b.y4m", b"YUV4MPEG2 F25:1\n", []))


@pytest.mark.parametrize("H,W", [(4, 6), (5, 7)])
def test_bare_and_parameterised_frame_lines(tmp_path, H, W):
    fr = _frames(4, H, W, seed=H)
    head = ("YUV4MPEG2 W%d H%d F25:1\n" % (W, H)).encode()
    bare = io.FrameReader(_write(tmp_path / "bare.y4m", head, fr))
    mixed = io.FrameReader(_write(tmp_path / "mixed.y4m", head, fr, line=lambda i: b"FRAME\n" if i % 2 else b"FRAME Ip Xnote=%d\n" % i))
    assert bare._y4m._offsets is None and mixed._y4m._offsets is not None        # arithmetic / one scan at open
    for v in (bare, mixed):
        assert len(v) == 4
        for i in (3, 0, 2, 1):                                                   # any order
            buf = np.full(R.i420_bytes(H, W), 0xEE, np.uint8)
            assert v.read_i420(i, buf) is buf and (buf == fr[i]).all()
            rgb = v[i]
            assert rgb.dtype == np.uint8 and rgb.shape == (H, W, 3) and (rgb == R.i420_to_rgb(fr[i], H, W)).all()
        with pytest.raises(ValueError):
            v.read_i420(0, np.empty(R.i420_bytes(H, W) + 1, np.uint8))
        with pytest.raises(IndexError):
            v.read_i420(4, np.empty(R.i420_bytes(H, W), np.uint8))
    # a row of a larger array (a ring slot) is a valid target
    slot = np.zeros((3, R.i420_bytes(H, W)), np.uint8)
    bare.read_i420(2, slot[1])
    assert (slot[1] == fr[2]).all() and not slot[0].any() and not slot[2].any()


def test_len_comes_from_the_file_size(tmp_path):
    H, W = 8, 8
    head = b"YUV4MPEG2 W8 H8 F25:1\n"
    for n in (0, 1, 5):
        p = _write(tmp_path / ("n%d.y4m" % n), head, _frames(n, H, W))
        assert os.path.getsize(p) == len(head) + n * (6 + R.i420_bytes(H, W))
        assert len(io.FrameReader(p)) == n


@pytest.mark.parametrize("line", [b"FRAME\n", b"FRAME Ip\n"])
def test_truncated_last_frame_names_the_frame(tmp_path, line):
    fr = _frames(3, 4, 4)
    p = _write(tmp_path / "t.y4m", b"YUV4MPEG2 W4 H4 F25:1\n", fr, line=line)
    with open(p, "r+b") as f:
        f.truncate(os.path.getsize(p) - 5)
    with pytest.raises(RuntimeError, match="frame 2 is truncated"):
        io.FrameReader(p)


@pytest.mark.parametrize("H,W", [(4, 6), (5, 7), (1, 1)])
def test_writer_streams_frame_by_frame(tmp_path, H, W):
    rng = np.random.default_rng(W)
    rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    p = str(tmp_path / "out.y4m")
    w = io.VideoWriter(width=999, height=999, frame_rate=Fraction(30000, 1001), filename=p)      # the size is the first frame's own
    assert os.path.getsize(p) == 0
    fb, sizes = R.i420_bytes(H, W), []
    w.write(rgb[0])
    sizes.append(os.path.getsize(p))
    w.write_i420(R.rgb_to_i420(rgb[1]), H, W)
    sizes.append(os.path.getsize(p))
    w.write(rgb[2])
    sizes.append(os.path.getsize(p))
    head = b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (W, H)
    assert sizes == [len(head) + k * (6 + fb) for k in (1, 2, 3)]             # on disk after every write: nothing is held back
    with pytest.raises(ValueError):
        w.write(np.zeros((H + 1, W, 3), np.uint8))                          # no rescale: a frame of another size is an error
    w.close()
    assert open(p, "rb").read() == head + b"".join(b"FRAME\n" + R.rgb_to_i420(f).tobytes() for f in rgb)
    v = io.FrameReader(p)
    assert len(v) == 3 and (v[1] == R.i420_to_rgb(R.rgb_to_i420(rgb[1]), H, W)).all()
    with pytest.raises(RuntimeError, match="write_i420"):
        io.VideoWriter(W, H, 24, str(tmp_path / "out.npy")).write_i420(R.rgb_to_i420(rgb[0]), H, W)
