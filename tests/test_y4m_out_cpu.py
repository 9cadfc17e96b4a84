"""Writing .y4m videos in any layout, without a GPU: PRISMA_Y4M_OUT's forms and refusals, the header line, VideoWriter -> Y4MFile round trips
(bands/common/io.py), and the built library's forward table (pb_yuv_fwd_coeffs) against the restatement tests/yuv_out_ref.py."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))
sys.path.insert(0, ROOT)
import yuv_fmt_ref as F  # noqa: E402
import yuv_out_ref as O  # noqa: E402
import yuv_ref as R  # noqa: E402
from common import io  # noqa: E402
from common import yuv as host  # noqa: E402

I420 = (420, 8, False, "bt601")


def test_out_format_forms(monkeypatch):
    monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    for unset in (None, ""):
        monkeypatch.delenv("PRISMA_Y4M_OUT", raising=False)
        if unset is not None:
            monkeypatch.setenv("PRISMA_Y4M_OUT", unset)
        assert io.y4m_out() == I420 and io.y4m_out((444, 10, True, "bt709")) == I420
    for tag, (chroma, depth) in io.Y4M_TAGS.items():
        for suffix, full, matrix in (("", False, "bt601"), (",full", True, "bt601"), (",bt709", False, "bt709"), (",full,bt709", True, "bt709"),
                                     (",bt709,full", True, "bt709")):
            monkeypatch.setenv("PRISMA_Y4M_OUT", tag + suffix)
            assert io.y4m_out() == (chroma, depth, full, matrix), tag + suffix
    monkeypatch.setenv("PRISMA_Y4M_OUT", "C444p12,full")
    assert io.y4m_out() == (444, 12, True, "bt601")
    monkeypatch.setenv("PRISMA_Y4M_OUT", "Cmono,full")
    assert io.y4m_out() == (400, 8, True, "bt601")
    monkeypatch.setenv("PRISMA_Y4M_OUT", "C422p10,bt709")
    assert io.y4m_out() == (422, 10, False, "bt709")
    # the matrix comes from this variable only
    monkeypatch.setenv("PRISMA_Y4M_MATRIX", "bt709")
    monkeypatch.setenv("PRISMA_Y4M_OUT", "C444")
    assert io.y4m_out() == (444, 8, False, "bt601")
    monkeypatch.delenv("PRISMA_Y4M_OUT")
    assert io.y4m_out() == I420


def test_out_format_source(monkeypatch):
    monkeypatch.setenv("PRISMA_Y4M_OUT", "source")
    monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    assert io.y4m_out() == I420                                                  # the clip is no .y4m
    assert io.y4m_out(host.Format(422, 10, True, "bt601")) == (422, 10, True, "bt601")
    monkeypatch.setenv("PRISMA_Y4M_MATRIX", "bt709")
    assert io.y4m_out(host.Format(400, 12, False, "bt709")) == (400, 12, False, "bt709")
    assert io.y4m_out((444, 8, True, "bt601")) == (444, 8, True, "bt709")          # PRISMA_Y4M_MATRIX names the source's matrix


@pytest.mark.parametrize("value, says", [("C411", "C411 is not a layout"), ("C999", "C999 is not a layout"), ("444p12", "444p12 is not a layout"),
                                         (",full", "(nothing) is not a layout"), ("C444,limited", "`,full` and / or `,bt709`"),
                                         ("C444,full,full", "`,full` and / or `,bt709`"), ("C444,", "`,full` and / or `,bt709`"),
                                         ("C444p12 ,full", "is not a layout"), ("c444", "c444 is not a layout")])
def test_out_format_refusals(monkeypatch, value, says):
    monkeypatch.setenv("PRISMA_Y4M_OUT", value)
    with pytest.raises(RuntimeError) as e:
        io.y4m_out()
    assert "PRISMA_Y4M_OUT=" + value in str(e.value) and says in str(e.value)


def test_header_line():
    rate = Fraction(30000, 1001)
    plain = b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert io.y4m_header(7, 5, rate) == plain == io.y4m_header(7, 5, rate, None) == io.y4m_header(7, 5, rate, I420)
    assert io.y4m_header(7, 5, rate, (444, 12, True, "bt601")) == b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C444p12 XCOLORRANGE=FULL\n"
    assert io.y4m_header(7, 5, rate, (400, 8, True, "bt709")) == b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 Cmono XCOLORRANGE=FULL\n"
    assert io.y4m_header(7, 5, rate, (400, 16, False, "bt601")) == b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 Cmono16 XCOLORRANGE=LIMITED\n"
    assert io.y4m_header(7, 5, rate, (422, 8, False, "bt601")) == b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C422 XCOLORRANGE=LIMITED\n"
    # every layout's tag is one the reader maps back to it
    for (chroma, depth) in set(io.Y4M_TAGS.values()):
        assert io.Y4M_TAGS[io.y4m_tag((chroma, depth, False, "bt601"))] == (chroma, depth)
    with pytest.raises(ValueError):
        io.y4m_tag((420, 11, False, "bt601"))


@pytest.mark.parametrize("fmt", [(400, 8, True, "bt601"), (420, 10, False, "bt709"), (422, 16, True, "bt709"), (444, 12, True, "bt601"), None],
                         ids=lambda f: "default" if f is None else "%d-%d-%s-%s" % (f[0], f[1], "full" if f[2] else "limited", f[3]))
@pytest.mark.parametrize("size", [(5, 7), (4, 16)], ids=lambda s: "%dx%d" % s)
def test_writer_round_trip(tmp_path, monkeypatch, fmt, size):
    H, W = size
    want = I420 if fmt is None else fmt
    monkeypatch.setenv("PRISMA_Y4M_MATRIX", want[3])        # a header has no tag for the matrix
    rgb = np.random.default_rng(H + W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    path = str(tmp_path / "out.y4m")
    w = io.VideoWriter(W, H, Fraction(24000, 1001), path, fmt=fmt)
    w.write(rgb[0])
    w.write_planes(O.rgb_to_yuv(want, rgb[1]), H, W)
    w.write(rgb[2])
    with pytest.raises(ValueError):
        w.write_planes(np.zeros(F.frame_bytes(want, H, W) + 1, np.uint8), H, W)
    if fmt is not None:
        with pytest.raises(RuntimeError):
            w.write_i420(np.zeros(R.i420_bytes(H, W), np.uint8), H, W)
    w.close()
    f = io.Y4MFile(path)
    assert tuple(f.format) == want and (f.height, f.width) == (H, W) and f.rate == Fraction(24000, 1001) and len(f) == 3
    assert f.frame_bytes == F.frame_bytes(want, H, W)
    for i in range(3):
        planes = f.read_i420(i, np.empty(f.frame_bytes, np.uint8))
        assert np.array_equal(planes, O.rgb_to_yuv(want, rgb[i])), i
    f.close()
    if fmt is None:
        raw = open(path, "rb").read()
        assert raw.startswith(b"YUV4MPEG2 W%d H%d F24000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\nFRAME\n" % (W, H))
        assert raw.endswith(R.rgb_to_i420(rgb[2]).tobytes())
    reader = io.FrameReader(path)
    for i in range(3):
        assert np.array_equal(reader[i], F.to_rgb(want, O.rgb_to_yuv(want, rgb[i]), H, W))
    if want == (444, 12, True, "bt601"):
        assert np.array_equal(np.stack([reader[i] for i in range(3)]), rgb)         # the lossless choice


def test_writer_refuses_an_unknown_layout(tmp_path):
    with pytest.raises(ValueError):
        io.VideoWriter(4, 4, 24, str(tmp_path / "x.y4m"), fmt=(411, 8, False, "bt601"))


def test_library_forward_table_equals_the_restatement():
    from prisma_amd import _lib, engine
    lib = _lib.load()
    for fmt in F.all_formats():
        assert engine.yuv_fwd_coeffs(fmt) == O.fwd_coeffs(fmt), fmt
    out = (C.c_int32 * 12)()
    for bad in ((411, 8, 0, 0), (420, 7, 0, 0), (420, 17, 0, 0), (444, 8, 2, 0), (444, 8, 0, 2)):
        assert lib.pb_yuv_fwd_coeffs(C.byref(_lib.pb_yuv_fmt(*bad)), out) < 0 and b"no such format" in lib.pb_last_error(), bad
    assert lib.pb_yuv_fwd_coeffs(None, out) < 0
    assert lib.pb_yuv_fwd_coeffs(C.byref(_lib.pb_yuv_fmt(444, 12, 1, 0)), None) < 0
    with pytest.raises(RuntimeError):
        engine.yuv_fwd_coeffs((420, 8, False, "bt2020"))


def test_process_passes_the_layout_to_the_bands(tmp_path, monkeypatch):
    """process.py --y4m_out: refused before anything runs when it names no layout; set for the band subprocesses otherwise, and the rgba band
    still copies a .y4m input as it is"""
    import subprocess
    import process
    monkeypatch.delenv("PRISMA_Y4M_OUT", raising=False)           # (and puts back what main() sets)
    rgb = np.random.default_rng(5).integers(0, 256, (3, 34, 50, 3), dtype=np.uint8)
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(b"YUV4MPEG2 W50 H34 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" + b"".join(b"FRAME\n" + R.rgb_to_i420(f).tobytes() for f in rgb))
    with pytest.raises(SystemExit):
        process.main(["-i", str(clip), "--y4m_out", "C411"])
    assert not (tmp_path / "clip").exists() and "PRISMA_Y4M_OUT" not in os.environ
    real, seen = subprocess.run, []

    def fake(cmd, **kw):
        seen.append((os.path.basename(cmd[1]), os.environ.get("PRISMA_Y4M_OUT"), kw.get("env")))
        return real(cmd, **kw) if os.path.basename(cmd[1]) == "rgba.py" else subprocess.CompletedProcess(cmd, 0)
    monkeypatch.setattr(process.subprocess, "run", fake)
    folder = process.main(["-i", str(clip), "--y4m_out", "C444p12,full"])
    assert len(seen) >= 3 and all(v == "C444p12,full" and env is None for _, v, env in seen), seen       # inherited: no band gets an environment of its own
    assert open(os.path.join(folder, "rgba.y4m"), "rb").read() == clip.read_bytes()
