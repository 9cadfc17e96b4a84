"""Every .y4m layout without a GPU: the restatement tests/yuv_fmt_ref.py against the published coefficient sets, against the float64
conversion and against tests/yuv_ref.py; the built library's table (pb_yuv_coeffs / pb_yuv_bytes) and the host's numpy form
(bands/common/yuv.py) against the restatement; and bands/common/io.py on files of every accepted tag."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))
sys.path.insert(0, ROOT)
import yuv_fmt_ref as F  # noqa: E402
import yuv_ref as R  # noqa: E402
from common import io  # noqa: E402
from common import yuv as host  # noqa: E402

I420 = (420, 8, False, "bt601")
SIZES = [(1, 1), (3, 5), (16, 64)]


def random_frames(fmt, n, H, W, seed, saturating=False):
    """packed frames of any bytes: 16-bit samples use all 16 bits, whatever the depth (the word is read whole)"""
    rng = np.random.default_rng(seed)
    shape = (n, F.frame_bytes(fmt, H, W))
    return rng.integers(0, 2, shape, dtype=np.uint8) * 255 if saturating else rng.integers(0, 256, shape, dtype=np.uint8)


def test_published_coefficient_sets():
    for d in range(8, 17):
        for c in F.CHROMAS:
            assert F.coeffs((c, d, False, "bt601"))[:5] == (298, 409, 100, 208, 516), d
            assert F.coeffs((c, d, False, "bt709"))[:5] == (298, 459, 55, 136, 541), d
            assert F.coeffs((c, d, False, "bt601"))[5:] == (16 << (d - 8), 1 << (d - 1))
            assert F.coeffs((c, d, True, "bt709"))[5:] == (0, 1 << (d - 1))
    assert F.coeffs((444, 8, True, "bt601"))[:5] == (256, 359, 88, 183, 454)
    assert F.coeffs((444, 8, True, "bt709"))[:5] == (256, 403, 48, 120, 475)
    assert F.coeffs((444, 10, True, "bt709"))[:5] == (255, 402, 48, 119, 474)


def test_library_table_and_frame_bytes_equal_the_restatement():
    from prisma_amd import _lib, engine
    lib = _lib.load()
    for fmt in F.all_formats():
        assert engine.yuv_coeffs(fmt) == F.coeffs(fmt), fmt
        for H, W in SIZES:
            assert engine.yuv_bytes(fmt, H, W) == F.frame_bytes(fmt, H, W), (fmt, H, W)
    assert engine.yuv_bytes(I420, 5, 7) == engine.i420_bytes(5, 7)
    # a bad format: 0 bytes, an error from the table, and the reason by name
    out = (C.c_int32 * 7)()
    for bad in ((411, 8, 0, 0), (420, 7, 0, 0), (420, 17, 0, 0), (444, 8, 2, 0), (444, 8, 0, 2), (444, 8, 0, -1)):
        st = _lib.pb_yuv_fmt(*bad)
        assert lib.pb_yuv_bytes(C.byref(st), 4, 4) == 0, bad
        assert lib.pb_yuv_coeffs(C.byref(st), out) < 0 and b"no such format" in lib.pb_last_error(), bad
    assert lib.pb_yuv_bytes(None, 4, 4) == 0 and lib.pb_yuv_coeffs(None, out) < 0
    good = _lib.pb_yuv_fmt(420, 8, 0, 0)
    assert lib.pb_yuv_bytes(C.byref(good), 0, 4) == 0 and lib.pb_yuv_bytes(C.byref(good), 4, -1) == 0
    assert engine.yuv_bytes((420, 8, False, "bt2020"), 4, 4) == 0          # a matrix name the library does not have
    with pytest.raises(RuntimeError):
        engine.yuv_coeffs((420, 8, False, "bt2020"))
    assert lib.pb_struct_size(6) == C.sizeof(_lib.pb_yuv_fmt) == 16


def test_restatement_at_i420_equals_yuv_ref():
    for H, W in [(1, 1), (2, 2), (3, 5), (5, 18), (6, 32), (17, 67)]:
        for sat in (False, True):
            yuv = random_frames(I420, 3, H, W, seed=H * 100 + W, saturating=sat)
            assert F.frame_bytes(I420, H, W) == R.i420_bytes(H, W)
            assert np.array_equal(F.to_rgb(I420, yuv, H, W), R.i420_to_rgb(yuv, H, W)), (H, W, sat)


def lattice(fmt, steps=24):
    """code values that matter: 0, yoff / coff, the nominal peaks and their neighbours, 2^d - 1, 0xFFFF (16-bit storage), and an even spread"""
    d, full = fmt[1], fmt[2]
    _, _, yoff, coff = F.scales(fmt)
    top = 2 ** d - 1
    word = 255 if d == 8 else 0xFFFF
    ypk = top if full else 235 << (d - 8)
    clo, chi = (0, top) if full else (16 << (d - 8), 240 << (d - 8))
    spread = np.linspace(0, top, steps).astype(np.int64)
    ys = np.unique(np.clip(np.concatenate([[0, 1, yoff - 1, yoff, yoff + 1, ypk - 1, ypk, ypk + 1, top, word], spread]), 0, word))
    cs = np.unique(np.clip(np.concatenate([[0, 1, coff - 1, coff, coff + 1, clo, chi, chi + 1, top, word], spread]), 0, word))
    return ys, cs


@pytest.mark.parametrize("d", range(8, 17))
def test_integer_form_within_one_and_a_half_of_float64(d):
    """The bound holds for samples inside the d-bit range, and only for those: 0.5 for the final floor + 0.5 (|C| + |D| + |E|) / 2^d <= 1 for the
    coefficient rounding.  It is asserted on in-range values at every depth 8 .. 16; the clamp to 0 .. 255 is applied to the real value too (it
    can only bring the two closer).  A word above 2^d - 1 (read whole, not masked) is outside the premise, and there the rule itself - not an
    implementation of it - leaves the bound: with 0xFFFF in this lattice 2.05 at d = 13 and 2.17 at d = 14, and more on lattices with several
    out-of-range values at once.  On this particular lattice, which adds the single value 0xFFFF, the distance happens to stay below 1.5 at
    d = 10, 12 and 16 (0.93 / 1.00 / 0.95 / 0.93 at d = 8 / 10 / 12 / 16), so the value is kept there; that is a property of the lattice, no bound."""
    worst = 0.0
    for chroma in F.CHROMAS:            # (the pixel rule of 420 and 422 is that of 444; 400 has no chroma terms)
        for full in (False, True):
            for m in F.MATRICES:
                fmt = (chroma, d, full, m)
                ys, cs = lattice(fmt)
                if d not in (8, 10, 12, 16):
                    ys, cs = ys[ys < 2 ** d], cs[cs < 2 ** d]
                if chroma == 400:
                    y, cb, cr = ys, None, None
                else:
                    y, cb, cr = np.meshgrid(ys, cs, cs, indexing="ij")
                got = np.stack(F.colour(fmt, y, cb, cr)).astype(np.float64)
                real = np.clip(np.stack(F.colour_real(fmt, y, cb, cr)), 0.0, 255.0)
                err = float(np.abs(got - real).max())
                worst = max(worst, err)
                assert err <= 1.5, (fmt, err)
    print("d = %d: max |integer - float64| = %.3f" % (d, worst))


def test_unmasked_words_stay_inside_int32():
    """a 16-bit word is read whole: at every depth the largest intermediate with 0xFFFF samples is below 2^27 only for d = 16, but stays inside
    int32 everywhere - what the kernels and the host compute in"""
    for fmt in F.all_formats():
        cy, crv, cgu, cgv, cbu, yoff, coff = F.coeffs(fmt)
        word = 255 if fmt[1] == 8 else 0xFFFF
        big = cy * max(word - yoff, yoff) + max(crv, cgu + cgv, cbu) * max(word - coff, coff) + coff
        assert big < 2 ** 31, (fmt, big)
        if fmt[1] in (8, 16):
            assert big < 2 ** 27, (fmt, big)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 4), (3, 5), (4, 6), (16, 64), (17, 67)])
def test_host_numpy_form_equals_the_restatement(H, W):
    for fmt in F.all_formats(depths=(8, 9, 10, 12, 14, 16)):
        assert host.yuv_bytes(fmt, H, W) == F.frame_bytes(fmt, H, W)
        assert host.yuv_coeffs(fmt) == F.coeffs(fmt)
        for sat in (False, True):
            yuv = random_frames(fmt, 2, H, W, seed=H + W + fmt[1], saturating=sat)
            for i in range(2):
                got = host.yuv_to_rgb(fmt, yuv[i], H, W)
                assert got.dtype == np.uint8 and np.array_equal(got, F.to_rgb(fmt, yuv[i], H, W)), (fmt, H, W, sat)
    with pytest.raises(ValueError):
        host.yuv_bytes((411, 8, False, "bt601"), 4, 4)
    with pytest.raises(ValueError):
        host.yuv_to_rgb(I420, np.zeros(5, np.uint8), 2, 2)


# ---- bands/common/io.py ------------------------------------------------------------------------------------------------------------------------
TAGS = dict([(t, (420, 8)) for t in ("C420", "C420jpeg", "C420mpeg2", "C420paldv")] + [("C422", (422, 8)), ("C444", (444, 8)), ("Cmono", (400, 8))]
            + [("C%dp%d" % (c, d), (c, d)) for c in (420, 422, 444) for d in (9, 10, 12, 14, 16)] + [("Cmono%d" % d, (400, d)) for d in (9, 10, 12, 14, 16)])


def _write(path, header, frames, line=b"FRAME\n"):
    with open(path, "wb") as f:
        f.write(header)
        for i, fr in enumerate(frames):
            f.write(line(i) if callable(line) else line)
            f.write(fr.tobytes())
    return str(path)


@pytest.mark.parametrize("matrix", [None, "bt601", "bt709"])
@pytest.mark.parametrize("rng_tok,full", [("", False), ("XCOLORRANGE=LIMITED", False), ("XCOLORRANGE=FULL", True)])
def test_every_accepted_tag(tmp_path, monkeypatch, rng_tok, full, matrix):
    if matrix is None:
        monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    else:
        monkeypatch.setenv("PRISMA_Y4M_MATRIX", matrix)
    H, W, n = 5, 7, 3
    assert set(io.Y4M_TAGS) == set(TAGS)
    # no C tag: 4:2:0, 8 bit - and limited range only (test_full_range_needs_a_c_tag)
    for tag, (chroma, depth) in list(TAGS.items()) + ([] if full else [("", (420, 8))]):
        fmt = (chroma, depth, full, matrix or "bt601")
        fr = random_frames(fmt, n, H, W, seed=depth + chroma)
        p = _write(tmp_path / "a.y4m", ("YUV4MPEG2 W%d H%d F25:1 Ip %s %s\n" % (W, H, tag, rng_tok)).encode(), fr)
        v = io.FrameReader(p)
        assert tuple(v.format) == fmt and v.i420, (tag, v.format)
        assert (v.width, v.height, len(v), v.frame_bytes) == (W, H, n, F.frame_bytes(fmt, H, W)), tag
        buf = np.full(v.frame_bytes, 0xEE, np.uint8)
        assert v.read_i420(2, buf) is buf and np.array_equal(buf, fr[2])          # the planes as they are in the file
        assert np.array_equal(v[1], F.to_rgb(fmt, fr[1], H, W)), tag               # [i]: converted on the host
        assert io.get_video_data(p) == (W, H, 25.0, n)


def test_parameterised_frame_lines_and_a_truncated_last_frame(tmp_path):
    H, W = 4, 6
    fmt = (422, 10, False, "bt601")
    fr = random_frames(fmt, 4, H, W, seed=1)
    head = ("YUV4MPEG2 W%d H%d F25:1 C422p10\n" % (W, H)).encode()
    mixed = io.FrameReader(_write(tmp_path / "mixed.y4m", head, fr, line=lambda i: b"FRAME\n" if i % 2 else b"FRAME Ip Xnote=%d\n" % i))
    assert len(mixed) == 4 and mixed._y4m._offsets is not None
    for i in range(4):
        assert np.array_equal(mixed[i], F.to_rgb(fmt, fr[i], H, W))
    p = _write(tmp_path / "cut.y4m", head, fr)
    with open(p, "r+b") as f:
        f.truncate(os.path.getsize(p) - 5)
    with pytest.raises(RuntimeError, match="frame 3 is truncated"):
        io.FrameReader(p)


@pytest.mark.parametrize("token,words", [("C411", ("C411", "C422p10", "Cmono16")), ("C444alpha", ("C444alpha", "C420jpeg", "C444p12")),
                                         ("C420p11", ("C420p11", "C420p10")), ("It", ("It", "interlaced")), ("XCOLORRANGE=WIDE", ("XCOLORRANGE=WIDE", "FULL"))])
def test_refused_tokens_are_named_with_what_is_accepted(tmp_path, monkeypatch, token, words):
    monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    p = _write(tmp_path / "bad.y4m", ("YUV4MPEG2 W4 H4 F25:1 %s\n" % token).encode(), random_frames(I420, 1, 4, 4, seed=0))
    with pytest.raises(RuntimeError) as e:
        io.FrameReader(p)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_full_range_needs_a_c_tag(tmp_path, monkeypatch):
    """a header that names no layout stays what it always was: 8-bit 4:2:0, limited range, anything else refused (tests/test_y4m_io_cpu.py
    pins that refusal); every writer of XCOLORRANGE writes the C tag too"""
    monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    fr = random_frames(I420, 2, 4, 6, seed=3)
    with pytest.raises(RuntimeError) as e:
        io.FrameReader(_write(tmp_path / "a.y4m", b"YUV4MPEG2 W6 H4 F25:1 XCOLORRANGE=FULL\n", fr))
    assert "XCOLORRANGE=FULL" in str(e.value) and "`C` tag" in str(e.value) and "C420jpeg" in str(e.value)
    for head in (b"YUV4MPEG2 W6 H4 F25:1 XCOLORRANGE=FULL C420jpeg\n", b"YUV4MPEG2 W6 H4 F25:1 C420 XCOLORRANGE=FULL\n"):       # either order
        v = io.FrameReader(_write(tmp_path / "b.y4m", head, fr))
        assert tuple(v.format) == (420, 8, True, "bt601") and np.array_equal(v[1], F.to_rgb(tuple(v.format), fr[1], 4, 6))


def test_frames_of_another_size_than_the_tag_says_are_diagnosed(tmp_path, monkeypatch):
    """8-bit 4:2:0 planes behind a header that names another layout: the error names the tag and both sizes; a file that fits its tag is never
    second-guessed, whatever else its size would also fit"""
    monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    H, W = 4, 4
    for tag in ("C422", "Cmono", "C444p16"):
        p = _write(tmp_path / "bad.y4m", ("YUV4MPEG2 W%d H%d F25:1 %s\n" % (W, H, tag)).encode(), random_frames(I420, 3, H, W, seed=1))
        with pytest.raises(RuntimeError) as e:
            io.FrameReader(p)
        assert tag in str(e.value) and "24 bytes" in str(e.value) and "4:2:0" in str(e.value), str(e.value)
    # 4 frames of C422 (32 bytes + FRAME = 38) are not a multiple of 30, 15 are: read as C422 all the same
    for n in (4, 15):
        fr = random_frames((422, 8, False, "bt601"), n, H, W, seed=2)
        v = io.FrameReader(_write(tmp_path / "ok.y4m", b"YUV4MPEG2 W4 H4 F25:1 C422\n", fr))
        assert len(v) == n and v.frame_bytes == 32


def test_a_bad_matrix_is_refused_by_name(tmp_path, monkeypatch):
    p = _write(tmp_path / "a.y4m", b"YUV4MPEG2 W4 H4 F25:1\n", random_frames(I420, 1, 4, 4, seed=0))
    for bad in ("bt2020", "BT709", "709"):
        monkeypatch.setenv("PRISMA_Y4M_MATRIX", bad)
        with pytest.raises(RuntimeError) as e:
            io.FrameReader(p)
        assert "PRISMA_Y4M_MATRIX" in str(e.value) and bad in str(e.value) and "bt709" in str(e.value)
    monkeypatch.setenv("PRISMA_Y4M_MATRIX", "")            # empty: unset
    assert io.FrameReader(p).format.matrix == "bt601"


def test_get_video_data_does_not_decode(tmp_path, monkeypatch):
    monkeypatch.delenv("PRISMA_Y4M_MATRIX", raising=False)
    H, W = 6, 10
    fmt = (422, 10, False, "bt601")
    p = _write(tmp_path / "a.y4m", ("YUV4MPEG2 W%d H%d F30000:1001 Ip C422p10\n" % (W, H)).encode(), random_frames(fmt, 5, H, W, seed=2))

    def boom(*a, **k):
        raise AssertionError("a frame was decoded")
    monkeypatch.setattr(io, "yuv_to_rgb", boom)
    assert io.get_video_data(p) == (W, H, 30000 / 1001, 5)


def test_frame_formats_hands_the_layout_to_the_engine():
    from common.loop import frame_formats

    class Model:
        frame_format, rgb_format = "rgb", "rgb"
    m = Model()
    assert frame_formats(m, False, False, 4, 6) == {} and (m.frame_format, m.rgb_format) == ("rgb", "rgb")
    assert frame_formats(m, True, False, 4, 6, host.Format(422, 10, True, "bt709")) == {"size": (4, 6)}
    assert (m.frame_format, m.rgb_format) == ((422, 10, True, "bt709"), "rgb")
    frame_formats(m, True, True, 4, 6, host.I420)
    assert (m.frame_format, m.rgb_format) == ("i420", "i420")          # the usual clip: the option it always was
    frame_formats(m, True, False, 4, 6)
    assert m.frame_format == "i420"
