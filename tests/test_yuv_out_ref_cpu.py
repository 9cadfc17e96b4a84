"""RGB -> every .y4m layout without a GPU: the restatement tests/yuv_out_ref.py against the published I420 integers, against tests/yuv_ref.py,
against the float64 conversion and - read back through tests/yuv_fmt_ref.py - against its own input over all 2^24 colours; and the host's numpy
form (bands/common/yuv.py rgb_to_yuv) against the restatement."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))
sys.path.insert(0, ROOT)
import yuv_fmt_ref as F  # noqa: E402
import yuv_out_ref as O  # noqa: E402
import yuv_ref as R  # noqa: E402
from common import yuv as host  # noqa: E402

I420 = (420, 8, False, "bt601")
SIZES = [(1, 1), (2, 4), (3, 5), (17, 67)]


def random_rgb(H, W, seed, n=None):
    return np.random.default_rng(seed).integers(0, 256, ((n,) if n else ()) + (H, W, 3), dtype=np.uint8)


def all_colours():
    """every RGB triple once, as one 4096 x 4096 frame"""
    g = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([g & 255, (g >> 8) & 255, g >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def round_trip(fmt, rgb, rows=512):
    """(colours that do not come back, the largest channel error) of a 4:4:4 / mono format over `rgb`, slab by slab (a pixel stands alone)"""
    assert fmt[0] in (400, 444)
    bad = worst = 0
    for s in range(0, rgb.shape[0], rows):
        part = rgb[s:s + rows]
        back = F.to_rgb(fmt, O.rgb_to_yuv(fmt, part), part.shape[0], part.shape[1])
        diff = np.abs(back.astype(np.int16) - part).max(axis=-1)
        bad += int((diff > 0).sum())
        worst = max(worst, int(diff.max()))
    return bad, worst


def test_the_exception_yields_the_published_integers():
    for c in F.CHROMAS:
        assert O.fwd_coeffs((c, 8, False, "bt601")) == (66, 129, 25, 38, 74, 112, 94, 18, 8, 16, 128, 255), c
    # and nowhere else is F anything but 24 - d
    for fmt in F.all_formats():
        if fmt[1:] != (8, False, "bt601"):
            assert O.fwd_coeffs(fmt)[8] == 24 - fmt[1], fmt


def test_restatement_at_i420_equals_yuv_ref():
    for H, W in SIZES:
        rgb = random_rgb(H, W, seed=H * 100 + W, n=3)
        assert np.array_equal(O.rgb_to_yuv(I420, rgb), np.stack([R.rgb_to_i420(f) for f in rgb])), (H, W)


def test_within_the_stated_bound_of_the_real_conversion():
    """0.5 for the final floor + 510 / 2^F for the rounded coefficients, on the 16^3 lattice of colours that holds black, white and every corner"""
    lat = np.arange(0, 256, 17)
    img = np.stack(np.meshgrid(lat, lat, lat, indexing="ij"), axis=-1).reshape(64, 64, 3).astype(np.uint8)
    for fmt in F.all_formats():
        bound = 0.5 + 510 / 2 ** O.frac_bits(fmt)
        for name, got, real in zip("Y Cb Cr".split(), O.samples(fmt, img), O.to_yuv_real(fmt, img)):
            if got is not None:
                err = float(np.abs(got - real).max())
                assert err <= bound, (fmt, name, err, bound)


def test_grey_white_and_the_code_range():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=-1).repeat(2, axis=0)      # [2, 256, 3]
    rgb = random_rgb(6, 8, seed=5)
    for fmt in F.all_formats():
        top, coff = 2 ** fmt[1] - 1, 2 ** (fmt[1] - 1)
        y, cb, cr = O.samples(fmt, grey)
        if cb is not None:
            assert (cb == coff).all() and (cr == coff).all(), fmt
        white = 219 * 2 ** (fmt[1] - 8) + 16 * 2 ** (fmt[1] - 8) if not fmt[2] else top
        assert y[0, 255] == white and y[0, 0] == (0 if fmt[2] else 16 * 2 ** (fmt[1] - 8)), fmt
        for p in O.samples(fmt, rgb) + O.samples(fmt, np.array([[[255, 0, 0], [0, 0, 255], [0, 255, 0], [255, 255, 0]]], np.uint8)):
            if p is not None:
                assert p.min() >= 0 and p.max() <= top, fmt


@pytest.mark.parametrize("matrix", F.MATRICES)
@pytest.mark.parametrize("full", (False, True))
@pytest.mark.parametrize("depth", (12, 14, 16))
def test_444_of_12_bits_and_more_returns_every_colour(depth, full, matrix):
    """a condition, not a tolerance: every one of the 2^24 colours comes back as it went in"""
    assert round_trip((444, depth, full, matrix), all_colours()) == (0, 0)


# colours of the 2^24 that 10-bit 4:4:4 does not return (all off by 1), as this restatement finds them: 0.06 %, 0.02 %, 0.24 %, 1.97 %
OFF_AT_10_BITS = {(False, "bt601"): 10339, (False, "bt709"): 3443, (True, "bt601"): 40929, (True, "bt709"): 330422}


@pytest.mark.parametrize("matrix", F.MATRICES)
@pytest.mark.parametrize("full", (False, True))
def test_444_of_10_bits_is_off_by_at_most_one(full, matrix):
    bad, worst = round_trip((444, 10, full, matrix), all_colours())
    assert worst == 1
    assert bad == OFF_AT_10_BITS[(full, matrix)]


def test_grey_through_8_bit_full_range_mono_is_exact():
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=-1)
    for matrix in F.MATRICES:
        fmt = (400, 8, True, matrix)
        assert O.rgb_to_yuv(fmt, grey).tolist() == list(range(256))
        assert round_trip(fmt, grey) == (0, 0)


def test_host_form_equals_the_restatement():
    for fmt in F.all_formats():
        assert host.yuv_fwd_coeffs(fmt) == O.fwd_coeffs(fmt), fmt
        for H, W in SIZES:
            rgb = random_rgb(H, W, seed=H * 7 + W + fmt[1])
            got = host.rgb_to_yuv(fmt, rgb)
            assert got.dtype == np.uint8 and got.shape == (F.frame_bytes(fmt, H, W),)
            assert np.array_equal(got, O.rgb_to_yuv(fmt, rgb)), (fmt, H, W)
    out = np.empty(host.yuv_bytes((422, 10, True, "bt709"), 3, 5), np.uint8)
    assert host.rgb_to_yuv((422, 10, True, "bt709"), random_rgb(3, 5, 1), out=out) is out
    with pytest.raises(ValueError):
        host.rgb_to_yuv((411, 8, False, "bt601"), random_rgb(2, 2, 1))
    with pytest.raises(ValueError):
        host.rgb_to_yuv(I420, random_rgb(2, 2, 1), out=np.empty(5, np.uint8))
