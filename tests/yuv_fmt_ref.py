"""Restatement of the project's planar YUV -> RGB arithmetic for every .y4m layout (include/prisma_bands.h pb_yuv_fmt), the way tests/yuv_ref.py
restates the I420 pair: written from the rule, sharing no code with bands/common/yuv.py or prisma_amd/csrc/yuv_formats.hip.  Coefficients are
fractions.Fraction values rounded half up, pixels int64 numpy.

A format is (chroma, depth, full_range, matrix): chroma 400 / 420 / 422 / 444, depth 8 .. 16, matrix "bt601" / "bt709".
  samples   one byte at depth 8, else a 16-bit little-endian word, read whole (not masked)
  planes    Y [H, W], then Cb and Cr [ceil(H / 2^sy), ceil(W / 2^sx)], (sx, sy) = (1, 1) / (1, 0) / (0, 0) for 420 / 422 / 444; none for 400
  pixel     C = Y - yoff, D = Cb - coff, E = Cr - coff of plane[y >> sy][x >> sx] (D = E = 0 for 400)
            R = clip8((cy C + crv E + half) >> d), G = clip8((cy C - cgu D - cgv E + half) >> d), B = clip8((cy C + cbu D + half) >> d)
`to_rgb_real` is the same conversion in real numbers (float64, nothing rounded): what the integers approximate to within 1.5."""
import itertools
from fractions import Fraction

import numpy as np

CHROMAS = (400, 420, 422, 444)
MATRICES = ("bt601", "bt709")
K = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}
SUB = {420: (1, 1), 422: (1, 0), 444: (0, 0)}


def all_formats(depths=range(8, 17)):
    return [(c, d, bool(f), m) for c, d, f, m in itertools.product(CHROMAS, depths, (0, 1), MATRICES)]


def round_half_up(q):
    q = Fraction(q)
    return (2 * q.numerator + q.denominator) // (2 * q.denominator)


def scales(fmt):
    """(sy, sc, yoff, coff) as exact numbers: output units per luma / chroma code step, and the codes of black and of no colour"""
    _, d, full, _ = fmt
    if full:
        return Fraction(255, 2 ** d - 1), Fraction(255, 2 ** d - 1), 0, 2 ** (d - 1)
    return Fraction(255, 219 * 2 ** (d - 8)), Fraction(255, 224 * 2 ** (d - 8)), 16 * 2 ** (d - 8), 2 ** (d - 1)


def real_coeffs(fmt):
    """(y, rv, gu, gv, bu): R = y C + rv E, G = y C - gu D - gv E, B = y C + bu D in real numbers"""
    kr, kb = K[fmt[3]]
    kg = 1 - kr - kb
    sy, sc, _, _ = scales(fmt)
    return sy, sc * 2 * (1 - kr), sc * 2 * kb * (1 - kb) / kg, sc * 2 * kr * (1 - kr) / kg, sc * 2 * (1 - kb)


def coeffs(fmt):
    """(cy, crv, cgu, cgv, cbu, yoff, coff) of the integer form"""
    _, _, yoff, coff = scales(fmt)
    return tuple(round_half_up(2 ** fmt[1] * c) for c in real_coeffs(fmt)) + (yoff, coff)


def chroma_shape(fmt, H, W):
    if fmt[0] == 400:
        return None
    sx, sy = SUB[fmt[0]]
    return -(-H // 2 ** sy), -(-W // 2 ** sx)


def frame_bytes(fmt, H, W):
    c = chroma_shape(fmt, H, W)
    return (H * W + (2 * c[0] * c[1] if c else 0)) * (1 if fmt[1] == 8 else 2)


def planes(fmt, yuv, H, W):
    """(Y [..., H, W], Cb, Cr [..., ch, cw] or None, None) as int64, of packed frames uint8 [..., frame_bytes]"""
    yuv = np.asarray(yuv)
    assert yuv.dtype == np.uint8 and yuv.shape[-1] == frame_bytes(fmt, H, W), (yuv.shape, fmt, H, W)
    lead = yuv.shape[:-1]
    if fmt[1] == 8:
        v = yuv.astype(np.int64)
    else:
        b = yuv.reshape(lead + (-1, 2)).astype(np.int64)
        v = b[..., 0] + 256 * b[..., 1]
    c = chroma_shape(fmt, H, W)
    y = v[..., :H * W].reshape(lead + (H, W))
    if c is None:
        return y, None, None
    n = c[0] * c[1]
    return y, v[..., H * W:H * W + n].reshape(lead + c), v[..., H * W + n:].reshape(lead + c)


def pack(fmt, y, cb=None, cr=None):
    """sample arrays [..., H, W] (+ [..., ch, cw] twice) -> packed frames uint8 [..., frame_bytes]"""
    parts = [np.asarray(p) for p in ((y,) if fmt[0] == 400 else (y, cb, cr))]
    lead = parts[0].shape[:-2]
    v = np.concatenate([p.reshape(lead + (-1,)) for p in parts], axis=-1)
    if fmt[1] == 8:
        return v.astype(np.uint8)
    return np.stack([v & 255, v >> 8], axis=-1).astype(np.uint8).reshape(lead + (-1,))


def _pixelwise(fmt, yuv, H, W):
    """(Y, Cb, Cr) per pixel, int64 [..., H, W]: the chroma of pixel (x, y) is plane[y >> sy][x >> sx]; for 400 None"""
    y, cb, cr = planes(fmt, yuv, H, W)
    if cb is None:
        return y, None, None
    sx, sy = SUB[fmt[0]]
    yy, xx = np.arange(H) >> sy, np.arange(W) >> sx
    return y, cb[..., yy[:, None], xx[None, :]], cr[..., yy[:, None], xx[None, :]]


def colour(fmt, y, cb, cr):
    """int64 arrays of code values -> (R, G, B) int64 in 0 .. 255, the integer form"""
    cy, crv, cgu, cgv, cbu, yoff, coff = coeffs(fmt)
    d = fmt[1]
    half = 2 ** (d - 1)
    c = np.asarray(y, np.int64) - yoff
    dd = np.zeros_like(c) if cb is None else np.asarray(cb, np.int64) - coff
    ee = np.zeros_like(c) if cr is None else np.asarray(cr, np.int64) - coff
    clip8 = lambda a: np.minimum(np.maximum(a, 0), 255)      # noqa: E731
    # floor division by 2^d: what an arithmetic shift does to a negative value too
    return (clip8((cy * c + crv * ee + half) // 2 ** d), clip8((cy * c - cgu * dd - cgv * ee + half) // 2 ** d), clip8((cy * c + cbu * dd + half) // 2 ** d))


def colour_real(fmt, y, cb, cr):
    """the same in real numbers: float64 (R, G, B), not rounded and not clipped"""
    fy, rv, gu, gv, bu = (float(c) for c in real_coeffs(fmt))
    _, _, yoff, coff = scales(fmt)
    c = np.asarray(y, np.float64) - yoff
    dd = np.zeros_like(c) if cb is None else np.asarray(cb, np.float64) - coff
    ee = np.zeros_like(c) if cr is None else np.asarray(cr, np.float64) - coff
    return fy * c + rv * ee, fy * c - gu * dd - gv * ee, fy * c + bu * dd


def to_rgb(fmt, yuv, H, W):
    """packed frames uint8 [..., frame_bytes(fmt, H, W)] -> uint8 [..., H, W, 3]"""
    return np.stack(colour(fmt, *_pixelwise(fmt, yuv, H, W)), axis=-1).astype(np.uint8)
