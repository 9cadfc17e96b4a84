"""Restatement of the project's RGB -> planar YUV arithmetic for every .y4m layout (include/prisma_bands.h pb_rgb_to_yuv), the way
tests/yuv_fmt_ref.py restates the read direction: written from the rule, sharing no code with bands/common/yuv.py or prisma_amd/csrc/yuv_out.hip.
Coefficients are fractions.Fraction values rounded half up, pixels int64 numpy.

A format is (chroma, depth, full_range, matrix) as in yuv_fmt_ref; plane order, plane sizes, sample size, yoff and coff are the read direction's.
  scales    limited: ys = 219 2^(d - 8) / 255, cs = 224 2^(d - 8) / 255; full: ys = cs = (2^d - 1) / 255; F = 24 - d, but 8 for {8, limited, bt601}
  table     yr = rhu(2^F ys Kr), yb = rhu(2^F ys Kb), yg = rhu(2^F ys) - yr - yb; h = rhu(2^F cs / 2),
            ur = rhu(2^F cs Kr / (2 (1 - Kb))), ug = h - ur, vb = rhu(2^F cs Kb / (2 (1 - Kr))), vg = h - vb
  samples   Y = clamp(((yr R + yg G + yb B + 2^(F-1)) >> F) + yoff) per pixel; Cb = clamp(((-ur R - ug G + h B + 2^(F-1)) >> F) + coff),
            Cr = clamp(((h R - vg G - vb B + 2^(F-1)) >> F) + coff) per chroma sample, of the rounded mean colour of the pixels it covers
            (indices clamped to the frame); clamp to 0 .. 2^d - 1
`to_yuv_real` is the same conversion in real numbers (float64, nothing rounded or clamped) of the same block-mean colours."""
from fractions import Fraction

import numpy as np

import yuv_fmt_ref as R


def frac_bits(fmt):
    _, d, full, m = fmt
    return 8 if (d == 8 and not full and m == "bt601") else 24 - d


def out_scales(fmt):
    """(ys, cs): code steps per unit of R, G, B - the inverse of yuv_fmt_ref.scales"""
    _, d, full, _ = fmt
    if full:
        return Fraction(2 ** d - 1, 255), Fraction(2 ** d - 1, 255)
    return Fraction(219 * 2 ** (d - 8), 255), Fraction(224 * 2 ** (d - 8), 255)


def real_fwd(fmt):
    """((yr, yg, yb), (ur, ug, h), (h, vg, vb)) as exact fractions: Y' = yr R + yg G + yb B, Cb' = -ur R - ug G + h B, Cr' = h R - vg G - vb B"""
    kr, kb = R.K[fmt[3]]
    kg = 1 - kr - kb
    ys, cs = out_scales(fmt)
    return ((ys * kr, ys * kg, ys * kb), (cs * kr / (2 * (1 - kb)), cs * kg / (2 * (1 - kb)), cs / 2), (cs / 2, cs * kg / (2 * (1 - kr)), cs * kb / (2 * (1 - kr))))


def fwd_coeffs(fmt):
    """(yr, yg, yb, ur, ug, h, vg, vb, F, yoff, coff, 2^d - 1) of the integer form"""
    kr, kb = R.K[fmt[3]]
    ys, cs = out_scales(fmt)
    one = 2 ** frac_bits(fmt)
    yr, yb = R.round_half_up(one * ys * kr), R.round_half_up(one * ys * kb)
    yg = R.round_half_up(one * ys) - yr - yb
    h = R.round_half_up(one * cs / 2)
    ur = R.round_half_up(one * cs * kr / (2 * (1 - kb)))
    vb = R.round_half_up(one * cs * kb / (2 * (1 - kr)))
    _, _, yoff, coff = R.scales(fmt)
    return yr, yg, yb, ur, h - ur, h, h - vb, vb, frac_bits(fmt), yoff, coff, 2 ** fmt[1] - 1


def block_means(fmt, rgb):
    """int64 [..., ch, cw, 3]: the rounded mean colour under every chroma sample, pixel indices clamped to the frame (None for 400)"""
    if fmt[0] == 400:
        return None
    sx, sy = R.SUB[fmt[0]]
    v = np.asarray(rgb).astype(np.int64)
    H, W = v.shape[-3:-1]
    ch, cw = R.chroma_shape(fmt, H, W)
    acc = np.zeros(v.shape[:-3] + (ch, cw, 3), np.int64)
    for dy in range(2 ** sy):
        for dx in range(2 ** sx):
            yy = np.minimum(np.arange(ch) * 2 ** sy + dy, H - 1)
            xx = np.minimum(np.arange(cw) * 2 ** sx + dx, W - 1)
            acc += v[..., yy[:, None], xx[None, :], :]
    count = 2 ** (sx + sy)
    return (acc + count // 2) // count


def samples(fmt, rgb):
    """(Y [..., H, W], Cb, Cr [..., ch, cw] or None, None) int64 code values of uint8 [..., H, W, 3]"""
    yr, yg, yb, ur, ug, h, vg, vb, F, yoff, coff, top = fwd_coeffs(fmt)
    half = 2 ** (F - 1)
    clamp = lambda a: np.minimum(np.maximum(a, 0), top)      # noqa: E731
    v = np.asarray(rgb).astype(np.int64)
    # floor division by 2^F: what an arithmetic shift does to a negative value too
    y = clamp((yr * v[..., 0] + yg * v[..., 1] + yb * v[..., 2] + half) // 2 ** F + yoff)
    m = block_means(fmt, rgb)
    if m is None:
        return y, None, None
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    return y, clamp((-ur * r - ug * g + h * b + half) // 2 ** F + coff), clamp((h * r - vg * g - vb * b + half) // 2 ** F + coff)


def rgb_to_yuv(fmt, rgb):
    """uint8 [..., H, W, 3] -> packed frames uint8 [..., yuv_fmt_ref.frame_bytes(fmt, H, W)]"""
    return R.pack(fmt, *samples(fmt, rgb))


def to_yuv_real(fmt, rgb):
    """float64 (Y, Cb, Cr) (Cb = Cr = None for 400), not rounded and not clamped, of the colours the integer form converts: the pixel for Y, the
    rounded block mean for Cb and Cr"""
    (yr, yg, yb), (ur, ug, h), (h2, vg, vb) = [[float(c) for c in row] for row in real_fwd(fmt)]
    _, _, yoff, coff = R.scales(fmt)
    v = np.asarray(rgb).astype(np.float64)
    y = yr * v[..., 0] + yg * v[..., 1] + yb * v[..., 2] + yoff
    m = block_means(fmt, rgb)
    if m is None:
        return y, None, None
    r, g, b = (m[..., i].astype(np.float64) for i in range(3))
    return y, -ur * r - ug * g + h * b + coff, h2 * r - vg * g - vb * b + coff
