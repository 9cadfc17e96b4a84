"""I420 <-> RGB on the host: the arithmetic of prisma_amd/csrc/yuv.hip in numpy, for what needs no GPU or is small and rare - a .y4m
FrameReader's `[i]`, a VideoWriter's `write(rgb)`, the flow bands' mask videos.  8 bit, BT.601 limited range, the published integer form
(against swscale PARITY UNPINNED, an LSB or two); tests/yuv_ref.py pins it.

A frame is H W bytes of Y, then ceil(H / 2) ceil(W / 2) bytes of Cb, then as many of Cr.  A chroma sample is computed from the rounded
mean of its 2 x 2 block (indices clamped to the frame) and read back by the block's four pixels (nearest).

Clips come in other layouts too - 4:2:2, 4:4:4, mono, 9 - 16 bit, full range, BT.709: yuv_to_rgb at the end of this file decodes any of them
(prisma_amd/csrc/yuv_formats.hip on the host), and rgb_to_yuv encodes to any of them (prisma_amd/csrc/yuv_out.hip on the host)."""
import collections

import numpy as np


def i420_bytes(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def rgb_to_i420(rgb, out=None):
    """uint8 [H, W, 3] -> uint8 [i420_bytes(H, W)] (`out`: the caller's buffer)"""
    h, w = rgb.shape[:2]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if out is None:
        out = np.empty(i420_bytes(h, w), np.uint8)
    v = rgb.astype(np.int32)
    out[:h * w] = (((66 * v[..., 0] + 129 * v[..., 1] + 25 * v[..., 2] + 128) >> 8) + 16).reshape(-1)
    if h & 1 or w & 1:
        v = np.pad(v, ((0, h & 1), (0, w & 1), (0, 0)), mode="edge")
    m = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    out[h * w:h * w + ch * cw] = (((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128).reshape(-1)
    out[h * w + ch * cw:] = (((112 * r - 94 * g - 18 * b + 128) >> 8) + 128).reshape(-1)
    return out


def i420_to_rgb(yuv, h, w):
    """uint8 [i420_bytes(H, W)] -> uint8 [H, W, 3]"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    yuv = np.asarray(yuv).reshape(-1)
    c = 298 * (yuv[:h * w].reshape(h, w).astype(np.int32) - 16) + 128
    up = lambda p: np.repeat(np.repeat(p.reshape(ch, cw).astype(np.int32) - 128, 2, axis=0), 2, axis=1)[:h, :w]      # noqa: E731 - nearest
    d, e = up(yuv[h * w:h * w + ch * cw]), up(yuv[h * w + ch * cw:])
    rgb = np.empty((h, w, 3), np.uint8)
    rgb[..., 0] = np.clip((c + 409 * e) >> 8, 0, 255)
    rgb[..., 1] = np.clip((c - 100 * d - 208 * e) >> 8, 0, 255)
    rgb[..., 2] = np.clip((c + 516 * d) >> 8, 0, 255)
    return rgb


# ---- every planar layout a .y4m can have, to RGB (the way in only) ----------------------------------------------------------------------------
# prisma_amd/csrc/yuv_formats.hip in numpy (include/prisma_bands.h pb_yuv_fmt has the rule; tests/yuv_fmt_ref.py pins both): chroma 400 / 420 /
# 422 / 444, depth 8 .. 16 (a byte per sample at 8, else a 16-bit little-endian word, read whole), limited or full range, "bt601" or "bt709".
# A format is any 4-tuple (chroma, depth, full_range, matrix) - the engine's YuvFormat is one; this module needs no engine.
Format = collections.namedtuple("Format", "chroma depth full_range matrix")
I420 = Format(420, 8, False, "bt601")
_SHIFTS = {400: None, 420: (1, 1), 422: (1, 0), 444: (0, 0)}      # (sx, sy) of the chroma planes
_MATRICES = {"bt601": (299, 114, 1000), "bt709": (2126, 722, 10000)}      # Kr, Kb as numerator, numerator, denominator


def _plane_shapes(fmt, h, w):
    """((ch, cw) of a chroma plane or None, bytes per sample)"""
    chroma, depth = int(fmt[0]), int(fmt[1])
    if chroma not in _SHIFTS or not 8 <= depth <= 16 or fmt[3] not in _MATRICES:
        raise ValueError("no such YUV format: %r" % (tuple(fmt),))
    s = _SHIFTS[chroma]
    return (None if s is None else (-(-h >> s[1]), -(-w >> s[0]))), 1 if depth == 8 else 2


def yuv_bytes(fmt, h, w):
    c, bps = _plane_shapes(fmt, h, w)
    return (h * w + (0 if c is None else 2 * c[0] * c[1])) * bps


def yuv_coeffs(fmt):
    """(cy, crv, cgu, cgv, cbu, yoff, coff): exact rationals rounded half up, floor((2 p + q) / (2 q)), in Python's integers"""
    _plane_shapes(fmt, 1, 1)
    d, full = int(fmt[1]), bool(fmt[2])
    kr, kb, den = _MATRICES[fmt[3]]
    kg = den - kr - kb
    top = (1 << d) - 1
    yn, yd, cd = (255 << d, top, top) if full else (255 * 256, 219, 224)      # 2^d sy = yn / yd, 2^d sc = yn / cd
    rhu = lambda p, q: (2 * p + q) // (2 * q)      # noqa: E731
    return (rhu(yn, yd), rhu(yn * 2 * (den - kr), cd * den), rhu(yn * 2 * kb * (den - kb), cd * den * kg),
            rhu(yn * 2 * kr * (den - kr), cd * den * kg), rhu(yn * 2 * (den - kb), cd * den), 0 if full else 16 << (d - 8), 1 << (d - 1))


def yuv_to_rgb(fmt, yuv, h, w):
    """uint8 [yuv_bytes(fmt, H, W)] -> uint8 [H, W, 3]"""
    c, bps = _plane_shapes(fmt, h, w)
    cy, crv, cgu, cgv, cbu, yoff, coff = yuv_coeffs(fmt)
    d = int(fmt[1])
    yuv = np.ascontiguousarray(yuv, np.uint8).reshape(-1)
    if yuv.size != yuv_bytes(fmt, h, w):
        raise ValueError("a %d x %d frame of %r is %d bytes, not %d" % (h, w, tuple(fmt), yuv_bytes(fmt, h, w), yuv.size))
    v = (yuv if bps == 1 else yuv.view("<u2")).astype(np.int32)
    lum = cy * (v[:h * w].reshape(h, w) - yoff) + (1 << (d - 1))
    if c is None:
        dd = ee = np.zeros((h, w), np.int32)
    else:
        sx, sy = _SHIFTS[int(fmt[0])]
        n = c[0] * c[1]
        up = lambda p: np.repeat(np.repeat(p.reshape(c) - coff, 1 << sy, axis=0), 1 << sx, axis=1)[:h, :w]      # noqa: E731 - nearest
        dd, ee = up(v[h * w:h * w + n]), up(v[h * w + n:])
    rgb = np.empty((h, w, 3), np.uint8)
    rgb[..., 0] = np.clip((lum + crv * ee) >> d, 0, 255)
    rgb[..., 1] = np.clip((lum - cgu * dd - cgv * ee) >> d, 0, 255)
    rgb[..., 2] = np.clip((lum + cbu * dd) >> d, 0, 255)
    return rgb


# ---- RGB to every one of those layouts (the way out) -------------------------------------------------------------------------------------------
# prisma_amd/csrc/yuv_out.hip in numpy (include/prisma_bands.h pb_rgb_to_yuv has the rule; tests/yuv_out_ref.py pins both), for frames that reach a
# writer on the host: a VideoWriter's `write(rgb)`, the flow bands' consistency-mask videos.
def yuv_fwd_coeffs(fmt):
    """(yr, yg, yb, ur, ug, h, vg, vb, F, yoff, coff, 2^d - 1): exact rationals rounded half up in Python's integers; the G terms are remainders"""
    _plane_shapes(fmt, 1, 1)
    d, full = int(fmt[1]), bool(fmt[2])
    kr, kb, den = _MATRICES[fmt[3]]
    f = 8 if (d, full, fmt[3]) == (8, False, "bt601") else 24 - d      # the one exception: the published 8-bit integers of rgb_to_i420
    top = (1 << d) - 1
    yn, cn = ((top, top) if full else (219 << (d - 8), 224 << (d - 8)))      # 255 ys, 255 cs
    yn, cn = yn << f, cn << f
    rhu = lambda p, q: (2 * p + q) // (2 * q)      # noqa: E731
    yr, yb = rhu(yn * kr, 255 * den), rhu(yn * kb, 255 * den)
    h = rhu(cn, 510)
    ur, vb = rhu(cn * kr, 510 * (den - kb)), rhu(cn * kb, 510 * (den - kr))
    return (yr, rhu(yn, 255) - yr - yb, yb, ur, h - ur, h, h - vb, vb, f, 0 if full else 16 << (d - 8), 1 << (d - 1), top)


def rgb_to_yuv(fmt, rgb, out=None):
    """uint8 [H, W, 3] -> uint8 [yuv_bytes(fmt, H, W)] (`out`: the caller's buffer); a 16-bit sample is two bytes, little-endian"""
    rgb = np.asarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    c, bps = _plane_shapes(fmt, h, w)
    if out is None:
        out = np.empty(yuv_bytes(fmt, h, w), np.uint8)
    if out.shape != (yuv_bytes(fmt, h, w),) or out.dtype != np.uint8:
        raise ValueError("a %d x %d frame of %r is %d bytes, not %r %s" % (h, w, tuple(fmt), yuv_bytes(fmt, h, w), out.shape, out.dtype))
    yr, yg, yb, ur, ug, hh, vg, vb, f, yoff, coff, top = yuv_fwd_coeffs(fmt)
    rnd = 1 << (f - 1)
    planes = out if bps == 1 else out.view("<u2")
    v = rgb.astype(np.int32)
    planes[:h * w] = np.clip(((yr * v[..., 0] + yg * v[..., 1] + yb * v[..., 2] + rnd) >> f) + yoff, 0, top).reshape(-1)
    if c is None:
        return out
    sx, sy = _SHIFTS[int(fmt[0])]
    ph, pw = (c[0] << sy) - h, (c[1] << sx) - w
    if ph or pw:
        v = np.pad(v, ((0, ph), (0, pw), (0, 0)), mode="edge")      # indices clamped to the frame
    m = sum(v[dy::1 << sy, dx::1 << sx] for dy in range(1 << sy) for dx in range(1 << sx))
    m = (m + ((1 << (sx + sy)) >> 1)) >> (sx + sy)
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    n = c[0] * c[1]
    planes[h * w:h * w + n] = np.clip(((hh * b - ur * r - ug * g + rnd) >> f) + coff, 0, top).reshape(-1)
    planes[h * w + n:] = np.clip(((hh * r - vg * g - vb * b + rnd) >> f) + coff, 0, top).reshape(-1)
    return out
