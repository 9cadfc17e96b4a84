"""Restatement of the project's I420 <-> RGB arithmetic (numpy, int64), the way tests/rgbd_ref.py restates the hue decode: the
published 8-bit integer form of BT.601, limited range.  It pins prisma_amd/csrc/yuv.hip (the kernels) and bands/common/yuv.py
(the host side of the .y4m reader and writer); it shares no code with either.

RGB -> I420      Y  = ((66 R + 129 G + 25 B + 128) >> 8) + 16                per pixel
                 Cb = ((-38 R - 74 G + 112 B + 128) >> 8) + 128              per 2 x 2 block
                 Cr = ((112 R - 94 G - 18 B + 128) >> 8) + 128               per 2 x 2 block
                 with R, G, B of a block = (sum of its 4 samples + 2) >> 2, pixel indices clamped to the frame
I420 -> RGB      C = Y - 16, D = Cb - 128, E = Cr - 128, chroma of pixel (x, y) = plane[y >> 1][x >> 1]
                 R = clip8((298 C + 409 E + 128) >> 8)
                 G = clip8((298 C - 100 D - 208 E + 128) >> 8)
                 B = clip8((298 C + 516 D + 128) >> 8)
`>>` is numpy's arithmetic shift on int64 (floor).  A frame is H W luma bytes, then ceil(H / 2) ceil(W / 2) bytes of Cb, then of Cr."""
import numpy as np


def chroma_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def i420_bytes(H, W):
    ch, cw = chroma_size(H, W)
    return H * W + 2 * ch * cw


def luma(r, g, b):
    """Y of int64 R, G, B arrays"""
    return ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16


def chroma(r, g, b):
    """(Cb, Cr) of int64 block-mean R, G, B arrays"""
    return ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128, ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128


def colour(y, cb, cr):
    """(R, G, B) uint8 of int64 Y, Cb, Cr arrays"""
    c, d, e = y - 16, cb - 128, cr - 128
    r = (298 * c + 409 * e + 128) >> 8
    g = (298 * c - 100 * d - 208 * e + 128) >> 8
    b = (298 * c + 516 * d + 128) >> 8
    return tuple(np.clip(v, 0, 255).astype(np.uint8) for v in (r, g, b))


def planes(yuv, H, W):
    """(Y [..., H, W], Cb, Cr [..., ch, cw]) views of packed I420 frames [..., i420_bytes(H, W)]"""
    ch, cw = chroma_size(H, W)
    lead = yuv.shape[:-1]
    assert yuv.shape[-1] == i420_bytes(H, W), (yuv.shape, H, W)
    return (yuv[..., :H * W].reshape(lead + (H, W)), yuv[..., H * W:H * W + ch * cw].reshape(lead + (ch, cw)),
            yuv[..., H * W + ch * cw:].reshape(lead + (ch, cw)))


def rgb_to_i420(rgb):
    """uint8 [..., H, W, 3] -> uint8 [..., i420_bytes(H, W)]"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.shape[-1] == 3
    H, W = rgb.shape[-3:-1]
    ch, cw = chroma_size(H, W)
    lead = rgb.shape[:-3]
    v = rgb.astype(np.int64)
    y = luma(v[..., 0], v[..., 1], v[..., 2])
    yi = np.minimum(np.arange(2 * ch), H - 1)                   # clamped indices: the last row / column again on odd sizes
    xi = np.minimum(np.arange(2 * cw), W - 1)
    p = v[..., yi, :, :][..., xi, :].reshape(lead + (ch, 2, cw, 2, 3))
    m = (p.sum(axis=(-4, -2)) + 2) >> 2
    cb, cr = chroma(m[..., 0], m[..., 1], m[..., 2])
    out = np.concatenate([a.reshape(lead + (-1,)) for a in (y, cb, cr)], axis=-1)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def i420_to_rgb(yuv, H, W):
    """uint8 [..., i420_bytes(H, W)] -> uint8 [..., H, W, 3]"""
    yuv = np.asarray(yuv)
    assert yuv.dtype == np.uint8
    y, cb, cr = planes(yuv, H, W)
    yi, xi = np.arange(H) >> 1, np.arange(W) >> 1
    up = lambda p: p[..., yi, :][..., xi].astype(np.int64)      # noqa: E731 - nearest
    return np.stack(colour(y.astype(np.int64), up(cb), up(cr)), axis=-1)
