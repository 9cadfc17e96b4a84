"""I420 <-> RGB on the host: the arithmetic of prisma_amd/csrc/yuv.hip in numpy, for what needs no GPU or is small and rare - a .y4m
FrameReader's `[i]`, a VideoWriter's `write(rgb)`, the flow bands' mask videos.  8 bit, BT.601 limited range, the published integer form
(against swscale PARITY UNPINNED, an LSB or two); tests/yuv_ref.py pins it.

A frame is H W bytes of Y, then ceil(H / 2) ceil(W / 2) bytes of Cb, then as many of Cr.  A chroma sample is computed from the rounded
mean of its 2 x 2 block (indices clamped to the frame) and read back by the block's four pixels (nearest)."""
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
