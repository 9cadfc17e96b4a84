"""Bilinear RGB resize on the host: the arithmetic of prisma_amd/csrc/resize.hip in numpy, for what is small and rare - the frames a
rescaling .y4m VideoWriter gets as RGB (the flow bands' mask videos and trailing zero frame).  8 bit, exact integers, half-pixel centres, the
same two taps for a shrink (include/prisma_bands.h, pb_rgb_resize; against swscale PARITY UNPINNED); tests/resize_ref.py pins it."""
import numpy as np


def taps(n_in, n_out):
    """per output index: the two clamped source indices and the weight (0 .. 256) of the second"""
    num = (2 * np.arange(n_out, dtype=np.int64) + 1) * n_in - n_out
    i0 = num // (2 * n_out)                                     # floor, also of a negative num
    w = (256 * (num - i0 * 2 * n_out) + n_out) // (2 * n_out)
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), w.astype(np.int32)


def resize_rgb(rgb, height, width):
    """uint8 [sh, sw, 3] -> uint8 [height, width, 3]"""
    rgb = np.asarray(rgb, np.uint8)
    sh, sw = rgb.shape[:2]
    ya, yb, wy = taps(sh, height)
    xa, xb, wx = taps(sw, width)
    p = rgb.astype(np.int32)
    wx, wy = wx[None, :, None], wy[:, None, None]
    rows = (256 - wx) * p[:, xa] + wx * p[:, xb]                # every source row at the output width, not yet rounded
    return (((256 - wy) * rows[ya] + wy * rows[yb] + 32768) >> 16).astype(np.uint8)
