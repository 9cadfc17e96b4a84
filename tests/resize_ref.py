"""Restatement of the project's bilinear RGB resize (Python integers for the taps, int64 for the pixels, no floats), the way tests/yuv_ref.py
restates the colour conversion.  It pins prisma_amd/csrc/resize.hip (the kernels) and bands/common/resize.py (the host side of a rescaling
.y4m writer); it shares no code with either.

Half-pixel centres.  Per axis, for output index x of n_out from n_in samples:
    num = (2 x + 1) n_in - n_out                    (may be negative)
    i0  = floor(num / (2 n_out)),  r = num - i0 * 2 n_out      (0 <= r < 2 n_out)
    w   = (256 r + n_out) // (2 n_out)              (0 .. 256)
    taps clamp(i0, 0, n_in - 1) and clamp(i0 + 1, 0, n_in - 1)
Per channel, with p00 p01 the taps of row i0 and p10 p11 those of row i0 + 1:
    out = ((256 - wy) ((256 - wx) p00 + wx p01) + wy ((256 - wx) p10 + wx p11) + 32768) >> 16

`bug=` states a wrong resize on purpose, for the mutation tests (tests/test_resize_ref_cpu.py: every one of them must differ from the
restatement on a shape the GPU tests use):
    corner        align-corners geometry: output 0 sits on sample 0 and the last output on the last sample
    floor         no + 32768: the result is truncated
    nearest       the nearer tap alone
    swap_xy       the horizontal weight applied vertically and the other way round
    wrap          no clamp: the taps wrap round the frame
    chroma_first  (resize_i420 only) the I420 planes of the source are resized instead of its RGB"""
import numpy as np

import yuv_ref

BUGS = ("corner", "floor", "nearest", "swap_xy", "wrap", "chroma_first")


def axis(n_in, n_out, bug=None):
    """three lists of Python integers per output index: first tap, second tap, weight of the second (0 .. 256)"""
    a, b, w = [], [], []
    for x in range(n_out):
        if bug == "corner":         # x (n_in - 1) / (n_out - 1) in the same 8-bit fixed point
            num, den = (x * (n_in - 1), n_out - 1) if n_out > 1 else (0, 1)
        else:
            num, den = (2 * x + 1) * n_in - n_out, 2 * n_out
        i0 = num // den             # Python's // floors
        r = num - i0 * den
        assert 0 <= r < den
        wt = (256 * r + den // 2) // den
        assert 0 <= wt <= 256
        if bug == "nearest":
            wt = 256 if wt >= 128 else 0
        if bug == "wrap":
            t0, t1 = i0 % n_in, (i0 + 1) % n_in
        else:
            t0, t1 = min(max(i0, 0), n_in - 1), min(max(i0 + 1, 0), n_in - 1)
        a.append(t0)
        b.append(t1)
        w.append(wt)
    return a, b, w


def resize(rgb, H, W, bug=None):
    """uint8 [..., sh, sw, C] -> uint8 [..., H, W, C]"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim >= 3
    sh, sw = rgb.shape[-3:-1]
    ya, yb, wy = (np.array(v, np.int64) for v in axis(sh, H, bug))
    xa, xb, wx = (np.array(v, np.int64) for v in axis(sw, W, bug))
    wy, wx = wy[:, None, None], wx[None, :, None]
    if bug == "swap_xy":
        wy, wx = np.broadcast_to(wx, (H, W, 1)), np.broadcast_to(wy, (H, W, 1))
    p = rgb.astype(np.int64)
    p00, p01 = p[..., ya, :, :][..., xa, :], p[..., ya, :, :][..., xb, :]
    p10, p11 = p[..., yb, :, :][..., xa, :], p[..., yb, :, :][..., xb, :]
    acc = (256 - wy) * ((256 - wx) * p00 + wx * p01) + wy * ((256 - wx) * p10 + wx * p11)
    assert acc.min() >= 0 and acc.max() + 32768 < 2 ** 31           # the kernels hold it in int32
    out = (acc + (0 if bug == "floor" else 32768)) >> 16
    assert out.max() <= 255
    return out.astype(np.uint8)


def resize_i420(rgb, H, W, bug=None):
    """uint8 [..., sh, sw, 3] -> packed I420 frames uint8 [..., i420_bytes(H, W)]: the colour conversion of the resized frames"""
    rgb = np.asarray(rgb)
    if bug == "chroma_first":
        sh, sw = rgb.shape[-3:-1]
        y, cb, cr = yuv_ref.planes(yuv_ref.rgb_to_i420(rgb), sh, sw)
        ch, cw = yuv_ref.chroma_size(H, W)
        lead = rgb.shape[:-3]
        return np.concatenate([resize(pl[..., None], h, w).reshape(lead + (-1,)) for pl, h, w in ((y, H, W), (cb, ch, cw), (cr, ch, cw))], axis=-1)
    return yuv_ref.rgb_to_i420(resize(rgb, H, W, bug))
