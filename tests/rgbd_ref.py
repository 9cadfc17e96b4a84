"""float64 restatement of the rgba band's RGB-D split (CPU only; a helper module of the tests, not a conftest).

split() of bands/rgba.py:24-75 with `--encoding_depth hue`: the depth half of a side-by-side frame is decoded as
clip(rgb_to_hsv(crop)[..., 0] / 360, 0, 1) and re-encoded as heat_to_rgb(.) * 255, truncated to uint8 by the video writer
(bands/common/encode.py:13-58).  Restated per pixel, numpy float64, one rounding per operation:

    r, g, b        the bytes as doubles;  mx, mn their max and min;  den = (mx - mn) + 2^-52
    r >= max(g, b) h = fmod((g - b) * 60 / den, 360), + 360 when negative         the FIRST maximum wins, like np.argmax
    else g >= b    h = (b - r) * 60 / den + 120
    else           h = (r - g) * 60 / den + 240
    d    = clip(h / 360, 0, 1)                                                     the heat value; float32(d) is what the ABI hands out
    hue6 = ((1 - d) * 0.65) * 6
    byte = trunc(clip(|fmod(hue6 + {0, 4, 2}[c], 6) - 3| - 1, 0, 1) * 255)

`fault=` plants one of the mistakes an implementation can make (FAULTS: name -> the number of the 2^24 colours on which it changes a byte;
the counts are properties of the reference, tests/test_rgbd_ref_cpu.py asserts them).
"""
from __future__ import annotations

import hashlib

import numpy as np

SIDES = ("left", "right", "top", "bottom")          # where the DEPTH is: pb_rgbd_boxes' side 0 .. 3
PX_PER_LANE = 4                                     # pixels one lane of hue_heat_kernel owns (elementwise.hip HH_PX)

FAULTS = {"float32": 137921,        # the whole formula in float32
          "mul_inv360": 51078,      # h * (1 / 360) instead of h / 360
          "inv_den_first": 2413,    # (g - b) * (60 / den): the quotient first
          "fold_3p9": 77202,        # (1 - d) * 3.9 instead of ((1 - d) * 0.65) * 6
          "round": 8395098,         # bytes rounded to nearest instead of truncated
          "no_mod": 2796160,        # the red branch without its % 360: negative hues clip to 0
          "last_max": 256}          # the LAST maximum channel wins: the greys land in the blue branch (h = 240)


def boxes(H: int, W: int, side):
    """(rgb_box, depth_box) of an H x W side-by-side frame, half-open (y0, y1, x0, x1); `side` (a name of SIDES or its index) is where the
    depth is.  The reference slices with int() of width / 2 and height / 2 (rgba.py:29-40, 58-59): the half that starts at the middle is
    one wider on an odd size.  An empty half is an error."""
    side = SIDES[side] if isinstance(side, int) and 0 <= side < 4 else side
    if side not in SIDES:
        raise ValueError("side %r: one of %s" % (side, ", ".join(SIDES)))
    if side in ("left", "right"):
        k = W // 2
        first, second = (0, H, 0, k), (0, H, k, W)
    else:
        k = H // 2
        first, second = (0, k, 0, W), (k, H, 0, W)
    if k < 1 or H < 1 or W < 1:
        raise ValueError("%d x %d frame has no %s half" % (H, W, side))
    return (second, first) if side in ("left", "top") else (first, second)


def hue_heat(crop_u8, fault=None):
    """crop [..., 3] uint8 -> (heat float64 [...], rgb uint8 [..., 3])"""
    assert fault is None or fault in FAULTS, fault
    ft = np.float32 if fault == "float32" else np.float64
    c = np.asarray(crop_u8)
    assert c.dtype == np.uint8 and c.shape[-1] == 3
    r, g, b = (c[..., k].astype(ft) for k in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    den = (mx - mn) + ft(2.0 ** -52)
    if fault == "inv_den_first":
        q = ft(60) / den
        hr, hg, hb = (g - b) * q, (b - r) * q + ft(120), (r - g) * q + ft(240)
    else:
        hr, hg, hb = (g - b) * ft(60) / den, (b - r) * ft(60) / den + ft(120), (r - g) * ft(60) / den + ft(240)
    if fault != "no_mod":
        hr = np.fmod(hr, ft(360))
        hr = np.where(hr < 0, hr + ft(360), hr)
    if fault == "last_max":
        h = np.where(b >= np.maximum(r, g), hb, np.where(g >= r, hg, hr))
    else:
        h = np.where(r >= np.maximum(g, b), hr, np.where(g >= b, hg, hb))
    d = h * (ft(1) / ft(360)) if fault == "mul_inv360" else h / ft(360)
    d = np.clip(d, ft(0), ft(1))
    hue6 = (ft(1) - d) * ft(3.9) if fault == "fold_3p9" else ((ft(1) - d) * ft(0.65)) * ft(6)
    out = np.empty(c.shape, np.uint8)
    for k, off in enumerate((0.0, 4.0, 2.0)):
        v = np.fmod(hue6 + ft(off), ft(6))
        v = np.clip(np.abs(v - ft(3)) - ft(1), ft(0), ft(1)) * ft(255)
        out[..., k] = (np.rint(v) if fault == "round" else v).astype(np.uint8)
    return d.astype(np.float64), out


def all_colours(lo: int = 0, hi: int = 1 << 24):
    """colours lo .. hi - 1 of the table in (r, g, b) order, r slowest: [hi - lo, 3] uint8"""
    i = np.arange(lo, hi, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8)


def table(fault=None, step: int = 1 << 20):
    """the full 2^24 table in chunks: yields (first colour index, heat float64 [step], rgb uint8 [step, 3])"""
    for lo in range(0, 1 << 24, step):
        d, o = hue_heat(all_colours(lo, lo + step), fault)
        yield lo, d, o


def table_sha256(fault=None) -> str:
    h = hashlib.sha256()
    for _, _, o in table(fault):
        h.update(o.tobytes())
    return h.hexdigest()


def sample_colours():
    """the fixture's sample: the 256 greys, the 1536 fully saturated ring colours (max 255, min 0), 4096 seeded random colours"""
    k = np.arange(256, dtype=np.uint8)
    z, f = np.zeros(256, np.uint8), np.full(256, 255, np.uint8)
    ring = [np.stack(t, -1) for t in ((f, k, z), (k[::-1], f, z), (z, f, k), (z, k[::-1], f), (k, z, f), (f, z, k[::-1]))]
    rnd = np.random.default_rng(20240).integers(0, 256, (4096, 3), dtype=np.uint8)
    return np.concatenate([np.stack([k, k, k], -1)] + ring + [rnd])


def make_frames(n: int, H: int, W: int, side, seed: int = 0):
    """n seeded side-by-side frames: random bytes, with greys and ring colours sprinkled over every fourth pixel"""
    g = np.random.default_rng(seed + 1000 * H + W)
    fr = g.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    s = sample_colours()[:256 + 1536]
    flat = fr.reshape(-1, 3)
    idx = np.arange(0, flat.shape[0], 4)
    flat[idx] = s[g.integers(0, len(s), len(idx))]
    return fr


def split_restated(frames, side, encoding="hue"):
    """frames [n, H, W, 3] -> (rgb crop, depth half as the band writes it, heat float64 or None)"""
    frames = np.asarray(frames)
    rb, db = boxes(frames.shape[1], frames.shape[2], side)
    rgb = frames[:, rb[0]:rb[1], rb[2]:rb[3]]
    dep = frames[:, db[0]:db[1], db[2]:db[3]]
    if encoding == "hue":
        heat, dep = hue_heat(dep)
        return rgb, dep, heat
    return rgb, dep, None
