"""Float64 truth and exact restatements for the flow bands' frame path outside the networks (CPU only; a helper module of the tests, not a
conftest): raft_prep_kernel - the first kernel of every flow_raft / flow_gmflow call - and the tail kernels flow_resize_back_kernel,
flow_encode_kernel and fwdbwd_mask_kernel (csrc/raft_kernels.hip).  Everything is built on the oracle's own functions
(oracle.raft_oracle: scaled_size, cubic_taps_u8, cv_resize_cubic_u8, pad_amounts, process_flow(exact_atan2=True), compute_fwdbwd_mask).

*_truth       float64 values with an element-wise tolerance derived from the kernel's float32 operation count
*_restated    the kernel operation by operation in numpy (integers, float32 without FMA), emitting the raw bytes the op entry points
              return; every planted fault is an argument (`bug`)
*_verify      the checks themselves: tests/test_gpu_flow_io_ops.py runs them on the kernels' output, tests/test_flow_io_ref_cpu.py on the
              restatements with and without the planted faults
"""
from __future__ import annotations

import numpy as np

import split_ref as S
from depth_ref import same_u8
from oracle import raft_oracle as O
from oracle.depth_oracle import _cubic_coeffs
from raft_ref import f16_step, maxd_of

F32 = np.float32
U24 = 2.0 ** -24            # one float32 rounding, relative to the magnitude it rounds
SLACK = 1.0 + 2.0 ** -20    # second-order terms of a handful of compounded roundings
GUARD_ROWS, GUARD = 8, 64

# (x / 255 - mean) / std with the values the reference's float32 tensors hold (gmflow/utils.py:53-58); RAFT: 2 (x / 255) - 1 (raft.py:91-92)
MEAN32 = np.array([0.485, 0.456, 0.406], F32)
STD32 = np.array([0.229, 0.224, 0.225], F32)
MEAN, STD = MEAN32.astype(np.float64), STD32.astype(np.float64)

# (H, W, scale, factor): issue table - no pad; odd pads, the smaller half on the left / top (factors 8 and 16); the two-scale model's factor;
# everything replicated; scaled and odd everywhere; a non-dyadic scale; a size the float32-widened scale gets wrong (4 x 10); an upscale with
# taps clamped at both borders; every tap clamped
PREP_CASES = [(8, 8, 1.0, 8), (13, 21, 1.0, 8), (13, 21, 1.0, 16), (33, 47, 1.0, 32), (1, 1, 1.0, 8), (45, 77, 0.75, 8), (40, 60, 0.6, 16),
              (15, 35, 0.3, 8), (20, 30, 1.5, 8), (2, 3, 0.75, 8)]
# (H, W, scale, (ih, iw)): flow_gmflow --inference_size; the last is the identity, where every weight is 0
PREP_ISZ_CASES = [(45, 77, 0.75, (32, 64)), (45, 77, 0.75, (64, 32)), (48, 80, 1.0, (48, 80))]
# the first inference-size case again on FULL-RANGE frames (prep_frames): the blend at full magnitude, the checker clamping at 0 and 255.  The
# share of elements with two admissible fp16 values is what full-range content gives (about 1e-2, reported, not capped)
PREP_ISZ_FULL = (45, 77, 0.75, (32, 64))
PREP_BUGS = ["pad_left", "clamp_sh", "swap_xy", "bgr", "no_round", "a_half", "no_half", "other_norm", "dydx", "scale_f32"]
N_FRAMES = 3


def prep_modes(factor: int):
    """(norm_mode, layout) as the bands run the factor: 8 is RAFT (fp16 and [hi | hi8 | lo8]), 16 / 32 GMFlow (fp16 and [hi | lo])"""
    return [(0, 0), (0, 2)] if factor == 8 else [(1, 0), (1, 1)]


def case_id(c) -> str:
    return "%dx%d-s%g-%s" % (c[0], c[1], c[2], "f%d" % c[3] if isinstance(c[3], int) else "to%dx%d" % c[3])


_CACHE: dict = {}


def prep_frames(H: int, W: int, dark: bool = False) -> np.ndarray:
    """three frames of differing content: noise, a 0 / 255 checker of 3 x 3 blocks (the cubic overshoot clamps at both ends), a ramp with noise.
    dark (the inference-size cases): the same content in 0 .. 31.  There an element's tolerance grows with the pixel value (the blend's
    roundings) while the fp16 spacing grows with the distance from the mean, so the share of elements whose tolerance straddles an fp16 tie is
    about 2 tol / spacing: 1e-2 for mid greys, 2e-3 for white, under 1e-3 only for dark pixels, |t| in 1.4 .. 2.2.  Neighbouring pixels still
    differ by up to 31 levels = 0.5 in t, 10^6 tolerances: a wrong weight or tap is as visible as in a full-range frame"""
    key = ("frames", H, W, dark)
    if key not in _CACHE:
        g = np.random.default_rng(1000 * H + W)
        f = np.empty((N_FRAMES, H, W, 3), np.uint8)
        f[0] = g.integers(0, 256, (H, W, 3))
        yy, xx = np.mgrid[0:H, 0:W]
        f[1] = ((((yy // 3) + (xx // 3)) & 1) * 255)[..., None]
        f[1, ..., 2] = 255 - f[1, ..., 2]
        ramp = (yy * 5 + xx * 3)[..., None] + np.array([0, 70, 140])
        f[2] = np.clip(ramp % 256 + g.integers(-6, 7, (H, W, 3)), 0, 255)
        _CACHE[key] = f >> 3 if dark else f
    return _CACHE[key]


# =====================================================================================================================
# the scaled frame: integer arithmetic, the oracle's rule with room for the planted faults
# =====================================================================================================================
def taps_u8(src: int, dst: int, scale: float, bug=None):
    """oracle.raft_oracle.cubic_taps_u8; bugs 'a_half' (A = -0.5), 'no_half' (no half-pixel offset)"""
    inv = 1.0 / scale
    d = np.arange(dst, dtype=np.float64)
    fx = (d * inv if bug == "no_half" else (d + 0.5) * inv - 0.5).astype(F32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(F32)
    idx = np.clip(sx[:, None] + np.arange(-1, 3)[None, :], 0, src - 1)
    if bug == "a_half":
        A, one = F32(-0.5), F32(1)
        c0 = ((A * (fx + one) - F32(5) * A) * (fx + one) + F32(8) * A) * (fx + one) - F32(4) * A
        c1 = ((A + F32(2)) * fx - (A + F32(3))) * fx * fx + one
        c2 = ((A + F32(2)) * (one - fx) - (A + F32(3))) * (one - fx) * (one - fx) + one
        c = np.stack([c0, c1, c2, one - c0 - c1 - c2], -1).astype(F32)
    else:
        c = _cubic_coeffs(fx)
    return idx, np.rint(c.astype(np.float64) * 2048.0).astype(np.int32)


def scaled_restated(frames: np.ndarray, scale: float, bug=None) -> np.ndarray:
    """frames [n, H, W, 3] -> [n, sh, sw, 3] uint8 as scaled_px computes it.  bugs: taps_u8's, 'scale_f32' (size and taps from the
    float32-widened scale), 'swap_xy' (each axis' table built for the other axis' lengths), 'no_round' (no 1 << 21)"""
    if scale == 1.0:
        return frames.copy()
    n, H, W, _ = frames.shape
    s = float(F32(scale)) if bug == "scale_f32" else scale
    sh, sw = O.scaled_size(H, W, s)
    tb = bug if bug in ("a_half", "no_half") else None
    if bug == "swap_xy":
        (xi, xc), (yi, yc) = taps_u8(H, sw, s), taps_u8(W, sh, s)
        xi, yi = np.minimum(xi, W - 1), np.minimum(yi, H - 1)
    else:
        (xi, xc), (yi, yc) = taps_u8(W, sw, s, tb), taps_u8(H, sh, s, tb)
    p = frames.astype(np.int64)
    acc = np.zeros((n, sh, sw, 3), np.int64)
    for ty in range(4):
        rows = p[:, yi[:, ty]]
        r = sum(rows[:, :, xi[:, tx]] * xc[None, None, :, tx, None].astype(np.int64) for tx in range(4))
        acc += r * yc[None, :, ty, None, None].astype(np.int64)
    return np.clip((acc + (0 if bug == "no_round" else 1 << 21)) >> 22, 0, 255).astype(np.uint8)


def scaled_oracle(frames: np.ndarray, scale: float) -> np.ndarray:
    return frames.copy() if scale == 1.0 else np.stack([O.cv_resize_cubic_u8(f, scale) for f in frames])


# =====================================================================================================================
# torch's align_corners=True source coordinates, in float32 as aten computes them
# =====================================================================================================================
def ac_coords(dst: int, src: int, fma: bool = False):
    """-> (i0, i1, l float32, 1 - l float32): scale = float(src - 1) / float(dst - 1) (0 for dst == 1), x = scale * float(d), i0 = int(x),
    i1 = i0 + (i0 < src - 1), l = x - i0, the complementary weight rounded to float32 on its own.  fma: l = fma(scale, d, -i0), the
    subtraction contracted with the product - the weight of the UNROUNDED coordinate beside the index of the rounded one (what the two
    kernels computed before these tests: 63 / 57 x 19 rounds to 21, l = -8.3e-7 instead of 0)"""
    sc = F32(src - 1) / F32(dst - 1) if dst > 1 else F32(0)
    x = (sc * np.arange(dst, dtype=F32)).astype(F32)
    i0 = x.astype(np.int64)
    l = (x - i0.astype(F32)).astype(F32)
    if fma:
        l = (np.float64(sc) * np.arange(dst) - i0).astype(F32)
    return i0, i0 + (i0 < src - 1), l, (F32(1) - l).astype(F32)


def _blend64(p, dst_h: int, dst_w: int, absolute: bool = False):
    """p [n, h, w, c] float64 -> [n, dst_h, dst_w, c]: the four-tap blend in float64 with the float32 weights (of |p| with absolute)"""
    h, w = p.shape[1:3]
    y0, y1, ly, my = ac_coords(dst_h, h)
    x0, x1, lx, mx = ac_coords(dst_w, w)
    p = np.abs(p) if absolute else p
    ly, my, lx, mx = (a.astype(np.float64) for a in (ly, my, lx, mx))
    top = p[:, y0][:, :, x0] * mx[None, None, :, None] + p[:, y0][:, :, x1] * lx[None, None, :, None]
    bot = p[:, y1][:, :, x0] * mx[None, None, :, None] + p[:, y1][:, :, x1] * lx[None, None, :, None]
    return top * my[None, :, None, None] + bot * ly[None, :, None, None]


def _blend32(p, dst_h: int, dst_w: int, fma: bool = False):
    """the kernels' expression in float32, every operation rounded: (1 - ly) ((1 - lx) p00 + lx p01) + ly ((1 - lx) p10 + lx p11)"""
    h, w = p.shape[1:3]
    y0, y1, ly, my = ac_coords(dst_h, h, fma)
    x0, x1, lx, mx = ac_coords(dst_w, w, fma)
    p = p.astype(F32)
    lx_, mx_, ly_, my_ = lx[None, None, :, None], mx[None, None, :, None], ly[None, :, None, None], my[None, :, None, None]
    top = (p[:, y0][:, :, x0] * mx_ + p[:, y0][:, :, x1] * lx_).astype(F32)
    bot = (p[:, y1][:, :, x0] * mx_ + p[:, y1][:, :, x1] * lx_).astype(F32)
    return (top * my_ + bot * ly_).astype(F32)


# =====================================================================================================================
# raft_prep_kernel
# =====================================================================================================================
def prep_geometry(H: int, W: int, scale: float, factor: int, isz=None) -> dict:
    """the oracle's plan: scaled_size, pad_amounts (InputPadder: the smaller half of the padding on the left / top)"""
    sh, sw = O.scaled_size(H, W, scale)
    if isz:
        return dict(sh=sh, sw=sw, Hp=isz[0], Wp=isz[1], padl=0, padt=0, h8=isz[0] // 8, w8=isz[1] // 8, P=(isz[0] // 8) * (isz[1] // 8))
    l, r, t, b = O.pad_amounts(sh, sw, factor)
    Hp, Wp = sh + t + b, sw + l + r
    return dict(sh=sh, sw=sw, Hp=Hp, Wp=Wp, padl=l, padt=t, h8=Hp // 8, w8=Wp // 8, P=(Hp // 8) * (Wp // 8))


def _norm64(v, norm: int):
    """v [..., 3] float64 pixel values -> (normalised, tolerance).  The kernel's separately rounded float32 operations after the pixel value:
    RAFT 2: v / 255 (rounds a magnitude of v / 255; the factor 2 is exact and doubles what came before it) and the subtraction of 1 (rounds
    the result); GMFlow 3: v / 255, the subtraction of the mean (rounds v / 255 - mean) and the division by std (rounds the result; it also
    divides the two earlier errors by std).  Each contributes 2^-24 of the magnitude it rounds; contraction into an FMA only removes one"""
    q = v / 255.0
    if norm == 0:
        t = 2.0 * q - 1.0
        return t, U24 * (2.0 * q + np.abs(t))
    t = (q - MEAN) / STD
    return t, U24 * (q / STD + np.abs(q - MEAN) / STD + np.abs(t))


def prep_truth(frames: np.ndarray, scale: float, factor: int, norm: int, isz=None):
    """-> (geo, scaled uint8 [n, sh, sw, 3] by the oracle's integer rule, truth float64 [n, Hp, Wp, 3], tolerance of the same shape).
    Direct mode: the scaled frame, replicate padded by pad_amounts, is an integer per element, so the tolerance is _norm64's 2 (RAFT) or
    3 (GMFlow) float32 roundings.  Inference-size mode: the scaled frame blended at torch's float32 align_corners coordinates (ac_coords),
    the blend itself in float64 with the float32 weights; the kernel's blend adds 4 roundings on every path - product, sum of the row,
    product with the row weight, final sum - each at most 2^-24 of the blended magnitude (pixels and weights are non-negative, so that is
    the value itself), carried through the normalisation's slope 1 / 255 (x 2 RAFT, / std GMFlow): 6 (RAFT) or 7 (GMFlow) roundings"""
    n, H, W, _ = frames.shape
    key = ("truth", H, W, scale, factor, norm, isz) if frames is _CACHE.get(("frames", H, W, bool(isz))) else None
    if key in _CACHE:
        return _CACHE[key]
    geo = prep_geometry(H, W, scale, factor, isz)
    sc = scaled_oracle(frames, scale)
    assert sc.shape[1:3] == (geo["sh"], geo["sw"])
    if isz:
        v = _blend64(sc.astype(np.float64), geo["Hp"], geo["Wp"])
        t, tol = _norm64(v, norm)
        tol = tol + 4 * U24 * v / 255.0 * (2.0 if norm == 0 else 1.0 / STD)
    else:
        l, r, tp, b = O.pad_amounts(geo["sh"], geo["sw"], factor)
        v = np.pad(sc, ((0, 0), (tp, b), (l, r), (0, 0)), mode="edge").astype(np.float64)
        t, tol = _norm64(v, norm)
    out = (geo, sc, t, tol * SLACK)
    if key:
        _CACHE[key] = out
    return out


def f16_tie_distance(t) -> np.ndarray:
    """distance of every value to the nearest fp16 rounding tie (the midpoint of two neighbouring fp16 values)"""
    t = np.asarray(t, np.float64)
    h = t.astype(np.float16)
    with np.errstate(over="ignore"):
        up, dn = np.nextafter(h, np.float16(np.inf)).astype(np.float64), np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    h = h.astype(np.float64)
    return np.minimum(np.abs(t - (h + up) / 2), np.abs(t - (h + dn) / 2))


def direct_values(norm: int):
    """the 256 (x 3 channels) values a direct-mode element can take -> (truth [256, 3], tolerance)"""
    v = np.repeat(np.arange(256, dtype=np.float64)[:, None], 3, 1)
    t, tol = _norm64(v, norm)
    return t, tol * SLACK


def s2d_rows(x: np.ndarray, bug=None) -> np.ndarray:
    """[n, Hp, Wp, 4] -> [n Hp/4 Wp/4, 64]: position ((y & 3) 4 + (x & 3)) 4 + c of block (y >> 2, x >> 2); bug 'dydx': (x & 3) 4 + (y & 3)"""
    n, Hp, Wp, _ = x.shape
    b = x.reshape(n, Hp // 4, 4, Wp // 4, 4, 4)                    # n by dy bx dx c
    b = b.transpose(0, 1, 3, 4, 2, 5) if bug == "dydx" else b.transpose(0, 1, 3, 2, 4, 5)
    return np.ascontiguousarray(b).reshape(n * (Hp // 4) * (Wp // 4), 64)


def s2d_pixels(rows: np.ndarray, n: int, Hp: int, Wp: int) -> np.ndarray:
    """the inverse of s2d_rows: [n Hp/4 Wp/4, 64] -> [n, Hp, Wp, 4]"""
    b = rows.reshape(n, Hp // 4, Wp // 4, 4, 4, 4).transpose(0, 1, 3, 2, 4, 5)
    return np.ascontiguousarray(b).reshape(n, Hp, Wp, 4)


def prep_restated(frames: np.ndarray, scale: float, factor: int, layout: int, norm: int, pa: int, isz=None, bug=None,
                  guard_rows: int = GUARD_ROWS, guard: int = GUARD):
    """raft_prep_kernel operation by operation -> (geo, raw uint8 [rows + guard_rows, 128 | 256], scaled [n, sh, sw, 3], its guard bytes):
    what Ops.flow_prep returns.  bugs: PREP_BUGS"""
    n, H, W, _ = frames.shape
    s = float(F32(scale)) if bug == "scale_f32" else scale
    geo = prep_geometry(H, W, s, factor, isz)
    sc = scaled_restated(frames, scale, bug)
    sh, sw, Hp, Wp = geo["sh"], geo["sw"], geo["Hp"], geo["Wp"]
    if isz:
        v = _blend32(sc, Hp, Wp)
    else:
        l, r, tp, b = O.pad_amounts(sh, sw, factor)
        if bug == "pad_left":
            l, r, tp, b = r, l, b, tp
            geo.update(padl=l, padt=tp)
        hi_y, hi_x = (sh, sw) if bug == "clamp_sh" else (sh - 1, sw - 1)
        ys, xs = np.clip(np.arange(Hp) - tp, 0, hi_y) % sh, np.clip(np.arange(Wp) - l, 0, hi_x) % sw     # row sh: some other row, here row 0
        v = sc[:, ys][:, :, xs].astype(F32)
    if bug == "bgr":
        v = v[..., ::-1]
    nm = 1 - norm if bug == "other_norm" else norm
    q = (v / F32(255)).astype(F32)
    t = (F32(2) * q - F32(1)).astype(F32) if nm == 0 else ((q - MEAN32).astype(F32) / STD32).astype(F32)
    t4 = np.zeros((n, Hp, Wp, 4), F32)
    t4[..., :3] = t
    hi = t4.astype(np.float16)
    res = (t4 - hi.astype(F32)).astype(F32)
    rows = n * (Hp // 4) * (Wp // 4)
    raw = np.full((rows + guard_rows, 256 if layout else 128), 0xFF, np.uint8)
    raw[:rows, :128] = s2d_rows(hi, bug).view(np.uint8)
    if layout == 1:
        raw[:rows, 128:] = s2d_rows(res.astype(np.float16), bug).view(np.uint8)
    if layout == 2:
        raw[:rows, 128:192] = s2d_rows(S.e4m3_bytes(np.ldexp(hi.astype(F32), pa)), bug)
        raw[:rows, 192:] = s2d_rows(S.e4m3_bytes(np.ldexp(res, pa + 12)), bug)
    scaled = np.full((n, sh, sw, 3), 0xFF, np.uint8) if isz else sc
    return geo, raw, scaled, np.full(guard, 0xFF, np.uint8)


def prep_verify(what: str, frames: np.ndarray, scale: float, factor: int, layout: int, norm: int, pa: int, geo: dict, raw: np.ndarray,
                scaled: np.ndarray, sguard: np.ndarray, isz=None, guard_rows: int = GUARD_ROWS) -> dict:
    """the checks of one prep launch.  The plan equals the oracle's; the scaled frame equals cv_resize_cubic_u8 byte for byte (inference
    size: left preset).  Direct mode: hi is the fp16 of the truth, bit for bit (no truth value lies within the tolerance of an fp16 tie:
    test_flow_io_ref_cpu).  Inference-size mode: hi lies between the fp16 roundings of truth -+ tolerance.  [hi | lo]: hi + lo within the
    tolerance plus lo's own fp16 half-step.  [hi | hi8 | lo8]: hi8 the e4m3 bytes of the kernel's own hi x 2^pa, lo8 within one e4m3 step
    (plus the tolerance) of the truth's residual.  Channel 3 is zero; the guard rows and guard bytes are still 0xFF"""
    n = frames.shape[0]
    want_geo, sc, t, tol = prep_truth(frames, scale, factor, norm, isz)
    assert geo == want_geo, (what, geo, want_geo)
    Hp, Wp = geo["Hp"], geo["Wp"]
    rows = n * (Hp // 4) * (Wp // 4)
    assert raw.shape == (rows + guard_rows, 256 if layout else 128), (what, raw.shape)
    assert (raw[rows:] == 0xFF).all(), what + ": guard rows written"
    assert (np.asarray(sguard) == 0xFF).all(), what + ": bytes behind the scaled frames written"
    if isz:
        assert (np.asarray(scaled) == 0xFF).all(), what + ": scaled_out written in the inference-size mode"
    else:
        same_u8(what + " scaled frame", scaled, sc)
    hi4 = s2d_pixels(np.ascontiguousarray(raw[:rows, :128]).view(np.float16), n, Hp, Wp)
    assert (hi4[..., 3].view(np.uint16) == 0).all(), what + ": channel 3 of hi is not +0"
    hi = hi4[..., :3]
    out = {}
    if isz:
        lo_ok, hi_ok = (t - tol).astype(np.float16), (t + tol).astype(np.float16)
        bad = ~((hi >= lo_ok) & (hi <= hi_ok))
        assert not bad.any(), "%s: hi %s = %r outside fp16(%r -+ %.3g); %d elements" % (
            what, tuple(np.argwhere(bad)[0]), float(hi[bad][0]), float(t[bad][0]), float(tol[bad][0]), int(bad.sum()))
        out["tie_share"] = float((lo_ok != hi_ok).mean())
    else:
        want = t.astype(np.float16)
        bad = hi.view(np.uint16) != want.view(np.uint16)
        assert not bad.any(), "%s: hi %s = %r, fp16 of the truth %r; %d elements" % (
            what, tuple(np.argwhere(bad)[0]), float(hi[bad][0]), float(want[bad][0]), int(bad.sum()))
    resid = t - hi.astype(np.float64)
    if layout == 1:
        lo4 = s2d_pixels(np.ascontiguousarray(raw[:rows, 128:]).view(np.float16), n, Hp, Wp)
        assert (lo4[..., 3].view(np.uint16) == 0).all(), what + ": channel 3 of lo is not +0"
        err = np.abs(lo4[..., :3].astype(np.float64) - resid)
        bound = tol + f16_step(np.abs(resid) + tol) / 2
        out["lo"] = float((err / bound).max())
        assert out["lo"] <= 1.0, "%s: hi + lo off by %.3g, bound %.3g" % (what, err.max(), bound[np.unravel_index(err.argmax(), err.shape)])
    if layout == 2:
        h8 = s2d_pixels(np.ascontiguousarray(raw[:rows, 128:192]), n, Hp, Wp)
        l8 = s2d_pixels(np.ascontiguousarray(raw[:rows, 192:]), n, Hp, Wp)
        same_u8(what + " hi8", h8, S.e4m3_bytes(np.ldexp(hi4.astype(F32), pa)))
        assert (l8[..., 3] == 0).all(), what + ": channel 3 of lo8 is not +0"
        got = np.ldexp(S.e4m3_decode(l8[..., :3]), -(pa + 12))
        bound = np.ldexp(S.e4m3_step(np.ldexp(np.abs(resid) + tol, pa + 12)), -(pa + 12)) + tol
        err = np.abs(got - resid)
        out["lo8"] = float((err / bound).max())
        assert out["lo8"] <= 1.0, "%s: lo8 off by %.3g" % (what, err.max())
    return out


# =====================================================================================================================
# flow_resize_back_kernel
# =====================================================================================================================
# (ih, iw) -> (sh, sw): the last is 135000 pixels - with 512 blocks of 256 lanes the grid-stride loop runs twice
BACK_CASES = [((32, 64), (34, 58)), ((64, 32), (34, 58)), ((48, 80), (48, 80)), ((16, 16), (1, 40)), ((16, 16), (40, 1)), ((96, 160), (300, 450))]
BACK_BUGS = ["ratio_swap", "max_before", "coord_fma"]


def back_data(ih: int, iw: int, amp: float = 1.0) -> np.ndarray:
    """three flows with differing maxima (x 1, x 7, x 0.05), smooth plus noise, both signs"""
    g = np.random.default_rng(77 * ih + iw)
    yy, xx = np.mgrid[0:ih, 0:iw].astype(np.float64)
    base = np.stack([3.0 * np.sin(yy / 5.0) + 0.1 * xx - 2.0, 2.0 * np.cos(xx / 4.0) - 0.07 * yy], -1)
    f = np.stack([base * s + g.standard_normal((ih, iw, 2)) * s for s in (1.0, 7.0, 0.05)])
    return (f * amp).astype(F32)


def back_truth(flow: np.ndarray, sh: int, sw: int):
    """float64 F.interpolate(bilinear, align_corners=True) at torch's float32 coordinates, u x sw / iw, v x sh / ih -> (truth, tolerance).
    The kernel: 4 roundings in the blend (as prep_truth's, here of sum w |p| - the flow has both signs), the product with the size and
    the division by the grid's: 6 float32 roundings, the last two of the result's own magnitude"""
    n, ih, iw, _ = flow.shape
    ratio = np.array([sw / iw, sh / ih])
    t = _blend64(flow.astype(np.float64), sh, sw) * ratio
    mag = _blend64(flow.astype(np.float64), sh, sw, absolute=True) * ratio
    return t, (U24 * (4 * mag + 2 * np.abs(t)) + 2.0 ** -149) * SLACK


def back_restated(flow: np.ndarray, sh: int, sw: int, bug=None, guard: int = GUARD):
    """flow_resize_back_kernel in float32 -> (out [n, sh, sw, 2], guard floats, maxd [n]).  bugs: 'ratio_swap' (u x sh / ih, v x sw / iw),
    'max_before' (the maximum of the blended flow, before the rescale), 'coord_fma' (ac_coords' fma)"""
    n, ih, iw, _ = flow.shape
    v = _blend32(flow, sh, sw, bug == "coord_fma")
    num, den = (F32([sh, sw]), F32([ih, iw])) if bug == "ratio_swap" else (F32([sw, sh]), F32([iw, ih]))
    out = ((v * num).astype(F32) / den).astype(F32)
    return out, np.full(guard * 4, 0xFF, np.uint8), maxd_of(v if bug == "max_before" else out)


def back_verify(what: str, flow: np.ndarray, sh: int, sw: int, out: np.ndarray, guard, maxd: np.ndarray) -> dict:
    """values within the derived bound; maxd bit-equal to the float32 maximum of sqrt(u u + v v) over the kernel's OWN output; guard preset"""
    t, tol = back_truth(flow, sh, sw)
    assert out.shape == t.shape, (what, out.shape)
    assert (np.asarray(guard).view(np.uint8) == 0xFF).all(), what + ": guard written"
    err = np.abs(out.astype(np.float64) - t)
    r = float((err / tol).max())
    assert np.isfinite(out).all() and r <= 1.0, "%s: err / tol %.3f at %s" % (what, r, np.unravel_index((err / tol).argmax(), err.shape))
    want = maxd_of(out)
    assert np.array_equal(np.asarray(maxd, F32).view(np.uint32), want.view(np.uint32)), (what, maxd, want)
    return dict(value=r)


# =====================================================================================================================
# flow_encode_kernel
# =====================================================================================================================
def _ulp_triple(v: float):
    v = F32(v)
    return [np.nextafter(v, F32(0)), v, np.nextafter(v, F32(1))]


def encode_vectors() -> np.ndarray:
    """adversarial (u, v) for a frame whose maximum is 4 (dx = u / 4 and dy = v / 4 are exact): the axes in both signs with +0 and -0 in
    the other component, the four diagonals, both zeros in every sign, denormals, and min / max ratios at and one float32 ulp either side
    of 1/8, 3/8, 5/8, 7/8 - where k = floor(4 t + 0.5) of atan2_rn switches - in every octant (the larger component is 2, so t is the
    smaller one's factor exactly)"""
    z, m = F32(0.0), F32(-0.0)
    v = [(4.0, z), (4.0, m), (-4.0, z), (-4.0, m), (z, 4.0), (m, 4.0), (z, -4.0), (m, -4.0)]
    v += [(a, b) for a in (2.0, -2.0) for b in (2.0, -2.0)]
    v += [(a, b) for a in (z, m) for b in (z, m)]
    d = F32(1e-40)
    v += [(d, z), (z, d), (d, d), (-d, d), (d, F32(3e-39)), (F32(2.0), d), (-d, F32(-2.0)), (F32(1.5e-45), F32(-1.5e-45))]
    for c in (0.125, 0.375, 0.625, 0.875):
        for r in _ulp_triple(c):
            for sa in (2.0, -2.0):
                for sb in (1.0, -1.0):
                    small = F32(2.0) * r * F32(sb)
                    v += [(F32(sa), small), (small, F32(sa))]
    return np.array(v, F32)


def encode_cases():
    """{name: flow [3, h, w, 2]}: 'adversarial' - encode_vectors at maxima 4 and 0.5, and a frame of signed zeros whose maximum is 0;
    '1x1'; 'random' - 520 x 520 = 270400 pixels, more than the 1024-block grid covers at once, three scales"""
    if "encode" not in _CACHE:
        v = encode_vectors()
        w = 16
        h = -(-len(v) // w)
        a = np.zeros((3, h * w, 2), F32)
        a[0, :len(v)] = v
        a[0, len(v):] = v[0]
        a[1] = a[0] * F32(0.125)
        a[2, ::2] = F32(-0.0)
        g = np.random.default_rng(5)
        rnd = np.stack([g.standard_normal((520, 520, 2)) * s for s in (1.0, 5.0, 40.0)]).astype(F32)
        rnd[1, 100:110, :, 1] = 0.0                     # stretches on the axes and the diagonals inside the noise
        rnd[2, :, 200:204, 0] = rnd[2, :, 200:204, 1]
        _CACHE["encode"] = {"adversarial": a.reshape(3, h, w, 2), "1x1": np.array([[3.0, -4.0], [-0.0, 1e-3], [0.0, 0.0]], F32).reshape(3, 1, 1, 2),
                            "random": rnd}
    return _CACHE["encode"]


def encode_truth(flow: np.ndarray):
    """-> (rgb [n, h, w, 3] of process_flow(exact_atan2=True), the per-frame float32 maximum it divides by).  A frame whose maximum is 0
    divides 0 by 0: the kernel writes 0 for a NaN colour, which is what numpy's cast gives on x86 (asserted in test_flow_io_ref_cpu)"""
    with np.errstate(all="ignore"):
        res = [O.process_flow(f, exact_atan2=True) for f in flow]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], F32)


def encode_verify(what: str, flow: np.ndarray, rgb: np.ndarray, guard, max_out: np.ndarray, maxd: np.ndarray) -> None:
    want, mx = encode_truth(flow)
    assert np.array_equal(mx.view(np.uint32), np.asarray(maxd, F32).view(np.uint32)), what
    assert (np.asarray(guard) == 0xFF).all(), what + ": guard written"
    assert np.array_equal(np.asarray(max_out, F32).view(np.uint32), mx.view(np.uint32)), (what, max_out, mx)
    same_u8(what, rgb, want)


# =====================================================================================================================
# fwdbwd_mask_kernel
# =====================================================================================================================
MASK_BUGS = ["trunc_div", "abs_and", "half_up"]


def _neg_pairs(g, n: int, h: int, w: int) -> np.ndarray:
    """n pairs on an h x w frame with a one-pixel axis (or both): along every one-pixel axis the forward flow is -frac, frac in
    1/32 .. 47/32 (plus 1e-3 noise), so the target lies left of / above the frame by a fraction, q = round(32 (p + f)) is a negative
    integer and the ONE tap inside the frame is pixel 0 with weight (q & 31) / 32 (none where q < -32); along the other axis it is 0.
    The backward flow at the tapped pixel is -f / weight, on every second pixel 15 % off - so whether the round trip closes is decided
    by q >> 5 and q & 31 of negatives, and about half of the forward bits are set"""
    frac = [g.integers(1, 48, (n, h, w)) / 32.0 + g.standard_normal((n, h, w)) * 1e-3 if size == 1 else None for size in (w, h)]
    fwd = np.zeros((n, h, w, 2))
    wgt = np.ones((n, h, w))
    for c in range(2):
        if frac[c] is not None:
            fwd[..., c] = -frac[c]
            wgt *= np.clip(1.0 - frac[c], 1.0 / 32, 1.0)
    bwd = -fwd / wgt[..., None] * (1.0 + 0.15 * g.integers(0, 2, (n, h, w, 1)))
    return np.stack([fwd, bwd], 1).astype(F32)


def mask_cases():
    """{name: flows [n, 2, h, w, 2]}: 'ties' - p + f(p) exactly on odd multiples of 1/64, the half-even ties of the 1/32-pixel
    quantisation, inside, left of and above the frame; 'neg_x', 'neg_y', 'neg_xy' - targets left of, above, and left of and above the
    frame by fractions (>> 5 and & 31 of negative integers decide: _neg_pairs); 'h1' and 'w1' - a one-pixel axis with ordinary flows"""
    if "mask" not in _CACHE:
        g = np.random.default_rng(23)

        def pair(h, w, fwd):
            yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
            tx, ty = np.clip(xx + fwd[..., 0], 0, w - 1).astype(int), np.clip(yy + fwd[..., 1], 0, h - 1).astype(int)
            bwd = -fwd[ty, tx] + g.standard_normal((h, w, 2)) * 0.4 * g.integers(0, 2, (h, w, 1))       # half of the round trips close
            return np.stack([fwd, bwd]).astype(F32)

        h, w = 23, 37
        odd = (2 * g.integers(-40, 41, (2, h, w, 2)) + 1) / 64.0                           # within +-1.3 pixels
        far = (2 * g.integers(-1600, 1601, (h, w, 2)) + 1) / 64.0                          # within +-50 pixels: off the frame on every side
        _CACHE["mask"] = {"ties": np.stack([pair(h, w, odd[0]), pair(h, w, odd[1]), pair(h, w, far)]),
                          "neg_x": _neg_pairs(g, 4, 29, 1), "neg_y": _neg_pairs(g, 4, 1, 37), "neg_xy": _neg_pairs(g, 96, 1, 1),
                          "h1": np.stack([pair(1, 37, g.standard_normal((1, 37, 2)) * 3.0), pair(1, 37, (2 * g.integers(-40, 41, (1, 37, 2)) + 1) / 64.0)]),
                          "w1": np.stack([pair(29, 1, g.standard_normal((29, 1, 2)) * 3.0), pair(29, 1, (2 * g.integers(-40, 41, (29, 1, 2)) + 1) / 64.0)])}
    return _CACHE["mask"]


def _remap_restated(img, map_xy, bug=None):
    """oracle.raft_oracle.remap_linear_const with room for the planted faults: 'trunc_div' (q / 32 truncated towards zero for q >> 5),
    'abs_and' (|q| & 31 for q & 31), 'half_up' (floor(x + 0.5) for the half-even round)"""
    h, w = img.shape[:2]
    x32 = map_xy.astype(F32) * F32(32.0)
    q = (np.floor(x32.astype(np.float64) + 0.5) if bug == "half_up" else np.rint(x32)).astype(np.int64)
    ix, iy = (np.trunc(q / 32.0).astype(np.int64)[..., c] for c in range(2)) if bug == "trunc_div" else (q[..., 0] >> 5, q[..., 1] >> 5)
    k = np.abs(q) & 31 if bug == "abs_and" else q & 31
    fx, fy = k[..., 0].astype(F32) * F32(1.0 / 32), k[..., 1].astype(F32) * F32(1.0 / 32)
    tx, ty = (F32(1.0) - fx, fx), (F32(1.0) - fy, fy)
    out = None
    for k1 in range(2):
        for k2 in range(2):
            yy, xx = iy + k1, ix + k2
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            v = np.where(ok[..., None], img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], F32(0.0))
            term = (v * (ty[k1] * tx[k2])[..., None]).astype(F32)
            out = term if out is None else (out + term).astype(F32)
    return out


def mask_restated(flows: np.ndarray, bug=None) -> np.ndarray:
    """fwdbwd_mask_kernel operation by operation (compute_fwdbwd_mask on _remap_restated) -> bool [n, 2, h, w].  bugs: MASK_BUGS"""
    def norm(a):
        return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]).astype(F32)).astype(F32)

    def one(f, other):
        h, w = f.shape[:2]
        grid = f.astype(F32).copy()
        grid[..., 0] += np.arange(w)
        grid[..., 1] += np.arange(h)[:, None]
        warped = _remap_restated(other.astype(F32), grid, bug)
        return norm(f + warped) < F32(0.05) * (norm(f) + norm(warped)) + F32(0.5)

    return np.stack([np.stack([one(f[0], f[1]), one(f[1], f[0])]) for f in flows])


def mask_truth(flows: np.ndarray) -> np.ndarray:
    return np.stack([np.stack(O.compute_fwdbwd_mask(f[0], f[1])) for f in flows])


def mask_quantised(flows: np.ndarray) -> np.ndarray:
    """(p + f(p)) x 32 before the rounding, float64 [n, 2, h, w, 2] - what the case descriptions are asserted on"""
    n, _, h, w, _ = flows.shape
    yy, xx = np.mgrid[0:h, 0:w]
    return (flows.astype(F32) + np.stack([xx, yy], -1).astype(F32)).astype(F32).astype(np.float64) * 32.0
