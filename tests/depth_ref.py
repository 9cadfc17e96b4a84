"""float64 truth and restatements of the depth bands' own kernels (CPU only; a helper module of the tests, not a conftest).

Every op has four pieces, shared by tests/test_depth_ref_cpu.py and tests/test_gpu_depth_ops.py:
  *_data      seeded inputs, exactly representable in the layout under test, and the case list;
  truth       torch / numpy on float64 (oracle/zoe_oracle.py where it already states the reference);
  *_restated  what the kernel computes, returned in the RAW form the pb_op_depth_* / pb_op_zoe_* entry points return (0xFF wherever the
              kernel owns nothing): source indices and blend weights in float32 exactly as bilerp_src / ac_src / torch compute them (they
              decide which taps are read), values carried in float64, rounding where the kernel stores.  `bug=` plants one fault;
  *_verify    the checks themselves: raw buffer in, AssertionError naming op, case and element out; returns the measured worst
              error / tolerance figures.  The GPU tests hand it the kernel's buffer, the CPU tests the restatement's - with and without
              a planted fault - so the tolerances are shown to pass the arithmetic they are derived for and to see each fault.

Tolerances that rest on an ASSUMED bound for a device math function (no document in the tree states ROCm's): rsqrtf, expf, logf, log1pf
are taken to be within 2 ulp of float32 (ULP2 = 2^-22 relative).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from gm_ref import check, preset, same_bytes, split16                       # noqa: F401
from mask_ref import bilinear_coord_tolerance, decode, lerp_taps, rep, rows16, store_tol       # noqa: F401
from oracle import zoe_oracle as Z
from raft_ref import U24, rng
from split_ref import BUDGET, F16, MX3, SPLIT16, e4m3_bytes, e4m3_decode, e4m3_q

F32 = np.float32
ULP2 = 2.0 ** -22           # 2 ulp of float32, relative: the ASSUMED accuracy of rsqrtf / expf / logf / log1pf on the device
GUARD = 8


def same_u8(what, got, want):
    got, want = np.ascontiguousarray(got, np.uint8), np.ascontiguousarray(want, np.uint8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: byte %s is 0x%02x, expected 0x%02x; %d bytes differ" % (what, i, got[i], want[i], int(bad.sum())))


def f16r(x) -> np.ndarray:
    """float32 -> float16 -> float32 (one fp16 rounding)"""
    return np.asarray(x, F32).astype(np.float16).astype(F32)


def ac_taps(dst: int, src: int, bug=None):
    """elementwise.hip bilerp_src(align = 1) / zoe_kernels.hip ac_src, every operation in float32: scale = (src - 1) / (dst - 1) (0 for
    dst = 1), s = scale d, i0 = min(int(s), src - 1), i1 = i0 + [i0 < src - 1], l1 = s - i0.  bug 'align': align_corners=False taps"""
    if bug == "align":
        return lerp_taps(dst, src)
    scale = F32(src - 1) / F32(dst - 1) if dst > 1 else F32(0)
    s = (scale * np.arange(dst, dtype=F32)).astype(F32)
    i0 = np.minimum(s.astype(np.int64), src - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    return i0, i0 + (i0 < src - 1), l1.astype(np.float64)


def blend(x, ytaps, xtaps):
    """x [n, H, W, C] float64 -> [n, OH, OW, C]: hy (hx v00 + lx v01) + ly (hx v10 + lx v11) with the float32 weights of the taps"""
    x = np.asarray(x, np.float64)
    (y0, y1, ly), (x0, x1, lx) = ytaps, xtaps
    hy = (F32(1) - ly.astype(F32)).astype(np.float64)[None, :, None, None]
    hx = (F32(1) - lx.astype(F32)).astype(np.float64)[None, None, :, None]
    LY, LX = ly[None, :, None, None], lx[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    return hy * (hx * r0[:, :, x0] + LX * r0[:, :, x1]) + LY * (hx * r1[:, :, x0] + LX * r1[:, :, x1])


def resize_truth(x, OH, OW, align):
    """F.interpolate(bilinear) of x [n, H, W, C] on float64"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64)).permute(0, 3, 1, 2)
    return F.interpolate(t, size=(OH, OW), mode="bilinear", align_corners=align).permute(0, 2, 3, 1).numpy()


def raw_rows(rows: int, nbytes: int) -> np.ndarray:
    return np.full((rows, nbytes), 0xFF, np.uint8)


# =====================================================================================================================
# LayerNorm (elementwise.hip layernorm_kernel) in the three modes DepthEngine::vit uses
# =====================================================================================================================
LN_DIMS = [384, 1024]       # 384: half of the wave idle in the second quarter of the row; 1024: all four quarters
LN_B, LN_NTP, LN_NTOK = 2, 32, 19           # 38 live rows: a partial last block of 4; pad rows 19 .. 31 stay preset
LN_EPS = 1e-6
LN_O8_SCALE = 2.0
LN_SPECIAL = {"offset": (0, 3), "const": (1, 5)}
LN_CONST = 3.25             # 13 / 4: every partial sum of up to 1024 copies is a float32, so mean = x exactly and the output is beta


def ln_mode(mode: str, D: int) -> dict:
    """a: the block LayerNorms (engine.hip: token rows [fp16 (D) | fp8 (D bytes)], here 64 halfs wider still); the row of D + 64 halfs the
    issue names cannot hold D bytes of fp8 behind D halfs for D > 128, so the row is the engine's D + D / 2 plus those 64 halfs.
    b / c: the four DPT taps, class token dropped, [hi | lo] and [hi | hi8 | lo8]"""
    return {"a": dict(drop_cls=0, ldy=D + D // 2 + 64, lo_off=0, o8_off=2 * D, lo8=0, layout=F16),
            "b": dict(drop_cls=1, ldy=2 * D, lo_off=D, o8_off=0, lo8=0, layout=SPLIT16),
            "c": dict(drop_cls=1, ldy=3 * D, lo_off=D, o8_off=0, lo8=1, layout=MX3)}[mode]


def ln_data(D: int):
    g = rng(100 + D)
    x = g.standard_normal((LN_B, LN_NTP, D)).astype(F32)
    b, t = LN_SPECIAL["offset"]
    x[b, t] = (50.0 + 0.01 * g.standard_normal(D)).astype(F32)          # a one-pass variance E[x^2] - mean^2 loses every digit here
    b, t = LN_SPECIAL["const"]
    x[b, t] = LN_CONST
    x[:, LN_NTOK:] = np.nan                                              # pad tokens: never read
    gamma = ((0.5 + g.random(D)) * np.where(g.random(D) < 0.5, -1, 1)).astype(F32)
    beta = (0.3 * g.standard_normal(D)).astype(F32)
    return x, gamma, beta


def ln_truth(x, gamma, beta):
    t = torch.from_numpy(np.asarray(x[:, :LN_NTOK], np.float64))
    return F.layer_norm(t, (x.shape[2],), torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), LN_EPS).numpy()


def ln_f32_term(x, gamma, beta, ref):
    """float32 arithmetic of the two-pass kernel against float64, element-wise.  With u = 2^-24: the mean is a sum of D terms and a
    division, |dm| <= (D + 1) u mean|x| whatever the order; d = fl(x - m) carries dm + u |d|; the centred sum of squares has a relative
    error of (D + 3) u plus dm^2 / (var + eps) (the first-order term of the mean's error cancels: sum d = 0); rsqrtf adds ULP2 (assumed)
    and its argument's error halves; three more roundings make (d r) g + b"""
    x = np.asarray(x[:, :LN_NTOK], np.float64)
    D = x.shape[2]
    m = x.mean(2, keepdims=True)
    d = np.abs(x - m)
    var = ((x - m) ** 2).mean(2, keepdims=True)
    r = 1.0 / np.sqrt(var + LN_EPS)
    dm = (D + 1) * U24 * np.abs(x).mean(2, keepdims=True)
    rr = 0.5 * ((D + 3) * U24 + dm ** 2 / (var + LN_EPS)) + ULP2 + U24
    ag = np.abs(gamma.astype(np.float64))
    return ag * r * (dm + U24 * d) + ag * d * r * (rr + 3 * U24) + U24 * (np.abs(ref) + np.abs(beta.astype(np.float64)))


def ln_restated(x, gamma, beta, mode: str, pa: int = 0, guard: int = GUARD, bug=None) -> np.ndarray:
    """the raw buffer pb_op_depth_layernorm returns.  bugs: 'one_pass' (var = E[x^2] - mean^2 in float32), 'cls_off' (the compacted row
    index forgets the - 1), 'swap' (lo and hi parts exchanged), 'o8_shift' (the fp8 copy one dword late)"""
    B, ntp, D = x.shape
    m = ln_mode(mode, D)
    xs = x[:, :LN_NTOK]
    if bug == "one_pass":
        x32 = xs.astype(F32)
        mean = (x32.sum(2, keepdims=True, dtype=F32) / F32(D)).astype(F32)
        var = ((x32 * x32).sum(2, keepdims=True, dtype=F32) / F32(D) - mean * mean).astype(F32)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = ((x32 - mean) * (F32(1) / np.sqrt(var + F32(LN_EPS))) * gamma + beta).astype(F32)
    else:
        x64 = xs.astype(np.float64)
        mean = x64.mean(2, keepdims=True)
        var = ((x64 - mean) ** 2).mean(2, keepdims=True)
        t = ((x64 - mean) / np.sqrt(var + LN_EPS) * gamma.astype(np.float64) + beta.astype(np.float64)).astype(F32)
    hi = t.astype(np.float16)
    res = (t - hi.astype(F32)).astype(F32)
    rows = B * (LN_NTOK - 1) if m["drop_cls"] else B * ntp
    raw = raw_rows(rows + guard, 2 * m["ldy"])
    h = raw.view(np.float16)
    for b in range(B):
        for tk in range(1 if m["drop_cls"] else 0, LN_NTOK):
            r = b * (LN_NTOK - 1) + tk - (0 if bug == "cls_off" else 1) if m["drop_cls"] else b * ntp + tk
            a, c = (res[b, tk].astype(np.float16), hi[b, tk]) if bug == "swap" else (hi[b, tk], res[b, tk].astype(np.float16))
            h[r, :D] = a
            if m["lo8"]:
                raw[r, 2 * D:3 * D] = e4m3_bytes(np.ldexp(hi[b, tk].astype(F32), pa))
                raw[r, 3 * D:4 * D] = e4m3_bytes(np.ldexp(res[b, tk], pa + 12))
            elif m["lo_off"]:
                h[r, D:2 * D] = c
            if m["o8_off"]:
                o = m["o8_off"] + (4 if bug == "o8_shift" else 0)
                raw[r, o:o + D] = e4m3_bytes(hi[b, tk].astype(F32) * F32(LN_O8_SCALE))
    return raw


def ln_verify(what, raw, x, gamma, beta, mode: str, pa: int = 0, guard: int = GUARD) -> dict:
    B, ntp, D = x.shape
    m = ln_mode(mode, D)
    t0 = 1 if m["drop_cls"] else 0
    rows = B * (LN_NTOK - 1) if m["drop_cls"] else B * ntp
    assert raw.shape == (rows + guard, 2 * m["ldy"]) and raw.dtype == np.uint8, (what, raw.shape)
    preset(what + ": guard rows", raw[rows:])
    body = raw[:rows]
    if m["drop_cls"]:       # row b (ntok - 1) + t - 1 holds token t; no row is left for the class token
        live = body.reshape(B, LN_NTOK - 1, -1)
    else:
        grid = body.reshape(B, ntp, -1)
        preset(what + ": pad token rows", grid[:, LN_NTOK:])
        live = grid[:, :LN_NTOK]
    own = D * 2 * {F16: 1, SPLIT16: 2, MX3: 2}[m["layout"]]
    tail = np.ones(live.shape[2], bool)
    tail[:own] = False
    if m["o8_off"]:
        tail[m["o8_off"]:m["o8_off"] + D] = False
    preset(what + ": row tails", live[:, :, tail])
    h = np.ascontiguousarray(live).view(np.float16)
    hi = h[:, :, :D].astype(np.float64)
    if m["layout"] == SPLIT16:
        value = hi + h[:, :, D:2 * D].astype(np.float64)
    elif m["layout"] == MX3:
        value = hi + np.ldexp(e4m3_decode(live[:, :, 3 * D:4 * D]), -(pa + 12))
        same_u8(what + ": hi8 = e4m3(stored hi 2^pa)", live[:, :, 2 * D:3 * D], e4m3_bytes(np.ldexp(hi.astype(F32), pa)))
    else:
        value = hi
    ref = ln_truth(x, gamma, beta)[:, t0:]
    floor = {F16: 2.0 ** -25, SPLIT16: 2.0 ** -25, MX3: 2.0 ** -22}[m["layout"]]      # half the subnormal step of the part that rounds last
    tol = BUDGET[m["layout"]] * np.abs(ref) + floor + ln_f32_term(x, gamma, beta, ln_truth(x, gamma, beta))[:, t0:]
    out = {"value": check(what + ": hi (+ lo) vs float64 layer_norm", value, ref, tol)}
    cb, ct = LN_SPECIAL["const"]    # variance 0: (x - mean) is exactly 0, the output is beta to one rounding
    bh, bl = split16(beta)
    same_bytes(what + ": constant row = f16(beta)", h[cb, ct - t0, :D], bh)
    if m["layout"] == SPLIT16:
        same_bytes(what + ": constant row lo = f16(beta - hi)", h[cb, ct - t0, D:2 * D], bl)
    if m["o8_off"]:
        same_u8(what + ": fp8 copy = e4m3(stored hi x scale) at byte o8_off", live[:, :, m["o8_off"]:m["o8_off"] + D],
                e4m3_bytes(hi.astype(F32) * F32(LN_O8_SCALE)))
    return out


# =====================================================================================================================
# attention (attention.hip attnq_kernel, head dim 64): the 8-wave and the 4-wave geometry
# =====================================================================================================================
ATTN_CASES = [              # (name, B, heads, N)
    ("n1", 1, 1, 1),                # ntp = 16: 15 masked keys
    ("n17", 1, 1, 17),
    ("n65", 1, 2, 65),              # a second key tile holding one live key
    ("xcd", 1, 9, 40),              # nine (b, head) pairs: the second group of 8 has seven dead workgroups
    ("n257", 1, 1, 257),            # a second 8-wave query block holding one live row
    ("b2h3", 2, 3, 200),
    ("spike", 1, 1, 300),           # one key dominates late in the sequence: the online-softmax rescale
]
ATTN_VARIANTS = {1: 8, 2: 4}        # launch_attention's variant -> waves per workgroup
ATTN_O8_SCALE = 2.0
QSCALE = F32(0.125) * F32(1.4426950408889634)       # common.h PB_QSCALE: 64^-0.5 log2(e), the kernel exponentiates in base 2


def attn_geometry(heads: int, with_o8: bool):
    """(ldo, o8_off).  Without the copy: heads 64 + 64 halfs.  With it the row is the engine's [fp16 (D) | fp8 (D bytes)] plus the same 64 halfs
    (D bytes of fp8 do not fit into 64 halfs for more than two heads)"""
    D = heads * 64
    return (D + D // 2 + 64, 2 * D) if with_o8 else (D + 64, 0)


def attn_data(case):
    name, B, heads, N = case
    g = rng(200 + N + heads)
    s = 1.0 if name == "spike" else 1.5
    q, k, v = [(g.standard_normal((B, heads, N, 64)) * a).astype(np.float16).astype(F32) for a in (s, s, 1.0)]
    if name == "spike":
        k[0, 0, 270] = f16r(q[0, 0, 17] * 6.0)
    return q, k, v


def attn_operands(q, k, v):
    """the fp16 operands the kernel multiplies, as float32: q pre-scaled by PB_QSCALE as the qkv epilogue (and the entry point) does"""
    return f16r(q.astype(F32) * QSCALE), f16r(k), f16r(v)


def attn_truth(q, k, v):
    """float64 softmax(q k^T / 8) v on the pre-rounded operands -> (o, sum_j p_j |v_j|)"""
    qs, ks, vs = [a.astype(np.float64) for a in attn_operands(q, k, v)]
    s = qs @ ks.transpose(0, 1, 3, 2)
    p = np.exp2(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p @ vs, p @ np.abs(vs)


def attn_tolerance(o, pav):
    """P is rounded to fp16 before the second matmul (2^-11 of every p_j, in the numerator and - the row sum adds the rounded values - in the
    denominator), O is rounded on store"""
    return 2.0 ** -10 * pav + 2.0 ** -11 * np.abs(o) + 2.0 ** -25


def attn_dead_workgroups(B: int, heads: int, N: int, waves: int) -> int:
    """launch_attention's own arithmetic: grid 8 nq ceil(B heads / 8); workgroup i serves pair (i >> 3) / nq * 8 + (i & 7) and leaves when
    that is >= B heads"""
    nq = -(-N // (32 * waves))
    grid = 8 * nq * -(-(B * heads) // 8)
    return sum(1 for i in range(grid) if ((i >> 3) // nq) * 8 + (i & 7) >= B * heads)


def attn_restated(q, k, v, with_o8: bool, guard: int = GUARD, bug=None) -> np.ndarray:
    """float32 scores, fp16 probabilities relative to the fp16-rounded row maximum, float32 sums, fp16 store.  bugs: 'pad_key' (the keys
    N .. ntp - 1 - zero rows of K and Vt - are not masked: each adds 2^(0 - m) to the row sum), 'o8_shift' (the fp8 copy one dword late)"""
    B, heads, N, _ = q.shape
    ntp = -(-N // 16) * 16
    ldo, o8_off = attn_geometry(heads, with_o8)
    qs, ks, vs = attn_operands(q, k, v)
    s = np.matmul(qs, ks.transpose(0, 1, 3, 2)).astype(F32)
    m = f16r(s.max(-1, keepdims=True))
    p = f16r(np.exp2((s - m).astype(F32)))
    l = p.sum(-1, keepdims=True, dtype=F32)
    if bug == "pad_key":
        l = l + F32(ntp - N) * f16r(np.exp2(-m))
    o = (np.matmul(p, vs).astype(F32) / l).astype(np.float16)                # [B, heads, N, 64]
    raw = raw_rows(B * ntp + guard, 2 * ldo)
    h = raw.view(np.float16)
    rows = o.transpose(0, 2, 1, 3).reshape(B, N, heads * 64)
    for b in range(B):
        h[b * ntp:b * ntp + N, :heads * 64] = rows[b]
        if with_o8:
            at = o8_off + (4 if bug == "o8_shift" else 0)
            raw[b * ntp:b * ntp + N, at:at + heads * 64] = e4m3_bytes(rows[b].astype(F32) * F32(ATTN_O8_SCALE))
    return raw


def attn_verify(what, raw, q, k, v, with_o8: bool, guard: int = GUARD) -> dict:
    B, heads, N, _ = q.shape
    ntp, D = -(-N // 16) * 16, heads * 64
    ldo, o8_off = attn_geometry(heads, with_o8)
    assert raw.shape == (B * ntp + guard, 2 * ldo) and raw.dtype == np.uint8, (what, raw.shape)
    preset(what + ": guard rows", raw[B * ntp:])
    grid = raw[:B * ntp].reshape(B, ntp, 2 * ldo)
    preset(what + ": pad token rows", grid[:, N:])
    live = np.ascontiguousarray(grid[:, :N])
    tail = np.ones(2 * ldo, bool)
    tail[:2 * D] = False
    if with_o8:
        tail[o8_off:o8_off + D] = False
    preset(what + ": row tails", live[:, :, tail])
    stored = live.view(np.float16)[:, :, :D]
    got = stored.astype(np.float64).reshape(B, N, heads, 64).transpose(0, 2, 1, 3)
    o, pav = attn_truth(q, k, v)
    out = {"value": check(what + ": vs float64 softmax(q k^T / 8) v", got, o, attn_tolerance(o, pav))}
    if with_o8:
        same_u8(what + ": fp8 copy = e4m3(stored fp16 x scale) at byte o8_off + head 64 + d", live[:, :, o8_off:o8_off + D],
                e4m3_bytes(stored.astype(F32) * F32(ATTN_O8_SCALE)))
    return out


# =====================================================================================================================
# cls_rows
# =====================================================================================================================
CLS_B, CLS_NTP, CLS_D = 3, 16, 384


def cls_data():
    g = rng(300)
    return g.standard_normal(CLS_D).astype(F32), g.standard_normal((5, CLS_D)).astype(F32)       # cls, pos (row 0 is the class token's)


def cls_restated(cls, pos, guard: int = 2, bug=None) -> np.ndarray:
    """bug 'row1': the sum lands in row 1 of every image"""
    out = np.frombuffer(raw_rows(CLS_B * CLS_NTP + guard, 4 * CLS_D).tobytes(), F32).reshape(-1, CLS_D).copy()
    out[np.arange(CLS_B) * CLS_NTP + (1 if bug == "row1" else 0)] = cls + pos[0]
    return out


def cls_verify(what, got, cls, pos, guard: int = 2):
    assert got.shape == (CLS_B * CLS_NTP + guard, CLS_D) and got.dtype == F32, (what, got.shape)
    first = np.arange(CLS_B) * CLS_NTP
    same_bytes(what + ": row 0 of every image = cls + pos[0]", got[first], np.broadcast_to(cls + pos[0], (CLS_B, CLS_D)))
    rest = np.ones(len(got), bool)
    rest[first] = False
    preset(what + ": every other float", got[rest])


# =====================================================================================================================
# DPT tail (elementwise.hip dpt_tail_kernel)
# =====================================================================================================================
DPT_CASES = [((3, 4), (7, 18)),         # OW, OH no multiples of the 16 x 4 block: blocks straddle the border
             ((5, 6), (5, 6)),          # scale 1
             ((1, 1), (4, 5)),          # scale 0
             ((2, 3), (1, 1)),          # every tap but the centre outside
             ((6, 5), (14, 33))]
DPT_LAYOUTS = {0: F16, 1: SPLIT16, 2: MX3}
DPT_B = 2


def dpt_ldz(layout: int) -> int:
    """pixel stride in halfs: the engine's 320-wide parts ([hi], [hi | lo], [hi | hi8 | lo8]: 320 / 640 / 640 halfs) and 64 halfs more"""
    return (320 if layout == 0 else 640) + 64


def z_decode(z, layout: int, pa: int) -> np.ndarray:
    """what SplitOpEngine::build_map stores for a float32 value, decoded to float64"""
    z = np.asarray(z, F32)
    hi = f16r(z)
    if layout == 0:
        return hi.astype(np.float64)
    if layout == 1:
        return hi.astype(np.float64) + f16r(z - hi).astype(np.float64)
    return hi.astype(np.float64) + e4m3_q(z - hi, pa + 12)


def dpt_data(case, layout: int, pa: int = 0):
    (H, W), (OH, OW) = case
    g = rng(400 + 10 * H + OW + layout)
    z = z_decode(g.standard_normal((DPT_B, H, W, 288)), layout, pa).astype(F32)      # representable: decoding it again changes nothing
    bias = (0.8 * g.standard_normal(32)).astype(F32)         # mixed sign against a tap sum of ~N(0, 3): the first ReLU cuts and passes
    w2 = (g.standard_normal(32) / 4).astype(F32)
    b2 = F32(-0.3)
    return z, bias, w2, float(b2)


def _tap_sum(U, mode="constant"):
    """U [B, OH, OW, 288] -> [B, OH, OW, 32]: sum over the nine taps of channel block t = ky 3 + kx at pixel (Y + ky - 1, X + kx - 1)"""
    B, OH, OW, _ = U.shape
    P = np.pad(U, ((0, 0), (1, 1), (1, 1), (0, 0)), mode=mode)
    acc = np.zeros((B, OH, OW, 32))
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            acc += P[:, ky:ky + OH, kx:kx + OW, t * 32:t * 32 + 32]
    return acc


def _dpt_head(acc, bias, w2, b2):
    pre = acc + bias.astype(np.float64)
    return np.maximum((np.maximum(pre, 0.0) * w2.astype(np.float64)).sum(-1) + b2, 0.0), pre


def dpt_truth(z, bias, w2, b2, OH, OW, layout: int, pa: int = 0):
    """the reference order in float64: decode z, F.interpolate(align_corners=True) of the 288 channels, nine shifted taps with zero padding,
    + bias, ReLU, . w2 + b2, ReLU -> (out [B, OH, OW], the first ReLU's argument, the second's)"""
    zd = z_decode(z, layout, pa)
    out, pre = _dpt_head(_tap_sum(resize_truth(zd, OH, OW, True)), bias, w2, b2)
    return out, pre, (np.maximum(pre, 0.0) * w2.astype(np.float64)).sum(-1) + b2


def dpt_restated(z, bias, w2, b2, OH, OW, layout: int, pa: int = 0, guard: int = 64, bug=None) -> np.ndarray:
    """bugs: 'border' (a tap outside the map reads the nearest row / column instead of 0), 'align' (align_corners=False source cells)"""
    zd = z_decode(z, layout, pa)
    B, H, W, _ = zd.shape
    U = blend(zd, ac_taps(OH, H, bug), ac_taps(OW, W, bug))
    out, _ = _dpt_head(_tap_sum(U, "edge" if bug == "border" else "constant"), bias, w2, b2)
    raw = np.frombuffer(raw_rows(1, 4 * (B * OH * OW + guard)).tobytes(), F32).copy()
    raw[:B * OH * OW] = out.astype(F32).ravel()
    return raw


def dpt_tolerance(z, bias, w2, b2, OH, OW, layout: int, pa: int = 0):
    """absolute, per pixel (|relu(a) - relu(b)| <= |a - b|, so the kinks need no exclusion).  With u = 2^-24 and A_c the tap sum of the blend
    of |z|: every one of the 36 products w z is added in float32 (36 u A_c) after two roundings of the weight product (2 u A_c), the bias add
    rounds once, the 1 x 1 sums 32 products and b2 ((32 + 3) u of the magnitudes); plus the coordinate round trip of the resize
    (mask_ref.bilinear_coord_tolerance) of the nine channel blocks a pixel reads"""
    zd = z_decode(z, layout, pa)
    B, H, W, _ = zd.shape
    A = _tap_sum(blend(np.abs(zd), ac_taps(OH, H), ac_taps(OW, W)))
    _, pre, _ = dpt_truth(z, bias, w2, b2, OH, OW, layout, pa)
    aw = np.abs(w2.astype(np.float64))
    ct = bilinear_coord_tolerance(zd, OH, OW).reshape(B, 9, 32).sum(1)[:, None, None, :]
    t = (aw * (38 * U24 * A + 2 * U24 * (np.abs(pre) + np.abs(bias)) + ct)).sum(-1)
    return t + 35 * U24 * ((aw * np.maximum(pre, 0.0)).sum(-1) + abs(b2))


def dpt_verify(what, raw, z, bias, w2, b2, OH, OW, layout: int, pa: int = 0, guard: int = 64) -> dict:
    B = z.shape[0]
    n = B * OH * OW
    assert raw.shape == (n + guard,) and raw.dtype == F32, (what, raw.shape)
    preset(what + ": guard", raw[n:])
    got = raw[:n].reshape(B, OH, OW)
    ref, _, _ = dpt_truth(z, bias, w2, b2, OH, OW, layout, pa)
    tol = dpt_tolerance(z, bias, w2, b2, OH, OW, layout, pa)
    border = np.zeros((B, OH, OW), bool)
    border[:, [0, -1]] = True
    border[:, :, [0, -1]] = True
    out = {"border": check(what + ": BORDER pixels (taps switched off)", got[border], ref[border], tol[border])}
    if (~border).any():
        out["interior"] = check(what + ": interior pixels", got[~border], ref[~border], tol[~border])
    return out


# =====================================================================================================================
# depth_resize_minmax
# =====================================================================================================================
RSZ_CASES = [((5, 7), (13, 9)),             # mixed up / down
             ((14, 14), (3, 3)),
             ((1, 1), (4, 4)),
             ((12, 16), (300, 450))]        # 135 000 pixels > 512 x 256 threads: the grid-stride loop runs
RSZ_B = 3


def rsz_data(case):
    """frame 0 all negative (the ordered-uint encoding's other branch), 1 all positive, 2 mixed with patches of +0 and -0"""
    (nh, nw), _ = case
    g = rng(500 + nh + nw)
    x = g.standard_normal((RSZ_B, nh, nw)).astype(F32)
    x[0] = -np.abs(x[0]) - F32(0.5)
    x[1] = np.abs(x[1]) + F32(0.5)
    if nh > 2:
        x[2, :nh // 3] = 0.0
        x[2, -(nh // 3):, :nw // 2] = -0.0
    return x


def ordered(v) -> np.ndarray:
    """elementwise.hip f2ord: float32 bits -> unsigned, monotonic in the value (-0 below +0)"""
    u = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unordered(o) -> np.ndarray:
    o = np.asarray(o, np.uint32)
    return np.where(o & 0x80000000, o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(F32)


def frame_minmax(out, bug=None) -> np.ndarray:
    """out [B, H, W] float32 -> [B, 2] = (min, max) in f2ord's total order.  bug 'neg_swap': the raw bits of negative floats are compared
    as unsigned, which reverses them - min and max of an all-negative frame change places"""
    o = ordered(out).reshape(out.shape[0], -1)
    mm = np.stack([unordered(o.min(1)), unordered(o.max(1))], 1)
    if bug == "neg_swap":
        neg = (out.reshape(out.shape[0], -1) < 0).all(1)
        mm[neg] = mm[neg][:, ::-1]
    return mm


def rsz_restated(x, H, W, guard: int = 64, bug=None):
    """-> (raw float32 [B H W + guard], mnmx [B, 2]).  bugs: 'align' (align_corners=True source cells), 'neg_swap'"""
    B, nh, nw = x.shape
    taps = (lambda d, s: ac_taps(d, s)) if bug == "align" else (lambda d, s: lerp_taps(d, s))
    out = blend(x[..., None], taps(H, nh), taps(W, nw))[..., 0].astype(F32)
    raw = np.frombuffer(raw_rows(1, 4 * (B * H * W + guard)).tobytes(), F32).copy()
    raw[:B * H * W] = out.ravel()
    return raw, frame_minmax(out, bug)


def rsz_verify(what, raw, mnmx, x, H, W, guard: int = 64) -> dict:
    B, nh, nw = x.shape
    n = B * H * W
    assert raw.shape == (n + guard,) and raw.dtype == F32 and mnmx.shape == (B, 2), (what, raw.shape, mnmx.shape)
    preset(what + ": guard", raw[n:])
    got = raw[:n].reshape(B, H, W)
    x4 = x[..., None]
    ref = resize_truth(x4, H, W, False)[..., 0]
    # float32 blend: two weight roundings and four operations on values no larger than the largest tap; plus the coordinate round trip
    mag = blend(np.abs(x4), lerp_taps(H, nh), lerp_taps(W, nw))[..., 0]
    tol = 8 * U24 * mag + bilinear_coord_tolerance(x4, H, W)[..., 0] + 2.0 ** -149
    out = {"value": check(what + ": vs float64 interpolate(align_corners=False)", got, ref, tol)}
    same_bytes(what + ": min / max bit-equal to those of the kernel's own output", np.ascontiguousarray(mnmx, F32), frame_minmax(got))
    return out


# =====================================================================================================================
# ZoeDepth head (zoe_kernels.hip), n = 2
# =====================================================================================================================
ZOE_N = 2
ZOE_PAIRS = [((3, 4), (6, 8)), ((3, 4), (7, 9)), ((1, 1), (3, 3)), ((5, 5), (5, 5))]
ZOE_LDS = [(128, 128, 128), (192, 192, 192), (192, 128, 192)]     # (lda, lds, ldo) of bilerp_add: the engine's, all wide, mixed


def halfs_verify(what, raw, rows: int, ld: int, cols: int, guard: int) -> np.ndarray:
    """raw uint8 [rows + guard, 2 ld] -> float16 [rows, cols]; guard rows and the columns behind `cols` must still be preset"""
    assert raw.shape == (rows + guard, 2 * ld) and raw.dtype == np.uint8, (what, raw.shape)
    preset(what + ": guard rows", raw[rows:])
    h = raw[:rows].view(np.float16)
    preset(what + ": row tails", h[:, cols:])
    return h[:, :cols]


# ---- softplus ----
SP_ROWS, SP_COLS, SP_LD = 6, 5, 8
SP_VALUES = [20.0, float(np.nextafter(F32(20), F32(30))), 25.0, -104.0, 0.0, 1e-3, -1e-3, 100.0, 19.999, 3.0, -3.0, 88.0]
# 100: expf overflows, so only the threshold keeps the result finite (20 .. 88 give x to float32 either way)


def sp_data(guard: int = 2):
    """the whole buffer [rows + guard, ld]: the values in columns [0, cols), 0xFF bytes elsewhere"""
    g = rng(600)
    v = np.concatenate([np.asarray(SP_VALUES, F32), (4 * g.standard_normal(SP_ROWS * SP_COLS - len(SP_VALUES))).astype(F32)])
    buf = np.frombuffer(raw_rows(SP_ROWS + guard, 4 * SP_LD).tobytes(), F32).reshape(-1, SP_LD).copy()
    buf[:SP_ROWS, :SP_COLS] = v.reshape(SP_ROWS, SP_COLS)
    return buf


def sp_restated(buf, bug=None):
    """float32 softplus, threshold 20.  bug 'no_threshold'"""
    out = buf.copy()
    x = buf[:SP_ROWS, :SP_COLS]
    with np.errstate(over="ignore"):
        y = np.log1p(np.exp(x)).astype(F32)
    out[:SP_ROWS, :SP_COLS] = y if bug == "no_threshold" else np.where(x > 20, x, y)
    return out


def sp_verify(what, got, buf, guard: int = 2) -> dict:
    assert got.shape == buf.shape and got.dtype == F32
    mask = np.zeros(buf.shape, bool)
    mask[:SP_ROWS, :SP_COLS] = True
    preset(what + ": columns and rows outside the payload", got[~mask])
    x = buf[:SP_ROWS, :SP_COLS].astype(np.float64)
    e = np.exp(x)
    ref = np.log1p(e)
    # log1pf's result within ULP2 (assumed); expf's within ULP2 (assumed), carried through d log1p(e) / de = 1 / (1 + e); one float32
    # rounding of x itself above the threshold; 2^-149: where exp underflows the result is 0 or the smallest subnormal
    tol = ULP2 * ref + ULP2 * e / (1 + e) + U24 * np.abs(x) * (x > 20) + 2.0 ** -149
    return {"value": check(what + ": vs float64 log1p(exp(x))", got[:SP_ROWS, :SP_COLS], ref, tol)}


# ---- dot32_relu ----
DOT_ROWS = 257
DOT_LDS = [32, 64]


def dot_data(ld: int):
    g = rng(610 + ld)
    return f16r(g.standard_normal((DOT_ROWS, 32))), (g.standard_normal(32) / 4).astype(F32), 0.1


def dot_restated(act, w2, b2, guard: int = GUARD, bug=None):
    """bug 'no_relu'"""
    s = act.astype(np.float64) @ w2.astype(np.float64) + np.float64(F32(b2))
    raw = np.frombuffer(raw_rows(1, 4 * (DOT_ROWS + guard)).tobytes(), F32).copy()
    raw[:DOT_ROWS] = (s if bug == "no_relu" else np.maximum(s, 0.0)).astype(F32)
    return raw


def dot_verify(what, raw, act, w2, b2, guard: int = GUARD) -> dict:
    assert raw.shape == (DOT_ROWS + guard,) and raw.dtype == F32
    preset(what + ": guard", raw[DOT_ROWS:])
    a, w = act.astype(np.float64), w2.astype(np.float64)
    ref = np.maximum(a @ w + np.float64(F32(b2)), 0.0)
    tol = 33 * U24 * (np.abs(a) @ np.abs(w) + abs(b2)) + 2.0 ** -149        # 32 float32 products added to b2
    return {"value": check(what + ": vs the float64 dot product", raw[:DOT_ROWS], ref, tol)}


# ---- bilerp_add ----
def ba_data(pair):
    (h, w), (H, W) = pair
    g = rng(620 + h + W)
    return f16r(g.standard_normal((ZOE_N, H, W, 128))), f16r(g.standard_normal((ZOE_N, h, w, 128)))


def ba_restated(a, src, ldo: int, guard: int = GUARD, bug=None):
    """bug 'align'"""
    n, H, W, C = a.shape
    v = a.astype(np.float64) + blend(src, ac_taps(H, src.shape[1], bug), ac_taps(W, src.shape[2], bug))
    raw = raw_rows(n * H * W + guard, 2 * ldo)
    raw.view(np.float16)[:n * H * W, :C] = v.astype(F32).astype(np.float16).reshape(-1, C)
    return raw


def ba_verify(what, raw, a, src, ldo: int, guard: int = GUARD) -> dict:
    n, H, W, C = a.shape
    got = halfs_verify(what, raw, n * H * W, ldo, C, guard).astype(np.float64).reshape(a.shape)
    ref = a.astype(np.float64) + resize_truth(src, H, W, True)
    mag = np.abs(a) + blend(np.abs(src), ac_taps(H, src.shape[1]), ac_taps(W, src.shape[2]))
    # one fp16 output rounding of truth; the float32 blend and add (8 roundings on the magnitudes); the coordinate round trip
    tol = 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + 8 * U24 * mag + bilinear_coord_tolerance(src, H, W)
    return {"value": check(what + ": vs float64 a + interpolate(src, align_corners=True)", got, ref, tol)}


# ---- attractor ----
AT_NA = [16, 8, 4, 1]
AT_LDA, AT_ALPHA = 16, 300.0
AT_PAIR = ((3, 4), (7, 9))


def at_data(nA: int):
    """bin centres ascending over the 64 bins (metric depths); attractor points at a centre +- about 1 / sqrt(alpha), where
    dx / (1 + alpha dx^2) peaks, at ordinary distances, and on a centre"""
    (h, w), (H, W) = AT_PAIR
    g = rng(630 + nA)
    bprev = (np.sort(g.random((ZOE_N, h, w, 64)) * 8 + 0.5, -1)).astype(F32)
    b = blend(bprev, ac_taps(H, h), ac_taps(W, w)).reshape(-1, 64)
    rows = b.shape[0]
    A = (g.random((rows, AT_LDA)) * 9).astype(F32)
    pick = g.integers(0, 64, (rows, AT_LDA))
    peak = np.take_along_axis(b, pick, 1) + np.where(g.random((rows, AT_LDA)) < 0.5, -1, 1) * (1 + 0.02 * g.standard_normal((rows, AT_LDA))) / np.sqrt(AT_ALPHA)
    near = g.random((rows, AT_LDA)) < 0.5
    A[near] = peak[near].astype(F32)
    A[:, nA:] = np.nan                          # columns the launch must not read
    return A, bprev


def at_truth(A, nA, bprev, H, W):
    """the oracle's attractor update on float64: b + mean_a inv_attractor(A_a - b), b = interpolate(b_prev, align_corners=True)"""
    b = torch.from_numpy(resize_truth(bprev, H, W, True)).permute(0, 3, 1, 2)                   # [n, 64, H, W]
    At = torch.from_numpy(A[:, :nA].astype(np.float64).reshape(b.shape[0], H, W, nA)).permute(0, 3, 1, 2)
    delta = torch.mean(Z.inv_attractor(At.unsqueeze(2) - b.unsqueeze(1)), dim=1)
    return (b + delta).permute(0, 2, 3, 1).numpy()


def at_restated(A, nA, bprev, H, W, guard: int = 2, bug=None):
    """bug 'sum' (the mean's division by nA missing), 'align'"""
    n, h, w, _ = bprev.shape
    b = blend(bprev, ac_taps(H, h, bug), ac_taps(W, w, bug)).reshape(-1, 64)
    dx = A[:, :nA].astype(np.float64)[:, :, None] - b[:, None, :]
    s = (dx / (1 + AT_ALPHA * dx * dx)).sum(1)
    v = b + (s if bug == "sum" else s / nA)
    raw = np.frombuffer(raw_rows(n * H * W + guard, 256).tobytes(), F32).reshape(-1, 64).copy()
    raw[:n * H * W] = v.astype(F32)
    return raw


def at_verify(what, raw, A, nA, bprev, H, W, guard: int = 2) -> dict:
    n, h, w, _ = bprev.shape
    rows = n * H * W
    assert raw.shape == (rows + guard, 64) and raw.dtype == F32
    preset(what + ": guard rows", raw[rows:])
    ref = at_truth(A, nA, bprev, H, W).reshape(rows, 64)
    b = resize_truth(bprev, H, W, True).reshape(rows, 64)
    a = A[:, :nA].astype(np.float64)
    dx = a[:, :, None] - b[:, None, :]
    f = np.abs(dx / (1 + AT_ALPHA * dx * dx))
    # the bin centre: float32 blend (8 u) and the coordinate round trip; f(dx) = dx / (1 + alpha dx^2) has |f'| <= 1, so the error of dx - the
    # centre's and one rounding of the difference - passes at most unchanged, once through b and once through the mean; f itself is four
    # float32 operations, the sum nA more, then the division and the final add
    db = 8 * U24 * blend(np.abs(bprev), ac_taps(H, h), ac_taps(W, w)).reshape(rows, 64) + \
        np.broadcast_to(bilinear_coord_tolerance(bprev, H, W), (n, H, W, 64)).reshape(rows, 64)
    tol = 2 * db + U24 * (np.abs(a).max(1, keepdims=True) + np.abs(b)) + (nA + 6) * U24 * f.mean(1) + 2 * U24 * np.abs(ref)
    return {"value": check(what + ": vs the oracle's attractor update in float64", raw[:rows], ref, tol)}


# ---- zoe_cat ----
CAT_LD_ACT, CAT_LD_EMB = 64, 192


def cat_data(pair):
    (h, w), (H, W) = pair
    g = rng(640 + h + W)
    rows = ZOE_N * H * W
    return f16r(g.standard_normal((rows, 32))), (3 * g.random(rows)).astype(F32), f16r(g.standard_normal((ZOE_N, h, w, 128)))


def cat_restated(act, rel, emb, H, W, guard: int = 4, bug=None):
    """bug 'shift': the embedding starts at column 32 (over rel) instead of 33"""
    n, h, w, _ = emb.shape
    rows = n * H * W
    raw = raw_rows(rows + guard, 384)
    o = raw.view(np.float16)
    o[:rows] = 0
    o[:rows, :32] = act.astype(np.float16)
    o[:rows, 32] = rel.astype(np.float16)
    e = blend(emb, ac_taps(H, h), ac_taps(W, w)).reshape(rows, 128).astype(F32).astype(np.float16)
    at = 32 if bug == "shift" else 33
    o[:rows, at:at + 128] = e
    return raw


def cat_verify(what, raw, act, rel, emb, H, W, guard: int = 4) -> dict:
    n, h, w, _ = emb.shape
    rows = n * H * W
    o = halfs_verify(what, raw, rows, 192, 192, guard)
    same_bytes(what + ": columns 0 .. 31 = act", o[:, :32], act.astype(np.float16))
    same_bytes(what + ": column 32 = f16(rel)", o[:, 32], rel.astype(np.float16))
    same_u8(what + ": columns 161 .. 191 zero bytes", o[:, 161:].copy().view(np.uint8), np.zeros((rows, 62), np.uint8))
    ref = resize_truth(emb, H, W, True).reshape(rows, 128)
    mag = blend(np.abs(emb), ac_taps(H, h), ac_taps(W, w)).reshape(rows, 128)
    tol = 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + 8 * U24 * mag + np.broadcast_to(bilinear_coord_tolerance(emb, H, W), (n, H, W, 128)).reshape(rows, 128)
    return {"emb": check(what + ": columns 33 .. 160 vs float64 interpolate(emb, align_corners=True)", o[:, 33:161].astype(np.float64), ref, tol)}


# ---- logbinom_depth ----
LB_LD_PT = 8
LB_PAIR = ((3, 4), (7, 9))
LB_MIN_T, LB_MAX_T = F32(0.0212), F32(50.0)
LB_CLAMPS = {"p_hi": (30.0, -30.0), "p_lo": (-30.0, 30.0), "t_hi": (30.0, -30.0), "t_lo": (-30.0, 30.0)}


def lb_data():
    """pt [rows, 8] (columns 4 .. 7 NaN: never read), bins [n, h, w, 64].  The first rows drive p to both clamps (q = +-30 -> p within 1e-4
    of 1 / 0) and t to both ends of [0.0212, 50], in all four combinations; the rest are ordinary"""
    (h, w), (H, W) = LB_PAIR
    g = rng(650)
    rows = ZOE_N * H * W
    pt = np.full((rows, LB_LD_PT), np.nan, F32)
    pt[:, :4] = (2 * g.standard_normal((rows, 4))).astype(F32)
    i = 0
    for pk in ("p_hi", "p_lo"):
        for tk in ("t_hi", "t_lo"):
            pt[i, 0:2] = LB_CLAMPS[pk]
            pt[i, 2:4] = LB_CLAMPS[tk]
            pt[i + 4, 0:2] = LB_CLAMPS[pk]          # one clamp at a time, the other pair ordinary
            pt[i + 8, 2:4] = LB_CLAMPS[tk]
            i += 1
    bins = np.sort(g.random((ZOE_N, h, w, 64)) * 9 + 0.3, -1).astype(F32)
    return pt, bins


def _sp64(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


def lb_truth(pt, bins, H, W):
    """the oracle's conditional_log_binomial after its MLP, and the expectation over the resized centres, on float64 -> (depth [rows], p, t)"""
    q = torch.from_numpy(pt[:, :4].astype(np.float64))
    s = F.softplus(q) + Z.P_EPS
    p = s[:, 0] / (s[:, 0] + s[:, 1])
    t = (Z.MAX_TEMP - Z.MIN_TEMP) * (s[:, 2] / (s[:, 2] + s[:, 3])) + Z.MIN_TEMP
    eps = 1e-4
    om, xx = torch.clamp(1 - p, eps, 1)[:, None], torch.clamp(p, eps, 1)[:, None]
    k = torch.arange(0, Z.N_BINS, dtype=torch.float64)[None]
    y = Z.log_binom(torch.tensor(float(Z.N_BINS - 1), dtype=torch.float64), k) + k * torch.log(xx) + (Z.N_BINS - 1 - k) * torch.log(om)
    prob = torch.softmax(y / t[:, None], dim=1).numpy()
    centers = resize_truth(bins, H, W, True).reshape(-1, 64)
    return (prob * centers).sum(1), p.numpy(), t.numpy()


def lb_restated(pt, bins, H, W, ulp=0.0, pattern=0, bug=None) -> np.ndarray:
    """logbinom_depth_kernel operation by operation in numpy float32 (63 + 1e-7 == 63; k + 1e-7 is k from k = 2 on; the k = 0 and k = 63
    terms multiply a logarithm by 1e-7 and by 0) -> float32 [rows].  ulp: every logf / expf / log1pf result and every product feeding y is
    moved by `ulp` float32 ulps, the sign chosen per bin by `pattern` (0 all up, 1 alternating, 2 low bins up and high bins down, 3 the
    reverse) - the hook the tolerance is made with.  bug 'k_swap': k and 63 - k exchanged in the two power terms"""
    n, h, w, _ = bins.shape
    kf = np.arange(64, dtype=F32)[None]
    sign = {0: np.ones(64), 1: np.where(np.arange(64) % 2 == 0, 1.0, -1.0), 2: np.where(np.arange(64) < 32, 1.0, -1.0),
            3: np.where(np.arange(64) < 32, -1.0, 1.0)}[pattern].astype(F32)[None]

    def nudge(v, s=F32(1)):
        return (v * (F32(1) + F32(ulp) * F32(2.0 ** -23) * s)).astype(F32) if ulp else v.astype(F32)

    def sp(x):
        with np.errstate(over="ignore"):
            return np.where(x > 20, x, nudge(np.log1p(nudge(np.exp(x))))).astype(F32)
    q = pt[:, :4].astype(F32)
    s = (sp(q) + F32(1e-4)).astype(F32)
    p = (s[:, 0] / (s[:, 0] + s[:, 1])).astype(F32)[:, None]
    t = ((LB_MAX_T - LB_MIN_T) * (s[:, 2] / (s[:, 2] + s[:, 3])) + LB_MIN_T).astype(F32)[:, None]
    eps = F32(1e-4)
    om = np.minimum(np.maximum(F32(1) - p, eps), F32(1))
    xp = np.minimum(np.maximum(p, eps), F32(1))
    nn = F32(63) + F32(1e-7)
    kk = (kf + F32(1e-7)).astype(F32)
    with np.errstate(divide="ignore"):
        lb = (nudge(nn * nudge(np.log(np.full((1, 1), nn, F32))), sign) - nudge(kk * nudge(np.log(kk), sign), sign)
              - nudge((nn - kk) * nudge(np.log((nn - kk + F32(1e-7)).astype(F32)), sign), sign)).astype(F32)
        k1, k2 = (F32(63) - kf, kf) if bug == "k_swap" else (kf, F32(63) - kf)
        y = ((lb + nudge(k1 * nudge(np.log(xp), sign), sign) + nudge(k2 * nudge(np.log(om), sign), sign)) / t).astype(F32)
    e = nudge(np.exp((y - y.max(1, keepdims=True)).astype(F32)), sign)
    center = blend(bins, ac_taps(H, h), ac_taps(W, w)).reshape(-1, 64).astype(F32)
    return ((e * center).sum(1, dtype=F32) / e.sum(1, dtype=F32)).astype(F32)


def lb_tolerance(pt, bins, H, W):
    """the restatement's own distance from truth (float32 arithmetic, computed here on the CPU) plus what 2 ulp (assumed) on every logf /
    expf / log1pf result - and as much on every product, for a compiler that contracts them into FMAs - does to the restatement through the
    softmax, the largest over four sign patterns; plus the centres' coordinate round trip and two roundings of the result"""
    ref, _, _ = lb_truth(pt, bins, H, W)
    base = lb_restated(pt, bins, H, W).astype(np.float64)
    moved = np.zeros_like(base)
    for pat in range(4):
        for u in (2.0, -2.0):
            moved = np.maximum(moved, np.abs(lb_restated(pt, bins, H, W, ulp=u, pattern=pat).astype(np.float64) - base))
    n = bins.shape[0]
    ct = np.broadcast_to(bilinear_coord_tolerance(bins, H, W), (n, H, W, 64)).reshape(-1, 64).max(1)
    return np.abs(base - ref) + moved + ct + 70 * U24 * np.abs(ref)


def lb_raw(depth, guard: int = GUARD):
    raw = np.frombuffer(raw_rows(1, 4 * (len(depth) + guard)).tobytes(), F32).copy()
    raw[:len(depth)] = depth
    return raw


def lb_verify(what, raw, pt, bins, H, W, guard: int = GUARD) -> dict:
    rows = pt.shape[0]
    assert raw.shape == (rows + guard,) and raw.dtype == F32
    preset(what + ": guard", raw[rows:])
    ref, _, _ = lb_truth(pt, bins, H, W)
    return {"value": check(what + ": vs the oracle's log-binomial expectation in float64", raw[:rows], ref, lb_tolerance(pt, bins, H, W))}


# ---- pil_resize ----
PIL_IN = (8, 12)
PIL_OUT = [(5, 7), (19, 30), (8, 30), (19, 12), (8, 12)]      # down, up, horizontal only, vertical only, copy


def pil_data():
    return (rng(660).standard_normal((ZOE_N,) + PIL_IN) * 3 + 5).astype(F32)


def pil_restated(x, H, W, guard: int = GUARD, bug=None):
    """zoe_oracle.pil_resize_f32 per map.  bug 'end': the bounds' second entry read as the END index instead of the tap count"""
    def one(img):
        if bug != "end":
            return Z.pil_resize_f32(img, H, W)
        cur = img
        for axis, out in ((1, W), (0, H)):
            if out == cur.shape[axis]:
                continue
            lo, cnt, kk = Z.pil_coeffs(cur.shape[axis], out)
            src = np.moveaxis(cur, axis, 0).astype(np.float64)
            res = np.stack([sum(src[lo[i] + j] * kk[i, j] for j in range(max(cnt[i] - lo[i], 0))) + np.zeros(src.shape[1]) for i in range(out)])
            cur = np.moveaxis(res.astype(F32), 0, axis)
        return cur
    out = np.stack([one(m) for m in x])
    return lb_raw(out.ravel(), guard)


def pil_truth(x, H, W):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(m, mode="F").resize((W, H), Image.BICUBIC), F32) for m in x])


def pil_verify(what, raw, x, H, W, guard: int = GUARD):
    n = x.shape[0] * H * W
    assert raw.shape == (n + guard,) and raw.dtype == F32
    preset(what + ": guard", raw[n:])
    got = raw[:n].reshape(x.shape[0], H, W)
    same_bytes(what + ": bit-equal to PIL.Image.resize", got, pil_truth(x, H, W))
    same_bytes(what + ": bit-equal to zoe_oracle.pil_resize_f32", got, np.stack([Z.pil_resize_f32(m, H, W) for m in x]))


# =====================================================================================================================
# pre-process (elementwise.hip preprocess_kernel): u8 frames -> normalised CHW + the fused 14 x 14 im2col, both tap tables
# =====================================================================================================================
PREP_CASES = {              # mode -> frame sizes (H, W); two frames each, one at 2160 x 3840
    "cubic": [(1, 1), (2, 3),           # every tap clamps
              (7, 13), (96, 128),       # upscale
              (600, 333),               # portrait, the network is not square
              (1080, 1920)],
    "metric": [(1, 1), (1, 7), (5, 1), (2, 3),      # scale 0 on one or both axes
               (392, 518),              # the identity table: lambda = 0 everywhere
               (393, 519), (360, 640), (1080, 1920), (2160, 3840)],
}
PREP_SAT = (7, 13)                      # the saturating frames: all 0, then all 255
PREP_KP = 640                           # halfs per im2col row (DepthEngine's patchA_), 588 of them live
PREP_ROUNDINGS = 13                     # product, 3 adds, product, 3 adds, 1 / 255 and its product, the subtract, 1 / std and its product
PREP_MEAN = np.array([0.485, 0.456, 0.406])
PREP_STD = np.array([0.229, 0.224, 0.225])
PREP_BUGS = {"cubic": ["a_half", "no_half", "no_clamp", "swap_xy", "bgr", "norm_rot", "pypx"],
             "metric": ["align", "coord64", "swap_xy", "bgr", "norm_rot", "pypx"]}


def prep_net(mode: str, H: int, W: int):
    if mode == "metric":
        return Z.NET_H, Z.NET_W
    from oracle import depth_oracle as O
    nw, nh = O.net_size(W, H)
    return nh, nw


def prep_frames_n(H: int, W: int) -> int:
    return 1 if H * W >= 2160 * 3840 else 2


_PREP_CACHE = {}


def prep_data(mode: str, H: int, W: int) -> np.ndarray:
    """seeded uint8 frames [n, H, W, 3], every frame its own noise (the hardest content for a resize: no two taps agree), with a patch of
    0 and a patch of 255 where there is room; shared, read-only"""
    key = ("data", mode, H, W)
    if key not in _PREP_CACHE:
        g = rng(700 + 7 * H + W + (1 if mode == "metric" else 0))
        f = g.integers(0, 256, (prep_frames_n(H, W), H, W, 3), dtype=np.uint8)
        if H >= 6 and W >= 6:
            f[0, :H // 3, :W // 3] = 0
            f[-1, -(H // 3):, -(W // 3):] = 255
        f.setflags(write=False)
        _PREP_CACHE[key] = f
    return _PREP_CACHE[key]


def prep_sat_data() -> np.ndarray:
    f = np.zeros((2,) + PREP_SAT + (3,), np.uint8)
    f[1] = 255
    return f


def _cubic_table(src: int, dst: int, bug=None):
    """oracle.depth_oracle.cubic_taps with room for the planted faults: A = -0.5, no half-pixel offset, taps that are not clamped (a tap
    outside reads the other end of the row / column - some other pixel, as the memory next to the row would be)"""
    from oracle import depth_oracle as O
    if bug not in ("a_half", "no_half", "no_clamp"):
        idx, w = O.cubic_taps(src, dst)
        return idx.astype(np.int64), w.astype(F32)
    scale = 1.0 / (dst / src)
    d = np.arange(dst, dtype=np.float64)
    fx = (d * scale if bug == "no_half" else (d + 0.5) * scale - 0.5).astype(F32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(F32)
    raw = sx[:, None] + np.arange(-1, 3)[None, :]
    idx = np.mod(raw, src) if bug == "no_clamp" else np.clip(raw, 0, src - 1)
    if bug == "a_half":
        A, one = F32(-0.5), F32(1)
        c0 = ((A * (fx + one) - F32(5) * A) * (fx + one) + F32(8) * A) * (fx + one) - F32(4) * A
        c1 = ((A + F32(2)) * fx - (A + F32(3))) * fx * fx + one
        c2 = ((A + F32(2)) * (one - fx) - (A + F32(3))) * (one - fx) * (one - fx) + one
        w = np.stack([c0, c1, c2, one - c0 - c1 - c2], -1).astype(F32)
    else:
        w = O._cubic_coeffs(fx)
    return idx, w.astype(F32)


def _ac_table(src: int, dst: int, bug=None):
    """engine.hip bilinear_ac_taps: torch's align_corners=True rule for float32 input as four taps (i0, i1, i1, i1) weighing
    (1 - lambda, lambda, 0, 0), the coordinate in float32.  bugs: 'align' (align_corners=False), 'coord64' (the coordinate in float64)"""
    if bug == "coord64":
        s = (src - 1) / (dst - 1) * np.arange(dst, dtype=np.float64) if dst > 1 else np.zeros(dst)
        i0 = np.minimum(s.astype(np.int64), src - 1)
        i1, l = i0 + (i0 < src - 1), (s - i0).astype(F32)
    else:
        i0, i1, l = ac_taps(dst, src, "align" if bug == "align" else None)
        l = l.astype(F32)
    idx = np.stack([i0, i1, i1, i1], -1).astype(np.int64)
    w = np.zeros((dst, 4), F32)
    w[:, 0] = F32(1) - l
    w[:, 1] = l
    return idx, w


def prep_tables(mode: str, H: int, W: int, bug=None):
    """-> (yi [nh, 4], yw float32 [nh, 4], xi [nw, 4], xw float32 [nw, 4]).  bug 'swap_xy': each axis' table built for the other axis'
    source length (indices held inside the frame)"""
    nh, nw = prep_net(mode, H, W)
    tab = _cubic_table if mode == "cubic" else _ac_table
    tb = bug if bug in ("a_half", "no_half", "no_clamp", "align", "coord64") else None
    sh, sw = (W, H) if bug == "swap_xy" else (H, W)
    yi, yw = tab(sh, nh, tb)
    xi, xw = tab(sw, nw, tb)
    return np.minimum(yi, H - 1), yw, np.minimum(xi, W - 1), xw


def _prep_resize(p, tables, absw=False):
    """p [n, H, W, 3] float64 -> [n, nh, nw, 3]: sum_ty sum_tx wy wx p in float64 with the float32 weights (their moduli with absw)"""
    yi, yw, xi, xw = tables
    yw, xw = yw.astype(np.float64), xw.astype(np.float64)
    if absw:
        yw, xw = np.abs(yw), np.abs(xw)
    tmp = sum(p[:, :, xi[:, t]] * xw[None, None, :, t, None] for t in range(4))
    return sum(tmp[:, yi[:, t]] * yw[None, :, t, None, None] for t in range(4))


def prep_truth(frames, mode: str):
    """-> (truth [n, 3, nh, nw] float64, tolerance of the same shape).  The tables are the reference's own - oracle.depth_oracle.cubic_taps
    with float32 coefficients; torch's float32 align_corners=True index rule - every value operation is float64:
    (sum w p / 255 - mean) / std.  tolerance = 13 x 2^-24 x (sum |w_y| |w_x| p / 255 + mean) / std, element-wise: 13 float32 roundings on the
    kernel's longest path (PREP_ROUNDINGS), each no larger than 2^-24 of the magnitude it rounds; contraction into FMAs only removes some"""
    n, H, W, _ = frames.shape
    key = ("truth", mode, H, W) if frames is _PREP_CACHE.get(("data", mode, H, W)) else None
    if key in _PREP_CACHE:
        return _PREP_CACHE[key]
    tables = prep_tables(mode, H, W)
    p = frames.astype(np.float64) / 255.0
    ref = ((_prep_resize(p, tables) - PREP_MEAN) / PREP_STD).transpose(0, 3, 1, 2)
    mag = ((_prep_resize(p, tables, absw=True) + PREP_MEAN) / PREP_STD).transpose(0, 3, 1, 2)
    out = (np.ascontiguousarray(ref), PREP_ROUNDINGS * U24 * np.ascontiguousarray(mag))
    if key:
        _PREP_CACHE[key] = out
    return out


def prep_patch_rows(chw, bug=None) -> np.ndarray:
    """chw float32 [n, 3, nh, nw] -> float16 [n P, 588]: row (b, gy, gx), column c 196 + py 14 + px.  bug 'pypx': px 14 + py"""
    n, _, nh, nw = chw.shape
    gh, gw = nh // 14, nw // 14
    t = chw.reshape(n, 3, gh, 14, gw, 14)                        # b c gy py gx px
    t = t.transpose(0, 2, 4, 1, 5, 3) if bug == "pypx" else t.transpose(0, 2, 4, 1, 3, 5)
    return np.ascontiguousarray(t).reshape(n * gh * gw, 588).astype(np.float16)


def prep_raw_rows(n: int, nh: int, nw: int, guard: int = GUARD) -> int:
    return -(-(n * (nh // 14) * (nw // 14)) // 256) * 256 + guard


def prep_restated(frames, mode: str, guard: int = GUARD, bug=None):
    """preprocess_kernel operation by operation in numpy float32 (no FMA): r = sum_tx float(p) wx, acc = sum_ty r wy, both from 0 in tap
    order; v = (acc (1 / 255) - mean) (1 / std) with the three constants rounded to float32 -> (chw float32 [n, 3, nh, nw], raw uint8
    [round_up(n P, 256) + guard, 1280]).  bugs: the table faults of prep_tables / _cubic_table / _ac_table, 'bgr' (channels reversed),
    'norm_rot' (mean / std of the next channel), 'pypx' (the im2col column px 14 + py)"""
    n, H, W, _ = frames.shape
    nh, nw = prep_net(mode, H, W)
    yi, yw, xi, xw = prep_tables(mode, H, W, bug)
    acc = np.zeros((n, nh, nw, 3), F32)
    for ty in range(4):
        rows = frames[:, yi[:, ty]]                              # [n, nh, W, 3] uint8
        r = np.zeros((n, nh, nw, 3), F32)
        for tx in range(4):
            r = (r + rows[:, :, xi[:, tx]].astype(F32) * xw[None, None, :, tx, None]).astype(F32)
        acc = (acc + r * yw[None, :, ty, None, None]).astype(F32)
    if bug == "bgr":
        acc = acc[..., ::-1]
    mean, istd = PREP_MEAN.astype(F32), (F32(1) / PREP_STD.astype(F32)).astype(F32)
    if bug == "norm_rot":
        mean, istd = np.roll(mean, -1), np.roll(istd, -1)
    v = ((acc * (F32(1) / F32(255)) - mean).astype(F32) * istd).astype(F32)
    chw = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    raw = raw_rows(prep_raw_rows(n, nh, nw, guard), 2 * PREP_KP)
    raw.view(np.float16)[:n * (nh // 14) * (nw // 14), :588] = prep_patch_rows(chw, bug)
    return chw, raw


def prep_verify(what, chw, raw, frames, mode: str, guard: int = GUARD, ref=None, tol=None) -> dict:
    """chw against float64 truth within the derived bound; the im2col rows bit-equal to fp16 of the SAME chw (both are stores of one
    register); columns 588 .. 639, the rows behind n P and the guard rows still 0xFF.  ref / tol: another truth for the same frames (the
    saturating case's constants)"""
    n, H, W, _ = frames.shape
    nh, nw = prep_net(mode, H, W)
    P = (nh // 14) * (nw // 14)
    assert chw.shape == (n, 3, nh, nw) and chw.dtype == F32, (what, chw.shape, chw.dtype)
    assert raw.shape == (prep_raw_rows(n, nh, nw, guard), 2 * PREP_KP) and raw.dtype == np.uint8, (what, raw.shape)
    if ref is None:
        ref, tol = prep_truth(frames, mode)
    out = {"value": check(what + ": chw vs float64 (sum w p / 255 - mean) / std", chw, ref, tol)}
    preset(what + ": rows behind the last patch and guard rows", raw[n * P:])
    h = raw[:n * P].view(np.float16)
    preset(what + ": columns 588 .. 639", h[:, 588:])
    same_bytes(what + ": im2col [(b, gy, gx), c 196 + py 14 + px] = fp16 of the kernel's own chw", h[:, :588], prep_patch_rows(chw))
    return out
