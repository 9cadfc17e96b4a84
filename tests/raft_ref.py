"""float64 truth and exact restatements of the flow_raft band's own kernels (CPU only; a helper module of the tests, not a conftest).

Truth is written from the reference's definitions (the formulas oracle/raft_oracle.py cites: corr_pyramid, corr_lookup, update_block,
upsample_flow) in float64.  A restatement computes the same thing but rounds where the kernel rounds - fp16 pooled features, fp16 volume
entries, the fp32 normalise / un-normalise round trip of the sample coordinates, fp16 operands - so that what is left between it and the
kernel is the accumulation order and the storage rounding, which the tolerances below bound from the arithmetic.  Every function takes a
`bug=` name that plants one fault (tests/test_raft_ref_cpu.py asserts the tolerances see each of them).
"""
from __future__ import annotations

import numpy as np

from split_ref import conv_nhwc, e4m3_q, f16, weight_pw

U24 = 2.0 ** -24          # half an fp32 ulp, relative (one rounding of an fp32 operation)


def f16_step(v) -> np.ndarray:
    """spacing of fp16 values at |v| (subnormal spacing 2^-24 below 2^-14)"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.ldexp(1.0, (e - 10).astype(int))


def rng(seed: int):
    return np.random.default_rng(seed)


# =====================================================================================================================
# pyramid geometry (csrc corr_pyramid_geometry restated; tests compare it with the library's own)
# =====================================================================================================================
def geometry(h8: int, w8: int):
    out = []
    h, w = h8, w8
    for l in range(4):
        wp, hp = -(-w // 8) * 8, -(-h // 8) * 8
        ld = hp * wp
        r = -(-ld // 256) * 256
        if r * 50 <= ld * 51:
            ld = r
        out.append(dict(h=h, w=w, wp=wp, hp=hp, ld=ld))
        h, w = h // 2, w // 2
    return out


# =====================================================================================================================
# correlation pyramid + 9 x 9 x 4 lookup (corr.py:13-60)
# =====================================================================================================================
def pool2(c, ceil: bool = False):
    """avg_pool2d(2, 2) over the last two axes, floor on odd sizes (ceil: the planted bug - a last partial window averaged over what exists)"""
    h, w = c.shape[-2:]
    if ceil:
        ph, pw = h + (h & 1), w + (w & 1)
        p = np.zeros(c.shape[:-2] + (ph, pw), c.dtype)
        cnt = np.zeros((ph, pw))
        p[..., :h, :w] = c
        cnt[:h, :w] = 1
        s = p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]
        k = cnt[0::2, 0::2] + cnt[0::2, 1::2] + cnt[1::2, 0::2] + cnt[1::2, 1::2]
        return s / k
    c = c[..., :h // 2 * 2, :w // 2 * 2]
    return 0.25 * ((c[..., 0::2, 0::2] + c[..., 0::2, 1::2]) + (c[..., 1::2, 0::2] + c[..., 1::2, 1::2]))


def pyramid_truth(fmap1, fmap2, rows=None, bug=None):
    """fmap1 [n, P, 256], fmap2 [n, h8, w8, 256] -> ([levels [R, h_l, w_l]], [magnitude levels]): corr = <f1, f2> / sqrt(256), pooled three
    times over the target dims, float64.  rows: a subset of the n P source rows.  The magnitude levels are the same with |f1|, |f2|."""
    n, h8, w8, _ = fmap2.shape
    P = h8 * w8
    rows = np.arange(n * P) if rows is None else np.asarray(rows)
    f1 = np.asarray(fmap1, np.float64).reshape(n * P, 256)[rows]
    f2 = np.asarray(fmap2, np.float64).reshape(n, P, 256)
    pair = rows // P
    c = np.empty((len(rows), h8, w8))
    m = np.empty_like(c)
    for i in range(n):
        s = pair == i
        c[s] = (f1[s] @ f2[i].T / 16.0).reshape(-1, h8, w8)
        m[s] = (np.abs(f1[s]) @ np.abs(f2[i]).T / 16.0).reshape(-1, h8, w8)
    lv, mg = [c], [m]
    for _ in range(3):
        lv.append(pool2(lv[-1], ceil=bug == "pool_ceil"))
        mg.append(pool2(mg[-1], ceil=bug == "pool_ceil"))
    return lv, mg


def pyramid_restated(fmap1, fmap2, rows=None):
    """the levels as the kernels build them: target features avg-pooled in fp32 and stored as fp16 (avgpool2_nhwc), scaled by 1/16 into fp16
    (corr_tile), one dot product per entry rounded to fp16 (corr_volume; its fp32 accumulation order is not restated - see volume_tolerance)"""
    n, h8, w8, _ = fmap2.shape
    P = h8 * w8
    rows = np.arange(n * P) if rows is None else np.asarray(rows)
    f1 = f16(fmap1).astype(np.float64).reshape(n * P, 256)[rows]
    pair = rows // P
    feat = f16(fmap2)                                        # [n, h, w, 256] float32 holding fp16 values
    lv, mg = [], []
    for l in range(4):
        if l:
            h, w = feat.shape[1] // 2 * 2, feat.shape[2] // 2 * 2
            t = feat[:, :h, :w]
            feat = f16(np.float32(0.25) * ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])))
        tile = f16(feat * np.float32(0.0625)).astype(np.float64)
        h, w = tile.shape[1:3]
        c = np.empty((len(rows), h, w))
        m = np.empty_like(c)
        for i in range(n):
            s = pair == i
            c[s] = (f1[s] @ tile[i].reshape(-1, 256).T).reshape(-1, h, w)
            m[s] = (np.abs(f1[s]) @ np.abs(tile[i].reshape(-1, 256)).T).reshape(-1, h, w)
        lv.append(f16(c).astype(np.float64))
        mg.append(m)
    return lv, mg


def volume_tolerance(level, mag):
    """kernel's volume entry vs pyramid_restated's: 256 products accumulated in fp32 in an order not restated (256 2^-24 sum |a||b|), and where
    that moves the sum across an fp16 rounding boundary the stored value differs by one fp16 step"""
    return 256 * U24 * mag + f16_step(np.abs(level) + 256 * U24 * mag)


def _coords32(flow, P: int, w8: int, l: int, dim_w: int, dim_h: int, rows, bug=None):
    """the kernel's sample coordinates of level l in fp32, operation by operation: (x [R, 9], y [R, 9]) float32"""
    p = (rows % P).astype(np.int64)
    f = np.asarray(flow, np.float32)
    inv = np.float32(1.0 / (1 << (l + 1 if bug == "level_scale" else l)))
    k = np.arange(-4, 5, dtype=np.float32)[None, :]
    out = []
    for base, fl, dim in (((p % w8).astype(np.float32), f[:, 0], dim_w), ((p // w8).astype(np.float32), f[:, 1], dim_h)):
        c = (base + fl)[:, None]                            # fp32 add
        d1 = np.float32(dim - 1)
        g = np.float32(2.0) * (c * inv + k) / d1 - np.float32(1.0)
        if bug == "align_false":                            # grid_sample(align_corners=False): ((g + 1) dim - 1) / 2
            v = ((g + np.float32(1.0)) * np.float32(dim) - np.float32(1.0)) * np.float32(0.5)
        else:
            v = (g + np.float32(1.0)) * np.float32(0.5) * d1
        out.append(v.astype(np.float32))
    return out


def _coords64(flow, P: int, w8: int, l: int, rows, bug=None):
    p = (rows % P).astype(np.int64)
    f = np.asarray(flow, np.float64)
    sc = float(1 << (l + 1 if bug == "level_scale" else l))
    k = np.arange(-4, 5, dtype=np.float64)[None, :]
    x = ((p % w8) + f[:, 0])[:, None] / sc + k
    y = ((p // w8) + f[:, 1])[:, None] / sc + k
    return x, y


def _window(level, x, y, bug=None):
    """bilinear samples of level [R, h, w] at (x[r, i], y[r, j]) -> [R, 9 (i: moves x), 9 (j: moves y)], zeros outside (padding_mode='zeros')"""
    R, h, w = level.shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    x0 = np.clip(x0, -65536, 65536).astype(np.int64)
    y0 = np.clip(y0, -65536, 65536).astype(np.int64)
    out = np.zeros((R, 9, 9))
    ridx = np.arange(R)[:, None, None]
    for dx in (0, 1):
        for dy in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            okx, oky = (xi >= 0) & (xi < w), (yi >= 0) & (yi < h)
            if bug == "third_segment":                      # columns >= 16 past the window's first tile column read as zero
                okx &= (xi - (x0[:, :1] & ~7)) < 16
            xc, yc = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
            v = level[ridx, yc[:, None, :], xc[:, :, None]]
            if bug != "border_clamp":
                v = v * (okx[:, :, None] & oky[:, None, :])
            out += v * ((ax if dx else 1 - ax)[:, :, None] * (ay if dy else 1 - ay)[:, None, :])
    return out


def lookup_truth(levels, flow, P: int, w8: int, rows=None, bug=None):
    """CorrBlock.__call__ in float64: channel l 81 + i 9 + j samples level l at (x / 2^l + i - 4, y / 2^l + j - 4) -> [R, 324]"""
    rows = np.arange(levels[0].shape[0]) if rows is None else np.asarray(rows)
    out = []
    for l, lv in enumerate(levels):
        x, y = _coords64(flow, P, w8, l, rows, bug)
        w = _window(lv, x, y, bug)
        if bug == "swap_ij":
            w = w.transpose(0, 2, 1)
        out.append(w.reshape(len(rows), 81))
    return np.concatenate(out, 1)


def lookup_restated(levels, flow, P: int, w8: int, rows=None, bug=None):
    """the same on fp16-valued levels with the kernel's fp32 coordinate round trip (floor and fraction taken from the fp32 value); the blend
    itself in float64 -> ([R, 324] before the fp16 store, tolerance [R, 324] of the kernel against it)

    tolerance = half an fp16 step of the result
              + the coordinate round trip: the restated fp32 sequence may differ from the compiled one by contraction / division rounding; at
                most 4 fp32 ulps of (dim + |flow| / 2^l + 4) per axis, times the largest difference between adjacent entries of the row's
                level (zero border included) - a bilinear surface's slope along an axis never exceeds that
              + 4 roundings of the fp32 blend (each <= 2^-24 of the largest entry the window can touch)."""
    rows = np.arange(levels[0].shape[0]) if rows is None else np.asarray(rows)
    f = np.abs(np.asarray(flow, np.float64))
    out, tol = [], []
    for l, lv in enumerate(levels):
        h, w = lv.shape[1:]
        x, y = _coords32(flow, P, w8, l, w, h, rows, bug)
        wv = _window(lv, x, y, bug)
        if bug == "swap_ij":
            wv = wv.transpose(0, 2, 1)
        pad = np.pad(lv, ((0, 0), (1, 1), (1, 1)))
        adj = np.maximum(np.abs(np.diff(pad, axis=1)).max((1, 2)), np.abs(np.diff(pad, axis=2)).max((1, 2)))
        vmax = np.abs(lv).max((1, 2))
        cerr = 4 * 2.0 ** -23 * ((w + f[:, 0] / (1 << l) + 4) + (h + f[:, 1] / (1 << l) + 4))
        t = (cerr * adj + 4 * U24 * vmax)[:, None, None]
        out.append(wv.reshape(len(rows), 81))
        tol.append((0.5 * f16_step(np.abs(wv) + t) + t).reshape(len(rows), 81))
    return np.concatenate(out, 1), np.concatenate(tol, 1)


def lookup_index_check(flow, P: int, w8: int, geo, n_rows: int):
    """the integer arithmetic of corr_lookup_kernel restated for every (row, level) of a launch, asserting that every address it forms lies
    inside the level's row (< ld) and inside the LDS window.  geo: the library's geometry.  Returns statistics the tests assert on:
    third-segment windows, rows admitted beyond the padded height by a `ld / wp` rule (the pre-fix bound) with tx >= 1, zero / inside /
    outside shares."""
    rows = np.arange(n_rows)
    st = dict(third=0, windows=0, beyond_hp=0)
    for l, g in enumerate(geo):
        x, y = _coords32(flow, P, w8, l, g["w"], g["h"], rows)
        cx = np.clip(np.floor(x), -65536, 65536).astype(np.int64)       # ci[0..8]
        cy = np.clip(np.floor(y), -65536, 65536).astype(np.int64)       # ci[9..17]
        wt = g["wp"] >> 3
        need3 = cx[:, 8] + 1 - (cx[:, 0] & ~7) >= 16
        # the blend's offsets into the 11 x 24 LDS window: xo + 1 <= 23, yo + 1 <= 10 without the defensive clamps
        xo, yo = cx - (cx[:, :1] & ~7), cy - cy[:, :1]
        assert xo.min() >= 0 and xo.max() <= 22 and yo.min() >= 0 and yo.max() <= 9, (l, xo.max(), yo.max())
        # the blend reads column xo + 1 <= 16 + 7: the third segment (columns 16..23) is read only when need3
        assert np.all((xo.max(1) + 1 >= 16) <= need3), l
        for seg in range(3):
            tx = (cx[:, 0] >> 3) + seg
            for row in range(11):
                yy = cy[:, 0] + row
                ok = ((seg < 2) | need3) & (yy >= 0) & (yy < g["hp"]) & (tx >= 0) & (tx < wt)
                addr = ((yy >> 3) * wt + tx) * 64 + (yy & 7) * 8
                assert np.all(addr[ok] >= 0) and np.all(addr[ok] + 8 <= g["hp"] * g["wp"]) and g["hp"] * g["wp"] <= g["ld"], (l, seg, row)
                old = ((seg < 2) | need3) & (yy >= g["hp"]) & (yy < g["ld"] // g["wp"]) & (tx >= 1) & (tx < wt)
                st["beyond_hp"] += int(old.sum())
        st["third"] += int(need3.sum()) if l == 0 else 0
        st["windows"] += n_rows if l == 0 else 0
    return st


def window_shares(flow, P: int, w8: int, h: int, w: int, n_rows: int):
    """level-0 windows in float64: share inside the level (every one of the 81 samples has weight on a real entry: -1 < x < w, -1 < y < h),
    fully outside (no sample has), and straddling a border (the rest)"""
    x, y = _coords64(flow, P, w8, 0, np.arange(n_rows))
    tx = (x > -1) & (x < w)
    ty = (y > -1) & (y < h)
    inside = tx.all(1) & ty.all(1)
    outside = ~(tx.any(1) & ty.any(1))
    return dict(inside=float(inside.mean()), outside=float(outside.mean()), straddle=float((~inside & ~outside).mean()))


# ---- seeded inputs of the lookup cases (shared by the CPU and the GPU tests) ----
LOOKUP_GRIDS = [            # (name, n, h8, w8, sub-pixel flow std, border flow std)
    ("16x16", 1, 16, 16, 2.0, 8.0),
    ("17x23", 1, 17, 23, 2.0, 8.0),
    ("46x62x3", 3, 46, 62, 4.0, 12.0),
    ("129x17x2", 2, 129, 17, 2.0, 8.0),
    ("24x40", 1, 24, 40, 3.0, 10.0),
]
LARGE_GRID = ("102x180", 1, 102, 180, 4.0, 12.0)


def lookup_features(seed: int, n: int, h8: int, w8: int, detector: bool = False):
    """fp16-representable feature maps.  detector: fmap1 rows are 16 e_c one-hots and fmap2 holds multiples of 64 in [-960, 960], so every
    volume entry (a multiple of 64) and every pooled feature (a multiple of 1 after three levels) is exact"""
    g = rng(seed)
    P = h8 * w8
    if detector:
        f1 = np.zeros((n, P, 256), np.float32)
        f1[np.arange(n)[:, None], np.arange(P)[None, :], g.integers(0, 256, (n, P))] = 16.0
        f2 = (g.integers(-15, 16, (n, h8, w8, 256)) * 64).astype(np.float32)
        return f1, f2
    # smooth + noise, so adjacent volume entries are correlated as real feature maps' are and |entries| are O(1)
    f1 = f16(g.standard_normal((n, P, 256)) * 0.5)
    f2 = f16(g.standard_normal((n, h8, w8, 256)) * 0.5 * 4)
    return f1, f2


def lookup_flows(seed: int, n: int, h8: int, w8: int, sub_std: float, border_std: float):
    """{family: flow [n P, 2] float32}: zero; integers and multiples of 1/8; sub-pixel random; across each border; far"""
    g = rng(seed)
    P = h8 * w8
    R = n * P
    p = np.arange(R) % P
    px, py = (p % w8).astype(np.float64), (p // w8).astype(np.float64)
    fam = {"zero": np.zeros((R, 2))}
    fam["eighths"] = np.where(g.random((R, 1)) < 0.5, g.integers(-6, 7, (R, 2)).astype(np.float64), g.integers(-48, 49, (R, 2)) / 8.0)
    fam["subpixel"] = g.standard_normal((R, 2)) * sub_std
    b = g.standard_normal((R, 2)) * border_std
    side = g.integers(0, 8, R)                              # half of the rows are sent to a chosen border, +- 6 targets around it
    tgt = g.uniform(-6, 6, R)
    b[side == 0, 0] = (tgt - px)[side == 0]
    b[side == 1, 0] = (w8 - 1 + tgt - px)[side == 1]
    b[side == 2, 1] = (tgt - py)[side == 2]
    b[side == 3, 1] = (h8 - 1 + tgt - py)[side == 3]
    fam["border"] = b
    far = g.standard_normal((R, 2)) * sub_std
    idx = g.choice(R, 16, replace=False)
    vals = np.array([1e4, -1e4, 1e6, -1e6])
    for k, r in enumerate(idx):
        far[r, k % 2] = vals[(k // 2) % 4]
        if k >= 8:
            far[r, 1 - k % 2] = vals[(k // 2 + 1) % 4]
    fam["far"] = far
    return {k: v.astype(np.float32) for k, v in fam.items()}


def downward_flows(seed: int, n: int, h8: int, w8: int):
    """129 x 17: flows of 3 .. 12 px downwards on the bottom 8 rows, so that windows reach target rows 136, 137 of the padded level"""
    g = rng(seed)
    P = h8 * w8
    R = n * P
    f = g.standard_normal((R, 2)) * 1.5
    py = (np.arange(R) % P) // w8
    bottom = py >= h8 - 8
    f[bottom, 1] = g.uniform(3.0, 12.0, int(bottom.sum()))
    return f.astype(np.float32)


# =====================================================================================================================
# convf1: 7 x 7, 2 -> 128, ReLU on the flow field (update.py:88)
# =====================================================================================================================
def convf1_truth(flow, w, bias, fp16_flow: bool = False):
    """flow [n, h8, w8, 2] -> (relu(conv + b) [rows, 128], sum |x||w| + |b|); fp16_flow: the operand rounded to fp16 first (by design)"""
    x = f16(flow).astype(np.float64) if fp16_flow else np.asarray(flow, np.float64)
    acc = conv_nhwc(x, w, 1) + np.asarray(bias, np.float64)
    return np.maximum(acc, 0), conv_nhwc(np.abs(x), np.abs(np.asarray(w, np.float64)), 1) + np.abs(np.asarray(bias, np.float64))


def convf1_restated(flow, w, bias, passes: int, mx2: bool = False, bug=None):
    """the kernel's operands: fp16(flow), w_hi (+ w_lo = fp16(w - w_hi) when passes = 2; mx2 - the im2col + GEMM path with fp8 copies - reads
    e4m3(fp16 flow) x e4m3((w - w_hi) 2^pw) instead) -> (value before the fp16 store [rows, 128], tolerance)

    tolerance = n 2^-24 (sum |x||w| + |b|) with n = 98 passes products accumulated in fp32, plus half an fp16 step of the result"""
    flow = np.asarray(flow, np.float32)
    w = np.asarray(w, np.float32)
    if bug == "tap_transposed":
        w = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
    if bug == "channels_swapped":
        flow = flow[..., ::-1]
    if bug == "next_image":                                 # the images stacked into one tall map: taps cross image boundaries
        flow = flow.reshape(1, -1, flow.shape[2], 2)
    a = f16(flow).astype(np.float64)
    w_hi = f16(w)
    segs = [(a, w_hi.astype(np.float64))]
    if passes == 2 and bug != "residual_dropped":
        if mx2:
            segs.append((e4m3_q(f16(flow), 0), e4m3_q(w - w_hi, weight_pw(w, False))))
        else:
            segs.append((a, f16(w - w_hi).astype(np.float64)))
    acc = sum(conv_nhwc(x, ww, 1) for x, ww in segs)
    mag = sum(conv_nhwc(np.abs(x), np.abs(ww), 1) for x, ww in segs) + np.abs(np.asarray(bias, np.float64))
    v = np.maximum(acc + np.asarray(bias, np.float64), 0)
    t = 98 * passes * U24 * mag
    return v, t + 0.5 * f16_step(v + t)


def convf1_data(seed: int, n: int, h8: int, w8: int, scale: float = 60.0, rounded: bool = True):
    g = rng(seed)
    flow = (g.standard_normal((n, h8, w8, 2)) * scale).astype(np.float32)
    flow += (g.standard_normal((n, 1, 1, 2)) * scale).astype(np.float32)
    if rounded:
        flow = f16(flow)
    w = (g.standard_normal((128, 2, 7, 7)) * 98 ** -0.5 / scale * 4).astype(np.float32)
    b = (g.standard_normal(128) * 0.5).astype(np.float32)
    return flow, w, b


# =====================================================================================================================
# flow_head2: 3 x 3, 256 -> 2, + the incoming flow (update.py:11-12, raft.py:131)
# =====================================================================================================================
def flow_head2_truth(x, w, bias, flow):
    acc = conv_nhwc(np.asarray(x, np.float64), w, 1)
    mag = conv_nhwc(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), 1)
    return np.asarray(flow, np.float64) + acc + np.asarray(bias, np.float64), mag


def flow_head2_restated(x, w, bias, flow, split: bool, bug=None):
    """fp16(x) x w_hi (+ w_lo in the split mode) accumulated in fp32, (acc + b) and old + that each one fp32 rounding -> (value, tolerance).

    tolerance = n 2^-24 sum |x||w| + 2^-24 (|acc + b| + |result|) with n = 72 (1 + split) + 5: a lane owns 8 of the 256 channels and
    chains 9 taps x 4 v_dot2 (x 2 in the split mode) into one accumulator - at most two roundings per v_dot2, each bounded by 2^-24 of the
    lane's own sum of |products| - and the 32 lanes' sums meet in a 5-step butterfly.  Summed over the lanes that is n 2^-24 of the whole
    sum |x||w|.  (The flat count n = 2304 (1 + split) treats all products as one chain; it is 30x looser, and at 2^-12 of sum |x||w| it
    could not tell a kernel that drops w_lo - a term of at most 2^-12 sum |x||w| - from a correct one.)"""
    a = f16(x).astype(np.float64)
    w = np.asarray(w, np.float32)
    w_hi = f16(w)
    ws = [w_hi.astype(np.float64)]
    if split and bug != "w_lo_dropped":
        ws.append(f16(w - w_hi).astype(np.float64))
    acc = sum(conv_nhwc(a, ww, 1) for ww in ws)
    mag = sum(conv_nhwc(np.abs(a), np.abs(ww), 1) for ww in ws)
    b = np.asarray(bias, np.float64) * (2 if bug == "bias_twice" else 1)
    old = 0 if bug == "old_flow_dropped" else np.asarray(flow, np.float64)
    v = old + (acc + b)
    return v, (72 * (1 + int(split)) + 5) * U24 * mag + U24 * (np.abs(acc + b) + np.abs(v))


def flow_head2_data(seed: int, n: int, H: int, W: int):
    g = rng(seed)
    x = f16(np.maximum(g.standard_normal((n, H, W, 256)), 0) * 0.7)          # a ReLU'd map, fp16-representable
    # weights whose fp16 rounding residuals all have one sign (0.4 of an fp16 step above w_hi): on a non-negative map the w_lo products add
    # up instead of averaging out, so the residual pass carries ~2^-12.3 of sum |x||w| - what a kernel that drops it loses
    w = f16(g.standard_normal((2, 256, 3, 3)) * 2304 ** -0.5 * 3)
    w = (w.astype(np.float64) + 0.4 * f16_step(w)).astype(np.float32)
    b = (g.standard_normal(2) * 0.2).astype(np.float32)
    flow = (g.standard_normal((n * H * W, 2)) * 5).astype(np.float32)
    return x, w, b, flow


# =====================================================================================================================
# convex upsample + crop + maximum displacement (raft.py:73-84, flow_raft.py:58-60)
# =====================================================================================================================
# __expf is exp2(fl(log2(e) x)) on the hardware's exp2: not IEEE, and the ROCm device-library documentation on the build machine states no
# bound.  tools/probe/expf_probe.hip measures it against float64 on [-170, 0] (nothing to do with the kernel under test): the figure is written
# next to the constant, which allows twice that.
# measured on an MI355X, 4 194 304 points: max relative error 3.853e-6 = 2^-17.99 over [-170, 0] (worst near exp(x) = 2^-126, at x = -87.33);
# 9.47e-7 = 2^-20.01 on [-17.33, 0]; absolute error 1.2e-38 where exp(x) < 2^-126 (flushed to zero).
EXPF_REL_MEASURED = 3.853e-6
EXPF_REL = 2 * EXPF_REL_MEASURED


def upsample_truth(flow, mask, h8: int, w8: int, pad_l: int, pad_t: int, sh: int, sw: int, bug=None):
    """flow [n, P, 2], mask [n P, 576] (channel k 64 + sy 8 + sx) -> (up [n, sh, sw, 2] float64, sum_k softmax_k |8 f_k| in the same layout,
    maxd [n] over the crop)"""
    n = flow.shape[0]
    m = np.asarray(mask, np.float64).reshape(n, h8, w8, 9, 64)
    ax = 4 if bug == "softmax_axis" else 3
    e = np.exp(m - m.max(ax, keepdims=True))
    sm = e / e.sum(ax, keepdims=True)
    f = np.asarray(flow, np.float64).reshape(n, h8, w8, 2) * (1.0 if bug == "no_8x" else 8.0)
    fp = np.pad(f, ((0, 0), (1, 1), (1, 1), (0, 0)))
    up = np.zeros((n, h8, w8, 64, 2))
    mag = np.zeros((n, h8, w8, 64, 2))
    for k in range(9):
        nb = fp[:, k // 3:k // 3 + h8, k % 3:k % 3 + w8]     # neighbour (py + k / 3 - 1, px + k % 3 - 1), zero outside (unfold's padding)
        up += sm[:, :, :, k, :, None] * nb[:, :, :, None, :]
        mag += sm[:, :, :, k, :, None] * np.abs(nb[:, :, :, None, :])
    full = up.reshape(n, h8, w8, 8, 8, 2).transpose(0, 1, 3, 2, 4, 5).reshape(n, 8 * h8, 8 * w8, 2)
    fmag = mag.reshape(n, h8, w8, 8, 8, 2).transpose(0, 1, 3, 2, 4, 5).reshape(n, 8 * h8, 8 * w8, 2)
    o = 1 if bug == "crop_off_by_one" else 0
    crop = full[:, pad_t + o:pad_t + o + sh, pad_l + o:pad_l + o + sw]
    src = full if bug == "maxd_uncropped" else crop
    maxd = np.sqrt((src ** 2).sum(-1)).reshape(n, -1).max(1)
    return crop, fmag[:, pad_t:pad_t + sh, pad_l:pad_l + sw], maxd


def upsample_tolerance(mag):
    """kernel vs float64: every weight e_k / den carries the fast exp's relative error twice (numerator, denominator) plus the fp32 roundings of
    the subtraction, 9 additions, the division, two products and 9 accumulations (22 2^-24); all relative to sum_k softmax_k |8 f_k|"""
    return (2 * EXPF_REL + 22 * U24) * mag + 2.0 ** -126


def maxd_of(up32: np.ndarray) -> np.ndarray:
    """float32 maximum of sqrt(u u + v v), every operation rounded separately, over an [n, sh, sw, 2] float32 array"""
    u, v = up32[..., 0].astype(np.float32), up32[..., 1].astype(np.float32)
    return np.sqrt(u * u + v * v, dtype=np.float32).reshape(up32.shape[0], -1).max(1)


def upsample_data(seed: int, n: int, h8: int, w8: int, logit_std: float = 3.0, extreme: bool = False):
    g = rng(seed)
    flow = (g.standard_normal((n, h8 * w8, 2)) * 6).astype(np.float32)
    mask = (g.standard_normal((n * h8 * w8, 576)) * logit_std).astype(np.float32)
    if extreme:
        mask = np.where(g.random(mask.shape) < 0.5, 80.0, -80.0).astype(np.float32) + (g.standard_normal(mask.shape) * 0.5).astype(np.float32)
    return flow, mask


def upsample_margin_case(flow, mask, w8: int):
    """a copy of (flow, mask) whose largest displacement sits in the cropped-away margin: the first 1/8 pixel of every image moves by 500 and
    only its own top-left sub-pixel (cropped when pad_l or pad_t > 0) puts weight on it"""
    flow, mask = flow.copy(), mask.copy()
    P = flow.shape[1]
    flow[:, 0] = 500.0
    for n in range(flow.shape[0]):
        for pix, k in ((0, 4), (1, 3), (w8, 1), (w8 + 1, 0)):      # the taps that read pixel 0
            mask[n * P + pix, k * 64:(k + 1) * 64] = -80.0
        mask[n * P, 4 * 64] = 80.0
    return flow, mask


def pad_geometry(h: int, w: int):
    """InputPadder('sintel') as flow_geometry (flow_chunk.h) with factor 8: (pad_l, pad_t, h8, w8)"""
    ph, pw = (((h // 8) + 1) * 8 - h) % 8, (((w // 8) + 1) * 8 - w) % 8
    return pw // 2, ph // 2, (h + ph) // 8, (w + pw) // 8


# =====================================================================================================================
# instance norm + ReLU (+ second operand) (extractor.py: nn.InstanceNorm2d defaults - biased variance, eps 1e-5, no affine)
# =====================================================================================================================
def map_value(x, layout: int, with_lo: bool = True):
    """the value a kernel reads from a host-built map of x: layout 0 fp16(x); 1 hi + fp16(x - hi); 2 hi + e4m3((x - hi) 2^12) 2^-12"""
    x = np.asarray(x, np.float32)
    hi = f16(x)
    if layout == 0 or not with_lo:
        return hi.astype(np.float64)
    if layout == 1:
        return hi.astype(np.float64) + f16(x - hi).astype(np.float64)
    return hi.astype(np.float64) + e4m3_q(x - hi, 12)


def instnorm_truth(a, b=None, normalise_b: bool = False, stats_of=None, bug=None, stats_of_b=None):
    """a (b) [B, HW, C] float64 as the kernel reads them -> (out, mean, rstd, var); stats_of: the values the statistics are taken from when they
    differ from a (hi parts alone); stats_of_b likewise for a normalised b"""
    def st(x):
        ax = (0, 1) if bug == "batch_shared" else 1
        mean = x.mean(ax, keepdims=True)
        var = ((x - mean) ** 2).mean(ax, keepdims=True)
        if bug == "unbiased" and x.shape[1] > 1:
            var = var * x.shape[1] / (x.shape[1] - 1)
        return np.broadcast_to(mean, (x.shape[0], 1, x.shape[2])), np.broadcast_to(var, (x.shape[0], 1, x.shape[2]))
    eps = 1e-6 if bug == "eps" else 1e-5
    a = np.asarray(a, np.float64)
    mean, var = st(a if stats_of is None else np.asarray(stats_of, np.float64))
    rstd = 1 / np.sqrt(var + eps)
    v = np.maximum((a - mean) * rstd, 0)
    if b is not None:
        b = np.asarray(b, np.float64)
        if normalise_b:
            mb, vb = st(b if stats_of_b is None else np.asarray(stats_of_b, np.float64))
            b = (b - mb) / np.sqrt(vb + eps)
        v = v + b
        if bug != "second_relu":
            v = np.maximum(v, 0)
    return v, mean, rstd, var


def instnorm_tolerance(x_stats, a, mean, rstd, var, C: int, out, split_out: bool):
    """in_stats sums x - p and (x - p)^2 in fp32, p = the channel's mean over the image's first 8 pixels: a thread adds
    t = ceil(min(HW, 2048) / npl) pixels (npl = 256 / (C / 8) pixel lanes), a block its npl partial sums, in_finalize the chunks: depth
    d = t + npl + chunks roundings (+ 1 for x - p).  With u = 2^-24 and y = x - p:
      mean = p + E[y]:  |d mean| <= (d + 1) u E|y| + u |mean|
      |d E[y^2]| <= (d + 2) u E[y^2]
      var = E[y^2] - E[y]^2 in fp32: |d var| <= (d + 4) u E[y^2] + 2 |E y| |d E y| <= 3 (d + 4) u E[y^2] = 3 (d + 4) u kappa var,
      kappa = E[y^2] / var = 1 + (mean - p)^2 / var - the cancellation factor of the one-pass formula (without the pivot: 1 + mean^2 / var);
      rstd = rsqrt(var + eps): relative error <= half of |d var| / (var + eps) + 2 u;
      out = (x - mean) rstd: |d out| <= rstd |d mean| + |x - mean| rstd (rel rstd + 2 u), then its storage (fp16: half a step; split: 2^-15).
    -> (tolerance of the map, of the mean, of rstd, kappa)"""
    HW = a.shape[1]
    npl = 256 // (C // 8)
    d = -(-min(HW, 2048) // npl) + npl + -(-HW // 2048) + 1
    xs = np.asarray(x_stats, np.float64)
    y = xs - xs[:, :8].mean(1, keepdims=True)
    e1 = np.abs(y).mean(1, keepdims=True)
    e2 = (y ** 2).mean(1, keepdims=True)
    dmean = (d + 1) * U24 * e1 + U24 * np.abs(mean)
    dvar = 3 * (d + 4) * U24 * e2
    rel = 0.5 * dvar / (var + 1e-5) + 2 * U24
    t = rstd * dmean + np.abs(a - mean) * rstd * (rel + 2 * U24)
    store = (2.0 ** -15 * np.abs(out) + 2.0 ** -22) if split_out else 0.5 * f16_step(np.abs(out) + t)
    return t + store, dmean, rstd * rel, e2 / np.maximum(var, 1e-30)


def instnorm_data(seed: int, B: int, HW: int, C: int, ratio: float, zero_from: int = 0):
    """per-channel mean / std = ratio; channels >= zero_from (if set) all zero"""
    g = rng(seed)
    sd = g.uniform(0.3, 2.0, (1, 1, C))
    sd[0, 0, 1], sd[0, 0, 2] = 0.004, 0.02                  # two low-variance channels: var ~ eps, where eps matters
    x = g.standard_normal((B, HW, C)) * sd + ratio * sd * np.where(g.random((1, 1, C)) < 0.5, -1, 1)
    x = x.astype(np.float32)
    if zero_from:
        x[:, :, zero_from:] = 0
    return x


# =====================================================================================================================
# init_state / put_flow (raft.py:112-115, update.py:97)
# =====================================================================================================================
def state_truth(c):
    """cnet rows [rows, 256] (fp16-representable) -> (tanh(c[:, :128]), relu(c[:, 128:])) float64"""
    c = np.asarray(c, np.float64)
    return np.tanh(c[:, :128]), np.maximum(c[:, 128:], 0)
