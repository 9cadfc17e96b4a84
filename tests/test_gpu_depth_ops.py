"""GPU: the depth bands' own kernels one by one (pb_op_depth_* / pb_op_zoe_*: the launchers of kernels.h and zoe_kernels.h in the modes
DepthEngine calls them) against tests/depth_ref.py - float64 truth with a tolerance derived from the number formats and the operation
counts, bytes where a kernel only moves, selects or re-encodes what it stored.  Everywhere the bytes a kernel does not own (row tails, pad
token rows, guard rows) must still be 0xFF.  A failure names the op, the case and the element.  The checks themselves live in
depth_ref.*_verify; tests/test_depth_ref_cpu.py runs the same checks on the restatements, with and without planted faults.

measured (MI355X; worst error / tolerance per op): see the "measured:" line of every test.
"""
import pytest

import depth_ref as R
from depth_ref import same_u8
from prisma_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    o = engine.Ops(0)
    yield o
    o.close()


def size_id(c):
    return "%dx%d-%dx%d" % (c[0] + c[1])


# ---- LayerNorm ----
@pytest.fixture(scope="module")
def ln_inputs():
    return {D: R.ln_data(D) for D in R.LN_DIMS}


@pytest.mark.parametrize("mode", ["a", "b", "c"])
@pytest.mark.parametrize("D", R.LN_DIMS)
def test_layernorm_engine_modes(ops, ln_inputs, D, mode):
    """launch_layernorm as DepthEngine::vit calls it, B 2 x 19 of 32 tokens: (a) the block norms - rows wider than D with the fp8 copy of
    the MX correction segment behind the fp16 part; (b) / (c) the DPT taps - class token dropped, rows compacted to b (ntok - 1) + t - 1,
    [hi | lo] and [hi | hi8 | lo8].  Value against float64 F.layer_norm at the layout's budget plus the float32 term of the two-pass
    statistics (depth_ref.ln_f32_term; rsqrtf is ASSUMED to be within 2 ulp); the constant row is beta to one rounding, bytes; the fp8
    copies are bytes of the hi the kernel itself stored; pad token rows, row tails and guard rows preset.
    measured: value err / tol <= 0.478 (a), <= 0.012 (b), <= 0.196 (c); every byte check equal."""
    x, g, b = ln_inputs[D]
    m = R.ln_mode(mode, D)
    raw, pa = ops.depth_layernorm(x, g, b, R.LN_NTOK, bool(m["drop_cls"]), m["ldy"], m["lo_off"], m["o8_off"], R.LN_O8_SCALE, bool(m["lo8"]), R.GUARD)
    R.ln_verify("layernorm D %d mode %s" % (D, mode), raw, x, g, b, mode, pa)


# ---- attention ----
@pytest.mark.parametrize("o8", [False, True], ids=["plain", "fp8copy"])
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: c[0])
def test_attention_both_geometries(ops, case, o8):
    """launch_attention with the variant given explicitly - 1: the 8-wave kernel of the benchmark shapes, which no other op test reaches
    (every small shape takes launch_attention's own switch to 4 waves), 2: the 4-wave kernel.  The two raw buffers must be byte-equal (the
    claim in launch_attention's comment); each is compared with float64 softmax(q k^T / 8) v on the pre-rounded operands at
    2^-10 sum p |v| + 2^-11 |o| + 2^-25; pad token rows, row tails, guard rows preset; the fp8 copy is bytes of the stored fp16 x scale.
    measured: the two geometries byte-equal in all 14 cases; value err / tol <= 0.421."""
    q, k, v = R.attn_data(case)
    ldo, o8_off = R.attn_geometry(case[2], o8)
    raws = {}
    for variant, waves in R.ATTN_VARIANTS.items():
        raws[variant] = ops.depth_attention(q, k, v, variant, ldo, o8_off, R.ATTN_O8_SCALE, R.GUARD)
        R.attn_verify("attention %s, %d waves" % (case[0], waves), raws[variant], q, k, v, o8)
    same_u8("attention %s: 8-wave buffer vs 4-wave buffer" % case[0], raws[1], raws[2])


# ---- cls_rows ----
def test_cls_rows(ops):
    """resid[b, 0, :] = cls + pos[0] as float32 bytes (B 3, ntp 16, D 384); every other float of the residual stream stays preset.
    measured: bytes equal."""
    cls, pos = R.cls_data()
    R.cls_verify("cls_rows", ops.depth_cls_rows(cls, pos[0], R.CLS_B, R.CLS_NTP), cls, pos)


# ---- DPT tail ----
@pytest.mark.parametrize("layout", [0, 1, 2], ids=["f16", "split16", "mx3"])
@pytest.mark.parametrize("case", R.DPT_CASES, ids=size_id)
def test_dpt_tail(ops, case, layout):
    """dpt_tail_kernel against the REFERENCE order in float64 (decode z, interpolate(align_corners=True) of 288 channels, nine shifted taps
    with zero padding, + bias, ReLU, 1 x 1, ReLU), absolute tolerance per pixel (depth_ref.dpt_tolerance), border pixels - where the taps
    are switched off per lane - reported apart from the interior.  Pixels are 64 halfs wider than the layout needs.
    measured: border err / tol <= 0.005, interior <= 0.003 (the bound adds magnitudes, the errors do not line up)."""
    z, bias, w2, b2 = R.dpt_data(case, layout)
    OH, OW = case[1]
    raw, pa = ops.depth_dpt_tail(z, bias, w2, b2, OH, OW, layout, R.dpt_ldz(layout))
    if layout == 2 and pa != 0:
        z, bias, w2, b2 = R.dpt_data(case, layout, pa)
        raw, pa = ops.depth_dpt_tail(z, bias, w2, b2, OH, OW, layout, R.dpt_ldz(layout))
    R.dpt_verify("dpt_tail %s layout %d" % (size_id(case), layout), raw, z, bias, w2, b2, OH, OW, layout, pa)


# ---- depth_resize_minmax ----
@pytest.mark.parametrize("case", R.RSZ_CASES, ids=size_id)
def test_depth_resize_minmax(ops, case):
    """out against float64 interpolate(align_corners=False) with the coordinate tolerance; the per-frame min / max (an all-negative frame,
    an all-positive one, one with +0 and -0) bit-equal to those of the kernel's own output; guard preset.  12 x 16 -> 300 x 450 runs the
    grid-stride loop.
    measured: value err / tol <= 0.151; min / max bits equal."""
    x = R.rsz_data(case)
    raw, mm = ops.depth_resize_minmax(x, *case[1])
    R.rsz_verify("depth_resize_minmax " + size_id(case), raw, mm, x, *case[1])


# ---- ZoeDepth head ----
def test_zoe_softplus(ops):
    """5 columns of rows 8 floats wide, the rest preset; 20, the next float, 25, 100 (expf overflows: only the threshold keeps it finite),
    -104 (expf underflows), 0, +-1e-3 against float64 log1p(exp(x)); expf and log1pf are ASSUMED to be within 2 ulp.
    measured: err / tol <= 0.486."""
    buf = R.sp_data()
    R.sp_verify("zoe_softplus", ops.zoe_softplus(buf, R.SP_ROWS, R.SP_COLS), buf)


@pytest.mark.parametrize("ld", R.DOT_LDS)
def test_zoe_dot32_relu(ops, ld):
    """257 rows of 32 channels in rows of ld halfs against the float64 dot product, 33 float32 roundings of the magnitudes.
    measured: err / tol <= 0.041."""
    act, w2, b2 = R.dot_data(ld)
    R.dot_verify("zoe_dot32_relu ld %d" % ld, ops.zoe_dot32_relu(act, ld, w2, b2, R.GUARD), act, w2, b2)


@pytest.mark.parametrize("lds", R.ZOE_LDS, ids=lambda l: "%d-%d-%d" % l)
@pytest.mark.parametrize("pair", R.ZOE_PAIRS, ids=size_id)
def test_zoe_bilerp_add(ops, pair, lds):
    """a + interpolate(src, align_corners=True), 128 channels, row strides 128 / 192: one fp16 rounding of float64 truth plus the
    coordinate term.
    measured: err / tol <= 0.995."""
    a, src = R.ba_data(pair)
    lda, ldsrc, ldo = lds
    R.ba_verify("zoe_bilerp_add %s ld %s" % (size_id(pair), lds), ops.zoe_bilerp_add(a, src, lda, ldsrc, ldo, R.GUARD), a, src, ldo)


@pytest.mark.parametrize("nA", R.AT_NA)
def test_zoe_attractor(ops, nA):
    """nA of 16 columns read (the others NaN), alpha 300, attractor points near centre +- 1 / sqrt(alpha), against the oracle's
    inv_attractor update in float64.
    measured: err / tol <= 0.138."""
    A, bprev = R.at_data(nA)
    H, W = R.AT_PAIR[1]
    R.at_verify("zoe_attractor nA %d" % nA, ops.zoe_attractor(A, nA, bprev, H, W, R.AT_ALPHA), A, nA, bprev, H, W)


@pytest.mark.parametrize("pair", R.ZOE_PAIRS, ids=size_id)
def test_zoe_cat(ops, pair):
    """columns 0 .. 31 the bytes of act, 32 f16(rel), 33 .. 160 the resized embedding (the 8-wide groups one off against the channels),
    161 .. 191 zero bytes.
    measured: copied columns bytes equal; embedding err / tol <= 0.987."""
    act, rel, emb = R.cat_data(pair)
    H, W = pair[1]
    R.cat_verify("zoe_cat " + size_id(pair), ops.zoe_cat(act, R.CAT_LD_ACT, rel, emb, R.CAT_LD_EMB, H, W), act, rel, emb, H, W)


def test_zoe_logbinom_depth(ops):
    """p driven to both clamps, t to both ends, ordinary values; against the oracle's log_binom / softmax expectation in float64.  The
    tolerance is the float32 restatement's own distance from truth plus the effect of 2 ulp (ASSUMED) on every logf / expf / log1pf result,
    carried through the softmax by re-evaluating the restatement (depth_ref.lb_tolerance).
    measured: err / tol <= 0.177."""
    pt, bins = R.lb_data()
    H, W = R.LB_PAIR[1]
    R.lb_verify("zoe_logbinom_depth", ops.zoe_logbinom_depth(pt, bins, H, W, float(R.LB_MIN_T), float(R.LB_MAX_T), R.GUARD), pt, bins, H, W)


@pytest.mark.parametrize("size", R.PIL_OUT, ids=lambda s: "%dx%d" % s)
def test_zoe_pil_resize(ops, size):
    """8 x 12 -> down, up, horizontal only, vertical only, copy: bit-equal to PIL.Image.resize of the same float32 maps and to
    zoe_oracle.pil_resize_f32, the tap tables built by the engine's own pil_coeffs / pil_ksize.
    measured: bits equal."""
    x = R.pil_data()
    R.pil_verify("zoe_pil_resize %dx%d" % size, ops.zoe_pil_resize(x, *size, R.GUARD), x, *size)


# ---- pre-process ----
@pytest.mark.parametrize("case", [(m, s) for m, sizes in R.PREP_CASES.items() for s in sizes], ids=lambda c: "%s-%dx%d" % ((c[0],) + c[1]))
def test_preprocess_both_outputs(ops, case):
    """launch_preprocess as DepthEngine::run_chunk issues it - one launch for both frames (one at 2160 x 3840), the tap tables of
    DepthEngine::prepare (cubic: pb_cubic_taps to pb_depth_net_size; metric: bilinear_ac_taps to 392 x 518) - with BOTH outputs.  chw against
    float64 truth on the reference's own tables at 13 x 2^-24 x (sum |w_y| |w_x| p / 255 + mean) / std, element-wise (13 roundings on the longest
    path, depth_ref.prep_truth); the im2col rows of 640 halfs bit-equal to fp16 of the kernel's own chw; columns 588 .. 639, the rows behind
    n P and the guard rows still 0xFF.  Sizes: every tap clamped (1 x 1, 2 x 3), scale 0 on an axis, the identity table, 4K.
    measured: chw err / tol <= 0.306 (cubic: 4.0 of the 13 roundings), <= 0.224 (metric: 2.9 of 13); every byte check equal."""
    mode, (H, W) = case
    frames = R.prep_data(mode, H, W)
    chw, raw = ops.depth_preprocess(frames, mode == "metric", R.GUARD)
    R.prep_verify("preprocess %s %dx%d" % (mode, H, W), chw, raw, frames, mode)


@pytest.mark.parametrize("mode", list(R.PREP_CASES))
def test_preprocess_saturating_frames(ops, mode):
    """a frame of 0 and a frame of 255, 7 x 13: every output is the constant (p / 255 - mean) / std of its channel within the same bound
    (a tap set's float32 weights sum to 1 only to rounding), the im2col bytes as above.
    measured: err / tol <= 0.216 (cubic), <= 0.219 (metric); bytes equal."""
    frames = R.prep_sat_data()
    _, tol = R.prep_truth(frames, mode)
    ref = ((frames[:, 0, 0].astype("float64") / 255 - R.PREP_MEAN) / R.PREP_STD)[:, :, None, None] + 0 * tol
    chw, raw = ops.depth_preprocess(frames, mode == "metric", R.GUARD)
    R.prep_verify("preprocess %s saturated" % mode, chw, raw, frames, mode, ref=ref, tol=tol)


def test_preprocess_refuses_bad_arguments(ops):
    """a net size that is not the mode's, a mode that does not exist, no frames: PB_ERR_ARG before any launch"""
    import numpy as np
    frames = R.prep_sat_data()
    chw, raw = np.empty((2, 3, 392, 518), np.float32), np.empty((R.prep_raw_rows(2, 392, 518), 1280), np.uint8)
    call = lambda n, mode, nh, nw, guard: ops.lib.pb_op_depth_preprocess(ops.ctx, engine._ptr(frames), n, 7, 13, mode, nh, nw, guard, engine._ptr(chw), engine._ptr(raw))   # noqa: E731
    assert call(2, 1, 392, 518, R.GUARD) == 0
    for bad in ((2, 1, 518, 392, R.GUARD), (2, 0, 392, 518, R.GUARD), (2, 2, 392, 518, R.GUARD), (0, 1, 392, 518, R.GUARD), (2, 1, 392, 518, -1)):
        assert call(*bad) == -1, bad
