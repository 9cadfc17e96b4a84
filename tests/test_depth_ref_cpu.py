"""CPU: the checks of tests/test_gpu_depth_ops.py, run on tests/depth_ref.py's own restatements instead of the kernels' buffers.  A
restatement - float32 indices and weights, values in float64, rounding where the kernel stores - must pass every check (so the tolerances
hold for the arithmetic they were derived for), and with one planted fault it must fail in at least one case of the list (so they see it).
The inputs are shown to meet what the GPU checks rely on: both ReLUs of the DPT tail cut and pass, the clamp cases of the log-binomial
clamp, the attention case meant to leave workgroups without a (batch, head) pair does so by the launcher's own arithmetic."""
import numpy as np
import pytest

import depth_ref as R
from depth_ref import F32


def caught(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


def seen(bug, runs):
    """runs: callables, one per case, each verifying the restatement with the fault planted; at least one must fail"""
    hits = [caught(r) for r in runs]
    assert any(hits), "planted fault '%s' passes every case" % bug
    return hits


# ---- LayerNorm ----
@pytest.fixture(scope="module")
def ln_inputs():
    return {D: R.ln_data(D) for D in R.LN_DIMS}


@pytest.mark.parametrize("mode", ["a", "b", "c"])
@pytest.mark.parametrize("D", R.LN_DIMS)
def test_layernorm_restatement_passes(ln_inputs, D, mode):
    x, g, b = ln_inputs[D]
    R.ln_verify("ln D %d mode %s" % (D, mode), R.ln_restated(x, g, b, mode), x, g, b, mode)


@pytest.mark.parametrize("bug,modes", [("one_pass", "abc"), ("cls_off", "bc"), ("swap", "b"), ("o8_shift", "a")])
def test_layernorm_faults_are_seen(ln_inputs, bug, modes):
    runs = []
    for D in R.LN_DIMS:
        x, g, b = ln_inputs[D]
        for mode in modes:
            runs.append(lambda x=x, g=g, b=b, mode=mode: R.ln_verify("ln", R.ln_restated(x, g, b, mode, bug=bug), x, g, b, mode))
    seen(bug, runs)


def test_layernorm_inputs(ln_inputs):
    """the offset row is one a one-pass float32 variance cannot do; the constant row's float32 mean is exact"""
    for D, (x, g, b) in ln_inputs.items():
        bo, to = R.LN_SPECIAL["offset"]
        row = x[bo, to].astype(np.float64)
        assert row.var() < 2.0 ** -23 * (row ** 2).mean() * 4           # the variance is below the float32 resolution of E[x^2]
        bc, tc = R.LN_SPECIAL["const"]
        assert np.cumsum(x[bc, tc], dtype=F32)[-1] == F32(R.LN_CONST) * D and np.isnan(x[:, R.LN_NTOK:]).all()
        assert (g > 0).any() and (g < 0).any()
        for mode in "ac":                                               # (b is the engine's packed [hi | lo] row: no tail)
            m = R.ln_mode(mode, D)
            used = max(2 * D * (1 if mode == "a" else 2), m["o8_off"] + D if m["o8_off"] else 0)
            assert used < 2 * m["ldy"], "mode %s leaves no row tail" % mode


# ---- attention ----
@pytest.fixture(scope="module")
def attn_inputs():
    return {c[0]: R.attn_data(c) for c in R.ATTN_CASES}


@pytest.mark.parametrize("o8", [False, True])
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: c[0])
def test_attention_restatement_passes(attn_inputs, case, o8):
    """the float32 / fp16 restatement stays inside 2^-10 sum p |v| + 2^-11 |o| + 2^-25"""
    q, k, v = attn_inputs[case[0]]
    R.attn_verify("attention " + case[0], R.attn_restated(q, k, v, o8), q, k, v, o8)


@pytest.mark.parametrize("bug,o8", [("pad_key", False), ("o8_shift", True)])
def test_attention_faults_are_seen(attn_inputs, bug, o8):
    hits = seen(bug, [lambda c=c: R.attn_verify("attention", R.attn_restated(*attn_inputs[c[0]], o8, bug=bug), *attn_inputs[c[0]], o8) for c in R.ATTN_CASES])
    if bug == "pad_key":
        assert hits[0], "N = 1 with 15 unmasked keys must fail"


def test_attention_cases_take_the_paths_they_are_for():
    by = {c[0]: c[1:] for c in R.ATTN_CASES}
    for variant, waves in R.ATTN_VARIANTS.items():
        assert R.attn_dead_workgroups(*by["xcd"], waves) == 7                 # 16 workgroups, 9 (batch, head) pairs
        assert R.attn_dead_workgroups(*by["n17"], waves) == 7                 # a single pair still starts 8 workgroups
        assert R.attn_dead_workgroups(2, 4, 40, waves) == 0
    assert -(-by["n257"][2] // 256) == 2 and by["n257"][2] % 256 == 1         # a second 8-wave query block with one live row
    assert -(-by["n65"][2] // 64) == 2 and by["n65"][2] % 64 == 1             # a second key tile with one live key
    assert -(-by["n1"][2] // 16) * 16 - by["n1"][2] == 15
    # every case is below launch_attention's own switch to the 4-wave geometry: only an explicit variant runs the 8-wave kernel
    assert all(-(-N // 256) * -(-(B * h) // 8) * 8 < 384 for B, h, N in by.values())


def test_attention_spike_forces_a_rescale(attn_inputs):
    """in the spiked case a late key tile outgrows the running reference by more than 2^10: the kernel's rare branch runs"""
    q, k, v = attn_inputs["spike"]
    qs, ks, _ = R.attn_operands(q, k, v)
    s = (qs.astype(np.float64) @ ks.astype(np.float64).transpose(0, 1, 3, 2))[0, 0, 17]
    assert s[270] - s[:64].max() > 10 + np.log2(64)


# ---- cls_rows ----
def test_cls_rows():
    cls, pos = R.cls_data()
    R.cls_verify("cls_rows", R.cls_restated(cls, pos), cls, pos)
    seen("row1", [lambda: R.cls_verify("cls_rows", R.cls_restated(cls, pos, bug="row1"), cls, pos)])


# ---- DPT tail ----
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("case", R.DPT_CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_dpt_tail_restatement_passes(case, layout):
    z, bias, w2, b2 = R.dpt_data(case, layout)
    OH, OW = case[1]
    R.dpt_verify("dpt_tail", R.dpt_restated(z, bias, w2, b2, OH, OW, layout), z, bias, w2, b2, OH, OW, layout)
    assert np.array_equal(R.z_decode(z, layout, 0), z.astype(np.float64)), "the generator's values are not representable in the layout"


@pytest.mark.parametrize("bug", ["border", "align"])
def test_dpt_tail_faults_are_seen(bug):
    runs = []
    for case in R.DPT_CASES:
        z, bias, w2, b2 = R.dpt_data(case, 1)
        OH, OW = case[1]
        runs.append(lambda a=(z, bias, w2, b2, OH, OW, 1): R.dpt_verify("dpt_tail", R.dpt_restated(*a, bug=bug), *a))
    seen(bug, runs)


def test_dpt_tail_border_fault_is_confined_to_the_border():
    """the planted border fault changes border pixels only - what a whole-image relative maximum cannot be relied on to see"""
    case = R.DPT_CASES[0]
    z, bias, w2, b2 = R.dpt_data(case, 1)
    OH, OW = case[1]
    n = R.DPT_B * OH * OW
    good = R.dpt_restated(z, bias, w2, b2, OH, OW, 1)[:n].reshape(R.DPT_B, OH, OW)
    bad = R.dpt_restated(z, bias, w2, b2, OH, OW, 1, bug="border")[:n].reshape(R.DPT_B, OH, OW)
    assert np.array_equal(good[:, 1:-1, 1:-1], bad[:, 1:-1, 1:-1]) and not np.array_equal(good, bad)


def test_dpt_tail_inputs_cut_and_pass_both_relus():
    for case in R.DPT_CASES:
        for layout in (0, 1, 2):
            z, bias, w2, b2 = R.dpt_data(case, layout)
            out, pre, pre2 = R.dpt_truth(z, bias, w2, b2, *case[1], layout)
            assert (pre > 0).any() and (pre < 0).any(), case
            assert (bias > 0).any() and (bias < 0).any() and (w2 > 0).any() and (w2 < 0).any()
        if case[1] != (1, 1):
            assert (pre2 > 0).any() and (pre2 < 0).any(), case
    assert all(R.dpt_ldz(l) > (320, 640, 640)[l] for l in (0, 1, 2))


# ---- depth_resize_minmax ----
@pytest.mark.parametrize("case", R.RSZ_CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_resize_minmax_restatement_passes(case):
    x = R.rsz_data(case)
    raw, mm = R.rsz_restated(x, *case[1])
    R.rsz_verify("resize_minmax", raw, mm, x, *case[1])
    out = raw[:x.shape[0] * case[1][0] * case[1][1]].reshape(x.shape[0], -1)
    assert (out[0] < 0).all() and (out[1] > 0).all()
    if case[0][0] > 2:
        assert (out[2] == 0).any() and np.signbit(out[2][out[2] == 0]).any() and not np.signbit(out[2][out[2] == 0]).all()


@pytest.mark.parametrize("bug", ["align", "neg_swap"])
def test_resize_minmax_faults_are_seen(bug):
    runs = []
    for case in R.RSZ_CASES[:3]:
        x = R.rsz_data(case)
        runs.append(lambda x=x, case=case: R.rsz_verify("resize_minmax", *R.rsz_restated(x, *case[1], bug=bug), x, *case[1]))
    seen(bug, runs)


def test_ordered_encoding_round_trips():
    v = np.asarray([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], F32)
    o = R.ordered(v)
    assert (np.diff(o.astype(np.int64)) > 0).all()
    assert np.array_equal(R.unordered(o).view(np.uint32), v.view(np.uint32))


# ---- ZoeDepth head ----
def test_softplus():
    buf = R.sp_data()
    R.sp_verify("softplus", R.sp_restated(buf), buf)
    seen("no_threshold", [lambda: R.sp_verify("softplus", R.sp_restated(buf, bug="no_threshold"), buf)])
    x = buf[:R.SP_ROWS, :R.SP_COLS]
    assert np.exp(F32(-104)) == 0 and (x == 20).any() and (x == np.nextafter(F32(20), F32(30))).any() and (x == 0).any()


@pytest.mark.parametrize("ld", R.DOT_LDS)
def test_dot32_relu(ld):
    act, w2, b2 = R.dot_data(ld)
    R.dot_verify("dot32_relu", R.dot_restated(act, w2, b2), act, w2, b2)
    seen("no_relu", [lambda: R.dot_verify("dot32_relu", R.dot_restated(act, w2, b2, bug="no_relu"), act, w2, b2)])


@pytest.mark.parametrize("pair", R.ZOE_PAIRS, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_bilerp_add_and_cat_restatements_pass(pair):
    a, src = R.ba_data(pair)
    for _, _, ldo in R.ZOE_LDS:
        R.ba_verify("bilerp_add", R.ba_restated(a, src, ldo), a, src, ldo)
    act, rel, emb = R.cat_data(pair)
    R.cat_verify("zoe_cat", R.cat_restated(act, rel, emb, *pair[1]), act, rel, emb, *pair[1])


def test_bilerp_add_and_cat_faults_are_seen():
    seen("align", [lambda p=p: R.ba_verify("bilerp_add", R.ba_restated(*R.ba_data(p), 128, bug="align"), *R.ba_data(p), 128) for p in R.ZOE_PAIRS])
    seen("shift", [lambda p=p: R.cat_verify("zoe_cat", R.cat_restated(*R.cat_data(p), *p[1], bug="shift"), *R.cat_data(p), *p[1]) for p in R.ZOE_PAIRS])


@pytest.mark.parametrize("nA", R.AT_NA)
def test_attractor(nA):
    A, bprev = R.at_data(nA)
    H, W = R.AT_PAIR[1]
    R.at_verify("attractor", R.at_restated(A, nA, bprev, H, W), A, nA, bprev, H, W)
    if nA > 1:
        seen("sum", [lambda: R.at_verify("attractor", R.at_restated(A, nA, bprev, H, W, bug="sum"), A, nA, bprev, H, W)])
    seen("align", [lambda: R.at_verify("attractor", R.at_restated(A, nA, bprev, H, W, bug="align"), A, nA, bprev, H, W)])
    b = R.resize_truth(bprev, H, W, True).reshape(-1, 64)
    dx = np.abs(A[:, :nA].astype(np.float64)[:, :, None] - b[:, None, :]) * np.sqrt(R.AT_ALPHA)
    assert ((dx > 0.9) & (dx < 1.1)).any(), "no |dx| near 1 / sqrt(alpha)"


def test_logbinom_depth():
    pt, bins = R.lb_data()
    H, W = R.LB_PAIR[1]
    R.lb_verify("logbinom", R.lb_raw(R.lb_restated(pt, bins, H, W)), pt, bins, H, W)
    seen("k_swap", [lambda: R.lb_verify("logbinom", R.lb_raw(R.lb_restated(pt, bins, H, W, bug="k_swap")), pt, bins, H, W)])
    # the clamp cases clamp: p beyond [1e-4, 1 - 1e-4] on both sides, t at both ends of [0.0212, 50]
    _, p, t = R.lb_truth(pt, bins, H, W)
    assert (p < 1e-4).any() and (1 - p < 1e-4).any()
    assert (t < 0.0212 * 1.01).any() and (t > 50 * 0.9999).any()          # (the 1e-4 added to both softplus values keeps t off the exact ends)
    # the float32 facts the restatement reproduces
    assert F32(63) + F32(1e-7) == F32(63) and F32(2) + F32(1e-7) == F32(2) and F32(1) + F32(1e-7) != F32(1)
    tol = R.lb_tolerance(pt, bins, H, W)
    ref, _, _ = R.lb_truth(pt, bins, H, W)
    assert np.median(tol / ref) < 1e-3, "the tolerance is no check"


@pytest.mark.parametrize("size", R.PIL_OUT, ids=lambda s: "%dx%d" % s)
def test_pil_resize_restatement_is_pillow(size):
    x = R.pil_data()
    R.pil_verify("pil_resize", R.pil_restated(x, *size), x, *size)


def test_pil_resize_fault_is_seen():
    x = R.pil_data()
    seen("end", [lambda s=s: R.pil_verify("pil_resize", R.pil_restated(x, *s, bug="end"), x, *s) for s in R.PIL_OUT])


# ---- pre-process ----
PREP_ALL = [(m, s) for m, sizes in R.PREP_CASES.items() for s in sizes]
prep_id = lambda c: "%s-%dx%d" % ((c[0],) + c[1])          # noqa: E731


@pytest.mark.parametrize("case", [c for c in PREP_ALL if c[1][0] * c[1][1] <= 1080 * 1920], ids=prep_id)
def test_preprocess_truth_is_the_oracles(case):
    """the float64 truth against the band oracles' own pre-process (depth_oracle: float64 values; zoe_oracle: torch float32, which also
    shows the float32 align_corners index rule to be torch's), within the bound the kernel gets.
    measured: <= 1.0 of the 13 roundings (cubic), <= 2.5 (metric)"""
    from oracle import depth_oracle as O
    mode, (H, W) = case
    frames = R.prep_data(mode, H, W)
    ref, tol = R.prep_truth(frames, mode)
    theirs = np.stack([O.preprocess(f) if mode == "cubic" else R.Z.preprocess(f.copy())[0] for f in frames])
    R.check("preprocess truth vs oracle %s %dx%d" % (mode, H, W), theirs, ref, tol)


@pytest.mark.parametrize("case", PREP_ALL, ids=prep_id)
def test_preprocess_restatement_passes(case):
    """plain float32 in the kernel's order stays inside 13 x 2^-24 x magnitude.  measured: <= 4.4 of the 13 over every size"""
    mode, (H, W) = case
    frames = R.prep_data(mode, H, W)
    assert frames.shape[0] == (1 if (H, W) == (2160, 3840) else 2) and (frames.shape[0] == 1 or not np.array_equal(frames[0], frames[1]))
    R.prep_verify("preprocess %s %dx%d" % (mode, H, W), *R.prep_restated(frames, mode), frames, mode)


@pytest.mark.parametrize("mode", list(R.PREP_CASES))
def test_preprocess_saturating_frames_are_constants(mode):
    """all 0, then all 255: (p / 255 - mean) / std per channel - the float32 weights of a tap set sum to 1 only to rounding, which the
    bound covers"""
    frames = R.prep_sat_data()
    _, tol = R.prep_truth(frames, mode)
    ref = np.broadcast_to(((frames[:, 0, 0].astype(np.float64) / 255 - R.PREP_MEAN) / R.PREP_STD)[:, :, None, None], tol.shape)
    R.prep_verify("preprocess %s saturated" % mode, *R.prep_restated(frames, mode), frames, mode, ref=ref, tol=tol)


@pytest.mark.parametrize("mode,bug", [(m, b) for m, bugs in R.PREP_BUGS.items() for b in bugs])
def test_preprocess_faults_are_seen(mode, bug):
    sizes = [s for s in R.PREP_CASES[mode] if s[0] * s[1] <= 360 * 640]

    def run(s):
        frames = R.prep_data(mode, *s)
        return lambda: R.prep_verify("preprocess", *R.prep_restated(frames, mode, bug=bug), frames, mode)
    hits = dict(zip(sizes, seen(bug, [run(s) for s in sizes])))
    if bug == "coord64":
        # the float64 coordinate is the float32 one at 392 x 518 (scale 1) and wherever the scale and its products are exact; it must be
        # seen from 360 x 640 on
        assert hits[(360, 640)] and not hits[(392, 518)]
        frames = R.prep_data(mode, 1080, 1920)
        assert caught(lambda: R.prep_verify("preprocess", *R.prep_restated(frames, mode, bug=bug), frames, mode))
    elif bug == "align":
        assert not hits[(392, 518)] and all(h for s, h in hits.items() if s not in ((392, 518), (1, 1)))
    elif bug in ("bgr", "norm_rot"):
        assert all(hits.values())
    else:       # a one-pixel frame is a constant image: no resize or index fault can show
        assert all(h for s, h in hits.items() if s != (1, 1))
