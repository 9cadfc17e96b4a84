"""CPU: tests/flow_io_ref.py itself, and the host side of the flow bands' --scale.
* the restatements of the prep, resize-back, encode and mask kernels equal the oracle (raft_oracle) and pass the checks the GPU tests run;
* every planted fault is seen by those checks on at least one of the chosen cases - the cases are sensitive before a GPU is involved;
* the float32 restatement of torch's align_corners coordinates is held against F.interpolate;
* no direct-mode value lies within its tolerance of an fp16 tie; the inference-size cases' tie share is under its cap;
* pb_flow_out_size and the engines' tap builder (host functions of the built library) equal scaled_size / cubic_taps_u8 of the oracle, which
  computes with Python's double as the reference does, for dyadic and non-dyadic scales;
* atan2_rn, rounded to float32, is the correctly rounded long-double arctan2 on the adversarial encode cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_io_ref as R
from oracle import raft_oracle as O

F32 = np.float32
PA = 0                     # any e4m3 storage scale serves the restatement; the GPU tests take the engine's


def caught(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


def prep_runs():
    """every (case, norm, layout, isz, dark frames) the GPU tests launch"""
    for c in R.PREP_CASES:
        for norm, layout in R.prep_modes(c[3]):
            yield c[0], c[1], c[2], c[3], norm, layout, None, False
    for (H, W, s, isz), dark in [(c, True) for c in R.PREP_ISZ_CASES] + [(R.PREP_ISZ_FULL, False)]:
        for norm, layout in R.prep_modes(16):
            yield H, W, s, 16, norm, layout, isz, dark


def prep_check(run, bug=None):
    H, W, s, factor, norm, layout, isz, dark = run
    fr = R.prep_frames(H, W, dark)
    geo, raw, sc, sg = R.prep_restated(fr, s, factor, layout, norm, PA, isz, bug)
    return R.prep_verify("%s norm %d layout %d bug %s" % (R.case_id((H, W, s, isz or factor)), norm, layout, bug), fr, s, factor, layout, norm, PA,
                         geo, raw, sc, sg, isz)


def test_restated_tables_and_frames_equal_the_oracle():
    for H, W, s, _ in R.PREP_CASES:
        if s == 1.0:
            continue
        sh, sw = O.scaled_size(H, W, s)
        for src, dst in ((H, sh), (W, sw)):
            gi, gc = R.taps_u8(src, dst, s)
            wi, wc = O.cubic_taps_u8(src, dst, s)
            assert np.array_equal(gi, wi) and np.array_equal(gc, wc), (H, W, s)
        fr = R.prep_frames(H, W)
        got = R.scaled_restated(fr, s)
        assert np.array_equal(got, R.scaled_oracle(fr, s)), (H, W, s)
        if min(sh, sw) >= 8:
            assert got[1].min() == 0 and got[1].max() == 255           # the checker frame reaches both clamps


def test_prep_restatement_passes_every_check():
    worst = {}
    for run in prep_runs():
        for k, v in prep_check(run).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\n  prep restatement: worst err / tol %s" % worst)
    assert worst["lo"] > 0.05 and worst["lo8"] > 0.05          # the bounds are of the errors' order, not far above them


@pytest.mark.parametrize("bug", R.PREP_BUGS)
def test_every_planted_prep_fault_is_seen(bug):
    seen = [run for run in prep_runs() if caught(lambda: prep_check(run, bug))]
    print("\n  %s: seen in %d of %d launches" % (bug, len(seen), len(list(prep_runs()))))
    assert seen, bug
    if bug == "scale_f32":
        # Of the chosen cases only 15 x 35 at 0.3 sees it: the widened float gives 5 x 11 where the reference gives 4 x 10.  At 40 x 60 x 0.6
        # the widened float's tap rows differ in 5 of 24 and 7 of 36 rows, but there only in how they name one pixel - (index s,
        # coefficients 0 2048 0 0) against (index s - 1, coefficients 0 0 2048 0) - so THAT case's bytes are the same.  At larger sizes
        # the 0.6 rows differ in coefficients (1514 of the table test's 2352 rows weigh a source pixel differently) and so do the pixels:
        # 273 of 202410 bytes of these frames at 216 x 288, 2.7 % of the bytes of a 720 x 1280 noise frame, each by one level - the widened
        # scale fed the networks other pixels at real clip sizes
        assert {r[2] for r in seen} == {0.3}
        fr = R.prep_frames(40, 60)
        assert np.array_equal(R.scaled_restated(fr, 0.6), R.scaled_restated(fr, 0.6, "scale_f32"))
        assert not np.array_equal(O.cubic_taps_u8(40, 24, 0.6)[0], O.cubic_taps_u8(40, 24, float(F32(0.6)))[0])
        big = R.prep_frames(216, 288)
        exact, widened = R.scaled_restated(big, 0.6), R.scaled_restated(big, 0.6, "scale_f32")
        assert exact.shape == widened.shape == (3, 130, 173, 3) and np.array_equal(exact, R.scaled_oracle(big, 0.6))
        diff = int((exact != widened).sum())
        print("  216 x 288 x 0.6: %d of %d bytes differ with the widened scale" % (diff, exact.size))
        assert diff > 100


def test_direct_mode_values_are_clear_of_fp16_ties():
    """a direct-mode element is one of 256 integers per channel: none of the normalised values lies within its float32 tolerance of an fp16
    rounding tie, so the kernel's hi must be the fp16 of the truth, bit for bit"""
    for norm in (0, 1):
        t, tol = R.direct_values(norm)
        d = R.f16_tie_distance(t)
        print("\n  norm %d: closest tie %.3g tolerances away" % (norm, (d / tol).min()))
        assert (d > tol).all(), (norm, np.argwhere(d <= tol))


def tie_share(H, W, s, isz, dark) -> float:
    _, _, t, tol = R.prep_truth(R.prep_frames(H, W, dark), s, 16, 1, isz)
    return float(((t - tol).astype(np.float16) != (t + tol).astype(np.float16)).mean())


def test_inference_size_tie_share_is_under_its_cap():
    for H, W, s, isz in R.PREP_ISZ_CASES:
        share = tie_share(H, W, s, isz, True)
        print("\n  %s: %.2e of the elements straddle an fp16 tie" % (R.case_id((H, W, s, isz)), share))
        assert share < 1e-3
    # the full-range repeat is outside the cap by construction (flow_io_ref.prep_frames): reported, and held to the arithmetic that predicts
    # it - at most 2 tol / (fp16 spacing) per element, which for mid greys (|t| < 1/4, spacing <= 2^-13, tol about 6e-7) reaches 1e-2
    share = tie_share(*R.PREP_ISZ_FULL, False)
    print("\n  %s, full range: %.2e" % (R.case_id(R.PREP_ISZ_FULL), share))
    assert 1e-3 < share < 3e-2


def test_align_corners_restatement_against_torch():
    """the float32 coordinates of ac_coords with a float64 blend against F.interpolate(bilinear, align_corners=True) in float32: within the
    4 roundings of a float32 blend - the bound the kernels are held to"""
    for H, W, s, isz in R.PREP_ISZ_CASES:
        sc = R.scaled_oracle(R.prep_frames(H, W, True), s).astype(np.float64)
        want = F.interpolate(torch.from_numpy(sc.astype(F32)).permute(0, 3, 1, 2), size=isz, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
        got = R._blend64(sc, *isz)
        assert (np.abs(got - want) <= 4 * R.U24 * got * R.SLACK).all(), (H, W, isz)
    for (ih, iw), (sh, sw) in R.BACK_CASES:
        fl = R.back_data(ih, iw)
        want = F.interpolate(torch.from_numpy(fl).permute(0, 3, 1, 2), size=(sh, sw), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
        got, mag = R._blend64(fl.astype(np.float64), sh, sw), R._blend64(fl.astype(np.float64), sh, sw, absolute=True)
        assert (np.abs(got - want) <= 4 * R.U24 * mag * R.SLACK + 2.0 ** -149).all(), (ih, iw, sh, sw)


def test_resize_back_restatement_and_its_faults():
    worst = 0.0
    seen = {b: 0 for b in R.BACK_BUGS}
    for (ih, iw), (sh, sw) in R.BACK_CASES:
        fl = R.back_data(ih, iw)
        what = "%dx%d->%dx%d" % (ih, iw, sh, sw)
        worst = max(worst, R.back_verify(what, fl, sh, sw, *R.back_restated(fl, sh, sw))["value"])
        small = R.back_data(ih, iw, 0.01)
        assert (R.back_restated(small, sh, sw)[2] < R.back_restated(fl, sh, sw)[2]).all()       # the second call of the GPU test: smaller maxima
        for b in R.BACK_BUGS:
            seen[b] += caught(lambda: R.back_verify(what + " " + b, fl, sh, sw, *R.back_restated(fl, sh, sw, b)))
    print("\n  resize-back restatement: worst err / tol %.3f; faults seen in %s of %d cases" % (worst, seen, len(R.BACK_CASES)))
    assert worst > 0.05 and all(seen.values()), seen
    assert seen["ratio_swap"] == len(R.BACK_CASES) - 1          # every case but the identity
    assert seen["coord_fma"] >= 2                               # wherever a coordinate's product rounds up to an integer


SCALES = [0.75, 0.5, 0.6, 0.3, 0.7, 0.9, 0.35, 1.5]
TAP_SRC = [157, 181, 720, 1080, 1280, 1920, 3840]


def test_out_size_and_tap_tables_equal_the_oracle_for_every_scale():
    """the C ABI carries --scale as a float; the reference (and the oracle) computes with Python's double.  Sizes for heights 1 .. 4399 and
    tap rows over seven source lengths, eight scales - five of which are not the double of their float"""
    from prisma_amd import engine
    for s in SCALES:
        bad = [h for h in range(1, 4400) if engine.flow_out_size(h, h, s) != O.scaled_size(h, h, s)]
        assert not bad, "scale %g: %d heights with another scaled size, first %s" % (s, len(bad), bad[:5])
        rows = diff = 0
        for src in TAP_SRC:
            dst = O.scaled_size(src, src, s)[0]
            gi, gc = engine.flow_taps(src, dst, s)
            wi, wc = O.cubic_taps_u8(src, dst, s)
            rows += dst
            diff += int(((gi != wi) | (gc != wc)).any(1).sum())
        assert diff == 0, "scale %g: %d of %d tap rows with another index or coefficient" % (s, diff, rows)
    for H, W, s, factor in R.PREP_CASES:
        assert engine.flow_geometry(H, W, s, factor) == R.prep_geometry(H, W, s, factor), (H, W, s, factor)


def test_encode_cases_hold_what_they_claim():
    cases = R.encode_cases()
    adv = cases["adversarial"]
    rgb, mx = R.encode_truth(adv)
    assert mx[0] == 4.0 and mx[1] == 0.5 and mx[2] == 0.0 and np.signbit(adv[2]).any() and not np.signbit(adv[2]).all()
    assert (rgb[2] == 0).all()                                   # 0 / 0: NaN colours cast to 0, as the kernel writes them
    dx, dy = (adv[0, ..., 0] / mx[0]).astype(np.float64), (adv[0, ..., 1] / mx[0]).astype(np.float64)
    with np.errstate(all="ignore"):
        t = np.minimum(np.abs(dx), np.abs(dy)) / np.maximum(np.abs(dx), np.abs(dy))
    for c in (0.125, 0.375, 0.625, 0.875):                       # at, just below and just above every switch of k = floor(4 t + 0.5)
        for r in R._ulp_triple(c):
            assert (t == float(r)).sum() >= 8, (c, r)
    k = np.floor(4 * t[np.isfinite(t)] + 0.5)
    assert set(k.astype(int)) == {0, 1, 2, 3, 4}
    fin = np.abs(adv[0][np.abs(adv[0]) > 0])
    assert (fin < 1.1754944e-38).any()                           # denormals
    assert cases["1x1"].shape == (3, 1, 1, 2) and cases["random"].shape[1] * cases["random"].shape[2] > 1024 * 256
    assert len(set(R.encode_truth(cases["random"])[1].tolist())) == 3


def test_atan2_rn_is_correctly_rounded_on_the_encode_cases():
    for name, fl in R.encode_cases().items():
        _, mx = R.encode_truth(fl)
        for f, m in zip(fl, mx):
            if m == 0:
                continue
            dx, dy = f[..., 0] / F32(m), f[..., 1] / F32(m)
            got = O.atan2_rn(dy, dx).astype(F32)
            want = np.arctan2(dy.astype(np.longdouble), dx.astype(np.longdouble)).astype(F32)
            bad = got.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), (name, dx[bad][:4], dy[bad][:4], got[bad][:4], want[bad][:4])


def test_mask_cases_hold_what_they_claim():
    cases = R.mask_cases()
    q = R.mask_quantised(cases["ties"])[:, 0]                    # the forward flows; the backward ones close the round trip
    tie = np.abs(q - np.floor(q) - 0.5) == 0
    assert tie.all()                                             # every coordinate of the case is a half-even tie ...
    half_away = np.floor(q + 0.5)
    assert (np.rint(q) != half_away).mean() > 0.3                # ... that round-half-up would send elsewhere
    assert (q[..., 0] < 0).any() and (q[..., 1] < 0).any() and (q[..., 0] > 37 * 32).any()
    for name, axes in (("neg_x", [0]), ("neg_y", [1]), ("neg_xy", [0, 1])):
        qn = np.rint(R.mask_quantised(cases[name])[:, 0][..., axes]).astype(np.int64)
        assert (qn < 0).all() and (qn >= -48).all() and (qn & 31 != 0).mean() > 0.9 and (qn < -32).any(), name
    assert cases["h1"].shape[2] == 1 and cases["w1"].shape[3] == 1 and cases["neg_x"].shape[3] == 1 and cases["neg_y"].shape[2] == 1
    flips = {}
    for name, fl in cases.items():
        m = R.mask_truth(fl)
        assert m.shape == fl.shape[:4] and np.array_equal(R.mask_restated(fl), m), name
        assert 0.05 < m.mean() < 0.95, (name, m.mean())         # both outcomes occur
        flips[name] = {b: int((R.mask_restated(fl, b) != m).sum()) for b in R.MASK_BUGS}
    print("\n  mask bits flipped by the planted faults: %s" % flips)
    # a truncating division for >> 5 and |q| & 31 for q & 31 each flip more than a fifth of the forward bits of the negative cases; half-up
    # rounding is what the ties case sees
    for name in ("neg_x", "neg_y", "neg_xy"):
        fwd_bits = cases[name].shape[0] * cases[name].shape[2] * cases[name].shape[3]
        assert flips[name]["trunc_div"] > fwd_bits // 6 and flips[name]["abs_and"] > fwd_bits // 6, (name, flips[name], fwd_bits)
    assert flips["ties"]["half_up"] > 20
