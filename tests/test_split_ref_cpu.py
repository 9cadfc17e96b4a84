"""CPU: the exact restatement of the split-precision layouts (tests/split_ref.py) against float64 truth, and proof that the GPU tests'
kernel-vs-restatement tolerance sees the bugs it exists for."""
import numpy as np
import pytest
import torch

import split_ref as R

SHAPES = {  # conv: x NHWC, w; dense: x, w
    "conv": ((2, 9, 11, 128), (96, 128, 3, 3)),
    "dense": ((300, 256), (128, 256)),
}


@pytest.mark.parametrize("cancel", [False, True], ids=["plain", "cancel"])
@pytest.mark.parametrize("kind", ["conv", "dense"])
@pytest.mark.parametrize("layout", ["f16", "split16", "split16_sa0", "mx3", "mx2"])
def test_restatement_within_budget(layout, kind, cancel):
    sa = 0 if layout.endswith("sa0") else 1
    lay = R.LAYOUTS[layout.replace("_sa0", "")]
    xs, ws = SHAPES[kind]
    x, w, _ = R.case_data(7, xs, ws, cancel=cancel)
    conv = kind == "conv"
    acc, _ = R.restate(lay, x, w, 0, R.weight_pw(w, lay == R.MX3), sa=sa, conv=conv)
    t, mag = R.truth(lay, x, w, conv=conv, sa=sa)
    err = float((np.abs(acc - t) / mag).max())
    # measured: f16 2^-12.7 .. -14.3, split16 2^-22.8 .. -23.5, mx3 2^-17.8 .. -19.0, mx2 2^-18.2 .. -19.6 (cancel / plain, conv / dense);
    # the worst-case budget sits above every figure, and no more than 2^6 above it (a budget that loose would hide a lost segment)
    assert R.BUDGET[lay] / 64 <= err <= R.BUDGET[lay], (layout, np.log2(err))
    if lay != R.F16:       # ... and the correction segments are doing their work: an fp16-only product is far outside the budget
        acc16, _ = R.restate(R.F16, R.truth_input(lay, x, sa), w, 0, 0, conv=conv)
        assert float((np.abs(acc16 - t) / mag).max()) > 16 * err


def test_e4m3_clamps_like_the_device_encoder():
    # torch's cast of 465 / 500 gives 0x7F (NaN in e4m3fn); the encoders clamp to 448 (0x7E) first
    assert torch.tensor([500.0]).to(torch.float8_e4m3fn).view(torch.uint8).item() & 0x7F == 0x7F
    assert list(R.e4m3_bytes([465.0, 500.0, -1e6, 448.0])) == [0x7E, 0x7E, 0xFE, 0x7E]
    assert list(R.e4m3_bytes([0.0, 2.0 ** -9, 2.0 ** -6, 1.0, 1.0625, 1.125 + 2 ** -10])) == [0x00, 0x01, 0x08, 0x38, 0x38, 0x39]
    v = np.float32([0.3, -7.7, 2.0 ** -8, 300.0])
    assert np.all(np.abs(R.e4m3_decode(R.e4m3_bytes(v)) - v) <= R.e4m3_step(v) / 2)


def test_weight_pw_rule():
    g = np.random.default_rng(3)
    w = (g.standard_normal((64, 64)) * 0.05).astype(np.float32)
    lo = float(np.abs(w - R.f16(w)).max())
    assert R.weight_pw(w, False) == 8 - int(np.frexp(np.float32(lo))[1])
    scaled = np.abs(np.ldexp(w - R.f16(w), R.weight_pw(w, False)))
    assert 128 <= scaled.max() < 256                    # the largest residual lands in [2^7, 2^8), below e4m3's 448
    wide = w.copy()
    wide[0, 0] = 3000.0            # mx3: w_hi 2^(pw - 12) must stay below 448: the 20 - e(max |w|) cap binds
    assert R.weight_pw(wide, True) == 20 - 12 < R.weight_pw(wide, False)
    assert R.weight_pw(np.zeros((8, 8), np.float32), True) == 0


@pytest.mark.parametrize("case", R.SENS_CASES, ids=[c[0] for c in R.SENS_CASES])
def test_tolerance_sees_the_bugs(case):
    """on the GPU tests' own data: a dropped correction segment, an E8M0 scale off by 2 and lo8 read without its 2^12 each move some output
    element by at least 4x the kernel-vs-restatement tolerance of a split output"""
    name, lay, xs, ws, stride, seed, cancel = case
    x, w, b = R.case_data(seed, xs, ws, cancel=cancel)
    pw = R.weight_pw(w, lay == R.MX3)
    acc, mag = R.restate(lay, x, w, 0, pw, stride=stride)
    v = R.epilogue(acc, b)
    tol = R.tolerance(mag, v, R.n_products(lay, int(np.prod(ws[1:]))), True, bias=b)
    for pname, seg, fac in R.perturbations(lay):
        pacc, _ = R.restate(lay, x, w, 0, pw, stride=stride, perturb=(seg, fac))
        margin = float((np.abs(R.epilogue(pacc, b) - v) / tol).max())
        assert margin >= 4, (name, pname, margin)
