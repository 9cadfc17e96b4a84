"""CPU: the float64 restatements of the local matching and the local-window propagation (tests/gm_local_ref.py) against the REAL reference's
vectors (tests/golden/gmflow_local_*.npz, tools/make_gmflow_local_golden.py), and the derived tolerance against every planted fault."""
import os

import numpy as np
import pytest

import gm_local_ref as L
from oracle import gmflow_oracle as G
from prisma_amd import synth


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def ops(golden_dir):
    return np.load(os.path.join(golden_dir, "gmflow_local_ops.npz"))


def test_restatements_equal_the_reference_functions(ops):
    """plain gathers, masking for the matching, counted zero pads for the propagation: fp32 round-off of the reference (<= 1e-5 of range;
    its grid_sample puts <= 2^-22 of a neighbour into every sample)"""
    print()
    for h8, w8, R, r in ops["cases"]:
        tag = "%dx%d_R%d_r%d" % (h8, w8, R, r)
        m = L.local_match_restated(ops["tok_" + tag], h8, w8, 1, R)["o"]
        q, k = L.prop_qk(ops["feat_" + tag], ops["q_proj.weight"], ops["q_proj.bias"], ops["k_proj.weight"], ops["k_proj.bias"])
        p = L.local_prop_restated(q, k, ops["flow_" + tag], h8, w8, r)["o"]
        em, ep = relmax(m, ops["match_" + tag]), relmax(p, ops["prop_" + tag])
        print("  %-14s match %.2e prop %.2e of range" % (tag, em, ep))
        assert em <= 1e-5 and ep <= 1e-5, tag


def worst(t, truth, radius):
    return float((np.abs(t["o"] - truth["o"]) / L.local_tolerance(truth, radius)).max())


@pytest.mark.parametrize("bug", ["dxdy", "no_mask", "dir_swap", "no_scale"])
def test_tolerance_sees_planted_matching_faults(bug):
    h8, w8, R = 6, 10, 4
    tok = L.match_tokens(11, 2, h8, w8)
    truth = L.local_match_restated(tok, h8, w8, 2, R)
    assert worst(L.local_match_restated(tok, h8, w8, 2, R, bug=bug), truth, R) > 100, bug


@pytest.mark.parametrize("bug", ["drop_pads", "dxdy", "no_scale"])
def test_tolerance_sees_planted_propagation_faults(bug):
    h8, w8, r = 6, 10, 1
    q, k, flow = L.prop_data(12, 2, h8, w8, 2)
    truth = L.local_prop_restated(q, k, flow, h8, w8, r)
    assert worst(L.local_prop_restated(q, k, flow, h8, w8, r, bug=bug), truth, r) > 100, bug


def test_tolerance_sees_the_global_forms_key(ops):
    """the local form projects the key from the feature (transformer.py:389); the global form's k_proj(q_proj(feature)) (:363-364) carried
    over is a fault the tolerance sees"""
    h8, w8, R, r = ops["cases"][1]
    tag = "%dx%d_R%d_r%d" % (h8, w8, R, r)
    wts = [ops[n] for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias")]
    q, k = L.prop_qk(ops["feat_" + tag], *wts)
    truth = L.local_prop_restated(q, k, ops["flow_" + tag], h8, w8, r)
    qb, kb = L.prop_qk(ops["feat_" + tag], *wts, bug="key_of_q")
    assert worst(L.local_prop_restated(qb, kb, ops["flow_" + tag], h8, w8, r), truth, r) > 100
    assert relmax(L.local_prop_restated(qb, kb, ops["flow_" + tag], h8, w8, r)["o"], ops["prop_" + tag]) > 1e-3


def test_a_float32_evaluation_stays_inside_the_tolerance():
    """the kernels' arithmetic in numpy float32 (one rounding per operation, sums in another order) is inside the derived bound"""
    h8, w8 = 6, 10
    tok = L.match_tokens(13, 1, h8, w8)
    truth = L.local_match_restated(tok, h8, w8, 2, 4)
    kw, valid = L._gather(tok[[1, 0]], h8, w8, 4)
    s = np.einsum("bpc,bpjc->bpj", tok, kw).astype(np.float32) * np.float32(128 ** -0.5)
    s = np.where(valid[None], s, np.float32(-1e9))
    p = np.exp(s - s.max(-1, keepdims=True), dtype=np.float32)
    dx, dy = L.window(4)
    o = np.stack([(p * dx.astype(np.float32)).sum(-1, dtype=np.float32), (p * dy.astype(np.float32)).sum(-1, dtype=np.float32)], -1) \
        / p.sum(-1, dtype=np.float32)[..., None]
    assert float((np.abs(o - truth["o"]) / L.local_tolerance(truth, 4)).max()) <= 1


@pytest.mark.parametrize("name", L.SIZES)
def test_end_to_end_vectors_from_the_oracle_stages_and_the_restatements(golden_dir, name):
    """oracle/gmflow_oracle.py's backbone, transformer and upsampler around the restatements reproduce the real GMFlow's local
    configurations to the 2e-4 the other GMFlow goldens are pinned to; the backward direction is the swapped pair"""
    z = np.load(os.path.join(golden_dir, name))
    h, w = [int(v) for v in z["hw"]]
    fr = synth.frame_pair_sequence(2, h, w, seed=int(z["frame_seed"]))
    import torch
    import torch.nn.functional as F
    wts = synth.gmflow_weights(seed=2468)
    pad = G.pad_amounts(h, w)
    pa, pc = (F.pad(torch.from_numpy(f).permute(2, 0, 1).float()[None], pad, mode="replicate").numpy() for f in fr)
    print()
    for cfg, corr, prop in L.CONFIGS:
        bidir = ("bwd_" + cfg) in z.files
        up, st = L.gmflow_local_forward(wts, pa, pc, corr, prop, bidir=bidir)
        up = up[..., pad[2]:up.shape[-2] - pad[3], pad[0]:up.shape[-1] - pad[1]].transpose(0, 2, 3, 1)
        errs = [relmax(up[0], z["fwd_" + cfg]), relmax(st["flow_match"][:1], z["flow_match_" + cfg]), relmax(st["flow_prop"][:1], z["flow_prop_" + cfg])]
        if bidir:
            errs.append(relmax(up[1], z["bwd_" + cfg]))
        print("  %s %-5s fwd %.2e match %.2e prop %.2e%s" % (name, cfg, errs[0], errs[1], errs[2], " bwd %.2e" % errs[3] if bidir else ""))
        assert max(errs) < 2e-4, (cfg, errs)
