"""float64 restatement of the on-the-fly correlation lookup (csrc/corr_otf.hip, flow_raft --alternate_corr); a helper module of the tests
beside raft_ref.py, CPU only.

The kernel computes a window entry c_l(r, t) = (1/16) sum_k fmap1[r, k] fpool_l[t, k] from the fp16 feature maps with fp32 accumulation and
blends the fp32 entries: unlike the volume path nothing is rounded to fp16 between the dot product and the final store.  pyramid_otf is
therefore raft_ref.pyramid_restated WITHOUT its last f16(c), and the kernel is held to raft_ref.lookup_restated on those levels plus the one
thing that is not restated - the fp32 accumulation order of the 256 products, blended over the window.  The design stages no entry as fp16,
so raft_ref.volume_tolerance does not appear here."""
from __future__ import annotations

import numpy as np

import raft_ref as R
from split_ref import BUDGET, F16, f16


def pyramid_otf(fmap1, fmap2, rows=None):
    """fmap1 [n, P, 256], fmap2 [n, h8, w8, 256] -> ([levels [R, h_l, w_l] float64], [magnitude levels]): fp16 operands, the target features
    avg-pooled in fp32 and stored as fp16 (avgpool2_nhwc), the dot products in float64, times 1/16 (exact); entries NOT rounded to fp16"""
    n, h8, w8, _ = fmap2.shape
    P = h8 * w8
    rows = np.arange(n * P) if rows is None else np.asarray(rows)
    f1 = f16(fmap1).astype(np.float64).reshape(n * P, 256)[rows]
    pair = rows // P
    feat = f16(fmap2)
    lv, mg = [], []
    for l in range(4):
        if l:
            h, w = feat.shape[1] // 2 * 2, feat.shape[2] // 2 * 2
            t = feat[:, :h, :w]
            feat = f16(np.float32(0.25) * ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])))
        tg = feat.astype(np.float64)
        h, w = tg.shape[1:3]
        c = np.empty((len(rows), h, w))
        m = np.empty_like(c)
        for i in range(n):
            s = pair == i
            c[s] = (f1[s] @ tg[i].reshape(-1, 256).T / 16.0).reshape(-1, h, w)
            m[s] = (np.abs(f1[s]) @ np.abs(tg[i].reshape(-1, 256)).T / 16.0).reshape(-1, h, w)
        lv.append(c)
        mg.append(m)
    return lv, mg


def lookup_otf_restated(levels, mags, flow, P: int, w8: int, rows=None, bug=None):
    """-> (value before the fp16 store [R, 324], tolerance of the kernel against it): raft_ref.lookup_restated on the unrounded levels, plus
    256 2^-24 of the blended sum |f1||f2| / 16 - the 256 products of an entry are accumulated in fp32 in the matrix unit's order, which is
    not restated.  Everything else (half an fp16 step of the result, the coordinate round trip, the 4 blend roundings) is lookup_restated's."""
    r, tol = R.lookup_restated(levels, flow, P, w8, rows, bug)
    return r, tol + 256 * R.U24 * R.lookup_truth(mags, flow, P, w8, rows)


def truth_budget(mags_truth, flow, P: int, w8: int, rows=None):
    """what the fp16 operands (pooled features stored as fp16) may cost against float64 truth: the fp16-operand budget of the blended magnitudes,
    as tests/test_gpu_raft_ops.py::test_lookup_chain"""
    return BUDGET[F16] * R.lookup_truth(mags_truth, flow, P, w8, rows)


def smooth_flow(n: int, h8: int, w8: int) -> np.ndarray:
    """an affine field: coherent 8 x 8 tiles (small bounding boxes) with non-zero, varying fractions -> [n P, 2] float32"""
    P = h8 * w8
    p = np.arange(n * P) % P
    x, y = (p % w8).astype(np.float64), (p // w8).astype(np.float64)
    return np.stack([1.7 + 0.03 * x - 0.02 * y, -2.3 + 0.01 * x + 0.04 * y], 1).astype(np.float32)


def otf_flows(seed: int, n: int, h8: int, w8: int, sub_std: float, border_std: float):
    """raft_ref.lookup_flows' families plus `smooth`"""
    fam = R.lookup_flows(seed, n, h8, w8, sub_std, border_std)
    fam["smooth"] = smooth_flow(n, h8, w8)
    return fam
