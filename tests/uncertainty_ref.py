"""
fp64 NumPy restatement of the per-voxel uncertainty of the fusion (multiplanarunet_amd/uncertainty.py) from an explicit
x[V, ..., K], W, b (test aid; imported like map_linear_cases.py):
  Hn(q) = -sum_k (q_k / s) ln(q_k / s) / ln K, s = sum_k q_k; terms with q_k <= 0 contribute 0, s <= 0 gives 0, K = 1 gives 0
  entropy   = Hn(p), p the fused vector (softmax(sum_v W[v] x_v + b), or sum_v x_v with sum_fusion)
  mi        = max(0, Hn(mean_v x^_v) - mean_v Hn(x^_v)), x^_v = x_v / sum_k x_v[k] (0 when that sum is <= 0)
  agreement = #{v: argmax x_v == fused label}, first maximum
x_v is gathered with oracle.geometry's nearest mapping or with map_linear_cases.oracle_map_linear.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def hn(q):
    """Hn over the last axis, fp64."""
    q = np.asarray(q, np.float64)
    K = q.shape[-1]
    if K == 1:
        return np.zeros(q.shape[:-1])
    s = q.sum(-1, keepdims=True)
    ok = s > 0
    r = np.where(ok, q / np.where(ok, s, 1.0), 0.0)
    pos = (q > 0) & (r > 0)
    t = np.where(pos, r * np.log(np.where(pos, r, 1.0)), 0.0)
    return np.where(ok[..., 0], -t.sum(-1) / np.log(K), 0.0)


def normalised(x):
    x = np.asarray(x, np.float64)
    s = x.sum(-1, keepdims=True)
    return np.where(s > 0, x / np.where(s > 0, s, 1.0), 0.0)


def fused(x, W=None, b=None, sum_fusion=False):
    """p [..., K] fp64 from x [V, ..., K] (the oracle's own fusion, in fp64)."""
    x = np.asarray(x, np.float64)
    if sum_fusion:
        return x.sum(0)
    V, K = x.shape[0], x.shape[-1]
    W = np.asarray(W, np.float64).reshape((V,) + (1,) * (x.ndim - 2) + (K,))
    z = (W * x).sum(0) + np.asarray(b, np.float64).reshape(K)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def entropy(p):
    return hn(p)


def mutual_information(x):
    """x [V, ..., K] -> [...]"""
    xh = normalised(x)
    return np.maximum(0.0, hn(xh.mean(0)) - hn(xh).mean(0))


def agreement(x, labels):
    """x [V, ..., K], labels [...] -> u8 [...]: np.argmax takes the first maximum."""
    return (np.argmax(np.asarray(x), axis=-1) == np.asarray(labels)[None]).sum(0).astype(np.uint8)


def uncertainty(x, W=None, b=None, sum_fusion=False):
    """(entropy, mi, agreement, label) of x [V, ..., K] by the definitions, all in fp64."""
    p = fused(x, W, b, sum_fusion)
    lab = np.argmax(p, axis=-1).astype(np.uint8)
    return entropy(p), mutual_information(x), agreement(x, lab), lab


def gather_views(view_inputs, method):
    """x [V, X, Y, Z, K] f32: what every voxel reads from every view. view_inputs: [(pred [d,d,P,K], grid, inv_basis, voxel_grid)]."""
    from oracle import geometry as G
    import map_linear_cases as MC
    out = []
    for pred, grid, ib, vg in view_inputs:
        out.append(G.map_real_space_pred(pred, grid, ib, vg) if method == "nearest" else MC.oracle_map_linear(pred, grid, ib, vg))
    return np.stack(out).astype(np.float32)


def table(labels, maps, n_classes, truth=None):
    """uncertainty.uncertainty_table in fp64 NumPy."""
    lab = np.asarray(labels).ravel()
    out = {}
    groups = [("", np.ones(lab.shape, bool))]
    if truth is not None:
        t = np.asarray(truth).ravel()
        groups += [("_correct", t == lab), ("_wrong", t != lab)]
    for suffix, sel in groups:
        n = np.bincount(lab[sel], minlength=n_classes)[:n_classes]
        out["n" + suffix] = n.astype(np.int64)
        for name in ("entropy", "mi", "agreement"):
            if name in maps:
                s = np.bincount(lab[sel], weights=np.asarray(maps[name], np.float64).ravel()[sel], minlength=n_classes)[:n_classes]
                with np.errstate(all="ignore"):
                    out["mean_" + name + suffix] = np.where(n > 0, s / np.where(n > 0, n, 1), np.nan)
    return out
