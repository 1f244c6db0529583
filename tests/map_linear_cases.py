"""
Shared data of the linear back-mapping tests (test_map_linear_host.py, test_gpu_map_linear.py): the cases of
tests/golden/geometry_golden.npz, the stored outputs of the reference's map_real_space_pred(method="linear")
(tests/golden/make_map_linear_golden.py) and the oracle composition the GPU tests compare against.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
AFFS = ("ident", "aniso", "rot")
VIEWS = (0, 1, 5, 6)
KS = (1, 3, 5)
ALL_CASES = [(an, v, K) for an in AFFS for v in VIEWS for K in KS]                       # the 36 g5_pred_* cases
GOLDEN_CASES = [(an, v, 3) for an in AFFS for v in (0, 6)] + [("rot", 6, 1), ("rot", 6, 5)]   # the eight stored ones

_cache = {}


def linear_golden():
    """lin_map_<affine>_<view>_<K> of both golden files."""
    if "golden" not in _cache:
        out = {}
        for name in ("map_linear_golden.npz", "map_linear_golden_rot.npz"):
            with np.load(os.path.join(HERE, "golden", name)) as z:
                out.update({k: z[k] for k in z.files if k.startswith("lin_map_")})
        _cache["golden"] = out
    return _cache["golden"]


def case_inputs(golden, an, v, K):
    """(pred [16,16,36,K], grid, inv_basis, voxel grid [3,32,28,24]) of one committed case."""
    key = "%s_16_%d" % (an, v)
    grid = (golden["g3_g_" + key], golden["g3_g_" + key], golden["g3_off_" + key])
    return golden["g5_pred_%s_%d_%d" % (an, v, K)], grid, golden["g3_invb_" + key], golden["g4_vgrid_" + an]


def oracle_map_linear(pred, grid, inv_basis, voxel_grid, with_oob=False):
    """map_real_space_pred(method="linear") composed from the oracle: the points rotated as G.map_real_space_pred
    rotates them, oracle.geometry.rgi_linear per class with the fill vector [1, 0, ..., 0], cast to float32."""
    from oracle import geometry as G
    K = pred.shape[-1]
    shp = voxel_grid[0].shape
    pts = np.stack([voxel_grid[i].ravel() for i in range(3)], axis=1)
    xi = inv_basis.dot(pts.T).T.T
    out = np.empty((pts.shape[0], K), np.float32)
    for k in range(K):
        out[:, k] = G.rgi_linear(pred[..., k], grid, xi, 1.0 if k == 0 else 0.0)
    out = out.reshape(shp + (K,))
    if with_oob:
        return out, G.rgi_find_indices(xi, grid)[2].reshape(shp)
    return out


def oracle_case(golden, an, v, K):
    """(oracle linear map, out-of-box mask) of one committed case: computed once, shared, never modified."""
    key = ("case", an, v, K)
    if key not in _cache:
        m, oob = oracle_map_linear(*case_inputs(golden, an, v, K), with_oob=True)
        m.setflags(write=False)
        oob.setflags(write=False)
        _cache[key] = (m, oob)
    return _cache[key]


def labels_equal_outside_float_ties(got, ref_labels, ref_scores, band=8e-6):
    """argmax of float scores: identical wherever the reference's top-2 margin exceeds `band` (relative to the largest
    score); returns the number of differing voxels inside the band."""
    srt = np.sort(np.asarray(ref_scores, np.float64), axis=-1)
    margin = srt[..., -1] - srt[..., -2]
    scale = np.maximum(1.0, np.abs(srt[..., -1]))
    diff = np.asarray(got) != np.asarray(ref_labels)
    outside = diff & (margin > band * scale)
    assert not outside.any(), "%d labels differ outside the float tie band (of %d differing)" % (outside.sum(), diff.sum())
    return int(diff.sum())
