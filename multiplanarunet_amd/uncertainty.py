"""
Per-voxel uncertainty of the multi-view fusion (no reference counterpart: mpunet/bin/predict.py writes the argmax or the fused
probabilities). At every voxel the fused back-mapping holds the K-vector x_v of each of the V views; from them and the fused
vector p (interpolation.map_and_fuse's), with Hn(q) = -sum_k (q_k/s) ln(q_k/s) / ln K, s = sum_k q_k (terms with q_k <= 0
contribute 0, s <= 0 gives 0, K = 1 gives 0):
  entropy   f32 [X,Y,Z]  Hn(p): where the fused distribution is flat
  mi        f32 [X,Y,Z]  max(0, Hn(mean_v x^_v) - mean_v Hn(x^_v)), x^_v = x_v / sum_k x_v[k]: the ensemble's mutual information,
                         0 when all views say the same, large when confident views contradict each other
  agreement u8  [X,Y,Z]  the number of views whose own argmax (first maximum) is the fused label
All of it in one pass of csrc/geometry.hip: map_fuse_uncertainty_kernel (mpu_map_fuse_views_uncertainty), the exact fused
kernel with two more accumulators; `combined[V,X,Y,Z,K]` is not materialised. uncertainty_table sums the maps per class of a
label map (mpu_uncertainty_table, integer sums: the same bytes call after call).
"""
import ctypes as C
import numpy as np
import torch

from . import _lib
from .interpolation import _ViewPredHolder, _map_entry

MAPS = ("entropy", "mi", "agreement")
_DTYPES = {"entropy": torch.float32, "mi": torch.float32, "agreement": torch.uint8}
TABLE_GROUPS = ("", "_correct", "_wrong")                 # d_table [K][3][4]: all, truth == class, truth != class
TABLE_COLS = ("n", "entropy", "mi", "agreement")          # count and the three sums


def check_maps(maps):
    """The map names asked for, in the order of MAPS. ValueError on an unknown name or none at all."""
    maps = (maps,) if isinstance(maps, str) else tuple(maps)
    for m in maps:
        if m not in MAPS:
            raise ValueError("unknown uncertainty map %r (known: %s)" % (m, ", ".join(MAPS)))
    if not maps:
        raise ValueError("no uncertainty map asked for (known: %s)" % ", ".join(MAPS))
    return tuple(m for m in MAPS if m in maps)


def fuse_with_uncertainty(volume, view_preds, W=None, b=None, sum_fusion=False, method="nearest", want_probs=False,
                          maps=MAPS, out_probs=None, out_labels=None):
    """
    interpolation.map_and_fuse (same arguments, same probabilities and labels byte for byte) that also returns the uncertainty
    maps named in `maps`: (merged f32 [X,Y,Z,K] or None, merged_map u8 [X,Y,Z], {name: tensor [X,Y,Z]}).
    """
    maps = check_maps(maps)
    linear = _map_entry(method, 0, 1)
    dev = volume.device
    holders = [_ViewPredHolder(vp[0], vp[1], vp[2], dev, vp[3] if len(vp) > 3 else None) for vp in view_preds]
    V = len(holders)
    K = int(holders[0].pred.shape[-1])
    arr = (_lib.ViewPred * V)(*[h.struct for h in holders])
    X, Y, Z = (int(v) for v in volume.image.shape[:3])
    probs = _lib.owned(out_probs, (X, Y, Z, K), torch.float32, dev, "out_probs") if want_probs else None
    labels = _lib.owned(out_labels, (X, Y, Z), torch.uint8, dev, "out_labels")
    out = {m: torch.empty((X, Y, Z), dtype=_DTYPES[m], device=dev) for m in maps}
    Wd = bd = None
    if not sum_fusion:
        Wd = torch.as_tensor(W, dtype=torch.float32).to(dev).reshape(V, K).contiguous()
        bd = torch.as_tensor(b, dtype=torch.float32).to(dev).reshape(K).contiguous()
    vg = volume.voxel_grid()
    _lib.call("mpu_map_fuse_views_uncertainty", C.byref(vg), arr, V, K, _lib.ptr(Wd), _lib.ptr(bd),
              1 if sum_fusion else 0, linear, _lib.ptr(probs), _lib.ptr(labels),
              _lib.ptr(out.get("entropy")), _lib.ptr(out.get("mi")), _lib.ptr(out.get("agreement")), _lib.stream_ptr())
    return probs, labels, out


def means_from_table(table, n_classes, with_truth):
    """The dict of per-class arrays from the raw f64 [K][3][4] table of mpu_uncertainty_table: n, mean_entropy, mean_mi,
    mean_agreement, and with a truth map their _correct / _wrong variants. A class (or group) without voxels gives NaN."""
    K = int(n_classes)
    raw = np.ascontiguousarray(table, dtype=np.float64).reshape(K, len(TABLE_GROUPS), len(TABLE_COLS))
    out = {}
    with np.errstate(all="ignore"):
        for g, suffix in enumerate(TABLE_GROUPS if with_truth else TABLE_GROUPS[:1]):
            n = raw[:, g, 0]
            out["n" + suffix] = n.astype(np.int64)
            for j, col in enumerate(TABLE_COLS[1:], 1):
                out["mean_" + col + suffix] = np.where(n > 0, raw[:, g, j] / np.where(n > 0, n, 1.0), np.nan)
    return out


def uncertainty_table(labels, maps, n_classes, truth=None):
    """Per class c of the u8 label map `labels` the voxel count `n` and mean_entropy, mean_mi, mean_agreement of the maps over the
    voxels labelled c (NumPy arrays of length n_classes; a map missing from `maps` gives NaN); with a u8 `truth` map of the same
    shape also n_correct, mean_*_correct (voxels with truth == c) and n_wrong, mean_*_wrong. A class with no voxels gives NaN.
    One pass on the device, one small copy to the host."""
    K = int(n_classes)
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8:
        raise ValueError("labels: expected a uint8 tensor, got %s" % (getattr(labels, "dtype", type(labels)),))
    dev, n = labels.device, labels.numel()
    labels = labels.contiguous()
    given = {}
    for name in check_maps(tuple(maps)):
        t = maps[name]
        if not torch.is_tensor(t) or t.dtype != _DTYPES[name] or t.numel() != n or t.device != dev:
            raise ValueError("maps[%r]: expected a %s tensor of %d elements on %s" % (name, _DTYPES[name], n, dev))
        given[name] = t.contiguous()
    if truth is not None:
        if not torch.is_tensor(truth) or truth.dtype != torch.uint8 or truth.numel() != n or truth.device != dev:
            raise ValueError("truth: expected a uint8 tensor of %d elements on %s" % (n, dev))
        truth = truth.contiguous()
    lib = _lib.load()
    nbytes = int(lib.mpu_uncertainty_table_scratch_bytes(n, K))
    with torch.cuda.device(dev):
        table = torch.empty((max(K, 1), len(TABLE_GROUPS), len(TABLE_COLS)), dtype=torch.float64, device=dev)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
        _lib.call("mpu_uncertainty_table", _lib.ptr(labels), _lib.ptr(truth), _lib.ptr(given.get("entropy")),
                  _lib.ptr(given.get("mi")), _lib.ptr(given.get("agreement")), n, K, _lib.ptr(table), _lib.ptr(scratch),
                  _lib.stream_ptr())
    out = means_from_table(table.cpu().numpy(), K, truth is not None)
    for name in MAPS:
        if name not in given:
            for k in [k for k in out if k.startswith("mean_" + name)]:
                out[k] = np.full(K, np.nan)
    return out
