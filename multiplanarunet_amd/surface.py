"""
Surface-distance evaluation on the device (csrc/surface.hip): an exact Euclidean distance transform with anisotropic voxel spacing
and, per class, the Hausdorff distance (HD), its 95th percentile (HD95), the average symmetric surface distance (ASSD) and the
normalized surface distance (NSD) of a prediction against a truth map -- `mp predict --surface_metrics`. The reference evaluates
Dice only; the host route this replaces is scipy.ndimage.distance_transform_edt twice per class on a copy of each volume.

The squared transform is DEFINED as the all-pairs minimum of fl(fl(wx dx^2) + fl(fl(wy dy^2) + fl(wz dz^2))), w = fl(spacing^2),
and the kernels return exactly that, bit for bit. Surfaces are medpy's: the voxels of a mask with a face neighbour outside it (the
volume's edge counts as outside). HD95 is medpy's hd95: np.percentile(., 95) over both directed distance lists together; the two
order statistics it needs are selected exactly on the device, the root and the interpolation are NumPy's own arithmetic here.
NSD is the VOXEL-BORDER form of the normalized surface Dice (the share of border voxels of either mask within `tolerance` of the
other mask's border), not the surface-element-area form of DeepMind's surface-distance package.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .postprocess import class_mask

EQUAL, NOT_EQUAL, BORDER = _lib.MPU_EDT_EQUAL, _lib.MPU_EDT_NOT_EQUAL, _lib.MPU_EDT_BORDER
TABLE_COLS = 8
KEYS = ("hd", "hd95", "assd", "nsd", "n_pred_border", "n_truth_border")

_scratch = {}                       # (device, stream, bytes) -> the scratch of the last call (one entry)


def _raise(name, status):
    """ValueError (MPU_EINVAL) / NotImplementedError (MPU_EUNSUPPORTED) carrying the library's message."""
    msg = (_lib.load().mpu_last_error() or b"").decode()
    if status == -3:
        raise NotImplementedError(msg)
    if status == -1:
        raise ValueError(msg)
    raise _lib.MpuError("%s failed (%d): %s" % (name, status, msg))


def _shape3(labels, what="labels"):
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3:
        raise ValueError("%s: expected a uint8 tensor [X, Y, Z], got %s %s"
                         % (what, getattr(labels, "dtype", type(labels)), tuple(getattr(labels, "shape", ()))))
    if labels.device.type != "cuda":
        raise _lib.MpuError("the distance transform needs a HIP device (no CPU path)")
    if not labels.is_contiguous():
        raise ValueError("%s: expected a contiguous (C order) tensor" % what)
    return (C.c_int64 * 3)(*[int(s) for s in labels.shape])


def _spacing3(spacing):
    s = [float(v) for v in np.asarray(spacing, dtype=np.float64).reshape(-1)]
    if len(s) != 3:
        raise ValueError("spacing: expected three values (sx, sy, sz), got %d" % len(s))
    return (C.c_double * 3)(*s)


def scratch_bytes(shape):
    """mpu_surface_scratch_bytes of a volume shape (X, Y, Z)."""
    lib = _lib.load()
    n = lib.mpu_surface_scratch_bytes((C.c_int64 * 3)(*[int(s) for s in shape]))
    if n < 0:
        raise NotImplementedError((lib.mpu_last_error() or b"").decode())
    return int(n)


def _scratch_for(shape3, device):
    lib = _lib.load()
    n = lib.mpu_surface_scratch_bytes(shape3)
    if n < 0:
        raise NotImplementedError((lib.mpu_last_error() or b"").decode())
    # (per stream: the buffer is used in stream order, and the allocator hands a freed block back to the stream it was made on)
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream, int(n))
    buf = _scratch.get(key)
    if buf is None:
        _scratch.clear()                                 # one shape at a time: a predict run sees few
        buf = _scratch[key] = torch.empty(int(n), dtype=torch.uint8, device=device)
    return buf


def voxel_sizes(affine):
    """The voxel edge lengths of an affine: the column norms of affine[:3, :3] (nibabel.affines.voxel_sizes)."""
    a = np.asarray(affine, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 3 or a.shape[1] < 3:
        raise ValueError("affine: expected a matrix of at least 3 x 3, got shape %s" % (a.shape,))
    return np.sqrt(np.sum(a[:3, :3] ** 2, axis=0))


def edt_squared(labels, spacing=(1.0, 1.0, 1.0), predicate=EQUAL, value=0, out=None, root=False):
    """f64 [X, Y, Z]: the squared distance (root=True: the distance) of every voxel to the nearest FEATURE voxel of the u8 label
    volume: labels == value (EQUAL), labels != value (NOT_EQUAL) or the border voxels of the mask labels == value (BORDER).
    +inf everywhere when there is no feature voxel. The labels are not changed."""
    shape3 = _shape3(labels)
    sp = _spacing3(spacing)
    lib = _lib.load()
    out = _lib.owned(out, labels.shape, torch.float64, labels.device, "out")
    if out.device != labels.device:
        raise ValueError("out: expected a tensor on %s" % (labels.device,))
    with torch.cuda.device(labels.device):
        scratch = _scratch_for(shape3, labels.device)
        st = lib.mpu_edt_squared(_lib.ptr(labels), shape3, sp, int(predicate), int(value), 1 if root else 0, _lib.ptr(out),
                                 _lib.ptr(scratch), _lib.stream_ptr())
    if st != 0:
        _raise("mpu_edt_squared", st)
    return out


def distance_transform_edt(mask, sampling=(1.0, 1.0, 1.0), squared=False):
    """scipy.ndimage.distance_transform_edt(mask, sampling=...) on the device: the distance of every non-zero voxel of `mask`
    (a u8 or bool tensor [X, Y, Z]) to the nearest zero voxel, 0 on zero voxels; an f64 tensor. squared=True: the squared
    distances (the exact quantity; the root is the device's sqrt of it)."""
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if np.ndim(sampling) == 0:
        sampling = (float(sampling),) * 3
    return edt_squared(mask, sampling, EQUAL, 0, root=not squared)


def percentile95_from_order_statistics(lo, hi, n):
    """np.percentile(a, 95) (linear method) of a sample of n values whose sorted neighbours of the virtual index are lo and hi:
    NumPy's own arithmetic, operation by operation (virtual index (n - 1) q, gamma = its fractional part, NumPy's two-sided lerp)."""
    q = np.true_divide(95, 100)
    vi = (n - 1) * q
    lo, hi = np.float64(lo), np.float64(hi)
    if vi >= n - 1:                                      # both neighbours are the last element
        return lo
    gamma = np.float64(vi - np.floor(vi))
    diff = np.subtract(hi, lo)
    if gamma >= 0.5:
        return np.float64(np.subtract(hi, diff * (1 - gamma)))
    return np.float64(np.add(lo, diff * gamma))


def metrics_from_table(table, n_classes, classes=None):
    """The dict of per-class arrays from the raw [n_classes, 8] table of mpu_surface_table (as NumPy f64 words)."""
    K = int(n_classes)
    raw = np.ascontiguousarray(table, dtype=np.float64).reshape(K, TABLE_COLS)
    ints = raw.view(np.int64)
    out = {k: np.full(K, np.nan, dtype=np.float64) for k in KEYS}
    with np.errstate(all="ignore"):
        for c in (range(1, K) if classes is None else sorted({int(c) for c in classes})):
            n_p, n_t, within = int(ints[c, 0]), int(ints[c, 1]), int(ints[c, 2])
            out["n_pred_border"][c], out["n_truth_border"][c] = n_p, n_t
            if n_p == 0 and n_t == 0:                    # both masks empty: nothing is defined
                continue
            if n_p == 0 or n_t == 0:                     # one mask empty: no distance is defined, no border voxel is matched
                out["nsd"][c] = 0.0
                continue
            out["hd"][c] = np.sqrt(raw[c, 3])
            out["hd95"][c] = percentile95_from_order_statistics(np.sqrt(raw[c, 6]), np.sqrt(raw[c, 7]), n_p + n_t)
            out["assd"][c] = (raw[c, 4] / np.float64(n_p) + raw[c, 5] / np.float64(n_t)) / 2
            out["nsd"][c] = np.float64(within) / np.float64(n_p + n_t)
    return out


def surface_distances(pred, truth, n_classes, spacing, tolerance=1.0, classes=None):
    """Per class c of `classes` (None: all foreground classes 1 .. n_classes - 1) the surface distances between the u8 label maps
    `pred` and `truth` ([X, Y, Z], same shape, same device): a dict of NumPy arrays of length n_classes --
      hd, hd95, assd   medpy's hd / hd95 / assd with voxelspacing = spacing (surfaces: border voxels, see the module text);
      nsd              the share of border voxels of either map within `tolerance` of the other map's border (voxel-border form);
      n_pred_border, n_truth_border   the border voxel counts.
    NaN for class 0 and for classes not asked for. Both masks empty: all four NaN. Exactly one empty: hd, hd95, assd NaN, nsd 0.
    One small device-to-host copy (the table, the selected order statistics in it)."""
    shape3 = _shape3(pred, "pred")
    _shape3(truth, "truth")
    if tuple(pred.shape) != tuple(truth.shape):
        raise ValueError("pred and truth: shapes differ (%s and %s)" % (tuple(pred.shape), tuple(truth.shape)))
    if truth.device != pred.device:
        raise ValueError("truth: expected a tensor on %s" % (pred.device,))
    sp = _spacing3(spacing)
    K = int(n_classes)
    mask = class_mask(K, classes)
    lib = _lib.load()
    with torch.cuda.device(pred.device):
        scratch = _scratch_for(shape3, pred.device)
        table = torch.empty((max(K, 1), TABLE_COLS), dtype=torch.float64, device=pred.device)
        st = lib.mpu_surface_table(_lib.ptr(pred), _lib.ptr(truth), shape3, sp, K, mask, float(tolerance), _lib.ptr(table),
                                   _lib.ptr(scratch), _lib.stream_ptr())
    if st != 0:
        _raise("mpu_surface_table", st)
    return metrics_from_table(table.cpu().numpy(), K, classes)
