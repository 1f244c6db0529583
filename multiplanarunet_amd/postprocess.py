"""
Post-processing of a fused label map on the device (csrc/components.hip): connected components and "keep the largest
connected component per class" (`mp predict --largest_component`), and the label-map clean-up that goes with it: a size threshold on
components (`--min_component_voxels`), hole filling with a face vote (`--fill_holes`) and opening / closing by a Euclidean ball in the
units of the voxel spacing (`--open_mm`, `--close_mm`; csrc/surface.hip: two thresholds of the exact distance transform). The
reference does none of it; the host route it replaces is scipy.ndimage once per class on a copy of the volume.
Integer work and exact comparisons: names, counts, the selections and the outputs are exact, and two calls give identical bytes.
"""
import ctypes as C

import torch

from . import _lib

CONNECTIVITIES = (6, 18, 26)        # scipy.ndimage.generate_binary_structure(3, 1 / 2 / 3)

_scratch = {}                       # (device, stream, bytes) -> the scratch of the last call (one entry)


def _raise(name, status):
    """ValueError (MPU_EINVAL) / NotImplementedError (MPU_EUNSUPPORTED) carrying the library's message."""
    msg = (_lib.load().mpu_last_error() or b"").decode()
    if status == -3:
        raise NotImplementedError(msg)
    if status == -1:
        raise ValueError(msg)
    raise _lib.MpuError("%s failed (%d): %s" % (name, status, msg))


def _shape3(labels):
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3:
        raise ValueError("labels: expected a uint8 tensor [X, Y, Z], got %s %s"
                         % (getattr(labels, "dtype", type(labels)), tuple(getattr(labels, "shape", ()))))
    if labels.device.type != "cuda":
        raise _lib.MpuError("connected components need a HIP device (no CPU path)")
    if not labels.is_contiguous():
        raise ValueError("labels: expected a contiguous (C order) tensor")
    return (C.c_int64 * 3)(*[int(s) for s in labels.shape])


def scratch_bytes(shape):
    """mpu_components_scratch_bytes of a volume shape (X, Y, Z)."""
    lib = _lib.load()
    n = lib.mpu_components_scratch_bytes((C.c_int64 * 3)(*[int(s) for s in shape]))
    if n < 0:
        raise NotImplementedError((lib.mpu_last_error() or b"").decode())
    return int(n)


def _scratch_for(shape3, device, query="mpu_components_scratch_bytes"):
    lib = _lib.load()
    n = getattr(lib, query)(shape3)
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


def class_mask(n_classes, classes=None):
    """Bit c set for every class to filter; None = all of 1 .. n_classes - 1. The library refuses bit 0 and bits >= n_classes."""
    if classes is None:
        classes = range(1, int(n_classes))
    mask = 0
    for c in classes:
        c = int(c)
        if c < 0 or c > 31:
            raise ValueError("class %d cannot be filtered: classes are 1 .. n_classes - 1" % c)
        mask |= 1 << c
    return mask


def connected_components(labels, n_classes, connectivity=26):
    """i32 [X, Y, Z]: the linear C-order index of the first voxel of each voxel's component, -1 where the label is 0 or >= n_classes."""
    shape3 = _shape3(labels)
    lib = _lib.load()
    with torch.cuda.device(labels.device):
        scratch = _scratch_for(shape3, labels.device)
        roots = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
        st = lib.mpu_label_components(_lib.ptr(labels), shape3, int(connectivity), int(n_classes), _lib.ptr(roots), _lib.ptr(scratch),
                                      _lib.stream_ptr())
    if st != 0:
        _raise("mpu_label_components", st)
    return roots


def keep_largest_component(labels, n_classes, connectivity=26, classes=None, out=None, report=False):
    """The label map with, for every class in `classes` (None: all foreground classes), only its largest connected component
    kept and the class's other voxels set to 0; the largest is the one with the smallest first index among equally large ones.
    out: None (a new tensor), `labels` itself (in place) or another u8 tensor of the same shape. report=True: also the
    [n_classes, 3] table (components found, voxels kept, voxels removed) as NumPy -- the one small device-to-host copy."""
    shape3 = _shape3(labels)
    lib = _lib.load()
    mask = class_mask(n_classes, classes)
    if out is None:
        out = torch.empty_like(labels)
    elif out is not labels:
        out = _lib.owned(out, labels.shape, torch.uint8, labels.device, "out")
        if out.device != labels.device:
            raise ValueError("out: expected a tensor on %s" % (labels.device,))
    with torch.cuda.device(labels.device):
        scratch = _scratch_for(shape3, labels.device)
        table = torch.empty((max(int(n_classes), 1), 3), dtype=torch.int64, device=labels.device)
        st = lib.mpu_keep_largest_components(_lib.ptr(labels), shape3, int(connectivity), int(n_classes), mask, _lib.ptr(out),
                                             _lib.ptr(table), _lib.ptr(scratch), _lib.stream_ptr())
    if st != 0:
        _raise("mpu_keep_largest_components", st)
    if report:
        return out, table.cpu().numpy()
    return out


def _filter_call(name, labels, n_classes, classes, out, report, cols, query, args):
    """The shared shape of the clean-up entries: checks, `out`, the scratch of `query`, the [n_classes, cols] report table, the call
    lib.<name>(labels, shape, *args(mask), out, table, scratch, stream)."""
    shape3 = _shape3(labels)
    lib = _lib.load()
    mask = class_mask(n_classes, classes)
    if out is None:
        out = torch.empty_like(labels)
    elif out is not labels:
        out = _lib.owned(out, labels.shape, torch.uint8, labels.device, "out")
        if out.device != labels.device:
            raise ValueError("out: expected a tensor on %s" % (labels.device,))
    with torch.cuda.device(labels.device):
        scratch = _scratch_for(shape3, labels.device, query)
        table = torch.empty((max(int(n_classes), 1), cols), dtype=torch.int64, device=labels.device)
        st = getattr(lib, name)(_lib.ptr(labels), shape3, *args(mask), _lib.ptr(out), _lib.ptr(table), _lib.ptr(scratch),
                                _lib.stream_ptr())
    if st != 0:
        _raise(name, st)
    if report:
        return out, table.cpu().numpy()
    return out


def remove_small_components(labels, n_classes, min_voxels, connectivity=26, classes=None, out=None, report=False):
    """The label map with, for every class in `classes` (None: all foreground classes), every connected component of fewer than
    `min_voxels` voxels set to 0 (min_voxels >= 1; 1 changes nothing). out / report as keep_largest_component; the table is
    [n_classes, 3]: components found, voxels kept, voxels removed."""
    return _filter_call("mpu_remove_small_components", labels, n_classes, classes, out, report, 3, "mpu_components_scratch_bytes",
                        lambda mask: (int(connectivity), int(n_classes), mask, int(min_voxels)))


def fill_holes(labels, n_classes, connectivity=6, classes=None, out=None, report=False):
    """The label map with every cavity filled: a connected component of the background {label == 0} (under `connectivity`; 6 is
    scipy.ndimage.binary_fill_holes' default) that does not reach a face of the volume. A cavity goes whole to the class with the
    most face contacts (a tie: the smallest class) if that class is in `classes` (None: all foreground classes); one that only
    labels >= n_classes border stays. The table is [n_classes, 2]: cavities and voxels given to class c; row 0: left unfilled."""
    return _filter_call("mpu_fill_holes", labels, n_classes, classes, out, report, 2, "mpu_fill_holes_scratch_bytes",
                        lambda mask: (int(connectivity), int(n_classes), mask))


def _ball(op, labels, n_classes, radius, spacing, classes, out, report):
    s = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * 3
    if len(s) != 3:
        raise ValueError("spacing: expected three values (sx, sy, sz), got %d" % len(s))
    sp = (C.c_double * 3)(*s)
    return _filter_call("mpu_morph_ball", labels, n_classes, classes, out, report, 2, "mpu_surface_scratch_bytes",
                        lambda mask: (sp, int(n_classes), mask, op, float(radius)))


def open_ball(labels, n_classes, radius, spacing=(1.0, 1.0, 1.0), classes=None, out=None, report=False):
    """Opening of every class in `classes` (ascending; None: all foreground classes) by a Euclidean ball of `radius`, in the units
    of `spacing`: the voxels of class c farther than radius from the class's erosion become 0 -- thin parts and specks go, nothing
    is added. Exact thresholds of the squared distance transform (surface.edt_squared); the volume's outside is not background.
    The table is [n_classes, 2]: voxels added (0), voxels removed."""
    return _ball(_lib.MPU_MORPH_OPEN, labels, n_classes, radius, spacing, classes, out, report)


def close_ball(labels, n_classes, radius, spacing=(1.0, 1.0, 1.0), classes=None, out=None, report=False):
    """Closing of every class in `classes` (ascending, each on the map the earlier ones left) by a Euclidean ball of `radius`: gaps
    and slits narrower than the ball are given to class c where the label is 0 -- no other class and no label >= n_classes is
    overwritten, nothing is removed. The table is [n_classes, 2]: voxels added, voxels removed (0)."""
    return _ball(_lib.MPU_MORPH_CLOSE, labels, n_classes, radius, spacing, classes, out, report)
