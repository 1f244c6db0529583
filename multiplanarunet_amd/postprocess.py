"""
Post-processing of a fused label map on the device (csrc/components.hip): connected components and "keep the largest
connected component per class" -- the one post-processing step this build has (`mp predict --largest_component`). The
reference does none; the host route it replaces is scipy.ndimage.label once per class on a copy of the volume.
Integer work: names, counts, the selection and the output are exact, and two calls give identical bytes.
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


def _scratch_for(shape3, device):
    lib = _lib.load()
    n = lib.mpu_components_scratch_bytes(shape3)
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
