"""Device -> host copies of the workspace tensors that the launch tap (mpu_unet_set_launch_tap) reports: raw hipMemcpy of a
device pointer, for the replay tests (tests/test_gpu_replay.py, tests/test_gpu_accumulator_range.py)."""
import ctypes as C

import numpy as np
import torch


def hip():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            return C.CDLL(name)
        except OSError:
            pass
    raise RuntimeError("libamdhip64 not found")


def _copy(hip_, host, dptr, nbytes):
    rc = hip_.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), C.c_size_t(nbytes), C.c_int(2))
    assert rc == 0, rc


def d2h_bf16(hip_, dptr, shape):
    """device bf16 tensor -> float64 numpy (exact)."""
    n = int(np.prod(shape))
    host = np.empty(n, np.uint16)
    _copy(hip_, host, dptr, 2 * n)
    return (host.astype(np.uint32) << 16).view(np.float32).reshape(shape).astype(np.float64)


def d2h_f32(hip_, dptr, shape):
    n = int(np.prod(shape))
    host = np.empty(n, np.float32)
    _copy(hip_, host, dptr, 4 * n)
    return host.reshape(shape).astype(np.float64)


def d2h_u8(hip_, dptr, shape):
    n = int(np.prod(shape))
    host = np.empty(n, np.uint8)
    _copy(hip_, host, dptr, n)
    return host.reshape(shape)


def d2h_rows(hip_, dptr, shape, bf16, lo, hi):
    """Rows [lo, hi) of the leading axis of a device bf16 (bf16=True) or f32 tensor of `shape` -> float64 torch-CPU tensor
    (exact). A batch too large to hold in fp64 as a whole is taken a few images at a time."""
    per = int(np.prod(shape[1:]))
    n = (hi - lo) * per
    esz = 2 if bf16 else 4
    host = np.empty(n, np.int16 if bf16 else np.float32)
    _copy(hip_, host, dptr + lo * per * esz, esz * n)
    t = torch.from_numpy(host)
    return (t.view(torch.bfloat16) if bf16 else t).to(torch.float64).reshape((hi - lo,) + tuple(shape[1:]))
