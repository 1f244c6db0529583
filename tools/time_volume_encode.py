"""mpu_volume_encode beside mpu_volume_decode of the same shape and type and the float4 copy (mpu_probe_stream_copy) of the same
number of bytes: event-timed, median of 20, one line per shape. Needs an MI355X."""
import os, sys, ctypes as C, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multiplanarunet_amd import _lib
lib = _lib.load(); st = _lib.stream_ptr()
def timed(fn, n=20):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)[len(ts) // 2]
def say(s):
    print(s, flush=True)
for shape, kind in (((256, 256, 256, 1), "u8"), ((256, 256, 256, 3), "f32"), ((512, 512, 512, 5), "f32"), ((255, 255, 255, 1), "u8"), ((255, 255, 255, 3), "f32")):
    n = 1
    for s in shape: n *= s
    image = kind == "f32"
    dt = torch.float32 if image else torch.uint8
    src = torch.randint(0, 200, (n,), device="cuda", dtype=torch.int32).to(dt).reshape(shape)
    dst = torch.empty(n, dtype=dt, device="cuda"); back = torch.empty(n, dtype=dt, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    sh = (C.c_int64 * 4)(*shape)
    width = 4 if image else 1
    moved = 2 * n * width
    te = timed(lambda: _lib.call("mpu_volume_encode", _lib.ptr(src), _lib.MPU_ENCODE_F32 if image else _lib.MPU_ENCODE_U8, sh, 16 if image else 2, _lib.ptr(dst), _lib.ptr(bad), st))
    td = timed(lambda: _lib.call("mpu_volume_decode", _lib.ptr(dst), 16 if image else 2, 0, sh, 0, 1.0, 0.0, 0 if image else 1, _lib.ptr(back), _lib.ptr(bad), st))
    ok = torch.equal(back.view(torch.uint8), src.reshape(-1).view(torch.uint8))
    nf = (n * width // 4) // 4096 * 4096
    if nf:
        tc = timed(lambda: _lib.call("mpu_probe_stream_copy", C.cast(_lib.ptr(back), C.c_void_p), C.cast(_lib.ptr(dst), C.c_void_p), nf, 0, st))
        copy_rate = 8 * nf / tc
    say("%s %s: moved %.1f MB; encode %.1f us = %.2f TB/s; decode %.1f us = %.2f TB/s; float4 copy of the same bytes %.1f us = %.2f TB/s; encode / copy = %.2f; round trip equal %s"
        % (shape, kind, moved / 1e6, te * 1e6, moved / te / 1e12, td * 1e6, moved / td / 1e12, tc * 1e6, copy_rate / 1e12, (moved / te) / copy_rate, ok))
    del src, dst, back
