"""Host arithmetic of the U-Net driver (no GPU): the workspace plan, the parameter / packed-operand sizes and the
gradient-ready points over a sweep of networks, against numbers recorded before the driver's layer table replaced the
per-consumer index arithmetic. The workspace size depends on every level, concat and bf16x3 decision of the plan."""
import ctypes as C
import json
import os

import numpy as np

from multiplanarunet_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_workspace_plan.json")
DTYPES = (("f32", _lib.MPU_F32), ("bf16", _lib.MPU_BF16), ("bf16x3", _lib.MPU_F32X3))
# (classes, loss): 9..16 classes are inference-only, so the per-image loss (Dice) goes with 3 classes
HEADS = ((3, "ce"), (12, "ce"), (3, "dice"))


def plan_records():
    lib = _lib.load()
    rec = {}
    for depth in range(1, 7):
        for dname, dtype in DTYPES:
            for cf in (0.25, 1):
                for K, loss in HEADS:
                    cfg = _lib.UNetConfig()
                    cfg.n_classes, cfg.n_channels, cfg.depth, cfg.H, cfg.W = K, 1, depth, 64, 64
                    cfg.dtype, cfg.softmax = dtype, 1
                    for l in range(depth + 1):
                        cfg.filters[l] = int(64 * (2 ** l) * np.sqrt(cf))        # as multiplanarunet_amd.unet.UNet derives them
                    h = C.c_void_p(lib.mpu_unet_create(C.byref(cfg)))
                    assert h, lib.mpu_last_error()
                    try:
                        if loss == "dice":
                            lc = _lib.LossConfig()
                            lc.kind, lc.smooth = _lib.MPU_LOSS_DICE, 1.0
                            _lib.call("mpu_unet_set_loss", h, C.byref(lc))
                        buf = (C.c_int64 * 32)()
                        n = lib.mpu_unet_grad_ready_points(h, buf, 32)
                        for B in (1, 3):
                            rec["d%d %s cf%g K%d %s B%d" % (depth, dname, cf, K, loss, B)] = {
                                "workspace_bytes": int(lib.mpu_unet_workspace_bytes(h, B)),
                                "probs_offset": int(lib.mpu_unet_workspace_probs_offset(h, B)),
                                "loss_mean_offset": int(lib.mpu_unet_workspace_loss_mean_offset(h, B)),
                                "param_floats": int(lib.mpu_unet_param_floats(h)),
                                "packed_bytes": int(lib.mpu_unet_packed_bytes(h)),
                                "grad_ready_points": [int(buf[i]) for i in range(n)],
                            }
                    finally:
                        lib.mpu_unet_destroy(h)
    return rec


def test_workspace_plan_sizes_and_ready_points_are_those_recorded():
    """Exact integer equality with tests/golden/unet_workspace_plan.json: depth 1..6, f32 / bf16 / bf16x3, batch 1 and 3, 64 x 64,
    complexity factor 0.25 and 1, 3 and 12 classes with the sparse cross-entropy and 3 classes with the Dice loss. The file was
    recorded, from the repository root, at the last commit whose driver derived levels and inputs from the conv index:

        import json, sys; sys.path.insert(0, "tests")
        from test_unet_plan_host import plan_records, GOLDEN
        json.dump(plan_records(), open(GOLDEN, "w"), indent=0, sort_keys=True)
    """
    want = json.load(open(GOLDEN))
    got = plan_records()
    assert len(want) == 6 * 3 * 2 * 3 * 2 and sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], k
