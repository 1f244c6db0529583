"""tools/time_validation.py [out.json]: Validation.evaluate over 50 steps at the configs[1] shape (B 16, 128 x 128, 3 classes, depth 4, bf16): the parent's code path
(a model without the evaluation hook: predict + count) against this change's (the same + loss and metric accumulators),
alternately, device events, warm-up pass first."""
import os, sys, json
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiplanarunet_amd.unet import UNet
from multiplanarunet_amd import validation as V
quiet = lambda *a, **k: None
B, H, K, STEPS = 16, 128, 3, 50
res = {}
for loss in ("SparseCategoricalCrossentropy", "SparseDiceLoss"):
    m = UNet(n_classes=K, dim=H, depth=4, dtype="bf16", logger=quiet, flatten_output=True, seed=1)
    m.compile("Adam", loss, ["sparse_categorical_accuracy", "sparse_fg_recall"])
    rng = np.random.RandomState(0)
    x = torch.tensor(rng.randn(B, H, H, 1).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, K, (B, H * H, 1)).astype(np.uint8), device="cuda")
    class Stub:
        device = m.device
        predict_on_batch = staticmethod(m.predict_on_batch)
    val = V.Validation(lambda: (x, y, None), STEPS, K, logger=quiet, verbose=False)
    def timed(model):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); val.evaluate(model); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for mdl in (Stub(), m, Stub(), m):
        timed(mdl)
    t = {"parent_path": [], "with_batch_wise": []}
    for _ in range(10):
        t["parent_path"].append(timed(Stub())); t["with_batch_wise"].append(timed(m))
    res[loss] = {k: {"ms_per_50_steps_median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                     "us_per_batch_median": float(np.median(v)) * 1000 / STEPS} for k, v in t.items()}
    print(loss, json.dumps(res[loss]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
