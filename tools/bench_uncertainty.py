"""Times mpu_map_fuse_views_uncertainty (all three maps, labels only as the predict asks for them) at the predict shapes against
the plain mpu_map_fuse_views, and the table pass mpu_uncertainty_table; writes JSON lines (profiles/uncertainty_times.jsonl was
made with it). Dev tool.

  python tools/bench_uncertainty.py --out uncertainty_times.jsonl     both shapes, HIP events, median of --calls after a first call
  python tools/bench_uncertainty.py --only 256 --calls 2              a short run to put under `rocprofv3 --kernel-trace --stats`

Shapes: BASELINE.json configs[2] (256^3, 6 views, 3 classes) and configs[4] (512^3, 6 views, 5 classes), random per-view
predictions with rows that sum to 1. Per shape and method:
  plain_exact_ms   mpu_map_fuse_views with the exact search for every lookup (mpu_geometry_set_fast_path(0)): map_fuse_kernel
  unc_exact_ms     the uncertainty call under the same switch: the same kernel form, the same lookups
  plain_fast_ms    mpu_map_fuse_views as the predict runs it: the straight-line kernel and its fix-up list
  unc_ms           the uncertainty call as the predict runs it (closed-form lookups, exact fall-back; no straight-line variant)
  store_ms         9 bytes per voxel written by fill kernels (two f32 maps, one u8 map): what the extra stores cost at the
                   measured store rate
  table_ms         mpu_uncertainty_table on the outputs, without and with a truth map
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiplanarunet_amd import _lib                                                    # noqa: E402
from multiplanarunet_amd.interpolation import Volume, ViewGeometry, map_and_fuse        # noqa: E402
from multiplanarunet_amd.uncertainty import fuse_with_uncertainty, uncertainty_table    # noqa: E402

VIEWS6 = [[0, 0, 1], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0.707], [-0.6, 0.64, 0.48], [0.7, -0.5, 0.5]]


def timed(fn, calls):
    """(first call ms, sorted ms of `calls` more calls) by HIP events."""
    out = []
    for _ in range(calls + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return round(out[0], 3), sorted(round(t, 3) for t in out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", type=int, default=None, help="256 or 512")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--methods", default="nearest,linear")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty.py needs a GPU: nothing is measured without one")
    sink = open(args.out, "a") if args.out else None
    med = lambda ts: ts[len(ts) // 2]
    lib = _lib.load()
    for D, K in ((256, 3), (512, 5)):
        if args.only and args.only != D:
            continue
        rng = np.random.RandomState(0)
        vol = Volume(torch.zeros((D, D, D, 1)), None, np.eye(4), bg_value=[0.0])
        geoms = [ViewGeometry(v, D, float(D), "same+20") for v in np.array(VIEWS6, float)]
        W = torch.tensor(rng.uniform(.5, 1.5, (len(geoms), K)).astype(np.float32), device="cuda")
        b = torch.tensor(rng.uniform(-.1, .1, (K,)).astype(np.float32), device="cuda")
        preds = []
        for g in geoms:
            p = torch.rand((g.n_planes, D, D, K), device="cuda") ** 4
            p /= p.sum(-1, keepdim=True)
            preds.append((p, (g.real_axis, g.real_axis, g.offsets), g.inv_basis, g.device_axes(vol.device)))
        n = D ** 3
        labels = torch.empty((D, D, D), dtype=torch.uint8, device="cuda")
        f32a, f32b = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")

        def stores():
            f32a.fill_(0.5)
            f32b.fill_(0.25)
            labels.fill_(1)

        _, ts = timed(stores, args.calls)
        store_ms = med(ts)
        for method in args.methods.split(","):
            rec = {"shape": "%d^3" % D, "voxels": n, "views": len(geoms), "n_classes": K, "method": method, "calls": args.calls,
                   "extra_store_bytes_per_voxel": 9, "store_ms": store_ms, "store_GBps": round(9 * n / store_ms / 1e6, 1)}
            plain = lambda: map_and_fuse(vol, preds, W, b, want_probs=False, method=method, out_labels=labels)
            unc = lambda: fuse_with_uncertainty(vol, preds, W, b, method=method, out_labels=labels)
            for fast, tag in ((0, "_exact"), (1, "")):
                _lib.check(lib.mpu_geometry_set_fast_path(fast), "mpu_geometry_set_fast_path")
                first, ts = timed(plain, args.calls)
                rec["plain%s_ms" % (tag or "_fast")] = med(ts)
                first, ts = timed(unc, args.calls)
                rec["unc%s_ms" % tag] = med(ts)
                rec["unc%s_all_ms" % tag] = ts
            rec["unc_minus_plain_exact_ms"] = round(rec["unc_exact_ms"] - rec["plain_exact_ms"], 3)
            rec["unc_over_plain_fast"] = round(rec["unc_ms"] / rec["plain_fast_ms"], 3)
            _, lab, maps = unc()
            truth = torch.roll(lab, 3, 2).contiguous()
            for with_truth in (False, True):
                first, ts = timed(lambda: uncertainty_table(lab, maps, K, truth=truth if with_truth else None), args.calls)
                rec["table%s_ms" % ("_truth" if with_truth else "")] = med(ts)
            t = uncertainty_table(lab, maps, K, truth=truth)
            rec.update({"mean_entropy": [round(float(x), 4) for x in t["mean_entropy"]], "mean_mi": [round(float(x), 4) for x in t["mean_mi"]],
                        "mean_agreement": [round(float(x), 3) for x in t["mean_agreement"]]})
            line = json.dumps(rec)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
            del maps, lab, truth
        del preds, labels, f32a, f32b, vol
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
