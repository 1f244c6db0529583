"""Times the label-map clean-up of postprocess.py (remove_small_components, fill_holes, open_ball, close_ball) on one GPU beside
keep_largest_component, the 6-view predict+fuse that made the map, and the host route (device -> host, scipy.ndimage per class,
host -> device), and writes JSON lines (profiles/cleanup_times.jsonl was made with it). Dev tool.

  python tools/time_cleanup.py --out cleanup_times.jsonl        both cases, HIP events, median of --calls after a first call
  python tools/time_cleanup.py --only "configs[2]" --no-host

Cases: the fused label maps of bench.py's predict legs, configs[2] (256^3, 3 classes) and configs[4] (512^3, 5 classes), with the
voxel spacing of tools/time_surface.py; opening and closing at radii of 1 and 3 voxel sizes (of the finest axis)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench                                                      # noqa: E402
from multiplanarunet_amd import postprocess as PP                 # noqa: E402
from multiplanarunet_amd.predict import multi_view_predict        # noqa: E402
from time_surface import SPACING, timed                           # noqa: E402


def predicted_map(D, K, C):
    """(label map u8 [D, D, D] of the bench's predict leg, seconds of the second predict+fuse)."""
    vol, views, model, fm = bench._predict_setup(torch.device("cuda", 0), lambda *a, **k: None, D, 6, K, C)
    multi_view_predict(model, vol, views, D, float(D), fm, batch_size=None, want_probs=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, labels = multi_view_predict(model, vol, views, D, float(D), fm, batch_size=None, want_probs=False)
    torch.cuda.synchronize()
    return labels.contiguous(), time.perf_counter() - t0


def ball(radius, spacing):
    """The voxels within `radius` of the origin, as a structuring element (the host's stand-in for the Euclidean ball)."""
    h = [int(radius / s) for s in spacing]
    g = np.meshgrid(*[np.arange(-k, k + 1) * s for k, s in zip(h, spacing)], indexing="ij")
    return (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= radius * radius


def host_route(labels, K, op, classes, **kw):
    """What a user does today: one copy to the host, scipy.ndimage once per class, one copy back. -> seconds."""
    from scipy import ndimage
    t0 = time.perf_counter()
    a = labels.cpu().numpy()
    out = a.copy()
    for c in classes:
        m = a == c
        if op == "small":
            lab, k = ndimage.label(m, structure=ndimage.generate_binary_structure(3, 3))
            out[m & (np.bincount(lab.ravel())[lab] < kw["min_voxels"])] = 0
        elif op == "fill":
            out[ndimage.binary_fill_holes(m) & (a == 0)] = c
        elif op == "open":
            out[m & ~ndimage.binary_opening(m, structure=ball(kw["radius"], SPACING))] = 0
        else:
            out[ndimage.binary_closing(m, structure=ball(kw["radius"], SPACING)) & (out == 0)] = c
    torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cleanup.py needs a GPU: nothing is measured without one")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    med = lambda ts: ts[len(ts) // 2]
    for name, D, K, C, host_classes in (("configs[2]", 256, 3, 1, (1, 2)), ("configs[4]", 512, 5, 2, (2,))):
        if args.only and args.only != name:
            continue
        labels, predict_s = predicted_map(D, K, C)
        base = {"case": name, "voxels": D ** 3, "n_classes": K, "spacing": SPACING, "predict_fuse_s": round(predict_s, 4)}
        emit(dict(base, histogram=torch.bincount(labels.reshape(-1).int(), minlength=K).tolist()))
        r1, r3 = min(SPACING), 3 * min(SPACING)
        ops = [("keep_largest", lambda: PP.keep_largest_component(labels, K, 26, report=True), None, {}),
               ("remove_small_100", lambda: PP.remove_small_components(labels, K, 100, 26, report=True), "small", {"min_voxels": 100}),
               ("fill_holes_6", lambda: PP.fill_holes(labels, K, 6, report=True), "fill", {}),
               ("fill_holes_26", lambda: PP.fill_holes(labels, K, 26, report=True), None, {}),
               ("open_r1", lambda: PP.open_ball(labels, K, r1, SPACING, report=True), "open", {"radius": r1}),
               ("close_r1", lambda: PP.close_ball(labels, K, r1, SPACING, report=True), "close", {"radius": r1}),
               ("open_r3", lambda: PP.open_ball(labels, K, r3, SPACING, report=True), "open", {"radius": r3}),
               ("close_r3", lambda: PP.close_ball(labels, K, r3, SPACING, report=True), "close", {"radius": r3})]
        for op, fn, host_op, kw in ops:
            first, ts = timed(fn, args.calls)
            rec = dict(base, op=op, first_call_ms=first, ms=med(ts), all_ms=ts, report=fn()[1].tolist())
            if op.startswith(("open", "close")):
                rec.update(radius=round(kw["radius"], 6), ms_per_class=round(med(ts) / (K - 1), 3))
            if host_op and not args.no_host and not (D == 512 and op.endswith("_r3")):
                print("# host route of %s %s ..." % (name, op), flush=True)
                rec.update(host_route_classes=list(host_classes), host_route_s=round(host_route(labels, K, host_op, host_classes, **kw), 3))
            emit(rec)
        del labels
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
