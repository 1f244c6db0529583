"""Times surface.distance_transform_edt and surface.surface_distances on one GPU against the host route (device -> host, scipy's
distance_transform_edt twice per class) and writes JSON lines (profiles/surface_times.jsonl was made with it). Dev tool.

  python tools/time_surface.py --out surface_times.jsonl            every case, HIP events, median of --calls after a first call
  python tools/time_surface.py --only blobs_512 --calls 2 --no-host  a short run to put under `rocprofv3 --kernel-trace --stats`

Cases: blob maps (smooth random fields, thresholded; the prediction is the truth's field plus a perturbation) at 256^3 with 3
classes and 512^3 with 5; and hard cases of the line scans at 512^3: one feature voxel in a corner, no feature at all, and the
features in the plane z = 0 (every line holds finite values, large ones far from the plane: the scans exit late everywhere)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiplanarunet_amd import surface as S                      # noqa: E402

SPACING = (0.78125, 0.78125, 1.5)


def blob_maps(n, K, seed):
    """(pred, truth) u8 [n, n, n] on the device: K - 1 foreground classes as bands of a smooth field."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    up = lambda t: torch.nn.functional.interpolate(t, size=(n, n, n), mode="trilinear", align_corners=True)[0, 0]
    field = up(torch.randn(1, 1, 6, 6, 6, device="cuda", generator=g))
    wobble = up(torch.randn(1, 1, 12, 12, 12, device="cuda", generator=g))
    edges = torch.linspace(0.6, 2.2, K, device="cuda")             # class c where edges[c - 1] <= field < edges[c]
    band = lambda f: (torch.bucketize(f.contiguous(), edges, right=True) % K).to(torch.uint8)
    return band(field + 0.08 * wobble), band(field)


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


def host_route(pred, truth, classes, spacing):
    """What a user does today: copy both maps to the host, then per class medpy's hd95 / assd written out with scipy."""
    from scipy import ndimage
    t0 = time.perf_counter()
    p, t = pred.cpu().numpy(), truth.cpu().numpy()
    fp = ndimage.generate_binary_structure(3, 1)
    out = {}
    for c in classes:
        a, b = p == c, t == c
        if not a.any() or not b.any():
            continue
        ba, bb = a ^ ndimage.binary_erosion(a, fp), b ^ ndimage.binary_erosion(b, fp)
        d1 = ndimage.distance_transform_edt(~bb, sampling=spacing)[ba]
        d2 = ndimage.distance_transform_edt(~ba, sampling=spacing)[bb]
        out[c] = (float(np.percentile(np.hstack((d1, d2)), 95)), float((d1.mean() + d2.mean()) / 2))
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_surface.py needs a GPU: nothing is measured without one")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    med = lambda ts: ts[len(ts) // 2]
    for name, n, K, host_classes in (("blobs_256", 256, 3, (1, 2)), ("blobs_512", 512, 5, (1,))):
        if args.only and args.only != name:
            continue
        pred, truth = blob_maps(n, K, seed=n)
        mask = (truth != 0).to(torch.uint8)
        first, ts = timed(lambda: S.distance_transform_edt(mask, SPACING), args.calls)
        rec = {"case": name, "voxels": n ** 3, "n_classes": K, "spacing": SPACING, "histogram": torch.bincount(truth.reshape(-1).int(), minlength=K).tolist(),
               "edt_first_call_ms": first, "edt_ms": med(ts), "edt_all_ms": ts}
        first, ts = timed(lambda: S.surface_distances(pred, truth, K, SPACING, tolerance=1.0), args.calls)
        m = S.surface_distances(pred, truth, K, SPACING, tolerance=1.0)
        rec.update({"surface_first_call_ms": first, "surface_ms": med(ts), "surface_all_ms": ts,
                    "surface_ms_per_class": round(med(ts) / (K - 1), 3),
                    "hd95": [round(float(x), 6) for x in m["hd95"][1:]], "assd": [round(float(x), 6) for x in m["assd"][1:]],
                    "nsd": [round(float(x), 6) for x in m["nsd"][1:]],
                    "n_border": [int(a + b) for a, b in zip(np.nan_to_num(m["n_pred_border"][1:]), np.nan_to_num(m["n_truth_border"][1:]))]})
        if not args.no_host:
            print("# host route of %s ..." % name, flush=True)
            secs, h = host_route(pred, truth, host_classes, SPACING)
            rec.update({"host_route_classes": list(host_classes), "host_route_s": round(secs, 3),
                        "host_route_s_per_class": round(secs / len(host_classes), 3),
                        "host_hd95": [h[c][0] for c in sorted(h)], "host_assd": [h[c][1] for c in sorted(h)],
                        "host_agrees": all(abs(h[c][0] - m["hd95"][c]) <= 1e-9 * max(1.0, h[c][0]) and
                                           abs(h[c][1] - m["assd"][c]) <= 1e-9 * max(1.0, h[c][1]) for c in h)})
        emit(rec)
        del pred, truth, mask
    for name, make in (("corner_512", lambda m: m.__setitem__((511, 511, 511), 0)), ("no_feature_512", lambda m: None),
                       ("plane_z0_512", lambda m: m[:, :, 0].zero_())):
        if args.only and args.only != name:
            continue
        mask = torch.ones((512, 512, 512), dtype=torch.uint8, device="cuda")
        make(mask)
        first, ts = timed(lambda: S.distance_transform_edt(mask, SPACING), args.calls)
        emit({"case": name, "voxels": 512 ** 3, "spacing": SPACING, "edt_first_call_ms": first, "edt_ms": med(ts), "edt_all_ms": ts})
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
