#!/usr/bin/env python
"""
Volume preparation of `mp predict` / `mp train` (data.as_volume: upload, '1pct' background value, RobustScaler), on the host
as before (fit_on="host": np.percentile / np.nanpercentile, then upload) against on the device (fit_on="device": upload, then
csrc/volume_stats.hip), alternating in one process. Random volumes 256^3 x 1 and 512^3 x 2; the median of --repeats runs each;
one JSON line per case. Both paths end with a device synchronisation; the two results are checked to be the same numbers.

  python tools/time_volume_prep.py [--repeats 5] [--cases 256x1,512x2]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="256x1,512x2")
    args = ap.parse_args()
    import numpy as np
    import torch
    from multiplanarunet_amd.data import as_volume
    from multiplanarunet_amd import _lib
    aff = np.eye(4)

    def prep(img, fit_on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vol = as_volume(img, None, aff, "1pct", "RobustScaler", "cuda", "timed", fit_on=fit_on)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, vol

    def upload(img):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = torch.as_tensor(img).to("cuda").contiguous()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del t
        return dt

    as_volume(np.random.RandomState(0).randn(8, 8, 8, 1).astype(np.float32), None, aff, "1pct", "RobustScaler", "cuda")   # warm-up
    for case in args.cases.split(","):
        n, c = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(n + c)
        img = rng.standard_normal((n, n, n, c), dtype=np.float32)
        img *= 50
        img += 100
        prep(img, "device")                                            # first touch of the allocations
        host, dev, up = [], [], []
        same = True
        for _ in range(args.repeats):
            th, vh = prep(img, "host")
            td, vd = prep(img, "device")
            up.append(upload(img))
            host.append(th)
            dev.append(td)
            ch, sh = vh.scaler
            cd, sd = vd.scaler
            same = same and vh.bg_value == vd.bg_value and np.array_equal(ch, cd) and np.array_equal(sh, sd)
            del vh, vd
        med = lambda v: float(np.median(v))
        print(json.dumps({"case": "%d^3 x %d" % (n, c), "bytes": int(img.nbytes), "repeats": args.repeats,
                          "host_s": round(med(host), 4), "device_s": round(med(dev), 4),
                          "upload_only_s": round(med(up), 4), "device_minus_upload_s": round(med(dev) - med(up), 4),
                          "host_over_device": round(med(host) / med(dev), 2),
                          "host_runs_s": [round(v, 4) for v in host], "device_runs_s": [round(v, 4) for v in dev],
                          "same_numbers": bool(same), "device": torch.cuda.get_device_name(0),
                          "build": _lib.build_hash()}), flush=True)


if __name__ == "__main__":
    main()
