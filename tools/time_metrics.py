#!/usr/bin/env python
"""
What the training metrics (`fit.metrics`, csrc/train_metrics.hip) cost per train step at BASELINE.json configs[1] (B = 16,
128 x 128 x 1, depth 4, 64 filters, bf16), by the method of bench.py's timed train leg: the whole step replayed from one HIP graph on
bench.py's batch, W warm-up steps, then R rounds of K timed steps between two HIP events. Two models live in the process -- one
compiled without metrics, one with --metrics -- and the rounds ALTERNATE between their graphs, so that the difference is taken
between windows a few hundred milliseconds apart. One JSON line per call.

  python tools/time_metrics.py [--metrics sparse_categorical_accuracy] [--steps 100 --warmup 20 --rounds 5]
  python tools/time_metrics.py --root /path/to/another/checkout --plain-only --tag parent     # a build without metrics (A/B)
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--metrics", default="sparse_categorical_accuracy", help="comma-separated fit.metrics names")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--root", default="")
    ap.add_argument("--plain-only", action="store_true", help="a build without metrics: time the plain leg alone")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.abspath(args.root or here))
    import torch
    from multiplanarunet_amd.unet import UNet
    quiet = lambda *a, **k: None
    B, dim = args.batch, args.dim
    g = torch.Generator(device="cpu").manual_seed(1234)                 # bench.py's batch
    x = torch.randn(B, dim, dim, 1, generator=g).cuda()
    xs = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 5, 1, 2)[:, 0]
    y = ((xs > 0.1).to(torch.uint8) + (xs > 0.45).to(torch.uint8)).reshape(B, dim * dim, 1).contiguous()
    sw = torch.ones(B, device="cuda")
    names = [n for n in args.metrics.split(",") if n]
    legs = {"plain": None} if args.plain_only else {"plain": None, "metrics": names}
    models, runs = {}, {}
    for leg, metrics in legs.items():
        m = UNet(n_classes=3, dim=dim, n_channels=1, depth=4, complexity_factor=1.0, flatten_output=True, dtype=args.dtype,
                 logger=quiet, seed=0)
        m.compile("Adam", "SparseCategoricalCrossentropy", metrics)
        models[leg], runs[leg] = m, m.make_graphed_train_step(x, y, sw)
    for run in runs.values():
        for _ in range(max(1, args.warmup)):
            run()
    torch.cuda.synchronize()
    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms[leg].append(round(e0.elapsed_time(e1) / args.steps, 4))
    out = {"tag": args.tag, "batch": B, "dim": dim, "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": ms["plain"], "last_logged_loss": float(models["plain"].loss_mean().item())}
    if "metrics" in legs:
        med = lambda v: sorted(v)[len(v) // 2]
        m = models["metrics"]
        out.update(metrics=names, ms_per_step_metrics=ms["metrics"],
                   paired_delta_us=[round((b - a) * 1e3, 2) for a, b in zip(ms["plain"], ms["metrics"])],
                   median_delta_us=round((med(ms["metrics"]) - med(ms["plain"])) * 1e3, 2),
                   bytes_read_per_step=B * dim * dim * (4 * 3 + 1), metric_values=m.metrics_result(),
                   same_parameters=bool(torch.equal(m.params, models["plain"].params)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
