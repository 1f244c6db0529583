#!/usr/bin/env python
"""
Time of one train step at BASELINE.json configs[1] (B = 16, 128 x 128 x 1, depth 4, 64 filters, bf16) under a given optimizer, by
the method of bench.py's timed train leg: the whole step replayed from one HIP graph, W >= 10 warm-up steps, K >= 50 timed steps
between two HIP events, R repeats. One JSON line per call.

  python tools/time_optimizers.py --optimizer SGD --optimizer-kwargs '{"lr": 1e-4, "momentum": 0.9}' [--steps 50 --warmup 10 --repeats 3]
  python tools/time_optimizers.py --root /path/to/another/checkout     # the same measurement on another build (A/B)
  python tools/time_optimizers.py --optimizer Adamax --eager --steps 5 --repeats 1      # eager launches (under a profiler)

--root: import multiplanarunet_amd from that checkout (with its own built library) instead of this one; a checkout that predates
the optimizers is given the default Adam only. MPU_TAIL_OVERLAP=0 in the environment times Adam's serial tail, the schedule every
other optimizer runs under.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", default="Adam")
    ap.add_argument("--optimizer-kwargs", default="{}")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from multiplanarunet_amd.unet import UNet
    quiet = lambda *a, **k: None
    B, dim = args.batch, args.dim
    model = UNet(n_classes=3, dim=dim, n_channels=1, depth=4, complexity_factor=1.0, flatten_output=True, dtype=args.dtype,
                 logger=quiet, seed=0)
    kw = json.loads(args.optimizer_kwargs)
    if args.optimizer == "Adam" and not kw:
        model.compile("Adam", "SparseCategoricalCrossentropy")
    else:
        model.compile(args.optimizer, "SparseCategoricalCrossentropy", optimizer_kwargs=kw)
    g = torch.Generator(device="cpu").manual_seed(1234)                 # bench.py's batch
    x = torch.randn(B, dim, dim, 1, generator=g).cuda()
    xs = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 5, 1, 2)[:, 0]
    y = ((xs > 0.1).to(torch.uint8) + (xs > 0.45).to(torch.uint8)).reshape(B, dim * dim, 1).contiguous()
    sw = torch.ones(B, device="cuda")
    if args.eager:
        run = lambda: model.train_step(x, y, sw, want_loss=False)
    else:
        run = model.make_graphed_train_step(x, y, sw)
    for _ in range(max(1, args.warmup)):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / args.steps)
    loss = float(model.loss_mean().item())
    slots = getattr(model, "_slots", None)
    print(json.dumps({"tag": args.tag, "optimizer": args.optimizer, "optimizer_kwargs": kw, "slots": 2 if slots is None else len(slots),
                      "tail_overlap": os.environ.get("MPU_TAIL_OVERLAP", "1"), "launch": "eager" if args.eager else "graph",
                      "params": int(model.params.numel()), "batch": B, "dim": dim, "dtype": args.dtype, "steps": args.steps,
                      "warmup": args.warmup, "ms_per_step": [round(v, 4) for v in ms], "last_logged_loss": loss}), flush=True)


if __name__ == "__main__":
    main()
