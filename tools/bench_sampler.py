"""Throughput of the train-time plane sampler (dev tool)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from multiplanarunet_amd.data import make_toy_volume, as_volume, random_views, TrainSampler
from multiplanarunet_amd.augmentation import build_augmenters
vols = []
for i in range(4):
    img, lab, aff = make_toy_volume(128, i)
    vols.append(as_volume(img, lab, aff, "1pct", "RobustScaler", "cuda", "toy%d" % i))
views = random_views(6, 60.0, 0)
for augs in (None, [{"cls_name": "Elastic2D", "kwargs": {"alpha": [0, 450], "sigma": [20, 30], "apply_prob": 0.333}}]):
    s = TrainSampler(vols, views, 128, 128.0, 16, 3, noise_sd=0.1, seed=0, augmenters=build_augmenters(augs, 1))
    for _ in range(3): s()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n = 20
    rounds = cands = 0
    for _ in range(n):
        x, y, w = s()
        rounds += s.rounds; cands += sum(len(c) for c in s.last_trace)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print("augmenters=%s: %.1f ms / batch of 16 -> %.0f slices/s; %.2f candidates, %.2f rounds (host reads) per batch"
          % (bool(augs), dt / n * 1e3, 16 * n / dt, cands / n, rounds / n))
