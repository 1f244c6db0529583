"""
The train sampler on the GPU (data.TrainSampler, csrc/augment.hip):

a. `mpu_plane_stats` (plane_stats_kernel), which feeds the accept / reject rule, against NumPy on the same values: the class
   mask is the OR of 1 << l over the labels < 32, the flag is `np.any(~np.isclose(x.astype(float64), float(b)))` over the
   channels. For finite inputs the kernel's f32 subtraction x - b is exact wherever |x - b| is near the tolerance
   1e-8 + 1e-5 |b| (Sterbenz: x within a factor 2 of b; or b == 0), and away from it a rounding error of half an ulp of the
   difference cannot cross the tolerance -- so the results must be EQUAL. Finite background values only: the background is a
   percentile of a finite volume (or a number from the YAML), which is finite.
b. The sampler end to end on a small volume: every decision of every batch, as recorded in `last_trace`, is the one the
   reference rule (tests/sampler_ref.py, pinned on the reference's own runs by tests/test_sampler_rule_host.py) takes on the
   same candidates, the returned planes are the accepted candidates, and the batches exercise every way a candidate is
   rejected or forced.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref                                                                      # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 65536, 65537, 65791)   # the last three: second pass of the grid-stride loop (256 blocks)


# ---------------------------------------------------------------------------------------------------------------- a. plane statistics
def ref_mask(y):
    m = 0
    for l in np.unique(y):
        if l < 32:
            m |= 1 << int(l)
    return m


def ref_flag(x, bg):
    """x f32 [n_pixels, C], bg f32 [C]."""
    return int(any(np.any(~np.isclose(x[:, c].astype(np.float64), float(bg[c]))) for c in range(x.shape[1])))


def plane_stats(y, x, bg, out=None):
    """(mask, flag) of mpu_plane_stats; y u8 [n] or None, x f32 [n, C] or None (NumPy). `out`: a device buffer to reuse."""
    from multiplanarunet_amd import _lib
    n = len(y) if y is not None else len(x)
    assert x is None or (len(x) == n and len(bg) == x.shape[1])             # the kernel reads n pixels of both
    yd = None if y is None else torch.as_tensor(np.ascontiguousarray(y)).cuda()
    xd = None if x is None else torch.as_tensor(np.ascontiguousarray(x)).cuda()
    bd = None if x is None else torch.as_tensor(np.asarray(bg, np.float32)).cuda()
    if out is None:
        out = torch.full((2,), -1, dtype=torch.int32, device="cuda")       # 0xFFFFFFFF: the call must clear it
    _lib.call("mpu_plane_stats", _lib.ptr(yd), _lib.ptr(xd), n, 0 if x is None else x.shape[1], _lib.ptr(bd), _lib.ptr(out),
              _lib.stream_ptr())
    m, f = out.tolist()
    return m & 0xFFFFFFFF, f & 0xFFFFFFFF


@pytest.mark.parametrize("n_channels", (1, 2, 3))
def test_plane_stats_equals_numpy_at_every_size(n_channels):
    rng = np.random.RandomState(100 + n_channels)
    C = n_channels
    flags = set()
    for n in SIZES:
        pool = rng.choice(np.arange(0, 48), 5, replace=False)               # some labels >= 32 among them
        y = pool[rng.randint(0, len(pool), n)].astype(np.uint8)
        bg = rng.uniform(-2, 2, C).astype(np.float32)
        x = np.broadcast_to(bg, (n, C)).copy()
        if rng.rand() < 0.5:
            x[rng.randint(0, n), C - 1] += np.float32(0.5)
        flags.add(ref_flag(x, bg))
        assert plane_stats(y, x, bg) == (ref_mask(y), ref_flag(x, bg)), (n, C)
        assert plane_stats(y, None, None) == (ref_mask(y), 0), (n, C, "labels only")
        assert plane_stats(None, x, bg) == (0, ref_flag(x, bg)), (n, C, "image only")
        xr = (bg + rng.randn(n, C) * (rng.rand(n, 1) < 0.01)).astype(np.float32)   # ~1 % of the pixels differ, any channel
        assert plane_stats(None, xr, bg)[1] == ref_flag(xr, bg), (n, C, "random image")
    assert flags == {0, 1}


def test_plane_stats_clears_and_reuses_its_output_buffer():
    rng = np.random.RandomState(7)
    out = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    bg = np.array([0.25, -1.0], np.float32)
    y1 = rng.choice([0, 3, 9], 257).astype(np.uint8)
    x1 = np.broadcast_to(bg, (257, 2)).copy(); x1[200, 1] = 5.0
    assert plane_stats(y1, x1, bg, out) == (ref_mask(y1), 1) == (1 | 1 << 3 | 1 << 9, 1)
    y2 = rng.choice([1, 2], 65).astype(np.uint8)                             # nothing of the first call may remain
    x2 = np.broadcast_to(bg, (65, 2)).copy()
    assert plane_stats(y2, x2, bg, out) == (ref_mask(y2), 0) == (1 << 1 | 1 << 2, 0)
    assert plane_stats(np.full(257, 40, np.uint8), x1, bg, out) == (0, 1)


def test_plane_stats_labels_31_32_and_255():
    for n in (64, 65791):
        y = np.zeros(n, np.uint8); y[n - 1] = 31
        assert plane_stats(y, None, None) == (1 | 1 << 31, 0)
        y = np.full(n, 32, np.uint8); y[n // 2] = 255
        assert plane_stats(y, None, None) == (0, 0) and ref_mask(y) == 0
        y = np.full(n, 255, np.uint8); y[0] = 32; y[n - 1] = 31; y[n // 3] = 30
        assert plane_stats(y, None, None) == (1 << 31 | 1 << 30, 0)


@pytest.mark.parametrize("where", (0, 65536, 65790))
def test_plane_stats_one_differing_pixel_in_the_last_channel(where):
    n, C = 65791, 3
    bg = np.array([1.0, -3.5, 0.125], np.float32)
    x = np.broadcast_to(bg, (n, C)).copy()
    assert plane_stats(None, x, bg) == (0, 0)
    x[where, C - 1] = np.float32(0.125) + np.float32(1e-3)
    assert ref_flag(x, bg) == 1 and plane_stats(None, x, bg) == (0, 1)


@pytest.mark.parametrize("b", (1.0, -3.5, 1e6, 0.0))
def test_plane_stats_tolerance_edges(b):
    """x = b +- (tolerance, rounded to f32) and its neighbours k f32 steps to either side: the comparison flips inside the
    range, and the kernel flips where NumPy does."""
    b32 = np.float32(b)
    tol = 1e-8 + 1e-5 * abs(float(b32))
    seen = set()
    for sign in (1.0, -1.0):
        x0 = np.float32(float(b32) + sign * tol)
        xs = [x0]
        for direction in (np.float32(np.inf), np.float32(-np.inf)):
            v = x0
            for _ in range(4):
                v = np.nextafter(v, direction)
                xs.append(v)
        for v in xs:
            assert np.isfinite(v)
            x = np.full((65, 1), b32, np.float32); x[33, 0] = v
            want = ref_flag(x, [b32])
            seen.add((sign, want))
            assert plane_stats(None, x, [b32])[1] == want, (b, float(v), float(v) - float(b32), tol)
    assert seen == {(1.0, 0), (1.0, 1), (-1.0, 0), (-1.0, 1)}


@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_plane_stats_nan_and_inf_pixels_are_not_background(value):
    for bg in ([0.0], [2.5, -1e6]):
        bg = np.asarray(bg, np.float32)
        x = np.broadcast_to(bg, (257, len(bg))).copy()
        x[256, len(bg) - 1] = value
        assert ref_flag(x, bg) == 1 and plane_stats(None, x, bg) == (0, 1)


# ---------------------------------------------------------------------------------------------------------------- b. the sampler end to end
SIZE, DIM, SPAN, BATCH, N_CLASSES = 64, 32, 96.0, 8, 4
FLOOR_X = 28                                                  # the image is exactly 0 (its 1 % background value) below this x
VIEWS = np.array([[1.0, 0.0, 0.0], [0.45, 0.6, 0.66]])
BLOBS = ((1, (12, 18, 20), 6.0), (2, (46, 18, 40), 4.0), (3, (36, 48, 44), 4.0), (7, (48, 46, 14), 6.0))
RUNS = {10: (50, 10), 3: (10, 10)}        # max_tries -> (seed, batches); seeds chosen with the host model below: it predicts
                                          # each event in at least 5 of the 10 batches


def sampler_volume():
    """64^3: three small separated blobs of classes 1, 2, 3 and one of value 7 (no class of a 4-class model); an image that is
    smooth for x >= FLOOR_X and exactly 0 below, so that the '1pct' background value is 0 and a plane that stays below
    FLOOR_X is all background INSIDE the volume -- it can carry class 1. real_space_span 96 > 64 lets offsets leave the volume."""
    g = np.mgrid[:SIZE, :SIZE, :SIZE].astype(np.float32)
    lab = np.zeros((SIZE,) * 3, np.uint8)
    for value, c, r in BLOBS:
        lab[(g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2 <= r * r] = value
    img = 1.0 + 0.3 * np.sin(g[0] / SIZE * 3) + 0.2 * np.cos(g[1] / SIZE * 5) + 0.1 * g[2] / SIZE
    img[:FLOOR_X] = 0.0
    return img[..., None].astype(np.float32), lab, np.eye(4)


def host_plane(lab, basis, off):
    """Host model of one candidate (nearest lookup along the plane_basis_fast basis): (class mask, nonbg). Good enough to
    choose seeds with; the test itself never uses it."""
    g = np.linspace(-(SPAN // 2), SPAN // 2, DIM)
    gi, gj = np.meshgrid(g, g, indexing="ij")
    p = np.asarray(basis, float).reshape(3, 3) @ np.stack([gi.ravel(), gj.ravel(), np.full(gi.size, off)])
    half = (SIZE - 1) / 2.0
    inside = (np.abs(p) <= half).all(0)
    idx = np.clip(np.rint(p + half).astype(int), 0, SIZE - 1)
    l = np.where(inside, lab[idx[0], idx[1], idx[2]], 0)
    return ref_mask(l), bool((inside & (p[0] + half > FLOOR_X - 1)).any())


def host_batch(lab, rng, max_tries):
    """The trace of one batch as the host model predicts it: TrainSampler.__call__'s random stream and round scheme (all
    undecided slots drawn in slot order, judged in order up to the first rejection) over host_plane."""
    from multiplanarunet_amd.data import SliceRule, plane_basis_fast
    rule = SliceRule(BATCH, N_CLASSES, 0.5, "auto", max_tries)
    trace, tries, stats, first = [[] for _ in range(BATCH)], [0] * BATCH, [None] * BATCH, 0
    while first < BATCH:
        for slot in range(first, BATCH):
            if stats[slot] is None:
                if tries[slot] == 0:
                    rng.randint(0, 1)                         # (the volume draw)
                tries[slot] += 1
                view = VIEWS[rng.randint(0, len(VIEWS))]
                off = rng.uniform(-(SPAN // 2), SPAN // 2)
                stats[slot] = host_plane(lab, plane_basis_fast(view, rng.normal(scale=0.1, size=3)), off)
        while first < BATCH:
            cand, stats[first] = stats[first], None
            trace[first].append(cand)
            if not rule.judge(first, tries[first], *cand):
                break
            first += 1
    return trace


def judge_trace(trace, max_tries, fg_batch_fraction=0.5, force_all_fg="auto"):
    """Replay one batch's last_trace through the reference rule. Asserts that every slot is accepted at its last judged
    candidate and at none before; returns the set of events seen."""
    events, has_fg = set(), 0
    assert len(trace) == BATCH
    for slot, cands in enumerate(trace):
        assert 1 <= len(cands) <= max_tries
        as_sets = [({c for c in range(32) if m >> c & 1}, nonbg) for m, nonbg in cands]
        t, change, verdicts, kept = sampler_ref.slot_tries(as_sets, slot, has_fg, BATCH, N_CLASSES, fg_batch_fraction,
                                                           force_all_fg, max_tries)
        assert t == len(cands), "slot %d: the reference accepts try %s of %s, %s" % (slot, t, cands, verdicts)
        has_fg += change
        events |= set(verdicts)
        fg = set(range(1, N_CLASSES))
        if any(k and (cl & fg) and v in ("fraction", "allbg") for (cl, _), k, v in zip(as_sets, kept, verdicts)):
            events.add("kept")                                # classes entered the slot's vector, the candidate was rejected after
    return events


@pytest.mark.parametrize("max_tries", sorted(RUNS))
def test_sampler_decisions_are_the_reference_rule_and_batches_are_the_accepted_planes(max_tries):
    from multiplanarunet_amd.data import as_volume, TrainSampler
    img, lab, aff = sampler_volume()
    vol = as_volume(img, lab, aff, "1pct", "RobustScaler", "cuda", "blobs")
    assert vol.bg_value == [0.0]
    seed, batches = RUNS[max_tries]
    s = TrainSampler([vol], VIEWS, DIM, SPAN, BATCH, N_CLASSES, noise_sd=0.1, seed=seed, max_tries=max_tries)
    bg_scaled = s._vc(vol).bg_scaled.cpu().numpy()
    assert np.isfinite(bg_scaled).all()
    events = set()
    for _ in range(batches):
        x, y, w = s()
        trace = s.last_trace
        assert s.rounds == 1 + sum(len(c) - 1 for c in trace)
        events |= judge_trace(trace, max_tries)
        xh, yh = x.cpu().numpy().reshape(BATCH, DIM * DIM, 1), y.reshape(BATCH, -1)
        for slot in range(BATCH):
            m, nonbg = trace[slot][-1]
            assert type(m) is int and type(nonbg) is bool
            assert ref_mask(torch.unique(yh[slot]).cpu().numpy()) == m, slot
            assert bool(ref_flag(xh[slot], bg_scaled)) == nonbg, slot
    print("max_tries %d: events %s" % (max_tries, sorted(events)))
    # coverage is a condition: a rejection by the vector check, by the foreground fraction, as all-background; a forced
    # acceptance at the last try; a candidate whose classes were kept after a later rejection
    assert events >= {"vec", "fraction", "allbg", "forced", "kept", "accept"}, events


if __name__ == "__main__":                                    # seed search with the host model (no GPU): batches with each event
    import collections
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _, lab_, _ = sampler_volume()
    for mt in sorted(RUNS):
        for seed_ in range(60):
            rng_, cnt = np.random.RandomState(seed_), collections.Counter()
            for _ in range(RUNS[mt][1]):
                cnt.update(judge_trace(host_batch(lab_, rng_, mt), mt))
            if min(cnt[e] for e in ("vec", "fraction", "allbg", "forced", "kept")) >= 5:
                print("max_tries %d seed %d: %s" % (mt, seed_, dict(cnt)))
