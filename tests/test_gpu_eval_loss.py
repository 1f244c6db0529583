"""
mpu_eval_loss (csrc/eval_loss.hip) through the C ABI: the loss value of a batch from its probabilities alone, all six loss kinds,
against the f64 restatements tests/loss_ref.py and oracle/unet_ref.py keras_sparse_ce on the SAME f32 probabilities.

Shapes: B = 3 images of 5000 pixels (two 4096-pixel chunks, a ragged tail, no multiple of 256), K in {1, 3, 8}. Into seeded softmax
probabilities go exact 0.0 and 1.0 entries (both clip edges), one image whose labels lack the last class (the infinite-weight branch
of generalized Dice), non-unit sample weights and one label >= K. That label is masked out of the references: a one-hot row of
zeros (tests/loss_ref.py's own _one_hot cannot encode it, so the test swaps in a masked one for the call), a zero per-pixel
cross-entropy. The clip to [1e-7, 1 - 1e-7] is an f32 operation in TensorFlow and in the kernels (1 - 1e-7 rounds to 1 - 1.19e-7
there): the references of the three clipping kinds receive the probabilities clipped in f32, so that their own f64 clip moves
nothing -- at K = 1, where every probability sits on the upper edge, an f64 clip alone would change the focal value by 70 %.
Tolerance: rtol 1e-5, as tests/test_gpu_losses.py:147-148 for the same comparison.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as LR                                                                   # noqa: E402

pytestmark = pytest.mark.gpu
B, PPI = 3, 5000
SW = np.array([1.0, 0.33, 2.0], np.float32)
CE = "SparseCategoricalCrossentropy"
KIND = {CE: 0, "SparseDiceLoss": 1, "SparseJaccardDistanceLoss": 2, "SparseGeneralizedDiceLoss": 3, "SparseFocalLoss": 4,
        "SparseExponentialLogarithmicLoss": 5}
CLIPS = (CE, "SparseFocalLoss", "SparseExponentialLogarithmicLoss")
# every kind with its default kwargs, then one non-default set per loss ("ramp": one class weight per class, .2 ... 1.4)
CASES = [(CE, {})] + [(n, {}) for n in LR.LOSSES] + [
    ("SparseDiceLoss", {"smooth": 0}), ("SparseJaccardDistanceLoss", {"smooth": 0.5}),
    ("SparseGeneralizedDiceLoss", {"type_weight": "Simple"}), ("SparseGeneralizedDiceLoss", {"type_weight": "Uniform"}),
    ("SparseFocalLoss", {"gamma": 0.3, "class_weights": "ramp"}),
    ("SparseExponentialLogarithmicLoss", {"gamma_dice": 1, "gamma_cross": 0.3, "weight_dice": 1, "weight_cross": 0.5})]
IDS = ["%s%s" % (n.replace("Sparse", "").replace("Loss", ""), "-".join([""] + ["%s=%s" % kv for kv in kw.items()])) for n, kw in CASES]


def _kw(kw, K):
    kw = dict(kw)
    if kw.get("class_weights") == "ramp":
        kw["class_weights"] = [float(v) for v in np.linspace(.2, 1.4, K)]
    return kw


def _cfg(name, kw, K):
    from multiplanarunet_amd import _lib
    a = dict(LR.DEFAULTS.get(name, {}))
    a.update(kw)
    c = _lib.LossConfig()
    c.kind = KIND[name]
    c.smooth = float(a.get("smooth", 1))
    c.type_weight = {"square": 0, "simple": 1, "uniform": 2}[str(a.get("type_weight", "Square")).lower()]
    c.gamma = float(a.get("gamma", 2))
    c.gamma_dice, c.gamma_cross = float(a.get("gamma_dice", .3)), float(a.get("gamma_cross", .3))
    c.weight_dice, c.weight_cross = float(a.get("weight_dice", 1)), float(a.get("weight_cross", 1))
    if a.get("class_weights") is not None:
        c.n_class_weights = K
        for i, v in enumerate(a["class_weights"]):
            c.class_weights[i] = v
    return c


_INPUTS = {}


def _inputs(K, seed=0):
    """(probs f32 [B, PPI, K], labels uint8 [B, PPI]) -- built once per (K, seed), never written again."""
    if (K, seed) not in _INPUTS:
        rng = np.random.RandomState(100 * K + seed)
        z = rng.randn(B, PPI, K) * 3.0
        p = np.exp(z - z.max(-1, keepdims=True))
        p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
        y = rng.randint(0, K, (B, PPI)).astype(np.uint8)
        if K > 1:
            y[1][y[1] == K - 1] = 0                                  # image 1: the last class never occurs
            p[0, 10] = np.eye(K, dtype=np.float32)[y[0, 10]]          # the label's probability exactly 1.0, the others 0.0
            p[0, 4200] = np.eye(K, dtype=np.float32)[(y[0, 4200] + 1) % K]     # ... exactly 0.0
        else:
            p[0, 4200] = 0.0
        y[2, PPI - 1] = K                                            # one label outside the classes, in the ragged tail
        p.setflags(write=False); y.setflags(write=False)
        _INPUTS[(K, seed)] = (p, y)
    return _INPUTS[(K, seed)]


def _masked_one_hot(y, K, dtype):
    y = y.reshape(y.shape[0], -1).long()
    oh = torch.nn.functional.one_hot(torch.clamp(y, max=K - 1), K).to(dtype)
    oh[y >= K] = 0
    return oh


def _reference(name, kw, p, y, sw, monkeypatch):
    """w_b * L_b [B] in f64."""
    from oracle import unet_ref as U
    K = p.shape[-1]
    if name in CLIPS:
        p = np.clip(p, np.float32(1e-7), np.float32(1) - np.float32(1e-7))
    pt = torch.tensor(p.astype(np.float64))
    yt = torch.tensor(y.astype(np.int64))
    w = np.ones(B) if sw is None else np.asarray(sw, np.float64)
    if name == CE:
        l = U.keras_sparse_ce(pt.reshape(B, PPI, 1, K), torch.clamp(yt, max=K - 1).reshape(B, PPI, 1), torch.tensor(w))
        l = l.reshape(B, PPI) * (yt < K)
        return l.mean(1).numpy()
    monkeypatch.setattr(LR, "_one_hot", _masked_one_hot)
    return LR.loss_ref(name, yt, pt, w, **kw).numpy().reshape(-1)


def _run(cfg, p, y, sw, K, want_loss=True, acc=None, b=B, ppi=PPI):
    """One call; returns (status, d_loss as numpy or None)."""
    import ctypes as C
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    dp, dy = torch.tensor(np.array(p), device="cuda"), torch.tensor(np.array(y), device="cuda")      # (copies: the inputs are read-only)
    dsw = None if sw is None else torch.as_tensor(np.asarray(sw, np.float32), device="cuda")
    n = int(lib.mpu_eval_loss_scratch_bytes(B, PPI, min(max(K, 1), 8)))
    assert n > 0 and n % 8 == 0
    scratch = torch.full((n // 8,), float("nan"), dtype=torch.float64, device="cuda")     # its contents must not matter
    out = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda") if want_loss else None
    rc = lib.mpu_eval_loss(C.byref(cfg), _lib.ptr(dp), _lib.ptr(dy), _lib.ptr(dsw), b, ppi, K, _lib.ptr(scratch), _lib.ptr(out),
                           _lib.ptr(acc), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, (out.cpu().numpy() if want_loss else None)


@pytest.mark.parametrize("K", (1, 3, 8))
@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_values_against_the_f64_restatements(name, kw, K, monkeypatch):
    p, y = _inputs(K)
    kw = _kw(kw, K)
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    rc, got = _run(_cfg(name, kw, K), p, y, SW, K, acc=acc)
    assert rc == 0
    want = _reference(name, kw, p, y, SW, monkeypatch)
    print("%s %s K=%d: got %s want %s rel %s" % (name, kw, K, got, want, np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=1e-5)
    a = acc.cpu().numpy()
    np.testing.assert_allclose(a[0], want.mean(), rtol=1e-5)
    assert a[1] == 1.0


@pytest.mark.parametrize("name", (CE, "SparseGeneralizedDiceLoss"))
def test_accumulator_over_three_batches(name, monkeypatch):
    K = 3
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    want = 0.0
    for seed in (0, 1, 2):
        p, y = _inputs(K, seed)
        rc, _ = _run(_cfg(name, {}, K), p, y, SW, K, acc=acc)
        assert rc == 0
        want += _reference(name, {}, p, y, SW, monkeypatch).mean()
    a = acc.cpu().numpy()
    print(name, "accumulated", a, "reference", want)
    np.testing.assert_allclose(a[0], want, rtol=1e-5)
    assert a[1] == 3.0


@pytest.mark.parametrize("name", (CE, "SparseDiceLoss", "SparseFocalLoss"))
def test_optional_arguments(name):
    K = 3
    p, y = _inputs(K)
    cfg = _cfg(name, {}, K)
    rc, ones = _run(cfg, p, y, np.ones(B, np.float32), K)
    rc2, none = _run(cfg, p, y, None, K)
    assert rc == 0 and rc2 == 0 and np.array_equal(ones, none) and np.isfinite(none).all()
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    rc, out = _run(cfg, p, y, SW, K, want_loss=False, acc=acc)                  # d_loss NULL
    assert rc == 0 and out is None and acc[1].item() == 1.0
    rc, out = _run(cfg, p, y, SW, K, acc=None)                                  # d_acc NULL
    assert rc == 0
    np.testing.assert_allclose(acc[0].item(), out.astype(np.float64).mean(), rtol=1e-6)     # (d_loss is the f32 rounding of the f64 values)
    rc, _ = _run(cfg, p, y, SW, K, want_loss=False, acc=None)                   # both
    assert rc == 0


def test_bad_arguments_are_refused():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    p, y = _inputs(8)
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    for name in (CE, "SparseDiceLoss"):
        cfg = _cfg(name, {}, 8)
        assert _run(cfg, p, y, SW, 9, acc=acc)[0] != 0 and lib.mpu_last_error()
        assert _run(cfg, p, y, SW, 0, acc=acc)[0] != 0
        assert _run(cfg, p, y, SW, 8, acc=acc, b=0)[0] != 0
        assert _run(cfg, p, y, SW, 8, acc=acc, ppi=0)[0] != 0
    cfg = _cfg(CE, {}, 8)
    cfg.kind = 6
    assert _run(cfg, p, y, SW, 8, acc=acc)[0] != 0
    for b, ppi, k in ((0, 10, 3), (3, 0, 3), (3, 10, 9), (65536, 10, 3)):
        assert lib.mpu_eval_loss_scratch_bytes(b, ppi, k) < 0
    assert not acc.cpu().numpy().any()                                           # nothing ran


@pytest.mark.parametrize("name", (CE, "SparseExponentialLogarithmicLoss"))
def test_two_calls_give_the_same_bits(name):
    K = 8
    p, y = _inputs(K)
    cfg = _cfg(name, {}, K)
    a0, a1 = (torch.zeros(2, dtype=torch.float64, device="cuda") for _ in range(2))
    _, l0 = _run(cfg, p, y, SW, K, acc=a0)
    _, l1 = _run(cfg, p, y, SW, K, acc=a1)
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and torch.equal(a0, a1) and a0[0].item() != 0.0
