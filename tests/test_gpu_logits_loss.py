"""
The cross-entropy from logits on the GPU: UNet(out_activation="linear").compile(loss_kwargs={"from_logits": True}) -- the train
step against the f64 restatement tests/logits_ref.py, the head's arithmetic alone in every dtype and for 1..8 classes, logits
beyond +-90, agreement with the clipped-probability kernels where nothing is clipped, both forms of the training head,
reproducibility, graph replay, evaluation and `mp train` end to end.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logits_ref as LG                                                                 # noqa: E402
import loss_ref as LR                                                                   # noqa: E402
import metrics_ref as MR                                                                # noqa: E402
from test_gpu_unet import CFGS, rand_weights, quiet                                      # noqa: E402
from test_gpu_losses import _ce_closed_form, _rel                                        # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE = "SparseCategoricalCrossentropy"
FL = {"from_logits": True}
SW3 = np.array([1.0, 0.33, 2.0], np.float32)


def _linear(K, dtype, dim=32, depth=2, cf=1, seed=2, **kw):
    from multiplanarunet_amd.unet import UNet
    return UNet(n_classes=K, dim=dim, depth=depth, complexity_factor=cf, out_activation="linear", dtype=dtype, logger=quiet,
                flatten_output=True, seed=seed, **kw)


def _workspace_logits(m, B, ppi, K):
    from multiplanarunet_amd import _lib
    off = int(_lib.load().mpu_unet_workspace_probs_offset(m._h, B))
    return m._ws[off:off + 4 * B * ppi * K].view(torch.float32).reshape(B, ppi, K).cpu().numpy().astype(np.float64)


def _bias_grad(m, K):
    kind, o, ps, ls = m._tensors["conv2d/bias"]
    return m.grads[o:o + K].cpu().numpy().astype(np.float64)


# ---- 5. the f32 step against the f64 restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS[:2])
def test_f32_train_step_vs_restatement(cfg, noise_mult=3, flip_frac=1e-2):
    """tests/test_gpu_losses.py::test_f32_train_step_vs_restatement on a linear model with the cross-entropy from logits: its
    inputs, its bounds (max(2e-3, 3 * noise) of each gradient tensor's maximum, noise = torch f32 against torch f64 of the same
    graph and loss; its close() rule for the updated weights), no gradient in the channel padding. The loss is [B, H*W]."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    K, C, D, cf, H, W, B = cfg
    w = rand_weights(U, K, C, D, cf, seed=5)
    rng = np.random.RandomState(1)
    x = rng.randn(B, H, W, C).astype(np.float32)
    y = rng.randint(0, K, (B, H * W, 1)).astype(np.uint8)
    y[B - 1][y[B - 1] == K - 1] = 0
    sw = np.array([1.0, 0.33, 2.0][:B], np.float32)
    m = UNet(n_classes=K, img_rows=H, img_cols=W, n_channels=C, depth=D, complexity_factor=cf, out_activation="linear",
             dtype="f32", logger=quiet, flatten_output=True)
    m.set_weights_dict(w)
    m.compile("Adam", CE, loss_kwargs=FL)
    ref = LG.train_step(w, x, y, sw, depth=D, dtype=torch.float64)
    ref32 = LG.train_step(w, x, y, sw, depth=D, dtype=torch.float32)
    logits, loss = m.forward_backward(x, y, sw)
    assert tuple(loss.shape) == (B, H * W)
    pn = np.abs(ref32["logits"] - ref["logits"]).max()
    np.testing.assert_allclose(logits.cpu().numpy(), ref["logits"], rtol=0, atol=max(2e-5, 3 * pn))
    got_l = loss.cpu().numpy()
    print("K=%d: logits noise %.2e, loss max err %.2e, logged mean %.7g (f64 %.7g)" % (
        K, pn, np.abs(got_l - ref["loss"]).max(), float(m.loss_mean().item()), ref["loss"].mean()))
    np.testing.assert_allclose(got_l, ref["loss"], rtol=1e-3, atol=max(1e-5, 30 * pn))
    np.testing.assert_allclose(float(m.loss_mean().item()), ref["loss"].mean(), rtol=1e-3, atol=max(1e-5, 30 * pn))
    g = m.grads.cpu().numpy()
    for tname, gr in ref["grads"].items():
        kind, off, ps, ls = m._tensors[tname]
        a = g[off:off + int(np.prod(ps))].reshape(ps)
        logical = m._from_stored(tname, a, ps, ls)
        assert np.count_nonzero(a) == np.count_nonzero(logical), "gradient leaked into channel padding of " + tname
        scale = np.abs(gr).max() + 1e-12
        e = np.abs(logical - gr).max() / scale
        noise = np.abs(ref32["grads"][tname] - gr).max() / scale
        assert e <= max(2e-3, noise_mult * noise), (tname, e, noise)
    m.apply_gradients()
    new = m.get_weights_dict()
    lr = 5e-5

    def close(tname, got, val, steps):
        d = np.abs(got - val)
        bad = d > 2e-6 + 1e-5 * np.abs(val).max()
        allowed = max(4, (flip_frac if steps == 1 else 3e-2) * bad.size)
        assert bad.sum() <= allowed and d.max() <= 2.2 * lr * steps + 1e-5 * np.abs(val).max(), \
            (tname, bad.sum(), bad.size, d.max())
    for tname, val in ref["weights"].items():
        close(tname, new[tname], val, 1)


# ---- 6. / 7. the head's arithmetic alone -----------------------------------------------------------------------------------------
def _head_inputs(K, B=3, H=32):
    rng = np.random.RandomState(4)
    x = rng.randn(B, H, H, 1).astype(np.float32)
    y = rng.randint(0, K, (B, H * H)).astype(np.uint8)
    y[1][y[1] == K - 1] = 0
    return x, y


def _head_model(K, dtype, scale):
    m = _linear(K, dtype)
    w = m.get_weights_dict()
    w["conv2d/kernel"] = w["conv2d/kernel"] * scale
    m.set_weights_dict(w)
    return m.compile("Adam", CE, loss_kwargs=FL)


def _check_head_against_f64(m, x, y, sw, K, tag):
    """One forward_backward; from the logits the GPU itself left in the workspace, recompute in f64 the per-image sums of the
    per-pixel losses, the logged mean and sum_m dz_mk. Bounds of test_gpu_losses.test_loss_arithmetic_on_the_gpus_own_probabilities:
    1e-5 relative; the bias gradient to 1e-5 * sum_m |dz_mk| per class. Returns (logits, dz) in f64."""
    B, ppi = y.shape
    _, loss = m.forward_backward(x, y.reshape(B, -1, 1), sw)
    z = _workspace_logits(m, B, ppi, K)
    Lpix, dz = LG.closed_form(z, y, sw.astype(np.float64))
    got = loss.cpu().numpy().astype(np.float64)
    assert got.shape == (B, ppi) and np.isfinite(got).all() and torch.isfinite(m.grads).all()
    got_l, want_l = got.sum(1), Lpix.sum(1)
    got_mean, want_mean = float(m.loss_mean().item()), Lpix.mean()
    got_db, want_db, bound = _bias_grad(m, K), dz.sum((0, 1)), 1e-5 * np.abs(dz).sum((0, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        print("%-22s losses rel %.2e  mean rel %.2e  bias-gradient err / sum|dz| %.2e  logits in [%.4g, %.4g]" % (
            tag, np.nanmax(np.abs(got_l / want_l - 1)) if want_l.any() else 0.0, abs(got_mean / want_mean - 1) if want_mean else 0.0,
            np.nanmax(np.abs(got_db - want_db) / (bound / 1e-5)) if bound.any() else 0.0, z.min(), z.max()))
    np.testing.assert_allclose(got_l, want_l, rtol=1e-5)
    np.testing.assert_allclose(got_mean, want_mean, rtol=1e-5)
    assert (np.abs(got_db - want_db) <= bound).all(), (tag, got_db, want_db, bound)
    return z, dz


@pytest.mark.parametrize("K", (3, 1, 2, 4, 8))
@pytest.mark.parametrize("dtype", ("f32", "bf16x3", "bf16"))
def test_loss_arithmetic_on_the_gpus_own_logits(dtype, K):
    """K = 3 is the shape of the per-image losses' test; 1, 2, 4, 8: one class (L = 0 and dz = 0 exactly), both launch-bound
    boundaries (K <= 3 / K <= 4) and the widest register footprint. cf = 1: bf16 (and bf16x3 up to 4 classes) run the fused head."""
    x, y = _head_inputs(K)
    m = _head_model(K, dtype, 4.0)                                  # spread the logits
    z, dz = _check_head_against_f64(m, x, y, SW3, K, "%s K=%d" % (dtype, K))
    if K == 1:
        assert not m.forward_backward(x, y.reshape(3, -1, 1), SW3)[1].any() and not _bias_grad(m, K).any()
    else:
        assert np.abs(dz).max() > 1e-2                              # a real gradient was checked


@pytest.mark.parametrize("dtype", ("f32", "bf16x3", "bf16"))
def test_large_logits_stay_finite_and_keep_their_gradient(dtype):
    """The head kernel scaled until the GPU's own logits pass +-90 (asserted). Loss and gradient are finite and match the f64
    recomputation to the bounds above. Then image 0 alone (weights [1, 0, 0]), its saturated pixels labelled by their LEAST likely
    class: the label's probability is below 1e-7 (asserted) and the clipped form's gradient is zero there (asserted on its NumPy
    restatement); the from-logits gradient is not."""
    K, B = 3, 3
    x, y = _head_inputs(K)
    m = _head_model(K, dtype, 1.0)
    m.forward_backward(x, y.reshape(B, -1, 1), SW3)
    z0 = _workspace_logits(m, B, y.shape[1], K)                      # (the head's bias is zero: the logits scale with its kernel)
    scale = 120.0 / min(z0.max(), -z0.min())
    m = _head_model(K, dtype, scale)
    z, dz = _check_head_against_f64(m, x, y, SW3, K, "%s large logits" % dtype)
    print("%s: head kernel x %.1f, logits in [%.2f, %.2f]" % (dtype, scale, z.min(), z.max()))
    assert z.max() > 90 and z.min() < -90, (z.min(), z.max())
    e = np.exp(z[0] - z[0].max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    low = ((p < 1e-7) | (p > 1 - 1e-7)).all(-1)                          # pixels of image 0 whose every probability the clip would move
    y2 = y.copy()                                                        # (its mask then passes no class: a zero gradient) ...
    y2[0][low] = p.argmin(-1)[low]                                       # ... are labelled with their least likely class
    sw = np.array([1.0, 0.0, 0.0], np.float32)
    z2, dz2 = _check_head_against_f64(m, x, y2, sw, K, "%s least likely labels" % dtype)
    assert np.array_equal(z2, z)
    py = np.take_along_axis(p, y2[0].astype(np.int64)[:, None], 1)[:, 0]
    assert low.sum() > 100 and py[low].max() < 1e-7, (low.sum(), py[low].max())
    _, g_clip = _ce_closed_form(y2[:1].astype(np.int64), p[None], sw[:1].astype(np.float64))
    clipped_dz = LR.softmax_backward(p[None], g_clip)[0]
    n_dead = int((np.abs(clipped_dz[low]).max(-1) == 0).sum())
    got_db, bound = _bias_grad(m, K), 1e-5 * np.abs(dz2).sum((0, 1))
    share = dz2[0][low].sum(0)                                           # what those pixels add to the bias gradient (f64)
    print("%s: %d pixels clipped in every class, %d of them with a zero clipped-form gradient; from logits: max |dz| %.3g there, their share of "
          "the bias gradient %s of %s (bound %s)" % (dtype, low.sum(), n_dead, np.abs(dz2[0][low]).max(), share, got_db, bound))
    assert n_dead == low.sum()
    # The bias gradient was just held to `bound` of the f64 sum over ALL weighted pixels. The pixels below 1e-7 contribute a hundred
    # bounds and more to it: had the kernel zeroed their dz, as the clipped form does, that check would have failed -- max |dz| > 0
    # on them.
    assert np.abs(dz2[0][low]).max() > 0.99 and (np.abs(share) > 100 * bound).any() and not dz2[1:].any()
    assert np.abs(got_db).max() > 0


# ---- 8. agreement with the kernels that already exist ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f32", "bf16x3", "bf16"))
def test_agrees_with_the_clipped_form_where_nothing_is_clipped(dtype):
    """The same weights in a softmax model with the default loss and in a linear model with the new one, on the inputs of the head
    test. No probability leaves [1e-7, 1 - 1e-7] (asserted), where the two forms are the same function: per pixel
    |L_new - L_old| <= 1e-5 * max(1, |L_old|) (the f32 rounding of log S), head weight and bias gradients to 1e-5 relative L2."""
    from multiplanarunet_amd.unet import UNet
    K, B = 3, 3
    x, y = _head_inputs(K)
    lin = _head_model(K, dtype, 1.0)                                # (unscaled: four times the logits and the clip moves entries)
    soft = UNet(n_classes=K, dim=32, depth=2, complexity_factor=1, dtype=dtype, logger=quiet, flatten_output=True, seed=2)
    soft.set_weights_dict(lin.get_weights_dict())
    soft.compile("Adam", CE)
    _, l_new = lin.forward_backward(x, y.reshape(B, -1, 1), SW3)
    probs, l_old = soft.forward_backward(x, y.reshape(B, -1, 1), SW3)
    p = probs.cpu().numpy()
    assert p.min() >= 1e-7 and p.max() <= 1 - 1e-7, (p.min(), p.max())
    l_new, l_old = l_new.cpu().numpy().astype(np.float64), l_old.cpu().numpy().astype(np.float64)
    err = np.abs(l_new - l_old) / np.maximum(1.0, np.abs(l_old))
    rels = {}
    for t in ("conv2d/kernel", "conv2d/bias"):
        kind, o, ps, ls = lin._tensors[t]
        n = int(np.prod(ps))
        rels[t] = _rel(lin.grads[o:o + n].cpu().numpy(), soft.grads[o:o + n].cpu().numpy().astype(np.float64))
    print("%s: probabilities in [%.3g, %.6f], per-pixel loss err %.2e, head gradients rel-L2 %s, means %.7g / %.7g" % (
        dtype, p.min(), p.max(), err.max(), rels, float(lin.loss_mean().item()), float(soft.loss_mean().item())))
    assert err.max() <= 1e-5
    for t, v in rels.items():
        assert v <= 1e-5, (t, v)


# ---- 9. both forms of the training head -------------------------------------------------------------------------------------------
_STEP_SCRIPT = r"""
import sys, json, numpy as np, torch, ctypes as C
sys.path.insert(0, %r)
from multiplanarunet_amd.unet import UNet
from multiplanarunet_amd import _lib
lib = _lib.load()
quiet = lambda *a, **k: None
out, B, K, D, dim, dtype = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
m = UNet(n_classes=K, dim=dim, n_channels=1, depth=D, complexity_factor=1, out_activation="linear", dtype=dtype, logger=quiet,
         flatten_output=True, seed=5)
w = m.get_weights_dict()
rng = np.random.RandomState(3)
for k in w:                                        # gammas of both signs, non-trivial betas
    if k.endswith("/gamma"): w[k] = rng.uniform(-1.5, 1.5, w[k].shape).astype(np.float32)
    if k.endswith("/beta"): w[k] = rng.uniform(-.3, .3, w[k].shape).astype(np.float32)
m.set_weights_dict(w)
m.compile("Adam", "SparseCategoricalCrossentropy", loss_kwargs={"from_logits": True})
rng = np.random.RandomState(7)
x = torch.tensor(rng.randn(B, dim, dim, 1).astype(np.float32), device="cuda")
yn = rng.randint(0, K, (B, dim * dim, 1)).astype(np.uint8)
yn[B - 1][yn[B - 1] == K - 1] = 0
y = torch.tensor(yn, device="cuda")
sw = torch.tensor(np.where(np.arange(B) %% 2 == 0, 0.4, 1.0).astype(np.float32), device="cuda")
lib.mpu_schedule_log_enable(1)
logits, loss = m.forward_backward(x, y, sw, want_loss=True)
n = lib.mpu_schedule_log_read(None, 0); buf = C.create_string_buffer(int(n) + 1); lib.mpu_schedule_log_read(buf, n + 1)
lib.mpu_schedule_log_enable(0)
nh = sum(1 for l in buf.value.decode().splitlines() if "head=1" in l)
torch.cuda.synchronize()
g = m.grads.cpu().numpy()
def grad_of(t):
    kind, off, ps, ls = m._tensors[t]
    return m._from_stored(t, g[off:off + int(np.prod(ps))].reshape(ps), ps, ls)
np.savez(out + ".npz", logits=logits.float().cpu().numpy(), loss=loss.float().cpu().numpy(), nh=np.int32(nh),
         loss_mean=np.float32(m.loss_mean().item()), state=m.bn_state.cpu().numpy(),
         **{"g:" + k: grad_of(k) for k in m._order if m._tensors[k][0] == 0})
"""


def _run_step(tmp_path, tag, env, B, K, D, dim, dtype):
    f = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _STEP_SCRIPT % ROOT, f, str(B), str(K), str(D), str(dim), dtype],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return dict(np.load(f + ".npz"))


@pytest.mark.parametrize("dtype", ("bf16", "bf16x3"))
def test_fused_and_unfused_training_head_agree(tmp_path, dtype):
    """test_gpu_losses.test_fused_and_unfused_training_head_agree_for_every_loss for the cross-entropy from logits, with its bounds:
    the three head_bn_* passes (head=1 twice in the schedule log) against head_backward_kernel behind MPU_HEAD_TRAIN_FUSED=0 (never).
    Logits, losses and moving statistics the same bits; the head's and the last BatchNorm's gradients to 1e-2 relative L2, all
    gradients cosine >= 0.995."""
    B, K, D, dim = 3, 3, 2, 48
    a = _run_step(tmp_path, "fused", {}, B, K, D, dim, dtype)
    b = _run_step(tmp_path, "chain", {"MPU_HEAD_TRAIN_FUSED": "0"}, B, K, D, dim, dtype)
    last = "upsample_L%d_BN2" % (D - 1)
    assert int(a["nh"]) == 2 and int(b["nh"]) == 0, (a["nh"], b["nh"])
    assert a["loss"].shape == (B, dim * dim)
    assert np.array_equal(a["logits"], b["logits"]) and np.array_equal(a["loss"], b["loss"]) and np.array_equal(a["state"], b["state"])
    assert abs(float(a["loss_mean"]) - float(b["loss_mean"])) <= 1e-6 * abs(float(b["loss_mean"]))
    tight = {k: _rel(a[k], b[k]) for k in a if k.startswith("g:") and (k[2:].split("/")[0] == last or
                                                                      not any(t in k for t in ("encoder", "bottom", "upsample")))}
    keys = sorted(k for k in a if k.startswith("g:"))
    ga = np.concatenate([a[k].ravel() for k in keys]).astype(np.float64)
    gb = np.concatenate([b[k].ravel() for k in keys]).astype(np.float64)
    cos = float(ga @ gb / np.sqrt((ga @ ga) * (gb @ gb)))
    print("fused head vs chain, %s: head / last-BN tensors rel-L2 %s; all gradients cosine %.5f"
          % (dtype, {k[2:]: "%.2e" % v for k, v in tight.items()}, cos))
    assert len(tight) >= 4, list(tight)
    for k, v in tight.items():
        assert v <= 1e-2, (k, v)
    assert cos >= 0.995, cos


# ---- 10. reproducibility and the graphed form --------------------------------------------------------------------------------------
def _small_batch(B=4, H=32, K=3, seed=3):
    rng = np.random.RandomState(seed)
    x = torch.tensor(rng.randn(B, H, H, 1).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, K, (B, H * H, 1)).astype(np.uint8), device="cuda")
    sw = torch.tensor([1.0, 0.33, 1.0, 2.0][:B], device="cuda")
    return x, y, sw


def test_two_passes_on_identical_inputs_are_bit_identical():
    x, y, sw = _small_batch()
    m = _linear(3, "bf16", seed=1).compile("Adam", CE, loss_kwargs=FL)
    state = m.bn_state.clone()
    _, l0 = m.forward_backward(x, y, sw)
    g0, l0, m0 = m.grads.clone(), l0.clone(), m.loss_mean().clone()
    m.bn_state.copy_(state)
    _, l1 = m.forward_backward(x, y, sw)
    assert tuple(l1.shape) == (4, 32 * 32) and torch.isfinite(l1).all() and torch.isfinite(m.grads).all() and float(m.grads.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(m0, m.loss_mean()) and torch.equal(g0, m.grads)


def test_graph_replay_equals_the_eager_loop():
    """20 replays of make_graphed_train_step against 20 train_step calls from the same start: bit-identical parameters, equal
    loss sums."""
    N = 20
    x, y, sw = _small_batch()
    mk = lambda: _linear(3, "bf16", seed=0).compile("Adam", CE, ["sparse_categorical_accuracy"], optimizer_kwargs={"lr": 1e-3},
                                                     loss_kwargs=FL)
    a, b = mk(), mk()
    sum_a = torch.zeros(1, dtype=torch.float64, device="cuda")
    for _ in range(N):
        a.train_step(x, y, sw, want_loss=False)
        sum_a += a.loss_mean().double()
    sum_b = torch.zeros(1, dtype=torch.float64, device="cuda")
    replay = b.make_graphed_train_step(x, y, sw, loss_sum=sum_b)        # performs (and counts) step 1 while warming up
    for _ in range(N - 1):
        replay()
    torch.cuda.synchronize()
    assert a.iterations == b.iterations == N
    assert torch.equal(a.params, b.params) and torch.equal(a.bn_state, b.bn_state)
    assert float(sum_a.item()) == float(sum_b.item()) and float(sum_a.item()) > 0
    assert a.metrics_result() == b.metrics_result() and 0 < a.metrics_result()["sparse_categorical_accuracy"] <= 1


@pytest.mark.parametrize("dtype", ("f32", "bf16x3", "bf16"))
@pytest.mark.parametrize("opt,okw", (("Adam", {"lr": 1e-3}), ("Adam", {"lr": 1e-3, "amsgrad": True}), ("SGD", {"lr": 2e-5, "momentum": 0.9}),
                                     ("RMSprop", {"lr": 1e-3}), ("Adamax", {"lr": 2e-3})),
                         ids=("adam", "amsgrad", "sgd", "rmsprop", "adamax"))
def test_every_optimizer_learns_with_l2_and_metrics(dtype, opt, okw):
    """train_on_batch on a fixed, learnable batch (labels are thresholds of the input), l2_reg set and two metrics compiled: 30 steps
    of each optimizer lower the loss; the values are finite and the accuracy is an arg-max count on the logits. (The gradient is
    that of the SUM over 4096 pixels: SGD's rate is 0.08 per pixel-mean.)"""
    rng = np.random.RandomState(0)
    B, H = 4, 32
    x = rng.randn(B, H, H, 1).astype(np.float32)
    y = ((x[..., 0] > 0).astype(np.uint8) + (x[..., 0] > 1).astype(np.uint8)).reshape(B, -1, 1)
    m = _linear(3, dtype, cf=0.25, seed=0, l2_reg=1e-5)
    m.compile(opt, CE, ["sparse_categorical_accuracy", "sparse_fg_recall"], optimizer_kwargs=okw, loss_kwargs=FL)
    hist = np.array([m.train_on_batch(x, y, [1.0, 0.33, 2.0, 1.0]) for _ in range(30)])
    print(dtype, opt, "loss %.4f -> %.4f, accuracy %.3f -> %.3f" % (hist[0, 0], hist[-1, 0], hist[0, 1], hist[-1, 1]))
    assert np.isfinite(hist).all() and hist[-5:, 0].mean() < hist[:5, 0].mean(), hist[:, 0]
    logits = m.predict_on_batch(x)
    assert float(logits.abs().max()) > 1.0 or float(logits.min()) < 0                # logits, not probabilities


# ---- 11. evaluation ----------------------------------------------------------------------------------------------------------------
EVAL_METRICS = ["sparse_categorical_accuracy", "sparse_fg_recall"]


def _eval_model(dtype, dim):
    m = _linear(3, dtype, dim=dim, cf=0.0625, seed=0)
    m.compile("Adam", CE, EVAL_METRICS, optimizer_kwargs={"lr": 1e-3}, loss_kwargs=FL)
    g = torch.Generator().manual_seed(7)
    for _ in range(3):                                                   # moving statistics away from their initial values
        x = torch.randn(4, dim, dim, 1, generator=g).cuda()
        y = torch.randint(0, 3, (4, dim * dim, 1), generator=g).to(torch.uint8).cuda()
        m.train_step(x, y, torch.rand(4, generator=g).cuda() + 0.5, want_loss=False)
    return m


@pytest.mark.parametrize("dim", (32, 80))                                # 80 x 80 = 6400 pixels per image: two chunks of 4096 are summed
@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_evaluation_equals_the_f64_restatement_and_leaves_the_model_alone(dtype, dim):
    K, B = 3, 6
    m = _eval_model(dtype, dim)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, dim, dim, 1, generator=g).cuda()
    y = torch.randint(0, K, (B, dim * dim, 1), generator=g).to(torch.uint8).cuda()
    w = (torch.rand(B, generator=g) + 0.5).cuda()
    z = m.predict_on_batch(x).cpu().numpy()                              # (refreshes the inference cache at the tail of `packed`)
    yn, wn = y.cpu().numpy().reshape(B, -1), w.cpu().numpy().astype(np.float64)
    torch.cuda.synchronize()
    before = {"params": m.params.clone(), "grads": m.grads.clone(), "bn_state": m.bn_state.clone(), "packed": m.packed.clone(),
              "metrics": m._metrics_state.clone(), "slots": [s.clone() for s in m._slots], "iterations": m.iterations}
    out = m.test_on_batch(x, y, w)
    want = float(LG.closed_form(z, yn, wn)[0].mean())
    one = MR.Mean().update_scores(yn.reshape(-1), z.reshape(-1, K)).result()
    print(dtype, dim, "test_on_batch", out, "f64 of predict's logits", want, [one[k] for k in EVAL_METRICS])
    assert m.metrics_names == ["loss"] + EVAL_METRICS
    np.testing.assert_allclose(out[0], want, rtol=1e-6)
    np.testing.assert_allclose(out[1:], [one[k] for k in EVAL_METRICS], rtol=1e-14, equal_nan=True)
    # evaluate in chunks of 4 + 2: the loss is the mean over the images; unit weights: the mean of the per-pixel losses
    ev = m.evaluate(x, y, batch_size=4, sample_weight=w)
    np.testing.assert_allclose(ev[0], want, rtol=1e-6)
    ev1 = m.evaluate(x, y, batch_size=4, return_dict=True)
    np.testing.assert_allclose(ev1["loss"], float(LG.closed_form(z, yn, np.ones(B))[0].mean()), rtol=1e-6)
    np.testing.assert_allclose(ev1["sparse_categorical_accuracy"], (z.argmax(-1).reshape(B, -1) == yn).mean(), rtol=1e-12)
    # the accumulator interface the Validation callback drives
    acc, state = m.evaluation_begin()
    m.evaluation_update(m.predict_on_batch(x[:4]), y[:4], acc, state, w[:4])
    m.evaluation_update(m.predict_on_batch(x[2:]), y[2:], acc, state, w[2:])
    tot = m.evaluation_totals(acc, state)
    want2 = float(LG.closed_form(z[:4], yn[:4], wn[:4])[0].mean()) + float(LG.closed_form(z[2:], yn[2:], wn[2:])[0].mean())
    assert tot["loss"][1] == 2.0
    np.testing.assert_allclose(tot["loss"][0], want2, rtol=1e-6)
    torch.cuda.synchronize()
    assert torch.equal(before["params"], m.params) and torch.equal(before["bn_state"], m.bn_state) and torch.equal(before["grads"], m.grads)
    assert torch.equal(before["packed"], m.packed) and torch.equal(before["metrics"], m._metrics_state)
    assert all(torch.equal(s, t) for s, t in zip(before["slots"], m._slots)) and before["iterations"] == m.iterations


def test_validation_callback_logs_val_loss_and_metrics():
    """The Validation callback on a linear model: val_loss is the mean over its batches of the from-logits loss of the inference-mode
    logits, val_<metric> the compiled metrics -- against evaluation through test_on_batch on the same batches."""
    from multiplanarunet_amd.validation import Validation
    m = _eval_model("bf16", 32)
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(4, 32, 32, 1, generator=g).cuda(), torch.randint(0, 3, (4, 32 * 32, 1), generator=g).to(torch.uint8).cuda(),
                torch.ones(4).cuda()) for _ in range(2)]

    it = iter(batches * 2)
    logs = {}
    Validation(lambda: next(it), 2, 3, logger=quiet, verbose=False).on_epoch_end(m, 0, logs)
    want = np.mean([m.test_on_batch(*b)[0] for b in batches])
    print("Validation logs:", logs, "test_on_batch mean:", want)
    assert np.isfinite(logs["val_loss"]) and set(logs) >= {"val_loss", "val_sparse_categorical_accuracy", "val_sparse_fg_recall"}
    assert abs(logs["val_loss"] - want) <= 0.5001e-4                     # (the callback logs four decimals)


# ---- 12. `mp train` end to end -----------------------------------------------------------------------------------------------------
def test_mp_train_then_predict_on_a_linear_project(tmp_path):
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text(
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 64\n  depth: 3\n"
        "  complexity_factor: 0.0625\n  out_activation: linear\n  biased_output_layer: false\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 64.0\n  batch_size: 8\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: SparseCategoricalCrossentropy\n  loss_kwargs: {from_logits: true}\n  fg_batch_fraction: 0.5\n  bg_value: 1pct\n"
        "  scaler: RobustScaler\n")
    model = mp.entry_func(["train", "--project_dir", str(proj), "--synthetic", "4", "--epochs", "2",
                           "--train_images_per_epoch", "160", "--val_images_per_epoch", "32"])
    assert (proj / "model" / "model_weights.npz").exists()
    assert any(f.startswith("@epoch") for f in os.listdir(proj / "model"))
    log = (proj / "logs" / "training.csv").read_text().strip().splitlines()
    head = log[0].split(",")
    rows = [dict(zip(head, l.split(","))) for l in log[1:]]
    print("mp train, linear output, from_logits:", rows)
    assert len(rows) == 2 and "val_loss" in head
    assert all(np.isfinite(float(r["val_loss"])) and np.isfinite(float(r["loss"])) for r in rows)
    assert float(rows[1]["loss"]) < float(rows[0]["loss"])
    mp.entry_func(["predict", "--project_dir", str(proj), "--synthetic", "1", "--sum_fusion", "--overwrite"])
    lab = np.load(proj / "predictions" / "nii_files" / "toy_5000_PRED.npz")["labels"]
    assert lab.shape == (64, 64, 64) and lab.dtype == np.uint8 and lab.max() <= 2
