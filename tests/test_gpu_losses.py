"""
The train step under the losses of mpunet/evaluate/loss_functions.py (UNet.compile(loss=..., loss_kwargs=...)) on the GPU,
against the f64 restatement tests/loss_ref.py (whose network is oracle/unet_ref.py): the f32 step tensor by tensor, the
loss arithmetic alone in every dtype, both forms of the training head, reproducibility, graph replay, the bf16 step
beside the cross-entropy's, and `mp train` end to end.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as LR                                                                   # noqa: E402
from test_gpu_unet import CFGS, rand_weights, quiet                                      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the five losses, generalized Dice in two type_weights (class_weights "ramp": one weight per class, .2 ... 1.4)
LOSS_CFGS = [("SparseDiceLoss", {"smooth": 1}), ("SparseJaccardDistanceLoss", {"smooth": 1}),
             ("SparseGeneralizedDiceLoss", {"type_weight": "Square"}), ("SparseGeneralizedDiceLoss", {"type_weight": "Simple"}),
             ("SparseFocalLoss", {"gamma": 2, "class_weights": "ramp"}), ("SparseExponentialLogarithmicLoss", {})]
IDS = ["dice", "jaccard", "gdl_square", "gdl_simple", "focal", "explog"]


def _kw(kw, K):
    kw = dict(kw)
    if kw.get("class_weights") == "ramp":
        kw["class_weights"] = [float(v) for v in np.linspace(.2, 1.4, K)]
    return kw


@pytest.mark.parametrize("cfg", CFGS[:2])
@pytest.mark.parametrize("name,kw", LOSS_CFGS, ids=IDS)
def test_f32_train_step_vs_restatement(name, kw, cfg, noise_mult=3, flip_frac=1e-2):
    """test_gpu_unet.test_f32_train_step_vs_oracle with the loss exchanged: same inputs, except that the last image's labels
    omit the last class; same bounds (max(2e-3, 3 * noise) of each gradient tensor's maximum, noise = torch f32 against torch
    f64 of the same graph and loss; its close() rule for the updated weights); no gradient in the channel padding."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    K, C, D, cf, H, W, B = cfg
    kw = _kw(kw, K)
    w = rand_weights(U, K, C, D, cf, seed=5)
    rng = np.random.RandomState(1)
    x = rng.randn(B, H, W, C).astype(np.float32)
    y = rng.randint(0, K, (B, H * W, 1)).astype(np.uint8)
    y[B - 1][y[B - 1] == K - 1] = 0
    sw = np.array([1.0, 0.33, 1.0][:B], np.float32)
    m = UNet(n_classes=K, img_rows=H, img_cols=W, n_channels=C, depth=D, complexity_factor=cf,
             dtype="f32", logger=quiet, flatten_output=True)
    m.set_weights_dict(w)
    m.compile("Adam", name, loss_kwargs=kw)
    ref = LR.train_step(name, kw, w, x, y, sw, depth=D, dtype=torch.float64)
    ref32 = LR.train_step(name, kw, w, x, y, sw, depth=D, dtype=torch.float32)
    probs, loss = m.forward_backward(x, y, sw)
    assert tuple(loss.shape) == (B, 1)
    pn = np.abs(ref32["probs"] - ref["probs"]).max()
    np.testing.assert_allclose(probs.cpu().numpy(), ref["probs"], rtol=0, atol=max(2e-5, 3 * pn))
    got_l = loss.cpu().numpy().reshape(-1)
    print("%s %s: losses %s (f64 %s), logged mean %.7g" % (name, kw, got_l, ref["loss"], float(m.loss_mean().item())))
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


def _ce_closed_form(y, p, w):
    """Keras sparse CE on clipped probabilities (oracle/unet_ref.py keras_sparse_ce) in NumPy f64: per-pixel weighted loss and
    its gradient at the probabilities."""
    B, M, K = p.shape
    q = np.clip(p, LR.EPS, 1 - LR.EPS)
    S = q.sum(-1)
    qy = np.take_along_axis(q, y[..., None], 2)[..., 0]
    oh = (y[..., None] == np.arange(K)).astype(np.float64)
    passm = ((p >= LR.EPS) & (p <= 1 - LR.EPS)).astype(np.float64)
    L = (-np.log(qy) + np.log(S)) * w[:, None]
    g = passm * (-oh / qy[..., None] + 1 / S[..., None]) * w[:, None, None]
    return L, g


@pytest.mark.parametrize("dtype", ("f32", "bf16x3", "bf16"))
def test_loss_arithmetic_on_the_gpus_own_probabilities(dtype):
    """Head only, every dtype: from the probabilities the GPU itself left in the workspace (mpu_unet_workspace_probs_offset),
    recompute in f64 the [B] losses, the logged mean and sum_m dz_mk (the gradient of conv2d/bias). Losses and mean to 1e-5
    relative; the bias gradient to 1e-5 * sum_m |dz_mk| per class (f32 per-pixel arithmetic, f32 chains of a few hundred
    addends, then f64 partials -- as in the cross-entropy kernels, which take the same check on the same bound here). This
    isolates the new arithmetic from the convolutions' bf16 error. cf = 1: bf16 / bf16x3 run the fused training head."""
    from multiplanarunet_amd.unet import UNet
    from multiplanarunet_amd import _lib
    K, H, B, D = 3, 32, 3, 2
    rng = np.random.RandomState(4)
    x = rng.randn(B, H, H, 1).astype(np.float32)
    y = rng.randint(0, K, (B, H * H)).astype(np.uint8)
    y[1][y[1] == K - 1] = 0
    sw = np.array([1.0, 0.33, 2.0], np.float32)
    for name, kw in [("SparseCategoricalCrossentropy", {})] + LOSS_CFGS:
        kw = _kw(kw, K)
        m = UNet(n_classes=K, dim=H, depth=D, complexity_factor=1, dtype=dtype, logger=quiet, flatten_output=True, seed=2)
        w = m.get_weights_dict()
        w["conv2d/kernel"] = w["conv2d/kernel"] * 4.0           # spread the probabilities
        m.set_weights_dict(w)
        m.compile("Adam", name, loss_kwargs=kw)
        _, loss = m.forward_backward(x, y.reshape(B, -1, 1), sw)
        off = int(_lib.load().mpu_unet_workspace_probs_offset(m._h, B))
        p = m._ws[off:off + 4 * B * H * H * K].view(torch.float32).reshape(B, H * H, K).cpu().numpy().astype(np.float64)
        yy = y.astype(np.int64)
        if name == "SparseCategoricalCrossentropy":
            Lpix, g = _ce_closed_form(yy, p, sw.astype(np.float64))
            want_l = Lpix.sum(1)                                # per image: the sum of its per-pixel losses
            got_l = loss.cpu().numpy().astype(np.float64).reshape(B, -1).sum(1)
            want_mean = Lpix.mean()
        else:
            want_l, g = LR.closed_form(name, yy, p, sw.astype(np.float64), **kw)
            got_l = loss.cpu().numpy().astype(np.float64).reshape(-1)
            want_mean = want_l.mean()
        dz = LR.softmax_backward(p, g)
        kind, o, ps, ls = m._tensors["conv2d/bias"]
        got_db = m.grads[o:o + K].cpu().numpy().astype(np.float64)
        want_db, bound = dz.sum((0, 1)), 1e-5 * np.abs(dz).sum((0, 1))
        got_mean = float(m.loss_mean().item())
        print("%-6s %-34s losses rel %.2e  mean rel %.2e  bias-gradient err / sum|dz| %.2e" % (
            dtype, name, np.abs(got_l / want_l - 1).max(), abs(got_mean / want_mean - 1), (np.abs(got_db - want_db) / (bound / 1e-5)).max()))
        np.testing.assert_allclose(got_l, want_l, rtol=1e-5)
        np.testing.assert_allclose(got_mean, want_mean, rtol=1e-5)
        assert (np.abs(got_db - want_db) <= bound).all(), (name, got_db, want_db, bound)


_STEP_SCRIPT = r"""
import sys, json, numpy as np, torch, ctypes as C
sys.path.insert(0, %r)
from multiplanarunet_amd.unet import UNet
from multiplanarunet_amd import _lib
lib = _lib.load()
quiet = lambda *a, **k: None
out, B, K, D, dim, dtype = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
for tag, name, kw in json.loads(sys.argv[7]):
    m = UNet(n_classes=K, dim=dim, n_channels=1, depth=D, complexity_factor=1, dtype=dtype, logger=quiet, flatten_output=True, seed=5)
    w = m.get_weights_dict()
    rng = np.random.RandomState(3)
    for k in w:                                        # gammas of both signs, non-trivial betas
        if k.endswith("/gamma"): w[k] = rng.uniform(-1.5, 1.5, w[k].shape).astype(np.float32)
        if k.endswith("/beta"): w[k] = rng.uniform(-.3, .3, w[k].shape).astype(np.float32)
    m.set_weights_dict(w)
    m.compile("Adam", name, loss_kwargs=kw)
    rng = np.random.RandomState(7)
    x = torch.tensor(rng.randn(B, dim, dim, 1).astype(np.float32), device="cuda")
    yn = rng.randint(0, K, (B, dim * dim, 1)).astype(np.uint8)
    yn[B - 1][yn[B - 1] == K - 1] = 0
    y = torch.tensor(yn, device="cuda")
    sw = torch.tensor(np.where(np.arange(B) %% 2 == 0, 0.4, 1.0).astype(np.float32), device="cuda")
    lib.mpu_schedule_log_enable(1)
    probs, loss = m.forward_backward(x, y, sw, want_loss=True)
    n = lib.mpu_schedule_log_read(None, 0); buf = C.create_string_buffer(int(n) + 1); lib.mpu_schedule_log_read(buf, n + 1)
    lib.mpu_schedule_log_enable(0)
    nh = sum(1 for l in buf.value.decode().splitlines() if "head=1" in l)
    torch.cuda.synchronize()
    g = m.grads.cpu().numpy()
    def grad_of(t):
        kind, off, ps, ls = m._tensors[t]
        return m._from_stored(t, g[off:off + int(np.prod(ps))].reshape(ps), ps, ls)
    np.savez(out + "." + tag + ".npz", probs=probs.float().cpu().numpy(), loss=loss.float().cpu().numpy(), nh=np.int32(nh),
             loss_mean=np.float32(m.loss_mean().item()), state=m.bn_state.cpu().numpy(),
             **{"g:" + k: grad_of(k) for k in m._order if m._tensors[k][0] == 0})
"""


def _run_steps(tmp_path, tag, env, B, K, D, dim, dtype, cfgs):
    f = str(tmp_path / tag)
    jobs = [(i, n, _kw(kw, K)) for i, (n, kw) in zip(IDS, cfgs)] if cfgs is LOSS_CFGS else cfgs
    r = subprocess.run([sys.executable, "-c", _STEP_SCRIPT % ROOT, f, str(B), str(K), str(D), str(dim), dtype, json.dumps(jobs)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return {j[0]: dict(np.load(f + "." + j[0] + ".npz")) for j in jobs}


_rel = lambda u, v: float(np.linalg.norm(u.astype(np.float64) - v) / (np.linalg.norm(v.astype(np.float64)) + 1e-30))


@pytest.mark.parametrize("dtype", ("bf16", "bf16x3"))
def test_fused_and_unfused_training_head_agree_for_every_loss(tmp_path, dtype):
    """test_gpu_unet.test_training_head_without_the_last_post_bn_tensor_equals_the_unfused_chain per loss kind, with its
    bounds: the three head_bn_* passes (which recompute the loss gradient twice) against head_backward_kernel behind
    MPU_HEAD_TRAIN_FUSED=0. Probabilities, losses and moving statistics the same bits; the head's and the last BatchNorm's
    gradients to 1e-2 relative L2, all gradients cosine >= 0.995 (depth 2)."""
    B, K, D, dim = 3, 3, 2, 48
    fused = _run_steps(tmp_path, "fused", {}, B, K, D, dim, dtype, LOSS_CFGS)
    chain = _run_steps(tmp_path, "chain", {"MPU_HEAD_TRAIN_FUSED": "0"}, B, K, D, dim, dtype, LOSS_CFGS)
    last = "upsample_L%d_BN2" % (D - 1)
    for tag in IDS:
        a, b = fused[tag], chain[tag]
        assert int(a["nh"]) == 2 and int(b["nh"]) == 0, (tag, a["nh"], b["nh"])
        assert a["loss"].shape == (B, 1)
        assert np.array_equal(a["probs"], b["probs"]) and np.array_equal(a["loss"], b["loss"]) and np.array_equal(a["state"], b["state"])
        assert abs(float(a["loss_mean"]) - float(b["loss_mean"])) <= 1e-6 * abs(float(b["loss_mean"]))
        tight = {k: _rel(a[k], b[k]) for k in a if k.startswith("g:") and (k[2:].split("/")[0] == last or
                                                                          not any(t in k for t in ("encoder", "bottom", "upsample")))}
        keys = sorted(k for k in a if k.startswith("g:"))
        ga = np.concatenate([a[k].ravel() for k in keys]).astype(np.float64)
        gb = np.concatenate([b[k].ravel() for k in keys]).astype(np.float64)
        cos = float(ga @ gb / np.sqrt((ga @ ga) * (gb @ gb)))
        print("fused head vs chain, %s %s: head / last-BN tensors rel-L2 %s; all gradients cosine %.5f"
              % (dtype, tag, {k[2:]: "%.2e" % v for k, v in tight.items()}, cos))
        assert len(tight) >= 4, list(tight)
        for k, v in tight.items():
            assert v <= 1e-2, (tag, k, v)
        assert cos >= 0.995, (tag, cos)


@pytest.mark.parametrize("name", ("SparseDiceLoss", "SparseExponentialLogarithmicLoss"))
def test_two_passes_on_identical_inputs_are_bit_identical(name):
    """configs[1] size (B = 16, 128 x 128, depth 4, bf16): gradients and losses of two forward_backward calls, bit for bit."""
    from multiplanarunet_amd.unet import UNet
    B, H, K = 16, 128, 3
    rng = np.random.RandomState(9)
    x = torch.tensor(rng.randn(B, H, H, 1).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, K, (B, H * H, 1)).astype(np.uint8), device="cuda")
    sw = torch.tensor(rng.uniform(.3, 1.5, B).astype(np.float32), device="cuda")
    m = UNet(n_classes=K, dim=H, depth=4, dtype="bf16", logger=quiet, flatten_output=True, seed=1)
    m.compile("Adam", name)
    state = m.bn_state.clone()
    _, l0 = m.forward_backward(x, y, sw)
    g0, l0, m0 = m.grads.clone(), l0.clone(), m.loss_mean().clone()
    m.bn_state.copy_(state)
    _, l1 = m.forward_backward(x, y, sw)
    assert tuple(l1.shape) == (B, 1) and torch.isfinite(l1).all() and torch.isfinite(m.grads).all() and float(m.grads.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(m0, m.loss_mean()) and torch.equal(g0, m.grads)


def test_graph_replay_equals_the_eager_loop_generalized_dice_bf16():
    """The form `mp train` runs: 20 replays of make_graphed_train_step against 20 train_step calls from the same start --
    bit-identical parameters, equal loss sums."""
    from multiplanarunet_amd.unet import UNet
    rng = np.random.RandomState(3)
    B, H, K, N = 4, 32, 3, 20
    x = torch.tensor(rng.randn(B, H, H, 1).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, K, (B, H * H, 1)).astype(np.uint8), device="cuda")
    sw = torch.tensor([1.0, 0.33, 1.0, 2.0], device="cuda")
    mk = lambda: UNet(n_classes=K, dim=H, depth=2, complexity_factor=1, dtype="bf16", logger=quiet, seed=0, flatten_output=True)
    a, b = mk(), mk()
    for m in (a, b):
        m.compile("Adam", "SparseGeneralizedDiceLoss", loss_kwargs={"type_weight": "Square"}, optimizer_kwargs={"lr": 1e-3})
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


def test_bf16_step_is_as_close_to_the_f32_step_as_the_cross_entropy_one(tmp_path):
    """Per gradient tensor, the relative L2 error of the bf16 step against the SAME build's f32 step on the same inputs, for each
    loss, beside the same figure for the cross-entropy (whose path is unchanged and validated by the existing tests). Each new
    loss's median over tensors must be <= 2 x the cross-entropy's median: parity is the expectation; 2 x is slack for the
    different dynamic range of the region losses' dz, not a target."""
    B, K, D, dim = 4, 3, 2, 64
    jobs = [("ce", "SparseCategoricalCrossentropy", {})] + [(i, n, _kw(kw, K)) for i, (n, kw) in zip(IDS, LOSS_CFGS)]
    lo = _run_steps(tmp_path, "bf16", {}, B, K, D, dim, "bf16", jobs)
    hi = _run_steps(tmp_path, "f32", {}, B, K, D, dim, "f32", jobs)
    med = {}
    for tag, _, _ in jobs:
        errs = {k[2:]: _rel(lo[tag][k], hi[tag][k]) for k in lo[tag] if k.startswith("g:")}
        med[tag] = float(np.median(list(errs.values())))
        print("bf16 vs f32 step, %-10s median %.3e  worst %.3e (%s)" % (tag, med[tag], max(errs.values()), max(errs, key=errs.get)))
    for tag in IDS:
        assert med[tag] <= 2 * med["ce"], (tag, med[tag], med["ce"])


def test_focal_loss_with_class_weights_learns():
    """60 steps of SparseFocalLoss(gamma=2, class_weights=[.2, 1, 1]) on a fixed batch: the mean of the last 10 logged losses is
    below the mean of the first 10."""
    from multiplanarunet_amd.unet import UNet
    rng = np.random.RandomState(0)
    B, H = 8, 32
    x = rng.randn(B, H, H, 1).astype(np.float32)
    y = ((x[..., 0] > 0).astype(np.uint8) + (x[..., 0] > 1).astype(np.uint8)).reshape(B, -1, 1)
    m = UNet(n_classes=3, dim=H, depth=2, complexity_factor=0.25, dtype="bf16", logger=quiet, seed=0, flatten_output=True)
    m.compile("Adam", "SparseFocalLoss", optimizer_kwargs=dict(lr=1e-3), loss_kwargs={"gamma": 2, "class_weights": [.2, 1, 1]})
    hist = [m.train_on_batch(x, y) for _ in range(60)]
    assert np.isfinite(hist).all() and np.mean(hist[-10:]) < np.mean(hist[:10]), (hist[:10], hist[-10:])


def test_mp_train_with_the_dice_loss(tmp_path):
    """`mp train` on a toy project (tests/test_gpu_cli.py's kind) with loss: SparseDiceLoss, loss_kwargs: {smooth: 1}, two
    epochs: the logged loss lies in (0, 1) and falls, checkpoints are written."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text(
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 64\n  depth: 3\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 64.0\n  batch_size: 8\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: \"SparseDiceLoss\"\n  loss_kwargs: {smooth: 1}\n  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n")
    model = mp.entry_func(["train", "--project_dir", str(proj), "--synthetic", "4", "--epochs", "2",
                           "--train_images_per_epoch", "160", "--val_images_per_epoch", "32"])
    assert (proj / "model" / "model_weights.npz").exists()
    assert any(f.startswith("@epoch") for f in os.listdir(proj / "model"))
    log = (proj / "logs" / "training.csv").read_text().strip().splitlines()
    col = log[0].split(",").index("loss")
    losses = [float(l.split(",")[col]) for l in log[1:]]
    print("mp train, SparseDiceLoss: logged loss per epoch", losses)
    assert len(losses) == 2 and 0 < losses[1] < losses[0] < 1, losses
