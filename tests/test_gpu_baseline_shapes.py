"""
The BASELINE.json configurations at their REAL shapes ("no BASELINE config is tested at its real shape").

configs[1]  depth-4 / 64-filter U-Net on 128x128 slices:
              * dtype="f32" logits vs the f64 oracle <= 1e-4 (north-star tolerance) at the full network size;
              * the benchmarked mode (bf16, B=16) per-tensor against the matched-rounding model of the storage mode
                (oracle/unet_ref.py: bf16_matched_step) and against the f32 kernels on bf16-rounded weights, with the
                kernel schedules the dispatcher took recorded (mpu_schedule_log_*) and asserted -- the same
                schedules bench.py times;
configs[2]  6-view predict+fuse of a 256^3 volume              -- size-independent properties at full size
configs[3]  train step B=32 of 256x256 (single-GPU share of it) -- properties at full size
configs[4]  6-view predict+fuse of a 512^3 x 2 volume, K=5     -- properties at full size
plus the end-to-end tolerance of the north star in the benchmarked dtype: a trained toy net, 6-view predict+fuse
in bf16, Dice delta <= 1e-3 against the f64 oracle pipeline with every class present.
"""
import ctypes as C
import os
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
quiet = lambda *a, **k: None

VIEWS6 = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0.707], [-0.6, 0.64, 0.48], [0.7, -0.5, 0.5]], float)


def _schedule_log(fn):
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    lib.mpu_schedule_log_enable(1)
    try:
        out = fn()
        n = lib.mpu_schedule_log_read(None, 0)
        buf = C.create_string_buffer(int(n) + 1)
        lib.mpu_schedule_log_read(buf, n + 1)
    finally:
        lib.mpu_schedule_log_enable(0)
    return out, [l.split() for l in buf.value.decode().splitlines()]


def _grad(m, g, name):
    kind, off, ps, ls = m._tensors[name]
    return m._from_stored(name, g[off:off + int(np.prod(ps))].reshape(ps), ps, ls)


def _cfg1_weights(U, seed):
    """glorot kernels, random biases / BN parameters and moving statistics, one negative gamma per BN."""
    w = U.init_weights(3, 1, 4, 1, seed=seed)
    rng = np.random.RandomState(seed + 1)
    for k in w:
        v = k.split("/")[1]
        if v == "bias":
            w[k] = rng.uniform(-.1, .1, w[k].shape).astype(np.float32)
        elif v == "gamma":
            w[k] = rng.uniform(.5, 1.5, w[k].shape).astype(np.float32)
            w[k][0] = -0.8
        elif v in ("beta", "moving_mean"):
            w[k] = rng.uniform(-.3, .3, w[k].shape).astype(np.float32)
        elif v == "moving_variance":
            w[k] = rng.uniform(.5, 2., w[k].shape).astype(np.float32)
    return w


def test_cfg1_network_f32_logits_vs_f64_oracle():
    """configs[1] network (depth 4, complexity_factor 1, 128x128x1, K=3), inference and training-mode forward."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    w = _cfg1_weights(U, 3)
    x = np.random.RandomState(0).randn(2, 128, 128, 1).astype(np.float32)
    m = UNet(n_classes=3, dim=128, n_channels=1, depth=4, complexity_factor=1, out_activation="linear", dtype="f32",
             logger=quiet)
    assert m.count_params() == 31046339                          # SURVEY: 31,030,723 conv + 15,616 BN
    m.set_weights_dict(w)
    p64 = U.to_torch(w, torch.float64)
    xt = torch.tensor(x, dtype=torch.float64)
    got = m._forward(m._as_input(x), training=False).cpu().numpy()
    ref = U.forward(p64, xt, 4, False, "linear").numpy()
    err = np.abs(got - ref).max()
    print("cfg1 f32 inference logits: max |err| = %.3g (|logits| max %.3g)" % (err, np.abs(ref).max()))
    assert err <= 1e-4, err
    got_t = m._forward(m._as_input(x), training=True).cpu().numpy()
    ref_t = U.forward(p64, xt, 4, True, "linear").numpy()
    ref32 = U.forward(U.to_torch(w, torch.float32), torch.tensor(x), 4, True, "linear").numpy()
    noise = np.abs(ref32 - ref_t).max()
    err_t = np.abs(got_t - ref_t).max()
    print("cfg1 f32 train-mode logits: max |err| = %.3g (torch-f32 noise floor %.3g)" % (err_t, noise))
    assert err_t <= max(1e-4, 3 * noise), (err_t, noise)


def test_cfg1_network_split_bf16_logits_vs_f64_oracle():
    """dtype "bf16x3" -- f32 storage, three bf16 MFMAs per product -- on the configs[1] network against the f64
    oracle: the north-star logits tolerance (1e-4) at bf16-class matrix rates; the f32 mode (exact-f32 MFMA, 1/16 rate) is 6e-7,
    the bf16 mode ~1e-2. Inference and train-mode forward, then one train step: gradients of every tensor against the f64 oracle
    at the f32 test's bound."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    w = _cfg1_weights(U, 3)
    x = np.random.RandomState(0).randn(2, 128, 128, 1).astype(np.float32)
    m = UNet(n_classes=3, dim=128, n_channels=1, depth=4, complexity_factor=1, out_activation="linear", dtype="bf16x3",
             logger=quiet)
    assert m.split_bf16 and m.dtype == torch.float32
    m.set_weights_dict(w)
    p64 = U.to_torch(w, torch.float64)
    xt = torch.tensor(x, dtype=torch.float64)
    got = m._forward(m._as_input(x), training=False).cpu().numpy()
    ref = U.forward(p64, xt, 4, False, "linear").numpy()
    err = np.abs(got - ref).max()
    print("cfg1 bf16x3 inference logits: max |err| = %.3g (|logits| max %.3g)" % (err, np.abs(ref).max()))
    assert err <= 1e-4, err
    got_t = m._forward(m._as_input(x), training=True).cpu().numpy()
    ref_t = U.forward(p64, xt, 4, True, "linear").numpy()
    ref32 = U.forward(U.to_torch(w, torch.float32), torch.tensor(x), 4, True, "linear").numpy()
    noise = np.abs(ref32 - ref_t).max()
    err_t = np.abs(got_t - ref_t).max()
    print("cfg1 bf16x3 train-mode logits: max |err| = %.3g (torch-f32 noise floor %.3g)" % (err_t, noise))
    # batch statistics over TWO slices (128 pixels per channel at the bottom level) amplify every rounding: the f32 graph
    # itself sits at `noise` here; a product of this mode carries ~256 f32 rounding units
    assert err_t <= max(1e-3, 256 * noise), (err_t, noise)


def test_cfg1_bf16_train_step_per_tensor_and_dispatch():
    """The benchmarked workload itself: B=16 bf16 slices of 128x128 through the depth-4 / 64-filter network: the
    dispatch taken is asserted; inference probabilities are held tightly to the matched-rounding model of the
    storage mode (oracle/unet_ref.py: bf16_matched_forward); every gradient tensor of the train step is held to
    the model's own noise floor (see bf16_matched_step: the graph amplifies perturbations ~45x, so any two correct
    bf16 evaluations differ by that much) and the head-side tensors to 2e-2."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    B = 16
    w = _cfg1_weights(U, 11)
    rng = np.random.RandomState(4)
    x = rng.randn(B, 128, 128, 1).astype(np.float32)
    y = (rng.randint(0, 3, (B, 128, 128)) * (rng.rand(B, 128, 128) < 0.5)).astype(np.uint8).reshape(B, -1, 1)
    sw = np.where(np.arange(B) % 3 == 0, 0.33, 1.0).astype(np.float32)
    m = UNet(n_classes=3, dim=128, n_channels=1, depth=4, complexity_factor=1, flatten_output=True, dtype="bf16",
             logger=quiet)
    m.set_weights_dict(w)
    (probs, loss), log = _schedule_log(lambda: m.forward_backward(x, y, sw))
    g = m.grads.cpu().numpy()
    assert np.isfinite(g).all() and torch.isfinite(loss).all()
    conv = [l for l in log if l[0] == "conv"]
    wg = [l for l in log if l[0] == "wgrad"]
    scheds = lambda ls: {k: sum(1 for l in ls if l[1] == k) for k in sorted({l[1] for l in ls})}
    print("cfg1 dispatch: conv", scheds(conv), "wgrad", scheds(wg))
    assert len(conv) == 47 and len(wg) == 22, (len(conv), len(wg))     # 22 forward + 25 data-gradient launches; 22 wgrads
    assert "regs" not in scheds(conv) and "regs" not in scheds(wg)      # no register-staged fallback on the bench path
    assert scheds(conv).get("c8") == 1 and scheds(wg).get("c8") == 1    # first layer kernels
    assert set(scheds(conv)) >= {"c8", "ws", "halo", "pipe"} and set(scheds(wg)) >= {"c8", "taps", "glds"}
    deep = scheds(conv).get("pipe", 0) + scheds(conv).get("deepk", 0) + scheds(conv).get("deep", 0)
    assert deep >= 14, scheds(conv)                                     # the deep levels: conv_pipe, and since round 5 ...
    assert scheds(conv).get("deepk", 0) >= 6, scheds(conv)              # ... conv_deepk for the 3x3 layers on the 16 x 16 maps

    # --- inference mode (well conditioned: BatchNorm with moving statistics): tight bound against the matched model
    m.flatten_output = False
    xi = x[:4]
    li = U.bf16_matched_forward(w, xi, depth=4, out_activation="softmax")
    gi = m.predict(xi, batch_size=4)
    di = np.abs(gi - li)
    print("cfg1 bf16 inference probs vs matched model: max %.3g mean %.3g" % (di.max(), di.mean()))
    assert di.max() <= 1e-2 and di.mean() <= 3e-3            # ~one bf16 ulp of the last stored activation

    # --- training step: two evaluations of the matched-rounding model (f32 / f64 arithmetic, same rounding
    # points) give the noise floor of the storage mode per tensor; the kernels must sit within 2x of it
    # (+ 1e-2 absolute), and agree in norm to 15 %. Head-side tensors (not reached by the chaos) are tight.
    r32 = U.bf16_matched_step(w, x, y, sw, depth=4, dtype=torch.float32)
    r64 = U.bf16_matched_step(w, x, y, sw, depth=4, dtype=torch.float64)
    pg = probs.cpu().numpy().reshape(r32["probs"].shape)
    floor_p = np.abs(r32["probs"] - r64["probs"]).mean()
    err_p = min(np.abs(pg - r32["probs"]).mean(), np.abs(pg - r64["probs"]).mean())
    print("cfg1 bf16 train probs: mean |hip - model| %.3g, model noise floor %.3g" % (err_p, floor_p))
    assert err_p <= 2 * floor_p + 1e-3
    rel = lambda a, b: float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
    worst = ("", 0.0, 0.0)
    projs = []
    for name, g64 in r64["grads"].items():
        a, g32_ = _grad(m, g, name).astype(np.float64), r32["grads"][name]
        floor = rel(g32_, g64)
        err = min(rel(a, g64), rel(a, g32_))
        ratio = np.linalg.norm(a) / (0.5 * (np.linalg.norm(g64) + np.linalg.norm(g32_)) + 1e-30)
        if err - 2 * floor > worst[1] - 2 * worst[2]:
            worst = (name, err, floor)
        assert err <= 2 * floor + 1e-2, (name, err, floor)
        assert 0.85 <= ratio <= 1.18, (name, ratio)
        # scale of the tensor: the projection coefficient <a, g> / <g, g> of a = s * g + noise is s up to noise / sqrt(n) -- unlike
        # the norm ratio it does not grow with the (chaotic) noise, so it is held much tighter (a kernel wrong in SCALE by a few
        # per cent on one deep tensor fails here even where the rel-L2 floor is tens of per cent)
        proj = float(np.vdot(a, g64) / (np.vdot(g64, g64) + 1e-300))
        proj_floor = abs(float(np.vdot(g32_, g64) / (np.vdot(g64, g64) + 1e-300)) - 1.0)
        projs.append((abs(proj - 1.0) - 2 * proj_floor, name, proj, proj_floor, a.size))
    print("cfg1 bf16 grads vs matched model: tightest margin at %s: rel-L2 %.3g (noise floor %.3g)" % worst)
    projs.sort(reverse=True)
    print("cfg1 bf16 grads: projection coefficient furthest from 1 (beyond twice the model's own): " +
          ", ".join("%s %.4f (model %.4f)" % (n_, p_, f_) for _, n_, p_, f_, _n in projs[:4]))
    big = [t for t in projs if t[4] >= 4096]                 # the kernels (>= 4096 elements: the noise averages out)
    print("   ... among the %d tensors of >= 4096 elements: " % len(big) +
          ", ".join("%s %.4f (model %.4f)" % (n_, p_, f_) for _, n_, p_, f_, _n in big[:3]))
    for _, n_, p_, f_, _n in big:
        assert abs(p_ - 1.0) <= 0.05 + 2 * f_, (n_, p_, f_)
    for name in ("conv2d/kernel", "conv2d/bias", "upsample_L3_BN2/gamma", "upsample_L3_BN2/beta"):
        a = _grad(m, g, name).astype(np.float64)
        print("   %-24s rel-L2 vs model %.3g (floor %.3g)" % (name, rel(a, r64["grads"][name]), rel(r32["grads"][name], r64["grads"][name])))
        assert rel(a, r64["grads"][name]) <= 2e-2, name


def test_bf16_six_view_pipeline_dice_delta_vs_f64_oracle():
    """North-star end-to-end tolerance in the benchmarked dtype: train a toy net (800 Adam steps on sampled planes),
    6-view predict+fuse of a 64^3 volume with the bf16 kernels, and the same weights through the f64 oracle
    pipeline (oracle geometry + oracle U-Net + FusionLayer): per-class Dice against the ground truth differs by
    <= 1e-3, every class present in both (mpunet/evaluate/metrics.py:26-52, mpunet/bin/predict.py:294-366)."""
    from multiplanarunet_amd.unet import UNet
    from multiplanarunet_amd.fusion_model import FusionModel
    from multiplanarunet_amd.interpolation import dice_all
    from multiplanarunet_amd.predict import multi_view_predict
    from multiplanarunet_amd.data import make_toy_volume, as_volume, TrainSampler
    from oracle import unet_ref as U
    from oracle import geometry as G
    K, D, depth, cf = 3, 64, 3, 0.0625
    def toy(seed):
        """background / ellipsoid / box with SIZEABLE structures (>= 8000 voxels each): a Dice delta of 1e-3 then
        means a real disagreement, not a handful of boundary voxels of a tiny object."""
        rng = np.random.RandomState(seed)
        g = np.mgrid[:D, :D, :D].astype(np.float32)
        c1 = D * (0.30 + 0.08 * rng.rand(3)); r1 = D * (0.19 + 0.04 * rng.rand(3))
        c2 = D * (0.66 + 0.06 * rng.rand(3)); h2 = D * (0.15 + 0.03 * rng.rand(3))
        lab = np.zeros((D, D, D), np.uint8)
        lab[(((g[0] - c1[0]) / r1[0]) ** 2 + ((g[1] - c1[1]) / r1[1]) ** 2 + ((g[2] - c1[2]) / r1[2]) ** 2) <= 1] = 1
        lab[(abs(g[0] - c2[0]) < h2[0]) & (abs(g[1] - c2[1]) < h2[1]) & (abs(g[2] - c2[2]) < h2[2])] = 2
        img = 0.3 * np.sin(g[0] / D * 3) + 0.2 * np.cos(g[1] / D * 5) + 0.05 * rng.randn(D, D, D)
        img = (img + 0.8 * (lab == 1) + 1.5 * (lab == 2))[..., None].astype(np.float32)
        assert np.bincount(lab.ravel(), minlength=K).min() >= 8000
        return img, lab, np.eye(4)
    vols = []
    for s in range(3):
        img, lab, aff = toy(40 + s)
        vols.append((img, lab, as_volume(img, lab, aff, "1pct", "RobustScaler", "cuda", "toy%d" % s)))
    m = UNet(n_classes=K, dim=D, depth=depth, complexity_factor=cf, flatten_output=True, dtype="bf16", logger=quiet, seed=0)
    m.compile("Adam", "SparseCategoricalCrossentropy", optimizer_kwargs=dict(lr=2e-3))
    tr = TrainSampler([v for _, _, v in vols[:2]], VIEWS6, D, float(D), 8, K, noise_sd=0.1, seed=1)
    first = last = None
    for it in range(800):                                       # (BatchNorm momentum 0.99: the moving statistics need
        x, y, w = tr()                                          #  several hundred steps to catch up with the weights)
        l = float(m.train_step(x, y, w).mean().item())
        first = l if first is None else first
        last = l
    assert last < 0.5 * first, (first, last)
    img, lab, vol = vols[2]                                     # held-out volume
    rng = np.random.RandomState(0)
    Wf = rng.uniform(.7, 1.3, (6, K)).astype(np.float32)
    bf = rng.uniform(-.05, .05, (1, K)).astype(np.float32)
    fm = FusionModel(6, K, verbose=False)
    fm.set_weights([Wf, bf])
    m.flatten_output = False
    _, got = multi_view_predict(m, vol, VIEWS6, D, float(D), fm, batch_size=None, want_probs=False)
    got = got.cpu().numpy()
    wts = m.get_weights_dict()
    c, s = vol.scaler
    _, ref_l, _ = G.multi_view_predict(img, np.eye(4), VIEWS6, D, float(D),
                                       lambda X: U.predict(wts, X, depth=depth, dtype=torch.float64), Wf, bf,
                                       bg_value=vol.bg_value, center=c, scale=s)
    d_hip = dice_all(lab, got, n_classes=K, ignore_zero=False)
    d_ref = dice_all(lab, ref_l, n_classes=K, ignore_zero=False)
    d_x = dice_all(ref_l, got, n_classes=K, ignore_zero=False)
    print("bf16 6-view pipeline: dice vs truth hip %s oracle %s | hip vs oracle %s | differing voxels %.2e"
          % (np.round(d_hip, 5), np.round(d_ref, 5), np.round(d_x, 5), (got != ref_l).mean()))
    for arr in (lab, got, ref_l):
        assert set(np.unique(arr)) == set(range(K))             # every class present everywhere: no NaN Dice
    assert np.all(d_ref[1:] > 0.85), d_ref                      # the net has learned the task (a crisp decision surface)
    assert np.abs(d_hip - d_ref).max() <= 1e-3, (d_hip, d_ref)


def test_real_network_bf16_six_view_dice_delta_vs_oracle():
    """the north-star Dice tolerance on the REAL network -- depth 4, 64 base filters (31 M parameters), dim 128 --
    not on a toy: 1300 Adam steps of 16 sampled planes on two 128^3 volumes (every class >= 2 % of the voxels), then the held-out
    volume through the bf16 6-view predict + fuse on the GPU and through the oracle pipeline with the SAME weights (NumPy geometry
    restatement, torch-CPU f32 U-Net, FusionLayer; mpunet/bin/predict.py:294-366, evaluate/metrics.py:26-52). Per-class Dice
    against the ground truth differs by <= 1e-3."""
    import time
    from multiplanarunet_amd.unet import UNet
    from multiplanarunet_amd.fusion_model import FusionModel
    from multiplanarunet_amd.interpolation import dice_all
    from multiplanarunet_amd.predict import multi_view_predict
    from multiplanarunet_amd.data import as_volume, TrainSampler
    from oracle import unet_ref as U
    from oracle import geometry as G
    K, D, depth, cf = 3, 128, 4, 1

    def toy(seed):
        rng = np.random.RandomState(seed)
        g = np.mgrid[:D, :D, :D].astype(np.float32)
        c1 = D * (0.30 + 0.08 * rng.rand(3)); r1 = D * (0.19 + 0.04 * rng.rand(3))
        c2 = D * (0.66 + 0.06 * rng.rand(3)); h2 = D * (0.15 + 0.03 * rng.rand(3))
        lab = np.zeros((D, D, D), np.uint8)
        lab[(((g[0] - c1[0]) / r1[0]) ** 2 + ((g[1] - c1[1]) / r1[1]) ** 2 + ((g[2] - c1[2]) / r1[2]) ** 2) <= 1] = 1
        lab[(abs(g[0] - c2[0]) < h2[0]) & (abs(g[1] - c2[1]) < h2[1]) & (abs(g[2] - c2[2]) < h2[2])] = 2
        img = 0.3 * np.sin(g[0] / D * 3) + 0.2 * np.cos(g[1] / D * 5) + 0.05 * rng.randn(D, D, D)
        img = (img + 0.8 * (lab == 1) + 1.5 * (lab == 2))[..., None].astype(np.float32)
        assert np.bincount(lab.ravel(), minlength=K).min() >= 0.02 * D ** 3
        return img, lab, np.eye(4)
    vols = []
    for s in range(3):
        img, lab, aff = toy(140 + s)
        vols.append((img, lab, as_volume(img, lab, aff, "1pct", "RobustScaler", "cuda", "toy%d" % s)))
    m = UNet(n_classes=K, dim=D, depth=depth, complexity_factor=cf, flatten_output=True, dtype="bf16", logger=quiet, seed=0)
    assert m.count_params() == 31046339
    m.compile("Adam", "SparseCategoricalCrossentropy", optimizer_kwargs=dict(lr=5e-4))
    tr = TrainSampler([v for _, _, v in vols[:2]], VIEWS6, D, float(D), 16, K, noise_sd=0.1, seed=1)
    first = last = None
    NSTEP = 700 + 600
    for it in range(NSTEP):
        if it == 700:            # the last 600 steps at a 25x smaller rate: the weights barely move, and BatchNorm's moving statistics
            m.optimizer_kwargs["lr"] = 2e-5     # (momentum 0.99) catch up with them -- inference then sees what training saw
        x, y, w = tr()
        l = m.train_step(x, y, w)
        if it == 0 or it == NSTEP - 1:
            v = float(l.mean().item())
            first = v if first is None else first
            last = v
    assert last < 0.3 * first, (first, last)
    img, lab, vol = vols[2]                                     # held-out volume
    rng = np.random.RandomState(0)
    Wf = rng.uniform(.7, 1.3, (6, K)).astype(np.float32)
    bf = rng.uniform(-.05, .05, (1, K)).astype(np.float32)
    fm = FusionModel(6, K, verbose=False)
    fm.set_weights([Wf, bf])
    m.flatten_output = False
    _, got = multi_view_predict(m, vol, VIEWS6, D, float(D), fm, batch_size=None, want_probs=False)
    got = got.cpu().numpy()
    wts = m.get_weights_dict()
    c, s = vol.scaler
    t0 = time.perf_counter()

    def net(X):                                                  # torch-CPU f32, 37 planes at a time
        return np.concatenate([U.predict(wts, X[i:i + 37], depth=depth, dtype=torch.float32) for i in range(0, X.shape[0], 37)])
    _, ref_l, _ = G.multi_view_predict(img, np.eye(4), VIEWS6, D, float(D), net, Wf, bf, bg_value=vol.bg_value, center=c, scale=s)
    t_ref = time.perf_counter() - t0
    d_hip = dice_all(lab, got, n_classes=K, ignore_zero=False)
    d_ref = dice_all(lab, ref_l, n_classes=K, ignore_zero=False)
    d_x = dice_all(ref_l, got, n_classes=K, ignore_zero=False)
    print("REAL network (depth 4, 64 filters, dim 128) bf16 6-view pipeline on a 128^3 volume: loss %.3f -> %.3f; dice vs truth hip %s "
          "oracle %s | hip vs oracle %s | differing voxels %.2e | oracle pipeline %.0f s of CPU"
          % (first, last, np.round(d_hip, 5), np.round(d_ref, 5), np.round(d_x, 5), (got != ref_l).mean(), t_ref))
    for arr in (lab, got, ref_l):
        assert set(np.unique(arr)) == set(range(K))
    assert np.all(d_ref[1:] > 0.85), d_ref
    assert np.abs(d_hip - d_ref).max() <= 1e-3, (d_hip, d_ref)


def _predict_properties(D, C_, K, dim_batch=None):
    """6-view predict+fuse at full size: labels < K, deterministic, fused kernel == accumulate + finalize path
    (sum_fusion: bitwise-comparable pre-activations; FusionLayer: <= 1e-4 of voxels at fp32 ties)."""
    from multiplanarunet_amd.unet import UNet
    from multiplanarunet_amd.fusion_model import FusionModel
    from multiplanarunet_amd.interpolation import Volume, ViewGeometry, sample_view, map_accumulate, fusion_finalize
    from multiplanarunet_amd.predict import multi_view_predict
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    image = torch.randn((D, D, D, C_), generator=g, device="cuda")
    vol = Volume(image, None, np.eye(4), bg_value=[0.0] * C_, scaler=(np.zeros(C_), np.full(C_, 1.3)), device="cuda")
    m = UNet(n_classes=K, dim=D, n_channels=C_, depth=4, complexity_factor=1, dtype="bf16", logger=quiet, seed=0)
    rng = np.random.RandomState(1)
    # A random-weight net in inference mode (moving statistics 0 / 1) collapses to one class wherever a view is in bounds
    # (histograms [5.8 M, 11 M, 0] -- two geometric regions), which makes "fused == accumulate" a two-class
    # statement. (1) Let the BatchNorm moving statistics converge to the statistics of sampled planes (train-mode
    # forwards, momentum 0.99), so that the features vary over the image; (2) give the 1x1 head a strong random kernel;
    # (3) calibrate the FUSION bias on the whole pipeline until every class holds a sizeable share of the voxels.
    cal = ViewGeometry(VIEWS6[3], D, float(D), "same+20")
    cal.offsets = cal.offsets[cal.n_planes // 2 - 2:cal.n_planes // 2 + 2]; cal.n_planes = 4
    Xc, _ = sample_view(vol, cal, want_labels=False)
    for _ in range(400):
        m._forward(m._as_input(Xc), training=True)
    del Xc
    wd = m.get_weights_dict()
    m.set_weights_dict({"conv2d/kernel": rng.randn(*wd["conv2d/kernel"].shape).astype(np.float32) * 0.7})
    fm = FusionModel(6, K, verbose=False)
    Wf, bf = rng.uniform(.5, 1.5, (6, K)).astype(np.float32), rng.uniform(-.1, .1, (1, K)).astype(np.float32)
    fm.set_weights([Wf, bf])
    for _ in range(8):
        _, lab = multi_view_predict(m, vol, VIEWS6, D, float(D), fm, want_probs=False)
        frac = np.maximum(torch.bincount(lab.reshape(-1).long(), minlength=K).float().cpu().numpy() / D ** 3, 1e-4)
        if frac.min() >= 0.08:
            break
        bf = (bf + 0.6 * np.log((1.0 / K) / frac)[None]).astype(np.float32)
        fm.set_weights([Wf, bf])
    t = {}
    _, lab = multi_view_predict(m, vol, VIEWS6, D, float(D), fm, want_probs=False, timings=t)
    assert tuple(lab.shape) == (D, D, D) and lab.dtype == torch.uint8
    hist = torch.bincount(lab.reshape(-1).long(), minlength=K)
    assert int(hist.sum()) == D ** 3 and hist.numel() == K and int(lab.max()) < K
    assert int(hist.min()) >= 0.02 * D ** 3, hist.tolist()      # every class holds >= 2 % of the voxels (calibrated net)
    _, lab2 = multi_view_predict(m, vol, VIEWS6, D, float(D), fm, want_probs=False)
    assert torch.equal(lab, lab2)                                # deterministic
    # plane-chunked accumulate path (the multi-GPU exchange's local part) == the fused kernel
    z = torch.zeros((D, D, D, K), dtype=torch.float32, device="cuda")
    P = D + 20
    cuts = [0, P // 3, P]
    for vi, view in enumerate(VIEWS6):
        geom = ViewGeometry(view, D, float(D), "same+20")
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            sub = ViewGeometry(view, D, float(D), "same+20")
            sub.offsets = geom.offsets[lo:hi]; sub.n_planes = hi - lo
            Xs, _ = sample_view(vol, sub, want_labels=False)
            pred = m.predict(Xs, batch_size=None)
            map_accumulate(vol, pred, (geom.real_axis, geom.real_axis, geom.offsets), geom.inv_basis, fm.W[vi],
                           lo, hi, owns_oob=(lo == 0), z=z)
            del Xs, pred
    _, lab3 = fusion_finalize(z, fm.b, want_probs=False)
    # Both paths take the SAME back-mapping decision for every voxel (integer work: exact); their f32 sums over the views
    # differ in contraction only, so a label may differ solely where the two largest fused scores tie within float noise.
    zb = z + torch.as_tensor(fm.b, device=z.device).reshape(1, 1, 1, K)
    top2 = zb.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    diff = lab3 != lab
    outside = diff & (margin > 8e-6 * top2[..., 0].abs().clamp_min(1.0))
    n_diff, n_out = int(diff.sum().item()), int(outside.sum().item())
    print("predict %d^3 x %d K=%d: %s; fused vs accumulate path: %d labels differ, %d outside the float tie band; label histogram %s"
          % (D, C_, K, {k: round(v, 1) for k, v in t.items()}, n_diff, n_out, hist.tolist()))
    assert n_out == 0 and n_diff <= 1e-5 * D ** 3
    del zb, top2, margin, diff, outside
    return t


def test_cfg2_predict_fuse_256_cubed_properties():
    """configs[2]: 6-view predict+fuse on one 256x256x256x1 volume (276 planes per view, K=3)."""
    _predict_properties(256, 1, 3)


def test_cfg4_predict_fuse_512_cubed_two_channels_properties():
    """configs[4] on one GPU: 512x512x512x2 volume, 5 classes, 532 planes of 512x512 per view."""
    _predict_properties(512, 2, 5)


def test_cfg3_train_step_batch32_256_properties():
    """configs[3] (global batch 32 of 256x256) as one GPU's workload: the loss on a fixed batch is finite and
    decreasing over the steps, two identically seeded models stay bitwise identical (deterministic kernels: the
    BatchNorm sums are integer atomics, exact in any order), BN moving statistics move. Sums past 2^63 fixed-point
    units at this shape: tests/test_gpu_accumulator_range.py."""
    from multiplanarunet_amd.unet import UNet
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    B, H = 32, 256
    x = torch.randn((B, H, H, 1), generator=g, device="cuda")
    y = ((x[..., 0] > 0).to(torch.uint8) + (x[..., 0] > 1).to(torch.uint8)).reshape(B, -1, 1).contiguous()
    w = torch.ones(B, device="cuda")
    ms = []
    for rep in range(2):
        m = UNet(n_classes=3, dim=H, n_channels=1, depth=4, complexity_factor=1, flatten_output=True, dtype="bf16",
                 logger=quiet, seed=0)
        m.compile("Adam", "SparseCategoricalCrossentropy", optimizer_kwargs=dict(lr=1e-4))
        losses = [float(m.train_step(x, y, w).mean().item()) for _ in range(6 if rep == 0 else 2)]
        ms.append((m, losses))
    losses = ms[0][1]
    print("cfg3 B=32 256^2 losses:", np.round(losses, 4))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    m = ms[0][0]
    assert torch.isfinite(m.params).all() and torch.isfinite(m.bn_state).all()
    assert float(m.bn_state.abs().max()) > 0 and not torch.equal(m.bn_state, torch.zeros_like(m.bn_state))
    # determinism: replay the first two steps
    m2 = UNet(n_classes=3, dim=H, n_channels=1, depth=4, complexity_factor=1, flatten_output=True, dtype="bf16",
              logger=quiet, seed=0)
    m2.compile("Adam", "SparseCategoricalCrossentropy", optimizer_kwargs=dict(lr=1e-4))
    for _ in range(2):
        m2.train_step(x, y, w, want_loss=False)
    assert torch.equal(m2.params, ms[1][0].params) and torch.equal(m2.bn_state, ms[1][0].bn_state)
    assert ms[1][1] == losses[:2]


@pytest.mark.parametrize("n_channels,cf", [(2, 1), (1, 2)])
def test_first_layer_wgrad_scratch_does_not_overrun_the_next_layer(n_channels, cf):
    """the first-layer weight-gradient schedule (wgrad_c8: one compact partial row per strip of image
    rows) used to be sized by the generic K-split plan and overran into the not-yet-reduced partials of
    encoder_L0_conv2 with 2 image channels at F0=64 (B=16, 128x128) and with F0>=128 for any channel count. A
    shallow net at exactly those shapes, every gradient tensor against the matched-rounding model (depth 1: the
    graph is well conditioned, so a fixed bound holds)."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    B, K, D = 16, 3, 1
    w = U.init_weights(K, n_channels, D, cf, seed=21)
    rng = np.random.RandomState(6)
    for k in w:
        if k.endswith("/bias"):
            w[k] = rng.uniform(-.1, .1, w[k].shape).astype(np.float32)
    x = rng.randn(B, 128, 128, n_channels).astype(np.float32)
    y = rng.randint(0, K, (B, 128 * 128, 1)).astype(np.uint8)
    sw = np.ones(B, np.float32)
    m = UNet(n_classes=K, dim=128, n_channels=n_channels, depth=D, complexity_factor=cf, flatten_output=True,
             dtype="bf16", logger=quiet)
    m.set_weights_dict(w)
    (probs, loss), log = _schedule_log(lambda: m.forward_backward(x, y, sw))
    wg = [l for l in log if l[0] == "wgrad"]
    print("first-layer case n_channels=%d cf=%g: wgrad schedules %s" % (n_channels, cf, [l[1] for l in wg]))
    g = m.grads.cpu().numpy()
    assert np.isfinite(g).all()
    r64 = U.bf16_matched_step(w, x, y, sw, depth=D, dtype=torch.float64)
    r32 = U.bf16_matched_step(w, x, y, sw, depth=D, dtype=torch.float32)
    rel = lambda a, b: float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
    for name, g64 in r64["grads"].items():
        a = _grad(m, g, name).astype(np.float64)
        e = min(rel(a, g64), rel(a, r32["grads"][name]))
        floor = rel(r32["grads"][name], g64)                   # two evaluations of the matched model (f32 / f64 arithmetic)
        # an overrun replaces ~4 % of encoder_L0_conv2's partial sums with foreign data: O(1) relative error there
        assert e <= max(5e-2, 2 * floor), (name, e, floor)


def test_configs0_single_slice_f32_one_train_step_vs_f64_oracle():
    """BASELINE configs[0], literally: ONE 128x128x1 slice, 3 classes, through the depth-4 / 64-filter network, one
    train step (forward with batch statistics, sparse CE on clipped probabilities, backward, Keras Adam, BN moving
    statistics) -- the reference's `mp train --cpu` plumbing case, here in the exact-f32 MFMA mode against the f64
    oracle: probabilities / loss / every gradient tensor / updated weights (tests/test_gpu_unet.py has the bounds).
    With a batch of ONE slice the batch-statistics BatchNorm of the bottom level normalises over 64 samples per
    channel and the graph is badly conditioned: a plain torch-f32 evaluation is already 1.8 % away from f64 in the
    deep kernels' gradients; the gradients are held to 8x that measured floor here (3x in the B >= 2 cases), up to 3 %
    of a tensor's elements with a ~0 gradient may take their +-lr Adam step the other way (1 % elsewhere), the forward
    side keeps the usual bounds."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_unet_tests", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                              "test_gpu_unet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.test_f32_train_step_vs_oracle((3, 1, 4, 1, 128, 128, 1), noise_mult=8, flip_frac=3e-2)


def test_default_yaml_network_cf2_bf16_inference_step_and_dispatch():
    """The network a default `mp init_project` builds (complexity_factor: 2 => 90/181/362/724/1448 filters,
    mpunet/bin/defaults/MultiPlanar/train_hparams.yaml:82) at 128x128, B = 8, bf16: odd channel counts are
    padded to multiples of 8 in storage (96/184/368/728/1448), every conv runs with channel tails. Inference
    probabilities against the matched-rounding model (well conditioned), a train step's head-side tensors and the
    absence of gradient leakage into the channel padding, the kernel schedules logged."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    B, K, D, cf = 8, 3, 4, 2
    w = U.init_weights(K, 1, D, cf, seed=51)
    rng = np.random.RandomState(52)
    for k in w:
        v = k.split("/")[1]
        if v == "bias":
            w[k] = rng.uniform(-.1, .1, w[k].shape).astype(np.float32)
        elif v == "gamma":
            w[k] = rng.uniform(.5, 1.5, w[k].shape).astype(np.float32)
        elif v in ("beta", "moving_mean"):
            w[k] = rng.uniform(-.3, .3, w[k].shape).astype(np.float32)
        elif v == "moving_variance":
            w[k] = rng.uniform(.5, 2., w[k].shape).astype(np.float32)
    assert w["encoder_L0_conv1/kernel"].shape[-1] == 90 and w["bottom_conv2/kernel"].shape[-1] == 1448
    x = rng.randn(B, 128, 128, 1).astype(np.float32)
    y = rng.randint(0, K, (B, 128 * 128, 1)).astype(np.uint8)
    m = UNet(n_classes=K, dim=128, n_channels=1, depth=D, complexity_factor=cf, dtype="bf16", logger=quiet)
    m.set_weights_dict(w)
    xi = x[:2]
    ref = U.bf16_matched_forward(w, xi, depth=D, out_activation="softmax")
    got, log = _schedule_log(lambda: m.predict(xi, batch_size=2))
    d = np.abs(got - ref)
    scheds = lambda ls: {k: sum(1 for l in ls if l[1] == k) for k in sorted({l[1] for l in ls})}
    print("cf=2 bf16 inference probs vs matched model: max %.3g mean %.3g; schedules %s"
          % (d.max(), d.mean(), scheds([l for l in log if l[0] == "conv"])))
    assert d.max() <= 1.5e-2 and d.mean() <= 3e-3
    assert "regs" not in scheds([l for l in log if l[0] == "conv"])
    # train step: finite, loss of the right size, head-side tensors tight, no gradient in the padding
    m.flatten_output = True
    (probs, loss), log = _schedule_log(lambda: m.forward_backward(x, y, np.ones(B, np.float32)))
    print("cf=2 bf16 train step schedules: conv %s wgrad %s" % (scheds([l for l in log if l[0] == "conv"]),
                                                               scheds([l for l in log if l[0] == "wgrad"])))
    g = m.grads.cpu().numpy()
    assert np.isfinite(g).all() and torch.isfinite(loss).all()
    assert "regs" not in scheds([l for l in log if l[0] == "wgrad"])      # concat layers (96 | 96 ...): one LDS-DMA job per source
    r32 = U.bf16_matched_step(w, x, y, np.ones(B, np.float32), depth=D, dtype=torch.float32)
    rel = lambda a, b: float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
    for name, bound in (("conv2d/kernel", 3e-2), ("conv2d/bias", 3e-2), ("upsample_L3_conv3/kernel", 1e-1),
                        ("upsample_L3_conv2/kernel", 1e-1)):     # (the concat conv: a wrong row mapping of its two jobs is O(1))
        assert rel(_grad(m, g, name).astype(np.float64), r32["grads"][name]) <= bound, name
    for name, (kind, off, ps, ls) in m._tensors.items():
        if kind != 0 or tuple(ps) == tuple(ls):
            continue
        a = g[off:off + int(np.prod(ps))].reshape(ps)
        assert np.count_nonzero(a) == np.count_nonzero(m._from_stored(name, a, ps, ls)), "gradient leaked into padding of " + name
    assert abs(float(loss.mean().item()) - float(r32["loss"].mean())) <= 3e-2 * abs(float(r32["loss"].mean()))
