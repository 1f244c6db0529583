"""
The optimizers of UNet.compile on the GPU: SGD (momentum, Nesterov), RMSprop (momentum, centered), Adam / AMSGrad, Adamax, each
with learning-rate decay (tests/optimizer_ref.ALL_CONFIGS: every rule and flag combination).

  (a) mpu_optimizer_step against the f32 restatement (optimizer_ref.step32);
  (b) mpu_unet_optimizer_pack == mpu_optimizer_step + mpu_unet_pack_weights, bit for bit;
  (c) apply_gradients on a small network against the f64 rule applied to the device's own gradients;
  (d) graph replay == eager, bit for bit, with decay and a re-capture after a learning-rate change;
  (e) plain Adam with decay 0 / amsgrad False given explicitly is the default path;
  (f) `mp train --synthetic` with Nesterov SGD and decay.

Yardsticks: the existing Adam entry points (mpu_adam_step, mpu_unet_adam_pack), measured by the tests themselves on the same
inputs and printed (-s): (a) if Adam's unit is bit-exact against its f32 restatement, every rule must be bit-equal, else a rule
may be twice Adam's distance away; (c) a rule may deviate from the f64 rule by twice what plain Adam does.
Measured on an MI355X: (a) mpu_adam_step is 0 ulp from its f32 restatement, so bit-equality is what (a) demands, and every rule
shows 0 ulp; (c) plain Adam deviates by 6.91e-6 of the largest update (bound 1.38e-5); the rules show SGD 4.1e-8, + momentum
1.1e-7, Nesterov 1.5e-7, RMSprop 3.1e-7 .. 3.4e-7 (its four variants), Adam with decay 6.91e-6, AMSGrad 6.90e-6, Adamax 4.4e-7.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimizer_ref as OR                                                              # noqa: E402

pytestmark = pytest.mark.gpu
quiet = lambda *a, **k: None
IDS = [c[0] + "".join("-" + k for k in ("momentum", "nesterov", "centered", "amsgrad") if c[1].get(k)) for c in OR.ALL_CONFIGS]


def lib_config(cfg):
    from multiplanarunet_amd import _lib
    name, kw = cfg
    c = _lib.OptimizerConfig()
    c.kind = {"Adam": _lib.MPU_OPT_ADAM, "SGD": _lib.MPU_OPT_SGD, "RMSprop": _lib.MPU_OPT_RMSPROP, "Adamax": _lib.MPU_OPT_ADAMAX}[name]
    c.flags = (_lib.MPU_OPT_NESTEROV if kw.get("nesterov") else 0) | (_lib.MPU_OPT_AMSGRAD if kw.get("amsgrad") else 0) \
        | (_lib.MPU_OPT_CENTERED if kw.get("centered") else 0)
    c.lr, c.decay = kw["lr"], kw["decay"]
    c.beta1, c.beta2 = kw.get("beta_1", 0.9), kw.get("beta_2", 0.999)
    c.epsilon, c.momentum, c.rho = kw.get("epsilon", 1e-7), kw.get("momentum", 0.0), kw.get("rho", 0.9)
    return c


def compile_kwargs(cfg):
    return dict(cfg[1])


def ulps(a, b):
    """Largest distance in f32 units in the last place between two f32 arrays (finite values)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
N_A, STEPS_A = 4099, 5          # not a multiple of 4; the buffers start one float behind a 16-byte boundary


def _inputs_a():
    rng = np.random.RandomState(21)
    p0 = rng.randn(N_A).astype(np.float32)
    gs = [(rng.randn(N_A) * (0.0 if t == 3 else 1.0)).astype(np.float32) for t in range(1, STEPS_A + 1)]   # step 3: all-zero gradients
    gs[0][:7] = 0.0                                                   # and zeros in the very first step (empty slots underneath)
    return p0, gs


def _unaligned(a):
    buf = torch.zeros(a.size + 5, dtype=torch.float32, device="cuda")
    v = buf[1:1 + a.size]
    assert v.data_ptr() % 16 == 4
    v.copy_(torch.from_numpy(a))
    return buf, v


def _device_steps(cfg, use_parent_adam=False):
    """STEPS_A steps of the element-wise entry point on the inputs above; returns the worst ulp distance to step32 over p and slots."""
    from multiplanarunet_amd import _lib
    p0, gs = _inputs_a()
    keep, p = _unaligned(p0)
    ns = OR.num_slots(cfg)
    slot_bufs = [_unaligned(np.zeros(N_A, np.float32)) for _ in range(ns)]
    slots = [v for _, v in slot_bufs]
    guard = [b.clone() for b, _ in [(keep, p)] + slot_bufs]
    ptrs = (C.c_void_p * 3)(*[s.data_ptr() for s in slots] + [None] * (3 - ns))       # a slot the rule does not have: NULL
    pr, sr = p0, [np.zeros(N_A, np.float32) for _ in range(ns)]
    worst = 0
    c = lib_config(cfg)
    for t in range(1, STEPS_A + 1):
        gk, g = _unaligned(gs[t - 1])
        if use_parent_adam:
            kw = cfg[1]
            _lib.call("mpu_adam_step", _lib.ptr(p), _lib.ptr(g), _lib.ptr(slots[0]), _lib.ptr(slots[1]), N_A, t, kw["lr"], kw["beta_1"],
                      kw["beta_2"], kw["epsilon"], _lib.stream_ptr())
        else:
            _lib.call("mpu_optimizer_step", C.byref(c), _lib.ptr(p), _lib.ptr(g), ptrs, N_A, t, None, _lib.stream_ptr())
        torch.cuda.synchronize()
        pr, sr = OR.step32(cfg, pr, gs[t - 1], sr, t)
        worst = max([worst, ulps(p.cpu().numpy(), pr)] + [ulps(s.cpu().numpy(), r) for s, r in zip(slots, sr)])
    for (b, v), g0 in zip([(keep, p)] + slot_bufs, guard):               # nothing outside [1, 1 + n) was written
        assert torch.equal(b[:1], g0[:1]) and torch.equal(b[1 + N_A:], g0[1 + N_A:])
    return worst


_ADAM_A = []


def adam_ulps_a():
    """What the existing Adam unit (mpu_adam_step) shows against ITS f32 restatement on the same inputs: the yardstick of (a)."""
    if not _ADAM_A:
        _ADAM_A.append(_device_steps(OR.config("Adam", lr=0.01, epsilon=1e-8), use_parent_adam=True))
        print("mpu_adam_step vs its f32 restatement: %d ulp" % _ADAM_A[0])
    return _ADAM_A[0]


@pytest.mark.parametrize("cfg", OR.ALL_CONFIGS, ids=IDS)
def test_optimizer_step_equals_the_f32_restatement(cfg):
    """mpu_optimizer_step, 5 steps (step 3 with all-zero gradients), decay 0.25, 4099 floats at a 4-byte-misaligned address, against
    optimizer_ref.step32. Yardstick: mpu_adam_step against the f32 restatement of adam_update on the same inputs; where that is
    bit-exact (0 ulp) bit-equality is demanded of every rule, else twice Adam's distance is allowed. Measured: Adam 0 ulp, so the
    bound is 0 -- bit-equality; it is this test, not (c), that pins the constants of the rules whose f32 error is far below Adam's."""
    base = adam_ulps_a()
    got = _device_steps(cfg)
    print("%s: %d ulp (Adam: %d)" % (cfg[0], got, base))
    assert got <= 2 * base, (cfg, got, base)


def test_optimizer_step_device_counter_equals_host_step_number():
    """The device-resident counter (t - 1, incremented by the call) gives the bits the host step number gives, for a rule whose
    constant moves with t (Adamax) and one that only decays (SGD)."""
    from multiplanarunet_amd import _lib
    p0, gs = _inputs_a()
    for cfg in (OR.config("Adamax", lr=0.01, decay=0.25), OR.config("SGD", lr=0.05, momentum=0.9, decay=0.25)):
        c = lib_config(cfg)
        ns = OR.num_slots(cfg)
        out = []
        for counter in (False, True):
            p = torch.from_numpy(p0).cuda()
            slots = [torch.zeros_like(p) for _ in range(ns)]
            ptrs = (C.c_void_p * 3)(*[s.data_ptr() for s in slots] + [None] * (3 - ns))
            step = torch.zeros(1, dtype=torch.int64, device="cuda")
            for t in range(1, 4):
                g = torch.from_numpy(gs[t - 1]).cuda()
                _lib.call("mpu_optimizer_step", C.byref(c), _lib.ptr(p), _lib.ptr(g), ptrs, N_A, 0 if counter else t,
                          _lib.ptr(step) if counter else None, _lib.stream_ptr())
            torch.cuda.synchronize()
            assert int(step.item()) == (3 if counter else 0)
            out.append([p] + slots)
        assert all(torch.equal(a, b) for a, b in zip(*out))


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,cf,Cch", [("bf16", 1, 1), ("bf16", 2, 2), ("f32", 0.25, 1), ("bf16x3", 0.5, 1), ("bf16x3", 2, 2)])
@pytest.mark.parametrize("cfg", OR.ALL_CONFIGS, ids=IDS)
def test_fused_optimizer_pack_equals_step_then_pack(cfg, dtype, cf, Cch):
    """mpu_unet_optimizer_pack (one launch: the update + both packed operand copies) == mpu_optimizer_step + mpu_unet_pack_weights,
    bit for bit: parameters, every slot and every byte of the packed buffer, over three steps; the grid of
    test_fused_adam_pack_equals_adam_then_pack (odd filter counts at cf = 2 exercise the channel tails)."""
    from multiplanarunet_amd.unet import UNet
    rng = np.random.RandomState(8)
    B, H, D = 2, 32, 2
    x = torch.tensor(rng.randn(B, H, H, Cch).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, 3, (B, H * H, 1)).astype(np.uint8), device="cuda")
    a = UNet(n_classes=3, dim=H, n_channels=Cch, depth=D, complexity_factor=cf, dtype=dtype, logger=quiet, seed=0)
    b = UNet(n_classes=3, dim=H, n_channels=Cch, depth=D, complexity_factor=cf, dtype=dtype, logger=quiet, seed=0)
    for m in (a, b):
        m.compile(cfg[0], "SparseCategoricalCrossentropy", optimizer_kwargs=compile_kwargs(cfg))
        assert not m._plain_adam()
    for _ in range(3):
        a.forward_backward(x, y, None, want_loss=False)
        a.apply_gradients(fused=True)
        b.forward_backward(x, y, None, want_loss=False)
        b.apply_gradients(fused=False)
        assert torch.equal(a.grads, b.grads) and torch.equal(a.params, b.params)
        assert len(a._slots) == len(b._slots) == OR.num_slots(cfg) and all(torch.equal(s, r) for s, r in zip(a._slots, b._slots))
        assert torch.equal(a.packed.view(torch.uint8), b.packed.view(torch.uint8))
    assert torch.isfinite(a.params).all() and a.iterations == 3


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def _net_deviation(cfg, steps=5):
    """apply_gradients on a small network against the f64 rule applied on the host to the device's own gradients and parameters:
    the largest |p_device - p_f64| beyond the final rounding of p to f32 (half an ulp of p, which no rule can avoid), relative to
    the largest update of the step; the worst step of `steps`."""
    from multiplanarunet_amd.unet import UNet
    rng = np.random.RandomState(5)
    B, H = 2, 32
    x = torch.tensor(rng.randn(B, H, H, 1).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, 3, (B, H * H, 1)).astype(np.uint8), device="cuda")
    m = UNet(n_classes=3, dim=H, depth=2, complexity_factor=0.25, dtype="bf16", logger=quiet, seed=1)
    m.compile(cfg[0], "SparseCategoricalCrossentropy", optimizer_kwargs=compile_kwargs(cfg))
    slots = [np.zeros(m.params.numel()) for _ in range(OR.num_slots(cfg))]
    worst = 0.0
    for t in range(1, steps + 1):
        m.forward_backward(x, y, None, want_loss=False)
        p0, g = m.params.cpu().numpy().astype(np.float64), m.grads.cpu().numpy().astype(np.float64)
        m.apply_gradients()
        want, slots = OR.step64(cfg, p0, g, slots, t)
        got = m.params.cpu().numpy().astype(np.float64)
        half_ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) / 2
        upd = np.abs(want - p0).max()
        assert upd > 0 and np.isfinite(got).all()
        worst = max(worst, float(np.maximum(np.abs(got - want) - half_ulp, 0).max() / upd))
    return worst


_ADAM_C = []


def adam_deviation_c():
    """Plain Adam (the existing mpu_unet_adam_pack path, untouched by the new rules) under the test of (c): its yardstick."""
    if not _ADAM_C:
        _ADAM_C.append(_net_deviation(OR.config("Adam", lr=0.01, epsilon=1e-8)))
        print("plain Adam vs the f64 rule: %.3g of the largest update" % _ADAM_C[0])
    return _ADAM_C[0]


@pytest.mark.parametrize("cfg", OR.ALL_CONFIGS, ids=IDS)
def test_apply_gradients_follows_the_f64_rule_on_a_real_network(cfg):
    """5 steps of a depth-2 bf16 network; the f64 rule runs on the gradients and parameters copied from the device after every
    forward_backward, which isolates the optimizer from the gradient tolerance. Bound: twice what plain Adam shows under this very
    test through the existing mpu_unet_adam_pack. Measured: 6.91e-6 of the largest update, i.e. half the relative error of the
    f32 `1 - beta_2` (1 - 0.999f is 1.3e-5 off, and the root halves it); the bound is therefore 1.38e-5. SGD, RMSprop and Adamax
    have no such constant and sit at 4e-8 .. 4.4e-7, far inside it: for them this test guards the wiring of the network path
    (slots, step number, decay), and the bit-equality of (a) and (b) guards the arithmetic."""
    base = adam_deviation_c()
    got = _net_deviation(cfg)
    print("%s: %.3g of the largest update (Adam: %.3g)" % (cfg[0], got, base))
    assert got <= 2 * base, (cfg, got, base)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", OR.ALL_CONFIGS, ids=IDS)
def test_graphed_step_equals_eager_with_decay_and_a_recapture(cfg):
    """Graph replay == eager step, bit for bit, over 8 steps with decay 0.25 (the device counter drives lr_t and the bias
    corrections), with a re-capture after optimizer_kwargs["lr"] was halved behind step 4, as ReduceLROnPlateau does, and junk
    tensors allocated and freed between the replays (a freed slot or counter would be theirs to reuse)."""
    from multiplanarunet_amd.unet import UNet
    rng = np.random.RandomState(3)
    B, H = 4, 32
    x = torch.tensor(rng.randn(B, H, H, 1).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, 3, (B, H * H, 1)).astype(np.uint8), device="cuda")
    sw = torch.ones(B, device="cuda")
    mk = lambda: UNet(n_classes=3, dim=H, depth=2, complexity_factor=0.25, dtype="bf16", logger=quiet, seed=0)
    a, b = mk(), mk()
    for m in (a, b):
        m.compile(cfg[0], "SparseCategoricalCrossentropy", optimizer_kwargs=compile_kwargs(cfg))
    for i in range(8):
        if i == 4:
            a.optimizer_kwargs["lr"] *= 0.5
        a.train_step(x, y, sw, want_loss=False)
    replay = b.make_graphed_train_step(x, y, sw)           # performs step 1 while warming up
    ns = OR.num_slots(cfg)
    assert len(b._slots) == ns and sum(1 for k in replay.keep_alive if isinstance(k, tuple) and len(k) == ns and all(s is t for s, t in zip(k, b._slots))) == 1
    for i in range(1, 8):
        if i == 4:
            b.optimizer_kwargs["lr"] *= 0.5
            old = replay
            replay = b.make_graphed_train_step(x, y, sw, warmup=False)
            del old
        junk = [torch.full((k + 1,), 7, dtype=torch.int64, device="cuda") for k in range(8)]
        junk += [torch.full((a.params.numel(),), 3.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        del junk
        replay()
    torch.cuda.synchronize()
    assert a.iterations == b.iterations == 8
    assert torch.equal(a.params, b.params) and torch.equal(a.bn_state, b.bn_state)
    assert all(torch.equal(s, r) for s, r in zip(a._slots, b._slots))
    assert torch.equal(a.packed.view(torch.uint8), b.packed.view(torch.uint8)) and torch.isfinite(a.params).all()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 1, 128, 16), (2, 0.25, 32, 2)])
def test_plain_adam_given_explicitly_is_the_default_path(shape):
    """compile("Adam", decay=0.0, amsgrad=False) is compile("Adam"): bit-identical over three steps, and at the configs[1] network
    the optimizer still runs beside the weight gradients (schedule log: "tail-overlap adam range=")."""
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.unet import UNet
    D, cf, H, B = shape
    rng = np.random.RandomState(12)
    x = torch.tensor(rng.randn(B, H, H, 1).astype(np.float32), device="cuda")
    y = torch.tensor(rng.randint(0, 3, (B, H * H, 1)).astype(np.uint8), device="cuda")
    mk = lambda: UNet(n_classes=3, dim=H, n_channels=1, depth=D, complexity_factor=cf, dtype="bf16", logger=quiet, seed=3)
    a, b = mk(), mk()
    a.compile("Adam", "SparseCategoricalCrossentropy", optimizer_kwargs=dict(lr=1e-3))
    b.compile("Adam", "SparseCategoricalCrossentropy", optimizer_kwargs=dict(lr=1e-3, decay=0.0, amsgrad=False))
    assert a._plain_adam() and b._plain_adam()
    lib = _lib.load()
    for i in range(3):
        a.train_step(x, y, None, want_loss=False)
        if i == 0:
            lib.mpu_schedule_log_enable(1)
        b.train_step(x, y, None, want_loss=False)
        if i == 0:
            buf = C.create_string_buffer(1 << 16)
            lib.mpu_schedule_log_read(buf, len(buf))
            lib.mpu_schedule_log_enable(0)
            if shape == (4, 1, 128, 16):
                assert "tail-overlap adam range=" in buf.value.decode(), buf.value.decode()[-400:]
    assert torch.equal(a.params, b.params) and torch.equal(a._adam_m, b._adam_m) and torch.equal(a._adam_v, b._adam_v)
    assert torch.equal(a.packed.view(torch.uint8), b.packed.view(torch.uint8)) and torch.equal(a.bn_state, b.bn_state)


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
def test_mp_train_synthetic_with_nesterov_sgd_and_decay(tmp_path, capsys):
    from multiplanarunet_amd.cli import mp
    from multiplanarunet_amd.unet import UNet
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text(
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 64\n  depth: 3\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 64.0\n  batch_size: 8\n  n_epochs: 2\n"
        "  optimizer: SGD\n  optimizer_kwargs: {lr: 0.01, momentum: 0.9, nesterov: true, decay: 1.0e-3}\n"
        "  loss: SparseCategoricalCrossentropy\n  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n")
    mp.entry_func(["train", "--project_dir", str(proj), "--synthetic", "4", "--epochs", "2",
                   "--train_images_per_epoch", "80", "--val_images_per_epoch", "16"])
    assert "Optimizer:   SGD(lr=0.01, momentum=0.9, nesterov=True, decay=0.001)" in capsys.readouterr().out
    with np.load(proj / "model" / "model_weights.npz") as z:
        w = {k.replace("__", "/"): z[k] for k in z.files}
    assert w and all(np.isfinite(v).all() for v in w.values())
    init = UNet(n_classes=3, n_channels=1, dim=64, depth=3, complexity_factor=0.0625, device="cpu", logger=quiet, seed=0).get_weights_dict()
    kernels = [k for k in w if k.endswith("/kernel")]
    assert kernels and all(w[k].shape == init[k].shape and not np.array_equal(w[k], init[k]) for k in kernels)
    rows = (proj / "logs" / "training.csv").read_text().strip().splitlines()
    head = rows[0].split(",")
    lr_col = head.index("lr")
    assert len(rows) == 3 and [float(r.split(",")[lr_col]) for r in rows[1:]] == [0.01, 0.01]      # the BASE rate, as Keras logs it
