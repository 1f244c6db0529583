"""The bounds of the inference replay (tests/replay_ref.py, tests/test_gpu_replay.py) checked without a GPU: a torch-f32
emulation of one inference conv launch -- bf16 operands, f32 accumulation, f32 affine, ONE bf16 rounding -- against the fp64
reference, at the widest reduction the replayed networks reach (K = 9 * 512). A correct kernel errs like the emulation; the
emulation must stay under a third of every bound, and a reference with the affine on the wrong side of the ReLU, or a shifted
shift vector, must break them."""
import numpy as np
import torch

import replay_ref as R


def _layer(seed, Cin=512, Cout=512, H=6, W=10):
    rng = np.random.RandomState(seed)
    x = R.bf16_round(np.maximum(rng.randn(2, H, W, Cin), 0) * rng.uniform(.2, 2., Cin) + rng.uniform(-.3, .3, Cin))
    lim = np.sqrt(6.0 / (9 * Cin + 9 * Cout))
    w = R.bf16_round(rng.uniform(-lim, lim, (3, 3, Cin, Cout)))
    b = torch.tensor(rng.uniform(-.1, .1, Cout).astype(np.float32).astype(np.float64))
    gamma = rng.uniform(.5, 1.5, Cout); gamma[0] = -0.8
    s = (gamma / np.sqrt(rng.uniform(.5, 2., Cout) + 1e-3)).astype(np.float32).astype(np.float64)
    t = rng.uniform(-.5, .5, Cout).astype(np.float32).astype(np.float64)
    s[-3:] = 0; t[-3:] = 0; w[..., -3:] = 0; b[-3:] = 0               # padded channels
    s[5] *= 1e-2; t[5] *= 1e-2                                        # a live channel far below the tensor's maximum
    return x, w, b, torch.tensor(s), torch.tensor(t)


def test_f32_emulation_of_a_folded_bn_conv_stays_under_a_third_of_the_bounds():
    worst_t = worst_c = 0.0
    for seed in (0, 1, 2):
        x, w, b, s, t = _layer(seed)
        ref = R.affine_relu_conv(0, x, w, b, s, t).numpy()
        f = torch.float32
        emu = R.bf16_round(R.affine_relu_conv(0, x.to(f), w.to(f), b.to(f), s.to(f), t.to(f))).numpy()
        e_t, e_c, c = R.conv_bound_ratios(emu, ref)
        worst_t, worst_c = max(worst_t, e_t), max(worst_c, e_c)
        assert e_t <= R.CONV_TOL / 3 and e_c <= 1.0 / 3, (seed, e_t, e_c, c)
    print("replay bounds (f32 emulation, K = 4608): tensor-wise %.3g of the maximum, per-channel %.3g of its bound" % (worst_t, worst_c))


def test_bounds_reject_a_misplaced_affine_and_a_shifted_shift_vector():
    x, w, b, s, t = _layer(3)
    ref = R.affine_relu_conv(0, x, w, b, s, t).numpy()
    z = R.layer_forward(0, x, w, b)
    before = torch.relu(s * z + t).numpy()                            # the affine before the ReLU
    assert R.conv_bound_ratios(before, ref)[1] > 1
    shifted = (s * torch.relu(z) + torch.roll(t, 1)).numpy()          # post_shift read one channel off
    assert R.conv_bound_ratios(shifted, ref)[1] > 1
    small = ref.copy(); small[..., 5] *= 1.05                         # 5 % on a channel ~1e-2 of the maximum: the tensor-wise bound is blind
    e_t, e_c, c = R.conv_bound_ratios(small, ref)
    assert e_t <= R.CONV_TOL and e_c > 1 and c == 5, (e_t, e_c, c)


def test_head_partial_bound_holds_for_the_emulation_and_rejects_a_swapped_half():
    rng = np.random.RandomState(4)
    y = rng.randn(40, 64) * rng.uniform(.1, 3., 64)
    Wh = rng.uniform(-.3, .3, (64, 5)).astype(np.float32).astype(np.float64)
    yb = R.bf16_round(y).to(torch.float32)
    hi = torch.tensor(Wh, dtype=torch.float32).to(torch.bfloat16).to(torch.float32)
    lo = (torch.tensor(Wh, dtype=torch.float32) - hi).to(torch.bfloat16).to(torch.float32)
    for h in (0, 1):
        sl = slice(32 * h, 32 * h + 32)
        emu = (yb[:, sl] @ hi[sl] + yb[:, sl] @ lo[sl]).numpy()
        assert R.head_partial_ratio(emu, y[:, sl], Wh[sl]) <= 1.0 / 3
        assert R.head_partial_ratio(emu, y[:, slice(32 - 32 * h, 64 - 32 * h)], Wh[slice(32 - 32 * h, 64 - 32 * h)]) > 1


# ---- the launch-tap helper (tests/replay_tap.py), driven through a C function pointer ------------------------------------------
import ctypes as C
import sys

import pytest


class _Info(C.Structure):
    _fields_ = [("kind", C.c_int32), ("conv_index", C.c_int32)]


_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(_Info))          # the prototype of mpu_launch_tap_fn, declared locally: no library is loaded


def _call_from_c(cb, kind, index=0):
    """What the library does with an installed tap: call the function POINTER. ctypes makes the foreign call through libffi into
    the callback's C thunk, so whatever the Python side raises meets a C frame."""
    addr = C.cast(cb, C.c_void_p).value
    _FN(addr)(None, C.byref(_Info(kind, index)))


class _StubApi:
    FN = _FN

    def __init__(self):
        self.installed, self.calls, self.syncs, self.log_on = None, [], 0, False

    def set_tap(self, model, cb):
        self.calls.append((model, cb is not None))
        self.installed = cb

    def synchronize(self):
        self.syncs += 1

    def log_enable(self, on):
        self.log_on = on

    def log_read(self):
        return "conv ws\nbn_fold fwd"


def test_an_assert_inside_a_bare_ctypes_callback_is_swallowed():
    """The hole the helper closes: a void callback whose assert fails returns normally to its C caller."""
    seen = []
    old = sys.unraisablehook
    sys.unraisablehook = lambda u: seen.append(u.exc_type)
    try:
        def bare(_user, pinfo):
            assert pinfo.contents.kind != 4, "wrong value"
        _call_from_c(_FN(bare), 4)                                     # no exception reaches this frame
    finally:
        sys.unraisablehook = old
    assert seen == [AssertionError], seen


def test_tapped_raises_after_the_body_with_the_first_failure_and_removes_the_tap():
    from replay_tap import tapped
    api, model, checked = _StubApi(), object(), []

    def check(li):
        checked.append((li.kind, li.conv_index))
        assert li.kind != 4, ("bn bwd dz", li.conv_index, 0.5)
        if li.kind == 7:
            raise KeyboardInterrupt("not an Exception either")

    body_done = []
    with pytest.raises(AssertionError) as ei:
        with tapped(model, check, schedule_log=True, api=api) as tap:
            assert api.installed is not None and api.log_on
            for kind, idx in ((3, 0), (4, 11), (5, 1), (4, 12), (7, -1)):
                _call_from_c(api.installed, kind, idx)                 # a failed check does not stop the pass
            body_done.append(True)
    msg = str(ei.value)
    assert body_done and checked == [(3, 0), (4, 11), (5, 1), (4, 12), (7, -1)]
    assert msg.startswith("3 of 5 tapped launches failed their check; the first:"), msg
    assert "launch 2" in msg and "('bn bwd dz', 11, 0.5)" in msg and "12, 0.5" not in msg, msg
    assert len(tap.failures) == 3 and "KeyboardInterrupt" in tap.failures[2]
    assert api.syncs >= 5                                              # synchronized before every check
    assert api.installed is None and api.calls == [(model, True), (model, False)] and not api.log_on


def test_tapped_passes_a_clean_pass_through_and_removes_the_tap():
    from replay_tap import tapped
    api, model, kinds = _StubApi(), object(), []
    with tapped(model, lambda li: kinds.append(li.kind), schedule_log=True, api=api) as tap:
        for kind in (0, 3, 6):
            _call_from_c(api.installed, kind)
    assert kinds == [0, 3, 6] and tap.launches == 3 and not tap.failures
    assert tap.log.splitlines() == ["conv ws", "bn_fold fwd"]
    assert api.installed is None and api.calls == [(model, True), (model, False)] and not api.log_on
    api2 = _StubApi()
    with tapped(model, kinds.append, api=api2):                        # without the schedule log: never switched on, nothing read
        pass
    assert api2.installed is None and not api2.log_on and api2.calls == [(model, True), (model, False)]


def test_tapped_removes_the_tap_when_the_body_raises_and_keeps_the_bodys_exception():
    from replay_tap import tapped
    api = _StubApi()

    def check(li):
        raise ValueError("bad shape")

    with pytest.raises(RuntimeError, match="the launch failed") as ei:
        with tapped(object(), check, schedule_log=True, api=api):
            _call_from_c(api.installed, 2)
            raise RuntimeError("the launch failed")
    assert api.installed is None and not api.log_on
    assert any("bad shape" in n for n in getattr(ei.value, "__notes__", ["bad shape"]))


# ---- f32-storage bounds of the training step's non-conv launches ---------------------------------------------------------------
# (B, H, W, padded C) of every BatchNorm level of networks T1-T3 (tests/test_gpu_replay.py: TRAIN_NETS) and (pixels, C, K) of their heads
_BN_SHAPES = [(3, 48, 40, 96), (3, 24, 20, 184), (3, 12, 10, 368),
              (5, 16, 32, 32), (5, 8, 16, 64), (5, 4, 8, 128), (5, 2, 4, 256), (5, 1, 2, 512),
              (3, 32, 160, 64), (3, 16, 80, 128), (3, 8, 40, 256)]
_HEAD_SHAPES = [(3, 48, 40, 96, 5), (5, 16, 32, 32, 3), (3, 32, 160, 64, 3)]


def _f32(a):
    return torch.tensor(np.asarray(a, np.float64).astype(np.float32).astype(np.float64))


def _measure_f32_emulation():
    """Worst error of a torch-f32 evaluation of replay_ref's formulas -- the plain form and the affine form the kernels evaluate --
    against the fp64 evaluation of the SAME f32 inputs, under the metrics of the GPU replay."""
    from oracle import unet_ref as U
    f = torch.float32
    worst = {"stats": 0.0, "out": 0.0, "reduce": 0.0}

    def out_err(emu, ref):
        e_t, e_c, _c = R.conv_bound_ratios(emu.to(torch.float64).numpy(), ref.numpy(), tol=1.0)
        return max(e_t, e_c)

    for i, (B, H, W, Cn) in enumerate(_BN_SHAPES):
        rng = np.random.RandomState(100 + i)
        x = _f32(np.maximum(rng.randn(B, H, W, Cn) * rng.uniform(.2, 2., Cn) + rng.uniform(-.3, .3, Cn), 0))
        dn = _f32(rng.randn(B, H, W, Cn) * rng.uniform(.01, 1., Cn))
        g = rng.uniform(.5, 1.5, Cn); g[0] = -0.8
        g, bt = _f32(g), _f32(rng.uniform(-.3, .3, Cn))
        mu, inv = R.bn_stats(x)
        mu32, inv32 = R.bn_stats(x.to(f))
        worst["stats"] = max(worst["stats"], R.rel_max(mu32, mu), R.rel_max(inv32, inv))
        mu_d, inv_d = mu32.to(torch.float64), inv32.to(torch.float64)          # the f32 statistics a launch stores, given to both sides
        ref = R.bn_out(x, mu_d, inv_d, g, bt)
        dz, dgamma, dbeta = R.bn_bwd(dn, x, mu_d, inv_d, g)
        for affine in (False, True):
            worst["out"] = max(worst["out"], out_err(R.bn_out(x.to(f), mu32, inv32, g.to(f), bt.to(f), affine), ref))
            dz32, dg32, db32 = R.bn_bwd(dn.to(f), x.to(f), mu32, inv32, g.to(f), affine)
            worst["out"] = max(worst["out"], out_err(dz32, dz))
            worst["reduce"] = max(worst["reduce"], R.rel_max(dg32, dgamma), R.rel_max(db32, dbeta))
    for i, (B, H, W, Cn, K) in enumerate(_HEAD_SHAPES):
        rng = np.random.RandomState(200 + i)
        n = _f32(rng.randn(B, H, W, Cn) * rng.uniform(.5, 1.5, Cn) + rng.uniform(-.3, .3, Cn))
        y = torch.tensor((rng.randint(0, K, (B, H, W)) * (rng.rand(B, H, W) < 0.5)).astype(np.int64))
        w = _f32(np.where(np.arange(B) % 2 == 0, 0.33, 1.0))
        lim = np.sqrt(6.0 / (Cn + K))
        Wh, bh = _f32(rng.uniform(-lim, lim, (Cn, K))), _f32(rng.uniform(-.1, .1, K))
        dn64, dW64, db64 = R.head_bwd(n, y, w, Wh, bh, U.keras_sparse_ce)
        dn32, dW32, db32 = R.head_bwd(n.to(f), y, w.to(f), Wh.to(f), bh.to(f), U.keras_sparse_ce)
        worst["out"] = max(worst["out"], R.rel_max(dn32, dn64))
        worst["reduce"] = max(worst["reduce"], R.rel_max(dW32, dW64), R.rel_max(db32, db64))
        p32 = R.head_fwd(n.to(f), Wh.to(f), bh.to(f))
        worst["probs"] = max(worst.get("probs", 0.0), float((p32.to(torch.float64) - R.head_fwd(n, Wh, bh)).abs().max()))
    return worst


def test_f32_emulation_sets_the_f32_storage_bounds_of_the_non_conv_kinds():
    """TOL_F32 of tests/replay_ref.py -- the bounds of kinds 3, 4 and 7 in dtypes "bf16x3" and "f32" -- is 3 x (the suite's noise_mult)
    the error a torch-f32 evaluation of the same formulas makes against fp64 on the BatchNorm and head shapes of T1-T3. Each number
    must cover 3 x its measurement and may not be looser than 10 x. Measured here (torch-CPU, seeds as below):
      stats   (mean, 1/std: of the vector max)                                    1.67e-7  -> bound 5.5e-7
      out     (BatchNorm forward / backward per channel and tensor-wise, head dn) 1.37e-5  -> bound 4.2e-5 (set by T2's 10-value
              statistics: a channel of nearly equal values has a scale of ~30 and an output far below its terms)
      reduce  (dgamma, dbeta, dWh, dbh: of the vector max)                        2.19e-7  -> bound 7e-7
      probs   (absolute; its bound 2e-5 is the project's, for f32 probabilities)  4.0e-7"""
    worst = _measure_f32_emulation()
    print("f32 emulation of the non-conv kinds against fp64 (T1-T3 shapes): %s" % ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    for k in ("stats", "out", "reduce"):
        assert 3 * worst[k] <= R.TOL_F32[k] <= 10 * worst[k], (k, worst[k], R.TOL_F32[k])
    assert 3 * worst["probs"] <= R.TOL_F32["probs"], worst["probs"]
    assert R.TOL_F32["pool"] == 2.0 ** -24 and R.TOL_BF16["pool"] == 2.0 ** -8       # unit roundoffs of the storage formats
    assert R.TOL_F32["conv"] == R.TOL_F32["wgrad"] == 5e-5


def test_non_conv_references_reject_a_dropped_beta_and_a_last_maximum():
    """The two mutations of the GPU replay's evidence, on the host: the bounds see a BatchNorm output without its beta and a pooled
    gradient routed to the last maximum of a window with ties."""
    rng = np.random.RandomState(7)
    x = _f32(np.maximum(rng.randn(2, 4, 6, 16), 0)); g = _f32(rng.uniform(.5, 1.5, 16)); bt = _f32(rng.uniform(-.3, .3, 16))
    mu, inv = R.bn_stats(x)
    ref = R.bn_out(x, mu, inv, g, bt).numpy()
    got = R.bf16_round(ref).numpy()
    assert R.conv_bound_ratios(got, ref)[1] <= 1.0 / 3
    assert R.conv_bound_ratios(got, R.bn_out(x, mu, inv, g, 0 * bt).numpy())[1] > 1
    n = np.maximum(rng.randn(2, 4, 6, 8), 0)                                       # post-ReLU: windows of equal zeros
    ds, dp = rng.randn(2, 4, 6, 8), rng.randn(2, 2, 3, 8)
    first = R.pool_bwd_skip(n, ds, dp)
    last = R.pool_bwd_skip(n[:, ::-1, ::-1], ds[:, ::-1, ::-1], dp[:, ::-1, ::-1])[:, ::-1, ::-1]
    assert np.abs(first - ds).sum() > 0 and not np.array_equal(first, last)
    assert np.array_equal(R.pool_bwd_skip(n, 0 * ds, dp).reshape(2, 2, 2, 3, 2, 8).sum((2, 4)), dp)       # each gradient lands once
