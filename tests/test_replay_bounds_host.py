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


# ---- the fused forms of the train step (kinds 11-13): references and bounds without a GPU --------------------------------------
# (B, H, W, K) of the head cases H1 / H3 / H3w and of T3 (tests/test_gpu_replay.py: FUSED_CASES), 64 channels; (B, H, W, C) of the
# recomputed levels of T3
_FUSED_HEAD_SHAPES = [(3, 10, 14, 3), (2, 18, 22, 8), (2, 18, 22, 4), (3, 32, 160, 3)]
_FUSED_POOL_SHAPES = [(3, 32, 160, 64), (3, 16, 80, 128)]


def _fused_inputs(seed, B, H, W, Cn, K, bf16):
    """A BatchNorm input as a conv leaves it (post-ReLU, storage-rounded), f32 statistics and coefficients as the forward pass
    stores them, gammas in [0.5, 1.5] with one negative (tests/test_gpu_replay.py: _train_case), a head, labels (zero on about
    half the pixels) and alternating sample weights; storage-rounded skip and pooled gradients."""
    rng = np.random.RandomState(seed)
    x = R.storage_round(np.maximum(rng.randn(B, H, W, Cn) * rng.uniform(.2, 2., Cn) + rng.uniform(-.3, .3, Cn), 0), bf16)
    g = rng.uniform(.5, 1.5, Cn); g[0] = -0.8
    g, bt = _f32(g), _f32(rng.uniform(-.3, .3, Cn))
    mu, inv = (_f32(t) for t in R.bn_stats(x))
    sc = _f32(g * inv)
    sh = _f32(bt - _f32(mu * sc))
    lim = np.sqrt(6.0 / (Cn + K))
    d = dict(x=x, g=g, bt=bt, mu=mu, inv=inv, sc=sc, sh=sh, Wh=_f32(rng.uniform(-lim, lim, (Cn, K))), bh=_f32(rng.uniform(-.1, .1, K)),
             y=torch.tensor((rng.randint(0, K, (B, H, W)) * (rng.rand(B, H, W) < 0.5)).astype(np.int64)),
             w=_f32(np.where(np.arange(B) % 2 == 0, 0.33, 1.0)),
             dskip=R.storage_round(rng.randn(B, H, W, Cn) * rng.uniform(.01, 1., Cn), bf16),
             dp=R.storage_round(rng.randn(B, H // 2, W // 2, Cn) * rng.uniform(.01, 1., Cn), bf16))
    return d


def _emu_head(d, bf16, fault=None, first_round=None):
    """The three head_bn_* passes as the kernels evaluate them (unet_ops.hip), in torch float32 (fmaf through replay_ref.fma32, which
    IS its float32 result; sums in f32; the prologue of head_bn_bwd_apply in double, as the kernel's). fault: a seeded mistake."""
    from oracle import unet_ref as U
    f = torch.float32
    x = d["x"]
    Cn, K = d["Wh"].shape
    aff = R.fma32(x, d["sc"], d["sh"])
    n2 = aff if fault == "n2 not rounded" else R.storage_round(aff, bf16)
    probs = torch.softmax(n2.to(f) @ d["Wh"].to(f) + d["bh"].to(f), -1)                 # f32 [B, H, W, K]: what the launch stores
    w = torch.roll(d["w"], 1) if fault == "neighbour's weight" else d["w"]
    dzh, loss = R.loss_grad_at_logits(probs.to(torch.float64), d["y"], w, U.keras_sparse_ce)
    dzh = dzh.to(f)
    xh = ((x.to(f) - d["mu"].to(f)) * d["inv"].to(f)).reshape(-1, Cn)
    dz2 = dzh.reshape(-1, K)
    M = x.numel() // Cn
    if fault == "tail pixel twice":                # the clamp of a ragged group without its guards: every missing lane repeats the tail
        G = 8 if bf16 else 16
        rep = (-M) % G
        xh, dz2 = torch.cat([xh] + [xh[-1:]] * rep), torch.cat([dz2] + [dz2[-1:]] * rep)
    if first_round is not None:                                                        # the grid-stride loop left after one round
        xh, dz2 = xh[:first_round], dz2[:first_round]
    # head_bn_backward_kernel's order: a lane group walks its G pixels with one fma each, the groups of a wave are summed by a
    # butterfly, the four waves one after the other -- all f32 (one partial row per workgroup of 256 pixels); the rows in double
    G = 8 if bf16 else 16
    nb = -(-xh.shape[0] // 256)
    pad = nb * 256 - xh.shape[0]
    xg = torch.cat([xh, torch.zeros(pad, Cn, dtype=f)]).reshape(nb, 256 // G, G, Cn).to(torch.float64)
    dg = torch.cat([dz2, torch.zeros(pad, K, dtype=f)]).reshape(nb, 256 // G, G, K).to(torch.float64)
    acc = torch.zeros(nb, 256 // G, Cn, K, dtype=f)
    for j in range(G):
        acc = (acc.to(torch.float64) + xg[:, :, j, :, None] * dg[:, :, j, None, :]).to(f)
    acc = acc.reshape(nb, 4, 64 // G, Cn, K)
    while acc.shape[2] > 1:
        acc = acc[:, :, 0::2] + acc[:, :, 1::2]
    T = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0] + acc[:, 3, 0]).to(torch.float64).sum(0)
    dbh = torch.cat([dz2, torch.zeros(pad, K, dtype=f)]).reshape(nb, 256, K).sum(1).to(torch.float64).sum(0)
    Wh = d["Wh"]
    s0, s1 = Wh @ dbh, (Wh * T).sum(1)                                                  # (double, from f32 values)
    k = [_f32(t) for t in R.bn_bwd_coeffs(s1, s0, M, d["mu"], d["inv"], d["g"])]
    dgamma, dbeta = _f32(s1), _f32(s0)
    if fault == "dgamma and dbeta swapped":
        dgamma, dbeta = dbeta, dgamma
    dWh = _f32(d["g"][:, None] * T + d["bt"][:, None] * dbh[None])
    dn = (dzh @ Wh.to(f).T).to(torch.float64)
    dz3 = R.storage_round(R.fma32(k[0], dn, R.fma32(k[1], x, k[2])), bf16)
    if fault != "ReLU mask dropped":
        dz3 = torch.where(x > 0, dz3, torch.zeros((), dtype=torch.float64))
    return dict(probs=probs.to(torch.float64), dz3=dz3, dgamma=dgamma, dbeta=dbeta, dWh=dWh, dbh=_f32(dbh), k=k, loss=loss)


def _judge_head(d, emu, bf16):
    """Every kind-11 / kind-12 comparison of tests/test_gpu_replay.py (_StepChecks) on host tensors: name -> error / bound."""
    from oracle import unet_ref as U
    tol = R.TOL_BF16 if bf16 else R.TOL_F32
    x = d["x"]
    Cn, K = d["Wh"].shape
    M = x.numel() // Cn
    out = {"probs": float((emu["probs"] - R.head_fwd(R.head_bn_n2(x, d["sc"], d["sh"], bf16), d["Wh"], d["bh"])).abs().max()) / tol["probs"]}
    dzh, _l = R.loss_grad_at_logits(emu["probs"], d["y"], d["w"], U.keras_sparse_ce)
    dn2, dgamma, dbeta, dWh = R.head_bn_bwd_sums(x, dzh, d["Wh"], d["mu"], d["inv"], d["g"], d["bt"])
    ce = R.ChannelErr()
    ce.add(emu["dz3"].numpy(), R.bn_bwd_apply(dn2, x, d["mu"], d["inv"], d["g"], dgamma, dbeta, M).numpy())
    e_t, e_c, _c = ce.ratios(tol["out"])
    out["dz3"], out["dz3, per channel"] = e_t / tol["out"], e_c
    for name, got, ref in (("dgamma", emu["dgamma"], dgamma), ("dbeta", emu["dbeta"], dbeta), ("dWh", emu["dWh"], dWh),
                           ("dbh", emu["dbh"], dzh.sum((0, 1, 2)))):
        out[name] = R.rel_max(got, ref) / tol["reduce"]
    for name, got, ref in zip(("k1", "k2", "k3"), emu["k"], R.bn_bwd_coeffs(dgamma, dbeta, M, d["mu"], d["inv"], d["g"])):
        out[name] = R.rel_max(got, ref) / tol["reduce"]
    return out


def _emu_pool(d, bf16, fault=None, blocks=None):
    """Both pool-backward recompute passes as the kernels evaluate them, in torch float32: n recomputed, the gradient routed to
    the first maximum, dn rounded, coefficients in double, dz through the two fmas. The sums as maxpool_bwd_add_kernel forms them: a
    thread keeps one channel chunk and walks the windows e, e + blocks * 256, ... adding their four elements in f32, in order;
    everything above a thread's partial sum is double (blocks: the grid; default the launch's own, one window per thread here)."""
    f = torch.float32
    x = d["x"]
    Cn = x.shape[-1]
    M = x.numel() // Cn
    n = R.storage_round(R.fma32(x, d["sc"], d["sh"]), bf16).numpy()
    ds, dp = d["dskip"].numpy(), d["dp"].numpy()
    if fault == "last maximum":
        summed = R.pool_bwd_skip(n[:, ::-1, ::-1], ds[:, ::-1, ::-1], dp[:, ::-1, ::-1])[:, ::-1, ::-1].copy()
    else:
        summed = R.pool_bwd_skip(n, ds, dp)
    dn = R.storage_round(summed, bf16)
    xh = (x.to(f) - d["mu"].to(f)) * d["inv"].to(f)
    B, H, W = x.shape[:3]
    cpr = Cn // (8 if bf16 else 4)
    nwin = B * (H // 2) * (W // 2)
    stride = nwin if blocks is None else blocks * 256 // cpr                         # windows between two items of one thread
    rounds = -(-nwin // stride)

    def thread_sums(t):                                                                # [B, H, W, C] f32 -> per channel, as above
        win = t.reshape(B, H // 2, 2, W // 2, 2, Cn).permute(0, 1, 3, 2, 4, 5).reshape(nwin, 4, Cn)
        win = torch.cat([win, torch.zeros(rounds * stride - nwin, 4, Cn, dtype=f)]).reshape(rounds, stride, 4, Cn)
        acc = torch.zeros(stride, Cn, dtype=f)
        for r in range(rounds):
            for q in range(4):
                acc = acc + win[r, :, q]
        return acc.to(torch.float64).sum(0)

    s0, s1 = thread_sums(dn.to(f)), thread_sums(dn.to(f) * xh)
    k = [_f32(t) for t in R.bn_bwd_coeffs(s1, s0, M, d["mu"], d["inv"], d["g"])]
    dz = torch.where(x > 0, R.storage_round(R.fma32(k[0], dn, R.fma32(k[1], x, k[2])), bf16), torch.zeros((), dtype=torch.float64))
    return dict(n=n, dz=dz, dgamma=_f32(s1), dbeta=_f32(s0), k=k)


def _judge_pool(d, emu, bf16):
    """Every kind-13 comparison of _StepChecks on host tensors: name -> error / bound."""
    tol = R.TOL_BF16 if bf16 else R.TOL_F32
    x = d["x"]
    Cn = x.shape[-1]
    M = x.numel() // Cn
    dn = R.storage_round(R.pool_bwd_skip(emu["n"], d["dskip"].numpy(), d["dp"].numpy()), bf16)
    dgamma, dbeta = R.bn_bwd_sums(dn, x, d["mu"], d["inv"])
    extra = R.acc_sum_error(M, R.BN_ACC_B)
    out = {}
    for name, got, ref in (("dgamma", emu["dgamma"], dgamma), ("dbeta", emu["dbeta"], dbeta)):
        out[name] = float((got - ref).abs().max() / (tol["reduce"] * ref.abs().max() + extra))
    lims = R.bn_bwd_coeff_bounds(tol["reduce"], extra, dgamma, dbeta, M, d["mu"], d["inv"], d["g"])
    for name, got, ref, lim in zip(("k1", "k2", "k3"), emu["k"], R.bn_bwd_coeffs(dgamma, dbeta, M, d["mu"], d["inv"], d["g"]), lims):
        out[name] = float(((got - ref).abs() / (lim + 1e-300)).max())
    ce = R.ChannelErr()
    ce.add(emu["dz"].numpy(), R.bn_bwd_apply(dn, x, d["mu"], d["inv"], d["g"], dgamma, dbeta, M).numpy())
    e_t, e_c, _c = ce.ratios(tol["out"])
    out["dz"], out["dz, per channel"] = e_t / tol["out"], e_c
    ref, lim = R.pool_bwd_bn_elementwise(dn, x, *emu["k"], bf16)
    out["per element"] = float(((emu["dz"] - ref).abs() / (lim + 1e-300)).max())
    return out


def test_f32_emulation_of_the_fused_head_and_the_pool_recompute_stays_under_a_third_of_the_new_bounds():
    """A torch-f32 evaluation of the three head passes (H1-, H3- and T3-shaped data) and of the two pool passes (T3's recomputed
    levels), in both storage formats, under every comparison the GPU replay makes of kinds 11, 12 and 13."""
    worst, worst7 = {}, {}
    for bf16 in (True, False):
        for i, (B, H, W, K) in enumerate(_FUSED_HEAD_SHAPES):
            if not bf16 and K > 4:
                continue                                                               # (f32 storage: the fused head takes 1..4 classes)
            d = _fused_inputs(300 + i, B, H, W, 64, K, bf16)
            for k, v in _judge_head(d, _emu_head(d, bf16), bf16).items():
                worst["head " + k] = max(worst.get("head " + k, 0.0), v)
        for i, (B, H, W, Cn) in enumerate(_FUSED_POOL_SHAPES):
            d = _fused_inputs(400 + i, B, H, W, Cn, 3, bf16)
            for k, v in _judge_pool(d, _emu_pool(d, bf16), bf16).items():
                worst["pool " + k] = max(worst.get("pool " + k, 0.0), v)
            # MPU_POOL_BWD_BLOCKS=7 (case P3) is a dev aid that makes a thread walk 17 (bf16) / 34 (f32 storage) windows of the
            # widest level instead of one: its f32 chains are that much longer than the launch's own, and it is held to the bound
            # itself, not to a third of it
            for k, v in _judge_pool(d, _emu_pool(d, bf16, blocks=7), bf16).items():
                worst7[k] = max(worst7.get(k, 0.0), v)
    print("f32 emulation of kinds 11-13, error / bound: %s" % ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    print("... pool passes on a grid of 7 workgroups: %s" % ", ".join("%s %.3g" % kv for kv in sorted(worst7.items())))
    assert all(v <= 1.0 / 3 for v in worst.values()), worst
    assert all(v <= 1.0 for v in worst7.values()), worst7


def _f32_of_fraction(fr):
    """The float32 nearest to an exact rational, ties to even (float(fr) is correctly rounded to fp64; its float32 neighbours are
    compared exactly)."""
    from fractions import Fraction
    c = np.float32(float(fr))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1))


def test_fma_emulation_equals_exact_rational_arithmetic():
    """replay_ref.fma32 (the fp64 evaluation of fmaf) and the storage rounding behind it against exact rational arithmetic on 10^4
    triples: half of them random, half with the shift chosen so that x * scale + shift falls next to a bf16 rounding boundary (a
    midpoint between two bf16 numbers) -- where a wrong last float32 bit flips the stored value."""
    from fractions import Fraction
    rng = np.random.RandomState(11)
    n = 5000
    x = np.concatenate([R.bf16_round(np.maximum(rng.randn(n), 0) * 3).numpy(), rng.randn(n)]).astype(np.float32)
    sc = (rng.uniform(.3, 30., 2 * n) * np.where(rng.rand(2 * n) < .2, -1, 1)).astype(np.float32)
    sh = rng.uniform(-.5, .5, 2 * n).astype(np.float32)
    x2, sc2 = x.copy(), sc.copy()
    mid = R.bf16_round(rng.randn(2 * n) * 2).numpy()
    mid = (mid + np.ldexp(1.0, np.frexp(mid + (mid == 0))[1] - 9)).astype(np.float32)      # half a bf16 ulp above a bf16 number
    sh2 = (mid.astype(np.float64) - x2.astype(np.float64) * sc2.astype(np.float64)).astype(np.float32)
    X, S, T = np.concatenate([x, x2]), np.concatenate([sc, sc2]), np.concatenate([sh, sh2])
    got = R.fma32(X.astype(np.float64), S.astype(np.float64), T.astype(np.float64))
    got_b, got_f = R.storage_round(got, True).numpy(), got.numpy()
    near = 0
    for i in range(len(X)):
        want = _f32_of_fraction(Fraction(float(X[i])) * Fraction(float(S[i])) + Fraction(float(T[i])))
        assert float(want) == got_f[i], (i, X[i], S[i], T[i], want, got_f[i])
        wb = float(torch.tensor(float(want), dtype=torch.float32).to(torch.bfloat16))
        assert wb == got_b[i], (i, want, wb, got_b[i])
        near += i >= 2 * n and abs(float(want) - float(mid[i - 2 * n])) <= 4 * abs(float(np.spacing(np.float32(want))))
    assert near >= n, near                                                            # the boundary triples do sit on their boundaries


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_fused_references_reject_seeded_faults(bf16):
    """Each mistake a fused kernel could make at the edges this replay was built for breaks at least one bound, on H1-shaped data
    (M = 420: ragged in both storages) and T3's level-1 pool shape; the unseeded emulation passes all of them."""
    K = 3
    d = _fused_inputs(500, 3, 10, 14, 64, K, bf16)
    assert max(_judge_head(d, _emu_head(d, bf16), bf16).values()) <= 1.0 / 3
    seeded = {"n2 not rounded": ("probs",), "ReLU mask dropped": ("dz3, per channel",), "tail pixel twice": ("dWh", "dbh", "dgamma"),
              "neighbour's weight": ("dz3, per channel", "dbh"), "dgamma and dbeta swapped": ("dgamma", "dbeta")}
    for fault, fams in seeded.items():
        if fault == "n2 not rounded" and not bf16:
            continue                                                                   # (f32 storage: the rounding is the fma's own)
        r = _judge_head(d, _emu_head(d, bf16, fault=fault), bf16)
        assert any(r[k] > 1.0 for k in fams), (fault, {k: r[k] for k in fams})
    r = _judge_head(d, _emu_head(d, bf16, first_round=256), bf16)                      # pixels beyond the first grid round left out
    assert r["dWh"] > 1.0 and r["dbh"] > 1.0 and r["dgamma"] > 1.0, r
    dpool = _fused_inputs(501, 3, 16, 80, 128, K, bf16)
    assert max(_judge_pool(dpool, _emu_pool(dpool, bf16), bf16).values()) <= 1.0 / 3
    r = _judge_pool(dpool, _emu_pool(dpool, bf16, fault="last maximum"), bf16)
    if bf16:
        assert r["per element"] > 1.0 and r["dz, per channel"] > 1.0, r
    else:
        # f32 storage: the windows that tie are those with several ZEROS of the post-ReLU input (equal x, equal n), and dz is masked
        # where x = 0 while dgamma / dbeta see equal xhat there -- the last maximum is the same function. In bf16 storage different
        # positive x round to the same n, and the routing shows (above).
        assert max(r.values()) <= 1.0 / 3, r


def test_post_relu_inputs_and_a_negative_gamma_yield_tied_windows():
    """What check (c) of kind 13 relies on: the BatchNorm of a post-ReLU tensor maps a window's equal zeros to equal values, and
    under the one negative gamma of _train_case they are the window's MAXIMUM -- so the first and the last maximum differ."""
    for bf16 in (True, False):
        d = _fused_inputs(600, 3, 16, 80, 128, 3, bf16)
        n = R.storage_round(R.fma32(d["x"], d["sc"], d["sh"]), bf16).numpy()
        tied, windows = R.tied_windows(n)
        tied0, windows0 = R.tied_windows(n[..., :1])
        assert tied > 0 and tied0 > windows0 // 10, (tied, windows, tied0, windows0)
        ds, dp = d["dskip"].numpy(), d["dp"].numpy()
        last = R.pool_bwd_skip(n[:, ::-1, ::-1], ds[:, ::-1, ::-1], dp[:, ::-1, ::-1])[:, ::-1, ::-1]
        assert not np.array_equal(R.pool_bwd_skip(n, ds, dp)[..., 0], last[..., 0])
    assert R.tied_windows(np.arange(16.).reshape(1, 4, 4, 1)) == (0, 4)


def test_launch_tap_fused_entry_is_declared_exported_and_bound_and_aux2_sits_at_the_headers_offset():
    import os
    import re
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    assert lib.mpu_abi_version() == _lib.ABI_VERSION == 2                              # the change is additive
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mpunet_hip.h")).read()
    name = "mpu_unet_set_launch_tap_fused"
    assert name in _lib.declared_symbols() and hasattr(lib, name) and "int %s(mpu_unet* m, int32_t on);" % name in hdr
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct mpu_launch_info \{(.*?)\} mpu_launch_info;", hdr, re.S).group(1), flags=re.S)
    fields, off, offs = [], 0, {}
    for decl in (t.strip() for t in body.split(";")):
        if not decl:
            continue
        ptr = decl.startswith("const void*")
        size = 8 if ptr or decl.startswith("int64_t") else 4
        assert ptr or decl.startswith(("int32_t", "int64_t")), decl
        for nm in decl.replace("const void*", "").replace("int32_t", "").replace("int64_t", "").split(","):
            off = (off + size - 1) // size * size
            offs[nm.strip()] = off
            fields.append(nm.strip())
            off += size
    assert fields == [f for f, _t in _lib.LaunchInfo._fields_] and fields[-1] == "aux2", fields
    assert {f: getattr(_lib.LaunchInfo, f).offset for f in fields} == offs and offs["aux2"] == 128
    assert C.sizeof(_lib.LaunchInfo) == (off + 7) // 8 * 8 == 136


def test_f32_emulation_of_a_batchnorm_over_one_value_stays_under_a_third_of_its_per_element_bounds():
    """The bottom of a one-image case (H2: 128 channels, P4: 2048) is a BatchNorm over ONE value per channel; kinds 3 and 4 hold it
    per element (replay_ref.one_value_bound). Emulated as the kernels evaluate it: mean out of the 2^-24 units of the forward
    accumulator, invstd / scale / shift as bn_fwd_coeffs rounds them, y = storage(fmaf(x, scale, shift)); backward sums out of the
    2^-40 units, coefficients as bn_bwd_coeffs rounds them, dz = storage([x > 0] fmaf(k1, dn, fmaf(k2, x, k3))). The f32 arithmetic
    stays under a third of the f32 part of the bound in both storages; with the storage rounding of the forward output the whole
    ratio may reach 1 in bf16 (ONE rounding reaches its unit roundoff, as the pool backward's bound) and stays under a third in f32."""
    worst = {}
    for bf16 in (True, False):
        for Cn, seed in ((128, 700), (2048, 701)):
            rng = np.random.RandomState(seed)
            x = R.storage_round(np.maximum(rng.randn(1, 1, 1, Cn) * rng.uniform(.2, 2., Cn) + rng.uniform(-.3, .3, Cn), 0), bf16)
            dn = R.storage_round(rng.randn(1, 1, 1, Cn) * rng.uniform(.01, 1., Cn), bf16)
            g = rng.uniform(.5, 1.5, Cn); g[0] = -0.8
            g, bt = _f32(g), _f32(rng.uniform(-.3, .3, Cn))
            xs = x.reshape(Cn)
            mu64 = torch.round(xs * 2.0 ** 24) / 2.0 ** 24                              # the accumulator's units; M = 1
            var = (torch.round(xs * xs * 2.0 ** 16) / 2.0 ** 16 - mu64 * mu64).clamp_min(0.0)
            inv = _f32(1.0 / torch.sqrt(var + R.BN_EPS))
            mu, sc = _f32(mu64), _f32(g * inv)
            sh = _f32(bt - _f32(mu * sc))
            ref = R.bn_out(x, mu, inv, g, bt).numpy()                                  # (the replay's reference: DEVICE statistics)
            aff = R.fma32(x, sc, sh)
            terms = np.abs(x.numpy() * sc.numpy()) + np.abs(sh.numpy())
            tag = "bf16" if bf16 else "f32"
            worst["forward, f32 part, " + tag] = max(worst.get("forward, f32 part, " + tag, 0.0),
                                                     float((np.abs(aff.numpy() - ref) / (R.one_value_bound(None, terms) + 1e-300)).max()))
            worst["forward, stored, " + tag] = max(worst.get("forward, stored, " + tag, 0.0), float(
                (np.abs(R.storage_round(aff, bf16).numpy() - ref) / (R.one_value_bound(ref, terms, bf16) + 1e-300)).max()))
            s0 = torch.round(dn.reshape(Cn) * 2.0 ** 40) / 2.0 ** 40                   # sum dn, sum dn * xhat out of their units
            s1 = torch.round(_f32(dn.reshape(Cn) * _f32(_f32(xs - mu) * inv)) * 2.0 ** 40) / 2.0 ** 40
            k = [_f32(t) for t in R.bn_bwd_coeffs(s1, s0, 1, mu, inv, g)]
            dz = torch.where(x > 0, R.storage_round(R.fma32(k[0], dn, R.fma32(k[1], x, k[2])), bf16), torch.zeros((), dtype=torch.float64))
            dref, dg, db = R.bn_bwd(dn, x, mu, inv, g)
            k64 = R.bn_bwd_coeffs(dg, db, 1, mu, inv, g)
            bterms = ((k64[0] * dn).abs() + (k64[1] * x).abs() + k64[2].abs()).numpy()
            worst["backward, " + tag] = max(worst.get("backward, " + tag, 0.0),
                                            float((np.abs(dz.numpy() - dref.numpy()) / (R.one_value_bound(None, bterms) + 1e-300)).max()))
    print("BatchNorm over one value, f32 emulation, error / bound: %s" % ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    for k, v in worst.items():
        assert v <= (1.0 if k == "forward, stored, bf16" else 1.0 / 3), worst
