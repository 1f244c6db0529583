"""
Teacher-forced replay of the benchmarked train step ("tighten bf16 parity"): BASELINE configs[1]
(depth 4, 64 filters, 16 bf16 slices of 128x128) runs ONE real forward + backward pass with a launch tap installed
(mpu_unet_set_launch_tap). For every one of its 22 forward, 25 data-gradient and 22 weight-gradient convolution
launches the test takes the launch's OWN inputs out of the workspace, computes the same convolution independently
(torch-CPU, fp64 accumulation) from exactly those inputs, and compares with what the HIP kernel stored.

This pins each launch *in situ* -- the kernel, its schedule, its epilogue, on the tensors of the real step --
without the ~45x error amplification of the train-mode BatchNorm network between launches that forces the
whole-network bf16 tests to noise-floor bounds. Tolerances are those of the per-layer suite (tests/test_gpu_conv.py):
forward / data gradient 1.2e-2 of the tensor max (one bf16 rounding of the stored output is 2^-9 relative), weight and
bias gradient 2e-3 of the tensor max (fp32 sums of exact bf16 products).

Forward and data-gradient references are evaluated on the first CMP images of the batch (a convolution's output for
an image depends on that image only); weight gradients sum over the whole batch and are evaluated on all of it.

The INFERENCE forward (run_forward_infer: every `mp predict`, the benchmark's predict leg) is replayed the same way
(_replay_inference, four small networks and three schedule switches). Its launches report as kind 0 (conv without a BatchNorm),
kind 8 (conv with the folded BatchNorm: out = s * relu(conv + b) + t, optionally its 2x2 max pooling as a second output, optionally
the 1x1 head's partial logits INSTEAD of the output), kind 9 (separate max pooling), kind 10 (head combine) and kind 6 (separate
head). References and bounds (tests/replay_ref.py; checked against a torch-f32 emulation in tests/test_replay_bounds_host.py):
  convs, on the first and the last image      1.2e-2 of the tensor max AND, per output channel, 1.2e-2 of the channel max (a channel
                                              below 1e-3 of the tensor max: 1.2e-5 of the tensor max) -- a wrong scale or shift on a
                                              small channel cannot hide under a large one
  s, t of every kind-8 launch                 1e-6 of the vector max against fp64 gamma / sqrt(var + eps), beta - mean * s
  pooled outputs, fused or kind 9             equal to the 2x2 max of the stored tensor (negative gammas: the pool follows the affine)
  partial logits of the fused head            p0 + p1 and each half of 32 channels against bf16round(ref) @ Wh:
                                              sum_c |Wh| * 2^-8 * |ref_c| + 1e-5 * sum_c |Wh * ref_c| per pixel and class
  probabilities (kind 10, kind 6)             2e-5 absolute against the fp64 softmax of the launch's own inputs
and completeness: 5 * depth + 2 conv launches, each conv once; exactly one head; `depth` pooled tensors; the returned
probabilities are the last head launch's output.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _devcopy import hip as _hip, d2h_bf16 as _d2h_bf16, d2h_f32 as _d2h_f32, d2h_u8 as _d2h_u8, d2h_rows as _d2h_rows

C_ = C                                                           # (the inference replay calls a channel count C)

pytestmark = pytest.mark.gpu
quiet = lambda *a, **k: None
CMP = 2


def _bf16_round(a):
    return torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).to(torch.float64)


def _layer_forward(mode, x_nhwc, w_hwio, bias):
    """y = conv(x) + b (pre-ReLU) of the reference layer: 3x3 SAME (mode 0) or UpSampling2D(2) + 2x2 SAME with
    TensorFlow's 0/1 padding (mode 1; mpunet/models/unet.py:148-160); NHWC in, NHWC out; fp64."""
    x = x_nhwc.permute(0, 3, 1, 2)
    w = w_hwio.permute(3, 2, 0, 1)
    if mode == 0:
        y = F.conv2d(x, w, bias, padding=1)
    else:
        up = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        y = F.conv2d(F.pad(up, (0, 1, 0, 1)), w, bias)
    return y.permute(0, 2, 3, 1)


def test_cfg1_bf16_step_every_conv_launch_against_fp64_on_its_own_inputs():
    _replay_conv_launches(16, 128, 1)


def test_default_yaml_network_cf2_every_conv_launch_against_fp64():
    """the same replay on the default project YAML's network (complexity_factor 2: 90 / 181 / 362 / 724 /
    1448 filters, every layer with channel tails; the concat weight gradients run as one job per source), B = 8 of 128 x 128."""
    _replay_conv_launches(8, 128, 2)


def test_configs3_per_gpu_share_every_conv_launch_against_fp64():
    """... and on one configs[3]-shaped step: 4 slices of 256 x 256 (the per-GPU share of the global batch 32 at N = 8)."""
    _replay_conv_launches(4, 256, 1)


def test_split_bf16_step_every_conv_launch_against_fp64():
    """dtype "bf16x3" (round 6): the same replay in the f32-storage / split-bf16-product mode -- forward and data gradients on the
    f32 kernels' split path, weight gradients as ONE bf16 reduction over three hi / lo plane pairs (batch 3 B) through the bf16
    schedules, grouped launches included. Each launch against fp64 on its own f32 inputs: 5e-5 of the tensor maximum (a product
    is good to ~2^-16), 240x tighter than the bf16 replay's bound."""
    _replay_conv_launches(4, 128, 1, dtype="bf16x3", tol_act=5e-5, tol_w=5e-5)


@pytest.mark.parametrize("B,cf", [(16, 1), (8, 2)], ids=["configs1", "default_yaml_cf2"])
def test_split_bf16_benchmarked_and_odd_channel_networks_every_conv_launch_against_fp64(B, cf):
    """The same at the BENCHMARKED shape (16 slices: all input planes in one launch, eleven layers on two stored planes through the
    grouped wgrad_taps launch, bias gradients out of the accumulators) and on the default-YAML network (complexity_factor 2:
    90 / 181 / 362 / 724 / 1448 filters -- channel counts that are no multiples of 64: three stored planes, concat sources as
    separate jobs, BatchNorms outside the folded kernels' shapes)."""
    _replay_conv_launches(B, 128, cf, dtype="bf16x3", tol_act=5e-5, tol_w=5e-5)


def _replay_conv_launches(B, dim, cf, dtype="bf16", tol_act=1.2e-2, tol_w=2e-3):
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    hip = _hip()
    K = 3
    w0 = U.init_weights(K, 1, 4, cf, seed=31)
    rng = np.random.RandomState(32)
    for k in w0:
        v = k.split("/")[1]
        if v == "bias":
            w0[k] = rng.uniform(-.1, .1, w0[k].shape).astype(np.float32)
        elif v == "gamma":
            w0[k] = rng.uniform(.5, 1.5, w0[k].shape).astype(np.float32)
            w0[k][0] = -0.8
        elif v == "beta":
            w0[k] = rng.uniform(-.3, .3, w0[k].shape).astype(np.float32)
    x = rng.randn(B, dim, dim, 1).astype(np.float32)
    y = (rng.randint(0, K, (B, dim, dim)) * (rng.rand(B, dim, dim) < 0.5)).astype(np.uint8).reshape(B, -1, 1)
    sw = np.where(np.arange(B) % 3 == 0, 0.33, 1.0).astype(np.float32)
    m = UNet(n_classes=K, dim=dim, n_channels=1, depth=4, complexity_factor=cf, flatten_output=True, dtype=dtype,
             logger=quiet)
    bf16 = dtype == "bf16"
    d2h = _d2h_bf16 if bf16 else _d2h_f32                       # activations / gradients as stored: bf16, or f32 ("bf16x3", "f32")
    m.set_weights_dict(w0)
    params = m.params.cpu().numpy()
    lib = _lib.load()
    torch.set_num_threads(max(1, torch.get_num_threads()))

    fwd_err, dg_err, wg_ref = [], [], []

    def kernel_of(li, kk):
        """bf16-rounded (as the MFMA operand) kernel [k][k][Cin_p][Cout_p] and fp32 bias of the layer."""
        Cin = li.C0 + li.C1 if li.kind != 1 else li.n_cnt_layer
        w = params[li.w_off:li.w_off + kk * kk * Cin * li.Cout].reshape(kk, kk, Cin, li.Cout)
        return (_bf16_round(w) if bf16 else torch.tensor(w, dtype=torch.float64)), \
            torch.tensor(params[li.b_off:li.b_off + li.Cout], dtype=torch.float64)

    class Rec:
        pass

    def on_launch(_user, pinfo):
        li = pinfo.contents
        torch.cuda.synchronize()
        kk = 2 if li.mode == 1 else 3
        r = Rec()
        for f, _t in _lib.LaunchInfo._fields_:
            setattr(r, f, getattr(li, f))
        Hi, Wi = (li.H // 2, li.W // 2) if li.mode == 1 else (li.H, li.W)     # kind 0 / 2: input resolution of the layer
        if li.kind == 0:
            r.n_cnt_layer = li.C0 + li.C1
            xin = d2h(hip, li.in0, (B, Hi, Wi, li.C0))[:CMP]
            if li.C1:
                xin = np.concatenate([xin, d2h(hip, li.in1, (B, Hi, Wi, li.C1))[:CMP]], -1)
            got = d2h(hip, li.out, (B, li.H, li.W, li.Cout))[:CMP]
            w, b = kernel_of(r, kk)
            ref = torch.relu(_layer_forward(li.mode, torch.tensor(xin), w, b)).numpy()
            fwd_err.append((li.conv_index, float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)), ref.shape))
        elif li.kind == 1:
            # data gradient w.r.t. input channels [n_off, n_off + n_cnt) of the layer; li.H/W = resolution of the result
            cin_layer = (params_shapes[li.conv_index])
            r.n_cnt_layer = cin_layer
            Hz, Wz = (2 * li.H, 2 * li.W) if li.mode == 1 else (li.H, li.W)
            dz = torch.tensor(d2h(hip, li.dz, (B, Hz, Wz, li.Cout))[:CMP])
            w, _b = kernel_of(r, kk)
            x0 = torch.zeros(CMP, li.H, li.W, cin_layer, dtype=torch.float64, requires_grad=True)
            _layer_forward(li.mode, x0, w, None).backward(dz)
            ref = x0.grad[..., li.n_off:li.n_off + li.n_cnt].numpy()
            if li.mask:
                ref = ref * (d2h(hip, li.mask, (B, li.H, li.W, li.n_cnt))[:CMP] > 0)
            got = d2h(hip, li.out, (B, li.H, li.W, li.n_cnt))[:CMP]
            dg_err.append((li.conv_index, li.n_off, float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)), ref.shape))
        elif li.kind == 2:
            # weight gradient: reference from the launch's x and dz (whole batch; fp32 mkldnn convolutions per chunk of
            # 4 images, chunk results accumulated in fp64: the chunk error ~1e-6 is far below the 2e-3 bound)
            xin = d2h(hip, li.in0, (B, Hi, Wi, li.C0))
            if li.C1:
                xin = np.concatenate([xin, d2h(hip, li.in1, (B, Hi, Wi, li.C1))], -1)
            dz = d2h(hip, li.dz, (B, li.H, li.W, li.Cout))
            Cin = li.C0 + li.C1
            dW = np.zeros((kk, kk, Cin, li.Cout), np.float64)
            for s in range(0, B, 4):
                wz = torch.zeros(kk, kk, Cin, li.Cout, dtype=torch.float32, requires_grad=True)
                _layer_forward(li.mode, torch.tensor(xin[s:s + 4], dtype=torch.float32), wz, None) \
                    .backward(torch.tensor(dz[s:s + 4], dtype=torch.float32))
                dW += wz.grad.numpy().astype(np.float64)
            wg_ref.append((li.conv_index, li.w_off, li.b_off, dW, dz.sum((0, 1, 2))))

    # input channels (padded) of every conv layer, by creation order (for the sliced data gradients)
    params_shapes = {}
    names = [n for n in m._keras_order() if n.endswith("/kernel")]
    for idx, n in enumerate(names):
        params_shapes[idx] = m._tensors[n][2][2]

    cb = _lib.LAUNCH_TAP_FN(on_launch)
    _lib.call("mpu_unet_set_launch_tap", m._h, C.cast(cb, C.c_void_p), None)
    lib.mpu_schedule_log_enable(1)
    try:
        m.forward_backward(x, y, sw)
        torch.cuda.synchronize()
        nlog = lib.mpu_schedule_log_read(None, 0)
        lbuf = C.create_string_buffer(int(nlog) + 1)
        lib.mpu_schedule_log_read(lbuf, nlog + 1)
    finally:
        lib.mpu_schedule_log_enable(0)
        _lib.call("mpu_unet_set_launch_tap", m._h, None, None)
    g = m.grads.cpu().numpy().astype(np.float64)

    assert len(fwd_err) == 22 and len(dg_err) == 25 and len(wg_ref) == 22, (len(fwd_err), len(dg_err), len(wg_ref))
    worst_f = max(fwd_err, key=lambda t: t[1]); worst_d = max(dg_err, key=lambda t: t[2])
    print("replay: forward launches worst rel-to-max error %.3g (conv %d), data-gradient launches %.3g (conv %d, offset %d)"
          % (worst_f[1], worst_f[0], worst_d[2], worst_d[0], worst_d[1]))
    for ci, e, shp in fwd_err:
        assert e <= tol_act, ("forward", ci, e, shp)
    for ci, off, e, shp in dg_err:
        assert e <= tol_act, ("dgrad", ci, off, e, shp)
    worst_w = 0.0
    for ci, w_off, b_off, dW, db in wg_ref:
        got = g[w_off:w_off + dW.size].reshape(dW.shape)
        e = np.abs(got - dW).max() / (np.abs(dW).max() + 1e-30)
        eb = np.abs(g[b_off:b_off + db.size] - db).max() / (np.abs(db).max() + 1e-30)
        worst_w = max(worst_w, e, eb)
        assert e <= tol_w and eb <= tol_w, ("wgrad", ci, e, eb)
    print("replay: weight / bias gradients of the 22 layers: worst rel-to-max error %.3g" % worst_w)


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_weight_gradient_reads_the_tensors_its_forward_read(dtype):
    """A conv's inputs are stated once, in the driver's layer table, and both passes resolve them from it. Depth 2 (the smallest
    network with both a first and a later encoder level and up block), 2 images of 16 x 16, 32 / 64 / 128 filters: for every conv
    the weight-gradient launch reports the input pointers, channel counts and output size of its forward launch, and every forward
    input is a tensor an earlier launch wrote -- a conv output, a BatchNorm output or its pooling -- or, for the first conv, the
    channel-padded input at the start of the workspace. Pointer and integer equality only."""
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.unet import UNet
    B, dim, K, depth = 2, 16, 3, 2
    rng = np.random.RandomState(7)
    x = rng.randn(B, dim, dim, 1).astype(np.float32)
    y = rng.randint(0, K, (B, dim * dim, 1)).astype(np.uint8)
    m = UNet(n_classes=K, dim=dim, n_channels=1, depth=depth, complexity_factor=0.25, dtype=dtype, logger=quiet, seed=3)
    recs = []

    def on_launch(_user, pinfo):
        recs.append({f: getattr(pinfo.contents, f) for f, _t in _lib.LaunchInfo._fields_})

    cb = _lib.LAUNCH_TAP_FN(on_launch)
    _lib.call("mpu_unet_set_launch_tap", m._h, C.cast(cb, C.c_void_p), None)
    try:
        m.forward_backward(x, y, None)
        torch.cuda.synchronize()
    finally:
        _lib.call("mpu_unet_set_launch_tap", m._h, None, None)
    n_conv = 2 * depth + 2 + 3 * depth                     # every conv but the 1x1 head
    fwd = {r["conv_index"]: r for r in recs if r["kind"] == 0}
    wg = {r["conv_index"]: r for r in recs if r["kind"] == 2}
    assert sorted(fwd) == sorted(wg) == list(range(n_conv))
    assert sum(r["kind"] == 0 for r in recs) == sum(r["kind"] == 2 for r in recs) == n_conv
    for ci in range(n_conv):
        for f in ("in0", "in1", "C0", "C1", "H", "W"):
            assert wg[ci][f] == fwd[ci][f], (ci, f, wg[ci][f], fwd[ci][f])
        assert fwd[ci]["in0"] and bool(fwd[ci]["in1"]) == (fwd[ci]["C1"] > 0), ci
    assert sum(fwd[ci]["C1"] > 0 for ci in fwd) == depth    # the concat conv of every up block
    written = set()
    for r in recs:
        if r["kind"] == 0:
            for f in ("in0", "in1"):
                if r[f] is None:
                    continue
                if r["conv_index"] == 0:
                    assert r[f] == m._ws.data_ptr(), (f, r[f])
                else:
                    assert r[f] in written, (r["conv_index"], f)
        if r["kind"] in (0, 3):
            written.update(p for p in (r["out"], r["mask"]) if p)


def test_cfg1_bf16_step_every_non_conv_launch_against_fp64_on_its_own_inputs():
    """the launch tap also reports the BatchNormalization forward / backward launches, the max-pool
    backward + skip add, the 1x1 head forward and the head backward of the benchmarked bf16 step; each is recomputed in fp64
    (NumPy / torch-CPU) from exactly the tensors the launch read and compared with what it stored. Tolerances: bf16 tensors
    1.2e-2 of the tensor max (one rounding of the stored value is 2^-9 relative; BatchNorm-backward outputs are differences
    of O(1) terms), fp32 reductions (batch statistics, dgamma / dbeta, head weight / bias gradients) 2e-3 of the tensor max,
    probabilities 2e-5 absolute."""
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    hip = _hip()
    B, dim, K = 16, 128, 3
    w0 = U.init_weights(K, 1, 4, 1, seed=41)
    rng = np.random.RandomState(42)
    for k in w0:
        v = k.split("/")[1]
        if v == "bias":
            w0[k] = rng.uniform(-.1, .1, w0[k].shape).astype(np.float32)
        elif v == "gamma":
            w0[k] = rng.uniform(.5, 1.5, w0[k].shape).astype(np.float32)
            w0[k][0] = -0.8                                  # a negative gamma: the pooling must follow the affine
        elif v == "beta":
            w0[k] = rng.uniform(-.3, .3, w0[k].shape).astype(np.float32)
    x = rng.randn(B, dim, dim, 1).astype(np.float32)
    y = (rng.randint(0, K, (B, dim, dim)) * (rng.rand(B, dim, dim) < 0.5)).astype(np.uint8).reshape(B, -1, 1)
    sw = np.where(np.arange(B) % 3 == 0, 0.33, 1.0).astype(np.float32)
    m = UNet(n_classes=K, dim=dim, n_channels=1, depth=4, complexity_factor=1, flatten_output=True, dtype="bf16",
             logger=quiet)
    m.set_weights_dict(w0)
    params = m.params.cpu().numpy().astype(np.float64)
    EPS = 1e-3
    rel = lambda got, ref: float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
    seen = {3: 0, 4: 0, 5: 0, 6: 0, 7: 0}
    worst = {3: 0.0, 4: 0.0, 5: 0.0, 6: 0.0, 7: 0.0}
    later = []                                             # (kind, w_off, b_off, ref at w_off, ref at b_off): gradients read after the pass

    def on_launch(_user, pinfo):
        li = pinfo.contents
        if li.kind < 3:
            return
        torch.cuda.synchronize()
        seen[li.kind] += 1
        H, W, Cc = li.H, li.W, li.C0
        if li.kind == 3:
            xx = _d2h_bf16(hip, li.in0, (B, H, W, Cc))
            got = _d2h_bf16(hip, li.out, (B, H, W, Cc))
            mean_d, inv_d = _d2h_f32(hip, li.aux0, (Cc,)), _d2h_f32(hip, li.aux1, (Cc,))
            g, bt = params[li.w_off:li.w_off + Cc], params[li.b_off:li.b_off + Cc]
            mu = xx.mean((0, 1, 2)); var = xx.var((0, 1, 2))
            inv = 1.0 / np.sqrt(var + EPS)
            e_stat = max(rel(mean_d, mu), rel(inv_d, inv))
            assert e_stat <= 1e-4, ("bn fwd statistics", li.conv_index, e_stat)
            ref = (xx - mu) * inv * g + bt
            e = rel(got, ref)
            assert e <= 1.2e-2, ("bn fwd", li.conv_index, e)
            worst[3] = max(worst[3], e)
            if li.mask:                                      # pooled = 2x2 max of the STORED (rounded) output, exactly
                pg = _d2h_bf16(hip, li.mask, (B, H // 2, W // 2, Cc))
                pr = got.reshape(B, H // 2, 2, W // 2, 2, Cc).max((2, 4))
                assert np.array_equal(pg, pr), ("bn fwd pooled", li.conv_index)
        elif li.kind == 4:
            dn = _d2h_bf16(hip, li.in0, (B, H, W, Cc)); xx = _d2h_bf16(hip, li.in1, (B, H, W, Cc))
            got = _d2h_bf16(hip, li.out, (B, H, W, Cc))
            mean_d, inv_d = _d2h_f32(hip, li.aux0, (Cc,)), _d2h_f32(hip, li.aux1, (Cc,))
            g = params[li.w_off:li.w_off + Cc]
            xh = (xx - mean_d) * inv_d
            M = float(B * H * W)
            dbeta = dn.sum((0, 1, 2)); dgamma = (dn * xh).sum((0, 1, 2))
            dxx = g * inv_d * (dn - dbeta / M - xh * dgamma / M)
            ref = np.where(xx > 0, dxx, 0.0)
            e = rel(got, ref)
            assert e <= 1.2e-2, ("bn bwd dz", li.conv_index, e)
            worst[4] = max(worst[4], e)
            later.append((4, li.w_off, li.b_off, dgamma, dbeta))
        elif li.kind == 5:
            n_ = _d2h_bf16(hip, li.in0, (B, H, W, Cc)); ds = _d2h_bf16(hip, li.in1, (B, H, W, Cc))
            dp = _d2h_bf16(hip, li.dz, (B, H // 2, W // 2, Cc))
            got = _d2h_bf16(hip, li.out, (B, H, W, Cc))
            win = n_.reshape(B, H // 2, 2, W // 2, 2, Cc).transpose(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, Cc, 4)
            first = win.argmax(-1)                           # np.argmax: the FIRST maximum, row-major inside the window
            routed = np.zeros_like(win)
            np.put_along_axis(routed, first[..., None], dp[..., None], -1)
            routed = routed.reshape(B, H // 2, W // 2, Cc, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, H, W, Cc)
            ref = ds + routed
            e = float((np.abs(got - ref) / (np.abs(ref) + 1e-6 * np.abs(ref).max())).max())
            assert e <= 2.0 ** -8, ("maxpool bwd + skip", li.conv_index, e)        # one bf16 rounding of an exact sum
            worst[5] = max(worst[5], e)
        elif li.kind == 6:
            n_ = _d2h_bf16(hip, li.in0, (B, H, W, Cc))
            got = _d2h_f32(hip, li.out, (B, H, W, li.Cout))
            Wh = params[li.w_off:li.w_off + Cc * li.Cout].reshape(Cc, li.Cout); bh = params[li.b_off:li.b_off + li.Cout]
            z = n_ @ Wh + bh
            ez = np.exp(z - z.max(-1, keepdims=True))
            ref = ez / ez.sum(-1, keepdims=True)
            e = float(np.abs(got - ref).max())
            assert e <= 2e-5, ("head fwd", e)
            worst[6] = max(worst[6], e)
        elif li.kind == 7:
            n_ = torch.tensor(_d2h_bf16(hip, li.in0, (B, H, W, Cc)), requires_grad=True)
            yy = torch.tensor(_d2h_u8(hip, li.dz, (B, H, W)).astype(np.int64))
            ww = torch.tensor(_d2h_f32(hip, li.mask, (B,)) if li.mask else np.ones(B))
            Wh = torch.tensor(params[li.w_off:li.w_off + Cc * li.Cout].reshape(Cc, li.Cout), requires_grad=True)
            bh = torch.tensor(params[li.b_off:li.b_off + li.Cout], requires_grad=True)
            probs = torch.softmax(n_ @ Wh + bh, -1)
            U.keras_sparse_ce(probs, yy, ww).sum().backward()
            got = _d2h_bf16(hip, li.out, (B, H, W, Cc))
            e = rel(got, n_.grad.numpy())
            assert e <= 1.2e-2, ("head bwd dn", e)
            worst[7] = max(worst[7], e)
            later.append((7, li.w_off, li.b_off, Wh.grad.numpy().ravel(), bh.grad.numpy()))

    cb = _lib.LAUNCH_TAP_FN(on_launch)
    _lib.call("mpu_unet_set_launch_tap", m._h, C.cast(cb, C.c_void_p), None)
    try:
        m.forward_backward(x, y, sw)
        torch.cuda.synchronize()
    finally:
        _lib.call("mpu_unet_set_launch_tap", m._h, None, None)
    g = m.grads.cpu().numpy().astype(np.float64)
    assert seen == {3: 13, 4: 13, 5: 4, 6: 1, 7: 1}, seen
    worst_red = 0.0
    for kind, w_off, b_off, rw, rb in later:
        ew, eb = rel(g[w_off:w_off + rw.size], rw), rel(g[b_off:b_off + rb.size], rb)
        worst_red = max(worst_red, ew, eb)
        assert ew <= 2e-3 and eb <= 2e-3, (kind, w_off, ew, eb)
    print("replay (non-conv): bn fwd %.3g, bn bwd %.3g, pool bwd %.3g, head fwd %.3g (abs), head bwd %.3g; fp32 reductions %.3g"
          % (worst[3], worst[4], worst[5], worst[6], worst[7], worst_red))


# ---- the inference forward (run_forward_infer), launch by launch -------------------------------------------------------------
def _replay_inference(K, C, depth, cf, B, H, W, tag="", seed=21):
    """One bf16 inference forward with the launch tap and the schedule log on. Every launch it reports (kinds 0, 6, 8, 9, 10 of
    mpu_launch_info) is recomputed on torch-CPU / NumPy in fp64 from the launch's own inputs and compared under the bounds of
    tests/replay_ref.py; conv outputs on the first and the last image of the batch (the last one sits in the ragged tail of the
    tile walk), everything else on the whole batch. Returns what the callers assert their schedules from."""
    import replay_ref as R
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    from test_gpu_unet import rand_weights
    hip = _hip()
    w0 = rand_weights(U, K, C, depth, cf, seed=seed)
    x = np.random.RandomState(seed + 2).randn(B, H, W, C).astype(np.float32)
    m = UNet(n_classes=K, img_rows=H, img_cols=W, n_channels=C, depth=depth, complexity_factor=cf, dtype="bf16", logger=quiet)
    m.set_weights_dict(w0)
    params = m.params.cpu().numpy().astype(np.float64)
    state = m.bn_state.cpu().numpy().astype(np.float64)
    bn_names = [n[:-len("/gamma")] for n in m._keras_order() if n.endswith("/gamma")]
    _k, hw_off, hps, _l = m._tensors["conv2d/kernel"]
    head_C = hps[2]
    Wh_all = params[hw_off:hw_off + head_C * K].reshape(head_C, K)
    bh_off = m._tensors["conv2d/bias"][1]
    imgs = sorted({0, B - 1})
    lib = _lib.load()
    EPS = 1e-3

    def rows(ptr, shape):                                   # the compared images of a device bf16 tensor, fp64
        return torch.cat([_d2h_rows(hip, ptr, shape, True, i, i + 1) for i in imgs])

    recs, failures = [], []
    worst = {"tensor": 0.0, "channel": 0.0, "coeff": 0.0, "head_partial": 0.0, "combine": 0.0, "head": 0.0}
    last_head_out = [None]

    def check(li):
        kind = li.kind
        rec = {"kind": kind, "conv_index": li.conv_index, "pooled": bool(li.mask) if kind == 8 else kind == 9,
               "head": kind == 8 and bool(li.dz), "bn": li.n_off if kind == 8 else -1}
        recs.append(rec)
        Hh, Ww = li.H, li.W
        if kind in (0, 8):
            kk = 2 if li.mode == 1 else 3
            Hi, Wi = (Hh // 2, Ww // 2) if li.mode == 1 else (Hh, Ww)
            Cin, Co = li.C0 + li.C1, li.Cout
            xin = rows(li.in0, (B, Hi, Wi, li.C0))
            if li.C1:
                xin = torch.cat([xin, rows(li.in1, (B, Hi, Wi, li.C1))], -1)
            wk = _bf16_round(params[li.w_off:li.w_off + kk * kk * Cin * Co].reshape(kk, kk, Cin, Co))
            bk = torch.tensor(params[li.b_off:li.b_off + Co])
            if kind == 8:
                assert li.aux0 and li.aux1 and 0 <= li.n_off < len(bn_names), ("kind 8 fields", li.conv_index, li.n_off)
                s, t = _d2h_f32(hip, li.aux0, (Co,)), _d2h_f32(hip, li.aux1, (Co,))
                tn = lambda v: m._tensors[bn_names[li.n_off] + "/" + v]
                assert tn("gamma")[2] == (Co,), (li.conv_index, li.n_off, tn("gamma")[2], Co)
                g, bt = params[tn("gamma")[1]:][:Co], params[tn("beta")[1]:][:Co]
                mm, mv = state[tn("moving_mean")[1]:][:Co], state[tn("moving_variance")[1]:][:Co]
                s_ref = g / np.sqrt(mv + EPS); t_ref = bt - mm * s_ref
                e = max(np.abs(s - s_ref).max() / np.abs(s_ref).max(), np.abs(t - t_ref).max() / np.abs(t_ref).max())
                worst["coeff"] = max(worst["coeff"], float(e))
                assert e <= 1e-6, ("folded BatchNorm coefficients", li.conv_index, li.n_off, e)
            else:
                s, t = np.ones(Co), np.zeros(Co)
            ref = R.affine_relu_conv(li.mode, xin, wk, bk, torch.tensor(s), torch.tensor(t)).numpy()
            if li.out:
                got = rows(li.out, (B, Hh, Ww, Co)).numpy()
                e_t, e_c, c = R.conv_bound_ratios(got, ref)
                rec["e_t"], rec["e_c"] = e_t, e_c
                worst["tensor"], worst["channel"] = max(worst["tensor"], e_t), max(worst["channel"], e_c)
                assert e_t <= R.CONV_TOL, ("conv, tensor-wise", kind, li.conv_index, e_t, ref.shape)
                assert e_c <= 1.0, ("conv, per channel (fraction of its bound)", kind, li.conv_index, c, e_c, ref.shape)
            else:
                assert kind == 8 and li.dz, ("a conv launch without an output", kind, li.conv_index)
            if kind == 8 and li.mask:                       # pooled = 2x2 max of the STORED output, exactly
                assert li.out, ("pooled output without the tensor it pools", li.conv_index)
                full = _d2h_bf16(hip, li.out, (B, Hh, Ww, Co))
                assert np.array_equal(_d2h_bf16(hip, li.mask, (B, Hh // 2, Ww // 2, Co)), R.pool2x2(full)), \
                    ("fused pool", li.conv_index)
            if kind == 8 and li.dz:                         # the head out of the epilogue: two halves of 32 channels, no bias
                assert Co == head_C == 64 and li.out is None, ("fused head", Co, head_C, li.out)
                part = _d2h_f32(hip, li.dz, (2, B, Hh, Ww, K))[:, imgs]
                e = max(R.head_partial_ratio(part[0] + part[1], ref, Wh_all),
                        R.head_partial_ratio(part[0], ref[..., :32], Wh_all[:32]),
                        R.head_partial_ratio(part[1], ref[..., 32:], Wh_all[32:]))
                worst["head_partial"] = max(worst["head_partial"], e)
                assert e <= 1.0, ("fused head partial logits (fraction of the bound)", e)
        elif kind == 9:
            yy = _d2h_bf16(hip, li.in0, (B, Hh, Ww, li.C0))
            assert np.array_equal(_d2h_bf16(hip, li.out, (B, Hh // 2, Ww // 2, li.C0)), R.pool2x2(yy)), ("maxpool", li.conv_index)
        elif kind in (6, 10):
            bh = params[li.b_off:li.b_off + li.Cout]
            assert li.Cout == K and li.b_off == bh_off and li.w_off == hw_off, ("head fields", li.Cout, li.w_off, li.b_off)
            got = _d2h_f32(hip, li.out, (B, Hh, Ww, K))
            if kind == 10:
                part = _d2h_f32(hip, li.in0, (2, B, Hh, Ww, K))
                e = float(np.abs(got - R.softmax64(part[0] + part[1] + bh)).max())
                worst["combine"] = max(worst["combine"], e)
            else:
                n_ = _d2h_bf16(hip, li.in0, (B, Hh, Ww, li.C0))
                e = float(np.abs(got - R.softmax64(n_ @ Wh_all + bh)).max())
                worst["head"] = max(worst["head"], e)
            assert e <= 2e-5, ("head probabilities", kind, e)
            last_head_out[0] = got

    def on_launch(_user, pinfo):                            # (an exception cannot cross the C frame: kept for the caller)
        try:
            torch.cuda.synchronize()
            check(pinfo.contents)
        except BaseException as e:
            import traceback
            failures.append("%r\n%s" % (e, traceback.format_exc(limit=3)))

    cb = _lib.LAUNCH_TAP_FN(on_launch)
    _lib.call("mpu_unet_set_launch_tap", m._h, C_.cast(cb, C_.c_void_p), None)
    lib.mpu_schedule_log_enable(1)
    try:
        probs = m._forward(m._as_input(x), training=False)
        torch.cuda.synchronize()
        nlog = lib.mpu_schedule_log_read(None, 0)
        lbuf = C_.create_string_buffer(int(nlog) + 1)
        lib.mpu_schedule_log_read(lbuf, nlog + 1)
    finally:
        lib.mpu_schedule_log_enable(0)
        _lib.call("mpu_unet_set_launch_tap", m._h, None, None)
    assert not failures, "%d launches failed; the first:\n%s" % (len(failures), failures[0])

    # completeness: every conv exactly once, one head, `depth` pooled tensors, and the returned probabilities are the head's
    convs = [r for r in recs if r["kind"] in (0, 8)]
    lines = [l for l in lbuf.value.decode().splitlines() if l.startswith("conv ")]
    assert sorted(r["conv_index"] for r in convs) == list(range(5 * depth + 2)), sorted(r["conv_index"] for r in convs)
    assert len(lines) == len(convs), (len(lines), len(convs))
    for r, l in zip(convs, lines):
        r["sched"] = l.split()[1]
        assert ("pool=1" in l) == r["pooled"] and ("head=1" in l) == r["head"], (l, r)
    assert sum(r["kind"] == 8 for r in recs) == 3 * depth + 1 and sum(r["kind"] == 0 for r in recs) == 2 * depth + 1
    heads = [r["kind"] for r in recs if r["kind"] in (6, 10) or r["head"]]
    assert heads in ([6], [8, 10]), heads
    assert recs[-1]["kind"] in (6, 10)
    assert sum(r["pooled"] for r in recs) == depth, [(r["kind"], r["conv_index"]) for r in recs if r["pooled"]]
    assert np.array_equal(probs.cpu().numpy().astype(np.float64), last_head_out[0])
    by = {}
    for r in recs:
        key = "%d:%s" % (r["kind"], r.get("sched", "-")) + ("+pool" if r["kind"] == 8 and r["pooled"] else "") + \
              ("+head" if r["head"] else "")
        by[key] = by.get(key, 0) + 1
    print("replay (inference %s): %d conv launches worst %.3g of the tensor max, per channel %.3g of its bound, coefficients %.3g; "
          "head partials %.3g of their bound, combine %.3g abs, head kernel %.3g abs; kind:schedule %s"
          % (tag, len(convs), worst["tensor"], worst["channel"], worst["coeff"], worst["head_partial"], worst["combine"],
             worst["head"], " ".join("%s=%d" % kv for kv in sorted(by.items()))))
    return {"recs": recs, "lines": lines, "worst": worst, "depth": depth}


def _kinds(res):
    return [r["kind"] for r in res["recs"]]


def test_inference_net_a_ws_fused_pool_and_head_halo_splitk_every_launch_against_fp64():
    """Network A: K 3, depth 3, cf 1, 8 images of 128 x 160 -- 1280 tiles at level 0: conv_ws with the fused pool and the fused
    head (K <= 8); levels 1-2 on the halo kernels with a ragged W tile (80 = 2.5 x 32); the deep levels on the split-K / glds
    schedules. The schedule switches of test_inference_net_a_under_schedule_switches_subprocess are read from the environment
    (once per process by the library): what each forces is asserted here."""
    import os
    res = _replay_inference(3, 1, 3, 1, 8, 128, 160, tag="A")
    lines, kinds = res["lines"], _kinds(res)
    unfused = os.environ.get("MPU_FUSED_POOL") == "0" and os.environ.get("MPU_FUSED_HEAD") == "0"
    if unfused:
        assert kinds.count(9) == 3 and kinds.count(6) == 1 and kinds.count(10) == 0, kinds
        assert not any("pool=1" in l or "head=1" in l for l in lines), lines
    else:
        assert any(l.split()[1] == "ws" and "head=1" in l for l in lines), lines
        assert sum("pool=1" in l for l in lines) >= 2, lines
        assert kinds.count(10) == 1 and kinds.count(6) == 0, kinds
    if os.environ.get("MPU_HALO16_MIN") == "1" and os.environ.get("MPU_HALO16P_WGS") == "5":
        p = [l for l in lines if l.split()[1] == "halo16p"]
        assert len(p) >= 6 and any("pool=1" in l for l in p), lines


def test_inference_net_b_channel_tails_unfused_head_every_launch_against_fp64():
    """Network B: K 5, 2 input channels, depth 2, cf 2 (90 / 181 / 362 filters: channel tails in every layer and in the scale /
    shift vectors), 3 images of 48 x 40; the head runs as its own kernel (kind 6)."""
    res = _replay_inference(5, 2, 2, 2, 3, 48, 40, tag="B")
    assert _kinds(res).count(6) == 1 and _kinds(res).count(10) == 0, _kinds(res)


def test_inference_net_c_wide_fused_head_every_launch_against_fp64():
    """Network C: K 16, depth 1, 8 images of 128 x 128 (1024 tiles: exactly conv_ws's bound): the wide (K <= 16) fused head."""
    res = _replay_inference(16, 1, 1, 1, 8, 128, 128, tag="C")
    assert any(l.split()[1] == "ws" and "head=1" in l for l in res["lines"]), res["lines"]
    assert _kinds(res).count(10) == 1, _kinds(res)


def test_inference_net_d_tiny_maps_separate_maxpool_every_launch_against_fp64():
    """Network D: K 3, depth 4, cf 0.25, 5 images of 16 x 32: the bottom works on 1 x 2 maps, the last pooling goes 2 x 4 -> 1 x 2,
    and W < 32 below level 0 keeps the layers off the patch kernels and the pooling mostly on the separate kernel (kind 9)."""
    res = _replay_inference(3, 1, 4, 0.25, 5, 16, 32, tag="D")
    assert _kinds(res).count(9) >= 1, _kinds(res)


@pytest.mark.parametrize("switches", [{"MPU_HALO16_MIN": "1", "MPU_HALO16P_WGS": "5"},
                                      {"MPU_FUSED_POOL": "0", "MPU_FUSED_HEAD": "0"},
                                      {"MPU_HALO_UP8_MIN": "1"}], ids=["halo16p_5wgs", "unfused_pool_and_head", "halo_up8"])
def test_inference_net_a_under_schedule_switches_subprocess(switches):
    """The library reads a schedule switch once per process, hence a fresh interpreter per set, one at a time: network A's replay
    under the persistent 16-row kernel on every eligible layer with 5 workgroups (each walks many tiles), with the separate
    max-pool and head kernels, and with the 8-row up-conv schedule from the smallest grid on."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_replay.py"), "-x", "-q", "-s", "-k",
                        "test_inference_net_a_ws_fused_pool_and_head"], env=dict(os.environ, **switches), capture_output=True,
                       text=True, cwd=os.path.dirname(here))
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("replay (inference")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]
