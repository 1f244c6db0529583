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

CHECKS INSIDE A TAP NEVER ASSERT DIRECTLY. The tap is a ctypes callback: an exception cannot cross its C frame, pytest only
warns, and the test passes. Every tap of the suite is installed by replay_tap.tapped(model, check), which records what a check
raises and fails the test after the pass, naming the launch (host test: tests/test_replay_bounds_host.py).

The references of kinds 0-7 live once, in _StepChecks (bounds: its docstring and tests/replay_ref.py), and serve the conv replays
above, the non-conv replay of configs[1] and _replay_train_step: ONE tapped step of a small odd network, every kind in one pass,
all images, in bf16 and bf16x3 (T1 also f32):
  T1  K 5, 2 channels, depth 2, cf 2 (90 / 181 / 362), 3 x 48 x 40    channel tails in every conv and every non-conv kind, BatchNorms off
                                                                     the accumulator path, concat sources as separate jobs, odd batch
  T2  K 3, depth 4, cf 0.25 (32 ... 512), 5 x 16 x 32                 bottom on 1 x 2 maps, pool backward 2 x 4 -> 1 x 2, statistics over 10 values
  T3  K 3, depth 2, cf 1 (64 / 128 / 256), 3 x 32 x 160               every BatchNorm on the folded / accumulator kernels; W = 80 = 2.5 tiles
                                                                     of 32 at level 1; also under the step's three schedule switches
  T4  K 8, depth 1, cf 1, 2 x 32 x 32                                 the widest head that trains (TRAIN_MAX_CLASSES)
Completeness from the depth D: forward convs and weight gradients 5 D + 2 (each conv index once), data gradients 6 D + 1, BatchNorm
forward and backward 3 D + 1 each, pool backward D, head forward and head backward one each (D = 4: 22 / 25 / 22 / 13 / 13 / 4 / 1 / 1).
Two forms of the step switch themselves off under a tap -- the fused training head (unet_model.hip: head_train_fused_wanted) and the
pool-backward recompute --, so the replays above see the unfused kernels; tests/test_gpu_unet.py pins the two forms against those bit
for bit. mpu_unet_set_launch_tap_fused(m, 1) keeps them on under the tap: they are the DEFAULT of the benchmarked bf16 step, and
_replay_fused_step (FUSED_CASES H1-H5, P1-P4) replays them as kinds 11 (head_bn_forward), 12 (head_bn_backward + head_bn_bwd_apply)
and 13 (both pool-recompute kernels) against fp64 -- at the ragged last pixel group of both storages, in the second grid-stride round
of each head pass, at every channel width of the pool passes and on a 7-workgroup grid (bounds: _StepChecks._kind11 / 12 / 13).

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
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _devcopy import hip as _hip, d2h_bf16 as _d2h_bf16, d2h_f32 as _d2h_f32, d2h_u8 as _d2h_u8, d2h_rows as _d2h_rows

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


def _train_case(K, C, depth, cf, B, H, W, dtype, seed, sw_period):
    """Model, inputs, labels (zero on about half the pixels) and per-image weights (1.0 / 0.33) of one replayed train step: Glorot
    kernels, random biases / betas, gammas in [0.5, 1.5] with one negative per BatchNorm (the pooling must follow the affine)."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    w0 = U.init_weights(K, C, depth, cf, seed=seed)
    rng = np.random.RandomState(seed + 1)
    for k in w0:
        v = k.split("/")[1]
        if v == "bias":
            w0[k] = rng.uniform(-.1, .1, w0[k].shape).astype(np.float32)
        elif v == "gamma":
            w0[k] = rng.uniform(.5, 1.5, w0[k].shape).astype(np.float32)
            w0[k][0] = -0.8
        elif v == "beta":
            w0[k] = rng.uniform(-.3, .3, w0[k].shape).astype(np.float32)
    x = rng.randn(B, H, W, C).astype(np.float32)
    y = (rng.randint(0, K, (B, H, W)) * (rng.rand(B, H, W) < 0.5)).astype(np.uint8).reshape(B, -1, 1)
    sw = np.where(np.arange(B) % sw_period == 0, 0.33, 1.0).astype(np.float32)
    m = UNet(n_classes=K, img_rows=H, img_cols=W, n_channels=C, depth=depth, complexity_factor=cf, flatten_output=True,
             dtype=dtype, logger=quiet)
    m.set_weights_dict(w0)
    return m, x, y, sw


def _env_on(name):
    import os
    return os.environ.get(name, "1") != "0"


class _StepChecks:
    """The references of one tapped train step, launch by launch (kinds 0-7 of mpu_launch_info), shared by every train-step
    replay of this module. check(li) recomputes the launch in fp64 (torch-CPU / NumPy) from the tensors THAT launch read and
    compares with what it stored; it runs inside replay_tap.tapped and raises ONE AssertionError per launch, after all of the
    launch's comparisons and after its after-the-pass references (weight / bias gradients, dgamma / dbeta, dWh / dbh: read from
    the gradient buffer by finish()) are recorded -- a launch that fails one check still gets its reductions checked.

    Bounds (tests/replay_ref.py: TOL_BF16, TOL_F32), each as a fraction of the tensor maximum unless stated:
      kind 0 forward conv, 1 data gradient   conv: 1.2e-2 (bf16) / 5e-5 (f32 storage); kind 0 also per output channel (bf16, f32) or, in
                                             bf16x3, per element against X3_PRODUCT * (sum |x| |w| + |b|)
      kind 2 weight / bias gradient          wgrad: 2e-3 / 5e-5, after the pass
      kind 3 BatchNorm forward               statistics against fp64 E[x], 1 / sqrt(E[x^2] - E[x]^2 + eps): stats, plus -- where they come
                                             out of the fixed-point accumulators -- the derived error of the units (acc_stats_error);
                                             output against gamma * (x - mean_d) * inv_d + beta with the DEVICE statistics: out (one
                                             rounding), tensor-wise and per channel; pooled output: exact 2x2 max of the stored output
      kind 4 BatchNorm backward              dz from the device statistics: out, tensor-wise and per channel; dgamma / dbeta: reduce
                                             (+ half a 2^-40 unit per add in accumulator mode), after the pass
      kind 5 max-pool backward + skip add    one rounding of an exact sum, per element: pool (2^-8 / 2^-24)
      kind 6 head forward                    probs: 2e-5 absolute
      kind 7 head backward                   dn: out; dWh / dbh: reduce, after the pass
    worst[...] holds the worst error of each family as a FRACTION OF ITS BOUND."""

    def __init__(self, m, B, dtype, imgs, kinds=range(8), derived=True, by_image=False, elem_imgs=None):
        import replay_ref as R
        from oracle import unet_ref as U
        self.R, self.U, self.m, self.B, self.dtype = R, U, m, B, dtype
        self.hip = _hip()
        self.bf16 = dtype == "bf16"
        self.tol = R.TOL_BF16 if self.bf16 else R.TOL_F32
        self.imgs = list(imgs)
        self.kinds = set(kinds)
        self.params = m.params.cpu().numpy().astype(np.float64)
        names = [n for n in m._keras_order() if n.endswith("/kernel")]
        self.cin_of = {idx: m._tensors[n][2][2] for idx, n in enumerate(names)}       # padded input channels, by creation order
        # the fixed-point accumulators can be behind a BatchNorm's statistics / sums (unet_model.hip: make_run, acc_mode): the error
        # derived from their units is added to those bounds (derived=False: the benchmarked-shape tests keep their plain bounds)
        self.head_out, self.x3_per_channel = None, 0.0
        self.acc_mode = derived and dtype in ("bf16", "bf16x3") and _env_on("MPU_BN_ATOMIC") and _env_on("MPU_BN_FOLD") and _env_on("MPU_FUSED_BN_STATS")
        self.seen = []                                         # (kind, conv_index) of every launch checked
        self.all_kinds = {}                                    # kind -> launches reported, checked or not
        self.worst = {}
        self.later = []                                        # (what, index, offset into grads, reference, tol, absolute extra)
        self.stats_plain = 0.0                                 # worst statistics error as a fraction of the bound WITHOUT the derived term
        self._bad = None
        # kinds 11-13 (the fused forms, mpu_unet_set_launch_tap_fused): evaluated image by image; by_image: kind 3 as well (the large
        # cases); elem_imgs: the images whose ELEMENTS are compared (default: all) -- every reduction runs over the whole batch
        self.by_image = by_image
        self.elem_imgs = list(range(B)) if elem_imgs is None else sorted(set(elem_imgs))
        self.bn_offs = {}                                      # BatchNorm index -> (gamma, beta) offsets, from its kind-3 record
        self.ties = []                                         # per kind-13 launch: (level's C, tied windows, windows)
        self.fused_probs = None                                # the kind-11 launch's output

    # -- device tensors as stored: bf16, or f32 (dtypes "bf16x3", "f32"); fp64 on the host, exact
    def rows(self, ptr, shape, imgs=None):
        imgs = range(self.B) if imgs is None else imgs
        return torch.cat([_d2h_rows(self.hip, ptr, shape, self.bf16, i, i + 1) for i in imgs])

    def hold(self, what, li, err, bound, detail=None):
        r = float(err / bound) if bound > 0 else (0.0 if err == 0 else float("inf"))
        self.worst[what] = float(np.max([self.worst.get(what, 0.0), r]))             # (np.max: a NaN stays visible)
        if not r <= 1.0:
            self._bad.append((what, "kind %d" % li.kind, "index %d" % li.conv_index, "error / bound %.3g" % r, detail))

    def hold_tensor(self, what, li, got, ref, tol, per_channel, note=None):
        e_t, e_c, c = self.R.conv_bound_ratios(got, ref, tol)
        self.hold(what, li, e_t, tol, ("tensor-wise", tuple(ref.shape), note))
        if per_channel:
            self.hold(what + ", per channel", li, e_c, 1.0, ("channel %d" % c, tuple(ref.shape), note))

    def check(self, li):
        self.all_kinds[li.kind] = self.all_kinds.get(li.kind, 0) + 1
        if li.kind not in self.kinds:
            return
        self.seen.append((li.kind, li.conv_index))
        self._bad = []
        getattr(self, "_kind%d" % li.kind)(li)
        assert not self._bad, self._bad

    def kernel_of(self, li, kk, Cin):
        """bf16-rounded (as the MFMA operand; f32 storage: as stored) kernel [k][k][Cin_p][Cout_p] and fp32 bias of the layer."""
        w = self.params[li.w_off:li.w_off + kk * kk * Cin * li.Cout].reshape(kk, kk, Cin, li.Cout)
        return (_bf16_round(w) if self.bf16 else torch.tensor(w)), torch.tensor(self.params[li.b_off:li.b_off + li.Cout])

    def _kind0(self, li):
        B, kk = self.B, 2 if li.mode == 1 else 3
        Hi, Wi = (li.H // 2, li.W // 2) if li.mode == 1 else (li.H, li.W)
        xin = self.rows(li.in0, (B, Hi, Wi, li.C0), self.imgs)
        if li.C1:
            xin = torch.cat([xin, self.rows(li.in1, (B, Hi, Wi, li.C1), self.imgs)], -1)
        got = self.rows(li.out, (B, li.H, li.W, li.Cout), self.imgs).numpy()
        w, b = self.kernel_of(li, kk, li.C0 + li.C1)
        ref = torch.relu(_layer_forward(li.mode, xin, w, b)).numpy()
        if self.dtype != "bf16x3":
            self.hold_tensor("forward conv", li, got, ref, self.tol["conv"], True)
            return
        # dtype "bf16x3": a PRODUCT is inexact (replay_ref.X3_PRODUCT), so the error of an output follows sum |x| |w|, not the output:
        # a channel whose terms cancel cannot be held to a fraction of its own maximum. Tensor-wise as before; in place of the
        # per-channel rule every ELEMENT is held to the bound its own operands give -- a small channel cannot hide here either
        self.hold_tensor("forward conv", li, got, ref, self.tol["conv"], False)
        mag = _layer_forward(li.mode, xin.abs(), w.abs(), b.abs()).numpy()
        e = float((np.abs(got - ref) / (self.R.X3_PRODUCT * mag + 1e-300)).max())
        self.hold("forward conv, per element (split products)", li, e, 1.0, tuple(ref.shape))
        e_c = self.R.conv_bound_ratios(got, ref, self.tol["conv"])[1]                  # (reported, not held: see above)
        self.x3_per_channel = max(self.x3_per_channel, e_c)

    def _kind1(self, li):
        # data gradient w.r.t. input channels [n_off, n_off + n_cnt) of the layer; li.H/W = resolution of the result
        B, kk, n = self.B, 2 if li.mode == 1 else 3, len(self.imgs)
        cin_layer = self.cin_of[li.conv_index]
        Hz, Wz = (2 * li.H, 2 * li.W) if li.mode == 1 else (li.H, li.W)
        dz = self.rows(li.dz, (B, Hz, Wz, li.Cout), self.imgs)
        w, _b = self.kernel_of(li, kk, cin_layer)
        x0 = torch.zeros(n, li.H, li.W, cin_layer, dtype=torch.float64, requires_grad=True)
        _layer_forward(li.mode, x0, w, None).backward(dz)
        ref = x0.grad[..., li.n_off:li.n_off + li.n_cnt].numpy()
        if li.mask:
            ref = ref * (self.rows(li.mask, (B, li.H, li.W, li.n_cnt), self.imgs).numpy() > 0)
        got = self.rows(li.out, (B, li.H, li.W, li.n_cnt), self.imgs).numpy()
        self.hold_tensor("data gradient", li, got, ref, self.tol["conv"], False, "channel offset %d" % li.n_off)

    def _kind2(self, li):
        # weight gradient: reference from the launch's x and dz (whole batch; fp32 mkldnn convolutions per chunk of 4 images,
        # chunk results accumulated in fp64: the chunk error ~1e-6 is far below the bounds)
        B, kk = self.B, 2 if li.mode == 1 else 3
        Hi, Wi = (li.H // 2, li.W // 2) if li.mode == 1 else (li.H, li.W)
        xin = self.rows(li.in0, (B, Hi, Wi, li.C0))
        if li.C1:
            xin = torch.cat([xin, self.rows(li.in1, (B, Hi, Wi, li.C1))], -1)
        dz = self.rows(li.dz, (B, li.H, li.W, li.Cout))
        Cin = li.C0 + li.C1
        dW = np.zeros((kk, kk, Cin, li.Cout), np.float64)
        for s in range(0, B, 4):
            wz = torch.zeros(kk, kk, Cin, li.Cout, dtype=torch.float32, requires_grad=True)
            _layer_forward(li.mode, xin[s:s + 4].to(torch.float32), wz, None).backward(dz[s:s + 4].to(torch.float32))
            dW += wz.grad.numpy().astype(np.float64)
        # (dtype "bf16x3" in accumulator mode: the bias gradient comes out of 2^-44 units, half a unit per workgroup add)
        extra = self.R.acc_sum_error(B * li.H * li.W, self.R.DB_ACC_SCALE) if self.dtype == "bf16x3" and self.acc_mode else 0.0
        self.later.append(("weight gradient", li.conv_index, li.w_off, dW.ravel(), self.tol["wgrad"], 0.0))
        self.later.append(("bias gradient", li.conv_index, li.b_off, dz.sum((0, 1, 2)).numpy(), self.tol["wgrad"], extra))

    def _kind3(self, li):
        R, B, H, W, Cc = self.R, self.B, li.H, li.W, li.C0
        self.bn_offs[li.conv_index] = (li.w_off, li.b_off)
        if self.by_image and B * H * W > 1:
            return self._kind3_by_image(li)
        x = self.rows(li.in0, (B, H, W, Cc))
        mean_d, inv_d = _d2h_f32(self.hip, li.aux0, (Cc,)), _d2h_f32(self.hip, li.aux1, (Cc,))
        g, bt = self.params[li.w_off:li.w_off + Cc], self.params[li.b_off:li.b_off + Cc]
        mu, inv = (t.numpy() for t in R.bn_stats(x))
        self._hold_stats(li, mean_d, inv_d, mu, inv)
        if not li.out:                                   # the fused head's BatchNorm: its y is not stored (kind 11 checks what is made of it)
            return
        got = self.rows(li.out, (B, H, W, Cc)).numpy()
        ref = R.bn_out(x, torch.tensor(mean_d), torch.tensor(inv_d), torch.tensor(g), torch.tensor(bt)).numpy()
        if B * H * W == 1:
            # ONE value per channel (the bottom of a one-image 2 x 2 case): x = mean, the output is beta, and the terms of the affine
            # the kernel evaluates, x * scale + (beta - mean * scale) with scale = gamma / sqrt(eps) ~ 30 gamma, cancel entirely: a
            # fraction of the channel's maximum has nothing to do with its error. Per element instead: one storage rounding of the
            # result plus the f32 roundings of shift and of the fma, 4 * 2^-24 * (|x scale_d| + |shift_d|) (cf. kind 13's bound)
            _m, _i, scale_d, shift_d = self._stats4(li)
            lim = R.one_value_bound(ref, np.abs(x.numpy() * scale_d) + np.abs(shift_d), self.bf16)
            self.hold("BatchNorm forward over one value", li, float((np.abs(got - ref) / (lim + 1e-300)).max()), 1.0)
            return
        self.hold_tensor("BatchNorm forward", li, got, ref, self.tol["out"], True)
        if li.mask:                                      # pooled = 2x2 max of the STORED (rounded) output, exactly
            pg = self.rows(li.mask, (B, H // 2, W // 2, Cc)).numpy()
            self.hold("BatchNorm forward, pooled output", li, float(not np.array_equal(pg, R.pool2x2(got))), 0.5)

    def _hold_stats(self, li, mean_d, inv_d, mu, inv):
        R, B, H, W, Cc = self.R, self.B, li.H, li.W, li.C0
        # statistics, on their own line: tol of the vector maximum, plus -- accumulator mode, a multiple of 64 channels (the folded
        # kernel's shapes) -- the error derived from the units: d_mean = adds * 2^-25 / M, d_inv = inv^3 / 2 * (adds * 2^-17 / M + ...)
        M = B * H * W
        d_mu, d_inv = R.acc_stats_error(M, mu, inv) if self.acc_mode and not Cc & 63 else (0.0, np.zeros(Cc))
        for what, dev, ref, extra in (("mean", mean_d, mu, d_mu), ("1/std", inv_d, inv, d_inv)):
            err, plain = np.abs(dev - ref), self.tol["stats"] * np.abs(ref).max()
            self.stats_plain = float(np.max([self.stats_plain, err.max() / (plain + 1e-300)]))
            c = int((err / (plain + extra + 1e-300)).argmax())
            self.hold("BatchNorm statistics", li, err[c], plain + (extra if np.ndim(extra) == 0 else extra[c]),
                      (what, "channel %d" % c, "M = %d" % M, "error %.3g" % err[c], "tol * max %.3g" % plain))

    def hold_channels(self, what, li, ce, tol, shape):
        e_t, e_c, c = ce.ratios(tol)
        self.hold(what, li, e_t, tol, ("tensor-wise", shape))
        self.hold(what + ", per channel", li, e_c, 1.0, ("channel %d" % c, shape))

    def _kind3_by_image(self, li):
        """Kind 3 with every reference evaluated one image at a time (the same formulas and bounds; sums over the whole batch)."""
        R, B, H, W, Cc = self.R, self.B, li.H, li.W, li.C0
        shape = (B, H, W, Cc)
        mean_d, inv_d = _d2h_f32(self.hip, li.aux0, (Cc,)), _d2h_f32(self.hip, li.aux1, (Cc,))
        g, bt = (torch.tensor(self.params[o:o + Cc]) for o in (li.w_off, li.b_off))
        s = torch.zeros(Cc, dtype=torch.float64); ss = torch.zeros(Cc, dtype=torch.float64)
        for i in range(B):
            x = self.rows(li.in0, shape, [i]).reshape(-1, Cc)
            s += x.sum(0); ss += (x * x).sum(0)
        M = B * H * W
        mu = s / M
        inv = 1.0 / torch.sqrt((ss / M - mu * mu).clamp_min(0.0) + R.BN_EPS)          # (replay_ref.bn_stats, from the sums)
        self._hold_stats(li, mean_d, inv_d, mu.numpy(), inv.numpy())
        if not li.out:
            return
        ce, pooled_bad = R.ChannelErr(), 0
        for i in self.elem_imgs:
            x = self.rows(li.in0, shape, [i]); got = self.rows(li.out, shape, [i]).numpy()
            ce.add(got, R.bn_out(x, torch.tensor(mean_d), torch.tensor(inv_d), g, bt).numpy())
            if li.mask:
                pooled_bad += int(not np.array_equal(self.rows(li.mask, (B, H // 2, W // 2, Cc), [i]).numpy(), R.pool2x2(got)))
        self.hold_channels("BatchNorm forward", li, ce, self.tol["out"], shape)
        if li.mask:
            self.hold("BatchNorm forward, pooled output", li, float(pooled_bad), 0.5)

    def _kind4(self, li):
        R, B, H, W, Cc = self.R, self.B, li.H, li.W, li.C0
        dn = self.rows(li.in0, (B, H, W, Cc)); x = self.rows(li.in1, (B, H, W, Cc))
        got = self.rows(li.out, (B, H, W, Cc)).numpy()
        mean_d, inv_d = _d2h_f32(self.hip, li.aux0, (Cc,)), _d2h_f32(self.hip, li.aux1, (Cc,))
        g = self.params[li.w_off:li.w_off + Cc]
        ref, dgamma, dbeta = R.bn_bwd(dn, x, torch.tensor(mean_d), torch.tensor(inv_d), torch.tensor(g))
        extra = R.acc_sum_error(B * H * W, R.BN_ACC_B) if self.acc_mode and not Cc & 63 else 0.0
        self.later.append(("dgamma", li.conv_index, li.w_off, dgamma.numpy(), self.tol["reduce"], extra))
        self.later.append(("dbeta", li.conv_index, li.b_off, dbeta.numpy(), self.tol["reduce"], extra))
        if B * H * W == 1:
            # ONE value per channel (the bottom of a one-image 2 x 2 case): xhat = 0 (up to the statistics' own rounding) and
            # dn - dbeta / M = 0, the gradient is zero and there is no maximum to take a fraction of. What the f32 evaluation of k1 * dn + k2 * x + k3 (k3 = -k1 * dn,
            # rounded) may leave: 4 * 2^-24 * (|k1 dn| + |k2 x| + |k3|), the f32 term of kind 13's per-element bound
            k1, k2, k3 = R.bn_bwd_coeffs(dgamma, dbeta, 1, torch.tensor(mean_d), torch.tensor(inv_d), torch.tensor(g))
            lim = R.one_value_bound(None, ((k1 * dn).abs() + (k2 * x).abs() + k3.abs()).numpy())
            self.hold("BatchNorm backward over one value (zero gradient)", li, float((np.abs(got - ref.numpy()) / (lim + 1e-300)).max()), 1.0)
            return
        self.hold_tensor("BatchNorm backward", li, got, ref.numpy(), self.tol["out"], True)

    def _kind5(self, li):
        B, H, W, Cc = self.B, li.H, li.W, li.C0
        n_ = self.rows(li.in0, (B, H, W, Cc)).numpy(); ds = self.rows(li.in1, (B, H, W, Cc)).numpy()
        dp = self.rows(li.dz, (B, H // 2, W // 2, Cc)).numpy()
        got = self.rows(li.out, (B, H, W, Cc)).numpy()
        ref = self.R.pool_bwd_skip(n_, ds, dp)
        e = float((np.abs(got - ref) / (np.abs(ref) + 1e-6 * np.abs(ref).max())).max())
        self.hold("max-pool backward + skip add", li, e, self.tol["pool"])              # one rounding of an exact sum

    def _head(self, li):
        Cc, K = li.C0, li.Cout
        return (torch.tensor(self.params[li.w_off:li.w_off + Cc * K].reshape(Cc, K)), torch.tensor(self.params[li.b_off:li.b_off + K]))

    def _kind6(self, li):
        B, H, W = self.B, li.H, li.W
        n_ = self.rows(li.in0, (B, H, W, li.C0))
        got = _d2h_f32(self.hip, li.out, (B, H, W, li.Cout))
        self.head_out = got
        ref = self.R.head_fwd(n_, *self._head(li)).numpy()
        self.hold("head forward (absolute)", li, float(np.abs(got - ref).max()), self.tol["probs"])

    def _kind7(self, li):
        B, H, W, Cc = self.B, li.H, li.W, li.C0
        n_ = self.rows(li.in0, (B, H, W, Cc))
        yy = torch.tensor(_d2h_u8(self.hip, li.dz, (B, H, W)).astype(np.int64))
        ww = torch.tensor(_d2h_f32(self.hip, li.mask, (B,)) if li.mask else np.ones(B))
        dn, dWh, dbh = self.R.head_bwd(n_, yy, ww, *self._head(li), self.U.keras_sparse_ce)
        self.later.append(("dWh", -1, li.w_off, dWh.numpy().ravel(), self.tol["reduce"], 0.0))
        self.later.append(("dbh", -1, li.b_off, dbh.numpy(), self.tol["reduce"], 0.0))
        got = self.rows(li.out, (B, H, W, Cc)).numpy()
        self.hold_tensor("head backward", li, got, dn.numpy(), self.tol["out"], False)

    def _stats4(self, li):
        """mean, invstd, scale, shift of a launch's BatchNorm: f32 [4][C0] from aux0 on (aux1 = the second row)."""
        Cc = li.C0
        assert li.aux0 and li.aux1 == li.aux0 + 4 * Cc, ("mean and invstd are not neighbours", li.kind, li.conv_index)
        return _d2h_f32(self.hip, li.aux0, (4, Cc))

    def _kind11(self, li):
        """head_bn_forward: probabilities against head_fwd(n2, Wh, bh) in fp64, n2 = storage-rounding(fmaf(c3, scale_d, shift_d)) in
        emulated float32 from the DEVICE scale and shift: probs (2e-5 absolute, kind 6's bound). The folded scale / shift themselves
        against gamma * inv_d and beta - mean_d * scale_d: 4 * 2^-24 of the terms (a rounded product; a product and a difference)."""
        R, B, H, W, Cc, K = self.R, self.B, li.H, li.W, li.C0, li.Cout
        mean_d, inv_d, scale_d, shift_d = self._stats4(li)
        g_off, b_off = self.m_bn_offsets(li.conv_index)
        g, bt = self.params[g_off:g_off + Cc], self.params[b_off:b_off + Cc]
        e = max(float((np.abs(scale_d - g * inv_d) / (4 * R.U_F32 * np.abs(g * inv_d) + 1e-300)).max()),
                float((np.abs(shift_d - (bt - mean_d * scale_d)) / (4 * R.U_F32 * (np.abs(bt) + np.abs(mean_d * scale_d)) + 1e-300)).max()))
        self.hold("fused head: folded scale / shift", li, e, 1.0)
        got = _d2h_f32(self.hip, li.out, (B, H, W, K))
        self.head_out = self.fused_probs = got
        Wh, bh = self._head(li)
        e = 0.0
        for i in self.elem_imgs:
            n2 = R.head_bn_n2(self.rows(li.in0, (B, H, W, Cc), [i]), torch.tensor(scale_d), torch.tensor(shift_d), self.bf16)
            e = max(e, float(np.abs(got[i:i + 1] - R.head_fwd(n2, Wh, bh).numpy()).max()))
        self.hold("fused head forward (absolute)", li, e, self.tol["probs"])

    def m_bn_offsets(self, bn_index):
        """(gamma, beta) float offsets of BatchNorm `bn_index` (creation order = the library's index)."""
        names = [n[:-len("/gamma")] for n in self.m._keras_order() if n.endswith("/gamma")]
        return self.m._tensors[names[bn_index] + "/gamma"][1], self.m._tensors[names[bn_index] + "/beta"][1]

    def _kind12(self, li):
        """head_bn_backward + head_bn_bwd_apply. In fp64 with nothing rounded in between: dzh from the DEVICE probabilities, labels
        and weights (keras_sparse_ce), dn2 = dzh @ Wh^T, BatchNorm backward of dn2 at c3 with the device statistics -> dz3, dgamma,
        dbeta; dWh = (gamma * xhat + beta)^T dzh, dbh = sum dzh. dz3: out, tensor-wise and per channel; the four reductions: reduce
        (no accumulator term: fp32 partial rows), after the pass; aux2 against fp64 k1, k2, k3: reduce of each vector's maximum."""
        R, B, H, W, Cc, K = self.R, self.B, li.H, li.W, li.C0, li.Cout
        shape, M = (B, H, W, Cc), B * H * W
        st = self._stats4(li)
        mean_d, inv_d = torch.tensor(st[0]), torch.tensor(st[1])
        g_off, b_off = self.bn_offs[li.conv_index]             # (of that BatchNorm's kind-3 record)
        g, bt = torch.tensor(self.params[g_off:g_off + Cc]), torch.tensor(self.params[b_off:b_off + Cc])
        probs = torch.tensor(_d2h_f32(self.hip, li.in1, (B, H, W, K)))
        yy = torch.tensor(_d2h_u8(self.hip, li.dz, (B, H, W)).astype(np.int64))
        ww = torch.tensor(_d2h_f32(self.hip, li.mask, (B,)) if li.mask else np.ones(B))
        dzh, _l = R.loss_grad_at_logits(probs, yy, ww, self.U.keras_sparse_ce)
        Wh, _bh = self._head(li)
        dgamma = torch.zeros(Cc, dtype=torch.float64); dbeta = torch.zeros(Cc, dtype=torch.float64)
        dWh = torch.zeros(Cc, K, dtype=torch.float64)
        for i in range(B):
            _dn2, dg_i, db_i, dW_i = R.head_bn_bwd_sums(self.rows(li.in0, shape, [i]), dzh[i:i + 1], Wh, mean_d, inv_d, g, bt)
            dgamma += dg_i; dbeta += db_i; dWh += dW_i
        self.later.append(("fused head dWh", -1, li.w_off, dWh.numpy().ravel(), self.tol["reduce"], 0.0))
        self.later.append(("fused head dbh", -1, li.b_off, dzh.sum((0, 1, 2)).numpy(), self.tol["reduce"], 0.0))
        self.later.append(("fused head dgamma", li.conv_index, g_off, dgamma.numpy(), self.tol["reduce"], 0.0))
        self.later.append(("fused head dbeta", li.conv_index, b_off, dbeta.numpy(), self.tol["reduce"], 0.0))
        coef = _d2h_f32(self.hip, li.aux2, (3, Cc))
        for name, dev, ref in zip(("k1", "k2", "k3"), coef, R.bn_bwd_coeffs(dgamma, dbeta, M, mean_d, inv_d, g)):
            ref = ref.numpy()
            self.hold("fused head coefficients", li, np.abs(dev - ref).max(), self.tol["reduce"] * np.abs(ref).max(), name)
        ce = R.ChannelErr()
        for i in self.elem_imgs:
            x = self.rows(li.in0, shape, [i])
            ce.add(self.rows(li.out, shape, [i]).numpy(), R.bn_bwd_apply(dzh[i:i + 1] @ Wh.T, x, mean_d, inv_d, g, dgamma, dbeta, M).numpy())
        self.hold_channels("fused head backward (dz3)", li, ce, self.tol["out"], shape)

    def _kind13(self, li):
        """launch_maxpool_bwd_bn (both kernels). (a) dn = storage-rounding(dskip + dp routed to the first maximum of the STORED n),
        BatchNorm backward of it in fp64 with the device statistics: dgamma, dbeta (after the pass) and k1, k2, k3 to reduce + the
        accumulator units' half unit per add (the coefficients: that bound of the sums carried through their formula, per channel:
        replay_ref.bn_bwd_coeff_bounds); its dz to out, tensor-wise and per channel. (b) EVERY output element against
        [x > 0] * storage-rounding(fmaf(k1_d, dn, fmaf(k2_d, x, k3_d))) from the DEVICE coefficients in emulated float32, to
        u |ref| + 4 * 2^-24 (|k1 dn| + |k2 x| + |k3|). (c) the stored n has windows whose maximum is attained more than once.
        Why the coefficients are not held to reduce (+ the units' term) of each VECTOR's maximum: on the 7-workgroup grid of case P3 the
        CPU emulation of a correct kernel (tests/test_replay_bounds_host.py) puts k2 at 2.25 (C 64) and 1.09 (C 128) of that bound in
        f32 storage while dgamma and dbeta are within theirs -- k2_c = -(k1_c inv_c / M) dgamma_c scales the error of dgamma with the
        channel's 1/std. The per-channel bound follows from the sums' bounds (0.32 / 0.21 there) and is tighter for small 1/std.
        What this replay cannot see: in f32 storage (bf16x3) the windows that tie are windows of several ZEROS of the post-ReLU input,
        where dz is masked and xhat is equal, so routing to the last maximum gives the same dz, dgamma and dbeta -- no power against
        a wrong tie-break there. In bf16 storage different positive x round to the same n and a wrong tie-break fails (b)."""
        R, B, H, W, Cc = self.R, self.B, li.H, li.W, li.C0
        shape, pshape, M = (B, H, W, Cc), (B, H // 2, W // 2, Cc), B * H * W
        st = self._stats4(li)
        mean_d, inv_d = torch.tensor(st[0]), torch.tensor(st[1])
        g = torch.tensor(self.params[li.w_off:li.w_off + Cc])
        coef = _d2h_f32(self.hip, li.aux2, (3, Cc))

        def dn_of(i):
            n_ = self.rows(li.mask, shape, [i]).numpy()
            dn = R.storage_round(R.pool_bwd_skip(n_, self.rows(li.in1, shape, [i]).numpy(), self.rows(li.dz, pshape, [i]).numpy()), self.bf16)
            return n_, dn, self.rows(li.in0, shape, [i])

        dgamma = torch.zeros(Cc, dtype=torch.float64); dbeta = torch.zeros(Cc, dtype=torch.float64)
        tied = windows = 0
        for i in range(B):
            n_, dn, x = dn_of(i)
            dg_i, db_i = R.bn_bwd_sums(dn, x, mean_d, inv_d)
            dgamma += dg_i; dbeta += db_i
            t_i, w_i = R.tied_windows(n_)
            tied += t_i; windows += w_i
        self.ties.append((Cc, tied, windows))
        print("replay (kind 13, C=%d %dx%d): %d of %d windows (%.3g) attain their maximum more than once" % (Cc, H, W, tied, windows, tied / windows))
        self.hold("pool recompute: tied windows present", li, float(tied == 0), 0.5)
        extra = R.acc_sum_error(M, R.BN_ACC_B)
        self.later.append(("pool recompute dgamma", li.conv_index, li.w_off, dgamma.numpy(), self.tol["reduce"], extra))
        self.later.append(("pool recompute dbeta", li.conv_index, li.b_off, dbeta.numpy(), self.tol["reduce"], extra))
        lims = R.bn_bwd_coeff_bounds(self.tol["reduce"], extra, dgamma, dbeta, M, mean_d, inv_d, g)
        for name, dev, ref, lim in zip(("k1", "k2", "k3"), coef, R.bn_bwd_coeffs(dgamma, dbeta, M, mean_d, inv_d, g), lims):
            self.hold("pool recompute coefficients", li, float((np.abs(dev - ref.numpy()) / (lim.numpy() + 1e-300)).max()), 1.0, name)
        ce, e = R.ChannelErr(), 0.0
        for i in self.elem_imgs:
            _n, dn, x = dn_of(i)
            got = self.rows(li.out, shape, [i])
            ce.add(got.numpy(), R.bn_bwd_apply(dn, x, mean_d, inv_d, g, dgamma, dbeta, M).numpy())
            ref, lim = R.pool_bwd_bn_elementwise(dn, x, *coef, self.bf16)
            e = max(e, float(((got - ref).abs() / (lim + 1e-300)).max()))
        self.hold("pool recompute, per element (device coefficients)", li, e, 1.0, shape)
        self.hold_channels("pool recompute backward (dz)", li, ce, self.tol["out"], shape)

    def check_returned(self, probs, loss, y, sw):
        """After the pass: the probabilities forward_backward returned are the kind-11 launch's output bit for bit, and the per-pixel
        loss it returned (written by head_bn_backward) against fp64 Keras sparse cross-entropy of the DEVICE probabilities: per image
        sum and the logged mean (UNet.loss_mean) to 1e-5 relative (tests/test_gpu_losses.py's bound for this loss), and, beside
        that, every pixel to 1e-5 |L| + w * (K + 2) * 2^-24 (the f32 sum of K clipped probabilities and the two logarithms'
        difference, each rounded once)."""
        p = self.fused_probs
        B, K = self.B, p.shape[-1]
        assert np.array_equal(probs.cpu().numpy().astype(np.float64).reshape(p.shape), p), "returned probabilities are not the kind-11 output"
        ww = torch.tensor(np.asarray(sw, np.float64))
        yy = torch.tensor(np.asarray(y).reshape(p.shape[:-1]).astype(np.int64))
        want = self.U.keras_sparse_ce(torch.tensor(p), yy, ww).numpy().reshape(B, -1)
        got = loss.cpu().numpy().astype(np.float64).reshape(B, -1)
        lim = 1e-5 * np.abs(want) + ww.numpy()[:, None] * (K + 2) * self.R.U_F32
        r_pix = float((np.abs(got - want) / lim).max())
        r_img = float((np.abs(got.sum(1) - want.sum(1)) / (1e-5 * np.abs(want.sum(1)))).max())
        r_mean = abs(float(self.m.loss_mean().item()) - want.mean()) / (1e-5 * abs(want.mean()))
        for what, r in (("fused head loss, per pixel", r_pix), ("fused head loss, per image (1e-5 relative)", r_img),
                        ("fused head loss, mean (1e-5 relative)", r_mean)):
            self.worst[what] = max(self.worst.get(what, 0.0), r)
        assert r_pix <= 1.0 and r_img <= 1.0 and r_mean <= 1.0, ("loss against fp64 of the device probabilities", r_pix, r_img, r_mean)

    def count(self, kind):
        return sum(k == kind for k, _i in self.seen)

    def finish(self):
        """After the pass: every recorded reduction against the gradient buffer; raises with ALL that miss."""
        g = self.m.grads.cpu().numpy().astype(np.float64)
        bad = []
        for what, idx, off, ref, tol, extra in self.later:
            err = np.abs(g[off:off + ref.size] - ref).max()
            r = float(err / (tol * np.abs(ref).max() + extra + 1e-300))
            self.worst[what] = float(np.max([self.worst.get(what, 0.0), r]))
            if not r <= 1.0:
                bad.append((what, idx, "error / bound %.3g" % r))
        assert not bad, bad

    def report(self, tag):
        print("replay (%s, %s): launches by kind %s; worst error / bound: %s; BatchNorm statistics without the derived fixed-point term %.3g"
              % (tag, self.dtype, " ".join("%d:%d" % (k, self.count(k)) for k in sorted(self.kinds)),
                 ", ".join("%s %.3g" % kv for kv in sorted(self.worst.items())), self.stats_plain)
              + ("; bf16x3 forward conv against %g of a channel's own maximum (not held) %.3g" % (self.tol["conv"], self.x3_per_channel)
                 if self.dtype == "bf16x3" else ""))


def _run_tapped_step(m, x, y, sw, checks, schedule_log=False, want_loss=False):
    from replay_tap import tapped
    with tapped(m, checks.check, schedule_log=schedule_log) as tap:
        probs, loss = m.forward_backward(x, y, sw)
        torch.cuda.synchronize()
    return (tap, probs, loss) if want_loss else (tap, probs)


def _replay_conv_launches(B, dim, cf, dtype="bf16", tol_act=1.2e-2, tol_w=2e-3):
    m, x, y, sw = _train_case(3, 1, 4, cf, B, dim, dim, dtype, seed=31, sw_period=3)
    torch.set_num_threads(max(1, torch.get_num_threads()))
    ck = _StepChecks(m, B, dtype, range(CMP), kinds=(0, 1, 2))
    assert ck.tol["conv"] == tol_act and ck.tol["wgrad"] == tol_w, (ck.tol, tol_act, tol_w)
    _run_tapped_step(m, x, y, sw, ck)
    assert (ck.count(0), ck.count(1), ck.count(2)) == (22, 25, 22), (ck.count(0), ck.count(1), ck.count(2))
    ck.finish()
    ck.report("conv launches, B=%d %d^2 cf=%s" % (B, dim, cf))


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

    from replay_tap import tapped
    with tapped(m, lambda li: recs.append({f: getattr(li, f) for f, _t in _lib.LaunchInfo._fields_})):
        m.forward_backward(x, y, None)
        torch.cuda.synchronize()
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
    (NumPy / torch-CPU) from exactly the tensors the launch read and compared with what it stored (_StepChecks). Tolerances: bf16
    tensors 1.2e-2 of the tensor max (one rounding of the stored value is 2^-9 relative; BatchNorm-backward outputs are differences
    of O(1) terms) and, BatchNorm forward / backward, of every channel's max; batch statistics 1e-4 of the vector max (no derived
    fixed-point term here); fp32 reductions (dgamma / dbeta, head weight / bias gradients) 2e-3 of the tensor max, probabilities
    2e-5 absolute. Every check runs through replay_tap.tapped: a miss fails the test and names the launch."""
    B, dim = 16, 128
    m, x, y, sw = _train_case(3, 1, 4, 1, B, dim, dim, "bf16", seed=41, sw_period=3)
    ck = _StepChecks(m, B, "bf16", range(B), kinds=(3, 4, 5, 6, 7), derived=False)
    _run_tapped_step(m, x, y, sw, ck)
    seen = {k: ck.count(k) for k in (3, 4, 5, 6, 7)}
    assert seen == {3: 13, 4: 13, 5: 4, 6: 1, 7: 1}, seen
    ck.finish()
    ck.report("non-conv launches, configs[1]")


# ---- small odd networks: every launch of one train step, kinds 0-7 in ONE pass ------------------------------------------------
def train_step_launch_counts(D, fused_levels=None, fused_head=True):
    """Launches a tapped train step of depth D reports, by kind (the one statement of the completeness rule; tests/test_gpu_ws_audit.py
    counts its intervals with it). fused_levels = n: the step with the fused forms on (mpu_unet_set_launch_tap_fused) -- the fused
    head (kind 11 + the kind-3 record of its BatchNorm, then kind 12 in place of kinds 7 and 4; fused_head=False: a network whose
    last block has no 64 filters keeps kinds 6, 7 and that kind 4) and n encoder levels on the pool-backward recompute (kind 13 in
    place of kinds 5 and 4)."""
    if fused_levels is None:
        return {0: 5 * D + 2, 1: 6 * D + 1, 2: 5 * D + 2, 3: 3 * D + 1, 4: 3 * D + 1, 5: D, 6: 1, 7: 1}
    n, h = fused_levels, int(bool(fused_head))
    return {0: 5 * D + 2, 1: 6 * D + 1, 2: 5 * D + 2, 3: 3 * D + 1, 4: 3 * D + 1 - n - h, 5: D - n, 6: 1 - h, 7: 1 - h, 11: h, 12: h, 13: n}


def _replay_train_step(K, C, depth, cf, B, H, W, dtype, tag=""):
    """One tapped forward_backward (alternating sample weights 1.0 / 0.33, labels zero on about half the pixels), every launch of
    kinds 0-7 checked by _StepChecks on ALL images, the fixed-point units' derived error added where a value comes out of an
    accumulator. Completeness from the depth D: 5 D + 2 forward convs and as many weight gradients (each conv index once),
    6 D + 1 data gradients, 3 D + 1 BatchNorm forwards and backwards, D pool backwards, one head forward, one head backward; the
    returned probabilities are the head launch's output. Returns (checks, schedule-log lines)."""
    import time
    t0 = time.time()
    m, x, y, sw = _train_case(K, C, depth, cf, B, H, W, dtype, seed=51, sw_period=2)
    ck = _StepChecks(m, B, dtype, range(B))
    try:
        tap, probs = _run_tapped_step(m, x, y, sw, ck, schedule_log=True)
    except AssertionError:                                  # failed launches: their reductions are still checked, every figure printed
        try:
            ck.finish()
        finally:
            ck.report("%s, FAILED" % tag)
        raise
    D = depth
    want = train_step_launch_counts(D)
    seen = {k: ck.count(k) for k in range(8)}
    assert seen == want, (seen, want)
    assert tap.launches == sum(want.values()), (tap.launches, want)
    for kind in (0, 2):
        assert sorted(i for k, i in ck.seen if k == kind) == list(range(5 * D + 2)), (kind, ck.seen)
    for kind in (3, 4):
        assert sorted(i for k, i in ck.seen if k == kind) == list(range(3 * D + 1)), (kind, ck.seen)
    assert np.array_equal(probs.cpu().numpy().astype(np.float64).reshape(ck.head_out.shape), ck.head_out)
    try:
        ck.finish()
    finally:
        ck.report("%s K=%d C=%d depth=%d cf=%s B=%d %dx%d" % (tag, K, C, depth, cf, B, H, W))
    print("replay (%s, %s): %.1f s" % (tag, dtype, time.time() - t0))
    return ck, tap.log.splitlines()


# K, C, depth, cf, B, H, W
TRAIN_NETS = {
    "T1": (5, 2, 2, 2, 3, 48, 40),         # 90 / 181 / 362 filters: channel tails in every conv and every non-conv kind; BatchNorms off the
                                           # accumulator path; concat sources as separate weight-gradient jobs; two input channels; odd batch
    "T2": (3, 1, 4, 0.25, 5, 16, 32),      # 32 ... 512 filters; bottom on 1 x 2 maps (statistics over 10 values), pool backward 2 x 4 -> 1 x 2
    "T3": (3, 1, 2, 1, 3, 32, 160),        # 64 / 128 / 256: every BatchNorm on the folded / accumulator kernels; W = 80 at level 1 = 2.5 tiles of 32
    "T4": (8, 1, 1, 1, 2, 32, 32),         # 8 classes: the widest head that trains (unet_model.hip: TRAIN_MAX_CLASSES), forward and backward
}


def _assert_t3_schedule(lines):
    """What the step's schedule switches force, read off the schedule log (the library reads a switch once per process; the sets of
    test_train_net_t3_under_schedule_switches_subprocess arrive through the environment)."""
    fold = [l for l in lines if l.startswith("bn_fold")]
    if not _env_on("MPU_BN_ATOMIC"):                       # partial rows + finalize instead of the accumulators
        assert not any("rows=-1" in l for l in lines), lines
    if not (_env_on("MPU_FUSED_BN_STATS") or _env_on("MPU_FUSED_BN_BWD_CONV") or _env_on("MPU_FUSED_BN_BWD")):
        assert not fold, fold                              # no producer leaves sums: colreduce + finalize + apply everywhere
    if not (_env_on("MPU_WGRAD_GROUP") or _env_on("MPU_WGRAD_BATCHED_REDUCE")):
        assert not any(l.startswith("wgrad-group") for l in lines), lines
        assert sum(l.startswith("wgrad ") for l in lines) == 5 * 2 + 2, lines      # every weight gradient as its own launch
    if all(_env_on(v) for v in ("MPU_BN_ATOMIC", "MPU_BN_FOLD", "MPU_FUSED_BN_STATS", "MPU_FUSED_BN_BWD_CONV", "MPU_FUSED_BN_BWD")):
        assert any("rows=-1" in l for l in fold), lines    # the accumulator form is what the default replay covers


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
@pytest.mark.parametrize("net", ["T1", "T2", "T3", "T4"])
def test_train_step_small_odd_networks_every_launch_against_fp64(net, dtype):
    """Networks T1-T4 (TRAIN_NETS): the smallest at which the listed code paths still differ from the workload's. Measured (one
    MI355X; the table per network and dtype is in DESIGN.md, section 2): every bf16 figure <= 0.35 of its bound (pool backward 0.996
    of 2^-8: one rounding reaches its unit roundoff), bf16x3 <= 0.37, 0.1-1.1 s per case. T2's 10-value statistics are 4.6 x (bf16)
    the plain 1e-4 and 0.18 of the bound with the accumulator units' derived error; a bf16x3 forward conv is up to 33 x (T2) 5e-5 of
    a channel's own maximum -- inexact products, see _StepChecks._kind0 -- and <= 0.25 of its per-element bound."""
    ck, lines = _replay_train_step(*TRAIN_NETS[net], dtype, tag=net)
    if net == "T3" and dtype == "bf16":
        _assert_t3_schedule(lines)


def test_train_step_t1_f32_every_launch_against_fp64():
    """T1 in dtype "f32" (exact-f32 products, no accumulators): convs 5e-5, the non-conv kinds under the f32-emulation bounds."""
    _replay_train_step(*TRAIN_NETS["T1"], "f32", tag="T1")


@pytest.mark.parametrize("switches", [{"MPU_BN_ATOMIC": "0"},
                                      {"MPU_FUSED_BN_STATS": "0", "MPU_FUSED_BN_BWD_CONV": "0", "MPU_FUSED_BN_BWD": "0"},
                                      {"MPU_WGRAD_GROUP": "0", "MPU_WGRAD_BATCHED_REDUCE": "0"}],
                         ids=["partial_rows", "colreduce_sums", "ungrouped_wgrad"])
def test_train_net_t3_under_schedule_switches_subprocess(switches):
    """The switch-selected forms of the step that were only ever compared with each other, launch by launch against fp64: partial
    rows instead of accumulators, colreduce sums instead of epilogue sums, ungrouped weight gradients. A fresh interpreter per
    set, one at a time (the library reads a switch once per process); _assert_t3_schedule holds what each set forces."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_replay.py"), "-x", "-q", "-s", "-k",
                        "test_train_step_small_odd_networks_every_launch_against_fp64 and T3 and bf16 and not bf16x3"],
                       env=dict(os.environ, **switches), capture_output=True, text=True, cwd=os.path.dirname(here))
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("replay (")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]


# ---- the fused forms of the step: fused training head (kinds 11, 12) and pool-backward recompute (kind 13) ----------------------
# K, C, depth, cf, B, H, W; dtypes; the environment the case needs (a fresh interpreter where it differs from this one's: the library
# reads a switch once per process); n = encoder levels the recompute takes; large = kinds 3, 11, 12, 13 only, image by image
FUSED_CASES = {
    "H1": ((3, 1, 1, 1, 3, 10, 14), ("bf16", "bf16x3"), {}, 0, False),     # M = 420 = 4 mod 8 = 4 mod 16: ragged last pixel group in both storages
    "H2": ((2, 1, 1, 1, 1, 2, 2), ("bf16", "bf16x3"), {}, 0, False),       # M = 4 < G: one partial group; statistics over 4 values
    "H3": ((8, 1, 1, 1, 2, 18, 22), ("bf16",), {}, 0, False),              # M = 792 = 8 mod 16; the widest head of bf16 storage
    "H3w": ((4, 1, 1, 1, 2, 18, 22), ("bf16x3",), {}, 0, False),           # ... and of f32 storage (16 K = 64 lanes), ragged there
    "H4": ((3, 1, 1, 1, 5, 232, 232), ("bf16",), {}, 1, True),             # M = 269 120 > 262 144: second, ragged round of head_bn_backward
    "H5": ((3, 1, 1, 1, 5, 460, 460), ("bf16",), {}, 1, True),             # M = 1 058 000 > 1 048 576: second round of forward and apply
    "P1": (TRAIN_NETS["T3"], ("bf16", "bf16x3"), {"MPU_POOL_BWD_RECOMPUTE": "2"}, 2, False),
    "P2": (TRAIN_NETS["T2"], ("bf16", "bf16x3"), {"MPU_POOL_BWD_RECOMPUTE": "2"}, 3, False),   # level 0 (C 32) refused: kinds 5 and 4 remain
                                                                           # (32 filters at level 0: no fused head either -- kinds 6, 7)
    "P3": (TRAIN_NETS["T3"], ("bf16", "bf16x3"), {"MPU_POOL_BWD_RECOMPUTE": "2", "MPU_POOL_BWD_BLOCKS": "7"}, 2, False),
    "P4": ((3, 1, 5, 1, 1, 32, 32), ("bf16x3",), {"MPU_POOL_BWD_RECOMPUTE": "2"}, 5, True),    # C 1024 in f32 storage: cpr = 256; level 4 on 2 x 2 maps
}


def _replay_fused_step(case, dtype):
    """One tapped forward_backward with mpu_unet_set_launch_tap_fused on. Small cases: every launch of every kind on all images;
    large ones: kinds 3, 11, 12, 13 with the references evaluated image by image. Completeness: train_step_launch_counts(D, n) by
    kind, the kind-4 launches are exactly the BatchNorms neither the fused head nor a recomputed level took over, `head=1` on one
    forward and one backward line of the schedule log (none where the last block has no 64 filters: P2), `pool=1` on n backward lines; every kind-13 launch saw tied windows."""
    import time
    from multiplanarunet_amd import _lib
    t0 = time.time()
    (K, C, depth, cf, B, H, W), _dtypes, _env, n, large = FUSED_CASES[case]
    # H5 measured 15.3 s with every element of all five images compared: its reductions stay on the whole batch, its per-element
    # comparisons run on the first, the middle and the last image -- pixels 846 400 .. 1 058 000, which hold the second grid round
    # of head_bn_forward and head_bn_bwd_apply (from pixel 1 048 576 on)
    elem_imgs = (0, B // 2, B - 1) if case == "H5" else None
    head = int(int(64 * cf) == 64)                           # the fused head needs 64 filters in the last block (unet_model.hip)
    m, x, y, sw = _train_case(K, C, depth, cf, B, H, W, dtype, seed=51, sw_period=2)
    _lib.call("mpu_unet_set_launch_tap_fused", m._h, 1)
    ck = _StepChecks(m, B, dtype, range(B), kinds=(3, 11, 12, 13) if large else tuple(range(8)) + (11, 12, 13), by_image=large,
                     elem_imgs=elem_imgs)
    tag = "%s K=%d depth=%d cf=%s B=%d %dx%d" % (case, K, depth, cf, B, H, W)
    try:
        tap, probs, loss = _run_tapped_step(m, x, y, sw, ck, schedule_log=True, want_loss=True)
    except AssertionError:
        try:
            ck.finish()
        finally:
            ck.report("%s, FAILED" % tag)
        raise
    finally:
        _lib.call("mpu_unet_set_launch_tap_fused", m._h, 0)
    D = depth
    want = train_step_launch_counts(D, n, head)
    seen = {k: ck.all_kinds.get(k, 0) for k in want}
    assert seen == want and sum(ck.all_kinds.values()) == tap.launches == sum(want.values()), (ck.all_kinds, want, tap.launches)
    assert sorted(i for k, i in ck.seen if k == 3) == list(range(3 * D + 1)), ck.seen
    taken = {i for k, i in ck.seen if k in (12, 13)}
    assert len(taken) == n + head, ck.seen
    if not large:
        for kind in (0, 2):
            assert sorted(i for k, i in ck.seen if k == kind) == list(range(5 * D + 2)), (kind, ck.seen)
        assert sorted(i for k, i in ck.seen if k == 4) == sorted(set(range(3 * D + 1)) - taken), ck.seen
    lines = tap.log.splitlines()
    assert sum(l.startswith("bn_fold fwd") and "head=1" in l for l in lines) == head, lines
    assert sum(l.startswith("bn_fold bwd") and "head=1" in l for l in lines) == head, lines
    assert sum(l.startswith("bn_fold bwd") and "pool=1" in l for l in lines) == n, lines
    assert len(ck.ties) == n and all(t > 0 for _c, t, _w in ck.ties), ck.ties
    try:
        try:
            if head:
                ck.check_returned(probs, loss, y, sw)
            else:
                assert np.array_equal(probs.cpu().numpy().astype(np.float64).reshape(ck.head_out.shape), ck.head_out)
        finally:
            ck.finish()
    finally:
        ck.report(tag)
    print("replay (%s, %s): %.1f s; tied windows per kind-13 launch (C, tied, windows): %s" % (case, dtype, time.time() - t0, ck.ties))
    return ck


@pytest.mark.parametrize("case,dtype", [(c, d) for c, v in FUSED_CASES.items() for d in v[1]],
                         ids=["%s-%s" % (c, d) for c, v in FUSED_CASES.items() for d in v[1]])
def test_train_step_fused_head_and_pool_recompute_every_launch_against_fp64(case, dtype):
    """The two forms of the step that are the DEFAULT of the benchmarked bf16 step and used to switch themselves off under a tap,
    launch by launch against fp64 (FUSED_CASES; bounds: _StepChecks._kind11 / _kind12 / _kind13, tests/replay_ref.py). A case whose
    switches this interpreter does not have runs in a fresh one (one at a time, with a timeout).
    Measured (one MI355X; the table per case and dtype is in DESIGN.md, section 2), worst error as a fraction of its bound -- bf16:
    probabilities <= 0.016, per-pixel loss <= 0.25, dz3 <= 0.31 (per channel 0.32: one storage rounding), the head's and the pool's
    coefficients and reductions <= 7e-5, pool dz 0.23 (per channel 0.31), pool per element 0 (every element IS the emulated value);
    bf16x3: probabilities <= 0.011, dz3 per channel <= 0.32 (H2), head reductions <= 0.30, pool reductions and coefficients <= 0.14
    and, on P3's 7-workgroup grid (f32 chains of 34 windows per thread), 0.27; 21 % of the windows of every kind-13 launch tie.
    P4 (bf16x3, C 64 ... 1024, 1.8 s): head reductions <= 0.14, pool reductions and coefficients <= 0.20, pool dz per channel 0.21,
    statistics 0.83 (level 4: 4 values), 9.6 % tied windows at C 1024. A BatchNorm over ONE value (the bottom of H2 and P4): forward
    0.91 (bf16: one storage rounding reaches its unit roundoff) / 0.25 (H2 bf16x3) / 0.22 (P4), backward 0.17 / 0.29 (H2).
    0.1-3.7 s per case (6-8 s with a fresh interpreter's start-up), H4 2.1 s; H5 took 15.3 s with every element of all five images
    compared, hence its per-element comparisons on the first, the middle and the last image (_replay_fused_step): 12.2 s."""
    import os, subprocess, sys
    env = FUSED_CASES[case][2]
    if all(os.environ.get(k) == v for k, v in env.items()):
        _replay_fused_step(case, dtype)
        return
    here = os.path.dirname(os.path.abspath(__file__))
    sel = "test_train_step_fused_head_and_pool_recompute_every_launch_against_fp64 and %s-%s" % (case, dtype)
    if dtype == "bf16":
        sel += " and not bf16x3"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_replay.py"), "-x", "-q", "-s", "-k", sel],
                       env=dict(os.environ, **env), capture_output=True, text=True, cwd=os.path.dirname(here), timeout=600)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("replay (")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]


# ---- the inference forward (run_forward_infer), launch by launch -------------------------------------------------------------
def _replay_inference(K, C, depth, cf, B, H, W, tag="", seed=21):
    """One bf16 inference forward with the launch tap and the schedule log on. Every launch it reports (kinds 0, 6, 8, 9, 10 of
    mpu_launch_info) is recomputed on torch-CPU / NumPy in fp64 from the launch's own inputs and compared under the bounds of
    tests/replay_ref.py; conv outputs on the first and the last image of the batch (the last one sits in the ragged tail of the
    tile walk), everything else on the whole batch. Returns what the callers assert their schedules from."""
    import replay_ref as R
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
    EPS = 1e-3

    def rows(ptr, shape):                                   # the compared images of a device bf16 tensor, fp64
        return torch.cat([_d2h_rows(hip, ptr, shape, True, i, i + 1) for i in imgs])

    recs = []
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

    from replay_tap import tapped
    with tapped(m, check, schedule_log=True) as tap:        # (a failed check fails the test after the pass: replay_tap.py)
        probs = m._forward(m._as_input(x), training=False)
        torch.cuda.synchronize()

    # completeness: every conv exactly once, one head, `depth` pooled tensors, and the returned probabilities are the head's
    convs = [r for r in recs if r["kind"] in (0, 8)]
    lines = [l for l in tap.log.splitlines() if l.startswith("conv ")]
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


# K, C, depth, cf, B, H, W (the docstrings of the four tests below say what each is for)
INFER_NETS = {
    "A": (3, 1, 3, 1, 8, 128, 160),
    "B": (5, 2, 2, 2, 3, 48, 40),
    "C": (16, 1, 1, 1, 8, 128, 128),
    "D": (3, 1, 4, 0.25, 5, 16, 32),
}


def _kinds(res):
    return [r["kind"] for r in res["recs"]]


def test_inference_net_a_ws_fused_pool_and_head_halo_splitk_every_launch_against_fp64():
    """Network A: K 3, depth 3, cf 1, 8 images of 128 x 160 -- 1280 tiles at level 0: conv_ws with the fused pool and the fused
    head (K <= 8); levels 1-2 on the halo kernels with a ragged W tile (80 = 2.5 x 32); the deep levels on the split-K / glds
    schedules. The schedule switches of test_inference_net_a_under_schedule_switches_subprocess are read from the environment
    (once per process by the library): what each forces is asserted here."""
    import os
    res = _replay_inference(*INFER_NETS["A"], tag="A")
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
    res = _replay_inference(*INFER_NETS["B"], tag="B")
    assert _kinds(res).count(6) == 1 and _kinds(res).count(10) == 0, _kinds(res)


def test_inference_net_c_wide_fused_head_every_launch_against_fp64():
    """Network C: K 16, depth 1, 8 images of 128 x 128 (1024 tiles: exactly conv_ws's bound): the wide (K <= 16) fused head."""
    res = _replay_inference(*INFER_NETS["C"], tag="C")
    assert any(l.split()[1] == "ws" and "head=1" in l for l in res["lines"]), res["lines"]
    assert _kinds(res).count(10) == 1, _kinds(res)


def test_inference_net_d_tiny_maps_separate_maxpool_every_launch_against_fp64():
    """Network D: K 3, depth 4, cf 0.25, 5 images of 16 x 32: the bottom works on 1 x 2 maps, the last pooling goes 2 x 4 -> 1 x 2,
    and W < 32 below level 0 keeps the layers off the patch kernels and the pooling mostly on the separate kernel (kind 9)."""
    res = _replay_inference(*INFER_NETS["D"], tag="D")
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
