"""Reference arithmetic and bounds of the inference replay and of the train-step replay's non-conv launches
(tests/test_gpu_replay.py), NumPy / torch-CPU only, so that the bounds themselves can be checked without a GPU
(tests/test_replay_bounds_host.py).

An inference conv launch stores  y = s * relu(conv(x, w) + b) + t  rounded ONCE to bf16 (s, t: the folded BatchNormalization of
mpu_unet_prepare_inference; s = 1, t = 0 for a conv without one); x and w are bf16, the sums and the affine are f32.

CONV_TOL, tensor-wise: max |got - ref| <= 1.2e-2 * max |ref| (the per-layer suite's bound).
Per output channel c: max |got_c - ref_c| <= 1.2e-2 * max |ref_c|; a channel whose maximum is below DEAD = 1e-3 of the tensor's
maximum (the padded channels among them) is held to 1.2e-5 * max |ref| instead. The worst legitimate error is one bf16 rounding
of the stored value -- unit roundoff 2^-8 of the element, hence at most 2^-8 = 3.9e-3 of the channel maximum -- plus an f32
accumulation over K <= 9216 products (~1e-6): a third of the bound.
"""
import numpy as np
import torch
import torch.nn.functional as F

CONV_TOL = 1.2e-2
DEAD = 1e-3
U_BF16 = 2.0 ** -8


def bf16_round(a):
    return torch.as_tensor(a, dtype=torch.float32).to(torch.bfloat16).to(torch.float64)


def layer_forward(mode, x_nhwc, w_hwio, bias):
    """conv(x) + b of the reference layer, pre-activation: 3x3 SAME (mode 0) or UpSampling2D(2) + 2x2 SAME with TensorFlow's 0/1
    padding (mode 1); NHWC in, NHWC out, in the dtype of its arguments."""
    x = x_nhwc.permute(0, 3, 1, 2)
    w = w_hwio.permute(3, 2, 0, 1)
    if mode == 0:
        y = F.conv2d(x, w, bias, padding=1)
    else:
        up = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        y = F.conv2d(F.pad(up, (0, 1, 0, 1)), w, bias)
    return y.permute(0, 2, 3, 1)


def affine_relu_conv(mode, x, w, b, s, t):
    """ref = s * relu(conv(x, w) + b) + t, no intermediate rounding (the dtype of the arguments: fp64 for the reference)."""
    return s * torch.relu(layer_forward(mode, x, w, b)) + t


def conv_bound_ratios(got, ref, tol=CONV_TOL):
    """(max |got - ref| / max |ref|, worst per-channel error as a fraction of ITS bound, that channel) of [..., C] arrays; `tol`:
    the relative bound, of the tensor's and of a channel's maximum alike (CONV_TOL for bf16 storage)."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    Cn = ref.shape[-1]
    err = np.abs(got - ref).reshape(-1, Cn).max(0)
    cmax = np.abs(ref).reshape(-1, Cn).max(0)
    tmax = float(cmax.max()) + 1e-300
    lim = np.where(cmax >= DEAD * tmax, tol * cmax, tol * DEAD * tmax)
    ratio = err / lim
    c = int(ratio.argmax())
    return float(err.max() / tmax), float(ratio[c]), c


def head_partial_ratio(got, y_ref, Wh):
    """The 1x1 head out of a conv epilogue, without its bias, over the channels of Wh's rows: got [..., K] against
    bf16round(y_ref) @ Wh in fp64. Per pixel and class  |got - ref| <= sum_c |Wh[c,k]| * 2^-8 * |y_c| + 1e-5 * sum_c |Wh[c,k] * y_c|:
    the one rounding of the staged pixel, and the f32 sums (head weights as hi + lo bf16 parts: 2^-18 relative). Returns the worst
    error as a fraction of its bound."""
    y_ref = np.asarray(y_ref, np.float64)
    ref = bf16_round(y_ref).numpy() @ Wh
    mag = np.abs(y_ref) @ np.abs(Wh)
    lim = U_BF16 * mag + 1e-5 * mag
    return float((np.abs(np.asarray(got, np.float64) - ref) / (lim + 1e-300)).max())


def softmax64(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def pool2x2(y):
    """MaxPooling2D(2) of [B, H, W, C] (an odd last row / column is dropped)."""
    B, H, W, Cn = y.shape
    return y[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, Cn).max((2, 4))


# ---- the training step's non-conv launches (kinds 3-7 of mpu_launch_info) ------------------------------------------------------
# Each formula is written once, on torch tensors, in the dtype of its arguments: fp64 is the reference of the GPU replay, f32 the
# emulation that sets the f32-storage bounds (tests/test_replay_bounds_host.py).
BN_EPS = 1e-3                                    # Keras BatchNormalization default


def bn_stats(x):
    """Batch statistics of [..., C]: (mean, 1 / sqrt(var + eps)), var = E[x^2] - mean^2 clamped at 0 (the kernels' formula)."""
    Cn = x.shape[-1]
    xf = x.reshape(-1, Cn)
    M = xf.shape[0]
    mu = xf.sum(0) / M
    var = ((xf * xf).sum(0) / M - mu * mu).clamp_min(0.0)
    return mu, 1.0 / torch.sqrt(var + BN_EPS)


def bn_out(x, mean, inv, gamma, beta, affine=False):
    """gamma * (x - mean) * inv + beta; affine=True: the same value as x * scale + shift, scale = gamma * inv,
    shift = beta - mean * scale (the form the kernels evaluate)."""
    if affine:
        scale = gamma * inv
        return x * scale + (beta - mean * scale)
    return gamma * (x - mean) * inv + beta


def bn_bwd(dn, x, mean, inv, gamma, affine=False):
    """BatchNorm backward through the ReLU in front of it, from the statistics given: (dz, dgamma, dbeta);
    dz = [x > 0] * gamma * inv * (dn - dbeta / M - xhat * dgamma / M). affine=True: dz as k1 * dn + k2 * x + k3 (the kernels' form)."""
    Cn = x.shape[-1]
    M = x.numel() // Cn
    xh = (x - mean) * inv
    red = tuple(range(x.dim() - 1))
    dbeta = dn.sum(red); dgamma = (dn * xh).sum(red)
    if affine:
        k1 = gamma * inv
        k2 = -k1 * (dgamma / M) * inv
        dxx = k1 * dn + k2 * x + (-k1 * (dbeta / M) - k2 * mean)
    else:
        dxx = gamma * inv * (dn - dbeta / M - xh * dgamma / M)
    return torch.where(x > 0, dxx, torch.zeros((), dtype=x.dtype)), dgamma, dbeta


def pool_bwd_skip(n, dskip, dp):
    """dskip + the pooled gradient dp routed to the FIRST maximum (row-major) of every 2 x 2 window of n; NumPy [B, H, W, C]."""
    B, H, W, Cn = n.shape
    win = n.reshape(B, H // 2, 2, W // 2, 2, Cn).transpose(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, Cn, 4)
    first = win.argmax(-1)                                           # np.argmax: the first maximum
    routed = np.zeros_like(win)
    np.put_along_axis(routed, first[..., None], dp[..., None], -1)
    routed = routed.reshape(B, H // 2, W // 2, Cn, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, H, W, Cn)
    return dskip + routed


def head_fwd(n, Wh, bh):
    return torch.softmax(n @ Wh + bh, -1)


def head_bwd(n, y, w, Wh, bh, loss):
    """(dn, dWh, dbh) of sum(loss(softmax(n @ Wh + bh), y, w)) by autograd; loss: oracle/unet_ref.py keras_sparse_ce."""
    n = n.detach().clone().requires_grad_(True)
    Wh = Wh.detach().clone().requires_grad_(True)
    bh = bh.detach().clone().requires_grad_(True)
    loss(head_fwd(n, Wh, bh), y, w.to(n.dtype)).sum().backward()
    return n.grad, Wh.grad, bh.grad


def rel_max(got, ref):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


# Bounds of the non-conv kinds. bf16 storage: the numbers of the project's per-launch replay (tests/test_gpu_replay.py). f32 storage
# (dtypes "bf16x3", "f32"): 3 x (the suite's noise_mult) the worst error of a torch-f32 evaluation of the formulas above -- both
# forms -- against fp64 on the BatchNorm / head shapes of networks T1-T3, measured by tests/test_replay_bounds_host.py
# (test_f32_emulation_sets_the_f32_storage_bounds_of_the_non_conv_kinds holds each number between 3 x and 10 x its measurement);
# the pool backward stores ONE rounding of an exact two-term sum, so its bound is the unit roundoff of the format. Probabilities
# are f32 sums and an f32 softmax whatever the storage type of the head's input: 2e-5 absolute in every dtype.
TOL_BF16 = {"out": CONV_TOL, "stats": 1e-4, "reduce": 2e-3, "pool": 2.0 ** -8, "probs": 2e-5, "conv": CONV_TOL, "wgrad": 2e-3}
TOL_F32 = {"out": 4.2e-5, "stats": 5.5e-7, "reduce": 7e-7, "pool": 2.0 ** -24, "probs": 2e-5, "conv": 5e-5, "wgrad": 5e-5}

# dtype "bf16x3": an operand is hi + lo, two bf16 numbers: x = hi + r with |r| <= u |x| (u = U_BF16), lo = bf16(r) with
# |r - lo| <= u^2 |x|. A product is hi hi' + hi lo' + lo hi': the dropped lo lo' and the two representation errors are each
# <= u^2 |x w| (to first order), so |error of a product| <= 3 u^2 |x w| = 4.6e-5 |x w|; plus 1e-5 |x w| for the f32 sums, the share
# head_partial_ratio gives them. Per output element: |got - ref| <= X3_PRODUCT * (sum |x| |w| + |b|).
X3_PRODUCT = 3 * U_BF16 ** 2 + 1e-5

# Fixed-point accumulators (multiplanarunet_amd/csrc/unet_model.hip): units per 1.0
BN_ACC_F = (2.0 ** 24, 2.0 ** 16)                # forward sum x, sum x^2
BN_ACC_B = 2.0 ** 40                             # backward sum dn, sum dn * xhat (dbeta, dgamma)
DB_ACC_SCALE = 2.0 ** 44                         # bias gradient of dtype "bf16x3"


def acc_adds(M):
    """Upper bound of the addends one (statistic, channel) of an accumulator receives from M pixels: a producer adds ONE rounded
    column sum per workgroup (kernels.h: stats_acc_add, __double2ll_rn), and a workgroup covers at least one pixel. (The conv
    epilogues cover 64 and more; the split-K finish and the column reductions are sized by elements, a few pixels each at the
    widest layers -- so no tighter count is claimed here.)"""
    return int(M)


def acc_sum_error(M, units):
    """Absolute error of a SUM that came out of a fixed-point accumulator: half a unit (round to nearest) per workgroup add."""
    return acc_adds(M) * 0.5 / units


def acc_stats_error(M, mean, inv):
    """Absolute errors (d_mean, d_inv) per channel that the forward units add to mean and 1 / sqrt(var + eps) over M values:
    d_mean = adds * 2^-25 / M; d_var = adds * 2^-17 / M + 2 |mean| d_mean; d_inv = inv^3 / 2 * d_var (first order)."""
    d_mean = acc_sum_error(M, BN_ACC_F[0]) / M
    d_var = acc_sum_error(M, BN_ACC_F[1]) / M + 2.0 * np.abs(mean) * d_mean
    return d_mean, 0.5 * np.asarray(inv, np.float64) ** 3 * d_var


# ---- the fused forms of the train step (kinds 11-13 of mpu_launch_info; mpu_unet_set_launch_tap_fused) ----------------------------
# The fused training head (head_bn_forward / head_bn_backward / head_bn_bwd_apply) and the pool-backward recompute
# (maxpool_bwd_add_kernel<T, true, true> + maxpool_bwd_bn_fold_kernel) store no post-BatchNorm tensor: they RECOMPUTE it per element
# as rounding(fmaf(x, scale, shift)) and the replay recomputes that recomputation from the device coefficients, in emulated float32.
U_F32 = 2.0 ** -24


def storage_round(a, bf16):
    """fp64 -> float32 -> the storage format (bf16, or f32 as it is) -> fp64: the rounding of a kernel's store of an f32 register."""
    t = torch.as_tensor(a, dtype=torch.float64).to(torch.float32)
    return (t.to(torch.bfloat16) if bf16 else t).to(torch.float64)


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 values held in fp64: the product of two 24-bit significands is exact in fp64, so
    float32(float64(a) * float64(b) + float64(c)) differs from the single rounding of the exact a * b + c only where the fp64 sum
    itself lands on a float32 tie (tests/test_replay_bounds_host.py compares with exact rational arithmetic)."""
    a, b, c = (torch.as_tensor(v, dtype=torch.float64) for v in (a, b, c))
    return (a * b + c).to(torch.float32).to(torch.float64)


def head_bn_n2(x, scale, shift, bf16):
    """The post-BatchNorm tensor the fused head never stores: storage-rounding(fmaf(x, scale, shift)) with the DEVICE scale / shift."""
    return storage_round(fma32(x, scale, shift), bf16)


def loss_grad_at_logits(p, y, w, loss):
    """d sum(loss(p, y, w)) / d logits from GIVEN probabilities p [..., K] (the device's, fp64): the gradient g at p by autograd of
    `loss` (oracle/unet_ref.py keras_sparse_ce), then the softmax backward at p, p * (g - sum_k p_k g_k). Also the loss itself."""
    p = torch.as_tensor(p, dtype=torch.float64).detach().clone().requires_grad_(True)
    l = loss(p, y, w.to(p.dtype))
    l.sum().backward()
    g, pd = p.grad, p.detach()
    return pd * (g - (pd * g).sum(-1, keepdim=True)), l.detach()


def bn_bwd_coeffs(dgamma, dbeta, M, mean, inv, gamma):
    """(k1, k2, k3) of dz = [x > 0] * (k1 * dn + k2 * x + k3): bn_bwd's affine form, from the sums given."""
    k1 = gamma * inv
    k2 = -k1 * (dgamma / M) * inv
    return k1, k2, -k1 * (dbeta / M) - k2 * mean


def bn_bwd_coeff_bounds(tol, extra, dgamma, dbeta, M, mean, inv, gamma):
    """Per-channel bounds of (k1, k2, k3) that follow from the bounds of the sums they are made of: dgamma and dbeta are held to
    e_g = tol * max |dgamma| + extra and e_b = tol * max |dbeta| + extra (extra: the accumulator units' share), and
    k2_c = -(k1_c inv_c / M) dgamma_c, k3_c = -(k1_c / M) dbeta_c - k2_c mean_c are linear in them:
      k1: tol * max |k1| (no sum in it);  k2_c: |k1_c inv_c| / M * e_g;  k3_c: |k1_c| / M * e_b + |mean_c| * (the bound of k2_c).
    A fraction of the VECTOR's maximum would not follow: a channel with a large 1/std turns the same error of dgamma into a larger
    error of k2. (The f32 rounding of a coefficient, 2^-24 of itself, is below each of these: e_g >= tol |dgamma_c|.)"""
    k1 = (gamma * inv).abs()
    e_g, e_b = tol * dgamma.abs().max() + extra, tol * dbeta.abs().max() + extra
    b2 = k1 * inv.abs() / M * e_g
    return tol * k1.max() * torch.ones_like(k1), b2, k1 / M * e_b + mean.abs() * b2


def bn_bwd_sums(dn, x, mean, inv):
    """(dgamma, dbeta) of bn_bwd over the pixels given (additive over chunks of pixels)."""
    red = tuple(range(x.dim() - 1))
    return (dn * ((x - mean) * inv)).sum(red), dn.sum(red)


def bn_bwd_apply(dn, x, mean, inv, gamma, dgamma, dbeta, M):
    """dz of bn_bwd (plain form) from sums over ALL M pixels, on the pixels given."""
    dxx = gamma * inv * (dn - dbeta / M - (x - mean) * inv * dgamma / M)
    return torch.where(x > 0, dxx, torch.zeros((), dtype=x.dtype))


def head_bn_bwd_sums(c3, dzh, Wh, mean, inv, gamma, beta):
    """The fused head's backward sums over the pixels given (additive over chunks): dn2 = dzh @ Wh^T (nothing rounded), then
    (dn2, dgamma, dbeta, dWh) with dWh = (gamma * xhat + beta)^T dzh -- the post-BatchNorm value BEFORE its storage rounding."""
    Cn, K = Wh.shape
    dn2 = dzh @ Wh.T
    dgamma, dbeta = bn_bwd_sums(dn2, c3, mean, inv)
    n2 = gamma * ((c3 - mean) * inv) + beta
    return dn2, dgamma, dbeta, n2.reshape(-1, Cn).T @ dzh.reshape(-1, K)


def pool_bwd_bn_elementwise(dn, x, k1, k2, k3, bf16):
    """What maxpool_bwd_bn_fold_kernel stores, from the DEVICE coefficients in emulated float32, and the bound of every element:
    ref = [x > 0] * storage-rounding(fmaf(k1, dn, fmaf(k2, x, k3))); |got - ref| <= u |ref| + 4 * 2^-24 (|k1 dn| + |k2 x| + |k3|) --
    one storage rounding (u = 2^-8 / 2^-24) plus the float32 roundings of the two fmas."""
    dn, x = torch.as_tensor(dn, dtype=torch.float64), torch.as_tensor(x, dtype=torch.float64)
    k1, k2, k3 = (torch.as_tensor(k, dtype=torch.float64) for k in (k1, k2, k3))
    ref = torch.where(x > 0, storage_round(fma32(k1, dn, fma32(k2, x, k3)), bf16), torch.zeros((), dtype=torch.float64))
    lim = (U_BF16 if bf16 else U_F32) * ref.abs() + 4 * U_F32 * ((k1 * dn).abs() + (k2 * x).abs() + k3.abs())
    return ref, lim


def one_value_bound(ref, terms, bf16=None):
    """Per-element bound of a BatchNorm over ONE value per channel (M = 1: x = mean, the output is beta and the gradient zero, both
    far below the terms of the affine the kernels evaluate, so no fraction of a maximum applies): 4 * 2^-24 * `terms` -- the f32
    roundings of the coefficients and of the fma(s); terms = |x scale| + |shift| forward, |k1 dn| + |k2 x| + |k3| backward -- plus,
    bf16 given, one storage rounding u |ref| of the result (forward). NumPy arrays."""
    lim = 4 * U_F32 * np.abs(terms)
    return lim if bf16 is None else lim + (U_BF16 if bf16 else U_F32) * np.abs(ref)


def tied_windows(n):
    """(windows whose maximum is attained more than once, windows) of the 2 x 2 pooling of NumPy [B, H, W, C]."""
    B, H, W, Cn = n.shape
    win = n.reshape(B, H // 2, 2, W // 2, 2, Cn).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    return int(((win == win.max(-1, keepdims=True)).sum(-1) > 1).sum()), int(win.shape[0])


class ChannelErr:
    """conv_bound_ratios over a tensor seen one chunk of pixels at a time: add(got, ref) per chunk, ratios(tol) at the end."""

    def __init__(self):
        self.err = self.cmax = None

    def add(self, got, ref):
        got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
        Cn = ref.shape[-1]
        e, c = np.abs(got - ref).reshape(-1, Cn).max(0), np.abs(ref).reshape(-1, Cn).max(0)
        self.err = e if self.err is None else np.maximum(self.err, e)
        self.cmax = c if self.cmax is None else np.maximum(self.cmax, c)

    def ratios(self, tol):
        tmax = float(self.cmax.max()) + 1e-300
        lim = np.where(self.cmax >= DEAD * tmax, tol * self.cmax, tol * DEAD * tmax)
        ratio = self.err / lim
        c = int(ratio.argmax())
        return float(self.err.max() / tmax), float(ratio[c]), c
