"""Reference arithmetic and bounds of the inference replay (tests/test_gpu_replay.py), NumPy / torch-CPU only, so that the bounds
themselves can be checked without a GPU (tests/test_replay_bounds_host.py).

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


def conv_bound_ratios(got, ref):
    """(max |got - ref| / max |ref|, worst per-channel error as a fraction of ITS bound, that channel) of [..., C] arrays."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    Cn = ref.shape[-1]
    err = np.abs(got - ref).reshape(-1, Cn).max(0)
    cmax = np.abs(ref).reshape(-1, Cn).max(0)
    tmax = float(cmax.max()) + 1e-300
    lim = np.where(cmax >= DEAD * tmax, CONV_TOL * cmax, CONV_TOL * DEAD * tmax)
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
