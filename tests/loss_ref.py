"""
TEST INFRASTRUCTURE ONLY. Restatement (torch, f64 or f32, autograd for the gradients) of the five segmentation losses of
the reference's mpunet/evaluate/loss_functions.py as the reference's train step uses them, line by line:

  sparse_jaccard_distance_loss ................ loss_functions.py:33-62
  sparse_dice_loss ............................ :80-97
  sparse_exponential_logarithmic_loss ......... :115-145
  sparse_focal_loss ........................... :166-189
  sparse_generalized_dice_loss ................ :207-246
  alias SparseExpLogDice ...................... :270

bin/train.py:288 forces flatten_output and :357 compiles with reduction=NONE, so inside a loss y_pred is [B, H*W, K],
y_true is [B, H*W, 1] and `reduction_dims = range(len(shape))[1:-1]` is the pixel axis alone: every loss returns ONE
value per image, shape [B, 1]. Keras multiplies it by sample_weight[b]; the tape differentiates the SUM over the batch
(oracle/unet_ref.py keras_sparse_ce states the same inference for the cross-entropy); the logged loss is the MEAN over
the batch of w_b * L_b. The TensorFlow binary is absent (as for oracle/unet_ref.py): the restatement is anchored on the
hand-computed known answers of tests/test_losses_host.py. The network is the existing oracle's (oracle.unet_ref).
"""
import numpy as np
import torch

from oracle import unet_ref as U

EPS = 1e-7          # _to_tensor(10e-8, ...) :130,179
LOSSES = ("SparseDiceLoss", "SparseJaccardDistanceLoss", "SparseGeneralizedDiceLoss", "SparseFocalLoss",
          "SparseExponentialLogarithmicLoss")
ALIASES = {"SparseExpLogDice": "SparseExponentialLogarithmicLoss"}
DEFAULTS = {
    "SparseDiceLoss": dict(smooth=1),
    "SparseJaccardDistanceLoss": dict(smooth=1),
    "SparseGeneralizedDiceLoss": dict(type_weight="Square"),
    "SparseFocalLoss": dict(gamma=2, class_weights=None),
    "SparseExponentialLogarithmicLoss": dict(gamma_dice=0.3, gamma_cross=0.3, weight_dice=1, weight_cross=1),
}


def _one_hot(y, K, dtype):
    """_get_shapes_and_one_hot :23-30: y [B, M] (or [B, M, 1]) -> [B, M, K]."""
    y = y.reshape(y.shape[0], -1).long()
    return torch.nn.functional.one_hot(y, K).to(dtype)


def sparse_dice_loss(y, p, smooth=1):
    yt = _one_hot(y, p.shape[-1], p.dtype)
    intersection = (yt * p).sum(1)                                   # :94
    union = (yt + p).sum(1)                                          # :95
    dice = (2 * intersection + smooth) / (union + smooth)            # :96
    return 1.0 - dice.mean(-1, keepdim=True)                         # :97


def sparse_jaccard_distance_loss(y, p, smooth=1):
    yt = _one_hot(y, p.shape[-1], p.dtype)
    intersection = (yt * p).sum(1)                                   # :59
    sum_ = (yt + p).sum(1)                                           # :60
    jac = (intersection + smooth) / (sum_ - intersection + smooth)   # :61
    return 1.0 - jac.mean(-1, keepdim=True)                          # :62


def sparse_generalized_dice_loss(y, p, type_weight="Square"):
    yt = _one_hot(y, p.shape[-1], p.dtype)
    ref_vol = yt.sum(1)                                              # :216
    intersect = (yt * p).sum(1)                                      # :217
    seg_vol = p.sum(1)                                               # :218
    tw = type_weight.lower()
    if tw == "square":
        weights = torch.reciprocal(ref_vol ** 2)                     # :221
    elif tw == "simple":
        weights = torch.reciprocal(ref_vol)                          # :223
    elif tw == "uniform":
        weights = torch.ones_like(ref_vol)                           # :225
    else:
        raise ValueError('The variable type_weight "{}"is not defined.'.format(type_weight))
    weights = weights.detach()        # a function of the labels alone: no gradient
    new_weights = torch.where(torch.isinf(weights), torch.zeros_like(weights), weights)             # :232-234
    weights = torch.where(torch.isinf(weights), torch.ones_like(weights) * new_weights.max(), weights)   # :238-239 (max of the [B, K] tensor)
    eps = 1e-6
    numerator = 2 * weights * intersect                              # :243
    denom = weights * (seg_vol + ref_vol) + eps                      # :244
    return 1 - (numerator / denom).mean(-1, keepdim=True)            # :245-246


def sparse_focal_loss(y, p, gamma=2, class_weights=None):
    K = p.shape[-1]
    yt = _one_hot(y, K, p.dtype)
    p = torch.clamp(p, EPS, 1.0 - EPS)                               # :180
    if class_weights is None:
        class_weights = [1] * K                                      # :182-183
    cw = torch.tensor(np.asarray(class_weights, np.float64), dtype=p.dtype)
    entropy = torch.log(p)                                           # :186
    modulator = torch.pow(1 - p, gamma)                              # :187
    loss = -(cw * yt * modulator * entropy).sum(-1, keepdim=True)    # :188
    return loss.mean(1)                                              # :189


def sparse_exponential_logarithmic_loss(y, p, gamma_dice=0.3, gamma_cross=0.3, weight_dice=1, weight_cross=1):
    yt = _one_hot(y, p.shape[-1], p.dtype)
    p = torch.clamp(p, EPS, 1.0 - EPS)                               # :131
    intersect = 2 * (yt * p).sum(1) + 1                              # :134
    union = (yt + p).sum(1) + 1                                      # :135
    exp_log_dice = torch.pow(-torch.log(intersect / union), gamma_dice)       # :136
    mean_exp_log_dice = exp_log_dice.mean(-1, keepdim=True)          # :137
    entropy = (yt * -torch.log(p)).sum(-1, keepdim=True)             # :140
    exp_entropy = torch.pow(entropy, gamma_cross).mean(1)            # :141
    return weight_dice * mean_exp_log_dice + weight_cross * exp_entropy       # :144


_FUNCS = {
    "SparseDiceLoss": sparse_dice_loss,
    "SparseJaccardDistanceLoss": sparse_jaccard_distance_loss,
    "SparseGeneralizedDiceLoss": sparse_generalized_dice_loss,
    "SparseFocalLoss": sparse_focal_loss,
    "SparseExponentialLogarithmicLoss": sparse_exponential_logarithmic_loss,
}


def loss_ref(name, y, probs, sample_w=None, **kwargs):
    """w_b * L_b, shape [B, 1]. probs [B, M, K] or [B, H, W, K] torch; y integer labels with B*M entries."""
    name = ALIASES.get(name, name)
    B, K = probs.shape[0], probs.shape[-1]
    p = probs.reshape(B, -1, K)
    if not torch.is_tensor(y):
        y = torch.tensor(np.asarray(y).astype(np.int64))
    L = _FUNCS[name](y.reshape(B, -1), p, **kwargs)
    assert tuple(L.shape) == (B, 1)
    if sample_w is not None:
        L = L * torch.as_tensor(np.asarray(sample_w), dtype=p.dtype).reshape(B, 1)
    return L


def train_step(name, kwargs, w, x, y, sample_w, depth=4, dtype=torch.float64, lr=5e-5, b1=0.9, b2=0.999, eps=1e-8):
    """oracle.unet_ref.train_step with the cross-entropy replaced by `name`: probs, the [B] losses, the gradients of
    the SUM over the batch, one Adam step from zero moments, the new BN moving statistics."""
    p = U.to_torch(w, dtype, requires_grad=True)
    new_stats = {}
    probs = U.forward(p, torch.tensor(x, dtype=dtype), depth, True, "softmax", new_stats)
    loss = loss_ref(name, y, probs, sample_w, **kwargs)
    loss.sum().backward()
    names = U.trainable_names(w)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    grads = {k: p[k].grad.numpy().astype(npdt) for k in names}
    new_w = dict(w)
    for k in names:
        th, _, _ = U.adam_update(np.asarray(w[k], npdt), grads[k], np.zeros_like(grads[k]), np.zeros_like(grads[k]), 1, lr, b1, b2, eps)
        new_w[k] = th.astype(np.float32)
    for k, v in new_stats.items():
        new_w[k] = v.numpy().astype(np.float32)
    return {"loss": loss.detach().numpy().reshape(-1), "probs": probs.detach().numpy(), "grads": grads, "weights": new_w}


# ---- the closed form the kernels implement (NumPy f64): g = w (a + [y=k] c + [y=k] f) pass ----------------------------
def closed_form(name, y, p, sample_w, **kwargs):
    """p [B, M, K] f64 probabilities, y [B, M] ints, sample_w [B]. Returns (w_b L_b [B], dL/dp [B, M, K])."""
    name = ALIASES.get(name, name)
    a_ = dict(DEFAULTS[name]); a_.update(kwargs)
    p = np.asarray(p, np.float64); B, M, K = p.shape
    y = np.asarray(y).reshape(B, M)
    oh = (y[..., None] == np.arange(K)).astype(np.float64)
    w = np.asarray(sample_w, np.float64)
    clip = name in ("SparseFocalLoss", "SparseExponentialLogarithmicLoss")
    q = np.clip(p, EPS, 1 - EPS) if clip else p
    passm = ((p >= EPS) & (p <= 1 - EPS)).astype(np.float64) if clip else np.ones_like(p)
    I, P, R = (oh * q).sum(1), q.sum(1), oh.sum(1)
    a = np.zeros((B, K)); c = np.zeros((B, K)); f = np.zeros((B, M)); L = np.zeros(B)
    qy = np.take_along_axis(q, y[..., None], 2)[..., 0]
    if name == "SparseDiceLoss":
        s = a_["smooth"]; Un = P + R + s; A = 2 * I + s
        L = 1 - (A / Un).mean(1); a = A / (K * Un ** 2); c = -2 / (K * Un)
    elif name == "SparseJaccardDistanceLoss":
        s = a_["smooth"]; V = P + R - I + s; A = I + s
        L = 1 - (A / V).mean(1); a = A / (K * V ** 2); c = -(1 / V + A / V ** 2) / K
    elif name == "SparseGeneralizedDiceLoss":
        tw = a_["type_weight"].lower()
        with np.errstate(divide="ignore"):
            wt = {"square": 1 / R ** 2, "simple": 1 / R, "uniform": np.ones_like(R)}[tw]
        fin = np.where(np.isinf(wt), 0.0, wt)
        wt = np.where(np.isinf(wt), fin.max(), wt)
        Dn = wt * (P + R) + 1e-6
        L = 1 - (2 * wt * I / Dn).mean(1); a = 2 * wt ** 2 * I / (K * Dn ** 2); c = -2 * wt / (K * Dn)
    elif name == "SparseFocalLoss":
        g = a_["gamma"]; cw = np.ones(K) if a_["class_weights"] is None else np.asarray(a_["class_weights"], np.float64)
        cwy = cw[y]
        L = (-cwy * (1 - qy) ** g * np.log(qy)).mean(1)
        f = cwy / M * (g * (1 - qy) ** (g - 1) * np.log(qy) - (1 - qy) ** g / qy)
    else:
        gd, gc, wd, wc = a_["gamma_dice"], a_["gamma_cross"], a_["weight_dice"], a_["weight_cross"]
        Un = P + R + 1; A = 2 * I + 1; X = A / Un; nl = -np.log(X)
        h = -wd / K * gd * nl ** (gd - 1) / X
        L = wd * (nl ** gd).mean(1) + wc * ((-np.log(qy)) ** gc).mean(1)
        a = -h * A / Un ** 2; c = 2 * h / Un
        f = -wc * gc / M * (-np.log(qy)) ** (gc - 1) / qy
    g = w[:, None, None] * (a[:, None, :] + oh * (c[:, None, :] + f[:, :, None])) * passm
    return w * L, g


def softmax_backward(p, g):
    """dz = p * (g - sum_k g_k p_k): what the head kernels do with g."""
    return p * (g - (g * p).sum(-1, keepdims=True))
