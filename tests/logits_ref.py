"""
TEST INFRASTRUCTURE ONLY. Restatement (torch, f64 or f32, autograd for the gradients) of the train step the reference compiles with
`fit.loss_kwargs: {from_logits: true}` on a `build.out_activation: linear` model (mpunet/train/trainer.py:82:
SparseCategoricalCrossentropy(reduction=NONE, from_logits=True)).

TF 2.3: backend.sparse_categorical_crossentropy(from_logits=True) skips the probability clip and calls
nn.sparse_softmax_cross_entropy_with_logits, so per pixel  L = logsumexp_k(z_k) - z_y.  Keras multiplies by sample_weight[b], the
tape differentiates the SUM over batch and pixels, the logged loss is the MEAN over the B*H*W pixels (as oracle/unet_ref.py
keras_sparse_ce states for the clipped form). The TensorFlow binary is absent: the restatement is anchored on the hand-computed
known answers of tests/test_logits_loss_host.py. The network is the existing oracle's (oracle.unet_ref).
"""
import numpy as np
import torch

from oracle import unet_ref as U


def ce_from_logits(z, y, sample_w=None):
    """Weighted per-pixel loss [B, M]. z [B, M, K] or [B, H, W, K] torch logits; y integer labels with B*M entries; sample_w [B]."""
    B, K = z.shape[0], z.shape[-1]
    z = z.reshape(B, -1, K)
    if not torch.is_tensor(y):
        y = torch.tensor(np.asarray(y).astype(np.int64))
    y = y.reshape(B, -1).long()
    mx = z.max(-1, keepdim=True).values.detach()                    # the shift cancels: subtracting it is exact mathematics
    lse = torch.log(torch.exp(z - mx).sum(-1)) + mx[..., 0]
    L = lse - torch.gather(z, 2, y[..., None])[..., 0]
    if sample_w is not None:
        L = L * torch.as_tensor(np.asarray(sample_w), dtype=z.dtype).reshape(B, 1)
    return L


def closed_form(z, y, sample_w):
    """NumPy f64: (weighted per-pixel loss [B, M], dz [B, M, K] = w_b (softmax(z) - onehot(y))) -- what the kernels implement."""
    z = np.asarray(z, np.float64)
    B, M, K = z.shape
    y = np.asarray(y).reshape(B, M).astype(np.int64)
    w = np.asarray(sample_w, np.float64)
    d = z - z.max(-1, keepdims=True)
    e = np.exp(d)
    S = e.sum(-1)
    oh = (y[..., None] == np.arange(K)).astype(np.float64)
    L = (np.log(S) - np.take_along_axis(d, y[..., None], 2)[..., 0]) * w[:, None]
    dz = (e / S[..., None] - oh) * w[:, None, None]
    return L, dz


def train_step(w, x, y, sample_w, depth=4, dtype=torch.float64, lr=5e-5, b1=0.9, b2=0.999, eps=1e-8):
    """oracle.unet_ref.train_step on a linear output with the cross-entropy from logits: logits, the [B, M] losses, the gradients
    of the SUM, one Adam step from zero moments, the new BN moving statistics."""
    p = U.to_torch(w, dtype, requires_grad=True)
    new_stats = {}
    logits = U.forward(p, torch.tensor(x, dtype=dtype), depth, True, "linear", new_stats)
    loss = ce_from_logits(logits, y, sample_w)
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
    return {"loss": loss.detach().numpy(), "logits": logits.detach().numpy(), "grads": grads, "weights": new_w}
