"""
mpunet.models.UNet on MI355X: same constructor, attributes and Keras-Model call
surface as the reference (mpunet/models/unet.py:20-251), with every tensor
operation executed by libmpunet_hip.so (hand-written gfx950 kernels).

Host code here only owns buffers (torch device tensors), converts weights
between Keras layouts and the library's flat parameter buffer, and drives the
C ABI: mpu_unet_forward / mpu_unet_backward / mpu_adam_step /
mpu_unet_pack_weights. There is no eager / CPU fallback.
"""
import ctypes as C
import os
import numpy as np
import torch

from . import _lib


# mpunet/evaluate/loss_functions.py: class name -> (mpu_loss_kind, constructor keywords with their defaults, takes **kwargs)
_CUSTOM_LOSSES = {
    "SparseDiceLoss": (_lib.MPU_LOSS_DICE, {"smooth": 1}, True),                                   # :100-112
    "SparseJaccardDistanceLoss": (_lib.MPU_LOSS_JACCARD, {"smooth": 1}, True),                     # :65-77
    "SparseGeneralizedDiceLoss": (_lib.MPU_LOSS_GENERALIZED_DICE, {"type_weight": "Square"}, False),   # :249-266
    "SparseFocalLoss": (_lib.MPU_LOSS_FOCAL, {"gamma": 2, "class_weights": None}, False),          # :192-204
    "SparseExponentialLogarithmicLoss": (_lib.MPU_LOSS_EXP_LOG, {"gamma_dice": 0.3, "gamma_cross": 0.3, "weight_dice": 1,
                                                                 "weight_cross": 1}, False),       # :148-163
}
_CUSTOM_LOSSES["SparseExpLogDice"] = _CUSTOM_LOSSES["SparseExponentialLogarithmicLoss"]          # :270
_GDL_WEIGHTS = {"square": _lib.MPU_GDL_SQUARE, "simple": _lib.MPU_GDL_SIMPLE, "uniform": _lib.MPU_GDL_UNIFORM}
_CE = "SparseCategoricalCrossentropy"


def resolve_ce_kwargs(loss_kwargs, out_activation):
    """from_logits of tf.keras.losses.SparseCategoricalCrossentropy(reduction=NONE, **loss_kwargs) (mpunet/train/trainer.py:82) on a
    model with the given out_activation. `name` is dropped, `reduction` and unknown keys raise TypeError as the constructor call
    would; from_logits=True on a softmax output raises ValueError (the loss would apply a second softmax to probabilities)."""
    kw = dict(loss_kwargs or {})
    if "reduction" in kw:                # trainer.py:82 passes it itself
        raise TypeError("%s() got multiple values for keyword argument 'reduction'" % _CE)
    kw.pop("name", None)
    from_logits = bool(kw.pop("from_logits", False))
    for k in kw:
        raise TypeError("%s() got an unexpected keyword argument %r" % (_CE, k))
    if from_logits and out_activation != "linear":
        raise ValueError("%s(from_logits=True) on out_activation=%r would apply the softmax twice: build the model with "
                         "out_activation=\"linear\" (build.out_activation: linear), or drop from_logits"
                         % (_CE, out_activation))
    return from_logits

# tf.keras.optimizers (TF 2.3), as mpunet/train/utils.py:100-111 resolves `fit.optimizer`: class name -> (mpu_optimizer_kind,
# constructor keywords with their defaults). Adam's lr and epsilon are the project YAML's (train_hparams.yaml:125-126), which
# this class has always started from; the others take the Keras defaults.
_OPTIMIZERS = {
    "Adam": (_lib.MPU_OPT_ADAM, dict(lr=5e-5, beta_1=0.9, beta_2=0.999, epsilon=1e-8, amsgrad=False, decay=0.0)),
    "SGD": (_lib.MPU_OPT_SGD, dict(lr=0.01, momentum=0.0, nesterov=False, decay=0.0)),
    "RMSprop": (_lib.MPU_OPT_RMSPROP, dict(lr=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, decay=0.0)),
    "Adamax": (_lib.MPU_OPT_ADAMAX, dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0)),
}
_UNSUPPORTED = "supported optimizers: Adam (also amsgrad), SGD, RMSprop, Adamax, each with learning-rate decay"

# `fit.metrics` (mpunet/train/utils.py:29-97: tf.keras.metrics first, then mpunet/evaluate/metrics.py), in the order of the state
# buffer of mpu_train_metrics_update (include/mpunet_hip.h): index = position here
METRICS = ("sparse_categorical_accuracy", "sparse_fg_recall", "sparse_fg_precision", "sparse_mean_fg_precision",
           "sparse_mean_fg_recall", "sparse_mean_fg_f1")


# Class limits (include/mpunet_hip.h, mpu_unet_config): a model with up to MAX_CLASSES classes is built and predicts; training and
# evaluation stop at TRAIN_MAX_CLASSES. The message is the library guard's (csrc/unet_model.hip: require_trainable).
MAX_CLASSES, TRAIN_MAX_CLASSES = 16, 8
INFERENCE_ONLY_MSG = "U-Net training and evaluation support 1..8 classes; 9..16 are inference-only"


def require_trainable(n_classes, what):
    """NotImplementedError for an entry point of the training / evaluation side on a model with more than TRAIN_MAX_CLASSES
    classes: raised up front, before any launch or allocation of training state."""
    if int(n_classes) > TRAIN_MAX_CLASSES:
        raise NotImplementedError("%s: %s (this model has %d)" % (what, INFERENCE_ONLY_MSG, int(n_classes)))


def mean_metric(total, count):
    """Keras Mean.result(): total / count, 0 where count == 0 (div_no_nan); a NaN total stays NaN."""
    return float(total) / float(count) if count else 0.0


def _resolve_metrics(metrics):
    """The validated list of `fit.metrics` names (None, [] -> []). A name that is not one of METRICS -- `accuracy`, a Keras metric
    class, sparse_top_k_categorical_accuracy, the NumPy helpers of metrics.py (dice, dice_all, class_wise_kappa, one_class_dice)
    -- raises NotImplementedError: nothing is accepted and then left out of the logs."""
    if metrics is None:
        return []
    if isinstance(metrics, str) or not isinstance(metrics, (list, tuple)):
        metrics = [metrics]
    names = []
    for m in metrics:
        name = m if isinstance(m, str) else getattr(m, "__name__", type(m).__name__)
        if name not in METRICS:
            raise NotImplementedError("metric %r is not supported (supported metrics: %s)" % (name, ", ".join(METRICS)))
        if name in names:
            raise ValueError("metric %r is listed twice" % name)
        names.append(name)
    return names


def _resolve_optimizer(optimizer, optimizer_kwargs):
    """(class name, validated keywords) of `fit.optimizer` / `fit.optimizer_kwargs`. Unknown keywords raise TypeError as the
    Keras constructor would; what is not built raises NotImplementedError -- nothing falls back to another optimizer."""
    name = optimizer if isinstance(optimizer, str) else type(optimizer).__name__
    by_lower = {k.lower(): k for k in _OPTIMIZERS}
    if name.lower() not in by_lower:
        raise NotImplementedError("optimizer %r is not supported (%s)" % (name, _UNSUPPORTED))
    name = by_lower[name.lower()]
    kw = dict(optimizer_kwargs or {})
    kw.pop("name", None)
    if "learning_rate" in kw:
        lr = kw.pop("learning_rate")
        kw.setdefault("lr", lr)
    for k in ("clipnorm", "clipvalue"):
        if kw.get(k) is not None:
            raise NotImplementedError("gradient clipping (%s) is not supported (%s)" % (k, _UNSUPPORTED))
        kw.pop(k, None)
    defaults = _OPTIMIZERS[name][1]
    for k in kw:
        if k not in defaults:
            raise TypeError("%s() got an unexpected keyword argument %r" % (name, k))
    for k in ("amsgrad", "nesterov", "centered"):
        if k in kw:
            kw[k] = bool(kw[k])
    for k, v in kw.items():
        if not isinstance(v, bool):
            kw[k] = float(v)
    return name, kw


class _ScreenLogger:
    def __call__(self, *args, **kwargs):
        print(*args)


class _OutputLayerShim:
    """What mpunet/utils/utils.py:190-241 (set_bias_weights) needs from the last layer."""

    class _Act:
        def __init__(self, name):
            self.__name__ = name

    def __init__(self, model):
        self._m = model
        self.activation = self._Act(model.out_activation)
        self.name = "conv2d"

    def get_weights(self):
        d = self._m.get_weights_dict()
        return [d["conv2d/kernel"], d["conv2d/bias"]]

    def set_weights(self, weights):
        self._m.set_weights_dict({"conv2d/kernel": weights[0], "conv2d/bias": weights[1]})


class UNet:
    """
    2D UNet implementation with batch normalization and complexity factor adj.
    See mpunet/models/unet.py:26-79 for the meaning of the arguments. Extra
    keyword arguments (model_class_name, l1_reg, biased_output_layer, ...) are
    accepted and ignored, as the reference does (unet.py:41).

    n_classes: 1..8 trains, evaluates and predicts; 9..16 is inference-only (predict, predict_on_batch, weight I/O): everything
               of the training / evaluation side raises NotImplementedError up front.

    Additions that have no counterpart in the reference:
      dtype  : "bf16" (default; bf16 storage + MFMA, f32 accumulate), "f32" (exact-f32 MFMA: the parity mode) or
               "bf16x3" (f32 storage, split-bf16 products: logits within the north-star tolerance at ~3x the f32 mode's speed)
               (exact-f32 MFMA; the parity mode)
      device : torch device of all buffers
      seed   : seed of the glorot-uniform initialisation
    """

    def __init__(self, n_classes, img_rows=None, img_cols=None, dim=None, n_channels=1, depth=4,
                 out_activation="softmax", activation="relu", kernel_size=3, padding="same",
                 complexity_factor=1, flatten_output=False, l2_reg=None, logger=None,
                 dtype="bf16", device="cuda", seed=None, **kwargs):
        if not ((img_rows and img_cols) or dim):
            raise ValueError("Must specify either img_rows and img_col or dim")
        if dim:
            img_rows, img_cols = dim, dim
        self.logger = logger or _ScreenLogger()
        self.img_shape = (img_rows, img_cols, n_channels)
        self.n_classes = n_classes
        self.cf = np.sqrt(complexity_factor)
        self.kernel_size = kernel_size
        self.activation = activation
        self.out_activation = out_activation
        self.l2_reg = l2_reg
        self.padding = padding
        self.depth = depth
        self.flatten_output = flatten_output
        self.label_crop = np.array([[0, 0], [0, 0]])
        self.stop_training = False
        if padding != "same" or activation != "relu" or kernel_size != 3:
            raise NotImplementedError("only padding='same', activation='relu', kernel_size=3 "
                                      "are on the MI355X path")
        if out_activation not in ("softmax", "linear"):
            raise NotImplementedError("out_activation must be 'softmax' or 'linear'")
        if img_rows % (2 ** depth) or img_cols % (2 ** depth):
            raise NotImplementedError("image dims must be multiples of 2**depth (no cropping path)")
        # "bf16x3" (round 6): f32 storage, every matrix product as three bf16 MFMAs on hi + lo split operands (mpu_dtype
        # MPU_F32X3) -- the tolerance-grade mode at bf16-class matrix rates; everything outside the MFMA loops is the f32 mode
        self.split_bf16 = isinstance(dtype, str) and dtype in ("bf16x3", "f32x3")
        if self.split_bf16:
            dtype = "f32"
        self.dtype = {"bf16": torch.bfloat16, "f32": torch.float32, "float32": torch.float32,
                      "bfloat16": torch.bfloat16}[dtype] if isinstance(dtype, str) else dtype
        self.device = torch.device(device)

        cfg = _lib.UNetConfig()
        cfg.n_classes, cfg.n_channels, cfg.depth = n_classes, n_channels, depth
        cfg.H, cfg.W = img_rows, img_cols
        cfg.dtype = _lib.MPU_BF16 if self.dtype == torch.bfloat16 else (_lib.MPU_F32X3 if self.split_bf16 else _lib.MPU_F32)
        cfg.softmax = 1 if out_activation == "softmax" else 0
        self.filters = [int(64 * (2 ** l) * self.cf) for l in range(depth + 1)]      # unet.py:91,120
        for l, f in enumerate(self.filters):
            cfg.filters[l] = f
        lib = _lib.load()
        self._h = lib.mpu_unet_create(C.byref(cfg))
        if not self._h:
            raise ValueError("mpu_unet_create: " + (lib.mpu_last_error() or b"").decode())
        self._h = C.c_void_p(self._h)

        # tensor table
        self._tensors = {}
        self._order = []
        name = C.create_string_buffer(96)
        kind, off = C.c_int32(), C.c_int64()
        ps, ls = (C.c_int32 * 4)(), (C.c_int32 * 4)()
        for i in range(lib.mpu_unet_num_tensors(self._h)):
            _lib.check(lib.mpu_unet_tensor_info(self._h, i, name, 96, C.byref(kind), C.byref(off), ps, ls),
                       "mpu_unet_tensor_info")
            nm = name.value.decode()
            self._tensors[nm] = (kind.value, off.value, tuple(v for v in ps if v), tuple(v for v in ls if v))
            self._order.append(nm)
        n_par = lib.mpu_unet_param_floats(self._h)
        n_st = lib.mpu_unet_bn_state_floats(self._h)
        dev = self.device
        self.params = torch.zeros(n_par, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(n_par, dtype=torch.float32, device=dev)
        self.bn_state = torch.zeros(n_st, dtype=torch.float32, device=dev)
        self.packed = torch.zeros(lib.mpu_unet_packed_bytes(self._h), dtype=torch.uint8, device=dev)
        self._slots = None             # the optimizer's slot buffers (Adam: m, v[, vhat]), allocated at the first step
        self._ws = None
        self._ws_batch = 0
        self.optimizer_name = "Adam"
        self.optimizer_kwargs = dict(_OPTIMIZERS["Adam"][1])
        self.iterations = 0
        self._l2_ws = None
        self.reg_loss = None
        self._grad_hook = None         # e.g. an all-reduce over RCCL (multiplanarunet_amd.distributed)
        self.loss_name = "SparseCategoricalCrossentropy"
        self._per_image_loss = False   # compile() with a loss of mpunet/evaluate/loss_functions.py: one value per image
        self.from_logits = False       # compile(loss_kwargs={"from_logits": True}) on a linear model: the cross-entropy reads logits
        self._init_weights(seed)

        # receptive field of the contracting path (unet.py:104-109, utils/conv_arithmetics.py:57)
        rf, jump = 1, 1
        for _ in range(depth):
            rf += 2 * jump; rf += 2 * jump          # two 3x3 convs
            jump *= 2; rf += jump                   # 2x2 max-pool, stride 2
        rf += 2 * jump; rf += 2 * jump              # bottom convs
        self.receptive_field = np.array([rf, rf])
        self.layers = [_OutputLayerShim(self)]
        self.metrics_names = ["loss"]
        self._metric_names = []        # compile(metrics=...): the compiled names, and the device state of mpu_train_metrics_update
        self._metrics_state = None     #   (f64 view: total[6] | count[6] | scratch); None = nothing is allocated or launched
        self._loss_cfg = _lib.LossConfig()     # the compiled loss as mpu_eval_loss takes it (kind 0: the sparse cross-entropy)
        self._eval_acc = None          # evaluation (test_on_batch / evaluate / the Validation callback): buffers of its own,
        self._eval_metrics_state = None    # allocated on first use -- never the state of the running training epoch
        self._eval_ws, self._eval_ws_shape = None, None
        self._eval_loss_sum, self._eval_loss_n = 0.0, 0
        self.log()

    # ------------------------------------------------------------------ #
    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().mpu_unet_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _init_weights(self, seed):
        """Keras defaults: glorot_uniform kernels, zero biases, BN gamma=1 beta=0 mean=0 var=1."""
        rng = np.random.RandomState(seed)
        w = {}
        for nm in self._order:
            kind, off, ps, ls = self._tensors[nm]
            var = nm.split("/")[1]
            if var == "kernel":
                kh, kw, ci, co = ls
                lim = np.sqrt(6.0 / (kh * kw * ci + kh * kw * co))
                w[nm] = rng.uniform(-lim, lim, ls).astype(np.float32)
            elif var in ("gamma", "moving_variance"):
                w[nm] = np.ones(ls, np.float32)
            else:
                w[nm] = np.zeros(ls, np.float32)
        self.set_weights_dict(w)

    # ---- weights ------------------------------------------------------ #
    def _buf(self, kind):
        return self.params if kind == 0 else self.bn_state

    def get_weights_dict(self):
        """{'<layer>/<var>': ndarray} in Keras layouts (kernels HWIO), padding stripped."""
        out = {}
        host = {0: self.params.cpu().numpy(), 1: self.bn_state.cpu().numpy()}
        for nm in self._order:
            kind, off, ps, ls = self._tensors[nm]
            a = host[kind][off:off + int(np.prod(ps))].reshape(ps)
            out[nm] = self._from_stored(nm, a, ps, ls)
        return out

    @staticmethod
    def _is_concat_kernel(nm):
        return nm.startswith("upsample_L") and nm.endswith("_conv2/kernel")

    def _from_stored(self, nm, a, ps, ls):
        """Strip the channel padding. The conv after the skip-concat reads [skip(F_p), up(F_p)]:
        its input-channel padding sits after EACH half (unet.py:168-169 concat order: skip first)."""
        if self._is_concat_kernel(nm):
            F, Fp = ls[3], ps[3]
            return np.ascontiguousarray(np.concatenate([a[:, :, :F, :F], a[:, :, Fp:Fp + F, :F]], axis=2))
        return np.ascontiguousarray(a[tuple(slice(0, s) for s in ls)])

    def _to_stored(self, nm, val, ps, ls):
        a = np.zeros(ps, np.float32)
        if self._is_concat_kernel(nm):
            F, Fp = ls[3], ps[3]
            a[:, :, :F, :F] = val[:, :, :F, :]
            a[:, :, Fp:Fp + F, :F] = val[:, :, F:, :]
        else:
            a[tuple(slice(0, s) for s in ls)] = val
        return a

    def set_weights_dict(self, weights, strict=False):
        host = {0: self.params.cpu().numpy(), 1: self.bn_state.cpu().numpy()}
        for nm, val in weights.items():
            if nm not in self._tensors:
                if strict:
                    raise KeyError(nm)
                continue
            kind, off, ps, ls = self._tensors[nm]
            val = np.asarray(val, np.float32)
            if tuple(val.shape) != tuple(ls):
                raise ValueError("shape mismatch for %s: got %s expected %s" % (nm, val.shape, ls))
            a = self._to_stored(nm, val, ps, ls)
            host[kind][off:off + a.size] = a.ravel()
        self.params.copy_(torch.from_numpy(host[0]))
        self.bn_state.copy_(torch.from_numpy(host[1]))
        self._repack()

    _KERAS_VARS = {"kernel": 0, "bias": 1, "gamma": 0, "beta": 1, "moving_mean": 2, "moving_variance": 3}

    def _keras_order(self):
        """Layer creation order of unet.py (encoder, bottom, upsample, head)."""
        names = []
        for i in range(self.depth):
            names += ["encoder_L%d_conv1" % i, "encoder_L%d_conv2" % i, "encoder_L%d_BN" % i]
        names += ["bottom_conv1", "bottom_conv2", "bottom_BN"]
        for i in range(self.depth):
            p = "upsample_L%d" % i
            names += [p + "_conv1", p + "_BN1", p + "_conv2", p + "_conv3", p + "_BN2"]
        names += ["conv2d"]
        out = []
        for n in names:
            vs = ("gamma", "beta", "moving_mean", "moving_variance") if "BN" in n else ("kernel", "bias")
            out += [n + "/" + v for v in vs]
        return out

    def get_weights(self):
        d = self.get_weights_dict()
        return [d[n] for n in self._keras_order()]

    def set_weights(self, weights):
        names = self._keras_order()
        if len(weights) != len(names):
            raise ValueError("expected %d arrays" % len(names))
        self.set_weights_dict(dict(zip(names, weights)), strict=True)

    def save_weights(self, path):
        """Name-keyed weights: .npz (native; keys "<layer>__<var>") or, with h5py installed, a tf.keras
        `save_weights` .h5 file (mpunet/callbacks/mcp_clean.py:57, multiplanarunet_amd/formats.py)."""
        d = self.get_weights_dict()
        if str(path).endswith((".h5", ".hdf5")):
            from .formats import save_keras_h5
            save_keras_h5(path, d, depth=self.depth)
            return
        with open(path, "wb") as f:
            np.savez(f, **{k.replace("/", "__"): v for k, v in d.items()})

    def load_weights(self, path, by_name=True):
        """load_weights(by_name=True) (mpunet/models/model_init.py:31,56): .npz or a reference Keras .h5 checkpoint.
        The 1x1 head is unnamed in the reference (unet.py:211), so a checkpoint written by a process that had built
        other models calls it conv2d_<N>: a lone 1x1 `conv2d(_N)` layer of the file is mapped onto the head. Model
        tensors the file does not supply are reported (Keras by_name loading skips them silently; here that almost
        always means a naming problem) -- `self.missing_on_load` lists them."""
        import re
        if str(path).endswith((".h5", ".hdf5")):
            from .formats import load_keras_h5
            d = load_keras_h5(path)
        else:
            with np.load(path) as z:
                d = {k.replace("__", "/"): z[k] for k in z.files}
        if "conv2d/kernel" not in d:
            auto = sorted({k.split("/")[0] for k, v in d.items()
                           if re.fullmatch(r"conv2d_\d+/kernel", k) and tuple(np.shape(v)[:2]) == (1, 1)})
            if len(auto) == 1:
                for v in ("kernel", "bias"):
                    if auto[0] + "/" + v in d:
                        d["conv2d/" + v] = d.pop(auto[0] + "/" + v)
        self.missing_on_load = sorted(n for n in self._tensors if n not in d)
        if self.missing_on_load:
            msg = "load_weights(%s): %d model tensors not in the file (kept as they are): %s" % (
                path, len(self.missing_on_load), ", ".join(self.missing_on_load[:6]) +
                (" ..." if len(self.missing_on_load) > 6 else ""))
            if not by_name:
                raise KeyError(msg)
            self.logger(msg)
        self.set_weights_dict(d, strict=not by_name)

    def count_params(self):
        """Keras count_params(): trainable + BN moving statistics, unpadded."""
        return int(sum(int(np.prod(ls)) for (_, _, _, ls) in self._tensors.values()))

    def _repack(self):
        self._infer_dirty = True
        if self.device.type != "cuda":
            return          # host-only introspection (layout, weight I/O); nothing can run without a GPU
        _lib.call("mpu_unet_pack_weights", self._h, _lib.ptr(self.params), _lib.ptr(self.packed),
                  _lib.stream_ptr())

    # ---- execution ---------------------------------------------------- #
    def _workspace(self, batch):
        if self._ws is None or self._ws_batch < batch:
            n = _lib.load().mpu_unet_workspace_bytes(self._h, batch)
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._ws_batch = batch
        return self._ws

    def _as_input(self, X):
        if not torch.is_tensor(X):
            X = torch.from_numpy(np.ascontiguousarray(X))
        X = X.to(device=self.device, dtype=torch.float32).contiguous()
        if X.ndim != 4 or tuple(X.shape[1:]) != tuple(self.img_shape):
            raise ValueError("expected input [B,%d,%d,%d], got %s" % (self.img_shape + (tuple(X.shape),)))
        return X

    def _require_trainable(self, what):
        require_trainable(self.n_classes, what)

    def _forward(self, X, training, out=None):
        if training:
            self._require_trainable("training-mode forward")
        if self.device.type != "cuda":
            raise _lib.MpuError("UNet needs a HIP device (MI355X); there is no CPU execution path")
        B = X.shape[0]
        # the workspace layout depends on the batch it was planned for
        ws = self._workspace_exact(B)
        if training:
            self._infer_dirty = True               # the moving statistics are about to change
        elif getattr(self, "_infer_dirty", True):
            _lib.call("mpu_unet_prepare_inference", self._h, _lib.ptr(self.params), _lib.ptr(self.bn_state),
                      _lib.ptr(self.packed), _lib.stream_ptr())
            self._infer_dirty = False
        shape = (B, self.img_shape[0], self.img_shape[1], self.n_classes)
        if training and out is None:
            # train-mode forward: the probabilities stay in the workspace (the backward pass reads them there);
            # the returned tensor is a VIEW of that region, valid until the next forward
            off = int(_lib.load().mpu_unet_workspace_probs_offset(self._h, B))
            n = 4 * B * shape[1] * shape[2] * shape[3]
            view = ws[off:off + n].view(torch.float32).reshape(shape)
            _lib.call("mpu_unet_forward", self._h, B, _lib.ptr(X), _lib.ptr(self.params), _lib.ptr(self.packed),
                      _lib.ptr(self.bn_state), _lib.ptr(ws), 1, None, _lib.stream_ptr())
            return view
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.call("mpu_unet_forward", self._h, B, _lib.ptr(X), _lib.ptr(self.params), _lib.ptr(self.packed),
                  _lib.ptr(self.bn_state), _lib.ptr(ws), 1 if training else 0, _lib.ptr(out), _lib.stream_ptr())
        return out

    def workspace_regions(self, batch):
        """The workspace plan of `batch` as a list of records (index, name, offset, bytes, cls, parent): every region the library
        cuts the workspace into, with byte offset, unrounded byte length and class (_lib.MPU_WS_TENSOR / _STATS / _SCRATCH), and the
        sub-entries of regions with an internal layout (parent = index of their region). Read-only (a test aid)."""
        return _lib.workspace_regions(self._h, int(batch))

    def _workspace_exact(self, batch):
        # plans for smaller batches fit inside a larger allocation
        return self._workspace(batch)

    def predict_on_batch(self, X):
        out = self._forward(self._as_input(X), training=False)
        return out.reshape(out.shape[0], -1, self.n_classes) if self.flatten_output else out

    def max_batch(self):
        """Largest batch whose activations stay below the kernels' 2 GiB (32-bit offset) operand bound."""
        H, W = self.img_shape[:2]
        f0 = 8 * ((self.filters[0] + 7) // 8)                       # level-0 filters (padded): the largest activations
        per_image = H * W * f0 * self.params_esz()
        return max(1, int((2 ** 31 - 1) // per_image))

    def params_esz(self):
        return 2 if self.dtype == torch.bfloat16 else 4

    def auto_batch(self, n, cap=160):
        """Even chunks of n images, as large as the operand bound (and `cap`) allow: big batches fill the chip at the deep
        levels. Among the smallest chunk count and the next two, the one whose chunk size fills the rounds of the persistent
        predict kernel best (conv_halo16p: one workgroup per CU walks `tiles / workgroups` tiles -- 138 planes of 256x256
        leave its 512-channel level at 4.3 rounds, 92 planes at 2.9: 276 planes -> 3 x 92, measured -1.5 % per volume)."""
        bmax = max(1, min(cap, self.max_batch()))
        cmin = -(-n // bmax)
        if self.dtype != torch.bfloat16:
            return -(-n // cmin)
        best, best_score = cmin, -1.0
        for c in range(cmin, cmin + 3):
            if c > cmin and -(-n // c) < 64:           # small batches lose more at the deep levels than a full round wins
                break                                   # (69 planes per launch: +6 % per volume, measured)
            score = self._round_fill(-(-n // c)) - 0.002 * (c - cmin)
            if score > best_score + 1e-9:
                best, best_score = c, score
        return -(-n // best)

    def _round_fill(self, B):
        """Mean over the levels with 128-channel tiles of (rounds of 16 x 32-pixel tiles per persistent workgroup) /
        ceil(rounds) for a batch of B images; a level too small for that kernel (< 512 tiles, rows not a multiple of 16,
        narrower than 32 pixels) counts 0.9 (two workgroups per CU of the 4-wave kernel, measured flat)."""
        H, W = self.img_shape[:2]
        ncu = 256
        if self.device.type == "cuda":
            ncu = torch.cuda.get_device_properties(self.device).multi_processor_count or 256
        effs = []
        for l in range(1, self.depth + 1):
            f = self.filters[l]
            h, w = H >> l, W >> l
            if f <= 64 or f % 32:
                continue
            if h % 16 or w < 32:
                effs.append(0.9)
                continue
            nt = -(-f // 128)
            tiles = B * (h // 16) * (-(-w // 32))
            if tiles * nt < 512:
                effs.append(0.9)
                continue
            rounds = tiles / max(1, ncu // nt)
            effs.append(rounds / float(-(-tiles // max(1, ncu // nt))))
        return sum(effs) / len(effs) if effs else 1.0

    def predict(self, X, batch_size=8, verbose=0):
        """model.predict: inference-mode forward in chunks of batch_size (None: auto_batch); returns a device tensor."""
        numpy_in = not torch.is_tensor(X)
        n = X.shape[0]
        if batch_size is None:
            batch_size = self.auto_batch(n)
        out = torch.empty((n, self.img_shape[0], self.img_shape[1], self.n_classes),
                          dtype=torch.float32, device=self.device)
        for s in range(0, n, batch_size):
            xb = self._as_input(X[s:s + batch_size])
            self._forward(xb, training=False, out=out[s:s + xb.shape[0]])
        if self.flatten_output:
            out = out.reshape(n, -1, self.n_classes)
        return out.cpu().numpy() if numpy_in else out

    __call__ = predict_on_batch

    # ---- training ------------------------------------------------------ #
    def compile(self, optimizer="Adam", loss=None, metrics=None, optimizer_kwargs=None, loss_kwargs=None, **kwargs):
        """
        Trainer.compile_model (mpunet/train/trainer.py:51-97): Adam with SparseCategoricalCrossentropy(reduction=NONE)
        (the reference default) or one of the losses of mpunet/evaluate/loss_functions.py -- SparseDiceLoss,
        SparseJaccardDistanceLoss, SparseGeneralizedDiceLoss, SparseFocalLoss, SparseExponentialLogarithmicLoss
        (alias SparseExpLogDice) -- with `loss_kwargs` as their constructors take them (trainer.py:82). Those five give ONE
        loss value per image (reduction=NONE over the flattened output): forward_backward / train_step return [B, 1].
        SparseCategoricalCrossentropy takes `loss_kwargs` too (resolve_ce_kwargs): {"from_logits": True} on a model built with
        out_activation="linear" is TF's sparse_softmax_cross_entropy_with_logits -- logsumexp(z) - z_y per pixel, no probability
        clip, gradient softmax(z) - onehot(y) -- and is what trains and evaluates such a model (`self.from_logits`); its output
        stays the logits. The five per-image losses need out_activation="softmax".

        `optimizer`: Adam, SGD, RMSprop or Adamax by their tf.keras.optimizers names, `optimizer_kwargs` as their constructors
        take them (an unknown key: TypeError; anything else Keras has: NotImplementedError). A key that is omitted takes the
        Keras default when the optimizer's NAME changes (Adam: this project's lr 5e-5, epsilon 1e-8) and slots and step count
        start from zero. Compiling the SAME name again UPDATES the stored kwargs and keeps the state, as it always did for
        Adam's lr: compile("SGD", momentum 0.9) then compile("SGD") still has momentum 0.9, and amsgrad / nesterov / centered /
        decay stay set until they are given again. Pass every key, or compile another name in between, for a fresh start.

        `metrics`: names out of METRICS -- tf.keras.metrics' sparse_categorical_accuracy and sparse_fg_recall, sparse_fg_precision,
        sparse_mean_fg_precision, sparse_mean_fg_recall, sparse_mean_fg_f1 of mpunet/evaluate/metrics.py:84-156 -- anything else
        raises NotImplementedError; None / [] compile none (nothing allocated, no launch added to the step). As in Keras they are
        UNWEIGHTED (sample_weight goes to the loss only) and each is the Mean over the epoch's batches (accuracy: over its
        pixels) of the batch's value, NaN batches included: metrics_result(), reset_metrics(). Every training forward then
        feeds the step's probabilities and labels to mpu_train_metrics_update (csrc/train_metrics.hip), eager or inside the
        graphed step. The three sparse_mean_fg_* call tf.confusion_matrix / tf.diag_part, TF-1 names that the reference's pinned
        TF 2.3 no longer has (there they raise AttributeError); they are built with the semantics of the renamed
        tf.math.confusion_matrix / tf.linalg.diag_part: classes above the largest one present in the batch's labels and
        predictions drop out of the mean. Values are f64 from exact integer counts; Keras keeps f32 totals (and rounds accuracy
        totals above 2**24 pixels), which is not imitated. Compiling another list starts the state from zero.
        """
        opt_name, opt_kw = _resolve_optimizer(optimizer, optimizer_kwargs)     # (all three raise before anything is changed)
        metric_names = _resolve_metrics(metrics)
        if metric_names:
            self._require_trainable("compile(metrics=...)")
        same = opt_name == self.optimizer_name  # another optimizer starts from its own defaults
        new_kw = dict(self.optimizer_kwargs if same else _OPTIMIZERS[opt_name][1])
        new_kw.update(opt_kw)
        n_slots = self._optimizer_config(opt_name, new_kw)[1]
        if loss is not None:
            lname = loss if isinstance(loss, str) else getattr(loss, "__name__", type(loss).__name__)
            if isinstance(loss, (list, tuple)):
                if len(loss) != 1:
                    raise NotImplementedError("one loss per model (the reference's U-Net has one output)")
                lname = loss[0] if isinstance(loss[0], str) else type(loss[0]).__name__
            if lname in _CUSTOM_LOSSES:
                self._require_trainable("compile(loss=%r)" % lname)
                self._set_loss(lname, dict(loss_kwargs or {}))
            elif "sparsecategoricalcrossentropy" in lname.lower().replace("_", ""):
                from_logits = resolve_ce_kwargs(loss_kwargs, self.out_activation)
                if from_logits:
                    self._require_trainable("compile(loss=%r)" % lname)
                self._set_loss(None, {}, from_logits=from_logits)
            else:
                raise NotImplementedError("loss %r is not supported: SparseCategoricalCrossentropy or one of %s"
                                          % (lname, ", ".join(sorted(_CUSTOM_LOSSES))))
        if not same or (self._slots is not None and len(self._slots) != n_slots):
            self._slots = None                  # no state of the previous optimizer (or of another variant: other slots)
            self.iterations = 0
        self.optimizer_name, self.optimizer_kwargs = opt_name, new_kw
        if metric_names != self._metric_names:
            self._metric_names = metric_names
            self.metrics_names = ["loss"] + metric_names
            self._metrics_state = None
            self._eval_metrics_state = None
            if metric_names:
                n = int(_lib.load().mpu_train_metrics_state_bytes())
                self._metrics_state = torch.zeros(n // 8, dtype=torch.float64, device=self.device)
        return self

    def metrics_description(self):
        """The line Trainer.compile_model logs (trainer.py:100, "Metrics:     %s")."""
        return str(list(self._metric_names))

    def reset_metrics(self):
        """Start the compiled metrics from zero (Keras does at the start of every epoch)."""
        if self._metrics_state is not None:
            self._metrics_state.zero_()

    def metrics_totals(self, reset=False):
        """{name: (total, count)} of the compiled metrics since the last reset: ONE device read."""
        if self._metrics_state is None:
            return {}
        nm = len(METRICS)
        host = self._metrics_state[:2 * nm].cpu().numpy()
        if reset:
            self._metrics_state.zero_()
        return {name: (float(host[METRICS.index(name)]), float(host[nm + METRICS.index(name)])) for name in self._metric_names}

    def metrics_result(self):
        """{name: value} of the compiled metrics since the last reset_metrics() (Keras Mean.result(): total / count, 0 where
        count == 0): ONE device read."""
        return {name: mean_metric(t, c) for name, (t, c) in self.metrics_totals().items()}

    def _update_metrics(self, probs, y):
        """One batch into the metric state: right behind the training forward, on its stream (probs: the f32 view the forward left
        in the workspace; y: uint8 [B, H*W])."""
        if self._metrics_state is None:
            return
        _lib.call("mpu_train_metrics_update", _lib.ptr(probs), _lib.ptr(y), int(y.numel()), int(self.n_classes),
                  _lib.ptr(self._metrics_state), _lib.stream_ptr())

    def optimizer_description(self):
        """The line Trainer.compile_model logs (trainer.py:98, "Optimizer:   %s")."""
        return "%s(%s)" % (self.optimizer_name, ", ".join("%s=%r" % kv for kv in self.optimizer_kwargs.items()))

    def _plain_adam(self):
        """The default configuration -- Adam without decay and AMSGrad -- keeps its own entry points (mpu_unet_backward_adam: the
        optimizer beside the weight gradients); every other one runs the backward pass, then ONE update-and-pack launch."""
        k = self.optimizer_kwargs
        return self.optimizer_name == "Adam" and not k.get("decay") and not k.get("amsgrad")

    def _optimizer_config(self, name=None, k=None):
        """(mpu_optimizer_config of the compiled optimizer, its number of slot buffers); the library validates the values
        (mpu_optimizer_num_slots: what the Keras constructors refuse)."""
        name, k = name or self.optimizer_name, self.optimizer_kwargs if k is None else k
        cfg = _lib.OptimizerConfig()
        cfg.kind = _OPTIMIZERS[name][0]
        cfg.flags = (_lib.MPU_OPT_NESTEROV if k.get("nesterov") else 0) | (_lib.MPU_OPT_AMSGRAD if k.get("amsgrad") else 0) \
            | (_lib.MPU_OPT_CENTERED if k.get("centered") else 0)
        cfg.lr, cfg.decay = float(k["lr"]), float(k.get("decay", 0.0))
        cfg.beta1, cfg.beta2 = float(k.get("beta_1", 0.9)), float(k.get("beta_2", 0.999))
        cfg.epsilon, cfg.momentum, cfg.rho = float(k.get("epsilon", 1e-7)), float(k.get("momentum", 0.0)), float(k.get("rho", 0.9))
        n = _lib.load().mpu_optimizer_num_slots(C.byref(cfg))
        if n < 0:
            raise ValueError("%s: %s" % (name, (_lib.load().mpu_last_error() or b"").decode()))
        return cfg, n

    def _slot_ptrs(self):
        return (C.c_void_p * 3)(*[s.data_ptr() for s in self._slots] + [None] * (3 - len(self._slots)))

    def _set_loss(self, lname, kw, from_logits=False):
        """Validate `kw` against the constructor of loss_functions.<lname> and attach the loss to the library handle
        (mpu_unet_set_loss). lname None: back to the sparse cross-entropy -- on probabilities (a softmax model; on a linear one what
        this class has always done there: it predicts, it does not train), or with from_logits on the logits of a linear model."""
        cfg = _lib.LossConfig()
        if lname is None:
            if not self._per_image_loss and not self.from_logits and not from_logits:
                return                     # nothing attached: the handle is as mpu_unet_create made it
            cfg.kind = _lib.MPU_LOSS_SPARSE_CE_LOGITS if from_logits else _lib.MPU_LOSS_SPARSE_CE
        else:
            kind, defaults, var_kw = _CUSTOM_LOSSES[lname]
            if self.out_activation != "softmax":
                raise ValueError("%s is defined on class probabilities: it needs out_activation='softmax'" % lname)
            if "reduction" in kw:        # trainer.py:82 passes it itself
                raise TypeError("%s() got multiple values for keyword argument 'reduction'" % lname)
            kw.pop("name", None)
            unknown = [k for k in kw if k not in defaults]
            if unknown and not var_kw:   # (SparseDiceLoss / SparseJaccardDistanceLoss take and drop **kwargs, :71,106)
                raise TypeError("%s() got an unexpected keyword argument %r" % (lname, unknown[0]))
            a = dict(defaults)
            a.update({k: v for k, v in kw.items() if k in defaults})
            cfg.kind = kind
            cfg.smooth = float(a.get("smooth", 1))
            if kind in (_lib.MPU_LOSS_DICE, _lib.MPU_LOSS_JACCARD) and not cfg.smooth >= 0:
                raise ValueError("%s: smooth must not be negative" % lname)
            if kind == _lib.MPU_LOSS_GENERALIZED_DICE:
                tw = str(a["type_weight"]).lower()
                if tw not in _GDL_WEIGHTS:                         # loss_functions.py:226-228
                    raise ValueError('The variable type_weight "%s" is not defined.' % a["type_weight"])
                cfg.type_weight = _GDL_WEIGHTS[tw]
            cfg.gamma = float(a.get("gamma", 2))
            cfg.gamma_dice, cfg.gamma_cross = float(a.get("gamma_dice", .3)), float(a.get("gamma_cross", .3))
            cfg.weight_dice, cfg.weight_cross = float(a.get("weight_dice", 1)), float(a.get("weight_cross", 1))
            cw = a.get("class_weights")
            if cw is not None:
                cw = [float(v) for v in np.asarray(cw, np.float64).ravel()]
                if len(cw) != self.n_classes:
                    raise ValueError("%s: class_weights needs %d entries, got %d" % (lname, self.n_classes, len(cw)))
                cfg.n_class_weights = len(cw)
                for i, v in enumerate(cw):
                    cfg.class_weights[i] = v
        _lib.call("mpu_unet_set_loss", self._h, C.byref(cfg))
        self._loss_cfg = cfg
        self.loss_name = lname or "SparseCategoricalCrossentropy"
        self._per_image_loss = lname is not None
        self.from_logits = bool(from_logits) and lname is None
        self._ws = None                    # the workspace plan of a handle with a per-image loss is larger
        self._ws_batch = 0

    def _ensure_slots(self):
        if self._slots is None:
            self._slots = [torch.zeros_like(self.params) for _ in range(self._optimizer_config()[1])]

    _ensure_adam = _ensure_slots

    @property
    def _adam_m(self):
        return self._slots[0] if self._slots and self.optimizer_name == "Adam" else None

    @property
    def _adam_v(self):
        return self._slots[1] if self._slots and self.optimizer_name == "Adam" else None

    def grad_ready_points(self):
        """Float offsets (descending) of the backward pass's gradient-ready points: after point k every gradient at
        offset >= offsets[k] of the flat buffer is final (head, up blocks, bottom, encoder levels)."""
        import ctypes as C
        buf = (C.c_int64 * 32)()
        n = _lib.load().mpu_unet_grad_ready_points(self._h, buf, 32)
        return [int(buf[i]) for i in range(n)]

    def forward_backward(self, x, y, sample_weight=None, want_loss=True, ready_events=None, adam=None, loss_out=None):
        """Train-mode forward + backward; fills self.grads (sum-gradient). Returns (probs, loss[B,H*W] or None); with a per-image
        loss (compile) the loss is [B,1]: sample_weight[b] * L_b.
        ready_events: optional list (one entry per grad_ready_points(), None = skip) of torch.cuda.Event recorded
        on the current stream when that part of the gradient buffer is final (data-parallel overlap).
        adam: (t, step_dev) -- ALSO apply the optimizer inside the same library call (mpu_unet_backward_adam: the
        update of the deep levels' parameters runs beside the weight gradients of the high-resolution levels).
        loss_out: caller-owned f32 device tensor for the loss (default: allocated here)."""
        self._require_trainable("forward_backward")
        X = self._as_input(x)
        B = X.shape[0]
        if not torch.is_tensor(y):
            y = torch.from_numpy(np.ascontiguousarray(y))
        y = y.to(device=self.device, dtype=torch.uint8).reshape(B, -1).contiguous()
        if y.shape[1] != self.img_shape[0] * self.img_shape[1]:
            raise ValueError("labels must have H*W entries per image")
        if sample_weight is None:
            sw = torch.ones(B, dtype=torch.float32, device=self.device)
        else:
            sw = torch.as_tensor(np.asarray(sample_weight, np.float32) if not torch.is_tensor(sample_weight)
                                 else sample_weight).to(device=self.device, dtype=torch.float32).contiguous()
        probs = self._forward(X, training=True)
        self._update_metrics(probs, y)
        loss = None
        if want_loss:
            loss = _lib.owned(loss_out, (B, 1 if self._per_image_loss else y.shape[1]), torch.float32, self.device, "loss_out")
        if adam is not None:
            if ready_events is not None:
                raise ValueError("forward_backward: adam= and ready_events= exclude each other")
            t, step_dev = adam
            k = self.optimizer_kwargs
            _lib.call("mpu_unet_backward_adam", self._h, B, _lib.ptr(y), _lib.ptr(sw), _lib.ptr(self.params),
                      _lib.ptr(self.packed), _lib.ptr(self.bn_state), _lib.ptr(self._ws), _lib.ptr(self.grads),
                      _lib.ptr(loss), _lib.ptr(self._adam_m), _lib.ptr(self._adam_v), int(t), _lib.ptr(step_dev),
                      float(k["lr"]), float(k["beta_1"]), float(k["beta_2"]), float(k["epsilon"]), _lib.stream_ptr())
            self._infer_dirty = True
        elif ready_events is None:
            _lib.call("mpu_unet_backward", self._h, B, _lib.ptr(y), _lib.ptr(sw), _lib.ptr(self.params),
                      _lib.ptr(self.packed), _lib.ptr(self.bn_state), _lib.ptr(self._ws), _lib.ptr(self.grads),
                      _lib.ptr(loss), _lib.stream_ptr())
        else:
            import ctypes as C
            arr = (C.c_void_p * len(ready_events))(*[None if e is None else e.cuda_event for e in ready_events])
            _lib.call("mpu_unet_backward_events", self._h, B, _lib.ptr(y), _lib.ptr(sw), _lib.ptr(self.params),
                      _lib.ptr(self.packed), _lib.ptr(self.bn_state), _lib.ptr(self._ws), _lib.ptr(self.grads),
                      _lib.ptr(loss), arr, len(ready_events), _lib.stream_ptr())
        self._ready_events_fresh = ready_events is not None      # the DP hook falls back to a full stream wait otherwise
        self._last_batch = B
        return probs, loss

    def loss_mean(self):
        """Device scalar (a [1] f32 VIEW into the workspace, valid until the next backward pass): the mean over all pixels of the
        weighted per-pixel loss (a per-image loss: the mean over the batch of w_b * L_b) of the last forward_backward / train_step
        -- what Keras logs per batch. Produced by the backward pass itself (mpu_unet_workspace_loss_mean_offset), so a training loop needs no reduction of the 1-MB loss tensor; inside a
        captured HIP graph that torch reduction (several blocks per output, semaphores) went stale for stretches of replays."""
        off = int(_lib.load().mpu_unet_workspace_loss_mean_offset(self._h, self._last_batch))
        return self._ws[off:off + 4].view(torch.float32)

    def _add_l2(self, want_loss=False):
        """kernel_regularizer=l2(self.l2_reg) (unet.py:189): grads += 2*l2*W on the 3x3 / 2x2 conv kernels; the
        term l2*sum(W^2) that Keras adds to the reported loss lands in self.reg_loss (device scalar)."""
        if not self.l2_reg:
            return
        if self._l2_ws is None:
            n = int(_lib.load().mpu_unet_l2_workspace_doubles())
            self._l2_ws = torch.empty(n, dtype=torch.float64, device=self.device)
            self.reg_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        _lib.call("mpu_unet_l2_regularizer", self._h, _lib.ptr(self.params), _lib.ptr(self.grads),
                  float(self.l2_reg), _lib.ptr(self._l2_ws), _lib.ptr(self.reg_loss) if want_loss else None,
                  _lib.stream_ptr())

    def apply_gradients(self, fused=True):
        """The compiled optimizer on the flat parameter buffer + refresh of the packed MFMA operands: one launch
        (mpu_unet_adam_pack; mpu_unet_optimizer_pack for anything but plain Adam); fused=False runs the two separate passes
        (mpu_adam_step / mpu_optimizer_step, mpu_unet_pack_weights; bit-identical, kept for the equality test)."""
        self._ensure_slots()
        self.iterations += 1
        k = self.optimizer_kwargs
        if not self._plain_adam():
            cfg = self._optimizer_config()[0]
            if fused:
                _lib.call("mpu_unet_optimizer_pack", self._h, C.byref(cfg), _lib.ptr(self.params), _lib.ptr(self.grads),
                          self._slot_ptrs(), self.iterations, None, _lib.ptr(self.packed), _lib.stream_ptr())
                self._infer_dirty = True
                return
            _lib.call("mpu_optimizer_step", C.byref(cfg), _lib.ptr(self.params), _lib.ptr(self.grads), self._slot_ptrs(),
                      self.params.numel(), self.iterations, None, _lib.stream_ptr())
            self._repack()
            return
        if fused:
            _lib.call("mpu_unet_adam_pack", self._h, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self._adam_m),
                      _lib.ptr(self._adam_v), self.iterations, None, float(k["lr"]), float(k["beta_1"]),
                      float(k["beta_2"]), float(k["epsilon"]), _lib.ptr(self.packed), _lib.stream_ptr())
            self._infer_dirty = True
            return
        _lib.call("mpu_adam_step", _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self._adam_m),
                  _lib.ptr(self._adam_v), self.params.numel(), self.iterations, float(k["lr"]),
                  float(k["beta_1"]), float(k["beta_2"]), float(k["epsilon"]), _lib.stream_ptr())
        self._repack()

    # ---- HIP-graph replay of the whole step (launch-bound regime) ---------------------------------
    def make_graphed_train_step(self, x, y, sample_weight=None, loss_sum=None, warmup=True):
        """
        Capture forward + backward + Adam + repack (~130 kernel launches) into one HIP graph that reads the
        given DEVICE tensors x, y, sample_weight in place; returns replay() which runs one train step per
        call. Single-GPU only (the RCCL all-reduce stays eager). The Adam step count lives on the device.
        loss_sum: optional f64 device scalar; every step adds its mean weighted per-pixel loss (+ the l2 term) to it ON THE
        DEVICE (`mp train` reads it once per epoch, pipeline.TrainPipeline). warmup=False: capture only (a re-capture after
        a learning-rate change -- the rate is a kernel argument of the captured launches); `replay.warmup_ran` tells.
        """
        self._require_trainable("make_graphed_train_step")
        if self._grad_hook is not None:
            raise NotImplementedError("graphed train step is single-GPU (gradient all-reduce is eager)")
        for t in (x, y):
            if not torch.is_tensor(t) or t.device.type != "cuda":
                raise ValueError("graphed train step needs device tensors")
        self._ensure_slots()
        if not warmup and (self._ws is None or (self.l2_reg and self._l2_ws is None)):
            #  a capture without a warm-up step is a RE-capture: the lazily created buffers must exist already, or
            # their allocations would land in the graph's private pool
            raise RuntimeError("make_graphed_train_step(warmup=False) needs a model that has already run a train step")
        step_dev = torch.tensor([self.iterations], dtype=torch.int64, device=self.device)
        k = self.optimizer_kwargs

        plain_adam = self._plain_adam()
        fused_tail = plain_adam and not self.l2_reg and os.environ.get("MPU_FUSED_ADAM") != "0"
        cfg = None if plain_adam else self._optimizer_config()[0]      # (lr is captured by value: a new rate needs a re-capture)
        slot_ptrs = None if plain_adam else self._slot_ptrs()

        def body():
            if fused_tail:               # backward + optimizer in one call: the optimizer beside the weight gradients
                self.forward_backward(x, y, sample_weight, want_loss=False, adam=(0, step_dev))
                if loss_sum is not None:
                    loss_sum.add_(self.loss_mean().double())     # (the pass's own mean: no torch reduction inside the graph)
                return
            self.forward_backward(x, y, sample_weight, want_loss=False)
            self._add_l2(want_loss=loss_sum is not None)
            if loss_sum is not None:
                loss_sum.add_(self.loss_mean().double())
                if self.l2_reg:
                    loss_sum.add_(self.reg_loss.double())
            if not plain_adam:           # the serial tail: ONE update-and-pack launch behind the backward pass
                _lib.call("mpu_unet_optimizer_pack", self._h, C.byref(cfg), _lib.ptr(self.params), _lib.ptr(self.grads),
                          slot_ptrs, 0, _lib.ptr(step_dev), _lib.ptr(self.packed), _lib.stream_ptr())
                self._infer_dirty = True
                return
            if os.environ.get("MPU_FUSED_ADAM") == "0":         # A/B: the two separate passes
                _lib.call("mpu_adam_step_device_counter", _lib.ptr(self.params), _lib.ptr(self.grads),
                          _lib.ptr(self._adam_m), _lib.ptr(self._adam_v), self.params.numel(), _lib.ptr(step_dev),
                          float(k["lr"]), float(k["beta_1"]), float(k["beta_2"]), float(k["epsilon"]), _lib.stream_ptr())
                self._repack()
                return
            _lib.call("mpu_unet_adam_pack", self._h, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self._adam_m),
                      _lib.ptr(self._adam_v), 0, _lib.ptr(step_dev), float(k["lr"]), float(k["beta_1"]),
                      float(k["beta_2"]), float(k["epsilon"]), _lib.ptr(self.packed), _lib.stream_ptr())
            self._infer_dirty = True

        if warmup:
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):               # warm-up outside capture (lazy inits, allocations): a REAL step
                body()
            torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        if warmup:
            self.iterations += 1                        # the warm-up step

        def replay():
            graph.replay()
            self.iterations += 1
            self._infer_dirty = True
        replay.graph = graph
        replay.warmup_ran = bool(warmup)
        # Everything the captured launches address must outlive the graph. The Adam step counter is created HERE: without this
        # reference it was freed when this function returned, the caching allocator handed its block to the next small tensor
        # on the stream, and the replayed Adam kernels then read that tensor's bytes as the step count -- a wrong bias correction
        # (up to NaN) from the first allocation after the capture on (found by tests/test_gpu_pipeline.py, round 5).
        # (The model's own buffers too: a later, larger eager batch REPLACES self._ws -- the graph keeps running on the one it
        # was captured with, which must therefore stay allocated.)
        replay.keep_alive = (step_dev, x, y, sample_weight, loss_sum, self._ws, self._l2_ws, getattr(self, "reg_loss", None),
                             tuple(self._slots), self.params, self.grads, self.packed, self.bn_state, self._metrics_state)
        return replay

    def train_step(self, x, y, sample_weight=None, want_loss=True, loss_out=None):
        """One Model.fit inner step. Returns the per-pixel loss [B,H*W] (device) or None (loss_out: as
        forward_backward)."""
        self._require_trainable("train_step")
        hook = self._grad_hook
        if hook is None and not self.l2_reg and self._plain_adam():     # single GPU, no l2 term: backward + optimizer as one library call
            self._ensure_slots()
            self.iterations += 1
            _, loss = self.forward_backward(x, y, sample_weight, want_loss, adam=(self.iterations, None), loss_out=loss_out)
            return loss
        events = getattr(hook, "ready_events", None)
        _, loss = self.forward_backward(x, y, sample_weight, want_loss, ready_events=events, loss_out=loss_out)
        if hook is not None:
            hook(self.grads)                     # data-parallel: SUM of replica gradients
        self._add_l2(want_loss)                  # once, after the replica sum (Keras scales it 1/replicas per replica)
        self.apply_gradients()
        return loss

    def _batch_loss(self, x, y, sample_weight=None):
        loss = float(self.train_step(x, y, sample_weight).mean().item())
        return loss + float(self.reg_loss.item()) if self.l2_reg else loss

    def train_on_batch(self, x, y, sample_weight=None):
        """Scalar Keras reports for the step: mean of the weighted per-pixel loss (+ the l2 term when l2_reg is set). With compiled
        metrics: [loss, m1, ...] of THIS batch in the order of metrics_names (Keras' default reset_metrics=True: the state holds
        this batch alone afterwards)."""
        self._require_trainable("train_on_batch")
        self.reset_metrics()
        loss = self._batch_loss(x, y, sample_weight)
        if not self._metric_names:
            return loss
        res = self.metrics_result()
        return [loss] + [res[n] for n in self._metric_names]

    # ---- evaluation ----------------------------------------------------- #
    def evaluation_begin(self):
        """(acc, metrics_state): the zeroed device accumulators of one evaluation pass, owned by the model and apart from the
        training epoch's metric state -- acc f64 [2] (sum of batch-mean losses, number of batches), metrics_state as
        mpu_train_metrics_update lays it out (None without compiled metrics)."""
        if self._eval_acc is None:
            self._eval_acc = torch.zeros(2, dtype=torch.float64, device=self.device)
        if self._metric_names and self._eval_metrics_state is None:
            n = int(_lib.load().mpu_train_metrics_state_bytes())
            self._eval_metrics_state = torch.zeros(n // 8, dtype=torch.float64, device=self.device)
        self._eval_acc.zero_()
        if self._eval_metrics_state is not None:
            self._eval_metrics_state.zero_()
        self._eval_loss_sum, self._eval_loss_n = 0.0, 0        # test_on_batch / evaluate: sum of w_b * L_b and number of images
        return self._eval_acc, self._eval_metrics_state

    def evaluation_update(self, probs, y, acc=None, metrics_state=None, sample_weight=None, loss_out=None):
        """One batch of already-computed probabilities (f32 device tensor, [B, ..., K]: predict_on_batch's output) and labels into
        device accumulators, no host read: the compiled loss of the batch by mpu_eval_loss (csrc/eval_loss.hip) -- acc[0] += mean
        over the batch of w_b * L_b, acc[1] += 1; loss_out f32 [B] receives w_b * L_b -- and the compiled metrics by
        mpu_train_metrics_update into metrics_state (unweighted). The Validation callback feeds its batches through here."""
        self._require_trainable("evaluation_update")
        K = int(self.n_classes)
        B = int(probs.shape[0])
        p = probs.reshape(B, -1, K)
        if p.dtype != torch.float32 or not p.is_contiguous():
            p = p.to(torch.float32).contiguous()
        if not torch.is_tensor(y):
            y = torch.from_numpy(np.ascontiguousarray(y))
        y = y.to(device=p.device, dtype=torch.uint8).reshape(B, -1).contiguous()
        ppi = int(p.shape[1])
        if y.shape[1] != ppi:
            raise ValueError("evaluation_update: %d labels for %d predictions per image" % (y.shape[1], ppi))
        sw = None
        if sample_weight is not None:
            sw = torch.as_tensor(np.asarray(sample_weight, np.float32) if not torch.is_tensor(sample_weight)
                                 else sample_weight).to(device=p.device, dtype=torch.float32).reshape(-1).contiguous()
            if sw.numel() != B:
                raise ValueError("evaluation_update: sample_weight needs one entry per image")
        if self._eval_ws is None or self._eval_ws_shape != (B, ppi):      # (validation batches share one shape: one query per run)
            need = int(_lib.load().mpu_eval_loss_scratch_bytes(B, ppi, K))
            if need < 0:
                raise ValueError("mpu_eval_loss: " + (_lib.load().mpu_last_error() or b"").decode())
            if self._eval_ws is None or self._eval_ws.numel() < need:
                self._eval_ws = torch.empty(need, dtype=torch.uint8, device=p.device)
            self._eval_ws_shape = (B, ppi)
        if self.from_logits:               # `probs` holds the linear model's logits
            _lib.call("mpu_eval_loss_logits", _lib.ptr(p), _lib.ptr(y), _lib.ptr(sw), B, ppi, K,
                      _lib.ptr(self._eval_ws), _lib.ptr(loss_out), _lib.ptr(acc), _lib.stream_ptr())
        else:
            _lib.call("mpu_eval_loss", C.byref(self._loss_cfg), _lib.ptr(p), _lib.ptr(y), _lib.ptr(sw), B, ppi, K,
                      _lib.ptr(self._eval_ws), _lib.ptr(loss_out), _lib.ptr(acc), _lib.stream_ptr())
        if metrics_state is not None and self._metric_names:
            _lib.call("mpu_train_metrics_update", _lib.ptr(p), _lib.ptr(y), B * ppi, K, _lib.ptr(metrics_state),
                      _lib.stream_ptr())

    def evaluation_totals(self, acc, metrics_state=None):
        """{"loss": (total, count), <metric>: (total, count), ...} of the accumulators, in metrics_names order: the pairs a Keras
        Mean holds (result: mean_metric), ready for a SUM all-reduce over replicas."""
        out = {"loss": tuple(float(v) for v in acc.cpu().tolist())}
        if metrics_state is not None and self._metric_names:
            nm = len(METRICS)
            host = metrics_state[:2 * nm].cpu().numpy()
            for name in self._metric_names:
                out[name] = (float(host[METRICS.index(name)]), float(host[nm + METRICS.index(name)]))
        return out

    def l2_penalty(self):
        """l2_reg * sum W^2 over the kernels mpu_unet_l2_regularizer covers (every conv kernel but the 1x1 head's), in f64,
        without touching the gradients: the term Keras adds to an evaluated loss. Device scalar; None without l2_reg."""
        if not self.l2_reg:
            return None
        tot = torch.zeros((), dtype=torch.float64, device=self.device)
        for nm in self._order:
            kind, off, ps, _ = self._tensors[nm]
            if kind == 0 and nm.endswith("/kernel") and nm != "conv2d/kernel":
                tot += self.params[off:off + int(np.prod(ps))].double().pow(2).sum()     # (the channel padding holds zeros)
        return tot * float(np.float32(self.l2_reg))                                      # (the train step's l2 is an f32 too)

    def _evaluate_chunks(self, x, y, sample_weight, batch_size, reset_metrics):
        """The inference-mode forward (BatchNorm on the moving statistics: predict_on_batch's path) over chunks of batch_size images,
        each fed to evaluation_update; the per-image losses w_b * L_b land in one [N] buffer whose mean is Keras' loss Mean
        (weighted by batch size). One host read at the end."""
        n = int(x.shape[0])
        if n < 1:
            raise ValueError("evaluation needs at least one image")
        if reset_metrics or self._eval_acc is None or (self._metric_names and self._eval_metrics_state is None):
            self.evaluation_begin()
        state = self._eval_metrics_state
        if not torch.is_tensor(y):
            y = torch.from_numpy(np.ascontiguousarray(y))
        y = y.reshape(n, -1)
        if sample_weight is not None and not torch.is_tensor(sample_weight):
            sample_weight = torch.from_numpy(np.asarray(sample_weight, np.float32))
        per_image = torch.empty(n, dtype=torch.float32, device=self.device)
        for s in range(0, n, batch_size):
            e = min(n, s + batch_size)
            probs = self._forward(self._as_input(x[s:e]), training=False)
            self.evaluation_update(probs, y[s:e], None, state, None if sample_weight is None else sample_weight[s:e],
                                   loss_out=per_image[s:e])
        self._eval_loss_sum += float(per_image.double().sum().item())
        self._eval_loss_n += n
        loss = self._eval_loss_sum / self._eval_loss_n
        reg = self.l2_penalty()
        if reg is not None:
            loss += float(reg.item())
        res = {"loss": loss}
        if self._metric_names:
            totals = self.evaluation_totals(self._eval_acc, state)
            res.update({k: mean_metric(*totals[k]) for k in self._metric_names})
        return res

    def _evaluation_output(self, res, return_dict):
        if return_dict:
            return res
        return res["loss"] if not self._metric_names else [res[k] for k in self.metrics_names]

    def test_on_batch(self, x, y, sample_weight=None, reset_metrics=True, return_dict=False):
        """Keras Model.test_on_batch: the compiled loss (sample-weighted; + the l2 term when l2_reg is set) and the compiled metrics
        (unweighted) of one batch under the inference-mode forward -- a scalar, or [loss, m1, ...] in metrics_names order as
        train_on_batch returns them; return_dict: {"loss": ..., name: ...}. reset_metrics=False continues the Means of the
        calls before. Nothing of the model changes: no gradient, no optimizer state, no moving statistic, and not the metric
        state of the running training epoch (the forward refreshes the folded BatchNorm coefficients at the tail of `packed`
        after a weight change, exactly as predict_on_batch does)."""
        self._require_trainable("test_on_batch")
        res = self._evaluate_chunks(x, y, sample_weight, max(1, int(x.shape[0])), reset_metrics)
        return self._evaluation_output(res, return_dict)

    def evaluate(self, x, y, batch_size=32, sample_weight=None, return_dict=False):
        """Keras Model.evaluate on arrays: test_on_batch's computation in chunks of batch_size. The loss is the Mean over the batches
        weighted by batch size (= the mean over the images of w_b * L_b; the cross-entropy: over all pixels), the metrics follow
        the accumulator semantics of compile()'s docstring over the chunks."""
        self._require_trainable("evaluate")
        res = self._evaluate_chunks(x, y, sample_weight, 32 if batch_size is None else int(batch_size), True)
        return self._evaluation_output(res, return_dict)

    def fit(self, data, steps_per_epoch, epochs=1, callbacks=None, initial_epoch=0, verbose=0, **kwargs):
        """Minimal Model.fit over an iterator of (x, y, w) batches (trainer.py:246-257). The compiled metrics run over the whole
        epoch (reset at its start); `verbose` reports them beside the loss."""
        self._require_trainable("fit")
        it = iter(data)
        history = []
        for ep in range(initial_epoch, epochs):
            tot = 0.0
            self.reset_metrics()
            for _ in range(steps_per_epoch):
                x, y, w = next(it)
                tot += self._batch_loss(x, y, w)
            history.append(tot / steps_per_epoch)
            if verbose:
                self.logger("epoch %d: loss %.5f" % (ep + 1, history[-1])
                            + "".join(" - %s: %.5f" % kv for kv in self.metrics_result().items()))
            if self.stop_training:
                break
        return history

    def log(self):
        self.logger("UNet Model Summary\n------------------")
        self.logger("Image rows:        %i" % self.img_shape[0])
        self.logger("Image cols:        %i" % self.img_shape[1])
        self.logger("Image channels:    %i" % self.img_shape[2])
        self.logger("N classes:         %i" % self.n_classes)
        self.logger("CF factor:         %.3f" % self.cf ** 2)
        self.logger("Depth:             %i" % self.depth)
        self.logger("l2 reg:            %s" % self.l2_reg)
        self.logger("Padding:           %s" % self.padding)
        self.logger("Conv activation:   %s" % self.activation)
        self.logger("Out activation:    %s" % self.out_activation)
        self.logger("Receptive field:   %s" % self.receptive_field)
        self.logger("N params:          %i" % self.count_params())
        self.logger("Compute dtype:     %s (MI355X / gfx950 HIP kernels)" % str(self.dtype))
        self.logger("Crop:              None")
