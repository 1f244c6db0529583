"""
The update rules of tf.keras.optimizers (TF 2.3) that UNet.compile accepts -- SGD, RMSprop, Adam / AMSGrad, Adamax, each with
learning-rate decay -- restated in NumPy, independently of csrc/optimizer.hip. Two forms of the same rules:

  step64   f64 throughout: the known answers of tests/test_optimizers_host.py and the reference of the end-to-end GPU test;
  step32   f32 per element in the kernel's operation order (every NumPy f32 operation rounds once, as the device's does with
           FMA contraction off); the scalars are formed in f64 and rounded to f32 once.

TensorFlow is not available to pin these against: they restate OptimizerV2._decayed_lr and the ResourceApply* kernels from their
published sources, as oracle/unet_ref.py's Adam does. Inferred: RMSprop's epsilon sits OUTSIDE the root without momentum (the
Python dense path) and INSIDE it with momentum (the fused ApplyRMSProp / ApplyCenteredRMSProp kernels).

A configuration is (name, kw): the Keras class name and its keywords, defaults filled by `config`. Slots, in the library's
order: Adam m, v[, vhat]; Adamax m, u; SGD [a]; RMSprop ms[, mom][, mg]. k = t - 1 steps were applied before step t.
"""
import math

import numpy as np

DEFAULTS = {
    "Adam": dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, decay=0.0),
    "SGD": dict(lr=0.01, momentum=0.0, nesterov=False, decay=0.0),
    "RMSprop": dict(lr=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, decay=0.0),
    "Adamax": dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0),
}


def config(name, **kw):
    out = dict(DEFAULTS[name])
    assert all(k in out for k in kw), kw
    out.update(kw)
    return name, out


def num_slots(cfg):
    name, kw = cfg
    if name == "Adam":
        return 3 if kw["amsgrad"] else 2
    if name == "Adamax":
        return 2
    if name == "SGD":
        return 1 if kw["momentum"] > 0 else 0
    return 1 + (1 if kw["momentum"] > 0 else 0) + (1 if kw["centered"] else 0)


def decayed_lr(lr, decay, t):
    """OptimizerV2._decayed_lr at step t (1-based): lr / (1 + decay * (t - 1)); decay == 0: lr itself."""
    return lr if decay == 0 else lr / (1.0 + decay * (t - 1))


def step_constant(cfg, t):
    """The one scalar of a rule that moves with the step, in f64: Adam's alpha_t, Adamax' lr_t / (1 - beta_1^t), else lr_t."""
    name, kw = cfg
    lr_t = decayed_lr(kw["lr"], kw["decay"], t)
    if name == "Adam":
        return lr_t * math.sqrt(1.0 - math.pow(kw["beta_2"], t)) / (1.0 - math.pow(kw["beta_1"], t))
    if name == "Adamax":
        return lr_t / (1.0 - math.pow(kw["beta_1"], t))
    return lr_t


def step64(cfg, p, g, slots, t):
    """One step in f64. p, g: arrays; slots: list of num_slots(cfg) arrays. Returns (p, slots), new arrays."""
    name, kw = cfg
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    s = [np.asarray(x, np.float64) for x in slots]
    assert len(s) == num_slots(cfg)
    lr_t = decayed_lr(kw["lr"], kw["decay"], t)
    if name == "SGD":
        if not kw["momentum"] > 0:
            return p - lr_t * g, []
        a = s[0] * kw["momentum"] - lr_t * g
        return (p + a * kw["momentum"] - lr_t * g if kw["nesterov"] else p + a), [a]
    if name == "RMSprop":
        ms = s[0] + (g * g - s[0]) * (1 - kw["rho"])
        out = [ms]
        d = ms
        if kw["centered"]:
            mg = s[-1] + (g - s[-1]) * (1 - kw["rho"])
            d = ms - mg * mg
        if kw["momentum"] > 0:
            mom = s[1] * kw["momentum"] + lr_t * g / np.sqrt(d + kw["epsilon"])
            out.append(mom)
            p = p - mom
        else:
            p = p - lr_t * g / (np.sqrt(d) + kw["epsilon"])
        if kw["centered"]:
            out.append(mg)
        return p, out
    if name == "Adam":
        m = s[0] + (g - s[0]) * (1 - kw["beta_1"])
        v = s[1] + (g * g - s[1]) * (1 - kw["beta_2"])
        alpha = step_constant(cfg, t)
        if kw["amsgrad"]:
            vhat = np.maximum(s[2], v)
            return p - m * alpha / (np.sqrt(vhat) + kw["epsilon"]), [m, v, vhat]
        return p - m * alpha / (np.sqrt(v) + kw["epsilon"]), [m, v]
    assert name == "Adamax"
    m = s[0] + (g - s[0]) * (1 - kw["beta_1"])
    u = np.maximum(kw["beta_2"] * s[1], np.abs(g))
    return p - step_constant(cfg, t) * m / (u + kw["epsilon"]), [m, u]


def step32(cfg, p, g, slots, t):
    """One step with f32 arithmetic per element, operation by operation as the device unit performs it."""
    f = np.float32
    name, kw = cfg
    p, g = np.asarray(p, f), np.asarray(g, f)
    s = [np.asarray(x, f) for x in slots]
    assert len(s) == num_slots(cfg)
    c0 = f(step_constant(cfg, t))
    one = f(1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        if name == "SGD":
            mom = f(kw["momentum"])
            sg = c0 * g
            if not kw["momentum"] > 0:
                return p - sg, []
            a = s[0] * mom - sg
            return (p + (a * mom - sg) if kw["nesterov"] else p + a), [a]
        if name == "RMSprop":
            rho, mom, eps = f(kw["rho"]), f(kw["momentum"]), f(kw["epsilon"])
            o = one - rho
            g2 = g * g
            ms = s[0] + (g2 - s[0]) * o
            out = [ms]
            d = ms
            if kw["centered"]:
                mg = s[-1] + (g - s[-1]) * o
                d = ms - mg * mg
            num = c0 * g
            if kw["momentum"] > 0:
                mm = s[1] * mom + num / np.sqrt(d + eps)
                out.append(mm)
                p = p - mm
            else:
                p = p - num / (np.sqrt(d) + eps)
            if kw["centered"]:
                out.append(mg)
            return p, out
        b1, b2, eps = f(kw["beta_1"]), f(kw["beta_2"]), f(kw["epsilon"])
        m = s[0] + (g - s[0]) * (one - b1)
        if name == "Adam":
            g2 = g * g
            v = s[1] + (g2 - s[1]) * (one - b2)
            if kw["amsgrad"]:
                vhat = np.maximum(s[2], v)
                return p - (m * c0) / (np.sqrt(vhat) + eps), [m, v, vhat]
            return p - (m * c0) / (np.sqrt(v) + eps), [m, v]
        assert name == "Adamax"
        u = np.maximum(b2 * s[1], np.abs(g))
        return p - (c0 * m) / (u + eps), [m, u]


# every rule and flag combination (the GPU tests run all of them), each with decay != 0
ALL_CONFIGS = [
    config("SGD", lr=0.05, decay=0.25),
    config("SGD", lr=0.05, momentum=0.9, decay=0.25),
    config("SGD", lr=0.05, momentum=0.9, nesterov=True, decay=0.25),
    config("RMSprop", lr=0.01, decay=0.25),
    config("RMSprop", lr=0.01, momentum=0.8, decay=0.25),
    config("RMSprop", lr=0.01, centered=True, decay=0.25),
    config("RMSprop", lr=0.01, momentum=0.8, centered=True, rho=0.95, decay=0.25),
    config("Adam", lr=0.01, epsilon=1e-8, decay=0.25),
    config("Adam", lr=0.01, amsgrad=True, decay=0.25),
    config("Adamax", lr=0.01, decay=0.25),
]
