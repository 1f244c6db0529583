"""
The optimizers of UNet.compile, host side (no GPU): the NumPy restatement tests/optimizer_ref.py against known answers derived by
hand from the update rules (the scalar problem loss = p^2 / 2, so g = p), its f32 form against its f64 form, and the compile /
C-ABI surface (UNet.compile, mpu_optimizer_num_slots, the header against the binding).
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimizer_ref as OR                                                              # noqa: E402

quiet = lambda *a, **k: None


def _run(cfg, p0, steps, grads=None):
    """p after each of `steps` steps of loss = p^2 / 2 (or of the given gradient sequence), f64; also the slots after each."""
    p, slots = np.float64(p0), [np.float64(0)] * OR.num_slots(cfg)
    ps, ss = [], []
    for t in range(1, steps + 1):
        p, slots = OR.step64(cfg, p, p if grads is None else grads[t - 1], slots, t)
        ps.append(float(p)); ss.append([float(s) for s in slots])
    return ps, ss


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_kat_sgd():
    # p -= 0.1 * p
    np.testing.assert_allclose(_run(OR.config("SGD", lr=0.1), 1.0, 1)[0], [0.9], rtol=1e-15)
    # a = -0.1, p = 0.9; a = -0.09 - 0.09 = -0.18, p = 0.72
    np.testing.assert_allclose(_run(OR.config("SGD", lr=0.1, momentum=0.9), 1.0, 2)[0], [0.9, 0.72], rtol=1e-15)
    # a = -0.1, p = 1 - 0.09 - 0.1 = 0.81; a = -0.09 - 0.081 = -0.171, p = 0.81 - 0.1539 - 0.081 = 0.5751
    np.testing.assert_allclose(_run(OR.config("SGD", lr=0.1, momentum=0.9, nesterov=True), 1.0, 2)[0], [0.81, 0.5751], rtol=1e-14)
    # Nesterov without momentum is the plain rule, and has no slot
    cfg = OR.config("SGD", lr=0.1, nesterov=True)
    assert OR.num_slots(cfg) == 0 and _run(cfg, 1.0, 1)[0] == _run(OR.config("SGD", lr=0.1), 1.0, 1)[0]


def test_kat_rmsprop_and_its_two_epsilon_placements():
    # ms = 0.1 * 100 = 10. No momentum: 10 - 0.1 * 10 / (sqrt(10) + 1e-7); momentum: mom = 1 / sqrt(10 + 1e-7), p = 10 - mom
    plain = _run(OR.config("RMSprop", lr=0.1), 10.0, 1)[0][0]
    mom = _run(OR.config("RMSprop", lr=0.1, momentum=0.9), 10.0, 1)[0][0]
    assert abs(plain - 9.683772243983162) <= 1e-15 * 10 and plain == 10 - 1 / (np.sqrt(10.0) + 1e-7)
    assert abs(mom - 9.683772235564302) <= 1e-15 * 10 and mom == 10 - 1 / np.sqrt(10.0 + 1e-7)
    assert 5e-9 < plain - mom < 1e-8                       # the ninth digit: what keeps the two placements apart
    # centered: mg = 1, d = 10 - 1 = 9: 10 - 1 / (3 + 1e-7)
    cen = _run(OR.config("RMSprop", lr=0.1, centered=True), 10.0, 1)[0][0]
    assert abs(cen - 9.666666677777778) <= 1e-15 * 10 and cen == 10 - 1 / (3.0 + 1e-7)
    # centered with momentum: mom = 1 / sqrt(9 + 1e-7); slots ms, mom, mg
    ps, ss = _run(OR.config("RMSprop", lr=0.1, momentum=0.9, centered=True), 10.0, 1)
    np.testing.assert_allclose(ss[0], [10.0, 1 / np.sqrt(9.0 + 1e-7), 1.0], rtol=1e-15)
    assert ps[0] == 10 - 1 / np.sqrt(9.0 + 1e-7)


def test_kat_adamax():
    # t = 1: m = 1, u = 10, p = 10 - (0.1 / 0.1) * 1 / (10 + 1e-7)
    ps, ss = _run(OR.config("Adamax", lr=0.1), 10.0, 3)
    np.testing.assert_allclose(ps, [9.900000001, 9.800426744523467, 9.701297121392873], rtol=1e-15)
    assert ps[0] == 10 - 1 / (10 + 1e-7)
    # t = 2 by hand: m = 1 + (9.900000001 - 1) * 0.1, u = max(9.99, 9.900000001) = 9.99, step (0.1 / 0.19) * m / (u + 1e-7)
    m2 = 1 + (ps[0] - 1) * (1 - 0.9)
    np.testing.assert_allclose(ss[1], [m2, 9.99], rtol=1e-15)
    np.testing.assert_allclose(ps[1], ps[0] - (0.1 / (1 - 0.81)) * m2 / (9.99 + 1e-7), rtol=1e-15)


def test_kat_amsgrad_and_adam():
    # Adam, t = 1: m = 0.1 g, v = 0.001 g^2, alpha = lr sqrt(0.001) / 0.1: the step is lr * g / (|g| + eps sqrt(1000)...) ~ lr
    ps, _ = _run(OR.config("Adam", lr=0.1), 10.0, 1)
    np.testing.assert_allclose(ps[0], 10 - (0.1 * np.sqrt(0.001) / 0.1) * 1.0 / (np.sqrt(0.1) + 1e-7), rtol=1e-15)
    # AMSGrad's first step is Adam's (vhat = max(0, v) = v)
    assert _run(OR.config("Adam", lr=0.1, amsgrad=True), 10.0, 1)[0] == ps
    # gradients 10, 0, 0: v falls, vhat keeps its first value
    _, ss = _run(OR.config("Adam", lr=0.1, amsgrad=True), 10.0, 3, grads=[10.0, 0.0, 0.0])
    v, vhat = [s[1] for s in ss], [s[2] for s in ss]
    np.testing.assert_allclose(v, [0.1, 0.1 * 0.999, 0.1 * 0.999 ** 2], rtol=1e-14)
    assert vhat == [vhat[0]] * 3 and vhat[0] == v[0] and v[2] < v[1] < v[0]


def test_learning_rate_decay():
    np.testing.assert_allclose([OR.decayed_lr(0.1, 0.5, t) for t in (1, 2, 3)], [0.1, 0.1 / 1.5, 0.05], rtol=1e-15)
    assert OR.decayed_lr(0.1, 0.0, 7) == 0.1                                   # bit for bit: no division by one
    # SGD(0.1, decay 0.5) on g = p: 1 -> 0.9 -> 0.9 (1 - 0.0666...) -> ... (1 - 0.05)
    np.testing.assert_allclose(_run(OR.config("SGD", lr=0.1, decay=0.5), 1.0, 3)[0],
                               [0.9, 0.9 * (1 - 0.1 / 1.5), 0.9 * (1 - 0.1 / 1.5) * 0.95], rtol=1e-15)
    # decay reaches every rule through its step constant
    for cfg in OR.ALL_CONFIGS:
        name, kw = cfg
        undecayed = OR.step_constant((name, dict(kw, decay=0.0)), 3)
        np.testing.assert_allclose(OR.step_constant(cfg, 3), undecayed / (1 + kw["decay"] * 2), rtol=1e-15)


@pytest.mark.parametrize("cfg", OR.ALL_CONFIGS, ids=lambda c: c[0] + "".join("-" + k for k in ("momentum", "nesterov", "centered", "amsgrad") if c[1].get(k)))
def test_f32_form_follows_the_f64_form(cfg):
    """The f32 restatement (the kernel's operation order) against the f64 one over 5 steps of random gradients, a zero-gradient
    step among them: a few f32 ulps of the parameters."""
    rng = np.random.RandomState(3)
    n = 1000
    p64 = rng.randn(n); p32 = p64.astype(np.float32); p64 = p32.astype(np.float64)
    s64 = [np.zeros(n) for _ in range(OR.num_slots(cfg))]
    s32 = [np.zeros(n, np.float32) for _ in s64]
    for t in range(1, 6):
        g = (rng.randn(n) * (t != 3)).astype(np.float32)
        p64, s64 = OR.step64(cfg, p64, g, s64, t)
        p32, s32 = OR.step32(cfg, p32, g, s32, t)
        assert all(a.dtype == np.float32 for a in [p32] + s32)
    assert np.isfinite(p32).all()
    assert np.abs(p32 - p64).max() <= 16 * np.finfo(np.float32).eps * max(1.0, np.abs(p64).max())
    # the slots: 1 - beta_2 is formed in f32 from the rounded beta_2 (as TF's kernels do), so a moment carries the relative error
    # of that difference, up to 2^-24 / (1 - 0.999) = 6e-5; twice that bounds every slot here
    for a, b in zip(s32, s64):
        assert np.abs(a - b).max() <= 2 * 2.0 ** -24 / 1e-3 * max(1e-3, np.abs(b).max())


# ---- compile surface (device="cpu": validation only; the library loads without a GPU) ----------------------------------------------
def _model():
    from multiplanarunet_amd.unet import UNet
    return UNet(n_classes=3, dim=32, depth=2, device="cpu", logger=quiet, seed=0)


SLOT_CASES = [("SGD", {}, 0), ("SGD", {"momentum": 0.9}, 1), ("RMSprop", {}, 1), ("RMSprop", {"momentum": 0.9}, 2),
              ("RMSprop", {"momentum": 0.9, "centered": True}, 3), ("Adam", {}, 2), ("Adam", {"amsgrad": True}, 3), ("Adamax", {}, 2)]


@pytest.mark.parametrize("name,kw,n", SLOT_CASES)
def test_compile_accepts_each_optimizer_and_counts_its_slots(name, kw, n):
    m = _model()
    assert m.compile(name, optimizer_kwargs=kw) is m                   # "SGD" raised NotImplementedError before
    assert m.optimizer_name == name and m._optimizer_config()[1] == n == OR.num_slots(OR.config(name, **kw))
    assert m.compile(name.lower(), optimizer_kwargs=dict(kw, name="opt")).optimizer_name == name
    assert "name" not in m.optimizer_kwargs
    assert m._plain_adam() == (name == "Adam" and not kw)
    assert m.optimizer_description().startswith(name + "(lr=")


def test_compile_flags_reach_the_library_config():
    from multiplanarunet_amd import _lib
    m = _model()
    cfg, n = m.compile("SGD", optimizer_kwargs={"lr": 0.01, "momentum": 0.9, "nesterov": True, "decay": 1e-3})._optimizer_config()
    assert (cfg.kind, cfg.flags, cfg.lr, cfg.momentum, cfg.decay, n) == (_lib.MPU_OPT_SGD, _lib.MPU_OPT_NESTEROV, 0.01, 0.9, 1e-3, 1)
    cfg, n = m.compile("RMSprop", optimizer_kwargs={"centered": True, "rho": 0.8})._optimizer_config()
    assert (cfg.kind, cfg.flags, cfg.rho, cfg.epsilon, n) == (_lib.MPU_OPT_RMSPROP, _lib.MPU_OPT_CENTERED, 0.8, 1e-7, 2)
    cfg, n = m.compile("Adam", optimizer_kwargs={"amsgrad": True})._optimizer_config()
    assert (cfg.kind, cfg.flags, n) == (_lib.MPU_OPT_ADAM, _lib.MPU_OPT_AMSGRAD, 3)
    cfg, n = m.compile("Adamax")._optimizer_config()
    assert (cfg.kind, cfg.flags, cfg.beta1, cfg.beta2, n) == (_lib.MPU_OPT_ADAMAX, 0, 0.9, 0.999, 2)


def test_compile_defaults():
    m = _model()
    # Adam keeps the project YAML's values (UNet.__init__), with and without kwargs
    assert m.optimizer_name == "Adam" and m.optimizer_kwargs["lr"] == 5e-5 and m.optimizer_kwargs["epsilon"] == 1e-8
    m.compile("Adam")
    assert (m.optimizer_kwargs["lr"], m.optimizer_kwargs["beta_1"], m.optimizer_kwargs["beta_2"], m.optimizer_kwargs["epsilon"]) \
        == (5e-5, 0.9, 0.999, 1e-8)
    m.compile("Adam", optimizer_kwargs={"learning_rate": 1e-3})         # the alias; the other keys stay
    assert m.optimizer_kwargs["lr"] == 1e-3 and m.optimizer_kwargs["epsilon"] == 1e-8 and "learning_rate" not in m.optimizer_kwargs
    # a new optimizer takes the Keras defaults for what optimizer_kwargs omits
    for name, want in (("SGD", dict(lr=0.01, momentum=0.0, nesterov=False)),
                       ("RMSprop", dict(lr=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False)),
                       ("Adamax", dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7))):
        m.compile(name)
        assert {k: m.optimizer_kwargs[k] for k in want} == want and m.optimizer_kwargs["decay"] == 0.0
    m.compile("SGD", optimizer_kwargs={"lr": 0.5})
    assert m.optimizer_kwargs["lr"] == 0.5 and m.optimizer_kwargs["momentum"] == 0.0
    # ... and Adam after another optimizer is the default Adam again, not what was compiled before
    m.compile("Adam")
    assert m.optimizer_kwargs["lr"] == 5e-5 and m._plain_adam()


def test_plain_adam_with_explicit_decay_zero_keeps_the_fused_tail():
    m = _model()
    m.compile("Adam", optimizer_kwargs={"lr": 1e-3, "decay": 0.0, "amsgrad": False, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-8})
    assert m._plain_adam()
    assert not _model().compile("Adam", optimizer_kwargs={"decay": 1e-4})._plain_adam()
    assert not _model().compile("Adam", optimizer_kwargs={"amsgrad": True})._plain_adam()


def test_second_compile_with_another_optimizer_drops_the_state():
    import torch
    m = _model()
    m._ensure_slots()
    m.iterations = 7
    assert len(m._slots) == 2 and m._adam_m is m._slots[0] and m._adam_v is m._slots[1]
    m.compile("Adam", optimizer_kwargs={"lr": 1e-3})                    # the same optimizer: the state stays (ReduceLROnPlateau & co.)
    assert m.iterations == 7 and m._slots is not None
    m.compile("SGD", optimizer_kwargs={"momentum": 0.9})
    assert m.iterations == 0 and m._slots is None and m._adam_m is None
    m._ensure_slots()
    assert len(m._slots) == 1 and m._slots[0].shape == m.params.shape and not torch.any(m._slots[0])
    m.iterations = 3
    m.compile("SGD")                                                    # momentum stays 0.9: compile updates, as for Adam
    assert m.iterations == 3 and len(m._slots) == 1
    m.compile("SGD", optimizer_kwargs={"momentum": 0.0})                # another variant: other slots
    assert m.iterations == 0 and m._slots is None


def test_compile_rejects_what_is_not_built():
    for name in ("Nadam", "Adagrad", "Adadelta", "Ftrl", "LAMB", "RectifiedAdam", "AdamW", "SGDW", "LazyAdam"):
        with pytest.raises(NotImplementedError, match="Adam.*SGD.*RMSprop.*Adamax"):
            _model().compile(name)
    for k in ("clipnorm", "clipvalue"):
        with pytest.raises(NotImplementedError, match="Adam.*SGD.*RMSprop.*Adamax"):
            _model().compile("SGD", optimizer_kwargs={k: 1.0})
    for name, kw in (("SGD", {"beta_1": 0.9}), ("Adam", {"momentum": 0.9}), ("RMSprop", {"nesterov": True}), ("Adamax", {"amsgrad": True}),
                     ("Adam", {"learning_rat": 1e-3})):
        with pytest.raises(TypeError, match="unexpected keyword argument"):
            _model().compile(name, optimizer_kwargs=kw)
    for name, kw in (("SGD", {"momentum": 1.5}), ("SGD", {"momentum": -0.1}), ("RMSprop", {"momentum": 2.0})):   # as the Keras constructors
        with pytest.raises(ValueError, match="momentum"):
            _model().compile(name, optimizer_kwargs=kw)
    m = _model()
    with pytest.raises(ValueError):
        m.compile("SGD", optimizer_kwargs={"momentum": 1.5})
    assert m.optimizer_name == "Adam" and m.optimizer_kwargs["lr"] == 5e-5        # a refused compile changes nothing


def test_capi_num_slots_and_validation():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.OptimizerConfig) == 2 * 4 + 7 * 8

    def cfg(kind, flags=0, **kw):
        c = _lib.OptimizerConfig()
        c.kind, c.flags, c.lr, c.beta1, c.beta2, c.epsilon, c.rho = kind, flags, 0.01, 0.9, 0.999, 1e-7, 0.9
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    S, R, A, X = _lib.MPU_OPT_SGD, _lib.MPU_OPT_RMSPROP, _lib.MPU_OPT_ADAM, _lib.MPU_OPT_ADAMAX
    want = [(cfg(S), 0), (cfg(S, momentum=0.9), 1), (cfg(R), 1), (cfg(R, momentum=0.9), 2),
            (cfg(R, _lib.MPU_OPT_CENTERED, momentum=0.9), 3), (cfg(A), 2), (cfg(A, _lib.MPU_OPT_AMSGRAD), 3), (cfg(X), 2),
            (cfg(S, _lib.MPU_OPT_NESTEROV, momentum=0.9), 1), (cfg(S, _lib.MPU_OPT_NESTEROV), 0), (cfg(R, _lib.MPU_OPT_CENTERED), 2),
            (cfg(A, decay=1e-4), 2)]
    assert [lib.mpu_optimizer_num_slots(C.byref(c)) for c, _ in want] == [n for _, n in want]
    for bad in (cfg(4), cfg(-1), cfg(S, _lib.MPU_OPT_AMSGRAD), cfg(A, _lib.MPU_OPT_NESTEROV), cfg(X, _lib.MPU_OPT_CENTERED), cfg(A, 8),
                cfg(S, momentum=1.5), cfg(R, rho=-0.1), cfg(A, beta1=1.0), cfg(A, lr=-1.0), cfg(S, decay=-1.0),
                cfg(A, epsilon=float("nan"))):
        assert lib.mpu_optimizer_num_slots(C.byref(bad)) == -1                    # MPU_EINVAL
        assert b"mpu_optimizer_config" in lib.mpu_last_error()
    assert lib.mpu_optimizer_num_slots(None) == -1
    # the step entry points refuse an invalid configuration and a missing slot before they touch the device
    slots = (C.c_void_p * 3)()
    one = C.c_void_p(16)
    assert lib.mpu_optimizer_step(C.byref(cfg(S, momentum=0.9)), one, one, slots, 4, 1, None, None) == -1
    assert b"slot" in lib.mpu_last_error()
    assert lib.mpu_optimizer_step(C.byref(cfg(4)), one, one, slots, 4, 1, None, None) == -1
    assert lib.mpu_optimizer_step(C.byref(cfg(S)), one, one, slots, 4, 0, None, None) == -1   # neither a counter nor a step number
    assert lib.mpu_abi_version() == _lib.ABI_VERSION == 2                         # the ABI change is additive


def _exported_functions(path):
    """Names of the functions a 64-bit little-endian ELF shared object defines in its dynamic symbol table (.dynsym)."""
    import struct
    blob = open(path, "rb").read()
    assert blob[:6] == b"\x7fELF\x02\x01", "not a 64-bit little-endian ELF file"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 11:                                                         # SHT_DYNSYM
            continue
        stroff = sections[link][4]
        for e in range(off, off + size, entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", blob, e)
            if st_shndx and (st_info & 15) == 2 and (st_info >> 4) in (1, 2):      # defined here, a function, global or weak
                names.add(blob[stroff + st_name:blob.index(b"\0", stroff + st_name)].decode())
    return names


def test_header_prototypes_equal_the_exported_symbols():
    """The functions include/mpunet_hip.h declares are exactly the mpu_* functions libmpunet_hip.so exports (its dynamic symbol
    table), and exactly what _lib._SIGS binds; mpu_build_hash alone, generated by the build, is exported and bound undeclared."""
    from multiplanarunet_amd import _lib
    _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mpunet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    declared = set(re.findall(r"\b(mpu_[a-z0-9_]+)\s*\(", text))
    bound = set(_lib.declared_symbols())
    exported = {n for n in _exported_functions(_lib.LIB_PATH) if n.startswith("mpu_")}
    assert {"mpu_optimizer_num_slots", "mpu_optimizer_step", "mpu_unet_optimizer_pack"} <= declared
    assert declared - bound == set() and bound - declared <= {"mpu_build_hash"}
    assert declared - exported == set() and exported - declared <= {"mpu_build_hash"}


def test_mp_train_passes_the_optimizer_through():
    """cli/train.py hands fit.optimizer / fit.optimizer_kwargs to compile unchanged; the default project still names plain Adam."""
    from multiplanarunet_amd.cli.common import DEFAULT_HPARAMS
    fit = DEFAULT_HPARAMS["fit"]
    m = _model().compile(fit["optimizer"], fit["loss"], fit.get("metrics"), optimizer_kwargs=fit["optimizer_kwargs"])
    assert m._plain_adam() and m.optimizer_kwargs["lr"] == 5e-5
    m = _model().compile("SGD", fit["loss"], optimizer_kwargs={"lr": 0.01, "momentum": 0.9, "nesterov": True, "decay": 1.0e-3})
    assert m.optimizer_description() == "SGD(lr=0.01, momentum=0.9, nesterov=True, decay=0.001)"
