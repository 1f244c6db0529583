"""
Host side of the cross-entropy from logits (UNet.compile(loss_kwargs={"from_logits": True}) on out_activation="linear",
MPU_LOSS_SPARSE_CE_LOGITS, mpu_eval_loss_logits), no GPU: the compile rules, the C-ABI surface, `mp train`'s up-front
refusals and the restatement tests/logits_ref.py against hand-computed known answers.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logits_ref as LG                                                                # noqa: E402

quiet = lambda *a, **k: None
CE = "SparseCategoricalCrossentropy"


def _model(K=3, out_activation="linear"):
    from multiplanarunet_amd.unet import UNet
    return UNet(n_classes=K, dim=32, depth=2, out_activation=out_activation, device="cpu", logger=quiet, seed=0)


def _plan(m):
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    return lib.mpu_unet_workspace_bytes(m._h, 2), lib.mpu_unet_workspace_loss_mean_offset(m._h, 2)


# ---- 1. the compile rules ------------------------------------------------------------------------------------------------------
def test_from_logits_is_honoured_on_a_linear_model():
    m = _model()
    assert m.from_logits is False
    assert m.compile("Adam", CE, ["sparse_categorical_accuracy"], loss_kwargs={"from_logits": True}) is m
    assert m.from_logits is True
    assert m.loss_name == CE and not m._per_image_loss
    assert _plan(m) == _plan(_model())                                   # no table, no scratch: the plan of a fresh model
    for loss in ([CE], type(CE, (), {})()):                              # a one-entry list, an object whose class carries the name
        m = _model()
        m.compile("Adam", loss, loss_kwargs={"from_logits": True})
        assert m.from_logits is True and m.loss_name == CE


def test_name_is_dropped_and_false_or_absent_keeps_todays_behaviour():
    for act in ("linear", "softmax"):
        for kw in (None, {}, {"from_logits": False}, {"name": "ce"}, {"name": "ce", "from_logits": False}):
            m = _model(out_activation=act)
            m.compile("Adam", CE, loss_kwargs=kw)                        # nothing new is refused at compile time
            assert m.from_logits is False and not m._per_image_loss and m.loss_name == CE
            assert _plan(m) == _plan(_model(out_activation=act))
    m = _model()
    m.compile("Adam", CE, loss_kwargs={"name": "ce", "from_logits": True})
    assert m.from_logits is True


def test_reduction_raises_the_per_image_losses_message():
    with pytest.raises(TypeError) as e:
        _model().compile("Adam", CE, loss_kwargs={"reduction": "none"})
    with pytest.raises(TypeError) as e_dice:
        _model(out_activation="softmax").compile("Adam", "SparseDiceLoss", loss_kwargs={"reduction": "none"})
    assert str(e.value) == str(e_dice.value).replace("SparseDiceLoss", CE)
    assert "multiple values for keyword argument 'reduction'" in str(e.value)


def test_an_unknown_key_raises_type_error_as_the_keras_constructor_would():
    for kw in ({"from_logit": True}, {"from_logits": True, "label_smoothing": 0.1}, {"axis": -1}):
        with pytest.raises(TypeError, match="got an unexpected keyword argument"):
            _model().compile("Adam", CE, loss_kwargs=kw)


def test_from_logits_on_a_softmax_model_is_refused_and_names_the_linear_output():
    with pytest.raises(ValueError, match=r'out_activation="linear"'):
        _model(out_activation="softmax").compile("Adam", CE, loss_kwargs={"from_logits": True})


def test_a_refused_compile_changes_nothing_on_the_model():
    m = _model(out_activation="softmax")
    m.compile("SGD", CE, ["sparse_categorical_accuracy"], optimizer_kwargs={"lr": 0.01, "momentum": 0.9})
    m.iterations = 7
    before = (m.optimizer_name, dict(m.optimizer_kwargs), m.iterations, list(m.metrics_names), m.loss_name, m.from_logits, _plan(m))
    for kw, exc in (({"from_logits": True}, ValueError), ({"reduction": "none"}, TypeError), ({"bogus": 1}, TypeError)):
        with pytest.raises(exc):
            m.compile("Adam", CE, ["sparse_fg_recall"], optimizer_kwargs={"lr": 1.0}, loss_kwargs=kw)
        assert before == (m.optimizer_name, dict(m.optimizer_kwargs), m.iterations, list(m.metrics_names), m.loss_name,
                          m.from_logits, _plan(m))
    lin = _model()
    lin.compile("Adam", CE, loss_kwargs={"from_logits": True})
    with pytest.raises(TypeError):
        lin.compile("Adam", CE, loss_kwargs={"bogus": 1})
    assert lin.from_logits is True                                       # the refused compile did not detach the loss either
    with pytest.raises(ValueError):                                      # the five per-image losses on logits stay refused
        lin.compile("Adam", "SparseDiceLoss")
    assert lin.from_logits is True and lin.loss_name == CE


def test_compiling_the_plain_cross_entropy_afterwards_restores_the_default():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    fresh = _plan(_model())
    m = _model()
    m.compile("Adam", CE, loss_kwargs={"from_logits": True})
    m.compile("Adam", CE)
    assert m.from_logits is False and not m._per_image_loss and m.loss_name == CE
    assert _plan(m) == fresh
    # ... and the handle refuses to train again, word for word (the check comes before any argument is looked at)
    one = C.c_void_p(8)
    assert lib.mpu_unet_backward(m._h, 1, one, one, one, one, one, one, one, None, None) == -1
    assert lib.mpu_last_error() == b"mpu_unet_backward: training needs out_activation='softmax'"


# ---- 2. the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_capi_the_new_kind_on_linear_softmax_and_null_handles():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    assert lib.mpu_abi_version() == _lib.ABI_VERSION == 2
    assert C.sizeof(_lib.LossConfig) == 68
    assert _lib.MPU_LOSS_SPARSE_CE_LOGITS == 6
    cfg = _lib.LossConfig()
    cfg.kind = _lib.MPU_LOSS_SPARSE_CE_LOGITS
    lin, soft = _model(), _model(out_activation="softmax")
    assert lib.mpu_unet_set_loss(lin._h, C.byref(cfg)) == 0
    assert lib.mpu_unet_set_loss(soft._h, C.byref(cfg)) == -1                      # MPU_EINVAL
    msg = lib.mpu_last_error()
    assert b"mpu_unet_set_loss" in msg and b"softmax" in msg
    assert lib.mpu_unet_set_loss(None, C.byref(cfg)) == -1 and b"mpu_unet_set_loss" in lib.mpu_last_error()
    for kind in range(1, 6):                                                       # the five per-image losses on a linear handle
        bad = _lib.LossConfig()
        bad.kind, bad.smooth = kind, 1.0
        assert lib.mpu_unet_set_loss(lin._h, C.byref(bad)) == -1 and b"softmax" in lib.mpu_last_error()
    bad = _lib.LossConfig()
    bad.kind = 7
    assert lib.mpu_unet_set_loss(soft._h, C.byref(bad)) == -1 and b"unknown loss kind" in lib.mpu_last_error()
    assert lib.mpu_unet_set_loss(lin._h, C.byref(bad)) == -1 and b"mpu_unet_set_loss" in lib.mpu_last_error()
    # a linear handle WITHOUT the loss: the three backward entries refuse as they always did, word for word, before they use an
    # argument (with it attached they run: tests/test_gpu_logits_loss.py)
    one = C.c_void_p(8)
    other = _model()
    for name, args in (("mpu_unet_backward", (1, one, one, one, one, one, one, one, None, None)),
                       ("mpu_unet_backward_events", (1, one, one, one, one, one, one, one, None, None, 0, None)),
                       ("mpu_unet_backward_adam", (1, one, one, one, one, one, one, one, None, one, one, 1, None, 1e-3, .9, .999, 1e-8,
                                                   None))):
        assert getattr(lib, name)(other._h, *args) == -1
        assert lib.mpu_last_error() == name.encode() + b": training needs out_activation='softmax'"
    # above 8 classes: the existing guard and message
    wide = _model(K=9)
    assert lib.mpu_unet_set_loss(wide._h, C.byref(cfg)) != 0 and b"9..16 are inference-only" in lib.mpu_last_error()
    # the evaluation entry: its own argument checks; mpu_eval_loss keeps refusing kind 6
    assert lib.mpu_eval_loss_logits(None, one, None, 1, 16, 3, one, None, None, None) == -1
    assert b"mpu_eval_loss_logits" in lib.mpu_last_error()
    assert lib.mpu_eval_loss_logits(one, one, None, 1, 16, 9, one, None, None, None) != 0
    assert lib.mpu_eval_loss(C.byref(cfg), one, one, None, 1, 16, 3, one, None, None, None) == -1
    assert b"mpu_eval_loss_logits" in lib.mpu_last_error()


def test_header_exports_and_bindings_name_the_new_entry_point():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mpunet_hip.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert re.search(r"\bmpu_eval_loss_logits\s*\(", code) and re.search(r"MPU_LOSS_SPARSE_CE_LOGITS\s*=\s*6\b", code)
    assert "mpu_eval_loss_logits" in _lib.declared_symbols() and hasattr(lib, "mpu_eval_loss_logits")
    assert _lib._SIGS["mpu_eval_loss_logits"][1] == _lib._SIGS["mpu_eval_loss"][1][1:]      # mpu_eval_loss's, without the config


# ---- 3. `mp train` ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,kw,match", [("linear", "{}", r"fit\.loss_kwargs: \{from_logits: true\}"),
                                          ("linear", "{from_logits: false}", r"fit\.loss_kwargs: \{from_logits: true\}"),
                                          ("softmax", "{from_logits: true}", r'out_activation="linear"')])
def test_mp_train_refuses_up_front(tmp_path, act, kw, match):
    from multiplanarunet_amd.cli import train as T
    (tmp_path / "train_hparams.yaml").write_text(
        "build:\n  n_classes: 3\n  dim: 32\n  n_channels: 1\n  depth: 2\n  out_activation: %s\n  biased_output_layer: false\n\n"
        "fit:\n  batch_size: 2\n  real_space_span: 32.0\n  loss_kwargs: %s\n" % (act, kw))
    before = sorted(os.listdir(tmp_path))
    args = T.get_argparser().parse_args(["--project_dir", str(tmp_path), "--synthetic", "2", "--no_val", "--epochs", "1"])
    with pytest.raises(ValueError, match=match):
        T.run(args)
    assert not (tmp_path / "model").exists() and not (tmp_path / "logs").exists()
    assert sorted(os.listdir(tmp_path)) == before


def test_the_compile_error_is_the_one_mp_train_stops_with():
    from multiplanarunet_amd.cli.common import validate_output_loss, DEFAULT_HPARAMS
    hp = {k: dict(v) for k, v in DEFAULT_HPARAMS.items()}
    hp["fit"]["loss_kwargs"] = {"from_logits": True}
    with pytest.raises(ValueError) as cli:
        validate_output_loss(hp)
    with pytest.raises(ValueError) as comp:
        _model(out_activation="softmax").compile("Adam", CE, loss_kwargs={"from_logits": True})
    assert str(cli.value) == str(comp.value)
    hp["build"]["out_activation"] = "linear"
    validate_output_loss(hp)                                             # the configuration that trains
    hp["fit"]["loss_kwargs"] = {}
    hp["build"]["out_activation"] = "softmax"
    validate_output_loss(hp)                                             # the default project


# ---- 4. the restatement against hand-computed known answers -----------------------------------------------------------------------
def _loss_and_grad(z, y, w):
    zt = torch.tensor(np.asarray(z, np.float64).reshape(1, 1, -1), requires_grad=True)
    L = LG.ce_from_logits(zt, np.array([[y]]), np.array([w], np.float64))
    L.sum().backward()
    return float(L.item()), zt.grad.numpy().reshape(-1)


def test_restatement_known_answers():
    for y in range(3):                                                   # z = (0, 0, 0): L = ln 3 whatever the label
        L, g = _loss_and_grad([0, 0, 0], y, 1.0)
        assert abs(L - np.log(3.0)) <= 1e-15
        np.testing.assert_allclose(g, np.full(3, 1 / 3) - np.eye(3)[y], rtol=0, atol=1e-15)
    w = 0.33
    L, g = _loss_and_grad([100, 0, -100], 1, w)                          # L = 100 + log(1 + e^-100 + e^-200) = 100 to f64 rounding
    assert np.isfinite(L) and abs(L - 100 * w) <= 2 * np.spacing(100.0)
    assert np.abs(g - np.array([w, -w, 0.0])).max() <= 1e-40
    L, g = _loss_and_grad([3.7], 0, 2.0)                                 # K = 1
    assert L == 0.0 and g[0] == 0.0
    L, g = _loss_and_grad([-250.0], 0, 2.0)
    assert L == 0.0 and g[0] == 0.0


def test_closed_form_equals_autograd():
    rng = np.random.RandomState(0)
    B, M, K = 3, 50, 5
    z = rng.randn(B, M, K) * 20
    y = rng.randint(0, K, (B, M))
    w = np.array([1.0, 0.33, 2.0])
    zt = torch.tensor(z, requires_grad=True)
    L = LG.ce_from_logits(zt, y, w)
    L.sum().backward()
    Lc, dz = LG.closed_form(z, y, w)
    np.testing.assert_allclose(Lc, L.detach().numpy(), rtol=1e-13, atol=1e-13)
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-14
