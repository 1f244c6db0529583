"""
The five losses of mpunet/evaluate/loss_functions.py, host side (no GPU): the restatement tests/loss_ref.py against
hand-computed known answers, the closed-form gradient the kernels implement against torch autograd of that restatement,
and the compile / C-ABI surface (UNet.compile, mpu_unet_set_loss, `mp train`'s loss_kwargs rules).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as LR                                                                   # noqa: E402

quiet = lambda *a, **k: None
ln = np.log

# Known-answer case: 2 images, 4 pixels, 3 classes; class 2 is ABSENT from image 1; sample_weight = [1, 0.33].
#   image 0: labels 0 1 2 1      image 1: labels 0 0 1 1
KAT_Y = np.array([[0, 1, 2, 1], [0, 0, 1, 1]])
KAT_P = np.array([[[.5, .25, .25], [.25, .5, .25], [.25, .25, .5], [.5, .25, .25]],
                  [[.75, .125, .125], [.5, .25, .25], [.25, .5, .25], [.125, .75, .125]]])
KAT_W = np.array([1.0, 0.33])
# per image and class, by hand:  I = sum [y=k] p_k,  P = sum p_k,  R = sum [y=k]
#   image 0: I = (.5, .5+.25, .5) = (.5, .75, .5)     P = (1.5, 1.25, 1.25)     R = (1, 2, 1)
#   image 1: I = (.75+.5, .5+.75, 0) = (1.25, 1.25, 0)  P = (1.625, 1.625, .75)   R = (2, 2, 0)


def _kat(name, **kw):
    out = LR.loss_ref(name, KAT_Y, torch.tensor(KAT_P), KAT_W, **kw)
    assert tuple(out.shape) == (2, 1)
    return out.numpy().reshape(-1)


def test_kat_dice():
    # (2I + 1) / (P + R + 1): image 0: 2/3.5 = 4/7, 2.5/4.25 = 10/17, 2/3.25 = 8/13
    #                          image 1: 3.5/4.625 = 28/37 twice; the absent class: (0 + 1) / (.75 + 0 + 1) = 4/7
    want = [1 - (4 / 7 + 10 / 17 + 8 / 13) / 3, 0.33 * (1 - (28 / 37 + 28 / 37 + 4 / 7) / 3)]
    np.testing.assert_allclose(_kat("SparseDiceLoss", smooth=1), want, rtol=1e-12)
    # smooth = 0: image 1's absent class contributes 0 / .75 = 0
    want0 = [1 - (1 / 2.5 + 1.5 / 3.25 + 1 / 2.25) / 3, 0.33 * (1 - (2.5 / 3.625 * 2 + 0) / 3)]
    np.testing.assert_allclose(_kat("SparseDiceLoss", smooth=0), want0, rtol=1e-12)


def test_kat_jaccard():
    # (I + 1) / (P + R - I + 1): image 0: 1.5/3 = 1/2, 1.75/3.5 = 1/2, 1.5/2.75 = 6/11
    #                             image 1: 2.25/3.375 = 2/3 twice; absent class: 1 / (.75 + 0 - 0 + 1) = 4/7
    want = [1 - (1 / 2 + 1 / 2 + 6 / 11) / 3, 0.33 * (1 - (2 / 3 + 2 / 3 + 4 / 7) / 3)]
    np.testing.assert_allclose(_kat("SparseJaccardDistanceLoss"), want, rtol=1e-12)


def test_kat_generalized_dice_square_and_simple():
    # Square: w = 1 / R^2: image 0 (1, 1/4, 1), image 1 (1/4, 1/4, inf -> the largest finite weight of the WHOLE [2, 3] tensor = 1,
    # which comes from image 0). score = 2 w I / (w (P + R) + 1e-6). The replaced weight multiplies I = 0: the absent class scores 0.
    e = 1e-6
    s0 = [2 * .5 / (2.5 + e), 2 * .25 * .75 / (.25 * 3.25 + e), 2 * .5 / (2.25 + e)]
    s1 = [2 * .25 * 1.25 / (.25 * 3.625 + e)] * 2 + [2 * 1 * 0 / (1 * .75 + e)]
    np.testing.assert_allclose(_kat("SparseGeneralizedDiceLoss", type_weight="Square"),
                               [1 - sum(s0) / 3, 0.33 * (1 - sum(s1) / 3)], rtol=1e-12)
    # Simple: w = 1 / R: image 0 (1, 1/2, 1), image 1 (1/2, 1/2, inf -> 1)
    s0 = [2 * .5 / (2.5 + e), 2 * .5 * .75 / (.5 * 3.25 + e), 2 * .5 / (2.25 + e)]
    s1 = [2 * .5 * 1.25 / (.5 * 3.625 + e)] * 2 + [0.0]
    np.testing.assert_allclose(_kat("SparseGeneralizedDiceLoss", type_weight="simple"),
                               [1 - sum(s0) / 3, 0.33 * (1 - sum(s1) / 3)], rtol=1e-12)
    # the replacement itself (image 1 alone has no finite weight larger than 1/4): the coupling across the batch is in the weights
    yt = torch.nn.functional.one_hot(torch.tensor(KAT_Y), 3).double()
    wts = 1 / yt.sum(1) ** 2
    assert torch.isinf(wts[1, 2]) and float(torch.where(torch.isinf(wts), torch.zeros_like(wts), wts).max()) == 1.0
    # Uniform: w = 1
    s0 = [2 * .5 / (2.5 + e), 2 * .75 / (3.25 + e), 2 * .5 / (2.25 + e)]
    s1 = [2 * 1.25 / (3.625 + e)] * 2 + [0.0]
    np.testing.assert_allclose(_kat("SparseGeneralizedDiceLoss", type_weight="Uniform"),
                               [1 - sum(s0) / 3, 0.33 * (1 - sum(s1) / 3)], rtol=1e-12)
    with pytest.raises(ValueError):
        _kat("SparseGeneralizedDiceLoss", type_weight="cubic")


def test_kat_focal():
    # gamma = 2, class_weights (.2, 1, 1): per pixel -cw_y (1 - p_y)^2 ln p_y, MEAN over the 4 pixels
    #   image 0: p_y = .5 .5 .5 .25, cw_y = .2 1 1 1 -> (.2 * .25 + .25 + .25) ln 2 + .75^2 ln 4 = (.05 + .25 + .25 + 1.125) ln 2
    #   image 1: p_y = .75 .5 .5 .75, cw_y = .2 .2 1 1 -> (.2 * .0625 + .0625) ln(4/3) + (.2 * .25 + .25) ln 2
    want = [1.675 * ln(2) / 4, 0.33 * (0.075 * ln(4 / 3) + 0.3 * ln(2)) / 4]
    np.testing.assert_allclose(_kat("SparseFocalLoss", gamma=2, class_weights=[.2, 1, 1]), want, rtol=1e-12)
    # no class weights: all ones
    want1 = [(3 * .25 * ln(2) + .5625 * ln(4)) / 4, 0.33 * (2 * .0625 * ln(4 / 3) + 2 * .25 * ln(2)) / 4]
    np.testing.assert_allclose(_kat("SparseFocalLoss"), want1, rtol=1e-12)


def test_kat_exp_log_and_alias():
    # Dice part: X = (2I + 1) / (P + R + 1) -- the Dice ratios with smooth = 1 above; mean_k (-ln X)^.3
    # cross part: mean over pixels of (-ln p_y)^.3: image 0: three times ln 2, once ln 4; image 1: twice ln(4/3), twice ln 2
    d0 = np.mean([(-ln(4 / 7)) ** .3, (-ln(10 / 17)) ** .3, (-ln(8 / 13)) ** .3])
    d1 = np.mean([(-ln(28 / 37)) ** .3, (-ln(28 / 37)) ** .3, (-ln(4 / 7)) ** .3])
    c0 = (3 * ln(2) ** .3 + ln(4) ** .3) / 4
    c1 = (2 * ln(4 / 3) ** .3 + 2 * ln(2) ** .3) / 4
    np.testing.assert_allclose(_kat("SparseExponentialLogarithmicLoss"), [d0 + c0, 0.33 * (d1 + c1)], rtol=1e-12)
    np.testing.assert_allclose(_kat("SparseExpLogDice", weight_dice=.5, weight_cross=2, gamma_dice=1, gamma_cross=1),
                               [.5 * np.mean([-ln(4 / 7), -ln(10 / 17), -ln(8 / 13)]) + 2 * (3 * ln(2) + ln(4)) / 4,
                                0.33 * (.5 * np.mean([-ln(28 / 37), -ln(28 / 37), -ln(4 / 7)]) + 2 * (2 * ln(4 / 3) + 2 * ln(2)) / 4)],
                               rtol=1e-12)


CONFIGS = [("SparseDiceLoss", {}), ("SparseDiceLoss", {"smooth": 0.25}), ("SparseJaccardDistanceLoss", {}),
           ("SparseGeneralizedDiceLoss", {"type_weight": "Square"}), ("SparseGeneralizedDiceLoss", {"type_weight": "Simple"}),
           ("SparseGeneralizedDiceLoss", {"type_weight": "Uniform"}), ("SparseFocalLoss", {}),
           ("SparseFocalLoss", {"gamma": 1.5, "class_weights": "ramp"}), ("SparseExponentialLogarithmicLoss", {}),
           ("SparseExponentialLogarithmicLoss", {"gamma_dice": .7, "gamma_cross": 1.3, "weight_dice": .4, "weight_cross": 2.})]


@pytest.mark.parametrize("K", (2, 3, 5))
@pytest.mark.parametrize("name,kw", CONFIGS)
def test_closed_form_gradient_equals_autograd(name, kw, K):
    """g = w (a + [y=k] c + [y=k] f) pass, the form the head kernels evaluate (NumPy f64, tests/loss_ref.closed_form), against
    torch autograd of the line-by-line restatement in f64: 1e-12 relative, H*W = 64, one image lacks a class; a few
    probabilities sit outside the clip range of focal / exp-log (zero gradient there)."""
    kw = dict(kw)
    if kw.get("class_weights") == "ramp":
        kw["class_weights"] = list(np.linspace(.2, 1.4, K))
    rng = np.random.RandomState(11 + K)
    B, M = 3, 64
    z = rng.randn(B, M, K) * 2
    z[0, :3, 0] += 40.0                                   # p ~ 1 - 1e-17 / 1e-18: outside [1e-7, 1 - 1e-7]
    p = np.exp(z - z.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    y = rng.randint(0, K, (B, M))
    y[1][y[1] == K - 1] = 0                               # image 1 lacks the last class
    y[0, 0] = 0; y[0, 1] = 1                              # a clipped pixel with the clipped class as label, one with another
    w = np.array([1.0, 0.33, 2.5])
    pt = torch.tensor(p, requires_grad=True)
    L = LR.loss_ref(name, y, pt, w, **kw)
    L.sum().backward()
    Lc, g = LR.closed_form(name, y, p, w, **kw)
    np.testing.assert_allclose(Lc, L.detach().numpy().reshape(-1), rtol=1e-12)
    ga = pt.grad.numpy()
    assert np.abs(g - ga).max() <= 1e-12 * np.abs(ga).max(), np.abs(g - ga).max() / np.abs(ga).max()


# ---- compile surface (device="cpu": layout and validation only; the library loads without a GPU) ------------------------------
def _model(K=3, out_activation="softmax"):
    from multiplanarunet_amd.unet import UNet
    return UNet(n_classes=K, dim=32, depth=2, out_activation=out_activation, device="cpu", logger=quiet, seed=0)


@pytest.mark.parametrize("name,kw", [("SparseDiceLoss", {"smooth": 1}), ("SparseJaccardDistanceLoss", {"smooth": 0.5}),
                                     ("SparseGeneralizedDiceLoss", {"type_weight": "Simple"}),
                                     ("SparseFocalLoss", {"gamma": 2, "class_weights": [.2, 1, 1]}),
                                     ("SparseExponentialLogarithmicLoss", {"gamma_dice": .3, "weight_cross": 2}),
                                     ("SparseExpLogDice", {"gamma_cross": .5})])
def test_compile_accepts_the_reference_losses(name, kw):
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    for loss in (name, [name]):
        for kwargs in (None, {}, kw):
            m = _model()
            n_ce = lib.mpu_unet_workspace_bytes(m._h, 2)
            assert m.compile("Adam", loss, ["sparse_categorical_accuracy"], loss_kwargs=kwargs) is m
            assert m._per_image_loss and m.loss_name == name
            assert lib.mpu_unet_workspace_bytes(m._h, 2) > n_ce          # the sums and the (a, c) table
    # an object whose class carries the name, as compile has always taken one
    obj = type(name, (), {})()
    m = _model()
    m.compile("Adam", obj, loss_kwargs=kw)
    assert m.loss_name == name
    # back to the cross-entropy: the plan is the original one again
    m.compile("Adam", "SparseCategoricalCrossentropy")
    assert not m._per_image_loss and lib.mpu_unet_workspace_bytes(m._h, 2) == n_ce
    assert lib.mpu_unet_workspace_loss_mean_offset(m._h, 2) == lib.mpu_unet_workspace_loss_mean_offset(_model()._h, 2)


def test_compile_rejects_what_the_reference_constructors_reject():
    for name in ("SparseGeneralizedDiceLoss", "SparseFocalLoss", "SparseExponentialLogarithmicLoss", "SparseExpLogDice"):
        with pytest.raises(TypeError):
            _model().compile("Adam", name, loss_kwargs={"smoooth": 1})
    with pytest.raises(TypeError):                                   # trainer.py:82 passes reduction itself
        _model().compile("Adam", "SparseDiceLoss", loss_kwargs={"reduction": "none"})
    with pytest.raises(ValueError):
        _model().compile("Adam", "SparseGeneralizedDiceLoss", loss_kwargs={"type_weight": "cubic"})
    with pytest.raises(ValueError):
        _model().compile("Adam", "SparseDiceLoss", loss_kwargs={"smooth": -1})
    with pytest.raises(ValueError):                                  # one weight per class
        _model().compile("Adam", "SparseFocalLoss", loss_kwargs={"class_weights": [1, 2]})
    with pytest.raises(ValueError):                                  # a probability loss on a linear output
        _model(out_activation="linear").compile("Adam", "SparseDiceLoss")
    for name in ("WeightedCrossEntropyWithLogits", "CategoricalCrossentropy", "MeanSquaredError"):
        with pytest.raises(NotImplementedError):
            _model().compile("Adam", name)
    m = _model()
    m.compile("Adam", "SparseCategoricalCrossentropy", loss_kwargs={})       # the default stays what it was
    assert not m._per_image_loss


def test_capi_set_loss_validates_its_config():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    assert lib.mpu_abi_version() == _lib.ABI_VERSION == 2
    assert C.sizeof(_lib.LossConfig) == 9 * 4 + 8 * 4
    m = _model()
    cfg = _lib.LossConfig()
    cfg.kind, cfg.smooth = _lib.MPU_LOSS_DICE, 1.0
    assert lib.mpu_unet_set_loss(m._h, C.byref(cfg)) == 0
    for bad in ({"kind": 6}, {"kind": -1}, {"kind": _lib.MPU_LOSS_JACCARD, "smooth": -0.5},
                {"kind": _lib.MPU_LOSS_GENERALIZED_DICE, "type_weight": 3},
                {"kind": _lib.MPU_LOSS_FOCAL, "n_class_weights": 2}):
        cfg = _lib.LossConfig()
        cfg.smooth = 1.0
        for k, v in bad.items():
            setattr(cfg, k, v)
        assert lib.mpu_unet_set_loss(m._h, C.byref(cfg)) == -1, bad                # MPU_EINVAL
        assert b"mpu_unet_set_loss" in lib.mpu_last_error()
    lin = _model(out_activation="linear")
    cfg = _lib.LossConfig()
    cfg.kind = _lib.MPU_LOSS_DICE
    assert lib.mpu_unet_set_loss(lin._h, C.byref(cfg)) == -1 and b"softmax" in lib.mpu_last_error()
    assert lib.mpu_unet_set_loss(None, C.byref(cfg)) == -1


def test_mp_train_loss_kwargs_rules():
    """bin/train.py:120-125: fit.class_weights only with SparseFocalLoss; counting the weights from the data is not built."""
    from multiplanarunet_amd.cli.train import loss_kwargs_of
    from multiplanarunet_amd.cli.common import DEFAULT_HPARAMS
    assert DEFAULT_HPARAMS["fit"]["loss_kwargs"] == {}
    assert loss_kwargs_of({"loss": "SparseDiceLoss", "loss_kwargs": {"smooth": 1}}) == {"smooth": 1}
    assert loss_kwargs_of({"loss": "SparseDiceLoss"}) == {} and loss_kwargs_of({"loss": "SparseDiceLoss", "loss_kwargs": None}) == {}
    with pytest.raises(ValueError, match="Invalid loss function 'SparseDiceLoss' used with the 'class_weights' parameter"):
        loss_kwargs_of({"loss": "SparseDiceLoss", "class_weights": True})
    with pytest.raises(ValueError, match="loss_kwargs.class_weights"):
        loss_kwargs_of({"loss": "SparseFocalLoss", "class_weights": True, "loss_kwargs": {"gamma": 2}})
    kw = {"gamma": 2, "class_weights": [.2, 1, 1]}
    assert loss_kwargs_of({"loss": ["SparseFocalLoss"], "class_weights": True, "loss_kwargs": kw}) == kw
