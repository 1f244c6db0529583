"""
9..16 classes, host side (no GPU): a wide U-Net is built, describes its tensors and moves its weights; everything of the
training / evaluation side refuses it up front with the message of the library's guard; `mp train` refuses the project
before it touches the project folder.
"""
import os
import numpy as np
import pytest

quiet = lambda *a, **k: None


def _model(K, **kw):
    from multiplanarunet_amd.unet import UNet
    kw.setdefault("dim", 32)
    kw.setdefault("depth", 2)
    return UNet(n_classes=K, device="cpu", logger=quiet, seed=0, **kw)


def test_constructor_accepts_9_and_16_and_rejects_17():
    for K in (9, 16):
        m = _model(K)
        assert m.n_classes == K
        assert m._tensors["conv2d/kernel"][3] == (1, 1, 64, K) and m._tensors["conv2d/bias"][3] == (K,)
    with pytest.raises(ValueError, match="n_classes<=16"):
        _model(17)
    with pytest.raises(ValueError):
        _model(0)


def test_tensor_names_and_shapes_equal_the_oracle_at_16_classes():
    from oracle import unet_ref as U
    m = _model(16, n_channels=2, complexity_factor=0.25)
    w = U.init_weights(16, 2, 2, 0.25, seed=1)
    assert sorted(m._tensors) == sorted(w)
    for name, val in w.items():
        assert tuple(m._tensors[name][3]) == tuple(val.shape), name
    assert m.count_params() == sum(v.size for v in w.values())


def test_npz_round_trip_at_16_classes(tmp_path):
    from oracle import unet_ref as U
    w = U.init_weights(16, 1, 2, 1, seed=4)
    rng = np.random.RandomState(5)
    w["conv2d/bias"] = rng.uniform(-1, 1, 16).astype(np.float32)
    a = _model(16)
    a.set_weights_dict(w, strict=True)
    path = str(tmp_path / "w.npz")
    a.save_weights(path)
    b = _model(16)
    b.load_weights(path)
    assert b.missing_on_load == []
    got = b.get_weights_dict()
    for name, val in w.items():
        assert np.array_equal(got[name], val), name
    assert len(b.get_weights()) == len(w)
    with pytest.raises(ValueError, match="shape mismatch"):          # a 9-class model does not take the 16-class head
        _model(9).load_weights(path)


def _assert_names_both_limits(exc):
    msg = str(exc.value)
    assert "1..8" in msg and "9..16" in msg and "inference-only" in msg, msg


@pytest.mark.parametrize("K", (9, 16))
def test_training_and_evaluation_entry_points_refuse_a_wide_model(K):
    m = _model(K)
    assert m.compile("Adam") is m                                    # the default loss, no metrics: nothing of the training side
    x = np.zeros((2, 32, 32, 1), np.float32)
    y = np.zeros((2, 32 * 32, 1), np.uint8)
    with pytest.raises(NotImplementedError) as e:
        m.train_on_batch(x, y)
    _assert_names_both_limits(e)
    calls = {
        "train_step": lambda: m.train_step(x, y),
        "forward_backward": lambda: m.forward_backward(x, y),
        "make_graphed_train_step": lambda: m.make_graphed_train_step(x, y),
        "fit": lambda: m.fit(iter([(x, y, None)]), 1),
        "evaluate": lambda: m.evaluate(x, y),
        "test_on_batch": lambda: m.test_on_batch(x, y),
        "evaluation_update": lambda: m.evaluation_update(np.zeros((2, 32, 32, K), np.float32), y),
        "compile_metrics": lambda: m.compile("Adam", metrics=["sparse_categorical_accuracy"]),
        "compile_loss": lambda: m.compile("Adam", "SparseDiceLoss"),
        "compile_focal": lambda: m.compile("Adam", "SparseFocalLoss", loss_kwargs={"class_weights": [1.0] * K}),
        "training_forward": lambda: m._forward(x, training=True),
    }
    for name, fn in calls.items():
        with pytest.raises(NotImplementedError) as e:
            fn()
        _assert_names_both_limits(e)
    # nothing of the training state was allocated or changed on the way
    assert m._slots is None and m._ws is None and m._metrics_state is None and m._eval_acc is None
    assert m.iterations == 0 and m.metrics_names == ["loss"] and m.loss_name == "SparseCategoricalCrossentropy"


def test_library_guard_refuses_a_non_default_loss_and_17_classes():
    import ctypes as C
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    m = _model(12)
    cfg = _lib.LossConfig()
    assert lib.mpu_unet_set_loss(m._h, C.byref(cfg)) == 0            # the default: sparse cross-entropy, no class weights
    cfg.kind = _lib.MPU_LOSS_DICE
    cfg.smooth = 1.0
    assert lib.mpu_unet_set_loss(m._h, C.byref(cfg)) != 0
    msg = lib.mpu_last_error().decode()
    assert "1..8" in msg and "9..16" in msg, msg
    from multiplanarunet_amd.unet import INFERENCE_ONLY_MSG
    assert msg == INFERENCE_ONLY_MSG
    # training-mode forward and backward: refused before any pointer is looked at (no GPU here: a launch would fail otherwise)
    one = C.c_void_p(256)
    assert lib.mpu_unet_forward(m._h, 1, one, one, one, one, one, 1, None, None) != 0
    assert lib.mpu_last_error().decode() == INFERENCE_ONLY_MSG
    assert lib.mpu_unet_backward(m._h, 1, one, one, one, one, one, one, one, None, None) != 0
    assert lib.mpu_last_error().decode() == INFERENCE_ONLY_MSG
    assert lib.mpu_abi_version() == 2 and C.sizeof(_lib.LossConfig) == 9 * 4 + 8 * 4
    c17 = _lib.UNetConfig()
    c17.n_classes, c17.n_channels, c17.depth, c17.H, c17.W, c17.dtype, c17.softmax = 17, 1, 1, 32, 32, _lib.MPU_F32, 1
    c17.filters[0], c17.filters[1] = 64, 128
    assert not lib.mpu_unet_create(C.byref(c17))
    assert "n_classes<=16" in lib.mpu_last_error().decode()


def test_mp_train_refuses_ten_classes_before_it_touches_the_project(tmp_path):
    from multiplanarunet_amd.cli import train as T
    (tmp_path / "train_hparams.yaml").write_text(
        "build:\n  n_classes: 10\n  dim: 32\n  n_channels: 1\n  depth: 2\n\nfit:\n  batch_size: 2\n  real_space_span: 32.0\n")
    before = sorted(os.listdir(tmp_path))
    args = T.get_argparser().parse_args(["--project_dir", str(tmp_path), "--synthetic", "2", "--no_val", "--epochs", "1"])
    with pytest.raises(NotImplementedError) as e:
        T.run(args)
    _assert_names_both_limits(e)
    assert not (tmp_path / "model").exists() and not (tmp_path / "logs").exists()
    assert sorted(os.listdir(tmp_path)) == before
