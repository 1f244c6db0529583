"""
Host side of the evaluation half of compile(): `mode: auto` of the three monitoring callbacks, the Validation callback's batch-wise
val_loss / val_<metric> keys driven by a fake model (no device), and the return forms of test_on_batch / evaluate.
"""
import numpy as np
import pytest
import torch


def quiet(*a, **k):
    pass


# monitor -> (ReduceLROnPlateau / EarlyStopping, ModelCheckpoint), tf.keras 2.3 callbacks.py: "acc" in the name (the checkpoint:
# or the name starts with "fmeasure") -> max, else min
AUTO = {"val_loss": ("min", "min"), "val_dice": ("min", "min"), "val_sparse_categorical_accuracy": ("max", "max"),
        "fmeasure_x": ("min", "max")}


@pytest.mark.parametrize("monitor", sorted(AUTO))
def test_mode_auto_resolves_as_keras_does(monitor, tmp_path):
    from multiplanarunet_amd import validation as V
    plain, ckpt = AUTO[monitor]
    rl = V.ReduceLROnPlateau(monitor=monitor, mode="auto", logger=quiet)
    es = V.EarlyStopping(monitor=monitor, mode="auto", logger=quiet)
    cp = V.ModelCheckPointClean(str(tmp_path / "w.npz"), monitor=monitor, mode="auto", logger=quiet)
    assert (rl.mode, es.mode, cp.mode) == (plain, plain, ckpt)
    for cb, mode in ((rl, plain), (es, plain), (cp, ckpt)):
        assert cb.best == (-np.inf if mode == "max" else np.inf)
    # explicit modes are untouched
    assert V.ReduceLROnPlateau(monitor=monitor, mode="max", logger=quiet).mode == "max"
    assert V.ModelCheckPointClean("x", monitor=monitor, mode="min", logger=quiet).mode == "min"


def test_auto_mode_through_the_yaml_descriptors(tmp_path):
    """init_callback_objects forwards `mode`; a val_loss monitor in auto mode reduces the rate when the loss stops FALLING."""
    from multiplanarunet_amd.cli.common import init_callback_objects
    descr = [{"class_name": "ReduceLROnPlateau", "kwargs": {"monitor": "val_loss", "mode": "auto", "patience": 1, "factor": 0.5}},
             {"class_name": "EarlyStopping", "kwargs": {"monitor": "val_sparse_categorical_accuracy", "mode": "auto", "patience": 1}}]
    objs, _ = init_callback_objects(descr, str(tmp_path), quiet, have_h5py=False)
    assert [o.mode for o in objs] == ["min", "max"]

    class M:
        optimizer_kwargs = {"lr": 1.0}
        stop_training = False
    m = M()
    for ep, (loss, accuracy) in enumerate([(1.0, 0.5), (0.5, 0.6), (0.6, 0.7)]):
        for o in objs:
            o.on_epoch_end(m, ep, {"val_loss": loss, "val_sparse_categorical_accuracy": accuracy})
    assert m.optimizer_kwargs["lr"] == 0.5 and not m.stop_training        # the loss rose once; the accuracy rose throughout


class FakeModel:
    """predict_on_batch, the evaluation hook and its accessors, all on the host: the loss of batch i is LOSSES[i], the accuracy
    counts HITS[i] of N pixels."""
    device = torch.device("cpu")
    LOSSES = (0.123456, 0.2, 0.4)
    HITS = (7, 8, 9)
    N = 12

    def __init__(self, K):
        self.K, self.i, self.updates = K, 0, 0

    def predict_on_batch(self, x):
        self.i += 1
        return torch.nn.functional.one_hot(torch.zeros(2, 6, dtype=torch.long), self.K).float()

    def evaluation_begin(self):
        return torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)

    def evaluation_update(self, probs, y, acc, state):
        assert tuple(probs.shape) == (2, 6, self.K) and tuple(y.shape) == (2, 6, 1)
        acc += torch.tensor([self.LOSSES[self.updates], 1.0], dtype=torch.float64)
        state += torch.tensor([self.HITS[self.updates], self.N], dtype=torch.float64)
        self.updates += 1

    def evaluation_totals(self, acc, state):
        return {"loss": tuple(acc.tolist()), "sparse_categorical_accuracy": tuple(state.tolist())}


def test_validation_logs_batch_wise_values_first_and_rounds_them(monkeypatch):
    from multiplanarunet_amd import validation as V
    K = 3
    labels = torch.tensor([[0, 1, 2, 0, 1, 1], [0, 0, 1, 2, 2, 0]], dtype=torch.uint8).reshape(2, 6, 1)

    def host_counts(pred, true, n_classes, counts=None):          # the counting kernel's contract, on the host
        p, t = pred.reshape(-1, n_classes).argmax(1), true.reshape(-1).long()
        for c in range(n_classes):
            counts[0, c] += int(((p == c) & (t == c)).sum()); counts[1, c] += int((t == c).sum()); counts[2, c] += int((p == c).sum())
        return counts
    monkeypatch.setattr(V, "count_cm_elements", host_counts)
    model, lines, logs = FakeModel(K), [], {"loss": 1.0}
    val = V.Validation(lambda: (None, labels, None), steps=3, n_classes=K, logger=lines.append, verbose=True)
    cw = val.on_epoch_end(model, 0, logs)
    assert model.i == 3 and model.updates == 3
    assert list(logs) == ["loss", "val_loss", "val_sparse_categorical_accuracy", "val_dice", "val_recall", "val_precision"]
    mean_loss = sum(FakeModel.LOSSES) / 3                         # 0.24115199...
    assert logs["val_loss"] == round(mean_loss, 4) == 0.2412 and logs["val_loss"] != mean_loss
    assert logs["val_sparse_categorical_accuracy"] == round(24 / 36, 4) == 0.6667
    # class-wise values: as before, unrounded, and the callback's return value
    assert set(cw) == {"dice", "recall", "precision"} and np.isnan(cw["dice"][0])
    with np.errstate(all="ignore"):
        for name in cw:
            assert logs["val_" + name] == float(np.nanmean(cw[name]))
    assert val.evaluate(FakeModel(K)).keys() == cw.keys()          # evaluate() keeps its return value
    # the table: one row per batch-wise value with the `mean` column alone, then the three class-wise rows
    rows = lines[0].splitlines()
    assert rows[0] == "Validation Results for epoch 0" and rows[1].split() == ["mean", "cls", "0", "cls", "1", "cls", "2"]
    assert rows[2].split() == ["loss", "0.2412", "-", "-", "-"]
    assert rows[3].split() == ["sparse_categorical_accuracy", "0.6667", "-", "-", "-"]
    assert [r.split()[0] for r in rows[4:]] == ["dice", "recall", "precision"] and len(rows) == 7


def _cpu_unet(metrics=None):
    """A UNet without a device whose forward and loss entry are replaced by host stand-ins: what remains under test is the
    bookkeeping of test_on_batch / evaluate (chunks, the size-weighted loss Mean, the return forms)."""
    from multiplanarunet_amd.unet import UNet
    m = UNet(n_classes=3, dim=32, depth=2, device="cpu", logger=quiet, seed=0, flatten_output=True)
    m.compile("Adam", "SparseCategoricalCrossentropy", metrics)
    m.chunks = []

    def forward(X, training, out=None):
        assert training is False
        return torch.full((X.shape[0], 32, 32, 3), 1 / 3.0)

    def update(probs, y, acc=None, metrics_state=None, sample_weight=None, loss_out=None):
        m.chunks.append(int(probs.shape[0]))
        w = torch.ones(probs.shape[0]) if sample_weight is None else torch.as_tensor(sample_weight, dtype=torch.float32)
        loss_out.copy_(w * float(len(m.chunks)))                  # chunk i: every image's loss is i
        if metrics_state is not None:
            metrics_state[0] += 1.0 * probs.shape[0]; metrics_state[6] += 2.0 * probs.shape[0]
    m._forward, m.evaluation_update = forward, update
    return m


def test_test_on_batch_and_evaluate_return_forms():
    x, y = np.zeros((10, 32, 32, 1), np.float32), np.zeros((10, 32 * 32, 1), np.uint8)
    m = _cpu_unet()
    out = m.test_on_batch(x[:4], y[:4])
    assert isinstance(out, float) and out == 1.0 and m.chunks == [4]
    assert m.test_on_batch(x[:4], y[:4], return_dict=True) == {"loss": 2.0}
    m.chunks = []
    out = m.evaluate(x, y, batch_size=4)
    assert isinstance(out, float) and m.chunks == [4, 4, 2] and out == (4 * 1 + 4 * 2 + 2 * 3) / 10.0      # weighted by batch size
    assert m.evaluate(x, y, batch_size=4, return_dict=True).keys() == {"loss"}
    m.chunks = []
    assert m.test_on_batch(x[:2], y[:2], sample_weight=[0.5, 2.0]) == 1.25
    # with a compiled metric: [loss, metric] in metrics_names order, or the dict
    m = _cpu_unet(["sparse_categorical_accuracy"])
    assert m.metrics_names == ["loss", "sparse_categorical_accuracy"]
    out = m.test_on_batch(x[:4], y[:4])
    assert isinstance(out, list) and out == [1.0, 0.5]
    m.chunks = []
    assert m.evaluate(x, y, batch_size=4, return_dict=True) == {"loss": 1.8, "sparse_categorical_accuracy": 0.5}
    # reset_metrics=False continues the Means of the call before
    m.chunks = []
    m.test_on_batch(x[:4], y[:4])
    assert m.test_on_batch(x[:2], y[:2], reset_metrics=False) == [(4 * 1 + 2 * 2) / 6.0, 0.5]
    assert m._metrics_state is not m._eval_metrics_state          # never the training epoch's state


def test_l2_penalty_is_the_regulariser_term_and_leaves_the_gradients_alone():
    from multiplanarunet_amd.unet import UNet
    m = UNet(n_classes=3, dim=32, depth=2, complexity_factor=0.0625, device="cpu", logger=quiet, seed=0, l2_reg=1e-3)
    assert UNet(n_classes=3, dim=32, depth=2, device="cpu", logger=quiet, seed=0).l2_penalty() is None
    w = m.get_weights_dict()
    want = float(np.float32(1e-3)) * sum(float((v.astype(np.float64) ** 2).sum()) for k, v in w.items()
                                         if k.endswith("/kernel") and k != "conv2d/kernel")
    g = m.grads.clone()
    np.testing.assert_allclose(float(m.l2_penalty()), want, rtol=1e-12)
    assert want > 0 and torch.equal(g, m.grads)
