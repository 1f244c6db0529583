"""
UNet.test_on_batch / evaluate, the batch-wise val_loss / val_<metric> of the Validation callback and `mp train` with them, on the
smallest real network (3 classes, 32 x 32, depth 2, complexity factor 1/16, batches of 4), in f32 and bf16. Every model first
takes three training steps, so that the moving statistics differ from their initial values.

References: tests/loss_ref.py and oracle/unet_ref.py keras_sparse_ce (f64) on the probabilities predict_on_batch returns for the same
input; tests/metrics_ref.py for the metrics (rtol 1e-14: the single-batch tolerance of tests/test_gpu_train_metrics.py).

`packed`: its tail holds the BatchNorm coefficients folded for inference, a cache that ANY inference forward (predict_on_batch, and
so the evaluation) refreshes after the weights changed; nothing in a training step reads it. The unchanged-model test therefore
compares `packed` after one predict_on_batch (the cache is fresh: evaluation must leave every byte alone) and, straight after
training, against a twin that ran predict_on_batch instead (evaluation does to the cache what prediction does, nothing else).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as LR                                                                   # noqa: E402
import metrics_ref as MR                                                                # noqa: E402

pytestmark = pytest.mark.gpu
B, DIM, K = 4, 32, 3
CE = "SparseCategoricalCrossentropy"
METRICS = ["sparse_categorical_accuracy", "sparse_fg_recall"]        # (finite on random labels: every class is labelled)


def quiet(*a, **k):
    pass


def _unet(dtype, loss=CE, metrics=METRICS, l2_reg=None, loss_kwargs=None):
    from multiplanarunet_amd.unet import UNet
    m = UNet(n_classes=K, dim=DIM, depth=2, complexity_factor=0.0625, flatten_output=True, seed=0, dtype=dtype, logger=quiet,
             l2_reg=l2_reg)
    return m.compile("Adam", loss, metrics, optimizer_kwargs={"lr": 1e-3}, loss_kwargs=loss_kwargs)


def _batches(n, seed=0, b=B):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn(b, DIM, DIM, 1, generator=g)
        y = torch.randint(0, K, (b, DIM * DIM, 1), generator=g).to(torch.uint8)
        w = torch.rand(b, generator=g) + 0.5
        out.append((x.cuda(), y.cuda(), w.cuda()))
    return out


def _trained(dtype, **kw):
    m = _unet(dtype, **kw)
    for x, y, w in _batches(3, seed=7):
        m.train_step(x, y, w, want_loss=False)
    return m


def _ref_loss(name, kw, probs, y, w):
    """mean over the batch of w_b * L_b, f64, on the given f32 probabilities [b, ppi, K]."""
    from oracle import unet_ref as U
    p = torch.tensor(probs.astype(np.float64))
    yt = torch.tensor(y.reshape(p.shape[0], -1).astype(np.int64))
    w = np.ones(p.shape[0]) if w is None else np.asarray(w, np.float64)
    if name == CE:
        b, ppi = yt.shape
        return float(U.keras_sparse_ce(p.reshape(b, ppi, 1, K), yt.reshape(b, ppi, 1), torch.tensor(w)).mean())
    return float(LR.loss_ref(name, yt, p, w, **(kw or {})).mean())


def _snapshot(m):
    torch.cuda.synchronize()
    d = {"params": m.params.clone(), "grads": m.grads.clone(), "bn_state": m.bn_state.clone(), "packed": m.packed.clone(),
         "metrics": m._metrics_state.clone(), "iterations": m.iterations}
    d.update({"slot%d" % i: s.clone() for i, s in enumerate(m._slots)})
    return d


def _same(a, b, skip=()):
    return [k for k in a if k not in skip and not (a[k] == b[k] if k == "iterations" else torch.equal(a[k], b[k]))]


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
@pytest.mark.parametrize("loss,kw", ((CE, None), ("SparseDiceLoss", {"smooth": 1})), ids=("ce", "dice"))
def test_test_on_batch_equals_the_references_on_the_predicted_probabilities(loss, kw, dtype):
    m = _trained(dtype, loss=loss, loss_kwargs=kw)
    x, y, w = _batches(1, seed=3)[0]
    probs = m.predict_on_batch(x).cpu().numpy()
    out = m.test_on_batch(x, y, w)
    assert isinstance(out, list) and len(out) == 3 and m.metrics_names == ["loss"] + METRICS
    want = _ref_loss(loss, kw, probs, y.cpu().numpy(), w.cpu().numpy())
    one = MR.Mean().update_scores(y.cpu().numpy().reshape(-1), probs.reshape(-1, K)).result()
    print(dtype, loss, "loss", out[0], "reference", want, "metrics", out[1:], [one[k] for k in METRICS])
    np.testing.assert_allclose(out[0], want, rtol=1e-5)
    np.testing.assert_allclose(out[1:], [one[k] for k in METRICS], rtol=1e-14, equal_nan=True)
    d = m.test_on_batch(x, y, w, return_dict=True)
    assert list(d) == ["loss"] + METRICS and [d[k] for k in d] == out
    # unweighted: another reference value, the same metrics
    out1 = m.test_on_batch(x, y)
    np.testing.assert_allclose(out1[0], _ref_loss(loss, kw, probs, y.cpu().numpy(), None), rtol=1e-5)
    assert out1[1:] == out[1:] and out1[0] != out[0]


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_evaluation_leaves_the_model_as_it_was(dtype):
    m, twin = _trained(dtype), _trained(dtype)
    (x, y, w), (x2, y2, w2) = _batches(2, seed=4)
    xs, ys = torch.cat([x, x2, x[:2]]), torch.cat([y, y2, y[:2]])
    # straight after training: everything but the inference cache at the tail of `packed` is untouched, and that is what
    # predict_on_batch leaves there
    before = _snapshot(m)
    m.test_on_batch(x, y, w)
    assert _same(before, _snapshot(m), skip=("packed",)) == []
    twin.predict_on_batch(x)
    assert torch.equal(m.packed, twin.packed)
    # with the cache fresh: not one byte changes, whatever runs
    before = _snapshot(m)
    m.test_on_batch(x2, y2, w2)
    m.evaluate(xs, ys, batch_size=4)
    m.test_on_batch(x, y, reset_metrics=False)
    assert _same(before, _snapshot(m)) == []
    assert m._eval_metrics_state is not None and m._eval_metrics_state is not m._metrics_state
    # and the next training step is the twin's, bit for bit
    m.train_step(x2, y2, w2, want_loss=False)
    twin.train_step(x2, y2, w2, want_loss=False)
    torch.cuda.synchronize()
    assert torch.equal(m.params, twin.params) and torch.equal(m.bn_state, twin.bn_state) and torch.equal(m._metrics_state, twin._metrics_state)
    assert all(torch.equal(a, b) for a, b in zip(m._slots, twin._slots)) and m.iterations == twin.iterations == 4


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_evaluate_on_a_ragged_set_is_the_size_weighted_mean_of_its_chunks(dtype):
    """10 images in chunks of 4, 4 and 2. The loss: the chunk means recombined in f64 (rtol 1e-12: both sides sum the same ten f32
    values in f64, in another grouping). The metrics: the Means of compile()'s docstring over the three chunks."""
    m = _trained(dtype)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(10, DIM, DIM, 1, generator=g).cuda()
    y = torch.randint(0, K, (10, DIM * DIM, 1), generator=g).to(torch.uint8).cuda()
    w = (torch.rand(10, generator=g) + 0.5).cuda()
    out = m.evaluate(x, y, batch_size=4, sample_weight=w)
    chunks = [(0, 4), (4, 8), (8, 10)]
    per = [m.test_on_batch(x[s:e], y[s:e], w[s:e]) for s, e in chunks]
    want = sum((e - s) * p[0] for (s, e), p in zip(chunks, per)) / 10.0
    print(dtype, "evaluate", out, "chunks", per)
    np.testing.assert_allclose(out[0], want, rtol=1e-12)
    ref = MR.Mean()
    for s, e in chunks:
        ref.update_scores(y[s:e].cpu().numpy().reshape(-1), m.predict_on_batch(x[s:e]).cpu().numpy().reshape(-1, K))
    np.testing.assert_allclose(out[1:], [ref.result()[k] for k in METRICS], rtol=1e-14, equal_nan=True)
    assert m.evaluate(x.cpu().numpy(), y.cpu().numpy(), batch_size=4, sample_weight=w.cpu().numpy()) == out      # host arrays too


def test_l2_reg_adds_its_term_to_the_evaluated_loss():
    a, b = _trained("f32", l2_reg=1e-3), _trained("f32", l2_reg=1e-3)
    assert torch.equal(a.params, b.params)
    b.l2_reg = None                                               # the same weights, evaluated without the term
    x, y, w = _batches(1, seed=5)[0]
    la, lb = a.test_on_batch(x, y, w)[0], b.test_on_batch(x, y, w)[0]
    ws = a.get_weights_dict()
    term = 1e-3 * sum(float((v.astype(np.float64) ** 2).sum()) for k, v in ws.items()
                     if k.endswith("/kernel") and k != "conv2d/kernel")      # (the 1x1 head carries no regulariser)
    print("with", la, "without", lb, "difference", la - lb, "l2 * sum W^2", term)
    assert term > 0
    np.testing.assert_allclose(la - lb, term, rtol=1e-6)
    np.testing.assert_allclose(a.evaluate(x, y, sample_weight=w)[0] - lb, term, rtol=1e-6)


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_validation_callback_with_the_real_model(dtype):
    from multiplanarunet_amd import validation as V
    m = _trained(dtype, loss="SparseDiceLoss")
    batches = _batches(3, seed=9)

    def sampler_over(bs):
        it = iter(bs * 4)
        return lambda: next(it)
    lines, logs = [], {"loss": 0.5}
    val = V.Validation(sampler_over(batches), 3, K, logger=lines.append, verbose=True)
    before = _snapshot(m)
    m.predict_on_batch(batches[0][0])
    before["packed"] = m.packed.clone()
    cw = val.on_epoch_end(m, 0, logs)
    assert _same(before, _snapshot(m)) == []
    assert list(logs) == ["loss", "val_loss"] + ["val_" + k for k in METRICS] + ["val_dice", "val_recall", "val_precision"]
    # the batch-wise values: the mean over the three batches of each batch's reference value (no sample weights), 4 decimals
    probs = [m.predict_on_batch(x).cpu().numpy() for x, _, _ in batches]
    want_loss = np.mean([_ref_loss("SparseDiceLoss", {}, p, y.cpu().numpy(), None) for p, (_, y, _) in zip(probs, batches)])
    ref = MR.Mean()
    for p, (_, y, _) in zip(probs, batches):
        ref.update_scores(y.cpu().numpy().reshape(-1), p.reshape(-1, K))
    print(dtype, logs, "reference", want_loss, ref.result())
    assert logs["val_loss"] == float(np.round(want_loss, 4))
    for k in METRICS:
        assert logs["val_" + k] == float(np.round(ref.result()[k], 4))
    # the class-wise values: what Validation.evaluate gives (the code path of a model without the hook), bit for bit
    class Stub:
        device = m.device
        predict_on_batch = staticmethod(m.predict_on_batch)
    plain = V.Validation(sampler_over(batches), 3, K, logger=quiet, verbose=False)
    plain_logs = {}
    cw0 = plain.on_epoch_end(Stub(), 0, plain_logs)
    assert set(plain_logs) == {"val_dice", "val_precision", "val_recall"}
    again = val.evaluate(m)
    for name in ("dice", "recall", "precision"):
        np.testing.assert_array_equal(cw[name], cw0[name]); np.testing.assert_array_equal(again[name], cw0[name])
        assert logs["val_" + name] == plain_logs["val_" + name] or (np.isnan(logs["val_" + name]) and np.isnan(plain_logs["val_" + name]))
    assert any(l.split()[:2] == ["loss", "%.4f" % logs["val_loss"]] for l in lines[0].splitlines())


def test_mp_train_logs_val_loss_and_monitors_it(tmp_path, capsys):
    """The tiny project of tests/test_gpu_cli.py with a metric, ReduceLROnPlateau on val_loss in auto mode and checkpoints named by
    val_loss."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text(
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 64\n  depth: 3\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 64.0\n  batch_size: 8\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: SparseCategoricalCrossentropy\n  metrics: [sparse_categorical_accuracy]\n"
        "  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n"
        "  callbacks:\n"
        "    - {class_name: ReduceLROnPlateau, kwargs: {monitor: val_loss, mode: auto, patience: 2, factor: 0.9}}\n"
        "    - {class_name: ModelCheckPointClean, kwargs: {filepath: \"./model/@epoch_{epoch:02d}_val_loss_{val_loss:.5f}.h5\","
        " monitor: val_loss, mode: min}}\n"
        "    - {class_name: CSVLogger, kwargs: {filename: logs/training.csv, separator: \",\", append: true}}\n")
    mp.entry_func(["train", "--project_dir", str(proj), "--synthetic", "4", "--epochs", "2",
                   "--train_images_per_epoch", "32", "--val_images_per_epoch", "16"])
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if l.startswith("Epoch 1/2 - ")][0]
    assert line.index("val_loss: ") < line.index("val_sparse_categorical_accuracy: ") < line.index("val_dice: ")
    rows = [r.split(",") for r in (proj / "logs" / "training.csv").read_text().strip().splitlines()]
    head = rows[0]
    assert "val_loss" in head and "val_sparse_categorical_accuracy" in head and len(rows) == 1 + 2
    for r in rows[1:]:
        vl, va = float(r[head.index("val_loss")]), float(r[head.index("val_sparse_categorical_accuracy")])
        print("val_loss", vl, "val_sparse_categorical_accuracy", va)
        assert np.isfinite(vl) and np.isfinite(va) and 0.0 <= va <= 1.0 and vl > 0.0
    files = os.listdir(proj / "model")
    assert any(f.startswith("@epoch_") and "_val_loss_" in f and f.endswith((".h5", ".npz")) for f in files), files
