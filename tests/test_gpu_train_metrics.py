"""
Training metrics on the GPU (csrc/train_metrics.hip): mpu_train_metrics_update through the C ABI against the NumPy restatement
tests/metrics_ref.py, then through UNet (eager steps, the graphed step), TrainPipeline and `mp train`. Totals and counts are f64:
integer-valued entries (the accuracy total, every count) are compared exactly, the ratios at rtol 1e-14 (a handful of f64
roundings: one division per class and metric, at most 15 additions, one division by the number of classes).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as MR                                                                # noqa: E402

pytestmark = pytest.mark.gpu
NM = len(MR.NAMES)


def quiet(*a, **k):
    pass


def _new_state():
    from multiplanarunet_amd import _lib
    n = int(_lib.load().mpu_train_metrics_state_bytes())
    assert n % 8 == 0 and n >= 2 * NM * 8
    return torch.zeros(n // 8, dtype=torch.float64, device="cuda")


def _update(state, scores, y, K):
    from multiplanarunet_amd import _lib
    p = torch.as_tensor(np.ascontiguousarray(scores, np.float32).reshape(-1, K), device="cuda")
    t = torch.as_tensor(np.ascontiguousarray(y, np.uint8).reshape(-1), device="cuda")
    _lib.call("mpu_train_metrics_update", _lib.ptr(p), _lib.ptr(t), int(t.numel()), K, _lib.ptr(state), _lib.stream_ptr())
    torch.cuda.synchronize()


def _check(state, ref):
    """state (device f64) against a metrics_ref.Mean: total[6] | count[6] | scratch left zeroed."""
    s = state.cpu().numpy()
    tot = np.array([ref.total[k] for k in MR.NAMES]); cnt = np.array([ref.count[k] for k in MR.NAMES])
    print("totals", s[:NM], "ref", tot, "counts", s[NM:2 * NM])
    assert s[0] == tot[0]                                                 # a sum of 0/1 values: exact
    np.testing.assert_array_equal(s[NM:2 * NM], cnt)
    np.testing.assert_allclose(s[1:NM], tot[1:], rtol=1e-14, atol=0, equal_nan=True)
    assert not s[2 * NM:].any(), "the finalize step must leave its scratch zeroed"


def _tied_scores(rng, n, K):
    """Scores on a grid of four values: nearly every pixel has its maximum more than once (the first one wins)."""
    return rng.randint(0, 4, (n, K)).astype(np.float32) * 0.25


@pytest.mark.parametrize("K", (1, 2, 3, 8, 16))
@pytest.mark.parametrize("n", (1, 63, 257, 256 * 2048 + 5))
def test_update_against_metrics_ref(n, K):
    """n = 256 * 2048 + 5: the grid is at its cap of 2048 workgroups and five threads take a second trip of the grid-stride loop."""
    rng = np.random.RandomState(1000 * K + n % 997)
    scores, y = _tied_scores(rng, n, K), rng.randint(0, K, n)
    if n > 1 and K > 1:
        assert (np.sort(scores, axis=1)[:, -1] == np.sort(scores, axis=1)[:, -2]).any()      # ties are present
    state = _new_state()
    _update(state, scores, y, K)
    _check(state, MR.Mean().update_scores(y, scores))


def test_first_maximum_wins():
    """Every pixel has all scores equal: every prediction is class 0, whatever K -- the last maximum would be class K - 1."""
    for K in (2, 3, 16):
        y = np.arange(130) % K
        state = _new_state()
        _update(state, np.full((130, K), 0.5, np.float32), y, K)
        ref = MR.Mean().update(y, np.zeros(130, int))
        _check(state, ref)
        assert state[0].item() == float((y == 0).sum())


def test_absent_class_all_background_and_unpredicted_middle_class():
    rng = np.random.RandomState(5)
    n = 300
    # class 3 of 4 neither labelled nor predicted: the means run over classes 1, 2 and are finite, equal to the 3-class problem's
    y = rng.randint(0, 3, n)
    s3 = rng.rand(n, 3).astype(np.float32)
    s4 = np.concatenate([s3, np.full((n, 1), -1.0, np.float32)], axis=1)
    a, b = _new_state(), _new_state()
    _update(a, s4, y, 4); _update(b, s3, y, 3)
    _check(a, MR.Mean().update_scores(y, s4))
    assert np.isfinite(a[:NM].cpu().numpy()).all() and torch.equal(a[:2 * NM], b[:2 * NM])
    # all-background labels: foreground recall is 0 / 0, accuracy stays finite
    st = _new_state()
    _update(st, s3, np.zeros(n, int), 3)
    _check(st, MR.Mean().update_scores(np.zeros(n, int), s3))
    h = st.cpu().numpy()
    assert np.isnan(h[1]) and np.isfinite(h[0]) and h[NM] == n
    # everything background, labels and predictions: a 1 x 1 confusion matrix, the mean over no class at all
    st = _new_state()
    _update(st, np.array([[1.0, 0.0, 0.0]] * 7, np.float32), np.zeros(7, int), 3)
    h = st.cpu().numpy()
    assert h[0] == 7 and np.isnan(h[1:NM]).all()
    # the middle class never predicted: mean precision and f1 are NaN, mean recall is finite
    st = _new_state()
    sc = np.eye(3, dtype=np.float32)[[0, 0, 2, 2]]
    _update(st, sc, [0, 1, 2, 2], 3)
    _check(st, MR.Mean().update_scores([0, 1, 2, 2], sc))
    h = st.cpu().numpy()
    assert np.isnan(h[3]) and np.isnan(h[5]) and h[4] == 0.5


def test_three_updates_accumulate_and_the_scratch_zeroes_itself():
    """Batches of different sizes into ONE state: the totals are the reference's accumulated ones, so the second and third step
    started from a zeroed scratch (counts left over from the step before would enter their ratios)."""
    rng = np.random.RandomState(9)
    K = 5
    state, ref = _new_state(), MR.Mean()
    for n in (700, 64, 3001):
        scores, y = _tied_scores(rng, n, K), rng.randint(0, K, n)
        _update(state, scores, y, K)
        ref.update_scores(y, scores)
        _check(state, ref)
    assert state[NM].item() == 700 + 64 + 3001 and state[NM + 1].item() == 3
    # and a NaN step makes the total NaN for good, the accuracy untouched by it
    _update(state, _tied_scores(rng, 10, K), np.zeros(10, int), K)
    _update(state, _tied_scores(rng, 50, K), rng.randint(0, K, 50), K)
    assert np.isnan(state[1].item()) and np.isfinite(state[0].item()) and state[NM + 1].item() == 5


def test_bad_arguments_are_refused():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    st = _new_state()
    p = torch.zeros(4, 17, device="cuda"); y = torch.zeros(4, dtype=torch.uint8, device="cuda")
    assert lib.mpu_train_metrics_update(_lib.ptr(p), _lib.ptr(y), 4, 17, _lib.ptr(st), None) != 0
    assert lib.mpu_train_metrics_update(_lib.ptr(p), _lib.ptr(y), 4, 0, _lib.ptr(st), None) != 0
    assert lib.mpu_train_metrics_update(None, _lib.ptr(y), 4, 3, _lib.ptr(st), None) != 0
    assert lib.mpu_train_metrics_update(_lib.ptr(p), _lib.ptr(y), 0, 3, _lib.ptr(st), None) == 0      # no pixels: nothing to add
    torch.cuda.synchronize()
    assert not st.any()


# ---- the model -----------------------------------------------------------------------------------------------------------------
B, DIM = 4, 32


def _unet(dtype, metrics=MR.NAMES, lr=1e-3):
    from multiplanarunet_amd.unet import UNet
    m = UNet(n_classes=3, dim=DIM, n_channels=1, depth=2, complexity_factor=1 / 16, flatten_output=True, dtype=dtype, logger=quiet,
             seed=0, device="cuda")
    return m.compile("Adam", "SparseCategoricalCrossentropy", list(metrics) if metrics else None, optimizer_kwargs={"lr": lr})


def _batches(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn(B, DIM, DIM, 1, generator=g)
        y = torch.randint(0, 3, (B, DIM * DIM, 1), generator=g).to(torch.uint8)
        w = torch.rand(B, generator=g) + 0.5                             # (metrics are unweighted: the weights must not show)
        out.append((x.cuda(), y.cuda(), w.cuda()))
    return out


def _probs(m):
    """The probabilities the last training forward left in the workspace."""
    from multiplanarunet_amd import _lib
    off = int(_lib.load().mpu_unet_workspace_probs_offset(m._h, B))
    return m._ws[off:off + 4 * B * DIM * DIM * 3].view(torch.float32).reshape(-1, 3).cpu().numpy()


def _state(m):
    torch.cuda.synchronize()
    return m._metrics_state[:2 * NM].cpu().numpy()


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_eager_steps_count_what_the_forward_returned_and_leave_the_training_alone(dtype):
    m, twin = _unet(dtype), _unet(dtype, metrics=None)
    assert m.metrics_names == ["loss"] + list(MR.NAMES) and twin._metrics_state is None
    ref = MR.Mean()
    for x, y, w in _batches(3):
        m.train_step(x, y, w)
        twin.train_step(x, y, w)
        ref.update_scores(y.cpu().numpy().reshape(-1), _probs(m))
        _check(m._metrics_state, ref)
    assert m._metrics_state[NM].item() == 3 * B * DIM * DIM
    assert torch.equal(m.params, twin.params) and torch.equal(m.bn_state, twin.bn_state) and torch.equal(m.packed, twin.packed)
    res = m.metrics_result()
    assert list(res) == list(MR.NAMES) and res[MR.NAMES[0]] == ref.result()[MR.NAMES[0]]
    m.reset_metrics()
    torch.cuda.synchronize()
    assert not m._metrics_state.any() and m.metrics_result()[MR.NAMES[0]] == 0.0
    # train_on_batch: [loss, metrics of THIS batch]; a float without metrics
    x, y, w = _batches(1, seed=3)[0]
    out, out_twin = m.train_on_batch(x, y, w), twin.train_on_batch(x, y, w)
    one = MR.Mean().update_scores(y.cpu().numpy().reshape(-1), _probs(m)).result()
    assert isinstance(out_twin, float) and isinstance(out, list) and out[0] == out_twin
    np.testing.assert_allclose(out[1:], [one[k] for k in MR.NAMES], rtol=1e-14, equal_nan=True)


def test_graphed_step_counts_every_replay_and_a_recapture_loses_nothing():
    """Inputs that change with every replay: a graphed step whose metric launches saw stale data (or ran once, at capture) cannot
    equal the eager twin. Then a re-capture after a learning-rate change, as TrainPipeline does it."""
    batches = _batches(8, seed=1)
    eager, graphed = _unet("bf16"), _unet("bf16")
    gx, gy, gw = (t.clone() for t in batches[0])
    replay = graphed.make_graphed_train_step(gx, gy, gw)                   # the warm-up is a real step on batch 0
    assert graphed._metrics_state is not None and any(t is graphed._metrics_state for t in replay.keep_alive)
    eager.train_step(*batches[0], want_loss=False)
    for x, y, w in batches[1:6]:
        gx.copy_(x); gy.copy_(y); gw.copy_(w)
        replay()
        eager.train_step(x, y, w, want_loss=False)
    np.testing.assert_array_equal(_state(graphed), _state(eager))
    assert _state(graphed)[NM] == 6 * B * DIM * DIM and _state(graphed)[NM + 1] == 6
    assert torch.equal(graphed.params, eager.params)
    for mdl in (eager, graphed):
        mdl.optimizer_kwargs["lr"] = 5e-4
    replay = graphed.make_graphed_train_step(gx, gy, gw, warmup=False)     # capture only: no step, nothing counted
    np.testing.assert_array_equal(_state(graphed), _state(eager))
    for x, y, w in batches[6:8]:
        gx.copy_(x); gy.copy_(y); gw.copy_(w)
        replay()
        eager.train_step(x, y, w, want_loss=False)
    np.testing.assert_array_equal(_state(graphed), _state(eager))
    assert _state(graphed)[NM] == 8 * B * DIM * DIM and _state(graphed)[NM + 1] == 8
    assert torch.equal(graphed.params, eager.params)


def test_pipeline_epoch_metrics_equal_the_serial_eager_loop():
    from multiplanarunet_amd.data import make_toy_volume, as_volume, random_views, TrainSampler
    from multiplanarunet_amd.pipeline import TrainPipeline
    dev = torch.device("cuda")
    img, lab, aff = make_toy_volume(64, 5)
    vol = as_volume(img, lab, aff, "1pct", "RobustScaler", dev, "toy64")

    def pipe(**kw):
        s = TrainSampler([vol], random_views(3, 60.0, 0), DIM, float(DIM), B, 3, noise_sd=0.1, fg_batch_fraction=0.5, seed=13)
        return TrainPipeline(_unet("bf16"), s, **kw)
    p0, p1 = pipe(graphed=False, overlap=False), pipe()
    assert p1.graphed and p1.overlap
    for steps in (5, 2):                                                  # (the second epoch: the read reset the state)
        l0, l1 = p0.run_epoch(steps), p1.run_epoch(steps)
        m0, m1 = p0.epoch_metrics(), p1.epoch_metrics()
        print(m0, m1)
        assert l0 == l1 and list(m0) == list(MR.NAMES)
        np.testing.assert_array_equal(np.array(list(m0.values())), np.array(list(m1.values())))
        assert m0[MR.NAMES[0]][1] == steps * B * DIM * DIM and m0[MR.NAMES[1]][1] == steps
        assert 0.0 <= m0[MR.NAMES[0]][0] / m0[MR.NAMES[0]][1] <= 1.0
    torch.cuda.synchronize()
    assert not p1.model._metrics_state.any()
    # a learning-rate change re-captures the step: still nothing lost, nothing counted twice
    for p in (p0, p1):
        p.model.optimizer_kwargs["lr"] = 2.5e-4
        p.run_epoch(3)
    m0, m1 = p0.epoch_metrics(), p1.epoch_metrics()
    np.testing.assert_array_equal(np.array(list(m0.values())), np.array(list(m1.values())))
    assert m1[MR.NAMES[0]][1] == 3 * B * DIM * DIM and m1[MR.NAMES[5]][1] == 3
    assert torch.equal(p0.model.params, p1.model.params)


def test_mp_train_logs_the_metrics(tmp_path, capsys):
    """The tiny project of tests/test_gpu_cli.py with two metrics in fit.metrics."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text(
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 64\n  depth: 3\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 64.0\n  batch_size: 8\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: SparseCategoricalCrossentropy\n  metrics: [sparse_categorical_accuracy, sparse_fg_recall]\n"
        "  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n")
    mp.entry_func(["train", "--project_dir", str(proj), "--synthetic", "4", "--epochs", "3",
                   "--train_images_per_epoch", "32", "--val_images_per_epoch", "16"])
    out = capsys.readouterr().out
    assert "Metrics:     ['sparse_categorical_accuracy', 'sparse_fg_recall']" in out
    lines = [l for l in out.splitlines() if l.startswith("Epoch 1/3 - ")]
    assert len(lines) == 1 and lines[0].startswith("Epoch 1/3 - loss: ")
    assert lines[0].index("loss: ") < lines[0].index("sparse_categorical_accuracy: ") < lines[0].index("sparse_fg_recall: ") \
        < lines[0].index("val_")
    rows = [r.split(",") for r in (proj / "logs" / "training.csv").read_text().strip().splitlines()]
    head = rows[0]
    assert head[0] == "epoch" and head[1] == "loss"
    assert "sparse_categorical_accuracy" in head and "sparse_fg_recall" in head and len(rows) == 1 + 3
    for r in rows[1:]:
        for k in ("sparse_categorical_accuracy", "sparse_fg_recall"):
            v = float(r[head.index(k)])
            print(k, v)
            assert np.isfinite(v) and 0.0 <= v <= 1.0
        assert np.isfinite(float(r[1]))
