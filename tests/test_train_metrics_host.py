"""
Training metrics (`fit.metrics`), host side (no GPU): the NumPy restatement tests/metrics_ref.py against known answers worked out by
hand, the names UNet.compile accepts and refuses, the reduce-then-divide helper of `mp train` on two gloo ranks, and the metric
keys in the callbacks' `logs`.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as MR                                                                # noqa: E402

quiet = lambda *a, **k: None
ACC, FG_R, FG_P, M_P, M_R, M_F1 = MR.NAMES


def _model():
    from multiplanarunet_amd.unet import UNet
    return UNet(n_classes=3, dim=32, depth=2, device="cpu", logger=quiet, seed=0)


# ---- metrics_ref ---------------------------------------------------------------------------------------------------------------
def test_known_answer_by_hand():
    """y = [0,1,1,2], pred = [0,1,2,2]: tp = [1,1,1], rel = [1,2,1], sel = [1,1,2]. accuracy 3/4; foreground recall and precision
    2/3 (two foreground hits of three foreground labels / predictions); per class 1, 2: precision 1, 1/2 and recall 1/2, 1 (means
    3/4), f1 2/3 and 2/3."""
    m = MR.batch_metrics([0, 1, 1, 2], [0, 1, 2, 2])
    assert m[ACC] == 0.75
    assert m[FG_R] == pytest.approx(2 / 3, rel=1e-15) and m[FG_P] == pytest.approx(2 / 3, rel=1e-15)
    assert m[M_P] == 0.75 and m[M_R] == 0.75
    assert m[M_F1] == pytest.approx(2 / 3, rel=1e-15)
    assert MR.argmax_first([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0]]).tolist() == [0, 1, 0]     # the first maximum


def test_all_background_labels():
    m = MR.batch_metrics([0, 0, 0, 0], [0, 1, 0, 0])
    assert math.isnan(m[FG_R]) and m[ACC] == 0.75 and m[FG_P] == 0.0


def test_absent_highest_class_shrinks_the_matrix():
    """Class 3 of a 4-class problem neither labelled nor predicted: the confusion matrix is 3 x 3 and the means run over classes
    1, 2 -- the same numbers as the 3-class problem, all finite (a fixed 4 x 4 matrix would put 0 / 0 into the means)."""
    y, p = np.array([0, 1, 1, 2, 2, 0]), np.array([0, 1, 2, 2, 2, 1])
    assert MR.confusion_matrix(y, p).shape == (3, 3)
    m = MR.batch_metrics(y, p)
    assert all(math.isfinite(v) for v in m.values())
    assert m[M_P] == pytest.approx((1 / 2 + 2 / 3) / 2, rel=1e-15) and m[M_R] == pytest.approx((1 / 2 + 1) / 2, rel=1e-15)
    # scores with a fourth, never-winning class give the same predictions and so the same values
    s3 = np.eye(3)[p]
    s4 = np.concatenate([s3, np.full((6, 1), -1.0)], axis=1)
    assert MR.Mean().update_scores(y, s4).result() == MR.Mean().update_scores(y, s3).result()


def test_middle_class_never_predicted():
    m = MR.batch_metrics([0, 1, 2, 2], [0, 0, 2, 2])
    assert math.isnan(m[M_P]) and math.isnan(m[M_F1])
    assert m[M_R] == 0.5 and m[ACC] == 0.75


def test_mean_over_batches_pixel_weighted_accuracy_batch_weighted_rest():
    batches = [([0, 1, 1, 2], [0, 1, 2, 2]),                             # accuracy 3/4, fg recall 2/3
               ([1, 1], [1, 1]),                                         # 1, 1
               ([0, 1, 2, 2, 1, 0, 1, 1], [0, 2, 2, 2, 0, 0, 1, 0])]     # 5/8, 3/6
    mean = MR.Mean()
    for y, p in batches:
        mean.update(y, p)
    r = mean.result()
    assert r[ACC] == (3 + 2 + 5) / (4 + 2 + 8)                           # over pixels, not the mean of 3/4, 1, 5/8
    assert r[ACC] != pytest.approx((3 / 4 + 1 + 5 / 8) / 3)
    assert r[FG_R] == pytest.approx((2 / 3 + 1 + 3 / 6) / 3, rel=1e-15)  # one value per batch
    assert mean.count[ACC] == 14 and mean.count[FG_R] == 3
    assert MR.Mean().result()[ACC] == 0.0                                # count 0: div_no_nan


def test_a_nan_batch_makes_the_epoch_nan():
    mean = MR.Mean().update([0, 1, 1, 2], [0, 1, 2, 2]).update([0, 0], [0, 0]).update([1, 2], [1, 2])
    r = mean.result()
    assert math.isnan(r[FG_R]) and math.isnan(r[FG_P]) and math.isnan(r[M_F1])
    assert r[ACC] == 7 / 8


# ---- compile -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MR.NAMES)
def test_compile_accepts_each_metric(name):
    from multiplanarunet_amd import unet, _lib
    assert unet.METRICS == MR.NAMES                                      # the state buffer's order
    m = _model().compile(metrics=[name])
    assert m.metrics_names == ["loss", name]
    assert m._metrics_state.dtype == torch.float64 and m._metrics_state.numel() * 8 == _lib.load().mpu_train_metrics_state_bytes()
    assert m._metrics_state.numel() >= 12 and not m._metrics_state.any()
    assert m.metrics_result() == {name: 0.0}


def test_compile_all_six_and_the_default_project():
    from multiplanarunet_amd.cli.common import DEFAULT_HPARAMS
    m = _model().compile(metrics=list(MR.NAMES))
    assert m.metrics_names == ["loss"] + list(MR.NAMES)
    fit = DEFAULT_HPARAMS["fit"]
    assert fit["metrics"] == ["sparse_categorical_accuracy"]
    m = _model().compile(fit["optimizer"], fit["loss"], fit.get("metrics"), optimizer_kwargs=fit["optimizer_kwargs"])
    assert m.metrics_names == ["loss", "sparse_categorical_accuracy"] and m._metrics_state is not None
    assert m.metrics_description() == "['sparse_categorical_accuracy']"


@pytest.mark.parametrize("bad", ["accuracy", "SparseCategoricalAccuracy", "sparse_top_k_categorical_accuracy", "dice", "dice_all",
                                 "class_wise_kappa", "one_class_dice", "MeanIoU"])
def test_unknown_metrics_raise_and_change_nothing(bad):
    m = _model().compile("SGD", metrics=[FG_R])
    state = m._metrics_state
    with pytest.raises(NotImplementedError, match="sparse_categorical_accuracy.*sparse_mean_fg_f1"):
        m.compile("Adam", metrics=[ACC, bad])
    assert m.metrics_names == ["loss", FG_R] and m._metrics_state is state and m.optimizer_name == "SGD"


def test_none_and_empty_compile_no_metrics():
    for none in (None, [], ()):
        m = _model().compile(metrics=none)
        assert m.metrics_names == ["loss"] and m._metrics_state is None and m.metrics_result() == {}
    m = _model().compile(metrics=[ACC])
    first = m._metrics_state
    assert m.compile(metrics=[ACC])._metrics_state is first              # the same list keeps the state
    assert m.compile(metrics=[ACC, FG_P])._metrics_state is not first    # another list starts from zero
    assert m.compile()._metrics_state is None and m.metrics_names == ["loss"]


# ---- data parallelism: reduce, then divide ----------------------------------------------------------------------------------------
RANK_TOTALS = [{ACC: (30.0, 64.0), FG_R: (1.25, 2.0), FG_P: (float("nan"), 2.0), M_F1: (0.0, 0.0)},
               {ACC: (10.0, 16.0), FG_R: (0.25, 3.0), FG_P: (1.0, 3.0), M_F1: (0.0, 0.0)}]


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from multiplanarunet_amd import distributed as D
    from multiplanarunet_amd.cli.train import epoch_logs
    D.init_from_env("gloo")
    logs = epoch_logs(0.5, RANK_TOTALS[rank], torch.device("cpu"))
    q.put((rank, list(logs.items())))
    torch.distributed.destroy_process_group()


def test_gloo_world2_metrics_are_pooled_before_the_division():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(r[0] for r in res) == [0, 1]
    for _, items in res:
        assert [k for k, _ in items] == ["loss", ACC, FG_R, FG_P, M_F1]
        logs = dict(items)
        assert logs[ACC] == 40.0 / 80.0                                  # not the mean of 30/64 and 10/16
        assert logs[FG_R] == 1.5 / 5.0
        assert math.isnan(logs[FG_P])                                    # one rank's NaN reaches every rank
        assert logs[M_F1] == 0.0                                         # count 0


def test_single_process_helper_divides_without_a_process_group():
    from multiplanarunet_amd.distributed import reduce_metrics
    assert reduce_metrics({}) == {}
    assert reduce_metrics({ACC: (3.0, 4.0), FG_R: (0.0, 0.0)}) == {ACC: 0.75, FG_R: 0.0}


# ---- callbacks -----------------------------------------------------------------------------------------------------------------
def test_csv_logger_and_plateau_see_the_metrics(tmp_path):
    from multiplanarunet_amd.cli.train import epoch_logs
    from multiplanarunet_amd.validation import CSVLogger, ReduceLROnPlateau, EarlyStopping

    class Model:
        optimizer_kwargs = {"lr": 1.0}
        stop_training = False
    model = Model()
    csv = CSVLogger(str(tmp_path / "training.csv"))
    plateau = ReduceLROnPlateau(monitor=ACC, mode="max", patience=2, factor=0.5, verbose=0)
    stop = EarlyStopping(monitor=FG_R, mode="max", patience=3, verbose=0)
    accs = [0.5, 0.6, 0.6, 0.6, 0.6, 0.6]
    for ep, a in enumerate(accs):
        logs = epoch_logs(1.0 / (ep + 1), {ACC: (a, 1.0), FG_R: (0.25 * (ep + 1), float(ep + 1))})
        assert list(logs) == ["loss", ACC, FG_R]
        logs["val_dice"] = 0.1                                            # (Validation adds its keys behind the metrics)
        logs["lr"] = model.optimizer_kwargs["lr"]
        for cb in (plateau, csv, stop):
            cb.on_epoch_end(model, ep, logs)
    assert model.optimizer_kwargs["lr"] == 0.25                           # fired after epochs 4 and 6 (two epochs without a gain each)
    assert model.stop_training                                            # fg recall 0.25 throughout: three epochs without a gain
    rows = [r.split(",") for r in (tmp_path / "training.csv").read_text().strip().splitlines()]
    assert rows[0] == ["epoch", "loss", "lr", ACC, FG_R, "val_dice"]
    assert [float(r[3]) for r in rows[1:]] == accs and all(float(r[4]) == 0.25 for r in rows[1:])
