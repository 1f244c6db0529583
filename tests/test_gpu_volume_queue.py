"""Volume queues on the GPU: the plane sampler over a limitation queue, `mp train --max_loaded_images`, `mp predict --dataset`
through the lazy queue. Toy 32^3 volumes as int16 .nii.gz files, a depth-2 model, dim 32."""
import contextlib
import gzip
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

YAML = ("train_data:\n  base_dir: data/train\nval_data:\n  base_dir: data/val\ntest_data:\n  base_dir: data/test\n"
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 32\n  depth: 2\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 32.0\n  batch_size: 4\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: SparseCategoricalCrossentropy\n  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n")


def write_set(folder, n, seed):
    from multiplanarunet_amd.data import make_toy_volume
    from multiplanarunet_amd.formats import save_nifti
    os.makedirs(os.path.join(folder, "images"))
    os.makedirs(os.path.join(folder, "labels"))
    for i in range(n):
        img, lab, aff = make_toy_volume(32, seed + i)
        save_nifti(os.path.join(folder, "images", "vol_%d.nii.gz" % (seed + i)), np.round(img[..., 0] * 1000).astype(np.int16), aff)
        save_nifti(os.path.join(folder, "labels", "vol_%d.nii.gz" % (seed + i)), lab, aff)


def entries_of(folder):
    from multiplanarunet_amd.cli.common import dataset_entries
    hp = {"fit": {"bg_value": "1pct", "scaler": "RobustScaler"}}
    return dataset_entries({"base_dir": str(folder)}, "/", hp, torch.device("cuda"))


def test_sampler_over_a_limitation_queue(tmp_path):
    from multiplanarunet_amd import volume_queue as VQ
    from multiplanarunet_amd.data import TrainSampler, random_views
    write_set(str(tmp_path / "set"), 5, 100)
    views = random_views(3, 60.0, 0)
    lines = []
    entries = entries_of(tmp_path / "set")
    q, _ = VQ.get_data_queues(entries, None, "limitation", None, 2, 3, lines.append, seed=0, rank_seed=1)
    assert isinstance(q, VQ.LimitationQueue) and q.n_resident == 2
    s = TrainSampler(q, views, 32, 32.0, 4, 3, seed=1, n_channels=1, device="cuda")
    seen = set()
    for _ in range(40):
        x, y, w = s()
        assert q.n_resident <= 2
        assert sum(1 for e in entries if e.volume is not None) <= 2
        assert tuple(x.shape) == (4, 32, 32, 1) and tuple(y.shape) == (4, 32 * 32, 1)
        assert bool(torch.isfinite(x).all()) and int(y.max()) < 3
        seen.update(s.last_identifiers)
        assert len(s._cache) <= 2                               # unloading drops the sampler's per-volume constants
    assert seen == {"vol_%d" % (100 + i) for i in range(5)}
    q.loading_pool.close()
    # max_loaded >= the set: the eager queue, and the batches of the list-based sampler under the same seed
    qe, _ = VQ.get_data_queues(entries_of(tmp_path / "set"), None, "limitation", None, 5, 3, lines.append, seed=0, rank_seed=1)
    assert isinstance(qe, VQ.EagerQueue) and any("Falling back to 'Eager' queue" in l for l in lines)
    from multiplanarunet_amd.cli.common import load_dataset
    vols = load_dataset({"base_dir": str(tmp_path / "set")}, "/", {"fit": {"bg_value": "1pct", "scaler": "RobustScaler"}},
                        torch.device("cuda"))
    sa = TrainSampler(qe, views, 32, 32.0, 4, 3, seed=5)
    sb = TrainSampler(vols, views, 32, 32.0, 4, 3, seed=5)
    for _ in range(3):
        for a, b in zip(sa(), sb()):
            assert torch.equal(a, b)


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """A project folder with 4 training, 3 validation and 3 test volumes, trained for two epochs under the image queue."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path_factory.mktemp("queue_proj")
    (proj / "train_hparams.yaml").write_text(YAML)
    write_set(str(proj / "data" / "train"), 4, 0)
    write_set(str(proj / "data" / "val"), 3, 1000)
    write_set(str(proj / "data" / "test"), 3, 5000)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mp.entry_func(["train", "--project_dir", str(proj), "--max_loaded_images", "2", "--num_access", "4", "--epochs", "2",
                       "--train_images_per_epoch", "16", "--val_images_per_epoch", "8"])
    return proj, out.getvalue()


def test_mp_train_honours_the_queue_flags(project):
    proj, out = project
    assert "'Limitation' queue created:\n  Dataset:      train_data (4 volumes)\n  Max loaded:   2\n  Reload limit: 4" in out
    assert "Dataset:      val_data (3 volumes)" in out
    assert "no effect" not in out
    rows = (proj / "logs" / "training.csv").read_text().strip().splitlines()
    assert len(rows) == 1 + 2
    cols = rows[0].split(",")
    for r in rows[1:]:
        vals = dict(zip(cols, r.split(",")))
        assert np.isfinite(float(vals["loss"])) and np.isfinite(float(vals["val_dice"]))
    assert out.count("Epoch ") >= 2 and (proj / "model" / "model_weights.npz").exists()


def test_mp_predict_walks_a_lazy_queue(project, monkeypatch):
    from multiplanarunet_amd.cli import mp, predict as P, common
    from multiplanarunet_amd import volume_queue as VQ
    from multiplanarunet_amd.data import load_volume_file, as_volume
    from multiplanarunet_amd.predict import multi_view_predict
    from multiplanarunet_amd.nifti import write_nifti
    from multiplanarunet_amd.unet import UNet
    proj, _ = project
    entries, peaks = [], []
    orig_entries, orig_load = common.dataset_entries, VQ.VolumeEntry.load_host

    def spy_entries(*a, **k):
        entries.extend(orig_entries(*a, **k))
        return list(entries)

    def spy_load(self):
        orig_load(self)
        peaks.append(sum(1 for e in entries if e.is_loaded))

    monkeypatch.setattr(P, "dataset_entries", spy_entries)
    monkeypatch.setattr(VQ.VolumeEntry, "load_host", spy_load)
    mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_q"])
    assert len(entries) == 3 and len(peaks) == 3 and max(peaks) <= 2
    assert not any(e.is_loaded for e in entries)
    hp = common.load_hparams(str(proj))
    build, fit = hp["build"], hp["fit"]
    model = UNet(logger=lambda *a, **k: None, dtype="bf16", device="cuda",
                 **{k: v for k, v in build.items() if k != "model_class_name"})
    model.load_weights(P.best_model_path(str(proj / "model")), by_name=True)
    views = np.load(proj / "views.npz")["arr_0"]
    for i in range(3):
        name = "vol_%d" % (5000 + i)
        img, _, aff = load_volume_file(str(proj / "data" / "test" / "images" / (name + ".nii.gz")))      # host-decoded
        vol = as_volume(img, None, aff, fit["bg_value"], fit["scaler"], "cuda", name)
        _, labels = multi_view_predict(model, vol, views, build["dim"], fit["real_space_span"], None, sum_fusion=True,
                                       batch_size=None)
        ref = str(proj / ("ref_%d.nii" % i))
        write_nifti(ref, labels.cpu().numpy().astype(np.uint8), aff)
        with gzip.open(proj / "pred_q" / "nii_files" / (name + "_PRED.nii.gz"), "rb") as f:
            got = f.read()
        with open(ref, "rb") as f:
            assert got == f.read(), name
    res = (proj / "pred_q" / "csv" / "results.csv").read_text().splitlines()
    assert len(res) == 1 + 3
