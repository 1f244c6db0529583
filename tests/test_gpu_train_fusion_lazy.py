"""`mp train_fusion` one image at a time: the rounds are planned on dataset entries and walked through a lazy queue. The 32^3 toy
project of tests/toy_project.py (depth 2, dim 32, 3 views) with 3 validation and 4 training volumes: fewer than 15 validation
images, so the set is topped up from the training set WITH replacement (12 draws from 4) and padded to a multiple of the round
size -- entries occur several times, also back to back."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import toy_project

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    proj = tmp_path_factory.mktemp("fusion_proj")
    hp, views = toy_project.make_project(proj)
    return proj, hp, views


@pytest.fixture(scope="module")
def fusion_run(project):
    """One `mp train_fusion --images_per_round 2` under a spy on the entries: after every load, adopt and unload, how many entries
    hold a resident volume and how many are loaded (payload or volume)."""
    from multiplanarunet_amd import volume_queue as VQ
    from multiplanarunet_amd.cli import mp, train_fusion as TF
    proj, hp, views = project
    entries, adopted, loaded, events = [], [], [], []
    orig_entries = TF.dataset_entries
    orig = {n: getattr(VQ.VolumeEntry, n) for n in ("load_host", "adopt", "unload")}

    def spy_entries(*a, **k):
        got = orig_entries(*a, **k)
        entries.extend(got)
        return got

    def spy(name):
        def call(self, *a, **k):
            out = orig[name](self, *a, **k)
            events.append((name, self.identifier))
            adopted.append(sum(1 for e in entries if e.volume is not None))
            loaded.append(sum(1 for e in entries if e.is_loaded))
            return out
        return call

    out = io.StringIO()
    with pytest.MonkeyPatch.context() as mpatch:
        mpatch.setattr(TF, "dataset_entries", spy_entries)
        for n in orig:
            mpatch.setattr(VQ.VolumeEntry, n, spy(n))
        with contextlib.redirect_stdout(out):
            history = mp.entry_func(["train_fusion", "--project_dir", str(proj), "--images_per_round", "2", "--epochs", "1",
                                     "--seed", "3", "--eval_prob", "0"])
    return dict(entries=entries, adopted=adopted, loaded=loaded, events=events, log=out.getvalue())


def test_one_volume_resident_at_a_time(fusion_run):
    r = fusion_run
    assert len(r["entries"]) == 3 + 4                            # the validation set and the training set, as entries
    n_adopts = sum(1 for name, _ in r["events"] if name == "adopt")
    assert n_adopts == 16                                         # 3 + 12 drawn = 15, padded to 16: 8 rounds of 2
    assert max(r["adopted"]) == 1, max(r["adopted"])
    assert max(r["loaded"]) <= 2, max(r["loaded"])
    assert not any(e.is_loaded for e in r["entries"])
    assert len(re.findall(r"^Set \d+/8: ", r["log"], re.M)) == 8


def test_top_up_with_replacement_runs_to_the_end(fusion_run, project):
    from multiplanarunet_amd.cli.common import fusion_weights_path
    from multiplanarunet_amd.cli.predict import best_model_path
    proj, hp, views = project
    used = [ident for name, ident in fusion_run["events"] if name == "adopt"]
    val = {"vol_%d" % (1000 + i) for i in range(3)}
    train = [u for u in used if u not in val]
    assert val <= set(used) and len(train) >= 12 and len(set(train)) <= 4      # 12 draws from 4: repeats
    path = fusion_weights_path(str(proj / "model"), best_model_path(str(proj / "model")))
    with np.load(path) as z:
        assert z["W"].shape == (3, 3) and np.isfinite(z["W"]).all() and np.isfinite(z["b"]).all()
        assert not np.array_equal(z["W"], np.ones((3, 3), np.float32))           # (it was fitted)
    assert "Saved fusion weights:" in fusion_run["log"]


def test_lazy_iterator_gives_the_points_of_the_list(project):
    from multiplanarunet_amd import volume_queue as VQ
    from multiplanarunet_amd.cli import common, train_fusion as TF
    from multiplanarunet_amd.interpolation import ViewSampler
    proj, hp, views = project
    build, fit = hp["build"], hp["fit"]
    dev = torch.device("cuda")
    model = toy_project.load_model(hp, str(proj / "model" / "model_weights.npz"))
    sampler = ViewSampler(views, build["dim"], fit["real_space_span"])
    quiet = lambda *a, **k: None
    vols = common.load_dataset(hp["val_data"], str(proj), hp, dev)
    entries = common.dataset_entries(hp["val_data"], str(proj), hp, dev)
    order = [0, 2, 2, 1]                                          # (with a repeat back to back)
    Xa, ya = TF.collect_points(model, sampler, [vols[i] for i in order], views, 3, 4, quiet, 0.0, np.random.RandomState(0))
    Xb, yb = TF.collect_points(model, sampler, VQ.LazyQueue(VQ.Dataset([entries[i] for i in order], "round")), views, 3, 4,
                               quiet, 0.0, np.random.RandomState(0))
    assert tuple(Xa.shape) == (4 * 32 ** 3, 3, 3) and ya.dtype == torch.uint8
    assert torch.equal(Xa, Xb) and torch.equal(ya, yb)
    assert not any(e.is_loaded for e in entries)
    Xe, ye = TF.collect_points(model, sampler, VQ.LazyQueue(VQ.Dataset([], "empty")), views, 3, 4, quiet)
    assert tuple(Xe.shape) == (0, 3, 3) and tuple(ye.shape) == (0,)
