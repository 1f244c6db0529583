"""`mp predict` through prediction_writer.PredictionWriter and mpu_volume_encode: every output file of a 32^3 toy project
(tests/toy_project.py: depth 2, dim 32, 3 views) holds the bytes nifti.write_nifti / np.savez give for multi_view_predict's own
results, computed here once from host-decoded volumes; the writes run on the writer's thread; and a lazy queue walks a list that
names an entry twice."""
import gzip
import threading

import numpy as np
import pytest
import torch

import toy_project

pytestmark = pytest.mark.gpu

NAMES = ["vol_%d" % (5000 + i) for i in range(3)]


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """(project folder, {name: (image f32 [X,Y,Z,1], labels u8, affine, fused probabilities f32 [X,Y,Z,K], fused labels u8)})."""
    from multiplanarunet_amd.cli.predict import best_model_path
    from multiplanarunet_amd.data import load_volume_file, as_volume
    from multiplanarunet_amd.predict import multi_view_predict
    proj = tmp_path_factory.mktemp("writer_proj")
    hp, views = toy_project.make_project(proj)
    build, fit = hp["build"], hp["fit"]
    model = toy_project.load_model(hp, best_model_path(str(proj / "model")))
    ref = {}
    for name in NAMES:
        img, _, aff = load_volume_file(str(proj / "data" / "test" / "images" / (name + ".nii.gz")))       # host-decoded
        lab, _, _ = load_volume_file(str(proj / "data" / "test" / "labels" / (name + ".nii.gz")))
        vol = as_volume(img, None, aff, fit["bg_value"], fit["scaler"], "cuda", name)
        probs, labels = multi_view_predict(model, vol, views, build["dim"], fit["real_space_span"], None, sum_fusion=True,
                                           batch_size=None, want_probs=True)
        ref[name] = (np.asarray(img, np.float32), np.asarray(lab[..., 0]).astype(np.uint8), aff, probs.cpu().numpy(),
                     labels.cpu().numpy().astype(np.uint8))
    assert len({r[4].tobytes() for r in ref.values()}) == 3 and all(len(np.unique(r[4])) > 1 for r in ref.values())
    return proj, ref


def predict(proj, out_dir, *flags):
    from multiplanarunet_amd.cli import mp
    mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--no_eval", "--out_dir", out_dir]
                  + list(flags))
    return proj / out_dir / "nii_files"


def file_bytes(path):
    with (gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")) as f:
        return f.read()


def written_by_write_nifti(tmp, data, affine):
    from multiplanarunet_amd.nifti import write_nifti
    write_nifti(str(tmp / "ref.nii"), data, affine)
    return (tmp / "ref.nii").read_bytes()


def test_label_maps(project, tmp_path):
    proj, ref = project
    nii = predict(proj, "pred_labels")
    for name in NAMES:
        got = file_bytes(nii / (name + "_PRED.nii.gz"))
        assert got == written_by_write_nifti(tmp_path, ref[name][4], ref[name][2]), name
        assert got[70:72] == b"\x02\x00" and got[40:48] == np.array([3, 32, 32, 32], "<i2").tobytes()
    assert sorted(p.name for p in nii.iterdir()) == sorted(n + "_PRED.nii.gz" for n in NAMES)      # (no temporary file stays)


def test_probabilities(project, tmp_path):
    proj, ref = project
    nii = predict(proj, "pred_probs", "--no_argmax")
    for name in NAMES:
        got = file_bytes(nii / (name + "_PRED.nii.gz"))
        assert got == written_by_write_nifti(tmp_path, ref[name][3], ref[name][2]), name
        assert got[70:72] == b"\x10\x00" and got[40:50] == np.array([4, 32, 32, 32, 3], "<i2").tobytes()


def test_input_files_beside_the_prediction(project, tmp_path):
    proj, ref = project
    nii = predict(proj, "pred_inputs", "--save_input_files")
    for name in NAMES:
        img, lab, aff, _, labels = ref[name]
        sub = nii / name
        assert file_bytes(sub / (name + "_PRED.nii.gz")) == written_by_write_nifti(tmp_path, labels, aff), name
        got = file_bytes(sub / (name + "_IMAGE.nii.gz"))
        assert got == written_by_write_nifti(tmp_path, img[..., 0], aff), name            # one channel: three header dimensions
        assert got[40:42] == b"\x03\x00"
        assert file_bytes(sub / (name + "_LABELS.nii.gz")) == written_by_write_nifti(tmp_path, lab, aff), name
        assert sorted(p.name for p in sub.iterdir()) == sorted(name + s + ".nii.gz" for s in ("_PRED", "_IMAGE", "_LABELS"))


def test_npz_outputs(project):
    proj, ref = project
    nii = predict(proj, "pred_npz", "--out_format", "npz", "--save_input_files", "--no_argmax")
    for name in NAMES:
        img, lab, aff, probs, labels = ref[name]
        sub = nii / name
        with np.load(sub / (name + "_PRED.npz")) as z:
            assert sorted(z.files) == ["affine", "labels", "probs"]
            assert z["labels"].dtype == np.uint8 and np.array_equal(z["labels"], labels)
            assert z["probs"].dtype == np.float32 and np.array_equal(z["probs"].view(np.uint32), probs.view(np.uint32))
            assert np.array_equal(z["affine"], aff)
        with np.load(sub / (name + "_IMAGE.npz")) as z:
            assert sorted(z.files) == ["affine", "image"] and np.array_equal(z["image"], img[..., 0])
        with np.load(sub / (name + "_LABELS.npz")) as z:
            assert sorted(z.files) == ["affine", "labels"] and np.array_equal(z["labels"], lab)
        assert sorted(p.name for p in sub.iterdir()) == sorted(name + s + ".npz" for s in ("_PRED", "_IMAGE", "_LABELS"))


def test_writes_run_on_the_writers_thread(project, monkeypatch, tmp_path):
    from multiplanarunet_amd import prediction_writer as PW
    proj, _ = project
    threads, writers = [], []
    real_write = PW._write_job

    def spy_write(job):
        threads.append(threading.current_thread())
        real_write(job)

    class SpyWriter(PW.PredictionWriter):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            writers.append(self)

    monkeypatch.setattr(PW, "_write_job", spy_write)
    monkeypatch.setattr(PW, "PredictionWriter", SpyWriter)
    nii = predict(proj, "pred_spy", "--save_input_files")
    assert len(writers) == 1 and len(threads) == 9
    assert all(t is not threading.main_thread() and t is writers[0]._thread for t in threads)
    w = writers[0]
    assert w.n_waiting == 0 and w.n_written == 9 and not w._thread.is_alive()
    assert len(list(nii.glob("*/*.nii.gz"))) == 9 and not list(nii.glob("*/*.part"))
    # an output that exists stops the run, after the writer is closed; --continue skips it, --overwrite replaces it
    with pytest.raises(OSError, match="exists"):
        predict(proj, "pred_spy", "--save_input_files")
    assert len(writers) == 2 and not writers[1]._thread.is_alive() and writers[1].n_written == 0
    (nii / NAMES[1] / (NAMES[1] + "_PRED.nii.gz")).rename(nii / NAMES[1] / (NAMES[1] + "_PRED.nii.gz.part"))     # a killed run
    predict(proj, "pred_spy", "--save_input_files", "--continue")
    assert writers[2].n_written == 3 and not list(nii.glob("*/*.part"))
    _, ref = project
    assert file_bytes(nii / NAMES[1] / (NAMES[1] + "_PRED.nii.gz")) == written_by_write_nifti(tmp_path, ref[NAMES[1]][4], ref[NAMES[1]][2])


def test_labels_a_u8_cannot_hold_name_the_file():
    from multiplanarunet_amd.data import encoded_payload_to_host
    t = torch.zeros((4, 4, 4), dtype=torch.int64, device="cuda")
    t[1, 2, 3] = 300
    with pytest.raises(ValueError, match=r"out/x_PRED\.nii\.gz: 1 label voxels"):
        encoded_payload_to_host(t, "out/x_PRED.nii.gz")
    t[1, 2, 3] = 255
    shape, dtype, payload = encoded_payload_to_host(t, "out/x_PRED.nii.gz")
    assert shape == (4, 4, 4) and dtype == "u1" and payload.dtype == np.uint8
    assert payload.tobytes() == np.asfortranarray(t.cpu().numpy().astype(np.uint8)).tobytes(order="F")


def test_lazy_queue_walks_a_repeated_entry(project, monkeypatch):
    """[a, a, b, a, b, b]: `mp train_fusion` draws with replacement and repeats images to fill a round."""
    from multiplanarunet_amd import volume_queue as VQ
    from multiplanarunet_amd.cli import common
    proj, ref = project
    hp = common.load_hparams(str(proj))
    a, b = common.dataset_entries(hp["test_data"], str(proj), hp, torch.device("cuda"))[:2]
    loads, peaks = [], []
    orig = VQ.VolumeEntry.load_host

    def spy_load(self):
        orig(self)
        loads.append(self.identifier)
        peaks.append(sum(1 for e in (a, b) if e.is_loaded))

    monkeypatch.setattr(VQ.VolumeEntry, "load_host", spy_load)
    order = [a, a, b, a, b, b]
    seen = []
    for vol in VQ.LazyQueue(VQ.Dataset(order, "round")):
        seen.append(vol.identifier)
        assert torch.equal(vol.image.cpu(), torch.from_numpy(ref[vol.identifier][0]))
        assert sum(1 for e in (a, b) if e.volume is not None) == 1
        del vol
    assert seen == [e.identifier for e in order]
    assert loads == [a.identifier, b.identifier, a.identifier, b.identifier] and max(peaks) <= 2
    assert not a.is_loaded and not b.is_loaded
    for vol in VQ.LazyQueue(VQ.Dataset([a, a, b], "left early")):   # a loop left on the first of two turns: nothing stays loaded
        break
    del vol
    assert not a.is_loaded and not b.is_loaded
