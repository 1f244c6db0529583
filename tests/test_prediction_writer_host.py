"""prediction_writer.PredictionWriter with NumPy payloads, nifti.write_nifti_payload, and the output planning of `mp predict`:
no GPU. Nothing here sleeps: a slow write is a write that waits for an event the test sets."""
import gzip
import os
import threading

import numpy as np
import pytest

WAIT = 20.0            # upper bound of a wait that is expected to end at once; no test waits for it to run out


def volume(seed=0, shape=(5, 4, 3), dtype=np.uint8):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 200, shape).astype(dtype)
    aff = np.array([[0.5, 0, 0, -3], [0, 2, 0, 4], [0, 0, 1.5, 5], [0, 0, 0, 1]], np.float64)
    return a, aff


def payload_of(a):
    return np.asfortranarray(a).tobytes(order="F")


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


class Gate:
    """A write function that announces each job and then waits until the test lets it through."""

    def __init__(self):
        from multiplanarunet_amd import prediction_writer as PW
        self.started = [threading.Event() for _ in range(8)]
        self.go = [threading.Event() for _ in range(8)]
        self.order, self.threads, self._real, self.n = [], [], PW._write_job, 0

    def __call__(self, job):
        i, self.n = self.n, self.n + 1
        self.threads.append(threading.current_thread())
        self.started[i].set()
        assert self.go[i].wait(WAIT)
        self._real(job)
        self.order.append(job[1])


def test_write_nifti_payload_is_write_nifti_in_two_steps(tmp_path):
    from multiplanarunet_amd.nifti import write_nifti, write_nifti_payload, read_nifti, NiftiError
    for dtype, shape in ((np.uint8, (5, 4, 3)), (np.float32, (5, 4, 3, 2)), (np.int16, (7,)), (np.float64, (2, 3))):
        a, aff = volume(1, shape, dtype)
        write_nifti(str(tmp_path / "a.nii"), a, aff)
        write_nifti_payload(str(tmp_path / "b.nii"), a.shape, a.dtype, aff, payload_of(a))
        assert (tmp_path / "a.nii").read_bytes() == (tmp_path / "b.nii").read_bytes()
        write_nifti(str(tmp_path / "a.nii.gz"), a, aff)
        write_nifti_payload(str(tmp_path / "b.nii.gz"), a.shape, a.dtype, aff, np.frombuffer(payload_of(a), np.uint8))
        assert gunzip(tmp_path / "a.nii.gz") == gunzip(tmp_path / "b.nii.gz") == (tmp_path / "a.nii").read_bytes()
        write_nifti_payload(str(tmp_path / "c.part"), a.shape, a.dtype, aff, payload_of(a), compress=True)
        assert gunzip(tmp_path / "c.part") == (tmp_path / "a.nii").read_bytes()
        back, aff2, _ = read_nifti(str(tmp_path / "b.nii.gz"), scaled=False)
        assert np.array_equal(back, a) and np.allclose(aff2, aff)
    a, aff = volume()
    with pytest.raises(NiftiError, match="payload of 59 bytes"):
        write_nifti_payload(str(tmp_path / "short.nii"), a.shape, a.dtype, aff, payload_of(a)[:-1])
    with pytest.raises(NiftiError, match="cannot store dtype"):
        write_nifti_payload(str(tmp_path / "c64.nii"), a.shape, np.complex64, aff, b"")
    with pytest.raises(NiftiError, match="affine must be 4x4"):
        write_nifti_payload(str(tmp_path / "aff.nii"), a.shape, a.dtype, np.eye(3), payload_of(a))


def test_final_name_appears_only_when_the_file_is_complete(tmp_path, monkeypatch):
    """The gzip step is held open: the final name does not exist, the temporary one does. After close() it is the other way."""
    from multiplanarunet_amd import prediction_writer as PW
    from multiplanarunet_amd.nifti import write_nifti
    a, aff = volume()
    dst = str(tmp_path / "x_PRED.nii.gz")
    opened, go = threading.Event(), threading.Event()
    real_open = gzip.open

    def slow_open(name, *args, **kwargs):
        f = real_open(name, *args, **kwargs)
        if str(name) == PW.temp_path(dst):
            opened.set()
            assert go.wait(WAIT)
        return f

    monkeypatch.setattr(gzip, "open", slow_open)
    w = PW.PredictionWriter()
    w.submit_nifti(dst, a.shape, a.dtype, aff, payload_of(a))
    assert opened.wait(WAIT)
    assert not os.path.exists(dst) and os.path.exists(PW.temp_path(dst)) and w.n_waiting == 1
    go.set()
    w.close()
    monkeypatch.setattr(gzip, "open", real_open)
    assert os.path.exists(dst) and not os.path.exists(PW.temp_path(dst)) and w.n_waiting == 0 and w.n_written == 1
    write_nifti(str(tmp_path / "ref.nii"), a, aff)
    assert gunzip(dst) == (tmp_path / "ref.nii").read_bytes()
    w.close()                                                    # twice: nothing happens


def test_bytes_of_every_kind_of_job(tmp_path):
    from multiplanarunet_amd import prediction_writer as PW
    from multiplanarunet_amd.nifti import write_nifti
    w = PW.PredictionWriter()
    refs = []
    for i, (dtype, shape) in enumerate(((np.uint8, (9, 8, 7)), (np.float32, (9, 8, 7, 3)), (np.float32, (4, 4, 4)))):
        a, aff = volume(i, shape, dtype)
        for name in ("v%d.nii.gz" % i, "v%d.nii" % i):
            w.submit_nifti(str(tmp_path / name), a.shape, a.dtype, aff, np.frombuffer(payload_of(a), np.uint8))
        refs.append((i, a, aff))
    lab, lab_aff = volume(7)
    w.submit_npz(str(tmp_path / "v.npz"), {"labels": lab, "affine": lab_aff})
    w.close()
    for i, a, aff in refs:
        write_nifti(str(tmp_path / "ref.nii"), a, aff)
        want = (tmp_path / "ref.nii").read_bytes()
        assert gunzip(tmp_path / ("v%d.nii.gz" % i)) == want and (tmp_path / ("v%d.nii" % i)).read_bytes() == want
    with np.load(tmp_path / "v.npz") as z:
        assert sorted(z.files) == ["affine", "labels"] and np.array_equal(z["labels"], lab) and np.array_equal(z["affine"], lab_aff)
    assert sorted(os.listdir(tmp_path)) == sorted(["ref.nii", "v.npz"] + ["v%d.nii%s" % (i, e) for i in range(3) for e in ("", ".gz")])


def test_jobs_complete_in_submission_order_on_one_other_thread(tmp_path):
    from multiplanarunet_amd import prediction_writer as PW
    gate = Gate()
    for e in gate.go:
        e.set()
    w = PW.PredictionWriter(write=gate)
    a, aff = volume()
    names = [str(tmp_path / ("n%d.nii.gz" % i)) for i in range(6)]
    for n in names:
        w.submit_nifti(n, a.shape, a.dtype, aff, payload_of(a))
    w.close()
    assert gate.order == names
    assert len(set(gate.threads)) == 1 and gate.threads[0] is not threading.current_thread()
    assert not w._thread.is_alive()


def test_submit_blocks_at_the_bound(tmp_path):
    """One job in the worker and two waiting: the fourth submit does not return until the worker takes the next job."""
    from multiplanarunet_amd import prediction_writer as PW
    gate = Gate()
    w = PW.PredictionWriter(write=gate)
    a, aff = volume()
    names = [str(tmp_path / ("b%d.nii" % i)) for i in range(4)]
    w.submit_nifti(names[0], a.shape, a.dtype, aff, payload_of(a))
    assert gate.started[0].wait(WAIT)                            # the worker holds job 0
    w.submit_nifti(names[1], a.shape, a.dtype, aff, payload_of(a))
    w.submit_nifti(names[2], a.shape, a.dtype, aff, payload_of(a))
    assert w.n_waiting == 3
    entered, done = threading.Event(), threading.Event()

    def fourth():
        entered.set()
        w.submit_nifti(names[3], a.shape, a.dtype, aff, payload_of(a))
        done.set()

    t = threading.Thread(target=fourth, daemon=True)
    t.start()
    assert entered.wait(WAIT)
    assert w._jobs.full() and not done.is_set()                  # (two wait: the queue is at its bound)
    assert not done.wait(0.2)                                    # the one time-boxed wait: the submit is still blocked
    gate.go[0].set()                                             # job 0 ends, the worker takes job 1: room for the fourth
    assert done.wait(WAIT)
    for e in gate.go:
        e.set()
    t.join()
    w.close()
    assert gate.order == names and all(os.path.exists(n) for n in names)


def test_a_worker_error_reaches_the_submitting_thread(tmp_path):
    from multiplanarunet_amd import prediction_writer as PW
    a, aff = volume()
    missing = str(tmp_path / "no_such_folder" / "e_PRED.nii.gz")
    w = PW.PredictionWriter()
    w.submit_nifti(missing, a.shape, a.dtype, aff, payload_of(a))
    w._jobs.join()                                               # (the worker has met the error)
    with pytest.raises(PW.WriterError, match="no_such_folder.*e_PRED") as ei:
        w.submit_nifti(str(tmp_path / "after.nii.gz"), a.shape, a.dtype, aff, payload_of(a))
    assert isinstance(ei.value, OSError) and isinstance(ei.value.__cause__, FileNotFoundError)
    with pytest.raises(PW.WriterError, match="no_such_folder"):   # later submits are refused as well
        w.submit_npz(str(tmp_path / "after.npz"), {"labels": a})
    w.close()                                                    # (already reported: close only ends the thread)
    assert not os.path.exists(tmp_path / "after.nii.gz") and not w._thread.is_alive()
    # ... or at close, when no submit came in between; the jobs behind the failed one are dropped
    w = PW.PredictionWriter()
    w.submit_nifti(missing, a.shape, a.dtype, aff, payload_of(a))
    w.submit_nifti(str(tmp_path / "behind.nii.gz"), a.shape, a.dtype, aff, payload_of(a))
    with pytest.raises(PW.WriterError, match="no_such_folder.*e_PRED"):
        w.close()
    w.close()
    assert not os.path.exists(tmp_path / "behind.nii.gz")
    with pytest.raises(PW.WriterError, match="closed"):
        w.submit_npz(str(tmp_path / "late.npz"), {"labels": a})
    # a payload that does not fit its header is the worker's error too
    w = PW.PredictionWriter()
    w.submit_nifti(str(tmp_path / "short.nii"), a.shape, a.dtype, aff, payload_of(a)[:-1])
    with pytest.raises(PW.WriterError, match=r"short\.nii.*payload of 59 bytes"):
        w.close()
    assert not os.path.exists(tmp_path / "short.nii")


def test_planning_looks_at_final_names_only(tmp_path):
    """A ".part" file of a killed run is no output: --continue predicts that volume again and the writer overwrites the file."""
    from types import SimpleNamespace
    from multiplanarunet_amd import prediction_writer as PW
    from multiplanarunet_amd.cli.predict import plan_todo
    from multiplanarunet_amd.nifti import write_nifti
    items = [SimpleNamespace(identifier="v%d" % i) for i in range(3)]
    dst_of = lambda it: str(tmp_path / ("%s_PRED.nii.gz" % it.identifier))
    a, aff = volume()
    write_nifti(dst_of(items[0]), a, aff)                                       # v0: done
    with open(PW.temp_path(dst_of(items[1])), "wb") as f:                        # v1: killed mid-write
        f.write(b"half a file")
    todo, conflict = plan_todo(items, dst_of, continue_=True, overwrite=False)
    assert [it.identifier for it in todo] == ["v1", "v2"] and conflict is None
    todo, conflict = plan_todo(items, dst_of, continue_=False, overwrite=False)
    assert todo == [] and conflict == dst_of(items[0])
    todo, conflict = plan_todo(items[1:], dst_of, continue_=False, overwrite=False)
    assert len(todo) == 2 and conflict is None
    todo, conflict = plan_todo(items, dst_of, continue_=False, overwrite=True)
    assert len(todo) == 3 and conflict is None
    with PW.PredictionWriter() as w:
        w.submit_nifti(dst_of(items[1]), a.shape, a.dtype, aff, payload_of(a))
    assert gunzip(dst_of(items[1])) == gunzip(dst_of(items[0]))
    assert not os.path.exists(PW.temp_path(dst_of(items[1])))


def test_no_device_contact(tmp_path):
    """A fresh interpreter (this one may have opened the device for other tests) plans, writes a NIfTI job and an .npz job through
    the writer, and has not initialised the device at the end."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from multiplanarunet_amd import prediction_writer as PW\n"
        "from multiplanarunet_amd.cli.predict import plan_todo\n"
        "a = np.arange(60, dtype=np.uint8).reshape(5, 4, 3)\n"
        "dst = %r\n"
        "todo, conflict = plan_todo(['v'], lambda it: dst, False, False)\n"
        "assert todo == ['v'] and conflict is None\n"
        "w = PW.PredictionWriter()\n"
        "w.submit_nifti(dst, a.shape, a.dtype, np.eye(4), np.asfortranarray(a).tobytes(order='F'))\n"
        "w.submit_npz(dst[:-7] + '.npz', {'labels': a, 'affine': np.eye(4)})\n"
        "w.close()\n"
        "assert w.n_written == 2\n"
        "print('device initialised:', torch.cuda.is_initialized())\n") % (root, str(tmp_path / "v_PRED.nii.gz"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device initialised: False" in out.stdout, out.stdout
    assert os.path.exists(tmp_path / "v_PRED.nii.gz") and os.path.exists(tmp_path / "v_PRED.npz")
