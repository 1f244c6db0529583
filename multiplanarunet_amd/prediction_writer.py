"""
The writer thread of `mp predict`: gzip, file write and rename of the outputs, beside the thread that drives the GPU.

  PredictionWriter   ONE worker thread and a bounded queue of jobs. A job is a destination path and either the description of a
                     NIfTI file (shape, dtype, affine) with its payload bytes on the host (nifti.write_nifti_payload), or a dict
                     of host arrays for np.savez_compressed.

THE THREADING RULE is the loaders' (volume_queue.py): the worker does FILE WORK ONLY -- gzip, write, rename -- and makes no call
into HIP or torch's device API. What makes a job's bytes (mpu_volume_encode, the device-to-host copy into a pinned buffer, the wait
for it: data.encoded_payload_to_host) runs on the compute thread, before submit.

BOUNDED MEMORY. At most `max_waiting` (2) jobs wait; submit blocks while the queue is full, so the host holds at most three
payloads: two waiting and the one being written.

ATOMIC OUTPUTS. A file is written under temp_path(destination) -- the final name + ".part", in the destination's folder -- and
moved onto the final name with os.replace only after it is closed: a final name never holds a partial file, and a run that was
killed leaves at most a ".part" file, which the next run overwrites and which nothing that looks for outputs (mp predict
--continue / --overwrite) takes for one.

ERRORS. A failure in the worker (disk full, a folder without write permission) is kept, the jobs behind it are dropped, and it is
raised on the submitting thread by the next submit or by close, as a WriterError that names the destination and chains the
original exception. After that no job is accepted. close() waits for every job, joins the thread and may be called twice.
"""
import os
import threading
from queue import Queue

import numpy as np


class WriterError(OSError):
    pass


def temp_path(path):
    return str(path) + ".part"


def _write_job(job):
    """WORKER THREAD: file work only."""
    from .nifti import write_nifti_payload
    kind, path, desc = job
    tmp = temp_path(path)
    if kind == "nifti":
        shape, dtype, affine, payload = desc
        write_nifti_payload(tmp, shape, dtype, affine, payload, compress=str(path).endswith(".gz"))
    else:
        with open(tmp, "wb") as f:                               # (a file object: savez appends no ".npz" to the temporary name)
            np.savez_compressed(f, **desc)
    os.replace(tmp, path)


class PredictionWriter:
    def __init__(self, max_waiting=2, write=None):
        self._jobs = Queue(maxsize=int(max_waiting))
        self._write = write or _write_job                       # (write: a test's stand-in for the file work)
        self._error = None                                      # (set by the worker, read by the submitting thread)
        self._closed = False
        self._reported = False                                  # (the failure has been raised once)
        self.n_written = 0
        self._thread = threading.Thread(target=self._work, name="prediction-writer", daemon=True)
        self._thread.start()

    def _work(self):
        while True:
            job = self._jobs.get()
            try:
                if job is None:
                    return
                if self._error is None:                         # (after a failure: drain without writing)
                    try:
                        self._write(job)
                        self.n_written += 1
                    except BaseException as e:                  # noqa: BLE001 (re-raised on the submitting thread)
                        err = WriterError("could not write %s: %s: %s" % (job[1], type(e).__name__, e))
                        err.__cause__ = e
                        self._error = err
            finally:
                self._jobs.task_done()

    @property
    def n_waiting(self):
        """Jobs submitted and not yet written (or dropped)."""
        return self._jobs.unfinished_tasks

    def _raise_pending(self):
        if self._error is not None:
            self._reported = True
            raise self._error

    def _submit(self, job):
        if self._closed:
            raise WriterError("could not write %s: the writer is closed" % job[1])
        if self._error is not None:                             # (again for every later job: none is accepted)
            self._reported = True
            raise self._error
        self._jobs.put(job)                                     # blocks while max_waiting jobs wait

    def submit_nifti(self, path, shape, dtype, affine, payload):
        """Queue the file nifti.write_nifti_payload(path, shape, dtype, affine, payload) writes. `payload` is host memory the
        caller no longer changes (bytes, a NumPy array over a pinned buffer, ...)."""
        self._submit(("nifti", str(path), (tuple(int(s) for s in shape), np.dtype(dtype), np.array(affine, np.float64), payload)))

    def submit_npz(self, path, arrays):
        """Queue np.savez_compressed(path, **arrays) of host arrays."""
        self._submit(("npz", str(path), dict(arrays)))

    def close(self):
        """Write what waits, end the thread, and raise the worker's failure if there was one and nobody has seen it yet."""
        if not self._closed:
            self._closed = True
            self._jobs.put(None)
            self._thread.join()
        if not self._reported:
            self._raise_pending()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                                   # (the caller's own error wins over a write failure)
            try:
                self.close()
            except WriterError:
                pass
        return False
