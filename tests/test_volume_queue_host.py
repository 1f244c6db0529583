"""Volume queues (volume_queue.py) with a fake loader, nifti.read_nifti_payload, and the declaration of mpu_volume_decode: no GPU.

The fake entries' payload is a string; without an adopter VolumeEntry.adopt hands the payload on, so the queues run as they do
with files, minus the files and the device."""
import gzip
import os
import struct
import threading
from queue import Empty

import numpy as np
import pytest

from multiplanarunet_amd import volume_queue as VQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Log:
    def __init__(self):
        self.lines, self.warnings = [], []

    def __call__(self, *a, **k):
        self.lines.append(" ".join(str(x) for x in a))

    def warn(self, msg):
        self.warnings.append(str(msg))


class Fake:
    """n fake entries; records every load, and the largest number of entries loaded at one time."""

    def __init__(self, n, fail=()):
        self.lock = threading.Lock()
        self.loads, self.peak, self.fail = [], 0, set(fail)
        self.entries = [VQ.VolumeEntry(identifier="v%d" % i, loader=self._load) for i in range(n)]

    def _load(self, e):
        with self.lock:
            if e.identifier in self.fail:
                self.fail.discard(e.identifier)                 # fails once
                raise IOError("cannot read " + e.identifier)
            self.loads.append(e.identifier)
        return "payload of " + e.identifier

    def resident(self):
        return sum(1 for e in self.entries if e.is_loaded)


def make(n=7, max_loaded=3, num_access=4, **kw):
    f, log = Fake(n, kw.pop("fail", ())), Log()
    q = VQ.LimitationQueue(VQ.Dataset(f.entries, "toy"), max_loaded=max_loaded, num_access_before_reload=num_access, logger=log,
                           seed=kw.pop("seed", 0), rank_seed=kw.pop("rank_seed", 1), **kw)
    return f, log, q


def test_max_loaded_clamping_and_eager_fallback():
    f, log, q = make(4, max_loaded=9)
    assert q.max_loaded == 4
    q.close()
    f, log, q = make(4, max_loaded=None)
    assert q.max_loaded == 4
    q.close()
    for max_loaded in (None, 4, 5):
        f, log = Fake(4), Log()
        tq, vq = VQ.get_data_queues(f.entries, None, "limitation", None, max_loaded, 4, log)
        assert isinstance(tq, VQ.EagerQueue) and vq is None
        assert len(tq.volumes) == 4 and f.resident() == 4
        assert len(log.warnings) == 1 and log.warnings[0].startswith("Falling back to 'Eager' queue for dataset train_data")
        assert "'max_loaded' value of %s" % max_loaded in log.warnings[0] and "(4)" in log.warnings[0]
    f, g, log = Fake(4), Fake(3), Log()
    tq, vq = VQ.get_data_queues(f.entries, g.entries, "limitation", "limitation", 3, 4, log)
    assert isinstance(tq, VQ.LimitationQueue) and isinstance(vq, VQ.EagerQueue)      # the same rule for both sets
    assert tq.loading_pool is not None and len(tq.loading_pool.pool) == 3
    assert any(l.startswith("'Limitation' queue created:") and "Max loaded:   3" in l and "Reload limit: 4" in l for l in log.lines)
    tq.loading_pool.close()
    f, g = Fake(4), Fake(4)
    tq, vq = VQ.get_data_queues(f.entries, g.entries, "limitation", "limitation", 2, 4, Log())
    assert tq.loading_pool is vq.loading_pool and len(tq.loading_pool.pool) == 3     # one shared pool of 3 threads
    tq.loading_pool.join()
    assert f.resident() == 2 and g.resident() == 2
    tq.loading_pool.close()


def test_preload_loads_exactly_max_loaded():
    f, log, q = make()
    assert f.resident() == 3 and q.n_resident == 3 and len(f.loads) == 3
    assert q.loaded_queue.qsize() == 3 and q.non_loaded_queue.qsize() == 4
    assert sorted(f.loads) == sorted(q.initial_order)
    q.close()


def test_initial_offsets():
    na = 40
    f, log, q = make(12, max_loaded=5, num_access=na)
    seen = []
    for _ in range(5):
        e, n = q.loaded_queue.get_nowait()
        seen.append(n)
    assert all(0 <= n < int(0.75 * na) for n in seen)
    assert len(set(seen)) > 1                                   # (random, not one value)
    # arrival max_loaded + 1 still draws an offset; every later one starts at 0
    q._add_images_to_load_queue(4)
    q.loading_pool.join()
    later = [q.loaded_queue.get_nowait()[1] for _ in range(4)]
    assert 0 <= later[0] < int(0.75 * na)
    assert later[1:] == [0, 0, 0]
    q.close()


def test_release_rules():
    f, log, q = make(5, max_loaded=2, num_access=4)
    e, _ = q.get()
    size = q.loaded_queue.qsize()
    q.release(e, 3)                                             # n_accesses = num_access - 1: re-queued with n + 1
    assert e.is_loaded and q.loaded_queue.qsize() == size + 1
    items = [q.loaded_queue.get_nowait() for _ in range(size + 1)]
    assert items[-1] == (e, 4)
    for it in items:
        q.loaded_queue.put(it)
    e2, _ = q.get()
    before = len(f.loads)
    q.release(e2, 4)                                            # n_accesses = num_access: unloaded, one new load requested
    q.loading_pool.join()
    assert not e2.is_loaded and len(f.loads) == before + 1
    assert f.loads[-1] == q.replacement_order[0]
    assert q.non_loaded_queue.queue[-1] is e2                   # at the back of the non-loaded queue
    assert f.resident() == 2
    q.close()


def test_fifo_order():
    f, log, q = make(6, max_loaded=3, num_access=1000)
    order = []
    for _ in range(9):
        with q.get_random_image() as v:
            order.append(v)
    assert order[:3] == order[3:6] == order[6:9] and len(set(order[:3])) == 3
    q.close()


def test_property_run():
    na = 4
    f, log, q = make(7, max_loaded=3, num_access=na)
    accesses = {}
    for _ in range(500):
        e, n = q.get()
        assert f.resident() <= 3
        key = (e.identifier, f.loads.count(e.identifier))       # one residency: the entry and how often it has been loaded
        accesses[key] = accesses.get(key, 0) + 1
        q.release(e, n)
        assert f.resident() <= 3
    q.loading_pool.join()
    assert f.resident() <= 3
    assert set(f.loads) == {e.identifier for e in f.entries}    # every entry was loaded at least once
    assert max(accesses.values()) <= na + 1
    q.close()


def test_failing_load_warns_and_is_replaced():
    f, log = Fake(5), Log()
    f.fail = {"v0", "v1", "v2", "v3", "v4"}
    probe = VQ.LimitationQueue(VQ.Dataset(Fake(5).entries, "p"), max_loaded=2, num_access_before_reload=4, seed=0, rank_seed=1)
    first = probe.initial_order[0]
    probe.close()
    f.fail = {first}
    q = VQ.LimitationQueue(VQ.Dataset(f.entries, "toy"), max_loaded=2, num_access_before_reload=4, logger=log, seed=0, rank_seed=1)
    assert any("Could not load image" in w and first in w for w in log.warnings)
    assert any(w.startswith("Load error on image") and first in w for w in log.warnings)
    assert f.resident() == 2 and q.loaded_queue.qsize() == 2 and first not in f.loads
    assert not [e for e in f.entries if e.identifier == first][0].is_loaded
    q.close()


def test_empty_message_after_timeout():
    import time
    f, log, q = make(5, max_loaded=2, num_access=4, timeout=0.2)
    q.loaded_queue.get_nowait(), q.loaded_queue.get_nowait()
    t0 = time.perf_counter()
    with pytest.raises(Empty) as ei:
        q.get()
    assert 0.15 < time.perf_counter() - t0 < 2.0
    assert str(ei.value) == ("Could not get ImagePair from dataset toy with timeout of 0.2 seconds. Consider increasing the number "
                             "of load threads / max loaded per dataset / access threshold")
    assert any("seems to block" in w for w in log.warnings)
    q.close()


def test_rank_seeds():
    qs = []
    for rank in (0, 1):
        f, log, q = make(12, max_loaded=4, num_access=8, seed=0, rank_seed=1000 + rank)
        qs.append(q)
        q.close()
    assert qs[0].initial_order == qs[1].initial_order
    assert sorted(qs[0].replacement_order) == sorted(qs[1].replacement_order)
    assert qs[0].replacement_order != qs[1].replacement_order
    assert set(qs[0].initial_order).isdisjoint(qs[0].replacement_order)


def test_lazy_queue_reads_one_ahead():
    f = Fake(4)
    q = VQ.LazyQueue(VQ.Dataset(f.entries, "toy"))
    seen = []
    for v in q:
        seen.append(v)
        assert f.resident() <= 2
    assert seen == ["payload of v%d" % i for i in range(4)] and f.resident() == 0
    for v in q:                                                 # a loop left early leaves nothing loaded
        break
    assert f.resident() == 0


# ---- nifti.read_nifti_payload ------------------------------------------------------------------------------------------------

def test_read_nifti_payload_agrees_with_read_nifti(tmp_path):
    from multiplanarunet_amd import nifti
    rng = np.random.RandomState(0)
    data = rng.randint(-1000, 1000, (5, 6, 7, 2)).astype(np.int16)
    aff = np.diag([1.5, 2.0, 0.5, 1.0])
    aff[:3, 3] = (3, -4, 5)
    for name in ("a.nii", "a.nii.gz"):
        p = str(tmp_path / name)
        nifti.write_nifti(p, data, aff)
        d0, a0, h0 = nifti.read_nifti(p, scaled=False)
        h, a, buf = nifti.read_nifti_payload(p)
        assert sorted(h) == sorted(h0)
        for k in h:                                             # (repr: the written scl_slope / scl_inter are NaN)
            assert k == "srow" or repr(h[k]) == repr(h0[k]), k
        np.testing.assert_array_equal(h["srow"], h0["srow"])
        np.testing.assert_array_equal(a, a0)
        got = np.frombuffer(buf, h["endian"] + "i2").reshape(h["shape"], order="F")
        np.testing.assert_array_equal(got, d0)
        assert len(buf) == data.size * 2
        h1, a1 = nifti.read_nifti_header(p)
        assert h1["shape"] == h["shape"] and np.array_equal(a1, a)
    # the same errors
    p = str(tmp_path / "a.nii")
    raw = open(p, "rb").read()
    for name, blob in (("t.nii", raw[:-10]), ("t.nii.gz", gzip.compress(raw[:-10]))):
        t = str(tmp_path / name)
        open(t, "wb").write(blob)
        with pytest.raises(nifti.NiftiError) as e0:
            nifti.read_nifti(t)
        with pytest.raises(nifti.NiftiError) as e1:
            nifti.read_nifti_payload(t)
        assert str(e0.value) == str(e1.value) and "truncated data" in str(e1.value)
    n2 = str(tmp_path / "n2.nii")
    open(n2, "wb").write(struct.pack("<i", 540) + bytes(600))
    with pytest.raises(nifti.NiftiError) as e0:
        nifti.read_nifti(n2)
    with pytest.raises(nifti.NiftiError) as e1:
        nifti.read_nifti_payload(n2)
    assert str(e0.value) == str(e1.value) == "NIfTI-2 files are not supported"


def test_scaling_condition_is_read_niftis():
    from multiplanarunet_amd.nifti import scaling_of
    nan = float("nan")
    cases = {(np.float32(0.1), np.float32(-1024.5)): True, (2.0, nan): True, (1.0, 0.0): False, (1.0, nan): False,
             (nan, 3.0): False, (0.0, 3.0): False, (1.0, 2.0): True, (float("inf"), 0.0): False}
    for (s, i), want in cases.items():
        scaled, slope, inter = scaling_of({"scl_slope": s, "scl_inter": i})
        assert scaled is want and np.isfinite(inter)
        assert inter == (0.0 if not np.isfinite(i) else float(i))


# ---- the new entry is declared ---------------------------------------------------------------------------------------------------

def test_volume_decode_is_declared():
    from multiplanarunet_amd import _lib, build
    with open(os.path.join(ROOT, "include", "mpunet_hip.h")) as f:
        header = f.read()
    assert "int mpu_volume_decode(" in header
    assert "mpu_volume_decode" in _lib.declared_symbols()
    assert _lib.ABI_VERSION == 2
    assert "-ffp-contract=off" in build.flags_of("volume_decode.hip")
    assert "volume_decode.hip" in build.sources()
