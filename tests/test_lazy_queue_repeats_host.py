"""volume_queue.LazyQueue over a list that names one entry several times (fake loader, no GPU): `mp train_fusion` draws its
top-up with replacement and repeats images to fill a round, so one VolumeEntry can follow itself."""
import threading

from multiplanarunet_amd import volume_queue as VQ


def make_entries(n, loads):
    def loader(e):
        assert threading.current_thread() is not threading.main_thread()      # (file work runs on the read-ahead thread)
        loads.append(e.identifier)
        return {"id": e.identifier}

    return [VQ.VolumeEntry(identifier="e%d" % i, loader=loader) for i in range(n)]


def walk(order, entries):
    seen = []
    for vol in VQ.LazyQueue(VQ.Dataset(order, "round")):
        seen.append(vol["id"])
        assert sum(1 for e in entries if e.volume is not None) == 1
        assert sum(1 for e in entries if e.is_loaded) <= 2
    assert not any(e.is_loaded for e in entries)
    return seen


def test_an_entry_that_follows_itself_is_loaded_once_and_kept():
    loads = []
    a, b, c = entries = make_entries(3, loads)
    assert walk([a, a, b, a, b, b, b, c], entries) == ["e0", "e0", "e1", "e0", "e1", "e1", "e1", "e2"]
    assert loads == ["e0", "e1", "e0", "e1", "e2"]
    del loads[:]
    assert walk([a, a], entries) == ["e0", "e0"] and loads == ["e0"]
    del loads[:]
    assert walk([a, b, a], entries) == ["e0", "e1", "e0"] and loads == ["e0", "e1", "e0"]       # (apart: read again, as before)


def test_a_loop_left_early_leaves_nothing_loaded():
    loads = []
    a, b, c = entries = make_entries(3, loads)
    for order, stop in (([a, a, b], 0), ([a, a, b], 1), ([a, b, b], 1), ([a, b, c], 0)):
        for i, vol in enumerate(VQ.LazyQueue(VQ.Dataset(order, "round"))):
            if i == stop:
                break
        del vol
        assert not any(e.is_loaded for e in entries), (order, stop)


def test_a_failed_read_of_a_repeated_entry_is_raised_where_the_loop_reaches_it():
    import pytest
    calls = []

    def loader(e):
        calls.append(e.identifier)
        if len(calls) == 2:
            raise OSError("disk error on " + e.identifier)
        return e.identifier

    a, b = (VQ.VolumeEntry(identifier=n, loader=loader) for n in "ab")
    seen = []
    with pytest.raises(OSError, match="disk error on b"):
        for vol in VQ.LazyQueue(VQ.Dataset([a, a, b, b], "round")):
            seen.append(vol)
    assert seen == ["a", "a"] and not a.is_loaded and not b.is_loaded
