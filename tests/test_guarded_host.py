"""The guard-band helper (tests/guarded.py) on CPU tensors: it places buffers where it says, and it can fail -- a planted guard
byte is reported with its offset, high_water finds the planted extent. The counterpart of test_replay_bounds_host.py for the
guard tests (test_gpu_guard_*.py)."""
import pytest
import torch

from guarded import ALIGN, Arena, BIG, NAN, POISONS, ZERO, high_water, last_written

DTYPES = (torch.uint8, torch.bfloat16, torch.float32, torch.float64)
SIZES = (1, 3, 255, 257)
G = 4096


def _arena(fill=NAN):
    return Arena("cpu", guard_bytes=G, capacity_bytes=1 << 20, fill=fill)


@pytest.mark.parametrize("fill", POISONS)
def test_carve_alignment_and_exact_end_guards(fill):
    a = _arena(fill)
    views = [(a.carve(n, dt), n, dt) for dt in DTYPES for n in SIZES]
    base = a.mem.data_ptr()
    spans = []
    for v, n, dt in views:
        esz = v.element_size()
        assert v.dtype == dt and v.numel() == n and v.is_contiguous()
        assert v.data_ptr() % ALIGN == 0
        lo = v.data_ptr() - base
        hi = lo + n * esz                                            # the exact last byte + 1, not a rounded-up size
        assert lo - G >= 0 and hi + G <= a.mem.numel()
        assert bool((a.mem[lo - G:lo] == fill).all()) and bool((a.mem[hi:hi + G] == fill).all())
        spans.append((lo - G, hi + G))
    spans.sort()
    assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))      # guards of neighbours do not overlap
    assert [(s, e) for _, s, e in a.bufs] == [(v.data_ptr() - base, v.data_ptr() - base + v.numel() * v.element_size())
                                              for v, _, _ in views]
    assert a.check() == []


def test_poison_values():
    a = _arena(NAN)
    assert bool(torch.isnan(a.carve(5, torch.float32)).all()) and bool(torch.isnan(a.carve(5, torch.bfloat16).float()).all())
    assert bool(torch.isnan(a.carve(5, torch.float64)).all())
    assert a.carve(3, torch.int64).tolist() == [-1] * 3 and a.carve(3, torch.uint8).tolist() == [255] * 3
    big = a.carve(4, torch.float32, fill=BIG)
    assert bool(torch.isfinite(big).all()) and 1e36 < float(big[0]) < 2e36
    bigh = a.carve(4, torch.bfloat16, fill=BIG).float()
    assert bool(torch.isfinite(bigh).all()) and 1e36 < float(bigh[0]) < 2e36
    assert a.carve(4, torch.float64, fill=ZERO).tolist() == [0.0] * 4
    src = torch.arange(7, dtype=torch.float32)
    assert torch.equal(a.put(src), src) and torch.equal(a.carve((7,), torch.float32, fill=src), src)
    assert a.check() == []                                           # filling the buffers touched no guard


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_planted_bytes_are_reported_with_their_offsets(dtype, n):
    a = _arena()
    a.carve(17, torch.float32, name="first")
    v = a.carve(n, dtype, name="victim")
    a.carve(9, torch.uint8, name="last")
    lo = v.data_ptr() - a.mem.data_ptr()
    hi = lo + n * v.element_size()
    a.mem[lo - 1] = 1                                                 # one before
    assert a.check() == [("victim", "before", 1, -1, -1)]
    a.mem[lo - 1] = NAN
    a.mem[hi] = 0                                                     # one behind: the byte after the last element
    assert a.check() == [("victim", "behind", 1, 1, 1)]
    a.mem[hi + 99] = 7
    a.mem[lo - G] = 7                                                 # the far end of the guard in front
    got = a.check()
    assert got == [("victim", "before", 1, -G, -G), ("victim", "behind", 2, 1, 100)]
    assert got[1].name == "victim" and got[1].side == "behind" and got[1].nbytes == 2 and got[1].first == 1 and got[1].last == 100
    a.mem[hi], a.mem[hi + 99], a.mem[lo - G] = NAN, NAN, NAN
    assert a.check() == []
    v.view(torch.uint8).fill_(0x55)                                   # writing the whole buffer is no violation
    assert a.check() == []


def test_a_write_with_the_poison_value_is_caught_under_another_poison():
    """One pattern alone can miss a stray store of that very byte: the tests run under three."""
    seen = []
    for fill in POISONS:
        a = _arena(fill)
        v = a.carve(3, torch.uint8)
        a.mem[v.data_ptr() - a.mem.data_ptr() + 3] = 0               # a stray zero byte behind the buffer
        seen.append(bool(a.check()))
    assert seen == [True, False, True]


def test_reset_forgets_buffers_and_repoisons():
    a = _arena(NAN)
    v = a.carve(10, torch.float32, fill=ZERO)
    p = v.data_ptr()
    a.mem[p - a.mem.data_ptr() + 40] = 3
    assert a.check()
    a.reset(BIG)
    assert a.bufs == [] and a.check() == [] and bool((a.mem == BIG).all())
    assert a.carve(10, torch.float32).data_ptr() == p                # the same carve sequence gives the same addresses


def test_full_arena_raises():
    a = Arena("cpu", guard_bytes=G, capacity_bytes=4 * G)
    a.carve(G, torch.uint8)
    with pytest.raises(MemoryError):
        a.carve(G, torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_high_water_returns_the_planted_extent(dtype):
    n = 257
    for extent in (0, 1, 3, 255, 257):
        a = _arena()
        ba, bb = a.carve(n, dtype, fill=NAN), a.carve(n, dtype, fill=BIG)
        assert high_water(ba, bb, NAN, BIG) == 0
        if extent:
            val = torch.tensor(3, dtype=dtype)
            ba[extent - 1] = val
            bb[extent - 1] = val
            ba[0] = val
        assert high_water(ba, bb, NAN, BIG) == extent
        assert max(last_written(ba, NAN), last_written(bb, BIG)) == extent          # (the form a test takes run by run)
    # a written value that EQUALS one poison is still seen through the other run
    a = _arena()
    ba, bb = a.carve(n, dtype, fill=ZERO), a.carve(n, dtype, fill=BIG)
    ba[100] = 0
    bb[100] = 0
    assert high_water(ba, bb, ZERO, BIG) == 101
    # ... and one changed byte of a wide element counts
    if dtype != torch.uint8:
        bb.view(torch.uint8)[200 * bb.element_size() + 1] = 0
        assert high_water(ba, bb, ZERO, BIG) == 201
