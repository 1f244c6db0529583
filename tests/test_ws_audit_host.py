"""The workspace audit helper (tests/ws_audit.py) on CPU tensors, no GPU and no library: every kind of finding the device tests
rely on is shown to FAIL here on a small hand-made region table, in the manner of tests/test_guarded_host.py, and a clean
interval is shown to pass.

  act/a     [   0,  512)  TENSOR                         gA       [1024, 2048)  TENSOR
  act/b     [ 512,  812)  TENSOR, tail gap [812, 1024)   partial  [2048, 6400)  SCRATCH: rows [2048, 2304) + trailer [2304, 6400)
  wpartial  [6400, 6912)  SCRATCH: conv/0 [6400, 6656), conv/1 [6656, 6912)
  stats     [6912, 6976)  STATS: bn/0 (C = 4), tail gap [6976, 7168); plan total 7168, buffer 7168 + 256
"""
from types import SimpleNamespace

import pytest
import torch

import ws_audit as A
from ws_audit import Finding, Region, SCRATCH, STATS, TENSOR

BASE, TOTAL, BUF = 0x10000, 7168, 7168 + 256
REGIONS = [
    Region(0, "act/a", 0, 512, TENSOR, -1),
    Region(1, "act/b", 512, 300, TENSOR, -1),
    Region(2, "gA", 1024, 1024, TENSOR, -1),
    Region(3, "partial", 2048, 4352, SCRATCH, -1),
    Region(4, "partial.rows", 2048, 256, SCRATCH, 3),
    Region(5, "partial.trailer", 2304, 4096, SCRATCH, 3),
    Region(6, "wpartial", 6400, 512, SCRATCH, -1),
    Region(7, "wpartial.conv/0", 6400, 256, SCRATCH, 6),
    Region(8, "wpartial.conv/1", 6656, 256, SCRATCH, 6),
    Region(9, "stats", 6912, 64, STATS, -1),
    Region(10, "stats.bn/0", 6912, 64, STATS, 9),
]


def launch(kind, **kw):
    """A stand-in for mpu_launch_info: bf16, 1 x 4 x 4 pixels; pointers are BASE + a region's offset."""
    f = dict(kind=kind, conv_index=0, mode=0, dtype=A.BF16, B=1, H=4, W=4, C0=0, C1=0, Cout=0, n_off=0, n_cnt=0, relu=0,
             in0=None, in1=None, dz=None, mask=None, out=None, w_off=0, b_off=0, aux0=None, aux1=None)
    f.update(kw)
    return SimpleNamespace(**f)


CONV_A = launch(0, Cout=16, out=BASE + 0)                    # a forward conv that declares all 512 bytes of act/a
HEAD_BWD = launch(7, C0=8, out=BASE + 1024)                  # a head backward that declares the first 256 bytes of gA


def buffers(fill=A.NAN):
    prev = torch.full((BUF,), fill, dtype=torch.uint8)
    return prev, prev.clone()


def audit(li, prev, now, **kw):
    return A.audit_interval(prev, now, A.allowed(li, REGIONS, BASE, BUF, **kw), REGIONS, TOTAL)


def test_gaps_are_the_round_up_tails_and_the_rest_of_the_buffer():
    assert A.gaps(REGIONS, BUF) == [(812, 1024), (6976, BUF)]
    assert A.gaps(REGIONS, TOTAL) == [(812, 1024), (6976, TOTAL)]
    assert A.watched(REGIONS, BUF) == [(0, 2048), (2304, 6400), (6912, BUF)]
    assert A.watched(REGIONS, BUF, wpartial_by_conv=True) == [(0, 2048), (2304, BUF)]


def test_clean_interval_passes():
    prev, now = buffers()
    now[0:512] = 1                                           # the declared output, all of it
    now[2048:2304] = 2                                       # free scratch
    now[6400:6912] = 3
    assert audit(CONV_A, prev, now) == []
    assert audit(None, prev, prev.clone()) == []             # nothing changed behind the last tap
    bn = launch(3, C0=4, out=BASE + 512, aux0=BASE + 6912, aux1=BASE + 6912 + 16)       # y = act/b's first 128 bytes; 4 C floats of stats
    prev, now = buffers()
    now[512:640] = 1
    now[6912:6976] = 2
    assert audit(bn, prev, now) == []
    assert [d[:4] for d in A.declared(bn, REGIONS, BASE, BUF)] == [("out", "act/b", 512, 640), ("aux0", "stats.bn/0", 6912, 6976)]


def test_fused_kinds_declare_their_writes():
    """Kinds 11-13 (mpu_unet_set_launch_tap_fused): head_bn_forward declares the statistics and the probabilities, the kind-3
    record of its BatchNorm (out = NULL) the statistics alone, kinds 12 and 13 the dz tensor; the trailer of `partial` is the
    kind-12 interval's by exemption only."""
    st = dict(aux0=BASE + 6912, aux1=BASE + 6912 + 16)
    fwd = launch(11, C0=4, Cout=3, out=BASE + 1024, **st)               # probabilities: 16 pixels x 3 classes x 4 bytes in "gA"
    assert [d[:4] for d in A.declared(fwd, REGIONS, BASE, BUF)] == [("aux0", "stats.bn/0", 6912, 6976), ("out", "gA", 1024, 1216)]
    assert [d[:4] for d in A.declared(launch(3, C0=4, **st), REGIONS, BASE, BUF, fused=True)] == [("aux0", "stats.bn/0", 6912, 6976)]
    with pytest.raises(AssertionError, match="outside the fused forms"):
        A.declared(launch(3, C0=4, **st), REGIONS, BASE, BUF)
    prev, now = buffers()
    now[1024:1216] = 1
    now[6912:6976] = 2
    assert audit(fwd, prev, now) == [] and audit(launch(3, C0=4, **st), prev, now, fused=True) == [Finding("gA", 0, 192, 1024)]
    for kind in (12, 13):
        bwd = launch(kind, C0=8, Cout=3, out=BASE + 0)
        assert [d[:4] for d in A.declared(bwd, REGIONS, BASE, BUF)] == [("out", "act/a", 0, 256)]
        prev, now = buffers()
        now[0:256] = 1
        now[2304:2304 + 64] = 3                                         # T of the fused head in the trailer
        assert audit(bwd, prev, now) == [Finding("partial.trailer", 0, 64, 2304)]
        assert audit(bwd, prev, now, exempt=[(kind, "partial.trailer", None)]) == []


def test_one_byte_into_a_gap_fails():
    prev, now = buffers()
    now[0:512] = 1
    now[817] = 0
    assert audit(CONV_A, prev, now) == [Finding("gap", 5, 1, 817)]


def test_one_byte_into_the_neighbouring_region_fails():
    prev, now = buffers()
    now[0:513] = 1                                           # 512 declared bytes and the first byte of act/b
    assert audit(CONV_A, prev, now) == [Finding("act/b", 0, 1, 512)]


def test_write_inside_ga_past_the_declared_extent_fails():
    prev, now = buffers()
    now[1024:1024 + 256] = 1
    assert audit(HEAD_BWD, prev, now) == []
    now[1024 + 300:1024 + 303] = 1
    assert audit(HEAD_BWD, prev, now) == [Finding("gA", 300, 3, 1324)]


def test_write_to_an_undeclared_tensor_region_fails():
    prev, now = buffers()
    now[0:512] = 1
    now[522:532] = 1
    now[540] = 1
    assert audit(CONV_A, prev, now) == [Finding("act/b", 10, 10, 522), Finding("act/b", 28, 1, 540)]
    now = prev.clone()
    now[6912] = 0                                            # ... and so does a STATS byte nobody declared
    assert audit(CONV_A, prev, now) == [Finding("stats.bn/0", 0, 1, 6912)]


def test_byte_past_the_plan_total_fails():
    prev, now = buffers()
    now[TOTAL + 3] = 0
    assert audit(None, prev, now) == [Finding("gap", 3, 1, TOTAL + 3)]
    now = prev.clone()
    now[6970:7000] = 0                                       # one run over the end of a region: cut where the name changes
    assert audit(None, prev, now) == [Finding("stats.bn/0", 58, 6, 6970), Finding("gap", 0, 24, 6976)]


def test_partial_trailer_is_not_free_scratch():
    prev, now = buffers()
    now[2304 + 8] = 0
    assert audit(CONV_A, prev, now) == [Finding("partial.trailer", 8, 1, 2312)]


def test_ungrouped_weight_gradient_may_only_change_its_own_slice_of_wpartial():
    prev, now = buffers()
    now[6656:6700] = 1                                       # conv 1's slice
    assert audit(CONV_A, prev, now) == []                    # grouped: wpartial is free
    assert audit(CONV_A, prev, now, wpartial_by_conv=True, pending_wgrad=1) == []
    assert audit(CONV_A, prev, now, wpartial_by_conv=True, pending_wgrad=0) == [Finding("wpartial.conv/1", 0, 44, 6656)]
    assert audit(CONV_A, prev, now, wpartial_by_conv=True) == [Finding("wpartial.conv/1", 0, 44, 6656)]


def test_exemptions_name_a_kind_a_region_and_optionally_an_index():
    prev, now = buffers()
    now[1024:1028] = 0
    assert audit(CONV_A, prev, now) == [Finding("gA", 0, 4, 1024)]
    assert audit(CONV_A, prev, now, exempt=[(0, "gA", None)]) == []
    assert audit(CONV_A, prev, now, exempt=[(0, "gA", 0)]) == []
    assert audit(CONV_A, prev, now, exempt=[(0, "gA", 1)]) == [Finding("gA", 0, 4, 1024)]
    assert audit(CONV_A, prev, now, exempt=[(7, "gA", None)]) == [Finding("gA", 0, 4, 1024)]


def test_declaration_past_the_end_of_its_region_is_clipped_and_what_lands_behind_it_is_a_finding():
    wide = launch(0, Cout=16, out=BASE + 512)                # 512 declared bytes from the start of the 300-byte act/b
    d, = A.declared(wide, REGIONS, BASE, BUF)
    assert d == A.Declared("out", "act/b", 512, 812, 212)
    prev, now = buffers()
    now[512:1024] = 1
    assert audit(wide, prev, now) == [Finding("gap", 0, 212, 812)]
    outside = launch(6, Cout=3, out=0x900000)                # the caller's own probabilities tensor: not in the buffer
    assert A.declared(outside, REGIONS, BASE, BUF) == []
    with pytest.raises(AssertionError):
        A.declared(launch(0, Cout=16, out=BASE + 900), REGIONS, BASE, BUF)       # an output that starts in a gap


def test_watch_ranges_give_the_findings_of_the_whole_buffer():
    prev, now = buffers()
    now[0:513] = 1
    now[2100] = 1                                            # free scratch: outside every watched range
    now[2312] = 1
    now[TOTAL + 9] = 1
    allow = A.allowed(CONV_A, REGIONS, BASE, BUF)
    want = [Finding("act/b", 0, 1, 512), Finding("partial.trailer", 8, 1, 2312), Finding("gap", 9, 1, TOTAL + 9)]
    assert A.audit_interval(prev, now, allow, REGIONS, TOTAL) == want
    assert A.audit_interval(prev, now, allow, REGIONS, TOTAL, watch=A.watched(REGIONS, BUF)) == want


def _first_write(cov, run, fill, stored, n_written=512):
    """One poison run of a launch that declares act/a and stores `stored` into its first n_written bytes."""
    prev, now = buffers(fill)
    now[0:n_written] = stored[:n_written]
    d, = A.declared(CONV_A, REGIONS, BASE, BUF)
    assert cov.first_write(run, d.region) and not cov.first_write(run, d.region)
    cov.add(run, (0, d.field, d.region), A.changed(prev[d.lo:d.hi], now[d.lo:d.hi]))


def test_coverage_needs_both_poisons_to_tell_a_stored_tail_from_an_unwritten_one():
    stored = (torch.arange(512) % 7 + 1).to(torch.uint8)
    stored[500:] = A.NAN                                     # the last 12 stored bytes EQUAL the first poison
    # (a) all 512 bytes stored: under 0xFF alone the tail looks unwritten, the 0x7B run shows that it was stored
    cov = A.Coverage()
    _first_write(cov, 0, A.NAN, stored)
    assert not bool(cov.masks[(0, "out", "act/a")][500:].any())
    _first_write(cov, 1, A.BIG, stored)
    assert cov.missing() == []
    # (b) the same values but the tail is NOT stored: under 0xFF alone (a) and (b) look the same; the second poison reveals (b)
    cov = A.Coverage()
    _first_write(cov, 0, A.NAN, stored, n_written=500)
    mask_a = cov.masks[(0, "out", "act/a")].clone()
    _first_write(cov, 1, A.BIG, stored, n_written=500)
    assert cov.missing() == [((0, "out", "act/a"), 12, 500)]
    cov_full = A.Coverage()
    _first_write(cov_full, 0, A.NAN, stored)
    assert torch.equal(mask_a, cov_full.masks[(0, "out", "act/a")])
    # (c) one unwritten byte in the middle, values that equal neither poison
    cov = A.Coverage()
    for run, fill in enumerate(A.POISONS):
        prev, now = buffers(fill)
        now[0:512] = 5
        now[77] = fill
        cov.first_write(run, "act/a")
        cov.add(run, (0, "out", "act/a"), A.changed(prev[0:512], now[0:512]))
    assert cov.missing() == [((0, "out", "act/a"), 1, 77)]


def test_coverage_refuses_runs_that_declare_different_outputs():
    cov = A.Coverage()
    cov.add(0, (0, "out", "act/a"), torch.ones(4, dtype=torch.bool))
    with pytest.raises(AssertionError):
        cov.add(1, (0, "out", "act/b"), torch.ones(4, dtype=torch.bool))
    cov = A.Coverage()
    cov.add(0, (0, "out", "act/a"), torch.ones(4, dtype=torch.bool))
    with pytest.raises(AssertionError):
        cov.missing()                                        # the second run never came
