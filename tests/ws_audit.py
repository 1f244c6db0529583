"""Audit of one launch interval against the U-Net workspace region table (test aid; imported like guarded.py and replay_tap.py).

The workspace is ONE caller-owned buffer that make_plan cuts into regions (mpu_unet_workspace_region_info, UNet.workspace_regions):
a guard band around the whole buffer cannot see a kernel that stores one tile row past the end of its own tensor -- it lands in
the next region. With the launch tap (replay_tap.tapped) stopping the step after every launch, the bytes that changed between two
taps are compared, exactly, with what that launch may write:

  * a TENSOR or STATS byte changes only inside an output the launch declares in mpu_launch_info (declared()), clipped to the
    region the output starts in;
  * a byte of no region -- the tail between a region's unrounded length and the next multiple of 256, and everything between
    the plan's total and the end of the buffer -- never changes (gaps());
  * SCRATCH regions are free, except the 1024 trailing floats of `partial` ("partial.trailer": the fused training head alone
    writes them; it is off under a tap unless mpu_unet_set_launch_tap_fused asked for it, and then only its kind-12 interval may:
    the caller's exemption table) and, where the caller asks for it (wpartial_by_conv: ungrouped weight gradients),
    `wpartial`, which a weight-gradient launch may change only inside its own conv's slice ("wpartial.conv/<i>");
  * exemptions are whole regions that a launch of one kind may change although the tap cannot declare it (the caller's table).

Everything is plain torch on uint8 tensors and works on CPU tensors as on device ones (tests/test_ws_audit_host.py). Offsets are
bytes from the start of the buffer; a range is (lo, hi) with hi exclusive.

Coverage (class Coverage) takes two runs of the same pass on buffers poisoned with two different bytes (guarded.NAN = 0xFF and
guarded.BIG = 0x7B, as guarded.high_water): within the interval that first writes a declared output, every byte of it must differ
from the poison in at least one of the runs. A stored byte can equal one poison by chance, not both; the results are bit-identical
between the runs, so the union of the two changed-masks is the set of bytes the launch stored.
"""
from collections import namedtuple

import torch

from guarded import BIG, NAN

TENSOR, STATS, SCRATCH = 0, 1, 2                 # _lib.MPU_WS_TENSOR / _STATS / _SCRATCH (restated: the host test loads no library)
POISONS = (NAN, BIG)
BF16 = 1                                         # _lib.MPU_BF16: mpu_launch_info.dtype of a 2-byte activation

Region = namedtuple("Region", "index name offset bytes cls parent")
Finding = namedtuple("Finding", "name offset length at")
Finding.__doc__ = """A run of changed bytes nobody may write: `name` is the region (the sub-entry where there is one) or "gap",
`offset` the first byte's offset inside that region (a gap: behind the end of the region in front of it; behind the plan's total
when there is none), `length` the run's bytes, `at` its offset in the buffer."""
Declared = namedtuple("Declared", "field region lo hi clipped")
Declared.__doc__ = """An output the launch declares: mpu_launch_info field, the region it starts in, its byte range clipped to that
region and the number of bytes the declaration reaches past the region's end (0 unless the shapes and the plan disagree)."""


def top_level(regions):
    return [r for r in regions if r.parent < 0]


def by_name(regions, name):
    return [r for r in regions if r.name == name][0]


def gaps(regions, total):
    """The byte ranges of a buffer of `total` bytes that belong to no region: the round-up tails and whatever lies behind the
    last region (the plan's total .. the end of a longer buffer)."""
    out, at = [], 0
    for r in sorted(top_level(regions), key=lambda r: (r.offset, r.bytes)):
        if r.offset > at:
            out.append((at, r.offset))
        at = max(at, r.offset + r.bytes)
    if total > at:
        out.append((at, total))
    return out


def changed(prev, now):
    """bool per byte: does it differ between two uint8 snapshots of the buffer (or of the same slice of it)?"""
    assert prev.dtype == now.dtype == torch.uint8 and prev.shape == now.shape
    return prev != now


def _esz(li):
    return 2 if li.dtype == BF16 else 4


def outputs(li, n_classes=None, fused=False):
    """[(field, device pointer, bytes)]: what a launch of li.kind writes through the pointers of mpu_launch_info, sized from its
    own shapes as the replay reads them (include/mpunet_hip.h; tests/test_gpu_replay.py: _StepChecks, _replay_inference)."""
    e, px = _esz(li), li.B * li.H * li.W
    pooled = li.B * (li.H // 2) * (li.W // 2)
    k = li.kind
    out = []
    if k in (0, 8) and li.out:
        out.append(("out", li.out, px * li.Cout * e))
    if k == 1:
        out.append(("out", li.out, px * li.n_cnt * e))                   # the channel-sliced data gradient: the declared channels only
    assert k != 3 or li.out or fused, "kind 3 without an output outside the fused forms"
    if k in (4, 5, 7, 12, 13) or (k == 3 and li.out):                    # (fused: kind 3 of the fused head's BatchNorm stores no y)
        out.append(("out", li.out, px * li.C0 * e))                      # kinds 12, 13: the dz of the conv in front of the BatchNorm
    if k in (3, 11):
        if li.mask:
            out.append(("mask", li.mask, pooled * li.C0 * e))
        assert li.aux1 == li.aux0 + 4 * li.C0, "kind %d: mean and invstd are not neighbours" % k
        out.append(("aux0", li.aux0, 4 * li.C0 * 4))                     # mean, invstd and, directly behind them, scale and shift
    if k in (6, 10, 11):                                                 # (kind 11, head_bn_forward: statistics AND probabilities)
        out.append(("out", li.out, px * li.Cout * 4))
    if k == 8:
        if li.mask:
            out.append(("mask", li.mask, pooled * li.Cout * e))
        if li.dz:                                                        # the partial logits of the head that rode in the epilogue
            assert n_classes, "kind 8 with partial logits: n_classes is needed"
            out.append(("dz", li.dz, 2 * px * n_classes * 4))
    if k == 9:
        out.append(("out", li.out, pooled * li.C0 * e))
    assert k in range(14), "unknown launch kind %d" % k
    assert all(p for _f, p, _n in out), ("a declared output is NULL", k, li.conv_index)
    return out


def declared(li, regions, base, total, n_classes=None, fused=False):
    """The declared outputs of `li` that lie in the buffer starting at device pointer `base`, as Declared records. An output
    outside the buffer (the caller's own probabilities tensor) is none of the audit's business. One that starts in the buffer
    must start inside a TENSOR or STATS region and is clipped to it: what it stores past that region's end is a finding."""
    out = []
    for field, p, n in outputs(li, n_classes, fused):
        lo = p - base
        if lo < 0 or lo >= total:
            continue
        home = [r for r in regions if r.cls != SCRATCH and r.offset <= lo < r.offset + r.bytes]
        assert home, ("a declared output starts outside every TENSOR / STATS region", li.kind, li.conv_index, field, lo)
        home = max(home, key=lambda r: r.parent >= 0)        # the sub-entry where there is one ("stats.bn/<i>")
        end = home.offset + home.bytes
        out.append(Declared(field, home.name, lo, min(lo + n, end), max(0, lo + n - end)))
    return out


def free_scratch(regions, wpartial_by_conv=False):
    """The SCRATCH byte ranges every interval may change."""
    out = []
    for r in top_level(regions):
        if r.cls != SCRATCH or (wpartial_by_conv and r.name == "wpartial"):
            continue
        if r.name == "partial":
            t = by_name(regions, "partial.trailer")
            assert t.offset + t.bytes == r.offset + r.bytes
            out.append((r.offset, t.offset))
        else:
            out.append((r.offset, r.offset + r.bytes))
    return [(a, b) for a, b in out if b > a]


def allowed(li, regions, base, total, n_classes=None, exempt=(), pending_wgrad=None, wpartial_by_conv=False, fused=False):
    """The byte ranges the interval that ends at the tap of `li` may change. li None: the interval behind the last tap.
    exempt: (kind, region name, conv_index or None) triples of the caller's table; pending_wgrad: the conv whose weight gradient
    the PREVIOUS tap reported (kind 2 reports before its launch, so its stores fall into this interval)."""
    out = free_scratch(regions, wpartial_by_conv)
    if wpartial_by_conv and pending_wgrad is not None:
        s = by_name(regions, "wpartial.conv/%d" % pending_wgrad)
        out.append((s.offset, s.offset + s.bytes))
    if li is not None:
        out += [(d.lo, d.hi) for d in declared(li, regions, base, total, n_classes, fused)]
        for kind, name, index in exempt:
            if kind == li.kind and (index is None or index == li.conv_index):
                r = by_name(regions, name)
                out.append((r.offset, r.offset + r.bytes))
    return out


def watched(regions, total, wpartial_by_conv=False):
    """The complement of free_scratch in a buffer of `total` bytes, merged: the only bytes an audit has to look at."""
    out, at = [], 0
    for a, b in sorted(free_scratch(regions, wpartial_by_conv)):
        if a > at:
            out.append((at, a))
        at = max(at, b)
    if total > at:
        out.append((at, total))
    return out


def _name_of(regions, plan_total, p):
    """(region or sub-entry name or "gap", offset inside it) of buffer offset p."""
    hit = [r for r in regions if r.offset <= p < r.offset + r.bytes]
    if hit:
        r = max(hit, key=lambda r: r.parent >= 0)            # the sub-entry where there is one
        return r.name, p - r.offset, r.offset + r.bytes
    if p >= plan_total:
        return "gap", p - plan_total, None
    front = max((r for r in top_level(regions) if r.offset + r.bytes <= p), key=lambda r: r.offset + r.bytes)
    return "gap", p - (front.offset + front.bytes), front.offset + (front.bytes + 255) // 256 * 256


def audit_interval(prev, now, allow, regions, plan_total, watch=None):
    """Every changed byte of the buffer outside `allow`, as Finding runs ([] = a clean interval). prev / now: uint8 snapshots of
    the whole buffer (it may be longer than the plan: the rest is a gap); watch: the ranges to look at (default: everything)."""
    n = now.numel()
    watch = [(0, n)] if watch is None else watch
    masks = []
    for lo, hi in watch:
        ch = changed(prev[lo:hi], now[lo:hi])
        for a, b in allow:
            a, b = max(a, lo), min(b, hi)
            if a < b:
                ch[a - lo:b - lo] = False
        masks.append(ch)
    if not masks or not bool(torch.stack([m.any() for m in masks]).any()):
        return []
    out = []
    for (lo, _hi), ch in zip(watch, masks):
        idx = ch.nonzero().flatten().cpu()
        if not idx.numel():
            continue
        idx = idx + lo
        cut = (idx[1:] != idx[:-1] + 1).nonzero().flatten() + 1                  # a run ends where the offsets stop being neighbours
        starts = torch.cat([idx[:1], idx[cut]]).tolist()
        ends = torch.cat([idx[cut - 1], idx[-1:]]).tolist()
        for s, e in zip(starts, ends):
            while s <= e:                                                        # (a run is cut where the region under it changes)
                name, off, end = _name_of(regions, plan_total, s)
                stop = e if end is None else min(e, end - 1)
                out.append(Finding(name, off, stop - s + 1, s))
                s = stop + 1
    return out


class Coverage:
    """First writes of declared outputs over two poison runs. add(run, key, mask): the changed-mask of the output inside the
    interval that first declares its region, run 0 then run 1 with the same keys in the same order; missing(): per output that
    some byte of was stored in neither run, (key, unwritten bytes, offset of the first one inside the output)."""

    def __init__(self):
        self.masks, self.order, self.seen = {}, ([], []), (set(), set())

    def first_write(self, run, region):
        """True once per run and region: is this the first interval of the run that declares an output in `region`?"""
        if region in self.seen[run]:
            return False
        self.seen[run].add(region)
        return True

    def add(self, run, key, mask):
        self.order[run].append(key)
        if run == 0:
            assert key not in self.masks, key
            self.masks[key] = mask.clone()
        else:
            assert key in self.masks and self.masks[key].shape == mask.shape, ("the second run declares another output", key)
            self.masks[key] |= mask

    def missing(self):
        assert self.order[0] == self.order[1], "the two poison runs declared different outputs"
        out = []
        for key in self.order[0]:
            hole = ~self.masks[key]
            if bool(hole.any()):
                out.append((key, int(hole.sum()), int(hole.nonzero()[0])))
        return out
