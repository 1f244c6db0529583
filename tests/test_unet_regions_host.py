"""Host arithmetic of the workspace region table (no GPU): mpu_unet_workspace_region_info over the sweep of
tests/test_unet_plan_host.py -- depth 1..6, f32 / bf16 / bf16x3, complexity factor 0.25 and 1, 3 and 12 classes with the sparse
cross-entropy and 3 classes with the Dice loss, batch 1 and 3. The table is a read-only view of make_plan (the golden file of
test_unet_plan_host.py pins that no offset moved): the top-level regions tile [0, mpu_unet_workspace_bytes) in 256-byte steps
without aliasing, sub-entries lie inside their parent without overlapping, and the number of regions follows from the depth,
the dtype and the loss alone."""
import ctypes as C

import numpy as np
import pytest

from multiplanarunet_amd import _lib
from test_unet_plan_host import DTYPES, HEADS

ALIGN = 256


def _handle(depth, dtype, cf, K, loss):
    lib = _lib.load()
    cfg = _lib.UNetConfig()
    cfg.n_classes, cfg.n_channels, cfg.depth, cfg.H, cfg.W = K, 1, depth, 64, 64
    cfg.dtype, cfg.softmax = dtype, 1
    for l in range(depth + 1):
        cfg.filters[l] = int(64 * (2 ** l) * np.sqrt(cf))
    h = C.c_void_p(lib.mpu_unet_create(C.byref(cfg)))
    assert h, lib.mpu_last_error()
    if loss == "dice":
        lc = _lib.LossConfig()
        lc.kind, lc.smooth = _lib.MPU_LOSS_DICE, 1.0
        _lib.call("mpu_unet_set_loss", h, C.byref(lc))
    return h


def _sweep():
    lib = _lib.load()
    for depth in range(1, 7):
        for dname, dtype in DTYPES:
            for cf in (0.25, 1):
                for K, loss in HEADS:
                    h = _handle(depth, dtype, cf, K, loss)
                    try:
                        for B in (1, 3):
                            yield ("d%d %s cf%g K%d %s B%d" % (depth, dname, cf, K, loss, B), h, B, depth, dname, loss,
                                   _lib.workspace_regions(h, B))
                    finally:
                        lib.mpu_unet_destroy(h)


def _roundup(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def test_top_level_regions_tile_the_workspace_and_sub_entries_stay_inside_their_parent():
    lib = _lib.load()
    n_cases = 0
    for tag, h, B, depth, dname, loss, regs in _sweep():
        n_cases += 1
        assert [r.index for r in regs] == list(range(len(regs))), tag
        top = [r for r in regs if r.parent < 0]
        assert len({r.name for r in regs}) == len(regs), (tag, "names repeat")
        # sorted, aligned, pairwise disjoint, gap-free up to the 256-byte round-up, and ending at the plan's total
        assert top[0].offset == 0, tag
        for a, b in zip(top, top[1:]):
            assert a.offset < b.offset or (a.bytes == 0 and a.offset == b.offset), (tag, a, b)
            assert a.offset + _roundup(a.bytes) == b.offset, (tag, a, b)
        for i, a in enumerate(top):
            assert a.offset % ALIGN == 0 and a.bytes >= 0 and a.cls in (_lib.MPU_WS_TENSOR, _lib.MPU_WS_STATS, _lib.MPU_WS_SCRATCH), (tag, a)
            for b in top[i + 1:]:                           # (pairwise, not only neighbours: the plan could in principle go backwards)
                assert a.offset + a.bytes <= b.offset, (tag, a, b)
        assert top[-1].offset + _roundup(top[-1].bytes) == lib.mpu_unet_workspace_bytes(h, B), tag
        by = {r.name: r for r in regs}
        assert by["probs"].offset == lib.mpu_unet_workspace_probs_offset(h, B), tag
        assert by["loss_mean"].offset == lib.mpu_unet_workspace_loss_mean_offset(h, B), tag
        # sub-entries: behind their parent in the list, the parent's class, inside its unrounded extent, disjoint among siblings
        kids = {}
        for r in regs:
            if r.parent >= 0:
                p = regs[r.parent]
                assert p.parent < 0 and r.parent < r.index and r.cls == p.cls and r.name.startswith(p.name + "."), (tag, r, p)
                assert p.offset <= r.offset and r.offset + r.bytes <= p.offset + p.bytes and r.bytes > 0, (tag, r, p)
                kids.setdefault(p.name, []).append(r)
        for name, ks in kids.items():
            ks = sorted(ks, key=lambda r: r.offset)
            for a, b in zip(ks, ks[1:]):
                assert a.offset + a.bytes <= b.offset, (tag, a, b)
            if name in ("partial", "wpartial", "bnacc", "stats"):           # these are made of their parts, nothing else
                assert sum(k.bytes for k in ks) == by[name].bytes, (tag, name)
        assert by["partial.trailer"].bytes == 4096 and by["partial.trailer"].offset + 4096 == by["partial"].offset + by["partial"].bytes, tag
    assert n_cases == 6 * 3 * 2 * 3 * 2


def test_region_classes_and_counts_follow_from_depth_dtype_and_loss():
    T, S, X = _lib.MPU_WS_TENSOR, _lib.MPU_WS_STATS, _lib.MPU_WS_SCRATCH
    counts = {}
    for tag, h, B, D, dname, loss, regs in _sweep():
        n_conv, n_bn = 5 * D + 2, 3 * D + 1                 # convs with a weight-gradient (all but the 1x1 head) / BatchNorms
        top = [r for r in regs if r.parent < 0]
        names = [r.name for r in top]
        stem = lambda r: r.name.split("/")[0].split(".")[0]
        for r in regs:
            want = T if stem(r) in ("act", "dz", "probs", "loss_mean", "gA", "gB") else S if stem(r) == "stats" else X
            assert r.cls == want, (tag, r)
        x3, per_image = dname == "bf16x3", loss == "dice"
        n_act = 1 + 5 * D + 3 + 5 * D                       # input; C1 C2 N P dskip per level; bottom; U1 N1 C2u C3u N2 per block
        assert sum(n.startswith("act/") for n in names) == n_act, tag
        assert sorted(n for n in names if n.startswith("dz/")) == sorted("dz/%d" % i for i in range(n_conv)), tag
        assert sum(n.startswith("x3x0/") for n in names) == sum(n.startswith("x3dz/") for n in names) == (n_conv if x3 else 0), tag
        assert sum(n.startswith("x3x1/") for n in names) == (D if x3 else 0), tag                 # the concat conv of every up block
        assert (names[-2:] == ["loss_scratch", "loss_coef"]) == per_image, tag
        assert ("loss_scratch" in names or "loss_coef" in names) == per_image, tag
        fixed = ["probs", "loss_mean", "gA", "gB", "partial", "partial2", "wpartial", "cpartial", "bnacc", "coeffs", "stats"]
        assert all(names.count(n) == 1 for n in fixed), tag
        assert len(top) == n_act + n_conv + len(fixed) + (2 * n_conv + D if x3 else 0) + (2 if per_image else 0), tag
        sub = [r.name for r in regs if r.parent >= 0]
        assert sorted(n for n in sub if n.startswith("wpartial.")) == sorted("wpartial.conv/%d" % i for i in range(n_conv)), tag
        for half in ("fwd", "bwd"):
            assert sorted(n for n in sub if n.startswith("bnacc.%s/" % half)) == sorted("bnacc.%s/%d" % (half, i) for i in range(n_bn)), tag
        assert sorted(n for n in sub if n.startswith("bnacc.db/")) == (sorted("bnacc.db/%d" % i for i in range(n_conv)) if x3 else []), tag
        assert sorted(n for n in sub if n.startswith("stats.")) == sorted("stats.bn/%d" % i for i in range(n_bn)), tag
        assert len(sub) == 2 + n_conv + 2 * n_bn + (n_conv if x3 else 0) + n_bn, tag
        counts[tag] = len(top)
    # a per-image loss adds exactly the two loss regions, and moves nothing in front of them
    for tag in counts:
        if " K3 ce " in tag:
            assert counts[tag.replace(" K3 ce ", " K3 dice ")] == counts[tag] + 2, tag


def test_per_image_loss_regions_come_last_and_leave_every_other_record_alone():
    for dname, dtype in DTYPES:
        a, b = _handle(2, dtype, 1, 3, "ce"), _handle(2, dtype, 1, 3, "dice")
        try:
            ra, rb = _lib.workspace_regions(a, 3), _lib.workspace_regions(b, 3)
            assert rb[:len(ra)] == ra and [r.name for r in rb[len(ra):]] == ["loss_scratch", "loss_coef"], dname
        finally:
            _lib.load().mpu_unet_destroy(a)
            _lib.load().mpu_unet_destroy(b)


def test_region_query_rejects_bad_arguments():
    lib = _lib.load()
    h = _handle(1, _lib.MPU_BF16, 1, 3, "ce")
    try:
        n = lib.mpu_unet_workspace_num_regions(h, 2)
        assert n > 0 and lib.mpu_unet_workspace_num_regions(h, 0) == 0 and lib.mpu_unet_workspace_num_regions(None, 2) == 0
        name = C.create_string_buffer(64)
        o, nb, c, p = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        for idx in (-1, n):
            assert lib.mpu_unet_workspace_region_info(h, 2, idx, name, 64, C.byref(o), C.byref(nb), C.byref(c), C.byref(p)) != 0
        with pytest.raises(_lib.MpuError):
            _lib.call("mpu_unet_workspace_region_info", h, 0, 0, name, 64, C.byref(o), C.byref(nb), C.byref(c), C.byref(p))
        short = C.create_string_buffer(4)                   # a short name buffer truncates, NUL-terminated
        assert lib.mpu_unet_workspace_region_info(h, 2, 0, short, 4, C.byref(o), C.byref(nb), C.byref(c), C.byref(p)) == 0
        assert short.value == b"act"
    finally:
        lib.mpu_unet_destroy(h)
