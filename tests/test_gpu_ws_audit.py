"""
Every launch's writes against the U-Net workspace region table. The guard bands (test_gpu_guard_unet.py)
see the workspace as one buffer and the replay (test_gpu_replay.py) looks at a launch's declared output alone: a kernel that
stores a tile row, a channel group or a partial copy past the end of its own tensor lands in the NEXT REGION of the same buffer,
which is neither. Here the launch tap stops the pass after every launch and the bytes that changed since the previous tap are
compared, exactly, with what that launch may write (tests/ws_audit.py; host test: tests/test_ws_audit_host.py):

  * no byte outside every region changes (256-byte round-up tails; 4 KiB of slack behind the plan's total; the arena's guards);
  * a TENSOR or STATS byte changes only inside an output the interval's launch declares in mpu_launch_info, sized as the replay
    reads it; inside gA / gB nothing changes past the declared extent;
  * SCRATCH is free, but the 1024 trailing floats of `partial` never change under a tap and, with ungrouped weight gradients, a
    weight-gradient launch changes `wpartial` only inside its own conv's slice. A kind-2 tap reports BEFORE its launch, so that
    launch's stores fall into the interval the next tap (or the end of the pass) closes: the slice is allowed there;
  * EXEMPT lists the writes the tap cannot declare, by (kind, region), each with its reason; every entry must be seen used;
  * over two runs on buffers poisoned with 0xFF and 0x7B, the interval that first declares an output of a region stores every
    byte of that output (later rewrites of gA / gB get the subset rule alone);
  * the intervals are the launches train_step_launch_counts (test_gpu_replay.py) gives for the depth, plus the one behind the
    last tap (deferred grouped weight gradients and reductions).

Cases: T1-T4 (test_gpu_replay.TRAIN_NETS) in bf16 and bf16x3 and T1 in f32; T3 bf16 under the step's three schedule switch sets
(a fresh interpreter each); T3 in bf16 and bf16x3 with the fused forms on (mpu_unet_set_launch_tap_fused, MPU_POOL_BWD_RECOMPUTE=2:
the fused head's kinds 11 / 12 and the pool recompute's kind 13 on both encoder levels; a fresh interpreter each); the inference forward of networks A-D (INFER_NETS) in bf16, A also under its three switch sets; and
one UNTAPPED train_step per network, where the fused training head and the pool-backward recompute run.
"""
import collections
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import guarded
import ws_audit as A
from test_gpu_replay import INFER_NETS, TRAIN_NETS, _assert_t3_schedule, _env_on, _train_case, quiet, train_step_launch_counts

pytestmark = pytest.mark.gpu
SLACK = 4096                    # bytes of the carved buffer behind the plan's total: a gap like any other

# Writes the tap cannot declare: (kind, region) -> (conv_index of the launch, passes that must use it, reason). No wildcards.
EXEMPT = {
    (0, "act/xin"): (0, ("train", "train_fused", "infer"), "the cast and channel padding of the input batch is an unreported launch in front of the first conv"),
    (7, "loss_mean"): (-1, ("train",), "the head backward stores the pass's mean loss (one float) beside its declared dn"),
    # (with the fused forms on: T3, the one net audited with them; the launch's index is its last BatchNorm's, 3 * depth = 6)
    (12, "loss_mean"): (6, ("train_fused",), "head_bn_backward stores the pass's mean loss (one float), as the unfused head backward does"),
    (12, "partial.trailer"): (6, ("train_fused",), "T [64][K] of the fused head: the finalizer of head_bn_backward writes it behind the partial rows, head_bn_bwd_apply reads it"),
}


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def _carve_workspace(m, B, fill):
    """The model's workspace as a poisoned view of a guarded arena, SLACK bytes longer than the plan."""
    from multiplanarunet_amd import _lib
    total = int(_lib.load().mpu_unet_workspace_bytes(m._h, B))
    arena = guarded.arena(__name__, total + SLACK, 1, fill)
    m._ws, m._ws_batch = arena.carve(total + SLACK, torch.uint8, name="workspace"), B
    return arena, m._ws, total


class Auditor:
    """The check of replay_tap.tapped (on_launch) and the interval behind the last tap (close)."""

    def __init__(self, m, B, fill, run, cov, passes, wpartial_by_conv=False):
        self.arena, self.ws, self.total = _carve_workspace(m, B, fill)
        self.regions = m.workspace_regions(B)
        self.m, self.run, self.cov, self.by_conv, self.fused = m, run, cov, wpartial_by_conv, passes == "train_fused"
        self.prev = self.ws.clone()
        self.watch = A.watched(self.regions, self.ws.numel(), wpartial_by_conv)
        self.exempt = [(k, name, idx) for (k, name), (idx, ps, _why) in EXEMPT.items() if passes in ps]
        self.used, self.kinds, self.n, self.pending, self.fused_head = set(), [], 0, None, False

    def on_launch(self, li):
        self._close(li)

    def close(self):
        torch.cuda.synchronize()
        self._close(None)
        assert not self.arena.check(), self.arena.check()

    def _close(self, li):
        ws, prev, base, n = self.ws, self.prev, self.ws.data_ptr(), self.ws.numel()
        what = "interval %d (%s)" % (self.n, "behind the last tap" if li is None else "kind %d, index %d" % (li.kind, li.conv_index))
        try:
            decl = [] if li is None else A.declared(li, self.regions, base, n, self.m.n_classes, self.fused)
            allow = A.allowed(li, self.regions, base, n, self.m.n_classes, self.exempt, self.pending, self.by_conv, self.fused)
            for d in decl:                                   # coverage of first writes, before `prev` moves on
                if self.cov.first_write(self.run, d.region):
                    self.cov.add(self.run, (self.n, d.field, d.region), A.changed(prev[d.lo:d.hi], ws[d.lo:d.hi]))
            for k, name, idx in self.exempt:
                if li is not None and k == li.kind and idx in (None, li.conv_index):
                    r = A.by_name(self.regions, name)
                    if bool(A.changed(prev[r.offset:r.offset + r.bytes], ws[r.offset:r.offset + r.bytes]).any()):
                        self.used.add((k, name))
            found = A.audit_interval(prev, ws, allow, self.regions, self.total, self.watch)
            clipped = [d for d in decl if d.clipped]
            assert not found and not clipped, "%s: %d stray runs, the first %s; declared outputs reaching past their region: %s" \
                % (what, len(found), found[:6], clipped)
        finally:
            prev.copy_(ws)
            self.n += 1
            if li is not None:
                self.kinds.append(li.kind)
                self.fused_head = self.fused_head or (li.kind == 8 and bool(li.dz))
            self.pending = li.conv_index if li is not None and li.kind == 2 else None


def _finish(cov, tag, dtype, t0, auds, extra=""):
    missing = cov.missing()
    assert not missing, "first writes that leave bytes of their declared output unwritten (key, bytes, first offset): %s" % missing[:6]
    a = auds[0]
    print("ws audit (%s, %s): %d intervals, %d regions, %.0f MB workspace of which %.0f MB watched, %d first writes covered%s; %.1f s"
          % (tag, dtype, a.n, len(a.regions), a.total / 1e6, sum(hi - lo for lo, hi in a.watch) / 1e6, len(cov.order[0]), extra,
             time.time() - t0))


# ---- tapped train step ------------------------------------------------------------------------------------------------------------
def _audit_train_step(net, dtype, fused_levels=None):
    """fused_levels = n: with the fused forms on (mpu_unet_set_launch_tap_fused): the fused head and n recomputed encoder levels."""
    from multiplanarunet_amd import _lib
    from replay_tap import tapped
    t0 = time.time()
    K, C, depth, cf, B, H, W = TRAIN_NETS[net]
    by_conv = not (_env_on("MPU_WGRAD_GROUP") or _env_on("MPU_WGRAD_BATCHED_REDUCE"))      # every weight gradient its own launch
    want = {k: v for k, v in train_step_launch_counts(depth, fused_levels).items() if v}
    passes = "train" if fused_levels is None else "train_fused"
    cov, auds, lines = A.Coverage(), [], None
    for run, fill in enumerate(A.POISONS):
        m, x, y, sw = _train_case(K, C, depth, cf, B, H, W, dtype, seed=51, sw_period=2)
        _lib.call("mpu_unet_set_launch_tap_fused", m._h, int(fused_levels is not None))
        aud = Auditor(m, B, fill, run, cov, passes, by_conv)
        auds.append(aud)
        with tapped(m, aud.on_launch, schedule_log=True) as tap:
            m.forward_backward(x, y, sw)
            torch.cuda.synchronize()
        aud.close()
        lines = tap.log.splitlines()
        assert tap.launches == aud.n - 1 == sum(want.values()), (tap.launches, aud.n, want)
        assert dict(collections.Counter(aud.kinds)) == want, (collections.Counter(aud.kinds), want)
        assert aud.used == {k for k, (_i, ps, _w) in EXEMPT.items() if passes in ps}, ("exemptions used", aud.used)
        t = A.by_name(aud.regions, "partial.trailer")       # (the audit held it interval by interval; the sum of it)
        assert bool((aud.ws[t.offset:t.offset + t.bytes] == fill).all()) == (fused_levels is None)
    assert auds[0].kinds == auds[1].kinds
    _finish(cov, net, dtype, t0, auds, "; wpartial by conv: %s" % ("on" if by_conv else "off"))
    return lines


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
@pytest.mark.parametrize("net", ["T1", "T2", "T3", "T4"])
def test_train_step_writes_stay_in_declared_regions(net, dtype):
    lines = _audit_train_step(net, dtype)
    if net == "T3" and dtype == "bf16":
        _assert_t3_schedule(lines)


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_train_step_t3_fused_forms_writes_stay_in_declared_regions(dtype):
    """T3 with the fused training head (kinds 11, 12) and the pool-backward recompute on both encoder levels (kind 13): the forms
    the benchmarked step takes. MPU_POOL_BWD_RECOMPUTE=2 (T3's levels are below the default's size threshold) is read once per
    process: a fresh interpreter, with a timeout, unless this one already has it."""
    if os.environ.get("MPU_POOL_BWD_RECOMPUTE") == "2":
        lines = _audit_train_step("T3", dtype, fused_levels=2)
        assert sum("head=1" in l for l in lines) == 2 and sum(l.startswith("bn_fold bwd") and "pool=1" in l for l in lines) == 2, lines
        return
    k = "test_train_step_t3_fused_forms_writes_stay_in_declared_regions and %s" % (dtype if dtype == "bf16x3" else "bf16 and not bf16x3")
    _subprocess(k, {"MPU_POOL_BWD_RECOMPUTE": "2"}, "ws audit (", timeout=600)


def test_train_step_t1_f32_writes_stay_in_declared_regions():
    _audit_train_step("T1", "f32")


def _subprocess(k, switches, prefix, timeout=None):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k", k],
                       env=dict(os.environ, **switches), capture_output=True, text=True, cwd=os.path.dirname(here), timeout=timeout)
    out = "\n".join(l for l in r.stdout.splitlines() if l.startswith(prefix))
    print(out)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]
    return out


@pytest.mark.parametrize("switches", [{"MPU_BN_ATOMIC": "0"},
                                      {"MPU_FUSED_BN_STATS": "0", "MPU_FUSED_BN_BWD_CONV": "0", "MPU_FUSED_BN_BWD": "0"},
                                      {"MPU_WGRAD_GROUP": "0", "MPU_WGRAD_BATCHED_REDUCE": "0"}],
                         ids=["partial_rows", "colreduce_sums", "ungrouped_wgrad"])
def test_train_net_t3_audit_under_schedule_switches_subprocess(switches):
    """T3 bf16 under the switch sets of test_gpu_replay's subprocess test (the library reads a switch once per process: a fresh
    interpreter per set, one at a time); _assert_t3_schedule holds what each set forces. The ungrouped set carries the per-conv
    attribution of `wpartial`."""
    out = _subprocess("test_train_step_writes_stay_in_declared_regions and T3 and bf16 and not bf16x3", switches, "ws audit (")
    assert ("wpartial by conv: on" in out) == ("MPU_WGRAD_GROUP" in switches), out


# ---- tapped inference forward -----------------------------------------------------------------------------------------------------
def _audit_inference(net):
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    from replay_tap import tapped
    from test_gpu_unet import rand_weights
    t0 = time.time()
    K, C, depth, cf, B, H, W = INFER_NETS[net]
    w0 = rand_weights(U, K, C, depth, cf, seed=21)
    x = np.random.RandomState(23).randn(B, H, W, C).astype(np.float32)
    cov, auds = A.Coverage(), []
    for run, fill in enumerate(A.POISONS):
        m = UNet(n_classes=K, img_rows=H, img_cols=W, n_channels=C, depth=depth, complexity_factor=cf, dtype="bf16", logger=quiet)
        m.set_weights_dict(w0)
        aud = Auditor(m, B, fill, run, cov, "infer")
        auds.append(aud)
        with tapped(m, aud.on_launch) as tap:
            m._forward(m._as_input(x), training=False)
            torch.cuda.synchronize()
        aud.close()
        kinds = collections.Counter(aud.kinds)
        assert set(kinds) <= {0, 6, 8, 9, 10} and kinds[0] == 2 * depth + 1 and kinds[8] == 3 * depth + 1, kinds
        assert tap.launches == aud.n - 1
        assert aud.used == {k for k, (_i, ps, _w) in EXEMPT.items() if "infer" in ps}, ("exemptions used", aud.used)
        last = A.by_name(aud.regions, "act/N2/%d" % (depth - 1))
        untouched = bool((aud.ws[last.offset:last.offset + last.bytes] == fill).all())
        if aud.fused_head:                                   # out = NULL: the last conv's output tensor is not stored, not a byte of it
            assert untouched and kinds[10] == 1 and kinds[6] == 0, (untouched, kinds)
        else:
            assert not untouched and kinds[6] == 1 and kinds[10] == 0, (untouched, kinds)
        for name in ("stats", "probs", "loss_mean", "gA", "gB"):        # nothing of the training step's is touched
            r = A.by_name(aud.regions, name)
            assert bool((aud.ws[r.offset:r.offset + r.bytes] == fill).all()), name
    assert auds[0].kinds == auds[1].kinds
    pooled = sorted(key[2] for key in cov.order[0] if key[2].startswith("act/P/"))
    assert pooled == ["act/P/%d" % i for i in range(depth)], pooled         # every pooled tensor, fused or separate, covered
    _finish(cov, "inference " + net, "bf16", t0, auds, "; fused head: %s, fused pools: %d" % (auds[0].fused_head, depth - auds[0].kinds.count(9)))
    return auds[0]


@pytest.mark.parametrize("net", ["A", "B", "C", "D"], ids=lambda n: n + "-bf16")
def test_inference_forward_writes_stay_in_declared_regions(net):
    aud = _audit_inference(net)
    unfused = os.environ.get("MPU_FUSED_POOL") == "0" and os.environ.get("MPU_FUSED_HEAD") == "0"
    if net in ("A", "C"):
        assert aud.fused_head != unfused, (aud.fused_head, unfused)
    if net == "A":
        assert (aud.kinds.count(9) == 3) == unfused, aud.kinds


@pytest.mark.parametrize("switches", [{"MPU_HALO16_MIN": "1", "MPU_HALO16P_WGS": "5"},
                                      {"MPU_FUSED_POOL": "0", "MPU_FUSED_HEAD": "0"},
                                      {"MPU_HALO_UP8_MIN": "1"}], ids=["halo16p_5wgs", "unfused_pool_and_head", "halo_up8"])
def test_inference_net_a_audit_under_schedule_switches_subprocess(switches):
    """Network A under the switch sets of test_gpu_replay's subprocess test, a fresh interpreter per set."""
    out = _subprocess("test_inference_forward_writes_stay_in_declared_regions and A-bf16", switches, "ws audit (")
    assert ("fused head: False" in out) == ("MPU_FUSED_HEAD" in switches), out


# ---- untapped train step ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _untapped_step(net):
    """One untapped bf16 train_step per poison on a poisoned workspace: no gap byte and no byte behind the plan's total changes, and
    the trailer of `partial` changes only where the schedule log shows the fused training head. Returns whether that head ran."""
    from replay_tap import _LibApi
    t0 = time.time()
    K, C, depth, cf, B, H, W = TRAIN_NETS[net]
    api, ran = _LibApi(), []
    for fill in A.POISONS:
        m, x, y, sw = _train_case(K, C, depth, cf, B, H, W, "bf16", seed=51, sw_period=2)
        arena, ws, total = _carve_workspace(m, B, fill)
        regions = m.workspace_regions(B)
        api.log_enable(True)
        try:
            m.train_step(x, y, sw)
            torch.cuda.synchronize()
            log = api.log_read().splitlines()
        finally:
            api.log_enable(False)
        assert m._ws.data_ptr() == ws.data_ptr(), "the workspace was replaced"
        fused = any(l.startswith("bn_fold") and "head=1" in l for l in log)
        ran.append(fused)
        holes = A.gaps(regions, ws.numel())
        assert holes[-1][0] <= total and holes[-1][1] == total + SLACK, holes[-1]          # (the slack behind the plan's total is one)
        bad = [(lo, hi, int((ws[lo:hi] != fill).sum())) for lo, hi in holes if bool((ws[lo:hi] != fill).any())]
        assert not bad, "gap bytes changed (lo, hi, count): %s" % bad[:6]
        assert not arena.check(), arena.check()
        t = A.by_name(regions, "partial.trailer")
        touched = int((ws[t.offset:t.offset + t.bytes] != fill).sum())
        assert fused or not touched, "%d bytes of partial's trailer changed although the fused training head did not run" % touched
        written = sum(int((ws[r.offset:r.offset + r.bytes] != fill).any()) for r in A.top_level(regions))
        assert written > len(A.top_level(regions)) // 2, "the step hardly wrote to the carved workspace"
    assert ran[0] == ran[1]
    print("ws audit (untapped %s, bf16): fused training head %s; %.1f s" % (net, "ran" if ran[0] else "did not run", time.time() - t0))
    return ran[0]


@pytest.mark.parametrize("net", ["T1", "T2", "T3", "T4"])
def test_untapped_train_step_leaves_gaps_and_the_partial_trailer_alone(net):
    _untapped_step(net)


def test_untapped_fused_training_head_ran_on_t3_or_t4():
    """The trailer rule above is vacuous unless the fused head runs somewhere (64 filters at level 0: T3, T4)."""
    if _env_on("MPU_HEAD_TRAIN_FUSED") and _env_on("MPU_BN_ATOMIC") and _env_on("MPU_BN_FOLD") and _env_on("MPU_FUSED_BN_STATS"):
        assert _untapped_step("T3") or _untapped_step("T4")
