"""
Guard bands and poisoned scratch around the single-layer entry points (mpu_conv2d_*): forward, masked data gradient,
channel-sliced data gradient and weight gradient with EVERY input, output and scratch buffer carved from a guarded arena
(tests/guarded.py). Per case:
  (a) no guard byte changes (outputs, scratch, inputs, weights);
  (b) the outputs are bit-identical in three runs that differ only in the poison (NaN / zero / large finite) of the outputs,
      the scratch and the guards around the inputs: an out-of-bounds read that reaches a result, or scratch read before it is
      written, changes bits (the library has no floating-point atomics, every reduction has a fixed order);
  (c) the outputs meet the fp64 bounds of tests/test_gpu_conv.py once (the guarded path is the real one);
  (d) the weight-gradient scratch high-water mark stays within what the size query promised (printed: `pytest -s`). The
      workspace is carved with exactly the promised floats, so for it (d) holds by construction and the check that bites is
      (a), the guard behind the workspace; in the workspace_floats sweep the buffer is larger than the size passed and (d)
      is a check of its own.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guarded
from guarded import BIG, NAN, POISONS, ZERO, bits, last_written, written
import test_gpu_conv as tc
from test_gpu_conv import CONV1, CONV3, CONV3S2, UPCONV2, ref_forward, rnd, tol, wgrad_tol

pytestmark = pytest.mark.gpu

GUARD_CASES = [
    # mode,   B, H,  W,  C0, C1, Cout
    (CONV3,   1, 12, 20, 8, 0, 72),        # ragged M and N
    (CONV3,   2, 36, 40, 72, 72, 64),      # concat, first source no multiple of 64: weight gradient as one job per source (C1 == C0)
    (CONV3,   2, 36, 40, 64, 0, 64),       # weight gradient with C1 != C0: the unknown-capacity branch (partial_cap = 0)
    (CONV3,   3, 2, 1, 136, 0, 72),        # degenerate maps
    (CONV3,   5, 1, 1, 128, 0, 128),
    (CONV3,   13, 3, 33, 128, 0, 128),     # second tile column of one pixel
    (CONV3,   33, 8, 32, 128, 0, 128),     # odd strip count in wgrad_taps, last workgroup half idle
    (CONV3,   8, 512, 32, 8, 0, 24),       # persistent level-0 kernel, 1024 tiles, one tile column
    (CONV3,   1, 64, 96, 72, 0, 40),       # patch kernel, channel tail
    (UPCONV2, 1, 8, 12, 72, 0, 40),        # up-conv edges
    (UPCONV2, 2, 36, 40, 64, 0, 64),
    (UPCONV2, 40, 2, 2, 64, 0, 72),        # 1 x 1 low-resolution maps
    (CONV1,   2, 16, 16, 64, 0, 8),        # 1 x 1 conv
]
PERSISTENT = (CONV3, 8, 512, 32, 8, 0, 24)

SPLITK_CASES = [                            # these take a workspace
    (CONV3,   3, 8, 12, 136, 72, 200),
    (CONV3,   4, 8, 8, 320, 0, 256),
    (CONV3,   12, 8, 8, 448, 0, 128),
    (CONV3,   12, 16, 16, 128, 0, 512),    # the deepk lower bound, 192 tiles
]
DEEPK = SPLITK_CASES[3]

HALO16_CASES = [                            # eligible for conv_halo16p under MPU_HALO16_MIN=1 (the subprocess pass)
    (CONV3,   1, 16, 40, 64, 0, 136),
    (CONV3,   1, 16, 32, 96, 32, 128),
]

X3_CASES = [(GUARD_CASES[2], False), (GUARD_CASES[1], False), (SPLITK_CASES[0], True)]      # plain, concat, split-K


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def arena(need_bytes, nbufs, fill):
    return guarded.arena(__name__, need_bytes, nbufs, fill)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def schedule_log(fn):
    """The schedule log lines (mpu_schedule_log_*) of the launches fn() makes."""
    import ctypes as C
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    lib.mpu_schedule_log_enable(1)
    try:
        fn()
        n = lib.mpu_schedule_log_read(None, 0)
        buf = C.create_string_buffer(int(n) + 1)
        lib.mpu_schedule_log_read(buf, n + 1)
    finally:
        lib.mpu_schedule_log_enable(0)
    return buf.value.decode().splitlines()


def conv_of(lines):
    return [l.split()[1] for l in lines if l.startswith("conv ")]


def wgrad_of(lines):
    """(kind, Cin, ksplit) per weight-gradient launch of the log."""
    out = []
    for l in lines:
        if l.startswith("wgrad "):
            f = dict(kv.split("=") for kv in l.split()[2:] if "=" in kv)
            out.append((l.split()[1], int(f["Cin"]), int(f["ksplit"])))
    return out


@functools.lru_cache(maxsize=4)
def inputs(case, dtype):
    """The operands of tests/test_gpu_conv.py::_run_case and its fp64 layer, computed once per (case, dtype)."""
    mode, B, H, W, C0, C1, Cout = case
    g = torch.Generator().manual_seed(hash(case) % 2**31)
    k = {CONV3: 3, UPCONV2: 2, CONV1: 1}[mode]
    Hi, Wi = (H // 2, W // 2) if mode == UPCONV2 else (H, W)
    Cin = C0 + C1
    x = rnd(torch.randn(B, Hi, Wi, Cin, generator=g), dtype)
    w = rnd(torch.randn(k, k, Cin, Cout, generator=g) / np.sqrt(k * k * Cin), dtype)
    b = torch.randn(Cout, generator=g).to(torch.float64) * 0.1
    dz = rnd(torch.randn(B, H, W, Cout, generator=g), dtype)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    pre = ref_forward(mode, xr, wr, b)
    y_ref = torch.relu(pre).detach()
    pre.backward(dz)
    mask = (torch.rand(B, Hi, Wi, Cin, generator=g) > 0.3).to(torch.float64)
    return dict(x=x, w=w, b=b, dz=dz, mask=mask, y=y_ref, dx=xr.grad * mask, dx1=xr.grad[..., C0:].contiguous(),
                dW=wr.grad.reshape(k * k, Cin, Cout), k=k, Hi=Hi, Wi=Wi)


def run_guarded(case, dtype, fill, x3=False, workspace=False, ws_floats=None, wgrad=True):
    """One pass over the layer with everything carved from the arena poisoned with `fill`. Returns (outputs on the host,
    guard violations, {scratch: one past its last element that no longer holds the poison}, promised scratch sizes). The
    split-K workspace is measured and poisoned again after each of its launches: forward, masked and sliced data gradient."""
    from multiplanarunet_amd import _lib, ops
    mode, B, H, W, C0, C1, Cout = case
    I = inputs(case, dtype)
    k, Hi, Wi, Cin = I["k"], I["Hi"], I["Wi"], C0 + C1
    esz = 2 if dtype == torch.bfloat16 else 4
    M = B * H * W
    nt = {CONV3: 9, UPCONV2: 4, CONV1: 1}[mode]
    n_wws = _lib.load().mpu_conv2d_wgrad_workspace_floats(mode, Cin, Cout, M)
    cap_ws = (16 * M * max(Cout, Cin) if ws_floats is not None else 8 * M * max(Cout, Cin)) if workspace else 0
    need = esz * (6 * B * Hi * Wi * Cin + 2 * M * Cout + 20 * Cin * Cout) + 4 * (n_wws + cap_ws + 2 * nt * Cin * Cout + Cout) + 4096
    A = arena(need, 20, fill)
    dev = A.mem.device
    xd = I["x"].to(dev, dtype)
    x0 = A.put(xd[..., :C0].contiguous(), "x0")
    x1 = A.put(xd[..., C0:].contiguous(), "x1") if C1 else None
    w32 = A.put(I["w"].to(dev, torch.float32), "w")
    bias = A.put(I["b"].to(dev, torch.float32), "bias")
    dzd = A.put(I["dz"].to(dev, dtype), "dz")
    mask = A.put(I["mask"].to(dev, dtype), "mask")
    wf = A.carve(k * k * Cout * Cin, dtype, name="wf")
    wd = A.carve(9 * Cin * Cout, dtype, name="wd")
    ops.pack_weights(w32, mode, dtype, x3=x3, out_fwd=wf, out_dgrad=wd)
    ws = None
    if workspace:
        ws_all = A.carve(cap_ws, torch.float32, name="ws")
        ws = ws_all if ws_floats is None else ws_all[:ws_floats]     # (the sweep: a prefix of a larger poisoned buffer)
    out, scratch = {}, {}

    def measure(which):
        if ws is not None:
            scratch[which] = last_written(ws_all, fill)
            ws_all.view(torch.uint8).fill_(fill)
    y = ops.conv2d(mode, x0, wf, Cout, (H, W), bias=bias, x1=x1, relu=True, workspace=ws, x3=x3,
                   out=A.carve((B, H, W, Cout), dtype, name="y"))
    measure("ws_fwd")
    dmode = CONV3S2 if mode == UPCONV2 else (CONV1 if mode == CONV1 else CONV3)
    wdg = wd if mode != CONV1 else A.put(I["w"].to(dev, dtype).reshape(-1), "w1x1")
    dx = ops.conv2d(dmode, dzd, wdg, Cin, (Hi, Wi), mask=mask, w_tap_stride=Cin * Cout, w_row_stride=Cout, workspace=ws,
                    x3=x3, out=A.carve((B, Hi, Wi, Cin), dtype, name="dx"))
    measure("ws_dgrad")
    out["y"], out["dx"] = y, dx
    if C1:
        out["dx1"] = ops.conv2d(dmode, dzd, wdg[C0 * Cout:], C1, (Hi, Wi), w_tap_stride=Cin * Cout, w_row_stride=Cout,
                                workspace=ws, x3=x3, out=A.carve((B, Hi, Wi, C1), dtype, name="dx1"))
        measure("ws_dx1")
    if wgrad:
        wws = A.carve(n_wws, torch.float32, name="wgrad_ws")
        out["dW"] = ops.conv2d_wgrad(mode, x0, dzd, x1=x1, x3=x3, workspace=wws,
                                     out=A.carve((nt, Cin, Cout), torch.float32, name="dW"))
        scratch["wgrad_ws"] = last_written(wws, fill)
    torch.cuda.synchronize()
    viol = A.check()
    return {n: t.cpu() for n, t in out.items()}, viol, scratch, dict(wgrad_ws=n_wws)


def check_bounds(case, dtype, out, x3=False):
    I = inputs(case, dtype)
    tc.X3_TOL[0] = 5e-5 if x3 else None
    try:
        for name in out:
            ref = I[name]
            rt, at = wgrad_tol(dtype, ref) if name == "dW" else tol(dtype, ref)
            np.testing.assert_allclose(out[name].double().numpy(), ref.numpy(), rtol=rt, atol=at, err_msg=name)
    finally:
        tc.X3_TOL[0] = None


def guarded_case(case, dtype, x3=False, workspace=False):
    runs = {}
    for fill in POISONS:
        out, viol, scratch, promised = run_guarded(case, dtype, fill, x3=x3, workspace=workspace)
        assert not viol, (fill, viol)                                            # (a)
        runs[fill] = (out, scratch)
    for fill in POISONS[1:]:                                                     # (b)
        for name, t in runs[NAN][0].items():
            assert same_bits(t, runs[fill][0][name]), "%s depends on the poison (0xFF vs 0x%02X)" % (name, fill)
    check_bounds(case, dtype, runs[ZERO][0], x3=x3)                              # (c)
    # (d) The carved workspace holds exactly the promised floats, so the mark cannot exceed them: what catches a plan that
    # needs more than the query promised is (a), the guard behind the workspace. The mark is taken for the record.
    hw = max(runs[fill][1]["wgrad_ws"] for fill in POISONS)
    print("GUARD-HW wgrad %s %s%s high_water=%d promised=%d" % (case, str(dtype).split(".")[1], " x3" if x3 else "", hw,
                                                               promised["wgrad_ws"]))
    assert hw <= promised["wgrad_ws"]


SWITCHED = any(os.environ.get(k) for k in ("MPU_HALO16_MIN", "MPU_HALO_UP8_MIN", "MPU_HALO16P_WGS"))   # (the child passes)
CONCAT, PLAIN64, TAPS_ODD = GUARD_CASES[1], GUARD_CASES[2], GUARD_CASES[6]


def logged_case(case, dtype, **kw):
    """guarded_case under the schedule log: (conv schedules, weight-gradient launches) of ONE of its three identical runs."""
    lines = schedule_log(lambda: guarded_case(case, dtype, **kw))
    conv, wg = conv_of(lines), wgrad_of(lines)
    assert len(conv) % 3 == 0 and conv[:len(conv) // 3] * 3 == conv, conv          # the poison does not steer the dispatcher
    assert len(wg) % 3 == 0 and wg[:len(wg) // 3] * 3 == wg, wg
    conv, wg = conv[:len(conv) // 3], wg[:len(wg) // 3]
    print("GUARD-SCHED %s %s conv=%s wgrad=%s" % (case, str(dtype).split(".")[1], conv, wg))
    return conv, wg


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("case", GUARD_CASES)
def test_guarded_layer(case, dtype):
    """Where a case is there for a named schedule, the log pins it: a dispatcher change must not move the edge elsewhere."""
    conv, wg = logged_case(case, dtype)
    bf16 = dtype == torch.bfloat16
    if case == PERSISTENT and bf16:       # its masked data gradient (24 -> 8 channels, 1024 tiles) is conv_ws's
        assert "ws" in conv, conv
    if SWITCHED:
        return
    if case == PERSISTENT and bf16:       # forward of the 8-channel first layer: conv_c8 (like conv_ws a bf16 kernel; f32 has neither)
        assert conv == ["c8", "ws"], conv
    if case == CONCAT and bf16:           # first source no multiple of 64 channels, capacity known (C1 == C0): one job per source
        assert [(k in ("taps", "glds"), cin) for k, cin, _ in wg] == [(True, 72), (True, 72)], wg
    if case == PLAIN64:                   # capacity unknown (partial_cap = 0): ONE job over all 64 channels, on split partials
        assert len(wg) == 1 and wg[0][1] == 64 and wg[0][2] > 1, wg
        assert not bf16 or wg[0][0] in ("taps", "glds"), wg
    if case == TAPS_ODD and bf16:         # wgrad_taps, 33 strips of one 8 x 32 image: 17 partial copies, the last from one strip
        assert wg == [("taps", 128, 17)], wg


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("case", SPLITK_CASES)
def test_guarded_split_k_layer(case, dtype):
    conv, _ = logged_case(case, dtype, workspace=True)
    if dtype == torch.bfloat16 or not SWITCHED:              # f32 too: the forward is on a schedule that takes the workspace
        assert conv and conv[0] in ("pipe", "glds", "deepk"), conv
    if dtype == torch.bfloat16 and case == DEEPK:
        assert conv[0] == "deepk", conv


@pytest.mark.parametrize("case,workspace", X3_CASES)
def test_guarded_layer_split_bf16_products(case, workspace):
    guarded_case(case, torch.float32, x3=True, workspace=workspace)


@pytest.mark.parametrize("case", HALO16_CASES)
def test_guarded_halo16_shapes(case):
    """(conv_halo16p under MPU_HALO16_MIN=1: test_subprocess_pass_under_the_halo_switches runs it that way and the schedule is asserted)"""
    conv, _ = logged_case(case, torch.bfloat16)
    if os.environ.get("MPU_HALO16_MIN") == "1":
        assert conv and conv[0] == "halo16p", conv


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("case", SPLITK_CASES)
def test_workspace_floats_is_honoured(case, dtype):
    """mpu_conv2d_igemm_ws with workspace_floats from 1 float to twice the default: whatever the size, nothing at or past
    index workspace_floats of a larger poisoned buffer changes, the guards stay clean and the result meets the fp64 bound (a
    size the split-K schedule cannot use falls back, it does not overrun)."""
    mode, B, H, W, C0, C1, Cout = case
    M = B * H * W
    for n in (1, 1000, M * Cout - 1, M * Cout, 2 * M * Cout + 3, 16 * M * max(Cout, C0 + C1)):
        runs = {}
        for fill in (NAN, BIG):
            out, viol, scratch, _ = run_guarded(case, dtype, fill, workspace=True, ws_floats=n, wgrad=False)
            assert not viol, (n, fill, viol)
            runs[fill] = (out, scratch)
        for name, t in runs[NAN][0].items():
            assert same_bits(t, runs[BIG][0][name]), "%s depends on the workspace poison at workspace_floats=%d" % (name, n)
        check_bounds(case, dtype, runs[BIG][0])
        for which in sorted(runs[NAN][1]):                                   # ws_fwd, ws_dgrad and, with a second source, ws_dx1
            hw = max(runs[NAN][1][which], runs[BIG][1][which])
            print("GUARD-HW igemm_ws %s %s %s workspace_floats=%d high_water=%d" % (case, str(dtype).split(".")[1], which, n, hw))
            assert hw <= n, (which, n, hw)


@pytest.mark.parametrize("case", tc.FIRST_LAYER_CASES[1:4] + [(4, 32, 128, 64, 1)] + tc.FIRST_LAYER_CASES[4:])
def test_guarded_first_layer_weight_gradient(case):
    """mpu_conv2d_wgrad_first_layer with workspace, dW and db carved (the B=16 128 x 128 case shrunk to 4 x 32 x 128)."""
    from multiplanarunet_amd import _lib, ops
    B, H, W, Cout, CI = case
    x, dz, ref, rb = tc.first_layer_inputs(case)
    n = _lib.load().mpu_conv2d_wgrad_first_layer_workspace_floats(Cout, B * H * W)
    runs = {}
    for fill in POISONS:
        A = arena(2 * B * H * W * (8 + Cout) + 4 * (n + 73 * Cout), 5, fill)
        xd, dzd = A.put(x.cuda(), "x"), A.put(dz.cuda(), "dz")
        ws = A.carve(n, torch.float32, name="workspace")
        dW, db = ops.conv2d_wgrad_first_layer(xd, CI, dzd, workspace=ws, out=A.carve((9, 8, Cout), torch.float32, name="dW"),
                                              out_db=A.carve(Cout, torch.float32, name="db"))
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        runs[fill] = (dW.cpu(), db.cpu(), last_written(ws, fill))
    for fill in POISONS[1:]:
        assert same_bits(runs[NAN][0], runs[fill][0]) and same_bits(runs[NAN][1], runs[fill][1]), fill
    tc.check_first_layer(runs[ZERO][0], runs[ZERO][1], ref, rb, CI)
    hw = max(runs[fill][2] for fill in POISONS)      # (within n by construction: the guard behind the workspace is the check)
    print("GUARD-HW first_layer %s high_water=%d promised=%d" % (case, hw, n))
    assert hw <= n


@pytest.mark.parametrize("mode,dtype,x3", [(m, d, False) for m in (CONV3, UPCONV2, CONV3S2, CONV1)
                                           for d in (torch.float32, torch.bfloat16)] +
                         [(m, torch.float32, True) for m in (CONV3, UPCONV2, CONV3S2)])   # (x3: f32 operands of the 3x3 / 2x2 layers)
def test_guarded_pack_weights(mode, dtype, x3):
    """Both outputs of mpu_conv2d_pack_weights: every element of the forward operand is written; of the 9 * Cin * Cout
    elements of the data-gradient operand all are written for the 3x3 and 2x2 modes, and exactly the first Cin * Cout for
    the 1x1 mode (include/mpunet_hip.h) -- the rest keeps the caller's bytes."""
    from multiplanarunet_amd import ops
    k = {CONV3: 3, UPCONV2: 2, CONV3S2: 3, CONV1: 1}[mode]
    for ci, co in ((8, 72), (72, 40), (136, 200)):
        w = torch.randn(k, k, ci, co, generator=torch.Generator().manual_seed(ci + co))
        runs = {}
        for fill in POISONS:
            A = arena(4 * (k * k + k * k + 9) * ci * co, 3, fill)
            wf = A.carve(k * k * co * ci, dtype, name="wf")
            wd = A.carve(9 * ci * co, dtype, name="wd")
            ops.pack_weights(A.put(w.cuda(), "w"), mode, dtype, x3=x3, out_fwd=wf, out_dgrad=wd)
            torch.cuda.synchronize()
            assert not A.check(), (fill, A.check())
            runs[fill] = (wf.clone(), wd.clone())
        nd = (1 if mode == CONV1 else 9) * ci * co
        for fill in POISONS[1:]:
            assert same_bits(runs[NAN][0], runs[fill][0]) and same_bits(runs[NAN][1][:nd], runs[fill][1][:nd]), fill
        assert bool((written(runs[NAN][0], NAN) | written(runs[BIG][0], BIG)).all())
        assert bool((written(runs[NAN][1][:nd], NAN) | written(runs[BIG][1][:nd], BIG)).all())
        for fill in POISONS:
            assert not bool(written(runs[fill][1][nd:], fill).any()), (mode, fill)


@pytest.mark.parametrize("extra", [{}, {"MPU_HALO16P_WGS": "3"}], ids=["one_tile_per_workgroup", "three_workgroups"])
def test_subprocess_pass_under_the_halo_switches(extra):
    """The layer cases of this module in a fresh interpreter (the switches are read once per process): every eligible shape on
    conv_halo16p and the 8-row up-conv tiles (MPU_HALO16_MIN=1 MPU_HALO_UP8_MIN=1); once more with 3 persistent workgroups
    walking many tiles each (MPU_HALO16P_WGS=3)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k",
                        "guarded_layer or guarded_split_k or guarded_halo16"],
                       env=dict(os.environ, MPU_HALO16_MIN="1", MPU_HALO_UP8_MIN="1", **extra),
                       capture_output=True, text=True, cwd=os.path.dirname(here))
    assert r.returncode == 0 and " passed" in r.stdout, str(extra) + r.stdout[-2000:] + r.stderr[-2000:]
