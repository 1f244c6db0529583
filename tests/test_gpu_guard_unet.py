"""
Guard bands and poisoned scratch around the U-Net's buffers: one eager train_step, one inference forward and a second
train_step on the small odd networks of the train-step replay (T1-T4 of tests/test_gpu_replay.py), with the workspace, grads,
params, packed, bn_state, the Adam slots, the probabilities, the loss and the input batch carved from a guarded arena
(tests/guarded.py). The whole workspace, the gradient buffer and the outputs start as 0xFF, 0x00 or 0x7B bytes:
  * no guard byte changes;
  * loss, probabilities, grads, params, bn_state, packed and the Adam slots are bit-identical under the three poisons -- the
    library zeroes its own fixed-point accumulators and reads no stale partial sums, first pass on a fresh workspace included,
    and every float of `grads` is written by the backward pass (and finite);
  * a second step on the now dirty workspace gives the bits of a second step on a workspace that was poisoned again between
    the steps.
No launch tap is installed, so the fused head and the pool-backward recompute run (they turn themselves off under a tap).
"""
import os
import subprocess
import sys

import pytest
import torch

import guarded
from guarded import BIG, NAN, POISONS, ZERO, bits
from test_gpu_replay import TRAIN_NETS, _train_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def arena(need_bytes, nbufs, fill):
    return guarded.arena(__name__, need_bytes, nbufs, fill)


def carved_at(A, name, t):
    """Is tensor `t` still the arena's buffer `name`? (A wrapper that allocated its own would leave the guards trivially clean.)"""
    return t.data_ptr() == A.mem.data_ptr() + [s for n, s, e in A.bufs if n == name][0]


def guarded_model(net, dtype, fill, loss=None, metrics=None):
    """(model, arena, x, y, sw, loss_out, probs_out): a fresh model of the replay's weights whose buffers are carved views with
    the same contents; workspace, grads and the outputs hold the poison."""
    from multiplanarunet_amd import _lib
    K, C, depth, cf, B, H, W = TRAIN_NETS[net]
    m, x, y, sw = _train_case(K, C, depth, cf, B, H, W, dtype, seed=51, sw_period=2)
    if loss or metrics:
        m.compile("Adam", loss, metrics=metrics)
    n_ws = int(_lib.load().mpu_unet_workspace_bytes(m._h, B))
    n_par = m.params.numel()
    need = n_ws + 4 * (6 * n_par + m.bn_state.numel()) + m.packed.numel() + B * H * W * (4 * C + 1 + 4 + 4 * K) + (8 << 20)
    A = arena(need, 16, fill)
    m._ws, m._ws_batch = A.carve(n_ws, torch.uint8, name="workspace"), B
    for name in ("params", "packed", "bn_state"):
        setattr(m, name, A.put(getattr(m, name), name))
    m.grads = A.carve(n_par, torch.float32, name="grads")
    m._slots = [A.carve(n_par, torch.float32, fill=ZERO, name="adam_%s" % s) for s in "mv"]
    xd = A.put(torch.from_numpy(x).cuda(), "x")
    yd = A.put(torch.from_numpy(y).cuda(), "y")
    swd = A.put(torch.from_numpy(sw).cuda(), "sample_weight")
    loss_out = A.carve((B, 1 if loss else H * W), torch.float32, name="loss")
    probs_out = A.carve((B, H, W, K), torch.float32, name="probs")
    return m, A, xd, yd, swd, loss_out, probs_out


def snapshot(m, loss, extra=()):
    from multiplanarunet_amd import _lib
    K, (H, W) = m.n_classes, m.img_shape[:2]
    B = m._last_batch
    off = int(_lib.load().mpu_unet_workspace_probs_offset(m._h, B))
    s = dict(loss=bits(loss), train_probs=bits(m._ws[off:off + 4 * B * H * W * K]), loss_mean=bits(m.loss_mean()),
             grads=bits(m.grads), params=bits(m.params), bn_state=bits(m.bn_state), packed=bits(m.packed),
             adam_m=bits(m._slots[0]), adam_v=bits(m._slots[1]))
    s.update({k: bits(v) for k, v in extra})
    return s


def run(net, dtype, fill, loss=None, repoison=None):
    """train_step, inference forward, [workspace poisoned again,] train_step. Returns the snapshots after the first step (with
    the inference probabilities) and after the second, and the gradients of the first step as floats."""
    m, A, xd, yd, swd, loss_out, probs_out = guarded_model(net, dtype, fill, loss)
    l1 = m.train_step(xd, yd, swd, loss_out=loss_out)
    torch.cuda.synchronize()
    assert l1.data_ptr() == loss_out.data_ptr()
    assert not A.check(), ("train_step", fill, A.check())
    assert all(carved_at(A, n, getattr(m, a)) for n, a in (("workspace", "_ws"), ("grads", "grads"), ("params", "params"),
                                                           ("packed", "packed"), ("bn_state", "bn_state"))), "a buffer was replaced"
    assert carved_at(A, "adam_m", m._slots[0]) and carved_at(A, "adam_v", m._slots[1])
    s1 = snapshot(m, l1)
    g1 = m.grads.cpu()
    p = m._forward(xd, training=False, out=probs_out)
    torch.cuda.synchronize()
    assert not A.check(), ("inference forward", fill, A.check())
    s1["probs"] = bits(p)
    p2 = m.predict_on_batch(xd)                            # the public entry point (it allocates its own output): the same bits
    torch.cuda.synchronize()
    assert not A.check(), ("predict_on_batch", fill, A.check())
    assert p2.numel() == p.numel() and torch.equal(bits(p2), s1["probs"])
    assert carved_at(A, "workspace", m._ws)
    if repoison is not None:
        m._ws.fill_(repoison)
    l2 = m.train_step(xd, yd, swd, loss_out=loss_out)
    torch.cuda.synchronize()
    assert not A.check(), ("second train_step", fill, A.check())
    assert carved_at(A, "workspace", m._ws)
    return s1, snapshot(m, l2), g1


def assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs in %d bytes" % (what, k, int((a[k] != b[k]).sum()))


NETS = [(n, d, None) for n in ("T1", "T2", "T3", "T4") for d in ("bf16", "bf16x3")] + [("T1", "f32", None)] + \
       [("T2", d, "SparseDiceLoss") for d in ("bf16", "bf16x3")]


@pytest.mark.parametrize("net,dtype,loss", NETS, ids=["%s-%s-%s" % (n, d, l or "ce") for n, d, l in NETS])
def test_guarded_train_steps(net, dtype, loss):
    first, second = {}, {}
    for fill in POISONS:
        first[fill], second[fill], g1 = run(net, dtype, fill, loss)
        assert bool(torch.isfinite(g1).all()), "grads: %d floats are not finite after the backward pass on a buffer of 0x%02X" \
            % (int((~torch.isfinite(g1)).sum()), fill)
    for fill in POISONS[1:]:
        assert_same(first[NAN], first[fill], "first step, poison 0xFF vs 0x%02X" % fill)
        assert_same(second[NAN], second[fill], "second step, poison 0xFF vs 0x%02X" % fill)
    for a, b in ((ZERO, NAN), (BIG, ZERO)):                 # dirty workspace == workspace poisoned again between the steps
        _, again, _ = run(net, dtype, a, loss, repoison=b)
        assert_same(second[a], again, "second step on the dirty workspace vs one poisoned with 0x%02X" % b)
    assert not torch.equal(first[NAN]["params"], second[NAN]["params"])          # (the steps did move the weights)


@pytest.mark.parametrize("switch", ["MPU_WGRAD_GROUP=0", "MPU_WGRAD_BATCHED_REDUCE=0", "MPU_TAIL_OVERLAP=0", "MPU_BN_ATOMIC=0",
                                    "MPU_POOL_BWD_RECOMPUTE=2", "MPU_HEAD_TRAIN_FUSED=0"])
def test_t3_under_schedule_switch_subprocess(switch):
    """The T3 runs of this module under one schedule switch of the step (read once per process: a fresh interpreter each)."""
    name, value = switch.split("=")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "guarded_train_steps and T3"],
                       env=dict(os.environ, **{name: value}), capture_output=True, text=True, cwd=os.path.dirname(here))
    assert r.returncode == 0 and " passed" in r.stdout, switch + r.stdout[-2000:] + r.stderr[-2000:]


def test_guarded_evaluation_t1():
    """evaluate / test_on_batch on T1 (mpu_eval_loss scratch, the loss accumulator, the metrics state; all six metrics
    compiled): guards clean, the per-image losses, the accumulators and the reported values do not depend on the poison."""
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.unet import METRICS
    K, C, depth, cf, B, H, W = TRAIN_NETS["T1"]
    got = {}
    for fill in POISONS:
        m, A, xd, yd, swd, _, probs_out = guarded_model("T1", "bf16", fill, metrics=list(METRICS))
        need = int(_lib.load().mpu_eval_loss_scratch_bytes(B, H * W, K))
        m._eval_ws, m._eval_ws_shape = A.carve(need, torch.uint8, name="eval_scratch"), (B, H * W)
        m._eval_acc = A.carve(2, torch.float64, name="eval_acc")
        m._eval_metrics_state = A.carve(int(_lib.load().mpu_train_metrics_state_bytes()) // 8, torch.float64, name="eval_metrics")
        per_image = A.carve(B, torch.float32, name="per_image_loss")
        acc, state = m.evaluation_begin()
        assert acc.data_ptr() == m._eval_acc.data_ptr() and state.data_ptr() == m._eval_metrics_state.data_ptr()
        p = m._forward(xd, training=False, out=probs_out)
        m.evaluation_update(p, yd, acc, state, swd, loss_out=per_image)
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        assert carved_at(A, "eval_scratch", m._eval_ws) and carved_at(A, "workspace", m._ws)
        s = dict(probs=bits(p), per_image=bits(per_image), acc=bits(acc), metrics=bits(state[:2 * len(METRICS)]))
        res = m.test_on_batch(xd, yd, swd, return_dict=True)             # the same through the public entry point
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        got[fill] = (s, res)
    for fill in POISONS[1:]:
        assert_same(got[NAN][0], got[fill][0], "evaluation, poison 0xFF vs 0x%02X" % fill)
        a, b = got[NAN][1], got[fill][1]
        assert a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a), (a, b)
    assert got[NAN][1]["loss"] > 0 and got[NAN][1]["loss"] == got[NAN][1]["loss"]


def test_guarded_l2_regularizer_t1():
    """mpu_unet_l2_regularizer on T1 with its mpu_unet_l2_workspace_doubles scratch and the penalty scalar carved."""
    from multiplanarunet_amd import _lib
    got = {}
    for fill in POISONS:
        m, A, xd, yd, swd, loss_out, _ = guarded_model("T1", "bf16", fill)
        m.l2_reg = 1e-3
        m._l2_ws = A.carve(int(_lib.load().mpu_unet_l2_workspace_doubles()), torch.float64, name="l2_scratch")
        m.reg_loss = A.carve(1, torch.float32, name="reg_loss")
        m.grads.zero_()
        m._add_l2(want_loss=True)
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        got[fill] = dict(grads=bits(m.grads), reg_loss=bits(m.reg_loss))
        want = float(m.l2_penalty().item())
        assert abs(float(m.reg_loss.item()) - want) <= 1e-5 * want and want > 0
        assert int(torch.count_nonzero(m.grads)) > 0
    for fill in POISONS[1:]:
        assert_same(got[NAN], got[fill], "l2 regularizer, poison 0xFF vs 0x%02X" % fill)
