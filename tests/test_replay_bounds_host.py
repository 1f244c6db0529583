"""The bounds of the inference replay (tests/replay_ref.py, tests/test_gpu_replay.py) checked without a GPU: a torch-f32
emulation of one inference conv launch -- bf16 operands, f32 accumulation, f32 affine, ONE bf16 rounding -- against the fp64
reference, at the widest reduction the replayed networks reach (K = 9 * 512). A correct kernel errs like the emulation; the
emulation must stay under a third of every bound, and a reference with the affine on the wrong side of the ReLU, or a shifted
shift vector, must break them."""
import numpy as np
import torch

import replay_ref as R


def _layer(seed, Cin=512, Cout=512, H=6, W=10):
    rng = np.random.RandomState(seed)
    x = R.bf16_round(np.maximum(rng.randn(2, H, W, Cin), 0) * rng.uniform(.2, 2., Cin) + rng.uniform(-.3, .3, Cin))
    lim = np.sqrt(6.0 / (9 * Cin + 9 * Cout))
    w = R.bf16_round(rng.uniform(-lim, lim, (3, 3, Cin, Cout)))
    b = torch.tensor(rng.uniform(-.1, .1, Cout).astype(np.float32).astype(np.float64))
    gamma = rng.uniform(.5, 1.5, Cout); gamma[0] = -0.8
    s = (gamma / np.sqrt(rng.uniform(.5, 2., Cout) + 1e-3)).astype(np.float32).astype(np.float64)
    t = rng.uniform(-.5, .5, Cout).astype(np.float32).astype(np.float64)
    s[-3:] = 0; t[-3:] = 0; w[..., -3:] = 0; b[-3:] = 0               # padded channels
    s[5] *= 1e-2; t[5] *= 1e-2                                        # a live channel far below the tensor's maximum
    return x, w, b, torch.tensor(s), torch.tensor(t)


def test_f32_emulation_of_a_folded_bn_conv_stays_under_a_third_of_the_bounds():
    worst_t = worst_c = 0.0
    for seed in (0, 1, 2):
        x, w, b, s, t = _layer(seed)
        ref = R.affine_relu_conv(0, x, w, b, s, t).numpy()
        f = torch.float32
        emu = R.bf16_round(R.affine_relu_conv(0, x.to(f), w.to(f), b.to(f), s.to(f), t.to(f))).numpy()
        e_t, e_c, c = R.conv_bound_ratios(emu, ref)
        worst_t, worst_c = max(worst_t, e_t), max(worst_c, e_c)
        assert e_t <= R.CONV_TOL / 3 and e_c <= 1.0 / 3, (seed, e_t, e_c, c)
    print("replay bounds (f32 emulation, K = 4608): tensor-wise %.3g of the maximum, per-channel %.3g of its bound" % (worst_t, worst_c))


def test_bounds_reject_a_misplaced_affine_and_a_shifted_shift_vector():
    x, w, b, s, t = _layer(3)
    ref = R.affine_relu_conv(0, x, w, b, s, t).numpy()
    z = R.layer_forward(0, x, w, b)
    before = torch.relu(s * z + t).numpy()                            # the affine before the ReLU
    assert R.conv_bound_ratios(before, ref)[1] > 1
    shifted = (s * torch.relu(z) + torch.roll(t, 1)).numpy()          # post_shift read one channel off
    assert R.conv_bound_ratios(shifted, ref)[1] > 1
    small = ref.copy(); small[..., 5] *= 1.05                         # 5 % on a channel ~1e-2 of the maximum: the tensor-wise bound is blind
    e_t, e_c, c = R.conv_bound_ratios(small, ref)
    assert e_t <= R.CONV_TOL and e_c > 1 and c == 5, (e_t, e_c, c)


def test_head_partial_bound_holds_for_the_emulation_and_rejects_a_swapped_half():
    rng = np.random.RandomState(4)
    y = rng.randn(40, 64) * rng.uniform(.1, 3., 64)
    Wh = rng.uniform(-.3, .3, (64, 5)).astype(np.float32).astype(np.float64)
    yb = R.bf16_round(y).to(torch.float32)
    hi = torch.tensor(Wh, dtype=torch.float32).to(torch.bfloat16).to(torch.float32)
    lo = (torch.tensor(Wh, dtype=torch.float32) - hi).to(torch.bfloat16).to(torch.float32)
    for h in (0, 1):
        sl = slice(32 * h, 32 * h + 32)
        emu = (yb[:, sl] @ hi[sl] + yb[:, sl] @ lo[sl]).numpy()
        assert R.head_partial_ratio(emu, y[:, sl], Wh[sl]) <= 1.0 / 3
        assert R.head_partial_ratio(emu, y[:, slice(32 - 32 * h, 64 - 32 * h)], Wh[slice(32 - 32 * h, 64 - 32 * h)]) > 1
