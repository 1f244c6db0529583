"""
Range of the fixed-point accumulators of the training step. The producers of a BatchNorm's input (and, in dtype "bf16x3", of every
conv's dz) add their per-workgroup column sums as integers into per-XCD accumulators (kernels.h: stats_acc_add; unet_ops.hip:
bn_acc_sum); units per 1.0 (unet_model.hip): forward sum x 2^24 and sum x^2 2^16 (BN_ACC_F), backward sum dn and sum dn * xhat 2^40
(BN_ACC_B), bias gradient sum dz 2^44 (DB_ACC_SCALE).

The loss the step differentiates is the SUM over pixels of the per-image-weighted cross entropy (oracle/unet_ref.py:
keras_sparse_ce), so a per-pixel gradient is O(1) times the sample weight and the backward sums grow with B * H * W * w. At the
configs[3] shape (32 slices of 256 x 256) a bias-gradient sum of this network passes 2^19 = 2^63 units from w ~ 3, and the
BatchNorm-backward sums of level 0 pass 2^23 from w ~ 27: a one-word int64 sum wraps there and returns a sign-flipped value, with
no NaN and no error.

(a) One tapped forward + backward pass per case (mpu_unet_set_launch_tap, as tests/test_gpu_replay.py): every value that comes out
    of an accumulator is recomputed in fp64 from the tensors THAT launch read -- batch mean / 1/std of every BatchNorm forward,
    dgamma / dbeta and the first CMP images' dz of every BatchNorm backward, the bias gradient of every conv -- summed a few images
    at a time (a 64-channel fp64 copy of a 32 x 256^2 batch is 1 GB). Each stress case asserts its own premise: in today's units
    one of its reference sums reaches 2^63, so the case cannot quietly lose its teeth if the network or the data change.
(b) The same sums on the benchmarked path (no tap: the fused head passes and the pool-backward recompute run only without one):
    the forward does not depend on the sample weight and the backward is linear in it, so scaling w by a power of two scales every
    gradient by exactly that power (every bf16 / f32 rounding scales with it).
"""
import numpy as np
import pytest
import torch

from _devcopy import hip, d2h_f32, d2h_rows

pytestmark = pytest.mark.gpu
quiet = lambda *a, **k: None
CMP = 2                  # images whose BatchNorm-backward output is compared element by element
CHUNK = 4                # images per fp64 piece of a full-batch sum
EPS = 1e-3               # BatchNormalization epsilon (Keras default)
TWO63 = 2.0 ** 63
UNITS_F = (2.0 ** 24, 2.0 ** 16)          # unet_model.hip: BN_ACC_F (sum x, sum x^2)
UNITS_B = 2.0 ** 40                       # BN_ACC_B (sum dn, sum dn * xhat)
UNITS_DB = 2.0 ** 44                      # DB_ACC_SCALE (bias gradient, bf16x3)


def _setup(dtype, B, dim, seed):
    """depth 4, complexity_factor 1 (64 ... 1024 filters: every BatchNorm has C % 64 == 0 and takes the accumulator path), 3
    classes; Glorot kernels, random biases / betas, gammas in [0.5, 1.5] and one negative per BatchNorm; unit-variance inputs."""
    from multiplanarunet_amd.unet import UNet
    from oracle import unet_ref as U
    K = 3
    w0 = U.init_weights(K, 1, 4, 1, seed=seed)
    rng = np.random.RandomState(seed + 1)
    for k in w0:
        v = k.split("/")[1]
        if v == "bias":
            w0[k] = rng.uniform(-.1, .1, w0[k].shape).astype(np.float32)
        elif v == "gamma":
            w0[k] = rng.uniform(.5, 1.5, w0[k].shape).astype(np.float32)
            w0[k][0] = -0.8
        elif v == "beta":
            w0[k] = rng.uniform(-.3, .3, w0[k].shape).astype(np.float32)
    x = rng.randn(B, dim, dim, 1).astype(np.float32)
    y = (rng.randint(0, K, (B, dim, dim)) * (rng.rand(B, dim, dim) < 0.5)).astype(np.uint8).reshape(B, -1, 1)
    m = UNet(n_classes=K, dim=dim, n_channels=1, depth=4, complexity_factor=1, flatten_output=True, dtype=dtype, logger=quiet)
    m.set_weights_dict(w0)
    return m, x, y


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


SEED = 61
# (dtype, B, H = W, sample weight of the even / odd images, the family whose premise the case asserts). Largest bias-gradient sum of
# this network in units of 2^63 (measured): 0.85 at configs[1] with w = 8, 0.32 at the configs[3] shape with w = 1
RANGE_CASES = [
    ("bf16x3", 16, 128, (32.0, 16.0), "bias"),         # configs[1]: ~2.5
    ("bf16x3", 32, 256, (8.0, 4.0), "bias"),           # the configs[3] shape: ~1.9
    ("bf16", 32, 256, (128.0, 64.0), "backward"),      # BatchNorm-backward sums of level 0: ~3.6
    ("bf16", 16, 128, (2.0 ** -20, 2.0 ** -20), None),  # the small end: partial sums of a few hundred fixed-point units
]


@pytest.mark.parametrize("dtype,B,dim,w,premise", RANGE_CASES,
                         ids=["bf16x3_b16_128_w32_16", "bf16x3_b32_256_w8_4", "bf16_b32_256_w128_64", "bf16_b16_128_w2e-20"])
def test_accumulator_sums_at_stressed_ranges_against_fp64_on_each_launchs_inputs(dtype, B, dim, w, premise):
    """Per-image weights alternate between images, so that a wrong image index in the weighting shows."""
    h = hip()
    m, x, y = _setup(dtype, B, dim, seed=SEED)
    sw = np.where(np.arange(B) % 2 == 0, w[0], w[1]).astype(np.float32)
    bf16 = dtype == "bf16"
    params = m.params.cpu().numpy().astype(np.float64)
    torch.set_num_threads(max(1, torch.get_num_threads()))
    seen = {2: 0, 3: 0, 4: 0}
    margin = {"forward": 0.0, "backward": 0.0, "bias": 0.0}      # largest |sum| * units / 2^63 per family
    stat_err, dz_err, bn_sums, db_sums = [], [], [], []

    def chunks(ptr, shape):
        for lo in range(0, B, CHUNK):
            yield lo, d2h_rows(h, ptr, shape, bf16, lo, min(B, lo + CHUNK))

    def grow(k, v):
        margin[k] = float(np.max([margin[k], v]))                   # (np.max: a NaN stays visible)

    def replay(li):
        H, W, Cc = li.H, li.W, li.C0
        M = B * H * W
        if li.kind == 3:                                             # BatchNorm forward: batch statistics of its input
            s = torch.zeros(Cc, dtype=torch.float64); ss = torch.zeros_like(s)
            for _lo, xb in chunks(li.in0, (B, H, W, Cc)):
                xb = xb.reshape(-1, Cc)
                s += xb.sum(0); ss += (xb * xb).sum(0)
            mu = s / M
            inv = 1.0 / torch.sqrt((ss / M - mu * mu).clamp_min(0.0) + EPS)
            e = max(_rel(d2h_f32(h, li.aux0, (Cc,)), mu), _rel(d2h_f32(h, li.aux1, (Cc,)), inv))
            stat_err.append((li.conv_index, e))
            grow("forward", float(s.abs().max()) * UNITS_F[0] / TWO63)
            grow("forward", float(ss.max()) * UNITS_F[1] / TWO63)
        elif li.kind == 4:                                           # BatchNorm backward: sum dn, sum dn * xhat, then dz
            mean_d = torch.from_numpy(d2h_f32(h, li.aux0, (Cc,))); inv_d = torch.from_numpy(d2h_f32(h, li.aux1, (Cc,)))
            sdn = torch.zeros(Cc, dtype=torch.float64); sdx = torch.zeros_like(sdn)
            for lo in range(0, B, CHUNK):
                dn = d2h_rows(h, li.in0, (B, H, W, Cc), bf16, lo, min(B, lo + CHUNK))
                xx = d2h_rows(h, li.in1, (B, H, W, Cc), bf16, lo, min(B, lo + CHUNK))
                xh = (xx - mean_d) * inv_d
                sdn += dn.sum((0, 1, 2)); sdx += (dn * xh).sum((0, 1, 2))
                if lo == 0:
                    dn0, x0, xh0 = dn[:CMP], xx[:CMP], xh[:CMP]
            g = torch.from_numpy(params[li.w_off:li.w_off + Cc])
            ref = torch.where(x0 > 0, g * inv_d * (dn0 - sdn / M - xh0 * sdx / M), torch.zeros((), dtype=torch.float64))
            dz_err.append((li.conv_index, _rel(d2h_rows(h, li.out, (B, H, W, Cc), bf16, 0, CMP), ref)))
            bn_sums.append((li.conv_index, li.w_off, li.b_off, sdx.numpy(), sdn.numpy()))
            grow("backward", float(torch.maximum(sdn.abs(), sdx.abs()).max()) * UNITS_B / TWO63)
        else:                                                        # a conv's weight gradient: its bias gradient is sum dz
            db = torch.zeros(li.Cout, dtype=torch.float64)
            for _lo, dz in chunks(li.dz, (B, H, W, li.Cout)):
                db += dz.sum((0, 1, 2))
            db_sums.append((li.conv_index, li.b_off, db.numpy()))
            if not bf16:                                             # (bf16: the bias gradients are fp32 partial rows)
                grow("bias", float(db.abs().max()) * UNITS_DB / TWO63)

    def on_launch(li):
        if li.kind in seen:
            seen[li.kind] += 1
            replay(li)

    from replay_tap import tapped
    with tapped(m, on_launch):                                       # (an exception cannot cross the ctypes callback: replay_tap.py)
        m.forward_backward(x, y, sw, want_loss=False)
        torch.cuda.synchronize()
    g = m.grads.cpu().numpy().astype(np.float64)
    assert seen == {2: 22, 3: 13, 4: 13}, seen

    bad = []
    worst = {"stat": 0.0, "dz": 0.0, "dgamma/dbeta": 0.0, "bias": 0.0}

    def check(what, idx, e, tol):
        worst[what] = float(np.max([worst[what], e]))
        if not e <= tol:
            bad.append((what, idx, e))

    for ci, e in stat_err:
        check("stat", ci, e, 1e-4)
    for ci, e in dz_err:
        check("dz", ci, e, 1.2e-2)
    for ci, w_off, b_off, dgamma, dbeta in bn_sums:
        check("dgamma/dbeta", ci, max(_rel(g[w_off:w_off + dgamma.size], dgamma), _rel(g[b_off:b_off + dbeta.size], dbeta)), 2e-3)
    for ci, b_off, db in db_sums:
        check("bias", ci, _rel(g[b_off:b_off + db.size], db), 2e-3 if bf16 else 5e-5)
    print("%s B=%d %d^2 w=%s: largest |sum| * units / 2^63: forward %.3g, backward %.3g, bias %s; worst rel-to-max error %s"
          % (dtype, B, dim, w, margin["forward"], margin["backward"], "%.3g" % margin["bias"] if not bf16 else "(fp32 rows)",
             ", ".join("%s %.3g" % kv for kv in worst.items())))
    if premise:
        assert margin[premise] >= 1.0, ("premise: no %s sum reaches 2^63 units" % premise, margin)
    assert not bad, bad


def _benchmarked_path_margins(m, g, x3):
    """Largest |sum| * units / 2^63 of the sums the untapped step takes out of accumulators, read off a gradient vector: dgamma /
    dbeta of every BatchNorm but the last (the fused head passes sum that one in fp32) and, in bf16x3, every 3x3 / up-conv bias."""
    last_bn = "upsample_L%d_BN2" % (m.depth - 1)
    out = {"backward": 0.0, "bias": 0.0}
    for nm in m._order:
        kind, off, ps, _ls = m._tensors[nm]
        layer, var = nm.split("/")
        v = float(g[off:off + int(np.prod(ps))].abs().max()) if kind == 0 else 0.0
        if var in ("gamma", "beta") and layer != last_bn:
            out["backward"] = max(out["backward"], v * UNITS_B / TWO63)
        elif var == "bias" and layer != "conv2d" and x3:
            out["bias"] = max(out["bias"], v * UNITS_DB / TWO63)
    return out


# (dtype, B, H = W, sample weight, power-of-two factor, the family whose premise the case asserts at weight c * w)
LINEAR_CASES = [
    ("bf16", 32, 256, 1.0, 2.0 ** 10, "backward"),
    ("bf16x3", 32, 256, 2.0 ** -4, 2.0 ** 7, "bias"),
    ("bf16x3", 16, 128, 1.0, 2.0 ** 5, "bias"),
]


@pytest.mark.parametrize("dtype,B,dim,w,c,premise", LINEAR_CASES,
                         ids=["bf16_b32_256_w1_x1024", "bf16x3_b32_256_w1-16_x128", "bf16x3_b16_128_w1_x32"])
def test_benchmarked_step_gradients_scale_exactly_with_a_power_of_two_sample_weight(dtype, B, dim, w, c, premise):
    """grads(c * w) == c * grads(w), bit for bit, on the path bench.py times (no launch tap), with a sum of the scaled step past
    2^63 units (asserted from c * grads(w)). The one rounding that does not scale is a fixed-point addend finer than one unit: a
    partial sum below 2^-17 (units 2^40) or 2^-21 (2^44) drops low bits, which at the scaled weight it may keep. Such a partial moves
    its sum by less than one unit -- 2^-40 of sums that are >= 1e-4 here -- and changes a BatchNorm coefficient only if that shift
    crosses an f32 rounding boundary. A wrapped sum instead is off by 2^64 units and flips the sign of its channel."""
    m, x, y = _setup(dtype, B, dim, seed=SEED)
    sw = np.full(B, w, np.float32)
    m.forward_backward(x, y, sw, want_loss=False)
    g1 = m.grads.clone()
    m.forward_backward(x, y, sw * np.float32(c), want_loss=False)
    g2 = m.grads.clone()
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    ref = g1 * c                                                    # exact: a power of two, far from f32 overflow / underflow
    margin = _benchmarked_path_margins(m, ref, dtype == "bf16x3")
    diff = []
    for nm in m._order:
        kind, off, ps, _ls = m._tensors[nm]
        if kind != 0:
            continue
        n = int(np.prod(ps))
        a, b = g2[off:off + n], ref[off:off + n]
        nd = int((a != b).sum())
        if nd:
            diff.append((nm, nd, n, float((a - b).abs().max() / (b.abs().max() + 1e-30))))
    print("%s B=%d %d^2: grads(%g * w) against %g * grads(w = %g): largest |sum| * units / 2^63 %s; %d parameter tensors differ %s"
          % (dtype, B, dim, c, c, w, margin, len(diff), diff[:8]))
    assert margin[premise] >= 1.0, ("premise: no %s sum reaches 2^63 units" % premise, margin)
    assert torch.equal(g2, ref), diff
