"""
Guard bands and poisoned scratch around the remaining caller-owned device buffers (tests/guarded.py): the NIfTI decode, the
volume statistics, the elastic transform, the fusion model's forward, finalize and step, the evaluation loss, the metrics state,
the optimizers, the plane statistics, the view sampling and the back-mapping.
Every buffer a call reads or writes is carved from a guarded arena; each call runs three times on outputs and scratch of 0xFF,
0x00 and 0x7B bytes and must leave every guard byte alone and give the same bits. The inputs are those of the entry points'
own parity tests (imported), cut to the shapes at which a masked store or a scratch row can go wrong; where a reference is at
hand the result is also compared with it once, so that the guarded call is known to be the real one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
from guarded import NAN, POISONS, ZERO, bits
import optimizer_ref as OR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)
    guarded.release("test_gpu_guard_unet")               # (test_guarded_update_and_pack_t1 builds its models there)


def arena(need_bytes, nbufs, fill):
    return guarded.arena(__name__, need_bytes, nbufs, fill)


def under_three_poisons(need_bytes, nbufs, body):
    """body(arena) -> {name: tensor or array} for each poison; guards clean, the same bits three times. Returns the 0x00 run."""
    got = {}
    for fill in POISONS:
        A = arena(need_bytes, nbufs, fill)
        res = body(A)
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        got[fill] = {k: (v if isinstance(v, np.ndarray) else v.detach().cpu()) for k, v in res.items()}
    for fill in POISONS[1:]:
        for k in got[NAN]:
            assert torch.equal(bits(got[NAN][k]), bits(got[fill][k])), "%s depends on the poison (0xFF vs 0x%02X)" % (k, fill)
    return got[ZERO]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- mpu_volume_decode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", (1, 3))
@pytest.mark.parametrize("shape", [(37, 5, 70), (1, 64, 3), (65, 66, 1)])
def test_guarded_volume_decode(tmp_path, shape, C_):
    """f32 image (64 x 64 transpose tiles with a one-element overhang on both axes; three stored types) and, one channel, the u8
    labels with their bad-value counter: the first guard byte of a u8 output is the byte behind its last voxel."""
    import test_gpu_volume_decode as VD
    from multiplanarunet_amd import data, nifti
    from multiplanarunet_amd.formats import load_nifti, load_nifti_labels
    rng = np.random.RandomState(7)
    full = shape if C_ == 1 else shape + (C_,)
    nvox = int(np.prod(full))
    for code, endian in ((4, "<"), (64, ">"), (2, "<")):
        path = VD.write_file(tmp_path / ("g%d.nii" % code), VD.random_values(rng, code, full), code, endian)
        h, _, buf = nifti.read_nifti_payload(path)
        shape4 = tuple(full) + (1,) * (4 - len(full))
        got = under_three_poisons(4 * nvox, 1, lambda A: dict(
            image=data.decode_nifti_payload(h, buf, "cuda", False, path, out=A.carve(shape4, torch.float32, name="image"))))
        want, _ = load_nifti(path)
        np.testing.assert_array_equal(got["image"].numpy().view(np.uint32), want.view(np.uint32))
    if C_ == 1:
        path = VD.write_file(tmp_path / "lab.nii", VD.random_values(rng, 4, shape, small=True), 4)
        h, _, buf = nifti.read_nifti_payload(path)

        def labels(A):
            bad = A.carve(1, torch.int64, name="bad")
            out = data.decode_nifti_payload(h, buf, "cuda", True, path, out=A.carve(shape, torch.uint8, name="labels"), bad=bad)
            return dict(labels=out, bad=bad)
        got = under_three_poisons(nvox + 8, 2, labels)
        assert int(got["bad"]) == 0
        np.testing.assert_array_equal(got["labels"].numpy(), load_nifti_labels(path))


# ---- mpu_volume_moments / mpu_volume_order_stats -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", (1, 3))
@pytest.mark.parametrize("n_vox", (1, 255, 4097))
def test_guarded_volume_statistics(n_vox, C_):
    from multiplanarunet_amd import _lib, scalers as S
    rng = np.random.RandomState(n_vox + C_)
    vol = (rng.standard_normal((n_vox, 1, 1, C_)) * 100).astype(np.float32)
    if n_vox > 4:
        vol[3, 0, 0, C_ - 1] = np.nan
    nb = int(_lib.load().mpu_volume_stats_workspace_bytes(C_))
    ranks = sorted({0, (n_vox - 1) // 2, max(0, n_vox - 2)})

    def body(A):
        image = A.put(dev(vol), "volume")
        ws = (A.carve(nb, torch.uint8, name="workspace"), nb)
        res = {"moments": S.moments(image, workspace=ws)}
        for c in range(C_):
            v, n_nan = S.order_stats(image, c, ranks, workspace=ws)
            res["order%d" % c] = np.concatenate([v.astype(np.float64), [float(n_nan)]])
        res["centered"] = S.moments(image, mean=np.nanmean(vol.astype(np.float64), axis=(0, 1, 2)), workspace=ws)
        return res
    got = under_three_poisons(vol.nbytes + nb, 2, body)
    for c in range(C_):
        col = vol[..., c].ravel()
        srt = np.sort(col[~np.isnan(col)])
        want = [srt[r] if r < srt.size else np.nan for r in ranks]
        np.testing.assert_array_equal(got["order%d" % c][:-1], np.asarray(want, np.float64))
        assert got["order%d" % c][-1] == np.isnan(col).sum()
        m = got["moments"][c]
        assert (m[0], m[1], m[2], m[3]) == (srt.size, srt.min(), srt.max(), np.abs(srt).max())
        np.testing.assert_allclose(m[4], srt.astype(np.float64).sum(), rtol=1e-12, atol=1e-9)


# ---- mpu_elastic_transform_2d ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C_", [(2, 2, 1), (9, 7, 2), (96, 160, 1)])
def test_guarded_elastic_transform(H, W, C_):
    """Workspace (mpu_elastic_workspace_doubles), image out and labels out (u8) carved; bit-exact against the oracle as in
    tests/test_gpu_augment.py (alpha 50, sigma 2: a 17-tap filter, wider than the two small images)."""
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.augmentation import elastic_transform_2d
    from oracle import augmentation as OA
    rng = np.random.RandomState(H + W)
    image = rng.randn(H, W, C_).astype(np.float32)
    labels = rng.randint(0, 5, (H, W)).astype(np.uint8)
    noise = (rng.rand(H, W), rng.rand(H, W))
    bg = [0.25] * C_
    n_ws = int(_lib.load().mpu_elastic_workspace_doubles(H, W))
    assert n_ws >= 4 * H * W

    def body(A):
        x, y = elastic_transform_2d(A.put(dev(image), "image"), A.put(dev(labels), "labels"), 50.0, 2.0, bg,
                                    noise=A.put(dev(np.stack(noise)), "noise"),
                                    workspace=A.carve(n_ws, torch.float64, name="workspace"),
                                    out=A.carve((H, W, C_), torch.float32, name="out"),
                                    out_labels=A.carve((H, W), torch.uint8, name="out_labels"))
        return dict(image=x, labels=y)
    got = under_three_poisons(H * W * (8 * C_ + 2 + 16) + 8 * n_ws, 6, body)
    ref_x, ref_y = OA.elastic_transform_2d(image, labels, 50.0, 2.0, bg, noise=noise)
    assert np.array_equal(got["labels"].numpy(), ref_y) and np.array_equal(got["image"].numpy(), ref_x)


# ---- mpu_fusion_forward / mpu_fusion_finalize / mpu_fusion_train_step / mpu_fusion_grad_sums / mpu_fusion_apply_sums -----------------
@pytest.mark.parametrize("V,K,N", [(1, 1, 1), (3, 2, 777), (16, 8, 300), (16, 16, 129), (16, 9, 128)])
def test_guarded_fusion_step(V, K, N):
    """The wide kernel's 128-points-per-block edge (N = 128, 129) and V * K + K + 1 = 273 > 256 accumulators (16 x 16). Workspace
    (mpu_fusion_train_workspace_floats), sums, grads out, loss out, W, b, m, v carved; the fused step equals its two halves.
    mpu_fusion_forward on the same points and the initial weights, and mpu_fusion_finalize on z = sum_v W[v,k] x[n,v,k], with
    x, W, b, z, the probabilities and the u8 labels carved: within 1e-6 of the fp64 layer (tests/test_gpu_geometry.py's bound),
    labels equal outside float ties."""
    from multiplanarunet_amd import _lib
    from test_gpu_fusion_train import make_points
    x, y = make_points(N, V, K, 3)
    rng = np.random.RandomState(4)
    W0 = (1 + 0.2 * rng.randn(V, K)).astype(np.float32)
    b0 = (0.1 * rng.randn(1, K)).astype(np.float32)
    n_ws = int(_lib.load().mpu_fusion_train_workspace_floats(V, K))
    P = V * K + K
    adam = (1e-3, 0.9, 0.999, 1e-7)

    def state(A, tag):
        return (A.put(dev(W0), "W" + tag), A.put(dev(b0), "b" + tag), A.carve(P, torch.float32, fill=ZERO, name="m" + tag),
                A.carve(P, torch.float32, fill=ZERO, name="v" + tag))

    z0 = np.einsum("nvk,vk->nk", x.astype(np.float64), W0.astype(np.float64)).astype(np.float32)

    def body(A):
        xd, yd = A.put(dev(x), "x"), A.put(dev(y), "y")
        Wf, bf = A.put(dev(W0), "W forward"), A.put(dev(b0), "b forward")
        probs, labels = A.carve((N, K), torch.float32, name="probs"), A.carve(N, torch.uint8, name="labels")
        _lib.call("mpu_fusion_forward", _lib.ptr(xd), N, V, K, _lib.ptr(Wf), _lib.ptr(bf), _lib.ptr(probs), _lib.ptr(labels),
                  _lib.stream_ptr())
        zd = A.put(dev(z0), "z")
        probs_z, labels_z = A.carve((N, K), torch.float32, name="probs of z"), A.carve(N, torch.uint8, name="labels of z")
        _lib.call("mpu_fusion_finalize", _lib.ptr(zd), N, K, _lib.ptr(bf), 0, _lib.ptr(probs_z), _lib.ptr(labels_z), _lib.stream_ptr())
        ws = A.carve(n_ws, torch.float32, name="workspace")
        W, b, m, v = state(A, "")
        grads, loss = A.carve(P, torch.float32, name="grads"), A.carve(1, torch.float32, name="loss")
        for t in (1, 2):
            _lib.call("mpu_fusion_train_step", _lib.ptr(xd), _lib.ptr(yd), N, V, K, _lib.ptr(W), _lib.ptr(b), _lib.ptr(m), _lib.ptr(v),
                      t, *adam, _lib.ptr(ws), _lib.ptr(grads), _lib.ptr(loss), _lib.stream_ptr())
        W2, b2, m2, v2 = state(A, "2")                                    # the same two steps as sums + apply
        sums = A.carve(P + 2, torch.float64, name="sums")
        grads2, loss2 = A.carve(P, torch.float32, name="grads2"), A.carve(1, torch.float32, name="loss2")
        for t in (1, 2):
            _lib.call("mpu_fusion_grad_sums", _lib.ptr(xd), _lib.ptr(yd), N, V, K, _lib.ptr(W2), _lib.ptr(b2), _lib.ptr(ws),
                      _lib.ptr(sums), _lib.stream_ptr())
            _lib.call("mpu_fusion_apply_sums", _lib.ptr(sums), V, K, _lib.ptr(W2), _lib.ptr(b2), _lib.ptr(m2), _lib.ptr(v2), t, *adam,
                      _lib.ptr(grads2), _lib.ptr(loss2), _lib.stream_ptr())
        return dict(W=W, b=b, m=m, v=v, grads=grads, loss=loss, W2=W2, b2=b2, m2=m2, v2=v2, grads2=grads2, loss2=loss2, sums=sums,
                    probs=probs, labels=labels, probs_z=probs_z, labels_z=labels_z, Wf=Wf, bf=bf)
    got = under_three_poisons(4 * (N * V * K + 3 * N * K + n_ws + 14 * P + 8) + 3 * N, 28, body)
    assert np.array_equal(got["Wf"].numpy(), W0) and np.array_equal(got["bf"].numpy(), b0)       # (inputs of the forward: untouched)
    from oracle import geometry as OG
    from test_gpu_geometry import assert_labels_equal_outside_float_ties
    ref = OG.fusion_layer(x, W0, b0[0])
    for tag in ("", "_z"):
        np.testing.assert_allclose(got["probs" + tag].numpy(), ref, rtol=0, atol=1e-6, err_msg="probs" + tag)
        assert assert_labels_equal_outside_float_ties(got["labels" + tag].numpy(), ref.argmax(-1), ref, band=4e-6) <= 2, tag
    for k in ("W", "b", "m", "v", "grads", "loss"):
        assert torch.equal(bits(got[k]), bits(got[k + "2"])), k
    if K > 1:
        assert np.isfinite(got["loss"].numpy()).all() and not np.array_equal(got["W"].numpy(), W0)


# ---- mpu_eval_loss / mpu_eval_loss_logits / mpu_train_metrics_update -----------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 3, 8))
@pytest.mark.parametrize("ppi", (1, 255, 4097))
@pytest.mark.parametrize("B", (1, 3))
def test_guarded_eval_loss_and_metrics(B, ppi, K):
    """Every loss kind with its default arguments, the cross-entropy from logits, and the metrics update: scratch
    (mpu_eval_loss_scratch_bytes, "contents irrelevant"), per-image loss, the f64 accumulator, the metrics state
    (mpu_train_metrics_state_bytes) carved. Each result also equals an unguarded call's bit for bit."""
    import test_gpu_eval_loss as EL
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    p_all, y_all = EL._inputs(K)
    p, y = np.ascontiguousarray(p_all[:B, :ppi]), np.ascontiguousarray(y_all[:B, :ppi])
    sw = EL.SW[:B]
    n_scr, n_state = int(lib.mpu_eval_loss_scratch_bytes(B, ppi, K)), int(lib.mpu_train_metrics_state_bytes())
    assert n_scr > 0
    kinds = [(n, EL._cfg(n, EL._kw(kw, K), K)) for n, kw in EL.CASES[:6]]

    def run(scratch, loss_of, acc_of, state, pd, yd, swd, logits):
        res = {}
        for name, cfg in kinds:
            loss, acc = loss_of(name), acc_of(name)
            _lib.call("mpu_eval_loss", C.byref(cfg), _lib.ptr(pd), _lib.ptr(yd), _lib.ptr(swd), B, ppi, K, _lib.ptr(scratch),
                      _lib.ptr(loss), _lib.ptr(acc), _lib.stream_ptr())
            res[name], res[name + "/acc"] = loss, acc
        loss, acc = loss_of("logits"), acc_of("logits")
        _lib.call("mpu_eval_loss_logits", _lib.ptr(logits), _lib.ptr(yd), _lib.ptr(swd), B, ppi, K, _lib.ptr(scratch), _lib.ptr(loss),
                  _lib.ptr(acc), _lib.stream_ptr())
        res["logits"], res["logits/acc"] = loss, acc
        for _ in range(2):
            _lib.call("mpu_train_metrics_update", _lib.ptr(pd), _lib.ptr(yd), B * ppi, K, _lib.ptr(state), _lib.stream_ptr())
        res["metrics"] = state
        return res

    def body(A):
        pd, yd, swd = A.put(dev(p), "probs"), A.put(dev(y), "labels"), A.put(dev(sw), "sample_weight")
        logits = A.put(dev(p * 6 - 3), "logits")
        return run(A.carve(n_scr, torch.uint8, name="scratch"), lambda n: A.carve(B, torch.float32, name="loss " + n),
                   lambda n: A.carve(2, torch.float64, fill=ZERO, name="acc " + n),            # (an accumulator: zero starts it)
                   A.carve(n_state // 8, torch.float64, fill=ZERO, name="metrics state"),        # (all-zero = a fresh state)
                   pd, yd, swd, logits)
    got = under_three_poisons(B * ppi * (8 * K + 1) + n_scr + n_state + 1024, 24, body)
    plain = run(torch.zeros(n_scr, dtype=torch.uint8, device="cuda"), lambda n: torch.empty(B, dtype=torch.float32, device="cuda"),
                lambda n: torch.zeros(2, dtype=torch.float64, device="cuda"),
                torch.zeros(n_state // 8, dtype=torch.float64, device="cuda"), dev(p), dev(y), dev(sw), dev(p * 6 - 3))
    for k in got:
        assert torch.equal(bits(got[k]), bits(plain[k])), k
    assert float(got["metrics"][6]) == 2.0 * B * ppi and not bool(got["metrics"][12:].any())    # count of accuracy; scratch left zeroed


# ---- mpu_optimizer_step / mpu_adam_step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 7, 1025))
def test_guarded_optimizer_steps(n):
    """Every rule and flag combination of tests/optimizer_ref.py and the plain Adam entry point, three steps on n floats with
    params, gradients and every slot carved; bit-equal to the f32 restatement (the bound tests/test_gpu_optimizers.py measured)."""
    from test_gpu_optimizers import lib_config
    from multiplanarunet_amd import _lib
    rng = np.random.RandomState(n)
    p0 = rng.randn(n).astype(np.float32)
    gs = [rng.randn(n).astype(np.float32) for _ in range(3)]

    def body(A):
        res = {}
        gd = [A.put(dev(g), "g%d" % i) for i, g in enumerate(gs)]
        for i, cfg in enumerate(OR.ALL_CONFIGS):
            ns = OR.num_slots(cfg)
            p = A.put(dev(p0), "params %d" % i)
            slots = [A.carve(n, torch.float32, fill=ZERO, name="slot %d.%d" % (i, k)) for k in range(ns)]
            ptrs = (C.c_void_p * 3)(*[s.data_ptr() for s in slots] + [None] * (3 - ns))
            c = lib_config(cfg)
            for t in (1, 2, 3):
                _lib.call("mpu_optimizer_step", C.byref(c), _lib.ptr(p), _lib.ptr(gd[t - 1]), ptrs, n, t, None, _lib.stream_ptr())
            res["p%d" % i] = p
            res.update({"s%d.%d" % (i, k): s for k, s in enumerate(slots)})
        p = A.put(dev(p0), "params adam")
        m, v = (A.carve(n, torch.float32, fill=ZERO, name="adam " + s) for s in "mv")
        for t in (1, 2, 3):
            _lib.call("mpu_adam_step", _lib.ptr(p), _lib.ptr(gd[t - 1]), _lib.ptr(m), _lib.ptr(v), n, t, 0.01, 0.9, 0.999, 1e-8,
                      _lib.stream_ptr())
        res.update(adam_p=p, adam_m=m, adam_v=v)
        return res
    got = under_three_poisons(50 * 4 * n, 50, body)
    for i, cfg in enumerate(OR.ALL_CONFIGS):
        pr, sr = p0, [np.zeros(n, np.float32) for _ in range(OR.num_slots(cfg))]
        for t in (1, 2, 3):
            pr, sr = OR.step32(cfg, pr, gs[t - 1], sr, t)
        assert np.array_equal(got["p%d" % i].numpy().view(np.uint32), np.asarray(pr, np.float32).view(np.uint32)), cfg
        for k, r in enumerate(sr):
            assert np.array_equal(got["s%d.%d" % (i, k)].numpy().view(np.uint32), np.asarray(r, np.float32).view(np.uint32)), (cfg, k)


# ---- mpu_unet_adam_pack / mpu_unet_optimizer_pack ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [None] + OR.ALL_CONFIGS, ids=["plain-Adam"] + ["%d-%s" % (i, c[0]) for i, c in enumerate(OR.ALL_CONFIGS)])
def test_guarded_update_and_pack_t1(cfg):
    """The one-launch update + repack of the packed operands on T1, plain Adam (mpu_unet_adam_pack) and every other rule
    (mpu_unet_optimizer_pack): params, grads, slots and packed carved, bit-equal to the two separate passes."""
    from test_gpu_guard_unet import guarded_model
    from test_gpu_optimizers import compile_kwargs
    got = {}
    for fill in POISONS:
        for fused in (True, False):
            m, A, *_ = guarded_model("T1", "bf16", fill)
            two = list(m._slots)                                 # (guarded_model carved Adam's two)
            if cfg is not None:
                m.compile(cfg[0], optimizer_kwargs=compile_kwargs(cfg))
            ns = m._optimizer_config()[1]
            m._slots = two[:ns] + [A.carve(m.params.numel(), torch.float32, fill=ZERO, name="slot%d" % k) for k in range(2, ns)]
            m.grads.copy_(torch.randn(m.grads.numel(), generator=torch.Generator().manual_seed(5)).cuda())
            m.apply_gradients(fused=fused)
            m.apply_gradients(fused=fused)
            torch.cuda.synchronize()
            assert not A.check(), (cfg, fill, fused, A.check())
            got[fill, fused] = [bits(m.params), bits(m.packed)] + [bits(s) for s in m._slots]
    for key in got:
        assert all(torch.equal(a, b) for a, b in zip(got[NAN, True], got[key])), (cfg, key)


# ---- mpu_plane_stats -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", (1, 2))
@pytest.mark.parametrize("dim", (1, 31, 33))
def test_guarded_plane_stats(dim, Cn):
    """Labels (u8), image (f32 [n, C]), background values and the 8-byte statistics of one dim x dim plane carved; the call must
    clear its output whatever it held. Equal to NumPy (tests/test_gpu_sampler.py's reference) with the one differing pixel and
    label 31 (the mask's top bit) in the plane's last pixel, and with either input absent."""
    from test_gpu_sampler import ref_flag, ref_mask
    from multiplanarunet_amd import _lib
    n = dim * dim
    rng = np.random.RandomState(10 * dim + Cn)
    bg = rng.uniform(-2, 2, Cn).astype(np.float32)
    pool = np.array([0, 3, 9, 40, 255])                                  # (labels >= 32 leave the mask alone)
    y = pool[rng.randint(0, len(pool), n)].astype(np.uint8)
    y[n - 1] = 31
    for differs in (False, True):
        x = np.broadcast_to(bg, (n, Cn)).copy()
        if differs:
            x[n - 1, Cn - 1] += np.float32(0.5)

        def body(A):
            yd, xd, bd = A.put(dev(y), "labels"), A.put(dev(x), "image"), A.put(dev(bg), "bg")
            res = {}
            for name, (yy, xx) in (("both", (yd, xd)), ("labels only", (yd, None)), ("image only", (None, xd))):
                out = A.carve(2, torch.int32, name="stats " + name)
                _lib.call("mpu_plane_stats", _lib.ptr(yy), _lib.ptr(xx), n, 0 if xx is None else Cn, _lib.ptr(bd if xx is not None else None),
                          _lib.ptr(out), _lib.stream_ptr())
                res[name] = out
            return res
        got = under_three_poisons(n * (1 + 4 * Cn) + 64, 6, body)
        stats = {k: tuple(int(v) & 0xFFFFFFFF for v in t.tolist()) for k, t in got.items()}
        assert ref_mask(y) >> 31 == 1 and ref_flag(x, bg) == int(differs)
        assert stats == {"both": (ref_mask(y), int(differs)), "labels only": (ref_mask(y), 0), "image only": (0, int(differs))}, (differs, stats)


# ---- mpu_sample_view_planes / mpu_sample_view_planes_sc / mpu_sample_plane_stats -------------------------------------------------------
@pytest.mark.parametrize("Cn", (1, 2))
@pytest.mark.parametrize("dim", (2, 31, 33))
def test_guarded_sample_view(dim, Cn):
    """Planes out (f32) and labels out (u8) of one oblique view, dim planes of dim x dim (2 is the smallest the view geometry
    defines: its step divides by dim - 1), scaled per channel: through the scaler descriptor (sample_view), through
    mpu_sample_view_planes with its center / scale arrays, and plane by plane through mpu_sample_plane_stats, whose 8 bytes of
    statistics are carved too. All three give the bits of the unguarded call; the statistics are NumPy's on the plane."""
    import ctypes as C
    from test_gpu_sampler import ref_flag, ref_mask
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.interpolation import ViewGeometry, Volume, sample_view
    rng = np.random.RandomState(dim + Cn)
    image = rng.randn(20, 18, 22, Cn).astype(np.float32)
    labels = rng.randint(0, 4, (20, 18, 22)).astype(np.uint8)
    center, scale = np.linspace(0.25, 0.5, Cn), np.linspace(1.5, 2.0, Cn)
    vol = Volume(image, labels, np.diag([1.0, 1.5, 0.75, 1.0]), bg_value=[12.5] * Cn, scaler=(center, scale))
    geom = ViewGeometry([0.3, -0.5, 0.81], dim, 24.0, "same")
    bg_scaled = vol._scaler.transform_host(np.full((1, Cn), 12.5, np.float32))[0]
    shape = (C.c_int32 * 4)(*image.shape)
    planes = sorted({0, dim // 2, dim - 1})

    def body(A):
        res = dict(zip(("X", "y"), sample_view(vol, geom, out=A.carve((dim, dim, dim, Cn), torch.float32, name="planes"),
                                               out_labels=A.carve((dim, dim, dim), torch.uint8, name="labels"))))
        vd, ld = A.put(vol.image, "volume"), A.put(vol.labels, "volume labels")
        axes = [A.put(a, "axis %d" % k) for k, a in enumerate(vol._axes_dev)]
        offs, bgd = A.put(dev(geom.offsets), "offsets"), A.put(vol._bg, "bg")
        cd, sd = A.put(dev(center), "center"), A.put(dev(scale), "scale")
        g = geom.struct(vol.rot_mat, vol.axes)
        res["X2"], res["y2"] = A.carve((dim, dim, dim, Cn), torch.float32, name="planes 2"), A.carve((dim, dim, dim), torch.uint8, name="labels 2")
        _lib.call("mpu_sample_view_planes", _lib.ptr(vd), _lib.ptr(ld), shape, *[_lib.ptr(a) for a in axes], C.byref(g), _lib.ptr(offs),
                  _lib.ptr(bgd), vol.bg_class, _lib.ptr(cd), _lib.ptr(sd), _lib.ptr(res["X2"]), _lib.ptr(res["y2"]), _lib.stream_ptr())
        g.n_planes = 1                                                   # one candidate of the train sampler per call
        bsd = A.put(dev(bg_scaled), "bg scaled")
        for pl in planes:
            xs, ys = A.carve((dim, dim, Cn), torch.float32, name="plane %d" % pl), A.carve((dim, dim), torch.uint8, name="plane labels %d" % pl)
            st = A.carve(2, torch.int32, name="stats %d" % pl)
            _lib.call("mpu_sample_plane_stats", _lib.ptr(vd), _lib.ptr(ld), shape, *[_lib.ptr(a) for a in axes], C.byref(g),
                      _lib.ptr(offs[pl:pl + 1]), _lib.ptr(bgd), vol.bg_class, _lib.ptr(cd), _lib.ptr(sd), _lib.ptr(xs), _lib.ptr(ys),
                      _lib.ptr(bsd), _lib.ptr(st), _lib.stream_ptr())
            res["X%d" % pl], res["y%d" % pl], res["stats%d" % pl] = xs, ys, st
        return res
    nplane = dim * dim * (4 * Cn + 1)
    got = under_three_poisons((2 * dim + len(planes)) * nplane + image.nbytes + labels.nbytes + 4096, 16 + 3 * len(planes), body)
    X, y = sample_view(vol, geom)
    assert torch.equal(bits(got["X"]), bits(X)) and torch.equal(bits(got["y"]), bits(y))
    assert torch.equal(bits(got["X2"]), bits(X)) and torch.equal(bits(got["y2"]), bits(y))
    assert bool(torch.isfinite(got["X"]).all()) and (dim == 2 or bool((got["y"] != 0).any()))     # (dim 2: both planes lie outside)
    for pl in planes:
        assert torch.equal(bits(got["X%d" % pl]), bits(X[pl])) and torch.equal(bits(got["y%d" % pl]), bits(y[pl])), pl
        want = (ref_mask(y[pl].cpu().numpy().ravel()), ref_flag(X[pl].cpu().numpy().reshape(-1, Cn), bg_scaled))
        assert tuple(int(v) & 0xFFFFFFFF for v in got["stats%d" % pl].tolist()) == want, (pl, want)


# ---- mpu_map_view_*, mpu_map_accumulate_view*, mpu_map_fuse_views*, mpu_fusion_finalize ----------------------------------------------
def _map_cases(golden):
    """(volume, [(pred [P,dim,dim,K] host, grid, inv_basis)] per view) of two committed cases of tests/map_linear_cases.py and of
    thin voxel grids with extents 1, 2 and 33 under their views."""
    import map_linear_cases as MC
    from multiplanarunet_amd.interpolation import Volume
    out = []
    for an, K in (("rot", 3), ("aniso", 1)):
        vol = Volume(golden["g3_vol"], golden["g3_lab"], golden["aff_" + an], bg_value=[12.5])
        vps = []
        for v in MC.VIEWS[:2]:
            pred, grid, ib, _ = MC.case_inputs(golden, an, v, K)
            vps.append((np.ascontiguousarray(np.moveaxis(pred, 2, 0)), grid, ib))
        out.append(("%s K=%d" % (an, K), vol, vps))
    _, grid, ib, _ = MC.case_inputs(golden, "rot", 6, 3)
    pred = np.ascontiguousarray(np.moveaxis(MC.case_inputs(golden, "rot", 6, 3)[0], 2, 0))
    for shape in ((1, 2, 33), (33, 1, 2), (2, 33, 1)):
        vol = Volume(np.zeros(shape + (1,), np.float32), None, np.diag([0.5, 0.5, 0.5, 1.0]))
        out.append(("thin %s" % (shape,), vol, [(pred, grid, ib), (pred[::-1].copy(), grid, ib)]))
    return out


@pytest.mark.parametrize("method", ("nearest", "linear"))
def test_guarded_back_mapping_and_fusion(golden, method):
    """One view mapped, the views fused in one launch, and the plane-sharded accumulate + finalize: predictions, voxel grids
    (f32), the accumulator and the fused probabilities / labels (u8) carved; equal to the unguarded calls bit for bit."""
    from multiplanarunet_amd.interpolation import fusion_finalize, linear_chunk_planes, map_accumulate, map_and_fuse, map_real_space_pred
    for tag, vol, vps in _map_cases(golden):
        X, Y, Z = (int(v) for v in vol.image.shape[:3])
        V, (P, dim, _, K) = len(vps), vps[0][0].shape
        rng = np.random.RandomState(5)
        W = rng.uniform(0.5, 1.5, (V, K)).astype(np.float32)
        b = rng.uniform(-0.2, 0.2, (K,)).astype(np.float32)
        cuts = [0, 7, 20, P]

        def run(carve, put):
            preds = [put(dev(p)) for p, _, _ in vps]
            res = {"mapped": map_real_space_pred(preds[0].permute(1, 2, 0, 3), vps[0][1], vps[0][2], vol, method=method,
                                                 out=carve((X, Y, Z, K), torch.float32))}
            res["probs"], res["labels"] = map_and_fuse(vol, [(p, g, ib) for p, (_, g, ib) in zip(preds, vps)], W, b, method=method,
                                                       out_probs=carve((X, Y, Z, K), torch.float32), out_labels=carve((X, Y, Z), torch.uint8))
            z = carve((X, Y, Z, K), torch.float32)
            z.zero_()                                                        # (an accumulator: zero starts it)
            for vi, (p, (_, g, ib)) in enumerate(zip(preds, vps)):
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    lo_, hi_ = linear_chunk_planes(lo, hi, P) if method == "linear" else (lo, hi)
                    map_accumulate(vol, put(p[lo_:hi_].contiguous()), g, ib, W[vi], lo, hi, lo == 0, z, method=method)
            res["z"] = z
            res["probs2"], res["labels2"] = fusion_finalize(z, b, out_probs=carve((X, Y, Z, K), torch.float32),
                                                            out_labels=carve((X, Y, Z), torch.uint8))
            return res
        nvox = X * Y * Z
        got = under_three_poisons(2 * V * 4 * P * dim * dim * K + nvox * (16 * K + 2) + (1 << 20), 6 + 4 * V, lambda A: run(A.carve, A.put))
        plain = run(lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda"), lambda t: t)
        for k in got:
            assert torch.equal(bits(got[k]), bits(plain[k])), (tag, method, k)
        assert float(np.abs(got["probs2"].numpy() - got["probs"].numpy()).max()) <= 2e-6, tag       # (tests/test_gpu_map_linear.py's bound)
