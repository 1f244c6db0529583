"""
GPU parity of the linear back-mapping (mpu_map_view_linear / mpu_map_fuse_views_linear / mpu_map_accumulate_view_linear)
through the host layer: map_real_space_pred(method="linear") is held to EXACT equality with the reference's own outputs
(tests/golden/map_linear_golden*.npz) and with the oracle composition that tests/test_map_linear_host.py ties to them;
the fused and the plane-sharded forms to the float bounds of the nearest path's fused test (probabilities 2e-6, labels
identical outside the float tie band, at most 4 differing inside it).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_linear_cases as MC                                                          # noqa: E402

pytestmark = pytest.mark.gpu


def _vol(golden, an):
    from multiplanarunet_amd.interpolation import Volume
    return Volume(golden["g3_vol"], golden["g3_lab"], golden["aff_" + an], bg_value=[12.5])


def _map(golden, an, pred, grid, ib, method):
    from multiplanarunet_amd.interpolation import map_real_space_pred
    out = map_real_space_pred(torch.tensor(pred, device="cuda"), grid, ib, _vol(golden, an), method=method)
    return out.cpu().numpy()


@pytest.mark.parametrize("an,v,K", MC.GOLDEN_CASES)
def test_map_linear_vs_reference_golden(golden, an, v, K):
    pred, grid, ib, _ = MC.case_inputs(golden, an, v, K)
    got = _map(golden, an, pred, grid, ib, "linear")
    np.testing.assert_array_equal(got, MC.linear_golden()["lin_map_%s_%d_%d" % (an, v, K)])     # bit for bit


@pytest.mark.parametrize("an,v,K", MC.ALL_CASES)
def test_map_linear_vs_oracle(golden, an, v, K):
    pred, grid, ib, _ = MC.case_inputs(golden, an, v, K)
    ref, oob = MC.oracle_case(golden, an, v, K)
    got = _map(golden, an, pred, grid, ib, "linear")
    near = _map(golden, an, pred, grid, ib, "nearest")
    oob_share = float(oob.mean())
    differs = float((got != near).any(axis=-1).mean())
    print("%s view %d K %d: out-of-box share %.4f, differs from nearest in %.4f of the voxels" % (an, v, K, oob_share, differs))
    np.testing.assert_array_equal(got, ref)
    assert oob_share <= 0.34                   # not satisfied by fill vectors ...
    assert differs > 0.5                       # ... nor by a fallback to nearest


def test_map_linear_sixteen_classes(golden):
    """The register-pressure corner: eight 16-wide corners in flight."""
    _, grid, ib, vg = MC.case_inputs(golden, "rot", 6, 3)
    pred = np.random.RandomState(16).rand(16, 16, 36, 16).astype(np.float32)
    ref = MC.oracle_map_linear(pred, grid, ib, vg)
    np.testing.assert_array_equal(_map(golden, "rot", pred, grid, ib, "linear"), ref)


def test_axis_ends_first_and_last_nodes():
    """Identity orientation, voxel size 0.5, integer axes: voxel centres fall exactly on the first and the last node of g and
    of the offsets (and on every node and half-way point between); the last node is in bounds (cell n-2, y = 1: the value
    AT the node), the first voxel beyond it takes the fill vector."""
    from multiplanarunet_amd.interpolation import Volume, map_real_space_pred
    from oracle import geometry as G
    K, dim, P = 3, 9, 11
    g = np.linspace(-4.0, 4.0, dim)
    offs = np.linspace(-5.0, 5.0, P)
    assert np.array_equal(g, np.arange(-4.0, 5.0)) and np.array_equal(offs, np.arange(-5.0, 6.0))
    shape = (23, 17, 25)                                   # x: -5.5 .. 5.5, y: -4 .. 4, z: -6 .. 6 in steps of 0.5
    aff = np.diag([0.5, 0.5, 0.5, 1.0])
    vg = G.voxel_grid_real_space(shape, aff)
    assert vg[0][19, 0, 0] == 4.0 and vg[0][3, 0, 0] == -4.0 and vg[1][0, 16, 0] == 4.0 and vg[1][0, 0, 0] == -4.0
    assert vg[2][0, 0, 22] == 5.0 and vg[2][0, 0, 2] == -5.0
    pred = np.random.RandomState(3).rand(dim, dim, P, K).astype(np.float32)
    ib = np.eye(3)
    ref = MC.oracle_map_linear(pred, (g, g, offs), ib, vg)
    vol = Volume(np.zeros(shape + (1,), np.float32), None, aff)
    got = map_real_space_pred(torch.tensor(pred, device="cuda"), (g, g, offs), ib, vol, method="linear").cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    fill = np.array([1.0, 0.0, 0.0], np.float32)
    np.testing.assert_array_equal(got[19, 16, 22], pred[dim - 1, dim - 1, P - 1])       # all three axes ON the last node
    np.testing.assert_array_equal(got[3, 0, 2], pred[0, 0, 0])                           # ... and on the first
    np.testing.assert_array_equal(got[20, 16, 22], fill)                                 # first voxel beyond g's last node
    np.testing.assert_array_equal(got[19, 16, 23], fill)                                 # ... beyond the last offset
    np.testing.assert_array_equal(got[2, 0, 2], fill)
    np.testing.assert_array_equal(got[3, 0, 1], fill)
    np.testing.assert_array_equal(got[19, 8, 12], pred[dim - 1, 4, 5])                   # last node of one axis, inner nodes


def _fused_inputs(golden, an, K=3):
    rng = np.random.RandomState(5)
    W = rng.uniform(0.5, 1.5, (len(MC.VIEWS), K)).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, (K,)).astype(np.float32)
    combined, vps = [], []
    for v in MC.VIEWS:
        pred, grid, ib, _ = MC.case_inputs(golden, an, v, K)
        combined.append(MC.oracle_case(golden, an, v, K)[0])
        vps.append((torch.tensor(np.moveaxis(pred, 2, 0).copy(), device="cuda"), grid, ib))
    return W, b, np.stack(combined), vps


@pytest.mark.parametrize("an", MC.AFFS)
@pytest.mark.parametrize("sum_fusion", (False, True))
def test_fused_and_sharded_linear_vs_oracle(golden, an, sum_fusion):
    """Stacked oracle maps -> oracle merge vs the fused kernel; the plane-sharded accumulate (chunk + one halo plane, voxels
    owned by cell) + finalize vs the fused kernel, for the cut lists [0, 7, 20, P] and [0, P-1, P] (a last chunk of one
    plane, which owns nothing)."""
    from multiplanarunet_amd.interpolation import map_and_fuse, map_accumulate, fusion_finalize
    from oracle import geometry as G
    K = 3
    vol = _vol(golden, an)
    W, b, combined, vps = _fused_inputs(golden, an, K)
    merged_ref, map_ref = G.merge_multi_view_preds(combined, W, b, sum_fusion)
    probs, labels = map_and_fuse(vol, vps, W, b, sum_fusion=sum_fusion, method="linear")
    torch.cuda.synchronize()
    p = probs.cpu().numpy()
    err = float(np.abs(p - merged_ref).max())
    n_ties = MC.labels_equal_outside_float_ties(labels.cpu().numpy(), map_ref, merged_ref)
    print("fused linear %s sum_fusion=%s: max |p - oracle| %.3g, %d labels differ inside the tie band" % (an, sum_fusion, err, n_ties))
    assert err <= 2e-6
    assert n_ties <= 4, n_ties
    # labels alone (probs == NULL) are the same labels
    _, l_only = map_and_fuse(vol, vps, W, b, sum_fusion=sum_fusion, want_probs=False, method="linear")
    np.testing.assert_array_equal(l_only.cpu().numpy(), labels.cpu().numpy())
    P = int(vps[0][0].shape[0])
    for cuts in ([0, 7, 20, P], [0, P - 1, P]):
        z = torch.zeros_like(probs)
        for vi, (pr, grid, ib) in enumerate(vps):
            Wv = np.ones(K, np.float32) if sum_fusion else W[vi]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                map_accumulate(vol, pr[lo:min(hi + 1, P)].contiguous(), grid, ib, Wv, lo, hi, lo == 0, z, method="linear")
        p2, l2 = fusion_finalize(z, b, sum_fusion=sum_fusion)
        np.testing.assert_allclose(p2.cpu().numpy(), p, rtol=0, atol=2e-6)
        assert MC.labels_equal_outside_float_ties(l2.cpu().numpy(), labels.cpu().numpy(), p) <= 4


@pytest.mark.parametrize("an", ("aniso", "rot"))
def test_closed_form_cells_equal_the_exact_search(golden, an):
    """find_cell's closed-form cell on the uniform axes (the only fast form the linear kernels use) against the exact search
    for every lookup (mpu_geometry_set_fast_path(0)): 96^3 voxels, dim 96, an oblique view -- bit for bit."""
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.interpolation import Volume, ViewGeometry, map_real_space_pred
    K, dim = 3, 96
    geom = ViewGeometry(golden["views"][6], dim, 100.0, "same+20")
    grid = (geom.real_axis, geom.real_axis, geom.offsets)
    pred = torch.rand((dim, dim, geom.n_planes, K), device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    vol = Volume(np.zeros((96, 96, 96, 1), np.float32), None, golden["aff_" + an])
    fast = map_real_space_pred(pred, grid, geom.inv_basis, vol, method="linear")
    try:
        _lib.call("mpu_geometry_set_fast_path", 0)
        exact = map_real_space_pred(pred, grid, geom.inv_basis, vol, method="linear")
    finally:
        _lib.call("mpu_geometry_set_fast_path", 1)
    assert torch.equal(fast, exact)
    inside = float((fast[..., 0] != 1.0).float().mean())
    print("%s: %.3f of the 96^3 voxels interpolated" % (an, inside))
    # not vacuous: the view's box (100 x 100 x 121, centred) holds the centred ball of radius 50, and the part of that ball inside
    # the grid's own box (96 x 48 x 192 / 96 x 76.8 x 144) is 0.38 / 0.45 of the grid
    assert inside > 0.25


def test_mp_predict_and_train_fusion_with_linear_map(tmp_path, capsys):
    """End to end on a freshly trained toy project: `mp predict --map_method linear` writes the prediction, logs the method
    and runs the per-view evaluation; `mp train_fusion --map_method linear` fits weights on linearly mapped points that the
    linear predict then uses."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text(
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 64\n  depth: 3\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 64.0\n  batch_size: 8\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: SparseCategoricalCrossentropy\n  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n")
    mp.entry_func(["train", "--project_dir", str(proj), "--synthetic", "4", "--epochs", "2",
                   "--train_images_per_epoch", "32", "--val_images_per_epoch", "16"])
    capsys.readouterr()
    mp.entry_func(["predict", "--project_dir", str(proj), "--synthetic", "1", "--sum_fusion", "--map_method", "linear",
                   "--eval_prob", "1.0"])
    out = capsys.readouterr().out
    assert "Back-mapping method: linear" in out
    dst = proj / "predictions" / "nii_files" / "toy_5000_PRED.npz"
    assert dst.exists()
    lab = np.load(dst)["labels"]
    assert lab.shape == (64, 64, 64) and lab.dtype == np.uint8
    pv = (proj / "predictions" / "csv" / "per_view.csv").read_text().splitlines()
    assert pv[0].startswith("image,view_index,view,mean_dice,class_0") and len(pv) == 1 + 3
    mp.entry_func(["train_fusion", "--project_dir", str(proj), "--synthetic", "1", "--epochs", "1", "--images_per_round", "1",
                   "--batch_size", "65536", "--seed", "0", "--map_method", "linear"])
    assert "Back-mapping method: linear" in capsys.readouterr().out
    assert len(os.listdir(proj / "model" / "fusion_weights")) == 1
    mp.entry_func(["predict", "--project_dir", str(proj), "--synthetic", "1", "--overwrite", "--map_method", "linear"])
    assert "Back-mapping method: linear" in capsys.readouterr().out
    assert np.load(dst)["labels"].shape == (64, 64, 64)


def test_sharded_predict_host_path_with_linear_map(monkeypatch):
    """multi_view_predict_sharded(map_method="linear") in one process, its work items cut into three plane chunks per view (each
    sampled and predicted with its halo plane), and the all_gather scheme: the label volume of multi_view_predict(map_method=
    "linear"). The chunks change the U-Net's batches, so the bound is the one the two-rank nearest test uses for that reason:
    at most 1e-4 of the labels (near-ties of two classes) may differ."""
    from multiplanarunet_amd import distributed as D
    from multiplanarunet_amd.unet import UNet
    from multiplanarunet_amd.fusion_model import FusionModel
    from multiplanarunet_amd.interpolation import Volume
    from multiplanarunet_amd.predict import multi_view_predict
    quiet = lambda *a, **k: None
    rng = np.random.RandomState(0)
    Dv, K = 32, 3
    vol = (rng.randn(Dv, Dv, Dv - 3, 1) * 40 + 90).astype(np.float32)
    views = np.array([[0, 0, 1], [1, 0, 0], [0.3, 0.5, 0.8]], float)
    model = UNet(n_classes=K, dim=Dv, depth=2, dtype="f32", logger=quiet, seed=3)
    fm = FusionModel(len(views), K, verbose=False)
    fm.set_weights([rng.uniform(.5, 1.5, (3, K)).astype(np.float32), rng.uniform(-.1, .1, (1, K)).astype(np.float32)])
    v = Volume(vol, None, np.eye(4), bg_value=[0.0])
    _, ref = multi_view_predict(model, v, views, Dv, float(Dv), fm, batch_size=8, map_method="linear")
    _, near = multi_view_predict(model, v, views, Dv, float(Dv), fm, batch_size=8)
    items = D.plane_work_items
    monkeypatch.setattr(D, "plane_work_items", lambda V, P, world: items(V, P, world, chunks_per_view=3))
    assert len(D.plane_work_items(3, Dv + 20, 1)[0]) == 9
    got = D.multi_view_predict_sharded(model, v, views, Dv, float(Dv), fm, batch_size=8, map_method="linear")
    got2 = D.multi_view_predict_sharded(model, v, views, Dv, float(Dv), fm, batch_size=8, exchange="all_gather", map_method="linear")
    for g in (got, got2):
        share = float((g != ref).float().mean().item())
        print("sharded linear labels differing from the single-process ones: %.2e (from the nearest ones: %.2e)"
              % (share, float((g != near).float().mean().item())))
        assert tuple(g.shape) == tuple(ref.shape) and share <= 1e-4
    with pytest.raises(NotImplementedError):
        D.multi_view_predict_sharded(model, v, views, Dv, float(Dv), fm, batch_size=8, map_method="kNN")
