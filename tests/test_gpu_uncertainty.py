"""
The per-voxel uncertainty of the fusion on the GPU (mpu_map_fuse_views_uncertainty through uncertainty.fuse_with_uncertainty,
mpu_uncertainty_table, `mp predict --uncertainty`) against the fp64 restatement tests/uncertainty_ref.py.

Inputs: the committed cases of tests/golden/geometry_golden.npz (voxel grid 32 x 28 x 24, view predictions [16,16,36,K], the four
views 0, 1, 5, 6 of one affine fused together, every row divided by its sum; a second set with the rows raised to the 6th power
first, so that confident views and low entropies are covered too), and synthetic identity-affine grids for the corners.
  labels, probs   bit-identical to map_and_fuse on the same inputs, fast path on and off
  agreement       exactly the restatement's count against the labels the call returned
  entropy         within 1e-5 of the fp64 Hn of the f32 probabilities the same call returned
  mi              within 3e-5 of the fp64 restatement on the x_v that map_real_space_pred returns
(<= 16 terms p logf(p), each <= 0.37 and a few ulp off, an f32 sum of at most ln 16, one normalisation; mi is a difference of two
such values plus a mean.)
"""
import contextlib
import gzip
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                                          # noqa: E402
import map_linear_cases as MC                                                          # noqa: E402
import uncertainty_ref as UR                                                           # noqa: E402
from guarded import POISONS, NAN, ZERO                                                  # noqa: E402

pytestmark = pytest.mark.gpu
ENT_TOL, MI_TOL = 1e-5, 3e-5
METHODS = ("nearest", "linear")


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def same_bits(a, b):
    return torch.equal(guarded.bits(a), guarded.bits(b))


@contextlib.contextmanager
def exact_search():
    from multiplanarunet_amd import _lib
    _lib.call("mpu_geometry_set_fast_path", 0)
    try:
        yield
    finally:
        _lib.call("mpu_geometry_set_fast_path", 1)


def run_and_check(vol, vps, W, b, sum_fusion, method):
    """One call with all outputs, held to the module text's four conditions. -> dict of host arrays (x: the views' vectors)."""
    from multiplanarunet_amd.interpolation import map_and_fuse, map_real_space_pred
    from multiplanarunet_amd.uncertainty import fuse_with_uncertainty
    probs, labels, maps = fuse_with_uncertainty(vol, vps, W, b, sum_fusion=sum_fusion, method=method, want_probs=True)
    again = fuse_with_uncertainty(vol, vps, W, b, sum_fusion=sum_fusion, method=method, want_probs=True)
    with exact_search():
        exact = fuse_with_uncertainty(vol, vps, W, b, sum_fusion=sum_fusion, method=method, want_probs=True)
        p_exact, l_exact = map_and_fuse(vol, vps, W, b, sum_fusion=sum_fusion, method=method)
    p_plain, l_plain = map_and_fuse(vol, vps, W, b, sum_fusion=sum_fusion, method=method)
    torch.cuda.synchronize()
    for other in (again, exact):                               # two calls, and the exact search for every lookup: the same bytes
        assert same_bits(probs, other[0]) and same_bits(labels, other[1])
        for k in maps:
            assert same_bits(maps[k], other[2][k]), k
    for p_ref, l_ref in ((p_plain, l_plain), (p_exact, l_exact)):
        assert same_bits(probs, p_ref), "probabilities differ from map_and_fuse: the kernel's arithmetic order is wrong"
        assert same_bits(labels, l_ref)
    x = np.stack([map_real_space_pred(vp[0].permute(1, 2, 0, 3), vp[1], vp[2], vol, method=method).cpu().numpy() for vp in vps])
    p, lab = probs.cpu().numpy(), labels.cpu().numpy()
    ent, mi, agree = (maps[k].cpu().numpy() for k in ("entropy", "mi", "agreement"))
    assert ent.dtype == np.float32 and mi.dtype == np.float32 and agree.dtype == np.uint8 and ent.shape == lab.shape == mi.shape
    ref_mi = UR.mutual_information(x)
    e_ent, e_mi = float(np.abs(ent - UR.entropy(p)).max()), float(np.abs(mi - ref_mi).max())
    print("%s V=%d K=%d sum_fusion=%s: max entropy error %.3g, max mi error %.3g" % (method, len(vps), p.shape[-1], sum_fusion, e_ent, e_mi))
    np.testing.assert_array_equal(agree, UR.agreement(x, lab))
    assert e_ent <= ENT_TOL and e_mi <= MI_TOL
    assert ent.min() >= 0.0 and ent.max() <= 1.0 and mi.min() >= 0.0 and mi.max() <= 1.0
    return dict(x=x, probs=p, labels=lab, entropy=ent, mi=mi, agreement=agree, dev=(labels, maps))


# ---- the committed cases -------------------------------------------------------------------------------------------------------------
_cases = {}


def golden_case(golden, an, K, method, sum_fusion=False, sharp=False):
    """The four views of affine `an` fused (computed and checked once, shared, never modified)."""
    key = (an, K, method, sum_fusion, sharp)
    if key not in _cases:
        from multiplanarunet_amd.interpolation import Volume
        W, b = _weights(K)
        vps = []
        for v in MC.VIEWS:
            pred, grid, ib, _ = MC.case_inputs(golden, an, v, K)
            pred = pred.astype(np.float64) ** (6 if sharp else 1)
            pred = (pred / pred.sum(-1, keepdims=True)).astype(np.float32)
            vps.append((dev(np.moveaxis(pred, 2, 0)), grid, ib))
        vol = Volume(golden["g3_vol"], golden["g3_lab"], golden["aff_" + an], bg_value=[12.5])
        _cases[key] = run_and_check(vol, vps, W, b, sum_fusion, method)
    return _cases[key]


def oob_shares(golden, an, K):
    from oracle import geometry as G
    out = []
    for v in MC.VIEWS:
        _, grid, ib, vg = MC.case_inputs(golden, an, v, K)
        pts = np.stack([vg[i].ravel() for i in range(3)], axis=1)
        out.append(float(G.rgi_find_indices(ib.dot(pts.T).T.T, grid)[2].mean()))
    return out


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", MC.KS)
@pytest.mark.parametrize("an", MC.AFFS)
def test_committed_cases(golden, an, K, method):
    r = golden_case(golden, an, K, method)
    oracle_ent, oracle_mi, oracle_agree, _ = UR.uncertainty(r["x"], *_weights(K))
    shares = np.bincount(oracle_agree.ravel(), minlength=5) / oracle_agree.size
    print("%s K=%d %s: oracle agreement shares %s, mean entropy %.3f, mean mi %.3f" % (an, K, method, np.round(shares, 3),
                                                                                       oracle_ent.mean(), oracle_mi.mean()))
    assert max(oob_shares(golden, an, K)) <= 0.34              # not satisfied by fill vectors
    if K == 1:
        assert not r["entropy"].any() and not r["mi"].any() and np.all(r["agreement"] == len(MC.VIEWS))
        return
    # (K = 5: rows of five uniform numbers are flat, the fused entropy of ident is 0.96 to 0.97; test_confident_views covers the range)
    assert 0.05 < oracle_mi.mean() < 0.95 and 0.05 < oracle_ent.mean() < (0.95 if K == 3 else 1.0)
    if K == 3:
        assert int((shares >= 0.05).sum()) >= 3, shares


def _weights(K):
    rng = np.random.RandomState(100 + K)
    return (rng.rand(len(MC.VIEWS), K) + 0.5).astype(np.float32), (0.1 * rng.randn(K)).astype(np.float32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", (3, 5))
def test_confident_views(golden, K, method):
    """Rows raised to the 6th power: views that are sure of themselves and contradict each other, entropies over the whole range."""
    r = golden_case(golden, "rot", K, method, sharp=True)
    ent, mi, _, _ = UR.uncertainty(r["x"], *_weights(K))
    print("confident views K=%d %s: mean entropy %.3f (min %.3f), mean mi %.3f (max %.3f)" % (K, method, ent.mean(), ent.min(), mi.mean(), mi.max()))
    assert 0.05 < ent.mean() < 0.95 and 0.05 < mi.mean() < 0.95
    assert ent.min() < 0.5 and mi.max() > 0.3


@pytest.mark.parametrize("method", METHODS)
def test_sum_fusion(golden, method):
    r = golden_case(golden, "rot", 3, method, sum_fusion=True)
    np.testing.assert_array_equal(r["labels"], r["probs"].argmax(-1))
    assert 0.05 < r["entropy"].mean() < 1.0


# ---- corners on synthetic identity-affine grids -----------------------------------------------------------------------------------
def synthetic(shape, K, V, seed, spacing=(0.5, 0.5, 0.5), repeat=False):
    """Voxel centres on the nodes, the ties and both ends of integer axes (test_gpu_map_linear.test_axis_ends_first_and_last_nodes);
    the views differ by an axis permutation / an oblique rotation, or (repeat) are ONE view under different weights."""
    from multiplanarunet_amd.interpolation import Volume
    rng = np.random.RandomState(seed)
    dim, P = 9, 11
    g, offs = np.linspace(-4.0, 4.0, dim), np.linspace(-5.0, 5.0, P)
    c, s = np.cos(0.5), np.sin(0.5)
    bases = [np.eye(3), np.eye(3)[[1, 2, 0]], np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), np.eye(3)[[2, 0, 1]]]
    vps = []
    for v in range(V):
        if repeat and v:
            vps.append(vps[0])
            continue
        pred = rng.rand(P, dim, dim, K) ** 3
        pred = (pred / pred.sum(-1, keepdims=True)).astype(np.float32)
        vps.append((dev(pred), (g, g, offs), bases[v % len(bases)]))
    W = (rng.rand(V, K) + 0.5).astype(np.float32)
    b = (0.1 * rng.randn(K)).astype(np.float32)
    vol = Volume(np.zeros(tuple(shape) + (1,), np.float32), None, np.diag(list(spacing) + [1.0]))
    return vol, vps, W, b


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", (9, 16))
def test_wide_classes_second_accumulator(K, method):
    r = run_and_check(*synthetic((23, 17, 25), K, 3, K), False, method)
    assert len(np.unique(r["agreement"])) >= 3 and r["mi"].max() > 0.1


@pytest.mark.parametrize("method", METHODS)
def test_one_view(method):
    vol, vps, W, b = synthetic((23, 17, 25), 3, 1, 1)
    # (equal weights and no bias, or the plain sum: the fused vector orders the classes as the view does)
    for r in (run_and_check(vol, vps, np.ones_like(W), np.zeros_like(b), False, method), run_and_check(vol, vps, None, None, True, method)):
        assert r["mi"].max() <= MI_TOL and np.all(r["agreement"] == 1)
        assert r["entropy"].max() > 0.5
    r = run_and_check(vol, vps, W, b, False, method)             # a weight per class can turn the one view's vote over
    assert r["mi"].max() <= MI_TOL and set(np.unique(r["agreement"])) <= {0, 1}


@pytest.mark.parametrize("method", METHODS)
def test_sixteen_views_of_one_prediction(method):
    """MAX_VIEWS, the whole vote word: the same view under 16 different weight rows."""
    r = run_and_check(*synthetic((23, 17, 25), 5, 16, 2, repeat=True), False, method)
    votes = np.unique(r["agreement"])                                      # one opinion: all 16 agree with the fused label, or none
    assert r["mi"].max() <= MI_TOL and set(votes) <= {0, 16} and 16 in votes
    r = run_and_check(*synthetic((9, 10, 21), 4, 16, 3), False, method)     # ... and 16 votes that differ
    assert len(np.unique(r["agreement"])) >= 4 and r["agreement"].max() <= 16


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", (3, 5, 9))
def test_brick_tails_on_all_three_axes(K, method):
    """5 x 7 x 70: tails of the 4 x 4 x (16 n) brick in x, y and z for n = 4, 2 and 1, more than one brick in z."""
    r = run_and_check(*synthetic((5, 7, 70), K, 3, 7 + K, spacing=(0.5, 0.5, 0.15)), False, method)
    assert (r["x"][:, :, :, :, 0] != 1.0).mean() > 0.3                      # not fill vectors


@pytest.mark.parametrize("method", METHODS)
def test_each_map_alone_and_no_probs(golden, method):
    from multiplanarunet_amd.uncertainty import fuse_with_uncertainty, MAPS
    full = golden_case(golden, "aniso", 3, method)
    vol, vps, W, b = _aniso_inputs(golden)
    for drop in MAPS:
        keep = tuple(m for m in MAPS if m != drop)
        probs, labels, maps = fuse_with_uncertainty(vol, vps, W, b, method=method, maps=keep)
        assert probs is None and sorted(maps) == sorted(keep)
        assert same_bits(labels, full["labels"])
        for m in keep:
            assert same_bits(maps[m], full[m]), (drop, m)
    _, labels, maps = fuse_with_uncertainty(vol, vps, W, b, method=method, maps="agreement", want_probs=False)
    assert same_bits(maps["agreement"], full["agreement"]) and same_bits(labels, full["labels"])


def _aniso_inputs(golden):
    from multiplanarunet_amd.interpolation import Volume
    vps = []
    for v in MC.VIEWS:
        pred, grid, ib, _ = MC.case_inputs(golden, "aniso", v, 3)
        pred = pred.astype(np.float64)
        vps.append((dev(np.moveaxis((pred / pred.sum(-1, keepdims=True)).astype(np.float32), 2, 0)), grid, ib))
    return (Volume(golden["g3_vol"], golden["g3_lab"], golden["aff_aniso"], bg_value=[12.5]), vps) + _weights(3)


def test_multi_view_predict_keyword():
    """predict.multi_view_predict(uncertainty={...}): the same labels as without, the dict filled with the maps asked for."""
    from multiplanarunet_amd.unet import UNet
    from multiplanarunet_amd.interpolation import Volume
    from multiplanarunet_amd.predict import multi_view_predict
    rng = np.random.RandomState(0)
    Dv, K = 32, 3
    vol = Volume((rng.randn(Dv, Dv, Dv - 3, 1) * 40 + 90).astype(np.float32), None, np.eye(4), bg_value=[0.0])
    views = np.array([[0, 0, 1], [1, 0, 0], [0.3, 0.5, 0.8]], float)
    model = UNet(n_classes=K, dim=Dv, depth=2, dtype="f32", logger=lambda *a, **k: None, seed=3)
    p0, l0 = multi_view_predict(model, vol, views, Dv, float(Dv), None, sum_fusion=True, batch_size=8)
    u = {"maps": ("entropy", "agreement")}
    p1, l1 = multi_view_predict(model, vol, views, Dv, float(Dv), None, sum_fusion=True, batch_size=8, uncertainty=u)
    assert same_bits(p0, p1) and same_bits(l0, l1)
    assert sorted(u) == ["agreement", "entropy", "maps"] and tuple(u["entropy"].shape) == tuple(l1.shape)
    assert u["agreement"].dtype == torch.uint8 and int(u["agreement"].max()) <= 3


# ---- mpu_uncertainty_table ---------------------------------------------------------------------------------------------------------
def table_inputs(golden):
    r = golden_case(golden, "rot", 3, "nearest")
    rng = np.random.RandomState(11)
    truth = np.where(rng.rand(*r["labels"].shape) < 0.3, rng.randint(0, 3, r["labels"].shape), r["labels"]).astype(np.uint8)
    return r, truth


def check_table(got, ref):
    assert sorted(got) == sorted(ref)
    for k in ref:
        if k.startswith("n"):
            np.testing.assert_array_equal(got[k], ref[k])                    # counts: exact
        else:
            assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
            ok = ~np.isnan(ref[k])
            assert np.abs(got[k][ok] - ref[k][ok]).max(initial=0.0) <= 1e-8, (k, got[k], ref[k])


@pytest.mark.parametrize("with_truth", (False, True))
def test_table_against_numpy(golden, with_truth):
    from multiplanarunet_amd.uncertainty import uncertainty_table
    r, truth = table_inputs(golden)
    labels, maps = r["dev"]
    host = {k: r[k] for k in ("entropy", "mi", "agreement")}
    K = 4                                                       # class 3 is in no voxel: NaN
    got = uncertainty_table(labels, maps, K, truth=dev(truth) if with_truth else None)
    ref = UR.table(r["labels"], host, K, truth if with_truth else None)
    check_table(got, ref)
    np.testing.assert_array_equal(got["n"], np.bincount(r["labels"].ravel(), minlength=K))
    assert got["n"][3] == 0 and np.isnan(got["mean_entropy"][3]) and got["n"][:3].min() > 0
    if with_truth:
        np.testing.assert_array_equal(got["n_correct"] + got["n_wrong"], got["n"])
        assert got["n_wrong"][:3].min() > 0
    # a subset of the maps: the others are NaN, the counts stay
    sub = uncertainty_table(labels, {"mi": maps["mi"]}, K)
    np.testing.assert_array_equal(sub["n"], got["n"])
    np.testing.assert_array_equal(sub["mean_mi"][:3], uncertainty_table(labels, maps, K)["mean_mi"][:3])
    assert np.isnan(sub["mean_entropy"]).all() and np.isnan(sub["mean_agreement"]).all()


def test_table_guarded_buffers_under_three_poisons_and_twice(golden):
    """Every buffer of the call carved from a guarded arena of 0xFF, 0x00 and 0x7B bytes: no guard byte changes, inputs stay, and
    the table is the same bytes three times and on a second call (integer sums: no order can show)."""
    from multiplanarunet_amd import _lib
    from multiplanarunet_amd.uncertainty import means_from_table
    r, truth = table_inputs(golden)
    K, n = 3, r["labels"].size
    nscratch = int(_lib.load().mpu_uncertainty_table_scratch_bytes(n, K))
    got = {}
    for fill in POISONS:
        A = guarded.arena(__name__, 11 * n + 8 * 12 * K + nscratch + 4096, 7, fill)
        bufs = [A.put(dev(a), name=k) for k, a in (("labels", r["labels"]), ("truth", truth), ("entropy", r["entropy"]),
                                                   ("mi", r["mi"]), ("agreement", r["agreement"]))]
        before = [t.clone() for t in bufs]
        table = A.carve((K, 3, 4), torch.float64, name="table")
        scratch = A.carve(nscratch, torch.uint8, name="scratch")
        tabs = []
        for _ in range(2):
            _lib.call("mpu_uncertainty_table", *[_lib.ptr(t) for t in bufs], n, K, _lib.ptr(table), _lib.ptr(scratch), _lib.stream_ptr())
            torch.cuda.synchronize()
            tabs.append(table.cpu().clone())
        assert not A.check(), (fill, A.check())
        assert all(torch.equal(x, y) for x, y in zip(bufs, before))
        assert same_bits(tabs[0], tabs[1])
        got[fill] = tabs[0]
    for fill in POISONS[1:]:
        assert same_bits(got[NAN], got[fill]), "the table depends on the poison (0xFF vs 0x%02X)" % fill
    check_table(means_from_table(got[ZERO].numpy(), K, True), UR.table(r["labels"], {k: r[k] for k in ("entropy", "mi", "agreement")}, K, truth))


def test_fused_call_guarded_buffers(golden):
    """probs, labels and the three maps of mpu_map_fuse_views_uncertainty in a guarded arena: no guard byte changes (5 x 7 x 70:
    brick tails on every axis)."""
    from multiplanarunet_amd.uncertainty import fuse_with_uncertainty
    vol, vps, W, b = synthetic((5, 7, 70), 5, 3, 12, spacing=(0.5, 0.5, 0.15))
    n = 5 * 7 * 70
    for method in METHODS:
        ref = fuse_with_uncertainty(vol, vps, W, b, method=method, want_probs=True)
        A = guarded.arena(__name__, n * (4 * 5 + 1) + 4096, 2, NAN)
        probs, labels = A.carve((5, 7, 70, 5), torch.float32, name="probs"), A.carve((5, 7, 70), torch.uint8, name="labels")
        got = fuse_with_uncertainty(vol, vps, W, b, method=method, want_probs=True, out_probs=probs, out_labels=labels)
        torch.cuda.synchronize()
        assert not A.check(), A.check()
        assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])


# ---- mp predict --uncertainty --------------------------------------------------------------------------------------------------------
NAMES = ["vol_%d" % (5000 + i) for i in range(3)]
SUFFIX = {"entropy": ("ENTROPY", np.float32), "mi": ("MI", np.float32), "agreement": ("AGREE", np.uint8)}


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """The 32^3 toy project, trained briefly, then predicted without the flag, with it (NIfTI and npz) and with the filter."""
    import toy_project
    from multiplanarunet_amd.cli import mp
    proj = tmp_path_factory.mktemp("unc_proj")
    toy_project.make_project(proj)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        mp.entry_func(["train", "--project_dir", str(proj), "--overwrite", "--epochs", "2", "--train_images_per_epoch", "16",
                       "--val_images_per_epoch", "8"])
        common = ["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion"]
        mp.entry_func(common + ["--out_dir", "pred_plain"])
        mp.entry_func(common + ["--out_dir", "pred_unc", "--uncertainty"])
        mp.entry_func(common + ["--out_dir", "pred_npz", "--uncertainty", "--out_format", "npz", "--uncertainty_maps", "mi,agreement"])
        mp.entry_func(common + ["--out_dir", "pred_cc", "--uncertainty", "--largest_component", "--cc_connectivity", "18"])
    return proj, log.getvalue()


def nii(proj, out_dir, name, suffix):
    from multiplanarunet_amd.nifti import read_nifti
    data, affine, _ = read_nifti(str(proj / out_dir / "nii_files" / ("%s_%s.nii.gz" % (name, suffix))), scaled=False)
    return np.ascontiguousarray(data), affine


def csv_rows(proj, out_dir):
    rows = (proj / out_dir / "csv" / "uncertainty_results.csv").read_text().strip().splitlines()
    head = rows[0].split(",")
    return head, [dict(zip(head, r.split(","))) for r in rows[1:]]


def test_mp_predict_uncertainty_files(project):
    proj, log = project
    for name in NAMES:
        pred, aff = nii(proj, "pred_unc", name, "PRED")
        for key, (suffix, dtype) in SUFFIX.items():
            data, a = nii(proj, "pred_unc", name, suffix)
            assert data.shape == (32, 32, 32) and data.dtype == dtype, (key, data.shape, data.dtype)
            np.testing.assert_array_equal(a, aff)
        ent, mi, agree = (nii(proj, "pred_unc", name, SUFFIX[k][0])[0] for k in ("entropy", "mi", "agreement"))
        assert 0.0 <= ent.min() and ent.max() <= 1.0 and 0.0 <= mi.min() and mi.max() <= 1.0 and agree.max() <= 3
        # the prediction itself: the same bytes with and without the flag
        plain = gzip.open(str(proj / "pred_plain" / "nii_files" / (name + "_PRED.nii.gz"))).read()
        assert plain == gzip.open(str(proj / "pred_unc" / "nii_files" / (name + "_PRED.nii.gz"))).read()
        assert ("%s: uncertainty per class: mean entropy" % name) in log
    assert not (proj / "pred_plain" / "csv" / "uncertainty_results.csv").exists()
    assert sorted(os.listdir(proj / "pred_plain" / "nii_files")) == sorted(n + "_PRED.nii.gz" for n in NAMES)
    assert sorted(os.listdir(proj / "pred_unc" / "nii_files")) == sorted("%s_%s.nii.gz" % (n, s) for n in NAMES
                                                                          for s in ("PRED", "ENTROPY", "MI", "AGREE"))
    head, rows = csv_rows(proj, "pred_unc")
    assert head[:6] == ["image", "class", "n", "mean_entropy", "mean_mi", "mean_agreement"] and "n_wrong" in head
    assert len(rows) == 3 * len(NAMES)
    for row in rows:                                                          # the table describes the saved files
        pred, ent = nii(proj, "pred_unc", row["image"], "PRED")[0], nii(proj, "pred_unc", row["image"], "ENTROPY")[0]
        sel = pred == int(row["class"])
        assert int(row["n"]) == int(sel.sum()) and int(row["n_correct"]) + int(row["n_wrong"]) == int(row["n"])
        if sel.any():
            assert abs(float(row["mean_entropy"]) - float(ent[sel].astype(np.float64).mean())) <= 1e-6      # (six decimals in the file)


def test_mp_predict_uncertainty_npz(project):
    proj, _ = project
    for name in NAMES:
        with np.load(str(proj / "pred_npz" / "nii_files" / (name + "_PRED.npz"))) as z:
            assert sorted(z.files) == ["affine", "agreement", "labels", "mi"]
            assert z["mi"].dtype == np.float32 and z["agreement"].dtype == np.uint8 and z["mi"].shape == z["labels"].shape == (32, 32, 32)
            np.testing.assert_array_equal(z["labels"], nii(proj, "pred_plain", name, "PRED")[0])
            np.testing.assert_array_equal(z["mi"], nii(proj, "pred_unc", name, "MI")[0])
            np.testing.assert_array_equal(z["agreement"], nii(proj, "pred_unc", name, "AGREE")[0])
    head, rows = csv_rows(proj, "pred_npz")
    assert len(rows) == 3 * len(NAMES) and all(r["mean_entropy"] == "nan" for r in rows)


def test_mp_predict_uncertainty_with_the_component_filter(project):
    """The maps are properties of the fusion: the filter leaves them alone; the table follows the map that is saved."""
    proj, _ = project
    changed = 0
    _, rows = csv_rows(proj, "pred_cc")
    for name in NAMES:
        for key, (suffix, _) in SUFFIX.items():
            np.testing.assert_array_equal(nii(proj, "pred_cc", name, suffix)[0], nii(proj, "pred_unc", name, suffix)[0])
        filtered, plain = nii(proj, "pred_cc", name, "PRED")[0], nii(proj, "pred_unc", name, "PRED")[0]
        changed += int((filtered != plain).sum())
        counts = [int(r["n"]) for r in rows if r["image"] == name]
        assert counts == np.bincount(filtered.ravel(), minlength=3).tolist()
    assert changed > 0                                                        # (the filter had something to do)


def test_continue_treats_the_maps_as_part_of_the_output(project):
    from multiplanarunet_amd.cli import mp
    proj, _ = project
    victim = proj / "pred_unc" / "nii_files" / (NAMES[1] + "_MI.nii.gz")
    keep = (proj / "pred_unc" / "nii_files" / (NAMES[0] + "_MI.nii.gz"))
    want, stamp = gzip.open(str(victim)).read(), os.stat(keep).st_mtime_ns
    os.remove(victim)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_unc", "--uncertainty", "--continue"])
    assert gzip.open(str(victim)).read() == want and os.stat(keep).st_mtime_ns == stamp       # only the incomplete volume was redone
    with pytest.raises(OSError, match="exists"):
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_unc", "--uncertainty"])
