"""Host side of the surface-distance evaluation (csrc/surface.hip, surface.py, `mp predict --surface_metrics`): the two NumPy forms
of the squared distance transform agree bit for bit; its root stays within 4 ulp of scipy.ndimage.distance_transform_edt; borders
and metrics equal the medpy formulas written out with scipy; the percentile arithmetic of surface.py is NumPy's; the CLI flags
and their refusals; the library's argument checks (they precede any HIP call: no GPU is needed); the ABI version."""
import ctypes as C
import os

import numpy as np
import pytest

import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulps(a, b):
    """Largest distance in units in the last place between two arrays of non-negative doubles (inf must meet inf)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    assert a.shape == b.shape and np.array_equal(np.isinf(a), np.isinf(b)) and not np.isnan(a).any() and not np.isnan(b).any()
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max())


def test_three_pass_form_equals_the_all_pairs_form_bit_for_bit():
    assert len(SR.small_cases()) >= 25
    for name, (labels, K, spacing) in SR.small_cases().items():
        for pred in SR.PREDICATES:
            f = SR.feature_of(labels, pred, 1)
            a, b = SR.edt2_brute(f, spacing), SR.edt2_three_pass(f, spacing)
            assert a.dtype == np.float64 and a.tobytes() == b.tobytes(), (name, pred)
            assert b.tobytes() == SR.reference(name, pred).tobytes()
            if not f.any():
                assert np.all(np.isinf(a))


def test_case_list_has_what_the_cases_are_there_for():
    cases = SR.cases()
    shapes = {v[0].shape for v in cases.values()}
    assert {(1, 1, 1), (1, 1, 50), (50, 1, 1), (1, 50, 1), (7, 9, 11), (33, 20, 65), (2, 300, 3)} <= shapes
    for axis in range(3):                                          # one 4100-long line per axis, the other two dimensions 1 and 2
        assert any(s[axis] == 4100 and sorted(s)[:2] == [1, 2] for s in shapes)
    assert {v[2] for v in cases.values()} == set(SR.SPACINGS)
    kinds = {k.split("_")[0] for k in cases}
    assert kinds == {"rand01", "rand30", "corner", "tie", "none", "all", "foreign"}
    lab = cases["foreign_7x9x11_s2"][0]
    assert (lab >= 3).sum() > 100 and (lab == 1).sum() > 50
    # nearest in millimetres is not nearest in index under 0.1 : 1 : 10
    labels, _, spacing = cases["rand30_7x9x11_s2"]
    d = np.argwhere(labels != 1)[:, None, :] - np.argwhere(labels == 1)[None, :, :]
    assert (((d * np.array(spacing)) ** 2).sum(-1).argmin(1) != (d ** 2).sum(-1).argmin(1)).any()
    pairs = SR.pairs()
    assert {v[2] for v in pairs.values()} >= {2, 3, 16}
    t = SR.reference_table("missing_K16")
    assert t["n_pred_border"][3] == 0 and t["n_truth_border"][3] > 0                # missing in the prediction
    assert t["n_pred_border"][5] > 0 and t["n_truth_border"][5] == 0                # missing in the truth
    assert t["n_pred_border"][9] == 0 and t["n_truth_border"][9] == 0               # missing in both
    assert t["n_pred_border"][15] > 0 and t["n_truth_border"][15] > 0


def test_root_of_the_restatement_is_within_4_ulp_of_scipy():
    """Ours carries <= 2 ulp on d2 (fl(s^2), one product, two sums), scipy <= 2.5; halved by the root plus the roots' own
    roundings: <= 3.25 ulp, whichever voxels the two minima pick."""
    from scipy import ndimage
    worst = 0
    for name, (labels, K, spacing) in SR.cases().items():
        if labels.size > 50000:
            continue
        for pred in SR.PREDICATES:
            f = SR.feature_of(labels, pred, 1)
            if not f.any():
                continue                                            # (scipy has no convention for "no zero voxel")
            ours = np.sqrt(SR.reference(name, pred))
            theirs = ndimage.distance_transform_edt(~f, sampling=spacing)
            worst = max(worst, ulps(ours, theirs))
    print("worst distance to scipy: %d ulp" % worst)
    assert worst <= 4


def scipy_medpy(pred, truth, spacing):
    """medpy.metric.binary hd / hd95 / assd written out with scipy: surfaces by binary erosion, distances by the EDT of the other
    surface's complement."""
    from scipy import ndimage
    fp = ndimage.generate_binary_structure(3, 1)
    bp, bt = pred ^ ndimage.binary_erosion(pred, structure=fp, iterations=1), truth ^ ndimage.binary_erosion(truth, structure=fp, iterations=1)
    a = ndimage.distance_transform_edt(~bt, sampling=spacing)[bp]
    b = ndimage.distance_transform_edt(~bp, sampling=spacing)[bt]
    return bp, bt, max(a.max(), b.max()), np.percentile(np.hstack((a, b)), 95), np.mean((a.mean(), b.mean()))


def test_borders_and_metrics_equal_the_medpy_formulas():
    from scipy import ndimage
    fp = ndimage.generate_binary_structure(3, 1)
    for name, (labels, K, spacing) in SR.small_cases().items():
        m = labels == 1
        np.testing.assert_array_equal(SR.border(m), m & ~ndimage.binary_erosion(m, fp), err_msg=name)
    checked = 0
    for name, (pred, truth, K, spacing, tau) in SR.pairs().items():
        t = SR.reference_table(name)
        for c in range(1, K):
            p, r = pred == c, truth == c
            np.testing.assert_array_equal(SR.border(p), p & ~ndimage.binary_erosion(p, fp))
            if not p.any() and not r.any():
                assert all(np.isnan(t[k][c]) for k in ("hd", "hd95", "assd", "nsd")), (name, c)
            elif not p.any() or not r.any():
                assert all(np.isnan(t[k][c]) for k in ("hd", "hd95", "assd")) and t["nsd"][c] == 0.0, (name, c)
            else:
                bp, bt, hd, hd95, assd = scipy_medpy(p, r, spacing)
                assert t["n_pred_border"][c] == bp.sum() and t["n_truth_border"][c] == bt.sum()
                assert ulps(t["hd"][c], hd) <= 4 and ulps(t["hd95"][c], hd95) <= 4 and ulps(t["assd"][c], assd) <= 4, (name, c)
                assert 0.0 <= t["nsd"][c] <= 1.0
                checked += 1
    assert checked >= 12
    t = SR.reference_table("identical_K3")
    assert np.all(t["hd"][1:] == 0) and np.all(t["hd95"][1:] == 0) and np.all(t["assd"][1:] == 0) and np.all(t["nsd"][1:] == 1.0)
    assert np.isnan(t["hd"][0]) and np.isnan(t["nsd"][0])


def test_percentile_arithmetic_is_numpys():
    from multiplanarunet_amd.surface import percentile95_from_order_statistics, metrics_from_table
    rng = np.random.default_rng(5)
    for n in list(range(1, 64)) + [100, 101, 120, 121, 1000, 1001, 4097, 65537]:
        a = np.sort(np.sqrt(rng.random(n) * rng.choice([1e-3, 1.0, 1e6])))
        q = np.true_divide(95, 100)
        vi = (n - 1) * q
        lo = n - 1 if vi >= n - 1 else int(np.floor(vi))
        hi = min(lo + 1, n - 1)
        got = percentile95_from_order_statistics(a[lo], a[hi], n)
        assert got.tobytes() == np.float64(np.percentile(a, 95)).tobytes(), n
    # a raw table row through the conventions
    raw = np.zeros((3, 8))
    ints = raw.view(np.int64)
    ints[1, :3] = (0, 5, 0)
    ints[2, :3] = (4, 4, 6)
    raw[2, 3:] = (9.0, 4.0, 8.0, 4.0, 4.0)
    m = metrics_from_table(raw, 3)
    assert np.isnan(m["hd"][1]) and np.isnan(m["hd95"][1]) and np.isnan(m["assd"][1]) and m["nsd"][1] == 0.0
    assert m["hd"][2] == 3.0 and m["hd95"][2] == 2.0 and m["assd"][2] == 1.5 and m["nsd"][2] == 0.75
    assert all(np.isnan(m[k][0]) for k in m)
    m = metrics_from_table(raw, 3, classes=[2])
    assert all(np.isnan(m[k][1]) for k in m) and m["n_pred_border"][2] == 4


def test_voxel_sizes_of_a_rotated_anisotropic_affine():
    from multiplanarunet_amd.surface import voxel_sizes
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.7), -np.sin(0.7)], [0, np.sin(0.7), np.cos(0.7)]])
    A = np.eye(4)
    A[:3, :3] = R @ np.diag([0.78125, 0.9, 3.3])
    A[:3, 3] = (-90, 12, 7)
    np.testing.assert_allclose(voxel_sizes(A), [0.78125, 0.9, 3.3], rtol=1e-15)
    np.testing.assert_array_equal(voxel_sizes(np.diag([2.0, -3.0, 0.5, 1.0])), [2.0, 3.0, 0.5])
    with pytest.raises(ValueError):
        voxel_sizes(np.eye(2))


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_default_to_off():
    from multiplanarunet_amd.cli.predict import get_argparser, surface_metrics_plan
    p = get_argparser()
    a = p.parse_args([])
    assert a.surface_metrics is False and a.nsd_tolerance is None and surface_metrics_plan(a) is None
    assert surface_metrics_plan(p.parse_args(["--surface_metrics"])) == 1.0
    assert surface_metrics_plan(p.parse_args(["--surface_metrics", "--nsd_tolerance", "2.5"])) == 2.5
    assert surface_metrics_plan(p.parse_args(["--surface_metrics", "-f", "a.nii", "-l", "b.nii"])) == 1.0


@pytest.mark.parametrize("flags, needle", [
    (["--surface_metrics", "--no_eval"], "--no_eval"),
    (["--surface_metrics", "--no_argmax"], "--no_argmax"),
    (["--nsd_tolerance", "2"], "needs --surface_metrics"),
    (["--surface_metrics", "-f", "image.nii.gz"], "needs labels"),
    (["--surface_metrics", "--nsd_tolerance", "0"], "finite and > 0"),
    (["--surface_metrics", "--nsd_tolerance", "-1"], "finite and > 0"),
    (["--surface_metrics", "--nsd_tolerance", "inf"], "finite and > 0"),
    (["--surface_metrics", "--nsd_tolerance", "nan"], "finite and > 0"),
])
def test_refusals_come_before_any_path_is_touched(tmp_path, flags, needle):
    """The project folder does not even exist: each refusal is a ValueError raised before that could be noticed."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "no_such_project"
    with pytest.raises(ValueError, match=needle):
        mp.entry_func(["predict", "--project_dir", str(proj), "--out_dir", "pred_sm"] + flags)
    assert os.listdir(tmp_path) == []


def test_flag_off_path_does_not_import_the_module():
    src = open(os.path.join(ROOT, "multiplanarunet_amd", "cli", "predict.py")).read()
    head = src[:src.index("def run(")]
    assert "surface import" not in head and "import surface" not in head
    assert "if sm is not None:" in src and src.index("from ..surface import") > src.index("if sm is not None:")


# ---- the library ---------------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -3
FAKE = C.c_void_p(1 << 20)          # an aligned non-NULL address: never dereferenced, the checks come before any HIP call
NAMES = ("mpu_surface_scratch_bytes", "mpu_edt_squared", "mpu_surface_table")


def _shape(*s):
    return (C.c_int64 * 3)(*s)


def _sp(*s):
    return (C.c_double * 3)(*s)


def _err(lib):
    return (lib.mpu_last_error() or b"").decode()


def test_abi_version_stays_2_and_the_entries_are_exported_and_bound():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    assert lib.mpu_abi_version() == 2 and _lib.ABI_VERSION == 2
    hdr = open(os.path.join(ROOT, "include", "mpunet_hip.h")).read()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(lib, name) and name + "(" in hdr
    assert (_lib.MPU_EDT_EQUAL, _lib.MPU_EDT_NOT_EQUAL, _lib.MPU_EDT_BORDER) == (SR.EQUAL, SR.NOT_EQUAL, SR.BORDER)
    assert "MPU_EDT_EQUAL = 0, MPU_EDT_NOT_EQUAL = 1, MPU_EDT_BORDER = 2" in hdr


def test_library_refuses_bad_arguments_without_a_gpu():
    from multiplanarunet_amd import _lib, surface
    lib = _lib.load()

    def edt(shape=(8, 8, 8), sp=(1, 1, 1), pred=0, value=1, out=FAKE, scratch=FAKE):
        return lib.mpu_edt_squared(FAKE, _shape(*shape), _sp(*sp), pred, value, 0, out, scratch, None)

    def table(shape=(8, 8, 8), sp=(1, 1, 1), K=4, mask=0b1110, tol=1.0, tab=FAKE, scratch=FAKE):
        return lib.mpu_surface_table(FAKE, FAKE, _shape(*shape), _sp(*sp), K, mask, tol, tab, scratch, None)

    for bad in ((0.0, 1, 1), (1, -1.0, 1), (1, 1, float("inf")), (float("nan"), 1, 1)):
        assert edt(sp=bad) == EINVAL and "spacing must be finite and > 0" in _err(lib)
        assert table(sp=bad) == EINVAL and "spacing must be finite and > 0" in _err(lib)
    for shape in ((2048, 2048, 512), (0, 8, 8), (8, -1, 8), (1 << 31, 1, 1)):
        assert edt(shape=shape) == EUNSUPPORTED and table(shape=shape) == EUNSUPPORTED
        assert lib.mpu_surface_scratch_bytes(_shape(*shape)) == -1 and ("2^31 - 1" in _err(lib) or "dimension" in _err(lib))
    for K in (0, 17, -1):
        assert table(K=K, mask=0) == EUNSUPPORTED and "1 <= n_classes <= 16" in _err(lib)
    for mask in (0b0001, 0b1111, 0b10000, 0x80000000):
        assert table(mask=mask) == EINVAL and "class_mask" in _err(lib)
    for tol in (0.0, -1.0, float("inf"), float("nan")):
        assert table(tol=tol) == EINVAL and "tolerance" in _err(lib)
    assert edt(pred=3) == EINVAL and "predicate" in _err(lib)
    assert edt(value=256) == EINVAL and "value" in _err(lib)
    assert edt(out=None) == EINVAL and "null" in _err(lib)
    assert edt(out=C.c_void_p((1 << 20) + 4)) == EINVAL and "aligned" in _err(lib)
    assert table(tab=None) == EINVAL and "null" in _err(lib)
    assert table(scratch=C.c_void_p((1 << 20) + 8)) == EINVAL and "aligned" in _err(lib)
    # the scratch: a header, two f64 volumes and a key list of two entries per voxel
    shapes = [(1, 1, 1), (1, 1, 50), (33, 20, 65), (256, 256, 256), (512, 512, 512), (2047, 1024, 1024)]
    sizes = [lib.mpu_surface_scratch_bytes(_shape(*s)) for s in shapes]
    assert sizes == sorted(sizes) and all(b >= 32 * int(np.prod(s)) for b, s in zip(sizes, shapes))
    assert surface.scratch_bytes((33, 20, 65)) == sizes[2]
    with pytest.raises(NotImplementedError, match="2\\^31 - 1"):
        surface.scratch_bytes((2048, 2048, 512))


def test_python_layer_refuses_bad_tensors_before_the_device():
    import torch
    from multiplanarunet_amd import surface
    with pytest.raises(ValueError, match="uint8"):
        surface.edt_squared(torch.zeros((4, 4, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="uint8"):
        surface.surface_distances(torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.uint8), 3, (1, 1, 1))
