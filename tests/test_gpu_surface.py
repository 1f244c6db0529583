"""The distance transform and the surface-distance table on the device (csrc/surface.hip through surface.py and the C entries)
against the NumPy restatement of tests/surface_ref.py (itself held to its all-pairs form and to scipy by
tests/test_surface_host.py): the squared transform bit for bit on every case and predicate; counts, nsd, hd and hd95 exactly and
assd within (n + 8) 2^-53 (one ulp per device root plus (n - 1) 2^-53 for any summation order of non-negative terms); unaligned
labels; class subsets; identical bytes run to run and on a side stream; guard bands and poisoned scratch around every caller-owned
buffer; and `mp predict --surface_metrics` end to end."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import guarded
import surface_ref as SR
from guarded import NAN, POISONS, ZERO, bits

pytestmark = pytest.mark.gpu

CASES = list(SR.cases())
PAIRS = list(SR.pairs())
EXACT = ("n_pred_border", "n_truth_border", "nsd", "hd", "hd95")


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = (np.array(t) if isinstance(t, np.ndarray) else t for t in (a, b))       # (the references are read-only arrays)
    return torch.equal(bits(a), bits(b))


def check_edt_case(name, d_labels):
    from multiplanarunet_amd import surface as S
    labels, K, spacing = SR.cases()[name]
    for pred in SR.PREDICATES:
        got = S.edt_squared(d_labels, spacing, pred, 1)
        assert got.dtype == torch.float64 and got.shape == d_labels.shape
        assert same_bits(got, SR.reference(name, pred)), (name, pred)
    np.testing.assert_array_equal(d_labels.cpu().numpy(), labels)                  # the input is left as it was


@pytest.mark.parametrize("name", CASES)
def test_squared_transform_equals_the_restatement_bit_for_bit(name):
    check_edt_case(name, dev(SR.cases()[name][0]))


@pytest.mark.parametrize("name", ["rand30_7x9x11_s2", "rand01_33x20x65_s2", "rand01_2x1x4100_s3"])
@pytest.mark.parametrize("offset", [1, 4])
def test_labels_that_are_not_16_byte_aligned(name, offset):
    labels = SR.cases()[name][0]
    buf = torch.zeros(labels.size + 64, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + labels.size].view(labels.shape)
    view.copy_(dev(labels))
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    check_edt_case(name, view)
    assert int(buf[:offset].sum()) == 0 and int(buf[offset + labels.size:].sum()) == 0


@pytest.mark.parametrize("name", ["rand30_7x9x11_s3", "rand01_33x20x65_s2", "tie_33x20x65_s0", "none_7x9x11_s0"])
def test_scipy_face_root_within_one_ulp(name):
    """distance_transform_edt: scipy's meaning (distance of non-zero voxels to the nearest zero voxel); the root is the device's."""
    from multiplanarunet_amd import surface as S
    labels, K, spacing = SR.cases()[name]
    mask = labels != 1                                                             # zero voxels = the case's features
    want2 = SR.reference(name, SR.EQUAL)
    for m in (dev(mask), dev(mask.astype(np.uint8) * 3)):                          # bool, and u8 with another non-zero value
        got2 = S.distance_transform_edt(m, sampling=spacing, squared=True)
        assert same_bits(got2, want2)
        got = S.distance_transform_edt(m, sampling=spacing).cpu().numpy()
        want = np.sqrt(want2)
        assert np.array_equal(np.isinf(got), np.isinf(want))
        fin = np.isfinite(want)
        assert np.abs(got[fin].view(np.int64) - want[fin].view(np.int64)).max(initial=0) <= 1
    assert S.distance_transform_edt(dev(mask), sampling=2.0, squared=True).shape == mask.shape


def check_table(got, want, K, classes=None):
    asked = range(1, K) if classes is None else classes
    for c in range(K):
        if c not in asked:
            assert all(np.isnan(got[k][c]) for k in got), c
            continue
        for k in EXACT:
            assert same_bits(np.float64(got[k][c]), np.float64(want[k][c])), (k, c, got[k][c], want[k][c])
        if np.isnan(want["assd"][c]):
            assert np.isnan(got["assd"][c])
        else:
            n = max(int(want["n_pred_border"][c]), int(want["n_truth_border"][c]))
            err = abs(got["assd"][c] - want["assd"][c])
            print("class %d assd %r restatement %r bound %r" % (c, got["assd"][c], want["assd"][c], (n + 8) * 2.0 ** -53 * want["assd"][c]))
            assert err <= (n + 8) * 2.0 ** -53 * want["assd"][c], (c, err)


@pytest.mark.parametrize("name", PAIRS)
def test_table_equals_the_restatement(name):
    from multiplanarunet_amd import surface as S
    pred, truth, K, spacing, tau = SR.pairs()[name]
    dp, dt = dev(pred), dev(truth)
    got = S.surface_distances(dp, dt, K, spacing, tolerance=tau)
    assert sorted(got) == sorted(S.KEYS) and all(v.shape == (K,) for v in got.values())
    check_table(got, SR.reference_table(name), K)
    np.testing.assert_array_equal(dp.cpu().numpy(), pred)
    np.testing.assert_array_equal(dt.cpu().numpy(), truth)


def test_class_subsets_and_refused_classes():
    from multiplanarunet_amd import surface as S
    pred, truth, K, spacing, tau = SR.pairs()["missing_K16"]
    dp, dt = dev(pred), dev(truth)
    want = SR.reference_table("missing_K16")
    for classes in ([1], [15], [2, 3, 5, 9]):
        check_table(S.surface_distances(dp, dt, K, spacing, tolerance=tau, classes=classes), want, K, classes)
    with pytest.raises(ValueError, match="class_mask"):
        S.surface_distances(dp, dt, K, spacing, classes=[0])
    with pytest.raises(ValueError, match="class_mask"):
        S.surface_distances(dp, dt, K, spacing, classes=[K])


def test_two_runs_give_identical_bytes_also_on_a_side_stream():
    from multiplanarunet_amd import surface as S
    pred, truth, K, spacing, tau = SR.pairs()["blobs_33x20x65_K4"]
    dp, dt = dev(pred), dev(truth)

    def run():
        t = S.surface_distances(dp, dt, K, spacing, tolerance=tau)
        return S.edt_squared(dp, spacing, SR.BORDER, 1), S.distance_transform_edt(dp, spacing), np.stack([t[k] for k in S.KEYS])

    runs = [run(), run()]
    side, busy = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):                                                 # another stream is busy meanwhile
        for _ in range(24):
            a = torch.tanh(a @ a)
    with torch.cuda.stream(side):
        runs.append(run())
    torch.cuda.synchronize()
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert same_bits(x, y)
    assert same_bits(runs[-1][0], SR.reference_border("blobs_33x20x65_K4"))


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs_33x20x65_K4", "line_2x1x4100_K3", "edge_K3"])
def test_guarded_buffers_under_three_poisons(name):
    """labels, output, table and scratch carved from a guarded arena of 0xFF, 0x00 and 0x7B bytes: no guard byte changes, and the
    outputs are the same bits three times (scratch and outputs are never read before they are written) and the restatement's."""
    from multiplanarunet_amd import _lib, surface as S
    lib = _lib.load()
    pred, truth, K, spacing, tau = SR.pairs()[name]
    shape3 = (C.c_int64 * 3)(*pred.shape)
    sp = (C.c_double * 3)(*spacing)
    nscratch = int(lib.mpu_surface_scratch_bytes(shape3))
    assert nscratch >= 32 * pred.size
    dp, dt = dev(pred), dev(truth)
    got = {}
    for fill in POISONS:
        A = guarded.arena(__name__, 2 * pred.size + 16 * pred.size + 64 * K + nscratch + 4096, 6, fill)
        lp, lt = A.put(dp, name="pred"), A.put(dt, name="truth")
        out = A.carve(pred.shape, torch.float64, name="out")
        root = A.carve(pred.shape, torch.float64, name="root")
        table = A.carve((K, S.TABLE_COLS), torch.float64, name="table")
        scratch = A.carve(nscratch, torch.uint8, name="scratch")
        st = _lib.stream_ptr()
        _lib.call("mpu_edt_squared", _lib.ptr(lp), shape3, sp, SR.BORDER, 1, 0, _lib.ptr(out), _lib.ptr(scratch), st)
        _lib.call("mpu_edt_squared", _lib.ptr(lt), shape3, sp, SR.NOT_EQUAL, 1, 1, _lib.ptr(root), _lib.ptr(scratch), st)
        _lib.call("mpu_surface_table", _lib.ptr(lp), _lib.ptr(lt), shape3, sp, K, (1 << K) - 2, float(tau), _lib.ptr(table),
                  _lib.ptr(scratch), st)
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        assert torch.equal(lp, dp) and torch.equal(lt, dt)
        got[fill] = (out.cpu(), root.cpu(), table.cpu())
    for fill in POISONS[1:]:
        for x, y in zip(got[NAN], got[fill]):
            assert same_bits(x, y), "an output depends on the poison (0xFF vs 0x%02X)" % fill
    assert same_bits(got[ZERO][0], SR.reference_border(name))
    check_table(S.metrics_from_table(got[ZERO][2].numpy(), K), SR.reference_table(name), K)


def test_bad_arguments_raise_with_the_librarys_message():
    from multiplanarunet_amd import surface as S
    d = dev(SR.cases()["rand30_7x9x11_s0"][0])
    for bad in ((0.0, 1, 1), (1, -2.0, 1), (1, 1, float("inf")), (float("nan"), 1, 1)):
        with pytest.raises(ValueError, match="spacing must be finite and > 0"):
            S.edt_squared(d, bad)
        with pytest.raises(ValueError, match="spacing must be finite and > 0"):
            S.surface_distances(d, d, 3, bad)
    with pytest.raises(ValueError, match="shapes differ"):
        S.surface_distances(d, dev(np.zeros((7, 9, 12), np.uint8)), 3, (1, 1, 1))
    with pytest.raises(ValueError, match="contiguous"):
        S.edt_squared(d.permute(2, 1, 0))
    with pytest.raises(ValueError, match="contiguous"):
        S.surface_distances(d, d.permute(2, 1, 0).contiguous().permute(2, 1, 0), 3, (1, 1, 1))
    with pytest.raises(NotImplementedError, match="n_classes"):
        S.surface_distances(d, d, 17, (1, 1, 1))
    with pytest.raises(ValueError, match="tolerance"):
        S.surface_distances(d, d, 3, (1, 1, 1), tolerance=0.0)
    with pytest.raises(ValueError, match="predicate"):
        S.edt_squared(d, (1, 1, 1), predicate=5)


# ---- mp predict --surface_metrics ----------------------------------------------------------------------------------------------------
NAMES = ["vol_%d" % (5000 + i) for i in range(3)]
HEADER = "image,class,hd,hd95,assd,nsd,n_pred_border,n_truth_border"


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """The 32^3 toy project, trained briefly, then predicted plainly, with the metrics, and with the filter and the metrics."""
    import toy_project
    from multiplanarunet_amd.cli import mp
    proj = tmp_path_factory.mktemp("sm_proj")
    toy_project.make_project(proj)
    log = io.StringIO()
    with contextlib.redirect_stdout(io.StringIO()):
        mp.entry_func(["train", "--project_dir", str(proj), "--overwrite", "--epochs", "2", "--train_images_per_epoch", "16",
                       "--val_images_per_epoch", "8"])
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_plain"])
    with contextlib.redirect_stdout(log):
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_sm",
                       "--surface_metrics", "--nsd_tolerance", "2"])
    with contextlib.redirect_stdout(io.StringIO()):
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_cc_sm",
                       "--largest_component", "--surface_metrics"])
    return proj, log.getvalue()


def saved_map(proj, out_dir, name):
    from multiplanarunet_amd.nifti import read_nifti
    data, affine, _ = read_nifti(str(proj / out_dir / "nii_files" / (name + "_PRED.nii.gz")), scaled=False)
    assert data.dtype == np.uint8 and data.shape == (32, 32, 32)
    return np.ascontiguousarray(data), affine


def check_csv(proj, out_dir, tolerance):
    from multiplanarunet_amd import surface as S
    from multiplanarunet_amd.nifti import read_nifti
    rows = (proj / out_dir / "csv" / "surface_results.csv").read_text().strip().splitlines()
    assert rows[0] == HEADER and len(rows) == 1 + 2 * len(NAMES)
    defined = 0
    for name in NAMES:
        pred, affine = saved_map(proj, out_dir, name)
        truth, _, _ = read_nifti(str(proj / "data" / "test" / "labels" / (name + ".nii.gz")), scaled=False)
        truth = np.ascontiguousarray(np.asarray(truth).reshape(32, 32, 32).astype(np.uint8))
        want = S.surface_distances(dev(pred), dev(truth), 3, S.voxel_sizes(affine), tolerance=tolerance)
        for c in (1, 2):
            row = [r for r in rows[1:] if r.startswith("%s,%d," % (name, c))]
            assert row == ["%s,%d,%.6f,%.6f,%.6f,%.6f,%d,%d" % (name, c, want["hd"][c], want["hd95"][c], want["assd"][c], want["nsd"][c],
                                                                  int(want["n_pred_border"][c]), int(want["n_truth_border"][c]))]
            f = row[0].split(",")
            for k, text in zip(("hd", "hd95", "assd", "nsd"), f[2:6]):             # parsed back at the precision written
                assert np.isnan(float(text)) if np.isnan(want[k][c]) else abs(float(text) - want[k][c]) <= 0.5e-6
            defined += not np.isnan(want["hd"][c])
    return defined


def test_mp_predict_surface_metrics(project):
    proj, log = project
    assert check_csv(proj, "pred_sm", 2.0) > 0
    for name in NAMES:
        assert "%s: surface distances (tolerance 2): hd95" % name in log
        a = (proj / "pred_plain" / "nii_files" / (name + "_PRED.nii.gz")).read_bytes()
        assert a == (proj / "pred_sm" / "nii_files" / (name + "_PRED.nii.gz")).read_bytes()
    assert (proj / "pred_plain" / "csv" / "results.csv").read_bytes() == (proj / "pred_sm" / "csv" / "results.csv").read_bytes()
    assert not (proj / "pred_plain" / "csv" / "surface_results.csv").exists()


def test_mp_predict_surface_metrics_describe_the_filtered_map(project):
    proj, _ = project
    check_csv(proj, "pred_cc_sm", 1.0)                                             # the saved (filtered) map against the labels
    assert any(not np.array_equal(saved_map(proj, "pred_plain", n)[0], saved_map(proj, "pred_cc_sm", n)[0]) for n in NAMES)


def test_mp_predict_refusals_leave_no_output_folder(project):
    from multiplanarunet_amd.cli import mp
    proj, _ = project
    for flags, needle in ((["--surface_metrics", "--no_eval"], "--no_eval"), (["--surface_metrics", "--no_argmax"], "--no_argmax"),
                          (["--nsd_tolerance", "2"], "needs --surface_metrics"), (["--surface_metrics", "--nsd_tolerance", "0"], "finite")):
        with pytest.raises(ValueError, match=needle):
            mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_refused"] + flags)
    assert not (proj / "pred_refused").exists()
