"""Connected components and the largest-component filter on the device (csrc/components.hip through postprocess.py and the C
entries) against the NumPy restatement of tests/components_ref.py (itself held to scipy by tests/test_components_host.py): exact
equality on every voxel, every name, every count, for 6 / 18 / 26 connectivity on the whole case list; in place, class subsets,
the report; identical bytes run to run and on a side stream; guard bands and poisoned scratch around every caller-owned buffer;
and `mp predict --largest_component` end to end."""
import contextlib
import ctypes as C
import io
import re

import numpy as np
import pytest
import torch

import components_ref as CR
import guarded
from guarded import NAN, POISONS, ZERO, bits

pytestmark = pytest.mark.gpu

CASES = list(CR.cases())


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_case(name, connectivity, d_labels):
    """Both entries on a device copy of the case against the shared reference; the input is left as it was."""
    from multiplanarunet_amd import postprocess as PP
    labels, K = CR.cases()[name]
    roots_ref, out_ref, table_ref = CR.reference(name, connectivity)
    roots = PP.connected_components(d_labels, K, connectivity)
    assert roots.dtype == torch.int32 and roots.shape == d_labels.shape
    np.testing.assert_array_equal(roots.cpu().numpy(), roots_ref)
    out, table = PP.keep_largest_component(d_labels, K, connectivity, report=True)
    assert out.dtype == torch.uint8 and table.dtype == np.int64 and table.shape == (K, 3)
    np.testing.assert_array_equal(out.cpu().numpy(), out_ref)
    np.testing.assert_array_equal(table, table_ref)
    np.testing.assert_array_equal(d_labels.cpu().numpy(), labels)


@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
@pytest.mark.parametrize("name", CASES)
def test_case_equals_the_restatement(name, connectivity):
    check_case(name, connectivity, dev(CR.cases()[name][0]))


@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["random_0.35", "blobs", "line_1x1x50"])
@pytest.mark.parametrize("offset", [1, 4])
def test_labels_that_are_not_16_byte_aligned(name, connectivity, offset):
    """The label volume needs no alignment: at offset 1 every load is the byte path, at offset 4 the dword loads stay and the
    16-byte path of the last pass does not."""
    labels, _ = CR.cases()[name]
    buf = torch.zeros(labels.size + 64, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + labels.size].view(labels.shape)
    view.copy_(dev(labels))
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    check_case(name, connectivity, view)
    assert int(buf[:offset].sum()) == 0 and int(buf[offset + labels.size:].sum()) == 0


@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["random_0.6", "tie", "foreign_label", "blobs"])
def test_in_place_subsets_and_the_report(name, connectivity):
    from multiplanarunet_amd import postprocess as PP
    labels, K = CR.cases()[name]
    _, out_ref, table_ref = CR.reference(name, connectivity)
    d = dev(labels)
    inplace = d.clone()
    got, table = PP.keep_largest_component(inplace, K, connectivity, out=inplace, report=True)
    assert got is inplace
    np.testing.assert_array_equal(inplace.cpu().numpy(), out_ref)              # in place = out of place = the reference
    np.testing.assert_array_equal(table, table_ref)
    other = torch.full_like(d, 99)
    assert PP.keep_largest_component(d, K, connectivity, out=other) is other and torch.equal(other, inplace)
    for classes in ([1], [K - 1], list(range(2, K))):
        want, want_table = CR.keep_largest(labels, K, connectivity, classes=classes, roots=CR.reference(name, connectivity)[0])
        out, table = PP.keep_largest_component(d, K, connectivity, classes=classes, report=True)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        np.testing.assert_array_equal(table, want_table)
        for c in range(1, K):                                                 # the other classes: bit-identical, removed = 0
            if c not in classes:
                assert torch.equal(out == c, d == c) and table[c, 2] == 0
    with pytest.raises(ValueError, match="class_mask"):
        PP.keep_largest_component(d, K, connectivity, classes=[0])
    with pytest.raises(ValueError, match="class_mask"):
        PP.keep_largest_component(d, K, connectivity, classes=[K])
    with pytest.raises(ValueError, match="connectivity"):
        PP.keep_largest_component(d, K, 8)
    with pytest.raises(NotImplementedError, match="n_classes"):
        PP.connected_components(d, 17, connectivity)


@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
def test_two_runs_give_identical_bytes_also_on_a_side_stream(connectivity):
    from multiplanarunet_amd import postprocess as PP
    labels, K = CR.cases()["blobs"]
    roots_ref, out_ref, table_ref = CR.reference("blobs", connectivity)
    d = dev(labels)
    runs = [(PP.connected_components(d, K, connectivity), *PP.keep_largest_component(d, K, connectivity, report=True)) for _ in range(2)]
    side, busy = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):                                             # another stream is busy meanwhile
        for _ in range(24):
            a = torch.tanh(a @ a)
    with torch.cuda.stream(side):
        runs.append((PP.connected_components(d, K, connectivity), *PP.keep_largest_component(d, K, connectivity, report=True)))
    torch.cuda.synchronize()
    for roots, out, table in runs:
        assert torch.equal(bits(roots), bits(runs[0][0])) and torch.equal(bits(out), bits(runs[0][1]))
        np.testing.assert_array_equal(table, table_ref)
    np.testing.assert_array_equal(runs[-1][0].cpu().numpy(), roots_ref)
    np.testing.assert_array_equal(runs[-1][1].cpu().numpy(), out_ref)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["random_0.35", "blobs"])
def test_guarded_buffers_under_three_poisons(name, connectivity):
    """labels, roots, out, report and scratch carved from a guarded arena of 0xFF, 0x00 and 0x7B bytes: no guard byte changes, and
    the outputs are the same bits three times (scratch and outputs are never read before they are written) and the reference's."""
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    labels, K = CR.cases()[name]
    roots_ref, out_ref, table_ref = CR.reference(name, connectivity)
    shape3 = (C.c_int64 * 3)(*labels.shape)
    nscratch = int(lib.mpu_components_scratch_bytes(shape3))
    assert nscratch > 0
    d = dev(labels)
    got = {}
    for fill in POISONS:
        A = guarded.arena(__name__, 6 * labels.size + nscratch + 1024, 5, fill)
        lab = A.put(d, name="labels")
        roots = A.carve(labels.shape, torch.int32, name="roots")
        out = A.carve(labels.shape, torch.uint8, name="out")
        report = A.carve((K, 3), torch.int64, name="report")
        scratch = A.carve(nscratch, torch.uint8, name="scratch")
        st = _lib.stream_ptr()
        _lib.call("mpu_label_components", _lib.ptr(lab), shape3, connectivity, K, _lib.ptr(roots), _lib.ptr(scratch), st)
        _lib.call("mpu_keep_largest_components", _lib.ptr(lab), shape3, connectivity, K, (1 << K) - 2, _lib.ptr(out), _lib.ptr(report),
                  _lib.ptr(scratch), st)
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        assert torch.equal(lab, d)
        got[fill] = (roots.cpu(), out.cpu(), report.cpu())
    for fill in POISONS[1:]:
        for x, y in zip(got[NAN], got[fill]):
            assert torch.equal(bits(x), bits(y)), "an output depends on the poison (0xFF vs 0x%02X)" % fill
    np.testing.assert_array_equal(got[ZERO][0].numpy(), roots_ref)
    np.testing.assert_array_equal(got[ZERO][1].numpy(), out_ref)
    np.testing.assert_array_equal(got[ZERO][2].numpy(), table_ref)


# ---- mp predict --largest_component --------------------------------------------------------------------------------------------------
NAMES = ["vol_%d" % (5000 + i) for i in range(3)]


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """The 32^3 toy project, trained briefly, then predicted without and with the filter -> (folder, log of the filtered run)."""
    import toy_project
    from multiplanarunet_amd.cli import mp
    proj = tmp_path_factory.mktemp("cc_proj")
    toy_project.make_project(proj)
    with contextlib.redirect_stdout(io.StringIO()):
        mp.entry_func(["train", "--project_dir", str(proj), "--overwrite", "--epochs", "2", "--train_images_per_epoch", "16",
                       "--val_images_per_epoch", "8"])
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_plain"])
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_cc",
                       "--largest_component", "--cc_connectivity", "18"])
    return proj, log.getvalue()


def saved_map(proj, out_dir, name):
    from multiplanarunet_amd.nifti import read_nifti
    data, _, _ = read_nifti(str(proj / out_dir / "nii_files" / (name + "_PRED.nii.gz")), scaled=False)
    assert data.dtype == np.uint8 and data.shape == (32, 32, 32)
    return np.ascontiguousarray(data)


def test_mp_predict_largest_component(project):
    from multiplanarunet_amd import postprocess as PP
    from multiplanarunet_amd.interpolation import dice_all
    from multiplanarunet_amd.nifti import read_nifti
    proj, log = project
    rows = (proj / "pred_cc" / "csv" / "results.csv").read_text().strip().splitlines()
    assert rows[0] == "image,mean_dice,class_1,class_2" and len(rows) == 1 + len(NAMES)
    removed_total = 0
    for name in NAMES:
        plain, filtered = saved_map(proj, "pred_plain", name), saved_map(proj, "pred_cc", name)
        want, table = PP.keep_largest_component(dev(plain), 3, 18, report=True)
        np.testing.assert_array_equal(filtered, want.cpu().numpy())           # the saved file = the filter of the unfiltered file
        np.testing.assert_array_equal(filtered, CR.keep_largest(plain, 3, 18)[0])
        for c in (1, 2):                                                       # the log names what was removed
            line = "%s: class %d: %d components found, %d voxels removed" % (name, c, table[c, 0], table[c, 2])
            assert line in log, (line, log[-2000:])
            assert table[c, 2] == int((plain == c).sum()) - int((filtered == c).sum())
        removed_total += int(table[:, 2].sum())
        truth, _, _ = read_nifti(str(proj / "data" / "test" / "labels" / (name + ".nii.gz")), scaled=False)
        d = dice_all(np.asarray(truth).reshape(32, 32, 32), filtered, n_classes=3, ignore_zero=True)
        row = [r for r in rows[1:] if r.startswith(name + ",")][0]
        assert row == "%s,%.5f,%s" % (name, float(np.nanmean(d)), ",".join("%.5f" % x for x in d))    # results.csv describes the saved map
        assert re.search(r"%s: dices .* mean %.4f" % (name, float(np.nanmean(d))), log)
    assert removed_total > 0                                                   # (the filter had something to do)


def test_mp_predict_refuses_the_filter_on_probabilities(project):
    from multiplanarunet_amd.cli import mp
    proj, _ = project
    with pytest.raises(ValueError, match="--no_argmax"):
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_refused",
                       "--largest_component", "--no_argmax"])
    with pytest.raises(ValueError, match="n_classes - 1 = 2"):
        mp.entry_func(["predict", "--project_dir", str(proj), "--dataset", "test", "--sum_fusion", "--out_dir", "pred_refused",
                       "--largest_component", "--cc_classes", "3"])
    assert not (proj / "pred_refused").exists()
