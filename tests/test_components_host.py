"""Host side of the connected-component filter (csrc/components.hip, postprocess.py, `mp predict --largest_component`): the NumPy
restatement the GPU tests compare with is held to scipy.ndimage.label + bincount + argmax on the whole case list; the CLI flags and
their refusals; the library's argument checks (they precede any HIP call: no GPU is needed); the scratch size; the ABI version."""
import ctypes as C
import os

import numpy as np
import pytest

import components_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_route(labels, n_classes, connectivity):
    """(roots, filtered map, table) the way a user does it on the host today: ndimage.label per class, bincount, argmax."""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    roots = np.full(labels.shape, -1, np.int32)
    out = labels.copy()
    table = np.zeros((n_classes, 3), np.int64)
    flat_index = np.arange(labels.size).reshape(labels.shape)
    for c in range(1, n_classes):
        lab, k = ndimage.label(labels == c, structure=structure)
        if k == 0:
            continue
        first = ndimage.minimum(flat_index, lab, index=np.arange(1, k + 1)).astype(np.int64)       # first voxel of each component
        assert np.all(np.diff(first) > 0)                       # scipy numbers components in raster order of their first voxel
        roots[lab > 0] = first[lab[lab > 0] - 1]
        sizes = np.bincount(lab.ravel())[1:]
        win = int(np.argmax(sizes)) + 1
        out[(lab > 0) & (lab != win)] = 0
        table[c] = (k, sizes[win - 1], sizes.sum() - sizes[win - 1])
    return roots, out, table


@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
def test_restatement_equals_scipy(connectivity):
    for name, (labels, K) in CR.cases().items():
        roots, out, table = CR.reference(name, connectivity)
        s_roots, s_out, s_table = scipy_route(labels, K, connectivity)
        np.testing.assert_array_equal(roots, s_roots, err_msg=name)
        np.testing.assert_array_equal(out, s_out, err_msg=name)
        np.testing.assert_array_equal(table, s_table, err_msg=name)
        assert out.dtype == np.uint8 and roots.dtype == np.int32


def test_case_list_has_the_properties_the_cases_are_there_for():
    comps = lambda name, conn: CR.reference(name, conn)[2][:, 0].tolist()
    for conn in CR.CONNECTIVITIES:
        assert comps("serpentine", conn) == [0, 1] and comps("serpentine_dense", conn) == [0, 1]
        assert comps("all_background", conn) == [0, 0, 0, 0] and comps("solid_64", conn) == [0, 1]
        assert CR.reference("class_absent", conn)[2][2].tolist() == [0, 0, 0]
    assert int(CR.cases()["serpentine"][0].sum()) > 3500 and int(CR.cases()["serpentine_dense"][0].sum()) > 7000
    assert comps("serpentine_gap", 6) == [0, 2] and comps("serpentine_gap", 18) == [0, 1] and comps("serpentine_gap", 26) == [0, 1]
    assert comps("checkerboard", 6) == [0, 2048] and comps("checkerboard", 18) == [0, 1] and comps("checkerboard", 26) == [0, 1]
    assert comps("interleaved", 6) == [0, 960, 960]              # different classes never merge
    for name in ("tie", "tie_mirrored"):                         # equal sizes: the component with the smaller first index stays
        labels, K = CR.cases()[name]
        roots, out, table = CR.reference(name, 26)
        assert table[1].tolist() == [3, 27, 28] and table[2].tolist() == [2, 4, 4]
        for c in (1, 2):
            kept = np.unique(roots[out == c])
            assert len(kept) == 1 and kept[0] == roots[labels == c].min()
    labels, K = CR.cases()["foreign_label"]
    roots, out, _ = CR.reference("foreign_label", 26)
    assert np.all(roots[labels == 7] == -1) and np.all(out[labels == 7] == 7) and int((labels == 7).sum()) > 100
    assert CR.reference("blobs", 26)[2][1:, 0].min() >= 2 and CR.reference("blobs", 26)[2][1:, 2].min() > 0
    # a subset of classes: the others are untouched and report removed = 0
    labels, K = CR.cases()["blobs"]
    out, table = CR.keep_largest(labels, K, 18, classes=(2, 5))
    full = CR.reference("blobs", 18)
    for c in range(1, K):
        if c in (2, 5):
            assert np.array_equal(out == c, full[1] == c) and table[c].tolist() == full[2][c].tolist()
        else:
            assert np.array_equal(out == c, labels == c) and table[c].tolist() == [full[2][c, 0], int((labels == c).sum()), 0]


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_flags_parse():
    from multiplanarunet_amd.cli.predict import get_argparser, component_filter_plan
    p = get_argparser()
    a = p.parse_args([])
    assert a.largest_component is False and a.cc_connectivity is None and a.cc_classes is None
    assert component_filter_plan(a, 4) is None
    assert component_filter_plan(p.parse_args(["--largest_component"]), 4) == (26, None)
    a = p.parse_args(["--largest_component", "--cc_connectivity", "6", "--cc_classes", "3,1"])
    assert component_filter_plan(a, 4) == (6, [1, 3])
    with pytest.raises(SystemExit):
        p.parse_args(["--largest_component", "--cc_connectivity", "8"])


@pytest.mark.parametrize("flags, needle", [
    (["--largest_component", "--no_argmax"], "--no_argmax"),
    (["--cc_connectivity", "18"], "need --largest_component"),
    (["--cc_classes", "1"], "need --largest_component"),
    (["--largest_component", "--cc_classes", "1,3"], "1 .. n_classes - 1 = 2"),
    (["--largest_component", "--cc_classes", "0"], "1 .. n_classes - 1 = 2"),
])
def test_refusals_come_before_anything_is_created(tmp_path, flags, needle):
    """A project of three classes that has its hyperparameters and nothing else: each refusal is a ValueError raised before a
    folder is created (and before the missing views / model / device could be noticed)."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text("build:\n  n_classes: 3\n")
    with pytest.raises(ValueError, match=needle):
        mp.entry_func(["predict", "--project_dir", str(proj), "--out_dir", "pred_cc"] + flags)
    assert sorted(os.listdir(proj)) == ["train_hparams.yaml"]


# ---- the library's checks ------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -3
FAKE = C.c_void_p(1 << 20)          # an aligned non-NULL address: never dereferenced, the checks come before any HIP call


def _shape(*s):
    return (C.c_int64 * 3)(*s)


def _err(lib):
    return (lib.mpu_last_error() or b"").decode()


def test_library_refuses_bad_arguments_without_a_gpu():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    label = lambda shape, conn, K, roots=FAKE, scratch=FAKE: lib.mpu_label_components(FAKE, _shape(*shape), conn, K, roots, scratch, None)
    keep = lambda shape, conn, K, mask, out=C.c_void_p((1 << 20) + (1 << 30)), report=FAKE, scratch=FAKE: \
        lib.mpu_keep_largest_components(FAKE, _shape(*shape), conn, K, mask, out, report, scratch, None)
    for call in (lambda **k: label((8, 8, 8), k.get("conn", 26), k.get("K", 4)),
                 lambda **k: keep(k.get("shape", (8, 8, 8)), k.get("conn", 26), k.get("K", 4), k.get("mask", 0b1110))):
        for conn in (0, 4, 8, 27, -6):
            assert call(conn=conn) == EINVAL and "connectivity must be 6, 18 or 26" in _err(lib)
        for K in (0, 17, -1):
            assert call(K=K) == EUNSUPPORTED and "1 <= n_classes <= 16" in _err(lib)
    for mask in (0b0001, 0b1111, 0b10000, 0x80000000):             # bit 0, or a bit >= n_classes = 4
        assert keep((8, 8, 8), 26, 4, mask) == EINVAL and "class_mask" in _err(lib)
    for shape in ((2048, 2048, 512), (0, 8, 8), (8, -1, 8), (1 << 31, 1, 1), (1 << 40, 1 << 40, 1 << 40)):
        assert label(shape, 26, 4) == EUNSUPPORTED and _err(lib)
        assert keep(shape, 26, 4, 0b10) == EUNSUPPORTED and ("2^31 - 1" in _err(lib) or "dimension" in _err(lib))
        assert lib.mpu_components_scratch_bytes(_shape(*shape)) == -1 and _err(lib)
    assert "2^31 - 1" in _err(lib)
    # NULL / misaligned pointers, and an output that overlaps the input without being it
    assert label((8, 8, 8), 26, 4, roots=None) == EINVAL and "null" in _err(lib)
    assert label((8, 8, 8), 26, 4, roots=C.c_void_p((1 << 20) + 2)) == EINVAL and "aligned" in _err(lib)
    assert label((8, 8, 8), 26, 4, scratch=C.c_void_p((1 << 20) + 8)) == EINVAL and "aligned" in _err(lib)
    assert keep((8, 8, 8), 26, 4, 0b10, report=C.c_void_p((1 << 20) + 4)) == EINVAL and "aligned" in _err(lib)
    assert keep((8, 8, 8), 26, 4, 0b10, out=None) == EINVAL and "null" in _err(lib)
    assert keep((8, 8, 8), 26, 4, 0b10, out=C.c_void_p((1 << 20) + 511)) == EINVAL and "overlap" in _err(lib)
    assert keep((8, 8, 8), 26, 4, 0b10, out=C.c_void_p((1 << 20) - 1)) == EINVAL and "overlap" in _err(lib)
    # the largest volume the entries take: 2^31 - 1 voxels
    assert lib.mpu_components_scratch_bytes(_shape(2047, 1024, 1024)) > 8 * 2047 * 1024 * 1024


def test_scratch_bytes_positive_and_monotone():
    from multiplanarunet_amd import _lib, postprocess
    lib = _lib.load()
    shapes = [(1, 1, 1), (1, 1, 50), (37, 19, 23), (64, 64, 64), (96, 80, 72), (256, 256, 256), (512, 512, 512), (2047, 1024, 1024)]
    sizes = [lib.mpu_components_scratch_bytes(_shape(*s)) for s in shapes]
    assert all(b > 0 for b in sizes) and sizes == sorted(sizes) and len(set(sizes[1:])) == len(sizes) - 1
    assert all(b >= 8 * int(np.prod(s)) for b, s in zip(sizes, shapes))       # two i32 words per voxel and a header
    assert postprocess.scratch_bytes((64, 64, 64)) == sizes[3]
    with pytest.raises(NotImplementedError, match="2\\^31 - 1"):
        postprocess.scratch_bytes((2048, 2048, 512))


def test_abi_version_stays_2_and_the_entries_are_bound():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    assert lib.mpu_abi_version() == 2 and _lib.ABI_VERSION == 2
    hdr = open(os.path.join(ROOT, "include", "mpunet_hip.h")).read()
    for name in ("mpu_components_scratch_bytes", "mpu_label_components", "mpu_keep_largest_components"):
        assert name in _lib.declared_symbols() and hasattr(lib, name) and name + "(" in hdr


def test_python_layer_refuses_bad_labels_before_the_device():
    import torch
    from multiplanarunet_amd import postprocess
    with pytest.raises(ValueError, match="uint8"):
        postprocess.keep_largest_component(torch.zeros((4, 4, 4), dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="uint8"):
        postprocess.connected_components(torch.zeros((4, 4), dtype=torch.uint8), 3)
    assert postprocess.class_mask(4) == 0b1110 and postprocess.class_mask(4, (1, 3)) == 0b1010
    with pytest.raises(ValueError):
        postprocess.class_mask(4, (40,))
