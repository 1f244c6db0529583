"""Host side of the label-map clean-up (csrc/components.hip, csrc/surface.hip, postprocess.py, the `mp predict` clean-up flags): the
NumPy restatement the GPU tests compare with (tests/cleanup_ref.py) is held to scipy (binary_fill_holes for the two consequences of the
fill rule, ndimage.label + bincount for the size threshold) and to thresholds of surface_ref.edt2_brute; closing is extensive and
opening anti-extensive on every case; the random cases exercise every path (asserted, so that none passes vacuously); the CLI flags
and their refusals; the library's argument checks (they precede any HIP call: no GPU is needed); the header and the binding."""
import ctypes as C
import os

import numpy as np
import pytest

import cleanup_ref as R
import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL = {6: 1, 18: 2, 26: 3}
BRUTE_MAX_VOXELS = 1500                 # the all-pairs transform is affordable below this (test_surface_host proves the two forms equal)


def _foreign(labels, K):
    return bool((labels >= K).any())


# ---- the restatement against scipy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_fill_holes_equals_scipy_binary_fill_holes(connectivity):
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, LEVEL[connectivity])
    for name, (labels, K) in R.cases().items():
        out, table = R.reference_fill(name, connectivity)
        assert out.dtype == np.uint8 and table.shape == (K, 2)
        if not _foreign(labels, K):                              # all classes asked: the foreground's holes are exactly scipy's
            np.testing.assert_array_equal(out != 0, ndimage.binary_fill_holes(labels != 0, st), err_msg=name)
            assert table[0].tolist() == [0, 0], name
        # as a two-class problem (class 1 against everything else as background): scipy itself
        two = (labels == 1).astype(np.uint8)
        got, t2 = R.fill_holes(two, 2, connectivity)
        np.testing.assert_array_equal(got, ndimage.binary_fill_holes(two, st).astype(np.uint8), err_msg=name)
        assert t2[1, 1] == int(got.sum()) - int(two.sum()) and t2[0].tolist() == [0, 0]
        # never rewrites a labelled voxel; the table counts what changed
        assert np.array_equal(out[labels != 0], labels[labels != 0])
        for c in range(1, K):
            assert table[c, 1] == int(((out == c) & (labels == 0)).sum())


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_remove_small_equals_scipy_label_and_bincount(connectivity):
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, LEVEL[connectivity])
    for name, (labels, K) in R.cases().items():
        for min_voxels in R.MIN_VOXELS:
            out, table = R.reference_small(name, connectivity, min_voxels)
            want, want_table = labels.copy(), np.zeros((K, 3), np.int64)
            for c in range(1, K):
                lab, k = ndimage.label(labels == c, structure=st)
                sizes = np.bincount(lab.ravel(), minlength=k + 1)
                small = np.flatnonzero(sizes < min_voxels)
                drop = np.isin(lab, small[small > 0])
                want[drop] = 0
                want_table[c] = (k, int((labels == c).sum()) - int(drop.sum()), int(drop.sum()))
            np.testing.assert_array_equal(out, want, err_msg="%s %d" % (name, min_voxels))
            np.testing.assert_array_equal(table, want_table, err_msg="%s %d" % (name, min_voxels))
            if min_voxels == 1:
                assert np.array_equal(out, labels)


def _ball_by_brute(labels, K, op, radius, spacing):
    return R.morph_ball(labels, K, op, radius, spacing, edt2=SR.edt2_brute)


@pytest.mark.parametrize("ball", range(len(R.BALLS)))
@pytest.mark.parametrize("op", [R.OPEN, R.CLOSE])
def test_morphology_is_two_thresholds_of_the_brute_force_transform(op, ball):
    spacing, radius = R.BALLS[ball]
    checked = 0
    for name, (labels, K) in R.cases().items():
        if labels.size > BRUTE_MAX_VOXELS:
            continue
        out, table = R.reference_ball(name, op, ball)
        want, want_table = _ball_by_brute(labels, K, op, radius, spacing)
        np.testing.assert_array_equal(out, want, err_msg=name)
        np.testing.assert_array_equal(table, want_table, err_msg=name)
        checked += 1
    assert checked >= 14                                         # (all but the 33 x 17 x 65 map, where all pairs take minutes)


def test_closing_is_extensive_and_opening_anti_extensive_on_every_case():
    for name, (labels, K) in R.cases().items():
        for ball in range(len(R.BALLS)):
            closed, tc = R.reference_ball(name, R.CLOSE, ball)
            opened, to = R.reference_ball(name, R.OPEN, ball)
            for c in range(1, K):
                assert not ((labels == c) & (closed != c)).any(), (name, ball, c)      # M inside close(M)
                assert not ((opened == c) & (labels != c)).any(), (name, ball, c)      # open(M) inside M
            assert np.array_equal(closed[labels != 0], labels[labels != 0])            # closing writes on background only
            assert np.array_equal(opened[opened != 0], labels[opened != 0])            # opening writes zeroes only
            assert np.array_equal(closed[labels >= K], labels[labels >= K]) and np.array_equal(opened[labels >= K], labels[labels >= K])
            assert tc[:, 1].sum() == 0 and to[:, 0].sum() == 0
            assert tc[:, 0].sum() == int((closed != labels).sum()) and to[:, 1].sum() == int((opened != labels).sum())


def test_designed_cases_have_the_properties_they_are_there_for():
    fill = lambda name, conn: R.reference_fill(name, conn)
    for conn in R.CONNECTIVITIES:
        out, t = fill("cavity_one_voxel", conn)
        assert t.tolist() == [[0, 0], [1, 1]] and out[3, 2, 1] == 1
        out, t = fill("cavity_multi", conn)
        assert t[1].tolist() == [1, 6 * 5 * 5] and t[2].tolist() == [0, 0]
        out, t = fill("nested_shells", conn)
        assert t[1, 0] == 1 and t[2].tolist() == [1, 3] and out[6, 5, 4] == 2 and out[2, 2, 2] == 1
        out, t = fill("vote_tie", conn)                            # 3 faces each: the smaller class
        assert t.tolist() == [[0, 0], [1, 1], [0, 0]] and out[3, 2, 1] == 1
        out, t = fill("foreign_bounds", conn)                      # partly foreign: filled by class 1; only foreign: stays
        assert t[1].tolist() == [1, 3 * 4 * 4] and t[0].tolist() == [1, 3 * 3 * 3] and t[2].tolist() == [0, 0]
        labels = R.cases()["foreign_bounds"][0]
        assert np.array_equal(out[labels >= 3], labels[labels >= 3]) and (out[8:11, 4:7, 3:6] == 0).all()
        out, t = fill("six_faces", conn)
        assert t.tolist() == [[0, 0], [1, 1]] and int((out == 0).sum()) == 6
        for name in ("empty_1x12x10", "all_one_12x1x10", "single_voxel", "line_1x1x50", "plane_1x12x10"):
            out, t = fill(name, conn)                              # a dimension of 1: no cavities at all
            assert t.sum() == 0 and np.array_equal(out, R.cases()[name][0])
    assert fill("edge_corner_contact", 6)[1][1].tolist() == [2, 2] and fill("edge_corner_contact", 6)[1][2].tolist() == [1, 1]
    assert fill("edge_corner_contact", 18)[1][1].tolist() == [1, 1] and fill("edge_corner_contact", 26)[1][1].tolist() == [0, 0]
    # a class subset: the cavity of a class that is not asked for is left, and reported in row 0
    labels, K = R.cases()["nested_shells"]
    out, t = R.fill_holes(labels, K, 6, classes=[2])
    assert t.tolist() == [[1, t[0, 1]], [0, 0], [1, 3]] and t[0, 1] > 100 and out[2, 2, 2] == 0 and out[6, 5, 4] == 2
    for conn in R.CONNECTIVITIES:                                  # sizes 4, 5, 6 around N = 5; two of 5 and a single voxel
        assert R.reference_small("sizes", conn, 5)[1].tolist() == [[0, 0, 0], [3, 11, 4], [3, 10, 1]]
        assert R.reference_small("sizes", conn, 6)[1].tolist() == [[0, 0, 0], [3, 6, 9], [3, 0, 11]]
    labels, K = R.cases()["touching_face"]                         # on the face x = 0: not shaved there, the spur goes, the slit closes
    opened, closed = R.reference_ball("touching_face", R.OPEN, 0)[0], R.reference_ball("touching_face", R.CLOSE, 0)[0]
    # (with scipy's border_value = 0 the plane x = 0 would keep its 3 x 3 centre only; here it keeps all but the rounded corners)
    assert (opened[0, 3, 3:6] == 1).all() and (opened[0, 4:7, 2] == 1).all() and (opened[0, 4:7, 3:6] == 1).all()
    assert (opened[4:8, 5, 4] == 0).all() and int((opened == 1).sum()) < int((labels == 1).sum())
    assert (closed[2, 4:7, 4] == 1).all() and (closed[0:4, 3:8, 2:7][labels[0:4, 3:8, 2:7] == 1] == 1).all()
    assert (closed[10, 1, 3:5] == 2).all()


def test_random_cases_exercise_every_path():
    for name in R.RANDOM_CASES:
        labels, K = R.cases()[name]
        assert set(np.unique(labels)) == set(range(K)), name
        for conn in (6, 26):
            roots, names = R.cavities(labels, conn)
            votes = R.cavity_votes(labels, K, roots, names)[:, 1:]
            top = votes.max(axis=1)
            assert len(names) >= 1 and (top > 0).any(), name                                         # a filled cavity
            assert ((votes == top[:, None]).sum(axis=1)[top > 0] >= 2).any(), (name, conn)         # a tie for the first place
            assert R.reference_fill(name, conn)[1][1:, 0].sum() >= 1
        assert R.reference_small(name, 26, 5)[1][:, 2].sum() >= 1                                    # a removed component
        assert R.reference_small(name, 26, 5)[1][:, 1].sum() >= 1                                    # ... and a kept one
        for ball in range(len(R.BALLS)):
            assert R.reference_ball(name, R.OPEN, ball)[1][:, 1].sum() >= 1, (name, ball)            # a voxel opened away
        assert any(R.reference_ball(name, R.CLOSE, ball)[1][:, 0].sum() >= 1 for ball in range(len(R.BALLS))), name
    assert R.reference_ball("blobs_K4", R.CLOSE, 0)[1][:, 0].sum() >= 1


def test_radii_on_and_between_attained_distances():
    """r2 of the ANISO balls: 2.25 and 6.25 are squared distances some voxel pair attains exactly, fl(1.2 * 1.2) is not."""
    attained = set()
    for dx in range(8):
        for dy in range(8):
            for dz in range(4):
                attained.add(float(np.float64(0.25) * dx * dx + (np.float64(1.0) * dy * dy + np.float64(6.25) * dz * dz)))
    r2 = [float(np.float64(r) * np.float64(r)) for sp, r in R.BALLS if sp == R.ANISO]
    assert r2[0] in attained and r2[1] in attained and r2[2] not in attained and 1.25 < r2[2] < 2.0


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_flags_parse():
    from multiplanarunet_amd.cli.predict import get_argparser, cleanup_plan, component_filter_plan
    p = get_argparser()
    a = p.parse_args([])
    assert a.open_mm is None and a.close_mm is None and a.fill_holes is False and a.min_component_voxels is None
    assert a.hole_connectivity is None and a.clean_connectivity is None and a.clean_classes is None
    assert cleanup_plan(a, 4) is None and component_filter_plan(a, 4) is None
    plan = cleanup_plan(p.parse_args(["--fill_holes"]), 4)
    assert plan == dict(open_mm=None, close_mm=None, hole_connectivity=6, min_voxels=None, clean_connectivity=26, classes=None)
    a = p.parse_args(["--open_mm", "1.5", "--close_mm", "2", "--fill_holes", "--hole_connectivity", "26", "--min_component_voxels", "10",
                      "--clean_connectivity", "6", "--clean_classes", "3,1"])
    assert cleanup_plan(a, 4) == dict(open_mm=1.5, close_mm=2.0, hole_connectivity=26, min_voxels=10, clean_connectivity=6, classes=[1, 3])
    assert component_filter_plan(a, 4) is None                     # --cc_* stay bound to --largest_component
    assert cleanup_plan(p.parse_args(["--min_component_voxels", "1"]))["min_voxels"] == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--fill_holes", "--hole_connectivity", "8"])


@pytest.mark.parametrize("flags, needle", [
    (["--fill_holes", "--no_argmax"], "--no_argmax"),
    (["--open_mm", "1", "--no_argmax"], "--no_argmax"),
    (["--hole_connectivity", "18"], "needs --fill_holes"),
    (["--hole_connectivity", "18", "--close_mm", "1"], "needs --fill_holes"),
    (["--clean_connectivity", "6"], "needs --min_component_voxels"),
    (["--clean_connectivity", "6", "--fill_holes"], "needs --min_component_voxels"),
    (["--clean_classes", "1"], "needs at least one of"),
    (["--clean_classes", "1", "--largest_component"], "needs at least one of"),
    (["--open_mm", "0"], "finite and > 0"),
    (["--close_mm", "-2"], "finite and > 0"),
    (["--close_mm", "inf"], "finite and > 0"),
    (["--open_mm", "nan"], "finite and > 0"),
    (["--min_component_voxels", "0"], ">= 1"),
    (["--fill_holes", "--clean_classes", "1,3"], "1 .. n_classes - 1 = 2"),
    (["--min_component_voxels", "4", "--clean_classes", "0"], "1 .. n_classes - 1 = 2"),
    (["--fill_holes", "--clean_classes", "a"], "comma-separated"),
])
def test_refusals_come_before_anything_is_created(tmp_path, flags, needle):
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "proj"
    proj.mkdir()
    (proj / "train_hparams.yaml").write_text("build:\n  n_classes: 3\n")
    with pytest.raises(ValueError, match=needle):
        mp.entry_func(["predict", "--project_dir", str(proj), "--out_dir", "pred_clean"] + flags)
    assert sorted(os.listdir(proj)) == ["train_hparams.yaml"]


# ---- the library's checks ------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -3
FAKE = C.c_void_p(1 << 20)              # an aligned non-NULL address: never dereferenced, the checks come before any HIP call
FAR = C.c_void_p((1 << 20) + (1 << 30))


def _shape(*s):
    return (C.c_int64 * 3)(*s)


def _err(lib):
    return (lib.mpu_last_error() or b"").decode()


def test_library_refuses_bad_arguments_without_a_gpu():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    sp = lambda *s: (C.c_double * 3)(*s)

    def small(shape=(8, 8, 8), conn=26, K=4, mask=0b1110, min_voxels=5, out=FAR, report=FAKE, scratch=FAKE):
        return lib.mpu_remove_small_components(FAKE, _shape(*shape), conn, K, mask, min_voxels, out, report, scratch, None)

    def fill(shape=(8, 8, 8), conn=6, K=4, mask=0b1110, out=FAR, report=FAKE, scratch=FAKE, **_):
        return lib.mpu_fill_holes(FAKE, _shape(*shape), conn, K, mask, out, report, scratch, None)

    def ball(shape=(8, 8, 8), K=4, mask=0b1110, out=FAR, report=FAKE, scratch=FAKE, spacing=(1.0, 1.0, 1.0), op=1, radius=1.0, **_):
        return lib.mpu_morph_ball(FAKE, _shape(*shape), sp(*spacing), K, mask, op, radius, out, report, scratch, None)

    for call in (small, fill, ball):
        for K in (0, 17, -1):
            assert call(K=K) == EUNSUPPORTED and "1 <= n_classes <= 16" in _err(lib)
        for mask in (0b0001, 0b1111, 0b10000, 0x80000000):
            assert call(mask=mask) == EINVAL and "class_mask" in _err(lib)
        for shape in ((2048, 2048, 512), (0, 8, 8), (8, -1, 8), (1 << 31, 1, 1), (1 << 40, 1 << 40, 1 << 40)):
            assert call(shape=shape) == EUNSUPPORTED and ("2^31 - 1" in _err(lib) or "dimension" in _err(lib))
        assert call(out=None) == EINVAL and "null" in _err(lib)
        assert call(report=None) == EINVAL and "null" in _err(lib)
        assert call(scratch=None) == EINVAL and "null" in _err(lib)
        assert call(report=C.c_void_p((1 << 20) + 4)) == EINVAL and "aligned" in _err(lib)
        assert call(scratch=C.c_void_p((1 << 20) + 8)) == EINVAL and "aligned" in _err(lib)
        assert call(out=C.c_void_p((1 << 20) + 511)) == EINVAL and "overlap" in _err(lib)
        assert call(out=C.c_void_p((1 << 20) - 1)) == EINVAL and "overlap" in _err(lib)
    for call in (small, fill):
        for conn in (0, 4, 8, 27, -6):
            assert call(conn=conn) == EINVAL and "connectivity must be 6, 18 or 26" in _err(lib)
    for bad in (0, -1, -(1 << 40)):
        assert small(min_voxels=bad) == EINVAL and "min_voxels" in _err(lib)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert ball(radius=bad) == EINVAL and "radius" in _err(lib)
        assert ball(spacing=(1.0, bad, 1.0)) == EINVAL and "spacing" in _err(lib)
    for op in (-1, 2):
        assert ball(op=op) == EINVAL and "op must be" in _err(lib)
    for shape in ((2048, 2048, 512), (0, 8, 8)):
        assert lib.mpu_fill_holes_scratch_bytes(_shape(*shape)) == -1 and _err(lib)


def test_scratch_bytes_stay_within_the_surface_scratch():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    shapes = [(1, 1, 1), (1, 1, 50), (7, 5, 3), (33, 17, 65), (256, 256, 256), (512, 512, 512), (2047, 1024, 1024)]
    sizes = [lib.mpu_fill_holes_scratch_bytes(_shape(*s)) for s in shapes]
    assert all(b > 0 for b in sizes) and sizes == sorted(sizes)
    for b, s in zip(sizes, shapes):
        n = int(np.prod(s))
        assert 25 * n <= b <= lib.mpu_surface_scratch_bytes(_shape(*s))       # at most the 32 bytes per voxel the surface entries ask for
        assert b <= 25 * n + 512 + 5 * 256


def test_abi_version_stays_2_and_the_entries_are_bound():
    from multiplanarunet_amd import _lib, postprocess
    lib = _lib.load()
    assert lib.mpu_abi_version() == 2 and _lib.ABI_VERSION == 2
    hdr = open(os.path.join(ROOT, "include", "mpunet_hip.h")).read()
    for name in ("mpu_remove_small_components", "mpu_fill_holes", "mpu_fill_holes_scratch_bytes", "mpu_morph_ball"):
        assert name in _lib.declared_symbols() and hasattr(lib, name) and name + "(" in hdr
    assert "MPU_MORPH_OPEN = 0, MPU_MORPH_CLOSE = 1" in hdr and (_lib.MPU_MORPH_OPEN, _lib.MPU_MORPH_CLOSE) == (0, 1)
    for name in ("remove_small_components", "fill_holes", "open_ball", "close_ball"):
        assert callable(getattr(postprocess, name))


def test_python_layer_refuses_bad_labels_before_the_device():
    import torch
    from multiplanarunet_amd import postprocess
    for call in (lambda t: postprocess.remove_small_components(t, 3, 5), lambda t: postprocess.fill_holes(t, 3),
                 lambda t: postprocess.open_ball(t, 3, 1.0), lambda t: postprocess.close_ball(t, 3, 1.0)):
        with pytest.raises(ValueError, match="uint8"):
            call(torch.zeros((4, 4, 4), dtype=torch.int32))
        with pytest.raises(ValueError, match="uint8"):
            call(torch.zeros((4, 4), dtype=torch.uint8))
