"""
Host side of the per-voxel uncertainty of the fusion (multiplanarunet_amd/uncertainty.py, mpu_map_fuse_views_uncertainty,
mpu_uncertainty_table, `mp predict --uncertainty`): known answers of the fp64 restatement tests/uncertainty_ref.py, the exported
symbols, the library's argument checks with fake pointers (they come before any HIP call) and the CLI's refusals. No GPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uncertainty_ref as UR                                                           # noqa: E402

EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # an aligned non-NULL address: never dereferenced, the checks come before any HIP call
NAMES = ("mpu_map_fuse_views_uncertainty", "mpu_uncertainty_table_scratch_bytes", "mpu_uncertainty_table")


# ---- the restatement: known answers --------------------------------------------------------------------------------------------
def test_all_views_the_same_one_hot():
    V, K = 5, 4
    x = np.zeros((V, 7, K), np.float32)
    x[..., 2] = 1.0
    W, b = np.full((V, K), 4.0), np.zeros(K)
    ent, mi, agree, lab = UR.uncertainty(x, W, b)
    assert np.all(lab == 2) and np.all(agree == V)
    np.testing.assert_array_equal(mi, 0.0)
    # softmax([0, 0, 20, 0]) is one-hot to 1e-8; the one-hot itself has entropy exactly 0
    assert np.all(ent < 1e-5) and np.all(UR.hn(x) == 0.0)
    ent, mi, agree, lab = UR.uncertainty(x, sum_fusion=True)
    np.testing.assert_array_equal(ent, 0.0)
    np.testing.assert_array_equal(mi, 0.0)
    assert np.all(agree == V)


def test_all_views_uniform():
    V, K = 3, 5
    x = np.full((V, 2, K), 1.0 / K, np.float32)
    ent, mi, agree, lab = UR.uncertainty(x, np.ones((V, K)), np.zeros(K))
    np.testing.assert_allclose(ent, 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(mi, 0.0, rtol=0, atol=1e-12)
    assert np.all(lab == 0) and np.all(agree == V)              # the first maximum


def test_two_opposite_one_hots():
    x = np.array([[[1.0, 0.0]], [[0.0, 1.0]]], np.float32)       # V = 2, one voxel, K = 2
    ent, mi, agree, lab = UR.uncertainty(x, np.ones((2, 2)), np.zeros(2))
    assert ent[0] == 1.0 and mi[0] == 1.0 and lab[0] == 0 and agree[0] == 1        # the first maximum wins: view 0 agrees


def test_one_class_is_all_zero():
    x = np.ones((4, 6, 1), np.float32)
    ent, mi, agree, lab = UR.uncertainty(x, np.ones((4, 1)), np.zeros(1))
    np.testing.assert_array_equal(ent, 0.0)
    np.testing.assert_array_equal(mi, 0.0)
    assert np.all(lab == 0) and np.all(agree == 4)              # (by its definition: every view votes the only class)


def test_all_zero_vector_gives_zero_not_nan():
    assert UR.hn(np.zeros((3, 4))).tolist() == [0.0, 0.0, 0.0]
    x = np.zeros((2, 3, 4), np.float32)
    ent, mi, agree, lab = UR.uncertainty(x, sum_fusion=True)
    assert np.all(ent == 0.0) and np.all(mi == 0.0) and np.all(agree == 2) and not np.isnan(ent).any()
    # negative entries contribute no term; a non-positive sum gives 0
    assert UR.hn(np.array([[-1.0, 0.5, 0.25]])).tolist() == [0.0]
    h = UR.hn(np.array([[-0.5, 1.0, 1.0]]))                       # s = 1.5: two terms (2/3) ln(2/3)
    np.testing.assert_allclose(h, -2 * (2 / 3) * np.log(2 / 3) / np.log(3), rtol=1e-15)


def test_table_restatement():
    lab = np.array([0, 0, 1, 1, 1, 3], np.uint8)
    truth = np.array([0, 1, 1, 1, 0, 3], np.uint8)
    maps = {"entropy": np.array([.1, .3, .5, .7, .9, 1.0], np.float32), "agreement": np.array([4, 2, 3, 3, 1, 4], np.uint8)}
    t = UR.table(lab, maps, 4, truth)
    assert t["n"].tolist() == [2, 3, 0, 1] and t["n_correct"].tolist() == [1, 2, 0, 1] and t["n_wrong"].tolist() == [1, 1, 0, 0]
    np.testing.assert_allclose(t["mean_entropy"][[0, 1, 3]], [np.mean(maps["entropy"][:2].astype(np.float64)), np.mean(maps["entropy"][2:5].astype(np.float64)), 1.0],
                               rtol=1e-15)
    assert np.isnan(t["mean_entropy"][2]) and np.isnan(t["mean_agreement_wrong"][3]) and "mean_mi" not in t
    assert t["mean_agreement_wrong"][:2].tolist() == [2.0, 1.0]


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def _err(lib):
    return (lib.mpu_last_error() or b"").decode()


def test_abi_version_stays_2_and_the_entries_are_exported_and_bound():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    assert lib.mpu_abi_version() == 2 and _lib.ABI_VERSION == 2
    hdr = open(os.path.join(ROOT, "include", "mpunet_hip.h")).read()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(lib, name) and name + "(" in hdr
    fuse = _lib._SIGS["mpu_map_fuse_views"][1]
    # mpu_map_fuse_views' arguments, `linear` after sum_fusion and the three maps before the stream
    assert _lib._SIGS["mpu_map_fuse_views_uncertainty"][1] == fuse[:7] + [_lib.i32] + fuse[7:9] + [_lib.c_p] * 3 + fuse[9:]


def test_library_refuses_bad_arguments_without_a_gpu():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    grid = _lib.VoxelGrid()
    grid.shape[:] = [8, 8, 8]
    views = (_lib.ViewPred * 16)()
    for v in views:
        v.d_pred = v.d_g = v.d_offsets = 1 << 20
        v.dim, v.n_planes = 4, 4

    def fuse(grid=C.byref(grid), views=views, V=3, K=3, W=FAKE, b=FAKE, sum_fusion=0, ent=FAKE, mi=FAKE, agree=FAKE):
        return lib.mpu_map_fuse_views_uncertainty(grid, views, V, K, W, b, sum_fusion, 0, FAKE, FAKE, ent, mi, agree, None)

    for K in (0, 17, -1):
        assert fuse(K=K) == EINVAL and "n_classes must be in 1..16" in _err(lib)
    for V in (0, 17, -2):
        assert fuse(V=V) == EINVAL and "n_views must be in 1..16" in _err(lib)
    assert fuse(ent=None, mi=None, agree=None) == EINVAL and "no map requested" in _err(lib)
    assert fuse(grid=None) == EINVAL and "null argument" in _err(lib)
    assert fuse(views=None) == EINVAL and "null argument" in _err(lib)
    assert fuse(W=None) == EINVAL and "W and b required" in _err(lib)
    assert _err(lib).startswith("mpu_map_fuse_views_uncertainty: ")
    views[2].d_pred = None
    assert fuse() == EINVAL and "null view field" in _err(lib)

    def table(labels=FAKE, n=100, K=3, tab=FAKE, scratch=FAKE):
        return lib.mpu_uncertainty_table(labels, None, FAKE, FAKE, FAKE, n, K, tab, scratch, None)

    for K in (0, 17, -1):
        assert table(K=K) == EINVAL and "n_classes must be in 1..16" in _err(lib)
        assert lib.mpu_uncertainty_table_scratch_bytes(100, K) == 0
    for n in (-1, 1 << 31):
        assert table(n=n) == EINVAL and "2^31 - 1" in _err(lib)
    assert table(labels=None) == EINVAL and "null" in _err(lib)
    assert table(tab=None) == EINVAL and "null" in _err(lib)
    assert table(scratch=None) == EINVAL and "null" in _err(lib)
    assert table(tab=C.c_void_p((1 << 20) + 4)) == EINVAL and "aligned" in _err(lib)
    # the scratch is one [K][2][4] table of 64-bit sums whatever n
    assert [lib.mpu_uncertainty_table_scratch_bytes(n, K) for n, K in ((0, 1), (1 << 27, 3), (5, 16))] == [64, 192, 1024]


def test_python_layer_refuses_bad_arguments_before_the_device():
    import torch
    from multiplanarunet_amd import uncertainty as U
    assert U.check_maps(("agreement", "entropy")) == ("entropy", "agreement") and U.check_maps("mi") == ("mi",)
    with pytest.raises(ValueError, match="unknown uncertainty map 'variance'"):
        U.check_maps(("entropy", "variance"))
    with pytest.raises(ValueError, match="no uncertainty map"):
        U.check_maps(())
    with pytest.raises(ValueError, match="uint8"):
        U.uncertainty_table(torch.zeros(4, dtype=torch.int32), {}, 3)
    with pytest.raises(ValueError, match=r"maps\['entropy'\]"):
        U.uncertainty_table(torch.zeros(4, dtype=torch.uint8), {"entropy": torch.zeros(5)}, 3)
    raw = np.zeros((2, 3, 4))
    raw[0, 0] = (4, 2.0, 1.0, 10)
    t = U.means_from_table(raw, 2, False)
    assert t["n"].tolist() == [4, 0] and t["mean_entropy"][0] == 0.5 and t["mean_agreement"][0] == 2.5 and np.isnan(t["mean_mi"][1])
    assert "n_correct" not in t and "n_wrong" in U.means_from_table(raw, 2, True)


# ---- `mp predict --uncertainty` ----------------------------------------------------------------------------------------------------
def _args(*flags):
    from multiplanarunet_amd.cli import predict as P
    return P.get_argparser().parse_args(list(flags))


def test_uncertainty_maps_flag_parses():
    from multiplanarunet_amd.cli import predict as P
    assert P.uncertainty_plan(_args()) is None
    assert P.uncertainty_plan(_args("--uncertainty")) == ("entropy", "mi", "agreement")
    assert P.uncertainty_plan(_args("--uncertainty", "--uncertainty_maps", "agreement, entropy")) == ("entropy", "agreement")
    assert P.uncertainty_plan(_args("--uncertainty", "--uncertainty_maps", "mi"), "softmax") == ("mi",)
    with pytest.raises(ValueError, match="unknown map 'variance'"):
        P.uncertainty_plan(_args("--uncertainty", "--uncertainty_maps", "entropy,variance"))
    with pytest.raises(ValueError, match="no map named"):
        P.uncertainty_plan(_args("--uncertainty", "--uncertainty_maps", ","))
    with pytest.raises(ValueError, match="needs --uncertainty"):
        P.uncertainty_plan(_args("--uncertainty_maps", "mi"))


def test_more_than_one_gpu_is_refused_before_anything_exists(tmp_path):
    """The project folder does not even exist: the refusal is a ValueError raised before that could be noticed (and before a
    process per GPU is started)."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path / "no_such_project"
    with pytest.raises(ValueError, match="--num_GPUs > 1"):
        mp.entry_func(["predict", "--project_dir", str(proj), "--uncertainty", "--num_GPUs", "2"])
    assert os.listdir(tmp_path) == []


def test_a_linear_output_model_is_refused_before_predictions_exists(tmp_path):
    from multiplanarunet_amd.cli import mp
    (tmp_path / "train_hparams.yaml").write_text(
        "build:\n  n_classes: 3\n  dim: 32\n  n_channels: 1\n  depth: 2\n  out_activation: linear\n  biased_output_layer: false\n\n"
        "fit:\n  batch_size: 2\n  real_space_span: 32.0\n")
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(ValueError, match="out_activation: linear"):
        mp.entry_func(["predict", "--project_dir", str(tmp_path), "--uncertainty", "--synthetic", "1"])
    assert not (tmp_path / "predictions").exists() and sorted(os.listdir(tmp_path)) == before


def test_extra_files_are_part_of_the_volumes_output(tmp_path):
    """plan_todo with several names per volume: done when all exist, a conflict when any exists."""
    from multiplanarunet_amd.cli.predict import plan_todo
    names = lambda i: [str(tmp_path / ("%s_PRED.nii.gz" % i)), str(tmp_path / ("%s_MI.nii.gz" % i))]
    for f in names("a") + names("b")[:1]:
        open(f, "w").close()
    assert plan_todo(["a", "b", "c"], names, True, False) == (["b", "c"], None)          # b lacks a map: predicted again
    assert plan_todo(["c", "b"], names, False, False) == (["c"], names("b")[0])
    assert plan_todo(["a", "b", "c"], names, False, True) == (["a", "b", "c"], None)
    assert plan_todo(["a", "b"], lambda i: names(i)[0], True, False) == ([], None)       # one name per volume: as ever


def test_flag_off_path_does_not_import_the_module():
    src = open(os.path.join(ROOT, "multiplanarunet_amd", "cli", "predict.py")).read()
    head = src[:src.index("def run(")]
    assert "uncertainty import" not in head and "import uncertainty" not in head
    assert src.index("from ..uncertainty import") > src.index("if unc is not None:")
    src = open(os.path.join(ROOT, "multiplanarunet_amd", "predict.py")).read()
    assert src.index("from .uncertainty import") > src.index("if uncertainty is not None:")
