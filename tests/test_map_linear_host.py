"""
Host side of the linear back-mapping (map_real_space_pred(method="linear")), no GPU: the stored outputs of the reference's
own function (tests/golden/map_linear_golden*.npz, made by tests/golden/make_map_linear_golden.py) against the oracle
composition the GPU tests use for the cases that are not stored; the refusals that stay; the command-line flags; the C ABI
declarations; the plane ranges and cell ownership of the sharded form.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_linear_cases as MC                                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mpu_map_view_linear", "mpu_map_fuse_views_linear", "mpu_map_accumulate_view_linear")


def test_the_golden_holds_the_eight_cases():
    assert sorted(MC.linear_golden()) == sorted("lin_map_%s_%d_%d" % c for c in MC.GOLDEN_CASES)
    for (an, v, K) in MC.GOLDEN_CASES:
        a = MC.linear_golden()["lin_map_%s_%d_%d" % (an, v, K)]
        assert a.dtype == np.float32 and a.shape == (32, 28, 24, K)


@pytest.mark.parametrize("an,v,K", MC.GOLDEN_CASES)
def test_oracle_composition_equals_the_reference_bit_for_bit(golden, an, v, K):
    """rgi_linear per class + fill vector + float32 cast IS the reference's map_real_space_pred(method='linear')."""
    ref = MC.linear_golden()["lin_map_%s_%d_%d" % (an, v, K)]
    got, oob = MC.oracle_case(golden, an, v, K)
    np.testing.assert_array_equal(got, ref)
    fill = np.zeros(K, np.float32)
    fill[0] = 1.0
    assert np.array_equal(ref[oob], np.broadcast_to(fill, ref[oob].shape))
    assert 0.0 <= oob.mean() <= 0.34


@pytest.mark.parametrize("method", ("kNN", "cubic"))
def test_other_methods_are_still_refused(method):
    import torch
    from multiplanarunet_amd.interpolation import map_real_space_pred, map_and_fuse, map_accumulate
    pred = torch.zeros((4, 4, 4, 2))
    grid = (np.linspace(-1, 1, 4),) * 3
    with pytest.raises(NotImplementedError):
        map_real_space_pred(pred, grid, np.eye(3), None, method=method)
    with pytest.raises(NotImplementedError):
        map_and_fuse(None, [(pred, grid, np.eye(3))], sum_fusion=True, method=method)
    with pytest.raises(NotImplementedError):
        map_accumulate(None, pred, grid, np.eye(3), np.ones(2), 0, 4, True, None, method=method)


@pytest.mark.parametrize("which", ("predict", "train_fusion"))
def test_cli_parsers_take_map_method(which, capsys):
    import importlib
    mod = importlib.import_module("multiplanarunet_amd.cli." + which)
    p = mod.get_argparser()
    assert p.parse_args([]).map_method == "nearest"
    assert p.parse_args(["--map_method", "linear"]).map_method == "linear"
    assert p.parse_args(["--map_method", "nearest"]).map_method == "nearest"
    for bad in ("kNN", "cubic", ""):
        with pytest.raises(SystemExit):
            p.parse_args(["--map_method", bad])
    capsys.readouterr()
    text = " ".join(p.format_help().split())
    assert "--map_method" in text and "trained with the method used at predict time" in text


def test_new_symbols_are_declared_in_the_header_and_the_binding():
    from multiplanarunet_amd import _lib
    with open(os.path.join(ROOT, "include", "mpunet_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.declared_symbols()
    # same argument lists as the nearest counterparts
    for lin, near in (("mpu_map_view_linear", "mpu_map_view_nearest"), ("mpu_map_fuse_views_linear", "mpu_map_fuse_views"),
                      ("mpu_map_accumulate_view_linear", "mpu_map_accumulate_view")):
        assert _lib._SIGS[lin] == _lib._SIGS[near]
    assert _lib.ABI_VERSION == 2


@pytest.mark.parametrize("cuts", ([0, 7, 20, 36], [0, 35, 36], [0, 36], [0, 1, 2, 36]))
def test_halo_planes_and_cell_ownership_cover_every_cell_once(cuts):
    """The kernel's rule: a chunk [lo, hi) owns the cells c in [lo, hi) that exist (c <= P - 2: cell c lies between the planes
    c and c + 1); the planes the host hands it must hold both planes of every cell it owns."""
    from multiplanarunet_amd.interpolation import linear_chunk_planes
    P = cuts[-1]
    owners = np.zeros(P - 1, int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        s_lo, s_hi = linear_chunk_planes(lo, hi, P)
        assert s_lo == lo and s_hi == min(hi + 1, P)
        cells = [c for c in range(P - 1) if lo <= c < hi]
        owners[cells] += 1
        assert all(s_lo <= c and c + 1 < s_hi for c in cells)
        if lo == P - 1:
            assert cells == []                             # a chunk of the last plane alone owns nothing
    assert np.array_equal(owners, np.ones(P - 1, int))     # every cell 0 .. P-2 exactly once
    assert linear_chunk_planes(0, 7, 36) == (0, 8) and linear_chunk_planes(20, 36, 36) == (20, 36)
