"""
The scalers on the GPU: csrc/volume_stats.hip (exact order statistics by radix select, fp64 moments), the device fits of
multiplanarunet_amd/scalers.py against NumPy / the sklearn golden, and apply_scaler of the sampling kernels (csrc/geometry.hip)
against Scaler.transform_host -- which tests/test_scalers_host.py pins on sklearn's own transforms.

Volumes (tests/scalers_data.py): v1 24x20x17x2 (odd extents: the vector loads' tails), v2 70x66x65x3 (~300 k voxels per
channel, three interleaved channels, many workgroups), v3 16^3 x 1 constant; normal values x 10^U(-3,3) mixed with a copy
quantised to 7 values, negatives, +-0.0, denormals; a variant with 1 % NaN; for the order statistics also +-inf at both ends
(sklearn refuses infinite input, so the fits and the golden use the finite volumes).

-0.0 and +0.0 are one value to the select (it returns +0.0) as they are to np.sort, whose order among them is arbitrary:
comparisons are np.array_equal / assert_array_equal, which take them as equal.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scalers_data as SD                                                             # noqa: E402
from multiplanarunet_amd import scalers as S                                          # noqa: E402
from multiplanarunet_amd.interpolation import Volume, ViewGeometry, sample_view       # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalers_golden.npz")
DEV = "cuda"


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_scaler(G, v, K):
    g = lambda a: G["%s/%s/%s" % (v, K, a)]
    if K == "MinMaxScaler":
        return S.Scaler(S.MUL_ADD, g("scale_"), g("min_"), name=K)
    if K == "StandardScaler":
        return S.Scaler(S.SUB_DIV, g("mean_"), g("scale_"), name=K)
    if K == "MaxAbsScaler":
        return S.Scaler(S.DIV, g("scale_"), name=K)
    if K == "RobustScaler":
        return S.Scaler(S.SUB_DIV, g("center_"), g("scale_"), name=K)
    return S.Scaler(S.QUANTILE, quantiles=g("quantiles_"), references=g("references_"), name=K)


def to_dev(a):
    return torch.as_tensor(a).to(DEV).contiguous()


# --------------------------------------------------------------------------- #
# 1. order statistics
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("v", ["v1", "v2", "v3"])
def test_order_stats_equal_sorted_values(v, with_nan):
    vol = SD.make_volume(v, with_inf=(v != "v3"), with_nan=with_nan and v != "v3")
    if v == "v3" and with_nan:
        vol = vol.copy()
        vol.reshape(-1)[::97] = np.nan
    dev = to_dev(vol)
    rs = np.random.RandomState(3)
    for c in range(vol.shape[-1]):
        col = vol[..., c].ravel()
        srt = np.sort(col[~np.isnan(col)])
        n = srt.size
        ranks = [0, 1, n // 100, n // 4, n // 2, n - 2, n - 1] + rs.randint(0, n, 16).tolist()
        got, n_nan = S.order_stats(dev, c, ranks)
        assert n_nan == int(np.isnan(col).sum())
        assert got.dtype == np.float32
        assert np.array_equal(got, srt[ranks]), (v, c)
        again, n_nan2 = S.order_stats(dev, c, ranks)
        assert got.tobytes() == again.tobytes() and n_nan2 == n_nan
        # a rank past the non-NaN values is answered with NaN, not with another element
        beyond, _ = S.order_stats(dev, c, [n - 1, n, col.size + 5, -1])
        assert beyond[0] == srt[-1] and np.isnan(beyond[1:]).all()


# --------------------------------------------------------------------------- #
# 2. device fit == host fit
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("v", list(SD.VOLUMES))
def test_device_fits_equal_host_fits(G, v):
    vol = SD.make_volume(v)
    dev = to_dev(vol)
    Cn = vol.shape[-1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bg_host = [float(np.percentile(vol[..., c], 1)) for c in range(Cn)]
        c_host, s_host = Volume.fit_robust_scaler(vol)
    bg_dev = S.bg_percentile_device(dev, 1)
    np.testing.assert_array_equal(np.array(bg_dev), np.array(bg_host))                # (NaN where the channel has a NaN)
    rob = S.fit_scaler("RobustScaler", dev)
    assert rob.kind == S.SUB_DIV
    np.testing.assert_array_equal(rob.p0, c_host)
    np.testing.assert_array_equal(rob.p1, s_host)
    bg2, rob2 = S.prepare_device(dev, 1, "RobustScaler")                              # both from one select per channel
    np.testing.assert_array_equal(np.array(bg2), np.array(bg_host))
    assert rob2.p0.tobytes() == rob.p0.tobytes() and rob2.p1.tobytes() == rob.p1.tobytes()

    mm = S.fit_scaler("MinMaxScaler", dev)
    for a in ("data_min_", "data_max_", "scale_", "min_"):
        assert mm.fitted[a].dtype == np.float32
        np.testing.assert_array_equal(mm.fitted[a], G["%s/MinMaxScaler/%s" % (v, a)])
    ma = S.fit_scaler("MaxAbsScaler", dev)
    for a in ("max_abs_", "scale_"):
        np.testing.assert_array_equal(ma.fitted[a], G["%s/MaxAbsScaler/%s" % (v, a)])

    # StandardScaler: an fp64 sum of n terms taken in any order is within n * 2^-53 * sum|terms| of the exact sum to first
    # order; the device's and sklearn's sums each carry that, hence 2 n u mean|x| for the mean (= sum / n) and, the terms of the
    # variance being (x - mean)^2, 2 n u mean((x - mean)^2) for the variance. (Not measured: the bounds of the summation.)
    st = S.fit_scaler("StandardScaler", dev)
    x = vol.reshape(-1, Cn).astype(np.float64)
    n = (~np.isnan(x)).sum(0)
    u = 2.0 ** -53
    g_mean, g_var = G[v + "/StandardScaler/mean_"], G[v + "/StandardScaler/var_"]
    err_mean = np.abs(st.fitted["mean_"] - g_mean)
    err_var = np.abs(st.fitted["var_"] - g_var)
    b_mean = 2 * n * u * np.nanmean(np.abs(x), axis=0)
    b_var = 2 * n * u * np.nanmean((x - g_mean) ** 2, axis=0)
    print("StandardScaler %s: |mean - golden| %s (bound %s), |var - golden| %s (bound %s)" % (v, err_mean, b_mean, err_var, b_var))
    assert np.all(err_mean <= b_mean)
    assert np.all(err_var <= b_var)
    np.testing.assert_array_equal(st.p1 == 1.0, G[v + "/StandardScaler/scale_"] == 1.0)     # the constant-feature mask
    np.testing.assert_allclose(st.p1, G[v + "/StandardScaler/scale_"], rtol=1e-12)
    st2 = S.fit_scaler("StandardScaler", dev)
    assert st2.p0.tobytes() == st.p0.tobytes() and st2.p1.tobytes() == st.p1.tobytes()
    assert st2.fitted["var_"].tobytes() == st.fitted["var_"].tobytes()
    m1, m2 = S.moments(dev), S.moments(dev)
    assert m1.tobytes() == m2.tobytes()
    np.testing.assert_array_equal(m1[:, 0], n)
    np.testing.assert_array_equal(m1[:, 1], np.nanmin(x, axis=0))
    np.testing.assert_array_equal(m1[:, 2], np.nanmax(x, axis=0))

    qt = S.fit_scaler("QuantileTransformer", dev)
    np.testing.assert_array_equal(qt.quantiles, G[v + "/QuantileTransformer/quantiles_"])
    np.testing.assert_array_equal(qt.references, G[v + "/QuantileTransformer/references_"])


# --------------------------------------------------------------------------- #
# 3. apply_scaler of the sampling kernels
# --------------------------------------------------------------------------- #
ROT = np.array([[0.8, -0.6, 0.0, 0.0], [0.6, 0.8, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])   # rot_mat is set
VIEW = (0.3, -0.5, 0.8)


@pytest.fixture(scope="module")
def sampled():
    """Unscaled planes, sampled once per (volume, dim): v1 / dim 32 and v2 / dim 32 run the generic kernel (two and three
    channels), v1 / dim 72 (92 planes, 477 k samples: above the straight-line kernel's threshold of 262 144) its fast path."""
    out = {}
    for v, dim, span in (("v1", 32, 30.0), ("v2", 32, 90.0), ("v1", 72, 30.0)):
        vol = SD.make_volume(v)
        lab = (np.random.RandomState(1).randint(0, 3, vol.shape[:3])).astype(np.uint8)
        raw = Volume(vol, lab, ROT, bg_value=[0.5] * vol.shape[-1], scaler=None, device=DEV)
        geom = ViewGeometry(VIEW, dim, span, "same+20")
        X, y = sample_view(raw, geom)
        torch.cuda.synchronize()
        out[(v, dim)] = (vol, lab, geom, X.cpu().numpy(), y.cpu().numpy())
    return out


@pytest.mark.parametrize("K", SD.SCALERS)
@pytest.mark.parametrize("case", [("v1", 32), ("v2", 32), ("v1", 72)])
def test_sample_view_applies_the_scaler_bit_for_bit(G, sampled, case, K):
    v, dim = case
    vol, lab, geom, X0, y0 = sampled[case]
    assert np.any(X0 == np.float32(0.5)) and np.any(X0 != np.float32(0.5))      # out-of-volume pixels occur, and others
    sc = golden_scaler(G, v, K)
    scaled = Volume(vol, lab, ROT, bg_value=[0.5] * vol.shape[-1], scaler=sc, device=DEV)
    X, y = sample_view(scaled, geom)
    np.testing.assert_array_equal(X.cpu().numpy(), sc.transform_host(X0))
    np.testing.assert_array_equal(y.cpu().numpy(), y0)


def _schedule_log(fn):
    import ctypes as C
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    lib.mpu_schedule_log_enable(1)
    try:
        out = fn()
        n = lib.mpu_schedule_log_read(None, 0)
        buf = C.create_string_buffer(int(n) + 1)
        lib.mpu_schedule_log_read(buf, n + 1)
    finally:
        lib.mpu_schedule_log_enable(0)
    return out, buf.value.decode().splitlines()


@pytest.fixture(scope="module")
def sampled_one_channel():
    """Channel 0 of v1 alone at dim 72 (92 planes, 477 k samples): the one-channel instantiations of the straight-line kernel,
    with and without labels -- the common `mp predict` shape."""
    vol = np.ascontiguousarray(SD.make_volume("v1")[..., :1])
    lab = (np.random.RandomState(1).randint(0, 3, vol.shape[:3])).astype(np.uint8)
    geom = ViewGeometry(VIEW, 72, 30.0, "same+20")
    X0, y0 = sample_view(Volume(vol, lab, ROT, bg_value=[0.5], scaler=None, device=DEV), geom)
    return vol, lab, geom, X0.cpu().numpy(), y0.cpu().numpy()


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("K", SD.SCALERS)
def test_fast_path_one_channel_applies_the_scaler_bit_for_bit(G, sampled_one_channel, K, with_labels):
    vol, lab, geom, X0, y0 = sampled_one_channel
    full = golden_scaler(G, "v1", K)
    cut = lambda a: None if a is None else a[:1]
    sc = S.Scaler(full.kind, cut(full.p0), cut(full.p1), cut(full.quantiles), full.references, name=K)
    V = Volume(vol, lab if with_labels else None, ROT, bg_value=[0.5], scaler=sc, device=DEV)
    (X, y), log = _schedule_log(lambda: sample_view(V, geom))
    assert any("sample fast" in l and "C=1 labels=%d" % int(with_labels) in l for l in log), log
    np.testing.assert_array_equal(X.cpu().numpy(), sc.transform_host(X0))
    if with_labels:
        np.testing.assert_array_equal(y.cpu().numpy(), y0)


def test_two_channel_case_at_dim_72_takes_the_fast_path(G, sampled):
    vol, lab, geom = sampled[("v1", 72)][:3]
    V = Volume(vol, lab, ROT, bg_value=[0.5, 0.5], scaler=golden_scaler(G, "v1", "QuantileTransformer"), device=DEV)
    _, log = _schedule_log(lambda: sample_view(V, geom))
    assert any("sample fast" in l and "C=2 labels=1" in l for l in log), log
    _, log = _schedule_log(lambda: sample_view(V, sampled[("v1", 32)][2]))
    assert any("sample generic" in l for l in log), log


def test_quantile_tables_beyond_the_lds_budget_are_refused_at_preparation():
    """(C + 1) * n_quantiles * 8 bytes must fit the 64 KiB the sampling kernels stage: 8 channels x 1000 quantiles do not, and
    the error comes when the scaler is made, not at the first sample_view."""
    refs = np.linspace(0, 1, 1000)
    S.Scaler(S.QUANTILE, quantiles=np.tile(refs, (7, 1)), references=refs)
    with pytest.raises(NotImplementedError):
        S.Scaler(S.QUANTILE, quantiles=np.tile(refs, (8, 1)), references=refs)


@pytest.mark.parametrize("K", SD.SCALERS)
def test_special_values_through_a_crafted_volume(G, K):
    """The golden plane batch's special values (exact hits on the first, the last and inner quantile knots, values beyond both
    ends, +-0.0, denormals, one NaN) reach apply_scaler unchanged: a volume of two equal z-slices = plane 3 of the batch,
    voxel size 2, cut along z on a grid that coincides with the voxel centres (span 62: axis -31 .. 31 step 2)."""
    planes = G["v1/planes"]
    q = G["v1/QuantileTransformer/quantiles_"]
    plane = planes[3].copy()                                                     # [32, 32, 2], holds the NaN
    for c in range(2):                                                           # (the shuffle left this plane without the end knots)
        plane[0:2, 0:2, c] = np.float32(q[c, 0])
        plane[4:6, 4:6, c] = np.float32(q[c, -1])
        assert np.float64(plane[0, 0, c]) == q[c, 0] and np.float64(plane[4, 4, c]) == q[c, -1]
    vol = np.stack([plane, plane], axis=2)                                       # [32, 32, 2, C]
    aff = np.diag([2.0, 2.0, 2.0, 1.0])
    geom = ViewGeometry((0.0, 0.0, 1.0), 32, 62.0, "same+20")
    raw = Volume(vol, None, aff, bg_value=[0.5, 0.5], scaler=None, device=DEV)
    X0 = sample_view(raw, geom)[0].cpu().numpy()
    inside = np.abs(geom.offsets) <= 1.0
    assert inside.sum() >= 1
    for c in range(2):
        got = X0[inside][..., c]
        assert np.any(got == q[c, 0]) and np.any(got == q[c, -1]) and np.any(got == q[c, 500])      # knot hits survive sampling
        assert np.any(got > q[c, -1]) and np.any(got < q[c, 0]) and np.isnan(X0[inside][..., 0]).any()
    sc = golden_scaler(G, "v1", K)
    X = sample_view(Volume(vol, None, aff, bg_value=[0.5, 0.5], scaler=sc, device=DEV), geom)[0].cpu().numpy()
    want = sc.transform_host(X0)
    np.testing.assert_array_equal(X, want)
    assert np.array_equal(np.signbit(X), np.signbit(want))


@pytest.mark.parametrize("K", SD.SCALERS)
def test_train_sampler_applies_the_scaler_bit_for_bit(G, sampled, K):
    """The one-plane path (mpu_sample_plane_stats_sc). max_tries=1 accepts every first candidate, so the sampler over the
    scaled volume and the one over the unscaled volume draw the same planes."""
    from multiplanarunet_amd.data import TrainSampler, random_views
    vol, lab = sampled[("v1", 32)][:2]
    sc = golden_scaler(G, "v1", K)
    views = random_views(3, seed=2)
    batches = []
    for s in (None, sc):
        V = Volume(vol, lab, ROT, bg_value=[0.5, 0.5], scaler=s, device=DEV)
        smp = TrainSampler([V], views, 32, 30.0, 6, 3, seed=4, max_tries=1)
        x, y, w = smp()
        batches.append((x.cpu().numpy(), y.cpu().numpy()))
    np.testing.assert_array_equal(batches[1][0], sc.transform_host(batches[0][0]))
    np.testing.assert_array_equal(batches[1][1], batches[0][1])


# --------------------------------------------------------------------------- #
# 4. as_volume: device preparation == host preparation
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("which", ["toy64", "v1", "v1n"])
def test_as_volume_device_equals_host(which):
    from multiplanarunet_amd.data import as_volume, make_toy_volume
    if which == "toy64":
        img, lab, aff = make_toy_volume(64, 0)
    else:
        img, lab, aff = SD.make_volume(which), None, ROT
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = as_volume(img, lab, aff, "1pct", "RobustScaler", DEV, "x", fit_on="host")
        dflt = as_volume(img, lab, aff, "1pct", "RobustScaler", DEV, "x")                  # default: fit_on="device"
        c, s = Volume.fit_robust_scaler(img)
        bg = [float(np.percentile(img[..., k], 1)) for k in range(img.shape[-1])]
    np.testing.assert_array_equal(np.array(host.bg_value), np.array(bg))                   # the numbers of the code before
    np.testing.assert_array_equal(np.array(dflt.bg_value), np.array(bg))
    for vol in (host, dflt):
        cc, ss = vol.scaler
        np.testing.assert_array_equal(cc, c)
        np.testing.assert_array_equal(ss, s)
    geom = ViewGeometry(VIEW, 32, 40.0, "same+20")
    old = Volume(img, lab, aff, bg_value=bg, scaler=(c, s), device=DEV)                    # the (center, scale) form
    Xo = sample_view(old, geom)[0].cpu().numpy()
    np.testing.assert_array_equal(sample_view(host, geom)[0].cpu().numpy(), Xo)
    np.testing.assert_array_equal(sample_view(dflt, geom)[0].cpu().numpy(), Xo)


# --------------------------------------------------------------------------- #
# 5. the data path by name
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("K", SD.SCALERS)
def test_load_dataset_trains_with_every_scaler(K):
    from multiplanarunet_amd.cli.common import load_dataset
    from multiplanarunet_amd.data import TrainSampler, random_views
    hp = {"fit": {"bg_value": "1pct", "scaler": K}}
    vols = load_dataset({}, ".", hp, DEV, synthetic=1, seed=0)
    assert len(vols) == 1 and vols[0]._scaler.name == K
    smp = TrainSampler(vols, random_views(3, seed=1), 32, 60.0, 4, 3, seed=0)
    x, y, w = smp()
    assert x.shape == (4, 32, 32, 1) and bool(torch.isfinite(x).all())
    assert float(x.std()) > 0


def test_load_dataset_refuses_other_scalers():
    from multiplanarunet_amd.cli.common import load_dataset
    with pytest.raises(NotImplementedError) as e:
        load_dataset({}, ".", {"fit": {"bg_value": "1pct", "scaler": "PowerTransformer"}}, DEV, synthetic=1, seed=0)
    for name in SD.SCALERS:
        assert name in str(e.value)
