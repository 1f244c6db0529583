"""
Host side of the scalers (multiplanarunet_amd/scalers.py), no GPU: the restatement of np.percentile's linear rule from two
order statistics, `Scaler.transform_host` against what scikit-learn 1.7.2 produced (tests/golden/scalers_golden.npz, made by
tests/golden/make_scalers_golden.py) and, where sklearn is installed, against a live sklearn; the host fits against the golden
attributes.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scalers_data as SD                                                             # noqa: E402
from multiplanarunet_amd import scalers as S                                          # noqa: E402
from multiplanarunet_amd.interpolation import Volume                                  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalers_golden.npz")
KIND = {"MinMaxScaler": S.MUL_ADD, "StandardScaler": S.SUB_DIV, "MaxAbsScaler": S.DIV, "RobustScaler": S.SUB_DIV,
        "QuantileTransformer": S.QUANTILE}


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_scaler(G, v, K):
    g = lambda a: G["%s/%s/%s" % (v, K, a)]
    if K == "MinMaxScaler":
        return S.Scaler(S.MUL_ADD, g("scale_"), g("min_"))
    if K == "StandardScaler":
        return S.Scaler(S.SUB_DIV, g("mean_"), g("scale_"))
    if K == "MaxAbsScaler":
        return S.Scaler(S.DIV, g("scale_"))
    if K == "RobustScaler":
        return S.Scaler(S.SUB_DIV, g("center_"), g("scale_"))
    return S.Scaler(S.QUANTILE, quantiles=g("quantiles_"), references=g("references_"))


def bits_equal(a, b):
    """Same dtype, shape and bits -- except that a zero may carry either sign: which of the equal values -0.0 and +0.0 lands on
    a rank is an accident of NumPy's partition, and the device select folds -0.0 onto +0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    zero = (a == 0) & (b == 0)
    return np.where(zero, 0, a).tobytes() == np.where(zero, 0, b).tobytes()


# n = 2 .. 3e6. At n = 229_402 and n = 2_999_002 with q = 99 the f32 virtual index (n - 1) * f32(0.99) floors to another rank
# than the f64 one (found by scanning n; asserted below); n = 101 / 201 / 401 put integer virtual indexes (gamma 0) in the set.
PCT_N = (2, 3, 7, 100, 101, 201, 401, 1000, 65537, 229_402, 2_999_002, 3_000_000)
PCT_Q = (1, 25, 37.5, 50, 75, 99)


@pytest.fixture(scope="module")
def pct_arrays():
    rs = np.random.RandomState(5)
    out = {}
    for n in PCT_N:
        a = SD.raw_values(rs, n)
        out[n] = (a, np.sort(a))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_percentile_from_order_stats_is_numpy_bit_for_bit(pct_arrays, dtype):
    differs = 0
    for n in PCT_N:
        a, srt = pct_arrays[n]
        a, srt = a.astype(dtype), srt.astype(dtype)
        for q in PCT_Q:
            lo_i, hi_i, _ = S.percentile_ranks(n, q, dtype)
            got = S.percentile_from_order_stats(srt[lo_i], srt[hi_i], n, q, dtype)
            want = np.percentile(a, q)
            assert bits_equal(got, want), (n, q, got, want)
            assert bits_equal(got, np.nanpercentile(a, q)), (n, q)
            if dtype == np.float32:
                differs += (lo_i, hi_i) != S.percentile_ranks(n, q, np.float64)[:2]
    if dtype == np.float32:
        assert differs > 0          # the set holds an n at which the f32 virtual index picks another rank than the f64 one


def test_percentile_with_nans_counts_only_the_rest(pct_arrays):
    a = pct_arrays[1000][0].copy()
    a[::7] = np.nan
    srt = np.sort(a[~np.isnan(a)])
    n = srt.size
    for dtype in (np.float32, np.float64):
        for q in PCT_Q:
            lo_i, hi_i, _ = S.percentile_ranks(n, q, dtype)
            got = S.percentile_from_order_stats(srt.astype(dtype)[lo_i], srt.astype(dtype)[hi_i], n, q, dtype)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert bits_equal(got, np.nanpercentile(a.astype(dtype), q)), (dtype, q)
    # the tuple form Volume.fit_robust_scaler uses: f64 quantiles
    q3 = np.nanpercentile(a.astype(np.float64), (25.0, 50.0, 75.0))
    for k, q in enumerate((25.0, 50.0, 75.0)):
        lo_i, hi_i, _ = S.percentile_ranks(n, np.float64(q), np.float64)
        assert bits_equal(S.percentile_from_order_stats(np.float64(srt[lo_i]), np.float64(srt[hi_i]), n, np.float64(q), np.float64),
                          q3[k])


@pytest.mark.parametrize("K", SD.SCALERS)
@pytest.mark.parametrize("v", list(SD.VOLUMES))
def test_transform_host_equals_the_golden_transform(G, v, K):
    sc = golden_scaler(G, v, K)
    assert sc.kind == KIND[K]
    got = sc.transform_host(G[v + "/planes"])
    want = G["%s/%s/transform" % (v, K)]
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)                        # (NaN == NaN here)
    assert np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("K", SD.SCALERS)
@pytest.mark.parametrize("v", list(SD.VOLUMES))
def test_host_fit_reproduces_the_golden_parameters(G, v, K):
    """MinMax / MaxAbs / Robust / Quantile attributes bit for bit (order statistics and f32 / f64 scalar operations);
    StandardScaler's mean and variance within the first-order bound of an fp64 sum of n terms taken in another order."""
    vol = SD.make_volume(v)
    sc = S.fit_scaler_host(K, vol)
    g = lambda a: G["%s/%s/%s" % (v, K, a)]
    if K == "StandardScaler":
        x = vol.reshape(-1, vol.shape[-1]).astype(np.float64)
        n = (~np.isnan(x)).sum(0)
        u = 2.0 ** -53
        mean_abs = np.nanmean(np.abs(x), axis=0)
        assert np.all(np.abs(sc.fitted["mean_"] - g("mean_")) <= 2 * n * u * mean_abs)
        dev2 = np.nanmean((x - g("mean_")) ** 2, axis=0)
        assert np.all(np.abs(sc.fitted["var_"] - g("var_")) <= 2 * n * u * dev2)
        np.testing.assert_allclose(sc.p1, g("scale_"), rtol=1e-9)
        return
    for a in {"MinMaxScaler": ("scale_", "min_", "data_min_", "data_max_"), "MaxAbsScaler": ("max_abs_", "scale_"),
              "RobustScaler": ("center_", "scale_"), "QuantileTransformer": ("quantiles_", "references_")}[K]:
        assert bits_equal(np.asarray(sc.fitted[a]), g(a)), a


def test_robust_fit_is_fit_robust_scaler():
    for v in SD.VOLUMES:
        vol = SD.make_volume(v)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c, s = Volume.fit_robust_scaler(vol)
        sc = S.fit_scaler_host("RobustScaler", vol)
        c2, s2 = sc                                                  # a SUB_DIV scaler unpacks like the old tuple
        assert bits_equal(c, c2) and bits_equal(s, s2)


def test_constant_channel_gives_scale_one(G):
    vol = SD.make_volume("v3")
    for K in ("MinMaxScaler", "StandardScaler", "MaxAbsScaler", "RobustScaler"):
        sc = S.fit_scaler_host(K, vol)
        if K == "MaxAbsScaler":
            assert sc.p0[0] == 7.25                                  # |x| is not zero: sklearn divides by it
        elif K == "MinMaxScaler":
            assert sc.p0[0] == 1.0
        else:
            assert sc.p1[0] == 1.0
        assert bits_equal(np.asarray(sc.p0, np.float64), np.asarray(golden_scaler(G, "v3", K).p0, np.float64))


def test_channel_with_nans_fits_as_sklearn_does(G):
    vol = SD.make_volume("v1n")
    assert np.isnan(vol).sum() > 50
    for K in ("MinMaxScaler", "MaxAbsScaler", "RobustScaler", "QuantileTransformer"):
        sc, ref = S.fit_scaler_host(K, vol), golden_scaler(G, "v1n", K)
        for a in ("p0", "p1", "quantiles"):
            if getattr(ref, a) is not None:
                assert bits_equal(getattr(sc, a), getattr(ref, a)), (K, a)
    sc = S.fit_scaler_host("StandardScaler", vol)
    np.testing.assert_allclose(sc.p0, G["v1n/StandardScaler/mean_"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sc.p1, G["v1n/StandardScaler/scale_"], rtol=1e-12)


def test_unknown_scaler_name_raises_naming_the_five():
    with pytest.raises(NotImplementedError) as e:
        S.fit_scaler_host("PowerTransformer", np.zeros((2, 2, 2, 1), np.float32))
    for name in SD.SCALERS:
        assert name in str(e.value)
    from multiplanarunet_amd.data import as_volume
    with pytest.raises(NotImplementedError) as e:
        as_volume(np.zeros((2, 2, 2, 1), np.float32), None, np.eye(4), 0.0, "PowerTransformer", "cpu", fit_on="host")
    for name in SD.SCALERS:
        assert name in str(e.value)


def test_scaler_descriptor_layout():
    import ctypes
    from multiplanarunet_amd import _lib
    assert ctypes.sizeof(_lib.ScalerDesc) == 8 + 4 * 8
    assert (_lib.MPU_SCALER_NONE, _lib.MPU_SCALER_SUB_DIV, _lib.MPU_SCALER_MUL_ADD, _lib.MPU_SCALER_DIV,
            _lib.MPU_SCALER_QUANTILE) == (S.NONE, S.SUB_DIV, S.MUL_ADD, S.DIV, S.QUANTILE)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpunet_hip.h")).read()
    for k, name in enumerate(("NONE", "SUB_DIV", "MUL_ADD", "DIV", "QUANTILE")):
        assert "MPU_SCALER_%s = %d" % (name, k) in hdr


def test_live_sklearn_agrees_with_the_golden_and_transform_host(G):
    pytest.importorskip("sklearn")
    from sklearn import preprocessing
    v = "v1n"
    vol, planes = SD.make_volume(v), G[v + "/planes"]
    for K in SD.SCALERS:
        ours = S.fit_scaler_host(K, vol)
        T = np.empty_like(planes)
        for c in range(vol.shape[-1]):
            col = vol[..., c].reshape(-1, 1)
            if K == "RobustScaler":
                col = col.astype(np.float64)
            kw = {"random_state": 0} if K == "QuantileTransformer" else {}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                obj = getattr(preprocessing, K)(**kw).fit(col)
                T[..., c] = obj.transform(planes[..., c].reshape(-1, 1).copy()).reshape(planes.shape[:-1])
            if K == "QuantileTransformer":
                np.testing.assert_array_equal(obj.quantiles_[:, 0], G["%s/%s/quantiles_" % (v, K)][c])
            elif K != "StandardScaler":
                np.testing.assert_array_equal(np.ravel(obj.scale_), G["%s/%s/scale_" % (v, K)][c:c + 1])
        np.testing.assert_array_equal(T, G["%s/%s/transform" % (v, K)])
        if K != "StandardScaler":                                    # (its parameters agree to rounding, not to the bit)
            np.testing.assert_array_equal(ours.transform_host(planes), T)
