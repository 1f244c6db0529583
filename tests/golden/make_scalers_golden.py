"""
Writes tests/golden/scalers_golden.npz: what scikit-learn (1.7.2 when the file was made) fits and transforms for the volumes
of tests/scalers_data.py. Run on the CPU:  python tests/golden/make_scalers_golden.py

Per volume v and class K, per channel (as mpunet/preprocessing/scaling.py's MultiChannelScaler fits them: one sklearn object
per channel on the [n, 1] column):
    <v>/<K>/<attribute>      fitted attributes stacked over the channels, in sklearn's dtypes
    <v>/planes               f32 [5, 32, 32, C]: values inside the data's range, beyond both ends, exact hits on quantile
                             knots (first, last and inner ones), +-0.0 and one NaN
    <v>/<K>/transform        scaler.transform(planes), channel by channel, f32
RobustScaler is fitted on the f64 copy of the column: the project's rule (Volume.fit_robust_scaler) is np.nanpercentile on
the f64 image, which is sklearn's RobustScaler on f64 input. QuantileTransformer is given random_state=0 (the reference
leaves it None: its fit is random).
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from scalers_data import VOLUMES, SCALERS, make_volume      # noqa: E402

ATTRS = {"MinMaxScaler": ("scale_", "min_", "data_min_", "data_max_"), "StandardScaler": ("mean_", "var_", "scale_"),
         "MaxAbsScaler": ("max_abs_", "scale_"), "RobustScaler": ("center_", "scale_"),
         "QuantileTransformer": ("quantiles_", "references_")}


def make_planes(vol, quantiles, seed):
    """quantiles: [C][nq] of the fitted QuantileTransformer (knots to hit exactly)."""
    C = vol.shape[-1]
    rs = np.random.RandomState(seed)
    P = np.empty((5, 32, 32, C), np.float32)
    for c in range(C):
        col = vol[..., c].ravel()
        col = col[~np.isnan(col)]
        lo, hi = float(col.min()), float(col.max())
        span = (hi - lo) or 1.0
        n = 5 * 32 * 32
        x = rs.choice(col, n).astype(np.float64)                                   # values of the data (ties with the knots)
        x[:n // 4] = rs.uniform(lo, hi, n // 4)                                    # inside the range
        x[n // 4:n // 4 + 64] = hi + span * rs.uniform(0, 2, 64)                   # beyond both ends
        x[n // 4 + 64:n // 4 + 128] = lo - span * rs.uniform(0, 2, 64)
        q = quantiles[c]
        knots = np.concatenate([q[[0, 0, -1, -1, 1, len(q) // 2, len(q) - 2]], rs.choice(q, 249)])
        x[n // 2:n // 2 + 256] = knots                                             # exact knot hits (those that are f32 values)
        x = x.astype(np.float32)
        x[n // 2 + 256:n // 2 + 264] = [0.0, -0.0, 0.0, -0.0, np.float32(lo), np.float32(hi), 1e-41, -1e-41]
        rs.shuffle(x)
        P[..., c] = x.reshape(5, 32, 32)
    P[3, 7, 9, 0] = np.nan
    return P


def main():
    import sklearn
    from sklearn import preprocessing
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for vi, v in enumerate(VOLUMES):
            vol = make_volume(v)
            C = vol.shape[-1]
            fitted = {}
            for K in SCALERS:
                objs = []
                for c in range(C):
                    col = vol[..., c].reshape(-1, 1)
                    if K == "RobustScaler":
                        col = col.astype(np.float64)
                    kw = {"random_state": 0} if K == "QuantileTransformer" else {}
                    objs.append(getattr(preprocessing, K)(**kw).fit(col))
                fitted[K] = objs
                for a in ATTRS[K]:
                    if a == "references_":
                        out["%s/%s/%s" % (v, K, a)] = objs[0].references_
                    else:
                        out["%s/%s/%s" % (v, K, a)] = np.stack([np.ravel(getattr(o, a)) for o in objs]).squeeze(-1) \
                            if a != "quantiles_" else np.stack([o.quantiles_[:, 0] for o in objs])
            planes = make_planes(vol, [o.quantiles_[:, 0] for o in fitted["QuantileTransformer"]], 100 + vi)
            out["%s/planes" % v] = planes
            for K in SCALERS:
                T = np.empty_like(planes)
                for c in range(C):
                    T[..., c] = fitted[K][c].transform(planes[..., c].reshape(-1, 1).copy()).reshape(planes.shape[:-1])
                assert T.dtype == np.float32
                out["%s/%s/transform" % (v, K)] = T
    path = os.path.join(HERE, "scalers_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
