"""
The five scalers the reference's YAML documents for `fit.scaler` (bin/defaults/MultiPlanar/train_hparams.yaml:132-136:
MinMaxScaler, StandardScaler, MaxAbsScaler, RobustScaler, QuantileTransformer), fitted per channel on the volume that is
already resident on the GPU, and the '<N>pct' background value (mpunet/image/image_pair.py:300-341,469-484;
mpunet/preprocessing/scaling.py:47-89, which fit sklearn objects on the host).

The statistics come from csrc/volume_stats.hip (exact order statistics by radix select; fp64 moments); the few scalar
operations that turn them into sklearn's fitted attributes are restated here from scikit-learn 1.7.2 (the reference only
requires >= 0.23; where versions differ, 1.7.2 is what tests/golden/scalers_golden.npz pins). The transform runs inside
the sampling kernels (csrc/geometry.hip apply_scaler); `Scaler.transform_host` is its NumPy restatement.

sklearn on an f32 image keeps MinMaxScaler's and MaxAbsScaler's attributes in f32 and StandardScaler's / QuantileTransformer's
in f64; so do the fits here. RobustScaler is the exception the project already had: `Volume.fit_robust_scaler` applies
np.nanpercentile's rule to the f64 image, and `fit_scaler("RobustScaler", ...)` returns exactly that.

QuantileTransformer draws its 10 000-sample subsample at random and the reference leaves `random_state=None`, so the
reference's own fit differs from run to run; here the draw is sklearn's (`utils.resample`: shuffle arange(n) with a
RandomState, keep the first 10 000) under a fixed seed, which equals `QuantileTransformer(random_state=seed)`.
"""
import ctypes as C
import numpy as np

from . import _lib

SCALER_NAMES = ("MinMaxScaler", "StandardScaler", "MaxAbsScaler", "RobustScaler", "QuantileTransformer")
NONE, SUB_DIV, MUL_ADD, DIV, QUANTILE = range(5)
MAX_RANKS = 16
QUANTILE_SUBSAMPLE = 10000
QUANTILE_N = 1000
QUANTILE_LDS_BYTES = 65536       # the sampling kernels stage references + every channel's quantiles in LDS (mpu_scaler)


def check_scaler_name(name):
    if name not in SCALER_NAMES:
        raise NotImplementedError("scaler %r: the supported scalers are %s (or Null)" % (name, ", ".join(SCALER_NAMES)))


# --------------------------------------------------------------------------- #
# np.percentile's 'linear' rule from two order statistics
# --------------------------------------------------------------------------- #
def percentile_ranks(n, q, dtype):
    """(previous, next, gamma) of np.percentile(a, q) for len(a) == n, a.dtype == dtype, method 'linear'.
    NumPy divides q by dtype.type(100): a Python-number q on an f32 array gives an f32 quantile, and the virtual index
    (n - 1) * q and gamma are then f32 as well -- which decides even which two ranks are read. An np.float64 q (what the
    elements of a q tuple become) keeps everything in f64."""
    dtype = np.dtype(dtype)
    quant = np.true_divide(q, dtype.type(100))
    vi = np.asanyarray((n - 1) * quant)
    prev = np.floor(vi)
    nxt = prev + 1
    if vi >= n - 1:                        # _get_indexes: index -1, which gamma is then taken against
        prev = nxt = -1
    if vi < 0:
        prev = nxt = 0
    prev, nxt = int(prev), int(nxt)
    gamma = np.asanyarray(vi - np.intp(prev), dtype=vi.dtype)
    return prev % n, nxt % n, gamma


def percentile_from_order_stats(lo, hi, n, q, dtype):
    """np.percentile(a, q) / np.nanpercentile(a, q) (n = number of non-NaN values) given lo = sort(a)[previous] and
    hi = sort(a)[next] of percentile_ranks(n, q, dtype): NumPy's _lerp, a + (b - a) t, switched to b - (b - a)(1 - t) for
    t >= 0.5, in the dtypes NumPy uses."""
    dtype = np.dtype(dtype)
    _, _, t = percentile_ranks(n, q, dtype)
    a, b = np.asanyarray(lo, dtype=dtype), np.asanyarray(hi, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.subtract(b, a)
        out = np.asanyarray(np.add(a, diff * t))
        if t >= 0.5:
            out = np.asanyarray(np.subtract(b, diff * (1 - t)), dtype=out.dtype)
    return out[()]


# --------------------------------------------------------------------------- #
# device statistics
# --------------------------------------------------------------------------- #
def _workspace(image_dev):
    import torch
    nb = int(_lib.load().mpu_volume_stats_workspace_bytes(int(image_dev.shape[-1])))
    return torch.empty(nb, dtype=torch.uint8, device=image_dev.device), nb


def _check_image(image_dev):
    if image_dev.ndim != 4 or str(image_dev.dtype) != "torch.float32" or not image_dev.is_contiguous():
        raise ValueError("need a contiguous f32 [X,Y,Z,C] device tensor")
    return int(image_dev.numel() // image_dev.shape[-1]), int(image_dev.shape[-1])


def order_stats(image_dev, channel, ranks, workspace=None):
    """(np.sort(x[~isnan(x)])[ranks] as f32, NaN count) of channel `channel` of a device image; <= 16 ranks per launch set."""
    import torch
    n_vox, Cn = _check_image(image_dev)
    ws, nb = workspace or _workspace(image_dev)
    ranks = [int(r) for r in ranks]
    out = np.empty(len(ranks), np.float32)
    nan_count = 0
    with torch.cuda.device(image_dev.device):
        for i in range(0, len(ranks), MAX_RANKS):
            part = ranks[i:i + MAX_RANKS]
            r = (C.c_int64 * len(part))(*part)
            v = (C.c_float * len(part))()
            nn = C.c_int64(0)
            _lib.call("mpu_volume_order_stats", _lib.ptr(image_dev), n_vox, Cn, int(channel), r, len(part), _lib.ptr(ws), nb,
                      v, C.byref(nn), _lib.stream_ptr())
            out[i:i + len(part)] = np.frombuffer(v, np.float32)
            nan_count = int(nn.value)
    return out, nan_count


MOMENT_KEYS = ("count", "min", "max", "max_abs", "sum", "sum_dev", "sum_dev2")


def moments(image_dev, mean=None, workspace=None):
    """Per channel, f64 [C, 8]: count, min, max, max|x|, sum of the non-NaN values (mean is None), or, given the means,
    columns 5, 6 = sum(x - mean), sum((x - mean)^2)."""
    import torch
    n_vox, Cn = _check_image(image_dev)
    ws, nb = workspace or _workspace(image_dev)
    out = np.zeros((Cn, 8), np.float64)
    m = None
    if mean is not None:
        m = np.ascontiguousarray(mean, np.float64)
        assert m.shape == (Cn,)
    with torch.cuda.device(image_dev.device):
        _lib.call("mpu_volume_moments", _lib.ptr(image_dev), n_vox, Cn,
                  None if m is None else m.ctypes.data_as(C.POINTER(C.c_double)), _lib.ptr(ws), nb,
                  out.ctypes.data_as(C.POINTER(C.c_double)), _lib.stream_ptr())
    return out


def percentiles_device(image_dev, channel, requests, workspace=None):
    """[np.nanpercentile-style value per (q, dtype, nan_rule) request] of one channel from ONE radix select when the
    channel has no NaN (the select is run for n = all voxels; a NaN count above zero means the ranks were those of the
    wrong n, and the select is repeated for the non-NaN count). nan_rule 'propagate' is np.percentile: NaN if any NaN."""
    n_vox, _ = _check_image(image_dev)
    workspace = workspace or _workspace(image_dev)

    def run(n):
        ranks = []
        for q, dtype, _ in requests:
            p, x, _ = percentile_ranks(n, q, dtype)
            ranks += [p, x]
        vals, n_nan = order_stats(image_dev, channel, ranks, workspace)
        return vals, n_nan

    vals, n_nan = run(n_vox)
    n = n_vox - n_nan
    if n_nan and n > 0 and any(rule != "propagate" for _, _, rule in requests):
        vals, _ = run(n)
    out = []
    for k, (q, dtype, rule) in enumerate(requests):
        dtype = np.dtype(dtype)
        if n == 0 or (n_nan and rule == "propagate"):
            out.append(dtype.type(np.nan))
        else:
            out.append(percentile_from_order_stats(dtype.type(vals[2 * k]), dtype.type(vals[2 * k + 1]), n, q, dtype))
    return out


# --------------------------------------------------------------------------- #
# the fitted scaler
# --------------------------------------------------------------------------- #
class Scaler:
    """A per-channel scaler as the numbers the sampling kernels apply (include/mpunet_hip.h, mpu_scaler):
        SUB_DIV   p0 = center_ / mean_, p1 = scale_     RobustScaler, StandardScaler
        MUL_ADD   p0 = scale_, p1 = min_                MinMaxScaler
        DIV       p0 = scale_                           MaxAbsScaler
        QUANTILE  quantiles [C, n_quantiles], references [n_quantiles]
    A SUB_DIV scaler unpacks like the (center, scale) tuple it replaces."""

    def __init__(self, kind, p0=None, p1=None, quantiles=None, references=None, name=None, fitted=None):
        self.kind = int(kind)
        self.name = name
        self.p0 = None if p0 is None else np.atleast_1d(np.asarray(p0, np.float64))
        self.p1 = None if p1 is None else np.atleast_1d(np.asarray(p1, np.float64))
        self.quantiles = None if quantiles is None else np.ascontiguousarray(quantiles, np.float64)
        self.references = None if references is None else np.ascontiguousarray(references, np.float64)
        self.fitted = dict(fitted or {})          # sklearn's attribute names -> arrays, in sklearn's dtypes (for inspection)
        if self.kind in (SUB_DIV, MUL_ADD) and (self.p0 is None or self.p1 is None):
            raise ValueError("this scaler kind needs p0 and p1")
        if self.kind == DIV and self.p0 is None:
            raise ValueError("DIV needs p0")
        if self.kind == QUANTILE and (self.quantiles is None or self.references is None or self.quantiles.ndim != 2
                                      or self.quantiles.shape[1] != self.references.shape[0]):
            raise ValueError("QUANTILE needs quantiles [C, n] and references [n]")
        if self.kind == QUANTILE and (self.quantiles.shape[0] + 1) * self.quantiles.shape[1] * 8 > QUANTILE_LDS_BYTES:
            raise NotImplementedError("QuantileTransformer on %d channels x %d quantiles: the sampling kernels hold the tables "
                                      "of all channels in %d bytes of LDS (at 1000 quantiles: up to 7 channels)"
                                      % (self.quantiles.shape[0], self.quantiles.shape[1], QUANTILE_LDS_BYTES))
        self._dev = {}

    @classmethod
    def from_center_scale(cls, center, scale, name=None):
        return cls(SUB_DIV, center, scale, name=name)

    def __iter__(self):
        if self.kind != SUB_DIV:
            raise TypeError("only a SUB_DIV scaler unpacks into (center, scale)")
        return iter((self.p0, self.p1))

    @property
    def n_channels(self):
        return int((self.quantiles if self.kind == QUANTILE else self.p0).shape[0])

    def transform_host(self, planes):
        """sklearn's transform of f32 planes [..., C], restated in NumPy: in-place operations of an f32 array with the f64
        parameters (an f64 operation and an f32 store per step)."""
        X = np.array(planes, dtype=np.float32, copy=True)
        if X.shape[-1] != self.n_channels:
            raise ValueError("planes have %d channels, the scaler %d" % (X.shape[-1], self.n_channels))
        with np.errstate(all="ignore"):
            if self.kind == SUB_DIV:
                X -= self.p0
                X /= self.p1
            elif self.kind == MUL_ADD:
                X *= self.p0
                X += self.p1
            elif self.kind == DIV:
                X /= self.p0
            elif self.kind == QUANTILE:
                r = self.references
                for c in range(X.shape[-1]):
                    q = self.quantiles[c]
                    col = X[..., c]                                  # QuantileTransformer._transform_col, uniform output
                    lower, upper = col == q[0], col == q[-1]
                    ok = ~np.isnan(col)
                    v = col[ok]
                    col[ok] = 0.5 * (np.interp(v, q, r) - np.interp(-v, -q[::-1], -r[::-1]))
                    col[upper] = 1
                    col[lower] = 0
        return X

    def device_struct(self, device):
        """ctypes mpu_scaler whose pointers are device tensors kept alive by this object (one upload per device)."""
        import torch
        key = str(device)
        hit = self._dev.get(key)
        if hit is None:
            t = {k: (None if v is None else torch.tensor(v, dtype=torch.float64, device=device).contiguous())
                 for k, v in (("p0", self.p0), ("p1", self.p1), ("quantiles", self.quantiles), ("references", self.references))}
            s = _lib.ScalerDesc()
            s.kind = self.kind
            s.n_quantiles = 0 if self.kind != QUANTILE else int(self.references.shape[0])
            for k, v in t.items():
                setattr(s, k, None if v is None else v.data_ptr())
            hit = self._dev[key] = (s, t)
        return hit[0]


def as_scaler(scaler):
    """None, a Scaler, or the (center, scale) tuple of older callers (= SUB_DIV)."""
    if scaler is None or isinstance(scaler, Scaler):
        return scaler
    c, s = scaler
    return Scaler.from_center_scale(c, s)


# --------------------------------------------------------------------------- #
# fits (scikit-learn 1.7.2 semantics; all ignore NaN)
# --------------------------------------------------------------------------- #
def _handle_zeros(scale):
    scale = np.array(scale, copy=True)
    scale[scale == 0.0] = 1.0
    return scale


def robust_from_quartiles(q25, q50, q75):
    """Volume.fit_robust_scaler's last step: center = median, scale = IQR, zero IQR -> 1."""
    c = np.asarray(q50, np.float64)
    s = np.asarray(q75, np.float64) - np.asarray(q25, np.float64)
    return c, np.where(s != 0, s, 1.0)


def minmax_from_stats(data_min, data_max):
    """MinMaxScaler.partial_fit, feature_range (0, 1), on f32 data: f32 attributes."""
    data_min, data_max = np.asarray(data_min, np.float32), np.asarray(data_max, np.float32)
    with np.errstate(all="ignore"):
        data_range = data_max - data_min
        rng = np.array(data_range, copy=True)
        rng[rng < 10 * np.finfo(np.float32).eps] = 1.0           # _handle_zeros_in_scale on an array: near-constant -> 1
        scale = (1 - 0) / rng
        mn = 0 - data_min * scale
    return {"data_min_": data_min, "data_max_": data_max, "data_range_": data_range, "scale_": scale, "min_": mn}


def maxabs_from_stats(max_abs):
    """MaxAbsScaler.partial_fit on f32 data: f32 attributes."""
    max_abs = np.asarray(max_abs, np.float32)
    scale = np.array(max_abs, copy=True)
    scale[scale < 10 * np.finfo(np.float32).eps] = 1.0
    return {"max_abs_": max_abs, "scale_": scale}


def standard_from_moments(count, total, sum_dev, sum_dev2):
    """StandardScaler's first partial_fit: _incremental_mean_and_var from zero state (mean = sum / n; the corrected
    two-pass variance (sum (x - mean)^2 - (sum (x - mean))^2 / n) / n), then _is_constant_feature and the square root."""
    n = np.asarray(count, np.float64)
    with np.errstate(all="ignore"):
        mean = np.asarray(total, np.float64) / n
        unnorm = np.asarray(sum_dev2, np.float64) - np.asarray(sum_dev, np.float64) ** 2 / n
        var = unnorm / n
        eps = np.finfo(np.float64).eps
        constant = var <= n * eps * var + (n * mean * eps) ** 2
        scale = np.sqrt(var)
    scale = np.array(scale, copy=True)
    scale[constant] = 1.0
    return {"mean_": mean, "var_": var, "scale_": scale}


def quantile_subsample_indices(n, seed=0):
    """The rows sklearn's QuantileTransformer(random_state=seed) fits on: all for n <= 10 000, else utils.resample's draw."""
    if n <= QUANTILE_SUBSAMPLE:
        return None
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    return idx[:QUANTILE_SUBSAMPLE]


def quantile_from_samples(samples, n_total):
    """QuantileTransformer._dense_fit on the (sub)sample of one channel: references and monotone quantiles."""
    nq = max(1, min(QUANTILE_N, int(n_total)))
    references = np.linspace(0, 1, nq, endpoint=True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        q = np.nanpercentile(np.asarray(samples), references * 100)
    return references, np.maximum.accumulate(q)


def fit_scaler_host(name, image_np, seed=0):
    """The fits from host NumPy statistics (the path before the device kernels; kept for A/B and tests)."""
    check_scaler_name(name)
    image_np = np.asarray(image_np, np.float32)
    Cn = image_np.shape[-1]
    flat = image_np.reshape(-1, Cn)
    import warnings
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        if name == "RobustScaler":
            qs = [np.nanpercentile(flat[:, c].astype(np.float64), (25.0, 50.0, 75.0)) for c in range(Cn)]
            c_, s_ = robust_from_quartiles([q[0] for q in qs], [q[1] for q in qs], [q[2] for q in qs])
            return Scaler(SUB_DIV, c_, s_, name=name, fitted={"center_": c_, "scale_": s_})
        if name == "MinMaxScaler":
            f = minmax_from_stats(np.nanmin(flat, axis=0), np.nanmax(flat, axis=0))
            return Scaler(MUL_ADD, f["scale_"], f["min_"], name=name, fitted=f)
        if name == "MaxAbsScaler":
            f = maxabs_from_stats(np.nanmax(np.abs(flat), axis=0))
            return Scaler(DIV, f["scale_"], name=name, fitted=f)
        if name == "StandardScaler":
            x = flat.astype(np.float64)
            n = (~np.isnan(x)).sum(axis=0).astype(np.float64)
            total = np.nansum(x, axis=0)
            d = x - total / n
            f = standard_from_moments(n, total, np.nansum(d, axis=0), np.nansum(d * d, axis=0))
            return Scaler(SUB_DIV, f["mean_"], f["scale_"], name=name, fitted=f)
        idx = quantile_subsample_indices(flat.shape[0], seed)
        sub = flat if idx is None else flat[idx]
        refs, qs = None, []
        for c in range(Cn):
            refs, q = quantile_from_samples(sub[:, c], flat.shape[0])
            qs.append(q)
        return Scaler(QUANTILE, quantiles=np.stack(qs), references=refs, name=name,
                      fitted={"quantiles_": np.stack(qs), "references_": refs})


def fit_scaler(name, image_dev, seed=0):
    """Fit the named sklearn scaler per channel on a device image f32 [X,Y,Z,C]; returns a Scaler."""
    check_scaler_name(name)
    n_vox, Cn = _check_image(image_dev)
    ws = _workspace(image_dev)
    if name == "RobustScaler":
        qs = [percentiles_device(image_dev, c, [(np.float64(q), np.float64, "omit") for q in (25.0, 50.0, 75.0)], ws)
              for c in range(Cn)]
        c_, s_ = robust_from_quartiles([q[0] for q in qs], [q[1] for q in qs], [q[2] for q in qs])
        return Scaler(SUB_DIV, c_, s_, name=name, fitted={"center_": c_, "scale_": s_})
    if name in ("MinMaxScaler", "MaxAbsScaler", "StandardScaler"):
        m = moments(image_dev, None, ws)
        with np.errstate(all="ignore"):
            empty = m[:, 0] == 0
            if name == "MinMaxScaler":
                f = minmax_from_stats(np.where(empty, np.nan, m[:, 1]), np.where(empty, np.nan, m[:, 2]))
                return Scaler(MUL_ADD, f["scale_"], f["min_"], name=name, fitted=f)
            if name == "MaxAbsScaler":
                f = maxabs_from_stats(np.where(empty, np.nan, m[:, 3]))
                return Scaler(DIV, f["scale_"], name=name, fitted=f)
            mean = m[:, 4] / m[:, 0]
        m2 = moments(image_dev, mean, ws)
        f = standard_from_moments(m[:, 0], m[:, 4], m2[:, 5], m2[:, 6])
        return Scaler(SUB_DIV, f["mean_"], f["scale_"], name=name, fitted=f)
    import torch
    flat = image_dev.reshape(-1, Cn)
    idx = quantile_subsample_indices(n_vox, seed)
    sub = flat if idx is None else flat[torch.as_tensor(idx, device=image_dev.device)]
    sub = sub.cpu().numpy()                                       # <= 10 000 rows
    refs, qs = None, []
    for c in range(Cn):
        refs, q = quantile_from_samples(sub[:, c], n_vox)
        qs.append(q)
    return Scaler(QUANTILE, quantiles=np.stack(qs), references=refs, name=name,
                  fitted={"quantiles_": np.stack(qs), "references_": refs})


def bg_percentile_device(image_dev, pct, workspace=None):
    """[float(np.percentile(image[..., c], pct)) for c] from the device image (NumPy's f32 rule; NaN if the channel has one)."""
    Cn = int(image_dev.shape[-1])
    workspace = workspace or _workspace(image_dev)
    return [float(percentiles_device(image_dev, c, [(pct, np.float32, "propagate")], workspace)[0]) for c in range(Cn)]


def prepare_device(image_dev, pct, scaler_name, seed=0):
    """bg percentile (pct None: skip) and scaler of one volume. With the default RobustScaler both come out of one radix
    select per channel: 8 ranks."""
    Cn = int(image_dev.shape[-1])
    if scaler_name:
        check_scaler_name(scaler_name)
    ws = _workspace(image_dev)
    if pct is not None and scaler_name == "RobustScaler":
        req = [(pct, np.float32, "propagate")] + [(np.float64(q), np.float64, "omit") for q in (25.0, 50.0, 75.0)]
        res = [percentiles_device(image_dev, c, req, ws) for c in range(Cn)]
        c_, s_ = robust_from_quartiles([r[1] for r in res], [r[2] for r in res], [r[3] for r in res])
        return [float(r[0]) for r in res], Scaler(SUB_DIV, c_, s_, name=scaler_name, fitted={"center_": c_, "scale_": s_})
    bg = None if pct is None else bg_percentile_device(image_dev, pct, ws)
    return bg, (fit_scaler(scaler_name, image_dev, seed) if scaler_name else None)
