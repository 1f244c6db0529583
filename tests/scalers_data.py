"""Volumes of the scaler tests (tests/golden/make_scalers_golden.py, test_scalers_host.py, test_gpu_scalers.py): regenerated
from a seed, because the larger ones are beyond what a golden file should carry; only what sklearn made of them is stored."""
import numpy as np

VOLUMES = {            # name: (shape, seed)
    "v1": ((24, 20, 17, 2), 11),       # odd extents: the 16-byte loads' tails
    "v2": ((70, 66, 65, 3), 12),       # ~300 k voxels per channel, three interleaved channels: many workgroups
    "v3": ((16, 16, 16, 1), 13),       # one constant channel
    "v1n": ((24, 20, 17, 2), 11),      # v1 with 1 % NaN
}
SCALERS = ("MinMaxScaler", "StandardScaler", "MaxAbsScaler", "RobustScaler", "QuantileTransformer")


def raw_values(rs, n):
    """Normal values x 10^U(-3,3), half of them replaced by a copy quantised to 7 distinct values (heavy ties inside one
    radix bin and across bins), with negatives, +-0.0 and denormals sprinkled in."""
    x = rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 3, n)
    levels = np.array([-250.0, -1.5, -1.4999999, 0.0, 1e-3, 3.0, 3.0000002])
    quant = levels[rs.randint(0, 7, n)]
    x = np.where(rs.rand(n) < 0.5, x, quant).astype(np.float32)
    k = max(4, n // 50)
    idx = rs.randint(0, n, (4, k))
    x[idx[0]] = np.float32(0.0)
    x[idx[1]] = np.float32(-0.0)
    x[idx[2]] = np.float32(1e-41) * rs.randint(-9, 10, k).astype(np.float32)       # denormals of both signs
    x[idx[3]] = -np.abs(x[idx[3]])
    return x


def make_volume(name, with_inf=False, with_nan=None):
    """f32 [X,Y,Z,C]. with_inf: +-inf at both ends (order statistics only: sklearn refuses infinite input); with_nan: 1 % NaN
    (default: the volumes whose name ends in n)."""
    shape, seed = VOLUMES[name]
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if name == "v3":
        return np.full(shape, np.float32(-7.25), np.float32)
    x = raw_values(rs, n)
    if name.endswith("n") if with_nan is None else with_nan:
        x[rs.rand(n) < 0.01] = np.nan
    if with_inf:
        j = rs.randint(0, n, 12)
        x[j[:6]] = np.inf
        x[j[6:]] = -np.inf
    return x.reshape(shape)
