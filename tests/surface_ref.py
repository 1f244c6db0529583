"""NumPy restatement of csrc/surface.hip (test aid; imported like components_ref.py): the squared Euclidean distance transform as
DEFINED in include/mpunet_hip.h, in its all-pairs form (edt2_brute) and in the separable three-pass form (edt2_three_pass), which
tests/test_surface_host.py proves equal bit for bit on the small cases and holds to scipy; the border of a mask; the per-class
surface-distance table; and the case lists both test files share."""
import functools
import math

import numpy as np

EQUAL, NOT_EQUAL, BORDER = 0, 1, 2
PREDICATES = (EQUAL, NOT_EQUAL, BORDER)
SPACINGS = ((1.0, 1.0, 1.0), (0.7, 1.0, 2.5), (0.1, 1.0, 10.0), (0.78125, 0.78125, 3.3))


def border(mask):
    """The voxels of `mask` with at least one of the six face neighbours outside it; outside the volume is outside the mask."""
    m = np.asarray(mask, dtype=bool)
    p = np.pad(m, 1, constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m & ~inner


def feature_of(labels, predicate, value):
    if predicate == EQUAL:
        return labels == value
    if predicate == NOT_EQUAL:
        return labels != value
    return border(labels == value)


def weights(spacing):
    s = np.asarray(spacing, dtype=np.float64)
    return s * s


def edt2_brute(feature, spacing):
    """d2(p) = min over feature voxels q of fl(fl(wx dx^2) + fl(fl(wy dy^2) + fl(wz dz^2))): every pair, exactly that order."""
    feature = np.asarray(feature, dtype=bool)
    wx, wy, wz = weights(spacing)
    out = np.full(feature.shape, np.inf, dtype=np.float64)
    q = np.argwhere(feature).astype(np.int64)                      # [F, 3]
    if q.shape[0] == 0:
        return out
    p = np.argwhere(np.ones(feature.shape, dtype=bool)).astype(np.int64)        # [N, 3], C order
    flat = out.reshape(-1)
    chunk = max(1, (1 << 22) // q.shape[0])
    for lo in range(0, p.shape[0], chunk):
        d = p[lo:lo + chunk, None, :] - q[None, :, :]
        sq = (d * d).astype(np.float64)                            # exact integers
        cand = wx * sq[..., 0] + (wy * sq[..., 1] + wz * sq[..., 2])
        flat[lo:lo + chunk] = cand.min(axis=1)
    return out


def _line_pass(g, axis, w):
    """min over k of fl(fl(w (i - k)^2) + g[k]) along `axis` (the true minimum of every line)."""
    g = np.moveaxis(g, axis, -1)
    L = g.shape[-1]
    k = np.arange(L, dtype=np.int64)
    out = np.empty_like(g)
    for lo in range(0, L, 128):
        i = k[lo:lo + 128]
        d = i[:, None] - k[None, :]
        a = w * (d * d).astype(np.float64)                         # [chunk, L]
        out[..., lo:lo + 128] = (a + g[..., None, :]).min(axis=-1)
    return np.moveaxis(out, -1, axis)


def edt2_three_pass(feature, spacing):
    """The same quantity by three line minima: Z, then Y, then X."""
    feature = np.asarray(feature, dtype=bool)
    wx, wy, wz = weights(spacing)
    g = np.where(feature, 0.0, np.inf)
    return np.ascontiguousarray(_line_pass(_line_pass(_line_pass(g, 2, wz), 1, wy), 0, wx))


def surface_table(pred, truth, K, spacing, tau, classes=None):
    """The dict multiplanarunet_amd.surface.surface_distances returns, restated: medpy's hd / hd95 / assd on border voxels and the
    voxel-border NSD; assd summed with math.fsum. Also "lists": per class the two directed lists of SQUARED distances."""
    out = {k: np.full(K, np.nan) for k in ("hd", "hd95", "assd", "nsd", "n_pred_border", "n_truth_border")}
    out["lists"] = {}
    tau2 = np.float64(tau) * np.float64(tau)
    for c in (range(1, K) if classes is None else classes):
        bp, bt = border(pred == c), border(truth == c)
        n_p, n_t = int(bp.sum()), int(bt.sum())
        out["n_pred_border"][c], out["n_truth_border"][c] = n_p, n_t
        if n_p == 0 and n_t == 0:
            continue
        if n_p == 0 or n_t == 0:
            out["nsd"][c] = 0.0
            continue
        a, b = edt2_three_pass(bt, spacing)[bp], edt2_three_pass(bp, spacing)[bt]
        both = np.concatenate([a, b])
        out["lists"][c] = (a, b)
        out["hd"][c] = np.sqrt(both.max())
        out["hd95"][c] = np.percentile(np.sqrt(both), 95)
        out["assd"][c] = (math.fsum(np.sqrt(a)) / n_p + math.fsum(np.sqrt(b)) / n_t) / 2
        out["nsd"][c] = np.float64(int((both <= tau2).sum())) / np.float64(n_p + n_t)
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _features(kind, shape, rng):
    """A u8 label map whose voxels == 1 are the features of `kind`; K = 3."""
    lab = np.zeros(shape, np.uint8)
    n = lab.size
    if kind == "rand01":
        lab[rng.random(shape) < 0.01] = 1
    elif kind == "rand30":
        r = rng.random(shape)
        lab[r < 0.30] = 1
        lab[r > 0.85] = 2
    elif kind == "corner":
        lab[-1, -1, -1] = 1
    elif kind == "tie":                                            # two features, every voxel between them has an equal-distance pair
        lab[0, 0, 0] = 1
        lab[-1, -1, -1] = 1
    elif kind == "none":
        pass
    elif kind == "all":
        lab[...] = 1
    elif kind == "foreign":                                        # labels >= K are nobody's class, and not the value asked for
        r = rng.random(shape)
        lab[r < 0.2] = 1
        lab[(r > 0.4) & (r < 0.7)] = 7
        lab[r > 0.9] = 255
    else:
        raise KeyError(kind)
    return lab


@functools.lru_cache(maxsize=None)
def _cases():
    rng = np.random.default_rng(20240)
    out = {}

    def add(shape, kind, spacing):
        out["%s_%dx%dx%d_s%d" % (kind, *shape, SPACINGS.index(spacing))] = (_features(kind, shape, rng), 3, spacing)

    for i, kind in enumerate(("rand01", "rand30", "corner", "tie", "none", "all", "foreign")):
        add((7, 9, 11), kind, SPACINGS[i % 4])
    for s in (SPACINGS[0], SPACINGS[2], SPACINGS[3]):              # (with the loop above: rand30 under every spacing)
        add((7, 9, 11), "rand30", s)
    add((7, 9, 11), "tie", SPACINGS[1])
    add((1, 1, 1), "none", SPACINGS[0])
    add((1, 1, 1), "all", SPACINGS[1])
    for shape, sp in (((1, 1, 50), SPACINGS[2]), ((50, 1, 1), SPACINGS[2]), ((1, 50, 1), SPACINGS[3])):
        for kind in ("rand01", "rand30", "corner", "tie"):
            add(shape, kind, sp)
    add((2, 300, 3), "rand01", SPACINGS[1])
    add((2, 300, 3), "rand30", SPACINGS[2])
    add((2, 300, 3), "foreign", SPACINGS[3])
    for kind, sp in (("rand01", SPACINGS[2]), ("rand30", SPACINGS[3]), ("corner", SPACINGS[1]), ("tie", SPACINGS[0]), ("none", SPACINGS[1])):
        add((33, 20, 65), kind, sp)
    add((4100, 1, 2), "rand01", SPACINGS[2])
    add((1, 4100, 2), "rand01", SPACINGS[1])
    add((2, 1, 4100), "rand01", SPACINGS[3])
    add((2, 1, 4100), "corner", SPACINGS[2])
    add((4100, 2, 1), "tie", SPACINGS[1])
    return out


def cases():
    """name -> (u8 labels [X, Y, Z], K, spacing). The features of a case are a predicate on value 1."""
    return _cases()


def small_cases():
    """The cases the all-pairs form is affordable on (under 10^4 voxels x 10^3 features)."""
    return {k: v for k, v in cases().items() if v[0].size <= 2000}


@functools.lru_cache(maxsize=None)
def reference(name, predicate):
    """edt2 of case `name` under `predicate` on value 1 (three-pass form; read-only)."""
    labels, _, spacing = cases()[name]
    r = edt2_three_pass(feature_of(labels, predicate, 1), spacing)
    r.setflags(write=False)
    return r


def _blobs(shape, K, rng, n_blobs, radius, classes=None):
    lab = np.zeros(shape, np.uint8)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)
    for b in range(n_blobs):
        c = (classes[b % len(classes)] if classes else 1 + b % (K - 1))
        centre = np.array([rng.integers(0, s) for s in shape])
        r = radius * (0.6 + 0.8 * rng.random())
        lab[((g - centre) ** 2).sum(-1) <= r * r] = c
    return lab


@functools.lru_cache(maxsize=None)
def _pairs():
    rng = np.random.default_rng(777)
    out = {}
    a = _blobs((14, 12, 10), 3, rng, 6, 3.0)
    out["identical_K3"] = (a, a.copy(), 3, SPACINGS[1], 1.0)
    out["shifted_K3"] = (a, np.roll(a, (1, 2, 0), axis=(0, 1, 2)), 3, SPACINGS[3], 1.0)
    out["shifted_K2_aniso"] = ((a == 1).astype(np.uint8), (np.roll(a, (2, 0, 1), axis=(0, 1, 2)) == 1).astype(np.uint8), 2, SPACINGS[2], 2.0)
    # K = 16: class 3 missing in the prediction, class 5 missing in the truth, class 9 (and most others) missing in both, 15 present
    p = _blobs((16, 15, 13), 16, rng, 10, 3.0, classes=(1, 2, 5, 15, 4))
    t = _blobs((16, 15, 13), 16, rng, 10, 3.0, classes=(1, 2, 3, 15, 4))
    p[p == 3] = 0
    t[t == 5] = 0
    p[0, 0, 0] = 200                                               # a foreign label
    out["missing_K16"] = (p, t, 16, SPACINGS[1], 1.5)
    # a class that touches the volume's edge: the edge voxels are border voxels
    p = np.zeros((9, 10, 11), np.uint8)
    t = np.zeros((9, 10, 11), np.uint8)
    p[:5, :, 3:] = 1
    t[:4, 1:, 2:] = 1
    p[6:, 6:, 6:] = 2
    t[7:, 5:, 6:] = 2
    out["edge_K3"] = (p, t, 3, SPACINGS[0], 1.0)
    out["empty_both_K3"] = (np.zeros((5, 4, 3), np.uint8), np.zeros((5, 4, 3), np.uint8), 3, SPACINGS[0], 1.0)
    one = np.zeros((1, 1, 1), np.uint8)
    out["single_voxel_K2"] = (one + 1, one + 1, 2, SPACINGS[3], 1.0)
    a = _blobs((33, 20, 65), 4, rng, 9, 7.0)
    b = _blobs((33, 20, 65), 4, rng, 9, 7.0)
    out["blobs_33x20x65_K4"] = (a, b, 4, SPACINGS[3], 3.3)
    r1, r2 = rng.random((2, 1, 4100)), rng.random((2, 1, 4100))
    out["line_2x1x4100_K3"] = ((r1 < 0.3).astype(np.uint8) + (r1 > 0.9) * np.uint8(2), (r2 < 0.3).astype(np.uint8) + (r2 > 0.8) * np.uint8(2),
                               3, SPACINGS[1], 2.5)
    r1, r2 = rng.random((4100, 2, 1)), rng.random((4100, 2, 1))
    out["line_4100x2x1_K2"] = ((r1 < 0.02).astype(np.uint8), (r2 < 0.02).astype(np.uint8), 2, SPACINGS[2], 1.0)
    return {k: (np.ascontiguousarray(v[0], np.uint8), np.ascontiguousarray(v[1], np.uint8)) + v[2:] for k, v in out.items()}


def pairs():
    """name -> (pred u8, truth u8, K, spacing, tolerance)."""
    return _pairs()


@functools.lru_cache(maxsize=None)
def reference_border(name):
    """edt2 to the border of class 1 of the prediction of pair `name` (read-only)."""
    pred, _, _, spacing, _ = pairs()[name]
    r = edt2_three_pass(border(pred == 1), spacing)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference_table(name):
    pred, truth, K, spacing, tau = pairs()[name]
    return surface_table(pred, truth, K, spacing, tau)
