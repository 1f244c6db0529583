"""
TEST INFRASTRUCTURE ONLY. Plain NumPy restatement of what csrc/components.hip computes (no reference counterpart: the reference
post-processes nothing; the host route this replaces is scipy.ndimage.label once per class, and tests/test_components_host.py
holds this restatement to exactly that).

  component_roots   labels one class at a time: two voxels are connected when they are neighbours under the structure
                    (6 / 18 / 26 = scipy.ndimage.generate_binary_structure(3, 1 / 2 / 3)) and carry the same label c,
                    1 <= c < n_classes. A component is NAMED by the linear C-order index of its first voxel. -1 elsewhere.
  keep_largest      per filtered class the largest component stays (a tie: the smallest first index), the class's other voxels
                    become 0; the [n_classes, 3] table: components found, voxels kept, voxels removed (removed = 0 for a class
                    that is not filtered; row 0 is zero).

Method: the edge list of each class (shifted slices), then rounds of "hook the larger root under the smaller" (np.minimum.at)
and pointer jumping until every edge joins one root; a root is the minimum of its tree throughout, so the final root is the
component's first index.

cases() is the case list of the issue, shared by the host and the GPU tests; reference results are cached per (case, connectivity).
"""
import numpy as np

CONNECTIVITIES = (6, 18, 26)


def backward_offsets(connectivity):
    """The neighbours of the structure with a smaller linear index: (dx, dy, dz) lexicographically below (0, 0, 0)."""
    level = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) < (0, 0, 0) and abs(dx) + abs(dy) + abs(dz) <= level:
                    out.append((dx, dy, dz))
    return out


def _pair(d, n):
    """Slices (a, b) along an axis of length n with b = a + d, both inside."""
    return slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d))


def component_roots(labels, n_classes, connectivity):
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    shape, n = labels.shape, labels.size
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    roots = np.full(shape, -1, dtype=np.int32)
    for c in range(1, int(n_classes)):
        m = labels == c
        if not m.any():
            continue
        us, vs = [], []
        for off in backward_offsets(connectivity):
            sl = [_pair(d, s) for d, s in zip(off, shape)]
            a, b = tuple(s[0] for s in sl), tuple(s[1] for s in sl)
            both = m[a] & m[b]
            us.append(idx[a][both])
            vs.append(idx[b][both])
        u, v = np.concatenate(us), np.concatenate(vs)
        parent = np.arange(n, dtype=np.int64)
        while True:
            pu, pv = parent[u], parent[v]
            ne = pu != pv
            if not ne.any():
                break
            u, v, pu, pv = u[ne], v[ne], pu[ne], pv[ne]
            np.minimum.at(parent, np.maximum(pu, pv), np.minimum(pu, pv))
            while True:                                          # pointer jumping: every tree becomes a star again
                pp = parent[parent]
                if np.array_equal(pp, parent):
                    break
                parent = pp
        roots[m] = parent.reshape(shape)[m]
    return roots


def keep_largest(labels, n_classes, connectivity, classes=None, roots=None):
    """-> (filtered label map u8, table i64 [n_classes, 3])."""
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    if roots is None:
        roots = component_roots(labels, n_classes, connectivity)
    classes = set(range(1, int(n_classes))) if classes is None else {int(c) for c in classes}
    out = labels.copy()
    table = np.zeros((int(n_classes), 3), dtype=np.int64)
    for c in range(1, int(n_classes)):
        m = labels == c
        if not m.any():
            continue
        names, counts = np.unique(roots[m], return_counts=True)          # names ascending = raster order of the first voxels
        total = int(m.sum())
        table[c, 0] = len(names)
        if c in classes:
            win = names[np.argmax(counts)]                                 # first maximum: the smallest first index among the largest
            out[m & (roots != win)] = 0
            table[c, 1], table[c, 2] = int(counts.max()), total - int(counts.max())
        else:
            table[c, 1] = total
    return out, table


# ---- the case list ----------------------------------------------------------------------------------------------------------------
def _random(shape, density, n_fg, seed):
    rng = np.random.default_rng(seed)
    fg = rng.random(shape) < density
    return np.where(fg, rng.integers(1, n_fg + 1, size=shape), 0).astype(np.uint8)


def serpentine(n=24, dense=False):
    """A one-voxel-wide path of class 1 in an n^3 volume. Every row it visits is filled along z; consecutive rows (two apart in y)
    are joined by one voxel at alternating ends, consecutive slices by one voxel. dense=False: the even slices x, rows y even --
    a simple path under every structure (rows and slices two apart never touch). dense=True: EVERY slice, rows y = x (mod 2), so
    that every row of every slice is visited or bridged (half of all voxels); neighbouring slices then meet at the joining voxels."""
    v = np.zeros((n, n, n), np.uint8)
    end = n - 1                                                      # the z end at which the next joining voxel sits
    xs = range(n) if dense else range(0, n, 2)
    for x in xs:
        ys = list(range(x % 2 if dense else 0, n, 2))
        if (x // (1 if dense else 2)) % 2:
            ys = ys[::-1]                                            # odd visits walk the slice backwards: the path goes on where it stopped
        for k, y in enumerate(ys):
            v[x, y, :] = 1
            if k + 1 < len(ys):
                v[x, (y + ys[k + 1]) // 2, end] = 1
                end = 0 if end else n - 1
        if not dense and x + 2 < n:
            v[x + 1, ys[-1], end] = 1                                # the voxel between two slices, at the end where the walk stopped
            end = 0 if end else n - 1                                # (the next slice's first row is walked from there to its other end)
    return v


def _blobs(shape, n_fg, seed):
    """Thresholded smoothed noise: one field decides foreground, a second one the class."""
    rng = np.random.default_rng(seed)

    def smooth(a):
        for _ in range(3):
            for ax in range(3):
                a = (a + np.roll(a, 1, ax) + np.roll(a, -1, ax)) / 3.0
        return a
    s1, s2 = smooth(rng.standard_normal(shape)), smooth(rng.standard_normal(shape))
    fg = s1 > np.quantile(s1, 0.55)
    cls = 1 + np.digitize(s2, np.quantile(s2, np.linspace(0, 1, n_fg + 1)[1:-1]))
    return np.where(fg, cls, 0).astype(np.uint8)


_cases = None


def cases():
    """{name: (labels u8 [X, Y, Z], n_classes)} -- built once."""
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    for k, dens in enumerate((0.15, 0.35, 0.6)):                             # 1: odd dims, every tile edge and vector tail
        c["random_%g" % dens] = (_random((37, 19, 23), dens, 3, 100 + k), 4)
    for k, shape in enumerate(((1, 1, 50), (1, 40, 1), (33, 1, 1))):         # 2: degenerate dims
        c["line_%dx%dx%d" % shape] = (_random(shape, 0.7, 2, 200 + k), 3)
    path = serpentine(24)                                                    # 3: long parent chains
    c["serpentine"] = (path, 2)
    gap = path.copy()
    gap[0, 0, 23] = 0                                                        # a corner of the path: its two neighbours are diagonal
    c["serpentine_gap"] = (gap, 2)
    c["serpentine_dense"] = (serpentine(24, dense=True), 2)
    g = np.indices((16, 16, 16)).sum(0)
    c["checkerboard"] = ((g % 2 == 0).astype(np.uint8), 2)                   # 4
    g = np.indices((16, 12, 10)).sum(0)
    c["interleaved"] = ((1 + g % 2).astype(np.uint8), 3)                     # 5: every voxel of class 1 touches class 2 only
    tie = np.zeros((12, 9, 11), np.uint8)                                    # 6: two components of one class, equal size
    tie[1:4, 2:5, 1:4] = 1
    tie[7:10, 3:6, 6:9] = 1
    tie[5, 0, 0] = 1                                                         # (and a smaller third one)
    tie[6, 7, 2:6] = 2
    tie[2, 8, 5:9] = 2
    c["tie"] = (tie, 3)
    c["tie_mirrored"] = (np.ascontiguousarray(tie[::-1, ::-1, ::-1]), 3)
    c["all_background"] = (np.zeros((9, 10, 11), np.uint8), 4)               # 7
    absent = _random((20, 17, 13), 0.5, 3, 300)
    absent[absent == 2] = 0
    c["class_absent"] = (absent, 4)
    foreign = _random((20, 17, 13), 0.5, 3, 301)
    foreign[4:9, 3:8, 2:7] = 7                                               # a label >= n_classes: joins nothing, never rewritten
    foreign[15, 1::2, 3] = 7
    c["foreign_label"] = (foreign, 4)
    c["solid_64"] = (np.ones((64, 64, 64), np.uint8), 2)
    c["blobs"] = (_blobs((96, 80, 72), 5, 400), 6)                           # 8: the realistic case, many tiles
    _cases = c
    return c


_ref = {}


def reference(name, connectivity):
    """(roots, filtered map, table) of a case with every foreground class filtered -- computed once, never modified."""
    key = (name, connectivity)
    if key not in _ref:
        labels, K = cases()[name]
        roots = component_roots(labels, K, connectivity)
        out, table = keep_largest(labels, K, connectivity, roots=roots)
        for a in (roots, out, table):
            a.setflags(write=False)
        _ref[key] = (roots, out, table)
    return _ref[key]
