"""
TEST INFRASTRUCTURE ONLY. Plain NumPy restatement of the three label-map clean-up operations of postprocess.py (kernels in
csrc/components.hip and csrc/surface.hip; no reference counterpart: the reference post-processes nothing), and the case list the
host and the GPU tests share. tests/test_cleanup_host.py holds this restatement to scipy and to surface_ref.edt2_brute.

  remove_small   per class of `classes`, every connected component (components_ref.component_roots) with fewer than min_voxels
                 voxels becomes 0. Table [n_classes, 3]: components found, voxels kept, voxels removed (row 0 zero; removed = 0
                 for a class that is not asked for).
  fill_holes     background = {label == 0}. A cavity is a connected component of the background (under `connectivity`) without a
                 voxel of index 0 or dim - 1 on any axis. Every cavity is filled whole with the winner of a face vote: the pairs
                 (p in the cavity, q a 6-neighbour of p inside the volume) with 1 <= label(q) < n_classes, counted per class; the
                 largest count wins, a tie goes to the smallest class. No vote, or a winner outside `classes`: left as it is.
                 Table [n_classes, 2]: cavities and voxels given to class c; row 0: cavities and voxels left unfilled.
  morph_ball     opening / closing by a Euclidean ball as two thresholds of the exact squared EDT (surface_ref.edt2_three_pass),
                 r2 = fl(radius * radius): dilate(M) = {d2(., M) <= r2}, erode(M) = {d2(., not M) > r2}. Classes ascending, each on
                 the map the earlier ones left; closing class c writes c on voxels that are 0 only, opening writes 0 on voxels of
                 class c only. Table [n_classes, 2]: voxels added, voxels removed.

Labels >= n_classes are never rewritten, are no background, belong to no class and cast no vote.
"""
import functools

import numpy as np

import components_ref as CR
import surface_ref as SR

OPEN, CLOSE = 0, 1
CONNECTIVITIES = CR.CONNECTIVITIES
MIN_VOXELS = (1, 5, 6)                                   # the thresholds every case is filtered with (5 = N of "sizes")
ANISO = (0.5, 1.0, 2.5)
# (spacing, radius): r2 = 1 is attained (one voxel step) and 2.25 lies between the attained 2 and 3 under unit spacing; under ANISO
# 2.25 = fl(0.25 * 9) and 6.25 = fl(6.25 * 1) are attained exactly, 1.44.. = fl(1.2 * 1.2) lies between 1.25 and 2
BALLS = (((1.0, 1.0, 1.0), 1.0), ((1.0, 1.0, 1.0), 1.5), (ANISO, 1.5), (ANISO, 2.5), (ANISO, 1.2))


def _classes(n_classes, classes):
    return list(range(1, int(n_classes))) if classes is None else sorted({int(c) for c in classes})


def remove_small(labels, n_classes, min_voxels, connectivity=26, classes=None, roots=None):
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    if roots is None:
        roots = CR.component_roots(labels, n_classes, connectivity)
    out = labels.copy()
    table = np.zeros((int(n_classes), 3), dtype=np.int64)
    asked = _classes(n_classes, classes)
    for c in range(1, int(n_classes)):
        m = labels == c
        if not m.any():
            continue
        names, counts = np.unique(roots[m], return_counts=True)
        table[c, 0] = len(names)
        if c in asked:
            small = names[counts < int(min_voxels)]
            drop = m & np.isin(roots, small)
            out[drop] = 0
            table[c, 1], table[c, 2] = int(m.sum()) - int(drop.sum()), int(drop.sum())
        else:
            table[c, 1] = int(m.sum())
    return out, table


def _shifted(shape, axis, step):
    """Index tuples (p, q) over the volume with q = p + step along `axis`, both inside."""
    a, b = [slice(None)] * 3, [slice(None)] * 3
    a[axis], b[axis] = CR._pair(step, shape[axis])
    return tuple(a), tuple(b)


def cavities(labels, connectivity):
    """(roots of the background components i32 [X, Y, Z] (-1 off the background), sorted names of the cavities)."""
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    bg = labels == 0
    roots = CR.component_roots(bg.astype(np.uint8), 2, connectivity)
    face = np.zeros(labels.shape, dtype=bool)
    for ax in range(3):
        sl = [slice(None)] * 3
        for k in (0, labels.shape[ax] - 1):
            sl[ax] = k
            face[tuple(sl)] = True
    open_names = np.unique(roots[bg & face])
    names = np.setdiff1d(np.unique(roots[bg]), open_names)
    return roots, names


def cavity_votes(labels, n_classes, roots, names):
    """i64 [len(names), n_classes]: the face pairs (p in cavity k, q a 6-neighbour with 1 <= label(q) < n_classes) per class."""
    votes = np.zeros((len(names), int(n_classes)), dtype=np.int64)
    if len(names) == 0:
        return votes
    in_cav = np.isin(roots, names)
    slot = np.searchsorted(names, np.where(in_cav, roots, names[0]))
    for ax in range(3):
        for step in (-1, 1):
            p, q = _shifted(labels.shape, ax, step)
            lq = labels[q].astype(np.int64)
            ok = in_cav[p] & (lq >= 1) & (lq < int(n_classes))
            np.add.at(votes, (slot[p][ok], lq[ok]), 1)
    return votes


def fill_holes(labels, n_classes, connectivity=6, classes=None):
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    K = int(n_classes)
    roots, names = cavities(labels, connectivity)
    votes = cavity_votes(labels, K, roots, names)
    asked = _classes(K, classes)
    out = labels.copy()
    table = np.zeros((K, 2), dtype=np.int64)
    for k, name in enumerate(names):
        size = int((roots == name).sum())
        v = votes[k, 1:] if K > 1 else votes[k, :0]
        win = 1 + int(np.argmax(v)) if v.size and v.max() > 0 else 0          # first maximum: the smallest class among equals
        if win not in asked:
            win = 0
        table[win, 0] += 1
        table[win, 1] += size
        if win:
            out[roots == name] = win
    return out, table


def morph_ball(labels, n_classes, op, radius, spacing=(1.0, 1.0, 1.0), classes=None, edt2=SR.edt2_three_pass):
    out = np.ascontiguousarray(labels, dtype=np.uint8).copy()
    K = int(n_classes)
    r2 = np.float64(radius) * np.float64(radius)
    table = np.zeros((K, 2), dtype=np.int64)
    for c in _classes(K, classes):
        m = out == c
        if op == CLOSE:
            dil = edt2(m, spacing) <= r2
            res = edt2(~dil, spacing) > r2
            add = res & (out == 0)
            out[add] = c
            table[c, 0] = int(add.sum())
        else:
            ero = edt2(~m, spacing) > r2
            res = edt2(ero, spacing) <= r2
            drop = m & ~res
            out[drop] = 0
            table[c, 1] = int(drop.sum())
    return out, table


def close_ball(labels, n_classes, radius, spacing=(1.0, 1.0, 1.0), classes=None):
    return morph_ball(labels, n_classes, CLOSE, radius, spacing, classes)


def open_ball(labels, n_classes, radius, spacing=(1.0, 1.0, 1.0), classes=None):
    return morph_ball(labels, n_classes, OPEN, radius, spacing, classes)


# ---- the case list ----------------------------------------------------------------------------------------------------------------
def _shell(v, lo, hi, c):
    """The one-voxel-thick faces of the box [lo, hi) set to c; the inside is left as it is."""
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    inner = tuple(slice(a + 1, b - 1) for a, b in zip(lo, hi))
    keep = v[inner].copy()
    v[box] = c
    v[inner] = keep


def _banded_blobs(shape, K, seed, band, background=0.45):
    """Thresholded smoothed noise decides foreground; the class comes in bands (band(x, y, z) -> 0 .. K - 2), so that cavities and
    gaps are bordered by several classes. One- and two-voxel holes are punched into the foreground, and crumbs strewn outside."""
    rng = np.random.default_rng(seed)

    def smooth(a):
        for _ in range(2):
            for ax in range(3):
                a = (a + np.roll(a, 1, ax) + np.roll(a, -1, ax)) / 3.0
        return a
    s = smooth(rng.standard_normal(shape))
    fg = s > np.quantile(s, background)
    x, y, z = np.indices(shape)
    v = np.where(fg, 1 + band(x, y, z) % (K - 1), 0).astype(np.uint8)
    r = rng.random(shape)
    v[fg & (r < 0.04)] = 0                                                   # one-voxel holes
    two = fg & (r > 0.97)
    v[two] = 0
    v[1:][two[:-1] & fg[1:]] = 0                                             # ... and pairs along x (across the bands)
    v[~fg & (rng.random(shape) < 0.03)] = 1 + int(rng.integers(0, K - 1))    # crumbs: small components
    return v


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (labels u8 [X, Y, Z], n_classes)} -- built once."""
    c = {}
    v = np.zeros((7, 5, 3), np.uint8)                                        # a one-voxel cavity
    v[2:5, 1:4, 0:3] = 1
    v[3, 2, 1] = 0
    c["cavity_one_voxel"] = (v, 2)
    v = np.zeros((13, 11, 9), np.uint8)                                      # a multi-voxel cavity in a one-class shell
    _shell(v, (2, 2, 1), (10, 9, 8), 1)
    v[11, 1:4, 2] = 2
    c["cavity_multi"] = (v, 3)
    v = np.zeros((13, 11, 9), np.uint8)                                      # two nested shells of different classes
    _shell(v, (1, 1, 1), (12, 10, 8), 1)
    _shell(v, (4, 4, 3), (9, 7, 6), 2)
    c["nested_shells"] = (v, 3)
    v = np.zeros((7, 5, 3), np.uint8)                                        # a tie: 3 faces of class 2 (first in raster order), 3 of class 1
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) != (0, 0, 0):
                    v[3 + dx, 2 + dy, 1 + dz] = 2 if dx + dy + dz < 0 else 1
    c["vote_tie"] = (v, 3)
    v = np.zeros((13, 11, 9), np.uint8)                                      # a cavity bounded partly / only by a foreign label
    _shell(v, (1, 2, 1), (6, 8, 7), 1)
    v[1, 3:6, 2:5] = 9
    v[3, 2, 3] = 200
    _shell(v, (7, 3, 2), (12, 8, 7), 9)
    c["foreign_bounds"] = (v, 3)
    v = np.zeros((13, 11, 9), np.uint8)                                      # reaches the face through an edge / a corner contact only
    v[0:5, 0:5, 0:5] = 1
    v[1, 1, 3] = v[0, 0, 3] = 0                                              # edge contact: a cavity at 6, open at 18 and 26
    v[1, 3, 1] = v[0, 2, 0] = 0                                              # corner contact: a cavity at 6 and 18, open at 26
    v[8:11, 6:9, 4:7] = 2
    v[9, 7, 5] = 0
    c["edge_corner_contact"] = (v, 3)
    v = np.ones((13, 11, 9), np.uint8)                                       # background touching each of the six faces, and one cavity
    for p in ((0, 5, 4), (12, 5, 4), (6, 0, 4), (6, 10, 4), (6, 5, 0), (6, 5, 8), (6, 5, 4)):
        v[p] = 0
    c["six_faces"] = (v, 2)
    v = np.zeros((13, 11, 9), np.uint8)                                      # components of 4, 5, 6 voxels; two of equal size
    v[1, 1, 1:5] = 1
    v[3, 1, 1:6] = 1
    v[5, 1, 1:7] = 1
    v[8, 3, 2:7] = 2
    v[10, 7, 2:7] = 2
    v[12, 10, 8] = 2
    c["sizes"] = (v, 3)
    v = np.zeros((13, 11, 9), np.uint8)                                      # an object on the volume face: a spur to open, a slit to close
    v[0:4, 3:8, 2:7] = 1
    v[4:8, 5, 4] = 1
    v[2, 3:8, 4] = 0
    v[9:13, 0:3, 0:9] = 2
    v[10, 1, 3:5] = 0
    c["touching_face"] = (v, 3)
    c["empty_1x12x10"] = (np.zeros((1, 12, 10), np.uint8), 4)
    c["all_one_12x1x10"] = (np.ones((12, 1, 10), np.uint8), 2)
    c["single_voxel"] = (np.ones((1, 1, 1), np.uint8), 2)
    rng = np.random.default_rng(50)
    r = rng.random((1, 1, 50))
    c["line_1x1x50"] = (((r < 0.5).astype(np.uint8) + (r > 0.8) * np.uint8(2)), 3)
    r = rng.random((1, 12, 10))
    c["plane_1x12x10"] = (((r < 0.6).astype(np.uint8) + (r > 0.9) * np.uint8(2)), 3)
    c["blobs_K4"] = (_banded_blobs((33, 17, 65), 4, 60, lambda x, y, z: x // 2), 4)
    c["blobs_K16"] = (_banded_blobs((17, 16, 15), 16, 61, lambda x, y, z: x, background=0.2), 16)
    return {k: (np.ascontiguousarray(a, np.uint8), K) for k, (a, K) in c.items()}


RANDOM_CASES = ("blobs_K4", "blobs_K16")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference_small(name, connectivity, min_voxels):
    labels, K = cases()[name]
    return _frozen(*remove_small(labels, K, min_voxels, connectivity, roots=_roots(name, connectivity)))


@functools.lru_cache(maxsize=None)
def _roots(name, connectivity):
    labels, K = cases()[name]
    return CR.component_roots(labels, K, connectivity)


@functools.lru_cache(maxsize=None)
def reference_fill(name, connectivity):
    labels, K = cases()[name]
    return _frozen(*fill_holes(labels, K, connectivity))


@functools.lru_cache(maxsize=None)
def reference_ball(name, op, ball):
    labels, K = cases()[name]
    spacing, radius = BALLS[ball]
    return _frozen(*morph_ball(labels, K, op, radius, spacing))
