"""
Callers on either side of the hot path: volume files, random
views, and the train-time plane sampler that feeds UNet.train_step. Volumes live on the GPU and
every plane is cut by the HIP sampling kernel; only the few random numbers per slice are host work.

Reference behaviour restated here:
  training batch sampler .... mpunet/sequences/isotrophic_live_view_sequence_2d.py:119-216
  fg balancing .............. mpunet/sequences/isotrophic_live_view_sequence.py:98-128
  random views .............. mpunet/interpolation/sample_grid.py:133-173
  views.npz / dim / span .... mpunet/preprocessing/data_preparation_funcs.py:116-154, mpunet/image/auditor.py:108-112,199-209
Volume files: NIfTI-1 (.nii / .nii.gz, read natively -- nifti.py) as in a reference project folder, or .npz files with
keys `image` [X,Y,Z(,C)], optional `labels` [X,Y,Z], optional `affine` [4,4].
"""
import os
import numpy as np
import torch

from .interpolation import Volume, ViewGeometry, sample_view


def load_volume_file(path):
    if path.endswith((".nii", ".nii.gz")):
        from .formats import load_nifti
        img, aff = load_nifti(path)
        return img, None, aff
    with np.load(path) as z:
        d = {k: z[k] for k in z.files}
    img = d.get("image", d.get("arr_0"))
    if img is None:
        raise ValueError("%s: no 'image' array" % path)
    if img.ndim == 3:
        img = img[..., None]
    return img.astype(np.float32), d.get("labels"), d.get("affine", np.eye(4))


def load_label_file(path):
    """Label volume [X,Y,Z] u8 of a NIfTI or .npz file (key `labels`, else the first array)."""
    if path.endswith((".nii", ".nii.gz")):
        from .formats import load_nifti_labels
        return load_nifti_labels(path)
    with np.load(path) as z:
        return z["labels"] if "labels" in z.files else z[z.files[0]]


def _is_nifti(path):
    return str(path).endswith((".nii", ".nii.gz"))


class HostPayload:
    """One volume as a loader thread leaves it: FILE WORK ONLY (read, gunzip, header parse), pageable host memory, no call into
    HIP or torch's device API (volume_queue.py: the threading rule). `image` is ("raw", header, payload bytes) for a NIfTI file
    of rank 3 or 4 -- decoded on the device by adopt_payload -- or ("host", f32 [X,Y,Z,C]) for everything that keeps the host
    path (.npz, other ranks); `labels` is None or one of the same two forms."""
    __slots__ = ("path", "label_path", "image", "labels", "affine")

    def __init__(self, path, label_path, image, labels, affine):
        self.path, self.label_path, self.image, self.labels, self.affine = path, label_path, image, labels, affine


def read_volume_host(path, label_path=None, raw_nifti=True, label_wins=False):
    """HostPayload of an image file and, unless the image file carries labels itself (.npz; label_wins: even then), of `label_path`.
    raw_nifti=False decodes NIfTI files on the host too (formats.load_nifti / load_nifti_labels: today's path)."""
    from .nifti import read_nifti_payload
    image = labels = affine = None
    if raw_nifti and _is_nifti(path):
        h, affine, buf = read_nifti_payload(path)
        if len(h["shape"]) in (3, 4):
            image = ("raw", h, buf)
    if image is None:                                         # .npz, a NIfTI file of another rank (today's errors), the host path
        img, lab, affine = load_volume_file(path)
        image = ("host", img)
        labels = None if lab is None else ("host", lab)
    if label_path and (labels is None or label_wins):
        labels = read_labels_host(label_path, raw_nifti)
    return HostPayload(path, label_path, image, labels, affine)


def read_labels_host(label_path, raw_nifti=True):
    """The `labels` member of a HostPayload for a label file."""
    from .nifti import read_nifti_payload
    if raw_nifti and _is_nifti(label_path):
        h, _, buf = read_nifti_payload(label_path)
        s = h["shape"]
        if len(s) == 3 or (len(s) == 4 and s[3] == 1):        # (load_nifti_labels drops a trailing singleton axis)
            return ("raw", h, buf)
    return ("host", load_label_file(label_path))


def decode_nifti_payload(header, payload, device, labels=False, path="", out=None, bad=None):
    """One host-to-device copy of the payload bytes and mpu_volume_decode (csrc/volume_decode.hip) on the current stream:
    f32 [X,Y,Z,C] with the bits of formats.load_nifti, or (labels=True) u8 [X,Y,Z] with the bits of formats.load_nifti_labels.
    A label value NumPy's astype(uint8) is platform-defined for (non-finite, or outside [0, 256) after truncation) is a
    ValueError naming the file. out / bad (labels: the int64 [1] counter of such values): caller-owned device tensors
    (default: allocated here)."""
    import ctypes as C
    import sys
    from . import _lib
    from .nifti import scaling_of
    shape = tuple(int(s) for s in header["shape"])
    if len(shape) not in (3, 4) or (labels and len(shape) == 4 and shape[3] != 1):
        raise ValueError("%s: the device decode takes NIfTI data of rank 3 or 4 (labels: one channel), got shape %r" % (path, shape))
    shape4 = shape + (1,) * (4 - len(shape))
    swap = (header["endian"] == ">") == (sys.byteorder == "little")
    scaled, slope, inter = scaling_of(header)
    dev = torch.device(device)
    raw = torch.frombuffer(payload, dtype=torch.uint8).to(dev)
    if labels:
        out = _lib.owned(out, shape4[:3], torch.uint8, dev, "out")
        bad = _lib.owned(bad, 1, torch.int64, dev, "bad")
    else:
        out = _lib.owned(out, shape4, torch.float32, dev, "out")
        bad = None
    _lib.call("mpu_volume_decode", _lib.ptr(raw), int(header["datatype"]), int(swap), (C.c_int64 * 4)(*shape4), int(scaled),
              float(slope), float(inter), _lib.MPU_DECODE_LABELS if labels else _lib.MPU_DECODE_IMAGE, _lib.ptr(out),
              _lib.ptr(bad), _lib.stream_ptr())
    if labels:
        n_bad = int(bad.item())
        if n_bad:
            raise ValueError("%s: %d label voxels are non-finite or outside [0, 256) after truncation: they cannot be stored "
                             "as uint8 class indices" % (path, n_bad))
    return out


_ENCODE_SOURCES = {torch.float32: ("MPU_ENCODE_F32", 16, "f4"), torch.uint8: ("MPU_ENCODE_U8", 2, "u1"),
                   torch.int32: ("MPU_ENCODE_I32", 2, "u1"), torch.int64: ("MPU_ENCODE_I64", 2, "u1")}


def encode_nifti_payload(t, path="", out=None, bad=None, check=True):
    """mpu_volume_encode (csrc/volume_encode.hip) on the current stream: a resident tensor of up to four axes [X,Y,Z,C] in C order
    -> (payload, bad): the bytes np.asfortranarray(t).tobytes(order="F") has for an f32 tensor (NIfTI datatype 16), or for a u8 /
    i32 / i64 label map stored as u8 (datatype 2), as a flat device tensor of that type, and the int64 [1] counter of the class
    indices outside [0, 256) (None for f32). check: wait for the counter and raise ValueError naming `path` when it is not zero
    (check=False: the caller does, after its own copy -- encoded_payload_to_host). out / bad: caller-owned device tensors."""
    import ctypes as C
    from . import _lib
    if t.dtype not in _ENCODE_SOURCES:
        raise ValueError("%s: no device encode for a %s tensor (f32 images; u8, i32, i64 label maps)" % (path, t.dtype))
    if not 1 <= t.ndim <= 4 or not t.is_contiguous():
        raise ValueError("%s: the device encode takes a contiguous tensor of 1 to 4 axes, got shape %r" % (path, tuple(t.shape)))
    source, _, _ = _ENCODE_SOURCES[t.dtype]
    image = t.dtype == torch.float32
    shape4 = tuple(int(s) for s in t.shape) + (1,) * (4 - t.ndim)
    out = _lib.owned(out, t.numel(), torch.float32 if image else torch.uint8, t.device, "out")
    bad = None if image else _lib.owned(bad, 1, torch.int64, t.device, "bad")
    _lib.call("mpu_volume_encode", _lib.ptr(t), getattr(_lib, source), (C.c_int64 * 4)(*shape4), 16 if image else 2,
              _lib.ptr(out), _lib.ptr(bad), _lib.stream_ptr())
    if check and bad is not None:
        check_encoded_labels(bad, path)
    return out, bad


def check_encoded_labels(bad, path):
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError("%s: %d label voxels are outside [0, 256): they cannot be stored as uint8 class indices" % (path, n_bad))


def encoded_payload_to_host(t, path=""):
    """What `mp predict` hands its writer thread for a NIfTI output: (shape, NumPy dtype string, payload) with the payload bytes
    of `t` (encode_nifti_payload) in a pinned host buffer, as a flat NumPy array. Encode, ONE device-to-host copy and the wait
    for it happen here, on the calling thread's current stream; nothing of the result touches the device again."""
    out, bad = encode_nifti_payload(t, path, check=False)
    host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
    host.copy_(out, non_blocking=True)
    n_bad = None if bad is None else bad.to("cpu", non_blocking=False)
    torch.cuda.current_stream(t.device).synchronize()
    if n_bad is not None:
        check_encoded_labels(n_bad, path)
    return tuple(int(s) for s in t.shape), _ENCODE_SOURCES[t.dtype][2], host.numpy()


def adopt_payload(payload, device, bg_value="1pct", scaler="RobustScaler", identifier=None, fit_on="device"):
    """HostPayload -> Volume, on the CALLING thread's current stream: upload, decode, then as_volume's background value and
    scaler fit on the resident tensor."""
    kind = payload.image[0]
    img = decode_nifti_payload(payload.image[1], payload.image[2], device, False, payload.path) if kind == "raw" \
        else payload.image[1]
    lab = payload.labels
    if lab is not None:
        lab = decode_nifti_payload(lab[1], lab[2], device, True, payload.label_path) if lab[0] == "raw" else lab[1]
    if identifier is None:
        from .nifti import volume_identifier
        identifier = volume_identifier(payload.path)
    vol = as_volume(img, lab, payload.affine, bg_value, scaler, device, identifier, fit_on=fit_on)
    vol.source_path = payload.path                    # (`mp predict` writes <id>_PRED.nii.gz for NIfTI inputs)
    return vol


def load_volume_to_device(path, label_path=None, device="cuda", bg_value="1pct", scaler="RobustScaler", identifier=None,
                          fit_on="device", label_wins=False):
    """File(s) -> resident Volume. A NIfTI file of rank 3 or 4 goes up as it lies in the file and is put into C order and f32
    (labels: u8) by mpu_volume_decode -- the same bits as the host conversion, without its two NumPy passes. .npz files, NIfTI
    files of another rank, a CPU `device` and fit_on="host" keep the host path and its errors."""
    on_device = torch.device(device).type == "cuda" and fit_on == "device"
    return adopt_payload(read_volume_host(path, label_path, on_device, label_wins), device, bg_value, scaler, identifier, fit_on)


def list_volume_files(base_dir, img_subdir="images"):
    d = os.path.join(base_dir, img_subdir)
    if not os.path.isdir(d):
        return []
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith((".npz", ".nii", ".nii.gz")))


def make_toy_volume(size=64, seed=0):
    """A 3-class synthetic volume (background, ellipsoid, box) in the spirit of `mp toy_data`."""
    rng = np.random.RandomState(seed)
    g = np.mgrid[:size, :size, :size].astype(np.float32)
    c1 = size * (0.35 + 0.3 * rng.rand(3)); r1 = size * (0.12 + 0.1 * rng.rand(3))
    ell = (((g[0] - c1[0]) / r1[0]) ** 2 + ((g[1] - c1[1]) / r1[1]) ** 2 + ((g[2] - c1[2]) / r1[2]) ** 2) <= 1
    c2 = size * (0.3 + 0.4 * rng.rand(3)); h2 = size * (0.08 + 0.08 * rng.rand(3))
    box = (abs(g[0] - c2[0]) < h2[0]) & (abs(g[1] - c2[1]) < h2[1]) & (abs(g[2] - c2[2]) < h2[2])
    lab = np.zeros((size,) * 3, np.uint8)
    lab[ell] = 1
    lab[box] = 2
    img = 0.3 * np.sin(g[0] / size * 3) + 0.2 * np.cos(g[1] / size * 5) + 0.05 * rng.randn(size, size, size)
    img = img + 0.8 * (lab == 1) + 1.5 * (lab == 2)
    return img[..., None].astype(np.float32), lab, np.eye(4)


def as_volume(image, labels, affine, bg_value="1pct", scaler="RobustScaler", device="cuda", identifier="volume",
              fit_on="device"):
    """The preparation the reference does lazily per ImagePair (image_pair.py:300-341,469-484): the '<N>pct' background
    value and the per-channel scaler, one of the five sklearn classes of the reference's YAML. fit_on="device" (default):
    upload first, then compute both from the resident image (scalers.py, csrc/volume_stats.hip); fit_on="host": NumPy on the
    host image, then upload -- the same numbers, kept for A/B and tests. A host image of another dtype is cast to f32 first, in both modes: f32 is what the
    device holds and what the planes are cut from."""
    from . import scalers
    if fit_on not in ("device", "host"):
        raise ValueError("fit_on must be 'device' or 'host'")
    if scaler:
        scalers.check_scaler_name(scaler)
    if not torch.is_tensor(image):
        image = np.asarray(image, np.float32)                 # the volume is f32 on the device: both modes prepare from f32
    C = image.shape[-1]
    pct = None
    if isinstance(bg_value, str) and bg_value.endswith("pct"):
        pct = int(bg_value[:-3])
        bg = None
    elif isinstance(bg_value, (list, tuple, np.ndarray)):
        bg = [float(b) for b in bg_value]
    else:
        bg = [float(bg_value or 0.0)] * C
    if fit_on == "host":
        if pct is not None:
            bg = [float(np.percentile(image[..., c], pct)) for c in range(C)]
        sc = scalers.fit_scaler_host(scaler, image) if scaler else None
        return Volume(image, labels, affine, bg_value=bg, scaler=sc, device=device, identifier=identifier)
    img_dev = torch.as_tensor(image).to(device=device, dtype=torch.float32).contiguous()
    if img_dev.ndim != 4:
        raise ValueError("Input img of dim %i must be dim 4." % img_dev.ndim)
    bg_dev, sc = scalers.prepare_device(img_dev, pct, scaler or None)
    return Volume(img_dev, labels, affine, bg_value=bg if pct is None else bg_dev, scaler=sc, device=device,
                  identifier=identifier)


def _volume_tensors(vol):
    """Every device tensor a sampling call of `vol` reads."""
    ts = [vol.image, vol._bg] + list(vol._axes_dev)
    if vol.labels is not None:
        ts.append(vol.labels)
    if vol._scaler is not None:
        for _, held in vol._scaler._dev.values():
            ts += [t for t in held.values() if t is not None]
    return ts


def random_views(n, min_angle_deg=60.0, seed=None):
    """n unit vectors with z >= 0 and pairwise angles above a threshold that relaxes by 1 degree per failure."""
    rng = np.random.RandomState(seed)
    thr = float(min_angle_deg)
    while True:
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v[:, 2] = np.abs(v[:, 2])
        cosines = np.clip(v @ v.T, -1, 1)
        ang = np.rad2deg(np.arccos(cosines))[np.triu_indices(n, 1)]
        if n < 2 or np.all(ang > thr):
            return v
        thr -= 1.0


def audit_dim_and_span(volumes, min_dim=128, max_dim=512):
    """real_space_span = 75th percentile of the real-space extents; sample dim at the median resolution,
    rounded to a multiple of 16 in [min_dim, max_dim]."""
    ext, res = [], []
    for v in volumes:
        pix = np.linalg.norm(v.affine[:3, :3], axis=0)
        ext += list(np.array(v.image.shape[:3]) * pix)
        res += list(pix)
    span = float(np.percentile(ext, 75))
    dim = int(np.clip(int(np.ceil(span / np.median(res) / 16.0) * 16), min_dim, max_dim))
    return dim, span


def plane_basis_fast(view, noise=None):
    """
    [u v n] (row-major 3x3, columns u, v, n) of interpolation.plane_basis in plain Python floats: the same
    construction (normalise, add noise, normalise, |.| rule for small x/y, u = R(axis, -90 deg) n, v = n x u)
    without the reference's float32 round trips - agrees to ~1e-7, which is far below the random `noise_sd`
    the training planes carry anyway. ~10x cheaper than the NumPy version (the sampler's host cost).
    """
    import math
    n0, n1, n2 = float(view[0]), float(view[1]), float(view[2])
    r = math.sqrt(n0 * n0 + n1 * n1 + n2 * n2)
    n0, n1, n2 = n0 / r, n1 / r, n2 / r
    if noise is not None:
        n0 += float(noise[0]); n1 += float(noise[1]); n2 += float(noise[2])
        r = math.sqrt(n0 * n0 + n1 * n1 + n2 * n2)
        n0, n1, n2 = n0 / r, n1 / r, n2 / r
    if n0 < 0.2 and n1 < 0.2:
        n0, n1 = abs(n0), abs(n1)
    if abs(n0) <= 1e-8 and abs(n1) <= 1e-8:
        u = (1.0, 0.0, 0.0); v = (0.0, 1.0, 0.0)
    else:
        s0, s1, s2 = n0, n1, n2 + 1.0
        r = math.sqrt(s0 * s0 + s1 * s1 + s2 * s2)
        s0, s1, s2 = s0 / r, s1 / r, s2 / r
        a0, a1, a2 = n1 * s2 - n2 * s1, n2 * s0 - n0 * s2, n0 * s1 - n1 * s0
        r = math.sqrt(a0 * a0 + a1 * a1 + a2 * a2)
        a0, a1, a2 = a0 / r, a1 / r, a2 / r
        th = math.radians(-90.0)
        qa = math.cos(th / 2.0); sn = math.sin(th / 2.0)
        b, c, d = -a0 * sn, -a1 * sn, -a2 * sn
        aa, bb, cc, dd = qa * qa, b * b, c * c, d * d
        bc, ad, ac, ab, bd, cd = b * c, qa * d, qa * c, qa * b, b * d, c * d
        R = ((aa + bb - cc - dd, 2 * (bc + ad), 2 * (bd - ac)),
             (2 * (bc - ad), aa + cc - bb - dd, 2 * (cd + ab)),
             (2 * (bd + ac), 2 * (cd - ab), aa + dd - bb - cc))
        u = tuple(R[i][0] * n0 + R[i][1] * n1 + R[i][2] * n2 for i in range(3))
        v = (n1 * u[2] - n2 * u[1], n2 * u[0] - n0 * u[2], n0 * u[1] - n1 * u[0])
    return [u[0], v[0], n0, u[1], v[1], n1, u[2], v[2], n2]


class _VolCache:
    """Per-volume constants of the sampling call (built once): ctypes pieces and device-side background values."""

    def __init__(self, vol, dim, span):
        import ctypes as C
        from . import _lib
        self.shape = (C.c_int32 * 4)(*[int(v) for v in vol.image.shape])
        g = _lib.ViewGeom()
        for k in range(3):
            g.vol_axis[k] = _lib.make_axis(vol.axes[k])
        rot = np.eye(3) if vol.rot_mat is None else np.asarray(vol.rot_mat, np.float64)
        g.rot[:] = rot.ravel().tolist()
        g.has_rot = 0 if vol.rot_mat is None else 1
        hd = span // 2
        g.dim, g.n_planes = int(dim), 1
        g.g_start, g.g_step = float(-hd), float((hd - (-hd)) / float(dim - 1))
        self.geom = g
        bg = np.asarray(vol.bg_value, np.float32)[None, :]
        if vol._scaler is not None:                          # planes come out scaled: compare with what the kernel makes of a fill
            bg = vol._scaler.transform_host(bg)
        self.bg_scaled = torch.tensor(bg[0], dtype=torch.float32, device=vol.device).contiguous()
        self.bg_scaled_ptr = self.bg_scaled.data_ptr()
        self.ptrs = [_lib.ptr(vol.image), _lib.ptr(vol.labels), _lib.ptr(vol._axes_dev[0]), _lib.ptr(vol._axes_dev[1]),
                     _lib.ptr(vol._axes_dev[2]), _lib.ptr(vol._bg), vol._sc]


class SliceRule:
    """
    The accept / reject rule of one training batch, host ints only: `_get_valid_slice_from`
    (isotrophic_live_view_sequence_2d.py:119-161) with `validate_lab_vec`, `validate_lab` and `is_valid_im`
    (isotrophic_live_view_sequence.py:91-128), as the reference EXECUTES it (tests/golden/sampler_rule_golden.json is
    recorded from the reference class). Two pieces of state:

    * `has_fg`: accepted slices with foreground so far; lives for the batch.
    * the "classes seen" mask of ONE slot. `validate_lab_vec` returns a new array and `_get_valid_slice_from` rebinds only
      its local name, so the vector `__getitem__` passes in is all zero for every slot: the mask starts at 0 per slot,
      accumulates over that slot's tries only, and keeps the classes of a candidate that passed the vector check even when the
      fraction or the all-background check then rejects it.

    A slot's verdicts depend on earlier slots only through `has_fg` and the slot index, so slots must be judged in order,
    each to its acceptance, but a slot's candidates may have been drawn at any time.
    """

    def __init__(self, batch_size, n_classes, fg_batch_fraction=0.5, force_all_fg="auto", max_tries=10):
        self.batch_size, self.max_tries = int(batch_size), int(max_tries)
        self.fg_classes = list(range(1, int(n_classes))) or [1]
        self.fg_mask = 0
        for c in self.fg_classes:
            self.fg_mask |= 1 << c
        self.n_fg_slices = int(np.ceil(batch_size * fg_batch_fraction))
        if isinstance(force_all_fg, str) and force_all_fg.lower() == "auto":
            self.force_all_fg = self.batch_size > len(self.fg_classes)
        else:
            self.force_all_fg = bool(force_all_fg)
        self.reset()

    def reset(self):
        """A new batch."""
        self.has_fg = 0
        self._slot, self._acc = -1, 0

    def judge(self, slot, n_try, mask, nonbg):
        """Candidate number n_try (1-based) of `slot`: mask = bit l set for every label l < 32 in the plane, nonbg = the image
        plane is not all background. True: accepted (the slot is done), False: rejected (the slot needs another candidate)."""
        if slot != self._slot:
            self._slot, self._acc = slot, 0
        left = self.batch_size - slot
        present = mask & self.fg_mask
        last = n_try >= self.max_tries
        if self.force_all_fg and not last:
            new = self._acc | present
            missing = len(self.fg_classes) - bin(new).count("1")
            if not (missing == 0 or missing < left):
                return False
            self._acc = new                                   # kept even if the candidate is rejected below
        if present:
            ok, inc = True, 1
        elif (self.n_fg_slices - self.has_fg) < left:
            ok, inc = True, 0
        else:
            ok, inc = False, 0
        if (ok or last) and (last or nonbg):
            self.has_fg += inc
            return True
        return False


class TrainSampler:
    """
    Random-plane batch sampler (training half of IsotrophicLiveViewSequence2D). Every plane is cut by the HIP
    sampling kernel straight into the batch tensors; the accept / reject statistics of a candidate (classes
    present, not-all-background) come back in one 8-byte read (mpu_plane_stats), which is the only host
    synchronisation per round of candidates. SliceRule decides.
    """

    def __init__(self, volumes, views, dim, real_space_span, batch_size, n_classes, noise_sd=0.1,
                 fg_batch_fraction=0.5, force_all_fg="auto", sample_weights=None, seed=None, max_tries=10,
                 augmenters=None, n_channels=None, device=None):
        # `volumes`: a list of resident Volumes, a volume_queue.EagerQueue (its list), or a volume_queue.LimitationQueue: then
        # every slot of a batch takes its volume from the queue's FIFO (n_channels and device cannot be read off a volume that
        # is not loaded yet: pass them)
        self.queue = volumes if hasattr(volumes, "loaded_queue") else None
        self.volumes = [] if self.queue is not None else list(getattr(volumes, "volumes", volumes))
        if self.queue is not None and (n_channels is None or device is None):
            raise ValueError("TrainSampler over a limitation queue needs n_channels and device")
        if self.queue is None and self.volumes:
            n_channels, device = self.volumes[0].n_channels, self.volumes[0].device
        self.n_channels = None if n_channels is None else int(n_channels)
        self.device = None if device is None else torch.device(device)
        self.views = np.asarray(views, float)
        self.dim, self.span = int(dim), real_space_span
        self.batch_size, self.n_classes = int(batch_size), int(n_classes)
        self.noise_sd = float(noise_sd)
        self.rule = SliceRule(batch_size, n_classes, fg_batch_fraction, force_all_fg, max_tries)
        self.sample_weights = sample_weights or [1.0] * len(self.volumes)
        self.rng = np.random.RandomState(seed)
        self.augmenters = list(augmenters or [])      # applied after scaling (isotrophic_live_view_sequence_2d.py:203-208)
        self._cache = {}
        self._views_l = [tuple(float(a) for a in v) for v in self.views]

    @property
    def max_tries(self):
        return self.rule.max_tries

    def _vc(self, vol):
        """The volume's _VolCache; keyed by the VOLUME (a list index names different volumes over time under a queue)."""
        if isinstance(vol, (int, np.integer)):
            vol = self.volumes[vol]
        c = self._cache.get(vol)
        if c is None:
            c = self._cache[vol] = _VolCache(vol, self.dim, self.span)
        return c

    def _take_from_queue(self, B):
        """The batch's volumes from the limitation queue's FIFO, one get / release per slot as get_random_image does it
        (isotrophic_live_view_sequence_2d.py:150-160), BEFORE the first cut: an arrival is adopted here -- upload, decode,
        scaler fit on this thread's current stream (volume_queue.py: the threading rule). An entry that reaches its access
        limit is only marked; __call__ retires it (unload, replacement load) once the batch's cuts are issued, because a
        rejected candidate is cut again from the same volume. Should every loaded entry expire inside one batch (max_loaded far
        below the batch size), the remaining slots reuse the expired ones in turn rather than wait for loads that are not
        requested before the batch is done."""
        q, cur = self.queue, torch.cuda.current_stream()
        vols, retiring = [], []
        for slot in range(B):
            if retiring and q.loaded_queue.empty() and q.n_loading == 0:
                vols.append(retiring[slot % len(retiring)].volume)
                continue
            entry, n = q.get()
            fresh = entry.volume is None
            vol = entry.adopt()
            if fresh:
                vol._alloc_stream, vol._marked_streams = cur, set()
            elif getattr(vol, "_alloc_stream", None) != cur:                       # (adopted elsewhere, e.g. by the bias count)
                marked = vol.__dict__.setdefault("_marked_streams", set())
                if cur not in marked:
                    for t in _volume_tensors(vol) + [self._vc(vol).bg_scaled]:  # read here, allocated on another stream
                        t.record_stream(cur)
                    marked.add(cur)
            if q.release(entry, n, defer_unload=True):
                retiring.append(entry)
            vols.append(vol)
        return vols, retiring

    def _issue_cut(self, vi, X, Y, slot, off_dev, stats):
        """Enqueue one candidate plane of volume vi into X[slot], Y[slot] and its statistics into stats[slot] (class mask,
        not-all-background flag): two launches, NO host synchronisation. off_dev: f64 [>= slot + 1] scratch, stats: i32 [., 2]."""
        import ctypes as C
        from . import _lib
        vol, vc = self.volumes[vi], self._vc(vi)
        view = self._views_l[self.rng.randint(0, len(self._views_l))]
        half = self.span // 2
        off = self.rng.uniform(-half, half)
        noise = self.rng.normal(scale=self.noise_sd, size=3) if self.noise_sd else None
        g = vc.geom
        g.basis[:] = plane_basis_fast(view, noise)
        od = off_dev[slot:slot + 1]
        od.fill_(off)                                         # scalar fill: no host->device copy of a tensor
        st = _lib.stream_ptr()
        p = vc.ptrs
        xs, ys = X[slot], Y[slot]
        _lib.call("mpu_sample_view_planes_sc", p[0], p[1], vc.shape, p[2], p[3], p[4], C.byref(g), _lib.ptr(od),
                  p[5], vol.bg_class, p[6], _lib.ptr(xs), _lib.ptr(ys), st)
        _lib.call("mpu_plane_stats", _lib.ptr(ys), _lib.ptr(xs), self.dim * self.dim, vol.n_channels,
                  _lib.ptr(vc.bg_scaled), _lib.ptr(stats[slot]), st)

    def _cut(self, vi, X, Y, slot, off_dev, stats):
        """One candidate plane of volume vi into X[slot], Y[slot]; returns (class mask, not-all-bg flag) -- synchronises."""
        if stats.ndim == 1:                                   # (the one-candidate form: off_dev [1], stats [2])
            self._issue_cut(vi, X[slot:slot + 1], Y[slot:slot + 1], 0, off_dev, stats.reshape(1, 2))
            m, nb = stats.tolist()
        else:
            self._issue_cut(vi, X, Y, slot, off_dev, stats)
            m, nb = stats[slot].tolist()
        return m, bool(nb)

    def __call__(self):
        """One batch. Round 5: the candidates of ALL undecided slots are cut before the host reads their statistics -- one
        read (one stream synchronisation) per ROUND instead of one per candidate: a batch whose first candidates are all
        accepted costs a single round trip, which is what lets the sampler run on a side stream beside a train step without
        queueing behind its kernels 2 x B times (pipeline.TrainPipeline). SliceRule alone decides, slot by slot in order: the
        foreground count runs over the batch, the classes-seen mask over the tries of one slot (which is what the reference
        executes, see SliceRule). Candidates are i.i.d. draws and a slot's verdicts depend on earlier slots only through the
        foreground count and the slot index, so deciding a slot on a candidate drawn before the earlier slots were settled
        changes nothing statistically. With no rejection the random stream is consumed in the same order as the
        one-candidate-at-a-time form. Diagnostics of the last batch: `rounds`, `last_identifiers`, `last_trace`."""
        B, d = self.batch_size, self.dim
        dev = self.device
        qvols, retiring = self._take_from_queue(B) if self.queue is not None else (None, ())
        X = torch.empty((B, d, d, self.n_channels), dtype=torch.float32, device=dev)
        Y = torch.empty((B, d, d), dtype=torch.uint8, device=dev)
        off_dev = torch.empty(B, dtype=torch.float64, device=dev)
        stats = torch.empty((B, 2), dtype=torch.int32, device=dev)
        rule = self.rule
        rule.reset()
        trace = self.last_trace = [[] for _ in range(B)]      # (diagnostic: per slot the judged candidates, (mask, nonbg))
        vis = [None] * B
        tries = [0] * B
        fresh = [False] * B                                   # slot holds a candidate not yet judged
        first = 0                                             # first undecided slot
        self.rounds = 0                                       # (diagnostic: host reads of this batch)
        import ctypes as C
        from . import _lib
        lib = _lib.load()
        off_host = getattr(self, "_off_host", None)
        if off_host is None or off_host.numel() != B:            # pinned: the round's offsets go up as ONE asynchronous copy
            off_host = self._off_host = torch.empty(B, dtype=torch.float64).pin_memory()
        xp, yp, op, sp = X.data_ptr(), Y.data_ptr(), off_dev.data_ptr(), stats.data_ptr()
        xs, ys = X.stride(0) * 4, Y.stride(0)
        half = self.span // 2
        nviews = len(self._views_l)
        stp = _lib.stream_ptr()
        while first < B:
            # (re)cut what is missing. Round 6: host work first -- the draws of every missing slot in slot order (the same random
            # stream as one candidate at a time), their plane bases, the offsets into a pinned buffer -- then ONE copy of the
            # offsets and one library call per candidate (mpu_sample_plane_stats: sample + statistics): about half the host time
            # per candidate, which is what bounded the mp-train loop once the train step had reached 2.4 ms
            todo = []
            for slot in range(first, B):
                if not fresh[slot]:
                    if vis[slot] is None:                     # (a list or an eager queue: the random stream as without queues)
                        vis[slot] = qvols[slot] if qvols is not None else self.volumes[self.rng.randint(0, len(self.volumes))]
                    tries[slot] += 1
                    view = self._views_l[self.rng.randint(0, nviews)]
                    off = self.rng.uniform(-half, half)
                    noise = self.rng.normal(scale=self.noise_sd, size=3) if self.noise_sd else None
                    off_host[slot] = off
                    todo.append((slot, vis[slot], plane_basis_fast(view, noise)))
                    fresh[slot] = True
            off_dev.copy_(off_host, non_blocking=True)
            for slot, vol, basis in todo:
                vc = self._vc(vol)
                g = vc.geom
                g.basis[:] = basis
                p = vc.ptrs
                _lib.check(lib.mpu_sample_plane_stats_sc(p[0], p[1], vc.shape, p[2], p[3], p[4], C.byref(g), op + 8 * slot, p[5],
                                                         vol.bg_class, p[6], xp + slot * xs, yp + slot * ys, vc.bg_scaled_ptr,
                                                         sp + 8 * slot, stp), "mpu_sample_plane_stats_sc")
            st = stats.tolist()                               # the round's one synchronisation
            self.rounds += 1
            while first < B:                                  # judge in slot order until a candidate is rejected
                slot = first
                m, nonbg = st[slot][0] & 0xFFFFFFFF, bool(st[slot][1])   # (i32 read of a u32 mask: label 31 is the sign bit)
                fresh[slot] = False
                trace[slot].append((m, nonbg))
                if not rule.judge(slot, tries[slot], m, nonbg):
                    break                                     # this slot gets a new candidate next round
                first += 1
        if qvols is None:
            index_of = {v: i for i, v in enumerate(self.volumes)}
            ws = [self.sample_weights[index_of[v]] for v in vis]
        else:
            ws = [1.0] * B
        bgs = [list(v.bg_value) for v in vis]
        for entry in retiring:                                # the cuts are issued (and judged): unload, request the replacement
            self._cache.pop(entry.volume, None)
            self.queue.retire(entry)
        self.last_identifiers = [v.identifier for v in vis]   # (diagnostic: which volumes this batch was cut from)
        x, y = X, Y
        w = torch.tensor(ws, dtype=torch.float32, device=dev)
        for aug in self.augmenters:
            x, y, w = aug(x, y, bgs, w)
        return x, y.reshape(B, -1, 1), w

    def __iter__(self):
        while True:
            yield self()
