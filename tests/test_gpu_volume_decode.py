"""mpu_volume_decode (csrc/volume_decode.hip) against nifti.read_nifti / formats.load_nifti_labels, bit for bit. The files are
written here byte by byte (header + payload), so that nothing of the writer under test takes part."""
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CODES = {2: "u1", 4: "i2", 8: "i4", 16: "f4", 64: "f8", 256: "i1", 512: "u2", 768: "u4", 1024: "i8", 1280: "u8"}
SHAPES = [(37, 5, 70), (1, 64, 3), (65, 66, 1)]
NAN = float("nan")
SCALINGS = [(float(np.float32(0.1)), float(np.float32(-1024.5))), (2.0, NAN), (1.0, 0.0), (1.0, NAN), (NAN, 3.0), (0.0, 3.0)]


def write_file(path, values, code, endian="<", slope=NAN, inter=NAN):
    """A NIfTI-1 file whose payload is `values` (an array of the stored shape) in Fortran order."""
    dt = np.dtype(endian + CODES[code])
    values = np.asarray(values)
    shape = values.shape
    hdr = bytearray(348)
    struct.pack_into(endian + "i", hdr, 0, 348)
    struct.pack_into(endian + "8h", hdr, 40, *([len(shape)] + list(shape) + [1] * (7 - len(shape))))
    struct.pack_into(endian + "2h", hdr, 70, code, dt.itemsize * 8)
    struct.pack_into(endian + "8f", hdr, 76, 1.0, 1.0, 2.0, 0.5, 1.0, 1.0, 1.0, 1.0)
    struct.pack_into(endian + "3f", hdr, 108, 352.0, slope, inter)
    struct.pack_into(endian + "2h", hdr, 252, 0, 2)
    struct.pack_into(endian + "12f", hdr, 280, 1, 0, 0, -3, 0, 2, 0, 4, 0, 0, 0.5, 5)
    hdr[344:348] = b"n+1\0"
    with open(path, "wb") as f:
        f.write(bytes(hdr) + b"\0\0\0\0" + values.astype(dt).tobytes(order="F"))
    return str(path)


def random_values(rng, code, shape, small=False):
    kind = np.dtype(CODES[code])
    if small:
        return rng.randint(0, 121, shape).astype(kind)
    if kind.kind == "f":
        return (rng.standard_normal(shape) * 1000.0).astype(kind)
    info = np.iinfo(kind)
    v = rng.randint(0, 256, shape + (kind.itemsize,), dtype=np.uint8).view(kind)[..., 0].copy()      # every bit random
    v.flat[:2] = (info.min, info.max)
    return v


def f32_of_int(x):
    """The f32 nearest to the integer x, ties to even, in integer arithmetic: ONE rounding (the expected value that does not
    come from NumPy)."""
    a = abs(x)
    shift = max(0, a.bit_length() - 24)
    q, r = divmod(a, 1 << shift)
    if shift and (2 * r > (1 << shift) or (2 * r == (1 << shift) and q & 1)):
        q += 1
    val = float(q) * float(1 << shift)                           # exact: q <= 2^24, a power of two
    return -val if x < 0 else val


def device_image(path):
    from multiplanarunet_amd import nifti, data
    h, _, buf = nifti.read_nifti_payload(path)
    return data.decode_nifti_payload(h, buf, "cuda", False, path)


def device_labels(path):
    from multiplanarunet_amd import nifti, data
    h, _, buf = nifti.read_nifti_payload(path)
    return data.decode_nifti_payload(h, buf, "cuda", True, path)


def check_image(path):
    from multiplanarunet_amd.formats import load_nifti
    want, _ = load_nifti(path)
    got = device_image(path)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=path)


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_datatype_and_endianness(tmp_path, shape, C):
    rng = np.random.RandomState(7)
    full = shape if C == 1 else shape + (C,)
    for code in CODES:
        for endian in "<>":
            check_image(write_file(tmp_path / ("t%d%s.nii" % (code, "le" if endian == "<" else "be")),
                                   random_values(rng, code, full), code, endian))


@pytest.mark.parametrize("slope,inter", SCALINGS)
def test_scaling(tmp_path, slope, inter):
    rng = np.random.RandomState(11)
    for code in CODES:
        for endian in ("<", ">") if code in (4, 1024, 64) else ("<",):
            with np.errstate(over="ignore"):
                check_image(write_file(tmp_path / ("s%d%s.nii" % (code, endian == "<")), random_values(rng, code, (37, 5, 70, 2)),
                                       code, endian, slope, inter))


def test_integer_rounding(tmp_path):
    big = 2 ** 60 + 2 ** 36 + 1
    assert np.array([big], np.int64).astype(np.float32)[0] == np.float32(2 ** 60 + 2 ** 37)           # one conversion
    assert np.array([big], np.int64).astype(np.float64).astype(np.float32)[0] == np.float32(2 ** 60)  # through f64: not this
    cases = [(1024, [big, -big, 0, 1, -1, 2 ** 62 + 2 ** 38 + 1, -(2 ** 63), 2 ** 63 - 1]),
             (1280, [big, 2 ** 63 + 2 ** 39 + 1, 0, 1, 2 ** 64 - 1, 2 ** 63, 2 ** 24 + 1, 2 ** 53 + 1]),
             (8, [2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), -(2 ** 24 + 3), 2 ** 31 - 1, -(2 ** 31), 2 ** 25 + 2, 0]),
             (768, [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 - 1, 2 ** 31 + 2 ** 7, 2 ** 31 + 2 ** 7 + 1, 0, 1, 2 ** 25 + 2])]
    for code, vals in cases:
        v = np.array(vals, np.dtype(CODES[code])).reshape(2, 2, 2)
        for endian in "<>":
            p = write_file(tmp_path / ("r%d%s.nii" % (code, endian == "<")), v, code, endian)
            check_image(p)
            got = device_image(p).cpu().numpy().ravel(order="C")
            want = np.array([f32_of_int(int(x)) for x in v.ravel()], np.float32)
            np.testing.assert_array_equal(got, want)
            check_image(write_file(tmp_path / "rs.nii", v, code, endian, 2.0, NAN))     # scaled: through f64, as NumPy
    got = device_image(write_file(tmp_path / "r.nii", np.array([big, -big], np.int64).reshape(2, 1, 1), 1024)).cpu().numpy().ravel()
    assert got[0] == np.float32(2 ** 60 + 2 ** 37) and got[1] == -np.float32(2 ** 60 + 2 ** 37)
    got = device_image(write_file(tmp_path / "r.nii", np.array([2 ** 63 + 2 ** 39 + 1], np.uint64).reshape(1, 1, 1), 1280))
    assert got.item() == float(np.float32(2 ** 63 + 2 ** 40))


def test_labels(tmp_path):
    from multiplanarunet_amd.formats import load_nifti_labels
    p = write_file(tmp_path / "l.nii", np.array([3.999, 0, 255, 255.9], np.float32).reshape(4, 1, 1), 16)
    got = device_labels(p)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 1, 1)
    assert got.cpu().numpy().ravel().tolist() == [3, 0, 255, 255]
    np.testing.assert_array_equal(got.cpu().numpy(), load_nifti_labels(p))
    for bad in (256.0, -1.0, 300.0, NAN):
        p = write_file(tmp_path / "bad.nii", np.array([1, bad, 2, 3], np.float64).reshape(2, 2, 1), 64)
        with pytest.raises(ValueError, match=r"bad\.nii: 1 label voxels"):
            device_labels(p)
    p = write_file(tmp_path / "bad4.nii", np.array([256, -1, 300, NAN, 5, -0.5], np.float32).reshape(6, 1, 1), 16)
    with pytest.raises(ValueError, match=r"bad4\.nii: 4 label voxels"):
        device_labels(p)
    # every stored type, both endiannesses, odd shapes, a trailing singleton axis, and a scaled label file
    rng = np.random.RandomState(3)
    for code in CODES:
        for endian in "<>":
            for shape in ((37, 5, 70), (65, 66, 1, 1)):
                p = write_file(tmp_path / "lab.nii", random_values(rng, code, shape, small=True), code, endian)
                want = load_nifti_labels(p)
                got = device_labels(p)
                assert tuple(got.shape) == want.shape == shape[:3]
                np.testing.assert_array_equal(got.cpu().numpy(), want)
    p = write_file(tmp_path / "labs.nii", random_values(rng, 2, (37, 5, 70), small=True), 2, "<", 2.0, 1.5)
    np.testing.assert_array_equal(device_labels(p).cpu().numpy(), load_nifti_labels(p))


def test_load_volume_to_device_equals_host_path(tmp_path):
    from multiplanarunet_amd import data
    from multiplanarunet_amd.formats import load_nifti, load_nifti_labels
    from multiplanarunet_amd.interpolation import ViewGeometry, sample_view
    rng = np.random.RandomState(5)
    shape = (37, 29, 41)
    img = write_file(tmp_path / "case.nii", rng.randint(-900, 2000, shape + (2,)).astype(np.int16), 4, "<", 0.5, -100.0)
    lab = write_file(tmp_path / "case_lab.nii", rng.randint(0, 4, shape).astype(np.uint8), 2)
    vol = data.load_volume_to_device(img, lab, "cuda", "1pct", "RobustScaler", "case")
    h_img, aff = load_nifti(img)
    ref = data.as_volume(h_img, load_nifti_labels(lab), aff, "1pct", "RobustScaler", "cuda", "case")
    assert torch.equal(vol.image, ref.image) and torch.equal(vol.labels, ref.labels)
    np.testing.assert_array_equal(vol.affine, ref.affine)
    assert vol.bg_value == ref.bg_value and vol.identifier == "case" and vol.source_path == img
    np.testing.assert_array_equal(vol._scaler.p0, ref._scaler.p0)
    np.testing.assert_array_equal(vol._scaler.p1, ref._scaler.p1)
    geom = ViewGeometry(np.array([0.3, 0.5, 0.8]), 32, 40.0, n_planes="same")
    xa, ya = sample_view(vol, geom)
    xb, yb = sample_view(ref, geom)
    assert torch.equal(xa, xb) and torch.equal(ya, yb)
    # what keeps the host path: .npz, fit_on="host"
    np.savez(tmp_path / "v.npz", image=h_img, labels=load_nifti_labels(lab), affine=aff)
    vz = data.load_volume_to_device(str(tmp_path / "v.npz"), None, "cuda", "1pct", "RobustScaler")
    assert torch.equal(vz.image, ref.image) and torch.equal(vz.labels, ref.labels) and vz.bg_value == ref.bg_value
    vh = data.load_volume_to_device(img, lab, "cuda", "1pct", "RobustScaler", fit_on="host")
    assert torch.equal(vh.image, ref.image) and torch.equal(vh.labels, ref.labels)
