"""mpu_volume_encode (csrc/volume_encode.hip) against np.asfortranarray(a).tobytes(order="F"), byte for byte. Every source, output
and counter is carved from a guarded arena (tests/guarded.py) and the guard bands are checked after every call.

Shapes: X and Z * C over {1, 3, 63, 64, 65, 130, 257} -- one element, less than a packed dword, one short of the 64-wide tile, the
tile, one over it, two tiles and a bit, four tiles and one -- with Y in {1, 3} and C in {1, 3}; for C = 3 the Z * C of the list that
3 divides and 192, 195, 258 for the rest of the edges. An odd X with Y * Z > 1 starts the u8 file rows at every byte offset of a
dword; Z * C % 4 and X % 4 choose between the kernel's one-element and four-element paths on either side."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
from guarded import POISONS

pytestmark = pytest.mark.gpu

EDGES = (1, 3, 63, 64, 65, 130, 257)
ZC_OF = {1: EDGES, 3: (3, 63, 192, 195, 258)}
SOURCES = {"f32": torch.float32, "u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def random_source(rng, shape, kind):
    """f32: every bit random (NaNs of any payload, infinities and denormals among them); labels: class indices in [0, 256)."""
    if kind == "f32":
        a = rng.randint(0, 256, tuple(shape) + (4,), dtype=np.uint8).view(np.uint32)[..., 0].copy()
        special = np.array([0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc12345, 0x00000001, 0x807fffff, 0x80000000],
                           np.uint32)
        a.flat[:min(a.size, special.size)] = special[:a.size]
        return a.view(np.float32)
    return rng.randint(0, 256, shape).astype({"u8": np.uint8, "i32": np.int32, "i64": np.int64}[kind])


def expected_bytes(a, kind):
    b = a.view(np.uint32) if kind == "f32" else a.astype(np.uint8)        # (as integers: no NaN is touched on the way)
    return np.frombuffer(np.asfortranarray(b).tobytes(order="F"), np.uint8)


def encode(a, kind, fill, offset=0, check=False):
    """One guarded call. offset: bytes by which a u8 payload is moved off its 256-byte alignment.
    -> (payload as host u8 array, counter or None)."""
    from multiplanarunet_amd import data
    image = kind == "f32"
    n = int(a.size)
    A = guarded.arena(__name__, a.nbytes + n * (4 if image else 1) + offset + 8, 3, fill)
    src = A.put(torch.from_numpy(np.ascontiguousarray(a)).cuda(), "source")
    room = A.carve(n + offset, torch.float32 if image else torch.uint8, name="payload")
    bad = None if image else A.carve(1, torch.int64, name="bad")
    try:
        out, _ = data.encode_nifti_payload(src, "case.nii.gz", out=room[offset:], bad=bad, check=check)
    finally:
        torch.cuda.synchronize()
        assert not A.check(), (a.shape, kind, fill, A.check())
        assert bool((room[:offset].view(torch.uint8) == fill).all()), "bytes in front of a moved payload were written"
        assert torch.equal(guarded.bits(src), guarded.bits(a)), "the source was written"
    return out.cpu().numpy().view(np.uint8).reshape(-1), (None if bad is None else int(bad.item()))


@pytest.mark.parametrize("C_", (1, 3))
@pytest.mark.parametrize("kind", sorted(SOURCES))
def test_every_pair_against_numpy(kind, C_):
    rng = np.random.RandomState(17 + C_)
    k = 0
    for X in EDGES:
        for zc in ZC_OF[C_]:
            for Y in (1, 3):
                shape = (X, Y, zc // C_, C_)
                a = random_source(rng, shape, kind)
                got, n_bad = encode(a, kind, POISONS[k % 3])
                k += 1
                assert np.array_equal(got, expected_bytes(a, kind)), (shape, kind)
                assert n_bad == (None if kind == "f32" else 0), (shape, kind, n_bad)


def test_u8_rows_at_every_byte_offset():
    """Odd X with Y * Z > 1: consecutive file rows start 0, 1, 2, 3 bytes behind a dword; and the payload itself moved by 1, 2 and 3
    bytes, which shifts all of them. The same for the source rows (odd Z)."""
    rng = np.random.RandomState(5)
    k = 0
    for shape in ((3, 3, 5, 1), (63, 3, 7, 1), (65, 3, 65, 1), (257, 2, 5, 1), (5, 3, 257, 1), (130, 3, 3, 1), (7, 5, 3, 3)):
        for kind in ("u8", "i32", "i64"):
            a = random_source(rng, shape, kind)
            for offset in ((0, 1, 2, 3) if kind == "u8" else (0, 3)):
                got, n_bad = encode(a, kind, POISONS[k % 3], offset)
                k += 1
                assert np.array_equal(got, expected_bytes(a, kind)), (shape, kind, offset)
                assert n_bad == 0


def test_lower_rank_tensors_and_determinism():
    from multiplanarunet_amd import data
    rng = np.random.RandomState(9)
    for shape in ((70,), (5, 67), (37, 5, 70)):                  # missing axes count as 1, as in the header of the file
        for kind in ("f32", "u8"):
            a = random_source(rng, shape, kind)
            t = torch.from_numpy(a).cuda()
            one, _ = data.encode_nifti_payload(t)
            two, _ = data.encode_nifti_payload(t)
            assert torch.equal(one.view(torch.uint8), two.view(torch.uint8))
            assert np.array_equal(one.cpu().numpy().view(np.uint8).reshape(-1), expected_bytes(a, kind))


@pytest.mark.parametrize("kind", ("f32", "u8"))
def test_round_trip_through_the_decode(kind):
    from multiplanarunet_amd import _lib, data
    rng = np.random.RandomState(3)
    for shape in ((65, 3, 43, 3), (64, 2, 64, 1), (1, 1, 1, 1), (130, 1, 63, 1)):
        a = random_source(rng, shape, kind)
        t = torch.from_numpy(a).cuda()
        payload, _ = data.encode_nifti_payload(t)
        back = torch.empty_like(t)
        bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        _lib.call("mpu_volume_decode", _lib.ptr(payload), 16 if kind == "f32" else 2, 0, (C.c_int64 * 4)(*shape), 0, 1.0, 0.0,
                  _lib.MPU_DECODE_IMAGE if kind == "f32" else _lib.MPU_DECODE_LABELS, _lib.ptr(back), _lib.ptr(bad),
                  _lib.stream_ptr())
        assert torch.equal(back.view(torch.uint8), t.view(torch.uint8)), shape
        assert kind == "f32" or int(bad.item()) == 0


@pytest.mark.parametrize("kind", ("i32", "i64"))
def test_labels_out_of_range(kind):
    rng = np.random.RandomState(23)
    outside = [-1, 256] + ([2 ** 40] if kind == "i64" else [2 ** 31 - 1])
    for shape in ((65, 3, 43, 1), (64, 2, 64, 1), (3, 1, 1, 1)):
        a = random_source(rng, shape, kind)
        n = min(a.size, 7)
        where = rng.choice(a.size, n, replace=False)
        a.flat[where] = [outside[i % 3] for i in range(n)]
        got, n_bad = encode(a, kind, POISONS[0])
        assert n_bad == n, (shape, n_bad, n)
        want = a.copy()
        want.flat[where] = 0
        assert np.array_equal(got, expected_bytes(want, kind)), shape
        with pytest.raises(ValueError, match=r"case\.nii\.gz: %d label voxels" % n):
            encode(a, kind, POISONS[1], check=True)


def test_payload_over_4_gib():
    """(1040, 1, 1040, 1000) f32: 4.33e9 payload bytes -- byte offsets pass 2^32, element offsets 2^30. Compared on the device,
    as integers, with t.permute(3, 2, 1, 0)."""
    shape = (1040, 1, 1040, 1000)
    n = int(np.prod(shape))
    if torch.cuda.mem_get_info()[0] < 16 * 2 ** 30:
        pytest.skip("needs 16 GB of free HBM")
    from multiplanarunet_amd import data
    try:
        A = guarded.arena(__name__, 8 * n, 2, POISONS[2])
        src = A.carve(shape, torch.float32, name="source")
        gen = torch.Generator(device="cuda").manual_seed(1)
        src.view(torch.int32).random_(-2 ** 31, 2 ** 31 - 1, generator=gen)
        out, _ = data.encode_nifti_payload(src, out=A.carve(n, torch.float32, name="payload"))
        torch.cuda.synchronize()
        assert not A.check(), A.check()
        got = out.view(torch.int32).reshape(shape[::-1])
        want = src.view(torch.int32).permute(3, 2, 1, 0)
        for c0 in range(0, shape[3], 50):                        # (in slabs: no third buffer of 4 GB)
            assert torch.equal(got[c0:c0 + 50], want[c0:c0 + 50]), c0
        del src, out, got, want, A
    finally:
        guarded.release(__name__)


def test_bad_arguments_write_nothing():
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    fill = POISONS[2]
    A = guarded.arena(__name__, 3 * 4096, 3, fill)
    src = A.carve(1024, torch.float32, fill=0, name="source")
    out = A.carve(1024, torch.float32, name="payload")
    bad = A.carve(1, torch.int64, name="bad")
    st = _lib.stream_ptr()

    def shape(*s):
        return (C.c_int64 * 4)(*s)

    EINVAL, EUNSUPPORTED = -1, -3
    good = shape(8, 4, 8, 4)
    calls = [
        (EINVAL, (None, _lib.MPU_ENCODE_F32, good, 16, _lib.ptr(out), None, st)),                  # NULL source
        (EINVAL, (_lib.ptr(src), _lib.MPU_ENCODE_F32, good, 16, None, None, st)),                  # NULL payload
        (EINVAL, (_lib.ptr(src), _lib.MPU_ENCODE_F32, None, 16, _lib.ptr(out), None, st)),         # NULL shape
        (EINVAL, (_lib.ptr(src), _lib.MPU_ENCODE_I32, good, 2, _lib.ptr(out), None, st)),          # labels without a counter
        (EINVAL, (_lib.ptr(src), _lib.MPU_ENCODE_F32, shape(8, 0, 8, 4), 16, _lib.ptr(out), None, st)),
        (EINVAL, (_lib.ptr(src), _lib.MPU_ENCODE_F32, shape(8, 4, 32768, 1), 16, _lib.ptr(out), None, st)),
        (EINVAL, (C.c_void_p(src.data_ptr() + 2), _lib.MPU_ENCODE_F32, good, 16, _lib.ptr(out), None, st)),       # misaligned
        (EINVAL, (_lib.ptr(src), _lib.MPU_ENCODE_F32, good, 16, C.c_void_p(out.data_ptr() + 1), None, st)),
        (EINVAL, (_lib.ptr(src), _lib.MPU_ENCODE_I64, good, 2, _lib.ptr(out), C.c_void_p(bad.data_ptr() + 4), st)),
        (EINVAL, (C.c_void_p(src.data_ptr() + 4), _lib.MPU_ENCODE_I64, good, 2, _lib.ptr(out), _lib.ptr(bad), st)),
        (EUNSUPPORTED, (_lib.ptr(src), _lib.MPU_ENCODE_F32, good, 2, _lib.ptr(out), _lib.ptr(bad), st)),          # f32 -> u8
        (EUNSUPPORTED, (_lib.ptr(src), _lib.MPU_ENCODE_U8, good, 16, _lib.ptr(out), _lib.ptr(bad), st)),          # u8 -> f32
        (EUNSUPPORTED, (_lib.ptr(src), _lib.MPU_ENCODE_F32, good, 64, _lib.ptr(out), None, st)),                  # f32 -> f64
        (EUNSUPPORTED, (_lib.ptr(src), _lib.MPU_ENCODE_I32, good, 8, _lib.ptr(out), _lib.ptr(bad), st)),          # i32 -> i32
        (EUNSUPPORTED, (_lib.ptr(src), 7, good, 16, _lib.ptr(out), None, st)),                                    # no such source
    ]
    for want, args in calls:
        assert lib.mpu_volume_encode(*args) == want, args
        assert lib.mpu_last_error()
    torch.cuda.synchronize()
    assert not A.check()
    assert bool((out.view(torch.uint8) == fill).all()) and bool((bad.view(torch.uint8) == fill).all())
    with pytest.raises(ValueError, match="no device encode"):
        from multiplanarunet_amd import data
        data.encode_nifti_payload(torch.zeros(4, dtype=torch.float64, device="cuda"))
