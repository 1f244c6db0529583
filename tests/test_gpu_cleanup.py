"""Label-map clean-up on the device (csrc/components.hip: size threshold, hole filling; csrc/surface.hip: opening / closing by a
Euclidean ball; through postprocess.py and the C entries) against the NumPy restatement of tests/cleanup_ref.py (itself held to scipy
and to the brute-force transform by tests/test_cleanup_host.py): exact equality on every voxel and every report entry on the whole
case list, the input left untouched; in place and out of place; class subsets; label volumes off 16-byte alignment; identical bytes
run to run and on a side stream; guard bands and poisoned scratch around every caller-owned buffer; the thresholds against
surface.edt_squared of the same build; and `mp predict --synthetic` with all clean-up flags end to end."""
import contextlib
import ctypes as C
import io
import re

import numpy as np
import pytest
import torch

import cleanup_ref as R
import guarded
from guarded import NAN, POISONS, ZERO, bits

pytestmark = pytest.mark.gpu

CASES = list(R.cases())
BALL_IDS = list(range(len(R.BALLS)))


@pytest.fixture(scope="module", autouse=True)
def free_arena():
    yield
    guarded.release(__name__)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want):
    out, table = got
    assert out.dtype == torch.uint8 and table.dtype == np.int64 and table.shape == want[1].shape
    np.testing.assert_array_equal(out.cpu().numpy(), want[0])
    np.testing.assert_array_equal(table, want[1])


def check_components_case(name, connectivity, d_labels):
    """Size threshold (three thresholds) and hole filling on a device copy of the case; the input is left as it was."""
    from multiplanarunet_amd import postprocess as PP
    labels, K = R.cases()[name]
    for min_voxels in R.MIN_VOXELS:
        same(PP.remove_small_components(d_labels, K, min_voxels, connectivity, report=True), R.reference_small(name, connectivity, min_voxels))
    same(PP.fill_holes(d_labels, K, connectivity, report=True), R.reference_fill(name, connectivity))
    np.testing.assert_array_equal(d_labels.cpu().numpy(), labels)


def check_ball_case(name, ball, d_labels):
    from multiplanarunet_amd import postprocess as PP
    labels, K = R.cases()[name]
    spacing, radius = R.BALLS[ball]
    same(PP.open_ball(d_labels, K, radius, spacing, report=True), R.reference_ball(name, R.OPEN, ball))
    same(PP.close_ball(d_labels, K, radius, spacing, report=True), R.reference_ball(name, R.CLOSE, ball))
    np.testing.assert_array_equal(d_labels.cpu().numpy(), labels)


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", CASES)
def test_size_threshold_and_hole_filling_equal_the_restatement(name, connectivity):
    check_components_case(name, connectivity, dev(R.cases()[name][0]))


@pytest.mark.parametrize("ball", BALL_IDS)
@pytest.mark.parametrize("name", CASES)
def test_opening_and_closing_equal_the_restatement(name, ball):
    check_ball_case(name, ball, dev(R.cases()[name][0]))


def test_defaults_are_those_of_the_issue():
    from multiplanarunet_amd import postprocess as PP
    labels, K = R.cases()["edge_corner_contact"]
    d = dev(labels)
    same(PP.fill_holes(d, K, report=True), R.reference_fill("edge_corner_contact", 6))                  # 6, as binary_fill_holes
    same(PP.remove_small_components(d, K, 5, report=True), R.reference_small("edge_corner_contact", 26, 5))
    same(PP.close_ball(d, K, 1.0, report=True), R.reference_ball("edge_corner_contact", R.CLOSE, 0))   # unit spacing
    assert torch.equal(PP.remove_small_components(d, K, 1), d)                                          # min_voxels = 1: the identity


@pytest.mark.parametrize("name", ["blobs_K4", "line_1x1x50", "nested_shells"])
@pytest.mark.parametrize("offset", [1, 4])
def test_labels_that_are_not_16_byte_aligned(name, offset):
    """The label volume needs no alignment: at offset 1 every access is the byte path, at offset 4 the dword paths stay."""
    labels, _ = R.cases()[name]
    for inplace in (False, True):
        buf = torch.zeros(labels.size + 64, dtype=torch.uint8, device="cuda")
        view = buf[offset:offset + labels.size].view(labels.shape)
        view.copy_(dev(labels))
        assert view.data_ptr() % 16 == offset and view.is_contiguous()
        if not inplace:
            check_components_case(name, 18, view)
            check_ball_case(name, 2, view)
        else:                                                  # the unaligned volume as the OUTPUT too
            from multiplanarunet_amd import postprocess as PP
            K = R.cases()[name][1]
            for call, want in ((lambda v: PP.fill_holes(v, K, 26, out=v), R.reference_fill(name, 26)),
                               (lambda v: PP.remove_small_components(v, K, 5, 6, out=v), R.reference_small(name, 6, 5)),
                               (lambda v: PP.open_ball(v, K, *R.BALLS[3][::-1], out=v), R.reference_ball(name, R.OPEN, 3))):
                view.copy_(dev(labels))
                assert call(view) is view
                np.testing.assert_array_equal(view.cpu().numpy(), want[0])
        assert int(buf[:offset].sum()) == 0 and int(buf[offset + labels.size:].sum()) == 0


@pytest.mark.parametrize("name", ["blobs_K4", "blobs_K16", "foreign_bounds", "touching_face"])
def test_in_place_subsets_and_the_reports(name):
    from multiplanarunet_amd import postprocess as PP
    labels, K = R.cases()[name]
    d = dev(labels)
    sp, rad = R.BALLS[2]
    ops = {"small": (lambda x, **k: PP.remove_small_components(x, K, 5, 18, **k), lambda cl: R.remove_small(labels, K, 5, 18, classes=cl)),
           "fill": (lambda x, **k: PP.fill_holes(x, K, 6, **k), lambda cl: R.fill_holes(labels, K, 6, classes=cl)),
           "open": (lambda x, **k: PP.open_ball(x, K, rad, sp, **k), lambda cl: R.open_ball(labels, K, rad, sp, classes=cl)),
           "close": (lambda x, **k: PP.close_ball(x, K, rad, sp, **k), lambda cl: R.close_ball(labels, K, rad, sp, classes=cl))}
    for op, (run, ref) in ops.items():
        want = ref(None)
        inplace = d.clone()
        got, table = run(inplace, out=inplace, report=True)
        assert got is inplace
        same((inplace, table), want)                                          # in place = the reference
        other = torch.full_like(d, 99)
        assert run(d, out=other) is other and torch.equal(other, inplace)    # = out of place into a caller's tensor
        for classes in ([1], [K - 1], list(range(2, K))):
            want = ref(classes)
            out, table = run(d, classes=classes, report=True)
            same((out, table), want)
            for c in range(1, K):                                             # the other classes: bit-identical
                if c not in classes:
                    assert torch.equal(out == c, d == c), (op, classes, c)
            assert torch.equal(out[d >= K], d[d >= K])                        # foreign labels are never rewritten
        with pytest.raises(ValueError, match="class_mask"):
            run(d, classes=[0])
        with pytest.raises(ValueError, match="class_mask"):
            run(d, classes=[K])
    with pytest.raises(ValueError, match="connectivity"):
        PP.fill_holes(d, K, 8)
    with pytest.raises(ValueError, match="min_voxels"):
        PP.remove_small_components(d, K, 0)
    with pytest.raises(ValueError, match="radius"):
        PP.open_ball(d, K, 0.0)
    with pytest.raises(ValueError, match="spacing"):
        PP.close_ball(d, K, 1.0, (1.0, 0.0, 1.0))
    with pytest.raises(NotImplementedError, match="n_classes"):
        PP.fill_holes(d, 17)


def test_two_runs_give_identical_bytes_also_on_a_side_stream():
    from multiplanarunet_amd import postprocess as PP
    name = "blobs_K4"
    labels, K = R.cases()[name]
    d = dev(labels)
    sp, rad = R.BALLS[2]

    def all_four():
        return (PP.remove_small_components(d, K, 5, 26, report=True) + PP.fill_holes(d, K, 6, report=True)
                + PP.open_ball(d, K, rad, sp, report=True) + PP.close_ball(d, K, rad, sp, report=True))
    runs = [all_four() for _ in range(2)]
    side, busy = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):                                             # another stream is busy meanwhile
        for _ in range(24):
            a = torch.tanh(a @ a)
    with torch.cuda.stream(side):
        runs.append(all_four())
    torch.cuda.synchronize()
    for run in runs:
        for x, y in zip(run, runs[0]):
            assert torch.equal(bits(x), bits(y))
    want = R.reference_small(name, 26, 5) + R.reference_fill(name, 6) + R.reference_ball(name, R.OPEN, 2) + R.reference_ball(name, R.CLOSE, 2)
    for x, y in zip(runs[-1], want):
        np.testing.assert_array_equal(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, y)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs_K4", "blobs_K16", "line_1x1x50"])
def test_guarded_buffers_under_three_poisons(name):
    """labels, the four outputs, the four reports and the three scratch buffers carved from a guarded arena of 0xFF, 0x00 and 0x7B
    bytes: no guard byte changes, and the outputs are the same bits three times (scratch and outputs are never read before they are
    written) and the reference's."""
    from multiplanarunet_amd import _lib
    lib = _lib.load()
    labels, K = R.cases()[name]
    shape3 = (C.c_int64 * 3)(*labels.shape)
    spacing, radius = R.BALLS[2]
    sp = (C.c_double * 3)(*spacing)
    n_cc, n_fh, n_sd = (int(getattr(lib, q)(shape3)) for q in ("mpu_components_scratch_bytes", "mpu_fill_holes_scratch_bytes",
                                                                "mpu_surface_scratch_bytes"))
    assert 0 < n_cc < n_fh <= n_sd
    want = (R.reference_small(name, 26, 5), R.reference_fill(name, 6), R.reference_ball(name, R.OPEN, 2), R.reference_ball(name, R.CLOSE, 2))
    d = dev(labels)
    mask = (1 << K) - 2
    got = {}
    for fill in POISONS:
        A = guarded.arena(__name__, 5 * labels.size + n_cc + n_fh + n_sd + 4096, 12, fill)
        lab = A.put(d, name="labels")
        outs = [A.carve(labels.shape, torch.uint8, name="out%d" % k) for k in range(4)]
        reps = [A.carve((K, cols), torch.int64, name="report%d" % k) for k, cols in enumerate((3, 2, 2, 2))]
        s_cc, s_fh, s_sd = (A.carve(nb, torch.uint8, name=nm) for nb, nm in ((n_cc, "scratch_cc"), (n_fh, "scratch_fh"), (n_sd, "scratch_sd")))
        st = _lib.stream_ptr()
        _lib.call("mpu_remove_small_components", _lib.ptr(lab), shape3, 26, K, mask, 5, _lib.ptr(outs[0]), _lib.ptr(reps[0]), _lib.ptr(s_cc), st)
        _lib.call("mpu_fill_holes", _lib.ptr(lab), shape3, 6, K, mask, _lib.ptr(outs[1]), _lib.ptr(reps[1]), _lib.ptr(s_fh), st)
        _lib.call("mpu_morph_ball", _lib.ptr(lab), shape3, sp, K, mask, _lib.MPU_MORPH_OPEN, radius, _lib.ptr(outs[2]), _lib.ptr(reps[2]),
                  _lib.ptr(s_sd), st)
        _lib.call("mpu_morph_ball", _lib.ptr(lab), shape3, sp, K, mask, _lib.MPU_MORPH_CLOSE, radius, _lib.ptr(outs[3]), _lib.ptr(reps[3]),
                  _lib.ptr(s_sd), st)
        torch.cuda.synchronize()
        assert not A.check(), (fill, A.check())
        assert torch.equal(lab, d)
        got[fill] = [t.cpu() for t in outs + reps]
    for fill in POISONS[1:]:
        for x, y in zip(got[NAN], got[fill]):
            assert torch.equal(bits(x), bits(y)), "an output depends on the poison (0xFF vs 0x%02X)" % fill
    for k in range(4):
        np.testing.assert_array_equal(got[ZERO][k].numpy(), want[k][0])
        np.testing.assert_array_equal(got[ZERO][4 + k].numpy(), want[k][1])


# ---- the thresholds are those of the transform of the same build -------------------------------------------------------------------
@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), R.ANISO])
def test_thresholds_agree_with_edt_squared_at_attained_radii(spacing):
    """One class, radius^2 EXACTLY an attained squared distance (the square of a representable root: multiples of 0.5 here): the
    dilation inside close_ball is {d2 <= r2} and the erosion inside open_ball {d2 > r2} of surface.edt_squared, voxel for voxel."""
    from multiplanarunet_amd import postprocess as PP, surface as S
    labels, K = R.cases()["blobs_K4"]
    one = (labels == 2).astype(np.uint8)
    d = dev(one)
    d2_in = S.edt_squared(d, spacing, S.EQUAL, 1)              # to the mask
    d2_out = S.edt_squared(d, spacing, S.NOT_EQUAL, 1)         # to its complement
    attained = np.unique(d2_in.cpu().numpy())
    radii = [r for r in (0.5, 1.0, 1.5, 2.0, 2.5, 3.0) if np.float64(r) * np.float64(r) in attained]
    assert len(radii) >= 3
    for radius in radii:
        r2 = float(np.float64(radius) * np.float64(radius))
        dil = (d2_in <= r2).to(torch.uint8)
        ero = (d2_out > r2).to(torch.uint8)
        closed = (S.edt_squared(dil, spacing, S.EQUAL, 0) > r2).to(torch.uint8)
        opened = (S.edt_squared(ero, spacing, S.EQUAL, 1) <= r2).to(torch.uint8)
        assert torch.equal(PP.close_ball(d, 2, radius, spacing), closed)
        assert torch.equal(PP.open_ball(d, 2, radius, spacing), opened)
        assert bool((closed >= d).all()) and bool((opened <= d).all())       # extensive / anti-extensive
        # one ulp below an attained distance the voxels AT that distance fall out of the ball
        below = float(np.sqrt(np.nextafter(r2, 0.0)))
        if np.float64(below) * np.float64(below) < r2:
            assert int((d2_in <= np.float64(below) * np.float64(below)).sum()) < int(dil.sum())


# ---- mp predict with every clean-up flag ---------------------------------------------------------------------------------------------
FLAGS = ["--open_mm", "1", "--close_mm", "1.5", "--fill_holes", "--hole_connectivity", "18", "--min_component_voxels", "12",
         "--clean_connectivity", "6", "--clean_classes", "1,2"]
CSV_COLS = ("voxels_added", "voxels_removed", "cavities", "voxels_filled", "components", "voxels_kept")


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """A 64^3 synthetic project, trained briefly; predicted plainly, with every clean-up flag (and the largest-component filter
    behind them), and plainly again -> (folder, log of the flagged run)."""
    from multiplanarunet_amd.cli import mp
    proj = tmp_path_factory.mktemp("clean_proj")
    (proj / "train_hparams.yaml").write_text(
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 64\n  depth: 3\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 64.0\n  batch_size: 8\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: SparseCategoricalCrossentropy\n  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n")
    base = ["predict", "--project_dir", str(proj), "--synthetic", "1", "--sum_fusion"]
    with contextlib.redirect_stdout(io.StringIO()):
        mp.entry_func(["train", "--project_dir", str(proj), "--synthetic", "4", "--epochs", "2", "--train_images_per_epoch", "32",
                       "--val_images_per_epoch", "16"])
        mp.entry_func(base + ["--out_dir", "pred_plain"])
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        mp.entry_func(base + ["--out_dir", "pred_clean", "--largest_component"] + FLAGS)
    with contextlib.redirect_stdout(io.StringIO()):
        mp.entry_func(base + ["--out_dir", "pred_again"])
    return proj, log.getvalue()


def saved(proj, out_dir):
    z = np.load(proj / out_dir / "nii_files" / "toy_5000_PRED.npz")
    assert z["labels"].dtype == np.uint8 and z["labels"].shape == (64, 64, 64)
    return np.ascontiguousarray(z["labels"]), z["affine"]


def test_mp_predict_with_every_cleanup_flag(project):
    import components_ref as CR
    from multiplanarunet_amd import surface as S
    from multiplanarunet_amd.data import make_toy_volume
    from multiplanarunet_amd.interpolation import dice_all
    proj, log = project
    plain, affine = saved(proj, "pred_plain")
    cleaned, _ = saved(proj, "pred_clean")
    spacing = tuple(float(s) for s in S.voxel_sizes(affine))
    # the stages in order, by the restatement, on the unflagged run's map
    cur, tables = plain, []
    for stage, step in (("open", lambda m: R.open_ball(m, 3, 1.0, spacing, classes=[1, 2])),
                        ("close", lambda m: R.close_ball(m, 3, 1.5, spacing, classes=[1, 2])),
                        ("fill_holes", lambda m: R.fill_holes(m, 3, 18, classes=[1, 2])),
                        ("small_components", lambda m: R.remove_small(m, 3, 12, 6, classes=[1, 2]))):
        cur, t = step(cur)
        tables.append((stage, t))
    want, _ = CR.keep_largest(cur, 3, 26)
    np.testing.assert_array_equal(cleaned, want)
    assert sum(int(t.sum()) for _, t in tables) > 0 and not np.array_equal(cleaned, plain)      # (the stages had something to do)
    # csv/cleanup_results.csv: one row per (class, stage) in stage order, the counts of the report tables
    rows = (proj / "pred_clean" / "csv" / "cleanup_results.csv").read_text().strip().splitlines()
    assert rows[0] == "image,class,stage," + ",".join(CSV_COLS)
    names = {"open": CSV_COLS[0:2], "close": CSV_COLS[0:2], "fill_holes": CSV_COLS[2:4], "small_components": (CSV_COLS[4], CSV_COLS[5], CSV_COLS[1])}
    expect = []
    for stage, t in tables:
        for c in ([0] if stage == "fill_holes" else []) + [1, 2]:
            counts = dict(zip(names[stage], (int(x) for x in t[c])))
            expect.append("toy_5000,%d,%s,%s" % (c, stage, ",".join(str(counts.get(k, "")) for k in CSV_COLS)))
            line = "toy_5000: class %d: %s: %s" % (c, stage, ", ".join("%d %s" % (counts[k], k.replace("_", " ")) for k in names[stage]))
            assert line in log, (line, log[-3000:])
    assert rows[1:] == expect
    # the Dice that is printed and written is that of the saved map
    _, truth, _ = make_toy_volume(64, 5000)
    d = dice_all(np.asarray(truth).reshape(64, 64, 64), cleaned, n_classes=3, ignore_zero=True)
    assert re.search(r"toy_5000: dices .* mean %.4f" % float(np.nanmean(d)), log)
    res = (proj / "pred_clean" / "csv" / "results.csv").read_text().strip().splitlines()
    assert res[1] == "toy_5000,%.5f,%s" % (float(np.nanmean(d)), ",".join("%.5f" % x for x in d))


def test_mp_predict_without_the_flags_is_unchanged(project):
    proj, _ = project
    a, aff_a = saved(proj, "pred_plain")
    b, aff_b = saved(proj, "pred_again")
    assert a.tobytes() == b.tobytes() and aff_a.tobytes() == aff_b.tobytes()
    for name in ("results.csv", "per_view.csv"):
        assert (proj / "pred_plain" / "csv" / name).read_bytes() == (proj / "pred_again" / "csv" / name).read_bytes()
    assert not (proj / "pred_plain" / "csv" / "cleanup_results.csv").exists()
    assert not (proj / "pred_again" / "csv" / "cleanup_results.csv").exists()


def test_mp_predict_refusals_leave_no_output_folder(project):
    from multiplanarunet_amd.cli import mp
    proj, _ = project
    for flags, needle in ((["--fill_holes", "--no_argmax"], "--no_argmax"), (["--hole_connectivity", "6"], "needs --fill_holes"),
                          (["--fill_holes", "--clean_classes", "3"], "n_classes - 1 = 2"), (["--open_mm", "0"], "finite")):
        with pytest.raises(ValueError, match=needle):
            mp.entry_func(["predict", "--project_dir", str(proj), "--synthetic", "1", "--sum_fusion", "--out_dir", "pred_refused"] + flags)
    assert not (proj / "pred_refused").exists()
