"""
`mp predict` on MI355X: flags / project layout of mpunet/bin/predict.py:19-78,433-470; the 6-view
loop, back-mapping and fusion run in multiplanarunet_amd.predict (distributed: plane-sharded).
Outputs <out_dir>/nii_files/<id>_PRED.nii.gz for NIfTI inputs (mpunet/bin/predict.py:90-117; native writer, nifti.py) and
<id>_PRED.npz (labels + affine) for .npz / synthetic volumes; --out_format forces one of them.
Rank 0 writes through ONE prediction_writer.PredictionWriter: the compute thread makes a NIfTI file's payload bytes on the device
(mpu_volume_encode) and fetches them with one copy; gzip, the write and the rename onto the final name run on the writer's thread
while the next volume is predicted. The writer is closed before run() returns or raises: every file is complete by then.
--largest_component (no reference counterpart; postprocess.py): rank 0 filters the fused label map on the device -- per class, only
the largest connected component stays -- before the Dice evaluation and before the file is made, so that the saved file,
results.csv and the log describe the same map.
--open_mm R, --close_mm R, --fill_holes [--hole_connectivity], --min_component_voxels N [--clean_connectivity], --clean_classes (no
reference counterpart; postprocess.py): rank 0 cleans the fused label map on the device BEFORE that filter, in the fixed order open ->
close -> fill holes -> size threshold (closing seals gaps so that holes become cavities; the size filters then judge the repaired
objects), with the voxel sizes of the affine as the spacing of the ball; one log line per stage and class and csv/cleanup_results.csv
from the report tables. Without these flags nothing of it is imported or launched.
--surface_metrics [--nsd_tolerance MM] (no reference counterpart; surface.py): rank 0 also evaluates that saved map against the labels
by surface distances on the device -- HD, HD95, ASSD and the voxel-border NSD per foreground class, with the voxel sizes of the
affine -- and writes csv/surface_results.csv. No other output changes, and without the flag surface.py is not imported.
--uncertainty [--uncertainty_maps entropy,mi,agreement] (no reference counterpart; uncertainty.py): the final fuse also gives, per
voxel, the entropy of the fused distribution, the mutual information between the views and the number of views that vote for the
winning class -- <id>_ENTROPY / _MI / _AGREE.nii.gz beside <id>_PRED.nii.gz, or the keys entropy / mi / agreement of the .npz; they
are properties of the fusion, so clean-up and the filter do not alter them -- and csv/uncertainty_results.csv has their means per
class of the map that is saved (over the correct and the wrong voxels too when the volume has labels). One GPU and softmax models
only: refused before a folder is created otherwise. The prediction is the same bytes, and without the flag uncertainty.py is not
imported.
"""
import os
from argparse import ArgumentParser
import numpy as np
import torch

from .common import (validate_project_dir, load_hparams, load_dataset, dataset_entries, require_audited_hparams,
                     fusion_weights_path, note_inert_flags)


def get_argparser():
    p = ArgumentParser(description="Predict using a mpunet model (MI355X hot path).")
    p.add_argument("--project_dir", type=str, default="./")
    p.add_argument("-f", help="Predict on a single file (.nii / .nii.gz / .npz)")
    p.add_argument("-l", help="Optional single label file (.nii / .nii.gz / .npz) to use with -f")
    p.add_argument("--out_format", default="auto", choices=("auto", "nii", "npz"),
                   help="auto: <id>_PRED.nii.gz for NIfTI inputs, <id>_PRED.npz otherwise")
    p.add_argument("--dataset", type=str, default="test")
    p.add_argument("--out_dir", type=str, default="predictions")
    p.add_argument("--num_GPUs", type=int, default=1)
    p.add_argument("--sum_fusion", action="store_true")
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--no_eval", action="store_true")
    p.add_argument("--eval_prob", type=float, default=1.0)
    p.add_argument("--force_GPU", type=str, default="")
    p.add_argument("--save_input_files", action="store_true")
    p.add_argument("--no_argmax", action="store_true")
    p.add_argument("--on_val", action="store_true")
    p.add_argument("--wait_for", type=str, default="")
    p.add_argument("--continue", action="store_true", dest="continue_")
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--map_method", default="nearest", choices=("nearest", "linear"),
                   help="how a voxel reads a view's prediction: nearest (default, the reference's predict) or linear (trilinear "
                        "interpolation of the class probabilities, map_real_space_pred(method='linear')). Fusion weights should be "
                        "trained with the method used at predict time (mp train_fusion --map_method)")
    p.add_argument("--dtype", default="bf16", choices=("bf16", "f32", "bf16x3"),
                   help="bf16 (default, the benchmarked mode), f32 (exact-f32 MFMAs: the parity mode), bf16x3 (f32 storage, three bf16 "
                        "MFMAs per product: f32-grade results at 2.6x the f32 speed)")
    p.add_argument("--largest_component", action="store_true",
                   help="keep only the largest connected component of every foreground class of the fused label map (on the device; "
                        "off by default)")
    p.add_argument("--cc_connectivity", type=int, default=None, choices=(6, 18, 26),
                   help="voxel neighbourhood of --largest_component (default 26)")
    p.add_argument("--cc_classes", type=str, default=None,
                   help="comma-separated classes --largest_component filters, e.g. 1,3 (default: all foreground classes)")
    p.add_argument("--open_mm", type=float, default=None,
                   help="open every class of the fused label map by a Euclidean ball of this radius, in the units of the affine (on "
                        "the device; off by default). Clean-up stages run in the order open, close, fill holes, size threshold, "
                        "then --largest_component")
    p.add_argument("--close_mm", type=float, default=None, help="close every class by a Euclidean ball of this radius (background only "
                                                                "is given to a class)")
    p.add_argument("--fill_holes", action="store_true",
                   help="fill every background cavity with the class that borders it most (face vote; a tie: the smallest class)")
    p.add_argument("--hole_connectivity", type=int, default=None, choices=(6, 18, 26),
                   help="background connectivity of --fill_holes (default 6, scipy's binary_fill_holes)")
    p.add_argument("--min_component_voxels", type=int, default=None,
                   help="remove every connected component of a class with fewer voxels than this")
    p.add_argument("--clean_connectivity", type=int, default=None, choices=(6, 18, 26),
                   help="voxel neighbourhood of --min_component_voxels (default 26)")
    p.add_argument("--clean_classes", type=str, default=None,
                   help="comma-separated classes the four clean-up operations work on, e.g. 1,3 (default: all foreground classes)")
    p.add_argument("--surface_metrics", action="store_true",
                   help="also evaluate the saved label map against the labels by surface distances, per foreground class: HD, HD95, "
                        "ASSD and NSD (on the device; csv/surface_results.csv; off by default)")
    p.add_argument("--nsd_tolerance", type=float, default=None,
                   help="tolerance of the NSD of --surface_metrics, in the units of the affine (default 1.0)")
    p.add_argument("--uncertainty", action="store_true",
                   help="also save per-voxel uncertainty maps of the multi-view fusion: <id>_ENTROPY (entropy of the fused "
                        "distribution), <id>_MI (spread between the views) and <id>_AGREE (views that vote for the winning class), "
                        "and csv/uncertainty_results.csv (on the device, one GPU, softmax models; off by default)")
    p.add_argument("--uncertainty_maps", type=str, default=None,
                   help="comma-separated maps --uncertainty computes, out of entropy,mi,agreement (default: all three)")
    return p


UNCERTAINTY_SUFFIX = (("entropy", "ENTROPY"), ("mi", "MI"), ("agreement", "AGREE"))      # map name, <id>_<SUFFIX>.nii.gz


def uncertainty_plan(args, out_activation=None):
    """The --uncertainty flags, checked: None when the maps are off, else the tuple of map names in the order entropy, mi,
    agreement. ValueError on a combination that cannot be served; with out_activation also on a model whose outputs are logits."""
    on, names = bool(getattr(args, "uncertainty", False)), getattr(args, "uncertainty_maps", None)
    if not on:
        if names is not None:
            raise ValueError("--uncertainty_maps needs --uncertainty")
        return None
    if int(getattr(args, "num_GPUs", 1) or 1) > 1:
        raise ValueError("--uncertainty cannot be combined with --num_GPUs > 1: the plane-sharded predict keeps only the weighted sum "
                         "of the views per voxel, agreement and mutual information need every view at the voxel")
    if out_activation is not None and str(out_activation).lower() == "linear":
        raise ValueError("--uncertainty needs a model with out_activation: softmax: the vectors of an out_activation: linear model "
                         "are logits, not distributions")
    known = [n for n, _ in UNCERTAINTY_SUFFIX]
    if names is None:
        return tuple(known)
    asked = [n.strip() for n in str(names).split(",") if n.strip() != ""]
    for n in asked:
        if n not in known:
            raise ValueError("--uncertainty_maps: unknown map %r (known: %s)" % (n, ", ".join(known)))
    if not asked:
        raise ValueError("--uncertainty_maps: no map named")
    return tuple(n for n in known if n in asked)


def surface_metrics_plan(args):
    """The --surface_metrics flags, checked: None when the evaluation is off, else the NSD tolerance. ValueError on a combination
    that cannot be served."""
    on, tol = bool(getattr(args, "surface_metrics", False)), getattr(args, "nsd_tolerance", None)
    if not on:
        if tol is not None:
            raise ValueError("--nsd_tolerance needs --surface_metrics")
        return None
    if getattr(args, "no_eval", False):
        raise ValueError("--surface_metrics is an evaluation: it cannot be combined with --no_eval")
    if getattr(args, "no_argmax", False):
        raise ValueError("--surface_metrics evaluates a label map: it cannot be combined with --no_argmax")
    if getattr(args, "f", None) and not getattr(args, "l", None):
        raise ValueError("--surface_metrics needs labels: give -l with -f")
    tol = 1.0 if tol is None else float(tol)
    if not (tol > 0.0) or tol == float("inf"):
        raise ValueError("--nsd_tolerance must be finite and > 0, got %r" % (args.nsd_tolerance,))
    return tol


def component_filter_plan(args, n_classes=None):
    """The --largest_component flags, checked: None when the filter is off, else (connectivity, classes or None = all foreground
    classes). ValueError on a combination that cannot be served; with n_classes also on a class outside 1 .. n_classes - 1."""
    on = bool(getattr(args, "largest_component", False))
    conn, classes = getattr(args, "cc_connectivity", None), getattr(args, "cc_classes", None)
    if not on:
        if conn is not None or classes is not None:
            raise ValueError("--cc_connectivity / --cc_classes need --largest_component")
        return None
    if getattr(args, "no_argmax", False):
        raise ValueError("--largest_component filters a label map: it cannot be combined with --no_argmax (a probability volume is "
                         "not filtered)")
    if classes is not None:
        try:
            classes = sorted({int(c) for c in str(classes).split(",") if c.strip() != ""})
        except ValueError:
            raise ValueError("--cc_classes: expected comma-separated class numbers, got %r" % (args.cc_classes,))
        if not classes:
            raise ValueError("--cc_classes: no class named")
        if n_classes is not None and (classes[0] < 1 or classes[-1] > int(n_classes) - 1):
            raise ValueError("--cc_classes %s: classes must be in 1 .. n_classes - 1 = %d" % (args.cc_classes, int(n_classes) - 1))
    return (26 if conn is None else int(conn)), classes


CLEANUP_STAGES = ("open", "close", "fill_holes", "small_components")      # the order they run in


def cleanup_plan(args, n_classes=None):
    """The clean-up flags (--open_mm, --close_mm, --fill_holes, --min_component_voxels and what qualifies them), checked: None when
    none of the four is given, else a dict with open_mm / close_mm (a radius or None), hole_connectivity (None: no hole filling),
    min_voxels (None: no size threshold), clean_connectivity and classes (None = all foreground classes). ValueError on a
    combination that cannot be served; with n_classes also on a class outside 1 .. n_classes - 1."""
    g = lambda k: getattr(args, k, None)
    open_mm, close_mm, fill, min_voxels = g("open_mm"), g("close_mm"), bool(g("fill_holes")), g("min_component_voxels")
    if g("hole_connectivity") is not None and not fill:
        raise ValueError("--hole_connectivity needs --fill_holes")
    if g("clean_connectivity") is not None and min_voxels is None:
        raise ValueError("--clean_connectivity needs --min_component_voxels")
    classes = g("clean_classes")
    if open_mm is None and close_mm is None and not fill and min_voxels is None:
        if classes is not None:
            raise ValueError("--clean_classes needs at least one of --open_mm, --close_mm, --fill_holes, --min_component_voxels")
        return None
    if getattr(args, "no_argmax", False):
        raise ValueError("--open_mm / --close_mm / --fill_holes / --min_component_voxels clean a label map: they cannot be combined "
                         "with --no_argmax (a probability volume is not cleaned)")
    for flag, r in (("--open_mm", open_mm), ("--close_mm", close_mm)):
        if r is not None and (not (float(r) > 0.0) or float(r) == float("inf")):
            raise ValueError("%s must be finite and > 0, got %r" % (flag, r))
    if min_voxels is not None and int(min_voxels) < 1:
        raise ValueError("--min_component_voxels must be >= 1, got %r" % (min_voxels,))
    if classes is not None:
        try:
            classes = sorted({int(c) for c in str(classes).split(",") if c.strip() != ""})
        except ValueError:
            raise ValueError("--clean_classes: expected comma-separated class numbers, got %r" % (args.clean_classes,))
        if not classes:
            raise ValueError("--clean_classes: no class named")
        if n_classes is not None and (classes[0] < 1 or classes[-1] > int(n_classes) - 1):
            raise ValueError("--clean_classes %s: classes must be in 1 .. n_classes - 1 = %d" % (args.clean_classes, int(n_classes) - 1))
    return dict(open_mm=None if open_mm is None else float(open_mm), close_mm=None if close_mm is None else float(close_mm),
                hole_connectivity=(6 if g("hole_connectivity") is None else int(g("hole_connectivity"))) if fill else None,
                min_voxels=None if min_voxels is None else int(min_voxels),
                clean_connectivity=26 if g("clean_connectivity") is None else int(g("clean_connectivity")), classes=classes)


def run_cleanup(labels, plan, n_classes, spacing):
    """The stages of a cleanup_plan on a resident label map, in place, in the order of CLEANUP_STAGES: closing seals gaps so that
    holes become cavities, the size threshold then judges the repaired objects. -> [(stage, counts' names, table)] per stage run."""
    from .. import postprocess as PP
    K, cls, done = int(n_classes), plan["classes"], []
    if plan["open_mm"] is not None:
        _, t = PP.open_ball(labels, K, plan["open_mm"], spacing, classes=cls, out=labels, report=True)
        done.append(("open", ("voxels_added", "voxels_removed"), t))
    if plan["close_mm"] is not None:
        _, t = PP.close_ball(labels, K, plan["close_mm"], spacing, classes=cls, out=labels, report=True)
        done.append(("close", ("voxels_added", "voxels_removed"), t))
    if plan["hole_connectivity"] is not None:
        _, t = PP.fill_holes(labels, K, plan["hole_connectivity"], classes=cls, out=labels, report=True)
        done.append(("fill_holes", ("cavities", "voxels_filled"), t))
    if plan["min_voxels"] is not None:
        _, t = PP.remove_small_components(labels, K, plan["min_voxels"], plan["clean_connectivity"], classes=cls, out=labels, report=True)
        done.append(("small_components", ("components", "voxels_kept", "voxels_removed"), t))
    return done


def best_model_path(model_dir):
    """get_best_model (mpunet/utils/utils.py:88-110) over this build's .npz and the reference's .h5 checkpoints."""
    from ..formats import get_best_model
    return get_best_model(model_dir)


def plan_todo(items, dst_of, continue_, overwrite):
    """(items to predict, first conflicting output or None). What there is to do is settled from the FINAL output names alone, so
    that a volume whose output exists is never read; an output that exists without --overwrite / --continue stops the run where
    the loop reaches it. A temporary file a killed run left behind (prediction_writer.temp_path) is no output: its volume is
    predicted again and the file is overwritten. dst_of may give several names (--uncertainty: the maps beside the prediction):
    the volume is done when all of them exist, and any of them that exists is a conflict."""
    todo, conflict = [], None
    for item in items:
        dsts = dst_of(item)
        dsts = [dsts] if isinstance(dsts, str) else list(dsts)
        have = [d for d in dsts if os.path.exists(d)]
        if len(have) == len(dsts) and continue_:
            continue
        if have and not overwrite and not (continue_ and len(dsts) > 1):
            conflict = have[0]
            break
        todo.append(item)
    return todo, conflict


def run(args):
    from .. import distributed as D
    from ..unet import UNet
    from ..fusion_model import FusionModel
    from ..predict import multi_view_predict
    from ..interpolation import dice_all
    from ..data import load_volume_to_device, encoded_payload_to_host
    from ..nifti import volume_identifier
    from ..prediction_writer import PredictionWriter
    project_dir = os.path.abspath(args.project_dir)
    cc = component_filter_plan(args)                      # (flag combinations: refused before anything is looked at)
    sm = surface_metrics_plan(args)
    cl = cleanup_plan(args)
    unc = uncertainty_plan(args)
    validate_project_dir(project_dir)
    if unc is not None:                                   # the model's output against the maps' meaning, before anything is created
        unc = uncertainty_plan(args, load_hparams(project_dir)["build"].get("out_activation"))
    if cc is not None:                                    # the classes against the project's, before anything is loaded or created
        cc = component_filter_plan(args, load_hparams(project_dir)["build"]["n_classes"])
    if cl is not None:
        cl = cleanup_plan(args, load_hparams(project_dir)["build"]["n_classes"])
    for req in ("views.npz", "model"):
        if not os.path.exists(os.path.join(project_dir, req)):
            raise RuntimeError("Invalid project folder: needs train_hparams.yaml, views.npz and model/ (missing %s)" % req)
    if args.force_GPU:
        os.environ["HIP_VISIBLE_DEVICES"] = args.force_GPU
    rank, world, device = D.init_from_env()
    if unc is not None and world > 1:
        raise ValueError("--uncertainty cannot be combined with a sharded predict (%d ranks): agreement and mutual information need "
                         "every view at the voxel" % world)
    log = (lambda *a, **k: print(*a, flush=True)) if rank == 0 else (lambda *a, **k: None)
    hp = load_hparams(project_dir)
    fit, build = hp["fit"], hp["build"]
    lazy = False
    if args.f:
        vols = [load_volume_to_device(args.f, args.l, device, fit.get("bg_value"), fit.get("scaler"),
                                      volume_identifier(args.f), label_wins=True)]
    else:
        key = "val_data" if args.on_val else args.dataset.replace("_data", "") + "_data"
        if args.synthetic:
            vols = load_dataset(hp[key], project_dir, hp, device, args.synthetic, seed=5000, need_labels=False)
        else:                                             # files: nothing is read yet (bin/predict.py:394, a lazy queue)
            vols = dataset_entries(hp[key], project_dir, hp, device, need_labels=False)
            lazy = True
    if not vols:
        raise OSError("no volumes to predict on")
    require_audited_hparams(hp, "mp predict")             # geometry of the training session, never re-audited here
    views = np.load(os.path.join(project_dir, "views.npz"))["arr_0"]
    bkw = {k: v for k, v in build.items() if k != "model_class_name"}
    model = UNet(logger=log, dtype=args.dtype, device=device, **bkw)
    wpath = best_model_path(os.path.join(project_dir, "model"))
    model.load_weights(wpath, by_name=True)
    log("Loaded weights:", wpath)
    log("Back-mapping method:", args.map_method)
    fm = None
    if not args.sum_fusion:
        fm = FusionModel(len(views), build["n_classes"], verbose=False, device=device)
        fpath = fusion_weights_path(os.path.join(project_dir, "model"), wpath)
        if os.path.exists(fpath):
            fm.load_weights(fpath)
            log("Loaded fusion weights:", fpath)
        else:
            log("[OBS] no fusion weights for this checkpoint (%s): using the FusionLayer initialisation "
                "(W=1, b=0)" % os.path.basename(fpath))
    out_dir = os.path.join(project_dir, args.out_dir) if not os.path.isabs(args.out_dir) else args.out_dir
    nii = os.path.join(out_dir, "nii_files")
    if rank == 0:
        os.makedirs(nii, exist_ok=True)
    results, per_view, surface, cleanup, unc_rows = {}, {}, {}, [], {}

    def plan(item):
        """(write a NIfTI file?, output folder, output file) of a volume or a dataset entry."""
        src = str(getattr(item, "source_path", None) or getattr(item, "path", None) or "")
        as_nii = args.out_format == "nii" or (args.out_format == "auto" and src.endswith((".nii", ".nii.gz")))
        # bin/predict.py:90-117: with --save_input_files the prediction goes into a sub-folder <identifier>/ of nii_files,
        # next to <identifier>_IMAGE and <identifier>_LABELS
        out_base = os.path.join(nii, item.identifier) if args.save_input_files else nii
        return as_nii, out_base, os.path.join(out_base, "%s_PRED.%s" % (item.identifier, "nii.gz" if as_nii else "npz"))

    def unc_path(dst, suffix):
        """<id>_<SUFFIX>.nii.gz beside <id>_PRED.nii.gz"""
        return dst[:-len("PRED.nii.gz")] + suffix + ".nii.gz"

    def outputs(item):
        """Every file that makes up a volume's output: the prediction and, for NIfTI outputs, the --uncertainty maps beside it."""
        as_nii, _, dst = plan(item)
        if unc is None or not as_nii:
            return dst
        return [dst] + [unc_path(dst, suf) for name, suf in UNCERTAINTY_SUFFIX if name in unc]

    todo, conflict = plan_todo(vols, outputs, args.continue_, args.overwrite)
    if lazy:                                              # at most the current and the next volume are loaded
        from ..volume_queue import LazyQueue, Dataset
        todo = LazyQueue(Dataset(todo, key), logger=log)
    writer = PredictionWriter() if rank == 0 else None

    def put_nifti(path, t, affine):
        """Compute thread: encode on the device, one copy to the host, then the job for the writer's thread."""
        shape, dtype, payload = encoded_payload_to_host(t, path)
        writer.submit_nifti(path, shape, dtype, affine, payload)

    try:
        for v in todo:
            as_nii, out_base, dst = plan(v)
            if sm is not None and v.labels is None:
                raise ValueError("--surface_metrics needs labels: %s has none" % v.identifier)
            if world > 1:
                res = D.multi_view_predict_sharded(model, v, views, build["dim"], fit["real_space_span"], fm,
                                                   sum_fusion=args.sum_fusion, batch_size=None, want_probs=args.no_argmax,
                                                   map_method=args.map_method)
                probs, labels = res if args.no_argmax else (None, res)
            else:
                pve, umaps = None, (None if unc is None else {"maps": unc})
                if v.labels is not None and not args.no_eval:     # bin/predict.py:334-346: per-view Dice inside the loop
                    rows = per_view.setdefault(v.identifier, {})
                    pve = dict(eval_prob=args.eval_prob, n_classes=build["n_classes"], log=log,
                               report=lambda i, view, vd, md, mean, rows=rows: rows.__setitem__(i, (view, vd, md, float(mean))))
                probs, labels = multi_view_predict(model, v, views, build["dim"], fit["real_space_span"], fm,
                                                   sum_fusion=args.sum_fusion, batch_size=None,
                                                   want_probs=args.no_argmax, per_view_eval=pve, map_method=args.map_method,
                                                   **({} if umaps is None else {"uncertainty": umaps}))
            if rank == 0 and cl is not None:                  # open -> close -> fill holes -> size threshold, before the filter below
                from .. import surface as edt            # (the ball's spacing: the voxel sizes of the affine)
                labels = labels.contiguous()
                for stage, names, table in run_cleanup(labels, cl, build["n_classes"], edt.voxel_sizes(v.affine)):
                    for c in ([0] if stage == "fill_holes" else []) + list(cl["classes"] or range(1, build["n_classes"])):
                        log("%s: class %d: %s: %s" % (v.identifier, c, stage, ", ".join("%d %s" % (int(x), k.replace("_", " "))
                                                                                       for k, x in zip(names, table[c]))))
                        cleanup.append((v.identifier, c, stage, dict(zip(names, (int(x) for x in table[c])))))
            if rank == 0 and cc is not None:                  # the map that is evaluated, logged and saved from here on
                from ..postprocess import keep_largest_component
                labels = labels.contiguous()
                labels, table = keep_largest_component(labels, build["n_classes"], connectivity=cc[0], classes=cc[1], out=labels,
                                                       report=True)
                for c in (cc[1] if cc[1] is not None else range(1, build["n_classes"])):
                    log("%s: class %d: %d components found, %d voxels removed (largest component, %d-connectivity)"
                        % (v.identifier, c, int(table[c, 0]), int(table[c, 2]), cc[0]))
            if rank == 0 and args.save_input_files:
                sub = out_base                            # the volume as it was read: unscaled image, label map
                os.makedirs(sub, exist_ok=True)
                raw = v.image                             # (the volume as read: the scaler is applied by the sampling kernel)
                raw = raw.reshape(raw.shape[:3]) if raw.shape[-1] == 1 else raw
                if as_nii:
                    put_nifti(os.path.join(sub, "%s_IMAGE.nii.gz" % v.identifier), raw, v.affine)
                    if v.labels is not None:
                        put_nifti(os.path.join(sub, "%s_LABELS.nii.gz" % v.identifier), v.labels, v.affine)
                else:
                    writer.submit_npz(os.path.join(sub, "%s_IMAGE.npz" % v.identifier),
                                      {"image": raw.cpu().numpy(), "affine": v.affine})
                    if v.labels is not None:
                        writer.submit_npz(os.path.join(sub, "%s_LABELS.npz" % v.identifier),
                                          {"labels": v.labels.cpu().numpy().astype(np.uint8), "affine": v.affine})
            if rank == 0:
                if as_nii:                            # the label map, or with --no_argmax the fused [X,Y,Z,K] probabilities
                    put_nifti(dst, probs if (args.no_argmax and probs is not None) else labels, v.affine)
                else:
                    out = {"labels": labels.cpu().numpy(), "affine": v.affine}
                    if args.no_argmax and probs is not None:
                        out["probs"] = probs.cpu().numpy()
                    if unc is not None:                   # (properties of the fusion: clean-up and the filter do not alter them)
                        out.update({name: umaps[name].cpu().numpy() for name in unc})
                    writer.submit_npz(dst, out)
                if unc is not None:
                    from ..uncertainty import uncertainty_table
                    if as_nii:
                        for name, suf in UNCERTAINTY_SUFFIX:
                            if name in unc:
                                put_nifti(unc_path(dst, suf), umaps[name], v.affine)
                    # the map that was saved (after clean-up and the filter), against the labels when the volume has them
                    t = uncertainty_table(labels.contiguous(), {name: umaps[name] for name in unc}, build["n_classes"],
                                          truth=None if v.labels is None else v.labels.reshape(labels.shape).contiguous())
                    unc_rows[v.identifier] = t
                    log("%s: uncertainty per class: mean entropy %s mean mi %s mean agreement %s"
                        % (v.identifier, np.round(t["mean_entropy"], 4), np.round(t["mean_mi"], 4), np.round(t["mean_agreement"], 3)))
                if v.labels is not None and not args.no_eval:
                    d = dice_all(v.labels, labels, n_classes=build["n_classes"], ignore_zero=True)
                    results[v.identifier] = d
                    log("%s: dices %s mean %.4f" % (v.identifier, np.round(d, 4), float(np.nanmean(d))))
                if sm is not None:                        # the map that was saved against the labels, on the device
                    from ..surface import surface_distances, voxel_sizes
                    s = surface_distances(labels.contiguous(), v.labels.reshape(labels.shape).contiguous(), build["n_classes"],
                                          voxel_sizes(v.affine), tolerance=sm)
                    surface[v.identifier] = s
                    log("%s: surface distances (tolerance %g): hd95 %s assd %s nsd %s"
                        % (v.identifier, sm, np.round(s["hd95"][1:], 4), np.round(s["assd"][1:], 4), np.round(s["nsd"][1:], 4)))
    except BaseException:
        if writer is not None:                            # (this error wins; what was queued is still written, completely)
            try:
                writer.close()
            except OSError:
                pass
        raise
    if writer is not None:
        writer.close()                                    # every file is complete from here on; a write failure is raised here
    if conflict is not None:
        raise OSError("%s exists (use --overwrite or --continue)" % conflict)
    if rank == 0 and results:
        os.makedirs(os.path.join(out_dir, "csv"), exist_ok=True)
        with open(os.path.join(out_dir, "csv", "results.csv"), "w") as f:
            f.write("image,mean_dice," + ",".join("class_%d" % (c + 1) for c in range(build["n_classes"] - 1)) + "\n")
            for k, d in results.items():
                f.write("%s,%.5f,%s\n" % (k, float(np.nanmean(d)), ",".join("%.5f" % x for x in d)))
        if any(per_view.values()):                      # one row per (image, evaluated view): mean + per-class mapped Dice
            with open(os.path.join(out_dir, "csv", "per_view.csv"), "w") as f:
                f.write("image,view_index,view,mean_dice," + ",".join("class_%d" % c for c in range(build["n_classes"])) + "\n")
                for k, rows in per_view.items():
                    for i in sorted(rows):
                        view, _, md, mean = rows[i]
                        f.write("%s,%d,%s,%.5f,%s\n" % (k, i, " ".join("%.6g" % x for x in np.asarray(view).ravel()), mean,
                                                        ",".join("%.5f" % x for x in md)))
    if rank == 0 and cleanup:                           # one row per (image, class, stage); class 0 of fill_holes: left unfilled
        os.makedirs(os.path.join(out_dir, "csv"), exist_ok=True)
        cols = ("voxels_added", "voxels_removed", "cavities", "voxels_filled", "components", "voxels_kept")
        with open(os.path.join(out_dir, "csv", "cleanup_results.csv"), "w") as f:
            f.write("image,class,stage," + ",".join(cols) + "\n")
            for ident, c, stage, counts in cleanup:
                f.write("%s,%d,%s,%s\n" % (ident, c, stage, ",".join(str(counts.get(k, "")) for k in cols)))
    if rank == 0 and surface:                           # one row per (image, foreground class)
        os.makedirs(os.path.join(out_dir, "csv"), exist_ok=True)
        with open(os.path.join(out_dir, "csv", "surface_results.csv"), "w") as f:
            f.write("image,class,hd,hd95,assd,nsd,n_pred_border,n_truth_border\n")
            for k, s in surface.items():
                for c in range(1, build["n_classes"]):
                    f.write("%s,%d,%.6f,%.6f,%.6f,%.6f,%d,%d\n" % (k, c, s["hd"][c], s["hd95"][c], s["assd"][c], s["nsd"][c],
                                                                   int(s["n_pred_border"][c]), int(s["n_truth_border"][c])))
    if rank == 0 and unc_rows:                          # one row per (image, class of the saved map); _correct / _wrong: with labels
        os.makedirs(os.path.join(out_dir, "csv"), exist_ok=True)
        cols = ["n", "mean_entropy", "mean_mi", "mean_agreement"]
        cols = cols + [c + g for g in ("_correct", "_wrong") for c in cols]
        with open(os.path.join(out_dir, "csv", "uncertainty_results.csv"), "w") as f:
            f.write("image,class," + ",".join(cols) + "\n")
            for k, t in unc_rows.items():
                for c in range(build["n_classes"]):
                    f.write("%s,%d,%s\n" % (k, c, ",".join("" if col not in t else ("%.6f" if col.startswith("mean_") else "%d") % t[col][c]
                                                            for col in cols)))
    return results


def entry_func(args=None):
    import sys
    argv = list(sys.argv[1:] if args is None else args)
    args = get_argparser().parse_args(argv)
    from .common import relaunch_per_gpu, await_pids
    if args.wait_for and "RANK" not in os.environ:        # (once, in the launching process: utils.py:337-375)
        await_pids(args.wait_for)
    uncertainty_plan(args)                               # (--num_GPUs N > 1 is refused here, before any process is started)
    relaunch_per_gpu("predict", argv, args.num_GPUs)     # --num_GPUs N > 1: one process per GPU (returns inside a torchrun job)
    run(args)


if __name__ == "__main__":
    entry_func()
