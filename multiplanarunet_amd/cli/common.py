"""Shared pieces of the `mp train` / `mp predict` shims: YAML hyper-parameters, views, datasets."""
import os
import numpy as np
import yaml

from ..data import (list_volume_files, load_label_file, as_volume, make_toy_volume, random_views, audit_dim_and_span)
from ..nifti import volume_identifier

DEFAULT_HPARAMS = {
    "train_data": {"base_dir": None, "img_subdir": "images", "label_subdir": "labels", "bg_class": 0},
    "val_data": {"base_dir": None, "img_subdir": "images", "label_subdir": "labels", "bg_class": 0},
    "test_data": {"base_dir": None, "img_subdir": "images", "label_subdir": "labels", "bg_class": 0},
    "build": {"model_class_name": "UNet", "n_classes": None, "n_channels": None, "dim": None,
              "complexity_factor": 2, "out_activation": "softmax", "l1_reg": False, "l2_reg": False,
              "biased_output_layer": True, "depth": 4},
    "fit": {"views": 6, "noise_sd": 0.1, "real_space_span": None, "intrp_style": "iso_live",
            "loss": "SparseCategoricalCrossentropy", "loss_kwargs": {}, "metrics": ["sparse_categorical_accuracy"],
            "batch_size": 16, "n_epochs": 500, "optimizer": "Adam",
            "optimizer_kwargs": {"lr": 5.0e-05, "decay": 0.0, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1.0e-8},
            "fg_batch_fraction": 0.50, "bg_value": "1pct", "scaler": "RobustScaler"},
}


def validate_project_dir(project_dir):
    if not os.path.exists(project_dir) or not os.path.exists(os.path.join(project_dir, "train_hparams.yaml")):
        raise RuntimeError("The script was launched from directory:\n'%s'\n... but this is not a valid project "
                           "folder (no 'train_hparams.yaml')." % project_dir)


def load_hparams(project_dir):
    """train_hparams.yaml with the reference's sections (bin/defaults/MultiPlanar/train_hparams.yaml)."""
    with open(os.path.join(project_dir, "train_hparams.yaml")) as f:
        raw = yaml.safe_load(f) or {}
    hp = {k: dict(v) for k, v in DEFAULT_HPARAMS.items()}
    for sec, vals in raw.items():
        if sec.startswith("__"):                               # the YAML's anchor sections (__CB_*, ...)
            continue
        if isinstance(vals, dict):
            hp.setdefault(sec, {}).update(vals)
        else:                                                  # top-level scalars / lists, e.g. `class_counts: [..]`
            hp[sec] = vals                                     #   (read by set_bias_weights_on_all_outputs)
    return hp


def validate_output_loss(hp):
    """build.out_activation against fit.loss / fit.loss_kwargs, before `mp train` creates anything: a linear output trains only
    with the cross-entropy from logits (bin/train.py:130 names that configuration), and from_logits on a softmax output is
    refused with UNet.compile's own error."""
    from ..unet import resolve_ce_kwargs
    fit, act = hp["fit"], hp["build"].get("out_activation", "softmax")
    loss = fit["loss"][0] if isinstance(fit["loss"], (list, tuple)) and len(fit["loss"]) == 1 else fit["loss"]
    if not (isinstance(loss, str) and "sparsecategoricalcrossentropy" in loss.lower().replace("_", "")):
        return
    from_logits = resolve_ce_kwargs(fit.get("loss_kwargs"), act)
    if act == "linear" and not from_logits:
        raise ValueError("build.out_activation: linear trains only with the cross-entropy from logits: add "
                         "fit.loss_kwargs: {from_logits: true} to train_hparams.yaml (or build a softmax output)")


def load_dataset(cfg, project_dir, hp, device, synthetic=0, seed=0, need_labels=True):
    """List of Volume objects for one of train_data / val_data / test_data (or synthetic toy volumes)."""
    fit = hp["fit"]
    vols = []
    if synthetic:
        for i in range(synthetic):
            img, lab, aff = make_toy_volume(64, seed + i)
            vols.append(as_volume(img, lab, aff, fit.get("bg_value"), fit.get("scaler"), device, "toy_%d" % (seed + i)))
        return vols
    for path, lp in list_dataset_entries(cfg, project_dir):
        vols.append(load_entry(path, lp, hp, device, need_labels))
    return vols


def list_dataset_entries(cfg, project_dir):
    """[(image path, label path or None), ...] of one of train_data / val_data / test_data: the files only, nothing is read."""
    base = cfg.get("base_dir")
    if not base:
        return []
    if not os.path.isabs(base):
        base = os.path.join(project_dir, base)
    out = []
    for path in list_volume_files(base, cfg.get("img_subdir", "images")):
        lp = os.path.join(base, cfg.get("label_subdir", "labels"), os.path.basename(path))
        out.append((path, lp if os.path.exists(lp) else None))
    return out


def check_has_labels(payload, need_labels):
    if payload.labels is None and need_labels:
        raise ValueError("no labels for %s" % payload.path)
    return payload


def load_entry(path, label_path, hp, device, need_labels=True):
    """One resident Volume of a dataset entry (data.load_volume_to_device: NIfTI files are decoded on the device)."""
    import torch
    from ..data import read_volume_host, adopt_payload
    fit = hp["fit"]
    payload = check_has_labels(read_volume_host(path, label_path, raw_nifti=torch.device(device).type == "cuda"), need_labels)
    return adopt_payload(payload, device, fit.get("bg_value"), fit.get("scaler"), volume_identifier(path))


def dataset_entries(cfg, project_dir, hp, device, synthetic=0, seed=0, need_labels=True):
    """The set load_dataset would load, as volume_queue.VolumeEntry objects: nothing is read yet. An entry's loader does file
    work only (a loader thread may run it); its adopter makes the resident Volume on the calling thread's stream."""
    import torch
    from ..volume_queue import VolumeEntry
    from ..data import read_volume_host, adopt_payload, HostPayload
    fit = hp["fit"]
    raw = torch.device(device).type == "cuda"

    def adopt(e, payload):
        return adopt_payload(payload, device, fit.get("bg_value"), fit.get("scaler"), e.identifier)

    if synthetic:
        def toy(i):
            def load(e):
                img, lab, aff = make_toy_volume(64, seed + i)
                return HostPayload(None, None, ("host", img), ("host", lab), aff)
            return load
        return [VolumeEntry(None, None, "toy_%d" % (seed + i), toy(i), adopt) for i in range(synthetic)]

    def load(e):
        return check_has_labels(read_volume_host(e.path, e.label_path, raw_nifti=raw), need_labels)
    return [VolumeEntry(p, lp, volume_identifier(p), load, adopt) for p, lp in list_dataset_entries(cfg, project_dir)]


def fill_build_from_entries(hp, entries, max_label_files=50):
    """fill_build_from_data without resident volumes: shape, affine and channel count come from the NIfTI HEADERS; an entry
    without one (.npz, a generated volume, a NIfTI file of a rank the header audit does not take) is loaded on the host, looked
    at and dropped, one at a time. build.n_classes, when the YAML leaves it open, is audited from at most 50 label files read
    one at a time (auditor._audit_classes; here the largest label + 1, the rule of fill_build_from_data)."""
    from types import SimpleNamespace
    from ..nifti import read_nifti_header

    def host_payload(e):
        e.load_host()
        p, e.payload = e.payload, None
        return p

    infos = []
    for e in entries:
        shape = aff = None
        if e.path and str(e.path).endswith((".nii", ".nii.gz")):
            h, aff = read_nifti_header(e.path)
            shape = tuple(h["shape"]) if len(h["shape"]) in (3, 4) else None
        if shape is None:
            p = host_payload(e)
            shape, aff = tuple(p.image[1].shape), p.affine
        shape4 = tuple(int(s) for s in shape) + (1,) * (4 - len(shape))
        infos.append(SimpleNamespace(affine=np.asarray(aff, np.float64), image=np.broadcast_to(np.float32(0), shape4),
                                     n_channels=shape4[3], labels=None))
    n_classes = None
    if not hp["build"].get("n_classes"):
        labelled = [e for e in entries if e.label_path or not e.path or str(e.path).endswith(".npz")]
        pick = np.random.RandomState(0).choice(len(labelled), min(int(max_label_files), len(labelled)), replace=False) \
            if labelled else []
        top = []
        for i in sorted(int(k) for k in pick):
            e = labelled[i]
            if e.label_path:
                lab = load_label_file(e.label_path)
            else:
                p = host_payload(e)
                lab = None if p.labels is None else p.labels[1]
            if lab is not None:
                top.append(int(np.asarray(lab).max()))
        n_classes = max(top) + 1 if top else None
    return fill_build_from_data(hp, infos, n_classes=n_classes)


def load_or_create_views(project_dir, n_views, seed=None):
    """views.npz (key arr_0, shape [V,3]) as data_preparation_funcs.py:116-154 persists it."""
    path = os.path.join(project_dir, "views.npz")
    if os.path.exists(path):
        return np.load(path)["arr_0"]
    views = random_views(int(n_views), 60.0, seed)
    np.savez(path, views)
    return views


def fill_build_from_data(hp, volumes, n_classes=None):
    """What Auditor.fill writes back into the YAML: dim, real_space_span, n_channels, n_classes
    (mpunet/image/auditor.py:100-120,199-209). Call on the FULL training set (before --just_one truncation)."""
    b, f = hp["build"], hp["fit"]
    dim, span = audit_dim_and_span(volumes, min_dim=32)
    if not b.get("dim"):
        b["dim"] = dim
    if not f.get("real_space_span"):
        f["real_space_span"] = span
    if not b.get("n_channels"):
        b["n_channels"] = volumes[0].n_channels
    if not b.get("n_classes"):
        labelled = [int(v.labels.max().item()) for v in volumes if v.labels is not None]
        if n_classes is None and not labelled:
            raise ValueError("build.n_classes is not set and no labelled volume is available to audit it from")
        b["n_classes"] = n_classes or max(labelled) + 1
    return hp


AUDITED_KEYS = (("build", "dim"), ("build", "n_channels"), ("build", "n_classes"), ("fit", "real_space_span"))


def _patch_yaml_value(text, sec, key, val):
    """Set `sec.key` in the YAML TEXT, touching only that line (comments, anchors and layout of the rest survive, as
    with the reference's YAMLHParams.set_value, mpunet/hyperparameters/hparams.py:161-221). Works on the block style
    the project YAMLs use (top-level `sec:` line, indented `key: value` lines)."""
    import re
    lines = text.split("\n")
    start = next((i for i, l in enumerate(lines) if re.match(r"^%s\s*:" % re.escape(sec), l)), None)
    if start is None:                                   # section missing: append it
        return text.rstrip("\n") + "\n\n%s:\n  %s: %s\n" % (sec, key, val)
    end = start + 1
    while end < len(lines) and (not lines[end].strip() or lines[end][:1] in " \t#"):
        end += 1
    if re.match(r"^%s\s*:\s*[^\s#]" % re.escape(sec), lines[start]):
        raise ValueError("section %r is not in block style" % sec)          # `build: {dim: 2}`: the caller rewrites the file
    # only keys at the section's FIRST indentation level (a deeper mapping may hold a key of the same name)
    ind = next((re.match(r"^(\s+)", lines[i]).group(1) for i in range(start + 1, end)
                if lines[i].strip() and not lines[i].lstrip().startswith("#")), "  ")
    pat = re.compile(r"^(%s)%s\s*:\s*([^#]*?)(\s*#.*)?$" % (re.escape(ind), re.escape(key)))
    for i in range(start + 1, end):
        mt = pat.match(lines[i])
        if mt:
            lines[i] = "%s%s: %s%s" % (mt.group(1), key, val, mt.group(3) or "")
            return "\n".join(lines)
    last = end - 1                                      # key missing: add it behind the section's last entry
    while last > start and not lines[last].strip():
        last -= 1
    lines.insert(last + 1, "%s%s: %s" % (ind, key, val))
    return "\n".join(lines)


def save_audited_hparams(project_dir, hp):
    """Write the audited values back into train_hparams.yaml (the reference's Auditor.fill +
    YAMLHParams.save_current, mpunet/bin/train.py:210-228), so that `mp predict` / `mp train_fusion` use the
    geometry the model was trained with instead of re-auditing whatever volumes they are given. Only the audited
    lines are patched in the text: the user's comments and formatting are kept."""
    path = os.path.join(project_dir, "train_hparams.yaml")
    with open(path) as f:
        text = f.read()
    raw = yaml.safe_load(text) or {}
    changed = False
    for sec, key in AUDITED_KEYS:
        val = hp[sec].get(key)
        if val is None:
            continue
        val = float(val) if key == "real_space_span" else int(val)
        cur = raw.get(sec) if isinstance(raw.get(sec), dict) else {}
        if cur.get(key) != val:
            changed = True
            if text is not None:
                try:
                    text = _patch_yaml_value(text, sec, key, repr(val))
                except ValueError:
                    text = None                         # layout the line patcher does not handle: rewrite below
            if not isinstance(raw.get(sec), dict):
                raw[sec] = {}
            raw[sec][key] = val
    if changed:
        def parses_back(t):                             # the new text must parse back to the audited values
            try:
                check = yaml.safe_load(t) or {}
                return all(hp[sec].get(key) is None or
                           float(((check.get(sec) if isinstance(check.get(sec), dict) else None) or {}).get(key, "nan")) ==
                           float(hp[sec][key]) for sec, key in AUDITED_KEYS)
            except (yaml.YAMLError, TypeError, ValueError):
                return False
        if text is None or not parses_back(text):
            # flow-style or otherwise unusual layout: fall back to a full rewrite (comments are lost, values are right)
            text = yaml.safe_dump(raw, default_flow_style=False, sort_keys=False)
            if not parses_back(text):
                raise RuntimeError("could not write the audited hyper-parameters into %s" % path)
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            f.write(text)
        os.replace(tmp, path)
    return changed


def require_audited_hparams(hp, what):
    """`mp predict` / `mp train_fusion`: the model geometry must come from the training session's YAML."""
    missing = ["%s.%s" % (sec, key) for sec, key in AUDITED_KEYS if not hp[sec].get(key)]
    if missing:
        raise RuntimeError("%s: train_hparams.yaml lacks %s -- these are written by `mp train` (Auditor); "
                           "run it first or set them by hand. Re-auditing the volumes given here could silently "
                           "change the sampling geometry the weights were trained with." % (what, ", ".join(missing)))


def fusion_weights_path(model_dir, weights_path):
    """<model>/fusion_weights/<checkpoint name>_fusion_weights.npz (mpunet/bin/predict.py:222-229,
    mpunet/bin/train_fusion.py:318-325): fusion weights belong to ONE U-Net checkpoint."""
    base = os.path.splitext(os.path.basename(weights_path))[0]
    return os.path.join(model_dir, "fusion_weights", "%s_fusion_weights.npz" % base)


# ---- output-layer bias from class frequencies (mpunet/bin/train.py:293-299, mpunet/utils/utils.py:179-241) ----------

def class_counts_from_volumes(volumes, n_classes):
    """np.bincount(labels.ravel(), minlength=n_classes) summed over the loaded training volumes (the reference counts
    once per image in the loading queue, utils.py:224-233; with every volume resident that is each volume once)."""
    import torch
    counts = np.zeros(int(n_classes), dtype=np.int64)
    for v in volumes:
        lab = getattr(v, "labels", None)
        if lab is None:
            continue
        if isinstance(lab, torch.Tensor):
            c = torch.bincount(lab.reshape(-1).to(torch.int64), minlength=int(n_classes)).cpu().numpy()
        else:
            c = np.bincount(np.asarray(lab).ravel().astype(np.int64), minlength=int(n_classes))
        if c.size > counts.size:                       # labels beyond n_classes: np.bincount grows, as in the reference
            counts = np.concatenate([counts, np.zeros(c.size - counts.size, np.int64)])
        counts[:c.size] += c
    return counts


def set_bias_weights(layer, class_counts, logger=None):
    """The reference's set_bias_weights (utils.py:204-241) on the object `model.layers[-1]` returns:
    freq = counts / sum(counts); bias = log(freq * sum(exp(freq))); bias /= ||bias||_2."""
    if layer.activation.__name__ != "softmax":
        raise ValueError("Setting output layer bias currently only supported with softmax activation functions. "
                         "Output layer has '%s'" % layer.activation.__name__)
    weights = layer.get_weights()
    if len(weights) != 2:
        raise ValueError("Output layer does not have bias weights.")
    bias_shape = weights[-1].shape
    counts = np.asarray(class_counts, dtype=np.float64)
    if counts.size != weights[-1].size:
        raise ValueError("class_counts has %d entries, the output layer %d classes" % (counts.size, weights[-1].size))
    with np.errstate(divide="ignore"):
        freq = np.asarray(counts / np.sum(counts))
        bias = np.log(freq * np.sum(np.exp(freq)))
    bias /= np.linalg.norm(bias)
    weights[-1] = bias.reshape(bias_shape).astype(weights[-1].dtype)
    layer.set_weights(weights)
    (logger or print)("Setting bias weights on output layer to:\n%s" % bias)
    return bias


def set_bias_weights_on_all_outputs(model, volumes, hparams, logger=None):
    """bin/train.py:293-299: last layer that has an activation (here: the 1x1 head shim), counts from
    hparams['class_counts'] (top-level YAML key) or estimated from the training volumes."""
    layer = next((l for l in model.layers[::-1] if hasattr(l, "activation")), None)
    if layer is None:
        raise ValueError("model has no output layer with an activation")
    counts = hparams.get("class_counts")
    if counts is None and hasattr(volumes, "max_loaded"):
        # a limitation queue: one count per image currently in the queue (utils.py:222-231) -- max_loaded draws from its FIFO,
        # which visit every preloaded volume once; the preload is the same on every rank (the queue's shared seed)
        (logger or print)("OBS: Estimating class counts from %d images" % volumes.max_loaded)
        counts = np.zeros(int(model.n_classes), dtype=np.int64)
        for _ in range(volumes.max_loaded):
            with volumes.get_random_image() as vol:
                c = class_counts_from_volumes([vol], model.n_classes)
            if c.size > counts.size:
                counts = np.concatenate([counts, np.zeros(c.size - counts.size, np.int64)])
            counts[:c.size] += c
    elif counts is None:
        volumes = getattr(volumes, "volumes", volumes)          # (an eager queue: its list)
        (logger or print)("OBS: Estimating class counts from %d images" % len(volumes))
        counts = class_counts_from_volumes(volumes, model.n_classes)
    return set_bias_weights(layer, counts, logger)


# ---- callbacks from the YAML `fit.callbacks` list (bin/defaults/MultiPlanar/train_hparams.yaml:7-45,139) -------------

DEFAULT_CALLBACKS = [
    {"nickname": "rlop", "class_name": "ReduceLROnPlateau",
     "kwargs": {"patience": 2, "factor": 0.90, "verbose": 1, "monitor": "val_dice", "mode": "max"}},
    {"nickname": "mcp_clean", "class_name": "ModelCheckPointClean",
     "kwargs": {"filepath": "./model/@epoch_{epoch:02d}_val_dice_{val_dice:.5f}.h5", "monitor": "val_dice",
                "save_best_only": True, "save_weights_only": True, "verbose": 1, "mode": "max"}},
    {"nickname": "es", "class_name": "EarlyStopping",
     "kwargs": {"monitor": "val_dice", "min_delta": 0, "patience": 15, "verbose": 1, "mode": "max"}},
    {"nickname": "csv", "class_name": "CSVLogger", "kwargs": {"filename": "logs/training.csv", "separator": ",", "append": True}},
]


def init_callback_objects(callbacks, project_dir, logger=None, have_h5py=None):
    """mpunet/callbacks/funcs.py:5-56 for the callbacks this path implements: the YAML descriptors
    {class_name, kwargs[, start_from]} become objects with on_epoch_end(model, epoch, logs). ReduceLROnPlateau,
    EarlyStopping, ModelCheckPointClean and CSVLogger honour their kwargs; descriptors of classes outside the hot path
    (TensorBoard, TrainTimer, ...) are reported and skipped. Returns (objects in list order, {class_name: object}).
    Relative paths are relative to the project folder (the reference chdirs into it, bin/train.py:330)."""
    from .. import validation as V
    log = logger or print
    if have_h5py is None:                       # can this host write Keras .h5 files (h5py, or libhdf5 through hdf5.py)?
        from ..formats import _h5_backend
        try:
            _h5_backend()
            have_h5py = True
        except ImportError:
            have_h5py = False
    objs, by_name = [], {}
    for i, cb in enumerate(callbacks if callbacks is not None else DEFAULT_CALLBACKS):
        if not isinstance(cb, dict):
            objs.append(cb); by_name[cb.__class__.__name__] = cb
            continue
        name, kw = cb["class_name"], dict(cb.get("kwargs") or {})
        if name == "ReduceLROnPlateau":
            ok = ("monitor", "factor", "patience", "mode", "min_delta", "cooldown", "min_lr", "verbose")
            obj = V.ReduceLROnPlateau(logger=log, **{k: kw[k] for k in ok if k in kw})
        elif name == "EarlyStopping":
            ok = ("monitor", "min_delta", "patience", "mode", "verbose")
            obj = V.EarlyStopping(logger=log, **{k: kw[k] for k in ok if k in kw})
        elif name in ("ModelCheckPointClean", "ModelCheckpoint"):
            path = kw.get("filepath", DEFAULT_CALLBACKS[1]["kwargs"]["filepath"])
            if not os.path.isabs(path):
                path = os.path.normpath(os.path.join(project_dir, path))
            if path.endswith((".h5", ".hdf5")) and not have_h5py:
                path = os.path.splitext(path)[0] + ".npz"          # neither h5py nor libhdf5 here: the .npz mirror (formats.py)
            obj = V.ModelCheckPointClean(path, monitor=kw.get("monitor", "val_dice"), mode=kw.get("mode", "max"),
                                         verbose=kw.get("verbose", 1), logger=log)
        elif name == "CSVLogger":
            path = kw.get("filename", "logs/training.csv")
            if not os.path.isabs(path):
                path = os.path.normpath(os.path.join(project_dir, path))
            obj = V.CSVLogger(path, separator=kw.get("separator", ","), append=bool(kw.get("append", False)))
        else:
            log("[%i] Skipping callback %s (outside the accelerated path)" % (i + 1, name))
            continue
        if cb.get("start_from"):
            log("OBS: '%s' activates at epoch %i" % (name, cb["start_from"]))
            obj = V.DelayedCallback(obj, int(cb["start_from"]), logger=log)
        objs.append(obj); by_name[name] = obj
        log("[%i] Using callback: %s(%s)" % (i + 1, name, ", ".join("%s=%s" % kv for kv in kw.items())))
    return objs, by_name


def remove_validation_callbacks(callbacks, logger=None):
    """funcs.py:59-82 (--no_val): drop descriptors whose kwargs mention 'val'. (The reference pops while it enumerates
    and therefore skips the entry behind each removed one; here every val-dependent descriptor goes.)"""
    keep = []
    for cb in callbacks:
        if isinstance(cb, dict) and any("val" in str(p).lower() for p in (cb.get("kwargs") or {}).values()):
            if logger:
                logger("Removing callback with parameters: %s (needs validation data)" % cb)
            continue
        keep.append(cb)
    return keep


def await_pids(pids, check_every=120, logger=print, sleep=None):
    """`--wait_for PID[,PID...]` (mpunet/utils/utils.py:337-375): return when none of the processes is running any more; the
    process table is looked at every `check_every` seconds. A PID that is not an integer is a ValueError, as there."""
    import time
    if not pids:
        return
    for tok in str(pids).split(","):
        tok = tok.strip()
        if not tok:
            continue
        try:
            pid = int(tok)
        except ValueError as e:
            raise ValueError("Cannot wait for PID '%s', must be an integer" % tok) from e
        while _pid_running(pid):
            logger("Process %i is still running... (sleeping %i seconds)" % (pid, check_every))
            (sleep or time.sleep)(check_every)


def _pid_running(pid):
    try:
        os.kill(pid, 0)                                    # signal 0: existence / permission check only
    except ProcessLookupError:
        return False
    except PermissionError:
        return True                                        # exists, owned by someone else
    try:                                                   # a zombie is in the table but no longer running
        with open("/proc/%d/stat" % pid) as f:
            return f.read().rsplit(")", 1)[1].split()[0] != "Z"
    except OSError:
        return True


def note_inert_flags(args, names, logger=print):
    """Flags of the reference's parser that are accepted for command-line compatibility but steer subsystems outside this build
    (image queues, TensorBoard images, the TF debugger, per-view evaluation): say so instead of ignoring them silently."""
    for name, why in names:
        val = getattr(args, name, None)
        if val not in (None, False, "", 0) and not (name == "eval_prob" and float(val) == 1.0) and not (name == "num_access" and int(val) == 50):
            logger("[OBS] --%s has no effect in this build (%s)" % (name, why))


def per_gpu_launch_command(script, argv, num_gpus, port=None):
    """`mp <script> --num_GPUs N` in the reference is ONE process driving N GPUs (tf.distribute.MirroredStrategy,
    mpunet/bin/train.py:349, bin/predict.py:214); here it is one process per GPU over RCCL. The command that re-runs the same
    script under torch.distributed.run on this node (rendezvous on 127.0.0.1: the host name of a container may not resolve)."""
    import socket
    import sys
    if port is None:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(num_gpus)),
            "--master-addr", "127.0.0.1", "--master-port", str(int(port)), "-m", "multiplanarunet_amd.cli.mp", script] + list(argv)


def relaunch_per_gpu(script, argv, num_gpus):
    """Called by the scripts' entry points: --num_GPUs N > 1 outside a torchrun job re-launches the script as N ranks and exits
    with their status; inside one (WORLD_SIZE set) or with N <= 1 it returns and the caller carries on."""
    import subprocess
    if int(num_gpus) <= 1 or "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(per_gpu_launch_command(script, argv, num_gpus), env=env))

