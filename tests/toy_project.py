"""A 32^3 toy project folder for CLI tests (test aid; imported like guarded.py): int16 .nii.gz volumes as in
test_gpu_volume_queue.py, a depth-2 U-Net of dim 32 with freshly initialised weights (nothing is trained: the tests that use it
compare outputs with what the same weights give), 3 views, and a train_hparams.yaml that carries the audited geometry."""
import os

import numpy as np

YAML = ("train_data:\n  base_dir: data/train\nval_data:\n  base_dir: data/val\ntest_data:\n  base_dir: data/test\n"
        "build:\n  model_class_name: UNet\n  n_classes: 3\n  n_channels: 1\n  dim: 32\n  depth: 2\n"
        "  complexity_factor: 0.0625\n  out_activation: softmax\n  seed: 0\n"
        "fit:\n  views: 3\n  noise_sd: 0.1\n  real_space_span: 32.0\n  batch_size: 4\n  n_epochs: 2\n"
        "  optimizer: Adam\n  optimizer_kwargs: {lr: 1.0e-3, decay: 0.0, beta_1: 0.9, beta_2: 0.999, epsilon: 1.0e-8}\n"
        "  loss: SparseCategoricalCrossentropy\n  fg_batch_fraction: 0.5\n  bg_value: 1pct\n  scaler: RobustScaler\n")


def write_set(folder, n, seed):
    from multiplanarunet_amd.data import make_toy_volume
    from multiplanarunet_amd.formats import save_nifti
    os.makedirs(os.path.join(folder, "images"))
    os.makedirs(os.path.join(folder, "labels"))
    for i in range(n):
        img, lab, aff = make_toy_volume(32, seed + i)
        aff = aff.copy()
        aff[:3, 3] = (-3.0, 4.0, 5.0 + i)                      # (an affine that is not the identity: it is written into the headers)
        save_nifti(os.path.join(folder, "images", "vol_%d.nii.gz" % (seed + i)), np.round(img[..., 0] * 1000).astype(np.int16), aff)
        save_nifti(os.path.join(folder, "labels", "vol_%d.nii.gz" % (seed + i)), lab, aff)


def make_project(proj, n_train=4, n_val=3, n_test=3):
    """-> (hparams, views). `proj`: an empty folder (a pathlib.Path)."""
    from multiplanarunet_amd.cli import common
    from multiplanarunet_amd.data import random_views
    from multiplanarunet_amd.unet import UNet
    (proj / "train_hparams.yaml").write_text(YAML)
    write_set(str(proj / "data" / "train"), n_train, 0)
    write_set(str(proj / "data" / "val"), n_val, 1000)
    write_set(str(proj / "data" / "test"), n_test, 5000)
    views = random_views(3, 60.0, 0)
    np.savez(str(proj / "views.npz"), views)
    hp = common.load_hparams(str(proj))
    os.makedirs(str(proj / "model"))
    load_model(hp).save_weights(str(proj / "model" / "model_weights.npz"))
    return hp, views


def load_model(hp, weights=None):
    from multiplanarunet_amd.unet import UNet
    model = UNet(logger=lambda *a, **k: None, dtype="bf16", device="cuda",
                 **{k: v for k, v in hp["build"].items() if k != "model_class_name"})
    if weights:
        model.load_weights(weights, by_name=True)
    return model
