"""
Writes tests/golden/map_linear_golden.npz and map_linear_golden_rot.npz: what the reference's own map_real_space_pred(..., method="linear")
(mpunet/utils/fusion/fuse_and_predict.py:92-137, unmodified, imported through oracle/ref_shim.py) returns on inputs that
tests/golden/geometry_golden.npz already holds. Run by hand on the CPU where the reference is installed:
    python tests/golden/make_map_linear_golden.py

Inputs (read from geometry_golden.npz, not stored again): the random predictions g5_pred_<affine>_<view>_<K> [16,16,36,K],
the view's axes g3_g_/g3_off_<affine>_16_<view>, its inverse basis g3_invb_<affine>_16_<view> and the voxel grid
g4_vgrid_<affine> [3,32,28,24].
Outputs: lin_map_<affine>_<view>_<K> f32 [32,28,24,K] for K = 3 on the three affines x views {0, 6} and K in {1, 5} on
(rot, view 6): eight arrays, the four of the `rot` affine in the second file (random floats do not compress: one file
would exceed the size limit for a committed file). The other 28 (affine, view, K) cases of geometry_golden.npz are covered by the oracle
composition (oracle.geometry.rgi_linear per class + fill + f32 cast) that tests/test_map_linear_host.py ties to these eight.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CASES = [(an, v, 3) for an in ("ident", "aniso", "rot") for v in (0, 6)] + [("rot", 6, 1), ("rot", 6, 5)]


def main():
    import ref_shim
    ref_shim.install()
    from mpunet.utils.fusion.fuse_and_predict import map_real_space_pred
    with np.load(os.path.join(HERE, "geometry_golden.npz")) as z:
        g = {k: z[k] for k in z.files}
    outs = {"map_linear_golden.npz": {"numpy_version": np.array(np.__version__)},
            "map_linear_golden_rot.npz": {"numpy_version": np.array(np.__version__)}}
    for an, v, K in CASES:
        key = "%s_16_%d" % (an, v)
        grid = (g["g3_g_" + key], g["g3_g_" + key], g["g3_off_" + key])
        pred = g["g5_pred_%s_%d_%d" % (an, v, K)]
        with contextlib.redirect_stdout(io.StringIO()):
            mapped = map_real_space_pred(pred, grid, g["g3_invb_" + key], g["g4_vgrid_" + an], method="linear")
        assert mapped.dtype == np.float32 and mapped.shape == (32, 28, 24, K), (mapped.dtype, mapped.shape)
        outs["map_linear_golden_rot.npz" if an == "rot" else "map_linear_golden.npz"]["lin_map_%s_%d_%d" % (an, v, K)] = mapped
    for name, out in outs.items():
        dst = os.path.join(HERE, name)
        np.savez_compressed(dst, **out)
        print(dst, "%.2f MiB" % (os.path.getsize(dst) / 2.0 ** 20))


if __name__ == "__main__":
    main()
