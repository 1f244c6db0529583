"""
Thin torch-tensor wrappers over the single-layer C-ABI entry points
(mpu_conv2d_*). Used by the unit tests and for layer-wise integration; the
U-Net itself runs through mpu_unet_forward / mpu_unet_backward.
"""
import torch
from . import _lib

CONV3, UPCONV2, CONV3S2, CONV1 = 0, 1, 2, 3
_NTAPS = {CONV3: 9, UPCONV2: 4, CONV3S2: 9, CONV1: 1}


def _dt(dtype):
    return {torch.float32: _lib.MPU_F32, torch.bfloat16: _lib.MPU_BF16}[dtype]


def pack_weights(w_hwio, mode, dtype, x3=False, out_fwd=None, out_dgrad=None):
    """fp32 Keras HWIO kernel (device) -> (forward operand, data-gradient operand). x3: the split-bf16 form of the f32 operands
    (mpu_dtype MPU_F32X3: each word holds bf16 hi | bf16 lo), for conv2d(x3=True). out_fwd / out_dgrad: caller-owned outputs
    (default: allocated here)."""
    kh, kw, ci, co = w_hwio.shape
    w = w_hwio.to(torch.float32).contiguous()
    wf = _lib.owned(out_fwd, kh * kw * co * ci, dtype, w.device, "out_fwd")
    wd = _lib.owned(out_dgrad, 9 * ci * co, dtype, w.device, "out_dgrad")
    _lib.call("mpu_conv2d_pack_weights", _lib.MPU_F32X3 if x3 else _dt(dtype), mode, _lib.ptr(w), ci, co,
              _lib.ptr(wf), _lib.ptr(wd), _lib.stream_ptr())
    return wf, wd


def _dtx(dtype, x3):
    if x3 and dtype != torch.float32:
        raise ValueError("x3 (split-bf16 products, MPU_F32X3) applies to f32 tensors")
    return _lib.MPU_F32X3 if x3 else _dt(dtype)


def conv2d(mode, x0, w_packed, cout, out_hw, bias=None, x1=None, mask=None, relu=False,
           w_tap_stride=None, w_row_stride=None, workspace=None, x3=False, out=None):
    """x0 [B,Hi,Wi,C0] (+ x1 concatenated on channels) -> [B,Ho,Wo,cout]. workspace: optional f32 scratch tensor
    (split-K partial sums of the deep-level schedules; 8*B*Ho*Wo*cout floats always suffice).
    x3: f32 tensors, every product as three bf16 MFMAs on hi + lo split operands (mpu_dtype MPU_F32X3).
    out: caller-owned output (default: allocated here)."""
    B = x0.shape[0]
    C0 = x0.shape[-1]
    C1 = 0 if x1 is None else x1.shape[-1]
    Ho, Wo = out_hw
    out = _lib.owned(out, (B, Ho, Wo, cout), x0.dtype, x0.device, "out")
    if w_row_stride is None:
        w_row_stride = C0 + C1
    if w_tap_stride is None:
        w_tap_stride = cout * (C0 + C1)
    args = [_dtx(x0.dtype, x3), mode, _lib.ptr(x0), C0, _lib.ptr(x1), C1,
            _lib.ptr(w_packed), w_tap_stride, w_row_stride, _lib.ptr(bias), _lib.ptr(mask),
            _lib.ptr(out), B, Ho, Wo, cout, int(relu)]
    if workspace is None:
        _lib.call("mpu_conv2d_igemm", *args, _lib.stream_ptr())
    else:
        _lib.call("mpu_conv2d_igemm_ws", *args, _lib.ptr(workspace), workspace.numel(), _lib.stream_ptr())
    return out


def conv2d_wgrad_first_layer(x, n_image_channels, dz, workspace=None, out=None, out_db=None):
    """(dW [9, 8, Cout], db [Cout]) f32 of the first 3x3 conv: x [B,H,W,8] holds n_image_channels real channels.
    workspace (mpu_conv2d_wgrad_first_layer_workspace_floats f32), out, out_db: caller-owned (default: allocated here)."""
    B, H, W, cout = dz.shape
    assert x.shape[-1] == 8
    n = _lib.load().mpu_conv2d_wgrad_first_layer_workspace_floats(cout, B * H * W)
    ws = _lib.owned(workspace, n, torch.float32, dz.device, "workspace")
    dW = _lib.owned(out, (9, 8, cout), torch.float32, dz.device, "out")
    db = _lib.owned(out_db, cout, torch.float32, dz.device, "out_db")
    _lib.call("mpu_conv2d_wgrad_first_layer", _dt(dz.dtype), _lib.ptr(x), n_image_channels, _lib.ptr(dz), cout,
              B, H, W, _lib.ptr(ws), _lib.ptr(dW), _lib.ptr(db), _lib.stream_ptr())
    return dW, db


def conv2d_wgrad(mode, x0, dz, x1=None, x3=False, workspace=None, out=None):
    """dW [taps, Cin, Cout] f32 of the conv whose input was concat(x0,x1) and output gradient dz (x3: as conv2d).
    workspace (mpu_conv2d_wgrad_workspace_floats f32), out: caller-owned (default: allocated here)."""
    B, Ho, Wo, cout = dz.shape
    C0 = x0.shape[-1]
    C1 = 0 if x1 is None else x1.shape[-1]
    nt = _NTAPS[mode]
    n = _lib.load().mpu_conv2d_wgrad_workspace_floats(mode, C0 + C1, cout, B * Ho * Wo)
    ws = _lib.owned(workspace, n, torch.float32, dz.device, "workspace")
    dW = _lib.owned(out, (nt, C0 + C1, cout), torch.float32, dz.device, "out")
    _lib.call("mpu_conv2d_wgrad", _dtx(dz.dtype, x3), mode, _lib.ptr(x0), C0, _lib.ptr(x1), C1,
              _lib.ptr(dz), cout, B, Ho, Wo, _lib.ptr(ws), _lib.ptr(dW), _lib.stream_ptr())
    return dW
