/*
 * mpunet_hip.h -- C ABI of libmpunet_hip.so: the MI355X (gfx950) hot path of
 * perslev/MultiPlanarUNet (mpunet 0.2.12).
 *
 * The reference reaches its arithmetic through tf.keras / NumPy; it has no FFI
 * of its own. Each entry point below therefore cites the reference call site
 * (file:line under /root/reference) whose work it replaces. INTEGRATION.md
 * shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory owned by the caller;
 *     everything else is host memory read before the call returns;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues
 *     work on it (no synchronisation, no allocation) unless stated;
 *   - return 0 on success, negative mpu_status otherwise; the message of the
 *     last failure on the calling thread is mpu_last_error();
 *   - activations are NHWC; `dtype` selects storage/arithmetic:
 *       MPU_F32  : f32 storage, exact-f32 MFMA (v_mfma_f32_32x32x2_f32)
 *       MPU_BF16 : bf16 storage, v_mfma_f32_32x32x16_bf16, f32 accumulate.
 *       MPU_F32X3: f32 storage, every product as three bf16 MFMAs on operands split hi + lo in registers (x ~ bf16(x) +
 *                  bf16(x - bf16(x)): ~2^-16 relative per product) -- the tolerance-grade mode at bf16-class matrix rates
 *                  (round 6; Python dtype "bf16x3"). Elementwise kernels, buffers and layouts are those of MPU_F32.
 */
#ifndef MPUNET_HIP_H
#define MPUNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MPU_OK = 0, MPU_EINVAL = -1, MPU_EHIP = -2, MPU_EUNSUPPORTED = -3 } mpu_status;
typedef enum { MPU_F32 = 0, MPU_BF16 = 1, MPU_F32X3 = 2 } mpu_dtype;

int         mpu_abi_version(void);
const char* mpu_last_error(void);
/* 16 hex digits: sha256 over every source, header and compiler flag this library was built from (compiled in by
 * multiplanarunet_amd/build.py). The ctypes host layer refuses a library whose hash is not that of the sources beside it. */
const char* mpu_build_hash(void);

/* ------------------------------------------------------------------------ *
 * Predict-time geometry (HBM-bound kernels)
 * ------------------------------------------------------------------------ */

/* A strictly increasing coordinate axis that also lives in device memory as an f64 array.
 * When the host has verified that a closed form reproduces the array BIT FOR BIT it says so
 * here and the kernels evaluate the form in registers instead of loading the array:
 *   kind 0: no closed form; only `step` is used (to seed the cell search)
 *   kind 1: value(i) = (i == n-1) ? last : fl(fl(i*step) + start)        (np.linspace)
 *   kind 2: value(i) = fl((i - start) * step)      (voxel axes: (arange(n)-(n-1)/2)*pixdim) */
typedef struct {
    int32_t kind;
    int32_t n;
    double  start, step, last;
} mpu_axis;

/* One view of IsotrophicLiveViewSequence2D.get_view_from
 * (mpunet/sequences/isotrophic_live_view_sequence_2d.py:29-117) expressed as
 * numbers: the plane basis of sample_plane_at (mpunet/interpolation/
 * sample_grid.py:192-244), the in-plane mgrid axis, and the optional rot_mat of
 * ViewInterpolator.apply_rotation (mpunet/interpolation/view_interpolator.py:54-60).
 * Matrices are row-major 3x3. */
typedef struct {
    double  basis[9];      /* columns u, v, n_hat                              */
    double  rot[9];        /* rot_mat; ignored unless has_rot                  */
    int32_t has_rot;
    int32_t dim;           /* sample_dim                                       */
    int32_t n_planes;      /* P = len(offsets)                                 */
    int32_t _pad;
    double  g_start;       /* np.mgrid[-hd:hd:dim*1j]: value(i) = i*g_step+g_start */
    double  g_step;
    mpu_axis vol_axis[3];  /* closed forms / spacings of the voxel axes d_ax, d_ay, d_az */
} mpu_view_geom;

/* get_view_from / sample_at: trilinear image planes (+ nearest label planes)
 * for every offset of one view, then MultiChannelScaler.transform.
 *   d_vol      f32 [X,Y,Z,C]            ImagePair.image
 *   d_labels   u8  [X,Y,Z] or NULL      ImagePair.labels
 *   d_ax,d_ay,d_az  f64 voxel axes of get_voxel_axes_real_space (sample_grid.py:63-98)
 *   d_offsets  f64 [P]                  np.linspace(-bounds, bounds, P)
 *   d_bg       f32 [C]                  RegularGridInterpolator fill_value per channel
 *   d_center,d_scale f64 [C] or NULL    sklearn scaler center_/scale_ (NULL = identity)
 *   d_out      f32 [P,dim,dim,C]        == np.moveaxis(Xs, 2, 0) of the reference
 *   d_out_lab  u8  [P,dim,dim] or NULL
 * Replaces isotrophic_live_view_sequence_2d.py:64-101 + view_interpolator.py:62-133
 * + regular_grid_interpolator.py:152-270 + preprocessing/scaling.py:75-89. */
int mpu_sample_view_planes(const float* d_vol, const uint8_t* d_labels,
                           const int32_t vol_shape[4],
                           const double* d_ax, const double* d_ay, const double* d_az,
                           const mpu_view_geom* geom, const double* d_offsets,
                           const float* d_bg, uint8_t bg_class,
                           const double* d_center, const double* d_scale,
                           float* d_out, uint8_t* d_out_lab, void* stream);

/* MultiChannelScaler.transform (mpunet/preprocessing/scaling.py:75-89) of a sampled value v, per channel c, for the five
 * sklearn classes the reference's YAML documents (bin/defaults/MultiPlanar/train_hparams.yaml:132-136). Every step is an
 * f64 operation followed by an f32 store, as sklearn's in-place operations on an f32 plane with f64 parameters are:
 *   MPU_SCALER_NONE      identity
 *   MPU_SCALER_SUB_DIV   RobustScaler, StandardScaler   v = f32(v - p0[c]); v = f32(v / p1[c])      (p0 center_/mean_, p1 scale_)
 *   MPU_SCALER_MUL_ADD   MinMaxScaler (0,1), no clip    v = f32(v * p0[c]); v = f32(v + p1[c])      (p0 scale_, p1 min_)
 *   MPU_SCALER_DIV       MaxAbsScaler                   v = f32(v / p0[c])                          (p0 scale_)
 *   MPU_SCALER_QUANTILE  QuantileTransformer (uniform)  v = f32(0.5 * (interp(v, q, r) - interp(-v, -q[::-1], -r[::-1]))) for
 *                        every non-NaN v, np.interp's rule; then v == q[-1] -> 1 and v == q[0] -> 0 (_transform_col).
 *                        q = quantiles[c], r = references; the tables of all channels are staged in LDS:
 *                        (n_channels + 1) * n_quantiles * 8 bytes <= 64 KiB, else MPU_EUNSUPPORTED. */
typedef enum { MPU_SCALER_NONE = 0, MPU_SCALER_SUB_DIV = 1, MPU_SCALER_MUL_ADD = 2, MPU_SCALER_DIV = 3,
               MPU_SCALER_QUANTILE = 4 } mpu_scaler_kind;
typedef struct {
    int32_t       kind;          /* mpu_scaler_kind                               */
    int32_t       n_quantiles;   /* QUANTILE only                                 */
    const double* p0;            /* device f64 [C]                                */
    const double* p1;            /* device f64 [C] (unused by DIV, QUANTILE)      */
    const double* quantiles;     /* device f64 [C][n_quantiles] or NULL           */
    const double* references;    /* device f64 [n_quantiles] or NULL              */
} mpu_scaler;

/* mpu_sample_view_planes with a scaler descriptor (NULL = identity) in place of d_center, d_scale. The call above is this
 * one with kind MPU_SCALER_SUB_DIV. */
int mpu_sample_view_planes_sc(const float* d_vol, const uint8_t* d_labels,
                              const int32_t vol_shape[4],
                              const double* d_ax, const double* d_ay, const double* d_az,
                              const mpu_view_geom* geom, const double* d_offsets,
                              const float* d_bg, uint8_t bg_class, const mpu_scaler* scaler,
                              float* d_out, uint8_t* d_out_lab, void* stream);

/* ------------------------------------------------------------------------ *
 * Volume statistics: what the per-channel scaler fits and the '<N>pct' background value need, computed on the resident
 * volume (the reference runs np.percentile / sklearn fits on the host: image_pair.py:300-341,469-484, scaling.py:47-73).
 * d_vol f32 [n_vox, n_channels], 16-byte aligned; n_vox < 2^31. Both calls below SYNCHRONISE the stream: they return
 * host values. The workspace (16-byte aligned, mpu_volume_stats_workspace_bytes) is the caller's.
 * ------------------------------------------------------------------------ */
int64_t mpu_volume_stats_workspace_bytes(int32_t n_channels);

/* Exact order statistics of one channel: values[i] = np.sort(x[~isnan(x)])[ranks[i]] for up to 16 zero-based ranks (host
 * i64; a rank outside [0, n_vox - nan_count) gives NaN), and the channel's NaN count. -0.0 and +0.0 are one value (+0.0 is
 * returned). Three-pass radix select: three reads of the volume, integer counters only -- the same bits on every run. */
int mpu_volume_order_stats(const float* d_vol, int64_t n_vox, int32_t n_channels, int32_t channel,
                           const int64_t* ranks, int32_t n_ranks, void* d_workspace, int64_t workspace_bytes,
                           float* values, int64_t* nan_count, void* stream);

/* Per channel c, out[c*8 + k], fp64, NaNs ignored. mean == NULL: k = 0..4 = count, min, max, max|x|, sum(x). mean = host f64
 * [n_channels]: k = 5, 6 = sum(x - mean[c]), sum((x - mean[c])^2) -- the two-pass form of sklearn's _incremental_mean_and_var
 * on a first batch. The entries of the pass not run are left alone. Fixed-order two-stage sums: bit-identical run to run. */
int mpu_volume_moments(const float* d_vol, int64_t n_vox, int32_t n_channels, const double* mean,
                       void* d_workspace, int64_t workspace_bytes, double* out, void* stream);

/* ------------------------------------------------------------------------ *
 * NIfTI-1 payload -> resident volume (csrc/volume_decode.hip): the order and type conversion nifti.read_nifti does with NumPy
 * on the host. d_payload: the file's bytes behind vox_offset as they lie there (Fortran order: x fastest, then y, z and the
 * fourth dimension), aligned to the element width. datatype: the NIfTI code (2 u8, 4 i16, 8 i32, 16 f32, 64 f64, 256 i8,
 * 512 u16, 768 u32, 1024 i64, 1280 u64; others MPU_EUNSUPPORTED). byteswap != 0: the file has the other endianness.
 * shape = (X, Y, Z, C), every entry in [1, 32767]; a 3-D file gives C = 1. scaled != 0 applies `f64(stored) * slope + inter`
 * (two rounded f64 operations); WHETHER a file's scl_slope / scl_inter ask for it is the caller's decision (nifti.py).
 *   MPU_DECODE_IMAGE   d_out f32 [X,Y,Z,C] (C order). Not scaled: stored type -> f32 in one conversion (i64 / u64 not through
 *                      f64; f32 bit for bit). Scaled: the f64 result rounded to f32, nearest even.
 *   MPU_DECODE_LABELS  d_out u8 [X,Y,Z,C]: the f64 value (scaled or not) truncated toward zero. *d_bad_count (device u64, zeroed
 *                      by the call) counts the voxels that are non-finite or whose truncation leaves [0, 256): NumPy's
 *                      astype(uint8) is platform-defined there; they are written as 0.
 * Asynchronous on `stream`; 64-bit indices throughout.
 * ------------------------------------------------------------------------ */
typedef enum { MPU_DECODE_IMAGE = 0, MPU_DECODE_LABELS = 1 } mpu_decode_kind;
int mpu_volume_decode(const void* d_payload, int32_t datatype, int32_t byteswap, const int64_t shape[4],
                      int32_t scaled, double slope, double inter, int32_t kind, void* d_out,
                      uint64_t* d_bad_count, void* stream);

/* ------------------------------------------------------------------------ *
 * Resident volume -> NIfTI-1 payload (csrc/volume_encode.hip): the inverse of mpu_volume_decode, and the
 * np.asfortranarray(data).tobytes(order="F") of nifti.write_nifti (nib.save(...), mpunet/bin/predict.py:90-117) done on the
 * device. d_in: [X,Y,Z,C] in C order, aligned to its element width. shape = (X, Y, Z, C), every entry in [1, 32767].
 * d_payload: the bytes as they lie behind vox_offset of a little-endian file (x fastest, then y, z and the fourth dimension):
 *   d_payload[((c * Z + z) * Y + y) * X + x] = convert(d_in[((x * Y + y) * Z + z) * C + c])
 * Pairs (every other one is MPU_EUNSUPPORTED):
 *   MPU_ENCODE_F32 -> datatype 16   bit for bit (NaN payloads included); d_payload aligned to 4 bytes; d_bad_count may be NULL
 *   MPU_ENCODE_U8 / _I32 / _I64 -> datatype 2   class indices; d_payload needs no alignment. A value outside [0, 256) is
 *                                   written as 0 and counted, once per element, in *d_bad_count (device u64, zeroed by the call).
 * Asynchronous on `stream`; 64-bit indices throughout; only the payload's X*Y*Z*C elements are written; the only atomic is the
 * counter's; two calls give the same bytes. A call that returns an error has written nothing, the counter included.
 * ------------------------------------------------------------------------ */
typedef enum { MPU_ENCODE_F32 = 0, MPU_ENCODE_U8 = 1, MPU_ENCODE_I32 = 2, MPU_ENCODE_I64 = 3 } mpu_encode_source;
int mpu_volume_encode(const void* d_in, int32_t source, const int64_t shape[4], int32_t datatype, void* d_payload,
                      uint64_t* d_bad_count, void* stream);

/* One view's prediction volume as seen by the back-mapping
 * (mpunet/utils/fusion/fuse_and_predict.py:92-137). */
typedef struct {
    double       inv_basis[9];   /* np.linalg.inv(basis) of the view            */
    const float* d_pred;         /* f32 [P,dim,dim,K] (model.predict output order) */
    const double* d_g;           /* f64 [dim]  real_axis = np.linspace(-hd,hd,dim) */
    const double* d_offsets;     /* f64 [P]                                     */
    int32_t      dim;
    int32_t      n_planes;
    mpu_axis     g_axis;         /* closed form / spacing of d_g       */
    mpu_axis     o_axis;         /* closed form / spacing of d_offsets */
} mpu_view_pred;

/* Voxel grid of get_voxel_grid_real_space (sample_grid.py:101-130), computed on
 * the fly: p = A*(i,j,k) - center. */
typedef struct {
    double  A[9];          /* affine[:3,:3]                                     */
    double  center[3];     /* mean over all voxels of A*(i,j,k)                 */
    int32_t shape[3];      /* X, Y, Z                                           */
    int32_t _pad;
} mpu_voxel_grid;

/* map_real_space_pred(method="nearest") for ONE view: d_mapped f32 [X,Y,Z,K],
 * OOB voxels -> [1,0,...,0] (fuse_and_predict.py:99-100). */
int mpu_map_view_nearest(const mpu_voxel_grid* grid, const mpu_view_pred* view,
                         int32_t n_classes, float* d_mapped, void* stream);

/* Fused _multi_view_predict_on + merge_multi_view_preds
 * (mpunet/bin/predict.py:294-366): for every voxel, nearest lookup in each of
 * the V view predictions, FusionLayer.call = softmax_k(sum_v W[v,k] x[v,k] + b[k])
 * (mpunet/models/fusion_model.py:38-39) or, with sum_fusion, sum_v x[v,k]
 * (predict.py:364); then pred_to_class argmax -> uint8 (utils/utils.py:326-328).
 * Nothing of `combined[V,X,Y,Z,K]` is materialised.
 *   views      host array of V mpu_view_pred
 *   d_W f32 [V,K], d_b f32 [K]  (ignored when sum_fusion)
 *   d_probs    f32 [X,Y,Z,K] or NULL ; d_labels u8 [X,Y,Z] or NULL */
int mpu_map_fuse_views(const mpu_voxel_grid* grid, const mpu_view_pred* views,
                       int32_t n_views, int32_t n_classes,
                       const float* d_W, const float* d_b, int32_t sum_fusion,
                       float* d_probs, uint8_t* d_labels, void* stream);

/* FusionModel.predict on an explicit x[N,V,K] (predict.py:358-361 layout). */
int mpu_fusion_forward(const float* d_x, int64_t n, int32_t n_views, int32_t n_classes,
                       const float* d_W, const float* d_b,
                       float* d_probs, uint8_t* d_labels, void* stream);

/* Multi-GPU predict: accumulate W[v,:] * nearest(x_v) of one
 * view's plane chunk [p_lo, p_hi) into d_z f32 [X,Y,Z,K]; the rank that owns
 * p_lo == 0 also adds the OOB contribution W[v,:]*[1,0..]. Then
 * mpu_fusion_finalize applies +b, softmax, argmax on a voxel slab. */
int mpu_map_accumulate_view(const mpu_voxel_grid* grid, const mpu_view_pred* view,
                            int32_t n_classes, const float* d_Wv,
                            int32_t p_lo, int32_t p_hi, int32_t owns_oob,
                            float* d_z, void* stream);
int mpu_fusion_finalize(const float* d_z, int64_t n, int32_t n_classes,
                        const float* d_b, int32_t sum_fusion,
                        float* d_probs, uint8_t* d_labels, void* stream);

/* map_real_space_pred(method="linear") (fuse_and_predict.py:92-137): the view's
 * prediction is the RegularGridInterpolator's `values` on (g, g, offsets), the
 * voxel's point q = inv_basis * p its query. Per axis _find_indices (cell
 * clipped to [0, n-2], y by IEEE division; a point ON the last node is in
 * bounds: cell n-2, y = 1); per class an fp64 sum from 0.0 over the eight
 * corners in itertools.product order (first axis slowest, plane axis fastest)
 * of (double)pred[corner][k] * (((1.0*wx)*wy)*wz), w = {1-y, y}, rounded once
 * to f32, no FMA contraction; a voxel out of the view's box on any axis takes
 * [1,0,...,0]. Bit for bit the reference's result. 1 <= n_classes <= 16, any
 * axis kind. The three calls take the arguments of their nearest counterparts:
 *   mpu_map_view_linear        d_mapped f32 [X,Y,Z,K]
 *   mpu_map_fuse_views_linear  the f32 vector above in the place of the gathered
 *                              one, then exactly mpu_map_fuse_views' arithmetic;
 *                              d_probs or d_labels may be NULL
 *   mpu_map_accumulate_view_linear  view->d_pred holds the planes
 *       [p_lo, min(p_hi + 1, P)): the chunk and ONE halo plane. A voxel belongs
 *       to the chunk when the CELL index of its plane axis lies in [p_lo, p_hi)
 *       (cells end at P-2: the last chunk owns that cell, a chunk of the last
 *       plane alone owns nothing), so a voxel's eight-corner sum stays on one
 *       rank and rounds as in the unsharded call. The chunk with owns_oob adds
 *       the fill vector of the out-of-box voxels. */
int mpu_map_view_linear(const mpu_voxel_grid* grid, const mpu_view_pred* view,
                        int32_t n_classes, float* d_mapped, void* stream);
int mpu_map_fuse_views_linear(const mpu_voxel_grid* grid, const mpu_view_pred* views,
                              int32_t n_views, int32_t n_classes,
                              const float* d_W, const float* d_b, int32_t sum_fusion,
                              float* d_probs, uint8_t* d_labels, void* stream);
int mpu_map_accumulate_view_linear(const mpu_voxel_grid* grid, const mpu_view_pred* view,
                                   int32_t n_classes, const float* d_Wv,
                                   int32_t p_lo, int32_t p_hi, int32_t owns_oob,
                                   float* d_z, void* stream);

/* Per-voxel uncertainty of the multi-view fusion, in the pass that fuses. For a
 * voxel let x_v (v = 0..V-1) be the f32 K-vector it reads from view v (exactly
 * what mpu_map_view_nearest / mpu_map_view_linear give, the fill vector
 * [1,0,...,0] outside the view's box included) and p what mpu_map_fuse_views
 * [_linear] computes from them. With
 *   Hn(q) = -sum_k (q_k/s) ln(q_k/s) / ln K,  s = sum_k q_k
 * (terms with q_k <= 0 contribute 0; s <= 0 gives 0; K = 1 gives 0):
 *   d_entropy   f32 [X,Y,Z]  Hn(p), in [0,1]
 *   d_mi        f32 [X,Y,Z]  max(0, Hn(mean_v x^_v) - mean_v Hn(x^_v)),
 *                            x^_v = x_v / sum_k x_v[k] (0 when that sum is <= 0),
 *                            unweighted means in view order
 *   d_agreement u8  [X,Y,Z]  number of views whose own argmax (first maximum,
 *                            strict >) equals the fused label of this call
 * linear != 0: the views are read as mpu_map_fuse_views_linear reads them, else
 * as mpu_map_fuse_views. d_probs / d_labels (either or both may be NULL) are
 * byte for byte what those calls give; the kernel is their exact form (no
 * straight-line variant). Each map pointer may be NULL, not all three. f32
 * logf and f32 sums: entropy within 1e-5, mi within 3e-5 of fp64.
 * MPU_EINVAL (message in mpu_last_error(), before any HIP call): NULL grid or
 * views, n_classes or n_views outside 1..16, all three maps NULL, W or b
 * missing without sum_fusion, a NULL view field.
 *
 * mpu_uncertainty_table: one pass over a label map d_labels u8 [n] (classes
 * >= n_classes are skipped), the three maps (each may be NULL: its sums are 0;
 * entropy and mi are clamped to [0,1], NaN counts as 0) and optionally a truth
 * map d_truth u8 [n]. d_table f64 [K][3][4]: per class c of d_labels and group
 * (0 all, 1 correct: truth == c, 2 wrong; 1 and 2 are zero when d_truth is
 * NULL) the voxel count and the sums of entropy, mi and agreement. Sums are
 * integers (entropy and mi in 2^-32 fixed point), so two calls give identical
 * bytes. 0 <= n < 2^31. d_scratch: mpu_uncertainty_table_scratch_bytes(n, K)
 * bytes, 8-byte aligned as d_table (0 for n_classes outside 1..16). */
int mpu_map_fuse_views_uncertainty(const mpu_voxel_grid* grid, const mpu_view_pred* views,
                                   int32_t n_views, int32_t n_classes,
                                   const float* d_W, const float* d_b, int32_t sum_fusion, int32_t linear,
                                   float* d_probs, uint8_t* d_labels,
                                   float* d_entropy, float* d_mi, uint8_t* d_agreement,
                                   void* stream);
size_t mpu_uncertainty_table_scratch_bytes(int64_t n, int32_t n_classes);
int mpu_uncertainty_table(const uint8_t* d_labels, const uint8_t* d_truth, const float* d_entropy,
                          const float* d_mi, const uint8_t* d_agreement, int64_t n, int32_t n_classes,
                          double* d_table, void* d_scratch, void* stream);


/* ------------------------------------------------------------------------ *
 * 2-D U-Net (MFMA-bound): mpunet.models.UNet (mpunet/models/unet.py:20-251)
 * ------------------------------------------------------------------------ */

/* conv modes of the implicit-GEMM kernels */
enum { MPU_CONV3 = 0,      /* Conv2D(k=3, padding="same")                 unet.py:120-179 */
       MPU_UPCONV2 = 1,    /* UpSampling2D(2) + Conv2D(k=2, "same")       unet.py:159-163 */
       MPU_CONV3S2 = 2,    /* 3x3 stride-2 pad-1: data gradient of MPU_UPCONV2           */
       MPU_CONV1 = 3 };    /* Conv2D(k=1)                                 unet.py:211     */

/* What UNet.__init__ / init_model (unet.py:26-112,182-216) derive from the
 * constructor arguments. filters[l] = int(64 * 2^l * sqrt(complexity_factor)),
 * l = 0..depth (unet.py:91,120,132). padding="same", activation="relu",
 * kernel_size=3 are the only supported values.
 * Two class limits: a handle with 1..8 classes trains, evaluates and predicts; one with 9..16 classes is INFERENCE-ONLY
 * (mpu_unet_forward with training == 0, the weight / packing / query entry points). On such a handle the training-mode forward,
 * mpu_unet_backward / _backward_events / _backward_adam and mpu_unet_set_loss with anything but the plain MPU_LOSS_SPARSE_CE
 * return MPU_EUNSUPPORTED ("U-Net training and evaluation support 1..8 classes; 9..16 are inference-only") before any launch
 * and without changing the handle. mpu_eval_loss likewise takes 1..8 classes. */
typedef struct {
    int32_t n_classes;     /* 1..16 (9..16: inference-only, see above)          */
    int32_t n_channels;
    int32_t depth;         /* 1..6                                              */
    int32_t H, W;          /* img_rows, img_cols: multiples of 2^depth          */
    int32_t dtype;         /* mpu_dtype of activations / MFMA operands          */
    int32_t softmax;       /* out_activation: 1 = "softmax", 0 = "linear"       */
    int32_t filters[8];
} mpu_unet_config;

typedef struct mpu_unet mpu_unet;   /* host-only layer table; owns no device memory */

mpu_unet* mpu_unet_create(const mpu_unet_config* cfg);      /* NULL + mpu_last_error() on bad config */
void      mpu_unet_destroy(mpu_unet* m);

/* Flat fp32 buffers the caller allocates (channel counts are padded to multiples
 * of 8; padded entries are zero and stay zero under training):
 *   params / grads / adam m / adam v : mpu_unet_param_floats()   floats each
 *   BN moving statistics             : mpu_unet_bn_state_floats() floats
 *   packed MFMA weight operands      : mpu_unet_packed_bytes()    bytes
 *   activations + scratch            : mpu_unet_workspace_bytes(batch) bytes
 * mpu_unet_tensor_info enumerates "<keras layer name>/<kernel|bias|gamma|beta|
 * moving_mean|moving_variance>" with its offset, stored (padded) and logical
 * Keras shape (kernels are HWIO), kind 0 = params buffer, 1 = BN-state buffer. */
int64_t mpu_unet_param_floats(const mpu_unet* m);
int64_t mpu_unet_bn_state_floats(const mpu_unet* m);
int64_t mpu_unet_packed_bytes(const mpu_unet* m);
int64_t mpu_unet_logical_param_count(const mpu_unet* m);   /* trainable, unpadded */
int64_t mpu_unet_workspace_bytes(const mpu_unet* m, int32_t batch);
int32_t mpu_unet_num_tensors(const mpu_unet* m);
int     mpu_unet_tensor_info(const mpu_unet* m, int32_t idx, char* name, int32_t name_cap,
                             int32_t* kind, int64_t* offset,
                             int32_t stored_shape[4], int32_t logical_shape[4]);

/* fp32 master weights -> MFMA operands (forward [tap][co][ci], data-gradient
 * [tap][ci][co] incl. the tap-combined 3x3 stride-2 form of the up-conv).
 * Call after every change of d_params (set_weights, load_weights, Adam). */
int mpu_unet_pack_weights(const mpu_unet* m, const float* d_params, void* d_packed, void* stream);

/* Inference-mode BatchNormalization is folded into the producing convolutions: this computes the
 * per-channel scale/shift (gamma, beta, moving statistics, epsilon 1e-3) into the tail of d_packed.
 * Call after every change of d_params / d_bn_state and before mpu_unet_forward(training = 0). */
int mpu_unet_prepare_inference(const mpu_unet* m, const float* d_params, const float* d_bn_state,
                               void* d_packed, void* stream);

/* model.predict_on_batch / the forward half of a Model.fit step
 * (mpunet/utils/fusion/fuse_and_predict.py:88, mpunet/train/trainer.py:246).
 *   d_x   f32 [B,H,W,n_channels] ; d_out f32 [B,H,W,n_classes] (probabilities or
 *   logits). training != 0: BatchNormalization uses batch statistics and updates
 *   the moving statistics in d_bn_state; activations stay in d_workspace for
 *   mpu_unet_backward. */
/* d_out may be NULL in training mode: the probabilities then stay in the workspace only, at byte offset
 * mpu_unet_workspace_probs_offset(m, batch) (f32 [B,H,W,n_classes]; valid until the next forward on that workspace). On a handle
 * created with softmax == 0 the region holds the LOGITS (what d_out would have received): the backward pass of
 * MPU_LOSS_SPARSE_CE_LOGITS reads them there. */
int64_t mpu_unet_workspace_probs_offset(const mpu_unet* m, int32_t batch);
/* Byte offset (inside the workspace of `batch`) of ONE float: the mean over the B*H*W pixels of the weighted per-pixel loss of the
 * last backward pass (= mean of the d_loss tensor mpu_unet_backward fills; written by the pass whether d_loss is NULL or not;
 * with a per-image loss the mean over the batch of w_b * L_b).
 * It is what a training loop accumulates per step without a reduction of its own (reference: the `loss` Keras logs per batch,
 * mpunet/train/trainer.py:246-257). Valid until the next backward pass on that workspace. */
int64_t mpu_unet_workspace_loss_mean_offset(const mpu_unet* m, int32_t batch);
/* Test aid (no reference counterpart): the region table of the workspace plan of `batch`, read-only. The workspace is ONE caller-owned
 * buffer that the plan cuts into regions, each starting at a multiple of 256 bytes, none aliasing another: region i + 1 starts at
 * offset_i + roundup(bytes_i, 256) and the last one ends at mpu_unet_workspace_bytes(m, batch). Records 0 .. n-1 come in plan order:
 * first every top-level region (parent = -1), interleaved with the sub-entries (parent = index of the top-level region they lie in,
 * dotted names) of the regions that have an internal layout. `bytes` is the UNROUNDED length the plan asked for, so
 * [offset + bytes, next offset) is padding that nothing may write. cls:
 *   MPU_WS_TENSOR   a tensor with one writer at a time: "act/xin", "act/<role>/<level or block>" (C1 C2 N P dskip; C1b C2b Nb;
 *                   U1 N1 C2u C3u N2), "probs", "loss_mean", the gradient ping-pong "gA" / "gB", every conv's "dz/<conv>";
 *   MPU_WS_STATS    "stats": the saved statistics; sub-entries "stats.bn/<bn>" = mean, invstd, scale, shift (4 C floats);
 *   MPU_WS_SCRATCH  "partial" (sub-entries "partial.rows" and "partial.trailer", the 1024 floats of the fused training head),
 *                   "partial2", "wpartial" (sub-entries "wpartial.conv/<conv>": each conv's own weight-gradient scratch), "cpartial",
 *                   "bnacc" (sub-entries "bnacc.fwd/<bn>", "bnacc.bwd/<bn>" and, dtype bf16x3, "bnacc.db/<conv>"), "coeffs", the bf16x3
 *                   plane triples "x3x0/<conv>", "x3x1/<conv>", "x3dz/<conv>", and with a per-image loss "loss_scratch", "loss_coef".
 * The "probs" and "loss_mean" records carry the offsets of the two queries above. The query moves no offset and costs the step path
 * nothing: names and records are built only while a query runs (tests/test_unet_regions_host.py, tests/test_gpu_ws_audit.py). */
enum { MPU_WS_TENSOR = 0, MPU_WS_STATS = 1, MPU_WS_SCRATCH = 2 };
int32_t mpu_unet_workspace_num_regions(const mpu_unet* m, int32_t batch);
int     mpu_unet_workspace_region_info(const mpu_unet* m, int32_t batch, int32_t idx, char* name, int32_t name_cap,
                                       int64_t* offset, int64_t* bytes, int32_t* cls, int32_t* parent);
int mpu_unet_forward(const mpu_unet* m, int32_t batch, const float* d_x, const float* d_params,
                     const void* d_packed, float* d_bn_state, void* d_workspace,
                     int32_t training, float* d_out, void* stream);

/* Backward half of the Keras train step compiled at mpunet/train/trainer.py:78-97
 * (SparseCategoricalCrossentropy(reduction=NONE) on clipped probabilities,
 * per-image sample weights, gradient of the SUM over batch and pixels).
 *   d_y u8 [B,H*W] ; d_sample_weight f32 [B] ; d_grads f32 [param_floats]
 *   d_loss f32 [B,H*W] per-pixel weighted loss or NULL (with a per-image loss attached by mpu_unet_set_loss: f32 [B]).
 * Must follow mpu_unet_forward(training=1) on the same workspace -- ONE backward pass per training forward: the forward's first
 * launch zeroes the fixed-point BatchNorm accumulators of both passes (round 6, bf16 / bf16x3), a second backward pass on the same
 * forward would add to the first one's sums. The handle remembers which form of the head the last training forward ran (with a
 * 64-channel last block and a head that trains it leaves NO post-BatchNorm tensor of that block in the workspace; the backward pass
 * then recomputes it): forward and backward of one step run on the same handle, not interleaved with another step's. */
int mpu_unet_backward(const mpu_unet* m, int32_t batch, const uint8_t* d_y,
                      const float* d_sample_weight, const float* d_params, const void* d_packed,
                      float* d_bn_state, void* d_workspace, float* d_grads, float* d_loss,
                      void* stream);

/* The loss of the train step (mpunet/train/trainer.py:51-53,79-82: `fit.loss` / `fit.loss_kwargs` resolved in tf.keras.losses and
 * then in mpunet/evaluate/loss_functions.py). A handle trains with MPU_LOSS_SPARSE_CE until mpu_unet_set_loss attaches another
 * kind; call it before the handle's first training step (the workspace plan of a handle with a region loss is a little larger:
 * query mpu_unet_workspace_bytes and the offsets again afterwards). The five losses of loss_functions.py are compiled with
 * reduction=NONE on the flattened output (bin/train.py:288,357): ONE value per image, L_b, times the per-image sample weight;
 * the gradient is that of the sum over the batch. With such a loss the d_loss argument of mpu_unet_backward / _backward_events /
 * _backward_adam receives B floats (w_b * L_b) instead of B*H*W, and the float at mpu_unet_workspace_loss_mean_offset is their
 * mean over the batch (what Keras logs). Fields a kind does not use are ignored.
 *   MPU_LOSS_DICE / MPU_LOSS_JACCARD : smooth >= 0                                   loss_functions.py:80-112 / :33-77
 *   MPU_LOSS_GENERALIZED_DICE        : type_weight (mpu_gdl_weight)                  :207-266
 *   MPU_LOSS_FOCAL                   : gamma, class_weights[n_class_weights] (0 or n_classes entries)   :166-204
 *   MPU_LOSS_EXP_LOG                 : gamma_dice, gamma_cross, weight_dice, weight_cross               :115-163
 * MPU_LOSS_SPARSE_CE_LOGITS is tf.keras.losses.SparseCategoricalCrossentropy(reduction=NONE, from_logits=True) on a handle created
 * with softmax == 0 (`build.out_activation: linear` + `fit.loss_kwargs: {from_logits: true}`): TF 2.3 goes straight to
 * sparse_softmax_cross_entropy_with_logits, without the probability clip of MPU_LOSS_SPARSE_CE. Per pixel, with z the K logits:
 * L = logsumexp_k(z_k) - z_y (the maximum subtracted first), d_loss f32 [B,H*W] = w_b * L as for MPU_LOSS_SPARSE_CE, the logged mean
 * over the B*H*W pixels, gradient of the sum dz_k = w_b * (softmax(z)_k - [k == y]) with no clip mask. It takes no field but `kind`,
 * changes no workspace size or offset, and is the only loss with which a softmax == 0 handle trains: mpu_unet_backward /
 * _backward_events / _backward_adam accept such a handle if and only if it is attached. MPU_LOSS_SPARSE_CE on such a handle detaches
 * it again. The output of the forward pass stays the logits. */
typedef enum { MPU_LOSS_SPARSE_CE = 0, MPU_LOSS_DICE = 1, MPU_LOSS_JACCARD = 2, MPU_LOSS_GENERALIZED_DICE = 3,
               MPU_LOSS_FOCAL = 4, MPU_LOSS_EXP_LOG = 5, MPU_LOSS_SPARSE_CE_LOGITS = 6 } mpu_loss_kind;
typedef enum { MPU_GDL_SQUARE = 0, MPU_GDL_SIMPLE = 1, MPU_GDL_UNIFORM = 2 } mpu_gdl_weight;
typedef struct {
    int32_t kind;              /* mpu_loss_kind                                        */
    int32_t type_weight;       /* mpu_gdl_weight                                       */
    float   smooth;
    float   gamma;
    float   gamma_dice, gamma_cross, weight_dice, weight_cross;
    int32_t n_class_weights;   /* 0: none (all ones)                                   */
    float   class_weights[8];
} mpu_loss_config;
/* MPU_EINVAL + mpu_last_error() on an unknown kind or type_weight, a negative smooth, a class-weight count that is neither 0 nor
 * n_classes, one of the five per-image kinds on a handle created with softmax == 0, or MPU_LOSS_SPARSE_CE_LOGITS on a handle created
 * with softmax == 1 (it would apply the softmax twice). MPU_EUNSUPPORTED on a handle with more than 8 classes unless cfg is the
 * default (MPU_LOSS_SPARSE_CE, no class weights). */
int mpu_unet_set_loss(mpu_unet* m, const mpu_loss_config* cfg);

/* Accept / reject statistics of one sampled training slice (mpunet/sequences/isotrophic_live_view_sequence.py:91-128:
 * np.isin(fg_classes, lab), np.any(~np.isclose(im, bg))): d_out2[0] = OR of (1 << label) over the labels (< 32),
 * d_out2[1] = 1 when some pixel differs from its channel's background value d_bg[c]. Either input may be NULL. */
int mpu_plane_stats(const uint8_t* d_labels, const float* d_image, int64_t n_pixels, int32_t n_channels,
                    const float* d_bg, uint32_t* d_out2, void* stream);

/* mpu_sample_view_planes for ONE plane followed by mpu_plane_stats of it: one candidate slice of the train-time sampler per call
 * (arguments as the two; d_bg_scaled = the background value as the scaled plane shows it). */
int mpu_sample_plane_stats(const float* d_vol, const uint8_t* d_labels, const int32_t vol_shape[4],
                           const double* d_ax, const double* d_ay, const double* d_az,
                           const mpu_view_geom* geom, const double* d_offset,
                           const float* d_bg, uint8_t bg_class, const double* d_center, const double* d_scale,
                           float* d_out, uint8_t* d_out_lab, const float* d_bg_scaled, uint32_t* d_stats2, void* stream);
/* The same with a scaler descriptor (mpu_sample_view_planes_sc). */
int mpu_sample_plane_stats_sc(const float* d_vol, const uint8_t* d_labels, const int32_t vol_shape[4],
                              const double* d_ax, const double* d_ay, const double* d_az,
                              const mpu_view_geom* geom, const double* d_offset,
                              const float* d_bg, uint8_t bg_class, const mpu_scaler* scaler,
                              float* d_out, uint8_t* d_out_lab, const float* d_bg_scaled, uint32_t* d_stats2, void* stream);

/* Elastic2D augmentation of one training slice (mpunet/augmentation/elastic_deformation.py:6-69, applied by
 * mpunet/augmentation/augmenters.py:87-107 after scaling): image [H][W][C] f32 bilinear with fill d_bg[c],
 * labels [H][W] u8 nearest with fill 0 (either pair may be NULL), displaced by alpha * gaussian_filter(2*noise-1)
 * of the two uniform [0,1) fields d_noise [2][H][W] (f64). d_gauss_w: the 2*radius+1 normalised Gaussian weights
 * (f64; radius = int(4*sigma + .5)); d_workspace: mpu_elastic_workspace_doubles(H, W) doubles. */
int64_t mpu_elastic_workspace_doubles(int32_t H, int32_t W);
int mpu_elastic_transform_2d(const float* d_image, const uint8_t* d_labels, int32_t H, int32_t W, int32_t C,
                             const double* d_noise, const double* d_gauss_w, int32_t radius, double alpha,
                             const float* d_bg, double* d_workspace, float* d_out_image,
                             uint8_t* d_out_labels, void* stream);

/* Fusion-model training (mpunet/bin/train_fusion.py:327-362 `fusion_model.fit`): one Adam step of the FusionLayer
 * (mpunet/models/fusion_model.py:14-39) on a batch of points x[n][V][K] with integer targets y[n] under the
 * reference's per-point generalized Dice loss (mpunet/evaluate/loss_functions.py:207-246, SUM_OVER_BATCH_SIZE) plus
 * its 1e-6 * mean(square) regularisers. t >= 1: Keras Adam step t is applied to d_W [V][K] / d_b [K] (moments in
 * d_adam_m / d_adam_v, V*K+K floats); t == 0: gradients and loss only. d_grads_out (V*K+K floats) and d_loss_out
 * (1 float, the batch loss BEFORE the update) may be NULL. 1 <= V <= 16 views, 1 <= K <= 16 classes (9..16: two lanes per
 * point, eight classes each; same partial rows, same fixed-order reduction, bit-reproducible run to run). */
int64_t mpu_fusion_train_workspace_floats(int32_t n_views, int32_t n_classes);
int mpu_fusion_train_step(const float* d_x, const uint8_t* d_y, int64_t n, int32_t n_views,
                          int32_t n_classes, float* d_W, float* d_b, float* d_adam_m, float* d_adam_v,
                          int64_t t, double lr, double beta1, double beta2, double eps,
                          float* d_workspace, float* d_grads_out, float* d_loss_out, void* stream);
/* The same step in two halves for data-parallel fitting (the reference builds its models under
 * tf.distribute.MirroredStrategy, mpunet/bin/train_fusion.py:336): every rank turns ITS share of the batch (n >= 0 points)
 * into d_sums[V*K + K + 2] doubles -- the gradient SUMS of the data term, the summed per-point loss and, last, its point count
 * -- the host SUM-all-reduces the doubles over the ranks, and mpu_fusion_apply_sums divides by the total count, adds the
 * regularisers and applies the Adam step. With one rank the pair gives bit for bit what mpu_fusion_train_step gives. */
int mpu_fusion_grad_sums(const float* d_x, const uint8_t* d_y, int64_t n, int32_t n_views, int32_t n_classes,
                         const float* d_W, const float* d_b, float* d_workspace, double* d_sums, void* stream);
int mpu_fusion_apply_sums(const double* d_sums, int32_t n_views, int32_t n_classes, float* d_W, float* d_b,
                          float* d_adam_m, float* d_adam_v, int64_t t, double lr, double beta1, double beta2,
                          double eps, float* d_grads_out, float* d_loss_out, void* stream);

/* Data-parallel training: the backward pass finishes the flat gradient buffer from its END towards its start
 * (head, up blocks, bottom, encoder levels). mpu_unet_grad_ready_points returns the number of ready points and
 * writes their float offsets (descending): after point k every gradient at offset >= offsets[k] is final.
 * mpu_unet_backward_events is mpu_unet_backward that also records ready_events[k] (hipEvent_t, NULL = skip) on
 * `stream` at point k, so the caller can start the all-reduce of a bucket (tf.distribute.MirroredStrategy's
 * gradient aggregation, mpunet/bin/train.py:349) while the rest of the backward pass is still running. */
int32_t mpu_unet_grad_ready_points(const mpu_unet* m, int64_t* offsets, int32_t cap);
int mpu_unet_backward_events(const mpu_unet* m, int32_t batch, const uint8_t* d_y,
                             const float* d_sample_weight, const float* d_params, const void* d_packed,
                             float* d_bn_state, void* d_workspace, float* d_grads, float* d_loss,
                             void* const* ready_events, int32_t n_events, void* stream);

/* kernel_regularizer=regularizers.l2(l2) of the encoder / bottom / up-sampling conv kernels (mpunet/models/unet.py:
 * 122-177,189; the 1x1 output conv at :211, biases and BatchNorm carry none): d_grads += 2*l2*W over those tensors,
 * to be called after mpu_unet_backward (after the replica all-reduce under data parallelism) and before the Adam
 * step. d_reg_loss (optional, 1 float) receives l2 * sum W^2, the term Keras adds to the reported loss; it needs
 * d_partial = mpu_unet_l2_workspace_doubles() doubles of scratch. Deterministic summation order. */
int mpu_unet_l2_regularizer(const mpu_unet* m, const float* d_params, float* d_grads, double l2, double* d_partial,
                            float* d_reg_loss, void* stream);
int64_t mpu_unet_l2_workspace_doubles(void);

/* The optimizer step of a U-Net in ONE launch: the Adam update of mpu_adam_step over the model's whole flat
 * parameter buffer AND the refresh of the packed MFMA operands (mpu_unet_pack_weights), tile by tile -- the updated
 * kernel tile is written to d_params and, converted, to both packed copies while it is in registers / LDS. Bit-identical
 * to mpu_adam_step followed by mpu_unet_pack_weights (tests/test_gpu_unet.py), 0.25 GB less HBM traffic per step of the
 * configs[1] network. d_step != NULL: step count t-1 in device memory, incremented by the call (graph replay, as
 * mpu_adam_step_device_counter); else t is the 1-based step. Replaces, for this path, Keras' optimizer.apply_gradients
 * inside Model.fit (mpunet/train/trainer.py:246). */
int mpu_unet_adam_pack(const mpu_unet* m, float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t t,
                       int64_t* d_step, double lr, double beta1, double beta2, double eps, void* d_packed, void* stream);

/* One Model.fit inner step's backward half AND its optimizer (mpunet/train/trainer.py:246: Keras runs the tape's
 * gradients and optimizer.apply_gradients inside one fit step): mpu_unet_backward followed by mpu_unet_adam_pack, with the
 * same results bit for bit, scheduled so that the HBM-bound optimizer runs BESIDE the MFMA-bound weight gradients
 * instead of behind them (round 6). The deep levels' weight gradients (every layer that is not on the strip-resident
 * wgrad_taps schedule: 86 % of the parameters of the configs[1] network) are finished first; their Adam update + operand
 * refresh then run on a library-owned side stream, as a register- and LDS-lean kernel that shares the compute units with
 * the grouped weight-gradient launch of the high-resolution levels; the remaining parameters follow that launch. Under
 * stream capture the fork / join become parallel branches of the graph (run one eager call first: the side stream and
 * its two events are created at the first use). MPU_TAIL_OVERLAP=0: the serial order. Single GPU, no l2 term (both need
 * the gradients between the two halves: use the two calls). Arguments as mpu_unet_backward + mpu_unet_adam_pack;
 * d_params / d_packed are read by the backward pass and updated by the optimizer. */
int mpu_unet_backward_adam(const mpu_unet* m, int32_t batch, const uint8_t* d_y, const float* d_sample_weight,
                           float* d_params, void* d_packed, float* d_bn_state, void* d_workspace, float* d_grads,
                           float* d_loss, float* d_m, float* d_v, int64_t t, int64_t* d_step, double lr, double beta1,
                           double beta2, double eps, void* stream);

/* Dev aid: on != 0 arms eight timing events that mpu_unet_backward_adam records at the branch points of its tail (0 before the
 * deep levels' weight gradients, 1 after their reductions = the fork, 2 / 3 side stream before / after its optimizer launch, 4 after
 * the grouped wgrad_taps launch, 5 after its reductions, 6 after the remaining optimizer launch, 7 after the join); on == 0
 * disarms, synchronises and writes the milliseconds of each since event 0 into ms_out[8] (-1: not recorded). Timestamps of BOTH
 * streams without rocprofv3, whose per-dispatch signals change how the two queues interleave. */
int mpu_debug_tail_events(int32_t on, float* ms_out);

/* Keras Adam (TF ApplyAdam form), t = 1-based step; YAML defaults
 * lr 5e-5, beta_1 .9, beta_2 .999, epsilon 1e-8
 * (mpunet/bin/defaults/MultiPlanar/train_hparams.yaml:126). */
int mpu_adam_step(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n,
                  int64_t t, double lr, double beta1, double beta2, double eps, void* stream);

/* Same update with the step count t-1 held in device memory (*d_step, incremented by the call): the form a
 * captured HIP graph can replay, since every replay must see a new bias-correction factor. */
int mpu_adam_step_device_counter(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n,
                                 int64_t* d_step, double lr, double beta1, double beta2, double eps,
                                 void* stream);

/* The other optimizers `fit.optimizer` may name (mpunet/train/utils.py:100-111 resolves it in tf.keras.optimizers;
 * `fit.optimizer_kwargs`, train_hparams.yaml:125-126) and learning-rate decay, as TF 2.3 computes them. k = steps applied
 * before this one, t = k + 1; lr_t = lr / (1 + decay * k) (OptimizerV2._decayed_lr; decay == 0: lr itself). Arithmetic per
 * element in f32, in the order written, no FMA contraction; the scalars are formed in f64 and rounded once.
 *   MPU_OPT_ADAM     m += (g-m)(1-beta1); v += (g*g-v)(1-beta2); alpha = lr_t*sqrt(1-beta2^t)/(1-beta1^t);
 *                    p -= m*alpha/(sqrt(v)+epsilon). MPU_OPT_AMSGRAD: vhat = max(vhat, v) in place of v in the root.
 *                    Slots m, v[, vhat].                                    (ApplyAdam / ApplyAdamWithAmsgrad)
 *   MPU_OPT_SGD      momentum == 0: p -= lr_t*g, no slot. Else a = a*momentum - lr_t*g; p += a, or with MPU_OPT_NESTEROV
 *                    p += a*momentum - lr_t*g. Slot a.                      (ApplyGradientDescent / ApplyKerasMomentum)
 *   MPU_OPT_RMSPROP  ms += (g*g-ms)(1-rho); MPU_OPT_CENTERED: mg += (g-mg)(1-rho), d = ms - mg*mg, else d = ms.
 *                    momentum == 0: p -= lr_t*g/(sqrt(d)+epsilon)  (epsilon outside the root: the Python dense path);
 *                    else mom = mom*momentum + lr_t*g/sqrt(d+epsilon); p -= mom  (inside: ApplyRMSProp /
 *                    ApplyCenteredRMSProp). Slots ms[, mom][, mg].
 *   MPU_OPT_ADAMAX   m += (g-m)(1-beta1); u = max(beta2*u, |g|); p -= (lr_t/(1-beta1^t))*m/(u+epsilon). Slots m, u.  (ApplyAdaMax)
 * Fields a kind does not use are ignored; a flag of another kind is refused. */
typedef enum { MPU_OPT_ADAM = 0, MPU_OPT_SGD = 1, MPU_OPT_RMSPROP = 2, MPU_OPT_ADAMAX = 3 } mpu_optimizer_kind;
/* (flag value 8 is used inside the library for momentum > 0 and refused in `flags`: a new public flag starts at 16) */
typedef enum { MPU_OPT_NESTEROV = 1, MPU_OPT_AMSGRAD = 2, MPU_OPT_CENTERED = 4 } mpu_optimizer_flag;
typedef struct {
    int32_t kind, flags;
    double lr, decay, beta1, beta2, epsilon, momentum, rho;
} mpu_optimizer_config;
/* Number of slot buffers (0..3, each as long as the parameters, zero before the first step) of a configuration;
 * < 0 + mpu_last_error() when it is invalid (replaces the checks of the tf.keras.optimizers constructors). */
int mpu_optimizer_num_slots(const mpu_optimizer_config* cfg);
/* One step on a flat buffer of n floats, element-wise (the two-pass reference form, as mpu_adam_step): replaces Keras'
 * optimizer.apply_gradients inside Model.fit (mpunet/train/trainer.py:246). d_slots[i] for i >= mpu_optimizer_num_slots
 * is not touched and may be NULL. d_step != NULL: step count t-1 in device memory, incremented by the call (graph replay);
 * else t is the 1-based step. */
int mpu_optimizer_step(const mpu_optimizer_config* cfg, float* d_params, const float* d_grads, float* const d_slots[3],
                       int64_t n, int64_t t, int64_t* d_step, void* stream);
/* mpu_unet_adam_pack for every configuration: the update of mpu_optimizer_step over the model's flat parameter buffer AND
 * the refresh of the packed MFMA operands in ONE launch, bit-identical to mpu_optimizer_step followed by
 * mpu_unet_pack_weights (tests/test_gpu_optimizers.py). A rule moves only the slots it has. t / d_step as above. Replaces
 * optimizer.apply_gradients inside Model.fit (mpunet/train/trainer.py:246) for a project whose `fit.optimizer` is not plain
 * Adam with decay 0; that one keeps mpu_unet_adam_pack / mpu_unet_backward_adam. */
int mpu_unet_optimizer_pack(const mpu_unet* m, const mpu_optimizer_config* cfg, float* d_params, const float* d_grads,
                            float* const d_slots[3], int64_t t, int64_t* d_step, void* d_packed, void* stream);

/* Single-layer entry points (unit tests / layer-wise integration). Channels
 * must be multiples of 8. d_w is the fp32 Keras HWIO kernel; d_w_dgrad may be
 * NULL; sizes: fwd taps*Cin*Cout elements, dgrad 9*Cin*Cout elements (every
 * element of both is written, except that the 1x1 mode writes only the first
 * Cin*Cout elements of d_w_dgrad and leaves the other 8*Cin*Cout untouched).
 * mpu_conv2d_igemm computes out[m][n] = act(sum_k in[m@tap][k] w[tap][n][k] + bias[n])
 * (* (mask[m][n] > 0) when d_mask is given) over the channel-concatenation of
 * in0 and in1. */
int mpu_conv2d_pack_weights(int32_t dtype, int32_t mode, const float* d_w, int32_t Cin, int32_t Cout,
                            void* d_w_fwd, void* d_w_dgrad, void* stream);
int mpu_conv2d_igemm(int32_t dtype, int32_t mode, const void* d_in0, int32_t C0,
                     const void* d_in1, int32_t C1, const void* d_w_packed,
                     int64_t w_tap_stride, int32_t w_row_stride, const float* d_bias,
                     const void* d_mask, void* d_out, int32_t B, int32_t Ho, int32_t Wo,
                     int32_t Cout, int32_t relu, void* stream);
/* Same, with a caller-owned scratch buffer: layers with few output tiles and a long reduction (the deep U-Net levels)
 * split K over workgroups and need room for their f32 partial sums (8 * B*Ho*Wo * Cout floats always suffice; with
 * less the split is reduced). mpu_unet_forward / backward pass their workspace the same way. */
int mpu_conv2d_igemm_ws(int32_t dtype, int32_t mode, const void* d_in0, int32_t C0,
                     const void* d_in1, int32_t C1, const void* d_w_packed,
                     int64_t w_tap_stride, int32_t w_row_stride, const float* d_bias,
                     const void* d_mask, void* d_out, int32_t B, int32_t Ho, int32_t Wo,
                     int32_t Cout, int32_t relu, float* d_workspace, int64_t workspace_floats, void* stream);
int64_t mpu_conv2d_wgrad_workspace_floats(int32_t mode, int32_t Cin, int32_t Cout, int64_t M);
/* Planning queries (host arithmetic only, no GPU needed): the floats ONE layer's weight-gradient job writes into its scratch
 * region (K-split / strip partials of dW + bias-gradient partial rows) when it runs stand-alone (grouped = 0) or inside a
 * grouped launch (grouped = 1: fewer strips / splits but other schedule thresholds, so either can be the larger), and the
 * region mpu_unet_workspace_bytes() reserves for that layer (>= both). tests/test_host_geometry.py sweeps shapes over them. */
int64_t mpu_conv2d_wgrad_job_floats(int32_t dtype, int32_t mode, int32_t B, int32_t Ho, int32_t Wo, int32_t C0, int32_t C1,
                                    int32_t Cout, int32_t grouped);
int64_t mpu_conv2d_wgrad_scratch_floats(int32_t dtype, int32_t mode, int32_t B, int32_t Ho, int32_t Wo, int32_t C0, int32_t C1,
                                        int32_t Cout);
int mpu_conv2d_wgrad(int32_t dtype, int32_t mode, const void* d_x0, int32_t C0, const void* d_x1,
                     int32_t C1, const void* d_dz, int32_t Cout, int32_t B, int32_t Ho, int32_t Wo,
                     float* d_workspace, float* d_dW, void* stream);

/* Weight and bias gradient of the FIRST layer (Conv2D(F, 3) on the n_channels-channel input image,
 * mpunet/models/unet.py:120-123): d_x holds the image in 8-channel pixel records of which the first
 * n_image_channels are real (the rest zero). d_dW is the fp32 kernel gradient [9][8][Cout] (zeros for the padding
 * channels), d_db (optional) the bias gradient [Cout]. With 1-2 image channels in bf16 this is a dedicated HBM-bound
 * kernel (wgrad_c8.hip); other shapes take the general path. Workspace: ..._workspace_floats(Cout, B*H*W) floats. */
int64_t mpu_conv2d_wgrad_first_layer_workspace_floats(int32_t Cout, int64_t M);
int mpu_conv2d_wgrad_first_layer(int32_t dtype, const void* d_x, int32_t n_image_channels, const void* d_dz,
                                 int32_t Cout, int32_t B, int32_t H, int32_t W, float* d_workspace, float* d_dW,
                                 float* d_db, void* stream);

/* Epoch-end validation counting (Validation._count_cm_elements_from_queue, mpunet/callbacks/validation.py:115-125):
 * p = argmax over the class axis of d_pred [n][n_classes] (f32 scores; first maximum, NaN counts as the maximum, as
 * np.argmax), then per class TP = #(y == p == c), relevant = #(y == c), selected = #(p == c), ADDED to
 * d_counts [3][n_classes] (int64; the caller zeroes it at the start of an epoch and may SUM all-reduce it across
 * replicas). Targets >= n_classes count for no class. Integer work: exact and order-independent. 1 <= n_classes <= 16. */
int mpu_validation_count(const float* d_pred, const uint8_t* d_y, int64_t n, int32_t n_classes, int64_t* d_counts,
                         void* stream);

/* Training metrics (`fit.metrics`; Trainer.compile_model, mpunet/train/utils.py:29-97), accumulated on the device: each call
 * is one batch of a Keras Mean-wrapped function metric. p = argmax over the class axis of d_pred [n][n_classes] (f32 scores,
 * probabilities or logits; first maximum, as tf.argmax), y = d_y [n]; per class tp = #(y == p == c), rel = #(y == c),
 * sel = #(p == c); Kb = 1 + the largest c with rel + sel > 0 (tf.math.confusion_matrix sized from the data). The step's
 * values, in f64 from the exact integers (0 / 0 = NaN, never filtered), are ADDED to the state:
 *
 *   index  name                          total[index] +=                                  count[index] +=
 *   0      sparse_categorical_accuracy   sum_c tp                                         n
 *   1      sparse_fg_recall              sum_{c>=1} tp / sum_{c>=1} rel                   1
 *   2      sparse_fg_precision           sum_{c>=1} tp / sum_{c>=1} sel                   1
 *   3      sparse_mean_fg_precision      mean_{c=1..Kb-1} tp/sel                          1
 *   4      sparse_mean_fg_recall         mean_{c=1..Kb-1} tp/rel                          1
 *   5      sparse_mean_fg_f1             mean_{c=1..Kb-1} 2pr/(p+r), p = tp/sel, r = tp/rel    1
 *
 * The metric's value over the calls so far is total / count (0 where count == 0). State buffer (8-byte aligned,
 * mpu_train_metrics_state_bytes() bytes): f64 total[6] at byte 0, f64 count[6] at byte 48, then private scratch that the call
 * leaves zeroed. An all-zero buffer is a fresh state; zeroing it resets every metric. Two launches (count, then a one-wave
 * finalize), no host synchronisation, nothing else read or written: the call may be captured into a HIP graph and replayed.
 * Targets >= n_classes count for no class. n == 0 is a no-op. 1 <= n_classes <= 16. */
int64_t mpu_train_metrics_state_bytes(void);
int mpu_train_metrics_update(const float* d_pred, const uint8_t* d_y, int64_t n, int32_t n_classes, void* d_state,
                             void* stream);

/* The compiled loss of one batch from its probabilities, with no training step around it (Model.evaluate / test_on_batch; the
 * batch-wise val_loss of the Validation callback, mpunet/callbacks/validation.py:148-206). d_pred f32 [B, ppi, n_classes]
 * probabilities (the output of mpu_unet_forward), d_y [B, ppi], d_sw [B] per-image weights or NULL (= ones). cfg: any
 * mpu_loss_kind. The five per-image kinds give L_b exactly as the train step reports it for the same probabilities (the same
 * kernels). MPU_LOSS_SPARSE_CE: L_b = the mean over the image's pixels of the Keras form on clipped probabilities,
 * -log q_y + log sum_k q_k with q = clip(p, 1e-7, 1 - 1e-7) (the second term is what TF's softmax cross-entropy makes of the
 * clipped row; it is zero unless the clip moved an entry), so that mean_b w_b L_b is the mean over all B * ppi pixels that Keras
 * logs for the flattened output. Outputs, each optional: d_loss [B] = w_b * L_b; d_acc f64 [2]: d_acc[0] += mean_b(w_b L_b),
 * d_acc[1] += 1 (a Keras Mean over batches; zero it to start, SUM all-reduce it across replicas).
 * 1 <= n_classes <= 8, 1 <= B <= 65535, 1 <= ppi <= 2^40, else MPU_EUNSUPPORTED; a NULL or misaligned (8 bytes: d_scratch, d_acc)
 * argument or a bad cfg: MPU_EINVAL. A label >= n_classes enters no sum and indexes nothing. d_scratch:
 * mpu_eval_loss_scratch_bytes(B, ppi, n_classes) bytes (< 0 + mpu_last_error() outside the ranges above), contents irrelevant
 * before and after. Two launches, f64 sums in a fixed order and no atomics (two calls on the same input give the same bits), no
 * host synchronisation, nothing read or written but the arguments: the call may be captured into a HIP graph. */
int64_t mpu_eval_loss_scratch_bytes(int32_t B, int64_t ppi, int32_t n_classes);
int mpu_eval_loss(const mpu_loss_config* cfg, const float* d_pred, const uint8_t* d_y, const float* d_sw, int32_t B, int64_t ppi,
                  int32_t n_classes, void* d_scratch, float* d_loss, double* d_acc, void* stream);
/* MPU_LOSS_SPARSE_CE_LOGITS of one batch: mpu_eval_loss reads probabilities and keeps refusing kind 6; this entry reads d_logits f32
 * [B, ppi, n_classes], the output of a handle created with softmax == 0. L_b = the mean over the image's pixels of
 * logsumexp_k(z_k) - z_y, formed in f64 from the f32 logits with the maximum subtracted. Everything else -- d_y, d_sw, d_loss, d_acc,
 * the ranges, the scratch size (mpu_eval_loss_scratch_bytes), the chunking and the fixed summation order, the skip of labels
 * >= n_classes, the error codes -- is mpu_eval_loss's. */
int mpu_eval_loss_logits(const float* d_logits, const uint8_t* d_y, const float* d_sw, int32_t B, int64_t ppi, int32_t n_classes,
                         void* d_scratch, float* d_loss, double* d_acc, void* stream);

/* Connected components of a resident label volume, and the one post-processing step of `mp predict` (--largest_component; no
 * reference counterpart): for every foreground class keep its largest connected component, send the rest to background.
 * d_labels u8 [X][Y][Z] in C order (shape = {X, Y, Z}); connectivity 6, 18 or 26 = scipy.ndimage.generate_binary_structure(3, 1 / 2 / 3).
 * Two voxels are connected when they are neighbours under that structure and carry the same label c with 1 <= c < n_classes;
 * label 0 and labels >= n_classes join no component and are never rewritten. All classes are labelled in one pass. A component
 * is named by the linear C-order index of its first voxel (its smallest index), so the result does not depend on scheduling.
 *
 * mpu_label_components: d_roots i32 [X * Y * Z]: d_roots[i] = the name of voxel i's component, or -1 where the label joins none.
 * mpu_keep_largest_components: d_out u8 [X][Y][Z] = d_labels, except that the voxels of a class whose bit is set in class_mask
 *   (bit c = class c) that lie outside that class's winning component become 0. The winner is the largest component; among
 *   equally large ones the one with the smallest first index (np.argmax(np.bincount(...)) over ndimage.label's numbering).
 *   d_out == d_labels (in place) is allowed, any other overlap is MPU_EINVAL. d_report i64 [n_classes][3]: components found,
 *   voxels kept, voxels removed; the row of an unmasked class reports its components and voxels with removed = 0, row 0 is zero.
 * Counts, names, the selection and the output are exact integers: two calls give identical bytes.
 * MPU_EUNSUPPORTED: n_classes outside [1, 16], a dimension < 1, X * Y * Z outside [1, 2^31 - 1] (i32 indices). MPU_EINVAL:
 * connectivity not in {6, 18, 26}; bit 0 or a bit >= n_classes set in class_mask; a NULL or misaligned pointer (d_roots 4,
 * d_report 8, d_scratch 16 bytes; the label volumes need no alignment, 16 bytes gives the vector path). Every check precedes the
 * first HIP call. d_scratch: mpu_components_scratch_bytes(shape) bytes (-1 + mpu_last_error() outside the ranges above), caller-owned,
 * contents irrelevant before and after; nothing outside it and the named outputs is written. A fixed sequence of launches
 * (4 / 7) on `stream`, no host synchronisation, no memset: the calls may be captured into a HIP graph. */
int64_t mpu_components_scratch_bytes(const int64_t shape[3]);
int mpu_label_components(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes,
                         int32_t* d_roots, void* d_scratch, void* stream);
int mpu_keep_largest_components(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes,
                                uint32_t class_mask, uint8_t* d_out, int64_t* d_report, void* d_scratch, void* stream);

/* Two more filters of a resident label map on the same labelling (`mp predict --min_component_voxels`, `--fill_holes`; no reference
 * counterpart). Shapes, classes, connectivity, class_mask, d_out (d_labels itself or no overlap), alignment, error codes and the
 * order of the checks are those of mpu_keep_largest_components; labels >= n_classes ("foreign") are never rewritten, are not
 * background, belong to no class and cast no vote. All results are exact integers: two calls give identical bytes.
 *
 * mpu_remove_small_components: d_out = d_labels, except that every connected component (under `connectivity`) of a class in
 *   class_mask with fewer than min_voxels voxels becomes 0. min_voxels >= 1 (else MPU_EINVAL); 1 is the identity. d_report i64
 *   [n_classes][3]: components found, voxels kept, voxels removed; an unmasked class reports removed = 0, row 0 is zero. 7 launches.
 *   d_scratch: mpu_components_scratch_bytes(shape).
 * mpu_fill_holes: the background is {label == 0}. A CAVITY is a connected component of the background under `connectivity` (6 is
 *   scipy.ndimage.binary_fill_holes' default structure) that contains no voxel with an index of 0 or dim - 1 on any axis -- a volume
 *   with a dimension of 1 has none. Each cavity is filled whole with the winner of a face vote: the pairs (p in the cavity, q one of
 *   the six face neighbours of p inside the volume) with 1 <= label(q) < n_classes are counted per class; the largest count wins, a
 *   tie goes to the smallest class. A cavity without a vote, or whose winner is not in class_mask, is left as it is. d_report i64
 *   [n_classes][2]: cavities and voxels given to class c; row 0: cavities and voxels left unfilled. With n_classes = 2 and
 *   class_mask = 2 the result is binary_fill_holes(labels == 1, generate_binary_structure(3, level)). 9 + 2 (n_classes - 1) launches
 *   (one vote and one fold per class, integer atomics). d_scratch: mpu_fill_holes_scratch_bytes(shape) bytes (25 per voxel and a
 *   header; -1 + mpu_last_error() outside the ranges).
 * Scratch is caller-owned, contents irrelevant before and after; nothing outside it and the named outputs is written. A fixed
 * sequence of launches on `stream`, no host synchronisation, no memset: the calls may be captured into a HIP graph. */
int64_t mpu_fill_holes_scratch_bytes(const int64_t shape[3]);
int mpu_remove_small_components(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes,
                                uint32_t class_mask, int64_t min_voxels, uint8_t* d_out, int64_t* d_report, void* d_scratch,
                                void* stream);
int mpu_fill_holes(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes, uint32_t class_mask,
                   uint8_t* d_out, int64_t* d_report, void* d_scratch, void* stream);

/* Exact Euclidean distance transform of a resident label volume with anisotropic voxel spacing, and the surface-distance table of
 * `mp predict --surface_metrics` (no reference counterpart; the host route is scipy.ndimage.distance_transform_edt twice per class).
 * d_labels u8 [X][Y][Z] in C order (shape = {X, Y, Z}), no alignment required; spacing = {sx, sy, sz}, finite and > 0.
 * The FEATURE voxels (the targets distances are measured to) are chosen by a predicate on the labels:
 *   MPU_EDT_EQUAL label == value, MPU_EDT_NOT_EQUAL label != value, MPU_EDT_BORDER the border voxels of the mask label == value:
 *   in the mask with at least one of the six face neighbours outside it, a neighbour outside the volume counting as outside the
 *   mask (M & ~binary_erosion(M, generate_binary_structure(3, 1)), scipy's border_value = 0; the surface medpy's hd / assd use).
 *
 * mpu_edt_squared: d_out f64 [X][Y][Z]: for every voxel p
 *     d2(p) = min over feature voxels q of fl( fl(wx dx^2) + fl( fl(wy dy^2) + fl(wz dz^2) ) ),   w_a = fl(spacing_a * spacing_a),
 *   dx, dy, dz the index differences, their squares converted to f64, every fl one rounded f64 operation (no FMA). +inf everywhere
 *   when no voxel is a feature. The three separable passes each take the true minimum of their line, so the result IS this
 *   all-pairs minimum, bit for bit. take_root != 0 stores sqrt(d2) instead (the device's sqrt).
 * mpu_surface_table: d_pred, d_truth u8 label volumes of the same shape; for every class c whose bit is set in class_mask
 *   (classes 1 .. n_classes - 1; a label >= n_classes belongs to no class), with bP / bT the border voxels of pred == c / truth == c,
 *   D_T / D_P the squared transforms to bT / bP and the two directed lists D_T[bP], D_P[bT], row c of d_table ([n_classes][8] words
 *   of 8 bytes) holds
 *     [0] i64 |bP|   [1] i64 |bT|   [2] i64 how many entries of both lists are <= fl(tolerance * tolerance)
 *     [3] f64 the maximum of both lists   [4] f64 sum of sqrt over D_T[bP]   [5] f64 sum of sqrt over D_P[bT]
 *     [6], [7] f64 the two order statistics (of both lists together, SQUARED values) that np.percentile(., 95) (linear method)
 *     interpolates between: ranks floor(vi) and floor(vi) + 1 with vi = fl((n - 1) * 0.95), n = [0] + [1], both the last element
 *     when vi >= n - 1. Found by an exact radix select on the bit patterns.
 *   All rows of classes not asked for (and row 0) are zero. Counts, [3], [6] and [7] are exact; the sums are two-stage f64 sums in a
 *   fixed order: two calls give identical bytes. An empty border set leaves +inf in the other direction's list; the caller applies its
 *   convention (surface.py: NaN). HD = sqrt([3]), ASSD = ([4] / [0] + [5] / [1]) / 2, NSD = [2] / ([0] + [1]).
 * MPU_EUNSUPPORTED: n_classes outside [1, 16], a dimension < 1, X * Y * Z outside [1, 2^31 - 1]. MPU_EINVAL: a spacing or tolerance
 * that is not finite and > 0; an unknown predicate; value outside 0 .. 255; bit 0 or a bit >= n_classes in class_mask; a NULL or
 * misaligned pointer (d_out / d_table 8, d_scratch 16 bytes). Every check precedes the first HIP call. d_scratch:
 * mpu_surface_scratch_bytes(shape) bytes (-1 + mpu_last_error() outside the ranges above; 32 bytes per voxel, 5 per Z line, a header),
 * caller-owned, contents irrelevant before and after; nothing outside it and the named outputs is written. A fixed sequence of
 * launches on `stream`, no host synchronisation, no memset. */
enum { MPU_EDT_EQUAL = 0, MPU_EDT_NOT_EQUAL = 1, MPU_EDT_BORDER = 2 };
int64_t mpu_surface_scratch_bytes(const int64_t shape[3]);
int mpu_edt_squared(const uint8_t* d_labels, const int64_t shape[3], const double spacing[3], int32_t predicate, int32_t value,
                    int32_t take_root, double* d_out, void* d_scratch, void* stream);
int mpu_surface_table(const uint8_t* d_pred, const uint8_t* d_truth, const int64_t shape[3], const double spacing[3], int32_t n_classes,
                      uint32_t class_mask, double tolerance, void* d_table, void* d_scratch, void* stream);

/* Opening and closing of the classes of a resident label map by a Euclidean ball (`mp predict --open_mm / --close_mm`; no reference
 * counterpart), as two thresholds of the exact transform above -- hence in the units of `spacing`, correct on anisotropic voxels.
 * With r2 = fl(radius * radius) and d2 as mpu_edt_squared defines it (same weights, one rounded operation each):
 *   dilate(M) = {p : d2(p, M) <= r2}   erode(M) = {p : d2(p, not M) > r2}   close = erode(dilate(M))   open = dilate(erode(M)).
 * Distances are measured to voxels inside the volume only and nothing is assumed outside it: an object on the volume face is not
 * shaved there (unlike scipy's border_value = 0). No feature voxel gives +inf: an empty mask stays empty, a full one full.
 * The classes of class_mask are processed in ascending order, each on the map the earlier ones left: MPU_MORPH_CLOSE sets to c only
 * voxels whose current label is 0 (never another class or a foreign label), MPU_MORPH_OPEN sets to 0 only voxels of class c. d2 is
 * symmetric in its two voxels, so closing is extensive and opening anti-extensive, exactly. d_report i64 [n_classes][2]: voxels
 * added, voxels removed (rows of classes not asked for, and row 0, are zero). d_out == d_labels (in place) is allowed, any other
 * overlap is MPU_EINVAL. Every comparison is exact: two calls give identical bytes.
 * MPU_EUNSUPPORTED / MPU_EINVAL as mpu_surface_table, and MPU_EINVAL for an unknown op, a radius that is not finite and > 0, a
 * misaligned d_report (8 bytes). Every check precedes the first HIP call. d_scratch: mpu_surface_scratch_bytes(shape) bytes (the two
 * f64 volumes of the transform; the one-byte mask between the two transforms lies in the key-list region), caller-owned, contents
 * irrelevant before and after; nothing outside it and the named outputs is written. 1 + 12 launches per class on `stream`, no host
 * synchronisation, no memset. */
enum { MPU_MORPH_OPEN = 0, MPU_MORPH_CLOSE = 1 };
int mpu_morph_ball(const uint8_t* d_labels, const int64_t shape[3], const double spacing[3], int32_t n_classes, uint32_t class_mask,
                   int32_t op, double radius, uint8_t* d_out, int64_t* d_report, void* d_scratch, void* stream);

/* Measurement aid (bench.py roofline leg; no reference counterpart): when
 * enabled, every MFMA convolution launch is bracketed by HIP events recorded on
 * its own stream. mpu_profile_summary synchronises on them and returns the summed
 * kernel time, the summed ALGORITHMIC FLOPs (2*M*N*K of the reference's layer,
 * SURVEY.md 8d) and the launch count. kind 0 = conv_igemm (forward + data
 * gradient), 1 = wgrad_igemm. mpu_profile_enable(0|1) also clears the records. */
int mpu_profile_enable(int32_t on);
int mpu_profile_summary(int32_t kind, double* total_ms, double* total_flops, int64_t* launches);

/* Test aid: the geometry kernels decide cells / nearest neighbours with a closed form on uniform axes wherever that
 * is provably the exact answer (coordinate farther than 1e-6 index units from every decision boundary) and run the
 * exact NumPy-order search otherwise. on = 0 forces the exact search for every sample (equality tests, A/B);
 * the environment variable MPU_GEOM_FAST=0 sets the same at first use. */
int mpu_geometry_set_fast_path(int32_t on);

/* Test aid for the plane sampler's cell division (csrc/geometry.hip cell_div): evaluates `count` pseudo-random
 * quotients (x - g[c]) / (g[c+1] - g[c]) on the closed-form axis both ways and returns in *n_bad how many differ
 * from the IEEE `/` (must be 0). Synchronous; default stream. */
int mpu_geometry_check_cell_division(const mpu_axis* axis, int64_t count, uint64_t seed, uint64_t* n_bad);

/* Measured machine peaks quoted next to the spec peaks in bench.py's roofline objects. The caller times
 * the launches with events on `stream`. mpu_probe_mfma_bf16: `blocks` workgroups x 4 waves each issue iters x 8
 * independent v_mfma_f32_32x32x16_bf16 (no memory traffic); *flops = FLOPs executed. mpu_probe_stream_triad:
 * a = b + 1.5 c over n floats (n % 4 == 0), 12 * n bytes of HBM traffic. */
int mpu_probe_mfma_bf16(int32_t blocks, int32_t iters, float* d_sink, double* flops, void* stream);
/* the same loop on pseudo-random bf16 operands: the matrix rate the part sustains under its POWER limit on real data */
int mpu_probe_mfma_bf16_random(int32_t blocks, int32_t iters, float* d_sink, double* flops, void* stream);
int mpu_probe_stream_triad(float* d_a, const float* d_b, const float* d_c, int64_t n, void* stream);
/* dst = src over n floats (n % 4096 == 0), 16 bytes per lane, four float4s per thread in flight: 8 * n bytes of HBM traffic -- the
 * "float4 copy" MI355X_MICROARCH.md quotes at 6.29 TB/s. variant 0: default cache policy; 1: non-temporal loads and stores;
 * 2: default policy, grid-stride. */
int mpu_probe_stream_copy(float* d_dst, const float* d_src, int64_t n, int32_t variant, void* stream);
/* Measurement aid: the n floats of d_src (n a power of two >= 8192) read once, in runs of run_bytes contiguous bytes (a power of
 * two >= 16) visited in a scattered order; per-thread sums to d_out (n / 32 floats). What HBM delivers to a kernel whose requests
 * are coalesced but whose DRAM pages are opened out of order (the gather kernels of fuse_and_predict.py:92-137). */
int mpu_probe_permuted_read(const float* d_src, float* d_out, int64_t n, int32_t run_bytes, void* stream);
/* out[i] = x[3i] + x[3i+1] + x[3i+2]: 12 contiguous bytes per lane, 12 n bytes read exactly once -- the access width of
 * the fused back-mapping's K = 3 gathers; calibrates rocprofv3's FETCH_SIZE for that width (MI355X_MICROARCH.md: the
 * gfx950 x2 correction is established for 16-byte accesses only). */
int mpu_probe_gather12(const float* d_x, float* d_out, int64_t n, void* stream);
/* Shader-clock sampler (measurement aid): ONE wave writes n pairs (s_memtime = shader cycles, s_memrealtime = 100-MHz ticks)
 * into d_samples [2 n] u64, about naps x 8 k cycles apart. Launch it on a side stream next to the work of interest; the
 * effective clock of a window is d(cycles) / d(ticks) x 100 MHz. bench.py reports it for its timed regions. */
int mpu_probe_clock(uint64_t* d_samples, int32_t n, int32_t naps, void* stream);

/* Test aid (no reference counterpart): when enabled, every convolution / weight-gradient launch appends one text
 * line naming the kernel schedule the dispatcher chose for the layer shape ("conv halo mode=0 B=.. H=.. W=.. Cin=..
 * Cout=.. dgrad=0", "wgrad taps ... ksplit=.."), so that parity tests at the BASELINE shapes can assert that the
 * schedules bench.py times are the ones they checked. mpu_schedule_log_enable(0|1) clears the log;
 * mpu_schedule_log_read copies it (NUL-terminated, truncated to cap) and returns its full length. */
int mpu_schedule_log_enable(int32_t on);
int64_t mpu_schedule_log_read(char* buf, int64_t cap);

/* Environment switches (csrc/env.h: the library's only getenv; schedule / fusion on-off pairs for A/B runs, dev aids). One line
 * per switch, "NAME\tvalue in force\tdefault\twhat it does", NUL-terminated and truncated to cap; returns the full length.
 * Values are read once per process, at the first query. */
int64_t mpu_env_describe(char* buf, int64_t cap);

/* Dev aid: with MPU_STAMPS=1 in the environment a few workgroups of the instrumented kernels (conv_halo8, wgrad_taps)
 * record s_memtime stamps at their phase boundaries (entry, prologue landed, main loop done, stores issued) into a
 * 64 x 8 table of uint64 (slot = a function of the workgroup index). Reads and clears it (synchronises the device). */
int mpu_debug_stamps_read(uint64_t* host_out, int32_t n);

/* Test aid (no reference counterpart): teacher-forced replay of a train step. While a tap is installed on a model,
 * mpu_unet_forward(training) / mpu_unet_backward call it right after enqueueing every convolution launch with the
 * device pointers and shapes of that launch, so that a test can synchronise the stream, copy the launch's OWN inputs
 * and output out of the workspace and compare the output with an independent fp64 convolution of exactly those
 * inputs -- launch by launch, without the error amplification of the train-mode network between them
 * (tests/test_gpu_replay.py). kind: 0 forward conv (out = relu(conv(in0|in1) + bias)), 1 data gradient
 * (out = conv^T(dz) restricted to input channels [n_off, n_off + n_cnt), times the ReLU mask 1[mask > 0] when mask
 * is set), 2 weight gradient (x = in0|in1, dz; the result lands in the flat gradient buffer at float offset w_off
 * once the backward pass has returned). H, W = resolution of the launch's OUTPUT (kind 0/1) or of dz (kind 2).
 * Round 4: the NON-convolution launches of the step report too (their inputs and outputs are final when the callback runs):
 *   kind 3  BatchNormalization forward, training (mpunet/models/unet.py:127,144,165,176): in0 = x [B,H,W,C0], out = y
 *           (= gamma * xhat + beta), mask = the 2x2 max-pooled y of an encoder level (or NULL), aux0 / aux1 = batch mean /
 *           1/sqrt(var + eps) (f32 [C0]), w_off / b_off = float offsets of gamma / beta in the flat parameter buffer; the launch
 *           also writes the folded scale and shift, f32 [C0] each, directly behind aux1 (aux0 .. aux0 + 4 C0 floats are the
 *           BatchNorm's "stats.bn/<index>" entry of mpu_unet_workspace_region_info: mean, invstd, scale, shift);
 *   kind 4  BatchNormalization backward: in0 = dn, in1 = x (the layer's post-ReLU input), out = dz = 1[x > 0] * d(x),
 *           aux0 / aux1 = saved mean / invstd; dgamma / dbeta land at w_off / b_off of the flat GRADIENT buffer;
 *   kind 5  MaxPooling2D backward + skip add: in0 = n (the level's BN output), in1 = dskip, dz = dp (gradient of the pooled
 *           tensor [B,H/2,W/2,C0]), out = dn = dskip + unpool(dp) (routed to the FIRST maximum of each window);
 *   kind 6  1x1 head forward: in0 = n [B,H,W,C0], out = probabilities f32 [B,H,W,Cout] (softmax of n @ Wh + bh; Wh at w_off
 *           with row stride Cout, bh at b_off);
 *   kind 7  head backward (Keras sparse CE on clipped probabilities, sum gradient): in0 = n, in1 = probabilities (f32),
 *           dz = labels (u8 [B,H*W]), mask = per-image sample weights (f32 [B]) or NULL, out = dn [B,H,W,C0]; dWh / dbh land
 *           at w_off / b_off of the gradient buffer.
 * The inference forward (mpu_unet_forward, training = 0) reports as well: a conv without a BatchNorm as kind 0, the separate
 * head kernel as kind 6, and
 *   kind 8  conv forward with the folded BatchNormalization of inference: fields as kind 0 (relu = 1) and
 *           out = post_scale * relu(conv(in0|in1) + bias) + post_shift; aux0 / aux1 = the device post_scale / post_shift
 *           (f32 [Cout], written by mpu_unet_prepare_inference), n_off = index of that BatchNorm; mask = the 2x2 max pooling
 *           of out [B,H/2,W/2,Cout] if the schedule wrote it from its epilogue (else NULL); dz = the partial logits
 *           (f32 [2][B*H*W][n_classes]: the 1x1 head, without its bias, over channels 0..31 / 32..63 of the rounded output) if
 *           the head rode in the epilogue (else NULL) -- then out = NULL: the output tensor is not stored;
 *   kind 9  separate MaxPooling2D forward: in0 = y [B,H,W,C0], out = its 2x2 max pooling [B,H/2,W/2,C0]; conv_index = the
 *           BatchNorm whose output y is;
 *   kind 10 head combine: in0 = the partial logits f32 [2][B*H*W][Cout] of a kind-8 launch, out = probabilities f32
 *           [B,H,W,Cout] (softmax of partial[0] + partial[1] + bh; bh at b_off, Wh at w_off).
 * Two forms of the train step are NOT taken while a tap is installed -- the fused training head (head_bn_forward /
 * head_bn_backward / head_bn_bwd_apply) and the pool-backward recompute (launch_maxpool_bwd_bn) -- unless
 * mpu_unet_set_launch_tap_fused(m, 1) asks for them (default 0: the tapped step is the unfused one, launch for launch). They report as
 *   kind 3  also for the fused head's BatchNormalization, with out = NULL (its y is not stored): statistics, w_off / b_off as above;
 *   kind 11 head_bn_forward: in0 = c3 [B,H,W,64] (the BatchNorm's input), out = probabilities f32 [B,H,W,Cout], aux0 / aux1 = batch
 *           mean / invstd with scale and shift directly behind (as kind 3), w_off / b_off = Wh / bh, conv_index = that BatchNorm;
 *   kind 12 head_bn_backward + head_bn_bwd_apply, ONE record after both launches: in0 = c3, in1 = probabilities, dz = labels,
 *           mask = sample weights or NULL, out = dz3 = 1[c3 > 0] * d(c3), aux0 / aux1 = mean / invstd, aux2 = the [3][64]
 *           BatchNorm-backward coefficients k1 | k2 | k3 the launch wrote, w_off / b_off = Wh / bh (dWh / dbh in the gradient
 *           buffer; dgamma / dbeta at the gamma / beta offsets of that BatchNorm's kind-3 record), conv_index = that BatchNorm;
 *   kind 13 launch_maxpool_bwd_bn (both kernels), ONE record: in0 = x (the level's BatchNorm input), in1 = dskip, dz = dp
 *           [B,H/2,W/2,C0], mask = the level's STORED BatchNorm output n (the launch does not read it: a reference takes its
 *           arg-max from it), out = dz of the level's second conv, aux0 / aux1 = mean / invstd (+ scale, shift), aux2 = k1 | k2 | k3
 *           [3][C0], w_off / b_off = gamma / beta offsets (dgamma / dbeta in the gradient buffer), conv_index = that BatchNorm.
 * The callback runs on the calling thread; NULL removes the tap. Not for use under graph capture. */
typedef struct mpu_launch_info {
    int32_t kind, conv_index, mode, dtype;      /* mode: 0 3x3, 1 up-conv 2x2, 3 1x1 (the LAYER's mode); kinds >= 3: conv_index = BN index */
    int32_t B, H, W, C0, C1, Cout;              /* C0/C1: channels of in0/in1 (kind 1: C0 = channels of dz) */
    int32_t n_off, n_cnt, relu, _pad;
    const void* in0; const void* in1; const void* dz; const void* mask; const void* out;
    int64_t w_off, b_off;                       /* float offsets of the layer's kernel / bias in the flat buffers */
    const void* aux0; const void* aux1;         /* kinds 3, 4, 11-13: batch mean, 1/sqrt(var + eps); kind 8: post_scale, post_shift */
    const void* aux2;                           /* kinds 12, 13: the BatchNorm-backward coefficients k1 | k2 | k3, f32 [3][C0] (else NULL) */
} mpu_launch_info;
typedef void (*mpu_launch_tap_fn)(void* user, const mpu_launch_info* info);
int mpu_unet_set_launch_tap(mpu_unet* m, mpu_launch_tap_fn fn, void* user);
/* on != 0: a tapped train step also takes the fused training head and the pool-backward recompute (kinds 11-13); 0 (default): not. */
int mpu_unet_set_launch_tap_fused(mpu_unet* m, int32_t on);

#ifdef __cplusplus
}
#endif
#endif /* MPUNET_HIP_H */
