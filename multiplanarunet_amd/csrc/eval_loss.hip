// mpu_eval_loss: the compiled loss of one batch from its probabilities alone -- no training step around it (Model.evaluate /
// test_on_batch, and the batch-wise val_loss of the Validation callback, mpunet/callbacks/validation.py:148-206).
//   the five per-image losses   the value path of unet_loss.hip as it stands (head_loss_stats_kernel + head_loss_coef_kernel in its
//                               value-only mode: no gradient table): L_b is what the train step reports for the same probabilities
//   sparse cross-entropy        the one kernel pair of this file, in the shape of that path: per (image, chunk of 4096 pixels) the
//                               f64 partial sum of the Keras form on clipped probabilities (oracle/unet_ref.py keras_sparse_ce; the
//                               per-pixel arithmetic of head_loss_grad<HL_CE>, unet_ops.hip): -log q_y + log sum_k q_k,
//                               q = clip(p, 1e-7, 1 - 1e-7) in f32, the logs in f64; then one finalize workgroup
// Determinism as in unet_loss.hip: a chunk is a fixed set of pixels, a thread adds its 16 pixels in order, fixed butterfly and wave
// order, chunks added in order. No atomics. (4K + 1) bytes per pixel, two launches, no host synchronisation.
#include <cmath>
#include "kernels.h"

namespace mpu {
namespace {

constexpr int CE_CHUNK = 4096, CE_PPT = CE_CHUNK / 256;          // pixels per workgroup / per thread (= unet_loss.hip's)
constexpr float CE_EPS = 1e-7f;

// part: [B][nchunk]
template <int K>
__global__ __launch_bounds__(256) void eval_ce_stats_kernel(const float* __restrict__ probs, const uint8_t* __restrict__ y, long ppi,
                                                           double* __restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const long base = (long)b * ppi;
    double s = 0.0;
    for (int i = 0; i < CE_PPT; ++i) {
        const long m = (long)chunk * CE_CHUNK + (long)i * 256 + threadIdx.x;
        if (m >= ppi) break;
        const int yy = y[base + m];
        if (yy >= K) continue;                                   // a label outside the classes: in no sum, and it indexes nothing
        double S = 0.0;
        float qy = 1.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float q = fminf(fmaxf(probs[(base + m) * K + k], CE_EPS), 1.f - CE_EPS);
            S += (double)q;
            if (k == yy) qy = q;
        }
        s += -log((double)qy) + log(S);
    }
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)b * gridDim.x + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// The cross-entropy from logits (MPU_LOSS_SPARSE_CE_LOGITS; the per-pixel value of head_loss_grad<HL_CE_LOGITS>, unet_ops.hip):
// logsumexp_k z_k - z_y in f64 from the f32 logits, the maximum subtracted. Same chunks, same order, same skip as above.
template <int K>
__global__ __launch_bounds__(256) void eval_ce_logits_stats_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ y, long ppi,
                                                                  double* __restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const long base = (long)b * ppi;
    double s = 0.0;
    for (int i = 0; i < CE_PPT; ++i) {
        const long m = (long)chunk * CE_CHUNK + (long)i * 256 + threadIdx.x;
        if (m >= ppi) break;
        const int yy = y[base + m];
        if (yy >= K) continue;                                   // a label outside the classes: in no sum, and it indexes nothing
        float z[K];
        float mx, zy;
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] = logits[(base + m) * K + k];
        mx = z[0]; zy = z[0];
#pragma unroll
        for (int k = 1; k < K; ++k) { mx = fmaxf(mx, z[k]); if (k == yy) zy = z[k]; }
        double S = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) S += exp((double)z[k] - (double)mx);
        s += log(S) - ((double)zy - (double)mx);
    }
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)b * gridDim.x + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup; scratch (doubles): part [B][nchunk] | wl [B]
__global__ __launch_bounds__(256) void eval_ce_finalize_kernel(const float* __restrict__ sw, int B, int nchunk, double inv_ppi,
                                                              double* __restrict__ scratch, float* __restrict__ d_loss,
                                                              double* __restrict__ acc) {
    const double* part = scratch;
    double* wl = scratch + (long)B * nchunk;
    for (int b = threadIdx.x; b < B; b += 256) {
        double t = 0.0;
        for (int c = 0; c < nchunk; ++c) t += part[(long)b * nchunk + c];
        const double v = (sw ? (double)sw[b] : 1.0) * (t * inv_ppi);
        wl[b] = v;
        if (d_loss) d_loss[b] = (float)v;
    }
    __syncthreads();
    if (threadIdx.x == 0 && acc) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += wl[b];
        acc[0] += s / (double)B; acc[1] += 1.0;
    }
}

int launch_eval_ce(const float* probs, const uint8_t* y, const float* sw, int B, long ppi, int K, double* scratch, float* d_loss,
                   double* acc, hipStream_t st, bool logits = false) {
    const int nchunk = (int)((ppi + CE_CHUNK - 1) / CE_CHUNK);
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    switch (K) {
#define MPU_CE_CASE(KK) case KK: if (logits) eval_ce_logits_stats_kernel<KK><<<grid, 256, 0, st>>>(probs, y, ppi, scratch); \
                                 else eval_ce_stats_kernel<KK><<<grid, 256, 0, st>>>(probs, y, ppi, scratch); break;
        MPU_CE_CASE(1) MPU_CE_CASE(2) MPU_CE_CASE(3) MPU_CE_CASE(4) MPU_CE_CASE(5) MPU_CE_CASE(6) MPU_CE_CASE(7) MPU_CE_CASE(8)
#undef MPU_CE_CASE
        default: return fail(MPU_EUNSUPPORTED, "%s", "mpu_eval_loss: 1..8 classes");
    }
    int rc = launch_ok();
    if (rc) return rc;
    eval_ce_finalize_kernel<<<1, 256, 0, st>>>(sw, B, nchunk, 1.0 / (double)ppi, scratch, d_loss, acc);
    return launch_ok();
}

bool eval_shape_ok(int B, long ppi, int K) { return B >= 1 && B <= 65535 && ppi >= 1 && ppi <= HEAD_LOSS_MAX_PPI && K >= 1 && K <= 8; }

}  // namespace
}  // namespace mpu

using namespace mpu;

// the per-image path's layout holds the cross-entropy's too (3K + 1 >= 4 doubles per chunk against one)
extern "C" int64_t mpu_eval_loss_scratch_bytes(int32_t B, int64_t ppi, int32_t n_classes) {
    if (!eval_shape_ok(B, (long)ppi, n_classes))
        return fail(MPU_EUNSUPPORTED, "%s", "mpu_eval_loss_scratch_bytes: need 1 <= B <= 65535, 1 <= ppi <= 2^40, 1 <= n_classes <= 8");
    return 8 * (int64_t)head_loss_scratch_doubles(B, (long)ppi, n_classes);
}

extern "C" int mpu_eval_loss(const mpu_loss_config* cfg, const float* d_pred, const uint8_t* d_y, const float* d_sw, int32_t B,
                             int64_t ppi, int32_t n_classes, void* d_scratch, float* d_loss, double* d_acc, void* stream) {
    MPU_REQUIRE(cfg && d_pred && d_y && d_scratch, "mpu_eval_loss: null argument");
    MPU_REQUIRE(cfg->kind != MPU_LOSS_SPARSE_CE_LOGITS, "mpu_eval_loss: reads probabilities; the cross-entropy from logits is mpu_eval_loss_logits");
    MPU_REQUIRE(cfg->kind >= MPU_LOSS_SPARSE_CE && cfg->kind <= MPU_LOSS_EXP_LOG, "mpu_eval_loss: unknown loss kind");
    MPU_REQUIRE(((uintptr_t)d_scratch & 7) == 0 && ((uintptr_t)d_acc & 7) == 0, "mpu_eval_loss: d_scratch and d_acc must be 8-byte aligned");
    if (!eval_shape_ok(B, (long)ppi, n_classes))
        return fail(MPU_EUNSUPPORTED, "%s", "mpu_eval_loss: need 1 <= B <= 65535, 1 <= ppi <= 2^40, 1 <= n_classes <= 8");
    if (cfg->kind == MPU_LOSS_GENERALIZED_DICE)
        MPU_REQUIRE(cfg->type_weight >= MPU_GDL_SQUARE && cfg->type_weight <= MPU_GDL_UNIFORM, "mpu_eval_loss: unknown type_weight");
    if (cfg->kind == MPU_LOSS_FOCAL)
        MPU_REQUIRE(cfg->n_class_weights == 0 || cfg->n_class_weights == n_classes, "mpu_eval_loss: class_weights needs 0 or n_classes entries");
    hipStream_t st = (hipStream_t)stream;
    if (cfg->kind == MPU_LOSS_SPARSE_CE)
        return launch_eval_ce(d_pred, d_y, d_sw, B, (long)ppi, n_classes, (double*)d_scratch, d_loss, d_acc, st);
    return launch_head_loss_coeffs(*cfg, d_pred, d_y, d_sw, B, (long)ppi, n_classes, (double*)d_scratch, nullptr, d_loss, nullptr, st,
                                   d_acc);
}

extern "C" int mpu_eval_loss_logits(const float* d_logits, const uint8_t* d_y, const float* d_sw, int32_t B, int64_t ppi,
                                    int32_t n_classes, void* d_scratch, float* d_loss, double* d_acc, void* stream) {
    MPU_REQUIRE(d_logits && d_y && d_scratch, "mpu_eval_loss_logits: null argument");
    MPU_REQUIRE(((uintptr_t)d_scratch & 7) == 0 && ((uintptr_t)d_acc & 7) == 0, "mpu_eval_loss_logits: d_scratch and d_acc must be 8-byte aligned");
    if (!eval_shape_ok(B, (long)ppi, n_classes))
        return fail(MPU_EUNSUPPORTED, "%s", "mpu_eval_loss_logits: need 1 <= B <= 65535, 1 <= ppi <= 2^40, 1 <= n_classes <= 8");
    return launch_eval_ce(d_logits, d_y, d_sw, B, (long)ppi, n_classes, (double*)d_scratch, d_loss, d_acc, (hipStream_t)stream, true);
}
