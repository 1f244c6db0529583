// The per-image segmentation losses of mpunet/evaluate/loss_functions.py on the device (mpu_loss_config, mpu_unet_set_loss):
// SparseDiceLoss :80-112, SparseJaccardDistanceLoss :33-77, SparseGeneralizedDiceLoss :207-266, SparseFocalLoss :166-204,
// SparseExponentialLogarithmicLoss :115-163. The reference compiles them with reduction=NONE on the flattened output
// (bin/train.py:288,357): y_pred [B, H*W, K], reduction over the pixel axis, ONE value L_b per image, times sample_weight[b];
// the tape differentiates the sum over the batch, Keras logs the mean over the batch.
//
// Two launches in front of the head's backward kernels (whose per-pixel part, head_loss_grad in unet_ops.hip, reads the table):
//   head_loss_stats_kernel  probs, labels -> per (image, chunk of 4096 pixels) the f64 partial sums of
//                           I_k = sum [y=k] p_k, P_k = sum p_k, R_k = sum [y=k]  and  E = sum of the per-pixel term
//                           (focal: -cw_y (1-q)^gamma log q; exp-log: (-log q)^gamma_cross; q = clip(p_y, 1e-7, 1 - 1e-7));
//                           exp-log takes I and P on the clipped probabilities. (4K + 1) bytes per pixel.
//   head_loss_coef_kernel   one workgroup: chunk partials -> sums (fixed order), the [B][K][2] table (a, c) with
//                           dL_b/dp_mk = a_bk + [y_m = k] c_bk (+ the per-pixel term's own derivative, formed per pixel), L_b,
//                           d_loss[b] = w_b L_b and the logged mean. No host read: the step is captured into a HIP graph.
//                           Value-only mode (mpu_eval_loss, eval_loss.hip): coef and loss_mean NULL, sw NULL = ones, and the mean
//                           ADDED to a f64 accumulator acc = (sum of batch means, number of batches).
// Determinism: a chunk is a fixed set of pixels (the grid depends on the image size alone), a thread adds its 16 pixels in order, the
// workgroup reduces by a fixed butterfly and wave order, the coefficient step adds the chunks in order. All sums in f64: every
// addend of I, P is in [0, 1] and a row has at most H*W <= 2^25 of them, so a sum carries ~2^-53 * log2 of relative rounding error.
#include <cmath>
#include "kernels.h"

namespace mpu {

namespace {

constexpr int LOSS_CHUNK = 4096, LOSS_PPT = LOSS_CHUNK / 256;    // pixels per workgroup / per thread
constexpr float LOSS_EPS = 1e-7f;                                // the source writes 10e-8

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// part: [B][nchunk][3K + 1] = I[K], P[K], R[K], E
template <int K>
__global__ __launch_bounds__(256) void head_loss_stats_kernel(const float* __restrict__ probs, const uint8_t* __restrict__ y, long ppi,
                                                             int kind, float gamma, HeadLoss cwv, double* __restrict__ part) {
    constexpr int NS = 3 * K + 1;
    __shared__ double red[4][NS];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const bool clipped = kind == MPU_LOSS_EXP_LOG, regional = kind != MPU_LOSS_FOCAL;
    double sI[K], sP[K], sR[K], sE = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { sI[k] = 0.0; sP[k] = 0.0; sR[k] = 0.0; }
    const long base = (long)b * ppi;
    for (int i = 0; i < LOSS_PPT; ++i) {
        const long m = (long)chunk * LOSS_CHUNK + (long)i * 256 + threadIdx.x;
        if (m >= ppi) break;
        const int yy = y[base + m];
        float qy = 1.f, cwy = 1.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float p = probs[(base + m) * K + k];
            const float q = fminf(fmaxf(p, LOSS_EPS), 1.f - LOSS_EPS);
            const float v = clipped ? q : p;
            if (k == yy) { qy = q; cwy = cwv.cw[k]; }
            if (regional) {
                sP[k] += (double)v;
                if (k == yy) { sI[k] += (double)v; sR[k] += 1.0; }
            }
        }
        if (yy >= K) continue;                                   // a label outside the classes has no per-pixel term
        if (kind == MPU_LOSS_FOCAL) sE += -(double)cwy * head_pow_f64((double)(1.f - qy), (double)gamma) * log((double)qy);
        else if (kind == MPU_LOSS_EXP_LOG) sE += head_pow_f64(-log((double)qy), (double)gamma);
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double a = wave_sum(sI[k]), c = wave_sum(sP[k]), d = wave_sum(sR[k]);
        if (lane == 0) { red[wv][k] = a; red[wv][K + k] = c; red[wv][2 * K + k] = d; }
    }
    sE = wave_sum(sE);
    if (lane == 0) red[wv][3 * K] = sE;
    __syncthreads();
    if (threadIdx.x < NS) {
        const int s = threadIdx.x;
        part[((long)b * gridDim.x + chunk) * NS + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
    }
}

// scratch (doubles): part [B][nchunk][NS] | sums [B][NS] | term [B][K] | wl [B]
__global__ __launch_bounds__(256) void head_loss_coef_kernel(mpu_loss_config cfg, const float* __restrict__ sw, int B, int K, int nchunk,
                                                            double inv_ppi, double* __restrict__ scratch, float* __restrict__ coef,
                                                            float* __restrict__ d_loss, float* __restrict__ loss_mean,
                                                            double* __restrict__ acc) {
    const int NS = 3 * K + 1;
    double* part = scratch;
    double* sums = part + (long)B * nchunk * NS;
    double* term = sums + (long)B * NS;
    double* wl = term + (long)B * K;
    __shared__ double wmax[256];
    for (int i = threadIdx.x; i < B * NS; i += 256) {
        const int b = i / NS, s = i - b * NS;
        double t = 0.0;
        for (int c = 0; c < nchunk; ++c) t += part[((long)b * nchunk + c) * NS + s];
        sums[i] = t;
    }
    __syncthreads();
    // generalized Dice: 1 / R^2 or 1 / R is infinite for a class absent from the image and then becomes the largest finite weight
    // of the WHOLE [B, K] tensor (loss_functions.py:232-239: tf.reduce_max(new_weights), infinite entries counted as zero)
    double gmax = 0.0;
    if (cfg.kind == MPU_LOSS_GENERALIZED_DICE) {
        double mx = 0.0;
        for (int i = threadIdx.x; i < B * K; i += 256) {
            const double R = sums[(i / K) * NS + 2 * K + (i % K)];
            const double w = cfg.type_weight == MPU_GDL_SQUARE ? 1.0 / (R * R) : cfg.type_weight == MPU_GDL_SIMPLE ? 1.0 / R : 1.0;
            if (!isinf(w) && w > mx) mx = w;
        }
        wmax[threadIdx.x] = mx;
        __syncthreads();
        for (int i = 0; i < 256; ++i) gmax = wmax[i] > gmax ? wmax[i] : gmax;
    }
    for (int i = threadIdx.x; i < B * K; i += 256) {
        const int b = i / K, k = i - b * K;
        const double I = sums[b * NS + k], P = sums[b * NS + K + k], R = sums[b * NS + 2 * K + k];
        const double iK = 1.0 / (double)K;
        double a = 0.0, c = 0.0, t = 0.0;                        // dL/dp = a + [y=k] c ; t: the class's share of L_b
        if (cfg.kind == MPU_LOSS_DICE) {                         // 1 - mean_k (2I + s) / (P + R + s)
            const double s = cfg.smooth, U = P + R + s, A = 2.0 * I + s;
            t = -iK * A / U; a = iK * A / (U * U); c = -iK * 2.0 / U;
        } else if (cfg.kind == MPU_LOSS_JACCARD) {               // 1 - mean_k (I + s) / (P + R - I + s)
            const double s = cfg.smooth, V = P + R - I + s, A = I + s;
            t = -iK * A / V; a = iK * A / (V * V); c = -iK * (1.0 / V + A / (V * V));
        } else if (cfg.kind == MPU_LOSS_GENERALIZED_DICE) {      // 1 - mean_k 2 w I / (w (P + R) + 1e-6), w constant
            double w = cfg.type_weight == MPU_GDL_SQUARE ? 1.0 / (R * R) : cfg.type_weight == MPU_GDL_SIMPLE ? 1.0 / R : 1.0;
            if (isinf(w)) w = gmax;
            const double Dn = w * (P + R) + 1e-6;
            t = -iK * 2.0 * w * I / Dn; a = iK * 2.0 * w * w * I / (Dn * Dn); c = -iK * 2.0 * w / Dn;
        } else if (cfg.kind == MPU_LOSS_EXP_LOG) {               // weight_dice * mean_k (-log((2I + 1) / (P + R + 1)))^gamma_dice
            const double U = P + R + 1.0, A = 2.0 * I + 1.0, X = A / U, nl = -log(X), gd = cfg.gamma_dice;
            const double h = -(double)cfg.weight_dice * iK * gd * pow(nl, gd - 1.0) / X;     // d(share)/dX
            t = (double)cfg.weight_dice * iK * pow(nl, gd); a = -h * A / (U * U); c = 2.0 * h / U;
        }
        if (coef) { coef[2 * i] = (float)a; coef[2 * i + 1] = (float)c; }
        term[i] = t;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 256) {
        double L = (cfg.kind == MPU_LOSS_DICE || cfg.kind == MPU_LOSS_JACCARD || cfg.kind == MPU_LOSS_GENERALIZED_DICE) ? 1.0 : 0.0;
        for (int k = 0; k < K; ++k) L += term[b * K + k];
        const double E = sums[b * NS + 3 * K] * inv_ppi;         // pixel mean of the per-pixel term
        if (cfg.kind == MPU_LOSS_FOCAL) L += E;
        else if (cfg.kind == MPU_LOSS_EXP_LOG) L += (double)cfg.weight_cross * E;
        const double v = (sw ? (double)sw[b] : 1.0) * L;
        wl[b] = v;
        if (d_loss) d_loss[b] = (float)v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += wl[b];
        if (loss_mean) *loss_mean = (float)(s / (double)B);
        if (acc) { acc[0] += s / (double)B; acc[1] += 1.0; }
    }
}

inline int loss_chunks(long ppi) { return (int)((ppi + LOSS_CHUNK - 1) / LOSS_CHUNK); }

}  // namespace

long head_loss_scratch_doubles(int B, long ppi, int K) {
    const long NS = 3L * K + 1;
    return (long)B * loss_chunks(ppi) * NS + (long)B * NS + (long)B * K + B;
}

int launch_head_loss_coeffs(const mpu_loss_config& cfg, const float* probs, const uint8_t* y, const float* sw, int B, long ppi, int K,
                            double* scratch, float* coef, float* d_loss, float* loss_mean, hipStream_t st, double* acc) {
    if (cfg.kind <= MPU_LOSS_SPARSE_CE || cfg.kind > MPU_LOSS_EXP_LOG) return fail(MPU_EINVAL, "%s", "head loss: not a per-image loss kind");
    if (B < 1 || B > 65535) return fail(MPU_EUNSUPPORTED, "%s", "head loss: batch must be 1..65535");
    if (ppi < 1 || ppi > HEAD_LOSS_MAX_PPI) return fail(MPU_EUNSUPPORTED, "%s", "head loss: pixels per image must be 1..2^40");
    const int nchunk = loss_chunks(ppi);
    HeadLoss cwv{};
    for (int k = 0; k < 8; ++k) cwv.cw[k] = (cfg.n_class_weights > 0 && k < cfg.n_class_weights) ? cfg.class_weights[k] : 1.f;
    const float gamma = cfg.kind == MPU_LOSS_FOCAL ? cfg.gamma : cfg.gamma_cross;
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    switch (K) {
#define MPU_LOSS_CASE(KK) case KK: head_loss_stats_kernel<KK><<<grid, 256, 0, st>>>(probs, y, ppi, cfg.kind, gamma, cwv, scratch); break;
        MPU_LOSS_CASE(1) MPU_LOSS_CASE(2) MPU_LOSS_CASE(3) MPU_LOSS_CASE(4) MPU_LOSS_CASE(5) MPU_LOSS_CASE(6) MPU_LOSS_CASE(7) MPU_LOSS_CASE(8)
#undef MPU_LOSS_CASE
        default: return fail(MPU_EUNSUPPORTED, "%s", "head loss: 1..8 classes");
    }
    int rc = launch_ok();
    if (rc) return rc;
    head_loss_coef_kernel<<<1, 256, 0, st>>>(cfg, sw, B, K, nchunk, 1.0 / (double)ppi, scratch, coef, d_loss, loss_mean, acc);
    return launch_ok();
}

}  // namespace mpu
