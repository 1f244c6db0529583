// Training metrics of `fit.metrics` (Trainer.compile_model, mpunet/train/utils.py:29-97): tf.keras.metrics
// sparse_categorical_accuracy and the five sparse_* functions of mpunet/evaluate/metrics.py:84-156, each inside a Keras Mean
// (total += sum(values), count += size(values)), accumulated ON THE DEVICE so that a replayed train step needs no host call.
// Two launches per step:
//   1. count     argmax + per-class TP / relevant / selected of the step's pixels into the state's scratch (class_counts.h: the
//                unit of the epoch-end validation; HBM-bound, 4K + 1 bytes per pixel; exact integers, order-independent)
//   2. finalize  one wave: the six step values in f64 from the integer counts, added to total / count, and the scratch zeroed
//                again -- so the next step (the next replay of a captured graph) needs no memset node between steps
// The kernel boundary between the two is what makes every workgroup's atomics visible to the finalize wave.
#include "kernels.h"
#include "class_counts.h"

namespace mpu {
namespace {

constexpr int TM_METRICS = 6;       // in the order of the table in include/mpunet_hip.h
struct TrainMetricsState {
    double total[TM_METRICS];
    double count[TM_METRICS];
    unsigned long long scratch[3 * VC_MAXK];      // tp | rel | sel of the step in flight, [3][K]; zero between steps
};

template <int K>
__global__ __launch_bounds__(VC_THREADS) void train_metrics_count_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ y,
                                                                         long n, TrainMetricsState* __restrict__ s) {
    class_counts_add<K>(pred, y, n, s->scratch);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one wave; lane c owns class c
__global__ __launch_bounds__(64) void train_metrics_finalize_kernel(TrainMetricsState* __restrict__ s, int K, double n) {
    const int c = threadIdx.x;
    unsigned long long tp = 0, rel = 0, sel = 0;
    if (c < K) {
        tp = s->scratch[c]; rel = s->scratch[K + c]; sel = s->scratch[2 * K + c];
        s->scratch[c] = 0ull; s->scratch[K + c] = 0ull; s->scratch[2 * K + c] = 0ull;
    }
    // tf.math.confusion_matrix without num_classes: 1 + the largest class among the labels and predictions of THIS batch
    const unsigned long long present = __ballot(rel + sel > 0ull);
    const int Kb = present ? 64 - __clzll((long long)present) : 1;
    const unsigned long long all_tp = wave_sum_u64(tp);
    const unsigned long long fg_tp = wave_sum_u64(c >= 1 ? tp : 0ull);
    const unsigned long long fg_rel = wave_sum_u64(c >= 1 ? rel : 0ull);
    const unsigned long long fg_sel = wave_sum_u64(c >= 1 ? sel : 0ull);
    // per class, 0 / 0 = NaN as in TF
    const double p = (double)tp / (double)sel, r = (double)tp / (double)rel;
    const double f = (2.0 * p * r) / (p + r);
    __shared__ double sh[3][VC_MAXK];
    if (c < VC_MAXK) { sh[0][c] = p; sh[1][c] = r; sh[2][c] = f; }
    __syncthreads();
    if (c == 0) {
        double sp = 0.0, sr = 0.0, sf = 0.0;
        for (int k = 1; k < Kb; ++k) { sp += sh[0][k]; sr += sh[1][k]; sf += sh[2][k]; }
        const double m = (double)(Kb - 1);          // Kb = 1: the mean of an empty set, 0 / 0
        const double v[TM_METRICS] = {(double)all_tp, (double)fg_tp / (double)fg_rel, (double)fg_tp / (double)fg_sel,
                                      sp / m, sr / m, sf / m};
#pragma unroll
        for (int i = 0; i < TM_METRICS; ++i) {
            s->total[i] += v[i];
            s->count[i] += i == 0 ? n : 1.0;
        }
    }
}

template <int K>
int launch_tm(const float* pred, const uint8_t* y, long n, TrainMetricsState* s, hipStream_t st) {
    train_metrics_count_kernel<K><<<dim3(class_counts_grid(n)), dim3(VC_THREADS), 0, st>>>(pred, y, n, s);
    train_metrics_finalize_kernel<<<dim3(1), dim3(64), 0, st>>>(s, K, (double)n);
    return launch_ok();
}

}  // namespace
}  // namespace mpu

using namespace mpu;

extern "C" int64_t mpu_train_metrics_state_bytes(void) { return (int64_t)sizeof(TrainMetricsState); }

extern "C" int mpu_train_metrics_update(const float* d_pred, const uint8_t* d_y, int64_t n, int32_t n_classes, void* d_state,
                                        void* stream) {
    MPU_REQUIRE(d_pred && d_y && d_state, "mpu_train_metrics_update: null argument");
    MPU_REQUIRE(((uintptr_t)d_state & 7) == 0, "mpu_train_metrics_update: d_state must be 8-byte aligned");
    MPU_REQUIRE(n >= 0 && n_classes >= 1 && n_classes <= VC_MAXK, "mpu_train_metrics_update: need 1 <= n_classes <= 16");
    if (n == 0) return MPU_OK;
    hipStream_t st = (hipStream_t)stream;
    TrainMetricsState* s = (TrainMetricsState*)d_state;
    switch (n_classes) {
#define TM_CASE(KK) case KK: return launch_tm<KK>(d_pred, d_y, (long)n, s, st);
        TM_CASE(1) TM_CASE(2) TM_CASE(3) TM_CASE(4) TM_CASE(5) TM_CASE(6) TM_CASE(7) TM_CASE(8)
        TM_CASE(9) TM_CASE(10) TM_CASE(11) TM_CASE(12) TM_CASE(13) TM_CASE(14) TM_CASE(15) TM_CASE(16)
#undef TM_CASE
    }
    return fail(MPU_EINVAL, "%s", "mpu_train_metrics_update: bad n_classes");
}
