// Argmax of the class scores fused with the per-class TP / relevant / selected counts: the device unit shared by the
// epoch-end validation (validation.hip) and the training metrics (train_metrics.hip). HBM-bound (4K + 1 bytes per pixel read
// once, nothing written but 3K integers); integer work, so the result does not depend on the order of the adds: per-thread
// register counters -> wave shuffle reduction -> LDS -> one 64-bit atomic per counter and workgroup.
#pragma once
#include "common.h"

namespace mpu {

constexpr int VC_MAXK = 16;
constexpr int VC_THREADS = 256;

// Whole body of a counting kernel of VC_THREADS threads per workgroup: ADDS tp | rel | sel of the pixels this grid's
// grid-stride loop gives the workgroup to counts[3][K]. A target >= K counts for no class (nothing is indexed by it).
template <int K>
__device__ __forceinline__ void class_counts_add(const float* __restrict__ pred, const uint8_t* __restrict__ y, long n,
                                                 unsigned long long* __restrict__ counts) {
    unsigned tp[K], rel[K], sel[K];
#pragma unroll
    for (int c = 0; c < K; ++c) { tp[c] = 0; rel[c] = 0; sel[c] = 0; }
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float* p = pred + i * K;
        float v[K];
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = p[c];
        // np.argmax / tf.argmax: first maximum; a NaN counts as the maximum (first NaN wins)
        int best = 0; float bv = v[0];
#pragma unroll
        for (int c = 1; c < K; ++c) {
            const bool take = (v[c] > bv) || (v[c] != v[c] && bv == bv);
            bv = take ? v[c] : bv; best = take ? c : best;
        }
        const int t = y[i];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            rel[c] += (t == c); sel[c] += (best == c); tp[c] += (t == c && best == c);
        }
    }
    __shared__ unsigned long long sh[3 * K];
    if (threadIdx.x < 3 * K) sh[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < K; ++c) {
        unsigned a = tp[c], b = rel[c], d = sel[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); d += __shfl_down(d, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&sh[c], (unsigned long long)a);
            atomicAdd(&sh[K + c], (unsigned long long)b);
            atomicAdd(&sh[2 * K + c], (unsigned long long)d);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * K && sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]);
}

// per-thread 32-bit counters: a thread sees at most n / (grid * VC_THREADS) + 1 pixels
inline unsigned class_counts_grid(long n) {
    long blocks = (n + VC_THREADS - 1) / VC_THREADS;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

}  // namespace mpu
