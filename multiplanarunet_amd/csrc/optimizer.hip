// The optimizer and the packed MFMA operands of the U-Net: weight packing (fp32 master -> forward and data-gradient operand
// copies), the Keras optimizers (Adam / AMSGrad, Adamax, SGD, RMSprop, learning-rate decay) alone and fused with that packing, the
// l2 kernel regulariser. Every device unit is written once and takes pointers and shapes; the kernels below only decide which
// unit a workgroup runs, and which update rule is a compile-time parameter of theirs.
//
// Reference semantics: `fit.optimizer` resolved in tf.keras.optimizers (mpunet/train/utils.py:100-111), each in the form of
// its TF ResourceApply* kernel; kernel_regularizer=l2 (mpunet/models/unet.py:122-177,189).
#include "optimizer_units.h"

namespace mpu {

// ------------------------------------------------------------------------- //
// weight packing: fp32 master (Keras HWIO = [tap][ci][co]) -> MFMA operands
// ------------------------------------------------------------------------- //
// forward operand of one layer, unit t = one (tap, 64 ci, 64 co) tile: 16-byte reads along co, transpose through LDS
template <typename T>
__device__ __forceinline__ void pack_fwd_tile(const float* __restrict__ W, T* wf, int Cin, int Cout, int t, float (*tile)[65]) {
    const Tile64 c = tile64_of(t, Cin, Cout);
    const float* src = W + (long)c.tap * Cin * Cout;
    const int ty = threadIdx.x >> 4, tx4 = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cil = ty + 16 * k;
        bool in;
        float4 v = *reinterpret_cast<const float4*>(src + clamped_off(c.ci0 + cil, c.co0 + tx4, Cin, Cout, in));
        if (!in) v = make_float4(0.f, 0.f, 0.f, 0.f);
        tile_put(&tile[cil][tx4], v);
    }
    __syncthreads();
    tile_store_fwd<T, false>(tile, wf + (long)c.tap * Cin * Cout, Cin, Cout, c.ci0, c.co0);
}

// data-gradient operand [dtaps][ci][co] of one layer, unit = 2048 consecutive elements (8 per thread; Cin * Cout is a multiple
// of 64, so they never straddle taps). CONV3 (dtaps 9) and CONV1 (dtaps 1): the taps rotated by 180 degrees; UPCONV2: combined
template <typename T>
__device__ __forceinline__ void pack_dgrad_chunk(int mode, int dtaps, const float* __restrict__ W, T* wd, int Cin, int Cout, int chunk) {
    const long per_tap = (long)Cin * Cout;
    const long e = (long)chunk * 2048 + threadIdx.x * 8;
    if (e >= dtaps * per_tap) return;
    const int tp = (int)(e / per_tap); const long r = e % per_tap;
    float v[8];
    auto load8 = [&](int k, float (&o)[8]) {
        const float* p = W + (long)k * per_tap + r;
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    };
    if (mode == UPCONV2) upconv_combined_tap<8>(tp, v, load8);
    else load8(dtaps - 1 - tp, v);
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int h = 0; h < 8 / N; ++h) {
        float w[N];
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = v[h * N + i];
        Vec<T>::store(wd + e + h * N, w);
    }
}

// units of one layer in the two kernels below: forward tiles, then data-gradient chunks
static inline int pack_fwd_units(int mode, int Cin, int Cout) {
    return (mode == UPCONV2 ? 4 : (mode == CONV1 ? 1 : 9)) * cdiv(Cin, 64) * cdiv(Cout, 64);
}
static inline int pack_dgrad_units(int mode, int Cin, int Cout) { return cdiv((mode == CONV1 ? 1L : 9L) * Cin * Cout, 2048L); }

// all layers of a model in ONE launch; the job table travels in the kernel arguments (no device-side table to keep in sync)
template <typename T>
__global__ __launch_bounds__(256) void pack_all_kernel(PackTable tab, const float* __restrict__ params, T* packed) {
    __shared__ float tile[64][65];
    const PackJob& j = tab.job[find_unit(tab.job, tab.njobs, (int)blockIdx.x)];
    const int u = (int)blockIdx.x - j.unit_begin;
    if (u < j.fwd_units) pack_fwd_tile<T>(params + j.w, packed + j.wf, j.Cin, j.Cout, u, tile);
    else pack_dgrad_chunk<T>(j.mode, 9, params + j.w, packed + j.wd, j.Cin, j.Cout, u - j.fwd_units);
}

int launch_pack_all(int dtype, PackTable& tab, const float* params, void* packed, hipStream_t st) {
    int units = 0;
    for (int i = 0; i < tab.njobs; ++i) {
        PackJob& j = tab.job[i];
        j.unit_begin = units;
        j.fwd_units = pack_fwd_units(j.mode, j.Cin, j.Cout);
        units += j.fwd_units + pack_dgrad_units(j.mode, j.Cin, j.Cout);
    }
    if (units == 0) return MPU_OK;
    if (dtype == MPU_BF16) pack_all_kernel<bf16_t><<<units, 256, 0, st>>>(tab, params, (bf16_t*)packed);
    else pack_all_kernel<float><<<units, 256, 0, st>>>(tab, params, (float*)packed);
    return launch_ok();
}

// one layer (CONV3 / UPCONV2 / CONV1), the data-gradient operand optional: the same units, the three pointers as arguments
template <typename T>
__global__ __launch_bounds__(256) void pack_layer_kernel(int mode, const float* __restrict__ W, int Cin, int Cout, int fwd_units,
                                                         T* wf, T* wd) {
    __shared__ float tile[64][65];
    const int u = (int)blockIdx.x;
    if (u < fwd_units) pack_fwd_tile<T>(W, wf, Cin, Cout, u, tile);
    else pack_dgrad_chunk<T>(mode, mode == CONV1 ? 1 : 9, W, wd, Cin, Cout, u - fwd_units);
}

int launch_pack_weights(int dtype, int mode, const float* W, int Cin, int Cout, void* wf, void* wd, hipStream_t st) {
    const int fwd_units = pack_fwd_units(mode, Cin, Cout);
    const int units = fwd_units + (wd ? pack_dgrad_units(mode, Cin, Cout) : 0);
    if (dtype == MPU_BF16) pack_layer_kernel<bf16_t><<<units, 256, 0, st>>>(mode, W, Cin, Cout, fwd_units, (bf16_t*)wf, (bf16_t*)wd);
    else pack_layer_kernel<float><<<units, 256, 0, st>>>(mode, W, Cin, Cout, fwd_units, (float*)wf, (float*)wd);
    return launch_ok();
}

// dtype "bf16x3": packed f32 operands -> (bf16 hi | bf16 lo << 16) words, in place, after every refresh of the packed copies
// that did not write the words itself. n = 32-bit words.
__global__ __launch_bounds__(256) void x3_words_kernel(uint32_t* __restrict__ buf, long n) {
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 + 4 <= n) {
        uint4 v = *reinterpret_cast<uint4*>(buf + i4);
        v.x = x3_word(__uint_as_float(v.x)); v.y = x3_word(__uint_as_float(v.y));
        v.z = x3_word(__uint_as_float(v.z)); v.w = x3_word(__uint_as_float(v.w));
        *reinterpret_cast<uint4*>(buf + i4) = v;
    } else {
        for (long i = i4; i < n; ++i) buf[i] = x3_word(__uint_as_float(buf[i]));
    }
}
int launch_x3_words(void* buf, long n, hipStream_t st) {
    if (n <= 0) return MPU_OK;
    x3_words_kernel<<<(unsigned)((n + 1023) / 1024), 256, 0, st>>>((uint32_t*)buf, n);
    return launch_ok();
}

// ------------------------------------------------------------------------- //
// plain Adam, decay == 0 (every other configuration: optimizer_rules.hip)
// ------------------------------------------------------------------------- //
// Plain Adam's step size of step t (1-based), on the host and from a device-resident counter (graph replay: a captured launch
// cannot take a new host-computed step size on every replay). step_bias: 1 = the counter holds t - 1 (the caller increments it
// after the update), 0 = it already holds t
static inline float adam_alpha_host(long long t, double lr, double b1, double b2) {
    return (float)(lr * std::sqrt(1.0 - std::pow(b2, (double)t)) / (1.0 - std::pow(b1, (double)t)));
}
__device__ __forceinline__ float adam_alpha_dev(const long long* step, double lr, double b1d, double b2d, int step_bias) {
    const double t = (double)(*step + step_bias);
    return (float)(lr * sqrt(1.0 - pow(b2d, t)) / (1.0 - pow(b1d, t)));
}
// the flat buffers and the step's constants, as every unit takes them
__device__ __forceinline__ OptArgs adam_args(float* p, const float* g, float* m, float* v, const long long* step, double lr,
                                             double b1d, double b2d, float alpha_host, float eps, int step_bias) {
    return {p, g, {m, v, nullptr}, {step ? adam_alpha_dev(step, lr, b1d, b2d, step_bias) : alpha_host, (float)b1d, (float)b2d, eps}};
}
// plain Adam, decay == 0 (the default configuration; also the serial half of mpu_unet_backward_adam's tail)
template <typename T, bool X3 = false>
__global__ __launch_bounds__(256) void adam_pack_all_kernel(AdamPackTable tab, float* __restrict__ params,
                                                            const float* __restrict__ grads, float* __restrict__ am,
                                                            float* __restrict__ av, T* packed, const long long* __restrict__ step,
                                                            double lr, double b1d, double b2d, float alpha_host, float eps, int step_bias) {
    __shared__ float tile_raw[4 * 32 * 33];                      // >= 64 x 65: both tile views live here
    const OptArgs a = adam_args(params, grads, am, av, step, lr, b1d, b2d, alpha_host, eps, step_bias);
    const int ji = opt_pack_job_of<AdamRule>(tab, a, (int)blockIdx.x);
    if (ji < 0) return;
    const PackJob& j = tab.job[ji];
    const int t = (int)blockIdx.x - j.unit_begin;
    if (j.mode == UPCONV2) opt_pack_upconv_tile<AdamRule, T, X3, 32>(a, j.w, packed + j.wf, packed + j.wd, j.Cin, j.Cout, t, tile_raw);
    else opt_pack_conv3_tile<AdamRule, T, X3>(a, j.w, packed + j.wf, packed + j.wd, j.Cin, j.Cout, t, reinterpret_cast<float (*)[65]>(tile_raw));
}
// ---- round 6: the optimizer beside the weight gradients -----------------------------------------------------------
// adam_pack_lean_kernel (bf16 operands, plain Adam only: its budget was tuned for two slots): the same update and the same two packed copies as adam_pack_all_kernel, but small
// enough -- <= 64 registers, 8.5 KB of LDS -- to be CO-RESIDENT with a wgrad_taps workgroup (448 of a SIMD's 512 registers,
// 148 of a CU's 160 KB): the grouped weight-gradient launch is bound by MFMA issue and LDS reads, this kernel by HBM, so the
// optimizer of the parameters whose gradients are already final (the deep levels: 90 % of the bytes) runs on a second stream
// UNDER the weight gradients of the high-resolution levels instead of behind them (run_backward_adam, unet_model.hip).
//   CONV3 job  : unit = (tap, 64 ci, 64 co) tile as in adam_pack_all_kernel, loaded in two halves of 32 ci (8 instead of 16
//                16-byte loads per thread in flight), the tile held in LDS as bf16 -- the values both copies store.
//   UPCONV2 job: unit = (16 ci, 32 co) x the four taps, fp32 in LDS (the data-gradient copy sums taps in fp32 before rounding).
// Bit-identical to adam_pack_all_kernel (tests/test_gpu_unet.py).
constexpr int LEAN_TP = 68;                      // bf16 tile pitch (elements): rows 8-byte aligned
__device__ __forceinline__ void adam_pack_conv3_tile_lean(const OptArgs& a, long w, bf16_t* wf, bf16_t* wd, int Cin, int Cout, int t,
                                                          bf16_t (*tile)[LEAN_TP]) {
    const Tile64 c = tile64_of(t, Cin, Cout);
    const int ci0 = c.ci0, co0 = c.co0;
    const long per_tap = (long)Cin * Cout, base = w + c.tap * per_tap;
    const int ty = threadIdx.x >> 4, tx4 = (threadIdx.x & 15) * 4;
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        Opt4<AdamRule> x[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            bool in;
            const long o = base + clamped_off(ci0 + ty + 16 * (2 * half + k), co0 + tx4, Cin, Cout, in);
            x[k].load(a, o, in);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float4 q = x[k].finish(a);
            *reinterpret_cast<uint2*>(&tile[ty + 16 * (2 * half + k)][tx4]) = make_uint2(f32x2_to_bf16x2(q.x, q.y), f32x2_to_bf16x2(q.z, q.w));
        }
    }
    __syncthreads();
    bf16_t* dstf = wf + c.tap * per_tap;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {                       // forward copy [co][ci]: columns of the tile
        const int col = threadIdx.x / 8 + pass * 32, cil = (threadIdx.x % 8) * 8;
        const int co = co0 + col, ci = ci0 + cil;
        if (ci < Cin && co < Cout) {
            uint32_t wv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) wv[e] = (uint32_t)tile[cil + 2 * e][col] | ((uint32_t)tile[cil + 2 * e + 1][col] << 16);
            *reinterpret_cast<uint4*>(dstf + (long)co * Cin + ci) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        }
    }
    bf16_t* dstd = wd + (8 - c.tap) * per_tap;                   // data-gradient copy: rotated taps, rows of the tile
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int row = threadIdx.x / 8 + pass * 32, col = (threadIdx.x % 8) * 8;
        const int ci = ci0 + row, co = co0 + col;
        if (ci < Cin && co < Cout) {
            const uint2 p = *reinterpret_cast<const uint2*>(&tile[row][col]), q = *reinterpret_cast<const uint2*>(&tile[row][col + 4]);
            *reinterpret_cast<uint4*>(dstd + (long)ci * Cout + co) = make_uint4(p.x, p.y, q.x, q.y);
        }
    }
}

__global__ __launch_bounds__(256, 8) void adam_pack_lean_kernel(AdamPackTable tab, float* __restrict__ params,
                                                                const float* __restrict__ grads, float* __restrict__ am,
                                                                float* __restrict__ av, bf16_t* packed, const long long* __restrict__ step,
                                                                double lr, double b1d, double b2d, float alpha_host, float eps, int step_bias) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[64 * LEAN_TP * 2];          // 8704 B >= 4 x 16 x 33 floats (8448)
    const OptArgs a = adam_args(params, grads, am, av, step, lr, b1d, b2d, alpha_host, eps, step_bias);
    const int ji = opt_pack_job_of<AdamRule>(tab, a, (int)blockIdx.x);
    if (ji < 0) return;
    const PackJob& j = tab.job[ji];
    const int t = (int)blockIdx.x - j.unit_begin;
    if (j.mode == UPCONV2) opt_pack_upconv_tile<AdamRule, bf16_t, false, 16>(a, j.w, packed + j.wf, packed + j.wd, j.Cin, j.Cout, t, lds_raw);
    else adam_pack_conv3_tile_lean(a, j.w, packed + j.wf, packed + j.wd, j.Cin, j.Cout, t, reinterpret_cast<bf16_t (*)[LEAN_TP]>(lds_raw));
}

__global__ void incr_step_kernel(long long* step) { *step += 1; }
int launch_incr_step(long long* step, hipStream_t st) {
    incr_step_kernel<<<1, 1, 0, st>>>(step);
    return launch_ok();
}

// The unit table of one update-and-pack launch over the parameters in the nr ascending, disjoint ranges [p_lo[k], p_hi[k]).
// jobs: every 3x3 / 2x2 kernel of the model (mode, Cin, Cout, w, wf, wd set), ordered by offset; a job is taken when its kernel
// lies inside a range, which must not cut one; the rest of each range are plain units. lean: the up-conv unit of the lean kernel.
int opt_pack_table(const PackTable& jobs, const long* p_lo, const long* p_hi, int nr, bool lean, AdamPackTable& tab, int& units) {
    tab.njobs = 0; tab.nranges = 0; tab._pad = 0;
    units = 0;
    long prev_w = -1;
    int job_range[PACK_MAX_JOBS];
    auto end_of = [](const PackJob& j) { return j.w + (long)(j.mode == UPCONV2 ? 4 : 9) * j.Cin * j.Cout; };
    for (int i = 0; i < jobs.njobs; ++i) {
        PackJob j = jobs.job[i];
        if (j.w < prev_w) return fail(MPU_EINVAL, "%s", "adam_pack: jobs must be ordered by parameter offset");
        prev_w = j.w;
        int in = -1;
        for (int k = 0; k < nr; ++k) {
            if (end_of(j) <= p_lo[k] || j.w >= p_hi[k]) continue;
            if (j.w < p_lo[k] || end_of(j) > p_hi[k]) return fail(MPU_EINVAL, "%s", "adam_pack: a parameter range cuts a kernel");
            in = k;
        }
        if (in < 0) continue;
        j.unit_begin = units;
        j.fwd_units = j.mode == UPCONV2 ? cdiv(j.Cin, lean ? 16 : 32) * cdiv(j.Cout, 32) : 9 * cdiv(j.Cin, 64) * cdiv(j.Cout, 64);
        units += j.fwd_units;
        job_range[tab.njobs] = in;
        tab.job[tab.njobs++] = j;
    }
    tab.plain_begin = units;
    for (int k = 0; k < nr; ++k) {                               // the complement of the packed kernels inside each range
        if (k > 0 && p_lo[k] < p_hi[k - 1]) return fail(MPU_EINVAL, "%s", "adam_pack: ranges must ascend and not overlap");
        long cur = p_lo[k];
        for (int i = 0; i <= tab.njobs; ++i) {
            if (i < tab.njobs && job_range[i] != k) continue;
            const long lo = i < tab.njobs ? tab.job[i].w : p_hi[k];
            if (lo > cur) {
                if (tab.nranges >= ADAM_MAX_RANGES) return fail(MPU_EINVAL, "%s", "adam_pack: too many parameter ranges");
                AdamRange& r = tab.range[tab.nranges++];
                r.off = cur; r.n = lo - cur; r.unit_begin = units; r._pad = 0;
                units += cdiv(r.n, 1024L);
            }
            if (i < tab.njobs) cur = end_of(tab.job[i]);
        }
    }
    return MPU_OK;
}

// Plain Adam (decay == 0) + both packed operand copies of the parameters in the ranges, ONE launch. dtype MPU_F32X3: f32 storage,
// the operand words written here. lean: the co-resident kernel (bf16 only). step == NULL: t_host is the 1-based step number;
// else the device counter holds this step's number already (step_is_t: mpu_unet_backward_adam advances it at the start of the
// backward pass, so that no launch of the tail has to wait for "every reader is done" before it moves) or the number before
// it, and is advanced here, behind the update.
int launch_adam_pack(int dtype, const PackTable& jobs, float* params, const float* grads, float* am, float* av, const long* p_lo,
                     const long* p_hi, int nr, void* packed, long long* step, bool step_is_t, long long t_host, double lr, double b1,
                     double b2, float eps, bool lean, hipStream_t st) {
    AdamPackTable tab;
    const bool use_lean = lean && dtype == MPU_BF16;
    int units = 0;
    if (const int rc = opt_pack_table(jobs, p_lo, p_hi, nr, use_lean, tab, units)) return rc;
    if (units == 0) return MPU_OK;
    const float alpha_host = step ? 0.f : adam_alpha_host(t_host, lr, b1, b2);
    const int step_bias = step_is_t ? 0 : 1;
    if (use_lean) {
        // ONE workgroup per compute unit, whatever arrives first: the launch claims 82 KB of LDS (8.5 KB used), so two of
        // them never share a CU, and 82 + 74 KB (wgrad_taps) do. Without the cap the 7 k short workgroups of this kernel
        // fill every CU eight deep and the weight-gradient workgroups (448 of 512 registers) wait for them to drain: the
        // two launches then run one after the other (measured, round 6: 135 + 311 us instead of side by side).
        constexpr int LEAN_CLAIM = 82 * 1024, LEAN_STATIC = 64 * LEAN_TP * 2;
        static unsigned long long attr_set = 0;
        if (first_use_on_device(attr_set)) {
            MPU_CHECK_HIP(hipFuncSetAttribute((const void*)adam_pack_lean_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LEAN_CLAIM - LEAN_STATIC));
            mark_used_on_device(attr_set);
        }
        adam_pack_lean_kernel<<<units, 256, LEAN_CLAIM - LEAN_STATIC, st>>>(tab, params, grads, am, av, (bf16_t*)packed, step, lr, b1, b2, alpha_host, eps, step_bias);
    } else if (dtype == MPU_BF16)
        adam_pack_all_kernel<bf16_t><<<units, 256, 0, st>>>(tab, params, grads, am, av, (bf16_t*)packed, step, lr, b1, b2, alpha_host, eps, step_bias);
    else if (dtype == MPU_F32X3)
        adam_pack_all_kernel<float, true><<<units, 256, 0, st>>>(tab, params, grads, am, av, (float*)packed, step, lr, b1, b2, alpha_host, eps, step_bias);
    else
        adam_pack_all_kernel<float><<<units, 256, 0, st>>>(tab, params, grads, am, av, (float*)packed, step, lr, b1, b2, alpha_host, eps, step_bias);
    if (step && !step_is_t) incr_step_kernel<<<1, 1, 0, st>>>(step);
    return launch_ok();
}

// the element-wise step (the two-pass form: Adam, then launch_pack_all); step as in launch_adam_pack with step_is_t false
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                            const long long* __restrict__ step, double lr, double b1d, double b2d, float alpha_host, float eps) {
    const OptArgs a = adam_args(p, g, m, v, step, lr, b1d, b2d, alpha_host, eps, 1);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) opt_update_one<AdamRule>(a, e);
}
int launch_adam(float* p, const float* g, float* m, float* v, long n, long long* step, long long t_host, double lr, double b1,
                double b2, float eps, hipStream_t st) {
    adam_kernel<<<ew_grid(n), 256, 0, st>>>(p, g, m, v, n, step, lr, b1, b2, step ? 0.f : adam_alpha_host(t_host, lr, b1, b2), eps);
    if (step) incr_step_kernel<<<1, 1, 0, st>>>(step);
    return launch_ok();
}

// kernel_regularizer=l2(lambda) of the 3x3 / 2x2 conv kernels (reference unet.py:122-177,189): g += 2*lambda*W and,
// when wanted, lambda * sum W^2 (fixed summation order: L2_BLOCKS partial sums per kernel tensor, combined by one block)
constexpr int L2_BLOCKS = 64;
__global__ __launch_bounds__(256) void l2_grad_kernel(L2Table tab, const float* __restrict__ p, float* __restrict__ g,
                                                      float two_l2, double* __restrict__ partial) {
    const long off = tab.off[blockIdx.y], n = tab.n[blockIdx.y];
    double acc = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)L2_BLOCKS * 256) {
        const float w = p[off + e];
        g[off + e] = g[off + e] + two_l2 * w;
        acc += (double)w * (double)w;
    }
    if (!partial) return;
    __shared__ double red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(long)blockIdx.y * L2_BLOCKS + blockIdx.x] = red[0];
}
__global__ void l2_loss_kernel(const double* __restrict__ partial, int n, float l2, float* __restrict__ out) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += partial[i];
    *out = (float)(s * (double)l2);
}
int launch_l2_regularizer(const L2Table& tab, const float* params, float* grads, float l2, double* partial,
                          float* reg_loss, hipStream_t st) {
    if (tab.njobs == 0) return MPU_OK;
    l2_grad_kernel<<<dim3(L2_BLOCKS, tab.njobs), 256, 0, st>>>(tab, params, grads, 2.f * l2, reg_loss ? partial : nullptr);
    if (reg_loss) l2_loss_kernel<<<1, 1, 0, st>>>(partial, tab.njobs * L2_BLOCKS, l2, reg_loss);
    return launch_ok();
}

}  // namespace mpu
