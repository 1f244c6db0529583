// Every optimizer configuration but plain Adam with decay 0 (mpu_optimizer_config: SGD, RMSprop, Adamax, AMSGrad, learning-rate
// decay): the element-wise kernel and the fused update-and-pack kernel, built from the units of optimizer_units.h with the rule
// and its flags as compile-time parameters of the instantiation. Serial tail only: backward pass, then ONE launch of these.
//
// Reference semantics: `fit.optimizer` / `fit.optimizer_kwargs` resolved in tf.keras.optimizers (mpunet/train/utils.py:100-111).
#include "optimizer_units.h"

namespace mpu {

// The step's constants of every rule, learning-rate decay included (OptimizerV2._decayed_lr: lr_t = lr / (1 + decay * (t - 1)); decay == 0: lr
// itself, no division). c0 is ALWAYS formed on the device, from the counter (which holds t - 1) or from t_host, so that an eager
// step and a replayed one take the same constant bit for bit; a rule whose c0 is lr itself reads no counter.
struct OptConsts { const long long* step; long long t_host; double lr, decay, b1, b2; float c1, c2, c3; int _pad; };
template <typename R>
__device__ __forceinline__ OptArgs opt_args(float* p, const float* g, float* s0, float* s1, float* s2, const OptConsts& k) {
    float c0 = (float)k.lr;
    if (R::STEP_DEP || k.decay != 0.0) {
        const double t = (double)(k.step ? *k.step + 1 : k.t_host);
        const double lr_t = k.decay != 0.0 ? k.lr / (1.0 + k.decay * (t - 1.0)) : k.lr;
        c0 = (float)R::c0(lr_t, k.b1, k.b2, t);
    }
    return {p, g, {s0, s1, s2}, {c0, k.c1, k.c2, k.c3}};
}

// every other configuration (a rule with its flags; Adam with decay): the same units, the rule a compile-time parameter
template <typename R, typename T, bool X3>
__global__ __launch_bounds__(256) void opt_pack_all_kernel(AdamPackTable tab, float* __restrict__ params, const float* __restrict__ grads,
                                                           float* __restrict__ s0, float* __restrict__ s1, float* __restrict__ s2,
                                                           T* packed, OptConsts k) {
    __shared__ float tile_raw[4 * 32 * 33];                      // >= 64 x 65: both tile views live here
    const OptArgs a = opt_args<R>(params, grads, s0, s1, s2, k);
    const int ji = opt_pack_job_of<R>(tab, a, (int)blockIdx.x);
    if (ji < 0) return;
    const PackJob& j = tab.job[ji];
    const int t = (int)blockIdx.x - j.unit_begin;
    if (j.mode == UPCONV2) opt_pack_upconv_tile<R, T, X3, 32>(a, j.w, packed + j.wf, packed + j.wd, j.Cin, j.Cout, t, tile_raw);
    else opt_pack_conv3_tile<R, T, X3>(a, j.w, packed + j.wf, packed + j.wd, j.Cin, j.Cout, t, reinterpret_cast<float (*)[65]>(tile_raw));
}

// ---- every configuration (mpu_optimizer_config) ----------------------------------------------------------------------
// 0..3 slot buffers of a valid configuration, else MPU_EINVAL with the reason (what the Keras constructors refuse, and flags
// that belong to another kind)
int optimizer_num_slots(const mpu_optimizer_config& c) {
    const bool mom = c.momentum > 0.0;
    const int allowed = c.kind == MPU_OPT_SGD ? MPU_OPT_NESTEROV : c.kind == MPU_OPT_ADAM ? MPU_OPT_AMSGRAD
                      : c.kind == MPU_OPT_RMSPROP ? MPU_OPT_CENTERED : 0;
    if (c.kind < MPU_OPT_ADAM || c.kind > MPU_OPT_ADAMAX) return fail(MPU_EINVAL, "%s: unknown kind %ld", "mpu_optimizer_config", (long)c.kind);
    if (c.flags & ~allowed) return fail(MPU_EINVAL, "%s: flags %ld do not belong to kind %ld", "mpu_optimizer_config", (long)c.flags, (long)c.kind);
    if (!(c.lr >= 0.0) || !(c.decay >= 0.0) || !(c.epsilon >= 0.0)) return fail(MPU_EINVAL, "%s", "mpu_optimizer_config: lr, decay and epsilon must not be negative");
    if (c.kind == MPU_OPT_SGD || c.kind == MPU_OPT_RMSPROP) {
        if (!(c.momentum >= 0.0 && c.momentum <= 1.0)) return fail(MPU_EINVAL, "%s", "mpu_optimizer_config: momentum must be between [0, 1]");
        if (c.kind == MPU_OPT_RMSPROP && !(c.rho >= 0.0 && c.rho <= 1.0)) return fail(MPU_EINVAL, "%s", "mpu_optimizer_config: rho must be in [0, 1]");
        return c.kind == MPU_OPT_SGD ? (mom ? 1 : 0) : 1 + (mom ? 1 : 0) + ((c.flags & MPU_OPT_CENTERED) ? 1 : 0);
    }
    if (!(c.beta1 >= 0.0 && c.beta1 < 1.0) || !(c.beta2 >= 0.0 && c.beta2 < 1.0)) return fail(MPU_EINVAL, "%s", "mpu_optimizer_config: beta1 and beta2 must be in [0, 1)");
    return c.kind == MPU_OPT_ADAM && (c.flags & MPU_OPT_AMSGRAD) ? 3 : 2;
}
// f(Rule<...>{}) for the rule of a valid configuration
template <typename F> static int with_rule(const mpu_optimizer_config& c, F&& f) {
    const bool mom = c.momentum > 0.0, cen = (c.flags & MPU_OPT_CENTERED) != 0;
    switch (c.kind) {
    case MPU_OPT_ADAM: return (c.flags & MPU_OPT_AMSGRAD) ? f(Rule<MPU_OPT_ADAM, MPU_OPT_AMSGRAD>{}) : f(AdamRule{});
    case MPU_OPT_ADAMAX: return f(Rule<MPU_OPT_ADAMAX, 0>{});
    case MPU_OPT_SGD:
        if (!mom) return f(Rule<MPU_OPT_SGD, 0>{});              // (Nesterov without momentum is the plain rule, as in Keras)
        return (c.flags & MPU_OPT_NESTEROV) ? f(Rule<MPU_OPT_SGD, OPT_MOMENTUM | MPU_OPT_NESTEROV>{}) : f(Rule<MPU_OPT_SGD, OPT_MOMENTUM>{});
    default:
        if (mom) return cen ? f(Rule<MPU_OPT_RMSPROP, OPT_MOMENTUM | MPU_OPT_CENTERED>{}) : f(Rule<MPU_OPT_RMSPROP, OPT_MOMENTUM>{});
        return cen ? f(Rule<MPU_OPT_RMSPROP, MPU_OPT_CENTERED>{}) : f(Rule<MPU_OPT_RMSPROP, 0>{});
    }
}
// scalar constants: f64 on the host, rounded to f32 once
static OptConsts opt_consts(const mpu_optimizer_config& c, const long long* step, long long t_host) {
    OptConsts k{step, t_host, c.lr, c.decay, c.beta1, c.beta2, 0.f, 0.f, 0.f, 0};
    if (c.kind == MPU_OPT_SGD) k.c1 = (float)c.momentum;
    else if (c.kind == MPU_OPT_RMSPROP) { k.c1 = (float)c.rho; k.c2 = (float)c.momentum; k.c3 = (float)c.epsilon; }
    else { k.c1 = (float)c.beta1; k.c2 = (float)c.beta2; k.c3 = (float)c.epsilon; }
    return k;
}

template <typename R>
__global__ void opt_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                           float* __restrict__ s2, long n, OptConsts k) {
    const OptArgs a = opt_args<R>(p, g, s0, s1, s2, k);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) opt_update_one<R>(a, e);
}
// element-wise step of any rule on a flat buffer; step != NULL: the device counter holds t - 1 and is incremented afterwards
int launch_optimizer(const mpu_optimizer_config& c, float* p, const float* g, float* const s[3], long n, long long* step,
                     long long t_host, hipStream_t st) {
    const OptConsts k = opt_consts(c, step, t_host);
    if (n > 0)
        with_rule(c, [&](auto r) {
            opt_kernel<decltype(r)><<<ew_grid(n), 256, 0, st>>>(p, g, s[0], s[1], s[2], n, k);
            return MPU_OK;
        });
    return step ? launch_incr_step(step, st) : launch_ok();
}
// ... and fused with both packed operand copies of every kernel in `jobs`, over the whole buffer [0, n_params): ONE launch
int launch_optimizer_pack(int dtype, const PackTable& jobs, const mpu_optimizer_config& c, float* params, const float* grads,
                          float* const s[3], long n_params, void* packed, long long* step, long long t_host, hipStream_t st) {
    AdamPackTable tab;
    int units = 0;
    const long lo = 0;
    if (const int rc = opt_pack_table(jobs, &lo, &n_params, 1, false, tab, units)) return rc;
    const OptConsts k = opt_consts(c, step, t_host);
    if (units > 0)
        with_rule(c, [&](auto r) {
            using R = decltype(r);
            if (dtype == MPU_BF16) opt_pack_all_kernel<R, bf16_t, false><<<units, 256, 0, st>>>(tab, params, grads, s[0], s[1], s[2], (bf16_t*)packed, k);
            else if (dtype == MPU_F32X3) opt_pack_all_kernel<R, float, true><<<units, 256, 0, st>>>(tab, params, grads, s[0], s[1], s[2], (float*)packed, k);
            else opt_pack_all_kernel<R, float, false><<<units, 256, 0, st>>>(tab, params, grads, s[0], s[1], s[2], (float*)packed, k);
            return MPU_OK;
        });
    return step ? launch_incr_step(step, st) : launch_ok();
}

}  // namespace mpu
