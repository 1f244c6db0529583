// Device units of the optimizer and of the packed MFMA operands, each written once: the tile writers of the two operand copies,
// one update unit per rule of tf.keras.optimizers, the rule-templated load / finish pair over up to three slot buffers, and the
// units of the fused update-and-pack launch. optimizer.hip builds the packing kernels and plain Adam's kernels from them,
// optimizer_rules.hip every other configuration's (a translation unit of its own, so that the LDS layout of the module that holds
// plain Adam's kernels -- and with it their instruction sequence -- is what it was before the other rules existed).
#pragma once
#include <cmath>
#include "kernels.h"

namespace mpu {

// index of the entry (PackJob / AdamRange, ascending unit_begin) that workgroup u belongs to
template <typename E>
__device__ __forceinline__ int find_unit(const E* e, int n, int u) {
    int i = 0;
    while (i + 1 < n && u >= e[i + 1].unit_begin) ++i;
    return i;
}

// offset of the float4 at (ci, co) inside one [Cin][Cout] tap, clamped into it (Cout % 4 == 0): loads are unconditional and a
// select follows, so that all loads of a thread are in flight together
__device__ __forceinline__ long clamped_off(int ci, int co, int Cin, int Cout, bool& in) {
    in = ci < Cin && co < Cout;
    return (long)(ci < Cin ? ci : Cin - 1) * Cout + (co < Cout ? co : Cout - 4);
}

// unit t of a layer cut into (tap, 64 ci, 64 co) tiles
struct Tile64 { int tap, ci0, co0; };
__device__ __forceinline__ Tile64 tile64_of(int t, int Cin, int Cout) {
    const int tci = (Cin + 63) / 64, tco = (Cout + 63) / 64;
    const int tap = t / (tci * tco), r = t % (tci * tco);
    return {tap, (r / tco) * 64, (r % tco) * 64};
}

// dtype "bf16x3": the packed f32 operand words hold bf16 hi | bf16 lo << 16 (common.h: x3_word)
template <int N> __device__ __forceinline__ void x3_words_of(float (&v)[N]) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = __uint_as_float(x3_word(v[e]));
}

__device__ __forceinline__ void tile_put(float* row, const float4& v) { row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w; }

// 64 x 64 fp32 tile [ci][co] -> forward operand [co][ci] of its tap: the tile's columns, 16-byte stores along ci
template <typename T, bool X3>
__device__ __forceinline__ void tile_store_fwd(const float (*tile)[65], T* dst, int Cin, int Cout, int ci0, int co0) {
    constexpr int N = Vec<T>::N, GPR = 64 / N, RPP = 256 / GPR;   // 16-byte groups per row, rows per pass
#pragma unroll
    for (int pass = 0; pass < 64 / RPP; ++pass) {
        const int col = threadIdx.x / GPR + pass * RPP, cil = (threadIdx.x % GPR) * N;
        const int co = co0 + col, ci = ci0 + cil;
        if (ci < Cin && co < Cout) {                              // Cin % 8 == 0: the whole vector is in range
            float v[N];
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = tile[cil + e][col];
            if (X3) x3_words_of<N>(v);
            Vec<T>::store(dst + (long)co * Cin + ci, v);
        }
    }
}
// ... -> data-gradient operand [ci][co] of its (rotated) tap: the tile's rows
template <typename T, bool X3>
__device__ __forceinline__ void tile_store_dgrad(const float (*tile)[65], T* dst, int Cin, int Cout, int ci0, int co0) {
    constexpr int N = Vec<T>::N, GPR = 64 / N, RPP = 256 / GPR;
#pragma unroll
    for (int pass = 0; pass < 64 / RPP; ++pass) {
        const int row = threadIdx.x / GPR + pass * RPP, col = (threadIdx.x % GPR) * N;
        const int ci = ci0 + row, co = co0 + col;
        if (ci < Cin && co < Cout) {
            float v[N];
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = tile[row][col + e];
            if (X3) x3_words_of<N>(v);
            Vec<T>::store(dst + (long)ci * Cout + co, v);
        }
    }
}

// The up-conv's data gradient is a 3x3 stride-2 convolution whose tap tp = (dy+1)*3 + (dx+1) is the sum of the 2x2 taps
// S(dy) x S(dx), S(-1) = {1}, S(0) = {0, 1}, S(1) = {0}. load(k, u) fetches N elements of tap k. The summation order (ky outer,
// kx inner, from zero) is part of the results: every path that forms this operand goes through here.
template <int N, typename Load>
__device__ __forceinline__ void upconv_combined_tap(int tp, float (&v)[N], Load load) {
    const int dy = tp / 3 - 1, dx = tp % 3 - 1;
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = 0.f;
    for (int ky = 0; ky < 2; ++ky) {
        if ((dy == -1 && ky != 1) || (dy == 1 && ky != 0)) continue;
        for (int kx = 0; kx < 2; ++kx) {
            if ((dx == -1 && kx != 1) || (dx == 1 && kx != 0)) continue;
            float u[N];
            load(ky * 2 + kx, u);
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] += u[e];
        }
    }
}

// [4 taps][R ci][32 co] fp32 tile of an up-conv kernel -> forward copy [tap][co][ci] and data-gradient copy [tap'][ci][co]
template <typename T, bool X3, int R>
__device__ __forceinline__ void upconv_tile_store(const float (*tile)[R][33], T* wf, T* wd, int Cin, int Cout, int ci0, int co0) {
    constexpr int N = Vec<T>::N, GI = R / N, GO = 32 / N;        // 16-byte groups along ci / along co
    const long per_tap = (long)Cin * Cout;
    for (int idx = threadIdx.x; idx < 4 * 32 * GI; idx += 256) {
        const int tp = idx / (32 * GI), rem = idx % (32 * GI);
        const int col = rem / GI, cil = (rem % GI) * N;
        const int co = co0 + col, ci = ci0 + cil;
        if (ci < Cin && co < Cout) {
            float v[N];
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = tile[tp][cil + e][col];
            if (X3) x3_words_of<N>(v);
            Vec<T>::store(wf + tp * per_tap + (long)co * Cin + ci, v);
        }
    }
    for (int idx = threadIdx.x; idx < 9 * R * GO; idx += 256) {
        const int tp = idx / (R * GO), rem = idx % (R * GO);
        const int row = rem / GO, col = (rem % GO) * N;
        const int ci = ci0 + row, co = co0 + col;
        if (ci < Cin && co < Cout) {
            float v[N];
            upconv_combined_tap<N>(tp, v, [&](int k, float (&u)[N]) {
#pragma unroll
                for (int e = 0; e < N; ++e) u[e] = tile[k][row][col + e];
            });
            if (X3) x3_words_of<N>(v);
            Vec<T>::store(wd + tp * per_tap + (long)ci * Cout + co, v);
        }
    }
}

// ------------------------------------------------------------------------- //
// update rules (tf.keras.optimizers as of TF 2.3: the OptimizerV2 classes and the ResourceApply* kernels they call)
// ------------------------------------------------------------------------- //
// One device unit per rule. Arithmetic per element in f32, in the order written here, which is part of the results.
// No FMA contraction inside (pragma): the compiler contracted the multiply-adds in one kernel and not in the other, and
// the fused and the plain path differed by one ulp in 1.4 % of the first moments (HIP's __fadd_rn & co. are plain
// operators and contract just the same).

// TF ApplyAdam: m += (g-m)(1-b1); v += (g*g-v)(1-b2); p -= m*alpha/(sqrt(v)+eps)
// (one definition for the plain and the fused kernels: the same instruction sequence, bit-identical results)
__device__ __forceinline__ void adam_update(float gg, float& m, float& v, float& p, float alpha, float b1, float b2, float eps) {
#pragma clang fp contract(off)
    const float d1 = gg - m, o1 = 1.f - b1;
    const float mm = m + d1 * o1;
    const float g2 = gg * gg;
    const float d2 = g2 - v, o2 = 1.f - b2;
    const float vv = v + d2 * o2;
    m = mm; v = vv;
    const float num = mm * alpha, den = sqrtf(vv) + eps;
    p = p - num / den;
}
// TF ApplyAdamWithAmsgrad: m, v as above; vhat = max(vhat, v); p -= m*alpha/(sqrt(vhat)+eps)
__device__ __forceinline__ void amsgrad_update(float gg, float& m, float& v, float& vhat, float& p, float alpha, float b1, float b2,
                                               float eps) {
#pragma clang fp contract(off)
    const float d1 = gg - m, o1 = 1.f - b1;
    const float mm = m + d1 * o1;
    const float g2 = gg * gg;
    const float d2 = g2 - v, o2 = 1.f - b2;
    const float vv = v + d2 * o2;
    const float vh = fmaxf(vhat, vv);
    m = mm; v = vv; vhat = vh;
    const float num = mm * alpha, den = sqrtf(vh) + eps;
    p = p - num / den;
}
// TF ApplyAdaMax: m += (g-m)(1-b1); u = max(b2*u, |g|); p -= (c*m)/(u+eps), c = lr_t/(1-b1^t)
__device__ __forceinline__ void adamax_update(float gg, float& m, float& u, float& p, float c, float b1, float b2, float eps) {
#pragma clang fp contract(off)
    const float d1 = gg - m, o1 = 1.f - b1;
    const float mm = m + d1 * o1;
    const float uu = fmaxf(b2 * u, fabsf(gg));
    m = mm; u = uu;
    const float num = c * mm, den = uu + eps;
    p = p - num / den;
}
// Keras SGD: plain p -= lr_t*g; TF ApplyKerasMomentum: a = a*momentum - lr_t*g; p += a, Nesterov: p += a*momentum - lr_t*g
template <bool MOMENTUM, bool NESTEROV>
__device__ __forceinline__ void sgd_update(float gg, float& a, float& p, float lr, float momentum) {
#pragma clang fp contract(off)
    const float s = lr * gg;
    if (!MOMENTUM) { p = p - s; return; }
    const float aa = a * momentum - s;
    a = aa;
    p = NESTEROV ? p + (aa * momentum - s) : p + aa;
}
// Keras RMSprop: ms += (g*g-ms)(1-rho); centered: mg += (g-mg)(1-rho), d = ms - mg*mg, else d = ms.
// Without momentum (the Python dense path): p -= lr_t*g/(sqrt(d)+eps) -- epsilon OUTSIDE the root; with momentum (TF
// ApplyRMSProp / ApplyCenteredRMSProp): mom = mom*momentum + lr_t*g/sqrt(d+eps); p -= mom -- epsilon INSIDE the root.
template <bool MOMENTUM, bool CENTERED>
__device__ __forceinline__ void rmsprop_update(float gg, float& ms, float& mom, float& mg, float& p, float lr, float rho,
                                               float momentum, float eps) {
#pragma clang fp contract(off)
    const float o = 1.f - rho;
    const float g2 = gg * gg;
    const float d2 = g2 - ms;
    const float s = ms + d2 * o;
    ms = s;
    float d = s;
    if (CENTERED) {
        const float d1 = gg - mg;
        const float c = mg + d1 * o;
        mg = c;
        d = s - c * c;
    }
    const float num = lr * gg;
    if (!MOMENTUM) { p = p - num / (sqrtf(d) + eps); return; }
    const float mm = mom * momentum + num / sqrtf(d + eps);
    mom = mm;
    p = p - mm;
}

// A rule at compile time: the kind (mpu_optimizer_kind) and its variant -- MPU_OPT_NESTEROV / _AMSGRAD / _CENTERED and
// OPT_MOMENTUM (momentum > 0) -- fix the slot buffers it has, NS of them in the order below, and its unit. There is no
// per-element branch on any of them.
//   Adam: m, v[, vhat]    Adamax: m, u    SGD: [a]    RMSprop: ms[, mom][, mg]
// Constants: c[0] is the one that may depend on the step (c0 below), c[1..3] are fixed:
//   Adam / Adamax: b1, b2, eps    SGD: momentum    RMSprop: rho, momentum, eps
constexpr int OPT_MOMENTUM = 8;      // internal: the bit above mpu_optimizer_flag's (1, 2, 4), never accepted in mpu_optimizer_config.flags
struct OptArgs { float* p; const float* g; float* s[3]; float c[4]; };
template <int KIND, int FLAGS> struct Rule {
    static constexpr bool MOM = (FLAGS & OPT_MOMENTUM) != 0, NEST = (FLAGS & MPU_OPT_NESTEROV) != 0;
    static constexpr bool AMS = (FLAGS & MPU_OPT_AMSGRAD) != 0, CEN = (FLAGS & MPU_OPT_CENTERED) != 0;
    static constexpr int NS = KIND == MPU_OPT_ADAM ? (AMS ? 3 : 2) : KIND == MPU_OPT_ADAMAX ? 2 : KIND == MPU_OPT_SGD ? (MOM ? 1 : 0)
                                                                                                : 1 + (MOM ? 1 : 0) + (CEN ? 1 : 0);
    static constexpr bool STEP_DEP = KIND == MPU_OPT_ADAM || KIND == MPU_OPT_ADAMAX;     // c0 moves with t even when decay == 0
    // the step's own constant in f64, from the decayed rate lr_t and t (1-based): Adam's alpha_t, Adamax' lr_t/(1-b1^t), else lr_t
    static __device__ __forceinline__ double c0(double lr_t, double b1, double b2, double t) {
        if (KIND == MPU_OPT_ADAM) return lr_t * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t));
        if (KIND == MPU_OPT_ADAMAX) return lr_t / (1.0 - pow(b1, t));
        return lr_t;
    }
    static __device__ __forceinline__ void update(float g, float& s0, float& s1, float& s2, float& p, const OptArgs& a) {
        if (KIND == MPU_OPT_ADAM) {
            if (AMS) amsgrad_update(g, s0, s1, s2, p, a.c[0], a.c[1], a.c[2], a.c[3]);
            else adam_update(g, s0, s1, p, a.c[0], a.c[1], a.c[2], a.c[3]);
        } else if (KIND == MPU_OPT_ADAMAX) adamax_update(g, s0, s1, p, a.c[0], a.c[1], a.c[2], a.c[3]);
        else if (KIND == MPU_OPT_SGD) sgd_update<MOM, NEST>(g, s0, p, a.c[0], a.c[1]);
        else if (MOM) rmsprop_update<true, CEN>(g, s0, s1, s2, p, a.c[0], a.c[1], a.c[2], a.c[3]);
        else rmsprop_update<false, CEN>(g, s0, s2, s1, p, a.c[0], a.c[1], a.c[2], a.c[3]);      // (mg is the second slot)
    }
};
using AdamRule = Rule<MPU_OPT_ADAM, 0>;

// One float4 of g, the rule's slots and p at a clamped offset. load() only issues the loads -- how many of these a thread holds
// in flight is its caller's schedule; finish() updates, stores the slots and p when the float4 is in range (a clamped duplicate
// would be updated twice) and hands the new p on (zeros outside). A slot the rule does not have is neither loaded nor stored.
template <typename R> struct Opt4 {
    float4 g, s[3], p; long off; bool in;
    __device__ __forceinline__ void load(const OptArgs& a, long o, bool inside) {
        off = o; in = inside;
        g = *reinterpret_cast<const float4*>(a.g + o);
#pragma unroll
        for (int i = 0; i < R::NS; ++i) s[i] = *reinterpret_cast<const float4*>(a.s[i] + o);
        p = *reinterpret_cast<const float4*>(a.p + o);
    }
    __device__ __forceinline__ float4 finish(const OptArgs& a) {
        R::update(g.x, s[0].x, s[1].x, s[2].x, p.x, a); R::update(g.y, s[0].y, s[1].y, s[2].y, p.y, a);
        R::update(g.z, s[0].z, s[1].z, s[2].z, p.z, a); R::update(g.w, s[0].w, s[1].w, s[2].w, p.w, a);
        if (in) {
#pragma unroll
            for (int i = 0; i < R::NS; ++i) *reinterpret_cast<float4*>(a.s[i] + off) = s[i];
            *reinterpret_cast<float4*>(a.p + off) = p;
        }
        return in ? p : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};
// one element, as the scalar tails and the element-wise kernel take it
template <typename R> __device__ __forceinline__ void opt_update_one(const OptArgs& a, long e) {
    float s0 = R::NS > 0 ? a.s[0][e] : 0.f, s1 = R::NS > 1 ? a.s[1][e] : 0.f, s2 = R::NS > 2 ? a.s[2][e] : 0.f, pp = a.p[e];
    R::update(a.g[e], s0, s1, s2, pp, a);
    if (R::NS > 0) a.s[0][e] = s0;
    if (R::NS > 1) a.s[1][e] = s1;
    if (R::NS > 2) a.s[2][e] = s2;
    a.p[e] = pp;
}

// plain unit: 1024 floats of [off, off + n) -- everything that is not a 3x3 / 2x2 kernel (biases, BatchNorm gamma / beta, the
// 1x1 head): the update only, float4 body, scalar tail and unaligned ranges
template <typename R> __device__ __forceinline__ void opt_plain_unit(const OptArgs& a, long off, long n, int unit) {
    const long e = (long)unit * 1024 + threadIdx.x * 4;
    if (e >= n) return;
    const long o = off + e;
    if (e + 4 <= n && (o & 3) == 0) {
        Opt4<R> x;
        x.load(a, o, true);
        x.finish(a);
    } else {
        for (int i = 0; i < 4 && e + i < n; ++i) opt_update_one<R>(a, o + i);
    }
}

// ---- update + weight packing in ONE pass (round 3) -------------------------------------------------------------
// The separate chain read the gradients and wrote the parameters (adam_kernel), then read the parameters twice more
// to write the two bf16 operand copies (pack_all_kernel). Here a unit loads g, the slots and p of one kernel tile, updates
// them, and writes the slots, p AND both packed copies from the tile: 0.25 GB less traffic per step and one launch less.
//   CONV3 job  : unit = (tap, 64 ci, 64 co) tile; forward copy [tap][co][ci] transposed through LDS, data-gradient
//                copy [8 - tap][ci][co] from the same tile (16-byte stores).
//   UPCONV2 job: unit = (32 ci, 32 co) x the four taps (the data-gradient copy is the 3x3 stride-2 combination,
//                which needs all four updated taps of an element).
//   plain units: opt_plain_unit, ranges in the table.
// dtype "bf16x3" (X3): the operand words are written by the optimizer pass itself.
struct AdamRange { long off, n; int unit_begin, _pad; };
constexpr int ADAM_MAX_RANGES = 48;
struct AdamPackTable { int njobs, nranges, plain_begin, _pad; PackJob job[PACK_MAX_JOBS]; AdamRange range[ADAM_MAX_RANGES]; };

// the job that workgroup u runs a unit of; a plain unit is run here (-1)
template <typename R>
__device__ __forceinline__ int opt_pack_job_of(const AdamPackTable& tab, const OptArgs& a, int u) {
    if (u < tab.plain_begin) return find_unit(tab.job, tab.njobs, u);
    const AdamRange& r = tab.range[find_unit(tab.range, tab.nranges, u)];
    opt_plain_unit<R>(a, r.off, r.n, u - r.unit_begin);
    return -1;
}

template <typename R, typename T, bool X3>
__device__ __forceinline__ void opt_pack_conv3_tile(const OptArgs& a, long w, T* wf, T* wd, int Cin, int Cout, int t,
                                                     float (*tile)[65]) {
    const Tile64 c = tile64_of(t, Cin, Cout);
    const long per_tap = (long)Cin * Cout, base = w + c.tap * per_tap;
    const int ty = threadIdx.x >> 4, tx4 = (threadIdx.x & 15) * 4;
    Opt4<R> x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                // all 16 loads of the thread in flight together
        bool in;
        const long o = base + clamped_off(c.ci0 + ty + 16 * k, c.co0 + tx4, Cin, Cout, in);
        x[k].load(a, o, in);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tile_put(&tile[ty + 16 * k][tx4], x[k].finish(a));
    __syncthreads();
    tile_store_fwd<T, X3>(tile, wf + c.tap * per_tap, Cin, Cout, c.ci0, c.co0);
    tile_store_dgrad<T, X3>(tile, wd + (8 - c.tap) * per_tap, Cin, Cout, c.ci0, c.co0);   // 180-degree rotated taps
}

// unit = (R ci, 32 co) x the four taps; a thread holds R / 8 taps of one float4
template <typename R, typename T, bool X3, int ROWS>
__device__ __forceinline__ void opt_pack_upconv_tile(const OptArgs& a, long w, T* wf, T* wd, int Cin, int Cout, int t, void* lds) {
    constexpr int TPT = ROWS / 8;
    float (*tile)[ROWS][33] = reinterpret_cast<float (*)[ROWS][33]>(lds);
    const int tco = (Cout + 31) / 32;
    const int ci0 = (t / tco) * ROWS, co0 = (t % tco) * 32;
    const long per_tap = (long)Cin * Cout;
    {
        const int tp0 = (threadIdx.x / (ROWS * 8)) * TPT, cil = (threadIdx.x % (ROWS * 8)) >> 3, tx4 = (threadIdx.x & 7) * 4;
        bool in;
        const long o0 = w + clamped_off(ci0 + cil, co0 + tx4, Cin, Cout, in);
        Opt4<R> x[TPT];
#pragma unroll
        for (int k = 0; k < TPT; ++k) x[k].load(a, o0 + (tp0 + k) * per_tap, in);
#pragma unroll
        for (int k = 0; k < TPT; ++k) tile_put(&tile[tp0 + k][cil][tx4], x[k].finish(a));
    }
    __syncthreads();
    upconv_tile_store<T, X3, ROWS>(tile, wf, wd, Cin, Cout, ci0, co0);
}

// advance a device-resident step counter by one, behind whatever was enqueued on st before (optimizer.hip)
int launch_incr_step(long long* step, hipStream_t st);
// The unit table of one update-and-pack launch over the parameters in the nr ascending, disjoint ranges [p_lo[k], p_hi[k])
// (optimizer.hip). jobs: every 3x3 / 2x2 kernel of the model (mode, Cin, Cout, w, wf, wd set), ordered by offset; a job is taken
// when its kernel lies inside a range, which must not cut one; the rest of each range are plain units. lean: the up-conv unit of
// the lean kernel.
int opt_pack_table(const PackTable& jobs, const long* p_lo, const long* p_hi, int nr, bool lean, AdamPackTable& tab, int& units);

}  // namespace mpu
