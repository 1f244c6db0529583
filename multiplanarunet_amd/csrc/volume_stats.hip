// Statistics of a resident volume, f32 [n_vox, C] interleaved: what fitting a sklearn scaler per channel and the '<N>pct'
// background value need (reference: mpunet/preprocessing/scaling.py:47-73, mpunet/image/image_pair.py:300-341,469-484, which run
// np.percentile / sklearn fits over the whole image on the host). Compiled with -ffp-contract=off.
//
//   mpu_volume_order_stats   exact order statistics of one channel by a three-pass radix select over a monotone u32 key
//                            (12 + 10 + 10 bits). Every pass is a histogram: per-workgroup LDS bins with LDS integer atomics,
//                            one global integer add per non-empty bin. Integer adds commute, so the counts -- and the values
//                            selected from them -- are the same bits on every run. Between the passes a one-workgroup kernel
//                            turns (rank) into (bin prefix, rank inside the bin); passes 2 and 3 count only the elements under
//                            one of the <= 16 selected prefixes, one 1024-bin LDS histogram per distinct prefix (16 x 4 KiB =
//                            the 64 KiB a workgroup gets without a launch attribute; two workgroups per CU).
//                            Traffic: three reads of the volume (all channels: the rows are interleaved), nothing written but
//                            ~130 KiB of counters.
//   mpu_volume_moments       count / min / max / max|x| / sum, or sum(x - mean) and sum((x - mean)^2), per channel in fp64:
//                            per-thread accumulators, an LDS tree per workgroup, one partial row per workgroup, and a
//                            one-workgroup second stage that adds the rows in index order. The grid is a function of the
//                            element count alone, so the summation order -- and the result -- is fixed.
//
// Both read the rows with 16-byte loads and pick the channel's elements in registers: the flat float index f belongs to
// channel f % C, tracked incrementally (no division in the loop).
#include "common.h"
#include <vector>

namespace mpu {
namespace {

constexpr int VS_THREADS = 512;
constexpr int VS_MAX_GRID = 2048;
constexpr int VS_MAX_RANKS = 16;
constexpr int VS_BINS1 = 4096, VS_BINS = 1024;              // 12 + 10 + 10 key bits
constexpr unsigned VS_NONE = 0xFFFFFFFFu;                     // no bin / no prefix (keys under a prefix have <= 22 bits)

// workspace, in 32-bit words
constexpr long VS_HIST1 = 0;
constexpr long VS_HIST2 = VS_HIST1 + VS_BINS1;
constexpr long VS_HIST3 = VS_HIST2 + (long)VS_MAX_RANKS * VS_BINS;
constexpr long VS_STATE = VS_HIST3 + (long)VS_MAX_RANKS * VS_BINS;
struct SelState {
    unsigned prefix[VS_MAX_RANKS];     // distinct selected prefixes (VS_NONE: unused)
    unsigned slot[VS_MAX_RANKS];       // per rank: index into prefix[] (VS_NONE: rank out of range)
    unsigned resid[VS_MAX_RANKS];      // per rank: rank among the elements under its prefix
    unsigned nan_count;
    unsigned _pad;
    float value[VS_MAX_RANKS];
};
constexpr long VS_WORDS = VS_STATE + (long)(sizeof(SelState) / 4);
// moments: partial rows of 8 doubles per workgroup and channel, behind the select's words
constexpr int VS_MOM = 8;

struct Ranks { long long r[VS_MAX_RANKS]; int n; };

// f32 bits -> key with the order of the values: -0.0 folded onto +0.0, negatives reversed
__device__ __forceinline__ unsigned key_of(unsigned u) {
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned bits_of_key(unsigned k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }
__device__ __forceinline__ bool is_nan_bits(unsigned u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

// f(bits, mine) for every float of this thread's share of vol[0 .. N); `mine`: the float belongs to channel ch.
// vol is 16-byte aligned (checked on the host); the <= 3 floats behind the last whole vector go to workgroup 0.
template <typename F>
__device__ __forceinline__ void for_each_value(const float* __restrict__ vol, long N, int C, int ch, F&& f) {
    const long nvec = N >> 2;
    const long stride = (long)gridDim.x * VS_THREADS;
    long v = (long)blockIdx.x * VS_THREADS + threadIdx.x;
    int m = (int)((4 * v) % C);                                // channel of the vector's first float
    const int dm = (int)((4 * stride) % C);
    const uint4* __restrict__ p = (const uint4*)vol;
    auto one = [&](const uint4& q, int m0) {
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        int mk = m0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f(w[k], mk == ch);
            mk = (mk + 1 == C) ? 0 : mk + 1;
        }
    };
    auto step = [&](int mm) { mm += dm; return mm >= C ? mm - C : mm; };
    for (; v + 3 * stride < nvec; v += 4 * stride) {            // four loads in flight per thread
        const uint4 q0 = p[v], q1 = p[v + stride], q2 = p[v + 2 * stride], q3 = p[v + 3 * stride];
        const int m1 = step(m), m2 = step(m1), m3 = step(m2);
        one(q0, m); one(q1, m1); one(q2, m2); one(q3, m3);
        m = step(m3);
    }
    for (; v < nvec; v += stride) { one(p[v], m); m = step(m); }
    if (blockIdx.x == 0 && (long)threadIdx.x < (N & 3)) {
        const long i = (nvec << 2) + threadIdx.x;
        f(__float_as_uint(vol[i]), (int)(i % C) == ch);
    }
}

// ++h[idx] for every active lane with idx != VS_NONE. The lanes that share the first active lane's bin (a constant region
// of the volume: the common case) are counted with one add instead of serialising on one LDS address.
__device__ __forceinline__ void hist_add(unsigned* h, unsigned idx) {
    const unsigned first = __builtin_amdgcn_readfirstlane(idx);
    const unsigned long long same = __ballot(idx == first);
    if (idx == first) {
        if (first != VS_NONE && (int)__lane_id() == __ffsll((long long)same) - 1) atomicAdd(&h[first], (unsigned)__popcll(same));
    } else if (idx != VS_NONE) {
        atomicAdd(&h[idx], 1u);
    }
}

// PASS 1: bins = key >> 20 of every non-NaN element, NaNs counted. PASS 2 / 3: bins = the next 10 bits of the elements whose
// higher bits are one of the selected prefixes.
template <int PASS>
__global__ __launch_bounds__(VS_THREADS) void select_hist_kernel(const float* __restrict__ vol, long N, int C, int ch,
                                                                 unsigned* __restrict__ ws) {
    constexpr int NB = PASS == 1 ? VS_BINS1 : VS_MAX_RANKS * VS_BINS;
    constexpr int PSHIFT = PASS == 2 ? 20 : 10, BSHIFT = PASS == 2 ? 10 : 0;
    __shared__ unsigned h[NB];
    SelState* st = (SelState*)(ws + VS_STATE);
    unsigned pf[VS_MAX_RANKS];
#pragma unroll
    for (int s = 0; s < VS_MAX_RANKS; ++s) pf[s] = PASS == 1 ? VS_NONE : st->prefix[s];
    for (int i = threadIdx.x; i < NB; i += VS_THREADS) h[i] = 0u;
    __syncthreads();
    unsigned nans = 0;
    for_each_value(vol, N, C, ch, [&](unsigned u, bool mine) {
        unsigned idx = VS_NONE;
        if (mine) {
            if (is_nan_bits(u)) {
                ++nans;
            } else {
                const unsigned k = key_of(u);
                if (PASS == 1) {
                    idx = k >> 20;
                } else {
                    const unsigned top = k >> PSHIFT;
#pragma unroll
                    for (int s = 0; s < VS_MAX_RANKS; ++s)
                        if (top == pf[s]) idx = (unsigned)s * VS_BINS + ((k >> BSHIFT) & (VS_BINS - 1));
                }
            }
        }
        hist_add(h, idx);
    });
    __syncthreads();
    unsigned* g = ws + (PASS == 1 ? VS_HIST1 : PASS == 2 ? VS_HIST2 : VS_HIST3);
    for (int i = threadIdx.x; i < NB; i += VS_THREADS) {
        const unsigned c = h[i];
        if (c) atomicAdd(&g[i], c);
    }
    if (PASS == 1) {
        for (int o = 32; o > 0; o >>= 1) nans += __shfl_xor(nans, o, 64);
        if ((threadIdx.x & 63) == 0 && nans) atomicAdd(&st->nan_count, nans);
    }
}

// One workgroup of 16 waves, wave w = rank w: the bin of hist[0 .. nbins) that holds rank r, and r's rank inside that bin.
__device__ __forceinline__ bool wave_select(const unsigned* __restrict__ hist, int nbins, unsigned r, unsigned& bin, unsigned& resid) {
    const int lane = (int)__lane_id(), per = nbins / 64;
    unsigned s = 0;
    for (int i = 0; i < per; ++i) s += hist[lane * per + i];
    unsigned incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const unsigned excl = incl - s;
    const bool mine = r >= excl && r < incl;                   // at most one lane
    const unsigned long long who = __ballot(mine);
    if (!who) return false;                                    // r >= number of elements
    unsigned b = 0, rr = 0;
    if (mine) {
        unsigned c = excl;
        for (int i = 0; i < per; ++i) {
            const unsigned n = hist[lane * per + i];
            if (r < c + n) { b = (unsigned)(lane * per + i); rr = r - c; break; }
            c += n;
        }
    }
    const int src = __ffsll((long long)who) - 1;
    bin = __shfl(b, src, 64); resid = __shfl(rr, src, 64);
    return true;
}

template <int PASS>
__global__ __launch_bounds__(1024) void select_scan_kernel(Ranks ranks, long n_vox, unsigned* __restrict__ ws) {
    __shared__ unsigned new_prefix[VS_MAX_RANKS], new_resid[VS_MAX_RANKS];
    SelState* st = (SelState*)(ws + VS_STATE);
    const int w = threadIdx.x >> 6;
    if (w < VS_MAX_RANKS) {                                    // (always: 1024 threads)
        unsigned np = VS_NONE, nr = 0;
        if (w < ranks.n) {
            unsigned bin = 0, resid = 0;
            if (PASS == 1) {
                const long long r = ranks.r[w];
                const long long total = (long long)n_vox - (long long)st->nan_count;
                if (r >= 0 && r < total && wave_select(ws + VS_HIST1, VS_BINS1, (unsigned)r, bin, resid)) { np = bin; nr = resid; }
            } else {
                const unsigned slot = st->slot[w];
                if (slot != VS_NONE) {
                    const unsigned* hist = ws + (PASS == 2 ? VS_HIST2 : VS_HIST3) + (long)slot * VS_BINS;
                    if (wave_select(hist, VS_BINS, st->resid[w], bin, resid)) { np = (st->prefix[slot] << 10) | bin; nr = resid; }
                }
            }
        }
        if ((threadIdx.x & 63) == 0) { new_prefix[w] = np; new_resid[w] = nr; }
    }
    __syncthreads();                                           // every read of the old state is behind us
    if (threadIdx.x == 0) {
        if (PASS == 3) {
            for (int i = 0; i < VS_MAX_RANKS; ++i)          // (a full key is never VS_NONE: that is a NaN's)
                st->value[i] = __uint_as_float(new_prefix[i] == VS_NONE ? 0x7FC00000u : bits_of_key(new_prefix[i]));
        } else {
            unsigned np_count = 0;
            for (int s = 0; s < VS_MAX_RANKS; ++s) st->prefix[s] = VS_NONE;
            for (int i = 0; i < VS_MAX_RANKS; ++i) {
                unsigned slot = VS_NONE;
                if (new_prefix[i] != VS_NONE) {
                    for (unsigned s = 0; s < np_count; ++s)
                        if (st->prefix[s] == new_prefix[i]) slot = s;
                    if (slot == VS_NONE) { slot = np_count; st->prefix[np_count++] = new_prefix[i]; }
                }
                st->slot[i] = slot; st->resid[i] = new_resid[i];
            }
        }
    }
}

// ---- moments ---------------------------------------------------------------------------------------------------------------
// SECOND == false: row = {count, min, max, max|x|, sum}; SECOND == true: row = {sum(x - mean), sum((x - mean)^2)}
template <bool SECOND>
__global__ __launch_bounds__(VS_THREADS) void moments_partial_kernel(const float* __restrict__ vol, long N, int C,
                                                                     const double* __restrict__ mean, double* __restrict__ partial) {
    __shared__ double red[VS_THREADS];
    const int ch = blockIdx.y;
    const double mu = SECOND ? mean[ch] : 0.0;
    double cnt = 0.0, mn = __longlong_as_double(0x7FF0000000000000LL), mx = -mn, ma = 0.0, s0 = 0.0, s1 = 0.0;
    for_each_value(vol, N, C, ch, [&](unsigned u, bool mine) {
        if (!mine || is_nan_bits(u)) return;
        const double x = (double)__uint_as_float(u);
        if (SECOND) {
            const double d = x - mu;
            s0 = s0 + d;
            s1 = s1 + d * d;
        } else {
            cnt += 1.0;
            mn = x < mn ? x : mn; mx = x > mx ? x : mx;
            const double ax = fabs(x); ma = ax > ma ? ax : ma;
            s0 = s0 + x;
        }
    });
    // fixed-order tree per statistic; op 0 = add, 1 = min, 2 = max
    auto tree = [&](double v, int op) -> double {
        red[threadIdx.x] = v;
        __syncthreads();
        for (int o = VS_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                const double a = red[threadIdx.x], b = red[threadIdx.x + o];
                red[threadIdx.x] = op == 0 ? a + b : op == 1 ? (b < a ? b : a) : (b > a ? b : a);
            }
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    double* row = partial + ((long)ch * gridDim.x + blockIdx.x) * VS_MOM;
    if (SECOND) {
        const double a = tree(s0, 0), b = tree(s1, 0);
        if (threadIdx.x == 0) { row[0] = a; row[1] = b; }
    } else {
        const double a = tree(cnt, 0), b = tree(mn, 1), c = tree(mx, 2), d = tree(ma, 2), e = tree(s0, 0);
        if (threadIdx.x == 0) { row[0] = a; row[1] = b; row[2] = c; row[3] = d; row[4] = e; }
    }
}

// second stage: one workgroup per channel adds the rows in index order (thread t: rows t, t + 256, ...; then a fixed tree)
template <bool SECOND>
__global__ __launch_bounds__(256) void moments_final_kernel(const double* __restrict__ partial, int nrows, double* __restrict__ out) {
    __shared__ double red[256];
    const int ch = blockIdx.x;
    const double* rows = partial + (long)ch * nrows * VS_MOM;
    constexpr int NS = SECOND ? 2 : 5;
    const double inf = __longlong_as_double(0x7FF0000000000000LL);
    for (int k = 0; k < NS; ++k) {
        const int op = SECOND ? 0 : (k == 1 ? 1 : (k == 2 || k == 3) ? 2 : 0);
        double v = op == 1 ? inf : op == 2 ? (k == 2 ? -inf : 0.0) : 0.0;
        for (int r = threadIdx.x; r < nrows; r += 256) {
            const double b = rows[(long)r * VS_MOM + k];
            v = op == 0 ? v + b : op == 1 ? (b < v ? b : v) : (b > v ? b : v);
        }
        red[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                const double a = red[threadIdx.x], b = red[threadIdx.x + o];
                red[threadIdx.x] = op == 0 ? a + b : op == 1 ? (b < a ? b : a) : (b > a ? b : a);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) out[(long)ch * VS_MOM + (SECOND ? 5 + k : k)] = red[0];
        __syncthreads();
    }
}

int stats_grid(long N) {                                        // a function of the element count alone (fixed summation order)
    const long b = ((N >> 2) + VS_THREADS - 1) / VS_THREADS;
    return (int)(b < 1 ? 1 : (b > VS_MAX_GRID ? VS_MAX_GRID : b));
}
long moments_bytes(int C) { return ((long)C * VS_MAX_GRID * VS_MOM + (long)C * VS_MOM + C) * (long)sizeof(double); }

}  // namespace
}  // namespace mpu

using namespace mpu;

extern "C" {

int64_t mpu_volume_stats_workspace_bytes(int32_t n_channels) {
    if (n_channels < 1) return 0;
    const long sel = VS_WORDS * 4L;
    return (sel + 15) / 16 * 16 + moments_bytes(n_channels);
}

int mpu_volume_order_stats(const float* d_vol, int64_t n_vox, int32_t n_channels, int32_t channel,
                           const int64_t* ranks, int32_t n_ranks, void* d_workspace, int64_t workspace_bytes,
                           float* values, int64_t* nan_count, void* stream) {
    MPU_REQUIRE(d_vol && ranks && d_workspace && values && nan_count, "mpu_volume_order_stats: null argument");
    MPU_REQUIRE(n_vox >= 1 && n_vox < (1LL << 31) && n_channels >= 1 && channel >= 0 && channel < n_channels,
                "mpu_volume_order_stats: need 1 <= n_vox < 2^31 and 0 <= channel < n_channels");
    MPU_REQUIRE(n_ranks >= 1 && n_ranks <= VS_MAX_RANKS, "mpu_volume_order_stats: 1 to 16 ranks");
    MPU_REQUIRE(((uintptr_t)d_vol & 15) == 0 && ((uintptr_t)d_workspace & 15) == 0,
                "mpu_volume_order_stats: volume and workspace must be 16-byte aligned");
    MPU_REQUIRE(workspace_bytes >= mpu_volume_stats_workspace_bytes(n_channels), "mpu_volume_order_stats: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    unsigned* ws = (unsigned*)d_workspace;
    Ranks rk;
    rk.n = n_ranks;
    for (int i = 0; i < VS_MAX_RANKS; ++i) rk.r[i] = i < n_ranks ? (long long)ranks[i] : -1;
    const long N = (long)n_vox * n_channels;
    const dim3 g((unsigned)stats_grid(N)), b(VS_THREADS);
    MPU_CHECK_HIP(hipMemsetAsync(ws, 0, VS_WORDS * 4L, st));
    select_hist_kernel<1><<<g, b, 0, st>>>(d_vol, N, n_channels, channel, ws);
    select_scan_kernel<1><<<dim3(1), dim3(1024), 0, st>>>(rk, (long)n_vox, ws);
    select_hist_kernel<2><<<g, b, 0, st>>>(d_vol, N, n_channels, channel, ws);
    select_scan_kernel<2><<<dim3(1), dim3(1024), 0, st>>>(rk, (long)n_vox, ws);
    select_hist_kernel<3><<<g, b, 0, st>>>(d_vol, N, n_channels, channel, ws);
    select_scan_kernel<3><<<dim3(1), dim3(1024), 0, st>>>(rk, (long)n_vox, ws);
    { const int rc_ = launch_ok(); if (rc_) return rc_; }
    SelState host;
    MPU_CHECK_HIP(hipMemcpyAsync(&host, ws + VS_STATE, sizeof(SelState), hipMemcpyDeviceToHost, st));
    MPU_CHECK_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n_ranks; ++i) values[i] = host.value[i];
    *nan_count = (int64_t)host.nan_count;
    return MPU_OK;
}

int mpu_volume_moments(const float* d_vol, int64_t n_vox, int32_t n_channels, const double* mean,
                       void* d_workspace, int64_t workspace_bytes, double* out, void* stream) {
    MPU_REQUIRE(d_vol && d_workspace && out, "mpu_volume_moments: null argument");
    MPU_REQUIRE(n_vox >= 1 && n_vox < (1LL << 31) && n_channels >= 1 && n_channels <= 65535,
                "mpu_volume_moments: need 1 <= n_vox < 2^31 and 1 <= n_channels < 65536");
    MPU_REQUIRE(((uintptr_t)d_vol & 15) == 0 && ((uintptr_t)d_workspace & 15) == 0,
                "mpu_volume_moments: volume and workspace must be 16-byte aligned");
    MPU_REQUIRE(workspace_bytes >= mpu_volume_stats_workspace_bytes(n_channels), "mpu_volume_moments: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int C = n_channels;
    double* partial = (double*)((char*)d_workspace + (VS_WORDS * 4L + 15) / 16 * 16);
    double* d_out = partial + (long)C * VS_MAX_GRID * VS_MOM;
    double* d_mean = d_out + (long)C * VS_MOM;
    const long N = (long)n_vox * C;
    const int nrows = stats_grid(N);
    const dim3 g((unsigned)nrows, (unsigned)C), b(VS_THREADS);
    if (mean) {
        MPU_CHECK_HIP(hipMemcpyAsync(d_mean, mean, sizeof(double) * C, hipMemcpyHostToDevice, st));
        moments_partial_kernel<true><<<g, b, 0, st>>>(d_vol, N, C, d_mean, partial);
        moments_final_kernel<true><<<dim3((unsigned)C), dim3(256), 0, st>>>(partial, nrows, d_out);
    } else {
        moments_partial_kernel<false><<<g, b, 0, st>>>(d_vol, N, C, nullptr, partial);
        moments_final_kernel<false><<<dim3((unsigned)C), dim3(256), 0, st>>>(partial, nrows, d_out);
    }
    { const int rc_ = launch_ok(); if (rc_) return rc_; }
    // (the rows of the pass not run are left as the caller gave them)
    const int k0 = mean ? 5 : 0, nk = mean ? 2 : 5;
    std::vector<double> host((size_t)C * VS_MOM);
    MPU_CHECK_HIP(hipMemcpyAsync(host.data(), d_out, sizeof(double) * host.size(), hipMemcpyDeviceToHost, st));
    MPU_CHECK_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < C; ++c)
        for (int k = k0; k < k0 + nk; ++k) out[(long)c * VS_MOM + k] = host[(size_t)c * VS_MOM + k];
    return MPU_OK;
}

}  // extern "C"
