// Exact Euclidean distance transform of a resident u8 label volume with anisotropic spacing, and the surface-distance table of
// `mp predict --surface_metrics` (HD, HD95, ASSD, NSD per class; no reference counterpart: the reference evaluates Dice only).
// Built with -ffp-contract=off: every f64 operation below is ONE rounded IEEE operation.
//
//   labels [X][Y][Z] u8 (C order). A FEATURE predicate selects the target voxels:
//     MPU_EDT_EQUAL      label == v
//     MPU_EDT_NOT_EQUAL  label != v
//     MPU_EDT_BORDER     label == v and at least one of the six face neighbours is != v; a neighbour outside the volume counts as
//                        != v  (M & ~binary_erosion(M, generate_binary_structure(3, 1)), border_value = 0: medpy's surface)
//   d2(p) = min over feature voxels q of fl( fl(wx dx^2) + fl( fl(wy dy^2) + fl(wz dz^2) ) ),  w_a = fl(spacing_a * spacing_a),
//   dx^2 .. the integer squares rounded to f64 (exact below 2^53). +inf everywhere when there is no feature voxel.
//
// Three passes, each the TRUE minimum of its line, so the result is the all-pairs minimum bit for bit (fl(a + .) is monotone: the
// minimum commutes with the rounded additions):
//   Z   one wave per line. Two sweeps over 64-voxel chunks: a ballot of the predicate gives every lane the nearest feature at or
//       before it (forward sweep, carried from chunk to chunk) and at or after it (backward sweep). The forward distance is parked in
//       the output word the same lane rewrites in the backward sweep with fl(wz dz^2). Any line length; O(1) per voxel.
//   Y,X one thread per voxel, threads along Z (every load of a wave is one contiguous run). The thread scans its line outwards
//       from its own position, k = 1, 2, ..., keeps the running minimum of fl(fl(w k^2) + g[pos -+ k]) and stops as soon as
//       fl(w k^2) alone is >= the minimum (g >= 0, so no farther candidate can win). No staging: any line length, worst case O(len).
//       The scan starts at the nearest position that can hold a finite value at all (the start tables below): a line with none is
//       +inf without a load.
//
// The table: per class c, bP / bT = border voxels of pred == c / truth == c; D_T = d2 to bT, D_P = d2 to bP. The directed lists
// D_T[bP] and D_P[bT] are gathered (counts, maximum, count <= tau^2: exact integers / bit patterns; sums of sqrt: fixed-order
// two-stage f64 sums) and compacted into one key list (non-negative doubles order like their bit patterns); the two order
// statistics NumPy's linear percentile needs are found by an exact 8 x 8-bit radix select on that list. The root and the
// interpolation of the percentile are the host's (NumPy's own arithmetic).
//
// Opening / closing by a Euclidean ball (`mp predict --open_mm / --close_mm`, mpu_morph_ball) are two thresholds of the same three
// passes; their kernels and the one change they need in a pass (a scan cut off at the radius) stand with mpu_morph_ball's kernels.
#include "common.h"
#include <math.h>

namespace mpu {
namespace {

constexpr int SD_THREADS = 256;
constexpr int SD_MAX_BLOCKS = 4096;                  // grid-stride beyond
constexpr int SD_PART_BLOCKS = 1024;                 // blocks of a gather launch = partial sums per direction (fixed by n alone)
constexpr int SD_MAXK = 16;
constexpr int SD_COLS = 8;                           // table columns (include/mpunet_hip.h)
constexpr long SD_HEADER_BYTES = 8192;

struct SdHeader {
    unsigned long long n_border[2], n_within, max_bits, list_n, rank[2], prefix[2], pad[7];
    unsigned long long hist[2][256];
};
static_assert(sizeof(SdHeader) <= SD_HEADER_BYTES, "header");

struct SdDims { int X, Y, Z, n; };

template <int MODE>
__device__ __forceinline__ bool is_feature(const uint8_t* __restrict__ L, const SdDims& d, int x, int y, int z, long i, int v) {
    const bool eq = (int)L[i] == v;
    if (MODE == MPU_EDT_EQUAL) return eq;
    if (MODE == MPU_EDT_NOT_EQUAL) return !eq;
    if (!eq) return false;
    const long sY = d.Z, sX = (long)d.Y * d.Z;
    if (z == 0 || z == d.Z - 1 || y == 0 || y == d.Y - 1 || x == 0 || x == d.X - 1) return true;
    return (int)L[i - 1] != v || (int)L[i + 1] != v || (int)L[i - sY] != v || (int)L[i + sY] != v || (int)L[i - sX] != v ||
           (int)L[i + sX] != v;
}

// Z pass: out[x][y][z] = fl(wz dz^2) to the nearest feature of the line, +inf when the line has none
template <int MODE>
__global__ __launch_bounds__(SD_THREADS) void edt_z_kernel(const uint8_t* __restrict__ labels, SdDims d, int v, double wz, double* out,
                                                           uint8_t* __restrict__ line_flag) {
    const int lane = (int)(threadIdx.x & 63u);
    const long wave = ((long)blockIdx.x * SD_THREADS + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * SD_THREADS) >> 6;
    const long nlines = (long)d.X * d.Y, Z = d.Z;
    const double inf = __builtin_huge_val();
    for (long line = wave; line < nlines; line += nwaves) {                    // (uniform per wave: the ballots see all 64 lanes)
        const int x = (int)(line / d.Y), y = (int)(line - (long)x * d.Y);
        const long base = line * Z;
        long last = -1;
        for (long z0 = 0; z0 < Z; z0 += 64) {
            const long z = z0 + lane;
            const bool f = z < Z && is_feature<MODE>(labels, d, x, y, (int)z, base + z, v);
            const unsigned long long m = __ballot(f);
            const unsigned long long below = m & (~0ull >> (63 - lane));       // features at chunk positions 0 .. lane
            const long p = below ? z0 + 63 - __clzll((long long)below) : last;
            if (z < Z) out[base + z] = p < 0 ? inf : (double)(z - p);
            if (m) last = z0 + 63 - __clzll((long long)m);
        }
        if (lane == 0) line_flag[line] = last >= 0 ? 1 : 0;
        long next = -1;
        for (long z0 = (Z - 1) / 64 * 64; z0 >= 0; z0 -= 64) {
            const long z = z0 + lane;
            const bool f = z < Z && is_feature<MODE>(labels, d, x, y, (int)z, base + z, v);
            const unsigned long long m = __ballot(f);
            const unsigned long long above = m >> lane;                        // features at chunk positions lane .. 63
            const long q = above ? z + (__ffsll((long long)above) - 1) : next;
            if (z < Z) {
                const double dp = out[base + z];                               // this lane's own word of the forward sweep
                const double dq = q < 0 ? inf : (double)(q - z);
                const double dd = dq < dp ? dq : dp;
                out[base + z] = wz * (dd * dd);
            }
            if (m) next = z0 + (__ffsll((long long)m) - 1);
        }
    }
}

// Where a scan may start. A Z line without a feature is +inf in all its voxels, so a Y line (x, ., z) holds finite values exactly
// at the y whose Z line (x, y) has a feature -- the same y for every z --, and an X line exactly at the planes x that have any.
// start_y[x][y] = distance in y to the nearest flagged Z line of plane x (-1: the plane has none); start_x[x] = distance to the
// nearest plane that has one (-1: the volume has no feature). Candidates nearer than that are +inf and are skipped unread.
__global__ __launch_bounds__(SD_THREADS) void edt_start_y_kernel(const uint8_t* __restrict__ line_flag, int X, int Y, int* __restrict__ start_y) {
    const long nlines = (long)X * Y, step = (long)gridDim.x * SD_THREADS;
    for (long l = (long)blockIdx.x * SD_THREADS + threadIdx.x; l < nlines; l += step) {
        const int y = (int)(l % Y);
        const int kmax = y > Y - 1 - y ? y : Y - 1 - y;
        int r = -1;
        for (int k = 0; k <= kmax; ++k)
            if ((k <= y && line_flag[l - k]) || (k <= Y - 1 - y && line_flag[l + k])) { r = k; break; }
        start_y[l] = r;
    }
}
__global__ __launch_bounds__(SD_THREADS) void edt_start_x_kernel(const int* __restrict__ start_y, int X, int Y, int* __restrict__ start_x) {
    const int step = (int)gridDim.x * SD_THREADS;
    for (int x = (int)blockIdx.x * SD_THREADS + (int)threadIdx.x; x < X; x += step) {
        const int kmax = x > X - 1 - x ? x : X - 1 - x;
        int r = -1;
        for (int k = 0; k <= kmax; ++k)
            if ((k <= x && start_y[(long)(x - k) * Y] >= 0) || (k <= X - 1 - x && start_y[(long)(x + k) * Y] >= 0)) { r = k; break; }
        start_x[x] = r;
    }
}

// Y / X pass over lines of `len` elements `stride` apart: out[i] = min over k of fl(fl(w k^2) + in[i + k stride]); start[i / stride]
// is the line's table entry above. ROOT: the last pass of a caller who wants distances stores sqrt of it.
// CUT (mpu_morph_ball, which only asks whether the result is <= cut): the scan also stops once fl(w k^2) > cut. Every candidate
// it skips is >= fl(w k^2) > cut (g >= 0, fl monotone), so a result <= cut is still the exact minimum and any other result is
// still > cut -- also through the next pass, where a value > cut can only make candidates > cut.
template <bool ROOT, bool CUT>
__global__ __launch_bounds__(SD_THREADS) void edt_line_kernel(const double* __restrict__ in, double* __restrict__ out, long n, long stride,
                                                              int len, double w, const int* __restrict__ start, double cut) {
    const long step = (long)gridDim.x * SD_THREADS;
    for (long i = (long)blockIdx.x * SD_THREADS + threadIdx.x; i < n; i += step) {
        const long line = i / stride;
        const int k0 = start[line];
        if (k0 < 0) { out[i] = __builtin_huge_val(); continue; }                // nothing finite in this line
        const int pos = (int)(line % len);
        const int nlo = pos, nhi = len - 1 - pos;                               // candidates below / above
        const int kmax = nlo > nhi ? nlo : nhi;
        double best = in[i];
        for (int k = k0 > 1 ? k0 : 1; k <= kmax; ++k) {
            const double dk = (double)k;
            const double a = w * (dk * dk);
            if (!(a < best)) break;
            if (CUT && a > cut) break;
            if (k <= nlo) { const double c = a + in[i - (long)k * stride]; best = c < best ? c : best; }
            if (k <= nhi) { const double c = a + in[i + (long)k * stride]; best = c < best ? c : best; }
        }
        out[i] = ROOT ? sqrt(best) : best;
    }
}

__global__ void sd_zero_table_kernel(unsigned long long* table, int words) {
    for (int t = threadIdx.x; t < words; t += blockDim.x) table[t] = 0ull;
}

__global__ void sd_begin_kernel(SdHeader* hdr) {
    unsigned long long* w = (unsigned long long*)hdr;
    for (int t = threadIdx.x; t < (int)(sizeof(SdHeader) / 8); t += blockDim.x) w[t] = 0ull;
}

// One direction: the voxels of the border of labels == c read D. DIR 0: labels = pred (D = d2 to the truth's border), 1: the reverse.
// gridDim.x is a function of n alone and every block stores its partial sum: the sum order is fixed.
__global__ __launch_bounds__(SD_THREADS) void sd_gather_kernel(const uint8_t* __restrict__ labels, SdDims d, int c,
                                                               const double* __restrict__ D, double tau2, int dir, SdHeader* hdr,
                                                               unsigned long long* __restrict__ list, double* __restrict__ partial) {
    __shared__ double s_sum[SD_THREADS];
    __shared__ unsigned long long s_cnt, s_within, s_max;
    if (threadIdx.x == 0) { s_cnt = 0ull; s_within = 0ull; s_max = 0ull; }
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63u);
    const long step = (long)gridDim.x * SD_THREADS;
    const long sYZ = (long)d.Y * d.Z;
    double sum = 0.0;
    unsigned long long cnt = 0ull, within = 0ull, mx = 0ull;
    for (long b = (long)blockIdx.x * SD_THREADS; b < d.n; b += step) {          // (uniform per workgroup)
        const long i = b + threadIdx.x;
        bool f = false;
        if (i < d.n && (int)labels[i] == c) {
            const int x = (int)(i / sYZ);
            const long r = i - (long)x * sYZ;
            const int y = (int)(r / d.Z), z = (int)(r - (long)y * d.Z);
            f = is_feature<MPU_EDT_BORDER>(labels, d, x, y, z, i, c);
        }
        const unsigned long long m = __ballot(f);
        if (m == 0ull) continue;
        unsigned long long base = 0ull;
        if (lane == 0) base = atomicAdd(&hdr->list_n, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        if (f) {
            const double v = D[i];
            const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
            list[base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = bits;
            sum += sqrt(v);
            ++cnt;
            within += v <= tau2 ? 1ull : 0ull;
            mx = bits > mx ? bits : mx;
        }
    }
    s_sum[threadIdx.x] = sum;
    if (cnt) { atomicAdd(&s_cnt, cnt); atomicAdd(&s_within, within); atomicMax(&s_max, mx); }
    __syncthreads();
    for (int h = SD_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_sum[threadIdx.x] = s_sum[threadIdx.x] + s_sum[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s_sum[0];
        if (s_cnt) {
            atomicAdd(&hdr->n_border[dir], s_cnt);
            atomicAdd(&hdr->n_within, s_within);
            atomicMax(&hdr->max_bits, s_max);
        }
    }
}

// NumPy's linear percentile at q = 95 / 100: virtual index vi = fl((n - 1) q); the neighbours floor(vi) and floor(vi) + 1, both the
// last element when vi >= n - 1.
__device__ __forceinline__ void percentile_ranks(unsigned long long n, unsigned long long& lo, unsigned long long& hi) {
    const double vi = (double)(n - 1ull) * 0.95;
    if (vi >= (double)(n - 1ull)) { lo = hi = n - 1ull; return; }
    lo = (unsigned long long)floor(vi);
    hi = lo + 1ull;
}

// the sums in fixed order, the counts and the ranks of the two order statistics -> table row / header. One workgroup.
__global__ __launch_bounds__(SD_THREADS) void sd_plan_kernel(SdHeader* hdr, const double* __restrict__ partial, int nblocks,
                                                             unsigned long long* __restrict__ row) {
    __shared__ double s_sum[2][SD_THREADS];
    for (int dir = 0; dir < 2; ++dir) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += SD_THREADS) s = s + partial[dir * SD_PART_BLOCKS + b];
        s_sum[dir][threadIdx.x] = s;
    }
    __syncthreads();
    for (int h = SD_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_sum[0][threadIdx.x] = s_sum[0][threadIdx.x] + s_sum[0][threadIdx.x + h];
            s_sum[1][threadIdx.x] = s_sum[1][threadIdx.x] + s_sum[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long n = hdr->list_n;                               // = n_border[0] + n_border[1]
        row[0] = hdr->n_border[0];
        row[1] = hdr->n_border[1];
        row[2] = hdr->n_within;
        row[3] = hdr->max_bits;
        row[4] = (unsigned long long)__double_as_longlong(s_sum[0][0]);
        row[5] = (unsigned long long)__double_as_longlong(s_sum[1][0]);
        unsigned long long lo = 0ull, hi = 0ull;
        if (n) percentile_ranks(n, lo, hi);
        hdr->rank[0] = lo;
        hdr->rank[1] = hi;
    }
}

// histogram of digit `shift / 8` over the keys that agree with prefix[r] above it, for both ranks
__global__ __launch_bounds__(SD_THREADS) void sd_hist_kernel(const unsigned long long* __restrict__ list, SdHeader* hdr, int shift) {
    __shared__ unsigned int s_hist[2][256];
    s_hist[0][threadIdx.x] = 0u;
    s_hist[1][threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long n = hdr->list_n, p0 = hdr->prefix[0], p1 = hdr->prefix[1];
    const int up = shift + 8;                                                   // bits [up, 64) are decided
    const unsigned long long step = (unsigned long long)gridDim.x * SD_THREADS;
    for (unsigned long long i = (unsigned long long)blockIdx.x * SD_THREADS + threadIdx.x; i < n; i += step) {
        const unsigned long long key = list[i];
        const unsigned int digit = (unsigned int)(key >> shift) & 255u;
        if (up >= 64 || ((key ^ p0) >> up) == 0ull) atomicAdd(&s_hist[0][digit], 1u);
        if (up >= 64 || ((key ^ p1) >> up) == 0ull) atomicAdd(&s_hist[1][digit], 1u);
    }
    __syncthreads();
    if (s_hist[0][threadIdx.x]) atomicAdd(&hdr->hist[0][threadIdx.x], (unsigned long long)s_hist[0][threadIdx.x]);
    if (s_hist[1][threadIdx.x]) atomicAdd(&hdr->hist[1][threadIdx.x], (unsigned long long)s_hist[1][threadIdx.x]);
}

// the digit that holds rank[r]; the rank becomes the rank inside that digit's bucket. Clears the histogram. After shift 0 the
// prefixes are the two keys: they go to the table row.
__global__ __launch_bounds__(SD_THREADS) void sd_pick_kernel(SdHeader* hdr, int shift, unsigned long long* __restrict__ row) {
    if (threadIdx.x < 2 && hdr->list_n) {
        const int r = (int)threadIdx.x;
        unsigned long long k = hdr->rank[r], cum = 0ull;
        int digit = 255;
        for (int b = 0; b < 256; ++b) {
            const unsigned long long h = hdr->hist[r][b];
            if (k < cum + h) { digit = b; break; }
            cum += h;
        }
        hdr->rank[r] = k - cum;
        const unsigned long long p = hdr->prefix[r] | ((unsigned long long)digit << shift);
        hdr->prefix[r] = p;
        if (shift == 0) row[6 + r] = p;
    }
    __syncthreads();
    hdr->hist[0][threadIdx.x] = 0ull;
    hdr->hist[1][threadIdx.x] = 0ull;
}

inline int sd_grid(long work_items, int cap) {
    const long b = (work_items + SD_THREADS - 1) / SD_THREADS;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
inline long sd_round(long bytes) { return (bytes + 255) / 256 * 256; }

int sd_check_shape(const char* who, const int64_t* shape, long* n_out) {
    if (!shape) return fail(MPU_EINVAL, "%s: null shape", who);
    long n = 1;
    for (int k = 0; k < 3; ++k) {
        if (shape[k] < 1) return fail(MPU_EUNSUPPORTED, "%s: every dimension must be >= 1 (dimension %ld is %ld)", who, (long)k, (long)shape[k]);
        if (shape[k] > 0x7fffffffL || n * shape[k] > 0x7fffffffL)
            return fail(MPU_EUNSUPPORTED, "%s: need 1 <= X * Y * Z <= 2^31 - 1 voxels (i32 indices)", who);
        n *= shape[k];
    }
    *n_out = n;
    return MPU_OK;
}
int sd_check_spacing(const char* who, const double* spacing) {
    if (!spacing) return fail(MPU_EINVAL, "%s: null spacing", who);
    for (int k = 0; k < 3; ++k)
        if (!(spacing[k] > 0.0) || !(spacing[k] < __builtin_huge_val()))
            return fail(MPU_EINVAL, "%s: spacing must be finite and > 0 (axis %ld)", who, (long)k);
    return MPU_OK;
}

// scratch: header | partial sums f64 [2][SD_PART_BLOCKS] | line flags u8 [X Y] | start_y i32 [X Y] | start_x i32 [X] | A f64 [n] |
// B f64 [n] | key list u64 [2 n]
struct SdScratch { SdHeader* hdr; double* partial; uint8_t* line_flag; int* start_y; int* start_x; double* A; double* B; unsigned long long* list; };
constexpr long SD_PARTIAL_BYTES = 2L * SD_PART_BLOCKS * 8;
inline long sd_table_bytes(const SdDims& d) { return sd_round((long)d.X * d.Y) + sd_round(4L * d.X * d.Y) + sd_round(4L * d.X); }
inline SdScratch sd_carve(void* d_scratch, const SdDims& d) {
    const long n = d.n;
    char* s = (char*)d_scratch;
    SdScratch r;
    r.hdr = (SdHeader*)s;
    r.partial = (double*)(s + SD_HEADER_BYTES);
    r.line_flag = (uint8_t*)(s + SD_HEADER_BYTES + SD_PARTIAL_BYTES);
    r.start_y = (int*)(r.line_flag + sd_round((long)d.X * d.Y));
    r.start_x = (int*)((char*)r.start_y + sd_round(4L * d.X * d.Y));
    r.A = (double*)(s + SD_HEADER_BYTES + SD_PARTIAL_BYTES + sd_table_bytes(d));
    r.B = (double*)((char*)r.A + sd_round(n * 8));
    r.list = (unsigned long long*)((char*)r.B + sd_round(n * 8));
    return r;
}

// the three passes: Z -> out, Y -> tmp, X -> out
// cut >= 0: only `result <= cut` is asked of the output (see edt_line_kernel); root must be false then
int edt_launch(const uint8_t* labels, const SdDims& d, const double* spacing, int mode, int v, bool root, double* out, double* tmp,
               const SdScratch& s, hipStream_t st, double cut = -1.0) {
    const double wx = spacing[0] * spacing[0], wy = spacing[1] * spacing[1], wz = spacing[2] * spacing[2];
    const long nlines = (long)d.X * d.Y;
    const int gz = sd_grid(nlines * 64, SD_MAX_BLOCKS * 4), gl = sd_grid(d.n, SD_MAX_BLOCKS * 4);
    switch (mode) {
        case MPU_EDT_EQUAL: edt_z_kernel<MPU_EDT_EQUAL><<<dim3(gz), dim3(SD_THREADS), 0, st>>>(labels, d, v, wz, out, s.line_flag); break;
        case MPU_EDT_NOT_EQUAL: edt_z_kernel<MPU_EDT_NOT_EQUAL><<<dim3(gz), dim3(SD_THREADS), 0, st>>>(labels, d, v, wz, out, s.line_flag); break;
        default: edt_z_kernel<MPU_EDT_BORDER><<<dim3(gz), dim3(SD_THREADS), 0, st>>>(labels, d, v, wz, out, s.line_flag); break;
    }
    edt_start_y_kernel<<<dim3(sd_grid(nlines, SD_MAX_BLOCKS)), dim3(SD_THREADS), 0, st>>>(s.line_flag, d.X, d.Y, s.start_y);
    edt_start_x_kernel<<<dim3(sd_grid(d.X, SD_MAX_BLOCKS)), dim3(SD_THREADS), 0, st>>>(s.start_y, d.X, d.Y, s.start_x);
    if (cut >= 0.0) {
        edt_line_kernel<false, true><<<dim3(gl), dim3(SD_THREADS), 0, st>>>(out, tmp, (long)d.n, (long)d.Z, d.Y, wy, s.start_y, cut);
        edt_line_kernel<false, true><<<dim3(gl), dim3(SD_THREADS), 0, st>>>(tmp, out, (long)d.n, (long)d.Y * d.Z, d.X, wx, s.start_x, cut);
        return launch_ok();
    }
    edt_line_kernel<false, false><<<dim3(gl), dim3(SD_THREADS), 0, st>>>(out, tmp, (long)d.n, (long)d.Z, d.Y, wy, s.start_y, 0.0);
    if (root) edt_line_kernel<true, false><<<dim3(gl), dim3(SD_THREADS), 0, st>>>(tmp, out, (long)d.n, (long)d.Y * d.Z, d.X, wx, s.start_x, 0.0);
    else edt_line_kernel<false, false><<<dim3(gl), dim3(SD_THREADS), 0, st>>>(tmp, out, (long)d.n, (long)d.Y * d.Z, d.X, wx, s.start_x, 0.0);
    return launch_ok();
}

// ---- mpu_morph_ball: opening / closing by a Euclidean ball as two thresholds of the transform above ------------------------------
// With r2 = fl(radius * radius): dilate(M) = {d2(., M) <= r2}, erode(M) = {d2(., not M) > r2}; close = erode(dilate), open =
// dilate(erode). Per class c of the mask, ascending, on the map `out` the earlier classes left (launches: 5 + 1 + 5 + 1):
//   close   A = d2 to {out == c};  mask = A <= r2 (the dilation);  A = d2 to {mask == 0};  out = c where out == 0 and A > r2
//   open    A = d2 to {out != c};  mask = A >  r2 (the erosion);   A = d2 to {mask == 1};  out = 0 where out == c and not A <= r2
// d2 is symmetric in its two voxels, so M is inside close(M) and open(M) inside M: closing only ever adds, opening only removes.
// The mask is one byte per voxel in the key-list region of the scratch, which the transform does not use.
__global__ __launch_bounds__(SD_THREADS) void mb_begin_kernel(const uint8_t* labels, uint8_t* out, long n, long long* __restrict__ report,
                                                              int words) {
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < words; t += SD_THREADS) report[t] = 0ll;
    if (labels == out) return;
    const long step = (long)gridDim.x * SD_THREADS;
    for (long i = (long)blockIdx.x * SD_THREADS + threadIdx.x; i < n; i += step) out[i] = labels[i];
}

__global__ __launch_bounds__(SD_THREADS) void mb_threshold_kernel(const double* __restrict__ D, double r2, int op, uint8_t* __restrict__ mask,
                                                                  long n) {
    const long step = (long)gridDim.x * SD_THREADS;
    for (long i = (long)blockIdx.x * SD_THREADS + threadIdx.x; i < n; i += step) {
        const bool within = D[i] <= r2;
        mask[i] = (op == MPU_MORPH_CLOSE ? within : !within) ? 1 : 0;
    }
}

// *counter += the voxels rewritten (one atomic per workgroup that rewrote any)
__global__ __launch_bounds__(SD_THREADS) void mb_apply_kernel(uint8_t* out, const double* __restrict__ D, double r2, int op, int c, long n,
                                                              unsigned long long* counter) {
    __shared__ unsigned long long s_cnt;
    if (threadIdx.x == 0) s_cnt = 0ull;
    __syncthreads();
    const long step = (long)gridDim.x * SD_THREADS;
    unsigned long long cnt = 0ull;
    for (long i = (long)blockIdx.x * SD_THREADS + threadIdx.x; i < n; i += step) {
        const int v = (int)out[i];
        if (op == MPU_MORPH_CLOSE) {
            if (v == 0 && D[i] > r2) { out[i] = (uint8_t)c; ++cnt; }
        } else {
            if (v == c && !(D[i] <= r2)) { out[i] = 0; ++cnt; }
        }
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(counter, s_cnt);
}

}  // namespace
}  // namespace mpu

using namespace mpu;

extern "C" {

int64_t mpu_surface_scratch_bytes(const int64_t shape[3]) {
    long n = 0;
    if (sd_check_shape("mpu_surface_scratch_bytes", shape, &n) != MPU_OK) return -1;
    const SdDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    return SD_HEADER_BYTES + SD_PARTIAL_BYTES + sd_table_bytes(d) + 2 * sd_round(n * 8) + sd_round(2 * n * 8);
}

int mpu_edt_squared(const uint8_t* d_labels, const int64_t shape[3], const double spacing[3], int32_t predicate, int32_t value,
                    int32_t take_root, double* d_out, void* d_scratch, void* stream) {
    const char* who = "mpu_edt_squared";
    long n = 0;
    int rc = sd_check_shape(who, shape, &n);
    if (rc != MPU_OK) return rc;
    if ((rc = sd_check_spacing(who, spacing)) != MPU_OK) return rc;
    if (predicate != MPU_EDT_EQUAL && predicate != MPU_EDT_NOT_EQUAL && predicate != MPU_EDT_BORDER)
        return fail(MPU_EINVAL, "%s: predicate must be MPU_EDT_EQUAL, MPU_EDT_NOT_EQUAL or MPU_EDT_BORDER, got %ld", who, (long)predicate);
    if (value < 0 || value > 255) return fail(MPU_EINVAL, "%s: value must be a u8 label (0 .. 255), got %ld", who, (long)value);
    MPU_REQUIRE(d_labels && d_out && d_scratch, "mpu_edt_squared: null argument");
    MPU_REQUIRE(((uintptr_t)d_out % 8) == 0 && ((uintptr_t)d_scratch % 16) == 0,
                "mpu_edt_squared: d_out must be aligned to 8 bytes and d_scratch to 16");
    const SdDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    const SdScratch s = sd_carve(d_scratch, d);
    return edt_launch(d_labels, d, spacing, predicate, value, take_root != 0, d_out, s.B, s, (hipStream_t)stream);
}

int mpu_surface_table(const uint8_t* d_pred, const uint8_t* d_truth, const int64_t shape[3], const double spacing[3], int32_t n_classes,
                      uint32_t class_mask, double tolerance, void* d_table, void* d_scratch, void* stream) {
    const char* who = "mpu_surface_table";
    long n = 0;
    int rc = sd_check_shape(who, shape, &n);
    if (rc != MPU_OK) return rc;
    if (n_classes < 1 || n_classes > SD_MAXK) return fail(MPU_EUNSUPPORTED, "%s: need 1 <= n_classes <= 16, got %ld", who, (long)n_classes);
    if ((rc = sd_check_spacing(who, spacing)) != MPU_OK) return rc;
    if ((class_mask & 1u) || (class_mask >> n_classes) != 0u)
        return fail(MPU_EINVAL, "%s: class_mask may name classes 1 .. n_classes - 1 only (mask 0x%lx, n_classes %ld)", who,
                    (long)class_mask, (long)n_classes);
    if (!(tolerance > 0.0) || !(tolerance < __builtin_huge_val()))
        return fail(MPU_EINVAL, "%s: tolerance must be finite and > 0", who);
    MPU_REQUIRE(d_pred && d_truth && d_table && d_scratch, "mpu_surface_table: null argument");
    MPU_REQUIRE(((uintptr_t)d_table % 8) == 0 && ((uintptr_t)d_scratch % 16) == 0,
                "mpu_surface_table: d_table must be aligned to 8 bytes and d_scratch to 16");
    const SdDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    hipStream_t st = (hipStream_t)stream;
    const SdScratch s = sd_carve(d_scratch, d);
    unsigned long long* table = (unsigned long long*)d_table;
    const double tau2 = tolerance * tolerance;
    const int gg = sd_grid(n, SD_PART_BLOCKS), gh = sd_grid(2 * n, SD_PART_BLOCKS);
    sd_zero_table_kernel<<<dim3(1), dim3(SD_THREADS), 0, st>>>(table, n_classes * SD_COLS);
    for (int c = 1; c < n_classes; ++c) {
        if (!((class_mask >> c) & 1u)) continue;
        unsigned long long* row = table + (long)c * SD_COLS;
        sd_begin_kernel<<<dim3(1), dim3(SD_THREADS), 0, st>>>(s.hdr);
        if ((rc = edt_launch(d_truth, d, spacing, MPU_EDT_BORDER, c, false, s.A, s.B, s, st)) != MPU_OK) return rc;
        sd_gather_kernel<<<dim3(gg), dim3(SD_THREADS), 0, st>>>(d_pred, d, c, s.A, tau2, 0, s.hdr, s.list, s.partial);
        if ((rc = edt_launch(d_pred, d, spacing, MPU_EDT_BORDER, c, false, s.A, s.B, s, st)) != MPU_OK) return rc;
        sd_gather_kernel<<<dim3(gg), dim3(SD_THREADS), 0, st>>>(d_truth, d, c, s.A, tau2, 1, s.hdr, s.list, s.partial + SD_PART_BLOCKS);
        sd_plan_kernel<<<dim3(1), dim3(SD_THREADS), 0, st>>>(s.hdr, s.partial, gg, row);
        for (int shift = 56; shift >= 0; shift -= 8) {
            sd_hist_kernel<<<dim3(gh), dim3(SD_THREADS), 0, st>>>(s.list, s.hdr, shift);
            sd_pick_kernel<<<dim3(1), dim3(SD_THREADS), 0, st>>>(s.hdr, shift, row);
        }
    }
    return launch_ok();
}

int mpu_morph_ball(const uint8_t* d_labels, const int64_t shape[3], const double spacing[3], int32_t n_classes, uint32_t class_mask,
                   int32_t op, double radius, uint8_t* d_out, int64_t* d_report, void* d_scratch, void* stream) {
    const char* who = "mpu_morph_ball";
    long n = 0;
    int rc = sd_check_shape(who, shape, &n);
    if (rc != MPU_OK) return rc;
    if (n_classes < 1 || n_classes > SD_MAXK) return fail(MPU_EUNSUPPORTED, "%s: need 1 <= n_classes <= 16, got %ld", who, (long)n_classes);
    if ((rc = sd_check_spacing(who, spacing)) != MPU_OK) return rc;
    if ((class_mask & 1u) || (class_mask >> n_classes) != 0u)
        return fail(MPU_EINVAL, "%s: class_mask may name classes 1 .. n_classes - 1 only (mask 0x%lx, n_classes %ld)", who,
                    (long)class_mask, (long)n_classes);
    if (op != MPU_MORPH_OPEN && op != MPU_MORPH_CLOSE)
        return fail(MPU_EINVAL, "%s: op must be MPU_MORPH_OPEN or MPU_MORPH_CLOSE, got %ld", who, (long)op);
    if (!(radius > 0.0) || !(radius < __builtin_huge_val())) return fail(MPU_EINVAL, "%s: radius must be finite and > 0", who);
    MPU_REQUIRE(d_labels && d_out && d_report && d_scratch, "mpu_morph_ball: null argument");
    MPU_REQUIRE(((uintptr_t)d_report % 8) == 0 && ((uintptr_t)d_scratch % 16) == 0,
                "mpu_morph_ball: d_report must be aligned to 8 bytes and d_scratch to 16");
    const uintptr_t a = (uintptr_t)d_labels, b = (uintptr_t)d_out;
    MPU_REQUIRE(a == b || a + (uintptr_t)n <= b || b + (uintptr_t)n <= a,
                "mpu_morph_ball: d_out must be d_labels itself (in place) or not overlap it");
    const SdDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    hipStream_t st = (hipStream_t)stream;
    const SdScratch s = sd_carve(d_scratch, d);
    uint8_t* mask = (uint8_t*)s.list;
    unsigned long long* report = (unsigned long long*)d_report;
    const double r2 = radius * radius;
    const int g = sd_grid(n, SD_MAX_BLOCKS);
    mb_begin_kernel<<<dim3(g), dim3(SD_THREADS), 0, st>>>(d_labels, d_out, n, (long long*)d_report, 2 * n_classes);
    for (int c = 1; c < n_classes; ++c) {
        if (!((class_mask >> c) & 1u)) continue;
        const bool closing = op == MPU_MORPH_CLOSE;
        if ((rc = edt_launch(d_out, d, spacing, closing ? MPU_EDT_EQUAL : MPU_EDT_NOT_EQUAL, c, false, s.A, s.B, s, st, r2)) != MPU_OK) return rc;
        mb_threshold_kernel<<<dim3(g), dim3(SD_THREADS), 0, st>>>(s.A, r2, op, mask, n);
        if ((rc = edt_launch(mask, d, spacing, MPU_EDT_EQUAL, closing ? 0 : 1, false, s.A, s.B, s, st, r2)) != MPU_OK) return rc;
        mb_apply_kernel<<<dim3(g), dim3(SD_THREADS), 0, st>>>(d_out, s.A, r2, op, c, n, report + 2 * c + (closing ? 0 : 1));
    }
    return launch_ok();
}

}  // extern "C"
