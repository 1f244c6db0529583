// Connected components of a resident u8 label volume and the "keep the largest component per class" filter of `mp predict
// --largest_component` (no reference counterpart: the reference post-processes nothing). Pure integer work, exact and
// deterministic by construction.
//
//   labels [X][Y][Z] u8 (C order), connectivity 6 / 18 / 26 (scipy.ndimage.generate_binary_structure(3, 1 / 2 / 3)).
//   Two voxels are connected when they are neighbours under that structure and carry the same label c, 1 <= c < n_classes.
//   Label 0 and labels >= n_classes join nothing. All classes are labelled in ONE pass.
//   A component's NAME is the linear index of its first voxel (its smallest index).
//
// Union-find directly in global memory (Komura-style), on parent[] (i32 per voxel, -1 for voxels that join nothing). Every link
// points to a SMALLER index, so a chain is strictly decreasing, bounded below by 0, and its end -- the root, parent[r] == r -- is
// the minimum of everything merged into it. Launches (fixed number, no host loop, no host synchronisation):
//
//   init      parent[i] = the smallest-index same-label BACKWARD neighbour (one of the up to 13 neighbours with a smaller
//             linear index), or i. Zeroes the header (selection keys, totals, component counts).
//   compress  parent[i] = min(parent[i], find(i)) with an atomicMin on the voxel's OWN entry: the init trees become stars.
//   merge     for every other same-label backward neighbour j: unite(find(i), find(j)). A neighbour is skipped when it is
//             provably merged by someone else: the init link itself, and -- when the z - 1 neighbour W carries the label too -- every
//             neighbour that is also a backward neighbour of W (W's own thread merges it, or skips it for the same reason).
//             Afterwards the voxel's own entry is lowered to the root it reached -- through unite(), the one write protocol.
//   flatten   roots[i] = find(i) with PLAIN loads of parent[] (immutable in this launch) into a SECOND array.
//   count     size of a component, kept in the root's own parent[] word: parent[r] = r + size (r + size <= X * Y * Z fits i32;
//             no zeroing pass). A thread run-length-compresses its voxels; the runs meet in a per-workgroup LDS table (slot =
//             hash of the root), then ONE global atomic per (workgroup, root); a root whose slot is taken adds directly.
//   select    per root: 64-bit atomicMax of (size << 32) | (0xFFFFFFFF - root) per class -- largest size, then smallest first
//             index, which is np.argmax(np.bincount(...)) over ndimage.label's raster numbering; component and voxel totals
//             per class. Block-local in LDS first, then at most 3 * n_classes global atomics per workgroup.
//   apply     out = labels with the voxels of a masked class outside its winner set to 0; block 0 writes the report.
// The same labelling and count serve the size threshold of `mp predict --min_component_voxels` (select<SMALL>, drop) and -- on a
// one-byte map of the background -- the hole filling of `--fill_holes` (the fh_* kernels; their protocol stands above them).
//
// Visibility (the per-XCD L2s are not coherent with each other, a CU's L1 is never refreshed): inside a launch the ONLY
// communication between workgroups is agent-scope atomic read-modify-writes on parent[] (atomicMin) whose returned old value is
// authoritative. find() in compress / merge reads with relaxed agent-scope atomic loads and stays correct on stale values: parents
// only ever decrease, so a stale parent is an OLDER ancestor -- still an ancestor; a stale "root" is caught by the atomicMin that
// follows (old != a) and the loop goes on with the returned value. No flags, no spin-waits, no grid barrier: nothing waits on
// another workgroup, every loop runs down a strictly decreasing chain. Plain loads and stores touch only data of EARLIER
// launches (flatten, count's reads, select, apply) or words that only this thread touches in this launch.
#include "common.h"

namespace mpu {
namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_MAX_BLOCKS = 2048;                 // memory-bound passes: 256 CUs x 8 workgroups, grid-stride beyond
constexpr int CC_MAXK = 16;
constexpr long CC_HEADER_BYTES = 512;               // u64 best[16] | u64 total[16] | u64 ncomp[16] | pad

struct CcHeader { unsigned long long best[CC_MAXK], total[CC_MAXK], ncomp[CC_MAXK]; };
static_assert(sizeof(CcHeader) <= CC_HEADER_BYTES, "header");

struct CcDims { int X, Y, Z, n; };

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int min_agent(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// end of the chain from x as this CU sees it (an ancestor of x: the root, or a former root when the view is stale)
__device__ __forceinline__ int find_agent(const int* L, int x) {
    int p;
    while ((p = ld_agent(L + x)) < x) x = p;
    return x;
}
__device__ __forceinline__ int find_plain(const int* __restrict__ L, int x) {
    int p;
    while ((p = L[x]) < x) x = p;
    return x;
}
// merges the trees of a and b; returns the smaller end it reached. max(a, b) strictly decreases per iteration.
__device__ __forceinline__ int unite(int* L, int a, int b) {
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = min_agent(L + a, b);            // authoritative: old == a  <=>  a WAS a root and now hangs under b
        if (old == a) return b;
        a = find_agent(L, old);                         // a's earlier parent lost (or kept) the word: its tree must meet b's too
        b = find_agent(L, b);
    }
    return a;
}

// the four labels of voxels [i0, i0 + 4) as one dword (missing ones 0); aligned4: labels is 4-byte aligned (i0 % 4 == 0)
__device__ __forceinline__ uint32_t load4(const uint8_t* labels, long i0, int n, bool aligned4) {
    if (aligned4 && i0 + 4 <= n) return *(const uint32_t*)(labels + i0);
    uint32_t w = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < n) w |= (uint32_t)labels[i0 + k] << (8 * k);
    return w;
}
__device__ __forceinline__ void store4(int* dst, long i0, int n, const int (&v)[4]) {
    if (i0 + 4 <= n && (((uintptr_t)dst) & 15) == 0) { *(int4*)(dst + i0) = make_int4(v[0], v[1], v[2], v[3]); return; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < n) dst[i0 + k] = v[k];
}
__device__ __forceinline__ void load4i(const int* src, long i0, int n, int (&v)[4]) {
    if (i0 + 4 <= n && (((uintptr_t)src) & 15) == 0) { const int4 t = *(const int4*)(src + i0); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? src[i0 + k] : -1;
}

// backward neighbour k of 13, ascending linear index: (dx, dy, dz) = (-1, *, *) x 9, (0, -1, *) x 3, (0, 0, -1)
__device__ __forceinline__ constexpr int nb_dx(int k) { return k < 9 ? -1 : 0; }
__device__ __forceinline__ constexpr int nb_dy(int k) { return k < 9 ? k / 3 - 1 : (k < 12 ? -1 : 0); }
__device__ __forceinline__ constexpr int nb_dz(int k) { return k < 9 ? k % 3 - 1 : (k < 12 ? k - 10 : -1); }
__device__ __forceinline__ constexpr int iabs(int v) { return v < 0 ? -v : v; }
// LEVEL 1 / 2 / 3 = connectivity 6 / 18 / 26
template <int LEVEL> __device__ __forceinline__ constexpr bool in_struct(int dx, int dy, int dz) {
    return iabs(dx) <= 1 && iabs(dy) <= 1 && iabs(dz) <= 1 && iabs(dx) + iabs(dy) + iabs(dz) <= LEVEL;
}
__device__ __forceinline__ bool nb_inside(int k, int x, int y, int z, const CcDims& d) {
    return x + nb_dx(k) >= 0 && (unsigned)(y + nb_dy(k)) < (unsigned)d.Y && (unsigned)(z + nb_dz(k)) < (unsigned)d.Z;
}
__device__ __forceinline__ void coords(unsigned i, const CcDims& d, int& x, int& y, int& z) {
    const unsigned t = i / (unsigned)d.Z;
    z = (int)(i - t * (unsigned)d.Z);
    x = (int)(t / (unsigned)d.Y);
    y = (int)(t - (unsigned)x * (unsigned)d.Y);
}
__device__ __forceinline__ void next_coords(const CcDims& d, int& x, int& y, int& z) {
    if (++z == d.Z) { z = 0; if (++y == d.Y) { y = 0; ++x; } }
}

template <int LEVEL>
__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const uint8_t* __restrict__ labels, int* __restrict__ parent, CcDims d,
                                                             int K, CcHeader* __restrict__ hdr) {
    if (blockIdx.x == 0 && threadIdx.x < 3 * CC_MAXK) ((unsigned long long*)hdr)[threadIdx.x] = 0ull;
    const bool aligned4 = (((uintptr_t)labels) & 3) == 0;
    const long ngroups = ((long)d.n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    const long sYZ = (long)d.Y * d.Z;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
        const uint32_t w = load4(labels, i0, d.n, aligned4);
        int out[4] = {-1, -1, -1, -1};
        if (w != 0u) {
            int x, y, z;
            coords((unsigned)i0, d, x, y, z);
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int c = (int)((w >> (8 * k4)) & 0xffu);
                if (c != 0 && c < K && i0 + k4 < d.n) {
                    const long i = i0 + k4;
                    int p = (int)i;
                    bool found = false;
#pragma unroll
                    for (int k = 0; k < 13; ++k) {
                        if (!in_struct<LEVEL>(nb_dx(k), nb_dy(k), nb_dz(k))) continue;
                        if (found || !nb_inside(k, x, y, z, d)) continue;
                        const long j = i + nb_dx(k) * sYZ + nb_dy(k) * (long)d.Z + nb_dz(k);
                        if ((int)labels[j] == c) { p = (int)j; found = true; }
                    }
                    out[k4] = p;
                }
                next_coords(d, x, y, z);
            }
        }
        store4(parent, i0, d.n, out);
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_compress_kernel(int* parent, int n) {
    const long ngroups = ((long)n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= n) break;
            const int i = (int)(i0 + k);
            const int p = ld_agent(parent + i);         // (init's value or lower: this launch only lowers it)
            if (p < 0 || p == i) continue;
            const int r = find_agent(parent, p);
            if (r < p) min_agent(parent + i, r);        // own entry, read-modify-write: an ancestor replaces an ancestor
        }
    }
}

template <int LEVEL>
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const uint8_t* __restrict__ labels, int* parent, CcDims d, int K) {
    const bool aligned4 = (((uintptr_t)labels) & 3) == 0;
    const long ngroups = ((long)d.n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    const long sYZ = (long)d.Y * d.Z;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
        const uint32_t w = load4(labels, i0, d.n, aligned4);
        if (w == 0u) continue;
        int x, y, z;
        coords((unsigned)i0, d, x, y, z);
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            const int c = (int)((w >> (8 * k4)) & 0xffu);
            if (c != 0 && c < K && i0 + k4 < d.n) {
                const long i = i0 + k4;
                const bool w_same = z > 0 && (int)labels[i - 1] == c;
                bool first = true;
                int a = -1;
#pragma unroll
                for (int k = 0; k < 13; ++k) {
                    if (!in_struct<LEVEL>(nb_dx(k), nb_dy(k), nb_dz(k))) continue;
                    if (!nb_inside(k, x, y, z, d)) continue;
                    const long j = i + nb_dx(k) * sYZ + nb_dy(k) * (long)d.Z + nb_dz(k);
                    if ((int)labels[j] != c) continue;
                    if (first) { first = false; continue; }                     // the init link
                    // also a backward neighbour of W = (x, y, z - 1): W's thread sees to it
                    if (k != 12 && in_struct<LEVEL>(nb_dx(k), nb_dy(k), nb_dz(k) + 1) && w_same) continue;
                    if (a < 0) a = find_agent(parent, (int)i);
                    a = unite(parent, a, find_agent(parent, (int)j));
                }
                // shorten the chain through this voxel. The same protocol as any union (i need not be a root there): should the
                // atomicMin displace a parent that is not on the way to a, unite() goes on with that parent
                if (a >= 0 && ld_agent(parent + (int)i) > a) unite(parent, (int)i, a);
            }
            next_coords(d, x, y, z);
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ roots, int n) {
    const long ngroups = ((long)n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
        int p[4];
        load4i(parent, i0, n, p);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p[k] >= 0 && p[k] != (int)(i0 + k)) p[k] = find_plain(parent, p[k]);
        store4(roots, i0, n, p);
    }
}

// A workgroup's counts meet in LDS first: slot = hash of the root; a slot belongs to the first root that claims it (CAS on the
// key), a root that finds its slot taken adds to the global word directly. Exact whatever the collisions.
constexpr int CC_SLOTS = 1024;
__device__ __forceinline__ void count_add(int* s_key, int* s_cnt, int* sizes, int r, int c) {
    const unsigned h = ((unsigned)r * 2654435761u) >> 22;                    // 10 bits
    const int k = atomicCAS(&s_key[h], -1, r);
    if (k == -1 || k == r) atomicAdd(&s_cnt[h], c);
    else atomicAdd(sizes + r, c);
}

// sizes[r] (= parent[r], holding r) += members of r. Only root words are touched, and only by atomic adds. A thread run-length
// compresses the roots it walks; runs go to the workgroup's LDS table, the table to the root words: a component that fills the
// volume costs one global atomic per workgroup, not one per run.
__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const int* __restrict__ roots, int* sizes, int n) {
    __shared__ int s_key[CC_SLOTS], s_cnt[CC_SLOTS];
    for (int t = threadIdx.x; t < CC_SLOTS; t += CC_THREADS) { s_key[t] = -1; s_cnt[t] = 0; }
    __syncthreads();
    const long ngroups = ((long)n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    int cur = -1, cnt = 0;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        int r[4];
        load4i(roots, g * 4, n, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (r[k] < 0) continue;
            if (r[k] == cur) { ++cnt; continue; }
            if (cnt) count_add(s_key, s_cnt, sizes, cur, cnt);
            cur = r[k]; cnt = 1;
        }
    }
    if (cnt) count_add(s_key, s_cnt, sizes, cur, cnt);
    __syncthreads();
    for (int t = threadIdx.x; t < CC_SLOTS; t += CC_THREADS)
        if (s_cnt[t]) atomicAdd(sizes + s_key[t], s_cnt[t]);
}

// SMALL (mpu_remove_small_components): `best` is not the key of the winner but the SUM of the sizes below min_voxels
template <bool SMALL>
__global__ __launch_bounds__(CC_THREADS) void cc_select_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ roots,
                                                               const int* __restrict__ sizes, int n, CcHeader* hdr, long long min_voxels) {
    __shared__ unsigned long long s_best[CC_MAXK], s_total[CC_MAXK], s_ncomp[CC_MAXK];
    if (threadIdx.x < CC_MAXK) { s_best[threadIdx.x] = 0ull; s_total[threadIdx.x] = 0ull; s_ncomp[threadIdx.x] = 0ull; }
    __syncthreads();
    const long ngroups = ((long)n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
        int r[4];
        load4i(roots, i0, n, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = (int)(i0 + k);
            if (r[k] < 0 || r[k] != i) continue;
            const int c = (int)labels[i] & (CC_MAXK - 1);                         // (a root carries 1 <= c < n_classes <= 16)
            const unsigned long long size = (unsigned long long)(unsigned)(sizes[i] - i);
            if (SMALL) { if ((long long)size < min_voxels) atomicAdd(&s_best[c], size); }
            else atomicMax(&s_best[c], (size << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
            atomicAdd(&s_total[c], size);
            atomicAdd(&s_ncomp[c], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < CC_MAXK && s_ncomp[threadIdx.x]) {
        if (SMALL) atomicAdd(&hdr->best[threadIdx.x], s_best[threadIdx.x]);
        else atomicMax(&hdr->best[threadIdx.x], s_best[threadIdx.x]);
        atomicAdd(&hdr->total[threadIdx.x], s_total[threadIdx.x]);
        atomicAdd(&hdr->ncomp[threadIdx.x], s_ncomp[threadIdx.x]);
    }
}

// labels / out may be the same pointer: a voxel is read and written by the same thread, and by no other
__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(const uint8_t* labels, const int* __restrict__ roots, int n, int K,
                                                              unsigned class_mask, const CcHeader* __restrict__ hdr, uint8_t* out,
                                                              long long* __restrict__ report) {
    __shared__ int s_win[CC_MAXK];                       // winning root of a filtered class, -2 = keep every voxel
    if (threadIdx.x < CC_MAXK) {
        const int c = (int)threadIdx.x;
        const bool masked = c < K && ((class_mask >> c) & 1u);
        const unsigned long long best = c < K ? hdr->best[c] : 0ull;
        s_win[c] = masked ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -2;      // (class absent: -1, matches no voxel)
        if (blockIdx.x == 0 && c < K) {
            const long long total = (long long)hdr->total[c], kept = masked ? (long long)(best >> 32) : total;
            report[3 * c + 0] = (long long)hdr->ncomp[c];
            report[3 * c + 1] = kept;
            report[3 * c + 2] = total - kept;
        }
    }
    __syncthreads();
    const bool vec = ((((uintptr_t)labels) | ((uintptr_t)out) | ((uintptr_t)roots)) & 15) == 0;
    const long ngroups = ((long)n + 15) / 16, stride = (long)gridDim.x * CC_THREADS;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 16;
        if (vec && i0 + 16 <= n) {
            const uint4 lw = *(const uint4*)(labels + i0);
            int4 rv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) rv[q] = *(const int4*)(roots + i0 + 4 * q);
            const uint32_t l[4] = {lw.x, lw.y, lw.z, lw.w};
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r[4] = {rv[q].x, rv[q].y, rv[q].z, rv[q].w};
                uint32_t ow = l[q];
                if (ow != 0u) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = (int)((ow >> (8 * k)) & 0xffu);
                        if (r[k] >= 0) {                                          // (1 <= c < K: flatten named it)
                            const int win = s_win[c & (CC_MAXK - 1)];
                            if (win != -2 && win != r[k]) ow &= ~(0xffu << (8 * k));
                        }
                    }
                }
                o[q] = ow;
            }
            *(uint4*)(out + i0) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            for (long i = i0; i < i0 + 16 && i < n; ++i) {                         // scalar: unaligned buffers, and the tail
                const int c = (int)labels[i], r = roots[i];
                uint8_t v = (uint8_t)c;
                if (r >= 0) {
                    const int win = s_win[c & (CC_MAXK - 1)];
                    if (win != -2 && win != r) v = 0;
                }
                out[i] = v;
            }
        }
    }
}

// ---- mpu_remove_small_components: label -> count -> select<SMALL> -> drop ------------------------------------------------------
__device__ __forceinline__ void store4b(uint8_t* out, long i0, int n, uint32_t w) {
    if (i0 + 4 <= n && (((uintptr_t)out) & 3) == 0) { *(uint32_t*)(out + i0) = w; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < n) out[i0 + k] = (uint8_t)(w >> (8 * k));
}

// out = labels with the voxels of a masked class whose component has fewer than min_voxels voxels set to 0; block 0 writes the
// report. labels / out may be the same pointer (a voxel is read and written by the same thread, and by no other).
__global__ __launch_bounds__(CC_THREADS) void cc_drop_small_kernel(const uint8_t* labels, const int* __restrict__ roots,
                                                                   const int* __restrict__ sizes, int n, int K, unsigned class_mask,
                                                                   long long min_voxels, const CcHeader* __restrict__ hdr, uint8_t* out,
                                                                   long long* __restrict__ report) {
    if (blockIdx.x == 0 && (int)threadIdx.x < K) {
        const int c = (int)threadIdx.x;
        const long long total = (long long)hdr->total[c], removed = ((class_mask >> c) & 1u) ? (long long)hdr->best[c] : 0ll;
        report[3 * c + 0] = (long long)hdr->ncomp[c];
        report[3 * c + 1] = total - removed;
        report[3 * c + 2] = removed;
    }
    const bool aligned4 = (((uintptr_t)labels) & 3) == 0;
    const long ngroups = ((long)n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
        uint32_t w = load4(labels, i0, n, aligned4);
        if (w != 0u) {
            int r[4];
            load4i(roots, i0, n, r);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (r[k] < 0) continue;                                           // (1 <= c < K from here on: flatten named it)
                const unsigned c = (w >> (8 * k)) & 0xffu;
                if (((class_mask >> c) & 1u) && (long long)(sizes[r[k]] - r[k]) < min_voxels) w &= ~(0xffu << (8 * k));
            }
        }
        store4b(out, i0, n, w);
    }
}

// ---- mpu_fill_holes ---------------------------------------------------------------------------------------------------------------
// The background {label == 0} is labelled by cc_label on a one-byte map (1 = background) as "class 1 of 2". Per ROOT of a background
// component two u64 words: best[r] and cnt[r] (only root words are ever read or written).
//   background  bg[i] = labels[i] == 0
//   (cc_label)  roots[i] = first voxel of i's background component, -1 off the background
//   init        best[r] = cnt[r] = 0 at every root
//   border      best[r] = FH_OPEN for the root of every background voxel with an index of 0 or dim - 1 on some axis: not a cavity
//   vote c      cnt[r] += the face neighbours with label c of every voxel of cavity r      }  once per class c = 1 .. K - 1: the
//   fold c      best[r] = max(best[r], cnt[r] << 4 | 15 - c) where cnt[r] > 0; cnt[r] = 0    }  running best of (count, smallest class)
//   fill        out = labels, the voxels of a cavity whose winner is in class_mask set to the winner; cavities and voxels per class
//               (row 0: left unfilled) meet in LDS, then in the header
//   report      header -> report
// cnt <= 6 * voxels < 2^34, so the key fits 64 bits with room. Communication inside a launch is by atomic adds / maxima on root
// words alone, and no launch reads a word that the same launch modifies (vote reads best, adds to cnt).
constexpr unsigned long long FH_OPEN = ~0ull;

__global__ __launch_bounds__(CC_THREADS) void fh_background_kernel(const uint8_t* __restrict__ labels, uint8_t* __restrict__ bg, int n) {
    const bool aligned4 = (((uintptr_t)labels) & 3) == 0;
    const long ngroups = ((long)n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const uint32_t w = load4(labels, g * 4, n, aligned4);
        uint32_t b = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (((w >> (8 * k)) & 0xffu) == 0u) b |= 1u << (8 * k);
        store4b(bg, g * 4, n, b);                                                 // (positions >= n of the last group are not stored)
    }
}

__global__ __launch_bounds__(CC_THREADS) void fh_init_kernel(const int* __restrict__ roots, unsigned long long* __restrict__ best,
                                                             unsigned long long* __restrict__ cnt, int n) {
    const long stride = (long)gridDim.x * CC_THREADS;
    for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += stride)
        if (roots[i] == (int)i) { best[i] = 0ull; cnt[i] = 0ull; }
}

// one thread per voxel of the six faces would do; all voxels are walked (the coordinates decide) to keep the indexing in one place
__global__ __launch_bounds__(CC_THREADS) void fh_border_kernel(const int* __restrict__ roots, CcDims d, unsigned long long* best) {
    const long stride = (long)gridDim.x * CC_THREADS;
    for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < d.n; i += stride) {
        const int r = roots[i];
        if (r < 0) continue;
        int x, y, z;
        coords((unsigned)i, d, x, y, z);
        if (x != 0 && y != 0 && z != 0 && x != d.X - 1 && y != d.Y - 1 && z != d.Z - 1) continue;
        // a stale read only repeats the maximum; the atomic is what marks
        if (__hip_atomic_load(best + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != FH_OPEN) atomicMax(best + r, FH_OPEN);
    }
}

__global__ __launch_bounds__(CC_THREADS) void fh_vote_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ roots,
                                                             const unsigned long long* __restrict__ best, unsigned long long* cnt,
                                                             CcDims d, int c) {
    const long ngroups = ((long)d.n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    const long sYZ = (long)d.Y * d.Z;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
        int r[4];
        load4i(roots, i0, d.n, r);
        if (r[0] < 0 && r[1] < 0 && r[2] < 0 && r[3] < 0) continue;
        int x, y, z;
        coords((unsigned)i0, d, x, y, z);
        int cur = -1;
        unsigned long long votes = 0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (r[k] >= 0) {
                const long i = i0 + k;
                int v = 0;
                if (x > 0) v += (int)labels[i - sYZ] == c;
                if (x < d.X - 1) v += (int)labels[i + sYZ] == c;
                if (y > 0) v += (int)labels[i - d.Z] == c;
                if (y < d.Y - 1) v += (int)labels[i + d.Z] == c;
                if (z > 0) v += (int)labels[i - 1] == c;
                if (z < d.Z - 1) v += (int)labels[i + 1] == c;
                if (v) {
                    if (r[k] != cur) {
                        if (votes && best[cur] != FH_OPEN) atomicAdd(cnt + cur, votes);
                        cur = r[k]; votes = 0ull;
                    }
                    votes += (unsigned long long)v;
                }
            }
            next_coords(d, x, y, z);
        }
        if (votes && best[cur] != FH_OPEN) atomicAdd(cnt + cur, votes);
    }
}

__global__ __launch_bounds__(CC_THREADS) void fh_fold_kernel(const int* __restrict__ roots, unsigned long long* __restrict__ best,
                                                             unsigned long long* __restrict__ cnt, int n, int c) {
    const long stride = (long)gridDim.x * CC_THREADS;
    for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += stride) {
        if (roots[i] != (int)i) continue;
        const unsigned long long v = cnt[i];
        if (v == 0ull) continue;                                                 // (an open component never counts: v > 0 is a cavity)
        const unsigned long long key = (v << 4) | (unsigned long long)(15 - c);
        if (key > best[i]) best[i] = key;
        cnt[i] = 0ull;
    }
}

// labels / out may be the same pointer: a voxel is read and written by the same thread, and by no other
__global__ __launch_bounds__(CC_THREADS) void fh_fill_kernel(const uint8_t* labels, const int* __restrict__ roots,
                                                             const unsigned long long* __restrict__ best, int n, unsigned class_mask,
                                                             CcHeader* hdr, uint8_t* out) {
    __shared__ unsigned long long s_vox[CC_MAXK], s_cav[CC_MAXK];
    if (threadIdx.x < CC_MAXK) { s_vox[threadIdx.x] = 0ull; s_cav[threadIdx.x] = 0ull; }
    __syncthreads();
    const bool aligned4 = (((uintptr_t)labels) & 3) == 0;
    const long ngroups = ((long)n + 3) / 4, stride = (long)gridDim.x * CC_THREADS;
    for (long g = (long)blockIdx.x * CC_THREADS + threadIdx.x; g < ngroups; g += stride) {
        const long i0 = g * 4;
        uint32_t w = load4(labels, i0, n, aligned4);
        int r[4];
        load4i(roots, i0, n, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (r[k] < 0) continue;                                               // (label 0 from here on)
            const unsigned long long b = best[r[k]];
            if (b == FH_OPEN) continue;
            unsigned win = b ? 15u - (unsigned)(b & 15ull) : 0u;                    // 0: no vote at all
            if (!((class_mask >> win) & 1u)) win = 0u;                            // (bit 0 is never set)
            atomicAdd(&s_vox[win], 1ull);
            if (r[k] == (int)(i0 + k)) atomicAdd(&s_cav[win], 1ull);
            w |= win << (8 * k);
        }
        store4b(out, i0, n, w);
    }
    __syncthreads();
    if (threadIdx.x < CC_MAXK && s_vox[threadIdx.x]) {
        atomicAdd(&hdr->total[threadIdx.x], s_vox[threadIdx.x]);
        if (s_cav[threadIdx.x]) atomicAdd(&hdr->ncomp[threadIdx.x], s_cav[threadIdx.x]);
    }
}

__global__ void fh_report_kernel(const CcHeader* __restrict__ hdr, int K, long long* __restrict__ report) {
    const int c = (int)threadIdx.x;
    if (c < K) { report[2 * c + 0] = (long long)hdr->ncomp[c]; report[2 * c + 1] = (long long)hdr->total[c]; }
}

inline int cc_grid(long work_items) {
    const long b = (work_items + CC_THREADS - 1) / CC_THREADS;
    return (int)(b < 1 ? 1 : (b > CC_MAX_BLOCKS ? CC_MAX_BLOCKS : b));
}
inline long cc_array_bytes(long n) { return (n * 4 + 255) / 256 * 256; }

// the argument checks shared by the entries; 0 or the status to return (mpu_last_error set). *n_out = voxels
int cc_check_shape(const char* who, const int64_t* shape, int32_t n_classes, long* n_out) {
    if (!shape) return fail(MPU_EINVAL, "%s: null shape", who);
    if (n_classes < 1 || n_classes > CC_MAXK) return fail(MPU_EUNSUPPORTED, "%s: need 1 <= n_classes <= 16, got %ld", who, (long)n_classes);
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
int cc_check_connectivity(const char* who, int32_t connectivity) {
    if (connectivity != 6 && connectivity != 18 && connectivity != 26)
        return fail(MPU_EINVAL, "%s: connectivity must be 6, 18 or 26, got %ld", who, (long)connectivity);
    return MPU_OK;
}

inline long fh_round(long bytes) { return (bytes + 255) / 256 * 256; }
// every check of a filter entry (mpu_remove_small_components, mpu_fill_holes), in the order of mpu_keep_largest_components
int cc_check_filter(const char* who, const int64_t* shape, int32_t connectivity, int32_t n_classes, uint32_t class_mask,
                    const uint8_t* d_labels, const uint8_t* d_out, const int64_t* d_report, const void* d_scratch, long* n_out) {
    int rc = cc_check_shape(who, shape, n_classes, n_out);
    if (rc != MPU_OK) return rc;
    if ((rc = cc_check_connectivity(who, connectivity)) != MPU_OK) return rc;
    if ((class_mask & 1u) || (class_mask >> n_classes) != 0u)
        return fail(MPU_EINVAL, "%s: class_mask may name classes 1 .. n_classes - 1 only (mask 0x%lx, n_classes %ld)", who,
                    (long)class_mask, (long)n_classes);
    if (!d_labels || !d_out || !d_report || !d_scratch) return fail(MPU_EINVAL, "%s: null argument", who);
    if (((uintptr_t)d_report % 8) != 0 || ((uintptr_t)d_scratch % 16) != 0)
        return fail(MPU_EINVAL, "%s: d_report must be aligned to 8 bytes and d_scratch to 16", who);
    const uintptr_t a = (uintptr_t)d_labels, b = (uintptr_t)d_out, n = (uintptr_t)*n_out;
    if (!(a == b || a + n <= b || b + n <= a))
        return fail(MPU_EINVAL, "%s: d_out must be d_labels itself (in place) or not overlap it", who);
    return MPU_OK;
}

// init -> compress -> merge -> flatten: roots[i] = first voxel of i's component, -1 where the label joins nothing
int cc_label(const uint8_t* labels, const CcDims& d, int connectivity, int K, CcHeader* hdr, int* parent, int* roots, hipStream_t st) {
    const int grid4 = cc_grid(((long)d.n + 3) / 4);
    switch (connectivity) {
#define CC_CASE(CONN, LEVEL)                                                                                        \
        case CONN:                                                                                                  \
            cc_init_kernel<LEVEL><<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(labels, parent, d, K, hdr);             \
            cc_compress_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(parent, d.n);                              \
            cc_merge_kernel<LEVEL><<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(labels, parent, d, K);                 \
            break;
        CC_CASE(6, 1) CC_CASE(18, 2) CC_CASE(26, 3)
#undef CC_CASE
    }
    cc_flatten_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(parent, roots, d.n);
    return launch_ok();
}

}  // namespace
}  // namespace mpu

using namespace mpu;

extern "C" {

int64_t mpu_components_scratch_bytes(const int64_t shape[3]) {
    long n = 0;
    if (cc_check_shape("mpu_components_scratch_bytes", shape, 1, &n) != MPU_OK) return -1;
    return CC_HEADER_BYTES + 2 * cc_array_bytes(n);
}

int mpu_label_components(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes,
                         int32_t* d_roots, void* d_scratch, void* stream) {
    const char* who = "mpu_label_components";
    long n = 0;
    int rc = cc_check_shape(who, shape, n_classes, &n);
    if (rc != MPU_OK) return rc;
    if ((rc = cc_check_connectivity(who, connectivity)) != MPU_OK) return rc;
    MPU_REQUIRE(d_labels && d_roots && d_scratch, "mpu_label_components: null argument");
    MPU_REQUIRE(((uintptr_t)d_roots % 4) == 0 && ((uintptr_t)d_scratch % 16) == 0,
                "mpu_label_components: d_roots must be aligned to 4 bytes and d_scratch to 16");
    const CcDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    char* s = (char*)d_scratch;
    return cc_label(d_labels, d, connectivity, n_classes, (CcHeader*)s, (int*)(s + CC_HEADER_BYTES), d_roots, (hipStream_t)stream);
}

int mpu_keep_largest_components(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes,
                                uint32_t class_mask, uint8_t* d_out, int64_t* d_report, void* d_scratch, void* stream) {
    const char* who = "mpu_keep_largest_components";
    long n = 0;
    int rc = cc_check_shape(who, shape, n_classes, &n);
    if (rc != MPU_OK) return rc;
    if ((rc = cc_check_connectivity(who, connectivity)) != MPU_OK) return rc;
    if ((class_mask & 1u) || (n_classes < 32 && (class_mask >> n_classes) != 0u))
        return fail(MPU_EINVAL, "%s: class_mask may name classes 1 .. n_classes - 1 only (mask 0x%lx, n_classes %ld)", who,
                    (long)class_mask, (long)n_classes);
    MPU_REQUIRE(d_labels && d_out && d_report && d_scratch, "mpu_keep_largest_components: null argument");
    MPU_REQUIRE(((uintptr_t)d_report % 8) == 0 && ((uintptr_t)d_scratch % 16) == 0,
                "mpu_keep_largest_components: d_report must be aligned to 8 bytes and d_scratch to 16");
    const uintptr_t a = (uintptr_t)d_labels, b = (uintptr_t)d_out;
    MPU_REQUIRE(a == b || a + (uintptr_t)n <= b || b + (uintptr_t)n <= a,
                "mpu_keep_largest_components: d_out must be d_labels itself (in place) or not overlap it");
    const CcDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)d_scratch;
    CcHeader* hdr = (CcHeader*)s;
    int* parent = (int*)(s + CC_HEADER_BYTES);
    int* roots = (int*)(s + CC_HEADER_BYTES + cc_array_bytes(n));
    if ((rc = cc_label(d_labels, d, connectivity, n_classes, hdr, parent, roots, st)) != MPU_OK) return rc;
    const int grid4 = cc_grid((n + 3) / 4);
    cc_count_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(roots, parent, d.n);
    cc_select_kernel<false><<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(d_labels, roots, parent, d.n, hdr, 0ll);
    cc_apply_kernel<<<dim3(cc_grid((n + 15) / 16)), dim3(CC_THREADS), 0, st>>>(d_labels, roots, d.n, n_classes, class_mask, hdr, d_out,
                                                                              (long long*)d_report);
    return launch_ok();
}

int64_t mpu_fill_holes_scratch_bytes(const int64_t shape[3]) {
    long n = 0;
    if (cc_check_shape("mpu_fill_holes_scratch_bytes", shape, 1, &n) != MPU_OK) return -1;
    return CC_HEADER_BYTES + 2 * cc_array_bytes(n) + fh_round(n) + 2 * fh_round(8 * n);
}

int mpu_remove_small_components(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes,
                                uint32_t class_mask, int64_t min_voxels, uint8_t* d_out, int64_t* d_report, void* d_scratch,
                                void* stream) {
    const char* who = "mpu_remove_small_components";
    long n = 0;
    int rc = cc_check_filter(who, shape, connectivity, n_classes, class_mask, d_labels, d_out, d_report, d_scratch, &n);
    if (rc != MPU_OK) return rc;
    if (min_voxels < 1) return fail(MPU_EINVAL, "%s: min_voxels must be >= 1, got %ld", who, (long)min_voxels);
    const CcDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)d_scratch;
    CcHeader* hdr = (CcHeader*)s;
    int* parent = (int*)(s + CC_HEADER_BYTES);
    int* roots = (int*)(s + CC_HEADER_BYTES + cc_array_bytes(n));
    if ((rc = cc_label(d_labels, d, connectivity, n_classes, hdr, parent, roots, st)) != MPU_OK) return rc;
    const int grid4 = cc_grid((n + 3) / 4);
    cc_count_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(roots, parent, d.n);
    cc_select_kernel<true><<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(d_labels, roots, parent, d.n, hdr, (long long)min_voxels);
    cc_drop_small_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(d_labels, roots, parent, d.n, n_classes, class_mask,
                                                                  (long long)min_voxels, hdr, d_out, (long long*)d_report);
    return launch_ok();
}

int mpu_fill_holes(const uint8_t* d_labels, const int64_t shape[3], int32_t connectivity, int32_t n_classes, uint32_t class_mask,
                   uint8_t* d_out, int64_t* d_report, void* d_scratch, void* stream) {
    const char* who = "mpu_fill_holes";
    long n = 0;
    int rc = cc_check_filter(who, shape, connectivity, n_classes, class_mask, d_labels, d_out, d_report, d_scratch, &n);
    if (rc != MPU_OK) return rc;
    const CcDims d = {(int)shape[0], (int)shape[1], (int)shape[2], (int)n};
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)d_scratch;
    CcHeader* hdr = (CcHeader*)s;
    int* parent = (int*)(s + CC_HEADER_BYTES);
    int* roots = (int*)(s + CC_HEADER_BYTES + cc_array_bytes(n));
    uint8_t* bg = (uint8_t*)(s + CC_HEADER_BYTES + 2 * cc_array_bytes(n));
    unsigned long long* best = (unsigned long long*)(bg + fh_round(n));
    unsigned long long* cnt = (unsigned long long*)((char*)best + fh_round(8 * n));
    const int grid4 = cc_grid((n + 3) / 4), grid1 = cc_grid(n);
    fh_background_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(d_labels, bg, d.n);
    if ((rc = cc_label(bg, d, connectivity, 2, hdr, parent, roots, st)) != MPU_OK) return rc;      // (zeroes the header)
    fh_init_kernel<<<dim3(grid1), dim3(CC_THREADS), 0, st>>>(roots, best, cnt, d.n);
    fh_border_kernel<<<dim3(grid1), dim3(CC_THREADS), 0, st>>>(roots, d, best);
    for (int c = 1; c < n_classes; ++c) {
        fh_vote_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(d_labels, roots, best, cnt, d, c);
        fh_fold_kernel<<<dim3(grid1), dim3(CC_THREADS), 0, st>>>(roots, best, cnt, d.n, c);
    }
    fh_fill_kernel<<<dim3(grid4), dim3(CC_THREADS), 0, st>>>(d_labels, roots, best, d.n, class_mask, hdr, d_out);
    fh_report_kernel<<<dim3(1), dim3(64), 0, st>>>(hdr, n_classes, (long long*)d_report);
    return launch_ok();
}

}  // extern "C"
