// NIfTI-1 payload -> resident volume: what nifti.read_nifti does with NumPy on the host (reshape(order="F"), the optional
// scl_slope / scl_inter pass, np.array(dtype=float32, order="C")), done on the device beside volume_stats.hip.
//
//   mpu_volume_decode   payload [C][Z][Y][X] (Fortran order: x fastest) of one of the ten NIfTI datatypes, either endianness
//                       -> image  f32 [X][Y][Z][C] (C order), or
//                       -> labels u8  [X][Y][Z][C] and a count of the voxels astype(uint8) is not defined for.
//
// Compiled with -ffp-contract=off (build.PER_FILE). The scaled branch is `f64(stored) * slope + inter`, two rounded f64
// operations, then one f64 -> f32 rounding. A contracted multiply-add differs from that only where the exact product lies
// within 2^-53 (relative) of a tie of the following add, and after the rounding to f32 only where that in turn decides an
// f32 tie: no test input can be built to hit it, so THE FLAG IS THE GUARD, not a test. Do not remove it.
//
// Arithmetic, per element (the stored value is byte-swapped first when the file has the other endianness):
//   image, not scaled   stored type -> f32 in ONE conversion (i64 / u64 do not pass through f64: 2^60 + 2^36 + 1 is
//                       2^60 + 2^37 directly and 2^60 through f64); an f32 payload is copied bit for bit
//   image, scaled       f64(stored) -> * slope (rounded) -> + inter (rounded) -> f32 (round to nearest even)
//   labels              f64(stored), scaled or not, truncated toward zero; non-finite values and values whose truncation
//                       leaves [0, 256) are counted and written as 0 (the host wrapper raises on a non-zero count)
//
// Layout: for one y, a transpose of the (x) and (z, c) axes: out[(x * Y + y) * Z * C + zc] = in[((c * Z + z) * Y + y) * X + x],
// zc = z * C + c. One workgroup moves a 64 (x) by 64 (zc) tile: every wave reads 64 consecutive x of one (z, c) row, converts,
// and writes the f32 (or u8) into an LDS tile whose rows are padded by one dword; then every wave writes 64 consecutive zc of
// one x row. Banks (32 for ds_write_b32 / ds_read_b32, per 32-lane half): the write of lane l goes to dword r * 65 + l, the read
// of lane l to dword l * 65 + r -- both hit 32 different banks, so neither side conflicts. Edges: every load and store is
// guarded by x < X and zc < Z * C. Every index is 64-bit.
//
// The kernel is HBM-bound: (element width + 4) bytes per image element, (element width + 1) per label. A lane loads ONE
// element, so a wave's read is 64 to 512 bytes wide, its image write 256 bytes; sixteen loads per lane are in flight.
#include "common.h"
#include <type_traits>

namespace mpu {
namespace {

constexpr int VD_TILE = 64;
constexpr int VD_THREADS = 256;
constexpr int VD_ROWS = VD_THREADS / VD_TILE;      // tile rows moved per pass
constexpr int VD_PASSES = VD_TILE / VD_ROWS;

template <int W> struct Raw;
template <> struct Raw<1> { typedef uint8_t type; };
template <> struct Raw<2> { typedef uint16_t type; };
template <> struct Raw<4> { typedef uint32_t type; };
template <> struct Raw<8> { typedef uint64_t type; };

__device__ __forceinline__ uint8_t bswap(uint8_t v) { return v; }
__device__ __forceinline__ uint16_t bswap(uint16_t v) { return (uint16_t)((v << 8) | (v >> 8)); }
__device__ __forceinline__ uint32_t bswap(uint32_t v) { return __builtin_bswap32(v); }
__device__ __forceinline__ uint64_t bswap(uint64_t v) { return __builtin_bswap64(v); }

struct Scale { int scaled; double slope, inter; };

// the stored value as f64: exact for every type but i64 / u64, which round to nearest even (as NumPy's astype(float64))
template <typename T> __device__ __forceinline__ double scaled_f64(T v, const Scale& s) {
    double d = (double)v;
    if (s.scaled) {
        d = d * s.slope;
        d = d + s.inter;
    }
    return d;
}

template <typename T> __device__ __forceinline__ uint32_t image_word(T v, const Scale& s) {
    if (s.scaled) return __float_as_uint((float)scaled_f64(v, s));
    if constexpr (std::is_same<T, float>::value) return __builtin_bit_cast(uint32_t, v);             // f32: the bits
    else return __float_as_uint((float)v);
}

// labels: (value, 0) or (0, 1) when astype(uint8) is not defined for the value
template <typename T> __device__ __forceinline__ uint32_t label_word(T v, const Scale& s, unsigned& bad) {
    const double d = scaled_f64(v, s);
    if (d > -1.0 && d < 256.0) return (uint32_t)(int)d;          // (false for NaN)
    bad = 1u;
    return 0u;
}

template <typename T, bool LABELS>
__global__ __launch_bounds__(VD_THREADS) void decode_kernel(const void* __restrict__ payload, int swap, long X, long Y, long Z,
                                                            long C, Scale sc, void* __restrict__ out,
                                                            unsigned long long* __restrict__ bad_count, long tiles_x) {
    typedef typename Raw<sizeof(T)>::type R;
    __shared__ uint32_t tile[VD_TILE][VD_TILE + 1];
    const long ZC = Z * C;
    const long tx = (long)blockIdx.x % tiles_x, tz = (long)blockIdx.x / tiles_x;
    const long x0 = tx * VD_TILE, zc0 = tz * VD_TILE, y = blockIdx.y;
    const int lane = threadIdx.x % VD_TILE, row = threadIdx.x / VD_TILE;
    const R* __restrict__ in = (const R*)payload;
    unsigned bad = 0u;

    R raw[VD_PASSES];
    const long x = x0 + lane;
#pragma unroll
    for (int p = 0; p < VD_PASSES; ++p) {                         // all loads first: sixteen in flight per lane
        const long zc = zc0 + p * VD_ROWS + row;
        raw[p] = 0;
        if (x < X && zc < ZC) {
            const long z = zc / C, c = zc - z * C;
            raw[p] = in[((c * Z + z) * Y + y) * X + x];
        }
    }
#pragma unroll
    for (int p = 0; p < VD_PASSES; ++p) {
        const R r = swap ? bswap(raw[p]) : raw[p];
        const T v = __builtin_bit_cast(T, r);
        uint32_t w;
        if constexpr (LABELS) {
            const long zc = zc0 + p * VD_ROWS + row;
            unsigned b = 0u;
            w = label_word(v, sc, b);
            if (x < X && zc < ZC) bad |= b;
        } else {
            w = image_word(v, sc);
        }
        tile[p * VD_ROWS + row][lane] = w;
    }
    __syncthreads();
    const long zc = zc0 + lane;
#pragma unroll
    for (int p = 0; p < VD_PASSES; ++p) {
        const int xr = p * VD_ROWS + row;
        const long xo = x0 + xr;
        if (xo < X && zc < ZC) {
            const uint32_t w = tile[lane][xr];
            const long o = (xo * Y + y) * ZC + zc;
            if constexpr (LABELS) ((uint8_t*)out)[o] = (uint8_t)w;
            else ((uint32_t*)out)[o] = w;
        }
    }
    if constexpr (LABELS) {
        const unsigned long long m = __ballot(bad != 0u);
        if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(bad_count, (unsigned long long)__popcll(m));
    }
}

template <typename T>
int launch(const void* payload, int swap, const int64_t* s, const Scale& sc, int kind, void* out,
           unsigned long long* bad, hipStream_t st) {
    const long tiles_x = (s[0] + VD_TILE - 1) / VD_TILE, tiles_zc = (s[2] * s[3] + VD_TILE - 1) / VD_TILE;
    const dim3 grid((unsigned)(tiles_x * tiles_zc), (unsigned)s[1]);
    if (kind == MPU_DECODE_LABELS)
        hipLaunchKernelGGL((decode_kernel<T, true>), grid, dim3(VD_THREADS), 0, st, payload, swap, (long)s[0], (long)s[1],
                           (long)s[2], (long)s[3], sc, out, bad, tiles_x);
    else
        hipLaunchKernelGGL((decode_kernel<T, false>), grid, dim3(VD_THREADS), 0, st, payload, swap, (long)s[0], (long)s[1],
                           (long)s[2], (long)s[3], sc, out, bad, tiles_x);
    return launch_ok();
}

}  // namespace
}  // namespace mpu

using namespace mpu;

extern "C" {

int mpu_volume_decode(const void* d_payload, int32_t datatype, int32_t byteswap, const int64_t shape[4],
                      int32_t scaled, double slope, double inter, int32_t kind, void* d_out,
                      uint64_t* d_bad_count, void* stream) {
    MPU_REQUIRE(d_payload && shape && d_out, "mpu_volume_decode: null argument");
    MPU_REQUIRE(kind == MPU_DECODE_IMAGE || kind == MPU_DECODE_LABELS, "mpu_volume_decode: kind must be MPU_DECODE_IMAGE or MPU_DECODE_LABELS");
    MPU_REQUIRE(kind == MPU_DECODE_IMAGE || d_bad_count, "mpu_volume_decode: labels need a device counter");
    for (int k = 0; k < 4; ++k)
        MPU_REQUIRE(shape[k] >= 1 && shape[k] <= 32767, "mpu_volume_decode: every dimension must be in [1, 32767] (NIfTI-1 dim is int16)");
    const long tiles = ((shape[0] + VD_TILE - 1) / VD_TILE) * ((shape[2] * shape[3] + VD_TILE - 1) / VD_TILE);
    MPU_REQUIRE(tiles <= 0x7fffffffL, "mpu_volume_decode: volume too large (more than 2^31 - 1 tiles per y)");
    int width = 0;
    switch (datatype) {
        case 2: case 256: width = 1; break;
        case 4: case 512: width = 2; break;
        case 8: case 768: case 16: width = 4; break;
        case 64: case 1024: case 1280: width = 8; break;
        default: return fail(MPU_EUNSUPPORTED, "mpu_volume_decode: %sunsupported NIfTI datatype code %ld", "", (long)datatype);
    }
    MPU_REQUIRE(((uintptr_t)d_payload % (uintptr_t)width) == 0 && ((uintptr_t)d_out % 4) == 0 &&
                (!d_bad_count || ((uintptr_t)d_bad_count % 8) == 0),
                "mpu_volume_decode: payload must be aligned to its element width, the output to 4 and the counter to 8 bytes");
    hipStream_t st = (hipStream_t)stream;
    Scale sc;
    sc.scaled = scaled ? 1 : 0;
    sc.slope = slope;
    sc.inter = inter;
    unsigned long long* bad = (unsigned long long*)d_bad_count;
    if (kind == MPU_DECODE_LABELS) MPU_CHECK_HIP(hipMemsetAsync(bad, 0, 8, st));
    switch (datatype) {
        case 2: return launch<uint8_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 256: return launch<int8_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 4: return launch<int16_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 512: return launch<uint16_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 8: return launch<int32_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 768: return launch<uint32_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 16: return launch<float>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 64: return launch<double>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        case 1024: return launch<int64_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
        default: return launch<uint64_t>(d_payload, byteswap, shape, sc, kind, d_out, bad, st);
    }
}

}  // extern "C"
