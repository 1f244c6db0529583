// Resident volume -> NIfTI-1 payload: the inverse of volume_decode.hip, and what nifti.write_nifti does with NumPy on the host
// (np.asfortranarray(data).tobytes(order="F")), done on the device so that `mp predict` fetches the bytes of the file.
//
//   mpu_volume_encode   in  [X][Y][Z][C] (C order) f32, or u8 / i32 / i64 class indices
//                       -> payload [C][Z][Y][X] (Fortran order: x fastest), little endian, datatype 16 (f32) or 2 (u8):
//                       out[((c * Z + z) * Y + y) * X + x] = convert(in[((x * Y + y) * Z + z) * C + c])
//
// Conversion: f32 -> f32 copies the bits (NaN payloads included). A class index outside [0, 256) is written as 0 and counted in
// *bad_count (one count per ELEMENT; the call zeroes the counter first); u8 -> u8 can count nothing.
//
// Layout: for one y, a transpose of the (x) and (zc = z * C + c) axes. One workgroup moves a 64 (x) by 64 (zc) tile through LDS,
// one dword per element: the load phase walks rows of x with its lanes along zc (contiguous in the source), the store phase
// walks rows of zc with its lanes along x (contiguous in the file). A lane moves FOUR elements per global access where the
// alignment allows, one otherwise:
//   load  scalar   64 lanes along zc, one element each                                   (any shape)
//         quad     16 lanes along zc, one 16-byte (i64: 32-byte) vector of four each     (Z * C % 4 == 0, source 16-byte aligned)
//         bytes    u8 source, 16 lanes along zc: an aligned dword of four labels each; the up to three bytes in front of the
//                  first aligned dword of the row segment and the up to three behind the last are loaded as bytes
//   store scalar   64 lanes along x, one dword each                                      (any shape)
//         quad     16 lanes along x, one 16-byte vector each                             (X % 4 == 0, payload 16-byte aligned)
//         bytes    u8 payload, 16 lanes along x: an aligned dword of four packed labels each, head and tail as bytes. A file
//                  row starts at byte ((c * Z + z) * Y + y) * X: with an odd X the head differs from row to row.
// No two lanes, and no two workgroups, store to the same byte, and nothing outside the payload is stored to.
//
// LDS: element (zc, x) of the tile lives at dword  zc * 69 + x + 2 * (x >> 5) + 2 * (zc >> 5).  ds_write_b32 / ds_read_b32 bank
// a dword address modulo 32 within each 32-lane half. With lanes (q = 0..15, two neighbouring rows per half):
//   quad load   writes (zc = 4q + k, x in {e, e + 1}):  69 * 4q = 20q (mod 32) takes the 8 multiples of 4 for q < 8 and again for
//               q >= 8, where 2 * (zc >> 5) adds 2; x adds 0 / 1: 32 different banks.
//   quad store  reads (zc in {r, r + 1}, x = 4q + j):   4q + 2 * (x >> 5) is {0, 4 .. 28} for q < 8 and {2, 6 .. 30} for q >= 8; the
//               second row adds 69 = 5 (mod 32), i.e. the odd banks: 32 different banks.
//   scalar      load: lane l writes (zc = l, x): 69 l = 5 l (mod 32) over 32 consecutive l, all different (the zc >> 5 term is the
//               same for a half); store: lane l reads (zc, x = l): 32 consecutive dwords.
//   bytes       as quad when every row segment starts on a dword; rows with different heads can meet 2-way.
// Every index is 64-bit; zc (< 2^30) is divided by C in 32 bits.
//
// The kernel is HBM-bound: (source width + target width) bytes per element.
#include "common.h"
#include <type_traits>

namespace mpu {
namespace {

constexpr int VE_TILE = 64;
constexpr int VE_THREADS = 256;
constexpr int VE_PITCH = 69;
constexpr int VE_LDS = VE_TILE * VE_PITCH + 8;

enum { VE_SCALAR = 0, VE_QUAD = 1, VE_BYTES = 2 };

__device__ __forceinline__ int tix(int zc, int x) { return zc * VE_PITCH + x + 2 * (x >> 5) + 2 * (zc >> 5); }

template <typename S> struct alignas(16) Vec4 { S v[4]; };

// the dword the tile holds for a source element; nbad counts the class indices a u8 cannot hold
template <typename S> __device__ __forceinline__ uint32_t word_of(S v, unsigned& nbad) {
    if constexpr (std::is_same<S, float>::value) return __builtin_bit_cast(uint32_t, v);
    else if constexpr (std::is_same<S, uint8_t>::value) return (uint32_t)v;
    else {
        typedef typename std::make_unsigned<S>::type U;
        if ((U)v < (U)256) return (uint32_t)v;
        ++nbad;
        return 0u;
    }
}

template <typename S, int MIN, int MOUT>
__global__ __launch_bounds__(VE_THREADS) void encode_kernel(const S* __restrict__ in, long X, long Y, long Z, long C,
                                                            void* __restrict__ out, unsigned long long* __restrict__ bad_count,
                                                            long tiles_x) {
    __shared__ uint32_t T[VE_LDS];
    const long ZC = Z * C;
    const long tx = (long)blockIdx.x % tiles_x, tz = (long)blockIdx.x / tiles_x;
    const long x0 = tx * VE_TILE, zc0 = tz * VE_TILE, y = blockIdx.y;
    const int nx = (int)(X - x0 < VE_TILE ? X - x0 : VE_TILE), nz = (int)(ZC - zc0 < VE_TILE ? ZC - zc0 : VE_TILE);
    const int tid = threadIdx.x;
    unsigned nbad = 0u;

    // ---- load: rows of x, lanes along zc --------------------------------------------------------------------------------------
    if constexpr (MIN == VE_SCALAR) {
        const int lane = tid % VE_TILE, row = tid / VE_TILE;
        constexpr int ROWS = VE_THREADS / VE_TILE, PASSES = VE_TILE / ROWS;
        S raw[PASSES];
        const S* __restrict__ src = in + ((x0 + row) * Y + y) * ZC + zc0 + lane;
        const long step = (long)ROWS * Y * ZC;                    // (one pass further: ROWS rows of x)
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {                        // all loads first: sixteen in flight per lane
            const int xl = p * ROWS + row;
            S v = S(0);
            if (xl < nx && lane < nz) v = src[p * step];
            raw[p] = v;
        }
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int xl = p * ROWS + row;
            if (xl < nx && lane < nz) T[tix(lane, xl)] = word_of(raw[p], nbad);
        }
    } else if constexpr (MIN == VE_QUAD) {
        const int q = tid % 16, row = tid / 16;
        constexpr int ROWS = VE_THREADS / 16, PASSES = VE_TILE / ROWS;
        Vec4<S> raw[PASSES];
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {                        // (Z * C % 4 == 0: a vector is inside the row or outside it)
            const int xl = p * ROWS + row;
            if (xl < nx && 4 * q < nz) raw[p] = *(const Vec4<S>*)(in + ((x0 + xl) * Y + y) * ZC + zc0 + 4 * q);
        }
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int xl = p * ROWS + row;
            if (xl < nx && 4 * q < nz) {
#pragma unroll
                for (int k = 0; k < 4; ++k) T[tix(4 * q + k, xl)] = word_of(raw[p].v[k], nbad);
            }
        }
    } else {
        static_assert(sizeof(S) == 1, "the byte path loads u8");
        const int q = tid % 16, row = tid / 16;
        constexpr int ROWS = VE_THREADS / 16, PASSES = VE_TILE / ROWS;
        uint32_t body[PASSES], head[PASSES];
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int xl = p * ROWS + row;
            body[p] = 0u;
            head[p] = 0u;
            if (xl < nx) {
                const uint8_t* a = (const uint8_t*)in + ((x0 + xl) * Y + y) * ZC + zc0;
                int h = (int)((0 - (uintptr_t)a) & 3);
                h = h < nz ? h : nz;
                const int off = h + 4 * q;
                if (off + 4 <= nz) {
                    body[p] = *(const uint32_t*)(a + off);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (off + k < nz) body[p] |= (uint32_t)a[off + k] << (8 * k);
                }
                if (q == 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (k < h) head[p] |= (uint32_t)a[k] << (8 * k);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int xl = p * ROWS + row;
            if (xl < nx) {
                const uint8_t* a = (const uint8_t*)in + ((x0 + xl) * Y + y) * ZC + zc0;
                int h = (int)((0 - (uintptr_t)a) & 3);
                h = h < nz ? h : nz;
                const int off = h + 4 * q;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (off + k < nz) T[tix(off + k, xl)] = (body[p] >> (8 * k)) & 0xffu;
                if (q == 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (k < h) T[tix(k, xl)] = (head[p] >> (8 * k)) & 0xffu;
                }
            }
        }
    }
    __syncthreads();

    // ---- store: rows of zc (file rows), lanes along x ---------------------------------------------------------------------------
    const unsigned Cu = (unsigned)C;
    if constexpr (MOUT == VE_SCALAR) {
        const int lane = tid % VE_TILE, row = tid / VE_TILE;
        constexpr int ROWS = VE_THREADS / VE_TILE, PASSES = VE_TILE / ROWS;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int zl = p * ROWS + row;
            if (zl < nz && lane < nx) {
                const unsigned zc = (unsigned)(zc0 + zl), z = zc / Cu, c = zc - z * Cu;
                ((uint32_t*)out)[(((long)c * Z + z) * Y + y) * X + x0 + lane] = T[tix(zl, lane)];
            }
        }
    } else if constexpr (MOUT == VE_QUAD) {
        const int q = tid % 16, row = tid / 16;
        constexpr int ROWS = VE_THREADS / 16, PASSES = VE_TILE / ROWS;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {                        // (X % 4 == 0: a vector is inside the row or outside it)
            const int zl = p * ROWS + row;
            if (zl < nz && 4 * q < nx) {
                const unsigned zc = (unsigned)(zc0 + zl), z = zc / Cu, c = zc - z * Cu;
                Vec4<uint32_t> w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w.v[j] = T[tix(zl, 4 * q + j)];
                *(Vec4<uint32_t>*)((uint32_t*)out + (((long)c * Z + z) * Y + y) * X + x0 + 4 * q) = w;
            }
        }
    } else {
        const int q = tid % 16, row = tid / 16;
        constexpr int ROWS = VE_THREADS / 16, PASSES = VE_TILE / ROWS;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int zl = p * ROWS + row;
            if (zl < nz) {
                const unsigned zc = (unsigned)(zc0 + zl), z = zc / Cu, c = zc - z * Cu;
                uint8_t* a = (uint8_t*)out + (((long)c * Z + z) * Y + y) * X + x0;     // first byte of this row's segment [0, nx)
                int h = (int)((0 - (uintptr_t)a) & 3);
                h = h < nx ? h : nx;
                const int off = h + 4 * q;
                if (off + 4 <= nx) {                              // an aligned dword of four labels
                    uint32_t w = 0u;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w |= (T[tix(zl, off + j)] & 0xffu) << (8 * j);
                    *(uint32_t*)(a + off) = w;
                } else {                                          // the tail: what is left of the segment behind the last dword
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        if (off + j < nx) a[off + j] = (uint8_t)T[tix(zl, off + j)];
                }
                if (q == 0) {                                     // the head: the bytes in front of the first aligned dword
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        if (j < h) a[j] = (uint8_t)T[tix(zl, j)];
                }
            }
        }
    }
    if constexpr (!std::is_same<S, float>::value && !std::is_same<S, uint8_t>::value) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o);
        if (nbad && __lane_id() == 0) atomicAdd(bad_count, (unsigned long long)nbad);
    }
}

template <typename S, int MIN, int MOUT>
int launch(const void* in, const int64_t* s, void* out, unsigned long long* bad, hipStream_t st) {
    const long tiles_x = (s[0] + VE_TILE - 1) / VE_TILE, tiles_zc = (s[2] * s[3] + VE_TILE - 1) / VE_TILE;
    const dim3 grid((unsigned)(tiles_x * tiles_zc), (unsigned)s[1]);
    hipLaunchKernelGGL((encode_kernel<S, MIN, MOUT>), grid, dim3(VE_THREADS), 0, st, (const S*)in, (long)s[0], (long)s[1],
                       (long)s[2], (long)s[3], out, bad, tiles_x);
    return launch_ok();
}

template <typename S>
int launch_labels(const void* in, const int64_t* s, bool quad_in, void* out, unsigned long long* bad, hipStream_t st) {
    return quad_in ? launch<S, VE_QUAD, VE_BYTES>(in, s, out, bad, st) : launch<S, VE_SCALAR, VE_BYTES>(in, s, out, bad, st);
}

}  // namespace
}  // namespace mpu

using namespace mpu;

extern "C" {

int mpu_volume_encode(const void* d_in, int32_t source, const int64_t shape[4], int32_t datatype, void* d_payload,
                      uint64_t* d_bad_count, void* stream) {
    MPU_REQUIRE(d_in && shape && d_payload, "mpu_volume_encode: null argument");
    for (int k = 0; k < 4; ++k)
        MPU_REQUIRE(shape[k] >= 1 && shape[k] <= 32767, "mpu_volume_encode: every dimension must be in [1, 32767] (NIfTI-1 dim is int16)");
    const long tiles = ((shape[0] + VE_TILE - 1) / VE_TILE) * ((shape[2] * shape[3] + VE_TILE - 1) / VE_TILE);
    MPU_REQUIRE(tiles <= 0x7fffffffL, "mpu_volume_encode: volume too large (more than 2^31 - 1 tiles per y)");
    int width = 0;
    switch (source) {
        case MPU_ENCODE_F32: width = 4; break;
        case MPU_ENCODE_U8: width = 1; break;
        case MPU_ENCODE_I32: width = 4; break;
        case MPU_ENCODE_I64: width = 8; break;
        default: return fail(MPU_EUNSUPPORTED, "mpu_volume_encode: %sunsupported source type %ld", "", (long)source);
    }
    const bool image = source == MPU_ENCODE_F32;
    if (datatype != (image ? 16 : 2))
        return fail(MPU_EUNSUPPORTED, "mpu_volume_encode: %sunsupported pair: source type %ld to NIfTI datatype %ld (f32 -> 16; u8, i32, i64 -> 2)",
                    "", (long)source, (long)datatype);
    MPU_REQUIRE(image || d_bad_count, "mpu_volume_encode: a label map needs a device counter");
    MPU_REQUIRE(((uintptr_t)d_in % (uintptr_t)width) == 0 && (!image || ((uintptr_t)d_payload % 4) == 0) &&
                (!d_bad_count || ((uintptr_t)d_bad_count % 8) == 0),
                "mpu_volume_encode: the source must be aligned to its element width, an f32 payload to 4 and the counter to 8 bytes");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* bad = (unsigned long long*)d_bad_count;
    if (!image) MPU_CHECK_HIP(hipMemsetAsync(bad, 0, 8, st));
    const bool quad_in = (shape[2] * shape[3]) % 4 == 0 && ((uintptr_t)d_in % 16) == 0;
    const bool quad_out = shape[0] % 4 == 0 && ((uintptr_t)d_payload % 16) == 0;
    switch (source) {
        case MPU_ENCODE_F32:
            if (quad_in) return quad_out ? launch<float, VE_QUAD, VE_QUAD>(d_in, shape, d_payload, bad, st)
                                         : launch<float, VE_QUAD, VE_SCALAR>(d_in, shape, d_payload, bad, st);
            return quad_out ? launch<float, VE_SCALAR, VE_QUAD>(d_in, shape, d_payload, bad, st)
                            : launch<float, VE_SCALAR, VE_SCALAR>(d_in, shape, d_payload, bad, st);
        case MPU_ENCODE_U8: return launch<uint8_t, VE_BYTES, VE_BYTES>(d_in, shape, d_payload, bad, st);
        case MPU_ENCODE_I32: return launch_labels<int32_t>(d_in, shape, quad_in, d_payload, bad, st);
        default: return launch_labels<int64_t>(d_in, shape, quad_in, d_payload, bad, st);
    }
}

}  // extern "C"
