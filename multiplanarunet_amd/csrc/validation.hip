// Epoch-end validation counting (mpunet/callbacks/validation.py:115-125): argmax of the class scores fused with
// the per-class TP / relevant / selected counts. The counting body is class_counts.h (shared with train_metrics.hip).
#include "kernels.h"
#include "class_counts.h"

namespace mpu {
namespace {

template <int K>
__global__ __launch_bounds__(VC_THREADS) void validation_count_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ y,
                                                                      long n, unsigned long long* __restrict__ counts) {
    class_counts_add<K>(pred, y, n, counts);
}

template <int K>
int launch_vc(const float* pred, const uint8_t* y, long n, unsigned long long* counts, hipStream_t st) {
    validation_count_kernel<K><<<dim3(class_counts_grid(n)), dim3(VC_THREADS), 0, st>>>(pred, y, n, counts);
    return launch_ok();
}

}  // namespace
}  // namespace mpu

using namespace mpu;

extern "C" int mpu_validation_count(const float* d_pred, const uint8_t* d_y, int64_t n, int32_t n_classes,
                                    int64_t* d_counts, void* stream) {
    MPU_REQUIRE(d_pred && d_y && d_counts, "mpu_validation_count: null argument");
    MPU_REQUIRE(n >= 0 && n_classes >= 1 && n_classes <= VC_MAXK, "mpu_validation_count: need 1 <= n_classes <= 16");
    if (n == 0) return MPU_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* c = (unsigned long long*)d_counts;
    switch (n_classes) {
#define VC_CASE(KK) case KK: return launch_vc<KK>(d_pred, d_y, (long)n, c, st);
        VC_CASE(1) VC_CASE(2) VC_CASE(3) VC_CASE(4) VC_CASE(5) VC_CASE(6) VC_CASE(7) VC_CASE(8)
        VC_CASE(9) VC_CASE(10) VC_CASE(11) VC_CASE(12) VC_CASE(13) VC_CASE(14) VC_CASE(15) VC_CASE(16)
#undef VC_CASE
    }
    return fail(MPU_EINVAL, "%s", "mpu_validation_count: bad n_classes");
}
