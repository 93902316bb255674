// grid_mass.h -- the fixed-point masses of a grid image, W_i = rint(expf(lp_i - m) * 2^S): the one definition grid_credible.h's histograms
// and grid_sample.h's prefix sums and draws share, so that their integer sums agree with each other.  No kernels here: the host builds
// of the tests include it (their expf is the host's, within an ulp of the device's).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rnf {
namespace gc {

typedef unsigned long long u64;

// S = 62 - ceil(log2 Q): Q * 2^S <= 2^62, so T = sum W_i <= Q * 2^S cannot overflow (W_i <= 2^S because expf(lp_i - m) <= 1)
inline int fixed_point_shift(long long Q) {
    int c = 0;
    while ((1LL << c) < Q) ++c;
    return 62 - c;
}

// the image has no set to report: a NaN or +inf maximum, or no finite value at all
__host__ __device__ __forceinline__ bool no_sets(float m) { return !(fabsf(m) < INFINITY); }

__host__ __device__ __forceinline__ u64 fixed_mass(float lp, float m, double scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (u64)__double2ull_rn((double)expf(lp - m) * scale);
#else
    return (u64)rint((double)expf(lp - m) * scale);       // the same rounding (to nearest, ties to even) on the host
#endif
}

}  // namespace gc
}  // namespace rnf
