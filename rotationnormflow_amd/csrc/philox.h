// philox.h -- the counter-based Philox4x32-10 stream of the samplers (sampler_kernel.h, grid_sample.h): a pure function of (key, counter),
// so a draw's numbers depend on its own indices alone and never on the launch that makes it.  Host and device: the host builds of the
// tests run the very same rounds.
#pragma once
#include <hip/hip_runtime.h>

namespace rnf {

struct Philox {
    unsigned k0, k1;
    __host__ __device__ __forceinline__ void round(unsigned (&c)[4], unsigned a, unsigned b) const {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ a, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ b, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    __host__ __device__ __forceinline__ void operator()(unsigned (&c)[4]) const {
        unsigned a = k0, b = k1;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            round(c, a, b);
            a += 0x9E3779B9u;
            b += 0xBB67AE85u;
        }
    }
};

}  // namespace rnf
