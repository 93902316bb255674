// fc_first.h -- the operands of fc_first (K = 3 + bias) as ONE split-fp16 matrix step (lean forward split-precision kernels).
//
// The exact form runs fc_first as two v_mfma_f32_32x32x2_f32 steps: lane (i, h) of the A side holds the float2 (W_i0, W_i2) for h = 0
// and (W_i1, b_i) for h = 1 (layout.h MOB_FIRST), lane (n, h) of the B side holds (y0, y2) and (y1, 1).  So every lane already owns one
// pair (p, q) of each side whose products p_A p_B + q_A q_B are its half's share of row i x sample n.  One v_mfma_f32_32x32x16_f16 gives
// every lane half eight k slots; six of them carry the three split terms of the lane's own two products, with
//     x = hi + lo,   hi = fp16(x) (RN),   lo = fp16(x - hi)                                            (split_pair without the ReLU)
//
//     slot j of a lane      0        1        2        3        4        5       6  7
//     A side (p, q)        p_hi     q_hi     p_hi     q_hi     p_lo     q_lo     0  0
//     B side (p, q)        p_hi     q_hi     p_lo     q_lo     p_hi     q_hi     0  0
//
// summed over both halves:  Whi.yhi + bhi + Whi.ylo + Wlo.yhi + blo  (1 = 1 + 0 exactly; Alo.Blo dropped, as in the 64-wide GEMMs), one
// fp32 accumulate.  No lane needs a value of its partner half, so no cross-lane instruction is spent, and each operand is one packed
// conversion and two mixed-precision FMAs: registers {P, P', L, 0} with P = (p_hi, q_hi), L = (p_lo, q_lo).
// A value beyond the fp16 range splits into (inf, -inf) and turns the product into NaN; a NaN stays a NaN.
#pragma once
#include <hip/hip_runtime.h>

namespace rnf {

typedef _Float16 fcf_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 fcf_h2 __attribute__((ext_vector_type(2)));
typedef float fcf_f2 __attribute__((ext_vector_type(2)));

// m1 = -1.0f, handed in so that the device caller can hide it from the optimiser (flow_kernels.h split_act: fma(m1, hi, v) then stays one
// v_fma_mixlo/mixhi_f16 that reads the fp16 `hi` directly).  v - hi is exact in fp32.
template <bool B_SIDE>
__host__ __device__ __forceinline__ fcf_h8 fc_first_operand(float p, float q, float m1) {
    const fcf_f2 v = {p, q};
    const fcf_h2 hi = __builtin_convertvector(v, fcf_h2);                       // v_cvt_pk_f16_f32 (RN)
    const fcf_h2 lo = {(_Float16)__builtin_fmaf(m1, (float)hi[0], p), (_Float16)__builtin_fmaf(m1, (float)hi[1], q)};
    const _Float16 z = (_Float16)0.0f;
    if (B_SIDE) return fcf_h8{hi[0], hi[1], lo[0], lo[1], hi[0], hi[1], z, z};
    return fcf_h8{hi[0], hi[1], hi[0], hi[1], lo[0], lo[1], z, z};
}

}  // namespace rnf
