// TEST INFRASTRUCTURE: csrc/fc_first.h compiled for the HOST (tests/test_fc_first_host.py builds and runs this program).  Not part of
// librnf_hip.so.
//
// For random fc_first rows (W_i0, W_i1, W_i2, b_i) and conditioning columns y the program builds the A and B operands of BOTH lane halves
// exactly as Mlp<1>::first_tile_h does -- lane (i, 0) from the float2 (W_i0, W_i2), lane (i, 1) from (W_i1, b_i); lane (n, 0) from
// (y0, y2), lane (n, 1) from (y1, 1) -- forms the 16-term sum over k = 8 h + j in fp32, as one v_mfma_f32_32x32x16_f16 does, and compares
// it with the fp64 product  W_i . y + b_i.
//
//   usage: host_fc_first SEED COUNT MODE SCALE      prints one JSON line; exit status 1 when a case misses its bound
//
// The bound, relative to  m = sum_k |W_ik y_k| + |b_i|:  2^-21.
//   x = hi + lo + e with |lo| <= 2^-11 |x| and |e| <= 2^-11 |lo| <= 2^-22 |x| (two roundings to 11 significant bits), so each product keeps
//   W y - (Whi yhi + Whi ylo + Wlo yhi) = Wlo ylo + e_W y + W e_y: 2^-22 |W y| each, with independent signs; the bias keeps 2^-22 |b|; the
//   fp32 sum of the terms adds a few 2^-24 m.
//   That derivation takes `lo` to be a normal fp16 number.  Below 2^-14 it is a subnormal (spacing 2^-24: flow_kernels.h, "22 significant
//   bits above 2^-2"), so a value below 2^-3 keeps an ABSOLUTE residual of up to 2^-25 instead, whatever its size.
//   MODE band:   |W_ik|, |b_i| log-uniform in [2^-3, 2^3] x SCALE with random signs -- the domain of the derivation; gate 2^-21 m.
//   MODE normal: W_ik, b_i = SCALE x N(0, 1), small values included; gate 2^-21 m + 2^-25 (sum_k (|W_ik| + |y_k|) + 1), the same bound
//                with the subnormal floor of each of the seven split values written out (e_W |y| + |W| e_y per product, e_b).
//   y is uniform on the unit sphere in both.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../rotationnormflow_amd/csrc/fc_first.h"

using namespace rnf;

static uint64_t g_state;
static double uniform01() {                       // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 9007199254740992.0;
}
static double normal() { return std::sqrt(-2.0 * std::log(uniform01())) * std::cos(6.283185307179586 * uniform01()); }

// the fp32 accumulate of one matrix step over both lane halves: sum over h, j of A(i, h)[j] * B(n, h)[j]
static float mfma_sum(const fcf_h8 (&a)[2], const fcf_h8 (&b)[2]) {
    float acc = 0.f;
    for (int h = 0; h < 2; ++h)
        for (int j = 0; j < 8; ++j) acc += (float)a[h][j] * (float)b[h][j];          // fp16 x fp16 is exact in fp32
    return acc;
}

int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s SEED COUNT band|normal SCALE\n", argv[0]); return 2; }
    g_state = std::strtoull(argv[1], nullptr, 10);
    const long count = std::strtol(argv[2], nullptr, 10);
    const bool band = argv[3][0] == 'b';
    const float scale = (float)std::atof(argv[4]);
    const float m1 = -1.0f;
    const double bound = std::ldexp(1.0, -21), floor25 = std::ldexp(1.0, -25);
    auto draw = [&]() { return band ? (float)((uniform01() < 0.5 ? -1.0 : 1.0) * std::exp2(6.0 * uniform01() - 3.0)) : (float)normal(); };
    double worst = 0.0, worst_gate = 0.0, sum = 0.0;
    long over = 0, nonfinite = 0;
    for (long c = 0; c < count; ++c) {
        float W[3], y[3];
        double yy[3], nrm = 0.0;
        for (int k = 0; k < 3; ++k) { W[k] = scale * draw(); yy[k] = normal(); nrm += yy[k] * yy[k]; }
        for (int k = 0; k < 3; ++k) y[k] = (float)(yy[k] / std::sqrt(nrm));
        const float b = scale * draw();
        const fcf_h8 A[2] = {fc_first_operand<false>(W[0], W[2], m1), fc_first_operand<false>(W[1], b, m1)};
        const fcf_h8 B[2] = {fc_first_operand<true>(y[0], y[2], m1), fc_first_operand<true>(y[1], 1.0f, m1)};
        const float got = mfma_sum(A, B);
        double want = b, mag = std::fabs((double)b);
        for (int k = 0; k < 3; ++k) { want += (double)W[k] * (double)y[k]; mag += std::fabs((double)W[k] * (double)y[k]); }
        double gate = bound * mag;
        if (!band) gate += floor25 * (std::fabs(W[0]) + std::fabs(W[1]) + std::fabs(W[2]) + std::fabs(y[0]) + std::fabs(y[1]) + std::fabs(y[2]) + 1.0);
        const double err = std::fabs((double)got - want), rel = err / mag;
        if (!std::isfinite(rel)) { ++nonfinite; continue; }
        sum += rel;
        if (err / gate > worst_gate) worst_gate = err / gate;
        if (rel > worst) worst = rel;
        if (err > gate) ++over;
    }
    // the pad slots are zero, 1 splits into (1, 0), and a value beyond the fp16 range poisons the product
    const fcf_h8 one = fc_first_operand<true>(0.25f, 1.0f, m1), big = fc_first_operand<false>(7.0e4f, 1.0f, m1);
    const bool shape_ok = (float)one[6] == 0.f && (float)one[7] == 0.f && (float)one[1] == 1.f && (float)one[3] == 0.f && (float)one[5] == 1.f &&
                          (float)one[0] == 0.25f && (float)one[2] == 0.f && (float)one[4] == 0.25f;
    const fcf_h8 Ab[2] = {big, big}, Bb[2] = {one, one};
    const bool range_ok = std::isinf((float)big[0]) && std::isnan(mfma_sum(Ab, Bb));
    std::printf("{\"count\": %ld, \"scale\": %g, \"max_rel\": %.6g, \"mean_rel\": %.6g, \"max_err_over_gate\": %.6g, \"bound\": %.6g, \"over\": %ld, \"nonfinite\": %ld, "
                "\"shape_ok\": %d, \"range_ok\": %d}\n", count, (double)scale, worst, sum / (double)(count > 0 ? count : 1), worst_gate, bound, over,
                nonfinite, (int)shape_ok, (int)range_ok);
    return (over == 0 && nonfinite == 0 && shape_ok && range_ok) ? 0 : 1;
}
