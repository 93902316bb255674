// fisher_exact.h -- the exact log-normaliser of the matrix-Fisher density, its derivative (the mean rotation) and the entropy.
//
// With the proper singular values s0 >= s1 >= |s2| of A (fisher_math.h proper_svd3) and the Haar PROBABILITY measure on SO(3):
//     c(A)   = s0 + s1 + s2 + log F,     F = int_{-1}^{1} f(u) du,     f = 1/2 i0e(a) i0e(b) exp(-(s1 + s2)(1 - u)),
//     a      = 1/2 (s0 - s1)(1 - u) >= 0,   b = 1/2 (s0 + s1)(1 + u) >= 0,   i0e(x) = exp(-x) I0(x),
//     dc/dA  = U diag(m) V^T = E[R],     m0, m1 = (+-P + Q) / (2 F),  m2 = int u f / F,
//     P = int (1 - u) 1/2 i1e(a) i0e(b) e,   Q = int (1 + u) 1/2 i0e(a) i1e(b) e          (I0' = I1),
//     H      = c - tr(A^T E[R]) = log F + int 1/2 e [a (i0e(a) - i1e(a)) i0e(b) + b (i0e(b) - i1e(b)) i0e(a) + (s1 + s2)(1 - u) i0e(a) i0e(b)] / F
// (the entropy in a form without the cancellation of c against tr(A^T E[R]), both ~ |s|).  0 < f <= 1/2 for every A, so nothing here
// overflows, and unlike the Laplace form (norm_type 1) c is smooth where singular values repeat or cancel (A = 0: c = 0, E[R] = 0).
//
// Quadrature: a FIXED rule of 224 nodes -- 16-point Gauss-Legendre on 14 panels of [-1, 1] with edges at 0 and +-(1 - 10^-k), k = 1..6:
// an anisotropic A puts boundary layers of width ~1/(s0 +- s1), 1/(s1 + s2) at u = +-1.  No adaptive step and no iteration: the work per
// matrix is constant, NaN / Inf in A come out as NaN.  The nodes are dealt to 64 lanes (node j to lane j % 64, each lane adding its nodes
// in increasing j) and the lanes are combined by the xor butterfly 32, 16, .. 1: the device kernel (one wave per matrix) and the host
// build add in this one order, so a matrix' result does not depend on the batch around it.
// Tables: tools/gen_fisher_exact_tables.py (mpmath, 40 digits).  Plain double arithmetic, host + device.
#pragma once
#include "fisher_math.h"

namespace rnf {

constexpr int kFisherExactNodes = 224, kFisherExactLanes = 64;
constexpr double kBesselSplit = 8.0;          // |x| <= 8: Taylor series in x^2/4; above: Chebyshev series in 16/x - 1

// exp(-|x|) I0(x) and exp(-|x|) I1(x), relative error ~1e-16 for every finite x (1e-12 is tested), 0 at x = +-inf.  The unscaled functions
// overflow at x ~ 713; these never do.
RNF_FM_HD void bessel_i01e(double x, double &i0, double &i1) {
    const double ax = fabs(x);
    if (ax <= kBesselSplit) {
        constexpr double c0[25] = {
            1.0, 1.0, 2.5e-1, 2.7777777777777778e-2, 1.7361111111111111e-3, 6.9444444444444444e-5,
            1.9290123456790123e-6, 3.9367598891408415e-8, 6.1511873267825649e-10, 7.5940584281266233e-12, 7.5940584281266233e-14, 6.2760813455591928e-16,
            4.358389823304995e-18, 2.5789288895295828e-20, 1.3157800456783586e-22, 5.8479113141260382e-25, 2.2843403570804837e-27, 7.9042918930120542e-30,
            2.4395962632753254e-32, 6.7578843858042254e-35, 1.6894710964510564e-37, 3.8310002187098784e-40, 7.9152897080782611e-43, 1.4962740468957015e-45,
            2.5976979980828151e-48};
        constexpr double c1[25] = {
            1.0, 5.0e-1, 8.3333333333333333e-2, 6.9444444444444444e-3, 3.4722222222222222e-4, 1.1574074074074074e-5,
            2.7557319223985891e-7, 4.9209498614260519e-9, 6.834652585313961e-11, 7.5940584281266233e-13, 6.9036894801151121e-15, 5.230067787965994e-17,
            3.3526075563884577e-19, 1.842092063949702e-21, 8.7718669711890573e-24, 3.6549445713287739e-26, 1.3437296218120492e-28, 4.3912732738955857e-31,
            1.2839980333028028e-33, 3.3789421929021127e-36, 8.0451004592907446e-39, 1.7413637357772174e-41, 3.4414303078601135e-44, 6.2344751953987564e-47,
            1.0390791992331261e-49};
        const double t = 0.25 * ax * ax;
        double p0 = c0[24], p1 = c1[24];
#pragma unroll 4
        for (int k = 23; k >= 0; --k) {
            p0 = p0 * t + c0[k];
            p1 = p1 * t + c1[k];
        }
        const double e = exp(-ax);
        i0 = e * p0;
        i1 = e * (0.5 * x) * p1;
    } else {
        constexpr double c0[27] = {
            4.0224520550705442e-1, 3.3691164782556941e-3, 6.889758346916824e-5, 2.8913705208347565e-6, 2.0489185894690637e-7, 2.2666689904981781e-8,
            3.3962320257083863e-9, 4.9406023882249696e-10, 1.1889147107846438e-11, -3.1499165279632414e-11, -1.3215811840447713e-11, -1.7941785315068061e-12,
            7.1801244513836662e-13, 3.8527783827421427e-13, 1.5400862175214098e-14, -4.1505693472872221e-14, -9.5548466988283076e-15, 3.8116806693526224e-15,
            1.7725601330565264e-15, -3.4254856196772191e-16, -2.8276239805165835e-16, 3.461222867697461e-17, 4.46562142029676e-17, -4.8305044859441783e-18,
            -7.2331804878747598e-18, 9.9214754121736755e-19, 1.1936508908460062e-18};
        constexpr double c1[27] = {
            3.8928811750914006e-1, -9.7610974913614684e-3, -1.1058893876262372e-4, -3.8825648088776904e-6, -2.5122362378702089e-7, -2.6314688468895195e-8,
            -3.835380385964237e-9, -5.5897434621965838e-10, -1.8974958123505412e-11, 3.2526035830154882e-11, 1.4125807436613781e-11, 2.0356285441470895e-12,
            -7.1985517762459085e-13, -4.0835511110921973e-13, -2.1015418427726643e-14, 4.2724400167119514e-14, 1.0420276984128803e-14, -3.8144030724370078e-15,
            -1.8803547755107824e-15, 3.3082023109209283e-16, 2.9626289976459501e-16, -3.2095259219934239e-17, -4.6503053684893583e-17, 4.4143483230717041e-18,
            7.5172963108421108e-18, -9.3141788673268624e-19, -1.2421932751949153e-18};
        const double w2 = 2.0 * (16.0 / ax - 1.0);                     // Clenshaw: b_k = c_k + 2 w b_{k+1} - b_{k+2}
        double p0 = 0.0, q0 = 0.0, p1 = 0.0, q1 = 0.0;
#pragma unroll 2
        for (int k = 26; k >= 1; --k) {
            const double n0 = c0[k] + w2 * p0 - q0, n1 = c1[k] + w2 * p1 - q1;
            q0 = p0; p0 = n0;
            q1 = p1; p1 = n1;
        }
        const double r = 1.0 / sqrt(ax);
        i0 = r * (c0[0] + 0.5 * w2 * p0 - q0);
        i1 = (x < 0.0 ? -r : r) * (c1[0] + 0.5 * w2 * p1 - q1);
    }
}
RNF_FM_HD double bessel_i0e(double x) { double i0, i1; bessel_i01e(x, i0, i1); return i0; }
RNF_FM_HD double bessel_i1e(double x) { double i0, i1; bessel_i01e(x, i0, i1); return i1; }

// node j of the rule: om = 1 - u, op = 1 + u (the one next to its end of [-1, 1] is built from the panel edge, never by 1 -+ u) and the weight
RNF_FM_HD void fisher_exact_node(int j, double &om, double &op, double &w) {
    constexpr double H[16] = {
            5.2995325041750337e-3, 2.7712488463383712e-2, 6.7184398806084128e-2, 1.2229779582249848e-1, 1.9106187779867813e-1, 2.7099161117138631e-1,
            3.5919822461037054e-1, 4.5249374508118128e-1, 5.4750625491881872e-1, 6.4080177538962946e-1, 7.2900838882861369e-1, 8.0893812220132187e-1,
            8.7770220417750152e-1, 9.3281560119391587e-1, 9.7228751153661629e-1, 9.9470046749582497e-1};                 // (1 + x_i) / 2 of the 16-point Gauss-Legendre rule
    constexpr double W[16] = {
            1.3576229705877047e-2, 3.1126761969323946e-2, 4.7579255841246392e-2, 6.2314485627766936e-2, 7.4797994408288366e-2, 8.4578259697501269e-2,
            9.1301707522461794e-2, 9.4725305227534248e-2, 9.4725305227534248e-2, 9.1301707522461794e-2, 8.4578259697501269e-2, 7.4797994408288366e-2,
            6.2314485627766936e-2, 4.7579255841246392e-2, 3.1126761969323946e-2, 1.3576229705877047e-2};                 // w_i / 2
    constexpr double D[8] = {0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0};      // panel edges as distances from the end
    const int p = j >> 4, i = j & 15;
    const bool right = p >= 7;
    const int q = right ? 13 - p : p, k = right ? 15 - i : i;
    const double len = D[q + 1] - D[q];
    const double near = D[q] + len * H[k];
    w = len * W[k];
    om = right ? near : 2.0 - near;
    op = right ? 2.0 - near : near;
}

// the five integrals (F, P, Q, int u f, the entropy integrand), one lane's share: nodes lane, lane + 64, ..
RNF_FM_HD void fisher_exact_lane(const double s[3], int lane, double acc[5]) {
    const double ha = 0.5 * (s[0] - s[1]), hb = 0.5 * (s[0] + s[1]), t = s[1] + s[2];
    for (int k = 0; k < 5; ++k) acc[k] = 0.0;
#pragma unroll 1                            // one node at a time: unrolled, the four Bessel evaluations cost ~300 registers
    for (int j = lane; j < kFisherExactNodes; j += kFisherExactLanes) {
        double om, op, w, i0a, i1a, i0b, i1b;
        fisher_exact_node(j, om, op, w);
        const double a = ha * om, b = hb * op;
        bessel_i01e(a, i0a, i1a);
        bessel_i01e(b, i0b, i1b);
        const double e = 0.5 * w * exp(-t * om), f = e * i0a * i0b;
        acc[0] += f;
        acc[1] += e * om * i1a * i0b;
        acc[2] += e * op * i0a * i1b;
        acc[3] += 0.5 * (op - om) * f;
        acc[4] += e * (a * (i0a - i1a) * i0b + b * (i0b - i1b) * i0a) + t * om * f;
    }
}

// c, m = dc/ds = diag E[Q] and the entropy from the five sums over all nodes
RNF_FM_HD void fisher_exact_finish(const double s[3], const double acc[5], double &c, double m[3], double &entropy) {
    const double lf = log(acc[0]), inv = 1.0 / acc[0];
    c = s[0] + s[1] + s[2] + lf;
    m[0] = 0.5 * (acc[2] + acc[1]) * inv;
    m[1] = 0.5 * (acc[2] - acc[1]) * inv;
    m[2] = acc[3] * inv;
    entropy = lf + acc[4] * inv;
}

// dc/dA = U diag(m) V^T, row-major
RNF_FM_HD void fisher_exact_mean(const double U[9], const double m[3], const double V[9], double dc[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) dc[3 * i + j] = m[0] * U[3 * i] * V[3 * j] + m[1] * U[3 * i + 1] * V[3 * j + 1] + m[2] * U[3 * i + 2] * V[3 * j + 2];
}

// the whole evaluation from the proper singular values, in the order of the device kernel: 64 lane sums, then the xor butterfly
inline void fisher_exact_from_s(const double s[3], double &c, double m[3], double &entropy) {
    double v[kFisherExactLanes][5], n[kFisherExactLanes][5];
    for (int l = 0; l < kFisherExactLanes; ++l) fisher_exact_lane(s, l, v[l]);
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < kFisherExactLanes; ++l)
            for (int k = 0; k < 5; ++k) n[l][k] = v[l][k] + v[l ^ o][k];
        for (int l = 0; l < kFisherExactLanes; ++l)
            for (int k = 0; k < 5; ++k) v[l][k] = n[l][k];
    }
    fisher_exact_finish(s, v[0], c, m, entropy);
}

// c(A), dc/dA (optional) and the entropy (optional) of one matrix
inline double fisher_exact(const double a[9], double *dc, double *entropy) {
    double U[9], s[3], V[9], c, m[3], h;
    proper_svd3(a, U, s, V);
    fisher_exact_from_s(s, c, m, h);
    if (dc) fisher_exact_mean(U, m, V, dc);
    if (entropy) *entropy = h;
    return c;
}

}  // namespace rnf
