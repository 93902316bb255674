// so3_grid_local.h -- neighbour-limited sums of isotropic matrix-Fisher kernels over the rows of the HEALPix SO(3) grid
// (rnf_so3_grid_local_sum, include/rnf_hip.h): the prediction step of a Bayes filter on the grid at the levels where the dense
// pairwise sum (so3_kernel_sum.h, Q^2 pairs) cannot run.
//
// With the grid rows G_j (so3_grid.h: row t * npix + p is Rx(phi_p) Rz(theta_p) Rx(tau_t) O), queries Q_i, one concentration kappa, a cut
// on the squared chordal distance d^2 = |G_j - Q_i|_F^2 = 4 (1 - cos omega) and rows of log-weights lw[g][j] (none: zeros),
//     out[g][i] = log sum_{j : d^2(G_j, Q_i) <= d2_cut} exp(lw[g][j]) k_kappa(G_j, Q_i),      count[i] = the number of such j,
// k_kappa the kernel of so3_kernel_sum.h (exponent from ks::dist2, l(kappa) from ks::log_normaliser).  The log-weights are NOT
// normalised here.
//
// Enumeration.  No search structure: with Q' = Q_i O^T and B = (Rx(phi_p) Rz(theta_p))^T Q',
//     d^2(tau) = |O|_F^2 + |Q_i|_F^2 - 2 (B00 + rho cos(tau - tau*)),   rho = hypot(B11 + B22, B21 - B12),  tau* = atan2(B21 - B12, B11 + B22),
// exactly, for any matrix Q_i (rho = 1 + B00 for a rotation).  A pixel can hold a neighbour only if its direction u_p = (z, s cos phi,
// s sin phi) lies within the spherical disc u_p . u >= 1 - d2_cut / 4 about u = Q' e_x.  A thread walks
//     the rings whose colatitude meets the disc (northern cap, belt and southern cap alike: ring_of),
//     on a ring the azimuth window cos(dphi) >= (cos omega - z z0) / (s s0) (the whole ring at <= -1, nothing at >= 1),
//     for a pixel the tilts with cos(tau - tau*) >= (|O|^2 + |Q|^2 - d2_cut - 2 B00) / (2 rho) (all tilts where rho < 0.01: the antipodal pixel).
// The windows are SUPERSETS: the disc is widened by one pixel spacing (1.1 / nside) plus the query's defect from a rotation
// (2 |Q'^T Q' - I|_F + |(|O|^2 + |Q|^2) - 6| / 4), the azimuth and tilt windows by one cell on either side, the distances by 1e-4.
// Membership is decided by the fp32 ks::dist2(G_j, Q_i) <= d2_cut on the stored rows alone (at d2_cut = 8 against CUT_ALL, so that 180
// degrees covers every row); dist2 is symmetric bit for bit, so neighbourhoods among grid rows are symmetric.  Rings, the pixels of a ring's window and the tilts of a pixel's window are visited in
// increasing index order -- a window that wraps is cut at index 0 -- and each at most once: a query's members come in the order of
// (ring, pixel, tilt) whatever the windows' margins, and every row is counted once.
//
// Arithmetic.  Base 2 as in so3_kernel_sum.h: t = fma(-h, d2, lw log2(e)), h = (kappa / 2) log2(e) in fp32.  Two sweeps over the same
// enumeration: the first takes M = max t (and the count), the second adds exp2(t - M) -- no term exceeds 1, the largest is exactly 1.
// The terms of one pixel's tilt run (at most 6 * 2^level) are added serially in fp32, the runs in fp64.  exp2 is exp2_soft, a
// degree-7 polynomial of fmaf and one ldexpf (relative error 5e-9 + one rounding), so that the host build below gives the device's
// bits.
//
// Shape: a thread owns ONE query; the enumeration state stays in registers; a row and its log-weights are loaded once and shared by up
// to GROUPS_PER_THREAD = 4 groups; further groups go across the launch grid.  No LDS, no barrier, no cross-lane traffic, no atomics, no
// workspace.  A query's result is a function of (level, offset, query, cut, kappa, its group's log-weights) alone: bit-identical from
// run to run, whatever m, G, the query's position in the call and the group's position are.
//
// Edge cases.  An empty neighbourhood, or one whose rows all have lw = -inf, gives -inf.  A row with lw = -inf drops out (it still
// counts).  A NaN log-weight inside a query's neighbourhood makes that output NaN.  A query with a non-finite entry gives NaN and
// count 0; a finite query with |Q|_F^2 > 25 is further than the largest cut from every rotation: -inf and count 0.  A grid row with a
// non-finite entry is at distance FLT_MAX: no member.
//
// The max-plus pass (rnf_so3_grid_local_max) is a third mode of the same sweep: over the same members, on the same fp32 term t,
//     out[g][i] = max_j (lw[g][j] - (kappa/2) d^2(G_j, Q_i)) - l(kappa) = (float)((double)M ln 2 - l(kappa)),     arg[g][i] = the smallest row with t == M.
// One sweep, no exp2.  The tie goes to the smallest ROW, compared explicitly: members arrive by (ring, pixel, tilt).  No live member
// (none, or all at -inf): -inf and -1; a NaN log-weight inside the neighbourhood (fmaxf would drop it: a flag carries it): NaN and -1;
// a non-finite query: NaN, -1, count 0.  The Viterbi recursion of grid_pose.grid_viterbi runs on it.
//
// The anisotropic variant (rnf_so3_grid_local_fisher; template parameter F of sweep, query_local and query_local_max, and
// so3_grid_local_fisher_kernel for both passes).  A general matrix-Fisher step x' = x E, E ~ MF(A), A = Delta K with the drift Delta = U V^T and the symmetric concentration
// K = V diag(s) V^T of the proper SVD, has for rotations Q, G with C = Q Delta and W = G - C
//     tr(A^T Q^T G) - (s1 + s2 + s3) = -1/2 tr(W K W^T) = -1/2 sum_r w_r K w_r^T        (w_r the rows of W),
// the difference form ks::dist2 gives the isotropic kernel (K = kappa I: -(kappa/2) |G - C|^2).  The drift needs nothing here: the
// caller passes the shifted rows C.  A member's term is  t = lw log2(e) - quad,  quad = sum_r w_r Kh w_r^T  on the SAME nine
// differences q[k] - c[k] the distance is taken from, Kh = (K / 2) log2(e) in fp32, six entries by value (Quad: the off-diagonal ones
// doubled), in a fixed order of fmaf under fp contract(off) (fisher_term).  Every product holds two differences, so the term of
// (query a, row b) is the term of (query b, row a) bit for bit.  Membership stays ks::dist2 <= cut; the enumeration, the sweep order,
// max-then-sum, the fp32 / fp64 split, exp2_soft, the tie rule and the edge cases are the isotropic pass's.  The log-normaliser is
// l(K) = c(K) - tr K with the exact c of fisher_exact.h, fp64 on the host (K = kappa I: ks::log_normaliser(kappa)).  The exponent is
// bounded by -(s2 + s3)/4 |G - C|^2 (equality for rotations about the loosest axis): the ball of the loosest axis is the neighbourhood.
#pragma once
#if defined(RNF_SGL_HOST_ONLY) && !defined(RNF_KS_HOST_ONLY)
#define RNF_KS_HOST_ONLY
#endif
#include "so3_kernel_sum.h"

namespace rnf {
namespace sgl {

constexpr int MAX_LEVEL = 6;                       // 72 * 8^6 = 18 874 368 rows: 9 * row stays below 2^31
constexpr int THREADS = 256, GROUPS_PER_THREAD = 4;
constexpr int MAX_G = 65535;
constexpr long long MAX_M = (1LL << 31) - 1;
constexpr double MAX_D2 = 8.0;
// d2_cut = 8 (180 degrees) covers EVERY row: the fp32 distance of two rows 180 degrees apart can round above 8 -- by at most twelve
// roundings, 6e-6 -- and a structured grid holds many such pairs, so the kernel compares against 8 (1 + 2.5e-6) there
constexpr float CUT_ALL = 8.00002f;
constexpr float TOL_D2 = 1e-4f;                    // slack on a distance of the enumeration: fp32 error of its closed forms is ~1e-5
constexpr float TWO_PI = 6.28318530717958647692f, INV_TWO_PI = 0.15915494309189533577f;

inline long long rows_of(int level) { return 72LL << (3 * level); }

struct Geometry {                                  // what (level, kappa, cut) fix; passed by value
    int nside, ntilt, npix, ncap;
    float cut, h, cell;                            // d2_cut; (kappa / 2) log2(e); the disc's widening, 1.1 / nside
};

inline Geometry geometry_of(int level, double kappa, double d2_cut) {
    Geometry ge;
    ge.nside = 1 << level;
    ge.ntilt = 6 * ge.nside;
    ge.npix = 12 * ge.nside * ge.nside;
    ge.ncap = 2 * ge.nside * (ge.nside - 1);
    ge.cut = d2_cut >= MAX_D2 ? CUT_ALL : (float)d2_cut;
    ge.h = (float)(0.5 * kappa * ks::LOG2E);
    ge.cell = 1.1f / (float)ge.nside;
    return ge;
}

// The anisotropic variant's (K / 2) log2(e) in fp32: k[0..2] the diagonal, k[3..5] TWICE the entries 01, 02, 12; passed by value
struct Quad { float k[6]; };

inline Quad quad_of(const double K[9]) {
    const double h = 0.5 * ks::LOG2E;
    Quad qd;
    qd.k[0] = (float)(h * K[0]);
    qd.k[1] = (float)(h * K[4]);
    qd.k[2] = (float)(h * K[8]);
    qd.k[3] = (float)(h * (K[1] + K[3]));          // the symmetric part: 2 * (K01 + K10) / 2
    qd.k[4] = (float)(h * (K[2] + K[6]));
    qd.k[5] = (float)(h * (K[5] + K[7]));
    return qd;
}

// The eigenvalues of the symmetric part of K by cyclic Jacobi in fp64, in decreasing order
inline void sym_eigenvalues3(const double K[9], double ev[3]) {
    double a[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i][j] = 0.5 * (K[3 * i + j] + K[3 * j + i]);
    for (int it = 0; it < 64; ++it) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (!(off > 1e-34 * diag)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {                                             // A <- A J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {                                             // A <- J^T A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
            }
    }
    ev[0] = a[0][0];
    ev[1] = a[1][1];
    ev[2] = a[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (ev[j] < ev[j + 1]) {
                const double t = ev[j];
                ev[j] = ev[j + 1];
                ev[j + 1] = t;
            }
}

constexpr double MAX_CONCENTRATION = 3e4;          // the largest |eigenvalue| of K: the range fisher_exact is tested on
constexpr double SYMMETRY_TOL = 1e-9;              // |K - K^T|_F and a negative pair sum of eigenvalues, relative to |K|_F

// What rnf_so3_grid_local_fisher refuses of a concentration: 0 fine, 1 non-finite, 2 not symmetric, 3 a negative pair sum of
// eigenvalues (not the symmetric factor of a proper SVD), 4 an eigenvalue beyond MAX_CONCENTRATION
inline int concentration_defect(const double K[9]) {
    double n2 = 0.0, a2 = 0.0;
    for (int k = 0; k < 9; ++k) {
        if (!(fabs(K[k]) < INFINITY)) return 1;
        n2 += K[k] * K[k];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a2 += (K[3 * i + j] - K[3 * j + i]) * (K[3 * i + j] - K[3 * j + i]);
    const double norm = sqrt(n2);
    if (!(n2 < INFINITY)) return 4;
    if (sqrt(a2) > SYMMETRY_TOL * norm) return 2;
    double ev[3];
    sym_eigenvalues3(K, ev);
    if (ev[1] + ev[2] < -SYMMETRY_TOL * norm) return 3;
    if (fmax(fabs(ev[0]), fabs(ev[2])) > MAX_CONCENTRATION) return 4;
    return 0;
}

// l(K) = c(K) - tr K with the exact log-normaliser c (fisher_exact.h, relative error 1e-10 of c), fp64 on the host; an exact
// K = kappa I takes ks::log_normaliser(kappa), the same number in closed form
inline double log_normaliser_fisher(const double K[9]) {
    double S[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[3 * i + j] = 0.5 * (K[3 * i + j] + K[3 * j + i]);
    double U[9], s[3], V[9], c, m[3], h;
    proper_svd3(S, U, s, V);
    if (s[0] == s[1] && s[1] == s[2]) return ks::log_normaliser(s[0]);                       // kappa I (0 included): the isotropic pass's own
    fisher_exact_from_s(s, c, m, h);
    return c - (s[0] + s[1] + s[2]);
}

// t = l2 - sum_r w_r Kh w_r^T on the rows w_r = (q - c)[3r..3r+2], the nine differences ks::dist2 takes (the same subtraction: the same
// bits): each row is w0 (k00 w0 + k01' w1 + k02' w2) + w1 (k11 w1 + k12' w2) +
// w2 (k22 w2), the rows added in order.  Negating every d leaves every rounding where it was: symmetric in (q, c) bit for bit.
RNF_FM_HD float fisher_term(const Quad &kq, const float *c, const float *q, float l2) {
#pragma clang fp contract(off)                     // the products and the difference below are not to be fused: the host build's bits
    float quad = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float w0 = q[3 * r] - c[3 * r], w1 = q[3 * r + 1] - c[3 * r + 1], w2 = q[3 * r + 2] - c[3 * r + 2];
        const float u0 = fmaf(kq.k[4], w2, fmaf(kq.k[3], w1, kq.k[0] * w0));
        const float u1 = fmaf(kq.k[5], w2, kq.k[1] * w1);
        const float u2 = kq.k[2] * w2;
        quad = fmaf(u0, w0, quad);
        quad = fmaf(u1, w1, quad);
        quad = fmaf(u2, w2, quad);
    }
    return l2 - quad;
}

// 2^x for x <= 0 (NaN: NaN; below -125: 0, so that no result is subnormal): the same bits on the host and on the device
RNF_FM_HD float exp2_soft(float x) {
    if (!(x >= -125.f)) return x != x ? x : 0.f;
    const float n = rintf(x), f = x - n;           // f in [-1/2, 1/2], exact
    float p = 1.5252733804059841e-5f;              // ln(2)^k / k!, k = 7 .. 1
    p = fmaf(p, f, 1.5403530393381608e-4f);
    p = fmaf(p, f, 1.3333558146428443e-3f);
    p = fmaf(p, f, 9.618129107628477e-3f);
    p = fmaf(p, f, 5.550410866482158e-2f);
    p = fmaf(p, f, 2.402265069591007e-1f);
    p = fmaf(p, f, 6.931471805599453e-1f);
    p = fmaf(p, f, 1.f);
    return ldexpf(p, (int)n);
}

// What a query fixes: Q' = Q O^T, its disc and the rings that meet it (ring_lo > ring_hi: no ring)
struct Frame {
    float qp[9];
    float z0, s0, phi0, cw, base;                  // u = (z0, s0 cos phi0, s0 sin phi0); cos of the widened disc; |O|^2 + |Q|^2 - cut - TOL_D2
    int ring_lo, ring_hi;
    bool finite;
};

// the continuous ring coordinate of colatitude theta: ring i has r = i
RNF_FM_HD float ring_coordinate(const Geometry &ge, float theta) {
    const float z = cosf(theta), ns = (float)ge.nside;
    if (z >= 2.f / 3.f) return ns * 2.4494897427831781f * sinf(0.5f * theta);               // z = 1 - r^2 / (3 nside^2)
    if (z > -2.f / 3.f) return ns * (2.f - 1.5f * z);
    return 4.f * ns - ns * 2.4494897427831781f * cosf(0.5f * theta);
}

RNF_FM_HD Frame frame_of(const Geometry &ge, const float *offset, const float q[9]) {
    Frame f;
    float o[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (offset) {
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = offset[k];
    }
    float no = 0.f, nq = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        no = fmaf(o[k], o[k], no);
        nq = fmaf(q[k], q[k], nq);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) f.qp[3 * r + c] = q[3 * r] * o[3 * c] + q[3 * r + 1] * o[3 * c + 1] + q[3 * r + 2] * o[3 * c + 2];
    f.finite = ks::finite9(q);
    f.base = no + nq - ge.cut - TOL_D2;
    f.z0 = 1.f;
    f.s0 = f.phi0 = 0.f;
    f.cw = -2.f;
    f.ring_lo = 1;
    f.ring_hi = 0;
    if (!f.finite || !(nq <= 25.f) || !(no <= 25.f)) return f;                               // nothing within sqrt(8) of such a query
    float defect = 0.f;                                                                     // |Q'^T Q' - I|_F^2
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float d = f.qp[a] * f.qp[b] + f.qp[3 + a] * f.qp[3 + b] + f.qp[6 + a] * f.qp[6 + b] - (a == b ? 1.f : 0.f);
            defect = fmaf(d, d, defect);
        }
    const float c = 1.f - 0.25f * ge.cut - 2.f * sqrtf(defect) - 0.25f * fabsf(no + nq - 6.f) - 1e-5f;
    const float uu = sqrtf(f.qp[0] * f.qp[0] + f.qp[3] * f.qp[3] + f.qp[6] * f.qp[6]);
    const int rings = 4 * ge.nside - 1;
    f.ring_hi = rings;                                                                      // from here on: every ring unless narrowed
    if (!(uu >= 0.5f) || c <= -1.f) return f;                                               // cw = -2: every ring whole
    const float omega = (c >= 1.f ? 0.f : acosf(c)) + ge.cell;
    if (omega >= 3.14159265f) return f;
    const float u0 = f.qp[0] / uu, u1 = f.qp[3] / uu, u2 = f.qp[6] / uu;
    f.z0 = u0;
    f.s0 = sqrtf(u1 * u1 + u2 * u2);
    f.phi0 = atan2f(u2, u1);
    f.cw = cosf(omega);
    const float theta0 = atan2f(f.s0, f.z0), lo = theta0 - omega, hi = theta0 + omega;
    if (lo > 0.f) {
        const int r = (int)floorf(ring_coordinate(ge, lo));
        f.ring_lo = r < 1 ? 1 : r > rings ? rings : r;
    }
    if (hi < 3.14159265f) {
        const int r = (int)ceilf(ring_coordinate(ge, hi));
        f.ring_hi = r < 1 ? 1 : r > rings ? rings : r;
    }
    return f;
}

// ring i (1 .. 4 nside - 1): cos and sin of its colatitude, its pixels, its first pixel, and its azimuths (j + shift) 2 pi / pixels
RNF_FM_HD void ring_of(const Geometry &ge, int i, float &z, float &s, int &pixels, int &first, float &shift) {
    const int ns = ge.nside;
    if (i < ns || i > 3 * ns) {
        const int k = i < ns ? i : 4 * ns - i;
        const float tmp = (float)(k * k) / (float)(3 * ns * ns);
        s = sqrtf(tmp * (2.f - tmp));
        z = i < ns ? 1.f - tmp : tmp - 1.f;
        pixels = 4 * k;
        first = i < ns ? 2 * k * (k - 1) : ge.npix - 2 * k * (k + 1);
        shift = 0.5f;
    } else {
        z = (float)(2 * ns - i) * 2.f / (float)(3 * ns);
        s = sqrtf((1.f - z) * (1.f + z));
        pixels = 4 * ns;
        first = ge.ncap + (i - ns) * 4 * ns;
        shift = ((i + ns) & 1) ? 0.f : 0.5f;
    }
}

// The cells lo .. lo + count - 1 modulo n of a cyclic window about centre x0 (in cells) of half-width w (in cells), widened by one
// cell on either side; the whole cycle (lo = 0, count = n) where it does not fit or the numbers are not finite
RNF_FM_HD void cyclic_window(float x0, float w, int n, int &lo, int &count) {
    lo = 0;
    count = n;
    if (!(w < (float)n) || !(fabsf(x0) <= 4.f * (float)n)) return;
    const int a = (int)ceilf(x0 - w) - 1, b = (int)floorf(x0 + w) + 1;
    if (b - a + 1 >= n) return;
    count = b - a + 1;
    lo = a % n;
    lo = lo < 0 ? lo + n : lo;
}

// One sweep of a query's enumeration for the GB groups g0 .. (clamped at G - 1).
//   SWEEP_MAX: M[gb] = max t, count = the members, visited = the rows looked at;   SWEEP_SUM: S[gb] = sum exp2(t - M[gb]) (M: finite);
//   SWEEP_ARGMAX: SWEEP_MAX, and A[gb] = the smallest row whose t is M[gb] (-1: none above -inf), bit gb of nans set where a member's t is NaN.
//   F: the anisotropic variant -- a member's term is fisher_term(kq, row, q, ..) on the distance's own differences; kq is not read otherwise.
enum Mode { SWEEP_MAX = 0, SWEEP_SUM = 1, SWEEP_ARGMAX = 2 };
template <int GB, bool W, int MODE, bool F = false>
RNF_FM_HD void sweep(const Geometry &ge, const Quad &kq, const Frame &fr, const float *__restrict__ grid, const float *__restrict__ lw, long long Q, int g0, int G,
                     const float q[9], float *M, double *S, int *A, unsigned &nans, int &count, int &visited) {
    const float *lwg[GB];
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) lwg[gb] = W ? lw + (long long)(g0 + gb < G ? g0 + gb : G - 1) * Q : nullptr;
    for (int i = fr.ring_lo; i <= fr.ring_hi; ++i) {
        float z, s, shift;
        int pixels, first;
        ring_of(ge, i, z, s, pixels, first, shift);
        const float a = fr.cw - z * fr.z0 - 1e-6f, b = s * fr.s0;
        if (a >= b) continue;                                                               // the ring misses the widened disc
        int plo = 0, pcount = pixels;
        if (a > -b) cyclic_window(fr.phi0 * INV_TWO_PI * (float)pixels - shift, acosf(a / b) * INV_TWO_PI * (float)pixels, pixels, plo, pcount);
        const int pwrap = plo + pcount > pixels ? plo + pcount - pixels : 0;                // pixels 0 .. pwrap - 1, then plo .. pend - 1
        const int pend = plo + pcount > pixels ? pixels : plo + pcount;
        const float dphi = TWO_PI / (float)pixels;
        for (int pseg = 0; pseg < 2; ++pseg) {
            const int ja = pseg ? plo : 0, jb = pseg ? pend : pwrap;
            for (int j = ja; j < jb; ++j) {
                float sp, cp;
                sincosf(((float)j + shift) * dphi, &sp, &cp);
                const float *qp = fr.qp;
                const float b00 = z * qp[0] + s * (cp * qp[3] + sp * qp[6]);
                const float b11 = -s * qp[1] + z * (cp * qp[4] + sp * qp[7]), b12 = -s * qp[2] + z * (cp * qp[5] + sp * qp[8]);
                const float b21 = cp * qp[7] - sp * qp[4], b22 = cp * qp[8] - sp * qp[5];
                const float x = b11 + b22, y = b21 - b12;
                const float num = fr.base - 2.f * b00, den = 2.f * sqrtf(x * x + y * y);
                if (num > den) continue;                                                    // the pixel's nearest tilt is beyond the cut
                int tlo = 0, tcount = ge.ntilt;
                if (den >= 0.02f && num > -den)
                    cyclic_window(atan2f(y, x) * INV_TWO_PI * (float)ge.ntilt, acosf(num / den) * INV_TWO_PI * (float)ge.ntilt, ge.ntilt, tlo, tcount);
                const int twrap = tlo + tcount > ge.ntilt ? tlo + tcount - ge.ntilt : 0;
                const int tend = tlo + tcount > ge.ntilt ? ge.ntilt : tlo + tcount;
                float part[GB];
#pragma unroll
                for (int gb = 0; gb < GB; ++gb) part[gb] = 0.f;
                for (int tseg = 0; tseg < 2; ++tseg) {
                    const int ta = tseg ? tlo : 0, tb = tseg ? tend : twrap;
                    for (int t = ta; t < tb; ++t) {
                        const int r = t * ge.npix + first + j;                              // < 72 * 8^level <= 2^31 / 9
                        const float d2 = ks::dist2(grid + 9 * r, q);
                        if (MODE != SWEEP_SUM) ++visited;                                   // dead code where the caller drops it
                        if (!(d2 <= ge.cut)) continue;
                        if (MODE != SWEEP_SUM) ++count;
#pragma unroll
                        for (int gb = 0; gb < GB; ++gb) {
                            const float l2 = W ? lwg[gb][r] * (float)ks::LOG2E : 0.f;
                            const float tt = F ? fisher_term(kq, grid + 9 * r, q, l2) : fmaf(-ge.h, d2, l2);
                            if (MODE == SWEEP_SUM)
                                part[gb] += exp2_soft(tt - M[gb]);
                            else if (MODE == SWEEP_MAX)
                                M[gb] = fmaxf(M[gb], tt);
                            else if (tt != tt)
                                nans |= 1u << gb;
                            else if (tt > M[gb] || (tt == M[gb] && r < A[gb])) {                // members come by (ring, pixel, tilt), not by row
                                M[gb] = tt;
                                A[gb] = r;
                            }
                        }
                    }
                }
                if (MODE == SWEEP_SUM) {
#pragma unroll
                    for (int gb = 0; gb < GB; ++gb) S[gb] += (double)part[gb];
                }
            }
        }
    }
}

// One query, GB groups: out[gb], the count, and the rows the enumeration looked at (the host build reports them)
template <int GB, bool W, bool F = false>
RNF_FM_HD void query_local(const Geometry &ge, const Quad &kq, const float *offset, const float *__restrict__ grid, const float *__restrict__ lw, long long Q,
                           int g0, int G, const float q[9], double l_kappa, float *out, int &count, int &visited) {
#pragma clang fp contract(off)                     // the last expression below: the host build rounds it the same way
    const Frame fr = frame_of(ge, offset, q);
    float M[GB];
    double S[GB];
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
        M[gb] = -INFINITY;
        S[gb] = 0.0;
    }
    count = visited = 0;
    unsigned none = 0;
    sweep<GB, W, SWEEP_MAX, F>(ge, kq, fr, grid, lw, Q, g0, G, q, M, S, nullptr, none, count, visited);
    float Mu[GB];                                  // no live member: M = -inf, every term exp2(-inf - 0) = 0 (a NaN log-weight stays NaN)
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) Mu[gb] = M[gb] == -INFINITY ? 0.f : M[gb];
    int unused = 0;
    sweep<GB, W, SWEEP_SUM, F>(ge, kq, fr, grid, lw, Q, g0, G, q, Mu, S, nullptr, none, unused, unused);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
        const double s = S[gb];
        float r;
        if (!fr.finite || s != s)
            r = NAN;
        else if (M[gb] == -INFINITY)
            r = -INFINITY;
        else
            r = (float)(((double)M[gb] + log2(s)) * ks::LN2 - l_kappa);
        out[gb] = r;
    }
}

// One query, GB groups of rnf_so3_grid_local_max: out[gb] = max_j (lw[g][j] - (kappa/2) d^2) - l(kappa) over the members, arg[gb] the
// smallest row attaining it.  ONE sweep: the maximum and the tie are decided on the sum's own fp32 term t, no exp2.
template <int GB, bool W, bool F = false>
RNF_FM_HD void query_local_max(const Geometry &ge, const Quad &kq, const float *offset, const float *__restrict__ grid, const float *__restrict__ lw, long long Q,
                               int g0, int G, const float q[9], double l_kappa, float *out, int *arg, int &count, int &visited) {
#pragma clang fp contract(off)                     // the last expression below: the host build rounds it the same way
    const Frame fr = frame_of(ge, offset, q);
    float M[GB];
    int A[GB];
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
        M[gb] = -INFINITY;
        A[gb] = -1;
    }
    count = visited = 0;
    unsigned nans = 0;
    sweep<GB, W, SWEEP_ARGMAX, F>(ge, kq, fr, grid, lw, Q, g0, G, q, M, nullptr, A, nans, count, visited);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
        const bool bad = !fr.finite || ((nans >> gb) & 1u);
        out[gb] = bad ? NAN : A[gb] < 0 ? -INFINITY : (float)((double)M[gb] * ks::LN2 - l_kappa);
        arg[gb] = bad ? -1 : A[gb];
    }
}

#if defined(__HIPCC__) && !defined(RNF_SGL_HOST_ONLY)
// grid (ceil(m / THREADS), ceil(G / GB)): out[g][i], count[i] (by the blocks of the first groups)
template <int GB, bool W>
__global__ __launch_bounds__(THREADS) void so3_grid_local_kernel(Geometry ge, const float *__restrict__ offset, const float *__restrict__ grid,
                                                                 const float *__restrict__ queries, const float *__restrict__ lw, long long Q, int m,
                                                                 int G, double l_kappa, float *__restrict__ out, int *__restrict__ count) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= m) return;
    const int g0 = blockIdx.y * GB;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = queries[9 * i + k];
    float res[GB];
    int cnt, visited;
    query_local<GB, W>(ge, Quad{}, offset, grid, lw, Q, g0, G, q, l_kappa, res, cnt, visited);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb)
        if (g0 + gb < G) out[(long long)(g0 + gb) * m + i] = res[gb];
    if (count && g0 == 0) count[i] = cnt;
}

// the same launch shape for rnf_so3_grid_local_max: out[g][i], arg[g][i], count[i]
template <int GB, bool W>
__global__ __launch_bounds__(THREADS) void so3_grid_local_max_kernel(Geometry ge, const float *__restrict__ offset, const float *__restrict__ grid,
                                                                     const float *__restrict__ queries, const float *__restrict__ lw, long long Q,
                                                                     int m, int G, double l_kappa, float *__restrict__ out, int *__restrict__ arg,
                                                                     int *__restrict__ count) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= m) return;
    const int g0 = blockIdx.y * GB;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = queries[9 * i + k];
    float res[GB];
    int at[GB], cnt, visited;
    query_local_max<GB, W>(ge, Quad{}, offset, grid, lw, Q, g0, G, q, l_kappa, res, at, cnt, visited);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb)
        if (g0 + gb < G) {
            out[(long long)(g0 + gb) * m + i] = res[gb];
            arg[(long long)(g0 + gb) * m + i] = at[gb];
        }
    if (count && g0 == 0) count[i] = cnt;
}

// rnf_so3_grid_local_fisher: the launch shape and the stores of the two kernels above on the anisotropic term; MAX: the max-plus pass
template <int GB, bool W, bool MAX>
__global__ __launch_bounds__(THREADS) void so3_grid_local_fisher_kernel(Geometry ge, Quad kq, const float *__restrict__ offset,
                                                                        const float *__restrict__ grid, const float *__restrict__ queries,
                                                                        const float *__restrict__ lw, long long Q, int m, int G, double l_k,
                                                                        float *__restrict__ out, int *__restrict__ arg, int *__restrict__ count) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= m) return;
    const int g0 = blockIdx.y * GB;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = queries[9 * i + k];
    float res[GB];
    int at[GB], cnt, visited;
    if (MAX)
        query_local_max<GB, W, true>(ge, kq, offset, grid, lw, Q, g0, G, q, l_k, res, at, cnt, visited);
    else
        query_local<GB, W, true>(ge, kq, offset, grid, lw, Q, g0, G, q, l_k, res, cnt, visited);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb)
        if (g0 + gb < G) {
            out[(long long)(g0 + gb) * m + i] = res[gb];
            if (MAX) arg[(long long)(g0 + gb) * m + i] = at[gb];
        }
    if (count && g0 == 0) count[i] = cnt;
}
#endif  // __HIPCC__ && !RNF_SGL_HOST_ONLY

// out [G][m] and count [m] (or null) of rnf_so3_grid_local_sum on the host, with the kernel's row functions in the kernel's order
// (queries null: the grid rows; offset: host float[9] or null), and visited [m] (or null), the rows each query's enumeration looked at;
// arguments are not checked
inline void host_grid_local_sum(int level, const float *offset, const float *grid, const float *queries, const float *lw, long long m, int G,
                                double kappa, double d2_cut, float *out, int *count, int *visited = nullptr) {
    const Geometry ge = geometry_of(level, kappa, d2_cut);
    const long long Q = rows_of(level);
    const double l_kappa = ks::log_normaliser(kappa);
    if (!queries) queries = grid;
    for (long long i = 0; i < m; ++i)
        for (int g = 0; g < G; ++g) {
            float r;
            int cnt, vis;
            if (lw)
                query_local<1, true>(ge, Quad{}, offset, grid, lw, Q, g, G, queries + 9 * i, l_kappa, &r, cnt, vis);
            else
                query_local<1, false>(ge, Quad{}, offset, grid, lw, Q, g, G, queries + 9 * i, l_kappa, &r, cnt, vis);
            out[(long long)g * m + i] = r;
            if (count && g == 0) count[i] = cnt;
            if (visited && g == 0) visited[i] = vis;
        }
}

// out [G][m], arg [G][m] and count [m] (or null) of rnf_so3_grid_local_max on the host, as host_grid_local_sum
inline void host_grid_local_max(int level, const float *offset, const float *grid, const float *queries, const float *lw, long long m, int G,
                                double kappa, double d2_cut, float *out, int *arg, int *count, int *visited = nullptr) {
    const Geometry ge = geometry_of(level, kappa, d2_cut);
    const long long Q = rows_of(level);
    const double l_kappa = ks::log_normaliser(kappa);
    if (!queries) queries = grid;
    for (long long i = 0; i < m; ++i)
        for (int g = 0; g < G; ++g) {
            float r;
            int at, cnt, vis;
            if (lw)
                query_local_max<1, true>(ge, Quad{}, offset, grid, lw, Q, g, G, queries + 9 * i, l_kappa, &r, &at, cnt, vis);
            else
                query_local_max<1, false>(ge, Quad{}, offset, grid, lw, Q, g, G, queries + 9 * i, l_kappa, &r, &at, cnt, vis);
            out[(long long)g * m + i] = r;
            arg[(long long)g * m + i] = at;
            if (count && g == 0) count[i] = cnt;
            if (visited && g == 0) visited[i] = vis;
        }
}

// host_grid_local_sum / host_grid_local_max on the anisotropic term: K [9] row-major, arg null: the sum, else the max-plus pass
inline void host_grid_local_fisher(int level, const float *offset, const float *grid, const float *queries, const float *lw, long long m, int G,
                                   const double K[9], double d2_cut, float *out, int *arg, int *count, int *visited = nullptr) {
    const Geometry ge = geometry_of(level, 0.0, d2_cut);
    const Quad kq = quad_of(K);
    const long long Q = rows_of(level);
    const double l_k = log_normaliser_fisher(K);
    if (!queries) queries = grid;
    for (long long i = 0; i < m; ++i)
        for (int g = 0; g < G; ++g) {
            float r;
            int at = -1, cnt, vis;
            if (arg && lw)
                query_local_max<1, true, true>(ge, kq, offset, grid, lw, Q, g, G, queries + 9 * i, l_k, &r, &at, cnt, vis);
            else if (arg)
                query_local_max<1, false, true>(ge, kq, offset, grid, lw, Q, g, G, queries + 9 * i, l_k, &r, &at, cnt, vis);
            else if (lw)
                query_local<1, true, true>(ge, kq, offset, grid, lw, Q, g, G, queries + 9 * i, l_k, &r, cnt, vis);
            else
                query_local<1, false, true>(ge, kq, offset, grid, lw, Q, g, G, queries + 9 * i, l_k, &r, cnt, vis);
            out[(long long)g * m + i] = r;
            if (arg) arg[(long long)g * m + i] = at;
            if (count && g == 0) count[i] = cnt;
            if (visited && g == 0) visited[i] = vis;
        }
}

}  // namespace sgl
}  // namespace rnf
