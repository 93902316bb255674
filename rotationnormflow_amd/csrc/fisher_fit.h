// fisher_fit.h -- the maximum-likelihood matrix-Fisher parameter of a moment matrix: the inverse of A -> E_A[R] = dc/dA (fisher_exact.h).
//
// For rotations R_i with weights w_i (sum 1) the log-likelihood of MF(A) is tr(A^T M) - c(A), M = sum w_i R_i.  With the proper SVD
// M = U diag(d) V^T (d0 >= d1 >= |d2|) the maximiser is A = U diag(s) V^T, where s maximises the concave
//     l(s) = s . d - c(s),        grad l = d - m(s),  m = dc/ds = diag E[Q],        Hess l = -H,  H_ij = d2c/ds_i ds_j = Cov(Q_ii, Q_jj).
// H by the 224-node rule of fisher_exact.h, in the coordinates ha = (s0 - s1)/2, hb = (s0 + s1)/2, s2 of the integrand
// phi = 1/2 I0(ha (1-u)) I0(hb (1+u)) exp(s2 u).  With r = I1/I0, r' = 1 - r^2 - r/x (I0' = I1, I1' = I0 - I1/x; r/x -> 1/2 at 0) and the
// expectation E under phi:
//     X = (1-u) r(a),   Y = (1+u) r(b) = 2 - Y',   Y' = (1-u) + (1+u)(1 - r(b)),   u = 1 - om
//     L_aa = Var X + E[(1-u)^2 r'(a)]   L_bb = Var Y' + E[(1+u)^2 r'(b)]   L_ab = -Cov(X, Y')   L_a2 = -Cov(X, om)   L_b2 = Cov(Y', om)
//     L_22 = Var om,        H = J^T L J,  J = d(ha, hb, s2)/ds.
// X, Y', om are all O(1/s) at high concentration, so the covariances lose nothing to cancellation there (Y and u themselves tend to 2
// and 1); everything is built from i0e / i1e, so nothing overflows.
//
// The solve is a damped Newton iteration on the box |s_i| <= max_concentration, started from the inverted Laplace form
// (m_i ~ 1 - 1/2 (1/(s_i+s_j) + 1/(s_i+s_k))): coordinates at a bound whose gradient points outward are held, the others take the Newton
// step of their Hessian block, halved until l has risen by 1e-4 of the predicted amount (once the predicted rise is below what l
// resolves in fp64 the full step is taken).  Every trial point is mapped to its representative in the chamber s0 >= s1 >= |s2|:
// c is invariant under permutations and even sign changes of s, and for ordered d the representative has the largest s . d, so this
// never lowers l.  Stop rule: every free component of d - m(s) is at most 5e-14 in magnitude.  A moment on the boundary of the
// tetrahedron conv{(1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1)} has no finite maximiser; it, and every moment whose maximiser leaves the
// box, gets the maximiser of l OVER THE BOX (s0 == max_concentration) and status CAPPED.  All arithmetic is wave-uniform on the
// device: the evaluator hands every lane the same 14 sums (64 lane sums, xor butterfly), so a row's result depends on the row alone.
#pragma once
#include "fisher_exact.h"

namespace rnf {

constexpr int kFisherFitSums = 14;
constexpr int kFisherFitMaxIter = 64;             // Newton iterations; the host tests need at most 15 from this start
constexpr int kFisherFitBacktracks = 40;
constexpr double kFisherFitGradTol = 5e-14;       // stop rule on |d - m(s)|_inf over the free coordinates
constexpr double kFisherFitInputTol = 1e-5;       // a moment this far outside the tetrahedron is refused (fp32 rotations are orthogonal to ~1e-7)
constexpr int kFisherFitCapped = 1, kFisherFitNotConverged = 2, kFisherFitInput = 4;

// one lane's share of the 14 integrals: 0 F, 1 P, 2 Q, 3 int u f (as fisher_exact_lane), 4 int om f, 5 int Y' f, 6 XX, 7 XY', 8 X om,
// 9 Y'Y', 10 Y' om, 11 om om, 12 int om^2 r'(a) f, 13 int op^2 r'(b) f.  s in the chamber s0 >= s1 >= |s2|.
RNF_FM_HD void fisher_fit_lane(const double s[3], int lane, double acc[kFisherFitSums]) {
    const double ha = 0.5 * (s[0] - s[1]), hb = 0.5 * (s[0] + s[1]), t = s[1] + s[2];
    for (int k = 0; k < kFisherFitSums; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int j = lane; j < kFisherExactNodes; j += kFisherExactLanes) {
        double om, op, w, i0a, i1a, i0b, i1b;
        fisher_exact_node(j, om, op, w);
        const double a = ha * om, b = hb * op;
        bessel_i01e(a, i0a, i1a);
        bessel_i01e(b, i0b, i1b);
        const double e = 0.5 * w * exp(-t * om), f = e * i0a * i0b;
        const double ra = i1a / i0a, rb = i1b / i0b, na = (i0a - i1a) / i0a, nb = (i0b - i1b) / i0b;       // r and 1 - r
        const double qa = a > 1e-8 ? ra / a : 0.5, qb = b > 1e-8 ? rb / b : 0.5;                           // r / x
        const double ka = na * (1.0 + ra) - qa, kb = nb * (1.0 + rb) - qb;                                 // r' = (1 - r)(1 + r) - r/x
        const double fx = e * om * i1a * i0b, yp = om + op * nb, x = om * ra;
        acc[0] += f;
        acc[1] += fx;
        acc[2] += e * op * i0a * i1b;
        acc[3] += 0.5 * (op - om) * f;
        acc[4] += om * f;
        acc[5] += yp * f;
        acc[6] += fx * x;
        acc[7] += fx * yp;
        acc[8] += fx * om;
        acc[9] += yp * yp * f;
        acc[10] += yp * om * f;
        acc[11] += om * om * f;
        acc[12] += om * om * ka * f;
        acc[13] += op * op * kb * f;
    }
}

// log F, m = dc/ds (the formulas of fisher_exact_finish) and H = d2c/ds2 as (00, 01, 02, 11, 12, 22) from the 14 sums over all nodes
RNF_FM_HD void fisher_fit_finish(const double acc[kFisherFitSums], double &lf, double m[3], double H[6]) {
    const double inv = 1.0 / acc[0];
    lf = log(acc[0]);
    m[0] = 0.5 * (acc[2] + acc[1]) * inv;
    m[1] = 0.5 * (acc[2] - acc[1]) * inv;
    m[2] = acc[3] * inv;
    const double ex = acc[1] * inv, ey = acc[5] * inv, eo = acc[4] * inv;
    const double laa = acc[6] * inv - ex * ex + acc[12] * inv, lbb = acc[9] * inv - ey * ey + acc[13] * inv;
    const double lab = -(acc[7] * inv - ex * ey), la2 = -(acc[8] * inv - ex * eo), lb2 = acc[10] * inv - ey * eo, l22 = acc[11] * inv - eo * eo;
    H[0] = 0.25 * (laa + 2.0 * lab + lbb);
    H[1] = 0.25 * (lbb - laa);
    H[2] = 0.5 * (la2 + lb2);
    H[3] = 0.25 * (laa - 2.0 * lab + lbb);
    H[4] = 0.5 * (lb2 - la2);
    H[5] = l22;
}

// the 14 sums in the order of the device kernel, on the host: 64 lane sums, then the xor butterfly
struct FisherFitHostEval {
    void operator()(const double s[3], double acc[kFisherFitSums]) const {
        double v[kFisherExactLanes][kFisherFitSums], n[kFisherExactLanes][kFisherFitSums];
        for (int l = 0; l < kFisherExactLanes; ++l) fisher_fit_lane(s, l, v[l]);
        for (int o = 32; o > 0; o >>= 1) {
            for (int l = 0; l < kFisherExactLanes; ++l)
                for (int k = 0; k < kFisherFitSums; ++k) n[l][k] = v[l][k] + v[l ^ o][k];
            for (int l = 0; l < kFisherExactLanes; ++l)
                for (int k = 0; k < kFisherFitSums; ++k) v[l][k] = n[l][k];
        }
        for (int k = 0; k < kFisherFitSums; ++k) acc[k] = v[0][k];
    }
};

// v -> its representative c in the chamber c0 >= c1 >= |c2| under permutations and even sign changes: c_i = sg_i v[p_i]
RNF_FM_HD void fisher_fit_canon(const double v[3], double c[3], int p[3], double sg[3]) {
    int p0 = 0, p1 = 1, p2 = 2, t;
    if (fabs(v[p0]) < fabs(v[p1])) { t = p0; p0 = p1; p1 = t; }
    if (fabs(v[p1]) < fabs(v[p2])) { t = p1; p1 = p2; p2 = t; }
    if (fabs(v[p0]) < fabs(v[p1])) { t = p0; p0 = p1; p1 = t; }
    p[0] = p0; p[1] = p1; p[2] = p2;
    sg[0] = v[p0] < 0.0 ? -1.0 : 1.0;
    sg[1] = v[p1] < 0.0 ? -1.0 : 1.0;
    sg[2] = sg[0] * sg[1];
    for (int i = 0; i < 3; ++i) c[i] = sg[i] * v[p[i]];
}

RNF_FM_HD int fit_hidx(int i, int j) {                                   // (i, j) -> 00 01 02 11 12 22
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo == 0 ? hi : lo + hi + 1;
}

// Newton direction of the free coordinates: (H_ff + ridge) x = g_f by Cholesky, x = 0 on the held ones
RNF_FM_HD void fisher_fit_direction(const double H[6], const double g[3], const bool held[3], double x[3]) {
    double M[3][3], r[3];
    const double ridge = 1e-14 * (H[0] + H[3] + H[5]) + 1e-300;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) M[i][j] = (held[i] || held[j]) ? (i == j ? 1.0 : 0.0) : H[fit_hidx(i, j)] + (i == j ? ridge : 0.0);
        r[i] = held[i] ? 0.0 : g[i];
    }
    double L[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = M[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            if (i == j) L[i][i] = sqrt(v > ridge ? v : ridge);
            else L[i][j] = v / L[j][j];
        }
    double y[3];
    for (int i = 0; i < 3; ++i) {
        double v = r[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 2; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 3; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
}

// d (any order and signs) -> s with grad c(s) = d, the Hessian of c there, the Newton iterations used and the status bits
template <class Eval>
RNF_FM_HD void fisher_fit_solve(const double d_in[3], double cap, int max_iter, const Eval &eval, double s_out[3], double H_out[6], int &iters,
                                int &status) {
    const double nan = NAN;
    iters = 0;
    status = 0;
    int p[3], q[3];
    double d[3], sg[3], sq[3];
    fisher_fit_canon(d_in, d, p, sg);
    const double x01 = 1.0 - d[0] - d[1] + d[2], x02 = 1.0 - d[0] + d[1] - d[2], x12 = 1.0 + d[0] - d[1] - d[2];
    if (!(fabs(d_in[0]) + fabs(d_in[1]) + fabs(d_in[2]) < INFINITY) || !(x01 >= -kFisherFitInputTol) || !(cap > 0.0) || !(cap < INFINITY)) {
        status = kFisherFitInput;
        for (int k = 0; k < 3; ++k) s_out[k] = nan;
        for (int k = 0; k < 6; ++k) H_out[k] = nan;
        return;
    }
    const double fl = 0.5 / cap;
    const double p01 = 1.0 / (x01 > fl ? x01 : fl) - 1.0, p02 = 1.0 / (x02 > fl ? x02 : fl) - 1.0, p12 = 1.0 / (x12 > fl ? x12 : fl) - 1.0;
    double s[3], t[3] = {0.5 * (p01 + p02 - p12), 0.5 * (p01 + p12 - p02), 0.5 * (p02 + p12 - p01)};
    for (int k = 0; k < 3; ++k) t[k] = t[k] > cap ? cap : (t[k] < -cap ? -cap : t[k]);
    fisher_fit_canon(t, s, q, sq);
    double acc[kFisherFitSums], lf, m[3], H[6], ell;
    eval(s, acc);
    fisher_fit_finish(acc, lf, m, H);
    ell = s[0] * (d[0] - 1.0) + s[1] * (d[1] - 1.0) + s[2] * (d[2] - 1.0) - lf;
    for (;;) {
        double g[3], gmax = 0.0;
        bool held[3];
        for (int k = 0; k < 3; ++k) {
            g[k] = d[k] - m[k];
            held[k] = (s[k] >= cap && g[k] > 0.0) || (s[k] <= -cap && g[k] < 0.0);
            if (!held[k] && fabs(g[k]) > gmax) gmax = fabs(g[k]);
        }
        if (!(gmax > kFisherFitGradTol)) break;
        if (iters >= max_iter) {
            status |= kFisherFitNotConverged;
            break;
        }
        double dir[3];
        fisher_fit_direction(H, g, held, dir);
        const double rise = g[0] * dir[0] + g[1] * dir[1] + g[2] * dir[2];
        const bool blind = rise <= 1e-9 * (1.0 + fabs(ell));          // below what l resolves: full step, Newton converges quadratically here
        double alpha = 1.0, ts[3], tacc[kFisherFitSums], tlf, tm[3], tH[6], tell;
        for (int bt = 0;; ++bt) {
            double gain = 0.0;
            for (int k = 0; k < 3; ++k) {
                double v = s[k] + alpha * dir[k];
                v = v > cap ? cap : (v < -cap ? -cap : v);
                gain += g[k] * (v - s[k]);
                t[k] = v;
            }
            fisher_fit_canon(t, ts, q, sq);
            eval(ts, tacc);
            fisher_fit_finish(tacc, tlf, tm, tH);
            tell = ts[0] * (d[0] - 1.0) + ts[1] * (d[1] - 1.0) + ts[2] * (d[2] - 1.0) - tlf;
            if (blind || bt >= kFisherFitBacktracks || tell >= ell + 1e-4 * gain) break;
            alpha *= 0.5;
        }
        for (int k = 0; k < 3; ++k) { s[k] = ts[k]; m[k] = tm[k]; }
        for (int k = 0; k < 6; ++k) H[k] = tH[k];
        ell = tell;
        ++iters;
    }
    if (s[0] >= cap) status |= kFisherFitCapped;
    for (int i = 0; i < 3; ++i) s_out[p[i]] = sg[i] * s[i];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) H_out[fit_hidx(p[i], p[j])] = sg[i] * sg[j] * H[fit_hidx(i, j)];
}

// moment matrix M (row-major) -> A = U diag(s) V^T with U, V of the proper SVD of M; s, H as fisher_fit_solve for d = the proper
// singular values of M.  M = 0 gives A = 0 exactly; a non-finite or refused M gives NaN.
template <class Eval>
RNF_FM_HD void fisher_fit_matrix(const double M[9], double cap, int max_iter, const Eval &eval, double A[9], double s[3], double H[6], int &iters,
                                 int &status) {
    double U[9], d[3], V[9], sum = 0.0;
    for (int k = 0; k < 9; ++k) sum += fabs(M[k]);
    if (!(sum < INFINITY)) {
        d[0] = d[1] = d[2] = NAN;
    } else {
        proper_svd3(M, U, d, V);
    }
    fisher_fit_solve(d, cap, max_iter, eval, s, H, iters, status);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            A[3 * i + j] = (status & kFisherFitInput) ? NAN : s[0] * U[3 * i] * V[3 * j] + s[1] * U[3 * i + 1] * V[3 * j + 1] + s[2] * U[3 * i + 2] * V[3 * j + 2];
}

}  // namespace rnf
