// fisher_mixture.h -- EM for a K-component mixture of matrix-Fisher distributions (K <= 8), w.r.t. the Haar probability measure:
//     log p(R) = logsumexp_k( log_pi_k + tr(A_k^T R) - c(A_k) ),        c the exact log-normaliser of fisher_exact.h.
//
// One EM iteration of one group of rows R_i with weights w_i = u_i / Z (u_i = exp(lw_i - max lw) in fp64, or 1 without log-weights;
// Z = sum u_i -- the softmax of rnf_rotation_moments, kept unnormalised until the sums are complete):
//   E-step, per row, fp64 from the fp32 inputs:      l_ik = (log_pi_k + tr(A_k^T R_i)) - c_k,   lse_i = m + log(sum_k exp(l_ik - m)),
//     m = max_k l_ik,   r_ik = exp(l_ik - lse_i);    sums  Wu_k = sum_i u_i r_ik,  Su_k = sum_i (u_i r_ik) R_i,  Z,  sum_i u_i lse_i,
//     sum_i u_i (lw_i - max lw)   -- 10 K + 3 numbers.
//   M-step:  pi_k = Wu_k / Z (fp64, log_pi_k = log pi_k),  M_k = Su_k / Wu_k,  A_k = fisher_fit_matrix(M_k) rounded to fp32, and c_k
//     recomputed from the ROUNDED A_k: the state between iterations is (fp32 A, fp64 log_pi) and nothing else.
//   L = sum_i w_i lse_i (the weighted log-likelihood),  E = sum_i w_i log w_i = (sum_i u_i (lw_i - max)) / Z - log Z.
// For K = 1 (log_pi = 0): lse = l and r = exp(0) = 1.0 exactly, so Wu, Su are the sums of rotation_moments_kernel and A, s, status those
// of rnf_rotation_moments followed by rnf_fisher_fit, bit for bit.
//
// A component is EMPTY when log_pi_k = -inf on entry or Wu_k = 0: it is left out of the max and the sum of the logsumexp (its r is an
// exact +0.0, so its sums are +0.0), keeps its A, gets log_pi = -inf and status kMixEmpty.  A group whose Z is not positive (all
// weights -inf), or whose L is not finite (a NaN anywhere in it, or every component empty) is NaN throughout with status INPUT.
//
// Order of the sums (that of rotation_moments_kernel): chunks of 4096 rows; within a chunk "thread" t adds rows t, t + 256, ..; the 64
// threads of a wave are combined by the xor butterfly 32, 16, .. 1, the four waves as ((0 + 1) + 2) + 3; chunk partials c, c + 64, ..
// are added by lane c % 64 and the lanes by the butterfly.  fisher_mixture_host_sums() below adds in this order on the host.
#pragma once
#include "fisher_fit.h"

namespace rnf {

constexpr int kMixMaxK = 8, kMixMaxIterations = 256;
constexpr int kMixEmpty = 8;                       // status bit beside kFisherFitCapped / NotConverged / Input
constexpr int kMixChunk = 4096, kMixThreads = 256;
RNF_FM_HD constexpr int mix_slots(int K) { return 10 * K + 3; }       // per component 9 Su + Wu; then Z, sum u lse, sum u (lw - max)

// The proper singular values of proper_svd3 (fisher_math.h) alone: the same Jacobi sweeps, the same formulas in the same order, with
// the rotations unrolled over (p, q) and the columns picked by selects instead of indexed loads -- the second SVD of the finalise
// kernel (the first is the fit's) then needs no private memory.  Bit-identical to proper_svd3's s on the host (tested).
template <int P, int Q>
RNF_FM_HD void mix_jacobi_rotate(double m[3][3], double v[3][3]) {
    if (m[P][Q] == 0.0) return;
    const double theta = (m[Q][Q] - m[P][P]) / (2.0 * m[P][Q]);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mkp = m[k][P], mkq = m[k][Q];
        m[k][P] = cs * mkp - sn * mkq;
        m[k][Q] = sn * mkp + cs * mkq;
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = cs * vkp - sn * vkq;
        v[k][Q] = sn * vkp + cs * vkq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mpk = m[P][k], mqk = m[Q][k];
        m[P][k] = cs * mpk - sn * mqk;
        m[Q][k] = sn * mpk + cs * mqk;
    }
}

RNF_FM_HD double mix_pick3(double x0, double x1, double x2, int o) { return o == 0 ? x0 : (o == 1 ? x1 : x2); }

RNF_FM_HD void proper_singular_values3(const double a[9], double s[3]) {
    double m[3][3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) m[i][j] = a[i] * a[j] + a[3 + i] * a[3 + j] + a[6 + i] * a[6 + j];
#pragma unroll 1
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(m[0][1]) + fabs(m[0][2]) + fabs(m[1][2]);
        if (off <= 1e-300 || off <= 1e-18 * (fabs(m[0][0]) + fabs(m[1][1]) + fabs(m[2][2]))) break;
        mix_jacobi_rotate<0, 1>(m, v);
        mix_jacobi_rotate<0, 2>(m, v);
        mix_jacobi_rotate<1, 2>(m, v);
    }
    const double e0 = m[0][0], e1 = m[1][1], e2 = m[2][2];
    int o0 = 0, o1 = 1, o2 = 2, t;                          // order of decreasing eigenvalue
    if (mix_pick3(e0, e1, e2, o0) < mix_pick3(e0, e1, e2, o1)) { t = o0; o0 = o1; o1 = t; }
    if (mix_pick3(e0, e1, e2, o1) < mix_pick3(e0, e1, e2, o2)) { t = o1; o1 = o2; o2 = t; }
    if (mix_pick3(e0, e1, e2, o0) < mix_pick3(e0, e1, e2, o1)) { t = o0; o0 = o1; o1 = t; }
    double v0[3], v1[3], u0[3], u1[3], u2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v0[i] = mix_pick3(v[i][0], v[i][1], v[i][2], o0);
        v1[i] = mix_pick3(v[i][0], v[i][1], v[i][2], o1);
    }
    const double v2[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u0[i] = a[3 * i] * v0[0] + a[3 * i + 1] * v0[1] + a[3 * i + 2] * v0[2];
        u1[i] = a[3 * i] * v1[0] + a[3 * i + 1] * v1[1] + a[3 * i + 2] * v1[2];
    }
    s[0] = sqrt(u0[0] * u0[0] + u0[1] * u0[1] + u0[2] * u0[2]);
    const double i0 = s[0] > 0.0 ? 1.0 / s[0] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) u0[i] *= i0;
    const double d01 = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] -= d01 * u0[i];
    s[1] = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    const double i1 = s[1] > 0.0 ? 1.0 / s[1] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] *= i1;
    if (s[0] == 0.0) {                                      // the rank <= 1 completions of proper_svd3
#pragma unroll
        for (int i = 0; i < 3; ++i) { u0[i] = v0[i]; u1[i] = v1[i]; }
    } else if (s[1] == 0.0) {
        const int k = fabs(u0[0]) <= fabs(u0[1]) ? (fabs(u0[0]) <= fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        u1[0] = u0[1] * e[2] - u0[2] * e[1];
        u1[1] = u0[2] * e[0] - u0[0] * e[2];
        u1[2] = u0[0] * e[1] - u0[1] * e[0];
        const double in = 1.0 / sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) u1[i] *= in;
    }
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
    u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
    u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    s[2] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) s[2] += u2[i] * (a[3 * i] * v2[0] + a[3 * i + 1] * v2[1] + a[3 * i + 2] * v2[2]);
}

// One row against K parameter sets: l_k (NaN-free -inf for an empty component) and lse.  A [K][9], log_pi [K], c [K] in fp64.
template <int K>
RNF_FM_HD void fisher_mixture_row(const float *R, const double *A, const double *log_pi, const double *c, double l[K], double &lse) {
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double tr = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) tr += A[9 * k + j] * (double)R[j];
        const bool empty = log_pi[k] == -INFINITY;
        l[k] = empty ? -INFINITY : (log_pi[k] + tr) - c[k];
        m = l[k] > m ? l[k] : m;
    }
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (log_pi[k] != -INFINITY) sum += exp(l[k] - m);                 // a NaN l_k makes the sum, the row and its group NaN
    lse = m == -INFINITY ? NAN : m + log(sum);                            // every component empty (or every l_k NaN): NaN
}

// Add one row with unnormalised weight u (and e = u (lw - max lw), 0 without log-weights) to the 10 K + 3 running sums
template <int K>
RNF_FM_HD void fisher_mixture_add_row(const float *R, double u, double e, const double *A, const double *log_pi, const double *c, double *acc,
                                      float *log_resp, long long resp_stride) {
    double l[K], lse;
    fisher_mixture_row<K>(R, A, log_pi, c, l, lse);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool empty = log_pi[k] == -INFINITY;
        const double r = empty ? 0.0 : exp(l[k] - lse), wr = u * r;
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[10 * k + j] += wr * (double)R[j];
        acc[10 * k + 9] += wr;
        if (log_resp) log_resp[k * resp_stride] = (float)(l[k] - lse);
    }
    acc[10 * K] += u;
    acc[10 * K + 1] += u * lse;
    acc[10 * K + 2] += e;
}

// L and -E of a group from its complete sums; false when the group is NaN (status INPUT)
RNF_FM_HD bool fisher_mixture_group(double Z, double ulse, double ue, bool weighted, double &L, double &weight_entropy) {
    L = ulse / Z;
    weight_entropy = weighted ? log(Z) - ue / Z : log(Z);
    const bool ok = Z > 0.0 && Z < INFINITY && fabs(L) < INFINITY && fabs(weight_entropy) < INFINITY;
    if (!ok) L = weight_entropy = NAN;
    return ok;
}

// The M-step of one live component from its ten sums: log_pi (fp64), A rounded to fp32, s and the fit's status.  Wu = 0 makes it empty:
// false is returned and nothing is written.
template <class Eval>
RNF_FM_HD bool fisher_mixture_mstep(const double part[10], double Z, double cap, const Eval &eval, double &log_pi, float A32[9], double s[3],
                                    int &status) {
    if (part[9] == 0.0) return false;
    double M[9], A[9], H[6];
    int iters;
#pragma unroll
    for (int j = 0; j < 9; ++j) M[j] = part[j] / part[9];
    fisher_fit_matrix(M, cap, kFisherFitMaxIter, eval, A, s, H, iters, status);
    log_pi = log(part[9] / Z);
#pragma unroll
    for (int j = 0; j < 9; ++j) A32[j] = (float)A[j];
    return true;
}

// ---- the host evaluator: the same arithmetic in the same order ----------------------------------------------------------------------

inline double mix_butterfly64(double v[64]) {
    double n[64];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ o];
        for (int l = 0; l < 64; ++l) v[l] = n[l];
    }
    return v[0];
}

// the 10 K + 3 sums of one group: rot [n][9], lw [n] or null, A [K][9] fp32, log_pi [K], c [K]; log_resp [K][n] or null
template <int K>
inline void fisher_mixture_host_sums_k(const float *rot, const float *lw, long long n, const float *A32, const double *log_pi, const double *c,
                                       double *sums, float *log_resp) {
    constexpr int S = mix_slots(K);
    double A[9 * K];
    for (int j = 0; j < 9 * K; ++j) A[j] = (double)A32[j];
    double gmax = 0.0;
    if (lw) {
        float m = -INFINITY;
        for (long long i = 0; i < n; ++i) m = fmaxf(m, lw[i]);
        gmax = (double)m;
    }
    const long long nchunk = (n + kMixChunk - 1) / kMixChunk;
    double *part = new double[(size_t)nchunk * S];
    double (*acc)[S] = new double[kMixThreads][S];
    for (long long ch = 0; ch < nchunk; ++ch) {
        const long long lo = ch * kMixChunk, hi = lo + kMixChunk < n ? lo + kMixChunk : n;
        for (int t = 0; t < kMixThreads; ++t) {
            for (int q = 0; q < S; ++q) acc[t][q] = 0.0;
            for (long long i = lo + t; i < hi; i += kMixThreads) {
                const double d = lw ? (double)lw[i] - gmax : 0.0, u = lw ? exp(d) : 1.0, e = u > 0.0 ? u * d : 0.0;
                fisher_mixture_add_row<K>(rot + 9 * i, u, e, A, log_pi, c, acc[t], log_resp ? log_resp + i : nullptr, n);
            }
        }
        for (int q = 0; q < S; ++q) {
            double w[4];
            for (int wv = 0; wv < 4; ++wv) {
                double v[64];
                for (int l = 0; l < 64; ++l) v[l] = acc[64 * wv + l][q];
                w[wv] = mix_butterfly64(v);
            }
            part[ch * S + q] = ((w[0] + w[1]) + w[2]) + w[3];
        }
    }
    for (int q = 0; q < S; ++q) {
        double v[64];
        for (int l = 0; l < 64; ++l) {
            v[l] = 0.0;
            for (long long ch = l; ch < nchunk; ch += 64) v[l] += part[ch * S + q];
        }
        sums[q] = mix_butterfly64(v);
    }
    delete[] acc;
    delete[] part;
}

inline void fisher_mixture_host_sums(int K, const float *rot, const float *lw, long long n, const float *A32, const double *log_pi, const double *c,
                                     double *sums, float *log_resp) {
    switch (K) {
        case 1: return fisher_mixture_host_sums_k<1>(rot, lw, n, A32, log_pi, c, sums, log_resp);
        case 2: return fisher_mixture_host_sums_k<2>(rot, lw, n, A32, log_pi, c, sums, log_resp);
        case 3: return fisher_mixture_host_sums_k<3>(rot, lw, n, A32, log_pi, c, sums, log_resp);
        case 4: return fisher_mixture_host_sums_k<4>(rot, lw, n, A32, log_pi, c, sums, log_resp);
        case 5: return fisher_mixture_host_sums_k<5>(rot, lw, n, A32, log_pi, c, sums, log_resp);
        case 6: return fisher_mixture_host_sums_k<6>(rot, lw, n, A32, log_pi, c, sums, log_resp);
        case 7: return fisher_mixture_host_sums_k<7>(rot, lw, n, A32, log_pi, c, sums, log_resp);
        default: return fisher_mixture_host_sums_k<8>(rot, lw, n, A32, log_pi, c, sums, log_resp);
    }
}

// c of a rounded fp32 parameter matrix, by the path of fisher_exact_kernel (fp64 proper singular values, 64 lane sums, butterfly)
inline double fisher_mixture_host_c(const float A32[9]) {
    double a[9], s[3], c, m[3], h;
    for (int j = 0; j < 9; ++j) a[j] = (double)A32[j];
    proper_singular_values3(a, s);
    fisher_exact_from_s(s, c, m, h);
    return c;
}

// EM on the host for one group, as rnf_fisher_mixture_fit runs it.  A [K][9] and log_pi [K] are the state, in and out; loglik
// [iterations + 1] (NaN after the group has finished); s [K][3], status [K]; log_resp [K][n] or null.  Returns the iterations used.
inline int fisher_mixture_host_fit(int K, const float *rot, const float *lw, long long n, int iterations, double tol, double cap, float *A,
                                   double *log_pi, double *s, double *loglik, double *weight_entropy, float *log_resp, int *status,
                                   double *sums_out /* [10 K + 3] of the first E-step, or null */) {
    double c[kMixMaxK], sums[mix_slots(kMixMaxK)];
    for (int k = 0; k < K; ++k) {
        c[k] = fisher_mixture_host_c(A + 9 * k);
        status[k] = log_pi[k] == -INFINITY ? kMixEmpty : 0;
        for (int j = 0; j < 3; ++j) s[3 * k + j] = NAN;
    }
    for (int t = 0; t <= iterations; ++t) loglik[t] = NAN;
    *weight_entropy = NAN;
    int used = 0;
    for (int t = 0;; ++t) {
        const bool last = t == iterations;
        fisher_mixture_host_sums(K, rot, lw, n, A, log_pi, c, sums, last ? log_resp : nullptr);
        if (t == 0 && sums_out)
            for (int q = 0; q < mix_slots(K); ++q) sums_out[q] = sums[q];
        double L, went;
        if (!fisher_mixture_group(sums[10 * K], sums[10 * K + 1], sums[10 * K + 2], lw != nullptr, L, went)) {
            for (int k = 0; k < K; ++k) {
                status[k] = kFisherFitInput;
                log_pi[k] = NAN;
                for (int j = 0; j < 9; ++j) A[9 * k + j] = NAN;
                for (int j = 0; j < 3; ++j) s[3 * k + j] = NAN;
            }
            for (int q = 0; q <= iterations; ++q) loglik[q] = NAN;
            *weight_entropy = NAN;
            if (log_resp)
                for (long long i = 0; i < (long long)K * n; ++i) log_resp[i] = NAN;
            return t;
        }
        loglik[t] = L;
        *weight_entropy = went;
        used = t;
        if (last) break;
        if (t > 0 && tol > 0.0 && L - loglik[t - 1] >= 0.0 && L - loglik[t - 1] <= tol) {
            if (log_resp) fisher_mixture_host_sums(K, rot, lw, n, A, log_pi, c, sums, log_resp);
            break;
        }
        for (int k = 0; k < K; ++k) {
            bool live = log_pi[k] != -INFINITY;
            if (live) live = fisher_mixture_mstep(sums + 10 * k, sums[10 * K], cap, FisherFitHostEval(), log_pi[k], A + 9 * k, s + 3 * k, status[k]);
            if (live) {
                c[k] = fisher_mixture_host_c(A + 9 * k);
            } else {
                log_pi[k] = -INFINITY;
                status[k] = kMixEmpty;
            }
        }
    }
    return used;
}

}  // namespace rnf
