// Host build of csrc/fisher_mixture.h for tests/test_fisher_mixture_host.py: the E-step sums of one group in the order of the device
// kernels, the whole EM of G groups as rnf_fisher_mixture_fit runs it, the evaluation of a mixture, and -- written out separately, for the
// K = 1 test -- the moment of rotation_moments_kernel followed by the fit of fisher_fit_kernel.
#include "../../rotationnormflow_amd/csrc/fisher_mixture.h"

using namespace rnf;

extern "C" {
void hfm_c(const float *A, int B, double *c) {
    for (int b = 0; b < B; ++b) c[b] = fisher_mixture_host_c(A + 9 * b);
}

// proper_singular_values3 beside proper_svd3's s, for the bit-identity test
void hfm_singular_values(const double *A, int B, double *s, double *s_svd) {
    for (int b = 0; b < B; ++b) {
        double U[9], V[9];
        proper_singular_values3(A + 9 * b, s + 3 * b);
        proper_svd3(A + 9 * b, U, s_svd + 3 * b, V);
    }
}

// one E-step: c [K] and the 10 K + 3 sums (per component 9 Su, Wu; then Z, sum u lse, sum u (lw - max)); log_resp [K][n] or null
void hfm_sums(int K, const float *rot, const float *lw, long long n, const float *A, const double *log_pi, double *c, double *sums, float *log_resp) {
    hfm_c(A, K, c);
    fisher_mixture_host_sums(K, rot, lw, n, A, log_pi, c, sums, log_resp);
}

// rot [G][n][9] or [n][9] (shared), lw [G][n] or null, A_init [G][K][9], log_pi_init [G][K] or null (uniform); outputs as the C ABI
void hfm_fit(int G, int shared, int K, const float *rot, const float *lw, long long n, int iterations, double tol, double cap, const float *A_init,
             const double *log_pi_init, float *A, double *log_pi, double *s, double *loglik, double *went, float *log_resp, int *status, int *iters) {
    for (int g = 0; g < G; ++g) {
        for (int j = 0; j < 9 * K; ++j) A[(long long)g * 9 * K + j] = A_init[(long long)g * 9 * K + j];
        for (int k = 0; k < K; ++k) log_pi[g * K + k] = log_pi_init ? log_pi_init[g * K + k] : -log((double)K);
        iters[g] = fisher_mixture_host_fit(K, rot + (shared ? 0 : (long long)g * n * 9), lw ? lw + (long long)g * n : nullptr, n, iterations, tol, cap,
                                           A + (long long)g * 9 * K, log_pi + g * K, s + g * 3 * K, loglik + (long long)g * (iterations + 1), went + g,
                                           log_resp ? log_resp + (long long)g * K * n : nullptr, status + g * K, nullptr);
    }
}

void hfm_log_prob(int K, const float *A, const double *log_pi, const float *rot, long long n, double *logp) {
    double c[kMixMaxK], a[9 * kMixMaxK], lp[kMixMaxK], l[kMixMaxK];
    for (int k = 0; k < kMixMaxK; ++k) {                                  // padded with empty components: K = 8 serves every K
        lp[k] = k < K ? log_pi[k] : -INFINITY;
        c[k] = k < K ? fisher_mixture_host_c(A + 9 * k) : 0.0;
        for (int j = 0; j < 9; ++j) a[9 * k + j] = k < K ? (double)A[9 * k + j] : 0.0;
    }
    for (long long i = 0; i < n; ++i) fisher_mixture_row<kMixMaxK>(rot + 9 * i, a, lp, c, l, logp[i]);
}

// the parent path for one group: the sums of rotation_moments_kernel / rotation_moments_final_kernel, then fisher_fit_matrix and the
// rounding of fisher_fit_kernel
void hfm_moments_fit(const float *rot, const float *lw, long long n, double cap, double *M, float *A32, double *s, int *status) {
    double gmax = 0.0;
    if (lw) {
        float m = -INFINITY;
        for (long long i = 0; i < n; ++i) m = fmaxf(m, lw[i]);
        gmax = (double)m;
    }
    const long long nchunk = (n + 4095) / 4096;
    double *part = new double[nchunk * 10];
    for (long long ch = 0; ch < nchunk; ++ch) {
        const long long lo = ch * 4096, hi = lo + 4096 < n ? lo + 4096 : n;
        static double acc[256][10];
        for (int t = 0; t < 256; ++t) {
            for (int k = 0; k < 10; ++k) acc[t][k] = 0.0;
            for (long long i = lo + t; i < hi; i += 256) {
                const double w = lw ? exp((double)lw[i] - gmax) : 1.0;
                for (int k = 0; k < 9; ++k) acc[t][k] += w * (double)rot[9 * i + k];
                acc[t][9] += w;
            }
        }
        for (int k = 0; k < 10; ++k) {
            double w[4];
            for (int wv = 0; wv < 4; ++wv) {
                double v[64];
                for (int l = 0; l < 64; ++l) v[l] = acc[64 * wv + l][k];
                w[wv] = mix_butterfly64(v);
            }
            part[ch * 10 + k] = ((w[0] + w[1]) + w[2]) + w[3];
        }
    }
    double tot[10];
    for (int k = 0; k < 10; ++k) {
        double v[64];
        for (int l = 0; l < 64; ++l) {
            v[l] = 0.0;
            for (long long ch = l; ch < nchunk; ch += 64) v[l] += part[ch * 10 + k];
        }
        tot[k] = mix_butterfly64(v);
    }
    delete[] part;
    for (int k = 0; k < 9; ++k) M[k] = tot[k] / tot[9];
    double A[9], H[6];
    int iters;
    fisher_fit_matrix(M, cap, kFisherFitMaxIter, FisherFitHostEval(), A, s, H, iters, *status);
    for (int k = 0; k < 9; ++k) A32[k] = (float)A[k];
}
}
