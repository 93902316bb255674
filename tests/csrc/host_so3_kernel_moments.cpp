// Host build of csrc/so3_kernel_moments.h for tests/test_so3_moments_host.py: the moments of rnf_so3_kernel_moments in the order of the
// device kernels (chunks of 4096, tiles of 64, the finalise over the chunks, polar3), the kernel sum they share their first output with,
// and l'(kappa) on its own.
#define RNF_KM_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_kernel_moments.h"

using namespace rnf;

extern "C" {
void hkm_dlog_normaliser(const double *kappa, int J, double *dl) {
    for (int a = 0; a < J; ++a) dl[a] = km::dlog_normaliser(kappa[a]);
}

// C [n][9], Q [m][9] or [G][m][9] (group_queries), lw [G][n] or null -> the outputs [G][m] (x 9), each may be null
void hkm_kernel_moments(const float *C, const float *Q, const float *lw, long long n, long long m, int G, double kappa, int group_queries,
                        float *log_density, float *mean, float *msd, float *rotation, float *step) {
    km::host_kernel_moments(C, Q, lw, n, m, G, kappa, group_queries != 0, log_density, mean, msd, rotation, step);
}

// out [G][m] of the kernel sum with J = 1
void hkm_kernel_sum(const float *C, const float *Q, const float *lw, long long n, long long m, int G, double kappa, float *out) {
    ks::host_kernel_sum(C, Q, lw, n, m, G, &kappa, 1, false, out);
}

unsigned long long hkm_workspace_bytes(long long n, long long m, int G) { return km::carve(nullptr, n, m, G).bytes; }
}
