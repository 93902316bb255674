// Host build of csrc/so3_kernel_sum.h for tests/test_so3_kde_host.py: the pairwise kernel sum of rnf_so3_kernel_sum in the order of the
// device kernels (chunks of 4096, tiles of 64, the weights pass's tree and butterfly), and the normaliser l(kappa) on its own.
#define RNF_KS_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_kernel_sum.h"

using namespace rnf;

extern "C" {
void hks_log_normaliser(const double *kappa, int J, double *l) {
    for (int a = 0; a < J; ++a) l[a] = ks::log_normaliser(kappa[a]);
}

// C [n][9], Q [m][9] or null (the centres), lw [G][n] or null, kappas [J] -> out [G][J][m]
void hks_kernel_sum(const float *C, const float *Q, const float *lw, long long n, long long m, int G, const double *kappas, int J, int loo, float *out) {
    ks::host_kernel_sum(C, Q, lw, n, m, G, kappas, J, loo != 0, out);
}

unsigned long long hks_workspace_bytes(long long n, long long m, int G, int J) { return ks::carve(nullptr, n, m, G, J).bytes; }
}
