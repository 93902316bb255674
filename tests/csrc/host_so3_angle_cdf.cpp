// Host build of csrc/so3_angle_cdf.h for tests/test_so3_angles_host.py: the outputs of rnf_so3_angle_cdf in the order of the device
// kernels (normalised fp32 weights, chunks of 4096, tiles of 64, the finalise over the chunks), tau of a shared angle and the
// workspace rule.
#define RNF_AC_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_angle_cdf.h"

using namespace rnf;

extern "C" {
// C [n][9], Q [m][9] or [G][m][9] (group_queries), lw [G][n] or null, thresholds double[T] or null, query_tau [G][T][m] or null ->
// mass [G][T][m], mean_angle, mean_sq_angle [G][m], each may be null
void hac_angle_cdf(const float *C, const float *Q, const float *lw, long long n, long long m, int G, int group_queries, int T,
                   const double *thresholds, const float *query_tau, float *mass, float *mean_angle, float *mean_sq_angle) {
    ac::host_angle_cdf(C, Q, lw, n, m, G, group_queries != 0, T, thresholds, query_tau, mass, mean_angle, mean_sq_angle);
}

void hac_tau(const double *theta, int T, float *tau) {
    for (int t = 0; t < T; ++t) tau[t] = ac::tau_of(theta[t]);
}

unsigned long long hac_workspace_bytes(long long n, long long m, int G, int slots) { return ac::carve(nullptr, n, m, G, slots).bytes; }
}
