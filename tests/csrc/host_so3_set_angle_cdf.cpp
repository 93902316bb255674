// Host build of csrc/so3_set_angle_cdf.h for tests/test_so3_set_angles_host.py: the outputs of rnf_so3_set_angle_cdf in the order of
// the device kernels (normalised fp32 weights, chunks of 4096, tiles of 64 with the minima over the members first, the finalise over
// the chunks), and rnf_so3_angle_cdf's host evaluator beside it for the K = 1 identity.
#define RNF_SAC_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_set_angle_cdf.h"

using namespace rnf;

extern "C" {
// C [n][9], Q [m][K][9] or [G][m][K][9] (group_queries), lw [G][n] or null, thresholds double[T] or null, query_tau [G][T][m] or null
// -> mass [G][T][m], mean_angle, mean_sq_angle [G][m], each may be null
void hsac_set_angle_cdf(const float *C, const float *Q, const float *lw, long long n, long long m, int K, int G, int group_queries, int T,
                        const double *thresholds, const float *query_tau, float *mass, float *mean_angle, float *mean_sq_angle) {
    sac::host_set_angle_cdf(C, Q, lw, n, m, K, G, group_queries != 0, T, thresholds, query_tau, mass, mean_angle, mean_sq_angle);
}

void hsac_angle_cdf(const float *C, const float *Q, const float *lw, long long n, long long m, int G, int group_queries, int T,
                    const double *thresholds, const float *query_tau, float *mass, float *mean_angle, float *mean_sq_angle) {
    ac::host_angle_cdf(C, Q, lw, n, m, G, group_queries != 0, T, thresholds, query_tau, mass, mean_angle, mean_sq_angle);
}

unsigned long long hsac_workspace_bytes(long long n, long long m, int G, int slots) { return ac::carve(nullptr, n, m, G, slots).bytes; }

int hsac_groups_for(int slots) { return sac::groups_for(slots); }

int hsac_wave_per_set(long long m, long long nchunk, long long G, int K) { return sac::wave_per_set(m, nchunk, G, K); }
}
