// Host build of csrc/so3_harmonics.h for tests/test_so3_harmonics_host.py: the outputs of rnf_so3_wigner, rnf_so3_fourier and
// rnf_so3_fourier_eval in the order of the device kernels (entry records in fp64 rounded once, power tables, normalised fp32 weights,
// chunks of 4096 added in fp64 in centre order, the finalise over the chunks; the walk of the entries), and the workspace rule.
#define RNF_SH_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_harmonics.h"

using namespace rnf;

extern "C" {
// R [n][9] -> out [n][C_L]
void hsh_wigner(const float *R, long long n, int L, float *out) { sh::host_wigner(R, n, L, out); }

// C [n][9], lw [G][n] or null -> out [G][C_L]
void hsh_fourier(const float *C, const float *lw, long long n, int G, int L, float *out) { sh::host_fourier(C, lw, n, G, L, out); }

// coeffs [G][C_L], Q [m][9] or [G][m][9] (group_queries) -> out [G][m]
void hsh_fourier_eval(const float *coeffs, const float *Q, long long m, int G, int group_queries, int L, float *out) {
    sh::host_fourier_eval(coeffs, Q, m, G, group_queries != 0, L, out);
}

unsigned long long hsh_fourier_workspace_bytes(long long n, int G, int L) { return sh::carve(nullptr, n, G, L).bytes; }
unsigned long long hsh_records_bytes(int L) { return sh::records_bytes(L); }
int hsh_coefficient_count(int L) { return sh::coefficient_count(L); }
int hsh_degree_offset(int l) { return sh::degree_offset(l); }
}
