// Host build of the anisotropic variant of csrc/so3_grid_local.h for tests/test_so3_grid_local_fisher_host.py: the two passes of
// rnf_so3_grid_local_fisher with the kernel's row functions in the kernel's order, the isotropic passes next to them, and the host
// pieces of the entry point (the log-normaliser, the eigenvalues, the refusals of a concentration).
#define RNF_SGL_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_grid_local.h"

using namespace rnf;

extern "C" {
// grid [Q][9], queries [m][9] or null (the grid rows), lw [G][Q] or null, offset [9] or null, K [9] -> out [G][m], arg [G][m] (null: the
// sum; else the max-plus pass), count [m] (or null)
void hsglf_local(int level, const float *offset, const float *grid, const float *queries, const float *lw, long long m, int G, const double *K,
                 double d2_cut, float *out, int *arg, int *count) {
    sgl::host_grid_local_fisher(level, offset, grid, queries, lw, m, G, K, d2_cut, out, arg, count);
}

// the isotropic passes of the same header
void hsglf_local_iso(int level, const float *offset, const float *grid, const float *queries, const float *lw, long long m, int G, double kappa,
                     double d2_cut, float *out, int *arg, int *count) {
    if (arg)
        sgl::host_grid_local_max(level, offset, grid, queries, lw, m, G, kappa, d2_cut, out, arg, count);
    else
        sgl::host_grid_local_sum(level, offset, grid, queries, lw, m, G, kappa, d2_cut, out, count);
}

double hsglf_log_normaliser(const double *K) { return sgl::log_normaliser_fisher(K); }
double hsglf_log_normaliser_iso(double kappa) { return ks::log_normaliser(kappa); }
int hsglf_concentration_defect(const double *K) { return sgl::concentration_defect(K); }
void hsglf_eigenvalues(const double *K, double *ev) { sgl::sym_eigenvalues3(K, ev); }
}
