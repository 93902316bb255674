// Host build of csrc/so3_grid_local.h for tests/test_so3_grid_viterbi_host.py: the max-plus pass of rnf_so3_grid_local_max with the
// kernel's row functions in the kernel's order.
#define RNF_SGL_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_grid_local.h"

using namespace rnf;

extern "C" {
// grid [Q][9], queries [m][9] or null (the grid rows), lw [G][Q] or null, offset [9] or null -> out [G][m], arg [G][m], count [m] (or null)
void hsgv_local_max(int level, const float *offset, const float *grid, const float *queries, const float *lw, long long m, int G, double kappa,
                    double d2_cut, float *out, int *arg, int *count) {
    sgl::host_grid_local_max(level, offset, grid, queries, lw, m, G, kappa, d2_cut, out, arg, count);
}
}
