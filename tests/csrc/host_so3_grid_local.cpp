// Host build of csrc/so3_grid_local.h for tests/test_so3_grid_local_host.py: the neighbour-limited kernel sum of rnf_so3_grid_local_sum
// with the kernel's row functions in the kernel's order, and the grid rows of csrc/so3_grid.h's definition to test it on.
#define RNF_SGL_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_grid_local.h"

using namespace rnf;

extern "C" {
// grid [Q][9], queries [m][9] or null (the grid rows), lw [G][Q] or null, offset [9] or null -> out [G][m], count [m] (or null),
// visited [m] (or null): the rows each query's enumeration looked at
void hsgl_local_sum(int level, const float *offset, const float *grid, const float *queries, const float *lw, long long m, int G, double kappa,
                    double d2_cut, float *out, int *count, int *visited) {
    sgl::host_grid_local_sum(level, offset, grid, queries, lw, m, G, kappa, d2_cut, out, count, visited);
}

void hsgl_exp2_soft(const float *x, long long n, float *y) {
    for (long long i = 0; i < n; ++i) y[i] = sgl::exp2_soft(x[i]);
}
}
