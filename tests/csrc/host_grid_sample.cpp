// Host build of csrc/grid_sample.h for tests/test_grid_sample_host.py: the chart of a grid cell, the grid's row function, the Philox words
// and the draws of rnf_grid_sample, all through the functions the kernels call (the host's expf stands in for the device's).
#define RNF_GSA_HOST_ONLY
#define RNF_SO3G_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/grid_sample.h"

using namespace rnf;

extern "C" {
// rows [n], u [n][3], offset [9] or null -> rot [n][9]
void hgs_cell_points(int level, const float *offset, const long long *rows, const float *u, long long n, float *rot) {
    gsa::host_cell_points(level, offset, rows, u, n, rot);
}

// the grid's own rows (so3_grid.h's grid_row)
void hgs_grid_rows(int level, const float *offset, const long long *rows, long long n, float *rot) {
    gsa::host_grid_rows(level, offset, rows, n, rot);
}

void hgs_philox(unsigned long long seed, long long draw, long long image, unsigned stream, unsigned *words) {
    unsigned c[4];
    gsa::philox_words(seed, draw, image, stream, c);
    for (int k = 0; k < 4; ++k) words[k] = c[k];
}

int hgs_shift(long long Q) { return gc::fixed_point_shift(Q); }

// rnf_grid_sample on host pointers (target, total and rot may be null)
void hgs_sample(const float *logp, long long Q, int g, int level, long long draws, long long draw_base, long long draws_total, long long image_base,
                int method, int jitter, unsigned long long seed, const float *offset, long long *index, unsigned long long *target,
                unsigned long long *total, float *rot) {
    gsa::host_grid_sample(logp, Q, g, level, draws, draw_base, draws_total, image_base, method, jitter, seed, offset, index, target, total, rot);
}
}
