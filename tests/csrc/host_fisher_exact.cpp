// Host build of csrc/fisher_exact.h for tests/test_fisher_exact_host.py: scaled Bessel functions, the fixed-node quadrature from given
// proper singular values, and the whole evaluation (proper SVD included) of c, dc/dA and the entropy.
#include "../../rotationnormflow_amd/csrc/fisher_exact.h"

using namespace rnf;

extern "C" {
double hfe_bessel_split() { return kBesselSplit; }
int hfe_nodes() { return kFisherExactNodes; }
void hfe_bessel(const double *x, int n, double *i0, double *i1) {
    for (int i = 0; i < n; ++i) {
        i0[i] = bessel_i0e(x[i]);
        i1[i] = bessel_i1e(x[i]);
    }
}
void hfe_node(int j, double *om, double *op, double *w) { fisher_exact_node(j, *om, *op, *w); }
void hfe_from_s(const double *s, int B, double *c, double *m, double *h) {
    for (int b = 0; b < B; ++b) fisher_exact_from_s(s + 3 * b, c[b], m + 3 * b, h[b]);
}
void hfe_exact(const double *A, int B, double *c, double *dc, double *h) {
    for (int b = 0; b < B; ++b) c[b] = fisher_exact(A + 9 * b, dc + 9 * b, h + b);
}
}
