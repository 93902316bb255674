// Host build of csrc/fisher_fit.h for tests/test_fisher_fit_host.py: the Hessian of c from given proper singular values, the solve from
// given moments d, and the whole fit of a moment matrix.  max_iter <= 0 means the library's own cap (a test passes 1 to see NOT_CONVERGED).
#include "../../rotationnormflow_amd/csrc/fisher_fit.h"

using namespace rnf;

extern "C" {
int hff_max_iter() { return kFisherFitMaxIter; }
void hff_hessian(const double *s, int B, double *m, double *H) {
    for (int b = 0; b < B; ++b) {
        double acc[kFisherFitSums], lf;
        FisherFitHostEval()(s + 3 * b, acc);
        fisher_fit_finish(acc, lf, m + 3 * b, H + 6 * b);
    }
}
void hff_solve(const double *d, int B, double cap, int max_iter, double *s, double *H, int *iters, int *status) {
    for (int b = 0; b < B; ++b)
        fisher_fit_solve(d + 3 * b, cap, max_iter > 0 ? max_iter : kFisherFitMaxIter, FisherFitHostEval(), s + 3 * b, H + 6 * b, iters[b], status[b]);
}
void hff_fit(const double *M, int B, double cap, int max_iter, double *A, double *s, double *H, int *iters, int *status) {
    for (int b = 0; b < B; ++b)
        fisher_fit_matrix(M + 9 * b, cap, max_iter > 0 ? max_iter : kFisherFitMaxIter, FisherFitHostEval(), A + 9 * b, s + 3 * b, H + 6 * b, iters[b],
                          status[b]);
}
}
