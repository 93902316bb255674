// Stand-alone program over csrc/fisher_fit.h for a host sanitizer build (tests/test_fisher_fit_host.py compiles its host code with the
// address and undefined-behaviour sanitizers and runs it as a process of its own): the round trip s -> d = grad c(s) -> fit on the list of the host
// tests, full moment matrices, and every status path.  Exit code 0 and "ok" when every row comes back as expected.
#include <cstdio>

#include "../../rotationnormflow_amd/csrc/fisher_fit.h"

using namespace rnf;

static int g_bad = 0;
static void expect(bool ok, const char *what, int row) {
    if (!ok) {
        std::printf("FAILED: %s (row %d)\n", what, row);
        ++g_bad;
    }
}

int main() {
    const double S[][3] = {{0, 0, 0}, {1, .5, -.3}, {5, 3, 1}, {5, 1, -1}, {2, 2, 2}, {4, 4, 1}, {3, 3, -3}, {1e-4, 2e-5, 0}, {30, 20, 10},
                           {3e4, 2e4, 1e4}, {1e4, 1, 1e-3}, {300, 200, 100}, {1e3, 1, 1e-3}, {50, 0, 0}};
    const int n = (int)(sizeof(S) / sizeof(S[0]));
    FisherFitHostEval eval;
    for (int b = 0; b < n; ++b) {
        double acc[kFisherFitSums], lf, d[3], H[6], s[3], m[3];
        int iters, status;
        eval(S[b], acc);
        fisher_fit_finish(acc, lf, d, H);
        fisher_fit_solve(d, 1e5, kFisherFitMaxIter, eval, s, H, iters, status);
        eval(s, acc);
        fisher_fit_finish(acc, lf, m, H);
        double res = 0.0;
        for (int k = 0; k < 3; ++k) res = fmax(res, fabs(m[k] - d[k]));
        expect(status == 0 && res <= 1e-13, "round trip", b);
        // the same row as a rotated moment matrix, and with the iteration cap of 1
        const double c = 0.6, sn = 0.8;
        const double M[9] = {c * d[0], -sn * d[1], 0, sn * d[0], c * d[1], 0, 0, 0, d[2]};
        double A[9];
        fisher_fit_matrix(M, 1e5, kFisherFitMaxIter, eval, A, s, H, iters, status);
        expect(status == 0 && fabs(A[0] - c * S[b][0]) <= 1e-6 * (1.0 + S[b][0] * S[b][0] * S[b][0]), "matrix", b);
        fisher_fit_matrix(M, 1e4, 1, eval, A, s, H, iters, status);
        expect(iters <= 1, "iteration cap", b);
    }
    const double D[][3] = {{1, 1, 1}, {1 - 1e-12, -(1 - 1e-12), -(1 - 1e-12)}, {1, 0, 0}, {.9, .9, .8}, {1.2, 0, 0}, {NAN, 0, 0}, {0, INFINITY, 0}};
    const int want[] = {1, 1, 1, 1, 4, 4, 4};
    for (int b = 0; b < 7; ++b) {
        double s[3], H[6];
        int iters, status;
        fisher_fit_solve(D[b], 1e4, kFisherFitMaxIter, eval, s, H, iters, status);
        expect(status == want[b], "status", b);
        expect(want[b] == 4 ? s[0] != s[0] : fmax(fabs(s[0]), fmax(fabs(s[1]), fabs(s[2]))) == 1e4, "capped or NaN value", b);
    }
    const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, N[9] = {NAN, 0, 0, 0, 0, 0, 0, 0, 0};
    double A[9], s[3], H[6];
    int iters, status;
    fisher_fit_matrix(Z, 1e4, kFisherFitMaxIter, eval, A, s, H, iters, status);
    expect(status == 0 && A[0] == 0.0 && A[8] == 0.0, "zero moment", 0);
    fisher_fit_matrix(N, 1e4, kFisherFitMaxIter, eval, A, s, H, iters, status);
    expect(status == 4 && A[4] != A[4], "NaN moment", 0);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
