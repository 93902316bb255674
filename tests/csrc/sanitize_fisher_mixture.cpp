// Stand-alone program over csrc/fisher_mixture.h for a host sanitizer build (tests/test_fisher_mixture_host.py compiles its host code
// with the address and undefined-behaviour sanitizers and runs it as a process of its own): EM on small groups through every status
// path -- converged, capped, empty on entry, emptied by underflow, NaN groups (a NaN row, all weights -inf, every component empty) --
// with and without log-weights and log-responsibilities, across a chunk boundary.  Exit code 0 and "ok" when every run comes back as
// expected.
#include <cstdio>
#include <vector>

#include "../../rotationnormflow_amd/csrc/fisher_mixture.h"

using namespace rnf;

static int g_bad = 0;
static void expect(bool ok, const char *what, int row) {
    if (!ok) {
        std::printf("FAILED: %s (case %d)\n", what, row);
        ++g_bad;
    }
}

// a rotation about the axis (1, 2, 3) / sqrt(14) by angle t, times a rotation about z by angle p: a deterministic spread of rows
static void rotation(double t, double p, float *R) {
    const double ax[3] = {1 / sqrt(14.0), 2 / sqrt(14.0), 3 / sqrt(14.0)}, c = cos(t), s = sin(t), cz = cos(p), sz = sin(p);
    double a[9], z[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[3 * i + j] = (i == j ? c : 0.0) + (1 - c) * ax[i] * ax[j];
    a[1] -= s * ax[2]; a[2] += s * ax[1]; a[3] += s * ax[2]; a[5] -= s * ax[0]; a[6] -= s * ax[1]; a[7] += s * ax[0];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (float)(a[3 * i] * z[j] + a[3 * i + 1] * z[3 + j] + a[3 * i + 2] * z[6 + j]);
}

struct Run {
    std::vector<float> A, resp;
    std::vector<double> log_pi, s, loglik;
    std::vector<int> status;
    double went;
    int used;
};

static Run run(int K, const std::vector<float> &rot, const float *lw, int iterations, double tol, const std::vector<float> &A0,
               const std::vector<double> &lp0, bool want_resp) {
    const long long n = (long long)rot.size() / 9;
    Run r;
    r.A = A0;
    r.log_pi = lp0;
    r.s.assign(3 * K, 0.0);
    r.loglik.assign(iterations + 1, 0.0);
    r.status.assign(K, -1);
    r.resp.assign(want_resp ? (size_t)K * n : 0, 0.f);
    r.used = fisher_mixture_host_fit(K, rot.data(), lw, n, iterations, tol, 1e4, r.A.data(), r.log_pi.data(), r.s.data(), r.loglik.data(), &r.went,
                                     want_resp ? r.resp.data() : nullptr, r.status.data(), nullptr);
    return r;
}

int main() {
    const int n = 4099;                                                  // one full chunk and three rows
    std::vector<float> rot(9 * n), lw(n);
    for (int i = 0; i < n; ++i) {
        rotation(0.37 * i, 0.11 * i, &rot[9 * i]);
        lw[i] = (float)(2.0 * sin(0.7 * i));
    }
    const std::vector<float> A2 = {3, 0, 0, 0, 3, 0, 0, 0, 3, -2, 0, 0, 0, -2, 0, 0, 0, 2};
    const std::vector<double> uniform2 = {log(0.5), log(0.5)};

    Run a = run(2, rot, lw.data(), 6, 0.0, A2, uniform2, true);           // 0: a plain weighted run
    expect(a.used == 6 && a.status[0] == 0 && a.status[1] == 0 && a.loglik[6] >= a.loglik[0], "weighted run", 0);
    Run b = run(2, rot, nullptr, 200, 1e-3, A2, uniform2, false);        // 1: unweighted, stops on tol, NaN after the last used entry
    expect(b.used < 200 && b.loglik[b.used] == b.loglik[b.used] && b.loglik[b.used + 1] != b.loglik[b.used + 1], "stops on tol", 1);
    Run c = run(2, rot, lw.data(), 3, 0.0, A2, {log(1.0), -INFINITY}, true);   // 2: empty on entry
    expect(c.status[1] == kMixEmpty && c.log_pi[1] == -INFINITY && c.A[9] == -2.f && c.resp[n] == -INFINITY && c.status[0] == 0, "empty on entry", 2);

    std::vector<float> two(9 * 40);                                      // 3: two points, both components capped
    for (int i = 0; i < 40; ++i) rotation(i < 20 ? 0.3 : 2.4, 0.0, &two[9 * i]);
    std::vector<float> At(18);
    for (int j = 0; j < 9; ++j) { At[j] = 3.f * two[j]; At[9 + j] = 3.f * two[9 * 20 + j]; }
    Run d = run(2, two, nullptr, 4, 0.0, At, uniform2, true);
    expect(d.status[0] == kFisherFitCapped && d.status[1] == kFisherFitCapped && d.log_pi[0] == log(0.5) && d.loglik[4] == d.loglik[4], "capped", 3);
    std::vector<float> far = At;                                         // 4: a component nobody owns underflows and becomes empty
    for (int j = 0; j < 9; ++j) far[9 + j] = -3000.f * two[j];
    for (int j = 0; j < 9; ++j) far[j] = 3000.f * two[j];
    std::vector<float> one(two.begin(), two.begin() + 9 * 20);
    Run e = run(2, one, nullptr, 2, 0.0, far, uniform2, false);
    expect(e.status[1] == kMixEmpty && e.log_pi[1] == -INFINITY && e.log_pi[0] == 0.0 && e.A[9] == far[9], "emptied by underflow", 4);

    std::vector<float> bad = rot;                                        // 5..7: NaN groups
    bad[9 * 4098 + 4] = NAN;
    Run f = run(2, bad, lw.data(), 2, 0.0, A2, uniform2, true);
    expect(f.status[0] == kFisherFitInput && f.A[0] != f.A[0] && f.loglik[0] != f.loglik[0] && f.resp[0] != f.resp[0], "NaN row", 5);
    std::vector<float> dead(n, -INFINITY);
    Run g = run(2, rot, dead.data(), 2, 0.0, A2, uniform2, false);
    expect(g.status[1] == kFisherFitInput && g.log_pi[0] != g.log_pi[0] && g.went != g.went, "all weights -inf", 6);
    Run h = run(2, rot, lw.data(), 2, 0.0, A2, {-INFINITY, -INFINITY}, false);
    expect(h.status[0] == kFisherFitInput && h.s[0] != h.s[0], "every component empty", 7);

    std::vector<float> A8(72);                                           // 8: the largest K, one row
    std::vector<double> lp8(8, log(0.125));
    for (int k = 0; k < 8; ++k) rotation(0.5 * k, 0.2 * k, &A8[9 * k]);
    std::vector<float> single(rot.begin(), rot.begin() + 9);
    Run i = run(8, single, nullptr, 1, 0.0, A8, lp8, true);
    expect(i.used == 1 && i.status[7] == kFisherFitCapped, "K = 8 on one row", 8);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
