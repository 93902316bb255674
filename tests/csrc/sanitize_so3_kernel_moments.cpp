// Stand-alone program over csrc/so3_kernel_moments.h for a host sanitizer build (tests/test_so3_moments_host.py compiles its host code
// with the address and undefined-behaviour sanitizers and runs it as a process of its own): ragged sizes across the tile and chunk
// boundaries, -inf weights, NaN rows, a mean without a direction (det <= 0), queries per group, null outputs.  Exit code 0 and "ok"
// when every run comes back as expected.
#include <cstdio>
#include <vector>

#define RNF_KM_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_kernel_moments.h"

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

static std::vector<float> rotations(int n, double dt, double dp) {
    std::vector<float> r(9 * (size_t)n);
    for (int i = 0; i < n; ++i) rotation(dt * i, dp * i, &r[9 * (size_t)i]);
    return r;
}

static bool all_finite(const float *v, size_t k) {
    for (size_t i = 0; i < k; ++i)
        if (!(fabsf(v[i]) < INFINITY)) return false;
    return true;
}
static bool all_nan(const float *v, size_t k) {
    for (size_t i = 0; i < k; ++i)
        if (v[i] == v[i]) return false;
    return true;
}

struct Out {
    std::vector<float> lp, mean, msd, rot, step;
    Out(int G, int m) : lp((size_t)G * m, -1.f), mean((size_t)G * m * 9, -1.f), msd((size_t)G * m, -1.f), rot((size_t)G * m * 9, -1.f), step((size_t)G * m, -1.f) {}
    bool finite3(int g, int m) const {             // log_density, mean, msd of group g
        return all_finite(&lp[(size_t)g * m], m) && all_finite(&mean[(size_t)g * m * 9], 9 * (size_t)m) && all_finite(&msd[(size_t)g * m], m);
    }
    bool nan5(int g, int m) const {
        return all_nan(&lp[(size_t)g * m], m) && all_nan(&mean[(size_t)g * m * 9], 9 * (size_t)m) && all_nan(&msd[(size_t)g * m], m) &&
               all_nan(&rot[(size_t)g * m * 9], 9 * (size_t)m) && all_nan(&step[(size_t)g * m], m);
    }
};

static void run(const float *C, const float *Q, const float *lw, int n, int m, int G, double kappa, bool gq, Out &o) {
    km::host_kernel_moments(C, Q, lw, n, m, G, kappa, gq, o.lp.data(), o.mean.data(), o.msd.data(), o.rot.data(), o.step.data());
}

int main() {
    const double kappas[4] = {0.0, 4.0, 256.0, 1e6};
    const int sizes[][2] = {{1, 1}, {63, 5}, {65, 257}, {4097, 3}};                       // ragged across tiles, blocks and the chunk
    int row = 0;
    for (const auto &sz : sizes) {
        const int n = sz[0], m = sz[1];
        const std::vector<float> C = rotations(n, 0.37, 0.11), Q = rotations(m, 0.53, 0.29);
        for (double kappa : kappas) {
            Out o(1, m);
            run(C.data(), Q.data(), nullptr, n, m, 1, kappa, false, o);
            expect(o.finite3(0, m), "unweighted run is finite", row++);
            std::vector<float> lp(m, -1.f), mean(9 * (size_t)m, -1.f);                    // null outputs are not written
            km::host_kernel_moments(C.data(), Q.data(), nullptr, n, m, 1, kappa, false, lp.data(), mean.data(), nullptr, nullptr, nullptr);
            expect(lp == o.lp && mean == o.mean, "fewer outputs, the same values", row++);
        }
    }
    {                                                                                     // three groups: plain, half -inf, all -inf
        const int n = 4099, m = 70, G = 3;
        std::vector<float> C = rotations(n, 0.37, 0.11), Q = rotations(m, 0.53, 0.29), lw((size_t)G * n);
        for (int j = 0; j < n; ++j) {
            lw[j] = (float)(2.0 * sin(0.7 * j));
            lw[n + j] = j % 2 ? -INFINITY : (float)cos(0.3 * j);
            lw[2 * n + j] = -INFINITY;
        }
        for (int j = 1; j < n; j += 2) C[9 * (size_t)j + 4] = j % 4 == 1 ? NAN : INFINITY;    // the dead centres of group 1 are not finite
        Out o(G, m);
        run(C.data(), Q.data(), lw.data(), n, m, G, 16.0, false, o);
        expect(o.nan5(0, m), "a non-finite centre with a finite weight makes the group NaN", row++);
        expect(o.finite3(1, m), "-inf weights leave non-finite centres out", row++);
        expect(o.nan5(2, m), "all weights -inf is NaN", row++);
        std::vector<float> Qg((size_t)G * m * 9);                                         // queries per group: group g's are the shared ones
        for (int g = 0; g < G; ++g) std::copy(Q.begin(), Q.end(), Qg.begin() + (size_t)g * m * 9);
        Out p(G, m);
        run(C.data(), Qg.data(), lw.data(), n, m, G, 16.0, true, p);
        expect(std::vector<float>(p.mean.begin() + 9 * m, p.mean.begin() + 18 * m) == std::vector<float>(o.mean.begin() + 9 * m, o.mean.begin() + 18 * m) &&
                   std::vector<float>(p.lp.begin() + m, p.lp.begin() + 2 * m) == std::vector<float>(o.lp.begin() + m, o.lp.begin() + 2 * m),
               "queries per group equal shared queries", row++);
        std::vector<float> Qn = Q;
        Qn[9 * 7 + 2] = INFINITY;
        Out q(1, m);
        run(C.data(), Qn.data(), lw.data() + n, n, m, 1, 16.0, false, q);
        expect(q.lp[7] != q.lp[7] && q.mean[63] != q.mean[63] && q.msd[7] != q.msd[7] && q.rot[63] != q.rot[63] && q.step[7] != q.step[7] &&
                   q.lp[6] == q.lp[6] && q.mean[62] == q.mean[62] && q.lp[8] == q.lp[8] && q.mean[72] == q.mean[72],
               "a non-finite query alone is NaN", row++);
        std::vector<float> nanw(lw.begin(), lw.begin() + n);
        nanw[4098] = NAN;
        std::vector<float> Cok = rotations(n, 0.37, 0.11);
        run(Cok.data(), Q.data(), nanw.data(), n, m, 1, 16.0, false, q);
        expect(q.nan5(0, m), "a NaN log-weight makes the group NaN", row++);
    }
    {                                                                                     // half-turns about x, y, z at kappa = 0: mean = -I / 3
        const float C[27] = {1, 0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0, 0, 1, 0, 0, 0, -1, -1, 0, 0, 0, -1, 0, 0, 0, 1};
        const float Q[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        Out o(1, 1);
        run(C, Q, nullptr, 3, 1, 1, 0.0, false, o);
        expect(fabsf(o.mean[0] + 1.f / 3.f) < 1e-6f && fabsf(o.mean[1]) < 1e-6f && o.lp[0] == o.lp[0], "the mean of three half-turns", row++);
        expect(all_nan(o.rot.data(), 9) && o.step[0] != o.step[0], "no mean direction: rotation and step are NaN", row++);
        run(C, Q, nullptr, 1, 1, 1, 8.0, false, o);                                       // one centre: its own mean, a rotation
        expect(o.mean[4] == -1.f && fabsf(o.rot[4] + 1.f) < 1e-6f && fabsf(o.step[0] - sqrtf(8.f)) < 1e-5f, "one centre", row++);
    }
    expect(km::carve(nullptr, 4097, 10, 3).bytes == ((92ull * 3 * 2 * 10 + 16 * 3 * 2 + 8 * 3 + 4 * 2 + 15) & ~15ull), "workspace rule", row++);
    expect(km::dlog_normaliser(0.0) == -3.0 && fabs(km::dlog_normaliser(1e6) + 1.5e-6) < 1e-12, "l'(kappa) at the ends of the range", row++);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
