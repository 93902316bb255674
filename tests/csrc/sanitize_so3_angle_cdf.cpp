// Stand-alone program over csrc/so3_angle_cdf.h for a host sanitizer build (tests/test_so3_angles_host.py compiles its host code with
// the address and undefined-behaviour sanitizers and runs it as a process of its own): ragged sizes across the tile and chunk
// boundaries, -inf weights, NaN rows, T = 8 and T = 0, thresholds per query, queries per group, null outputs.  Exit code 0 and "ok"
// when every run comes back as expected.
#include <algorithm>
#include <cstdio>
#include <vector>

#define RNF_AC_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_angle_cdf.h"

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
    int T;
    std::vector<float> mass, mean, sq;
    Out(int G, int T_, int m) : T(T_), mass((size_t)G * T_ * m, -1.f), mean((size_t)G * m, -1.f), sq((size_t)G * m, -1.f) {}
    bool finite(int g, int m) const {
        return all_finite(mass.data() + (size_t)g * T * m, (size_t)T * m) && all_finite(&mean[(size_t)g * m], m) && all_finite(&sq[(size_t)g * m], m);
    }
    bool nan(int g, int m) const {
        return all_nan(mass.data() + (size_t)g * T * m, (size_t)T * m) && all_nan(&mean[(size_t)g * m], m) && all_nan(&sq[(size_t)g * m], m);
    }
};

int main() {
    const double PI = ac::PI;
    const double th8[8] = {PI / 36, PI / 12, PI / 6, PI / 3, PI / 2, 2 * PI / 3, 5 * PI / 6, PI};
    const int sizes[][2] = {{1, 1}, {63, 5}, {65, 257}, {4097, 3}};                       // ragged across tiles, blocks and the chunk
    int row = 0;
    for (const auto &sz : sizes) {
        const int n = sz[0], m = sz[1];
        const std::vector<float> C = rotations(n, 0.37, 0.11), Q = rotations(m, 0.53, 0.29);
        for (int T : {8, 5, 3, 1}) {
            Out o(1, T, m);
            ac::host_angle_cdf(C.data(), Q.data(), nullptr, n, m, 1, false, T, th8 + (8 - T), nullptr, o.mass.data(), o.mean.data(), o.sq.data());
            expect(o.finite(0, m), "unweighted run is finite", row++);
            bool top = true, mono = true;
            for (int i = 0; i < m; ++i) {
                top = top && fabsf(o.mass[(size_t)(T - 1) * m + i] - 1.f) < 1e-5f;        // the last threshold is pi: everything counts
                for (int t = 1; t < T; ++t) mono = mono && o.mass[(size_t)t * m + i] >= o.mass[(size_t)(t - 1) * m + i];
            }
            expect(top && mono, "the mass reaches 1 at pi and does not decrease", row++);
            std::vector<float> mass((size_t)T * m, -1.f);                                 // null outputs are not written
            ac::host_angle_cdf(C.data(), Q.data(), nullptr, n, m, 1, false, T, th8 + (8 - T), nullptr, mass.data(), nullptr, nullptr);
            expect(mass == o.mass, "the masses alone, the same values", row++);
            Out z(1, 0, m);                                                               // T = 0: the moments alone
            ac::host_angle_cdf(C.data(), Q.data(), nullptr, n, m, 1, false, 0, nullptr, nullptr, nullptr, z.mean.data(), z.sq.data());
            expect(z.mean == o.mean && z.sq == o.sq, "the moments alone, the same values", row++);
        }
    }
    {                                                                                     // three groups: plain, half -inf, all -inf
        const int n = 4099, m = 70, G = 3, T = 8;
        std::vector<float> C = rotations(n, 0.37, 0.11), Q = rotations(m, 0.53, 0.29), lw((size_t)G * n);
        for (int j = 0; j < n; ++j) {
            lw[j] = (float)(2.0 * sin(0.7 * j));
            lw[n + j] = j % 2 ? -INFINITY : (float)cos(0.3 * j);
            lw[2 * n + j] = -INFINITY;
        }
        for (int j = 1; j < n; j += 2) C[9 * (size_t)j + 4] = j % 4 == 1 ? NAN : INFINITY;    // the dead centres of group 1 are not finite
        Out o(G, T, m);
        ac::host_angle_cdf(C.data(), Q.data(), lw.data(), n, m, G, false, T, th8, nullptr, o.mass.data(), o.mean.data(), o.sq.data());
        expect(o.nan(0, m), "a non-finite centre with a finite weight makes the group NaN", row++);
        expect(o.finite(1, m), "-inf weights leave non-finite centres out", row++);
        expect(o.nan(2, m), "all weights -inf is NaN", row++);
        std::vector<float> Qg((size_t)G * m * 9);                                         // queries per group: group g's are the shared ones
        for (int g = 0; g < G; ++g) std::copy(Q.begin(), Q.end(), Qg.begin() + (size_t)g * m * 9);
        Out p(G, T, m);
        ac::host_angle_cdf(C.data(), Qg.data(), lw.data(), n, m, G, true, T, th8, nullptr, p.mass.data(), p.mean.data(), p.sq.data());
        expect(std::vector<float>(p.mass.begin() + T * m, p.mass.begin() + 2 * T * m) == std::vector<float>(o.mass.begin() + T * m, o.mass.begin() + 2 * T * m) &&
                   std::vector<float>(p.mean.begin() + m, p.mean.begin() + 2 * m) == std::vector<float>(o.mean.begin() + m, o.mean.begin() + 2 * m),
               "queries per group equal shared queries", row++);
        std::vector<float> tau((size_t)G * T * m);                                        // the same thresholds, per (group, query)
        for (int g = 0; g < G; ++g)
            for (int t = 0; t < T; ++t)
                for (int i = 0; i < m; ++i) tau[((size_t)g * T + t) * m + i] = ac::tau_of(th8[t]);
        tau[((size_t)1 * T + 2) * m + 9] = NAN;
        tau[((size_t)1 * T + 3) * m + 9] = -1.f;
        Out r(G, T, m);
        ac::host_angle_cdf(C.data(), Qg.data(), lw.data(), n, m, G, true, T, nullptr, tau.data(), r.mass.data(), r.mean.data(), r.sq.data());
        bool same = std::equal(r.mean.begin() + m, r.mean.begin() + 2 * m, p.mean.begin() + m) && r.nan(0, m) && r.nan(2, m);
        for (int t = 0; t < T; ++t)
            for (int i = 0; i < m; ++i) {
                const size_t at = ((size_t)1 * T + t) * m + i;
                if (i == 9 && t == 2) same = same && r.mass[at] != r.mass[at];
                else if (i == 9 && t == 3) same = same && r.mass[at] == 0.f;
                else same = same && r.mass[at] == p.mass[at];
            }
        expect(same, "thresholds per query: the shared ones' bits, a NaN slot alone is NaN, a negative one 0", row++);
        std::vector<float> Qn = Q;
        Qn[9 * 7 + 2] = INFINITY;
        Out q(1, T, m);
        ac::host_angle_cdf(C.data(), Qn.data(), lw.data() + n, n, m, 1, false, T, th8, nullptr, q.mass.data(), q.mean.data(), q.sq.data());
        expect(q.mass[7] != q.mass[7] && q.mass[(size_t)7 * m + 7] != q.mass[(size_t)7 * m + 7] && q.mean[7] != q.mean[7] && q.sq[7] != q.sq[7] &&
                   q.mass[6] == q.mass[6] && q.mean[6] == q.mean[6] && q.mean[8] == q.mean[8] && q.sq[8] == q.sq[8],
               "a non-finite query alone is NaN", row++);
        std::vector<float> nanw(lw.begin(), lw.begin() + n);
        nanw[4098] = NAN;
        std::vector<float> Cok = rotations(n, 0.37, 0.11);
        ac::host_angle_cdf(Cok.data(), Q.data(), nanw.data(), n, m, 1, false, T, th8, nullptr, q.mass.data(), q.mean.data(), q.sq.data());
        expect(q.nan(0, m), "a NaN log-weight makes the group NaN", row++);
    }
    {                                                                                     // half-turns about x, y, z seen from the identity
        const float C[27] = {1, 0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0, 0, 1, 0, 0, 0, -1, -1, 0, 0, 0, -1, 0, 0, 0, 1};
        const float Q[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double th[2] = {3.0, PI};
        float mass[2], mean, sq;
        ac::host_angle_cdf(C, Q, nullptr, 3, 1, 1, false, 2, th, nullptr, mass, &mean, &sq);
        expect(mass[0] == 0.f && fabsf(mass[1] - 1.f) < 1e-6f && fabsf(mean - (float)PI) < 1e-6f && fabsf(sq - (float)(PI * PI)) < 1e-5f,
               "three half-turns: all of the mass at pi", row++);
    }
    expect(ac::carve(nullptr, 4097, 10, 3, 10).bytes == ((8ull * 3 * 10 * 2 * 10 + 16 * 3 * 2 + 8 * 3 + 4ull * 3 * 4097 + 15) & ~15ull), "workspace rule", row++);
    expect(ac::tau_of(0.0) == 0.f && ac::tau_of(PI) == FLT_MAX && ac::tau_of(PI / 2) == 4.f, "tau at the ends and the middle of the range", row++);
    expect(ac::slots_for(0) == 0 && ac::slots_for(3) == 4 && ac::slots_for(5) == 8 && ac::block_for(1000, 2, 3) == 64 && ac::block_for(70001, 1, 4) == 256,
           "kernel choice", row++);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
