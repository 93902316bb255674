// Stand-alone program over csrc/so3_set_angle_cdf.h for a host sanitizer build (tests/test_so3_set_angles_host.py compiles its host
// code with the address and undefined-behaviour sanitizers and runs it as a process of its own): ragged sizes across the tile and chunk
// boundaries, K = 1, 2, 12 and 720, padding members, sets of padding only, -inf weights, NaN rows, T = 8 and T = 0, thresholds per set,
// sets per group, null outputs, and ac::carve.  Exit code 0 and "ok" when every run comes back as expected.
#include <algorithm>
#include <cstdio>
#include <vector>

#define RNF_SAC_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_set_angle_cdf.h"

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

static bool all_finite(const std::vector<float> &v) {
    for (float x : v)
        if (!(fabsf(x) < INFINITY)) return false;
    return true;
}
static bool nan_at(const std::vector<float> &v, size_t at) { return v[at] != v[at]; }

struct Out {
    std::vector<float> mass, mean, sq;
    Out(int G, int T, int m) : mass((size_t)G * T * m, -1.f), mean((size_t)G * m, -1.f), sq((size_t)G * m, -1.f) {}
    bool operator==(const Out &o) const { return mass == o.mass && mean == o.mean && sq == o.sq; }
};

static Out run(const std::vector<float> &C, const std::vector<float> &Q, const float *lw, int n, int m, int K, int G, bool per_group, int T,
               const double *th, const float *tau) {
    Out o(G, T, m);
    sac::host_set_angle_cdf(C.data(), Q.data(), lw, n, m, K, G, per_group, T, th, tau, T ? o.mass.data() : nullptr, o.mean.data(), o.sq.data());
    return o;
}

int main() {
    const double PI = ac::PI;
    const double th8[8] = {PI / 36, PI / 12, PI / 6, PI / 3, PI / 2, 2 * PI / 3, 5 * PI / 6, PI};
    const int sizes[][3] = {{1, 1, 1}, {63, 5, 2}, {65, 67, 12}, {4097, 3, 12}, {130, 2, 720}};     // n, m, K
    int row = 0;
    for (const auto &sz : sizes) {
        const int n = sz[0], m = sz[1], K = sz[2];
        const std::vector<float> C = rotations(n, 0.37, 0.11), Q = rotations(m * K, 0.53, 0.29);
        for (int T : {8, 3, 0}) {
            const Out o = run(C, Q, nullptr, n, m, K, 1, false, T, T ? th8 + (8 - T) : nullptr, nullptr);
            expect(all_finite(o.mass) && all_finite(o.mean) && all_finite(o.sq), "unweighted run is finite", row++);
            bool top = true, mono = true;
            for (int i = 0; i < m && T; ++i) {
                top = top && fabsf(o.mass[(size_t)(T - 1) * m + i] - 1.f) < 1e-5f;        // the last threshold is pi: everything counts
                for (int t = 1; t < T; ++t) mono = mono && o.mass[(size_t)t * m + i] >= o.mass[(size_t)(t - 1) * m + i];
            }
            expect(top && mono, "the mass reaches 1 at pi and does not decrease", row++);
            if (T) {
                std::vector<float> mass((size_t)T * m, -1.f);                             // null outputs are not written
                sac::host_set_angle_cdf(C.data(), Q.data(), nullptr, n, m, K, 1, false, T, th8 + (8 - T), nullptr, mass.data(), nullptr, nullptr);
                expect(mass == o.mass, "the masses alone, the same values", row++);
            }
            // members reversed and padded with NaN and inf members in between: the same bits
            const int K2 = 2 * K + 1;
            std::vector<float> P((size_t)m * K2 * 9, NAN);
            for (int i = 0; i < m; ++i)
                for (int s = 0; s < K; ++s) {
                    std::copy(Q.begin() + ((size_t)i * K + s) * 9, Q.begin() + ((size_t)i * K + s + 1) * 9, P.begin() + ((size_t)i * K2 + 2 * (K - 1 - s) + 1) * 9);
                    P[((size_t)i * K2 + 2 * s) * 9 + 4] = s % 2 ? INFINITY : 0.f;         // one entry of a padding member suffices
                }
            expect(run(C, P, nullptr, n, m, K2, 1, false, T, T ? th8 + (8 - T) : nullptr, nullptr) == o, "padding and order do not change a bit", row++);
        }
        if (K == 1) {                                                                     // one member: rnf_so3_angle_cdf's evaluator
            Out a(1, 8, m);
            ac::host_angle_cdf(C.data(), Q.data(), nullptr, n, m, 1, false, 8, th8, nullptr, a.mass.data(), a.mean.data(), a.sq.data());
            expect(run(C, Q, nullptr, n, m, 1, 1, false, 8, th8, nullptr) == a, "K = 1 is the single-query evaluator", row++);
        }
    }
    {                                                                                     // three groups: plain, half -inf, all -inf
        const int n = 4099, m = 9, K = 5, G = 3, T = 8;
        std::vector<float> C = rotations(n, 0.37, 0.11), Q = rotations(m * K, 0.53, 0.29), lw((size_t)G * n);
        for (int j = 0; j < n; ++j) {
            lw[j] = (float)(2.0 * sin(0.7 * j));
            lw[n + j] = j % 2 ? -INFINITY : (float)cos(0.3 * j);
            lw[2 * n + j] = -INFINITY;
        }
        for (int j = 1; j < n; j += 2) C[9 * (size_t)j + 4] = j % 4 == 1 ? NAN : INFINITY;    // the dead centres of group 1 are not finite
        for (int s = 0; s < K; ++s) Q[((size_t)4 * K + s) * 9 + s] = NAN;                 // set 4 is padding only
        Q[((size_t)6 * K + 2) * 9] = INFINITY;                                            // set 6 has one padding member
        const Out o = run(C, Q, lw.data(), n, m, K, G, false, T, th8, nullptr);
        bool g0 = true, g1 = true, g2 = true;
        for (int i = 0; i < m; ++i) {
            g0 = g0 && nan_at(o.mean, i) && nan_at(o.mass, i);
            g1 = g1 && (i == 4 ? nan_at(o.mean, m + i) && nan_at(o.sq, m + i) && nan_at(o.mass, ((size_t)T + 3) * m + i)
                               : !nan_at(o.mean, m + i) && !nan_at(o.mass, ((size_t)T + 3) * m + i));
            g2 = g2 && nan_at(o.mean, 2 * m + i);
        }
        expect(g0, "a non-finite centre with a finite weight makes the group NaN", row++);
        expect(g1, "-inf weights leave non-finite centres out; a set of padding only is NaN, alone", row++);
        expect(g2, "all weights -inf is NaN", row++);
        std::vector<float> Qg((size_t)G * m * K * 9);                                     // sets per group: group g's are the shared ones
        for (int g = 0; g < G; ++g) std::copy(Q.begin(), Q.end(), Qg.begin() + (size_t)g * m * K * 9);
        const Out p = run(C, Qg, lw.data(), n, m, K, G, true, T, th8, nullptr);
        bool same = true;
        for (int i = 0; i < m; ++i)
            if (i != 4) same = same && p.mean[m + i] == o.mean[m + i] && p.mass[((size_t)T + 2) * m + i] == o.mass[((size_t)T + 2) * m + i];
        expect(same, "sets per group equal shared sets", row++);
        std::vector<float> tau((size_t)G * T * m);                                        // the same thresholds, per (group, set)
        for (int g = 0; g < G; ++g)
            for (int t = 0; t < T; ++t)
                for (int i = 0; i < m; ++i) tau[((size_t)g * T + t) * m + i] = ac::tau_of(th8[t]);
        tau[((size_t)1 * T + 2) * m + 7] = NAN;
        tau[((size_t)1 * T + 3) * m + 7] = -1.f;
        const Out r = run(C, Qg, lw.data(), n, m, K, G, true, T, nullptr, tau.data());
        same = true;
        for (int t = 0; t < T; ++t)
            for (int i = 0; i < m; ++i) {
                const size_t at = ((size_t)1 * T + t) * m + i;
                if (i == 4) same = same && nan_at(r.mass, at);
                else if (i == 7 && t == 2) same = same && nan_at(r.mass, at);
                else if (i == 7 && t == 3) same = same && r.mass[at] == 0.f;
                else same = same && r.mass[at] == p.mass[at];
            }
        expect(same, "thresholds per set: the shared ones' bits, a NaN slot alone is NaN, a negative one 0", row++);
    }
    {                                                                                     // half-turns about x, y, z seen from {identity, Rx(pi)}
        const std::vector<float> C = {1, 0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0, 0, 1, 0, 0, 0, -1, -1, 0, 0, 0, -1, 0, 0, 0, 1};
        const std::vector<float> Q = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, -1, 0, 0, 0, -1};
        const double th[2] = {3.0, PI};
        const Out o = run(C, Q, nullptr, 3, 1, 2, 1, false, 2, th, nullptr);
        expect(fabsf(o.mass[0] - 1.f / 3.f) < 1e-6f && fabsf(o.mass[1] - 1.f) < 1e-6f && fabsf(o.mean[0] - (float)(2 * PI / 3)) < 1e-6f,
               "three half-turns against a set that holds one of them", row++);
    }
    expect(ac::carve(nullptr, 4097, 10, 3, 10).bytes == ((8ull * 3 * 10 * 2 * 10 + 16 * 3 * 2 + 8 * 3 + 4ull * 3 * 4097 + 15) & ~15ull), "workspace rule", row++);
    {
        std::vector<char> ws(ac::carve(nullptr, 65, 3, 2, 4).bytes);
        const ac::Workspace w = ac::carve(ws.data(), 65, 3, 2, 4);
        expect((char *)w.psum == ws.data() && (char *)w.wn + 4 * 2 * 65 <= ws.data() + ws.size() && (char *)w.wpart == ws.data() + 8 * 2 * 4 * 1 * 3,
               "the carved parts lie inside the workspace", row++);
    }
    expect(sac::groups_for(6) == 4 && sac::groups_for(10) == 2 && sac::MAX_K == 4096, "kernel choice", row++);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
