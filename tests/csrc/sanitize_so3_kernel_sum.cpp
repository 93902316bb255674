// Stand-alone program over csrc/so3_kernel_sum.h for a host sanitizer build (tests/test_so3_kde_host.py compiles its host code with the
// address and undefined-behaviour sanitizers and runs it as a process of its own): ragged sizes across the tile and chunk boundaries,
// -inf weights, NaN rows, leave-one-out down to n = 1.  Exit code 0 and "ok" when every run comes back as expected.
#include <cstdio>
#include <vector>

#define RNF_KS_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_kernel_sum.h"

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
static bool all_nan(const float *v, size_t k) {
    for (size_t i = 0; i < k; ++i)
        if (v[i] == v[i]) return false;
    return true;
}

int main() {
    const double kap8[8] = {0.0, 1.0, 4.0, 16.0, 64.0, 256.0, 1e4, 1e6};
    const int sizes[][2] = {{1, 1}, {63, 5}, {65, 257}, {4097, 3}};                       // ragged across tiles, blocks and the chunk
    int row = 0;
    for (const auto &sz : sizes) {
        const int n = sz[0], m = sz[1];
        const std::vector<float> C = rotations(n, 0.37, 0.11), Q = rotations(m, 0.53, 0.29);
        for (int J : {1, 3, 8}) {
            std::vector<float> out((size_t)J * m, -1.f);
            ks::host_kernel_sum(C.data(), Q.data(), nullptr, n, m, 1, kap8 + (8 - J), J, false, out.data());
            expect(all_finite(out), "unweighted run is finite", row++);
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
        for (int j = 1; j < n; j += 2) C[9 * (size_t)j + 4] = NAN;                        // the dead centres of group 1 hold NaNs: group 0 is NaN
        std::vector<float> out((size_t)G * 2 * m);
        ks::host_kernel_sum(C.data(), Q.data(), lw.data(), n, m, G, kap8 + 3, 2, false, out.data());
        expect(all_nan(out.data(), 2 * m), "a NaN centre with a finite weight makes the group NaN", row++);
        expect(all_finite(std::vector<float>(out.begin() + 2 * m, out.begin() + 4 * m)), "-inf weights leave NaN centres out", row++);
        expect(all_nan(out.data() + 4 * m, 2 * m), "all weights -inf is NaN", row++);
        std::vector<float> Qn = Q;
        Qn[9 * 7 + 2] = INFINITY;
        ks::host_kernel_sum(C.data(), Qn.data(), lw.data() + n, n, m, 1, kap8 + 3, 2, false, out.data());
        expect(out[7] != out[7] && out[m + 7] != out[m + 7] && out[6] == out[6] && out[8] == out[8], "a non-finite query alone is NaN", row++);
        std::vector<float> nanw(lw.begin(), lw.begin() + n);
        nanw[4098] = NAN;
        std::vector<float> Cok = rotations(n, 0.37, 0.11);
        ks::host_kernel_sum(Cok.data(), Q.data(), nanw.data(), n, m, 1, kap8 + 3, 2, false, out.data());
        expect(all_nan(out.data(), 2 * m), "a NaN log-weight makes the group NaN", row++);
    }
    for (int n : {1, 2, 65, 4097}) {                                                      // leave-one-out
        const std::vector<float> C = rotations(n, 0.37, 0.11);
        const int J = n > 100 ? 2 : 8;                                                    // the pairs grow as n^2
        std::vector<float> out((size_t)J * n), lw(n);
        for (int j = 0; j < n; ++j) lw[j] = (float)sin(0.9 * j);
        ks::host_kernel_sum(C.data(), nullptr, nullptr, n, n, 1, kap8, J, true, out.data());
        expect(n == 1 ? all_nan(out.data(), out.size()) : all_finite(out), "leave-one-out", row++);
        ks::host_kernel_sum(C.data(), nullptr, lw.data(), n, n, 1, kap8, J, true, out.data());
        expect(n == 1 ? all_nan(out.data(), out.size()) : all_finite(out), "weighted leave-one-out", row++);
    }
    expect(ks::carve(nullptr, 4097, 10, 3, 2).bytes == ((12ull * 3 * 2 * 2 * 10 + 16 * 3 * 2 + 8 * 3 + 15) & ~15ull), "workspace rule", row++);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
