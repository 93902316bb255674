// Stand-alone program over csrc/so3_harmonics.h for a host sanitizer build (tests/test_so3_harmonics_host.py compiles its host code
// with the address and undefined-behaviour sanitizers and runs it as a process of its own): ragged sizes across the tile and chunk
// boundaries, L = 0 and 16 and between, -inf weights, NaN rows, queries per group, non-finite coefficients.  Exit code 0 and "ok" when
// every run comes back as expected.
#include <algorithm>
#include <cstdio>
#include <vector>

#define RNF_SH_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_harmonics.h"

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

int main() {
    int row = 0;
    for (int L : {0, 1, 5, 8, 9, 16}) {                                                    // the matrices: orthogonal rows, D^0 = 1
        const int n = 7, CL = sh::coefficient_count(L);
        const std::vector<float> R = rotations(n, 0.37, 0.11);
        std::vector<float> D((size_t)n * CL, -7.f);
        sh::host_wigner(R.data(), n, L, D.data());
        bool ok = all_finite(D.data(), D.size());
        for (int i = 0; i < n && ok; ++i) {
            ok = fabsf(D[(size_t)i * CL] - 1.f) < 1e-6f;
            for (int l = 0; l <= L && ok; ++l) {
                const float *b = &D[(size_t)i * CL + sh::degree_offset(l)];
                const int W = 2 * l + 1;
                for (int r = 0; r < W && ok; ++r) {
                    double s = 0;
                    for (int c = 0; c < W; ++c) s += (double)b[r * W + c] * b[r * W + c];
                    ok = fabs(s - 1.0) < 1e-4;
                }
            }
        }
        expect(ok, "matrices: finite, D^0 = 1, unit rows", row++);
    }
    const int sizes[] = {1, 63, 65, 4097};                                                 // ragged across the tile and the chunk
    for (int n : sizes)
        for (int L : {0, 7, 16}) {
            const int CL = sh::coefficient_count(L);
            const std::vector<float> C = rotations(n, 0.37, 0.11);
            std::vector<float> F((size_t)CL, -7.f);
            sh::host_fourier(C.data(), nullptr, n, 1, L, F.data());
            expect(all_finite(F.data(), F.size()) && fabsf(F[0] - 1.f) < 1e-5f, "unweighted analysis is finite, F^0 = 1", row++);
            std::vector<float> f(5, -7.f);
            const std::vector<float> Q = rotations(5, 0.53, 0.29);
            sh::host_fourier_eval(F.data(), Q.data(), 5, 1, false, L, f.data());
            expect(all_finite(f.data(), f.size()), "synthesis of it is finite", row++);
        }
    {                                                                                     // three groups: plain, half -inf, all -inf
        const int n = 4099, G = 3, L = 8, CL = sh::coefficient_count(L), m = 70;
        std::vector<float> C = rotations(n, 0.37, 0.11), lw((size_t)G * n);
        for (int j = 0; j < n; ++j) {
            lw[j] = (float)(2.0 * sin(0.7 * j));
            lw[n + j] = j % 2 ? -INFINITY : (float)cos(0.3 * j);
            lw[2 * n + j] = -INFINITY;
        }
        for (int j = 1; j < n; j += 2) C[9 * (size_t)j + 4] = j % 4 == 1 ? NAN : INFINITY;    // the dead centres of group 1 are not finite
        std::vector<float> F((size_t)G * CL, -7.f);
        sh::host_fourier(C.data(), lw.data(), n, G, L, F.data());
        expect(all_nan(&F[0], CL), "a non-finite centre with a finite weight makes the group NaN", row++);
        expect(all_finite(&F[CL], CL) && fabsf(F[CL] - 1.f) < 1e-5f, "-inf weights leave non-finite centres out", row++);
        expect(all_nan(&F[2 * (size_t)CL], CL), "all weights -inf is NaN", row++);
        std::vector<float> one((size_t)CL, -7.f);
        sh::host_fourier(C.data(), lw.data() + n, n, 1, L, one.data());
        expect(std::equal(one.begin(), one.end(), F.begin() + CL), "a group alone has the same bits", row++);
        std::vector<float> nanw(lw.begin(), lw.begin() + n), Cok = rotations(n, 0.37, 0.11);
        nanw[4098] = NAN;
        sh::host_fourier(Cok.data(), nanw.data(), n, 1, L, one.data());
        expect(all_nan(one.data(), CL), "a NaN log-weight makes the group NaN", row++);

        std::vector<float> Q = rotations(m, 0.53, 0.29), Qg((size_t)G * m * 9), f((size_t)G * m, -7.f), fg((size_t)G * m, -7.f);
        for (int g = 0; g < G; ++g) std::copy(Q.begin(), Q.end(), Qg.begin() + (size_t)g * m * 9);
        sh::host_fourier_eval(F.data(), Q.data(), m, G, false, L, f.data());
        sh::host_fourier_eval(F.data(), Qg.data(), m, G, true, L, fg.data());
        expect(all_nan(&f[0], m) && all_finite(&f[m], m) && all_nan(&f[2 * (size_t)m], m), "non-finite coefficients stay in their group", row++);
        expect(std::equal(f.begin() + m, f.begin() + 2 * m, fg.begin() + m), "queries per group equal shared queries", row++);
        Q[9 * 7 + 2] = INFINITY;
        sh::host_fourier_eval(F.data() + CL, Q.data(), m, 1, false, L, f.data());
        expect(f[7] != f[7] && f[6] == fg[m + 6] && f[8] == fg[m + 8], "a non-finite query alone is NaN", row++);
    }
    {                                                                                     // half-turns and the identity: a = 0 or b = 0
        const float R[36] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0, 0, 1, 0, 0, 0, -1, -1, 0, 0, 0, -1, 0, 0, 0, 1};
        const int L = 16, CL = sh::coefficient_count(L);
        std::vector<float> D(4 * (size_t)CL);
        sh::host_wigner(R, 4, L, D.data());
        bool ok = all_finite(D.data(), D.size());
        for (int l = 0; l <= L && ok; ++l)
            for (int r = 0; r < 2 * l + 1 && ok; ++r)
                for (int c = 0; c < 2 * l + 1 && ok; ++c) ok = fabsf(D[sh::degree_offset(l) + r * (2 * l + 1) + c] - (r == c ? 1.f : 0.f)) < 2e-5f;
        expect(ok, "the identity's matrices are the identity", row++);
        for (int i = 1; i < 4 && ok; ++i)
            for (int k = 0; k < CL && ok; ++k) ok = fabsf(fabsf(fabsf(D[(size_t)i * CL + k]) - 0.5f) - 0.5f) < 2e-5f;     // a signed permutation
        expect(ok, "a half-turn about an axis has entries 0 and +-1", row++);
    }
    expect(sh::carve(nullptr, 4097, 3, 8).bytes ==
               ((8ull * 3 * 2 * 969 + 16 * 3 * 2 + 8 * 3 + 4ull * 3 * 4097 + 15) & ~15ull) + 4ull * 4097 * 80 + ((4ull * 289 * 34 + 15) & ~15ull),
           "workspace rule", row++);
    expect(sh::coefficient_count(8) == 969 && sh::coefficient_count(16) == 6545 && sh::degree_offset(17) == 6545 && sh::groups_per_thread(8) == 4 &&
               sh::groups_per_thread(9) == 2,
           "layout", row++);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
