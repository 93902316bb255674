// Stand-alone program over the anisotropic variant of csrc/so3_grid_local.h for a host sanitizer build
// (tests/test_so3_grid_local_fisher_host.py compiles its host code with the address and undefined-behaviour sanitizers and runs it as a
// process of its own): the enumerations of levels 0 to 2 at the cuts 0, one spacing, 15 and 60 degrees and 8, the concentrations 64 I,
// V diag(200, 5, 5) V^T, V diag(40, 12, -3) V^T, 1e4 I and 0, the sum and the max-plus pass, for the grid rows (every fortieth at level 2, where the max-plus pass runs on one concentration),
// the rows of a shifted grid, the poles, rotations next to phi = 0 and tilt 0, non-finite and oversized queries, with and without an
// offset; then the refusals of a concentration.  Exit code 0 and "ok" when every run comes back as expected.
#include <cstdio>
#include <vector>

#define RNF_SGL_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/so3_grid_local.h"

using namespace rnf;

static int g_bad = 0;
static void expect(bool ok, const char *what, int row) {
    if (!ok) {
        std::printf("FAILED: %s (case %d)\n", what, row);
        ++g_bad;
    }
}

// Rx(phi) Rz(theta) Rx(tau) O, one rounding per entry
static void euler_row(double phi, double theta, double tau, const double *o, float *dst) {
    const double z = cos(theta), s = sin(theta), cp = cos(phi), sp = sin(phi), ct = cos(tau), st = sin(tau);
    const double a[9] = {z, -s * ct, s * st, cp * s, cp * z * ct - sp * st, -cp * z * st - sp * ct, sp * s, sp * z * ct + cp * st, -sp * z * st + cp * ct};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) dst[3 * r + c] = (float)(a[3 * r] * o[c] + a[3 * r + 1] * o[3 + c] + a[3 * r + 2] * o[6 + c]);
}

static std::vector<float> make_grid(int level, const double *o) {
    const sgl::Geometry ge = sgl::geometry_of(level, 0.0, 0.0);
    std::vector<float> grid(9 * (size_t)sgl::rows_of(level));
    for (int i = 1; i <= 4 * ge.nside - 1; ++i) {
        float z, s, shift;
        int pixels, first;
        sgl::ring_of(ge, i, z, s, pixels, first, shift);
        const int k = i < ge.nside ? i : i > 3 * ge.nside ? 4 * ge.nside - i : 0;          // the colatitude again, in fp64
        const double tmp = (double)(k * k) / (3.0 * ge.nside * ge.nside);
        const double zz = k ? (i < ge.nside ? 1.0 - tmp : tmp - 1.0) : (double)(2 * ge.nside - i) * 2.0 / (3.0 * ge.nside);
        for (int j = 0; j < pixels; ++j)
            for (int t = 0; t < ge.ntilt; ++t)
                euler_row(((double)j + shift) * 2.0 * M_PI / pixels, acos(zz), 2.0 * M_PI * t / ge.ntilt, o,
                          &grid[9 * ((size_t)t * ge.npix + first + j)]);
    }
    return grid;
}

int main() {
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double off[9], V[9], shift[9];
    {
        float f[9];
        euler_row(0.7, 1.1, 2.3, eye, f);
        for (int k = 0; k < 9; ++k) off[k] = f[k];
        euler_row(2.1, 0.6, 4.0, eye, f);
        for (int k = 0; k < 9; ++k) V[k] = f[k];
        euler_row(0.05, 0.17, 0.02, eye, f);                                                // a drift of about 11 degrees
        for (int k = 0; k < 9; ++k) shift[k] = f[k];
    }
    const double spectra[5][3] = {{64, 64, 64}, {200, 5, 5}, {40, 12, -3}, {1e4, 1e4, 1e4}, {0, 0, 0}};
    double Ks[5][9];
    for (int a = 0; a < 5; ++a)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double v = 0.0;
                for (int k = 0; k < 3; ++k) v += V[3 * i + k] * spectra[a][k] * V[3 * j + k];
                Ks[a][3 * i + j] = v;
            }
    for (int a = 0; a < 5; ++a)                                                             // symmetric to the last bit
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < i; ++j) Ks[a][3 * i + j] = Ks[a][3 * j + i];
    int row = 0;
    for (int level = 0; level <= 2; ++level)
        for (int with_offset = 0; with_offset < 2; ++with_offset) {
            const double *o = with_offset ? off : eye;
            float of[9];
            for (int k = 0; k < 9; ++k) of[k] = (float)o[k];
            const std::vector<float> grid = make_grid(level, o);
            const long long Q = sgl::rows_of(level);
            std::vector<float> queries;                                                    // grid rows, shifted rows, then the special ones
            const int stride = level < 2 ? 1 : 40;
            for (long long r = 0; r < Q; r += stride) queries.insert(queries.end(), &grid[9 * r], &grid[9 * r] + 9);
            const long long on_grid = (long long)queries.size() / 9;
            for (long long r = 0; r < Q; r += stride) {
                float c[9];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j)
                        c[3 * i + j] = (float)(grid[9 * r + 3 * i] * shift[j] + grid[9 * r + 3 * i + 1] * shift[3 + j] + grid[9 * r + 3 * i + 2] * shift[6 + j]);
                queries.insert(queries.end(), c, c + 9);
            }
            const double specials[][3] = {{0, 0, 0}, {0, 0, 0.3}, {0, M_PI, 0}, {0, M_PI, 3.0}, {0.004, 0.4, 1.0}, {2 * M_PI - 0.004, 0.84, 1.0},
                                          {2.0, 0.8410686705679303, 0.003}, {2.0, 2.3, 2 * M_PI - 0.003}, {1.0, 1.5707963, 5.0}};
            for (const auto &sp : specials) {
                float q[9];
                euler_row(sp[0], sp[1], sp[2], o, q);
                queries.insert(queries.end(), q, q + 9);
            }
            const long long m = (long long)queries.size() / 9;
            std::vector<float> lw(2 * (size_t)Q);
            for (long long j = 0; j < Q; ++j) {
                lw[j] = (float)(2.0 * sin(0.7 * j));
                lw[Q + j] = j % 3 ? (float)cos(0.3 * j) : -INFINITY;
            }
            const double spacing = 2.0 * M_PI / (6 << level);
            const double cuts[] = {0.0, 4.0 * (1.0 - cos(spacing)), 4.0 * (1.0 - cos(M_PI / 12)), 4.0 * (1.0 - cos(M_PI / 3)), 8.0};
            for (double cut : cuts)
                for (int a = 0; a < 5; ++a)
                    for (int with_arg = 0; with_arg < (level < 2 || a == 2 ? 2 : 1); ++with_arg) {
                        std::vector<float> out(2 * (size_t)m, -1.f);
                        std::vector<int> arg(2 * (size_t)m, -2), count((size_t)m, -1);
                        sgl::host_grid_local_fisher(level, with_offset ? of : nullptr, grid.data(), queries.data(), lw.data(), m, 2, Ks[a], cut,
                                                    out.data(), with_arg ? arg.data() : nullptr, count.data());
                        bool ok = true;
                        for (long long i = 0; i < m; ++i) {
                            ok = ok && count[i] >= (i < on_grid ? 1 : 0) && count[i] <= Q && out[i] == out[i] && out[m + i] == out[m + i];
                            ok = ok && (count[i] > 0) == (out[i] != -INFINITY);
                            if (with_arg) ok = ok && arg[i] >= -1 && arg[i] < Q && (arg[i] >= 0) == (out[i] != -INFINITY);
                            if (cut == 8.0) ok = ok && count[i] == Q;
                        }
                        expect(ok, "counts and values of a sweep", row++);
                        if (with_arg || (level == 2 && (a != 1 || cut == 8.0))) continue;
                        std::vector<float> all((size_t)Q, -1.f);
                        sgl::host_grid_local_fisher(level, with_offset ? of : nullptr, grid.data(), nullptr, nullptr, Q, 1, Ks[a], cut, all.data(),
                                                    nullptr, nullptr);
                        expect(all[0] == all[0] && all[Q - 1] != -INFINITY, "null queries, weights and count", row++);
                    }
            std::vector<float> bad(queries.begin(), queries.begin() + 27);
            bad[4] = NAN;
            bad[9 + 2] = INFINITY;
            for (int k = 0; k < 9; ++k) bad[18 + k] *= 1e18f;
            float out[3];
            int arg[3], count[3];
            sgl::host_grid_local_fisher(level, with_offset ? of : nullptr, grid.data(), bad.data(), nullptr, 3, 1, Ks[2], 8.0, out, arg, count);
            expect(out[0] != out[0] && out[1] != out[1] && out[2] == -INFINITY && !count[0] && !count[1] && !count[2] && arg[0] == -1 && arg[2] == -1,
                   "non-finite and huge queries", row++);
        }
    double K[9];
    for (int k = 0; k < 9; ++k) K[k] = Ks[2][k];
    expect(sgl::concentration_defect(K) == 0, "a proper concentration", row++);
    K[1] += 1e-3;
    expect(sgl::concentration_defect(K) == 2, "asymmetry", row++);
    K[1] = NAN;
    expect(sgl::concentration_defect(K) == 1, "a non-finite entry", row++);
    const double neg[9] = {5, 0, 0, 0, -2, 0, 0, 0, -2}, big[9] = {3.1e4, 0, 0, 0, 1, 0, 0, 0, 1};
    expect(sgl::concentration_defect(neg) == 3 && sgl::concentration_defect(big) == 4, "eigenvalues", row++);
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
