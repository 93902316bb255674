// Stand-alone program over csrc/so3_grid_local.h's max-plus pass for a host sanitizer build (tests/test_so3_grid_viterbi_host.py compiles
// its host code with the address and undefined-behaviour sanitizers and runs it as a process of its own): host_grid_local_max at levels
// 0 to 2 at the cuts 0, half a spacing, one spacing, 15, 60 and 180 degrees and 8, for the grid rows (every fifth at level 2), the two
// poles, rotations next to phi = 0 and tilt 0, non-finite and oversized queries, with and without an offset, with -inf and NaN
// log-weights.  Exit code 0 and "ok" when every run comes back as expected.
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
    double off[9];
    {
        float f[9];
        euler_row(0.7, 1.1, 2.3, eye, f);
        for (int k = 0; k < 9; ++k) off[k] = f[k];
    }
    int row = 0;
    for (int level = 0; level <= 2; ++level)
        for (int with_offset = 0; with_offset < 2; ++with_offset) {
            const double *o = with_offset ? off : eye;
            float of[9];
            for (int k = 0; k < 9; ++k) of[k] = (float)o[k];
            const std::vector<float> grid = make_grid(level, o);
            const long long Q = sgl::rows_of(level);
            std::vector<float> queries;                                                    // grid rows (every fifth at level 2), then the special ones
            std::vector<long long> own;                                                    // the grid row a query is, or -1
            for (long long r = 0; r < Q; r += level < 2 ? 1 : 5) {
                queries.insert(queries.end(), &grid[9 * r], &grid[9 * r] + 9);
                own.push_back(r);
            }
            const double specials[][3] = {{0, 0, 0}, {0, 0, 0.3}, {0, M_PI, 0}, {0, M_PI, 3.0}, {0.004, 0.4, 1.0}, {2 * M_PI - 0.004, 0.84, 1.0},
                                          {2.0, 0.8410686705679303, 0.003}, {2.0, 2.3, 2 * M_PI - 0.003}, {1.0, 1.5707963, 5.0}};
            for (const auto &sp : specials) {
                float q[9];
                euler_row(sp[0], sp[1], sp[2], o, q);
                queries.insert(queries.end(), q, q + 9);
                own.push_back(-1);
            }
            const long long m = (long long)queries.size() / 9;
            std::vector<float> lw(3 * (size_t)Q);                                           // zeros; a third of the rows at -inf; one NaN
            for (long long j = 0; j < Q; ++j) {
                lw[j] = 0.f;
                lw[Q + j] = j % 3 ? (float)cos(0.3 * j) : -INFINITY;
                lw[2 * Q + j] = j == Q / 2 ? NAN : (float)(2.0 * sin(0.7 * j));
            }
            const double spacing = 2.0 * M_PI / (6 << level);
            const double cuts[] = {0.0, 2.0 * (1.0 - cos(0.5 * spacing)), 4.0 * (1.0 - cos(spacing)), 4.0 * (1.0 - cos(M_PI / 12)),
                                   4.0 * (1.0 - cos(M_PI / 3)), 4.0 * (1.0 - cos(M_PI)), 8.0};
            for (double cut : cuts)
                for (double kappa : {0.0, 64.0, 1e4}) {
                    std::vector<float> out(3 * (size_t)m, -1.f);
                    std::vector<int> arg(3 * (size_t)m, -7), count((size_t)m, -1);
                    sgl::host_grid_local_max(level, with_offset ? of : nullptr, grid.data(), queries.data(), lw.data(), m, 3, kappa, cut, out.data(),
                                             arg.data(), count.data());
                    bool ok = true;
                    for (long long i = 0; i < m; ++i) {
                        ok = ok && count[i] >= (own[i] >= 0 ? 1 : 0) && count[i] <= Q;
                        for (int g = 0; g < 3; ++g) {
                            const float v = out[g * m + i];
                            const int a = arg[g * m + i];
                            ok = ok && a >= -1 && a < Q && (a >= 0) == (v == v && v != -INFINITY);
                            if (a >= 0) ok = ok && lw[g * Q + a] == lw[g * Q + a] && lw[g * Q + a] != -INFINITY;    // a live row
                            if (g < 2) ok = ok && v == v;
                        }
                        ok = ok && (count[i] > 0) == (arg[i] >= 0);
                        if (own[i] >= 0 && kappa > 0.0) ok = ok && arg[i] == own[i];         // zero weights: a grid row's own row is nearest
                        if (kappa == 0.0 && cut == 8.0) ok = ok && arg[i] == 0 && out[2 * m + i] != out[2 * m + i];      // every row ties: the smallest
                        if (cut == 8.0) ok = ok && count[i] == Q;
                    }
                    expect(ok, "values, args and counts of a sweep", row++);
                    if (level == 2 && kappa != 64.0) continue;                             // every row of level 2 once per cut
                    std::vector<float> all((size_t)Q, -1.f);
                    std::vector<int> at((size_t)Q, -7);
                    sgl::host_grid_local_max(level, with_offset ? of : nullptr, grid.data(), nullptr, nullptr, Q, 1, kappa, cut, all.data(), at.data(),
                                             nullptr);
                    expect(all[0] == all[0] && at[0] == 0 && (kappa == 0.0 || at[Q - 1] == Q - 1), "null queries, weights and count", row++);
                }
            std::vector<float> bad(queries.begin(), queries.begin() + 27);
            bad[4] = NAN;
            bad[9 + 2] = INFINITY;
            for (int k = 0; k < 9; ++k) bad[18 + k] *= 1e18f;
            float out[3];
            int arg[3], count[3];
            sgl::host_grid_local_max(level, with_offset ? of : nullptr, grid.data(), bad.data(), nullptr, 3, 1, 4.0, 8.0, out, arg, count);
            expect(out[0] != out[0] && out[1] != out[1] && out[2] == -INFINITY && !count[0] && !count[1] && !count[2] && arg[0] == -1 &&
                       arg[1] == -1 && arg[2] == -1,
                   "non-finite and huge queries", row++);
        }
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
