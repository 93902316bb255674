// Stand-alone program over csrc/grid_sample.h for a host sanitizer build (tests/test_grid_sample_host.py compiles its host code with the
// address and undefined-behaviour sanitizers and runs it as a process of its own): the exact cases of that file (flat rows drawn three
// times each, with holes, a single finite row, a ragged Q over many chunks, rows beyond 2^24), the chart at the poles, on every corner of
// row 0 and row Q - 1 and on rows and uniforms outside their range, and every degenerate image, with both methods, with and without jitter.
// Exit code 0 and "ok" when every run comes back as expected.
#include <cstdio>
#include <vector>

#define RNF_GSA_HOST_ONLY
#define RNF_SO3G_HOST_ONLY
#include "../../rotationnormflow_amd/csrc/grid_sample.h"

using namespace rnf;
typedef unsigned long long u64;

static int g_bad = 0;
static void expect(bool ok, const char *what, int row) {
    if (!ok) {
        std::printf("FAILED: %s (case %d)\n", what, row);
        ++g_bad;
    }
}

struct Draws {
    std::vector<long long> index;
    std::vector<u64> target, total;
    std::vector<float> rot;
};

static Draws sample(const std::vector<float> &lp, long long Q, int g, int level, long long n, int method, int jitter, u64 seed,
                    const float *offset = nullptr, long long draw_base = 0, long long total = -1, long long image_base = 0) {
    Draws d;
    d.index.assign((size_t)(g * n), -7);
    d.target.assign((size_t)(g * n), 7);
    d.total.assign((size_t)g, 7);
    if (level >= 0) d.rot.assign((size_t)(g * n * 9), -7.f);
    gsa::host_grid_sample(lp.data(), Q, g, level, n, draw_base, total < 0 ? n : total, image_base, method, jitter, seed, offset, d.index.data(),
                          d.target.data(), d.total.data(), level >= 0 ? d.rot.data() : nullptr);
    return d;
}

static bool counts_are(const Draws &d, long long first, long long rows, long long stride, long long each) {
    std::vector<long long> c((size_t)rows, 0);
    for (long long i : d.index) {
        if (i < first || (i - first) % stride || (i - first) / stride >= rows) return false;
        ++c[(size_t)((i - first) / stride)];
    }
    for (long long v : c)
        if (v != each) return false;
    return true;
}

static bool is_rotation(const float *r) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += (double)r[3 * a + k] * r[3 * b + k];
            if (!(fabs(s - (a == b)) < 1e-6)) return false;
        }
    return true;
}

int main() {
    int row = 0;
    float off[9];
    {
        const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        gsa::euler_store(cos(1.1), sin(1.1), 0.7, 2.3, eye, off);
    }
    // the exact cases
    for (u64 seed : {1ULL, 0x8000000000003039ULL}) {
        const long long Q = 576;
        std::vector<float> flat((size_t)Q, 0.f), holes((size_t)Q, 0.f), one((size_t)Q, -INFINITY);
        for (long long i = 1; i < Q; i += 2) holes[(size_t)i] = -INFINITY;
        one[123] = -4.5f;
        expect(counts_are(sample(flat, Q, 1, 1, 3 * Q, gsa::SYSTEMATIC, 1, seed, off), 0, Q, 1, 3), "flat rows, three draws each", row++);
        expect(counts_are(sample(holes, Q, 1, 1, 3 * (Q / 2), gsa::SYSTEMATIC, 0, seed), 0, Q / 2, 2, 3), "every other row", row++);
        for (int method : {gsa::MULTINOMIAL, gsa::SYSTEMATIC})
            expect(counts_are(sample(one, Q, 1, 1, 500, method, 1, seed), 123, 1, 1, 500), "a single finite row", row++);
    }
    {
        const long long Q = 3 * 8192 + 17;
        expect(counts_are(sample(std::vector<float>((size_t)Q, 2.5f), Q, 1, -1, 3 * Q, gsa::SYSTEMATIC, 0, 5), 0, Q, 1, 3), "a ragged last chunk", row++);
        const Draws m = sample(std::vector<float>((size_t)Q, 2.5f), Q, 1, -1, 1000, gsa::MULTINOMIAL, 0, 5, nullptr, 500, 4000, 3);
        bool ok = m.total[0] == ((u64)Q << gc::fixed_point_shift(Q));
        for (size_t k = 0; k < m.index.size(); ++k) ok = ok && m.index[k] >= 0 && m.index[k] < Q && m.target[k] < m.total[0];
        expect(ok, "a tile of multinomial draws", row++);
    }
    {
        const long long Q = (1LL << 24) + 4099;
        std::vector<float> lp((size_t)Q, -INFINITY);
        for (long long i = Q - 5000; i < Q; ++i) lp[(size_t)i] = 1.f;
        expect(counts_are(sample(lp, Q, 1, -1, 15000, gsa::SYSTEMATIC, 0, 8), Q - 5000, 5000, 1, 3), "rows beyond 2^24", row++);
    }
    // the chart: every corner and the centre of row 0, row Q - 1 and the polar rows; rows and uniforms outside their range
    for (int level : {0, 1, 3, 6}) {
        const long long Q = 72LL << (3 * level), npix = Q / (6LL << level);
        const long long rows[] = {0, 1, 2, 3, npix - 4, npix - 1, Q - npix, Q - 1, Q / 2};
        for (long long r : rows)
            for (int c = 0; c < 9; ++c) {
                const float u[3] = {c == 8 ? 0.5f : (float)(c & 1), c == 8 ? 0.5f : (float)((c >> 1) & 1), c == 8 ? 0.5f : (float)((c >> 2) & 1)};
                float rot[9], centre[9];
                gsa::host_cell_points(level, c & 1 ? off : nullptr, &r, u, 1, rot);
                bool ok = is_rotation(rot);
                if (c == 8) {
                    gsa::host_grid_rows(level, nullptr, &r, 1, centre);
                    for (int k = 0; k < 9; ++k) ok = ok && fabsf(rot[k] - centre[k]) < 3e-7f;
                }
                expect(ok, "a chart corner or centre", row++);
            }
        const long long bad_rows[] = {-1, Q, 1LL << 40, 5, 5, 5, 5};
        float u[7 * 3], rot[7 * 9];
        for (float &v : u) v = 0.5f;
        u[3 * 3] = NAN;
        u[4 * 3 + 1] = INFINITY;
        u[5 * 3 + 2] = -1e-3f;
        gsa::host_cell_points(level, off, bad_rows, u, 7, rot);
        bool ok = true;
        for (int k = 0; k < 6 * 9; ++k) ok = ok && rot[k] != rot[k];
        expect(ok && is_rotation(rot + 6 * 9), "rows and uniforms outside their range", row++);
    }
    {
        const long long north[] = {0, 1, 2, 3}, south[] = {8, 9, 10, 11};
        const float un[12] = {1, 1, 0.5f, 1, 1, 0.5f, 1, 1, 0.5f, 1, 1, 0.5f}, us[12] = {0, 0, 0.5f, 0, 0, 0.5f, 0, 0, 0.5f, 0, 0, 0.5f};
        float rn[36], rs[36];
        gsa::host_cell_points(0, nullptr, north, un, 4, rn);
        gsa::host_cell_points(0, nullptr, south, us, 4, rs);
        bool ok = true;
        for (int k = 0; k < 4; ++k) ok = ok && rn[9 * k] == 1.f && rs[9 * k] == -1.f && is_rotation(rn + 9 * k) && is_rotation(rs + 9 * k);
        expect(ok, "the poles", row++);
    }
    // every degenerate image beside a regular one, both methods, with and without jitter
    {
        const long long Q = 576, n = 200;
        std::vector<float> lp((size_t)(5 * Q));
        for (long long i = 0; i < 5 * Q; ++i) lp[(size_t)i] = (float)(2.0 * sin(0.37 * (double)i));
        lp[(size_t)(Q + 17)] = NAN;
        lp[(size_t)(2 * Q + 40)] = INFINITY;
        for (long long i = 0; i < Q; ++i) lp[(size_t)(3 * Q + i)] = -INFINITY;
        for (int method : {gsa::MULTINOMIAL, gsa::SYSTEMATIC})
            for (int jitter : {0, 1}) {
                const Draws d = sample(lp, Q, 5, 1, n, method, jitter, 31, off);
                bool ok = true;
                for (int b = 0; b < 5; ++b) {
                    const bool dead = b >= 1 && b <= 3;
                    ok = ok && (d.total[(size_t)b] == 0) == dead;
                    for (long long k = 0; k < n; ++k) {
                        const size_t at = (size_t)(b * n + k);
                        ok = ok && (dead ? d.index[at] == -1 && d.target[at] == 0 && d.rot[9 * at] != d.rot[9 * at]
                                         : d.index[at] >= 0 && d.index[at] < Q && d.target[at] < d.total[(size_t)b] && is_rotation(&d.rot[9 * at]));
                    }
                }
                expect(ok, "degenerate images", row++);
            }
        const Draws none = sample(lp, Q, 5, 1, 0, gsa::SYSTEMATIC, 1, 31, off, 0, 10);
        expect(none.total[0] > 0 && none.total[3] == 0, "no draws, the totals alone", row++);
    }
    std::printf(g_bad ? "%d failures\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
