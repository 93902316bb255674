// so3_harmonics.h -- harmonic analysis on SO(3): the real Wigner matrices D^l(R) of rotations (rnf_so3_wigner), the Fourier
// coefficients of a weighted set of rotations (rnf_so3_fourier) and the evaluation of a band-limited function at rotations
// (rnf_so3_fourier_eval), include/rnf_hip.h.  DESIGN.md 3.3i has the definitions; in short:
//
// Basis.  Y_l(x): the 2l+1 orthonormal real spherical harmonics of degree l, m = -l..l: sqrt2 (-1)^m Re Y_l^m for m > 0,
// sqrt2 (-1)^m Im Y_l^|m| for m < 0, Y_l^0 for m = 0 (Condon-Shortley Y_l^m; for l = 1 the order is y, z, x).  D^l(R) is the real
// orthogonal matrix with Y_l(R x) = D^l(R) Y_l(x).  Layout: degrees 0..L one after the other, each row-major with m' (row) and m
// (column) from -l to l; degree l starts at l (4 l^2 - 1) / 3, C_L = (L + 1)(2L + 1)(2L + 3) / 3 entries in all, L <= MAX_DEGREE = 16.
//
// The row function.  No Euler angles, hence no singular chart.  A 3x3 row is read through its unit quaternion (w, x, y, z) -- the
// largest of the four candidates about the row's own scale |R|_F / sqrt3 (so that s R gives R's), refined by one multiplication by
// the matrix whose dominant eigenvector is the quaternion of the nearest rotation, in fp64 -- and the Cayley-Klein pair
// a = w + iz, b = y - ix.  In the complex basis Y_l^m(R x) = sum D_c[m'][m] Y_l^m'(x) has
//     D_c[m'][m] = (-1)^max(m'-m, 0) sqrt(C(2 l0, |m'-m|)) (a or conj a)^|m'+m| (b or conj b)^|m'-m|          at l = l0 = max(|m'|, |m|)
// (conj where the exponent's sign is negative), and from there the three-term recurrence of the Wigner d functions in l,
//     D_c^l = (c1 X + c2) D_c^(l-1) - c3 D_c^(l-2),  X = |a|^2 - |b|^2,  c1 = (2l-1) l / den,  c2 = -(2l-1) m m' / ((l-1) den),
//     c3 = l sqrt(((l-1)^2 - m'^2)((l-1)^2 - m^2)) / ((l-1) den),  den = sqrt((l^2 - m'^2)(l^2 - m^2)),
// whose coefficients are real: it runs on real and imaginary parts alone.  X = cos(beta) is never formed: near X = +-1 the entries
// are smooth in the rotation but steep in X (P_l'(1) = l (l+1) / 2), and an fp32 X cannot come closer to 1 than 2^-24.  The recurrence
// takes y = 2 min(|a|^2, |b|^2) = 1 -+ X in [0, 1], small with a small error where X is near +-1:  c1 X + c2 = (c1 + c2) - c1 y on
// the side X = 1 - y and -((c1 - c2) - c1 y) on the side X = y - 1, with c1 + c2 and c1 - c2 formed in fp64 in the record.  The
// quaternion is normalised in fp64 and rounded once per component.  With mu = |m'|, nu = |m|, X = D_c[mu][nu], Y = D_c[mu][-nu]
// the real entry (m', m) is cx P(X) + cy P(Y): P = Im where exactly one of m', m is negative, else Re; see entry_record for the
// signs.  So an entry is the sum of TWO real sequences u_l, v_l with seeds from four complex powers a^(mu+nu), b^(mu+nu), a^|mu-nu|,
// b^|mu-nu| and constants that depend on (m', m, l) alone: an ENTRY RECORD (seedX, seedY; c1, c1 + c2, c1 - c2, c3 per degree), formed in fp64 and
// rounded once, the same bits on the host and on the device.  Every entry is a polynomial of even degree in q: q and -q agree.
//
// Kernels.
//   records   one thread per (m', m): the entry records [(2L+1)^2][2 + 4L] into the workspace (every call builds its own: no state).
//   wigner    one thread per rotation walks the entries with its powers kept up by single multiplications (walk_entries) -> [n][C_L].
//   analysis  F_g = sum_j w_gj D(C_j): a [G, n] x [n, C_L] product whose right factor is made on the fly.  A prepass writes each
//             centre's power table a^k, b^k (k <= 2L), y and its side; the normalised weights wn are so3_angle_cdf.h's.  In the hot kernel a thread
//             owns one (m', m) for all its degrees and GB groups in registers; the centre index is wave-uniform (its weights, y and side
//             arrive by scalar loads, its four powers by one load each from the centre's row).
//   synthesis f_gi = sum c_g . D(Q_i): a thread owns one query and GB groups, walks the entries like wigner with the coefficients
//             wave-uniform (scalar loads), adds an entry's degrees in fp32 (at most 17 terms) and the entries in fp64, in walk order.
//
// Determinism (analysis): the chunks of so3_kernel_sum.h.  fp64 over the centres of a chunk of 4096 (a function of n alone) in centre
// order, each term the exact product of its two fp32 factors; one fp64 partial per (group, chunk, coefficient), a finalise that adds
// the chunks in order and rounds once.
// No floating-point atomics.  A group's coefficients are bit-identical whatever G and the group's position are, and a coefficient's
// bits do not depend on L.  Synthesis: a (group, query)'s value is bit-identical however queries and groups are tiled.
//
// Edge cases.  A centre with lw = -inf is left out whatever its entries (a row that is not finite gets the table of a = b = 0: finite
// entries, times a weight of exactly 0); any other non-finite centre, or a NaN log-weight, makes its group NaN; a group without mass is
// NaN.  A non-finite query (or rotation of wigner) gives NaN for that row alone; non-finite coefficients stay in their group.
#pragma once
#if defined(RNF_SH_HOST_ONLY) && !defined(RNF_AC_HOST_ONLY)
#define RNF_AC_HOST_ONLY
#endif
#include "so3_angle_cdf.h"

namespace rnf {
namespace sh {

constexpr int MAX_DEGREE = 16;
constexpr long long MAX_N = ks::MAX_N, MAX_M = ks::MAX_M;
using ks::CHUNK;
using ks::THREADS;

RNF_FM_HD int degree_offset(int l) { return l * (4 * l * l - 1) / 3; }
RNF_FM_HD int coefficient_count(int L) { return (L + 1) * (2 * L + 1) * (2 * L + 3) / 3; }
RNF_FM_HD int entry_count(int L) { return (2 * L + 1) * (2 * L + 1); }
RNF_FM_HD int record_stride(int L) { return 2 + 4 * L; }                 // seedX, seedY, then (c1, c1 + c2, c1 - c2, c3) of l = 1..L
RNF_FM_HD int table_stride(int L) { return 8 * L + 16; }                 // (a^k, b^k) of k = 0..2L as four floats each, y, side, D^1, padding
RNF_FM_HD int coefficient_index(int l, int mp, int m) { return degree_offset(l) + (mp + l) * (2 * l + 1) + (m + l); }

// ---- the entry records -------------------------------------------------------------------------------------------------------------------

RNF_FM_HD double binomial(int n, int k) {
    double c = 1.0;
    for (int i = 1; i <= k; ++i) c = c * (double)(n - k + i) / (double)i;     // exact in fp64 for n <= 32: every partial is a binomial
    return c;
}

// The record of entry (mp, m) for degrees up to L: rec[0] = cx sgnX sqrt(C(2 l0, |mu - nu|)), rec[1] = cy sgnY sqrt(C(2 l0, mu + nu))
// and rec[2 + 4 (l - 1) ..] = c1, c1 + c2, c1 - c2, c3 of degree l (0 for l <= l0).  The real entry is
//     mu, nu > 0:  (+,+) e Re X + emu Re Y   (+,-) -e Im X + emu Im Y   (-,+) e Im X + emu Im Y   (-,-) e Re X - emu Re Y
//     nu = 0:      sqrt2 emu (Re X | Im X for m' < 0)       mu = 0:  sqrt2 enu (Re X | -Im X for m < 0)       (0, 0): X
// with e = (-1)^(mu + nu), emu = (-1)^mu, enu = (-1)^nu, and the signs of the seeds of X and Y are (-1)^max(mu - nu, 0) and e.
RNF_FM_HD void entry_record(int mp, int m, int L, float *rec) {
    const int mu = mp < 0 ? -mp : mp, nu = m < 0 ? -m : m, l0 = mu > nu ? mu : nu, d = mu > nu ? mu - nu : nu - mu;
    const double e = (mu + nu) & 1 ? -1.0 : 1.0, emu = mu & 1 ? -1.0 : 1.0, enu = nu & 1 ? -1.0 : 1.0, r2 = sqrt(2.0);
    double cx, cy = 0.0;
    if (mu > 0 && nu > 0) {
        cx = mp > 0 && m < 0 ? -e : e;
        cy = mp < 0 && m < 0 ? -emu : emu;
    } else if (mu > 0) {
        cx = r2 * emu;
    } else if (nu > 0) {
        cx = m > 0 ? r2 * enu : -r2 * enu;
    } else {
        cx = 1.0;
    }
    const double sgn_x = mu > nu && ((mu - nu) & 1) ? -1.0 : 1.0;
    rec[0] = (float)(cx * sgn_x * sqrt(binomial(2 * l0, d)));
    rec[1] = (float)(cy * e * sqrt(binomial(2 * l0, mu + nu)));
    for (int l = 1; l <= L; ++l) {
        float *c = rec + 2 + 4 * (l - 1);
        if (l <= l0) {
            c[0] = c[1] = c[2] = c[3] = 0.f;
            continue;
        }
        const double den = sqrt((double)(l * l - mu * mu) * (double)(l * l - nu * nu)), inv = l > 1 ? 1.0 / (double)(l - 1) : 0.0;
        const double c1 = (double)((2 * l - 1) * l) / den, c2 = -(double)((2 * l - 1) * mu * nu) * inv / den;
        c[0] = (float)c1;
        c[1] = (float)(c1 + c2);
        c[2] = (float)(c1 - c2);
        c[3] = (float)((double)l * sqrt((double)((l - 1) * (l - 1) - mu * mu) * (double)((l - 1) * (l - 1) - nu * nu)) * inv / den);
    }
}

// ---- a row -> its Cayley-Klein pair ------------------------------------------------------------------------------------------------------

struct CayleyKlein {                                                     // a = w + iz, b = y - ix
    float ar, ai, br, bi;
    float y;                                                             // 2 min(|a|^2, |b|^2) = 1 - |X|, X = |a|^2 - |b|^2 = cos(beta)
    bool neg;                                                            // X < 0: |a| < |b|
    float d1[9];                                                         // D^1: the rotation of the quaternion, formed in fp64, rows and columns (y, z, x)
};

// The unit quaternion of a row-major 3x3 row, from the four candidates about the row's own scale; zeros where the row is not finite
// or is zero
RNF_FM_HD CayleyKlein cayley_klein(const float *r) {
    CayleyKlein k = {0.f, 0.f, 0.f, 0.f, 0.f, false, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
    if (!ks::finite9(r)) return k;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) ss = fmaf(r[i], r[i], ss);
    const float s = sqrtf(ss * (1.f / 3.f));
    // M = K + s I, K the symmetric 4x4 matrix that is linear in the row and has the quaternion of the nearest rotation as its
    // dominant eigenvector (for s R: s (4 q q^T - I)); its rows are the four candidates.  The row of the largest diagonal entry, then
    // one multiplication by M, which takes in all nine entries: to first order in the row's rounding it is that eigenvector.
    const double sd = s, r0 = r[0], r4 = r[4], r8 = r[8];
    const double a = (double)r[7] - r[5], b = (double)r[2] - r[6], c = (double)r[3] - r[1];
    const double p = (double)r[1] + r[3], q = (double)r[2] + r[6], t = (double)r[5] + r[7];
    const double d0 = sd + r0 + r4 + r8, d1 = sd + r0 - r4 - r8, d2 = sd - r0 + r4 - r8, d3 = sd - r0 - r4 + r8;      // M's diagonal
    const int best = d0 >= d1 && d0 >= d2 && d0 >= d3 ? 0 : (d1 >= d2 && d1 >= d3 ? 1 : (d2 >= d3 ? 2 : 3));
    const double m0 = best == 0 ? d0 : (best == 1 ? a : (best == 2 ? b : c)), m1 = best == 0 ? a : (best == 1 ? d1 : (best == 2 ? p : q));
    const double m2 = best == 0 ? b : (best == 1 ? p : (best == 2 ? d2 : t)), m3 = best == 0 ? c : (best == 1 ? q : (best == 2 ? t : d3));
    const double wd = d0 * m0 + a * m1 + b * m2 + c * m3, xd = a * m0 + d1 * m1 + p * m2 + q * m3;
    const double yd = b * m0 + p * m1 + d2 * m2 + t * m3, zd = c * m0 + q * m1 + t * m2 + d3 * m3;
    const double n2 = wd * wd + xd * xd + yd * yd + zd * zd;
    if (!(n2 > 0.0)) return k;
    const double inv = 1.0 / sqrt(n2), a2 = (wd * wd + zd * zd) / n2, b2 = (xd * xd + yd * yd) / n2;
    k.ar = (float)(wd * inv); k.ai = (float)(zd * inv); k.br = (float)(yd * inv); k.bi = (float)(-xd * inv);
    k.neg = a2 < b2;
    k.y = (float)(2.0 * (k.neg ? a2 : b2));
    const double h = 2.0 / n2;                                           // R[i][j] of the quaternion; D^1[i][j] = R[p_i][p_j], p = (1, 2, 0)
    k.d1[0] = (float)(1.0 - h * (xd * xd + zd * zd)); k.d1[1] = (float)(h * (yd * zd - wd * xd)); k.d1[2] = (float)(h * (xd * yd + wd * zd));
    k.d1[3] = (float)(h * (yd * zd + wd * xd)); k.d1[4] = (float)(1.0 - h * (xd * xd + yd * yd)); k.d1[5] = (float)(h * (xd * zd - wd * yd));
    k.d1[6] = (float)(h * (xd * yd - wd * zd)); k.d1[7] = (float)(h * (xd * zd + wd * yd)); k.d1[8] = (float)(1.0 - h * (yd * yd + zd * zd));
    return k;
}

// (pr + i pi)(qr + i qi)
RNF_FM_HD void cmul(float pr, float pi, float qr, float qi, float &zr, float &zi) {
    zr = fmaf(-pi, qi, pr * qr);
    zi = fmaf(pr, qi, pi * qr);
}

// Re or Im of (pr + i pi)(dr + i di)
RNF_FM_HD float part_of(bool imag, float pr, float pi, float dr, float di) { return imag ? fmaf(pr, di, pi * dr) : fmaf(-pi, di, pr * dr); }

// The seeds u, v at l0 of entry (mp, m) from the four powers a^s, b^s (s = mu + nu), a^d, b^d (d = |mu - nu|) and its record
RNF_FM_HD void entry_seeds(int mp, int m, const float *rec, float asr, float asi, float bsr, float bsi, float adr, float adi, float bdr, float bdi,
                           float &u, float &v) {
    const int mu = mp < 0 ? -mp : mp, nu = m < 0 ? -m : m;
    const bool imag = (mp < 0) != (m < 0);
    const float sg = mu < nu ? -1.f : 1.f;                               // a negative exponent mu - nu: the conjugate power
    u = rec[0] * part_of(imag, asr, asi, bdr, sg * bdi);
    v = rec[1] * part_of(imag, bsr, bsi, adr, sg * adi);
}

// One step of the two recurrences with the record's (c1, c1 + c2, c1 - c2, c3) of degree l: (u1, u2), (v1, v2) are degrees l - 1, l - 2
RNF_FM_HD void entry_step(const float *c, float y, bool neg, float u1, float u2, float v1, float v2, float &u, float &v) {
    const float p = fmaf(-c[0], y, c[1]), q = fmaf(-c[0], y, c[2]);      // c1 X + c2 and c1 X - c2 on the side X = 1 - y, negated on the other
    const float tx = neg ? -q : p, ty = neg ? -p : q;
    u = fmaf(tx, u1, -(c[3] * u2));
    v = fmaf(ty, v1, -(c[3] * v2));
}

// d[i] of nine values held in registers: selects, no indexed access
RNF_FM_HD float pick9(const float *d, int i) {
    return i < 4 ? (i < 2 ? (i == 0 ? d[0] : d[1]) : (i == 2 ? d[2] : d[3])) : (i < 6 ? (i == 4 ? d[4] : d[5]) : (i == 6 ? d[6] : (i == 7 ? d[7] : d[8])));
}

// The degrees l0..L of entry (mp, m) from its seeds: f(l, value).  Degree 1 is the rotation itself, which the quaternion gives to half
// an ulp (k.d1); the recurrence goes on from its own values.
template <class F>
RNF_FM_HD void entry_degrees(const float *rec, int mp, int m, int l0, int L, const CayleyKlein &k, float u, float v, F &&f) {
    float u1 = u, v1 = v, u2 = 0.f, v2 = 0.f;
    f(l0, l0 == 1 ? pick9(k.d1, (mp + 1) * 3 + (m + 1)) : u + v);
    for (int l = l0 + 1; l <= L; ++l) {
        entry_step(rec + 2 + 4 * (l - 1), k.y, k.neg, u1, u2, v1, v2, u, v);
        f(l, l == 1 ? k.d1[4] : u + v);
        u2 = u1; v2 = v1; u1 = u; v1 = v;
    }
}

// Every entry of one rotation, with the powers kept up by single multiplications: s = mu + nu = 0..2L outside, d = |mu - nu| = s mod 2,
// +2, .. inside; per (s, d) the ordered pairs (hi, lo) and (lo, hi) and their signs.  f(mp, m, l0, record, u, v): the seeds of (mp, m).
// records: [(2L+1)^2][record_stride(L)].  The order is fixed: what a caller adds up in it does not depend on anything else.
template <class F>
RNF_FM_HD void walk_entries(const CayleyKlein &k, int L, const float *records, F &&f) {
    const int W = 2 * L + 1, RS = record_stride(L);
    float a2r, a2i, b2r, b2i;
    cmul(k.ar, k.ai, k.ar, k.ai, a2r, a2i);
    cmul(k.br, k.bi, k.br, k.bi, b2r, b2i);
    float asr = 1.f, asi = 0.f, bsr = 1.f, bsi = 0.f;
    for (int s = 0; s <= 2 * L; ++s) {
        float adr = s & 1 ? k.ar : 1.f, adi = s & 1 ? k.ai : 0.f, bdr = s & 1 ? k.br : 1.f, bdi = s & 1 ? k.bi : 0.f;
        const int dmax = s < 2 * L - s ? s : 2 * L - s;
        for (int d = s & 1; d <= dmax; d += 2) {
            const int hi = (s + d) / 2, lo = (s - d) / 2;
            for (int swap = 0; swap < (d > 0 ? 2 : 1); ++swap) {
                const int mu = swap ? lo : hi, nu = swap ? hi : lo;
                for (int sp = 0; sp < (mu > 0 ? 2 : 1); ++sp)
                    for (int sm = 0; sm < (nu > 0 ? 2 : 1); ++sm) {
                        const int mp = sp ? -mu : mu, m = sm ? -nu : nu;
                        const float *rec = records + (long long)((mp + L) * W + (m + L)) * RS;
                        float u, v;
                        entry_seeds(mp, m, rec, asr, asi, bsr, bsi, adr, adi, bdr, bdi, u, v);
                        f(mp, m, hi, rec, u, v);
                    }
            }
            float tr, ti;
            cmul(adr, adi, a2r, a2i, tr, ti); adr = tr; adi = ti;
            cmul(bdr, bdi, b2r, b2i, tr, ti); bdr = tr; bdi = ti;
        }
        float tr, ti;
        cmul(asr, asi, k.ar, k.ai, tr, ti); asr = tr; asi = ti;
        cmul(bsr, bsi, k.br, k.bi, tr, ti); bsr = tr; bsi = ti;
    }
}

// D^l of one row, l <= L, into out[C_L] (NaN where the row is not finite)
RNF_FM_HD void wigner_row(const float *r, int L, const float *records, float *out) {
    const CayleyKlein k = cayley_klein(r);
    const bool ok = ks::finite9(r);
    walk_entries(k, L, records, [&](int mp, int m, int l0, const float *rec, float u, float v) {
        entry_degrees(rec, mp, m, l0, L, k, u, v, [&](int l, float val) { out[coefficient_index(l, mp, m)] = ok ? val : NAN; });
    });
}

// The synthesis of one query for GB groups: acc[gb] = sum over the entries, in walk order, of the fp32 sum over an entry's degrees
template <int GB>
RNF_FM_HD void eval_row(const float *r, int L, const float *records, const float *coeffs, int g0, int G, double *acc) {
    const CayleyKlein k = cayley_klein(r);
    const long long CL = coefficient_count(L);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) acc[gb] = 0.0;
    walk_entries(k, L, records, [&](int mp, int m, int l0, const float *rec, float u, float v) {
        float t[GB];
#pragma unroll
        for (int gb = 0; gb < GB; ++gb) t[gb] = 0.f;
        entry_degrees(rec, mp, m, l0, L, k, u, v, [&](int l, float val) {
            const int at = coefficient_index(l, mp, m);
#pragma unroll
            for (int gb = 0; gb < GB; ++gb) {
                const int g = g0 + gb < G ? g0 + gb : G - 1;
                t[gb] = fmaf(coeffs[g * CL + at], val, t[gb]);
            }
        });
#pragma unroll
        for (int gb = 0; gb < GB; ++gb) acc[gb] += (double)t[gb];
    });
}

// The power table of one centre: row[4k..4k+3] = a^k, b^k for k = 0..2L, row[8L+4] = y, row[8L+5] = 1 on the side X < 0, else 0,
// row[8L+6..8L+14] = D^1
RNF_FM_HD void table_row(const float *r, int L, float *row) {
    const CayleyKlein k = cayley_klein(r);
    float ar = 1.f, ai = 0.f, br = 1.f, bi = 0.f;
    for (int p = 0; p <= 2 * L; ++p) {
        row[4 * p] = ar; row[4 * p + 1] = ai; row[4 * p + 2] = br; row[4 * p + 3] = bi;
        float tr, ti;
        cmul(ar, ai, k.ar, k.ai, tr, ti); ar = tr; ai = ti;
        cmul(br, bi, k.br, k.bi, tr, ti); br = tr; bi = ti;
    }
    row[8 * L + 4] = k.y;
    row[8 * L + 5] = k.neg ? 1.f : 0.f;
    for (int i = 0; i < 9; ++i) row[8 * L + 6 + i] = k.d1[i];
    row[8 * L + 15] = 0.f;
}

// What a thread of the analysis owns: entry (mp, m) and its record for degrees up to LT, in registers
template <int LT>
struct Entry {
    int mp, m, l0, s, d;
    float rec[2 + 4 * LT];
};

template <int LT>
RNF_FM_HD void load_entry(int e, int L, const float *records, Entry<LT> &en) {
    const int W = 2 * L + 1, RS = record_stride(L);
    en.mp = e / W - L;
    en.m = e % W - L;
    const int mu = en.mp < 0 ? -en.mp : en.mp, nu = en.m < 0 ? -en.m : en.m;
    en.l0 = mu > nu ? mu : nu;
    en.s = mu + nu;
    en.d = mu > nu ? mu - nu : nu - mu;
#pragma unroll
    for (int i = 0; i < 2 + 4 * LT; ++i) en.rec[i] = i < RS ? records[(long long)e * RS + i] : 0.f;
}

// The centres j0..j1-1 of one chunk for one entry and GB groups -> S[gb * (LT + 1) + l] = sum_j wn_gj D^l_entry(C_j), in centre order.
// Every term is the exact fp64 product of two fp32 numbers and is added in fp64: under uniform weights the terms of a low degree run
// with one sign over the grid rows of a pixel, and an fp32 sum over 64 of them drifts by about half of 2^-23 in a coefficient whose
// value is a cancellation to nearly 0 -- as much as the whole synthesis gate of a flat density.  Degrees below l0 and above L add
// exact zeros (their record is 0) and are never written.
template <int LT, int GB>
RNF_FM_HD void fourier_chunk(const float *__restrict__ tab, const float *__restrict__ wn, long long n, int j0, int j1, int g0, int G, int L,
                             const Entry<LT> &en, double *S) {
    constexpr int NS = GB * (LT + 1);
    const int RT = table_stride(L);
#pragma unroll
    for (int s = 0; s < NS; ++s) S[s] = 0.0;
    for (int j = j0; j < j1; ++j) {
        const float *row = tab + (long long)j * RT;
        const float *ps = row + 4 * en.s, *pd = row + 4 * en.d;
        const float y = row[8 * L + 4];
        const bool neg = row[8 * L + 5] != 0.f;
        const float first = row[8 * L + 6 + (en.l0 <= 1 ? (en.mp + 1) * 3 + (en.m + 1) : 0)];      // D^1 of the entry, where it has one
        float u0, v0;
        entry_seeds(en.mp, en.m, en.rec, ps[0], ps[1], ps[2], ps[3], pd[0], pd[1], pd[2], pd[3], u0, v0);
        double w[GB];
#pragma unroll
        for (int gb = 0; gb < GB; ++gb) w[gb] = (double)wn[(long long)(g0 + gb < G ? g0 + gb : G - 1) * n + j];
        float u1 = 0.f, u2 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
        for (int l = 0; l <= LT; ++l) {
            if (l <= L) {
                float u = 0.f, v = 0.f;
                if (l > 0) entry_step(en.rec + 2 + 4 * (l > 0 ? l - 1 : 0), y, neg, u1, u2, v1, v2, u, v);
                if (l == en.l0) {
                    u = u0;
                    v = v0;
                }
                const double val = (double)(l == 1 && en.l0 <= 1 ? first : u + v);
#pragma unroll
                for (int gb = 0; gb < GB; ++gb) S[gb * (LT + 1) + l] = fma(w[gb], val, S[gb * (LT + 1) + l]);
                u2 = u1; v2 = v1; u1 = u; v1 = v;
            }
        }
    }
}

inline int groups_per_thread(int L) { return L <= 8 ? 4 : 2; }           // of the analysis: what its registers hold

#if defined(__HIPCC__) && !defined(RNF_SH_HOST_ONLY)       // the host builds of the tests define it: no device code to link
// grid (ceil((2L+1)^2 / THREADS)): the entry records
__global__ __launch_bounds__(THREADS) void so3_harmonics_records_kernel(int L, float *__restrict__ records) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= entry_count(L)) return;
    const int W = 2 * L + 1;
    entry_record(e / W - L, e % W - L, L, records + (long long)e * record_stride(L));
}

// grid (ceil(n / THREADS)): out[i][C_L]
__global__ __launch_bounds__(THREADS) void so3_wigner_kernel(const float *__restrict__ R, long long n, int L, const float *__restrict__ records,
                                                             float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = R[9 * i + k];
    wigner_row(r, L, records, out + i * coefficient_count(L));
}

// grid (ceil(n / THREADS)): the power tables of the centres
__global__ __launch_bounds__(THREADS) void so3_fourier_table_kernel(const float *__restrict__ C, int n, int L, float *__restrict__ tab) {
    const long long j = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (j >= n) return;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = C[9 * j + k];
    table_row(r, L, tab + j * table_stride(L));
}

// The analysis: grid (ceil((2L+1)^2 / THREADS), nchunk, ceil(G / GB)).  psum [G][nchunk][C_L].
template <int LT, int GB>
__global__ __launch_bounds__(THREADS) void so3_fourier_kernel(const float *__restrict__ tab, const float *__restrict__ wn,
                                                              const float *__restrict__ records, int n, int L, int G,
                                                              double *__restrict__ psum) {
    const int E = entry_count(L), e = blockIdx.x * THREADS + threadIdx.x;
    const int chunk = blockIdx.y, nchunk = gridDim.y, g0 = blockIdx.z * GB;
    const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    Entry<LT> en;
    load_entry<LT>(e < E ? e : E - 1, L, records, en);                   // the threads past the last entry repeat it and write nothing
    double S[GB * (LT + 1)];
    fourier_chunk<LT, GB>(tab, wn, n, j0, j1, g0, G, L, en, S);
    if (e >= E) return;
    const long long CL = coefficient_count(L);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
        if (g0 + gb >= G) break;
#pragma unroll
        for (int l = 0; l <= LT; ++l)
            if (l >= en.l0 && l <= L) psum[((long long)(g0 + gb) * nchunk + chunk) * CL + coefficient_index(l, en.mp, en.m)] = S[gb * (LT + 1) + l];
    }
}

// grid (ceil(C_L / THREADS), G): out[g][C_L], the chunks in order
__global__ __launch_bounds__(THREADS) void so3_fourier_final_kernel(const double *__restrict__ psum, int nchunk, int CL, float *__restrict__ out) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= CL) return;
    const long long g = blockIdx.y;
    out[g * CL + c] = (float)ac::chunk_sum(psum + g * nchunk * CL + c, CL, nchunk);
}

// The synthesis: grid (ceil(m / block), ceil(G / GB)), block = THREADS or ac::SMALL_BLOCK.  q_group: floats between the query sets of
// two groups (0: shared; then GB may exceed 1).  out [G][m].
template <int GB>
__global__ __launch_bounds__(THREADS) void so3_fourier_eval_kernel(const float *__restrict__ Q, const float *__restrict__ coeffs,
                                                                   const float *__restrict__ records, long long m, int L, int G,
                                                                   long long q_group, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int g0 = blockIdx.y * GB;
    const float *qp = Q + (long long)g0 * q_group + 9 * i;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = qp[k];
    double acc[GB];
    eval_row<GB>(r, L, records, coeffs, g0, G, acc);
    const bool ok = ks::finite9(r);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb)
        if (g0 + gb < G) out[(long long)(g0 + gb) * m + i] = ok ? (float)acc[gb] : NAN;
}
#endif  // __HIPCC__ && !RNF_SH_HOST_ONLY

// ---- workspaces ---------------------------------------------------------------------------------------------------------------------------

inline size_t records_bytes(int L) { return ((size_t)entry_count(L) * record_stride(L) * 4 + 15) & ~(size_t)15; }

// The workspace of one analysis, carved in this order (the parts of 8-byte elements first)
struct Workspace {
    double *psum;                                  // [G][nchunk][C_L]
    ks::WeightPart *wpart;                         // [G][nchunk]
    double *log_z;                                 // [G]
    float *wn;                                     // [G][n]
    float *tab;                                    // [n][table_stride(L)]
    float *records;                                // [(2L+1)^2][record_stride(L)]
    size_t bytes;
};

inline Workspace carve(void *base, long long n, int G, int L) {
    Workspace w = {};
    const size_t nc = (size_t)ks::chunks_for(n), CL = (size_t)coefficient_count(L);
    const size_t wpart = (size_t)G * nc * CL * 8, log_z = wpart + (size_t)G * nc * sizeof(ks::WeightPart), wn = log_z + (size_t)G * 8;
    const size_t tab = (wn + (size_t)G * (size_t)n * 4 + 15) & ~(size_t)15, rec = tab + (size_t)n * table_stride(L) * 4;
    w.bytes = rec + records_bytes(L);              // G <= 65535, n <= 2^24, C_L <= 6545: below 2^50
    if (!base) return w;
    char *p = static_cast<char *>(base);
    w.psum = reinterpret_cast<double *>(p);
    w.wpart = reinterpret_cast<ks::WeightPart *>(p + wpart);
    w.log_z = reinterpret_cast<double *>(p + log_z);
    w.wn = reinterpret_cast<float *>(p + wn);
    w.tab = reinterpret_cast<float *>(p + tab);
    w.records = reinterpret_cast<float *>(p + rec);
    return w;
}

// ---- the host evaluators: the same row functions in the same order ------------------------------------------------------------------------

inline std::vector<float> host_records(int L) {
    std::vector<float> rec((size_t)entry_count(L) * record_stride(L));
    const int W = 2 * L + 1;
    for (int e = 0; e < entry_count(L); ++e) entry_record(e / W - L, e % W - L, L, rec.data() + (size_t)e * record_stride(L));
    return rec;
}

// out [n][C_L]
inline void host_wigner(const float *R, long long n, int L, float *out) {
    const std::vector<float> rec = host_records(L);
    for (long long i = 0; i < n; ++i) wigner_row(R + 9 * i, L, rec.data(), out + i * coefficient_count(L));
}

template <int LT>
inline void host_fourier_group(const float *tab, const float *wn, long long n, int L, const float *records, float *out) {
    const int nchunk = (int)ks::chunks_for(n), CL = coefficient_count(L);
    std::vector<double> psum((size_t)nchunk * (LT + 1));
    for (int e = 0; e < entry_count(L); ++e) {
        Entry<LT> en;
        load_entry<LT>(e, L, records, en);
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : (int)n;
            fourier_chunk<LT, 1>(tab, wn, n, j0, j1, 0, 1, L, en, psum.data() + (size_t)chunk * (LT + 1));
        }
        for (int l = en.l0; l <= L; ++l) out[coefficient_index(l, en.mp, en.m)] = (float)ac::chunk_sum(psum.data() + l, LT + 1, nchunk);
    }
    (void)CL;
}

// C [n][9], lw [G][n] or null -> out [G][C_L]; arguments are not checked
inline void host_fourier(const float *C, const float *lw, long long n, int G, int L, float *out) {
    const std::vector<float> rec = host_records(L);
    std::vector<float> tab((size_t)n * table_stride(L)), wn((size_t)n);
    for (long long j = 0; j < n; ++j) table_row(C + 9 * j, L, tab.data() + (size_t)j * table_stride(L));
    for (int g = 0; g < G; ++g) {
        const double log_z = ks::host_log_z(C, lw, g, n);
        for (long long j = 0; j < n; ++j) wn[(size_t)j] = ac::weight_norm(lw ? lw[(long long)g * n + j] : 0.f, log_z);
        float *o = out + (long long)g * coefficient_count(L);
        if (L <= 8) host_fourier_group<8>(tab.data(), wn.data(), n, L, rec.data(), o);
        else host_fourier_group<16>(tab.data(), wn.data(), n, L, rec.data(), o);
    }
}

// coeffs [G][C_L], Q [m][9] or [G][m][9] (group_queries) -> out [G][m]; arguments are not checked
inline void host_fourier_eval(const float *coeffs, const float *Q, long long m, int G, bool group_queries, int L, float *out) {
    const std::vector<float> rec = host_records(L);
    for (int g = 0; g < G; ++g)
        for (long long i = 0; i < m; ++i) {
            const float *q = Q + ((group_queries ? (long long)g * m : 0) + i) * 9;
            double acc;
            eval_row<1>(q, L, rec.data(), coeffs, g, G, &acc);
            out[(long long)g * m + i] = ks::finite9(q) ? (float)acc : NAN;
        }
}

}  // namespace sh
}  // namespace rnf
