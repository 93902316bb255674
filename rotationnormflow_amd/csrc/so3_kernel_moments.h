// so3_kernel_moments.h -- responsibility-weighted first moments of the pairwise matrix-Fisher kernel sum of so3_kernel_sum.h
// (rnf_so3_kernel_moments, include/rnf_hip.h): the score of the kernel density estimate on SO(3), its mean-shift step and its
// derivative with respect to the bandwidth, from one pass over the pairs.
//
// With centres C[n], queries Q[m] (shared by the G groups, or one set per group), ONE concentration kappa and G rows of log-weights
// (none: G = 1, lw = 0), w_g = softmax(lw_g) and k_kappa of so3_kernel_sum.h:
//     r_ij        = w_j k(C_j, Q_i) / sum_l w_l k(C_l, Q_i)                         (the responsibilities of query i)
//     log_density = log sum_j w_j k(C_j, Q_i)                                       (bit-identical to rnf_so3_kernel_sum with J = 1)
//     mean        = M_i = sum_j r_ij C_j                                            ([9], fp32)
//     msd         = D_i = sum_j r_ij |Q_i - C_j|_F^2
//     rotation    = polar3(M_i) where det M_i > 0, else NaN                         (the rotation that maximises tr(M_i^T R))
//     step        = |rotation - Q_i|_F                                              (NaN where rotation is)
// so that  d log p(Q_i) / dQ_i = kappa (M_i - Q_i),  d log p(Q_i) / dkappa = -D_i / 2 - l'(kappa),  and Q_i <- rotation is the mean-shift
// step of a matrix-Fisher kernel.  A convex combination of rotations can have det <= 0 (three half-turns about orthogonal axes
// average to -I / 3): there is no mean direction then, and rotation is NaN.
//
// Arithmetic.  The exponent t = fma(-h, d2, lw2) of a pair is that of so3_kernel_sum.h, from its row functions (ks::dist2, ks::Scales,
// ks::exp2_bare), and so is the first sweep over a chunk (ks::tile_pass with SUM = false: the maximum M).  The second sweep forms
// e = exp2(t - M) once per pair and adds 11 sums: e, e d2 and e C[k], k = 0..8 -- fp32 over a tile of 64 centres, fp64 over the tiles of
// a chunk.  No e exceeds 1 and the entries of a rotation do not exceed 1 in size.  A centre whose log-weight is -inf has e = 0 exactly,
// which leaves every sum as it is -- unless one of its entries is not finite, when 0 times the entry is NaN.  A flags pass marks the
// chunks that hold a non-finite centre (a property of the centres alone); in those chunks only, a centre with lw = -inf is skipped by
// a branch on its (wave-uniform) log-weight, in all others the loop has no branch.  Both give the same bits.
//
// Shape of the hot kernel: a thread owns ONE (group, query) pair in registers; the centre index is wave-uniform, so the centre and its
// log-weight arrive by scalar loads and enter the VALU as scalar operands -- no LDS, no barrier, no cross-lane traffic.
//
// Determinism: as so3_kernel_sum.h.  Chunks of 4096 centres (a function of n alone); one partial (fp32 max, 11 fp64 sums) per (group,
// chunk, query); the finalise combines a query's chunks in chunk order in fp64 as sum_c S_c 2^(M_c - M) for each of the 11 sums,
// divides by the first, rounds once to fp32, then runs polar3 and forms the step.  No floating-point atomics.  A query's outputs are
// bit-identical from run to run and whatever m, G, the query's position and the group's position are, and whether the queries are
// given per group or shared.
//
// Edge cases: those of so3_kernel_sum.h, for every output of the (group, query).  A centre with lw = -inf is left out whatever its
// entries; any other non-finite centre, or a NaN log-weight, makes its group NaN; a non-finite query is NaN; a group with no mass is NaN.
// kappa = 0 gives mean = sum_j w_j C_j for every query.
#pragma once
#if defined(RNF_KM_HOST_ONLY) && !defined(RNF_KS_HOST_ONLY)
#define RNF_KS_HOST_ONLY
#endif
#include "so3_kernel_sum.h"
#include "so3_math.h"

namespace rnf {
namespace km {

constexpr int NSUM = 11;                           // sum e, sum e d2, sum e C[0..8]
constexpr int SMALL_BLOCK = 64;                    // one wave per block while blocks of THREADS would leave compute units idle
constexpr long long FEW_BLOCKS = 1024;             // 4 per compute unit of an MI355X

// threads per block of the pairwise pass for m queries per group
inline int block_for(long long m, long long nchunk, long long G) {
    return (m + ks::THREADS - 1) / ks::THREADS * nchunk * G < FEW_BLOCKS ? SMALL_BLOCK : ks::THREADS;
}
using ks::CHUNK;
using ks::THREADS;
using ks::TILE;

// l'(kappa) = d/dkappa log(i0e(2 kappa) - i1e(2 kappa)) = -E[d2] / 2 under the kernel, l'(0) = -3.  With s = sin(t / 2) and x = 4 kappa,
//     l'(kappa) = -4 I_4 / I_2,   I_p = int_0^pi exp(-x s^2) s^p dt = 2 int_0^1 exp(-x u^2) u^p (1 - u^2)^(-1/2) du.
// Below kappa = 16 the closed form -4 + i1e / (kappa (i0e - i1e)) is used: its difference loses about 4 kappa 1e-16, relatively.  From 16
// on, (1 - u^2)^(-1/2) = sum_k a_k u^(2k) (a_k = binom(2k, k) / 4^k) under the Gaussian gives the asymptotic series of both integrals,
//     I_p ~ x^(-(p+1)/2) sum_k a_k Gamma(k + (p+1)/2) x^-k      (the tail beyond u = 1 is below exp(-64)),
// whose terms are all positive: nothing cancels.  At x >= 64 the terms fall below 1e-17 of the sum before they grow again.
RNF_FM_HD double dlog_normaliser(double kappa) {
    if (kappa == 0.0) return -3.0;
    if (kappa < 16.0) {
        double i0, i1;
        bessel_i01e(2.0 * kappa, i0, i1);
        return -4.0 + i1 / (kappa * (i0 - i1));
    }
    const double x = 4.0 * kappa;
    double a = 1.0, g = 1.0, pw = 1.0;             // a_k, Gamma(k + 3/2) / Gamma(3/2), x^-k
    double s2 = 0.0, s4 = 0.0, last = INFINITY;
    for (int k = 0; k < 64; ++k) {
        const double g1 = g * (k + 1.5);           // Gamma(k + 5/2) / Gamma(3/2)
        const double t2 = a * g * pw, t4 = a * g1 * pw;
        if (t4 > last || t4 < 1e-19 * s4) break;   // the smallest term of an asymptotic series, or nothing left to add
        s2 += t2;
        s4 += t4;
        last = t4;
        a *= (2.0 * k + 1.0) / (2.0 * k + 2.0);
        g = g1;
        pw /= x;
    }
    return -4.0 * s4 / (x * s2);
}

RNF_FM_HD bool left_out(float l) { return l == -INFINITY; }

// Centres ja..jb-1 of one tile against one query of group g: acc[0] += e, acc[1] += e d2, acc[2 + k] += e C[k], e = exp2(t - Mu).
// SKIP: the chunk holds a non-finite centre, so the centres that are left out are stepped over.
template <bool W, bool SKIP>
RNF_FM_HD void moment_tile(const float *__restrict__ C, const float *__restrict__ lw, long long n, int ja, int jb, int g, const float q[9], float h,
                           float Mu, float *acc) {
#pragma unroll 4
    for (int j = ja; j < jb; ++j) {
        float l2 = 0.f;
        if (W) {
            const float l = lw[(long long)g * n + j];
            if (SKIP && left_out(l)) continue;     // e = 0 exactly: no sum changes, and 0 * (an entry that is not finite) is kept out
            l2 = l * (float)ks::LOG2E;
        }
        const float *c = C + 9LL * j;
        const float d2 = ks::dist2(c, q);
        const float e = ks::exp2_bare(fmaf(-h, d2, l2) - Mu);
        acc[0] += e;
        acc[1] = fmaf(e, d2, acc[1]);
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[2 + k] = fmaf(e, c[k], acc[2 + k]);
    }
}

// One query of group g against the centres j0..j1-1 of one chunk -> the chunk's maximum M and its 11 sums about it.  skip: the chunk's flag.
RNF_FM_HD void moment_chunk(const float *__restrict__ C, const float *__restrict__ lw, long long n, int j0, int j1, int g, const float q[9],
                            const ks::Scales &sc, bool skip, float &M, double *S) {
    M = -INFINITY;
    for (int ja = j0; ja < j1; ja += TILE) {       // the first sweep of so3_kernel_sum.h, one slot
        const int jb = ja + TILE < j1 ? ja + TILE : j1;
        ks::tile_switch<1, 1, false>(false, C, lw, n, ja, jb, 0, g, g + 1, q, sc, nullptr, &M);
    }
    const float Mu = M == -INFINITY ? 0.f : M;
#pragma unroll
    for (int s = 0; s < NSUM; ++s) S[s] = 0.0;
    for (int ja = j0; ja < j1; ja += TILE) {
        const int jb = ja + TILE < j1 ? ja + TILE : j1;
        float part[NSUM];
#pragma unroll
        for (int s = 0; s < NSUM; ++s) part[s] = 0.f;
        if (!lw)
            moment_tile<false, false>(C, lw, n, ja, jb, g, q, sc.h[0], Mu, part);
        else if (skip)
            moment_tile<true, true>(C, lw, n, ja, jb, g, q, sc.h[0], Mu, part);
        else
            moment_tile<true, false>(C, lw, n, ja, jb, g, q, sc.h[0], Mu, part);
#pragma unroll
        for (int s = 0; s < NSUM; ++s) S[s] += (double)part[s];
    }
}

struct Result {
    float log_density, mean[9], msd, rotation[9], step;
};

// A query's chunk partials -> its outputs.  pmax[c * stride], psum[s * plane + c * stride]; log_z as ks::combine.
RNF_FM_HD void finish(const float *pmax, const double *psum, long long stride, long long plane, int nchunk, double l_kappa, double log_z,
                      const float q[9], bool project, Result &r) {
    r.log_density = ks::combine(pmax, psum, stride, nchunk, l_kappa, log_z, false, 0.0);      // sum 0 is the kernel sum's
    r.msd = r.step = NAN;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.mean[k] = r.rotation[k] = NAN;
    if (r.log_density != r.log_density) return;
    double M = -INFINITY;
    for (int c = 0; c < nchunk; ++c) {
        const double mc = (double)pmax[c * stride];
        M = mc > M ? mc : M;
    }
    double T[NSUM];
#pragma unroll
    for (int s = 0; s < NSUM; ++s) T[s] = 0.0;
    for (int c = 0; c < nchunk; ++c) {
        const double mc = (double)pmax[c * stride];
        if (mc == -INFINITY) continue;
        const double f = exp2(mc - M);
#pragma unroll
        for (int s = 0; s < NSUM; ++s) T[s] += psum[s * plane + c * stride] * f;
    }
    r.msd = (float)(T[1] / T[0]);
#pragma unroll
    for (int k = 0; k < 9; ++k) r.mean[k] = (float)(T[2 + k] / T[0]);
    if (!project) return;
    const float(&a)[9] = r.mean;
    const double det = (double)a[0] * ((double)a[4] * a[8] - (double)a[5] * a[7]) - (double)a[1] * ((double)a[3] * a[8] - (double)a[5] * a[6]) +
                       (double)a[2] * ((double)a[3] * a[7] - (double)a[4] * a[6]);
    if (!(det > 0.0)) return;                      // no mean direction
    v3f p0, p1, p2;
    polar3(r.mean, p0, p1, p2);                    // a rotation to 16 * 2^-23, or NaN
    const float rot[9] = {p0.x, p0.y, p0.z, p1.x, p1.y, p1.z, p2.x, p2.y, p2.z};
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        r.rotation[k] = rot[k];
        const float d = rot[k] - q[k];
        d2 = fmaf(d, d, d2);
    }
    r.step = sqrtf(d2);
}

#if defined(__HIPCC__) && !defined(RNF_KM_HOST_ONLY)       // the host builds of the tests define it: no device code to link
// grid (nchunk), THREADS threads: flags[chunk] = whether the chunk holds a centre with an entry that is not finite
__global__ __launch_bounds__(THREADS) void so3_kernel_moments_flags_kernel(const float *__restrict__ C, int n, int *__restrict__ flags) {
    const int chunk = blockIdx.x, j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    bool bad = false;
    for (int j = j0 + (int)threadIdx.x; j < j1; j += THREADS) bad = bad || !ks::finite9(C + 9LL * j);
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) flags[chunk] = any;
}

// The pairwise pass: grid (ceil(m / block), nchunk, G), block = THREADS or, for few queries, SMALL_BLOCK threads (a thread owns its query
// whatever the block: the same bits).  pmax [G][nchunk][m], psum [G][NSUM][nchunk][m]; q_group: floats between
// the query sets of two groups (0: shared).
__global__ __launch_bounds__(THREADS) void so3_kernel_moments_kernel(const float *__restrict__ C, const float *__restrict__ Q,
                                                                     const float *__restrict__ lw, int n, int m, long long q_group,
                                                                     ks::Scales sc, const int *__restrict__ flags, float *__restrict__ pmax,
                                                                     double *__restrict__ psum) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long ii = i < m ? i : m - 1;        // the threads past m repeat the last query and write nothing
    const int chunk = blockIdx.y, nchunk = gridDim.y, g = blockIdx.z;
    const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    const float *qp = Q + (long long)g * q_group + 9 * ii;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = qp[k];
    float M;
    double S[NSUM];
    moment_chunk(C, lw, n, j0, j1, g, q, sc, flags[chunk] != 0, M, S);
    if (i >= m) return;
    pmax[((long long)g * nchunk + chunk) * m + i] = ks::finite9(q) ? M : NAN;
#pragma unroll
    for (int s = 0; s < NSUM; ++s) psum[(((long long)g * NSUM + s) * nchunk + chunk) * m + i] = S[s];
}

// grid (ceil(m / THREADS), G): the outputs of (g, i); null outputs are not written
__global__ __launch_bounds__(THREADS) void so3_kernel_moments_final_kernel(const float *__restrict__ pmax, const double *__restrict__ psum,
                                                                           const double *__restrict__ log_z, const float *__restrict__ Q,
                                                                           long long q_group, int m, int nchunk, double l_kappa,
                                                                           float *__restrict__ log_density, float *__restrict__ mean,
                                                                           float *__restrict__ msd, float *__restrict__ rotation,
                                                                           float *__restrict__ step) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= m) return;
    const int g = blockIdx.y;
    const float *qp = Q + (long long)g * q_group + 9 * i;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = qp[k];
    Result r;
    finish(pmax + (long long)g * nchunk * m + i, psum + (long long)g * NSUM * nchunk * m + i, m, (long long)nchunk * m, nchunk, l_kappa, log_z[g], q,
           rotation != nullptr, r);
    const long long at = (long long)g * m + i;
    if (log_density) log_density[at] = r.log_density;
    if (msd) msd[at] = r.msd;
    if (step) step[at] = r.step;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        if (mean) mean[9 * at + k] = r.mean[k];
        if (rotation) rotation[9 * at + k] = r.rotation[k];
    }
}
#endif  // __HIPCC__ && !RNF_KM_HOST_ONLY

// The workspace of one call, carved in this order (the parts of 8-byte elements first)
struct Workspace {
    double *psum;                                  // [G][NSUM][nchunk][m]
    ks::WeightPart *wpart;                         // [G][nchunk]
    double *log_z;                                 // [G]
    float *pmax;                                   // [G][nchunk][m]
    int *flags;                                    // [nchunk]
    size_t bytes;                                  // 0: does not fit a size_t
};

inline Workspace carve(void *base, long long n, long long m, int G) {
    Workspace w = {};
    const long double cells = (long double)G * (long double)ks::chunks_for(n) * (long double)m;
    if (cells * (8.0L * NSUM + 4.0L) > 4.0e18L) return w;
    const size_t nc = (size_t)ks::chunks_for(n), part = (size_t)G * nc * (size_t)m;
    const size_t wpart = part * NSUM * 8, log_z = wpart + (size_t)G * nc * sizeof(ks::WeightPart), pmax = log_z + (size_t)G * 8;
    const size_t flags = pmax + part * 4;
    w.bytes = (flags + nc * 4 + 15) & ~(size_t)15;
    if (!base) return w;
    char *p = static_cast<char *>(base);
    w.psum = reinterpret_cast<double *>(p);
    w.flags = reinterpret_cast<int *>(p + flags);
    w.wpart = reinterpret_cast<ks::WeightPart *>(p + wpart);
    w.log_z = reinterpret_cast<double *>(p + log_z);
    w.pmax = reinterpret_cast<float *>(p + pmax);
    return w;
}

// ---- the host evaluator: the same arithmetic in the same order (exp2f and exp of the host's libm in place of the device's) ----------
// Q [m][9], or [G][m][9] with group_queries; lw [G][n] or null; every output [G][m] (x 9) may be null; arguments are not checked
inline void host_kernel_moments(const float *C, const float *Q, const float *lw, long long n, long long m, int G, double kappa, bool group_queries,
                                float *log_density, float *mean, float *msd, float *rotation, float *step) {
    ks::Scales sc;
    ks::Normalisers nm;
    ks::scales_of(&kappa, 1, sc, nm);
    const int nchunk = (int)ks::chunks_for(n);
    std::vector<float> pmax((size_t)nchunk);
    std::vector<double> psum((size_t)NSUM * nchunk);
    std::vector<char> flags((size_t)nchunk, 0);    // the flags pass
    for (long long j = 0; j < n; ++j)
        if (!ks::finite9(C + 9 * j)) flags[(size_t)(j / CHUNK)] = 1;
    for (int g = 0; g < G; ++g) {
        const double log_z = ks::host_log_z(C, lw, g, n);
        for (long long i = 0; i < m; ++i) {
            const float *q = Q + ((group_queries ? (long long)g * m : 0) + i) * 9;
            for (int chunk = 0; chunk < nchunk; ++chunk) {
                const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : (int)n;
                float M;
                double S[NSUM];
                moment_chunk(C, lw, n, j0, j1, g, q, sc, flags[chunk] != 0, M, S);
                pmax[chunk] = ks::finite9(q) ? M : NAN;
                for (int s = 0; s < NSUM; ++s) psum[(size_t)s * nchunk + chunk] = S[s];
            }
            Result r;
            finish(pmax.data(), psum.data(), 1, nchunk, nchunk, nm.l[0], log_z, q, rotation != nullptr, r);
            const long long at = (long long)g * m + i;
            if (log_density) log_density[at] = r.log_density;
            if (msd) msd[at] = r.msd;
            if (step) step[at] = r.step;
            for (int k = 0; k < 9; ++k) {
                if (mean) mean[9 * at + k] = r.mean[k];
                if (rotation) rotation[9 * at + k] = r.rotation[k];
            }
        }
    }
}

}  // namespace km
}  // namespace rnf
