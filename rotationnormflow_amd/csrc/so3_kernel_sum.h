// so3_kernel_sum.h -- pairwise sums of isotropic matrix-Fisher kernels between two sets of rotations (rnf_so3_kernel_sum,
// include/rnf_hip.h): the kernel density estimate on SO(3) and the prediction step of a Bayes filter on the SO(3) grid.
//
// With centres C[n], queries Q[m], J concentrations kappa_a and G rows of log-weights lw[g][n] (none: G = 1, lw = 0), w_g = softmax(lw_g):
//     out[g][a][i] = log sum_j w_gj k_a(C_j, Q_i),      k_kappa(C, Q) = exp(-(kappa/2) |Q - C|_F^2 - l(kappa)),
//     l(kappa)     = c(kappa I) - 3 kappa = log(i0e(2 kappa) - i1e(2 kappa)),  l(0) = 0       (fp64, bessel_i01e of fisher_exact.h),
// a density w.r.t. the Haar probability measure: k_kappa(C, .) is MF(kappa C) because tr(C^T Q) - 3 = -1/2 |Q - C|_F^2.  The exponent is
// formed from the nine differences of the fp32 entries, their squares and a sum of non-negative terms, never from the trace, which has
// lost its digits once kappa (3 - tr) is small beside kappa.
// Leave-one-out (the queries ARE the centres): out[g][a][i] = log sum_{j != i} w_gj k_a(C_j, C_i) - log1p(-w_gi).  Only index i is left
// out; a duplicate of C_i at another index counts.
//
// Arithmetic.  Everything up to the chunk partials is base 2: h_a = (kappa_a / 2) log2(e) and lw log2(e) in fp32,
//     t = fma(-h_a, d2, lw2),   d2 = fma chain of the nine squared differences (capped at FLT_MAX: see the edge cases),
// so that the exponential is the bare v_exp_f32.  Two sweeps over a chunk of centres per (query, bandwidth, group): the first takes
// M = max_j t with no exponential, the second adds exp2(t - M) -- no term exceeds 1, the largest is exactly 1, nothing is rescaled.  The
// second sweep adds TILE = 64 terms serially in fp32 and the tile sums in fp64, so no fp32 sum runs over more than one tile.
//
// Shape of the hot kernel: a thread owns ONE query in registers and walks the chunk's centres; the centre index is wave-uniform, so the
// centre's nine entries and its log-weight arrive by scalar loads and enter the VALU as scalar operands -- no LDS, no barrier, no
// cross-lane traffic.  d2 is computed once per pair and shared by the J bandwidths (and, for J = 1, by GROUPS_PER_THREAD = 4 groups).
//
// Determinism.  Centres are split into chunks of CHUNK = 4096, a function of n alone.  A thread writes one (M, S) partial per (query,
// bandwidth, group, chunk); the finalise combines a query's chunk partials in chunk order in fp64, subtracts the normalisers and
// rounds once to fp32.  The softmax normaliser log Z_g is summed per chunk by a fixed tree and over the chunks by a fixed lane
// assignment and butterfly.  No floating-point atomics anywhere.  A query's result is therefore bit-identical from run to run and
// whatever m, G, the query's position in the call and the group's position are: callers may tile queries and groups freely.
//
// Edge cases.  A centre with lw = -inf is left out whatever its entries (d2 is capped at FLT_MAX, so t = -inf and exp2 gives 0).  Any
// other centre with a non-finite entry, or a NaN log-weight, makes every output of its group NaN (found by the weights pass).  A query
// with a non-finite entry is NaN.  A group with no mass left is NaN: all weights -inf, leave-one-out with n = 1, w_gi = 1.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <vector>

#include "fisher_exact.h"

namespace rnf {
namespace ks {

constexpr int MAX_J = 8, CHUNK = 4096, TILE = 64, THREADS = 256;
constexpr int GROUPS_PER_THREAD = 4;               // for J = 1 without leave-one-out: groups that share one d2
constexpr long long MAX_N = 1LL << 24, MAX_M = (1LL << 31) - 1;
constexpr int MAX_G = 65535;
constexpr double MAX_KAPPA = 1e6;
constexpr double LOG2E = 1.4426950408889634074, LN2 = 0.69314718055994530942;

inline long long chunks_for(long long n) { return (n + CHUNK - 1) / CHUNK; }

// l(kappa) = log(i0e(2 kappa) - i1e(2 kappa)); the difference is ~ i0e / (4 kappa), so its relative error is ~ 4 kappa 1e-16
RNF_FM_HD double log_normaliser(double kappa) {
    if (kappa == 0.0) return 0.0;
    double i0, i1;
    bessel_i01e(2.0 * kappa, i0, i1);
    return log(i0 - i1);
}

struct Scales { float h[MAX_J]; };                 // (kappa_a / 2) log2(e), fp32
struct Normalisers { double l[MAX_J]; };           // l(kappa_a)

RNF_FM_HD float exp2_bare(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(x);              // v_exp_f32: x <= 0 here, a result below 2^-126 may flush to 0
#else
    return exp2f(x);
#endif
}

// |q - c|_F^2 of two row-major 3x3 matrices; a NaN or an overflow comes out as FLT_MAX, so that fma(-h, d2, -inf) is -inf for every h >= 0
RNF_FM_HD float dist2(const float *c, const float *q) {
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float d = q[k] - c[k];
        d2 = fmaf(d, d, d2);
    }
    return fminf(d2, FLT_MAX);
}

// Centres ja..jb-1 against one query for the J * GB slots (group gb, bandwidth a) -> slot gb * J + a.
//   SUM = false: acc[s] = max(acc[s], t);   SUM = true: acc[s] += exp2(t - M[s]).
//   MASK: centre j == i is left out (leave-one-out; only the tiles that meet the block's own queries are run with it).
//   W: with log-weights (lw is not null).
template <int J, int GB, bool MASK, bool SUM, bool W>
RNF_FM_HD void tile_pass(const float *__restrict__ C, const float *__restrict__ lw, long long n, int ja, int jb, int i, int g0, int G,
                         const float q[9], const Scales &sc, const float *M, float *acc) {
#pragma unroll 4
    for (int j = ja; j < jb; ++j) {
        const float d2 = dist2(C + 9LL * j, q);
#pragma unroll
        for (int gb = 0; gb < GB; ++gb) {
            const int g = g0 + gb < G ? g0 + gb : G - 1;
            const float l2 = W ? lw[(long long)g * n + j] * (float)LOG2E : 0.f;
#pragma unroll
            for (int a = 0; a < J; ++a) {
                float t = fmaf(-sc.h[a], d2, l2);
                if (MASK) t = j == i ? -INFINITY : t;
                if (SUM)
                    acc[gb * J + a] += exp2_bare(t - M[gb * J + a]);
                else
                    acc[gb * J + a] = fmaxf(acc[gb * J + a], t);
            }
        }
    }
}

// tile_pass with its two run-time switches hoisted out of the loop over the centres (both are uniform over the block)
template <int J, int GB, bool SUM>
RNF_FM_HD void tile_switch(bool mask, const float *__restrict__ C, const float *__restrict__ lw, long long n, int ja, int jb, int i, int g0, int G,
                           const float q[9], const Scales &sc, const float *M, float *acc) {
    if (lw) {
        if (mask)
            tile_pass<J, GB, true, SUM, true>(C, lw, n, ja, jb, i, g0, G, q, sc, M, acc);
        else
            tile_pass<J, GB, false, SUM, true>(C, lw, n, ja, jb, i, g0, G, q, sc, M, acc);
    } else {
        if (mask)
            tile_pass<J, GB, true, SUM, false>(C, lw, n, ja, jb, i, g0, G, q, sc, M, acc);
        else
            tile_pass<J, GB, false, SUM, false>(C, lw, n, ja, jb, i, g0, G, q, sc, M, acc);
    }
}

// One query against the centres j0..j1-1 of one chunk: the partial (M, S) of each slot, sum_j 2^t_j = S 2^M.  blk_lo: the first query
// index of the thread's block (a multiple of THREADS); with LOO the centres blk_lo..blk_lo+THREADS-1 are the block's own queries.
template <int J, int GB, bool LOO>
RNF_FM_HD void query_chunk(const float *__restrict__ C, const float *__restrict__ lw, long long n, int j0, int j1, int i, int blk_lo, int g0,
                           int G, const float q[9], const Scales &sc, float *M, double *S) {
    constexpr int NS = J * GB;
#pragma unroll
    for (int s = 0; s < NS; ++s) M[s] = -INFINITY;
    for (int ja = j0; ja < j1; ja += TILE) {
        const int jb = ja + TILE < j1 ? ja + TILE : j1;
        tile_switch<J, GB, false>(LOO && ja < blk_lo + THREADS && jb > blk_lo, C, lw, n, ja, jb, i, g0, G, q, sc, nullptr, M);
    }
    float Mu[NS];                                  // a chunk without a live centre: M = -inf, every term exp2(-inf - 0) = 0
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        Mu[s] = M[s] == -INFINITY ? 0.f : M[s];
        S[s] = 0.0;
    }
    for (int ja = j0; ja < j1; ja += TILE) {
        const int jb = ja + TILE < j1 ? ja + TILE : j1;
        float part[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) part[s] = 0.f;
        tile_switch<J, GB, true>(LOO && ja < blk_lo + THREADS && jb > blk_lo, C, lw, n, ja, jb, i, g0, G, q, sc, Mu, part);
#pragma unroll
        for (int s = 0; s < NS; ++s) S[s] += (double)part[s];
    }
}

RNF_FM_HD bool finite9(const float *r) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && fabsf(r[k]) < INFINITY;
    return ok;
}

// A query's chunk partials (stride: elements between chunks) -> the output.  log_z: the group's log sum exp(lw) (NaN: the group is
// NaN); loo_lw: the query's own log-weight with leave-one-out (0 without log-weights), unused otherwise.
RNF_FM_HD float combine(const float *pmax, const double *psum, long long stride, int nchunk, double l_kappa, double log_z, bool loo,
                        double loo_lw) {
    double M = -INFINITY;
    bool nan = false;
    for (int c = 0; c < nchunk; ++c) {
        const double mc = (double)pmax[c * stride];
        nan = nan || mc != mc;                     // a non-finite query
        M = mc > M ? mc : M;
    }
    if (nan || M == -INFINITY || M == INFINITY || log_z != log_z) return NAN;      // no mass left: nothing but -inf terms
    double S = 0.0;
    for (int c = 0; c < nchunk; ++c) {
        const double mc = (double)pmax[c * stride];
        if (mc != -INFINITY) S += psum[c * stride] * exp2(mc - M);
    }
    double r = ((M + log2(S)) * LN2 - l_kappa) - log_z;
    if (loo) {
        const double w = exp(loo_lw - log_z);
        if (!(w < 1.0)) return NAN;                // the query holds all of its group's mass
        r -= log1p(-w);
    }
    return (float)r;
}

// ---- the weights pass: log Z_g = log sum_j exp(lw_gj), and whether the group is NaN ---------------------------------------------------

struct WeightPart {                                // one chunk of one group: sum_j exp(lw_j - M) = S, 16 bytes
    double S;
    float M;
    int bad;                                       // a NaN log-weight, or a live centre with a non-finite entry
};

RNF_FM_HD void weight_row(const float *__restrict__ C, const float *__restrict__ lw, long long g, long long n, long long j, float &l,
                          bool &bad) {
    l = lw ? lw[g * n + j] : 0.f;
    bad = bad || l != l || (l != -INFINITY && !finite9(C + 9 * j));
}

RNF_FM_HD double weight_term(float l, float M) { return M == -INFINITY ? 0.0 : exp((double)l - (double)M); }

// log Z from the chunk partials of one group, as lane `lane` of 64 sees them: its maximum and its sum about the group's maximum
RNF_FM_HD float weight_lane_max(const WeightPart *p, int nchunk, int lane, bool &bad) {
    float M = -INFINITY;
    for (int c = lane; c < nchunk; c += 64) {
        M = fmaxf(M, p[c].M);
        bad = bad || p[c].bad != 0;
    }
    return M;
}
RNF_FM_HD double weight_lane_sum(const WeightPart *p, int nchunk, int lane, float M) {
    double S = 0.0;
    for (int c = lane; c < nchunk; c += 64)
        if (p[c].M != -INFINITY) S += p[c].S * exp((double)p[c].M - (double)M);
    return S;
}
RNF_FM_HD double weight_log_z(float M, double S, bool bad) {
    return bad || M == -INFINITY || M == INFINITY ? (double)NAN : (double)M + log(S);
}

#if defined(__HIPCC__) && !defined(RNF_KS_HOST_ONLY)       // the host builds of the tests define it: no device code to link
// grid (nchunk, G), THREADS threads: part[g][chunk].  Thread t takes rows t, t + THREADS, ..; the block adds by the tree 128, 64, .. 1.
__global__ __launch_bounds__(THREADS) void so3_kernel_weights_kernel(const float *__restrict__ C, const float *__restrict__ lw, int n,
                                                                     WeightPart *__restrict__ part) {
    __shared__ double sv[THREADS];
    __shared__ float sm[THREADS];
    __shared__ int sbad;
    const int t = threadIdx.x, chunk = blockIdx.x, g = blockIdx.y;
    const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    if (t == 0) sbad = 0;
    float M = -INFINITY;
    bool bad = false;
    for (int j = j0 + t; j < j1; j += THREADS) {
        float l;
        weight_row(C, lw, g, n, j, l, bad);
        M = fmaxf(M, l);
    }
    sm[t] = M;
    __syncthreads();
    if (bad) sbad = 1;
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] = fmaxf(sm[t], sm[t + s]);
        __syncthreads();
    }
    M = sm[0];
    double S = 0.0;
    for (int j = j0 + t; j < j1; j += THREADS) S += weight_term(lw ? lw[(long long)g * n + j] : 0.f, M);
    sv[t] = S;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sv[t] += sv[t + s];
        __syncthreads();
    }
    if (t == 0) part[(long long)g * gridDim.x + chunk] = WeightPart{sv[0], M, sbad};
}

// grid (G), 64 threads: log_z[g]
__global__ __launch_bounds__(64) void so3_kernel_weights_final_kernel(const WeightPart *__restrict__ part, int nchunk, double *__restrict__ log_z) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const WeightPart *p = part + (long long)g * nchunk;
    bool bad = false;
    float M = weight_lane_max(p, nchunk, lane, bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    bad = __any(bad);
    double S = weight_lane_sum(p, nchunk, lane, M);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o, 64);
    if (lane == 0) log_z[g] = weight_log_z(M, S, bad);
}

// The pairwise pass: grid (ceil(m / THREADS), nchunk, ceil(G / GB)).  pmax, psum: [G][J][nchunk][m].
template <int J, int GB, bool LOO>
__global__ __launch_bounds__(THREADS) void so3_kernel_sum_kernel(const float *__restrict__ C, const float *__restrict__ Q,
                                                                 const float *__restrict__ lw, int n, int m, int G, Scales sc,
                                                                 float *__restrict__ pmax, double *__restrict__ psum) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int ii = (int)(i < m ? i : m - 1);       // the threads past m repeat the last query and write nothing
    const int chunk = blockIdx.y, nchunk = gridDim.y, g0 = blockIdx.z * GB;
    const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = Q[9LL * ii + k];
    float M[J * GB];
    double S[J * GB];
    query_chunk<J, GB, LOO>(C, lw, n, j0, j1, ii, LOO ? (int)(blockIdx.x * THREADS) : 0, g0, G, q, sc, M, S);
    if (i >= m) return;
    const bool ok = finite9(q);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
        if (g0 + gb >= G) break;
#pragma unroll
        for (int a = 0; a < J; ++a) {
            const long long at = (((long long)(g0 + gb) * J + a) * nchunk + chunk) * m + i;
            pmax[at] = ok ? M[gb * J + a] : NAN;
            psum[at] = S[gb * J + a];
        }
    }
}

// grid (ceil(m / THREADS), J, G): out[g][a][i]
__global__ __launch_bounds__(THREADS) void so3_kernel_sum_final_kernel(const float *__restrict__ pmax, const double *__restrict__ psum,
                                                                       const double *__restrict__ log_z, const float *__restrict__ lw, int n,
                                                                       int m, int nchunk, Normalisers nm, int loo, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= m) return;
    const int a = blockIdx.y, J = gridDim.y, g = blockIdx.z;
    const long long at = ((long long)g * J + a) * nchunk * m + i;
    const double loo_lw = loo && lw ? (double)lw[(long long)g * n + i] : 0.0;
    out[((long long)g * J + a) * m + i] = combine(pmax + at, psum + at, m, nchunk, nm.l[a], log_z[g], loo != 0, loo_lw);
}
#endif  // __HIPCC__ && !RNF_KS_HOST_ONLY

// The workspace of one call, carved in this order (the parts of 8-byte elements first)
struct Workspace {
    double *psum;                                  // [G][J][nchunk][m]
    WeightPart *wpart;                             // [G][nchunk]
    double *log_z;                                 // [G]
    float *pmax;                                   // [G][J][nchunk][m]
    size_t bytes;                                  // 0: does not fit a size_t
};

inline Workspace carve(void *base, long long n, long long m, int G, int J) {
    Workspace w = {};
    const long double cells = (long double)G * J * (long double)chunks_for(n) * (long double)m;
    if (cells * 12.0L > 4.0e18L) return w;
    const size_t nc = (size_t)chunks_for(n), part = (size_t)G * J * nc * (size_t)m;
    const size_t wpart = part * 8, log_z = wpart + (size_t)G * nc * sizeof(WeightPart), pmax = log_z + (size_t)G * 8;
    w.bytes = (pmax + part * 4 + 15) & ~(size_t)15;
    if (!base) return w;
    char *p = static_cast<char *>(base);
    w.psum = reinterpret_cast<double *>(p);
    w.wpart = reinterpret_cast<WeightPart *>(p + wpart);
    w.log_z = reinterpret_cast<double *>(p + log_z);
    w.pmax = reinterpret_cast<float *>(p + pmax);
    return w;
}

// ---- the host evaluator: the same arithmetic in the same order (exp2f and exp of the host's libm in place of the device's) ----------

inline double host_log_z(const float *C, const float *lw, long long g, long long n) {
    const int nchunk = (int)chunks_for(n);
    std::vector<WeightPart> part(nchunk);
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        const long long j0 = (long long)chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
        float sm[THREADS];
        double sv[THREADS];
        bool bad = false;
        for (int t = 0; t < THREADS; ++t) {
            sm[t] = -INFINITY;
            for (long long j = j0 + t; j < j1; j += THREADS) {
                float l;
                weight_row(C, lw, g, n, j, l, bad);
                sm[t] = fmaxf(sm[t], l);
            }
        }
        for (int s = THREADS / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) sm[t] = fmaxf(sm[t], sm[t + s]);
        const float M = sm[0];
        for (int t = 0; t < THREADS; ++t) {
            sv[t] = 0.0;
            for (long long j = j0 + t; j < j1; j += THREADS) sv[t] += weight_term(lw ? lw[g * n + j] : 0.f, M);
        }
        for (int s = THREADS / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) sv[t] += sv[t + s];
        part[chunk] = WeightPart{sv[0], M, bad ? 1 : 0};
    }
    float lm[64], M = -INFINITY;
    double ls[64];
    bool bad = false;
    for (int l = 0; l < 64; ++l) lm[l] = weight_lane_max(part.data(), nchunk, l, bad);
    for (int l = 0; l < 64; ++l) M = fmaxf(M, lm[l]);                     // a maximum does not depend on its order
    for (int l = 0; l < 64; ++l) ls[l] = weight_lane_sum(part.data(), nchunk, l, M);
    for (int o = 32; o > 0; o >>= 1) {
        double nx[64];
        for (int l = 0; l < 64; ++l) nx[l] = ls[l] + ls[l ^ o];
        for (int l = 0; l < 64; ++l) ls[l] = nx[l];
    }
    return weight_log_z(M, ls[0], bad);
}

template <int J>
inline void host_queries(const float *C, const float *Q, const float *lw, long long n, long long m, int G, const Scales &sc,
                         const Normalisers &nm, bool loo, float *out) {
    const int nchunk = (int)chunks_for(n);
    std::vector<float> pmax((size_t)J * nchunk);
    std::vector<double> psum((size_t)J * nchunk);
    for (int g = 0; g < G; ++g) {
        const double log_z = host_log_z(C, lw, g, n);
        for (long long i = 0; i < m; ++i) {
            const float *q = Q + 9 * i;
            const int blk_lo = (int)(i / THREADS) * THREADS;
            for (int chunk = 0; chunk < nchunk; ++chunk) {
                const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : (int)n;
                float M[J];
                double S[J];
                if (loo)
                    query_chunk<J, 1, true>(C, lw, n, j0, j1, (int)i, blk_lo, g, G, q, sc, M, S);
                else
                    query_chunk<J, 1, false>(C, lw, n, j0, j1, (int)i, 0, g, G, q, sc, M, S);
                for (int a = 0; a < J; ++a) {
                    pmax[(size_t)a * nchunk + chunk] = finite9(q) ? M[a] : NAN;
                    psum[(size_t)a * nchunk + chunk] = S[a];
                }
            }
            for (int a = 0; a < J; ++a)
                out[((long long)g * J + a) * m + i] = combine(pmax.data() + (size_t)a * nchunk, psum.data() + (size_t)a * nchunk, 1, nchunk, nm.l[a],
                                                              log_z, loo, loo && lw ? (double)lw[(long long)g * n + i] : 0.0);
        }
    }
}

inline void scales_of(const double *kappas, int J, Scales &sc, Normalisers &nm) {
    for (int a = 0; a < MAX_J; ++a) {
        sc.h[a] = a < J ? (float)(0.5 * kappas[a] * LOG2E) : 0.f;
        nm.l[a] = a < J ? log_normaliser(kappas[a]) : 0.0;
    }
}

// out [G][J][m] of rnf_so3_kernel_sum on the host (Q null: the centres); arguments are not checked
inline void host_kernel_sum(const float *C, const float *Q, const float *lw, long long n, long long m, int G, const double *kappas, int J, bool loo,
                            float *out) {
    Scales sc;
    Normalisers nm;
    scales_of(kappas, J, sc, nm);
    if (!Q) Q = C;
    switch (J) {
        case 1: host_queries<1>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        case 2: host_queries<2>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        case 3: host_queries<3>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        case 4: host_queries<4>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        case 5: host_queries<5>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        case 6: host_queries<6>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        case 7: host_queries<7>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        case 8: host_queries<8>(C, Q, lw, n, m, G, sc, nm, loo, out); break;
        default: break;
    }
}

}  // namespace ks
}  // namespace rnf
