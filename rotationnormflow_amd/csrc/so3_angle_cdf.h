// so3_angle_cdf.h -- the distribution function of the geodesic angle from query rotations to a weighted set of rotations
// (rnf_so3_angle_cdf, include/rnf_hip.h): the mass of a ball about an estimate, its error radii and its expected error, from one
// pass over the pairs.  A top-hat kernel where so3_kernel_sum.h and so3_kernel_moments.h have the matrix-Fisher kernel.
//
// With centres C[n], queries Q[m] (shared by the G groups, or one set per group), G rows of log-weights (none: lw = 0),
// w_g = softmax(lw_g), d2_ij = ks::dist2(C_j, Q_i) = |Q_i - C_j|_F^2 = 8 sin^2(theta_ij / 2) and
// theta_ij = 2 asin(min(1, sqrt(d2_ij / 8))), per group g and query i:
//     mass[g][t][i]       = sum_j w_gj [d2_ij <= tau_t]          (T <= 8 thresholds, shared or one set per (group, query))
//     mean_angle[g][i]    = sum_j w_gj theta_ij                  (radians)
//     mean_sq_angle[g][i] = sum_j w_gj theta_ij^2
// The comparison is made on d2, never on an angle: the host build and the device agree on every indicator bit.  A shared threshold
// is an angle on the host, tau = (float)(8 sin^2(theta / 2)) formed in fp64 and rounded once; an angle >= pi is FLT_MAX, so that
// everything counts (d2 is capped at FLT_MAX).
//
// Arithmetic.  A normalising prepass writes wn[g][j] = (float)exp((double)lw_gj - log Z_g) with log Z_g from the weights pass of
// so3_kernel_sum.h and its finalise, as they are.  A centre with lw = -inf has wn = 0 exactly and drops out whatever its entries: d2
// is capped, so theta is finite, the indicator is 0 or 1, and 0 times either is 0.  A bad group (a NaN log-weight, a live centre that
// is not finite, no mass) has log Z = NaN, hence NaN weights, and every sum takes fma(wn, indicator, sum): NaN.  So no flags pass
// like so3_kernel_moments.h's is needed.  One sweep: there is no exponent of the distance, hence no maximum to take first.  Sums run
// in fp32 over one tile of 64 centres and in fp64 over the tiles of a chunk; fma(w, 1, s) = s + w and fma(w, 0, s) = s exactly, so a
// threshold's mass does not depend on the other T - 1.
//
// Shape of the hot kernel: a thread owns ONE (group, query) in registers; the centre index is wave-uniform, so the centre and its
// weight arrive by scalar loads and enter the VALU as scalar operands -- no LDS, no barrier, no cross-lane traffic.  Where the queries
// and the thresholds are shared, d2, the indicators and theta are computed once per pair for GROUPS_PER_THREAD = 4 groups.  The
// kernel is instantiated for 0, 1, 2, 4 and 8 threshold slots (a slot past T has tau = -1: it adds 0 and is not written) and with
// and without the angle moments, so that a mass-only call pays no sqrt and no asin.
//
// Determinism: as so3_kernel_sum.h.  Chunks of 4096 centres (a function of n alone); one fp64 partial per (group, chunk, query,
// slot); the finalise adds a query's chunks in chunk order in fp64 and rounds once to fp32 (a mass above 1 by rounding is 1).  No
// floating-point atomics.  A (group, query)'s outputs are bit-identical from run to run and whatever m, G, the query's position and
// the group's position are, whether the queries are given per group or shared, and however the thresholds are split over calls.
//
// Edge cases: a centre with lw = -inf is left out whatever its entries; any other non-finite centre, or a NaN log-weight, makes its
// group NaN; a non-finite query is NaN; a group with no mass is NaN; a NaN query_tau entry gives a NaN mass for that slot only;
// tau < 0 gives 0.
#pragma once
#if defined(RNF_AC_HOST_ONLY) && !defined(RNF_KS_HOST_ONLY)
#define RNF_KS_HOST_ONLY
#endif
#include "so3_kernel_sum.h"

namespace rnf {
namespace ac {

constexpr int MAX_T = 8;
constexpr int SMALL_BLOCK = 64;                    // one wave per block while blocks of THREADS would leave compute units idle
constexpr long long FEW_BLOCKS = 1024;             // 4 per compute unit of an MI355X
constexpr double PI = 3.14159265358979323846;
using ks::CHUNK;
using ks::GROUPS_PER_THREAD;
using ks::THREADS;
using ks::TILE;

// threads per block of the pairwise pass: m queries per group, zblocks = the groups (or sets of GROUPS_PER_THREAD groups) of the grid
inline int block_for(long long m, long long nchunk, long long zblocks) {
    return (m + THREADS - 1) / THREADS * nchunk * zblocks < FEW_BLOCKS ? SMALL_BLOCK : THREADS;
}

// the threshold slots of the kernel that serves T thresholds: 0, 1, 2, 4 or 8
inline int slots_for(int T) { return T <= 2 ? T : (T <= 4 ? 4 : MAX_T); }

// tau of a shared angle in radians: 8 sin^2(theta / 2) in fp64, rounded once; FLT_MAX from pi on
inline float tau_of(double theta) {
    if (theta >= PI) return FLT_MAX;
    const double s = sin(0.5 * theta);
    return (float)(8.0 * s * s);
}

struct Taus { float t[MAX_T]; };                   // the shared thresholds (-1 past T)

RNF_FM_HD float weight_norm(float l, double log_z) { return (float)exp((double)l - log_z); }

RNF_FM_HD float angle_of(float d2) { return 2.f * asinf(fminf(1.f, sqrtf(d2 * 0.125f))); }

// Centres ja..jb-1 of one tile against one query for GB groups g0..: acc[gb * NS + t] += wn [d2 <= tau[t]], and with MOM
// acc[gb * NS + TT] += wn theta, acc[gb * NS + TT + 1] += wn theta^2  (NS = TT + 2 MOM)
template <int TT, bool MOM, int GB>
RNF_FM_HD void cdf_tile(const float *__restrict__ C, const float *__restrict__ wn, long long n, int ja, int jb, int g0, int G, const float q[9],
                        const float *tau, float *acc) {
    constexpr int NS = TT + (MOM ? 2 : 0);
    constexpr int UNROLL = GB * NS > 32 ? 2 : 4;   // 4 groups of 10 slots: four centres in flight would spill scalar registers
#pragma unroll UNROLL
    for (int j = ja; j < jb; ++j) {
        const float d2 = ks::dist2(C + 9LL * j, q);
        float ind[TT > 0 ? TT : 1];
#pragma unroll
        for (int t = 0; t < TT; ++t) ind[t] = d2 <= tau[t] ? 1.f : 0.f;
        float th = 0.f, th2 = 0.f;
        if (MOM) {
            th = angle_of(d2);
            th2 = th * th;
        }
#pragma unroll
        for (int gb = 0; gb < GB; ++gb) {
            const int g = g0 + gb < G ? g0 + gb : G - 1;
            const float w = wn[(long long)g * n + j];
#pragma unroll
            for (int t = 0; t < TT; ++t) acc[gb * NS + t] = fmaf(w, ind[t], acc[gb * NS + t]);
            if (MOM) {
                acc[gb * NS + TT] = fmaf(w, th, acc[gb * NS + TT]);
                acc[gb * NS + TT + 1] = fmaf(w, th2, acc[gb * NS + TT + 1]);
            }
        }
    }
}

// One query against the centres j0..j1-1 of one chunk -> the chunk's sums S[GB * NS]: fp32 over a tile, fp64 over the tiles
template <int TT, bool MOM, int GB>
RNF_FM_HD void cdf_chunk(const float *__restrict__ C, const float *__restrict__ wn, long long n, int j0, int j1, int g0, int G, const float q[9],
                         const float *tau, double *S) {
    constexpr int NS = TT + (MOM ? 2 : 0);
#pragma unroll
    for (int s = 0; s < GB * NS; ++s) S[s] = 0.0;
    for (int ja = j0; ja < j1; ja += TILE) {
        const int jb = ja + TILE < j1 ? ja + TILE : j1;
        float part[GB * NS];
#pragma unroll
        for (int s = 0; s < GB * NS; ++s) part[s] = 0.f;
        cdf_tile<TT, MOM, GB>(C, wn, n, ja, jb, g0, G, q, tau, part);
#pragma unroll
        for (int s = 0; s < GB * NS; ++s) S[s] += (double)part[s];
    }
}

// One slot of one (group, query) from its chunk partials (stride: elements between chunks), in chunk order
RNF_FM_HD double chunk_sum(const double *psum, long long stride, int nchunk) {
    double S = 0.0;
    for (int c = 0; c < nchunk; ++c) S += psum[c * stride];
    return S;
}

// The mass of a slot: NaN for a query that is not finite or a NaN threshold, at most 1
RNF_FM_HD float finish_mass(double S, bool q_ok, float tau) {
    if (!q_ok || tau != tau) return NAN;
    return (float)(S > 1.0 ? 1.0 : S);
}
RNF_FM_HD float finish_moment(double S, bool q_ok) { return q_ok ? (float)S : NAN; }

}  // namespace ac
namespace sac {                                    // so3_set_angle_cdf.h: a query is a set of K = 1
// whether any of the K members of a set is live
RNF_FM_HD bool any_live(const float *Qs, int K) {
    bool live = false;
    for (int s = 0; s < K; ++s) live = live || ks::finite9(Qs + 9LL * s);
    return live;
}

#if defined(__HIPCC__) && !defined(RNF_AC_HOST_ONLY)       // the host builds of the tests define it: no device code to link
// The finalise of both entries, grid (ceil(m / THREADS), G): the outputs of (g, i) for sets of K members, Q [m][K][9]; null outputs
// are not written
__global__ __launch_bounds__(ks::THREADS) void so3_set_angle_cdf_final_kernel(const double *__restrict__ psum, const float *__restrict__ Q,
                                                                              long long q_group, int m, int K, int nchunk, int T, int mom,
                                                                              ac::Taus taus, const float *__restrict__ query_tau,
                                                                              float *__restrict__ mass, float *__restrict__ mean_angle,
                                                                              float *__restrict__ mean_sq_angle) {
    const long long i = (long long)blockIdx.x * ks::THREADS + threadIdx.x;
    if (i >= m) return;
    const int g = blockIdx.y, nsw = T + (mom ? 2 : 0);
    const bool q_ok = any_live(Q + (long long)g * q_group + 9LL * K * i, K);
    const double *p = psum + (long long)g * nsw * nchunk * m + i;
    const long long plane = (long long)nchunk * m;
    for (int t = 0; t < T; ++t) {
        const long long at = ((long long)g * T + t) * m + i;
        mass[at] = ac::finish_mass(ac::chunk_sum(p + t * plane, m, nchunk), q_ok, query_tau ? query_tau[at] : taus.t[t]);
    }
    if (mean_angle) mean_angle[(long long)g * m + i] = ac::finish_moment(ac::chunk_sum(p + T * plane, m, nchunk), q_ok);
    if (mean_sq_angle) mean_sq_angle[(long long)g * m + i] = ac::finish_moment(ac::chunk_sum(p + (T + 1) * plane, m, nchunk), q_ok);
}
#endif
}  // namespace sac
namespace ac {

#if defined(__HIPCC__) && !defined(RNF_AC_HOST_ONLY)       // the host builds of the tests define it: no device code to link
// grid (ceil(n / THREADS), G): wn[g][j]
__global__ __launch_bounds__(THREADS) void so3_angle_cdf_weights_kernel(const float *__restrict__ lw, const double *__restrict__ log_z, int n,
                                                                        float *__restrict__ wn) {
    const long long j = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (j >= n) return;
    const long long at = (long long)blockIdx.y * n + j;
    wn[at] = weight_norm(lw ? lw[at] : 0.f, log_z[blockIdx.y]);
}

// The pairwise pass: grid (ceil(m / block), nchunk, ceil(G / GB)), block = THREADS or, for few queries, SMALL_BLOCK threads (a thread
// owns its query whatever the block: the same bits).  psum [G][NSW][nchunk][m] with NSW = T + 2 MOM written slots (the masses first);
// q_group: floats between the query sets of two groups (0: shared); query_tau [G][T][m] or null (then taus.t).
template <int TT, bool MOM, int GB, bool PERQ>
__global__ __launch_bounds__(THREADS) void so3_angle_cdf_kernel(const float *__restrict__ C, const float *__restrict__ Q,
                                                                const float *__restrict__ wn, int n, int m, int G, long long q_group, Taus taus,
                                                                const float *__restrict__ query_tau, int T, double *__restrict__ psum) {
    constexpr int NS = TT + (MOM ? 2 : 0);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long ii = i < m ? i : m - 1;        // the threads past m repeat the last query and write nothing
    const int chunk = blockIdx.y, nchunk = gridDim.y, g0 = blockIdx.z * GB;
    const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    const float *qp = Q + (long long)g0 * q_group + 9 * ii;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = qp[k];
    double S[GB * NS];
    if (PERQ) {                                    // GB = 1: the thread's own thresholds, in registers
        float tau[TT > 0 ? TT : 1];
#pragma unroll
        for (int t = 0; t < TT; ++t) tau[t] = t < T ? query_tau[((long long)g0 * T + t) * m + ii] : -1.f;
        cdf_chunk<TT, MOM, GB>(C, wn, n, j0, j1, g0, G, q, tau, S);
    } else {
        cdf_chunk<TT, MOM, GB>(C, wn, n, j0, j1, g0, G, q, taus.t, S);
    }
    if (i >= m) return;
    const int nsw = T + (MOM ? 2 : 0);
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
        if (g0 + gb >= G) break;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int slot = s < TT ? s : T + (s - TT);                 // the moments follow the T masses
            if (s < TT && s >= T) continue;
            psum[(((long long)(g0 + gb) * nsw + slot) * nchunk + chunk) * m + i] = S[gb * NS + s];
        }
    }
}

#endif  // __HIPCC__ && !RNF_AC_HOST_ONLY

// The workspace of one call, carved in this order (the parts of 8-byte elements first); slots = T + 2 (with a moment output) or T
struct Workspace {
    double *psum;                                  // [G][slots][nchunk][m]
    ks::WeightPart *wpart;                         // [G][nchunk]
    double *log_z;                                 // [G]
    float *wn;                                     // [G][n]
    size_t bytes;                                  // 0: does not fit a size_t
};

inline Workspace carve(void *base, long long n, long long m, int G, int slots) {
    Workspace w = {};
    const long double cells = (long double)G * (long double)ks::chunks_for(n) * (long double)m;
    if (cells * 8.0L * slots + 4.0L * G * (long double)n > 4.0e18L) return w;
    const size_t nc = (size_t)ks::chunks_for(n), part = (size_t)G * nc * (size_t)m * (size_t)slots;
    const size_t wpart = part * 8, log_z = wpart + (size_t)G * nc * sizeof(ks::WeightPart), wn = log_z + (size_t)G * 8;
    w.bytes = (wn + (size_t)G * (size_t)n * 4 + 15) & ~(size_t)15;
    if (!base) return w;
    char *p = static_cast<char *>(base);
    w.psum = reinterpret_cast<double *>(p);
    w.wpart = reinterpret_cast<ks::WeightPart *>(p + wpart);
    w.log_z = reinterpret_cast<double *>(p + log_z);
    w.wn = reinterpret_cast<float *>(p + wn);
    return w;
}

// ---- the host evaluator: the same row functions in the same order (the host's libm in place of the device's) --------------------------

// A row of the outputs is one query here and one set in so3_set_angle_cdf.h: where it lies in Q, its chunk function, whether it counts
struct QueryRow {
    const float *q;
    static long long floats(int) { return 9; }
    QueryRow(const float *q_, int) : q(q_) {}
    bool ok() const { return ks::finite9(q); }
    template <int TT, bool MOM>
    void chunk(const float *C, const float *wn, long long n, int j0, int j1, const float *tau, double *S) const {
        cdf_chunk<TT, MOM, 1>(C, wn, n, j0, j1, 0, 1, q, tau, S);
    }
};

template <int TT, bool MOM, class Row>
inline void host_row(const float *C, const float *wn, long long n, const Row &row, const float *tau, int T, float *mass, long long mass_stride,
                     float *mean_angle, float *mean_sq_angle) {
    constexpr int NS = TT + (MOM ? 2 : 0);
    const int nchunk = (int)ks::chunks_for(n);
    std::vector<double> psum((size_t)(NS > 0 ? NS : 1) * nchunk);
    float tt[TT > 0 ? TT : 1];
    for (int t = 0; t < TT; ++t) tt[t] = t < T ? tau[t] : -1.f;
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : (int)n;
        double S[NS > 0 ? NS : 1];
        row.template chunk<TT, MOM>(C, wn, n, j0, j1, tt, S);
        for (int s = 0; s < NS; ++s) psum[(size_t)s * nchunk + chunk] = S[s];
    }
    const bool q_ok = row.ok();
    if (mass)
        for (int t = 0; t < T; ++t) mass[t * mass_stride] = finish_mass(chunk_sum(psum.data() + (size_t)t * nchunk, 1, nchunk), q_ok, tau[t]);
    if (MOM && mean_angle) *mean_angle = finish_moment(chunk_sum(psum.data() + (size_t)TT * nchunk, 1, nchunk), q_ok);
    if (MOM && mean_sq_angle) *mean_sq_angle = finish_moment(chunk_sum(psum.data() + (size_t)(TT + 1) * nchunk, 1, nchunk), q_ok);
}

// Q [m] rows of Row::floats(K) floats, or [G][m] with group_queries; lw [G][n] or null; thresholds: HOST double[T] angles, or null with
// query_tau [G][T][m]; mass [G][T][m], mean_angle and mean_sq_angle [G][m] may each be null; arguments are not checked
template <class Row>
inline void host_cdf(const float *C, const float *Q, int K, const float *lw, long long n, long long m, int G, bool group_queries, int T,
                     const double *thresholds, const float *query_tau, float *mass, float *mean_angle, float *mean_sq_angle) {
    const bool mom = mean_angle || mean_sq_angle;
    if (!mass) T = 0;
    std::vector<float> wn((size_t)n);
    for (int g = 0; g < G; ++g) {
        const double log_z = ks::host_log_z(C, lw, g, n);
        for (long long j = 0; j < n; ++j) wn[(size_t)j] = weight_norm(lw ? lw[(long long)g * n + j] : 0.f, log_z);
        for (long long i = 0; i < m; ++i) {
            const Row row(Q + ((group_queries ? (long long)g * m : 0) + i) * Row::floats(K), K);
            float tau[MAX_T];
            for (int t = 0; t < T; ++t) tau[t] = thresholds ? tau_of(thresholds[t]) : query_tau[((long long)g * T + t) * m + i];
            float *ms = mass ? mass + (long long)g * T * m + i : nullptr;
            float *ma = mean_angle ? mean_angle + (long long)g * m + i : nullptr, *m2 = mean_sq_angle ? mean_sq_angle + (long long)g * m + i : nullptr;
#define RNF_AC_HOST_CASE(TT)                                                                 \
    case TT:                                                                                 \
        if (mom) host_row<TT, true>(C, wn.data(), n, row, tau, T, ms, m, ma, m2);            \
        else host_row<TT, false>(C, wn.data(), n, row, tau, T, ms, m, ma, m2);               \
        break;
            switch (slots_for(T)) {
                case 0:
                    if (mom) host_row<0, true>(C, wn.data(), n, row, tau, T, ms, m, ma, m2);
                    break;
                RNF_AC_HOST_CASE(1) RNF_AC_HOST_CASE(2) RNF_AC_HOST_CASE(4) RNF_AC_HOST_CASE(8)
            }
#undef RNF_AC_HOST_CASE
        }
    }
}

// Q [m][9], or [G][m][9] with group_queries
inline void host_angle_cdf(const float *C, const float *Q, const float *lw, long long n, long long m, int G, bool group_queries, int T,
                           const double *thresholds, const float *query_tau, float *mass, float *mean_angle, float *mean_sq_angle) {
    host_cdf<QueryRow>(C, Q, 1, lw, n, m, G, group_queries, T, thresholds, query_tau, mass, mean_angle, mean_sq_angle);
}

}  // namespace ac
}  // namespace rnf
