// so3_set_angle_cdf.h -- the distribution function of the geodesic angle from a weighted set of rotations to the NEAREST member of a
// set of query rotations (rnf_so3_set_angle_cdf, include/rnf_hip.h): the error about an estimate of a symmetric object (the set is
// the estimate's orbit under the object's symmetry group) and the best-of-k error of k modes (the set is the modes).  so3_angle_cdf.h
// with a min over members inside the pairwise pass; the indicator of a union of balls is not a sum of the balls' indicators, so no
// composition of rnf_so3_angle_cdf calls gives it.
//
// Centres C[n], log-weights [G][n] or none, groups, thresholds, weights w_g = softmax(lw_g) as so3_angle_cdf.h.  Queries are m sets
// of K members, Q[m][K] shared by the groups or Q[G][m][K].  A member is live when its nine entries are finite; any other member is
// padding (sets of unequal size are padded to K).  With
//     d2_ijs = ks::dist2(C_j, Q_is)      (FLT_MAX for padding: ks::dist2 caps a NaN or an overflow at FLT_MAX)
//     d2_ij  = min_s d2_ijs,   theta_ij = ac::angle_of(d2_ij)
// mass, mean_angle and mean_sq_angle are so3_angle_cdf.h's sums over j.  A set with no live member is NaN in all of its outputs.
// min is exact: the outputs depend neither on the order of the members nor on padding among them, and with K = 1 every output has the
// bits of rnf_so3_angle_cdf.
//
// Arithmetic and determinism: so3_angle_cdf.h's.  The weights pass, its finalise, ac::weight_norm, the per-centre indicator and
// moment code and the finalise's row functions are the same; a tile's minima are complete before its centres are summed in index
// order, so the fp32 sums over a tile, the fp64 sums over the tiles of a chunk and the finalise in chunk order are those of
// so3_angle_cdf.h with d2_ij in place of the single distance.
//
// Shape of the hot kernels: for many sets a thread owns ONE (group, set), or one set for groups_for(NS) groups that share sets and
// thresholds.  The centre index is wave-uniform (scalar loads, scalar operands).  Per tile of 64 centres the thread holds the 64
// running minima in registers -- the tile loops are fully unrolled, so they are statically indexed -- walks its members in the outer
// loop (nine loads, the next member's issued before this one's arithmetic), and runs the indicator and moment code once per centre on
// the minima.  A slot past the end of a ragged tile repeats the tile's last centre in the min phase and is not summed.  No LDS, no
// barrier, no cross-lane traffic, no floating-point atomics.  For few sets (wave_per_set) a wave owns one (group, set, chunk) and its
// lanes share out the members, with the same bits; see so3_set_angle_cdf_wave_kernel.
#pragma once
#if defined(RNF_SAC_HOST_ONLY) && !defined(RNF_AC_HOST_ONLY)
#define RNF_AC_HOST_ONLY
#endif
#include "so3_angle_cdf.h"

namespace rnf {
namespace sac {

constexpr int MAX_K = 4096;                        // members of a set: a cylinder sampled at 1 degree has 720
using ac::MAX_T;
using ac::Taus;
using ks::CHUNK;
using ks::THREADS;
using ks::TILE;

// groups per thread where the groups share sets and thresholds: the minima are shared; 64 minima, GB * NS fp32 and fp64 sums stay
// clear of spills
constexpr int groups_for(int NS) { return NS <= 6 ? 4 : 2; }

// A wave per (group, set, chunk) in place of a thread per (group, set), where the sets are few and have members enough to share out:
// at most 4096 waves (4 per SIMD of an MI355X) and K >= 8.  The same bits either way.
constexpr int WAVE_MIN_K = 8;
constexpr long long WAVE_MAX_WAVES = 4096;
inline bool wave_per_set(long long m, long long nchunk, long long G, int K) { return K >= WAVE_MIN_K && m * nchunk * G <= WAVE_MAX_WAVES; }

// The tile's centres are the same for every member, and the compiler would lift their 576 scalar loads out of the member loop and
// spill them; an offset it cannot see through keeps the loads inside the loop, where they stream through a few scalar registers.
RNF_FM_HD int opaque_zero() {
    int zero = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(zero));
    zero = __builtin_amdgcn_readfirstlane(zero);   // wave-uniform to the compiler: the loads stay scalar
#endif
    return zero;
}

// dmin[jj] = min(dmin[jj], d2(Ct[jj], q)) for the tile's centres Ct[0..last]; a slot past `last` repeats centre `last`.  FULL: last =
// TILE - 1, known when compiling, so that every load has an immediate offset.
template <bool FULL>
RNF_FM_HD void min_tile(const float *__restrict__ Ct, int last, const float q[9], float dmin[TILE]) {
#pragma unroll
    for (int jj = 0; jj < TILE; ++jj) {
        const int j = FULL || jj < last ? jj : last;
        dmin[jj] = fminf(dmin[jj], ks::dist2(Ct + 9 * j, q));
    }
}

// The minima of the tile's centres ja..jb-1 over the K members of one set
template <bool FULL>
RNF_FM_HD void set_minima(const float *__restrict__ C, int ja, int jb, const float *__restrict__ Qs, int K, float dmin[TILE]) {
#pragma unroll
    for (int jj = 0; jj < TILE; ++jj) dmin[jj] = FLT_MAX;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = Qs[k];
    for (int s = 0; s < K; ++s) {
        const float *nx = Qs + 9LL * (s + 1 < K ? s + 1 : s);
        float qn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) qn[k] = nx[k];
        const int zero = opaque_zero();
        min_tile<FULL>(C + 9LL * ja + zero, jb - ja - 1 + zero, q, dmin);          // a ragged tile's clamped indices likewise
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k] = qn[k];
    }
}

// ac::cdf_tile's code for one centre with the minimum d2 and the centre's weight w[gb] in each of GB groups:
// acc[gb * NS + t] += w[gb] [d2 <= tau[t]] and the two moments
template <int TT, bool MOM, int GB>
RNF_FM_HD void sum_centre(float d2, const float *w, const float *tau, float *acc) {
    constexpr int NS = TT + (MOM ? 2 : 0);
    float ind[TT > 0 ? TT : 1];
#pragma unroll
    for (int t = 0; t < TT; ++t) ind[t] = d2 <= tau[t] ? 1.f : 0.f;
    float th = 0.f, th2 = 0.f;
    if (MOM) {
        th = ac::angle_of(d2);
        th2 = th * th;
    }
#pragma unroll
    for (int gb = 0; gb < GB; ++gb) {
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[gb * NS + t] = fmaf(w[gb], ind[t], acc[gb * NS + t]);
        if (MOM) {
            acc[gb * NS + TT] = fmaf(w[gb], th, acc[gb * NS + TT]);
            acc[gb * NS + TT + 1] = fmaf(w[gb], th2, acc[gb * NS + TT + 1]);
        }
    }
}

// The centres ja..jb-1 of a tile in index order, on their minima
template <int TT, bool MOM, int GB>
RNF_FM_HD void sum_tile(const float *__restrict__ wn, long long n, int ja, int jb, int g0, int G, const float dmin[TILE], const float *tau,
                        float *acc) {
#pragma unroll
    for (int jj = 0; jj < TILE; ++jj) {
        if (ja + jj >= jb) continue;               // no break: the loop unrolls fully and dmin stays in registers
        float w[GB];
#pragma unroll
        for (int gb = 0; gb < GB; ++gb) w[gb] = wn[(long long)(g0 + gb < G ? g0 + gb : G - 1) * n + ja + jj];
        sum_centre<TT, MOM, GB>(dmin[jj], w, tau, acc);
    }
}

// One set against the centres j0..j1-1 of one chunk -> the chunk's sums S[GB * NS]: fp32 over a tile, fp64 over the tiles
template <int TT, bool MOM, int GB>
RNF_FM_HD void set_chunk(const float *__restrict__ C, const float *__restrict__ wn, long long n, int j0, int j1, int g0, int G,
                         const float *__restrict__ Qs, int K, const float *tau, double *S) {
    constexpr int NS = TT + (MOM ? 2 : 0);
#pragma unroll
    for (int s = 0; s < GB * NS; ++s) S[s] = 0.0;
    for (int ja = j0; ja < j1; ja += TILE) {
        const int jb = ja + TILE < j1 ? ja + TILE : j1;
        float dmin[TILE];
        float part[GB * NS];
#pragma unroll
        for (int s = 0; s < GB * NS; ++s) part[s] = 0.f;
        if (jb - ja == TILE) set_minima<true>(C, ja, jb, Qs, K, dmin);
        else set_minima<false>(C, ja, jb, Qs, K, dmin);
        sum_tile<TT, MOM, GB>(wn, n, ja, jb, g0, G, dmin, tau, part);
#pragma unroll
        for (int s = 0; s < GB * NS; ++s) S[s] += (double)part[s];
    }
}

#if defined(__HIPCC__) && !defined(RNF_SAC_HOST_ONLY)      // the host builds of the tests define it: no device code to link
// The pairwise pass: grid (ceil(m / block), nchunk, ceil(G / GB)), block = THREADS or, for few sets, ac::SMALL_BLOCK threads (a thread
// owns its set whatever the block: the same bits).  Q [m][K][9]; q_group: floats between the sets of two groups (0: shared); psum and
// query_tau as so3_angle_cdf_kernel's.
template <int TT, bool MOM, int GB, bool PERQ>
__global__ __launch_bounds__(THREADS) void so3_set_angle_cdf_kernel(const float *__restrict__ C, const float *__restrict__ Q,
                                                                    const float *__restrict__ wn, int n, int m, int K, int G, long long q_group,
                                                                    Taus taus, const float *__restrict__ query_tau, int T,
                                                                    double *__restrict__ psum) {
    constexpr int NS = TT + (MOM ? 2 : 0);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long ii = i < m ? i : m - 1;        // the threads past m repeat the last set and write nothing
    const int chunk = blockIdx.y, nchunk = gridDim.y, g0 = blockIdx.z * GB;
    const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    const float *Qs = Q + (long long)g0 * q_group + 9LL * K * ii;
    double S[GB * NS];
    if (PERQ) {                                    // GB = 1: the thread's own thresholds, in registers
        float tau[TT > 0 ? TT : 1];
#pragma unroll
        for (int t = 0; t < TT; ++t) tau[t] = t < T ? query_tau[((long long)g0 * T + t) * m + ii] : -1.f;
        set_chunk<TT, MOM, GB>(C, wn, n, j0, j1, g0, G, Qs, K, tau, S);
    } else {
        set_chunk<TT, MOM, GB>(C, wn, n, j0, j1, g0, G, Qs, K, taus.t, S);
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

// Few sets: a thread per set leaves most of the machine idle (64 sets are one wave per chunk and group, its threads walking K members
// each), so there a WAVE owns one (group, set, chunk): grid (m, nchunk, G), one wave per block.  Lane l takes the members l, l + 64,
// ... against the tile's 64 centres (the same min_tile, the centre index still wave-uniform); a butterfly of 63 shuffles and mins
// leaves the minimum over all lanes for centre ja + l in lane l; then every lane runs sum_centre on the centres in index order, d2 and
// the weight read from their lanes -- the same instructions on the same numbers as the thread that owns a set: the same bits.
template <int O>
__device__ inline void scatter_min_stage(float v[TILE], int lane) {
    const bool hi = (lane & O) != 0;
#pragma unroll
    for (int i = 0; i < O; ++i) {
        const float keep = hi ? v[i + O] : v[i], send = hi ? v[i] : v[i + O];
        v[i] = fminf(keep, __shfl_xor(send, O, 64));
    }
}

// v[jj] of every lane -> the minimum over the lanes of v[lane], in lane `lane`
__device__ inline float scatter_min(float v[TILE], int lane) {
    scatter_min_stage<32>(v, lane);
    scatter_min_stage<16>(v, lane);
    scatter_min_stage<8>(v, lane);
    scatter_min_stage<4>(v, lane);
    scatter_min_stage<2>(v, lane);
    scatter_min_stage<1>(v, lane);
    return v[0];
}

template <bool FULL>
__device__ inline void wave_minima(const float *__restrict__ C, int ja, int jb, const float *__restrict__ Qs, int K, int lane, float dmin[TILE]) {
#pragma unroll
    for (int jj = 0; jj < TILE; ++jj) dmin[jj] = FLT_MAX;
    for (int s = lane; s < K; s += 64) {
        float q[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k] = Qs[9LL * s + k];
        const int zero = opaque_zero();
        min_tile<FULL>(C + 9LL * ja + zero, jb - ja - 1 + zero, q, dmin);
    }
}

__device__ inline float lane_value(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

template <int TT, bool MOM, bool PERQ>
__global__ __launch_bounds__(64) void so3_set_angle_cdf_wave_kernel(const float *__restrict__ C, const float *__restrict__ Q,
                                                                    const float *__restrict__ wn, int n, int m, int K, long long q_group, Taus taus,
                                                                    const float *__restrict__ query_tau, int T, double *__restrict__ psum) {
    constexpr int NS = TT + (MOM ? 2 : 0);
    const int lane = threadIdx.x, i = blockIdx.x, chunk = blockIdx.y, nchunk = gridDim.y, g = blockIdx.z;
    const int j0 = chunk * CHUNK, j1 = j0 + CHUNK < n ? j0 + CHUNK : n;
    const float *Qs = Q + (long long)g * q_group + 9LL * K * i;
    const float *wg = wn + (long long)g * n;
    float tau[TT > 0 ? TT : 1];
#pragma unroll
    for (int t = 0; t < TT; ++t) tau[t] = t < T ? (PERQ ? query_tau[((long long)g * T + t) * m + i] : taus.t[t]) : -1.f;
    double S[NS > 0 ? NS : 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) S[s] = 0.0;
    for (int ja = j0; ja < j1; ja += TILE) {
        const int jb = ja + TILE < j1 ? ja + TILE : j1;
        float dmin[TILE];
        if (jb - ja == TILE) wave_minima<true>(C, ja, jb, Qs, K, lane, dmin);
        else wave_minima<false>(C, ja, jb, Qs, K, lane, dmin);
        const float d2 = scatter_min(dmin, lane);
        const float w = ja + lane < jb ? wg[ja + lane] : 0.f;
        float part[NS > 0 ? NS : 1];
#pragma unroll
        for (int s = 0; s < NS; ++s) part[s] = 0.f;
        for (int jj = 0; jj < jb - ja; ++jj) {
            const float ws = lane_value(w, jj);
            sum_centre<TT, MOM, 1>(lane_value(d2, jj), &ws, tau, part);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) S[s] += (double)part[s];
    }
    if (lane != 0) return;
    const int nsw = T + (MOM ? 2 : 0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int slot = s < TT ? s : T + (s - TT);                     // the moments follow the T masses
        if (s < TT && s >= T) continue;
        psum[(((long long)g * nsw + slot) * nchunk + chunk) * m + i] = S[s];
    }
}

// The finalise, so3_set_angle_cdf_final_kernel, is in so3_angle_cdf.h: rnf_so3_angle_cdf launches it with K = 1.
#endif  // __HIPCC__ && !RNF_SAC_HOST_ONLY

// The workspace is ac::carve's for m sets: it does not grow with K.

// ---- the host evaluator: ac::host_cdf on sets ------------------------------------------------------------------------------------------

struct SetRow {
    const float *Qs;
    int K;
    static long long floats(int K) { return 9LL * K; }
    SetRow(const float *Qs_, int K_) : Qs(Qs_), K(K_) {}
    bool ok() const { return any_live(Qs, K); }
    template <int TT, bool MOM>
    void chunk(const float *C, const float *wn, long long n, int j0, int j1, const float *tau, double *S) const {
        set_chunk<TT, MOM, 1>(C, wn, n, j0, j1, 0, 1, Qs, K, tau, S);
    }
};

// Q [m][K][9], or [G][m][K][9] with group_queries; the other arguments as ac::host_angle_cdf; arguments are not checked
inline void host_set_angle_cdf(const float *C, const float *Q, const float *lw, long long n, long long m, int K, int G, bool group_queries, int T,
                               const double *thresholds, const float *query_tau, float *mass, float *mean_angle, float *mean_sq_angle) {
    ac::host_cdf<SetRow>(C, Q, K, lw, n, m, G, group_queries, T, thresholds, query_tau, mass, mean_angle, mean_sq_angle);
}

}  // namespace sac
}  // namespace rnf
