// grid_locate.h -- from a rotation back to its cell of the equivolumetric SO(3) grid (rnf_so3_grid_locate), the histogram of rotations over
// the cells, and the fit of such a histogram against a density on the grid (rnf_grid_fit, include/rnf_hip.h).
//
// Locate is the inverse of so3_grid.h's grid_row.  With R' = R O^T = Rx(phi) Rz(theta) Rx(tau): z = R'00, sin(theta) = hypot(R'10, R'20),
// phi = atan2(R'20, R'10), tau = atan2(R'02, -R'01); the pixel is ang2pix in the RING ordering at nside = 2^level (Gorski et al. 2005;
// in the polar caps with sin(theta) itself, tmp = nside sin(theta) / sqrt((1 + |z|) / 3), which keeps its digits near the poles where
// sqrt(1 - z^2) has lost them), the tilt is rint(tau / tilt_step) modulo 6 nside, the row t * npix + p.  At a pole (R'10 = R'20 = 0 exactly)
// only phi + tau (north) or tau - phi (south) is defined: phi = 0 and tau from the lower right 2x2 block.  fp64 from the fp32 entries, one
// thread per rotation.  A cell is the set of rotations that land on its row: the cells partition SO(3) into 72 * 8^level parts of equal
// Haar volume (HEALPix pixels have equal area, tilt cells equal length), each holds its grid rotation, and none of them is the Voronoi
// cell of that rotation.
// Whatever the input -- a matrix that is no rotation, an offset that is none -- the row is either -1 (a non-finite entry) or inside
// 0..Q-1: tmp is capped at nside and the ring and pixel-in-ring indices are clamped, so the histogram's atomic never leaves its image.
//
// Histogram: counts[b][row] += 1 by an integer atomic.  Integer sums do not depend on their order (the argument of grid_credible.h), so
// the counts are bit-identical from run to run although the atomics land in any order.
//
// Fit: image b's maximum M by grid_modes.h's arg-max pass, then ONE grid-stride pass over (lp_i, c_i) with w_i = expf(lp_i - M):
//   Z = sum w_i, S1 = sum c_i log c_i, S2 = sum c_i (lp_i - M), S3 = sum c_i^2 / w_i over the cells with c_i > 0 (fp64), and the integers
//   n = sum c_i and the number of occupied cells;
// a one-workgroup-per-image finalise sums the block partials in index order and writes the statistics.  Blocks per image depend on Q alone
// (blocks_for), threads walk their rows in a fixed order, blocks reduce with fixed shuffle trees, no floating-point atomics: bit-identical
// from run to run and whatever number of images share a call.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "grid_modes.h"
#include "so3_grid.h"

namespace rnf {
namespace gl {

constexpr int THREADS = 256;                      // 4 waves of 64
constexpr long long MAX_Q = 1LL << 26;            // of a histogram and of a fit (rnf_grid_credible's limit: level 6 fits)
constexpr long long ROWS_PER_BLOCK = 8192;
constexpr long long MAX_BLOCKS = 512;
constexpr int N_STATS = 7;                        // RNF_GRID_FIT_STATS

// blocks of one image in the fit pass: a function of Q alone (the determinism rule above)
inline long long blocks_for(long long Q) {
    const long long b = (Q + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    return b < MAX_BLOCKS ? b : MAX_BLOCKS;
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

// the row of rotation r[9] (fp32, row-major) in the level-`level` grid times O (o: row-major fp64); -1 for a non-finite entry
__device__ __forceinline__ long long locate_row(int level, const float *r, const double *o) {
    double a[9];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 9; ++c) finite = finite && fabsf(r[c]) < INFINITY;
#pragma unroll
    for (int row = 0; row < 3; ++row)
#pragma unroll
        for (int col = 0; col < 3; ++col)         // R O^T
            a[row * 3 + col] = (double)r[row * 3] * o[col * 3] + (double)r[row * 3 + 1] * o[col * 3 + 1] + (double)r[row * 3 + 2] * o[col * 3 + 2];
#pragma unroll
    for (int c = 0; c < 9; ++c) finite = finite && fabs(a[c]) < (double)INFINITY;
    if (!finite) return -1;
    const long long nside = 1LL << level, npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1), nl4 = 4 * nside;
    const long long tilts = 6 * nside;
    const double z = fmin(fmax(a[0], -1.0), 1.0), za = fabs(z);
    const double sth = hypot(a[3], a[6]);
    double phi, tau;
    if (a[3] == 0.0 && a[6] == 0.0) {             // a pole: the azimuth is free, the tilt takes all of the in-plane angle
        phi = 0.0;
        tau = z > 0.0 ? atan2(a[7], a[4]) : atan2(a[7], a[8]);
    } else {
        phi = atan2(a[6], a[3]);
        tau = atan2(a[2], -a[1]);
    }
    double tt = phi * (2.0 / M_PI);               // in [0, 4)
    if (tt < 0.0) tt += 4.0;
    if (tt >= 4.0) tt -= 4.0;
    long long p;
    if (za <= 2.0 / 3.0) {                        // the belt
        const double t1 = (double)nside * (0.5 + tt), t2 = (double)nside * z * 0.75;
        const long long jp = (long long)floor(t1 - t2), jm = (long long)floor(t1 + t2);      // ascending and descending edge lines
        const long long ir = clampll(nside + 1 + jp - jm, 1, 2 * nside + 1);                 // ring, counted from the belt's first
        const long long kshift = 1 - (ir & 1);
        const long long ip = ((jp + jm - nside + kshift + 1 + 2 * nl4) >> 1) & (nl4 - 1);
        p = ncap + (ir - 1) * nl4 + ip;
    } else {                                      // the caps
        const double tp = tt - floor(tt);
        const double tmp = fmin((double)nside * sth / sqrt((1.0 + za) / 3.0), (double)nside);
        const long long jp = (long long)floor(tp * tmp), jm = (long long)floor((1.0 - tp) * tmp);
        const long long ir = clampll(jp + jm + 1, 1, nside);                                 // ring, counted from the closest pole
        const long long ip = clampll((long long)floor(tt * (double)ir), 0, 4 * ir - 1);
        p = z > 0.0 ? 2 * ir * (ir - 1) + ip : npix - 2 * ir * (ir + 1) + ip;
    }
    const long long k = (long long)rint(tau / (2.0 * M_PI / (double)tilts));                 // |k| <= 3 nside
    const long long t = ((k % tilts) + tilts) % tilts;
    return t * npix + clampll(p, 0, npix - 1);
}

// one thread per rotation: rows_out[k] (optional) the row of rotation k of [g][n]; counts[b][row] += 1 (optional; rows -1 are skipped)
__global__ __launch_bounds__(THREADS) void so3_grid_locate_kernel(int level, long long n, long long total, const float *rot,
                                                                  const float *offset, long long *rows_out, int *counts) {
    double o[9];
    so3g::load_offset(offset, o);
    const long long Q = 72LL << (3 * level);
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
        float r[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) r[c] = rot[k * 9 + c];
        const long long row = locate_row(level, r, o);
        if (rows_out) rows_out[k] = row;
        if (counts && row >= 0 && row < Q) atomicAdd(counts + (k / n) * Q + row, 1);
    }
}

struct FitPart {                                  // one block's partial sums: 48 bytes
    double Z, S1, S2, S3;
    long long n, occupied;
};

// the workspace of one rnf_grid_fit call, carved in this order (every part 8-byte aligned but the last)
struct Workspace {
    gm::ArgPart *max_part;                        // [g][gm::blocks_for(Q)]
    FitPart *part;                                // [g][blocks_for(Q)]
    long long *max_index;                         // [g]
    float *max_value;                             // [g]: M
    size_t bytes;
};

inline Workspace carve(void *base, long long Q, int g) {
    const size_t ng = (size_t)g;
    const size_t max_part = 0, part = max_part + ng * (size_t)gm::blocks_for(Q) * sizeof(gm::ArgPart);
    const size_t max_index = part + ng * (size_t)blocks_for(Q) * sizeof(FitPart), max_value = max_index + ng * 8;
    Workspace w = {};
    w.bytes = (max_value + ng * 4 + 15) & ~(size_t)15;
    if (!base) return w;                          // the size alone (rnf_grid_fit_workspace_bytes)
    char *p = static_cast<char *>(base);
    w.max_part = reinterpret_cast<gm::ArgPart *>(p + max_part);
    w.part = reinterpret_cast<FitPart *>(p + part);
    w.max_index = reinterpret_cast<long long *>(p + max_index);
    w.max_value = reinterpret_cast<float *>(p + max_value);
    return w;
}

// the block's integer sum, valid in thread 0
__device__ __forceinline__ long long block_sum_ll(long long v) {
    __shared__ long long sw[THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < THREADS / 64; ++q) v += sw[q];
    __syncthreads();
    return v;
}

// the pass: grid (nb, g); part[b][nb]
__global__ __launch_bounds__(THREADS) void grid_fit_kernel(const float *logp, const int *counts, long long Q, const float *max_value,
                                                           FitPart *part) {
    const int b = blockIdx.y, nb = gridDim.x;
    const float M = max_value[b];
    const float *lp = logp + (long long)b * Q;
    const int *cn = counts + (long long)b * Q;
    double Z = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0;
    long long n = 0, occupied = 0;
    for (long long r = (long long)blockIdx.x * THREADS + threadIdx.x; r < Q; r += (long long)nb * THREADS) {
        const float x = lp[r];
        const int c = cn[r];
        const double w = M == -INFINITY ? 0.0 : (double)expf(x - M);         // no finite value in the row: no mass anywhere
        Z += w;
        if (c > 0) {                              // an empty cell adds to Z alone: no 0 * inf
            const double cd = (double)c;
            S1 += cd * log(cd);
            S2 += w > 0.0 ? cd * ((double)x - (double)M) : -(double)INFINITY;   // a sample in a cell without mass
            S3 += cd * cd / w;
            n += c;
            ++occupied;
        }
    }
    Z = gm::block_sum(Z);
    S1 = gm::block_sum(S1);
    S2 = gm::block_sum(S2);
    S3 = gm::block_sum(S3);
    n = block_sum_ll(n);
    occupied = block_sum_ll(occupied);
    if (threadIdx.x == 0) part[(long long)b * nb + blockIdx.x] = FitPart{Z, S1, S2, S3, n, occupied};
}

// the finalise: grid (g); stats[b][N_STATS] = {log_norm, log_likelihood, grid_log_likelihood, g_stat, chi2, n, occupied}
__global__ __launch_bounds__(THREADS) void grid_fit_final_kernel(const FitPart *part, int nb, long long Q, const float *max_value,
                                                                 double *stats) {
    const int b = blockIdx.x;
    double Z = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0;
    long long n = 0, occupied = 0;
    for (int q = threadIdx.x; q < nb; q += THREADS) {
        const FitPart p = part[(long long)b * nb + q];
        Z += p.Z;
        S1 += p.S1;
        S2 += p.S2;
        S3 += p.S3;
        n += p.n;
        occupied += p.occupied;
    }
    Z = gm::block_sum(Z);
    S1 = gm::block_sum(S1);
    S2 = gm::block_sum(S2);
    S3 = gm::block_sum(S3);
    n = block_sum_ll(n);
    occupied = block_sum_ll(occupied);
    if (threadIdx.x != 0) return;
    const double M = (double)max_value[b], nd = (double)n;
    double *out = stats + (long long)b * N_STATS;
    out[5] = nd;
    out[6] = (double)occupied;
    if (M != M || M == (double)INFINITY) {        // a NaN in the row, or a +inf maximum
        for (int v = 0; v < 5; ++v) out[v] = NAN;
        return;
    }
    const double log_norm = M + log(Z) - log((double)Q);                     // -inf for a row without a finite value
    out[0] = log_norm;
    if (n == 0) {
        for (int v = 1; v < 5; ++v) out[v] = NAN;
    } else if (S2 == -(double)INFINITY) {         // a sample in a cell without mass
        out[1] = -(double)INFINITY;
        out[2] = -(double)INFINITY - log_norm;    // NaN when the row has no mass at all
        out[3] = (double)INFINITY;
        out[4] = (double)INFINITY;
    } else {
        const double ll = M + S2 / nd;
        out[1] = ll;
        out[2] = ll - log_norm;
        out[3] = 2.0 * (S1 - S2 + nd * log(Z) - nd * log(nd));
        out[4] = Z * S3 / nd - nd;
    }
}

}  // namespace gl
}  // namespace rnf
