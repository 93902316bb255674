// grid_modes.h -- top-k pose modes and their probability mass on the equivolumetric SO(3) grid (rnf_grid_modes, include/rnf_hip.h).
//
// Image b's log-densities lp[b][0..Q) on the grid rows R_i (float[Q][9], rnf_so3_healpix_grid) are reduced in k + 1 grid-stride passes,
// each followed by a one-workgroup-per-image finalise:
//   pass j < k  arg-max of lp over the rows i with tr(M_m^T R_i) <= thr for every earlier mode m (thr = 1 + 2 cos(sep); sep = pi: no row),
//               first index on a tie, a NaN wins (torch.argmax); the finalise writes mode j to index_out / logp_out, -1 / -inf when no row
//               qualifies or an earlier mode is missing or mode 0 is NaN;
//   pass k      with M = mode 0's value and w_i = exp(lp_i - M) (fp32 exp, fp64 sums): S = sum w_i, the mass of every mode's region (the
//               rows within sep of mode j, tr > thr, and of no earlier mode) and, with ground truths, sum w_i min_g acos(clip((tr(G^T R_i)
//               - 1) / 2)) (min_geodesic_kernel's formula); the finalise writes log_norm = M + log(S / Q), mass_j = sum_j / S, spread.
// Determinism: the block count of a pass depends only on Q (blocks_for), every thread walks its rows in a fixed order, blocks reduce with
// fixed shuffle trees and the finalise sums the block partials in a fixed order -- no atomics, so results are bit-identical from run to run
// and whatever number of images share a launch.  Grid rows are staged through LDS 256 at a time with 16-byte loads; the modes and the
// ground truths of the image stay in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rnf {
namespace gm {

constexpr int THREADS = 256;                      // 4 waves of 64
constexpr int MAX_K = 16;
constexpr int MAX_GT = 128;                       // ground truths per image (SYMSOL's icosahedron has 60)
constexpr long long ROWS_PER_BLOCK = 2048;
constexpr long long MAX_BLOCKS = 2048;

// blocks of one image in every pass: a function of Q alone (the determinism rule above)
inline long long blocks_for(long long Q) {
    const long long b = (Q + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    return b < MAX_BLOCKS ? b : MAX_BLOCKS;
}

struct ArgPart {                                  // one block's arg-max: 16 bytes, written as one vector store
    float v;
    int32_t pad;
    long long i;
};

// (v, i) beats (bv, bi): an index < 0 is "none"; a NaN beats any number; otherwise the larger value, then the smaller index
__device__ __forceinline__ bool arg_better(float v, long long i, float bv, long long bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ float trace9(const float *a, const float *r) {          // tr(A^T R) in min_geodesic_kernel's order
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < 9; ++c) t = fmaf(r[c], a[c], t);
    return t;
}

// rows [r0, r0 + rows) of the grid into LDS; r0 is a multiple of THREADS, so the source is 16-byte aligned when the grid is
__device__ __forceinline__ void load_tile(const float *grid, long long r0, int rows, float4 *tile4) {
    const float4 *src4 = reinterpret_cast<const float4 *>(grid + r0 * 9);
    const int n = rows * 9, n4 = n >> 2;
    for (int q = threadIdx.x; q < n4; q += THREADS) tile4[q] = src4[q];
    float *tile = reinterpret_cast<float *>(tile4);
    for (int q = (n4 << 2) + threadIdx.x; q < n; q += THREADS) tile[q] = grid[r0 * 9 + q];
}

__device__ __forceinline__ void wave_arg(float &bv, long long &bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(bv, off, 64);
        const long long oi = __shfl_down(bi, off, 64);
        if (arg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}

// the block's arg-max, valid in thread 0
__device__ __forceinline__ void block_arg(float &bv, long long &bi) {
    __shared__ float sv[THREADS / 64];
    __shared__ long long si[THREADS / 64];
    wave_arg(bv, bi);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sv[w] = bv; si[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < THREADS / 64; ++q)
            if (arg_better(sv[q], si[q], bv, bi)) { bv = sv[q]; bi = si[q]; }
    __syncthreads();
}

// the block's sum in a fixed order, valid in thread 0
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double sw[THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < THREADS / 64; ++q) v += sw[q];
    __syncthreads();
    return v;
}

// the image's modes 0..n-1 (grid rows) into LDS
__device__ __forceinline__ void load_modes(const float *grid, const long long *idx, int n, float *modes) {
    for (int q = threadIdx.x; q < n * 9; q += THREADS) modes[q] = grid[idx[q / 9] * 9 + q % 9];
}

// pass j < k: grid (nb, g); part[b][nb]
__global__ __launch_bounds__(THREADS) void grid_modes_argmax_kernel(const float *logp, const float *grid, long long Q, int k, int j,
                                                                    float thr, const long long *index_out, const float *logp_out,
                                                                    ArgPart *part) {
    __shared__ float4 tile4[THREADS * 9 / 4];
    __shared__ float modes[MAX_K * 9];
    const int b = blockIdx.y, nb = gridDim.x;
    const long long *idx_b = index_out + (long long)b * k;
    // block-uniform: nothing to find after a missing mode or a NaN mode 0
    const bool skip = j > 0 && (idx_b[j - 1] < 0 || logp_out[(long long)b * k] != logp_out[(long long)b * k]);
    if (j > 0 && !skip) load_modes(grid, idx_b, j, modes);
    float bv = -INFINITY;
    long long bi = -1;
    if (!skip) {
        const float *lp = logp + (long long)b * Q;
        const float *tile = reinterpret_cast<const float *>(tile4);
        for (long long t0 = (long long)blockIdx.x * THREADS; t0 < Q; t0 += (long long)nb * THREADS) {
            const long long r = t0 + threadIdx.x;
            if (j > 0) {
                __syncthreads();                  // the previous tile is consumed (and, the first time, the modes are in)
                load_tile(grid, t0, (int)(Q - t0 < THREADS ? Q - t0 : THREADS), tile4);
                __syncthreads();
            }
            if (r < Q) {
                const float v = lp[r];
                bool ok = true;
                for (int m = 0; m < j && ok; ++m) ok = trace9(modes + 9 * m, tile + 9 * threadIdx.x) <= thr;
                if (ok && arg_better(v, r, bv, bi)) { bv = v; bi = r; }
            }
        }
    }
    block_arg(bv, bi);
    if (threadIdx.x == 0) part[(long long)b * nb + blockIdx.x] = ArgPart{bv, 0, bi};
}

// finalise of pass j: grid (g), mode j of image b from its nb partials
__global__ __launch_bounds__(THREADS) void grid_modes_argmax_final_kernel(const ArgPart *part, int nb, int k, int j, long long *index_out,
                                                                          float *logp_out) {
    const int b = blockIdx.x;
    float bv = -INFINITY;
    long long bi = -1;
    for (int q = threadIdx.x; q < nb; q += THREADS) {
        const ArgPart p = part[(long long)b * nb + q];
        if (arg_better(p.v, p.i, bv, bi)) { bv = p.v; bi = p.i; }
    }
    block_arg(bv, bi);
    if (threadIdx.x == 0) {
        index_out[(long long)b * k + j] = bi;
        logp_out[(long long)b * k + j] = bi < 0 ? -INFINITY : bv;
    }
}

// pass k: grid (nb, g); part[b][nb][k + 2] = {S, spread sum, region sums 0..k-1}
__global__ __launch_bounds__(THREADS) void grid_modes_mass_kernel(const float *logp, const float *grid, long long Q, int k, float thr,
                                                                  const float *gt, int n_gt, const long long *index_out,
                                                                  const float *logp_out, double *part) {
    __shared__ float4 tile4[THREADS * 9 / 4];
    __shared__ float modes[MAX_K * 9];
    __shared__ float gts[MAX_GT * 9];
    const int b = blockIdx.y, nb = gridDim.x;
    const long long *idx_b = index_out + (long long)b * k;
    int n_modes = 0;
    while (n_modes < k && idx_b[n_modes] >= 0) ++n_modes;
    load_modes(grid, idx_b, n_modes, modes);
    if (gt)
        for (int q = threadIdx.x; q < n_gt * 9; q += THREADS) gts[q] = gt[(long long)b * n_gt * 9 + q];
    const float M = logp_out[(long long)b * k];
    const float *lp = logp + (long long)b * Q;
    const float *tile = reinterpret_cast<const float *>(tile4);
    double S = 0.0, spread = 0.0, acc[MAX_K];
#pragma unroll
    for (int m = 0; m < MAX_K; ++m) acc[m] = 0.0;
    for (long long t0 = (long long)blockIdx.x * THREADS; t0 < Q; t0 += (long long)nb * THREADS) {
        const long long r = t0 + threadIdx.x;
        __syncthreads();
        load_tile(grid, t0, (int)(Q - t0 < THREADS ? Q - t0 : THREADS), tile4);
        __syncthreads();
        if (r < Q) {
            const float *R = tile + 9 * threadIdx.x;
            const double w = M == -INFINITY ? 0.0 : (double)expf(lp[r] - M);     // no finite value in the row: no mass anywhere
            S += w;
            int region = -1;
            for (int m = 0; m < n_modes && region < 0; ++m)
                if (trace9(modes + 9 * m, R) > thr) region = m;
#pragma unroll
            for (int m = 0; m < MAX_K; ++m) acc[m] += m == region ? w : 0.0;
            if (gt) {
                float best = -4.0f;
                for (int q = 0; q < n_gt; ++q) best = fmaxf(best, trace9(gts + 9 * q, R));
                spread += w * (double)acosf(fminf(fmaxf((best - 1.0f) * 0.5f, -1.0f), 1.0f));
            }
        }
    }
    double *dst = part + ((long long)b * nb + blockIdx.x) * (k + 2);
    S = block_sum(S);
    spread = block_sum(spread);
    if (threadIdx.x == 0) { dst[0] = S; dst[1] = spread; }
#pragma unroll
    for (int m = 0; m < MAX_K; ++m)
        if (m < k) {
            const double s = block_sum(acc[m]);
            if (threadIdx.x == 0) dst[2 + m] = s;
        }
}

// finalise of pass k: grid (g)
__global__ __launch_bounds__(THREADS) void grid_modes_mass_final_kernel(const double *part, int nb, long long Q, int k, int has_gt,
                                                                        const long long *index_out, const float *logp_out, float *mass_out,
                                                                        float *log_norm_out, float *spread_out) {
    __shared__ double sums[MAX_K + 2];
    const int b = blockIdx.x;
    for (int v = 0; v < k + 2; ++v) {
        double s = 0.0;
        for (int q = threadIdx.x; q < nb; q += THREADS) s += part[((long long)b * nb + q) * (k + 2) + v];
        s = block_sum(s);
        if (threadIdx.x == 0) sums[v] = s;
    }
    if (threadIdx.x == 0) {
        const float M = logp_out[(long long)b * k];
        const bool nan = M != M;
        const double S = sums[0];
        log_norm_out[b] = nan ? NAN : (float)((double)M + log(S) - log((double)Q));
        for (int m = 0; m < k; ++m)
            mass_out[(long long)b * k + m] = nan ? NAN : index_out[(long long)b * k + m] < 0 ? 0.0f : (float)(sums[2 + m] / S);
        if (has_gt) spread_out[b] = nan ? NAN : (float)(sums[1] / S);
    }
}

}  // namespace gm
}  // namespace rnf
