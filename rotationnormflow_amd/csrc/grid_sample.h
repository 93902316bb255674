// grid_sample.h -- draws from posteriors on the equivolumetric SO(3) grid (rnf_grid_sample) and the chart of a grid cell that carries a
// drawn row to a rotation inside its cell (rnf_so3_grid_cell_points, include/rnf_hip.h).
//
// The chart.  A cell of the level-l grid (grid_locate.h) is a HEALPix pixel times a tilt interval.  Pixel p (RING) is the square
// [ix, ix + 1) x [iy, iy + 1) / nside of its face (ring2nest, so3_grid.h), and the HEALPix projection from face coordinates (x, y) to the
// sphere is equal-area (Gorski et al. 2005); the tilt cell of t is [(t - 1/2), (t + 1/2)) * 2 pi / (6 nside).  So with (u0, u1, u2)
// uniform on [0, 1]^3,
//   x = (ix + u0) / nside, y = (iy + u1) / nside,  jr = jrll(face) - x - y,
//   north cap (jr < 1): nr = jr, z = 1 - nr^2 / 3;  south cap (jr > 3): nr = 4 - jr, z = nr^2 / 3 - 1;  belt: nr = 1, z = (2 - jr) 2 / 3,
//   phi = (pi / 4) ((jpll(face) nr + x - y) mod 8) / nr,   tau = (t + u2 - 1/2) 2 pi / (6 nside),
// the rotation Rx(phi) Rz(theta) Rx(tau) O is Haar-uniform in the cell of row t * npix + p, and u = (1/2, 1/2, 1/2) is the grid's row (to
// rounding: grid_row reaches the same angles by the ring formulas).  In the caps sin(theta) = sqrt(tmp (2 - tmp)), tmp = nr^2 / 3, as
// grid_row forms it, never sqrt(1 - z^2).  fp64 throughout, one rounding per entry at the store.  A row outside 0..Q-1 or a u outside
// [0, 1] (a NaN included) gives nine NaNs and reads nothing.
//
// The draws.  Image b's masses are grid_mass.h's W_i = rint(expf(lp_i - m) 2^S) (m by grid_modes.h's arg-max pass, S = 62 - ceil(log2 Q)),
// C their inclusive prefix sum in row order, T = C_{Q-1} <= 2^62.  A target v in [0, T) draws the row i with C_{i-1} <= v < C_i; a row
// with W_i = 0 is never drawn.  With r64(k, b, s) = (word0 << 32) | word1 of Philox4x32-10 keyed by the seed on the counter
// (global draw k, global image b (two words), stream s) and mulhi the high half of a 64 x 64 product,
//   multinomial   v_k = mulhi(r64(k, b, 0), T);
//   systematic    a = mulhi(r64(0, b, 0), T), T = q N + r with N = draws_total:  v_k = k q + (k r + a) / N  = floor((k T + a) / N)
//                 (k r + a < 2^60 + 2^62: no 128-bit division);
//   jitter        u_j = (word_j of stream 1 + 1/2) / 2^32, j = 0..2, in fp64.
// Three kernels after the arg-max: a wave sums each chunk of CHUNK = 64 consecutive rows (integer sums: exact in any order); one
// workgroup per image scans the chunk sums in place into an inclusive u64 prefix and writes T; one thread per draw binary-searches the
// chunk prefix and walks its one chunk, recomputing W_i by the same function.  O(log Q) + one chunk per draw.  Block counts depend on
// Q (and on the draws of the call) alone, nothing floating-point is summed, a draw's numbers depend on its global indices alone: outputs
// are bit-identical from run to run, whatever images share a call (image_base) and however the draws are tiled over calls (draw_base).
// An image with a NaN, a +inf maximum or no finite value (T = 0) has index -1, target 0, total 0 and NaN rotations; the others of the
// call are not touched by it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "grid_mass.h"
#include "philox.h"
#include "so3_grid.h"
#if defined(__HIPCC__) && !defined(RNF_GSA_HOST_ONLY)
#include "grid_modes.h"
#endif

namespace rnf {
namespace gsa {

typedef unsigned long long u64;

constexpr int THREADS = 256;                      // 4 waves of 64
constexpr int WAVES = THREADS / 64;
constexpr int SCAN_THREADS = 1024;
constexpr int CHUNK = 64;                         // rows per entry of the prefix: a draw walks half of one on average, and the prefix
                                                  // takes Q / 8 bytes per image (2.25 MiB at level 6, 1/32 of the image itself)
constexpr int MAX_LEVEL = 6;                      // Q = 72 * 8^6 <= 2^26
constexpr long long MAX_Q = 1LL << 26;
constexpr long long MAX_DRAWS = 1LL << 30;        // draws_total
constexpr long long MAX_SUM_BLOCKS = 2048;
constexpr int MULTINOMIAL = 0, SYSTEMATIC = 1;    // RNF_GRID_SAMPLE_*

inline long long chunks_for(long long Q) { return (Q + CHUNK - 1) / CHUNK; }

// blocks of one image in the chunk-sum pass, four chunks per block and step: a function of Q alone
inline long long sum_blocks_for(long long Q) {
    const long long b = (chunks_for(Q) + 4 * WAVES - 1) / (4 * WAVES);
    return b < MAX_SUM_BLOCKS ? b : MAX_SUM_BLOCKS;
}

__host__ __device__ __forceinline__ u64 mulhi(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

// the four Philox words of (draw, image, stream) under the seed
__host__ __device__ __forceinline__ void philox_words(u64 seed, long long draw, long long image, unsigned stream, unsigned (&c)[4]) {
    const Philox rng{(unsigned)seed, (unsigned)(seed >> 32)};
    c[0] = (unsigned)draw;
    c[1] = (unsigned)(u64)image;
    c[2] = (unsigned)((u64)image >> 32);
    c[3] = stream;
    rng(c);
}

__host__ __device__ __forceinline__ u64 r64_of(const unsigned (&c)[4]) { return ((u64)c[0] << 32) | (u64)c[1]; }

// the target of global draw k (0 <= k < N) of global image `image`: an integer in [0, T), T >= 1
__host__ __device__ __forceinline__ u64 target_of(int method, u64 seed, long long image, long long k, long long N, u64 T) {
    unsigned c[4];
    if (method == MULTINOMIAL) {
        philox_words(seed, k, image, 0u, c);
        return mulhi(r64_of(c), T);
    }
    philox_words(seed, 0, image, 0u, c);
    const u64 a = mulhi(r64_of(c), T), q = T / (u64)N, r = T % (u64)N;
    return (u64)k * q + ((u64)k * r + a) / (u64)N;
}

// the row i with C_{i-1} <= v < C_i, from the inclusive chunk prefix (nc entries, the last one T > v) and one walk through its chunk
__host__ __device__ __forceinline__ long long draw_row(const float *lp, long long Q, const u64 *prefix, long long nc, float m, double scale,
                                                       u64 v) {
    long long lo = 0, hi = nc - 1;                 // the first chunk whose inclusive sum exceeds v
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (prefix[mid] > v) hi = mid;
        else lo = mid + 1;
    }
    u64 acc = lo ? prefix[lo - 1] : 0;
    const long long r0 = lo * CHUNK, r1 = r0 + CHUNK < Q ? r0 + CHUNK : Q;
    long long last = r0;                           // the chunk's last row with mass: what a walk that found nothing would return
    for (long long r = r0; r < r1; ++r) {          // (it cannot: the chunk's sum was formed from these very values)
        const u64 W = gc::fixed_mass(lp[r], m, scale);
        acc += W;
        if (v < acc) return r;
        if (W) last = r;
    }
    return last;
}

__host__ __device__ __forceinline__ void nan9(float *dst) {
#pragma unroll
    for (int c = 0; c < 9; ++c) dst[c] = NAN;
}

// (Rx(phi) Rz(theta) Rx(tau)) O from z = cos(theta), sth = sin(theta): grid_row's entries
__host__ __device__ __forceinline__ void euler_store(double z, double sth, double phi, double tau, const double *o, float *dst) {
    double sphi, cphi, stau, ctau;
    sincos(phi, &sphi, &cphi);
    sincos(tau, &stau, &ctau);
    const double a[9] = {z, -sth * ctau, sth * stau,
                         cphi * sth, cphi * z * ctau - sphi * stau, -cphi * z * stau - sphi * ctau,
                         sphi * sth, sphi * z * ctau + cphi * stau, -sphi * z * stau + cphi * ctau};
    for (int row = 0; row < 3; ++row)
        for (int col = 0; col < 3; ++col)
            dst[row * 3 + col] = (float)(a[row * 3] * o[col] + a[row * 3 + 1] * o[3 + col] + a[row * 3 + 2] * o[6 + col]);
}

// the chart: the point (u0, u1, u2) of [0, 1]^3 of the cell of row r of the level-`level` grid times O, into dst[9]
__host__ __device__ __forceinline__ void chart_row(int level, long long r, double u0, double u1, double u2, const double *o, float *dst) {
    const long long nside = 1LL << level, npix = 12 * nside * nside, Q = 6 * nside * npix;
    if (!(r >= 0 && r < Q) || !(u0 >= 0.0 && u0 <= 1.0) || !(u1 >= 0.0 && u1 <= 1.0) || !(u2 >= 0.0 && u2 <= 1.0)) {
        nan9(dst);
        return;
    }
    const long long t = r / npix, p = r - t * npix;
    const long long nest = so3g::ring2nest(nside, p), face = nest / (nside * nside), ipf = nest - face * nside * nside;
    const long long ix = so3g::compress_bits(ipf), iy = so3g::compress_bits(ipf >> 1);
    const double x = ((double)ix + u0) / (double)nside, y = ((double)iy + u1) / (double)nside;
    const double jr = (double)so3g::jrll(face) - x - y;
    double nr, z, sth;
    if (jr < 1.0) {                                           // north polar cap
        nr = jr;
        const double tmp = nr * nr / 3.0;
        z = 1.0 - tmp;
        sth = sqrt(tmp * (2.0 - tmp));
    } else if (jr > 3.0) {                                    // south polar cap
        nr = 4.0 - jr;
        const double tmp = nr * nr / 3.0;
        z = tmp - 1.0;
        sth = sqrt(tmp * (2.0 - tmp));
    } else {                                                  // belt
        nr = 1.0;
        z = (2.0 - jr) * 2.0 / 3.0;
        sth = sqrt((1.0 - z) * (1.0 + z));
    }
    double tt = (double)so3g::jpll(face) * nr + x - y;        // in eighths of a turn, times nr
    if (tt < 0.0) tt += 8.0;
    if (tt >= 8.0) tt -= 8.0;
    const double phi = nr > 0.0 ? (M_PI / 4.0) * tt / nr : 0.0;            // nr = 0: the pole itself (a face's far corner at u = 1)
    const double tau = ((double)t + u2 - 0.5) * (2.0 * M_PI / (double)(6 * nside));
    euler_store(z, sth, phi, tau, o, dst);
}

// what one draw writes: its row, its target and (optionally) its rotation
__host__ __device__ __forceinline__ void draw_one(const float *lp, long long Q, const u64 *prefix, long long nc, float m, double scale, u64 T,
                                                  int level, int method, int jitter, u64 seed, long long image, long long k, long long N,
                                                  const double *o, long long *index_out, u64 *target_out, float *rot_out) {
    if (gc::no_sets(m) || T == 0) {
        *index_out = -1;
        if (target_out) *target_out = 0;
        if (rot_out) nan9(rot_out);
        return;
    }
    const u64 v = target_of(method, seed, image, k, N, T);
    const long long row = draw_row(lp, Q, prefix, nc, m, scale, v);
    *index_out = row;
    if (target_out) *target_out = v;
    if (!rot_out) return;
    if (jitter) {
        unsigned c[4];
        philox_words(seed, k, image, 1u, c);
        const double s = 1.0 / 4294967296.0;
        chart_row(level, row, ((double)c[0] + 0.5) * s, ((double)c[1] + 0.5) * s, ((double)c[2] + 0.5) * s, o, rot_out);
    } else {
        so3g::grid_row(level, row, o, rot_out);
    }
}

// the workspace of one rnf_grid_sample call, carved in this order (every part 8-byte aligned but the last)
struct Workspace {
    void *max_part;                               // gm::ArgPart [g][gm::blocks_for(Q)] (16 bytes each)
    long long *max_index;                         // [g]
    u64 *prefix;                                  // [g][chunks_for(Q)]
    u64 *total;                                   // [g]: T
    float *max_value;                             // [g]: m
    size_t bytes;
};

inline Workspace carve(void *base, long long Q, int g, long long max_blocks) {
    const size_t ng = (size_t)g;
    const size_t max_part = 0, max_index = max_part + ng * (size_t)max_blocks * 16, prefix = max_index + ng * 8;
    const size_t total = prefix + ng * (size_t)chunks_for(Q) * 8, max_value = total + ng * 8;
    Workspace w = {};
    w.bytes = (max_value + ng * 4 + 15) & ~(size_t)15;
    if (!base) return w;                          // the size alone (rnf_grid_sample_workspace_bytes)
    char *p = static_cast<char *>(base);
    w.max_part = p + max_part;
    w.max_index = reinterpret_cast<long long *>(p + max_index);
    w.prefix = reinterpret_cast<u64 *>(p + prefix);
    w.total = reinterpret_cast<u64 *>(p + total);
    w.max_value = reinterpret_cast<float *>(p + max_value);
    return w;
}

// ---- the host build of the tests: the same functions in plain loops --------------------------------------------------------------------

inline void host_cell_points(int level, const float *offset, const long long *rows, const float *u, long long n, float *rot) {
    double o[9];
    so3g::load_offset(offset, o);
    for (long long k = 0; k < n; ++k) chart_row(level, rows[k], (double)u[3 * k], (double)u[3 * k + 1], (double)u[3 * k + 2], o, rot + 9 * k);
}

inline void host_grid_rows(int level, const float *offset, const long long *rows, long long n, float *rot) {
    double o[9];
    so3g::load_offset(offset, o);
    for (long long k = 0; k < n; ++k) so3g::grid_row(level, rows[k], o, rot + 9 * k);
}

// every argument as rnf_grid_sample's (host pointers; target, total and rot may be null); the arguments are taken as checked
inline void host_grid_sample(const float *logp, long long Q, int g, int level, long long draws, long long draw_base, long long draws_total,
                             long long image_base, int method, int jitter, u64 seed, const float *offset, long long *index, u64 *target,
                             u64 *total, float *rot) {
    double o[9];
    so3g::load_offset(offset, o);
    const long long nc = chunks_for(Q);
    const double scale = ldexp(1.0, gc::fixed_point_shift(Q));
    std::vector<u64> prefix((size_t)nc);
    for (int b = 0; b < g; ++b) {
        const float *lp = logp + (long long)b * Q;
        float m = lp[0];                           // the arg-max pass: a NaN wins, otherwise the largest value
        for (long long r = 1; r < Q && m == m; ++r)
            if (lp[r] != lp[r] || lp[r] > m) m = lp[r];
        u64 T = 0;
        if (!gc::no_sets(m))
            for (long long c = 0; c < nc; ++c) {
                const long long r1 = (c + 1) * CHUNK < Q ? (c + 1) * CHUNK : Q;
                for (long long r = c * CHUNK; r < r1; ++r) T += gc::fixed_mass(lp[r], m, scale);
                prefix[(size_t)c] = T;
            }
        if (total) total[b] = T;
        for (long long k = 0; k < draws; ++k) {
            const long long out = (long long)b * draws + k;
            draw_one(lp, Q, prefix.data(), nc, m, scale, T, level, method, jitter, seed, image_base + b, draw_base + k, draws_total, o,
                     index + out, target ? target + out : nullptr, rot ? rot + 9 * out : nullptr);
        }
    }
}

#if defined(__HIPCC__) && !defined(RNF_GSA_HOST_ONLY)      // the host builds of the tests define it: no device code to link

// one thread per point: rot[k] = the chart of rows[k] at u[k]
__global__ __launch_bounds__(THREADS) void so3_grid_cell_points_kernel(int level, long long n, const long long *rows, const float *u,
                                                                       const float *offset, float *rot) {
    double o[9];
    so3g::load_offset(offset, o);
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x)
        chart_row(level, rows[k], (double)u[3 * k], (double)u[3 * k + 1], (double)u[3 * k + 2], o, rot + 9 * k);
}

// the chunk sums: grid (sum_blocks_for(Q), g), one wave per chunk and step; prefix[b][c] = the sum of chunk c
__global__ __launch_bounds__(THREADS) void grid_sample_sum_kernel(const float *logp, long long Q, long long nc, double scale,
                                                                  const float *max_value, u64 *prefix) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const float m = max_value[b];
    if (gc::no_sets(m)) return;                   // block-uniform; the scan never reads this image's sums
    const float *lp = logp + (long long)b * Q;
    for (long long c = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); c < nc; c += (long long)gridDim.x * WAVES) {
        u64 s = 0;
#pragma unroll
        for (int j = 0; j < CHUNK / 64; ++j) {
            const long long r = c * CHUNK + j * 64 + lane;
            if (r < Q) s += gc::fixed_mass(lp[r], m, scale);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) prefix[(long long)b * nc + c] = s;
    }
}

// the scan: grid (g), SCAN_THREADS threads; thread t owns a run of consecutive chunks.  In place: sums in, inclusive prefix out; total[b] = T
__global__ __launch_bounds__(SCAN_THREADS) void grid_sample_scan_kernel(long long nc, const float *max_value, u64 *prefix, u64 *total) {
    __shared__ u64 s[SCAN_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    if (gc::no_sets(max_value[b])) {              // block-uniform
        if (t == 0) total[b] = 0;
        return;
    }
    u64 *p = prefix + (long long)b * nc;
    const long long per = (nc + SCAN_THREADS - 1) / SCAN_THREADS;
    const long long i0 = (long long)t * per < nc ? (long long)t * per : nc, i1 = i0 + per < nc ? i0 + per : nc;
    u64 sum = 0;
    for (long long i = i0; i < i1; ++i) sum += p[i];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
        const u64 add = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    u64 run = s[t] - sum;                         // of the chunks before this thread's
    for (long long i = i0; i < i1; ++i) {
        run += p[i];
        p[i] = run;
    }
    if (t == SCAN_THREADS - 1) total[b] = s[t];
}

// the draws: grid (blocks, g), one thread per draw of the call
__global__ __launch_bounds__(THREADS) void grid_sample_draw_kernel(const float *logp, long long Q, long long nc, double scale, int level,
                                                                   long long draws, long long draw_base, long long draws_total,
                                                                   long long image_base, int method, int jitter, u64 seed, const float *offset,
                                                                   const float *max_value, const u64 *prefix, const u64 *total,
                                                                   long long *index_out, u64 *target_out, u64 *total_out, float *rot_out) {
    const int b = blockIdx.y;
    const float m = max_value[b];
    const u64 T = total[b];
    double o[9];
    so3g::load_offset(offset, o);
    const float *lp = logp + (long long)b * Q;
    const u64 *pf = prefix + (long long)b * nc;
    if (total_out && blockIdx.x == 0 && threadIdx.x == 0) total_out[b] = T;
    for (long long k = (long long)blockIdx.x * THREADS + threadIdx.x; k < draws; k += (long long)gridDim.x * THREADS) {
        const long long out = (long long)b * draws + k;
        draw_one(lp, Q, pf, nc, m, scale, T, level, method, jitter, seed, image_base + b, draw_base + k, draws_total, o, index_out + out,
                 target_out ? target_out + out : nullptr, rot_out ? rot_out + 9 * out : nullptr);
    }
}

#endif  // __HIPCC__ && !RNF_GSA_HOST_ONLY

}  // namespace gsa
}  // namespace rnf
