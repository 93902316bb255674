// grid_credible.h -- highest-density credible sets and HPD levels on the equivolumetric SO(3) grid (rnf_grid_credible, include/rnf_hip.h).
//
// Image b's log-densities lp[b][0..Q) become fixed-point masses W_i = rint(expf(lp_i - m) * 2^S), m the row's maximum (mode 0 of
// grid_modes.h, found by its arg-max kernels) and S = 62 - ceil(log2 Q), so that T = sum W_i < 2^63 whatever the order of the sum: every
// reduction below is an integer sum, exact and therefore independent of the order it is taken in.  That is what allows histograms here.
// The threshold of level alpha_j is the largest value tau of the image with sum_{lp_i >= tau} W_i >= need_j = ceil(alpha_j T).  It is found
// by an MSD radix select on key_i = rank_bits(lp_i) (grid_beam.h: ascending key = descending value, -0 and +0 tie), 4 passes of 8 bits:
//   pass p     every block builds, per level, the histogram (count, mass) of digit p of the rows whose higher digits equal the level's
//              prefix, in LDS with integer atomics, and writes it to the workspace.  Levels that share a prefix share a histogram (the
//              first of them builds it); pass 0 has a single one, and also accumulates the count and mass of the rows above each of the
//              image's query values (lp_i > v_q) in registers;
//   finalise   one workgroup per (level, image) sums the block histograms bin by bin (4 threads per bin), scans the 256 bins from the top
//              value down, fixes the digit at which the running mass reaches need_j and writes the longer prefix and the count and mass
//              above it to the workspace; after pass 3 the prefix is tau's key and the running count and mass are the set's.
// Nothing returns to the host between passes.  Determinism: the block count depends on Q alone (blocks_for), all sums are integer sums, so
// results are bit-identical from run to run and whatever number of images share a call.
// The contended first digit (one grid's log p spans a few binary exponents, so nearly every row of pass 0 has the same top 8 key bits): in
// pass 0 a thread keeps the (count, mass) of its current run of equal digits in registers and touches LDS only when the digit changes, so a
// block issues a few hundred LDS atomics on the hot bin instead of one per row.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "grid_beam.h"
#include "grid_mass.h"                            // u64, fixed_point_shift, no_sets, fixed_mass
#include "grid_modes.h"

namespace rnf {
namespace gc {

constexpr int THREADS = 256;                      // 4 waves of 64
constexpr int FINAL_PARTS = 4;                    // the finalise sums the block histograms in 4 interleaved parts,
constexpr int FINAL_THREADS = 1024;               // one thread per (part, bin)
constexpr int BINS = 256;                         // 8 bits per pass
constexpr int PASSES = 4;
constexpr int MAX_LEVELS = 8;
constexpr int MAX_QUERIES = 16;
constexpr long long MAX_Q = 1LL << 26;
constexpr long long ROWS_PER_BLOCK = 8192;
constexpr long long MAX_BLOCKS = 512;

// blocks of one image in every pass: a function of Q alone (the determinism rule above)
inline long long blocks_for(long long Q) {
    const long long b = (Q + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    return b < MAX_BLOCKS ? b : MAX_BLOCKS;
}

struct Levels {                                   // the levels alpha_j, by value in the kernel arguments
    double a[MAX_LEVELS];
};

struct State {                                    // of one (pass, image, level): 32 bytes
    unsigned prefix;                              // the key's digits fixed so far
    unsigned pad;
    u64 count;                                    // rows whose key is below the prefix (denser than every row under it)
    u64 mass;                                     // their mass
    u64 need;                                     // ceil(alpha_j T), clamped to 1..T
};

// the workspace of one call, carved in this order (every part 8-byte aligned but the last two)
struct Workspace {
    gm::ArgPart *max_part;                        // [g][gm::blocks_for(Q)]
    long long *max_index;                         // [g]
    State *state;                                 // [PASSES][g][J]
    u64 *total;                                   // [g]: T
    u64 *hist_mass;                               // [g][nb][J][BINS]
    u64 *query_mass;                              // [g][nb][G]
    unsigned *hist_count;                         // [g][nb][J][BINS]
    unsigned *query_count;                        // [g][nb][G]
    float *max_value;                             // [g]: m
    size_t bytes;
};

inline Workspace carve(void *base, long long Q, int g, int J, int G) {
    const size_t nb = (size_t)blocks_for(Q), ng = (size_t)g;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += bytes; return at; };
    const size_t max_part = take(ng * (size_t)gm::blocks_for(Q) * sizeof(gm::ArgPart)), max_index = take(ng * 8);
    const size_t state = take((size_t)PASSES * ng * J * sizeof(State)), total = take(ng * 8);
    const size_t hist_mass = take(ng * nb * J * BINS * 8), query_mass = take(ng * nb * G * 8);
    const size_t hist_count = take(ng * nb * J * BINS * 4), query_count = take(ng * nb * G * 4), max_value = take(ng * 4);
    Workspace w = {};
    w.bytes = (off + 15) & ~(size_t)15;
    if (!base) return w;                          // the size alone (rnf_grid_credible_workspace_bytes)
    char *p = static_cast<char *>(base);
    w.max_part = reinterpret_cast<gm::ArgPart *>(p + max_part);
    w.max_index = reinterpret_cast<long long *>(p + max_index);
    w.state = reinterpret_cast<State *>(p + state);
    w.total = reinterpret_cast<u64 *>(p + total);
    w.hist_mass = reinterpret_cast<u64 *>(p + hist_mass);
    w.query_mass = reinterpret_cast<u64 *>(p + query_mass);
    w.hist_count = reinterpret_cast<unsigned *>(p + hist_count);
    w.query_count = reinterpret_cast<unsigned *>(p + query_count);
    w.max_value = reinterpret_cast<float *>(p + max_value);
    return w;
}

// the query slots pass 0 is built with: the smallest of 0, 1 (grid_pose_credible's ground truth), 4 and 16 that holds G
inline int query_slots(int G) { return G == 0 ? 0 : G == 1 ? 1 : G <= 4 ? 4 : MAX_QUERIES; }

// pass 0: grid (nb, g).  One histogram of the top digit per block, and the rows above the image's G <= NQ query values.
template <int NQ>
__global__ __launch_bounds__(THREADS) void grid_credible_first_kernel(const float *logp, long long Q, int J, const float *queries, int G,
                                                                      double scale, const float *max_value, u64 *hist_mass,
                                                                      unsigned *hist_count, u64 *query_mass, unsigned *query_count) {
    __shared__ u64 hm[BINS];
    __shared__ unsigned hc[BINS];
    __shared__ u64 qm[MAX_QUERIES];
    __shared__ unsigned qc[MAX_QUERIES];
    const int b = blockIdx.y, nb = gridDim.x, t = threadIdx.x;
    const float m = max_value[b];
    if (no_sets(m)) return;                       // block-uniform; the finalises never read this image's partials
    hm[t] = 0;
    hc[t] = 0;
    if (t < MAX_QUERIES) { qm[t] = 0; qc[t] = 0; }
    constexpr int NV = NQ > 0 ? NQ : 1;
    float v[NV];
    u64 vm[NV];
    unsigned vc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        v[q] = q < G ? queries[(long long)b * G + q] : NAN;        // a NaN compares false: nothing is above it
        vm[q] = 0;
        vc[q] = 0;
    }
    __syncthreads();
    const float *lp = logp + (long long)b * Q;
    unsigned cur = 0, run_count = 0;              // the thread's current run of equal digits
    u64 run_mass = 0;
    for (long long r = (long long)blockIdx.x * THREADS + t; r < Q; r += (long long)nb * THREADS) {
        const float x = lp[r];
        const u64 W = fixed_mass(x, m, scale);
        const unsigned d = gb::rank_bits(x) >> 24;
        if (d != cur) {
            if (run_count) {
                atomicAdd(&hm[cur], run_mass);
                atomicAdd(&hc[cur], run_count);
            }
            cur = d;
            run_count = 0;
            run_mass = 0;
        }
        ++run_count;
        run_mass += W;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const bool above = x > v[q];
            vm[q] += above ? W : 0;
            vc[q] += above ? 1u : 0u;
        }
    }
    if (run_count) {
        atomicAdd(&hm[cur], run_mass);
        atomicAdd(&hc[cur], run_count);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (q < G && vc[q]) {
            atomicAdd(&qm[q], vm[q]);
            atomicAdd(&qc[q], vc[q]);
        }
    __syncthreads();
    const long long slot = (long long)b * nb + blockIdx.x;
    hist_mass[slot * J * BINS + t] = hm[t];       // level 0's slot holds the shared histogram
    hist_count[slot * J * BINS + t] = hc[t];
    if (t < G) {
        query_mass[slot * G + t] = qm[t];
        query_count[slot * G + t] = qc[t];
    }
}

// the first level with level j's prefix: the one whose histogram serves them all
__device__ __forceinline__ int alias_of(const State *prev, int j) {
    int a = j;
    for (int i = j - 1; i >= 0; --i)
        if (prev[i].prefix == prev[j].prefix) a = i;
    return a;
}

// pass p = 1..3: grid (nb, g).  prev = state[p - 1]; per level (first of its prefix), the histogram of digit p under the prefix.
__global__ __launch_bounds__(THREADS) void grid_credible_pass_kernel(const float *logp, long long Q, int J, int pass, double scale,
                                                                     const float *max_value, const State *prev, u64 *hist_mass,
                                                                     unsigned *hist_count) {
    __shared__ u64 hm[MAX_LEVELS * BINS];
    __shared__ unsigned hc[MAX_LEVELS * BINS];
    const int b = blockIdx.y, nb = gridDim.x, t = threadIdx.x;
    const float m = max_value[b];
    if (no_sets(m)) return;
    const State *st = prev + (long long)b * J;
    unsigned pre[MAX_LEVELS];
    bool own[MAX_LEVELS];
#pragma unroll
    for (int j = 0; j < MAX_LEVELS; ++j) {
        own[j] = j < J && alias_of(st, j) == j;
        pre[j] = j < J ? st[j].prefix : 0u;
    }
    for (int j = 0; j < J; ++j) {
        hm[j * BINS + t] = 0;
        hc[j * BINS + t] = 0;
    }
    __syncthreads();
    const int shift = 24 - 8 * pass;              // of this pass's digit; the prefix is the key above it
    const float *lp = logp + (long long)b * Q;
    for (long long r = (long long)blockIdx.x * THREADS + t; r < Q; r += (long long)nb * THREADS) {
        const float x = lp[r];
        const unsigned key = gb::rank_bits(x);
        const unsigned hi = key >> (shift + 8), d = (key >> shift) & (BINS - 1);
        bool any = false;
#pragma unroll
        for (int j = 0; j < MAX_LEVELS; ++j) any = any || (own[j] && hi == pre[j]);
        if (any) {
            const u64 W = fixed_mass(x, m, scale);
#pragma unroll
            for (int j = 0; j < MAX_LEVELS; ++j)
                if (own[j] && hi == pre[j]) {
                    atomicAdd(&hm[j * BINS + d], W);
                    atomicAdd(&hc[j * BINS + d], 1u);
                }
        }
    }
    __syncthreads();
    const long long slot = (long long)b * nb + blockIdx.x;
#pragma unroll
    for (int j = 0; j < MAX_LEVELS; ++j)
        if (own[j]) {
            hist_mass[(slot * J + j) * BINS + t] = hm[j * BINS + t];
            hist_count[(slot * J + j) * BINS + t] = hc[j * BINS + t];
        }
}

// inclusive scan over the 256 bins by the workgroup's first 256 threads (lead), in LDS; every thread of the workgroup calls it
__device__ __forceinline__ u64 block_scan(u64 v, u64 *s, bool lead) {
    const int t = threadIdx.x & (BINS - 1);
    if (lead) s[t] = v;
    __syncthreads();
    for (int off = 1; off < BINS; off <<= 1) {
        const u64 add = lead && t >= off ? s[t - off] : 0;
        __syncthreads();
        if (lead) s[t] += add;
        __syncthreads();
    }
    const u64 r = lead ? s[t] : 0;
    __syncthreads();
    return r;
}

// finalise of pass p: grid (J, g), 1024 threads: thread (part, t) sums bin t of every fourth block's histogram, the first 256 threads
// (part 0) then own bin t.  Writes state[p]; pass 0 also T, log_norm and (level 0's workgroup) the query outputs; pass 3 the level's
// threshold, count and mass.
__global__ __launch_bounds__(FINAL_THREADS) void grid_credible_final_kernel(long long Q, int J, int G, int pass, int nb, int S, Levels levels,
                                                                            const float *queries, const float *max_value,
                                                                            const u64 *hist_mass, const unsigned *hist_count,
                                                                            const u64 *query_mass_part, const unsigned *query_count_part,
                                                                            const State *prev, State *next, u64 *total, float *threshold_out,
                                                                            long long *count_out, float *mass_out, float *log_norm_out,
                                                                            float *query_mass_out, long long *query_count_out) {
    __shared__ u64 pm[FINAL_PARTS][BINS];
    __shared__ u64 pc[FINAL_PARTS][BINS];
    __shared__ u64 scan[BINS];
    __shared__ u64 qm[MAX_QUERIES];
    __shared__ unsigned qc[MAX_QUERIES];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, t = tid & (BINS - 1), part = tid / BINS;
    const bool lead = part == 0;
    const float m = max_value[b];
    const long long out = (long long)b * J + j;
    if (no_sets(m)) {                             // block-uniform
        if (tid == 0) {
            next[out] = State{0u, 0u, 0, 0, 0};
            if (pass == 0 && j == 0) log_norm_out[b] = m == -INFINITY ? -INFINITY : NAN;
            if (pass == PASSES - 1) {
                threshold_out[out] = NAN;
                count_out[out] = -1;
                mass_out[out] = NAN;
            }
        }
        if (pass == 0 && j == 0 && tid < G) {
            query_mass_out[(long long)b * G + tid] = NAN;
            query_count_out[(long long)b * G + tid] = -1;
        }
        return;
    }
    const State *pv = prev ? prev + (long long)b * J : nullptr;
    const int a = pass == 0 ? 0 : alias_of(pv, j);
    u64 hm = 0, hc = 0;
#pragma unroll 4
    for (int x = part; x < nb; x += FINAL_PARTS) {
        const long long at = (((long long)b * nb + x) * J + a) * BINS + t;
        hm += hist_mass[at];
        hc += hist_count[at];
    }
    pm[part][t] = hm;
    pc[part][t] = hc;
    __syncthreads();
    if (lead) {
#pragma unroll
        for (int q = 1; q < FINAL_PARTS; ++q) {
            hm += pm[q][t];
            hc += pc[q][t];
        }
    }
    const u64 cm = block_scan(hm, scan, lead), cc = block_scan(hc, scan, lead);       // inclusive, from the top value down
    u64 T, need, above_mass, above_count;
    unsigned prefix;
    if (pass == 0) {
        if (lead) scan[t] = cm;
        __syncthreads();
        T = scan[BINS - 1];
        __syncthreads();
        need = (u64)ceil(levels.a[j] * (double)T);
        need = need < 1 ? 1 : need > T ? T : need;
        above_mass = 0;
        above_count = 0;
        prefix = 0;
        if (j == 0) {
            if (tid == 0) {
                total[b] = T;
                log_norm_out[b] = (float)((double)m + log(ldexp((double)T, -S)) - log((double)Q));
            }
            if (G > 0) {                          // the query partials: thread tid sums blocks tid / 16, tid / 16 + 64, ... of query tid % 16
                if (tid < MAX_QUERIES) { qm[tid] = 0; qc[tid] = 0; }
                __syncthreads();
                const int q = tid % MAX_QUERIES;
                if (q < G) {
                    u64 sm = 0;
                    unsigned sc = 0;
                    for (int x = tid / MAX_QUERIES; x < nb; x += FINAL_THREADS / MAX_QUERIES) {
                        sm += query_mass_part[((long long)b * nb + x) * G + q];
                        sc += query_count_part[((long long)b * nb + x) * G + q];
                    }
                    if (sc) {
                        atomicAdd(&qm[q], sm);
                        atomicAdd(&qc[q], sc);
                    }
                }
                __syncthreads();
                if (tid < G) {
                    const float v = queries[(long long)b * G + tid];
                    query_mass_out[(long long)b * G + tid] = v != v ? NAN : (float)((double)qm[tid] / (double)T);
                    query_count_out[(long long)b * G + tid] = v != v ? -1 : (long long)qc[tid];
                }
            }
        }
    } else {
        T = total[b];
        need = pv[j].need;
        above_mass = pv[j].mass;
        above_count = pv[j].count;
        prefix = pv[j].prefix;
    }
    // the digit: the first bin at which the running mass reaches need (the running mass never decreases, so exactly one thread)
    const u64 run = above_mass + cm;
    if (lead && run >= need && run - hm < need) {
        const unsigned key = (prefix << 8) | (unsigned)t;
        next[out] = State{key, 0u, above_count + cc - hc, run - hm, need};
        if (pass == PASSES - 1) {
            threshold_out[out] = gb::rank_value(key);
            count_out[out] = (long long)(above_count + cc);
            mass_out[out] = (float)((double)run / (double)T);
        }
    }
}

}  // namespace gc
}  // namespace rnf
