// grid_beam.h -- per-image beam selection of the coarse-to-fine grid search (rnf_grid_beam_select, include/rnf_hip.h).
//
// Each candidate (log p, row) becomes one 64-bit key, rank << 32 | row, whose ascending order is the selection order: rank = rank_bits(log
// p) puts a NaN first, then larger values first (-0 and +0 tie, as in torch.argmax), and the row breaks ties, smaller first.  A missing
// candidate (row < 0 or > ROW_MAX) is the key NONE, which sorts after every real one.  A pass sorts one CHUNK of an image's keys in LDS
// (bitonic) and keeps the first `keep`:
//   dedup   with explicit rows, the chunk is first sorted by row (the key rotated by 32 bits), every key but the first of a row becomes NONE,
//           and it is rotated back: a row keeps its best candidate;
//   passes  the first pass reads the candidates ([g][M]); while an image has more than one chunk, every block writes its `beam` best keys
//           to the workspace ([g][nb][beam]) and the next pass reads those (nb * beam keys, beam <= CHUNK / 4, so each pass cuts the keys
//           by 4 or more); a single chunk writes rows_out / logp_out (row -1, log p -inf past the distinct rows).
// A row's best candidate survives every pass: the rows ahead of it in its chunk are ahead of it overall, so it is among its chunk's first
// `beam` whenever it is among the image's first `beam`.  Determinism: the block count of every pass depends on (M, beam) alone, sorts are
// data-independent networks and there are no atomics, so results are bit-identical from run to run and whatever g.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rnf {
namespace gb {

constexpr int THREADS = 256;                        // 4 waves of 64
constexpr int CHUNK = 4096;                         // keys per block: 32 KB of LDS
constexpr int MAX_BEAM = 1024;
constexpr long long ROW_MAX = 0x7FFFFFFELL;         // rows fit in the low 32 bits of a key, 0xFFFFFFFF is NONE's
constexpr unsigned long long NONE = ~0ULL;

inline long long blocks_for(long long n) { return (n + CHUNK - 1) / CHUNK; }

// ascending rank: NaN 0, then +inf, ..., -inf (0xFF800000); never 0xFFFFFFFF
__device__ __forceinline__ unsigned rank_bits(float v) {
    if (v != v) return 0u;
    const unsigned u = __float_as_uint(v == 0.0f ? 0.0f : v);
    const unsigned m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // ascending with the value
    return ~m;
}

__device__ __forceinline__ float rank_value(unsigned rank) {
    const unsigned m = ~rank;
    return __uint_as_float((m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m);
}

__device__ __forceinline__ unsigned long long rotate32(unsigned long long k) { return (k << 32) | (k >> 32); }

// ascending bitonic sort of s[0..P), P a power of two
__device__ __forceinline__ void bitonic_sort(unsigned long long *s, int P) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = s[i], b = s[l];
                    if ((a > b) == ((i & k) == 0)) { s[i] = b; s[l] = a; }
                }
            }
            __syncthreads();
        }
}

// grid (nb, g).  Block x of image b sorts keys [x * CHUNK, min(n, (x + 1) * CHUNK)) of the image's n: from logp / rows (keys_in NULL;
// rows NULL: row = candidate index) or from keys_in.  Writes its first `keep` keys to keys_out[b][x][keep], or (keys_out NULL, nb = 1)
// the image's result to rows_out[b][keep], logp_out[b][keep].
__global__ __launch_bounds__(THREADS) void beam_select_kernel(const float *logp, const long long *rows, const unsigned long long *keys_in,
                                                              long long n, int dedup, int keep, unsigned long long *keys_out,
                                                              long long *rows_out, float *logp_out) {
    __shared__ unsigned long long s[CHUNK];
    const int b = blockIdx.y, x = blockIdx.x;
    const long long base = (long long)b * n, lo = (long long)x * CHUNK;
    const int len = (int)(n - lo < CHUNK ? n - lo : CHUNK);
    int P = 1;
    while (P < len) P <<= 1;
    for (int i = threadIdx.x; i < P; i += THREADS) {
        unsigned long long key = NONE;
        if (i < len) {
            const long long c = base + lo + i;
            if (keys_in) {
                key = keys_in[c];
            } else {
                const long long r = rows ? rows[c] : lo + i;
                if (r >= 0 && r <= ROW_MAX) key = ((unsigned long long)rank_bits(logp[c]) << 32) | (unsigned long long)r;
            }
        }
        s[i] = dedup ? rotate32(key) : key;
    }
    __syncthreads();
    if (dedup) {
        bitonic_sort(s, P);                          // by row, then rank: a row's best candidate first
        unsigned long long mine[CHUNK / THREADS];
#pragma unroll
        for (int q = 0; q < CHUNK / THREADS; ++q) {
            const int i = threadIdx.x + q * THREADS;
            if (i < P) mine[q] = (i > 0 && (s[i] >> 32) == (s[i - 1] >> 32)) ? NONE : rotate32(s[i]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < CHUNK / THREADS; ++q) {
            const int i = threadIdx.x + q * THREADS;
            if (i < P) s[i] = mine[q];
        }
        __syncthreads();
    }
    bitonic_sort(s, P);
    for (int i = threadIdx.x; i < keep; i += THREADS) {
        const unsigned long long key = i < P ? s[i] : NONE;
        if (keys_out) {
            keys_out[((long long)b * gridDim.x + x) * keep + i] = key;
        } else {
            rows_out[(long long)b * keep + i] = key == NONE ? -1 : (long long)(key & 0xFFFFFFFFull);
            logp_out[(long long)b * keep + i] = key == NONE ? -INFINITY : rank_value((unsigned)(key >> 32));
        }
    }
}

}  // namespace gb
}  // namespace rnf
