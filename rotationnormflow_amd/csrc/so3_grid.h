// so3_grid.h -- the equivolumetric HEALPix grid over SO(3) (rnf_so3_healpix_grid) and its hierarchy (rnf_so3_grid_children,
// include/rnf_hip.h).
//
// Row r = t * npix + p of the level-l grid is Rx(phi_p) Rz(theta_p) Rx(tau_t) O (utils/sd.py:47-82 generate_healpix_grid, offset on the
// right as eval.py:440-442 `grid @ random_rot`), with (cos theta_p, phi_p) the centre of HEALPix pixel p in the RING ordering for
// nside = 2^l (Gorski et al. 2005, pix2ang_ring), tau_t = 2 pi t / (6 nside) (np.linspace(..., endpoint=False)), Rx / Rz active
// rotations (scipy's from_euler("X" / "Z")).  fp64 throughout, one rounding per entry at the store.  grid_row is the one definition of a
// row: the full grid and the children of the beam search both call it, so that a child is bit-identical to the full grid's row.
//
// Hierarchy: the children of cell (l, t, p) are the 12 level-(l + 1) rows with pixel ring(4 nest(p) + c), c = 0..3 (the four NESTED
// sub-pixels; ring2nest / nest2ring of Gorski et al. 2005 at nside and 2 nside) and tilt 2t - 1, 2t, 2t + 1 modulo 6 * 2^(l + 1) (tilt
// 2t is the parent's own angle, the odd ones lie on its tilt cell's boundaries and are shared with the neighbouring parents).  Child
// j = 4 k + c takes tilt 2t - 1 + k.  The children of all level-l cells cover every level-(l + 1) row.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rnf {
namespace so3g {

constexpr int MAX_LEVEL = 8;

__host__ __device__ inline long long isqrt_ll(long long v) {
    long long s = (long long)sqrt((double)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

// row r of the level-`level` grid times O (o: row-major fp64) into dst[9]
__host__ __device__ __forceinline__ void grid_row(int level, long long r, const double *o, float *dst) {
    const long long nside = 1LL << level, npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1);
    const double pi = M_PI, tilt_step = 2.0 * M_PI / (double)(6LL << level);
    const long long t = r / npix, p = r - t * npix;
    double z, sth, phi;                                      // cos / sin of the polar angle, azimuth
    if (p < ncap) {                                          // north polar cap: ring i holds 4 i pixels
        const long long i = (1 + isqrt_ll(1 + 2 * p)) >> 1, j = p + 1 - 2 * i * (i - 1);
        const double tmp = (double)(i * i) / (double)(3 * nside * nside);
        z = 1.0 - tmp;
        sth = sqrt(tmp * (2.0 - tmp));
        phi = ((double)j - 0.5) * pi / (double)(2 * i);
    } else if (p < npix - ncap) {                            // belt: 2 nside + 1 rings of 4 nside pixels
        const long long q = p - ncap, i = q / (4 * nside) + nside, j = q % (4 * nside) + 1;
        const double f = ((i + nside) & 1) ? 1.0 : 0.5;
        z = (double)(2 * nside - i) * 2.0 / (double)(3 * nside);
        sth = sqrt((1.0 - z) * (1.0 + z));
        phi = ((double)j - f) * pi / (double)(2 * nside);
    } else {                                                 // south polar cap, mirrored
        const long long q = npix - p, i = (1 + isqrt_ll(2 * q - 1)) >> 1, j = 4 * i + 1 - (q - 2 * i * (i - 1));
        const double tmp = (double)(i * i) / (double)(3 * nside * nside);
        z = tmp - 1.0;
        sth = sqrt(tmp * (2.0 - tmp));
        phi = ((double)j - 0.5) * pi / (double)(2 * i);
    }
    double sphi, cphi, stau, ctau;
    sincos(phi, &sphi, &cphi);
    sincos((double)t * tilt_step, &stau, &ctau);
    // Rx(phi) Rz(theta): columns (cos t, cphi sin t, sphi sin t), (-sin t, cphi cos t, sphi cos t), (0, -sphi, cphi); then Rx(tau)
    // mixes the last two columns
    const double a[9] = {z, -sth * ctau, sth * stau,
                         cphi * sth, cphi * z * ctau - sphi * stau, -cphi * z * stau - sphi * ctau,
                         sphi * sth, sphi * z * ctau + cphi * stau, -sphi * z * stau + cphi * ctau};
    for (int row = 0; row < 3; ++row)
        for (int col = 0; col < 3; ++col)
            dst[row * 3 + col] = (float)(a[row * 3] * o[col] + a[row * 3 + 1] * o[3 + col] + a[row * 3 + 2] * o[6 + col]);
}

__host__ __device__ __forceinline__ void load_offset(const float *offset, double *o) {
    for (int c = 0; c < 9; ++c) o[c] = (c % 4 == 0) ? 1.0 : 0.0;
    if (offset)
        for (int c = 0; c < 9; ++c) o[c] = (double)offset[c];
}

#if defined(__HIPCC__) && !defined(RNF_SO3G_HOST_ONLY)     // the host builds of the tests define it: no device code to link
__global__ void so3_healpix_grid_kernel(int level, long long rows, const float *offset, float *out) {
    double o[9];
    load_offset(offset, o);
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x)
        grid_row(level, r, o, out + r * 9);
}
#endif  // __HIPCC__ && !RNF_SO3G_HOST_ONLY

// HEALPix face tables of Gorski et al. 2005: jrll = {2,2,2,2,3,3,3,3,4,4,4,4}, jpll = {1,3,5,7,0,2,4,6,1,3,5,7}
__host__ __device__ __forceinline__ long long jrll(long long f) { return 2 + (f >> 2); }
__host__ __device__ __forceinline__ long long jpll(long long f) { return 2 * (f & 3) + ((f >> 2) != 1); }

__host__ __device__ __forceinline__ long long spread_bits(long long v) {           // bit b -> bit 2b (v < 2^16)
    long long r = 0;
    for (int b = 0; b < 16; ++b) r |= ((v >> b) & 1) << (2 * b);
    return r;
}

__host__ __device__ __forceinline__ long long compress_bits(long long v) {         // bit 2b -> bit b
    long long r = 0;
    for (int b = 0; b < 16; ++b) r |= ((v >> (2 * b)) & 1) << b;
    return r;
}

// RING pixel -> NESTED pixel at nside (ring2xyf, then xyf2nest)
__host__ __device__ inline long long ring2nest(long long nside, long long pix) {
    const long long npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1), nl2 = 2 * nside;
    long long iring, iphi, kshift, nr, face;
    if (pix < ncap) {
        iring = (1 + isqrt_ll(1 + 2 * pix)) >> 1;
        iphi = pix + 1 - 2 * iring * (iring - 1);
        kshift = 0;
        nr = iring;
        face = (iphi - 1) / nr;
    } else if (pix < npix - ncap) {
        const long long ip = pix - ncap, tmp = ip / (4 * nside);
        iring = tmp + nside;
        iphi = ip - tmp * 4 * nside + 1;
        kshift = (iring + nside) & 1;
        nr = nside;
        const long long ire = tmp + 1, irm = nl2 + 2 - ire;
        const long long ifm = (iphi - (ire >> 1) + nside - 1) / nside, ifp = (iphi - (irm >> 1) + nside - 1) / nside;
        face = ifp == ifm ? (ifp | 4) : ifp < ifm ? ifp : ifm + 8;
    } else {
        const long long ip = npix - pix;
        nr = (1 + isqrt_ll(2 * ip - 1)) >> 1;
        iphi = 4 * nr + 1 - (ip - 2 * nr * (nr - 1));
        kshift = 0;
        iring = 4 * nside - nr;
        face = 8 + (iphi - 1) / nr;
    }
    const long long irt = iring - jrll(face) * nside + 1;
    long long ipt = 2 * iphi - jpll(face) * nr - kshift - 1;
    if (ipt >= nl2) ipt -= 8 * nside;
    const long long ix = (ipt - irt) >> 1, iy = (-ipt - irt) >> 1;
    return face * nside * nside + spread_bits(ix) + (spread_bits(iy) << 1);
}

// NESTED pixel -> RING pixel at nside (nest2xyf, then xyf2ring)
__host__ __device__ inline long long nest2ring(long long nside, long long pix) {
    const long long npface = nside * nside, npix = 12 * npface, ncap = 2 * nside * (nside - 1), nl4 = 4 * nside;
    const long long face = pix / npface, ipf = pix - face * npface;
    const long long ix = compress_bits(ipf), iy = compress_bits(ipf >> 1);
    const long long jr = jrll(face) * nside - ix - iy - 1;
    long long nr, n_before, kshift;
    if (jr < nside) {
        nr = jr;
        n_before = 2 * jr * (jr - 1);
        kshift = 0;
    } else if (jr < 3 * nside) {
        nr = nside;
        n_before = ncap + (jr - nside) * nl4;
        kshift = (jr - nside) & 1;
    } else {
        nr = nl4 - jr;
        n_before = npix - 2 * nr * (nr + 1);
        kshift = 0;
    }
    long long jp = (jpll(face) * nr + ix - iy + 1 + kshift) / 2;
    if (jp > nl4) jp -= nl4;
    else if (jp < 1) jp += nl4;
    return n_before + jp - 1;
}

// child j (0..11) of level-`level` row r (0 <= r < 72 * 8^level), as a level-(level + 1) row
__host__ __device__ __forceinline__ long long child_row(int level, long long r, int j) {
    const long long nside = 1LL << level, npix = 12 * nside * nside, tilts = 12 * nside;     // the child level's 6 * 2 nside tilts
    const long long t = r / npix, p = r - t * npix;
    const long long ct = (2 * t - 1 + (j >> 2) + tilts) % tilts;
    const long long cp = nest2ring(2 * nside, 4 * ring2nest(nside, p) + (j & 3));
    return ct * (4 * npix) + cp;
}

#if defined(__HIPCC__) && !defined(RNF_SO3G_HOST_ONLY)
// one thread per child: rows_out[q * 12 + j] = child j of parents[q] (-1 for a parent outside the level's rows), rot_out (optional) its
// row of the level-(level + 1) grid times O (the rotation of row 0 for a missing child, so that every output is a rotation)
__global__ void so3_grid_children_kernel(int level, long long n, const long long *parents, const float *offset, long long *rows_out,
                                         float *rot_out) {
    double o[9];
    load_offset(offset, o);
    const long long rows = 72LL << (3 * level), total = n * 12;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
        const long long q = k / 12, r = parents[q];
        const long long c = (r >= 0 && r < rows) ? child_row(level, r, (int)(k - q * 12)) : -1;
        rows_out[k] = c;
        if (rot_out) grid_row(level + 1, c < 0 ? 0 : c, o, rot_out + k * 9);
    }
}
#endif  // __HIPCC__ && !RNF_SO3G_HOST_ONLY

}  // namespace so3g
}  // namespace rnf
