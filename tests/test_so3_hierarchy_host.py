"""The hierarchy of the HEALPix SO(3) grid that the coarse-to-fine beam search walks (rnf_so3_grid_children, include/rnf_hip.h), CPU part:
a numpy restatement of HEALPix's ring2nest / nest2ring (Gorski et al. 2005) and of the children rule, checked for levels 0..4 -- the
conversions are inverse bijections, the children of all level-l rows cover level l + 1, and every child pixel's centre lies within its
parent pixel's maximal radius.  tests/test_gpu_grid_beam.py checks the device children against this rule.  Also the C ABI's refusals of
the two new entry points, which need no device."""
import ctypes as C

import numpy as np
import pytest

from tests.test_so3_grid import ring_pix2ang

JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], np.int64)
JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7], np.int64)


def _isqrt(v):
    s = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    s -= s * s > v
    s += (s + 1) * (s + 1) <= v
    return s


def _spread(v):
    r = np.zeros_like(v)
    for b in range(16):
        r |= ((v >> b) & 1) << (2 * b)
    return r


def _compress(v):
    r = np.zeros_like(v)
    for b in range(16):
        r |= ((v >> (2 * b)) & 1) << b
    return r


def ring2nest(nside: int, pix) -> np.ndarray:
    """RING -> NESTED pixel numbers at ``nside`` (healpix_base ring2xyf + xyf2nest)."""
    p = np.asarray(pix, np.int64)
    npix, ncap, nl2 = 12 * nside * nside, 2 * nside * (nside - 1), 2 * nside
    iring, iphi, kshift, nr, face = (np.zeros_like(p) for _ in range(5))
    north, south = p < ncap, p >= npix - ncap
    belt = ~north & ~south
    q = p[north]
    i = (1 + _isqrt(1 + 2 * q)) >> 1
    iring[north], iphi[north], nr[north] = i, q + 1 - 2 * i * (i - 1), i
    face[north] = (iphi[north] - 1) // i
    q = p[belt] - ncap
    tmp = q // (4 * nside)
    iring[belt], iphi[belt], nr[belt] = tmp + nside, q - tmp * 4 * nside + 1, nside
    kshift[belt] = (iring[belt] + nside) & 1
    ire, irm = tmp + 1, nl2 + 2 - (tmp + 1)
    ifm = (iphi[belt] - (ire >> 1) + nside - 1) // nside
    ifp = (iphi[belt] - (irm >> 1) + nside - 1) // nside
    face[belt] = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))
    q = npix - p[south]
    i = (1 + _isqrt(2 * q - 1)) >> 1
    iphi[south], nr[south], iring[south] = 4 * i + 1 - (q - 2 * i * (i - 1)), i, 4 * nside - i
    face[south] = 8 + (iphi[south] - 1) // i
    irt = iring - JRLL[face] * nside + 1
    ipt = 2 * iphi - JPLL[face] * nr - kshift - 1
    ipt = np.where(ipt >= nl2, ipt - 8 * nside, ipt)
    ix, iy = (ipt - irt) >> 1, (-ipt - irt) >> 1
    return face * nside * nside + _spread(ix) + (_spread(iy) << 1)


def nest2ring(nside: int, pix) -> np.ndarray:
    """NESTED -> RING pixel numbers at ``nside`` (healpix_base nest2xyf + xyf2ring)."""
    p = np.asarray(pix, np.int64)
    npface = nside * nside
    npix, ncap, nl4 = 12 * npface, 2 * nside * (nside - 1), 4 * nside
    face = p // npface
    ipf = p - face * npface
    ix, iy = _compress(ipf), _compress(ipf >> 1)
    jr = JRLL[face] * nside - ix - iy - 1
    north, south = jr < nside, jr >= 3 * nside
    nr = np.where(north, jr, np.where(south, nl4 - jr, nside))
    n_before = np.where(north, 2 * jr * (jr - 1), np.where(south, npix - 2 * nr * (nr + 1), ncap + (jr - nside) * nl4))
    kshift = np.where(north | south, 0, (jr - nside) & 1)
    jp = (JPLL[face] * nr + ix - iy + 1 + kshift) // 2
    jp = np.where(jp > nl4, jp - nl4, np.where(jp < 1, jp + nl4, jp))
    return n_before + jp - 1


def children(level: int, rows) -> np.ndarray:
    """[n, 12] level-(level + 1) children of level-``level`` grid rows: child 4 k + c has pixel ring(4 nest(p) + c) and tilt 2t - 1 + k."""
    r = np.asarray(rows, np.int64)
    nside = 2 ** level
    npix, tilts = 12 * nside * nside, 12 * nside
    t, p = r // npix, r % npix
    sub = 4 * ring2nest(nside, p)[:, None] + np.arange(4)[None, :]
    cp = nest2ring(2 * nside, sub.reshape(-1)).reshape(-1, 4)
    ct = (2 * t[:, None] - 1 + np.arange(3)[None, :]) % tilts
    return (ct[:, :, None] * (4 * npix) + cp[:, None, :]).reshape(-1, 12)


def max_pixrad(nside: int) -> float:
    """The largest angle between a pixel centre and its corners (healpix_base::max_pixrad)."""
    za, pa = 2.0 / 3.0, np.pi / (4 * nside)
    t1 = (1.0 - 1.0 / nside) ** 2
    zb, pb = 1.0 - t1 / 3.0, 0.0
    va = np.array([np.sqrt(1 - za * za) * np.cos(pa), np.sqrt(1 - za * za) * np.sin(pa), za])
    vb = np.array([np.sqrt(1 - zb * zb) * np.cos(pb), np.sqrt(1 - zb * zb) * np.sin(pb), zb])
    return float(np.arctan2(np.linalg.norm(np.cross(va, vb)), va @ vb))


def _vec(nside, pix):
    z, phi = ring_pix2ang(nside, pix)
    s = np.sqrt(np.maximum(0.0, (1 - z) * (1 + z)))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4, 5])
def test_ring_nest_conversions_are_inverse_bijections(level):
    nside = 2 ** level
    pix = np.arange(12 * nside * nside)
    nest = ring2nest(nside, pix)
    assert np.array_equal(np.sort(nest), pix)
    assert np.array_equal(nest2ring(nside, nest), pix)
    assert np.array_equal(ring2nest(nside, nest2ring(nside, pix)), pix)
    if level == 0:
        assert np.array_equal(nest, pix)                     # nside = 1: one pixel per base face, both schemes number the faces alike


def test_published_nside_2_numbering():
    # nside = 2: NESTED pixels 0..3 make up base face 0, whose RING numbers are the first pixel of ring 1 and the belt below it
    assert nest2ring(2, np.arange(4)).tolist() == [13, 5, 4, 0]
    # the north pole's four ring-1 pixels are the last sub-pixel of faces 0..3
    assert ring2nest(2, np.arange(4)).tolist() == [3, 7, 11, 15]


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_children_cover_the_next_level(level):
    rows = np.arange(72 * 8 ** level)
    ch = children(level, rows)
    assert ch.shape == (rows.size, 12) and ch.min() >= 0 and ch.max() < 72 * 8 ** (level + 1)
    assert np.array_equal(np.unique(ch), np.arange(72 * 8 ** (level + 1)))
    # the tilt 2t child is the parent's own angle; each tilt of the next level is a child of one or two parents' tilts
    nside = 2 ** level
    npix = 12 * nside * nside
    assert np.array_equal(ch[:, 4:8] // (4 * npix), np.repeat(2 * (rows // npix), 4).reshape(-1, 4))
    counts = np.bincount(ch.reshape(-1), minlength=72 * 8 ** (level + 1))
    assert set(np.unique(counts).tolist()) == {1, 2}


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_child_pixels_lie_within_the_parent_pixel(level):
    nside = 2 ** level
    pix = np.arange(12 * nside * nside)
    sub = nest2ring(2 * nside, (4 * ring2nest(nside, pix))[:, None] + np.arange(4)[None, :])
    parent, child = _vec(nside, pix), _vec(2 * nside, sub.reshape(-1)).reshape(-1, 4, 3)
    ang = np.arccos(np.clip(np.einsum("pk,pck->pc", parent, child), -1.0, 1.0))
    assert ang.max() < max_pixrad(nside)
    # and the parents' sub-pixels partition the next level's pixels
    assert np.array_equal(np.sort(sub.reshape(-1)), np.arange(48 * nside * nside))


def test_c_abi_refuses_bad_children_and_selection_structs():
    from rotationnormflow_amd import _lib
    L = _lib.lib()
    ch = _lib.GridChildren(level=8, parents=1, n=1, rows_out=1)
    assert L.rnf_so3_grid_children(C.byref(ch)) != 0 and b"level" in L.rnf_last_error()
    ch = _lib.GridChildren(level=2, parents=None, n=4, rows_out=None)
    assert L.rnf_so3_grid_children(C.byref(ch)) != 0
    ch = _lib.GridChildren(level=2, parents=None, n=0)
    assert L.rnf_so3_grid_children(C.byref(ch)) == 0                  # nothing to do
    ch = _lib.GridChildren(level=2)
    ch.struct_bytes = 8
    assert L.rnf_so3_grid_children(C.byref(ch)) != 0 and b"struct_bytes" in L.rnf_last_error()
    for kw in (dict(M=100, g=1, beam=0), dict(M=100, g=1, beam=1025), dict(M=0, g=1, beam=4), dict(M=100, g=0, beam=4),
               dict(M=1 << 31, g=1, beam=4)):
        sel = _lib.GridBeamSelect(logp=1, rows_out=1, logp_out=1, **kw)
        assert L.rnf_grid_beam_select_workspace_bytes(C.byref(sel)) == 0
        assert L.rnf_grid_beam_select(C.byref(sel)) != 0
    sel = _lib.GridBeamSelect(logp=1, rows_out=1, logp_out=1, M=4096, g=3, beam=16)
    assert L.rnf_grid_beam_select_workspace_bytes(C.byref(sel)) == 8
    sel = _lib.GridBeamSelect(logp=1, rows_out=1, logp_out=1, M=4097, g=3, beam=16)
    assert L.rnf_grid_beam_select_workspace_bytes(C.byref(sel)) == 2 * 3 * 2 * 16 * 8
    assert L.rnf_grid_beam_select(C.byref(sel)) != 0 and b"workspace" in L.rnf_last_error()
