"""Mirror of the reference's utils/sd.py: query rotations for pose estimation -- uniform random ones (the pytorch3d rule) or the
equivolumetric HEALPix grid over SO(3) of the IPDF line (Yershova et al. 2010), 72 * 8^level rotations.

The grid is generated on the GPU by ``rnf_so3_healpix_grid`` (no healpy, scipy or numpy build on the host), optionally already multiplied on
the right by an offset rotation (eval.py:440-442 ``grid @ random_rot``).  As in the reference, the functions return CPU tensors unless a
``device`` is given; the GPU does the work either way.
"""
import numpy as np
import torch

from .. import _lib
from .fisher import quaternion_to_matrix

MAX_LEVEL = 8


def grid_size(recursion_level: int) -> int:
    """Rotations in the level-``recursion_level`` grid: 72 * 8^level."""
    return 72 * 8 ** int(recursion_level)


def closest_grid_level(num_queries) -> int:
    """The level whose grid size is closest to ``num_queries`` in log space (utils/sd.py:31-33; the first on a tie)."""
    sizes = 72 * 8 ** np.arange(MAX_LEVEL + 1)
    return int(np.argmin(np.abs(np.log(num_queries) - np.log(sizes))))


def random_rotations(n: int, dtype=None, device=None) -> torch.Tensor:
    """``pytorch3d.transforms.random_rotations``: normalised Gaussian quaternions from torch's generator, real part made non-negative."""
    o = torch.randn((n, 4), dtype=dtype, device=device)
    s = (o * o).sum(1)
    return quaternion_to_matrix(o / torch.copysign(torch.sqrt(s), o[:, 0])[:, None])


def _devices(device):
    """-> (the GPU the grid is generated on, the device it is returned on: the CPU when ``device`` is None)."""
    want = torch.device("cpu") if device is None else torch.device(device)
    gen = want if want.type == "cuda" else torch.device("cuda")
    if gen.index is None:
        gen = torch.device("cuda", torch.cuda.current_device())
    return gen, (gen if want.type == "cuda" else want)


def generate_healpix_grid(recursion_level=None, size=None, device=None, offset=None) -> torch.Tensor:
    """utils/sd.py:47-82: the [72 * 8^level, 3, 3] float32 grid, row t * npix + p = Rx(azimuth_p) Rz(polar_p) Rx(tilt_t) (tilt-major).

    ``size``: the level is round(log8(size / 72)), as in the reference.  ``offset`` [3,3]: every row is multiplied on the right by it (on the
    device, fp64).  ``device``: where the result lives (default: the CPU, as in the reference; the grid is built on the current GPU and
    copied back)."""
    if recursion_level is None and size is None:
        raise ValueError("generate_healpix_grid: give recursion_level or size")
    if size:
        recursion_level = max(int(np.round(np.log(size / 72.0) / np.log(8.0))), 0)
    level = int(recursion_level)
    if not 0 <= level <= MAX_LEVEL:
        raise ValueError(f"generate_healpix_grid: recursion level {level} outside 0..{MAX_LEVEL}")
    dev, where = _devices(device)
    out = torch.empty((grid_size(level), 3, 3), dtype=torch.float32, device=dev)
    off = None
    if offset is not None:
        off = offset.reshape(3, 3).to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rnf_so3_healpix_grid(level, off.data_ptr() if off is not None else None, out.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream))
    return out.to(where)


_grids = {}


def get_closest_available_grid(num_queries, device=None) -> torch.Tensor:
    """utils/sd.py:30-44: the grid whose size is closest to ``num_queries`` in log space, built once per (level, device) and cached."""
    level = closest_grid_level(num_queries)
    key = (level, str(_devices(device)[1]))
    grid = _grids.get(key)
    if grid is None:
        grid = _grids[key] = generate_healpix_grid(recursion_level=level, device=device)
    return grid


def generate_queries(number_queries, mode="random", device=None) -> torch.Tensor:
    """utils/sd.py:11-26: [number_queries, 3, 3] uniform random rotations (``mode='random'``) or the closest available grid
    (``mode='grid'``, 72 * 8^level rows)."""
    if mode == "random":
        return random_rotations(number_queries, device=device)
    if mode == "grid":
        return get_closest_available_grid(number_queries, device=device)
    raise ValueError(f"generate_queries: mode must be 'random' or 'grid', got {mode!r}")
