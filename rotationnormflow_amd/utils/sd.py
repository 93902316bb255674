"""Mirror of the reference's utils/sd.py: query rotations for pose estimation -- uniform random ones (the pytorch3d rule) or the
equivolumetric HEALPix grid over SO(3) of the IPDF line (Yershova et al. 2010), 72 * 8^level rotations.

The grid is generated on the GPU by ``rnf_so3_healpix_grid`` (no healpy, scipy or numpy build on the host), optionally already multiplied on
the right by an offset rotation (eval.py:440-442 ``grid @ random_rot``).  As in the reference, the functions return CPU tensors unless a
``device`` is given; the GPU does the work either way.

``grid_index`` and ``grid_histogram`` go the other way, from rotations on the device to the grid cells that hold them
(``rnf_so3_grid_locate``); ``grid_cell_points`` is the chart of a cell, from a row and a point of the unit cube to a rotation inside the cell
(``rnf_so3_grid_cell_points``).
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


GRID_HISTOGRAM_MAX_ROWS = 1 << 26                  # rnf_so3_grid_locate's limit on a histogram (include/rnf_hip.h): level 6 fits


def _locate_inputs(rotations, recursion_level, offset, who: str, histogram: bool = False):
    """Argument checks of the locate functions, all before a launch -> (level, rotations float32 contiguous, offset [9] or None)."""
    level = int(recursion_level)
    if not 0 <= level <= MAX_LEVEL:
        raise ValueError(f"{who}: recursion level {level} outside 0..{MAX_LEVEL}")
    if rotations.dim() < 2 or tuple(rotations.shape[-2:]) != (3, 3) or (histogram and rotations.dim() not in (3, 4)):
        raise ValueError(f"{who}: rotations of shape {tuple(rotations.shape)} (want {'[n,3,3] or [g,n,3,3]' if histogram else '[..., 3, 3]'})")
    if histogram and grid_size(level) > GRID_HISTOGRAM_MAX_ROWS:
        raise ValueError(f"{who}: level {level} has {grid_size(level)} grid rows (at most 2^26)")
    if offset is not None and offset.numel() != 9:
        raise ValueError(f"{who}: offset of shape {tuple(offset.shape)} (want [3, 3])")
    if not rotations.is_cuda:
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    rot = rotations.detach().to(torch.float32).contiguous()
    off = offset.detach().reshape(9).to(device=rot.device, dtype=torch.float32).contiguous() if offset is not None else None
    return level, rot, off


def grid_index(rotations: torch.Tensor, recursion_level: int, offset=None) -> torch.Tensor:
    """The row of ``generate_healpix_grid(recursion_level, offset=offset)`` whose cell holds each of ``rotations`` [..., 3, 3] (on the
    device): the inverse of the grid's row function (``rnf_so3_grid_locate``, include/rnf_hip.h).  Every grid row is in its own cell; the
    cells have equal Haar volume and are not the Voronoi cells of the grid rotations.  A rotation with a non-finite entry has row -1.
    -> int64 [...]"""
    level, rot, off = _locate_inputs(rotations, recursion_level, offset, "grid_index")
    rows = torch.empty(rot.shape[:-2], dtype=torch.int64, device=rot.device)
    if rows.numel() == 0:                                  # nothing to locate (an empty tensor has no address to pass)
        return rows
    _lib.call("so3_grid_locate", _lib.GridLocate(level=level, rotations=rot.data_ptr(), n=rows.numel(), g=1,
                                                  offset=off.data_ptr() if off is not None else None, rows_out=rows.data_ptr()), rot.device)
    return rows


def grid_histogram(rotations: torch.Tensor, recursion_level: int, offset=None, out: torch.Tensor = None) -> torch.Tensor:
    """How many of each image's ``rotations`` ([n,3,3]: one image, or [g,n,3,3]; on the device) lie in each cell of the level's grid
    (``grid_index``'s cells; rows -1 are not counted) -> int32 [g, 72 * 8^level].  With ``out`` (int32 [g,Q], contiguous, on the
    device) the counts are added to it and it is returned, so a large sample set can be streamed through several calls.  Integer atomics:
    bit-identical from run to run.  Levels 0..6 (Q <= 2^26), g <= 65535."""
    level, rot, off = _locate_inputs(rotations, recursion_level, offset, "grid_histogram", histogram=True)
    Q = grid_size(level)
    g, n = (1, rot.shape[0]) if rot.dim() == 3 else rot.shape[:2]
    if not 1 <= g <= 65535:
        raise ValueError(f"grid_histogram: {g} images (1 to 65535)")
    if out is None:
        out = torch.zeros(g, Q, dtype=torch.int32, device=rot.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (g, Q) or not out.is_contiguous() or out.device != rot.device:
        raise ValueError(f"grid_histogram: out must be a contiguous int32 [{g},{Q}] tensor on {rot.device}")
    if n == 0:
        return out
    _lib.call("so3_grid_locate", _lib.GridLocate(level=level, rotations=rot.data_ptr(), n=n, g=g,
                                                  offset=off.data_ptr() if off is not None else None, counts=out.data_ptr()), rot.device)
    return out


GRID_CELL_POINTS_MAX_LEVEL = 6                     # rnf_so3_grid_cell_points' limit (include/rnf_hip.h)


def grid_cell_points(index: torch.Tensor, u: torch.Tensor, recursion_level: int, offset=None) -> torch.Tensor:
    """The chart of the grid's cells (``rnf_so3_grid_cell_points``, include/rnf_hip.h): the rotation at ``u`` [..., 3] in [0, 1]^3 inside
    the cell of row ``index`` [...] (int64) of ``generate_healpix_grid(recursion_level, offset=offset)``, both on the device.  u[..., 0:2]
    move across the HEALPix pixel in its face coordinates (an equal-area map), u[..., 2] along the tilt interval, so uniform ``u`` are
    Haar-uniform in the cell (``grid_index`` of the result is ``index``, up to points within rounding of a cell's boundary) and
    u = (0.5, 0.5, 0.5) is the grid's row.  A row outside the grid or a ``u`` outside [0, 1] gives NaNs.  Levels 0..6.
    -> float32 [..., 3, 3]"""
    level = int(recursion_level)
    if not 0 <= level <= GRID_CELL_POINTS_MAX_LEVEL:
        raise ValueError(f"grid_cell_points: recursion level {level} outside 0..{GRID_CELL_POINTS_MAX_LEVEL}")
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise ValueError(f"grid_cell_points: index of dtype {getattr(index, 'dtype', type(index))} (want int64 grid rows)")
    if not isinstance(u, torch.Tensor) or u.dim() < 1 or tuple(u.shape) != tuple(index.shape) + (3,):
        raise ValueError(f"grid_cell_points: u of shape {tuple(getattr(u, 'shape', ()))} for index {tuple(index.shape)} (want [..., 3])")
    if offset is not None and offset.numel() != 9:
        raise ValueError(f"grid_cell_points: offset of shape {tuple(offset.shape)} (want [3, 3])")
    if not index.is_cuda or not u.is_cuda:
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    dev = index.device
    rows = index.detach().contiguous()
    uu = u.detach().to(device=dev, dtype=torch.float32).contiguous()
    off = offset.detach().reshape(9).to(device=dev, dtype=torch.float32).contiguous() if offset is not None else None
    rot = torch.empty(tuple(index.shape) + (3, 3), dtype=torch.float32, device=dev)
    if rows.numel() == 0:
        return rot
    _lib.call("so3_grid_cell_points", _lib.GridCellPoints(level=level, offset=off.data_ptr() if off is not None else None, rows=rows.data_ptr(),
                                                           u=uu.data_ptr(), n=rows.numel(), rot_out=rot.data_ptr()), dev)
    return rot
