"""Kernel density estimates on SO(3) with an isotropic matrix-Fisher kernel, from one pairwise HIP kernel sum (``rnf_so3_kernel_sum``,
csrc/so3_kernel_sum.h).  Densities are w.r.t. the Haar probability measure, like every density in the package.

``so3_kernel_log_density`` is the primitive: log sum_j w_j k_kappa(C_j, Q_i) for sets of centres and queries, several bandwidths and
several rows of log-weights at once, with leave-one-out.  ``so3_kernel_moments`` (``rnf_so3_kernel_moments``, csrc/so3_kernel_moments.h)
adds the responsibility-weighted first moments of the same sum: the score, the mean-shift step and the derivative with respect to the
bandwidth.  ``SO3KernelDensity`` is the estimate with its bandwidth chosen by the leave-one-out likelihood; its ``log_prob`` is
differentiable with respect to the rotations, and it has ``score``, ``mean_shift``, ``modes`` and ``sample``.  ``grid_pose.grid_diffuse``
builds the prediction step of a Bayes filter on the SO(3) grid on the primitive, ``grid_pose.grid_modes_refine`` takes grid modes off the
grid by mean shift."""
from __future__ import annotations

import ctypes as C
import math
import warnings

import torch

from .. import _lib

MAX_BANDWIDTHS = 8                                  # J of one launch (include/rnf_hip.h)
MAX_KAPPA = 1.0e6
MAX_CENTRES = 1 << 24
MAX_GROUPS = 65535
CHUNK = 4096                                        # centres per chunk: the workspace holds 12 bytes per (group, bandwidth, chunk, query)
WORKSPACE_CAP = 64 << 20                            # bytes; the queries (and, where one query's share exceeds it, the groups) are tiled
DEFAULT_KAPPAS = tuple(2.0 ** (k / 2.0) for k in range(4, 29))   # 4 .. 16384 in steps of sqrt(2): 25 candidates


def _rotations(x, name: str, who: str):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or tuple(x.shape[-2:]) != (3, 3):
        raise ValueError(f"{who}: {name} {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}, expected [n,3,3]")
    if not x.is_cuda:
        raise ValueError(f"{who}: {name} is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    return _aligned(x.detach().to(torch.float32).contiguous())


def _aligned(x):
    """The library takes 16-byte aligned rotation arrays; a view that starts inside an allocation (rows of 36 bytes) is copied."""
    return x if x.data_ptr() % 16 == 0 else x.clone()


def _kappas(kappa, who: str):
    """-> (list of floats, whether ``kappa`` was a scalar)"""
    if isinstance(kappa, torch.Tensor):
        kappa = kappa.detach().cpu().tolist()
    scalar = not isinstance(kappa, (list, tuple))
    ks = [float(kappa)] if scalar else [float(k) for k in kappa]
    if not ks:
        raise ValueError(f"{who}: kappa is empty")
    for k in ks:
        if not (math.isfinite(k) and 0.0 <= k <= MAX_KAPPA):
            raise ValueError(f"{who}: kappa={k} outside 0..1e6")
    return ks, scalar


def so3_kernel_log_density(centres, queries=None, kappa=None, log_weights=None, leave_one_out: bool = False, workspace_cap: int = None):
    """log sum_j w_gj k_a(C_j, Q_i) on the device: ``centres`` [n,3,3], ``queries`` [m,3,3] (None: the centres), ``kappa`` a scalar or a
    sequence of J concentrations (each in 0..1e6; any J: launches take 8 at a time), ``log_weights`` None (w = 1/n), [n] or [G,n] with
    w_g = softmax(log_weights[g]).  k_kappa(C, Q) = exp(-(kappa/2) |Q - C|_F^2 - l(kappa)) is the density of MF(kappa C) at Q.
    ``leave_one_out``: the queries are the centres and index i is left out of query i's sum, which is renormalised by 1 - w_gi.
    -> float32 [m], [J,m], [G,m] or [G,J,m]: a rank per sequence-valued ``kappa`` and per 2-D ``log_weights``.
    A centre with log-weight -inf is left out; another non-finite centre or a NaN log-weight makes its group NaN, a non-finite query its
    outputs, a group without mass (all -inf, leave-one-out of one centre) everything.  A query's result is bit-identical however the
    call is tiled, so the tiling that keeps the workspace under ``workspace_cap`` (64 MiB) is invisible; leave-one-out cannot tile
    its queries and raises ValueError where one bandwidth's workspace, 12 ceil(n/4096) n bytes, exceeds the cap.  Stream-ordered, no host
    synchronisation, no gradient."""
    who = "so3_kernel_log_density"
    Cn = _rotations(centres, "centres", who)
    n, dev = Cn.shape[0], Cn.device
    if not 1 <= n <= MAX_CENTRES:
        raise ValueError(f"{who}: centres holds {n} rotations (1 to 2^24)")
    if kappa is None:
        raise ValueError(f"{who}: kappa is required")
    ks, scalar_kappa = _kappas(kappa, who)
    if leave_one_out and queries is not None and queries is not centres:
        raise ValueError(f"{who}: queries must be None with leave_one_out (the queries are the centres)")
    Qr = Cn if queries is None or queries is centres else _rotations(queries, "queries", who)
    if Qr.device != dev:
        raise ValueError(f"{who}: queries on {Qr.device}, centres on {dev}")
    m = Qr.shape[0]
    if m >= 1 << 31:
        raise ValueError(f"{who}: queries holds {m} rotations (below 2^31)")
    lw, grouped = None, False
    if log_weights is not None:
        if not isinstance(log_weights, torch.Tensor) or log_weights.dim() not in (1, 2) or log_weights.shape[-1] != n:
            raise ValueError(f"{who}: log_weights {tuple(getattr(log_weights, 'shape', ()))} for {n} centres, expected [n] or [G,n]")
        if not log_weights.is_cuda:
            raise ValueError(f"{who}: log_weights is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        grouped = log_weights.dim() == 2
        lw = log_weights.detach().to(device=dev, dtype=torch.float32).reshape(-1, n).contiguous()
    G = lw.shape[0] if lw is not None else 1
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"{who}: log_weights holds {G} groups (1 to 65535)")
    cap = WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    J = len(ks)
    out = torch.empty(G, J, m, dtype=torch.float32, device=dev)
    if m > 0:
        nchunk = (n + CHUNK - 1) // CHUNK
        # leave-one-out takes all queries in one call (they are the centres): there the bandwidths per launch shrink instead, and
        # beyond cap / (12 nchunk) centres (about 1.5e5 at 64 MiB) the workspace of one bandwidth exceeds the cap: refused
        if leave_one_out and 12 * nchunk * m > cap:
            raise ValueError(f"{who}: leave_one_out of {n} centres needs a workspace of {12 * nchunk * m} bytes per bandwidth and group, above "
                             f"workspace_cap={cap}; pass a larger workspace_cap")
        j_tile = max(1, min(MAX_BANDWIDTHS, cap // (12 * nchunk * m))) if leave_one_out else MAX_BANDWIDTHS
        for a0 in range(0, J, j_tile):
            ja = min(j_tile, J - a0)
            kap = (C.c_double * ja)(*ks[a0:a0 + ja])
            per_query = 12 * ja * nchunk                    # bytes per query and group
            g_tile = max(1, min(G, cap // (per_query * (m if leave_one_out else min(m, 256)))))
            m_tile = m if leave_one_out else max(1, min(m, cap // (per_query * g_tile)))
            m_tile = m_tile if m_tile < 4 or m_tile == m else m_tile // 4 * 4      # rows of 36 bytes: every fourth is 16-byte aligned
            for g0 in range(0, G, g_tile):
                g1 = min(G, g0 + g_tile)
                for i0 in range(0, m, m_tile):
                    i1 = min(m, i0 + m_tile)
                    part = out[g0:g1, a0:a0 + ja, i0:i1]
                    tile = _aligned(Qr[i0:i1])
                    whole = part.is_contiguous()
                    dst = part if whole else torch.empty(g1 - g0, ja, i1 - i0, dtype=torch.float32, device=dev)
                    args = _lib.So3KernelSum(centres=Cn.data_ptr(), queries=None if leave_one_out else tile.data_ptr(),
                                             log_weights=lw[g0:g1].data_ptr() if lw is not None else None, n=n, m=i1 - i0, G=g1 - g0,
                                             kappas=C.cast(kap, C.c_void_p), J=ja, leave_one_out=int(bool(leave_one_out)), out=dst.data_ptr())
                    _lib.call("so3_kernel_sum", args, dev)
                    if not whole:
                        part.copy_(dst)
    if scalar_kappa:
        out = out[:, 0]
    return out if grouped else out[0]


LOCAL_MAX_LEVEL = 6                                 # levels of rnf_so3_grid_local_sum (include/rnf_hip.h)
LOCAL_QUERY_TILE = 1 << 22                          # queries per launch of so3_grid_local_log_sum (a multiple of 4: rows of 36 bytes) ..
LOCAL_GROUP_TILE = 4096                             # .. and groups per launch; a result does not depend on either
LOCAL_NATS = 18.0                                   # the default cut: where (kappa/2) d^2 reaches 18 nats, e^-18 of the peak


def local_radius_to_d2_cut(radius_deg: float) -> float:
    """The squared chordal distance 4 (1 - cos omega) of a radius in degrees (0..180)"""
    r = float(radius_deg)
    if not (math.isfinite(r) and 0.0 <= r <= 180.0):
        raise ValueError(f"so3_grid_local_log_sum: radius_deg={radius_deg} outside 0..180")
    return 8.0 if r == 180.0 else 4.0 * (1.0 - math.cos(math.radians(r)))


def local_default_d2_cut(kappa: float) -> float:
    """The default cut of ``so3_grid_local_log_sum``: the d^2 at which (kappa/2) d^2 = 18 nats -- such a term is e^-18 = 1.5e-8 of the
    peak, below fp32 resolution -- capped at 8 (180 degrees)."""
    k = float(kappa)
    return 8.0 if k * 8.0 <= 2.0 * LOCAL_NATS else 2.0 * LOCAL_NATS / k


LOCAL_MAX_CONCENTRATION = 3.0e4                     # the largest |eigenvalue| rnf_so3_grid_local_fisher takes (include/rnf_hip.h)
LOCAL_FLOOR_SPACINGS = 1.25                         # the floor of a drifting model's cut, in grid spacings 360 / (6 2^level) degrees


def _matrix33(x, name: str, who: str):
    """A 3x3 matrix given as nested sequences, a numpy array or a tensor -> float64 numpy [3,3]; a GPU tensor is read back (a host
    synchronisation)."""
    import numpy as np
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().to(torch.float64).numpy()
    a = np.asarray(x, dtype=np.float64)
    if a.shape != (3, 3):
        raise ValueError(f"{who}: {name} {a.shape}, expected [3,3]")
    if not np.isfinite(a).all():
        raise ValueError(f"{who}: {name} holds a non-finite entry")
    return a


def motion_factors(A):
    """The drift and the concentration of a matrix-Fisher motion model x' = x E, E ~ MF(A): with the proper SVD A = U diag(s) V^T
    (U, V rotations, s1 >= s2 >= |s3|, s3 with the sign of det A),
        drift Delta = U V^T (a rotation: the mode of the step),   concentration K = V diag(s) V^T (symmetric),   A = Delta K.
    ``A`` [3,3]: nested sequences, a numpy array or a tensor -- a GPU tensor is READ BACK to the host (a synchronisation); a non-finite
    ``A`` is refused.  -> (drift [3,3] float64, concentration [3,3] float64, s [3] float64), numpy arrays."""
    import numpy as np
    a = _matrix33(A, "A", "motion_factors")
    U, s, Vt = np.linalg.svd(a)
    V = Vt.T
    s = s.copy()
    if np.linalg.det(U) < 0.0:
        U = U * np.array([1.0, 1.0, -1.0])
        s[2] = -s[2]
    if np.linalg.det(V) < 0.0:
        V = V * np.array([1.0, 1.0, -1.0])
        s[2] = -s[2]
    K = (V * s) @ V.T
    return U @ V.T, 0.5 * (K + K.T), s


def motion_matrix(drift=None, sigma_deg=(5.0, 5.0, 5.0), axes=None):
    """A motion model written in degrees -> A [3,3] float64 (numpy) for the ``motion`` arguments of ``grid_pose``.  ``drift`` [3,3]: the
    mean step, a rotation (None: none).  ``sigma_deg`` (sx, sy, sz): the standard deviations of the step's small-angle rotation vector
    about the principal axes, the columns of ``axes`` [3,3] (a rotation; None: the body axes x, y, z).  For MF(A) the rotation-vector
    variance about principal axis k is 1 / (s_i + s_j) of the OTHER two proper singular values, so with p_k = 1 / sigma_k^2 (radians)
        s_k = (p_x + p_y + p_z - 2 p_k) / 2,      A = drift  axes diag(s) axes^T.
    Every pair sum s_i + s_j = p_k is positive; one s_k is negative where one axis is much tighter than the other two.  The passes take
    |s_k| up to 3e4 (sigma down to about 0.25 degrees)."""
    import numpy as np
    who = "motion_matrix"
    sig = np.asarray(sigma_deg, dtype=np.float64).reshape(-1)
    if sig.shape != (3,) or not (np.isfinite(sig).all() and (sig > 0.0).all()):
        raise ValueError(f"{who}: sigma_deg={sigma_deg}, expected three positive finite angles")
    p = 1.0 / np.radians(sig) ** 2
    sv = 0.5 * (p.sum() - 2.0 * p)
    V = np.eye(3) if axes is None else _matrix33(axes, "axes", who)
    D = np.eye(3) if drift is None else _matrix33(drift, "drift", who)
    for name, R in (("axes", V), ("drift", D)):
        if np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0.0:
            raise ValueError(f"{who}: {name} is not a rotation")
    return D @ (V * sv) @ V.T


def local_floor_d2_cut(level: int) -> float:
    """The smallest cut of a DRIFTING model at ``level``: the chord of 1.25 grid spacings.  A shifted row C_j = G_j Delta is no grid row,
    so its nearest row is not at distance 0; the largest angle from 20 000 uniform rotations to their nearest row is 0.81 to 0.89
    spacings at levels 0 to 3."""
    return 4.0 * (1.0 - math.cos(math.radians(LOCAL_FLOOR_SPACINGS * 360.0 / (6 * 2 ** int(level)))))


def local_default_d2_cut_fisher(s, level: int, drifting: bool) -> float:
    """The default cut of the anisotropic passes: the exponent is bounded by -(s2 + s3)/4 d^2 with the two SMALLEST proper singular
    values, so the 18 nats of ``local_default_d2_cut`` are reached at d^2 = 72 / (s2 + s3) (36 / kappa for K = kappa I), capped at 8
    (180 degrees; 8 where s2 + s3 <= 9) and, where the model drifts, not below ``local_floor_d2_cut(level)``."""
    v = sorted(float(x) for x in s)
    pair = v[0] + v[1]
    cut = 8.0 if pair * 8.0 <= 4.0 * LOCAL_NATS else 4.0 * LOCAL_NATS / pair
    return min(8.0, max(cut, local_floor_d2_cut(level))) if drifting else cut


def _concentration(concentration, who: str):
    """-> (K float64 numpy [3,3], its eigenvalues in decreasing order, kappa where K is exactly kappa I else None)"""
    import numpy as np
    K = _matrix33(concentration, "concentration", who)
    norm = float(np.linalg.norm(K))
    if float(np.linalg.norm(K - K.T)) > 1e-9 * norm:
        raise ValueError(f"{who}: concentration is not symmetric")
    ev = np.linalg.eigvalsh(0.5 * (K + K.T))[::-1]
    if ev[1] + ev[2] < -1e-9 * norm:
        raise ValueError(f"{who}: concentration has two eigenvalues with a negative sum; it is not the symmetric factor of a proper SVD")
    if np.abs(ev).max() > LOCAL_MAX_CONCENTRATION:
        raise ValueError(f"{who}: concentration has an eigenvalue beyond 3e4 in magnitude")
    kappa = float(K[0, 0]) if np.array_equal(K, K[0, 0] * np.eye(3)) and K[0, 0] >= 0.0 else None
    return K, ev, kappa


def so3_grid_local_log_sum(grid, level: int, kappa: float = None, radius_deg: float = None, d2_cut: float = None, queries=None, log_weights=None,
                           offset=None, return_count: bool = False, concentration=None):
    """The neighbour-limited kernel sum over the rows of the SO(3) grid on the device (``rnf_so3_grid_local_sum``,
    csrc/so3_grid_local.h): out[g][i] = log sum_{j: d^2(G_j, Q_i) <= cut} exp(log_weights[g][j]) k_kappa(G_j, Q_i) with the kernel of
    ``so3_kernel_log_density`` and d^2 = |G_j - Q_i|_F^2 = 4 (1 - cos angle).  The log-weights are NOT normalised.
    ``grid`` [Q,3,3]: the rows of ``sd.generate_healpix_grid(level, offset=offset)``, Q = 72 * 8^level, level 0..6 (``offset`` [3,3] must be
    the grid's own; None: the identity).  ``queries`` [m,3,3] any rotations (None: the grid rows).  ``log_weights`` None (zeros), [Q] or [G,Q].
    The cut: ``d2_cut`` (0..8), or ``radius_deg`` (0..180), or by default the distance at which (kappa/2) d^2 = 18 nats, capped at 180 degrees.
    -> float32 [m] or [G,m] (with ``return_count`` also int32 [m], the rows within the cut).  An empty or massless neighbourhood gives -inf,
    a row with log-weight -inf drops out, a NaN log-weight inside a query's neighbourhood gives NaN, a non-finite query NaN and count 0.
    A result is bit-identical from run to run and however the call is tiled, so the tiling of queries and groups is invisible.
    Stream-ordered, no host synchronisation, no workspace, no gradient.
    ``concentration`` [3,3] in place of ``kappa`` (exactly one of the two): the anisotropic kernel
    k_K(G_j, Q_i) = exp(-1/2 tr((Q_i - G_j) K (Q_i - G_j)^T) - l(K)) of ``rnf_so3_grid_local_fisher``, K symmetric with eigenvalue pair
    sums >= 0 and |eigenvalues| <= 3e4 (``motion_factors``); the default cut is then ``local_default_d2_cut_fisher`` without the floor.
    A concentration that is exactly kappa I runs the isotropic entry point: the bits of ``kappa=kappa``."""
    return _grid_local_pass("so3_grid_local_log_sum", False, grid, level, kappa, radius_deg, d2_cut, queries, log_weights, offset, return_count,
                            concentration)


def so3_grid_local_log_max(grid, level: int, kappa: float = None, radius_deg: float = None, d2_cut: float = None, queries=None, log_weights=None,
                           offset=None, return_count: bool = False, concentration=None):
    """The max-plus pass over the neighbourhoods of ``so3_grid_local_log_sum`` on the device (``rnf_so3_grid_local_max``,
    csrc/so3_grid_local.h): out[g][i] = max_{j: d^2(G_j, Q_i) <= cut} (log_weights[g][j] - (kappa/2) d^2(G_j, Q_i)) - l(kappa), the largest
    TERM of that sum, and arg[g][i] = the smallest grid row j attaining it -- the step of a Viterbi recursion (``grid_pose.grid_viterbi``).
    Arguments, cut, membership and tiling are those of ``so3_grid_local_log_sum``.
    -> (float32 [m] or [G,m], int64 of the same shape) (with ``return_count`` also int32 [m]).  An empty neighbourhood, or one whose rows
    all have log-weight -inf, gives -inf and arg -1; a NaN log-weight inside a query's neighbourhood gives NaN and -1, a non-finite query
    NaN, -1 and count 0.  The maximum and the tie are decided on the kernel's fp32 term.  A result is bit-identical from run to run and
    however the call is tiled.  Stream-ordered, no host synchronisation, no workspace, no gradient.
    ``concentration`` [3,3] in place of ``kappa``: as in ``so3_grid_local_log_sum``; the term is lw - 1/2 tr((Q_i - G_j) K (Q_i - G_j)^T)."""
    return _grid_local_pass("so3_grid_local_log_max", True, grid, level, kappa, radius_deg, d2_cut, queries, log_weights, offset, return_count,
                            concentration)


def _grid_local_pass(who: str, with_arg: bool, grid, level, kappa, radius_deg, d2_cut, queries, log_weights, offset, return_count,
                     concentration=None):
    """The argument checks and the tiling the two neighbour-limited passes share; ``with_arg``: the max pass, -> (out, arg int64[, count])"""
    if (kappa is None) == (concentration is None):
        raise ValueError(f"{who}: give exactly one of kappa and concentration")
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3 or tuple(grid.shape[-2:]) != (3, 3):
        raise ValueError(f"{who}: grid {tuple(getattr(grid, 'shape', ()))}, expected [Q,3,3]")
    level = int(level)
    if not 0 <= level <= LOCAL_MAX_LEVEL:
        raise ValueError(f"{who}: level={level} outside 0..{LOCAL_MAX_LEVEL}")
    Q = 72 * 8 ** level
    if grid.shape[0] != Q:
        raise ValueError(f"{who}: grid holds {grid.shape[0]} rows, level {level} has {Q}")
    Gr = _rotations(grid, "grid", who)
    dev = Gr.device
    K = None
    if concentration is not None:
        K, ev, kappa = _concentration(concentration, who)                    # kappa: where K is exactly kappa I, the isotropic entry
    if kappa is not None:
        K = None
        (k,), scalar = _kappas(kappa, who)
        if not scalar:
            raise ValueError(f"{who}: kappa is one concentration, not a sequence")
    if radius_deg is not None and d2_cut is not None:
        raise ValueError(f"{who}: give radius_deg or d2_cut, not both")
    if radius_deg is None and d2_cut is None:
        cut = local_default_d2_cut(k) if K is None else local_default_d2_cut_fisher(ev, level, False)
    else:
        cut = local_radius_to_d2_cut(radius_deg) if radius_deg is not None else float(d2_cut)
    if not (math.isfinite(cut) and 0.0 <= cut <= 8.0):
        raise ValueError(f"{who}: d2_cut={cut} outside 0..8")
    Qr = Gr if queries is None or queries is grid else _rotations(queries, "queries", who)
    if Qr.device != dev:
        raise ValueError(f"{who}: queries on {Qr.device}, grid on {dev}")
    m = Qr.shape[0]
    if m >= 1 << 31:
        raise ValueError(f"{who}: queries holds {m} rotations (below 2^31)")
    lw, grouped = None, False
    if log_weights is not None:
        if not isinstance(log_weights, torch.Tensor) or log_weights.dim() not in (1, 2) or log_weights.shape[-1] != Q:
            raise ValueError(f"{who}: log_weights {tuple(getattr(log_weights, 'shape', ()))} for {Q} grid rows, expected [Q] or [G,Q]")
        if not log_weights.is_cuda:
            raise ValueError(f"{who}: log_weights is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        grouped = log_weights.dim() == 2
        lw = log_weights.detach().to(device=dev, dtype=torch.float32).reshape(-1, Q).contiguous()
    G = lw.shape[0] if lw is not None else 1
    if G < 1:
        raise ValueError(f"{who}: log_weights holds no group")
    off = None
    if offset is not None:
        off = offset.detach().reshape(9).to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty(G, m, dtype=torch.float32, device=dev)
    arg = torch.empty(G, m, dtype=torch.int32, device=dev) if with_arg else None
    count = torch.empty(m, dtype=torch.int32, device=dev) if return_count else None
    m_tile = max(4, int(LOCAL_QUERY_TILE) // 4 * 4)
    g_tile = max(1, min(int(LOCAL_GROUP_TILE), MAX_GROUPS))
    for g0 in range(0, G, g_tile):
        g1 = min(G, g0 + g_tile)
        for i0 in range(0, m, m_tile):
            i1 = min(m, i0 + m_tile)
            part = out[g0:g1, i0:i1]
            whole = part.is_contiguous()
            dst = part if whole else torch.empty(g1 - g0, i1 - i0, dtype=torch.float32, device=dev)
            all_rows = Qr is Gr and i0 == 0 and i1 == m                      # a null pointer stands for the grid rows
            tile = None if all_rows else _aligned(Qr[i0:i1])
            common = dict(level=level, offset=None if off is None else off.data_ptr(), grid=Gr.data_ptr(),
                          queries=None if all_rows else tile.data_ptr(), log_weights=lw[g0:g1].data_ptr() if lw is not None else None,
                          m=i1 - i0, G=g1 - g0, d2_cut=cut, out=dst.data_ptr(),
                          count=count[i0:i1].data_ptr() if return_count and g0 == 0 else None)
            if K is None:
                common["kappa"] = k
            else:
                common["concentration"] = (C.c_double * 9)(*[float(x) for x in K.reshape(9)])
            adst = None
            if with_arg:
                adst = arg[g0:g1, i0:i1] if whole else torch.empty(g1 - g0, i1 - i0, dtype=torch.int32, device=dev)
            if K is not None:
                _lib.call("so3_grid_local_fisher", _lib.So3GridLocalFisher(arg=adst.data_ptr() if with_arg else None, **common), dev)
            elif with_arg:
                _lib.call("so3_grid_local_max", _lib.So3GridLocalMax(arg=adst.data_ptr(), **common), dev)
            else:
                _lib.call("so3_grid_local_sum", _lib.So3GridLocalSum(**common), dev)
            if with_arg and not whole:
                arg[g0:g1, i0:i1].copy_(adst)
            if not whole:
                part.copy_(dst)
    out = out if grouped else out[0]
    if with_arg:
        arg = arg.to(torch.int64)
        return (out, arg if grouped else arg[0]) + ((count,) if return_count else ())
    return (out, count) if return_count else out


MOMENT_BYTES = 92                                 # workspace bytes per (group, chunk, query) of rnf_so3_kernel_moments: 11 fp64 sums, one fp32 max


def so3_kernel_moments(centres, queries, kappa, log_weights=None, project: bool = False, group_queries: bool = False,
                       workspace_cap: int = None) -> dict:
    """The responsibility-weighted first moments of the kernel sum on the device (``rnf_so3_kernel_moments``): with
    r_ij = w_j k(C_j, Q_i) / sum_l w_l k(C_l, Q_i) for ONE ``kappa`` in 0..1e6,
    ``log_density`` [m] (the bits of ``so3_kernel_log_density``), ``mean`` [m,3,3] = M_i = sum_j r_ij C_j, ``msd`` [m] = D_i =
    sum_j r_ij |Q_i - C_j|_F^2, ``dlogp_dkappa`` [m] float64 = -D_i / 2 - l'(kappa), and with ``project`` ``rotation`` [m,3,3] =
    polar(M_i) -- the mean-shift step; NaN where det M_i <= 0, where there is no mean direction -- and ``step`` [m] = |rotation - Q_i|_F.
    d log p(Q_i) / dQ_i = kappa (M_i - Q_i).  ``centres`` [n,3,3]; ``queries`` [m,3,3], shared by the groups, or with ``group_queries``
    [G,m,3,3], one set per group; ``log_weights`` None, [n] or [G,n] as ``so3_kernel_log_density``: a 2-D ``log_weights`` (or
    ``group_queries``) gives every output a leading G.  Edge cases as ``so3_kernel_log_density``, for every output of the (group, query).
    A query's outputs are bit-identical however the call is tiled, so the tiling of queries and groups that keeps the workspace (92
    ceil(n/4096) bytes per group and query) under ``workspace_cap`` (64 MiB) is invisible.  Stream-ordered, no host synchronisation, no
    gradient (``SO3KernelDensity.log_prob`` carries one)."""
    who = "so3_kernel_moments"
    ks, scalar = _kappas(kappa, who)
    if not scalar:
        raise ValueError(f"{who}: kappa is one concentration, not a sequence")
    k = ks[0]
    Cn = _rotations(centres, "centres", who)
    n, dev = Cn.shape[0], Cn.device
    if not 1 <= n <= MAX_CENTRES:
        raise ValueError(f"{who}: centres holds {n} rotations (1 to 2^24)")
    group_queries = bool(group_queries)
    if group_queries:
        if not isinstance(queries, torch.Tensor) or queries.dim() != 4 or tuple(queries.shape[-2:]) != (3, 3):
            raise ValueError(f"{who}: queries {tuple(getattr(queries, 'shape', ()))}, expected [G,m,3,3] with group_queries")
        if not queries.is_cuda:
            raise ValueError(f"{who}: queries is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        Qr = queries.detach().to(torch.float32).contiguous()
    else:
        Qr = _rotations(queries, "queries", who)
    if Qr.device != dev:
        raise ValueError(f"{who}: queries on {Qr.device}, centres on {dev}")
    m = Qr.shape[-3]
    if m >= 1 << 31:
        raise ValueError(f"{who}: queries holds {m} rotations (below 2^31)")
    lw, grouped = None, group_queries
    if log_weights is not None:
        if not isinstance(log_weights, torch.Tensor) or log_weights.dim() not in (1, 2) or log_weights.shape[-1] != n:
            raise ValueError(f"{who}: log_weights {tuple(getattr(log_weights, 'shape', ()))} for {n} centres, expected [n] or [G,n]")
        if not log_weights.is_cuda:
            raise ValueError(f"{who}: log_weights is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        grouped = grouped or log_weights.dim() == 2
        lw = log_weights.detach().to(device=dev, dtype=torch.float32).reshape(-1, n).contiguous()
    G = Qr.shape[0] if group_queries else (lw.shape[0] if lw is not None else 1)
    if lw is not None and lw.shape[0] != G:
        raise ValueError(f"{who}: log_weights holds {lw.shape[0]} groups, queries {G}")
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"{who}: {G} groups (1 to 65535)")
    cap = WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    names = ("log_density", "mean", "msd") + (("rotation", "step") if project else ())
    out = {name: torch.empty((G, m, 3, 3) if name in ("mean", "rotation") else (G, m), dtype=torch.float32, device=dev) for name in names}
    dl = C.c_double(0.0)
    if m == 0:
        _lib.call("so3_kernel_moments", _lib.So3KernelMoments(n=n, m=0, G=G, kappa=k, dlog_normaliser=C.addressof(dl)), dev)
    else:
        per_query = MOMENT_BYTES * ((n + CHUNK - 1) // CHUNK)             # bytes per query and group
        g_tile = max(1, min(G, cap // (per_query * min(m, 256))))
        m_tile = max(1, min(m, cap // (per_query * g_tile)))
        m_tile = m_tile if m_tile < 4 or m_tile == m else m_tile // 4 * 4          # rows of 36 bytes: every fourth is 16-byte aligned
        for g0 in range(0, G, g_tile):
            g1 = min(G, g0 + g_tile)
            for i0 in range(0, m, m_tile):
                i1 = min(m, i0 + m_tile)
                tile = _aligned(Qr[g0:g1, i0:i1].contiguous() if group_queries else Qr[i0:i1])
                part = {name: v[g0:g1, i0:i1] for name, v in out.items()}
                dst = {name: v if v.is_contiguous() else torch.empty(v.shape, dtype=torch.float32, device=dev) for name, v in part.items()}
                args = _lib.So3KernelMoments(centres=Cn.data_ptr(), queries=tile.data_ptr(),
                                             log_weights=lw[g0:g1].data_ptr() if lw is not None else None, n=n, m=i1 - i0, G=g1 - g0,
                                             group_queries=int(group_queries), kappa=k, dlog_normaliser=C.addressof(dl),
                                             **{name: v.data_ptr() for name, v in dst.items()})
                _lib.call("so3_kernel_moments", args, dev)
                for name, v in part.items():
                    if dst[name] is not v:
                        v.copy_(dst[name])
    out["dlogp_dkappa"] = -0.5 * out["msd"].to(torch.float64) - dl.value
    return out if grouped else {name: v[0] for name, v in out.items()}


class _KernelLogProb(torch.autograd.Function):
    """log p(R) of an ``SO3KernelDensity`` with its gradient kappa (M - R) with respect to R, both from ONE moments call"""

    @staticmethod
    def forward(ctx, R, est):
        kappa = float(est.kappa)
        flat = R.detach().reshape(-1, 3, 3)
        out = so3_kernel_moments(est.rotations, flat, kappa, est.log_weights)
        ctx.save_for_backward(kappa * (out["mean"].to(torch.float64) - flat.to(device=out["mean"].device, dtype=torch.float64)))
        return out["log_density"].reshape(R.shape[:-2])

    @staticmethod
    def backward(ctx, grad):
        (dR,) = ctx.saved_tensors
        g = grad.reshape(-1, 1, 1).to(torch.float64) * dR
        return g.reshape(grad.shape + (3, 3)).to(torch.float32), None


def _mean_shift(centres, starts, kappa, log_weights, group_queries, tol, max_steps, check_every, workspace_cap=None):
    """Mean shift of ``starts`` ([s,3,3], or [G,s,3,3] with ``group_queries``) on the kernel estimate -> (rotations, converged,
    steps_taken) of the starts' shape.  One host read-back per ``check_every`` steps."""
    cur = starts.detach().to(torch.float32).clone()
    frozen = torch.zeros(cur.shape[:-2], dtype=torch.bool, device=cur.device)
    taken = torch.zeros(cur.shape[:-2], dtype=torch.int32, device=cur.device)
    for it in range(int(max_steps)):
        out = so3_kernel_moments(centres, cur, kappa, log_weights, project=True, group_queries=group_queries, workspace_cap=workspace_cap)
        step = out["step"].reshape(frozen.shape)
        frozen = frozen | (step < tol)                                   # frozen now or before: written back unchanged from here on
        cur = torch.where(frozen[..., None, None], cur, out["rotation"].reshape(cur.shape))
        taken = taken + (~frozen).to(torch.int32)
        if (it + 1) % int(check_every) == 0 and bool((frozen | torch.isnan(step)).all()):
            break
    return cur, frozen, taken


class SO3KernelDensity(torch.nn.Module):
    """A kernel density estimate on SO(3): p(R) = sum_j w_j MF(kappa R_j)(R) with buffers ``rotations`` [n,3,3], ``log_weights`` [n]
    (log w up to a constant; zeros for uniform weights) and ``kappa`` (a 0-d float64 tensor).  ``fit`` chooses kappa from the data.
    The three buffers are the whole state: ``log_prob`` always weights by ``log_weights`` (zeros give the bits of the unweighted sum), so
    a ``load_state_dict`` changes nothing but the numbers.  ``kappa`` is created on the CPU because the library takes its bandwidths
    from the host; after ``.to(device)`` it follows the module and every ``log_prob`` reads it back (one host synchronisation).
    ``log_prob`` is differentiable with respect to its rotations (not to the buffers); ``score``, ``mean_shift``, ``modes`` and ``sample``
    rest on the same moments pass (``so3_kernel_moments``)."""

    def __init__(self, rotations, kappa, log_weights=None):
        super().__init__()
        who = "SO3KernelDensity"
        R = _rotations(rotations, "rotations", who)
        (k,), _ = _kappas(float(kappa), who)
        if log_weights is None:
            lw = torch.zeros(R.shape[0], dtype=torch.float32, device=R.device)
        else:
            if not isinstance(log_weights, torch.Tensor) or tuple(log_weights.shape) != (R.shape[0],):
                raise ValueError(f"{who}: log_weights {tuple(getattr(log_weights, 'shape', ()))} for {R.shape[0]} rotations, expected [n]")
            if not log_weights.is_cuda:
                raise ValueError(f"{who}: log_weights is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
            lw = log_weights.detach().to(device=R.device, dtype=torch.float32).contiguous()
        self.register_buffer("rotations", R)
        self.register_buffer("log_weights", lw)
        self.register_buffer("kappa", torch.tensor(k, dtype=torch.float64))
        self.kappas = None                          # set by fit: the candidates and their scores
        self.loo_log_likelihood = None

    @classmethod
    def fit(cls, rotations, log_weights=None, kappas=None, workspace_cap: int = None):
        """The estimate on ``rotations`` [n,3,3] (weights softmax(``log_weights``) [n], or uniform) with the candidate of ``kappas`` that
        maximises the weighted mean leave-one-out log-likelihood sum_i w_i log p_{-i}(R_i) (rows of weight 0 do not count).  The default
        candidates are 2^(k/2), k = 4..28.  The result carries ``kappas`` (float64 [J], on the CPU), ``loo_log_likelihood`` (float64
        [J], on the device) and ``kappa``.  One host synchronisation, to read the winner; a warning if it is at either end of the list.
        ``workspace_cap``: as ``so3_kernel_log_density`` (leave-one-out of more than about 1.5e5 rotations needs more than its 64 MiB)."""
        who = "SO3KernelDensity.fit"
        ks, _ = _kappas(list(DEFAULT_KAPPAS if kappas is None else kappas), who)
        self = cls(rotations, ks[0], log_weights)
        lw = self.log_weights
        loo = so3_kernel_log_density(self.rotations, None, ks, lw, leave_one_out=True, workspace_cap=workspace_cap).to(torch.float64)   # [J,n]
        w = torch.softmax(lw.to(torch.float64), dim=0)
        score = torch.where(w > 0, w * loo, torch.zeros_like(loo)).sum(dim=1)
        best = int(torch.argmax(torch.where(torch.isnan(score), torch.full_like(score, -math.inf), score)))
        if len(ks) > 1 and best in (0, len(ks) - 1):
            warnings.warn(f"{who}: the best kappa {ks[best]:g} is at the end of the candidate list ({ks[0]:g} .. {ks[-1]:g}); widen it",
                          stacklevel=2)
        self.kappa.fill_(ks[best])
        self.kappas = torch.tensor(ks, dtype=torch.float64)
        self.loo_log_likelihood = score
        return self

    def _queries(self, R, who: str):
        if not isinstance(R, torch.Tensor) or R.dim() < 2 or tuple(R.shape[-2:]) != (3, 3):
            raise ValueError(f"SO3KernelDensity.{who}: R {tuple(getattr(R, 'shape', ()))}, expected [...,3,3]")
        if not self.rotations.is_cuda:
            raise ValueError(f"SO3KernelDensity.{who}: rotations is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        return R.shape[:-2]

    def log_prob(self, R):
        """log p(R) w.r.t. the Haar probability measure for R [...,3,3] on the device -> float32 [...].  Where ``R`` requires a gradient
        the result carries d log p / dR = kappa (M - R), the Euclidean gradient with respect to the nine entries (M: the
        responsibility-weighted mean of the estimate's rotations, ``so3_kernel_moments``), from the same pass as the value; the value has
        the same bits either way.  No gradient with respect to the buffers."""
        lead = self._queries(R, "log_prob")
        if R.requires_grad and torch.is_grad_enabled():
            if not R.is_cuda:
                raise ValueError("SO3KernelDensity.log_prob: R is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
            return _KernelLogProb.apply(R, self)
        out = so3_kernel_log_density(self.rotations, R.reshape(-1, 3, 3), float(self.kappa), self.log_weights)
        return out.reshape(lead)

    def score(self, R, frame: str = "body"):
        """The gradient of log p at R [...,3,3].  ``frame="ambient"``: kappa (M - R) [...,3,3], the Euclidean gradient of ``log_prob``.
        ``frame="body"``: kappa vee(R^T M - M^T R) [...,3], the derivative along R exp(hat(v)) at v = 0 (vee(A) = (A21, A02, A10)); R^T R
        drops out of it.  float32, detached."""
        if frame not in ("body", "ambient"):
            raise ValueError(f"SO3KernelDensity.score: frame={frame!r}, expected 'body' or 'ambient'")
        lead = self._queries(R, "score")
        flat = R.detach().reshape(-1, 3, 3)
        kappa = float(self.kappa)
        M = so3_kernel_moments(self.rotations, flat, kappa, self.log_weights)["mean"].to(torch.float64)
        Rd = flat.to(device=M.device, dtype=torch.float64)
        D = kappa * (M - Rd)
        if frame == "ambient":
            return D.to(torch.float32).reshape(lead + (3, 3))
        A = Rd.transpose(1, 2) @ D
        A = A - A.transpose(1, 2)
        return torch.stack([A[:, 2, 1], A[:, 0, 2], A[:, 1, 0]], dim=1).to(torch.float32).reshape(lead + (3,))

    def mean_shift(self, starts, kappa: float = None, tol: float = 1e-5, max_steps: int = 200, check_every: int = 8):
        """Mean shift of ``starts`` [s,3,3] to modes of the estimate: R <- polar(M(R)), the rotation closest to the responsibility-weighted
        mean, a host loop of ``so3_kernel_moments`` calls with one host read-back per ``check_every`` steps.  ``kappa``: the kernel of the
        search (default: the estimate's; see ``modes``).  A start whose step |polar(M) - R|_F falls below ``tol`` is frozen -- written back
        unchanged from then on -- so its endpoint does not depend on how long the others take, and is bit-identical whatever other starts
        share the call.  A start that meets det M <= 0 ends as NaN.
        -> (rotations [s,3,3], log_density [s] at the endpoints under ``kappa``, converged [s] bool, steps_taken [s] int32)"""
        who = "SO3KernelDensity.mean_shift"
        S = _rotations(starts, "starts", who)
        if not self.rotations.is_cuda:
            raise ValueError(f"{who}: rotations is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        if not (tol > 0 and int(max_steps) >= 1 and int(check_every) >= 1):
            raise ValueError(f"{who}: tol={tol}, max_steps={max_steps}, check_every={check_every}")
        k = float(self.kappa) if kappa is None else _kappas(float(kappa), who)[0][0]
        rot, converged, taken = _mean_shift(self.rotations, S, k, self.log_weights, False, float(tol), max_steps, check_every)
        return rot, so3_kernel_log_density(self.rotations, rot, k, self.log_weights), converged, taken

    def modes(self, top_k: int = 4, separation_deg: float = 15.0, starts=None, kappa: float = None, tol: float = 1e-5, max_steps: int = 200,
              check_every: int = 8) -> dict:
        """The ``top_k`` modes of the estimate at no fixed resolution: mean shift (``mean_shift``) from ``starts``, then the endpoints are
        merged as ``grid_pose.grid_modes`` merges grid rows -- mode 0 the endpoint of the largest log-density, mode j the largest among
        those at least ``separation_deg`` from the earlier modes.  ``starts``: None (up to 1024 of the estimate's own rotations at a fixed
        stride), an int (that many) or a tensor [s,3,3].  Each mode's ``mass`` is the weight share of the starts whose endpoint lies
        within ``separation_deg`` of it and of no earlier mode (the estimate's weights for its own rotations, equal weights for given
        starts; endpoints that are not finite count for no mode).
        ``kappa`` is the kernel of the search, by default the estimate's.  Mode seeking wants a smoother kernel than density estimation:
        on 4096 draws of 1/2 MF(20 I) + 1/2 MF(20 Rz(180)) the likelihood-optimal bandwidth that ``fit`` picks (kappa = 128) yields 4 to
        10 spurious modes, kappa = 32 exactly two.
        -> dict(est [k,3,3], log_prob [k], mass [k], converged_fraction); modes that do not exist are NaN with mass 0."""
        from ..grid_pose import grid_modes
        who = "SO3KernelDensity.modes"
        if not 1 <= int(top_k) <= 16:
            raise ValueError(f"{who}: top_k={top_k} outside 1..16")
        if not 0.0 < float(separation_deg) <= 180.0:
            raise ValueError(f"{who}: separation_deg={separation_deg} outside (0, 180]")
        n = self.rotations.shape[0]
        if starts is None or isinstance(starts, int):
            want = 1024 if starts is None else int(starts)
            if want < 1:
                raise ValueError(f"{who}: starts={starts}")
            stride = max(1, -(-n // want))
            pick = torch.arange(0, n, stride, device=self.rotations.device)
            S = self.rotations[pick]
            w = torch.softmax(self.log_weights[pick].to(torch.float64), dim=0)
        else:
            S = _rotations(starts, "starts", who)
            w = torch.full((S.shape[0],), 1.0 / max(1, S.shape[0]), dtype=torch.float64, device=S.device)
        sep = math.radians(float(separation_deg))
        rot, lp, converged, _ = self.mean_shift(S, kappa, tol, max_steps, check_every)
        ok = torch.isfinite(rot).all(dim=2).all(dim=1) & torch.isfinite(lp)
        clean = torch.where(ok[:, None, None], rot, torch.eye(3, device=rot.device).expand_as(rot)).contiguous()
        index, log_prob, _, _, _ = grid_modes(torch.where(ok, lp, torch.full_like(lp, -math.inf))[None], clean, int(top_k), sep)
        index, log_prob = index[0], log_prob[0]
        est = clean[index.clamp(min=0)].clone()
        est[index < 0] = float("nan")
        # within sep: tr(E_k^T R_s) > 1 + 2 cos(sep), the rule of rnf_grid_modes; a start counts for the first mode it is within sep of
        tr = torch.einsum("kij,sij->ks", torch.nan_to_num(est).to(torch.float64), clean.to(torch.float64))
        near = (tr > 1.0 + 2.0 * math.cos(sep)) & (index >= 0)[:, None] & ok[None, :]
        first = near & (torch.cumsum(near.to(torch.int32), dim=0) == 1)
        mass = (first.to(torch.float64) * w[None, :]).sum(dim=1).to(torch.float32)
        log_prob = torch.where(index >= 0, log_prob, torch.full_like(log_prob, float("nan")))
        return dict(est=est, log_prob=log_prob, mass=mass, converged_fraction=float(converged.to(torch.float64).mean()))

    def sample(self, n: int):
        """``n`` rotations [n,3,3] from the estimate: a centre j drawn with probability softmax(log_weights)_j (``torch.multinomial``),
        times a draw of MF(kappa I) from the device sampler (``MatrixFisherN``), whose Philox key comes from torch's default generator:
        ``torch.manual_seed`` reproduces the samples."""
        from .fisher import MatrixFisherN
        if not self.rotations.is_cuda:
            raise ValueError("SO3KernelDensity.sample: rotations is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        n = int(n)
        if n < 1:
            raise ValueError(f"SO3KernelDensity.sample: n={n}")
        dev = self.rotations.device
        pick = torch.multinomial(torch.softmax(self.log_weights.to(torch.float64), dim=0).to(torch.float32), n, replacement=True)
        noise = MatrixFisherN(float(self.kappa) * torch.eye(3, dtype=torch.float32, device=dev)[None])._sample(n)[0]
        return self.rotations[pick] @ noise
