"""Kernel density estimates on SO(3) with an isotropic matrix-Fisher kernel, from one pairwise HIP kernel sum (``rnf_so3_kernel_sum``,
csrc/so3_kernel_sum.h).  Densities are w.r.t. the Haar probability measure, like every density in the package.

``so3_kernel_log_density`` is the primitive: log sum_j w_j k_kappa(C_j, Q_i) for sets of centres and queries, several bandwidths and
several rows of log-weights at once, with leave-one-out.  ``SO3KernelDensity`` is the estimate with its bandwidth chosen by the
leave-one-out likelihood.  ``grid_pose.grid_diffuse`` builds the prediction step of a Bayes filter on the SO(3) grid on the primitive."""
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


class SO3KernelDensity(torch.nn.Module):
    """A kernel density estimate on SO(3): p(R) = sum_j w_j MF(kappa R_j)(R) with buffers ``rotations`` [n,3,3], ``log_weights`` [n]
    (log w up to a constant; zeros for uniform weights) and ``kappa`` (a 0-d float64 tensor).  ``fit`` chooses kappa from the data.
    The three buffers are the whole state: ``log_prob`` always weights by ``log_weights`` (zeros give the bits of the unweighted sum), so
    a ``load_state_dict`` changes nothing but the numbers.  ``kappa`` is created on the CPU because the library takes its bandwidths
    from the host; after ``.to(device)`` it follows the module and every ``log_prob`` reads it back (one host synchronisation).
    There is no gradient (``log_prob`` is not differentiable) and no ``sample()``."""

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

    def log_prob(self, R):
        """log p(R) w.r.t. the Haar probability measure for R [...,3,3] on the device -> float32 [...]; no gradient."""
        if not isinstance(R, torch.Tensor) or R.dim() < 2 or tuple(R.shape[-2:]) != (3, 3):
            raise ValueError(f"SO3KernelDensity.log_prob: R {tuple(getattr(R, 'shape', ()))}, expected [...,3,3]")
        lead = R.shape[:-2]
        if not self.rotations.is_cuda:
            raise ValueError("SO3KernelDensity.log_prob: rotations is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        out = so3_kernel_log_density(self.rotations, R.reshape(-1, 3, 3), float(self.kappa), self.log_weights)
        return out.reshape(lead)
