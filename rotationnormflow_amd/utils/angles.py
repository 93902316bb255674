"""Error distributions on SO(3): the distribution function of the geodesic angle from query rotations to a weighted set of rotations,
F_i(theta) = sum_j w_j [angle(C_j, Q_i) <= theta], from one pairwise HIP pass (``rnf_so3_angle_cdf``, csrc/so3_angle_cdf.h).

``so3_angle_cdf`` is the primitive: the mass of balls about the queries, and the mean and root-mean-square angle.
``so3_angle_quantile`` inverts it: the radius at which a ball about a query reaches a given mass.  ``grid_pose.grid_error`` and
``grid_pose.grid_ball_estimate`` put a grid posterior's predicted Acc@theta, expected error, error radii and the Acc@theta-optimal
estimate on them."""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _lib
from .kde import CHUNK, MAX_CENTRES, MAX_GROUPS, WORKSPACE_CAP, _aligned, _rotations

MAX_THRESHOLDS = 8                                  # T of one launch (include/rnf_hip.h)
SLOT_BYTES = 8                                      # workspace bytes per (group, chunk, query, slot) of rnf_so3_angle_cdf: one fp64 sum


def _inputs(centres, queries, log_weights, group_queries, who: str):
    """The checks shared by the entry points -> (centres [n,3,3], queries [m,3,3] or [G,m,3,3], log-weights [G,n] or None, G, whether
    the outputs carry a leading G)"""
    Cn = _rotations(centres, "centres", who)
    n, dev = Cn.shape[0], Cn.device
    if not 1 <= n <= MAX_CENTRES:
        raise ValueError(f"{who}: centres holds {n} rotations (1 to 2^24)")
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
    if Qr.shape[-3] >= 1 << 31:
        raise ValueError(f"{who}: queries holds {Qr.shape[-3]} rotations (below 2^31)")
    lw, grouped = None, bool(group_queries)
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
    return Cn, Qr, lw, G, grouped


def _angle_cdf(who, one, many, Cn, Qr, lw, G, grouped, K, thresholds, query_tau, group_queries, moments, workspace_cap):
    """``so3_angle_cdf`` (``K`` None: the rows of ``Qr`` are queries) and ``so3_set_angle_cdf`` (sets of ``K`` members) after their input
    checks: the thresholds, the outputs, the tiling under ``workspace_cap`` and the copy-back.  ``who`` names the public function and the
    library's entry, ``one`` and ``many`` a row of ``Qr`` in the messages."""
    struct, members = (_lib.So3AngleCdf, {}) if K is None else (_lib.So3SetAngleCdf, {"K": K})
    n, dev, m = Cn.shape[0], Cn.device, Qr.shape[-3 if K is None else -4]
    if thresholds is not None and query_tau is not None:
        raise ValueError(f"{who}: both thresholds and query_tau are given; pass one of the two")
    th, tau, T = None, None, 0
    if thresholds is not None:
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.detach().cpu().reshape(-1).tolist()
        th = [float(thresholds)] if not isinstance(thresholds, (list, tuple)) else [float(t) for t in thresholds]
        T = len(th)
        for t in th:
            if not (math.isfinite(t) and 0.0 <= t <= math.pi):
                raise ValueError(f"{who}: threshold {t} outside 0..pi radians")
    elif query_tau is not None:
        want = "[G,T,m]" if grouped else "[T,m]"
        if not isinstance(query_tau, torch.Tensor) or query_tau.dim() != (3 if grouped else 2) or query_tau.shape[-1] != m or (
                grouped and query_tau.shape[0] != G):
            raise ValueError(f"{who}: query_tau {tuple(getattr(query_tau, 'shape', ()))} for {G} groups of {m} {many}, expected {want}")
        if not query_tau.is_cuda:
            raise ValueError(f"{who}: query_tau is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        tau = query_tau.detach().to(device=dev, dtype=torch.float32).reshape(G, -1, m).contiguous()
        T = tau.shape[1]
    if T > MAX_THRESHOLDS or (T == 0 and (th is not None or tau is not None)):
        raise ValueError(f"{who}: {T} thresholds (1 to {MAX_THRESHOLDS})")
    if T == 0 and not moments:
        raise ValueError(f"{who}: no thresholds, no query_tau and no moments: nothing to compute")
    cap = WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    out = {"mass": torch.empty(G, T, m, dtype=torch.float32, device=dev)}
    if moments:
        out["mean_angle"] = torch.empty(G, m, dtype=torch.float32, device=dev)
        out["mean_sq_angle"] = torch.empty(G, m, dtype=torch.float32, device=dev)
    per_row = SLOT_BYTES * (T + (2 if moments else 0)) * ((n + CHUNK - 1) // CHUNK)        # bytes per query (set) and group
    if per_row > cap:
        raise ValueError(f"{who}: one {one}'s partial sums take {per_row} bytes, above workspace_cap={cap}; pass a larger workspace_cap")
    host = (C.c_double * T)(*th) if th is not None else None
    if m > 0:
        g_tile = max(1, min(G, cap // (per_row * min(m, 256))))
        m_tile = max(1, min(m, cap // (per_row * g_tile)))
        m_tile = m_tile if m_tile < 4 or m_tile == m else m_tile // 4 * 4          # rows of 36 (K) bytes: every fourth is 16-byte aligned
        for g0 in range(0, G, g_tile):
            g1 = min(G, g0 + g_tile)
            for i0 in range(0, m, m_tile):
                i1 = min(m, i0 + m_tile)
                tile = _aligned(Qr[g0:g1, i0:i1].contiguous() if group_queries else Qr[i0:i1])
                part = {name: v[g0:g1, ..., i0:i1] for name, v in out.items() if name != "mass" or T > 0}
                dst = {name: v if v.is_contiguous() else torch.empty(v.shape, dtype=torch.float32, device=dev) for name, v in part.items()}
                tau_tile = tau[g0:g1, :, i0:i1].contiguous() if tau is not None else None
                args = struct(centres=Cn.data_ptr(), queries=tile.data_ptr(), log_weights=lw[g0:g1].data_ptr() if lw is not None else None,
                              n=n, m=i1 - i0, G=g1 - g0, group_queries=int(bool(group_queries)), T=T,
                              thresholds=C.cast(host, C.c_void_p) if host is not None else None,
                              query_tau=tau_tile.data_ptr() if tau_tile is not None else None, **members,
                              **{name: v.data_ptr() for name, v in dst.items()})
                _lib.call(who, args, dev)
                for name, v in part.items():
                    if dst[name] is not v:
                        v.copy_(dst[name])
    if moments:
        out["rms_angle"] = torch.sqrt(out["mean_sq_angle"])
    return out if grouped else {name: v[0] for name, v in out.items()}


def so3_angle_cdf(centres, queries, thresholds=None, query_tau=None, log_weights=None, group_queries: bool = False, moments: bool = True,
                  workspace_cap: int = None) -> dict:
    """The distribution function of the geodesic angle on the device (``rnf_so3_angle_cdf``): with w = softmax(``log_weights``) (uniform
    without), d2_ij = |Q_i - C_j|_F^2 = 8 sin^2(theta_ij / 2) and theta_ij the angle between centre j and query i,
    ``mass`` [T,m] = sum_j w_j [d2_ij <= tau_t], the mass of the ball of each threshold about each query, and with ``moments``
    ``mean_angle`` [m] = sum_j w_j theta_ij, ``mean_sq_angle`` [m] = sum_j w_j theta_ij^2 and ``rms_angle`` [m], its root, in radians.
    ``centres`` [n,3,3]; ``queries`` [m,3,3], shared by the groups, or with ``group_queries`` [G,m,3,3], one set per group;
    ``log_weights`` None, [n] or [G,n]: a 2-D ``log_weights`` (or ``group_queries``) gives every output a leading G.
    The thresholds come in one of two forms: ``thresholds``, up to 8 angles in radians in [0, pi] shared by all queries (a float or a
    sequence; each becomes tau = 8 sin^2(theta / 2), pi and beyond nothing: everything counts), or ``query_tau`` [T,m] ([G,T,m] where the
    outputs carry a G), squared chordal distances on the device, one set per query.  Neither: ``mass`` is empty ([0,m]).
    A centre with log-weight -inf is left out; another non-finite centre or a NaN log-weight makes its group NaN, a non-finite query its
    outputs, a NaN ``query_tau`` entry its own mass; tau < 0 gives 0.  A query's outputs are bit-identical however the call is tiled,
    so the tiling of queries (in multiples of 4 rows) and groups that keeps the partial sums (8 (T + 2) ceil(n/4096) bytes per group
    and query; the weights' 4 n + 16 ceil(n/4096) + 8 bytes per group come on top) under ``workspace_cap`` (64 MiB) is invisible; a cap
    below one query's partial sums raises ValueError.  Stream-ordered, no host synchronisation, no gradient."""
    who = "so3_angle_cdf"
    Cn, Qr, lw, G, grouped = _inputs(centres, queries, log_weights, bool(group_queries), who)
    return _angle_cdf(who, "query", "queries", Cn, Qr, lw, G, grouped, None, thresholds, query_tau, group_queries, moments, workspace_cap)


def _tau(theta):
    """8 sin^2(theta / 2) of fp64 angles, rounded once to fp32"""
    s = torch.sin(0.5 * theta)
    return (8.0 * s * s).to(torch.float32)


def _quantile_search(cdf, G, m, lv, passes, dev):
    """The bracket search of ``so3_angle_quantile``: ``cdf(thresholds=..)`` / ``cdf(query_tau=[G,T,L*m])`` -> float64 masses [G,T,L*m] of
    the m queries repeated once per level (level-major), so that one call per pass serves every level.  torch operations only, on
    ``dev`` -> dict of [G,L,m]"""
    L = len(lv)
    alpha = torch.tensor(lv, dtype=torch.float64, device=dev).repeat_interleave(m)[None]      # [1,L*m]
    f0 = cdf(thresholds=0.0)[:, 0]                                        # [G,L*m]: the mass at the query itself
    parts = torch.arange(1, 9, dtype=torch.float64, device=dev).reshape(1, 8, 1) / 9.0
    lo = torch.zeros(G, L * m, dtype=torch.float64, device=dev)
    hi = torch.full((G, L * m), math.pi, dtype=torch.float64, device=dev)
    f_lo, f_hi = f0.clone(), torch.ones(G, L * m, dtype=torch.float64, device=dev)
    for _ in range(passes):
        theta = lo[:, None, :] + (hi - lo)[:, None, :] * parts           # [G,8,L*m], increasing
        f = cdf(query_tau=_tau(theta))
        reach = f >= alpha[:, None]                                       # monotone in the slot: once reached, reached
        k = 8 - reach.sum(dim=1)                                          # the first slot that reaches alpha; 8: none does
        th9 = torch.cat([lo[:, None], theta, hi[:, None]], dim=1)         # [G,10,L*m]
        f9 = torch.cat([f_lo[:, None], f, f_hi[:, None]], dim=1)
        lo, hi = th9.gather(1, k[:, None])[:, 0], th9.gather(1, k[:, None] + 1)[:, 0]
        f_lo, f_hi = f9.gather(1, k[:, None])[:, 0], f9.gather(1, k[:, None] + 1)[:, 0]
    at0 = f0 >= alpha
    nan = torch.isnan(f0)
    zero = torch.zeros_like(lo)
    lo, hi = torch.where(at0, zero, lo), torch.where(at0, zero, hi)
    f_lo, f_hi = torch.where(at0, f0, f_lo), torch.where(at0 | nan, f0, f_hi)
    bad = torch.full_like(lo, float("nan"))
    lo, hi = torch.where(nan, bad, lo), torch.where(nan, bad, hi)
    res = dict(radius=hi, lo=lo, mass_lo=f_lo.to(torch.float32), mass_hi=f_hi.to(torch.float32))
    return {key: v.reshape(G, L, m) for key, v in res.items()}


def _angle_quantile(who, cdf_fn, rows, Cn, Qr, lw, G, grouped, levels, group_queries, tol, workspace_cap):
    """``so3_angle_quantile`` and ``so3_set_angle_quantile`` after their input checks: the levels, ``tol`` and the bracket search on
    ``cdf_fn`` (``so3_angle_cdf`` or ``so3_set_angle_cdf``); ``rows``: the axis of ``Qr`` that counts the queries (sets)"""
    if isinstance(levels, torch.Tensor):
        levels = levels.detach().cpu().reshape(-1).tolist()
    lv = [float(levels)] if not isinstance(levels, (list, tuple)) else [float(a) for a in levels]
    if not lv:
        raise ValueError(f"{who}: levels is empty")
    for a in lv:
        if not 0.0 < a < 1.0:
            raise ValueError(f"{who}: level {a} outside (0, 1)")
    if not (math.isfinite(float(tol)) and 0.0 < float(tol) <= math.pi):
        raise ValueError(f"{who}: tol={tol} outside (0, pi] radians")
    dev, m = Cn.device, Qr.shape[rows]
    passes = max(1, math.ceil(math.log(math.pi / float(tol)) / math.log(9.0) - 1e-12))
    kw = dict(log_weights=lw, group_queries=group_queries, moments=False, workspace_cap=workspace_cap)
    lead = lw is not None or group_queries                                # lw is [G,n] here: the calls below carry a G whenever it is given
    Qrep = torch.cat([Qr] * len(lv), dim=rows) if len(lv) > 1 else Qr     # level-major: one call per pass serves every level

    def cdf(thresholds=None, query_tau=None):
        if query_tau is not None and not lead:
            query_tau = query_tau[0]
        out = cdf_fn(Cn, Qrep, thresholds, query_tau, **kw)["mass"].to(torch.float64)
        return out if lead else out[None]                                 # [G,T,L*m]

    out = _quantile_search(cdf, G, m, lv, passes, dev)                    # [G,L,m]
    return out if grouped else {key: v[0] for key, v in out.items()}


def so3_angle_quantile(centres, queries, levels, log_weights=None, group_queries: bool = False, tol: float = 1e-3,
                       workspace_cap: int = None) -> dict:
    """The error radii of the queries: for each level alpha in (0, 1) the angle at which the ball about query i reaches mass alpha
    under w = softmax(``log_weights``) -- the alpha-quantile of the angle to the weighted ``centres``; level 0.5 is the median error.
    Inputs as ``so3_angle_cdf``; ``levels`` a float or a sequence of L.  The search keeps a bracket lo < hi with F(lo) < alpha <= F(hi)
    per (level, query), starting from [0, pi] with pi taken to satisfy every level, and splits it into 9 equal parts in angle per pass
    (8 interior thresholds as ``query_tau`` of one ``so3_angle_cdf`` call, whose queries are the m queries once per level; tau formed
    in fp64, rounded once), for
    ceil(log9(pi / tol)) passes, until hi - lo <= ``tol`` radians.  No host read-back inside the loop.  Where the mass at tau = 0
    already reaches alpha (the query is a centre that heavy) the radius is 0 and lo = hi = 0.  Each query's bracket depends on its own
    masses only: the result is bit-identical however the call is tiled.  A NaN query or group gives NaN.
    -> dict(radius [L,m] float64 radians = hi, lo [L,m] float64, mass_lo [L,m], mass_hi [L,m] float32: F at lo and at hi as evaluated, 1
    at a hi still pi); a leading G as ``so3_angle_cdf``."""
    who = "so3_angle_quantile"
    Cn, Qr, lw, G, grouped = _inputs(centres, queries, log_weights, bool(group_queries), who)
    return _angle_quantile(who, so3_angle_cdf, -3, Cn, Qr, lw, G, grouped, levels, bool(group_queries), tol, workspace_cap)


MAX_MEMBERS = 4096                                  # K of rnf_so3_set_angle_cdf (include/rnf_hip.h)


def _set_inputs(centres, query_sets, log_weights, group_queries, who: str):
    """``_inputs`` for sets: query_sets [m,K,3,3] or, with ``group_queries``, [G,m,K,3,3] -> (centres, sets [m,K,3,3] or [G,m,K,3,3],
    log-weights [G,n] or None, G, whether the outputs carry a leading G)"""
    dims = 5 if group_queries else 4
    if not isinstance(query_sets, torch.Tensor) or query_sets.dim() != dims or tuple(query_sets.shape[-2:]) != (3, 3):
        want = "[G,m,K,3,3] with group_queries" if group_queries else "[m,K,3,3]"
        raise ValueError(f"{who}: query_sets {tuple(getattr(query_sets, 'shape', ()))}, expected {want}")
    K = query_sets.shape[-3]
    if not 1 <= K <= MAX_MEMBERS:
        raise ValueError(f"{who}: sets of {K} members (1 to {MAX_MEMBERS})")
    flat = query_sets.reshape(*query_sets.shape[:-4], query_sets.shape[-4] * K, 3, 3)      # members as queries: the checks of _inputs
    Cn, Qr, lw, G, grouped = _inputs(centres, flat, log_weights, group_queries, who)
    return Cn, Qr.reshape(*query_sets.shape), lw, G, grouped


def so3_set_angle_cdf(centres, query_sets, thresholds=None, query_tau=None, log_weights=None, group_queries: bool = False,
                      moments: bool = True, workspace_cap: int = None) -> dict:
    """The distribution function of the angle to the NEAREST member of a set (``rnf_so3_set_angle_cdf``): ``so3_angle_cdf`` with
    d2_ij = min over the live members s of |Q_is - C_j|_F^2 in place of the single distance.  ``query_sets`` [m,K,3,3], shared by the
    groups, or with ``group_queries`` [G,m,K,3,3]: m sets of K members; a member with a non-finite entry is padding and is skipped (sets
    of unequal size are padded with NaN), a set of padding only is NaN.  The set is the orbit of an estimate under a symmetry group
    (``utils.symmetry.orbit``) for the error of a symmetric object, or k modes for a best-of-k error.  The other arguments, the
    outputs (``mass`` [T,m], ``mean_angle``, ``mean_sq_angle``, ``rms_angle`` [m], a leading G as ``so3_angle_cdf``) and the edge cases
    are ``so3_angle_cdf``'s; ``query_tau`` is [T,m] or [G,T,m], one set of thresholds per set.  A set's outputs do not depend on the
    order of its members or on padding among them; with K = 1 they are ``so3_angle_cdf``'s bits.  The sets and groups are tiled under
    ``workspace_cap`` exactly as ``so3_angle_cdf`` tiles queries (the workspace does not grow with K), bit-identically.  Stream-ordered,
    no host synchronisation, no gradient."""
    who = "so3_set_angle_cdf"
    Cn, Qr, lw, G, grouped = _set_inputs(centres, query_sets, log_weights, bool(group_queries), who)
    return _angle_cdf(who, "set", "sets", Cn, Qr, lw, G, grouped, Qr.shape[-3], thresholds, query_tau, group_queries, moments, workspace_cap)


def so3_set_angle_quantile(centres, query_sets, levels, log_weights=None, group_queries: bool = False, tol: float = 1e-3,
                           workspace_cap: int = None) -> dict:
    """``so3_angle_quantile`` for sets: the angle at which the union of the balls about a set's members reaches each level -- the
    quantiles of the angle to the nearest member.  The same 9-way bracket search on ``so3_set_angle_cdf``; ``query_sets`` as there, the
    other arguments and the result ([L,m], a leading G) as ``so3_angle_quantile``.  Bit-identical however the call is tiled."""
    who = "so3_set_angle_quantile"
    Cn, Qr, lw, G, grouped = _set_inputs(centres, query_sets, log_weights, bool(group_queries), who)
    return _angle_quantile(who, so3_set_angle_cdf, -4, Cn, Qr, lw, G, grouped, levels, bool(group_queries), tol, workspace_cap)
