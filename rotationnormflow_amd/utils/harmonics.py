"""Harmonic analysis on SO(3): the real Wigner matrices D^l(R), the Fourier coefficients of weighted sets of rotations and the
evaluation of band-limited densities at rotations, on three HIP passes (``rnf_so3_wigner``, ``rnf_so3_fourier``,
``rnf_so3_fourier_eval``, csrc/so3_harmonics.h).

Basis: Y_l(x) is the vector of the 2l+1 orthonormal real spherical harmonics of degree l (m = -l..l; for l = 1 the order is y, z, x)
and D^l(R) the real orthogonal matrix with Y_l(R x) = D^l(R) Y_l(x), so D^l(R1 R2) = D^l(R1) D^l(R2).  A coefficient vector holds the
degrees 0..L one after the other (``degree_offset``), each (2l+1) x (2l+1) block row-major: ``coefficient_count(L)`` entries.

``so3_fourier`` is the analysis F^l = sum_j w_j D^l(C_j) of the measure sum_j w_j delta_{C_j}; ``so3_fourier_density`` the synthesis
f(Q) = sum_l (2l+1) h_l <F^l, D^l(Q)>, the measure convolved with the zonal kernel of multipliers h_l as a density relative to the Haar
probability measure (uniform = 1): ``fisher_multipliers`` (the kernel of ``so3_kde`` and ``grid_diffuse``), ``heat_multipliers``, or
none (band limiting).  In coefficients the density of a product of independent rotations is a product of blocks (``compose``), that
of R^T a transpose, that of S R a multiplication by D(S) (``rotate``); ``power_spectrum`` says how sharp a density is."""
from __future__ import annotations

import math

import torch

from .. import _lib
from .kde import CHUNK, MAX_CENTRES, MAX_GROUPS, WORKSPACE_CAP, _aligned, _rotations

MAX_DEGREE = _lib.SO3_MAX_DEGREE


def _lmax(lmax, who: str) -> int:
    if isinstance(lmax, bool) or not isinstance(lmax, int) or not 0 <= lmax <= MAX_DEGREE:
        raise ValueError(f"{who}: lmax={lmax!r}, expected an integer in 0..{MAX_DEGREE}")
    return lmax


def coefficient_count(lmax: int) -> int:
    """C_L = (L+1)(2L+1)(2L+3)/3: the entries of the degrees 0..L"""
    L = _lmax(lmax, "coefficient_count")
    return (L + 1) * (2 * L + 1) * (2 * L + 3) // 3


def degree_offset(l: int) -> int:
    """Where degree l starts in a coefficient vector: l (4 l^2 - 1) / 3"""
    if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l <= MAX_DEGREE + 1:
        raise ValueError(f"degree_offset: l={l!r}, expected an integer in 0..{MAX_DEGREE + 1}")
    return l * (4 * l * l - 1) // 3


def _coeffs(coeffs, lmax, who: str, name: str = "coeffs"):
    L = _lmax(lmax, who)
    if not isinstance(coeffs, torch.Tensor) or coeffs.dim() not in (1, 2) or coeffs.shape[-1] != coefficient_count(L):
        raise ValueError(f"{who}: {name} {tuple(getattr(coeffs, 'shape', ()))}, expected [{coefficient_count(L)}] or [G,{coefficient_count(L)}] "
                         f"for lmax={L}")
    return L


def blocks(coeffs, lmax: int) -> list:
    """The degrees of a coefficient tensor [..,C_L] as views [..,2l+1,2l+1], l = 0..lmax"""
    L = _lmax(lmax, "blocks")
    if not isinstance(coeffs, torch.Tensor) or coeffs.dim() < 1 or coeffs.shape[-1] != coefficient_count(L):
        raise ValueError(f"blocks: coeffs {tuple(getattr(coeffs, 'shape', ()))}, expected [..,{coefficient_count(L)}] for lmax={L}")
    return [coeffs[..., degree_offset(l):degree_offset(l + 1)].unflatten(-1, (2 * l + 1, 2 * l + 1)) for l in range(L + 1)]


def from_blocks(blks) -> torch.Tensor:
    """The coefficient tensor [..,C_L] of blocks [..,2l+1,2l+1], l = 0..L"""
    blks = list(blks)
    for l, b in enumerate(blks):
        if not isinstance(b, torch.Tensor) or b.dim() < 2 or tuple(b.shape[-2:]) != (2 * l + 1, 2 * l + 1):
            raise ValueError(f"from_blocks: block {l} is {tuple(getattr(b, 'shape', ()))}, expected [..,{2 * l + 1},{2 * l + 1}]")
    _lmax(len(blks) - 1, "from_blocks")
    return torch.cat([b.flatten(-2) for b in blks], dim=-1)


def wigner_matrices(rotations, lmax: int) -> torch.Tensor:
    """D^l(R_i), l = 0..lmax, written out: [n,C_L] float32 (``blocks`` gives the matrices).  A rotation is read through its normalised
    quaternion; one with a non-finite entry gives NaN for its row.  For tests and small uses: n C_L floats."""
    who = "wigner_matrices"
    L = _lmax(lmax, who)
    R = _rotations(rotations, "rotations", who)
    n = R.shape[0]
    if n > MAX_CENTRES:
        raise ValueError(f"{who}: rotations holds {n} rotations (at most 2^24)")
    out = torch.empty(n, coefficient_count(L), dtype=torch.float32, device=R.device)
    if n > 0:
        _lib.call("so3_wigner", _lib.So3Wigner(rotations=R.data_ptr(), n=n, lmax=L, out=out.data_ptr()), R.device)
    return out


def so3_fourier(rotations, lmax: int, log_weights=None, workspace_cap: int = None) -> torch.Tensor:
    """The Fourier coefficients F^l = sum_j w_j D^l(C_j), l = 0..lmax, of the rotations ``rotations`` [n,3,3] under
    w = softmax(``log_weights``) (None: uniform; [n] -> [C_L]; [G,n] -> [G,C_L]), float32.  F^0 = 1.  The rotations need not be grid rows.
    A rotation with log-weight -inf is left out; another non-finite rotation, a NaN log-weight or a group without mass makes its group
    NaN.  A group's coefficients are bit-identical whatever the other groups are, so the tiling of the groups that keeps the partial
    sums and weights (8 ceil(n/4096) (C_L + 2) + 4 n + 8 bytes per group) under ``workspace_cap`` (64 MiB) is invisible; the power
    tables of the rotations, 4 n (8 lmax + 16) bytes, come on top.  Stream-ordered, no host synchronisation, no gradient."""
    who = "so3_fourier"
    L = _lmax(lmax, who)
    Cn = _rotations(rotations, "rotations", who)
    n, dev = Cn.shape[0], Cn.device
    if not 1 <= n <= MAX_CENTRES:
        raise ValueError(f"{who}: rotations holds {n} rotations (1 to 2^24)")
    lw, grouped = None, False
    if log_weights is not None:
        if not isinstance(log_weights, torch.Tensor) or log_weights.dim() not in (1, 2) or log_weights.shape[-1] != n:
            raise ValueError(f"{who}: log_weights {tuple(getattr(log_weights, 'shape', ()))} for {n} rotations, expected [n] or [G,n]")
        if not log_weights.is_cuda:
            raise ValueError(f"{who}: log_weights is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        grouped = log_weights.dim() == 2
        lw = log_weights.detach().to(device=dev, dtype=torch.float32).reshape(-1, n).contiguous()
    G = lw.shape[0] if lw is not None else 1
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"{who}: {G} groups (1 to 65535)")
    cap = WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    CL = coefficient_count(L)
    per_group = 8 * ((n + CHUNK - 1) // CHUNK) * (CL + 2) + 4 * n + 8
    if per_group > cap:
        raise ValueError(f"{who}: one group's partial sums take {per_group} bytes, above workspace_cap={cap}; pass a larger workspace_cap")
    out = torch.empty(G, CL, dtype=torch.float32, device=dev)
    g_tile = max(1, min(G, cap // per_group))
    for g0 in range(0, G, g_tile):
        g1 = min(G, g0 + g_tile)
        args = _lib.So3Fourier(centres=Cn.data_ptr(), log_weights=lw[g0:g1].data_ptr() if lw is not None else None, n=n, G=g1 - g0, lmax=L,
                               out=out[g0:g1].data_ptr())
        _lib.call("so3_fourier", args, dev)
    return out if grouped else out[0]


def so3_fourier_density(coeffs, rotations, lmax: int, multiplier=None, group_queries: bool = False) -> torch.Tensor:
    """The band-limited density of the coefficients ``coeffs`` ([C_L] or [G,C_L], as ``so3_fourier`` gives them) at the rotations
    ``rotations`` ([m,3,3], shared by the groups, or with ``group_queries`` [G,m,3,3]):
    f(Q) = sum_l (2l+1) h_l sum_{m'm} F^l_{m'm} D^l_{m'm}(Q), relative to the Haar probability measure (uniform = 1), [m] or [G,m] float32.
    ``multiplier``: h_0..h_lmax (a sequence or tensor of lmax+1 numbers: ``fisher_multipliers``, ``heat_multipliers``; a tensor on the
    device of ``coeffs`` keeps the call free of host copies, hence capturable), None: ones (band limiting; the result may then be
    negative).  The factor (2l+1) is applied here.  A non-finite rotation gives NaN for itself;
    non-finite coefficients stay in their group.  A value is bit-identical however rotations and groups are tiled.  Stream-ordered, no
    host synchronisation, no gradient."""
    who = "so3_fourier_density"
    L = _coeffs(coeffs, lmax, who)
    if not coeffs.is_cuda:
        raise ValueError(f"{who}: coeffs is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    dev = coeffs.device
    grouped = coeffs.dim() == 2 or bool(group_queries)
    c = coeffs.detach().to(torch.float32).reshape(-1, coeffs.shape[-1])
    if group_queries:
        if not isinstance(rotations, torch.Tensor) or rotations.dim() != 4 or tuple(rotations.shape[-2:]) != (3, 3):
            raise ValueError(f"{who}: rotations {tuple(getattr(rotations, 'shape', ()))}, expected [G,m,3,3] with group_queries")
        if not rotations.is_cuda:
            raise ValueError(f"{who}: rotations is on the CPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        Q = _aligned(rotations.detach().to(torch.float32).contiguous())
        if c.shape[0] == 1 and Q.shape[0] > 1:
            c = c.expand(Q.shape[0], -1)
        if Q.shape[0] != c.shape[0]:
            raise ValueError(f"{who}: rotations holds {Q.shape[0]} groups, coeffs {c.shape[0]}")
    else:
        Q = _rotations(rotations, "rotations", who)
    if Q.device != dev:
        raise ValueError(f"{who}: rotations on {Q.device}, coeffs on {dev}")
    G, m = c.shape[0], Q.shape[-3]
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"{who}: {G} groups (1 to 65535)")
    if m >= 1 << 31:
        raise ValueError(f"{who}: rotations holds {m} rotations (below 2^31)")
    scale = _degree_scale(multiplier, L, who, dev)
    c = (c.to(torch.float64) * scale).to(torch.float32).contiguous()
    out = torch.empty(G, m, dtype=torch.float32, device=dev)
    if m > 0:
        args = _lib.So3FourierEval(coeffs=c.data_ptr(), queries=Q.data_ptr(), m=m, G=G, group_queries=int(bool(group_queries)), lmax=L,
                                   out=out.data_ptr())
        _lib.call("so3_fourier_eval", args, dev)
    return out if grouped else out[0]


_ENTRY_DEGREE = {}                                   # (L, device) -> int64 [C_L], the degree of each entry, on the device


def _degree_scale(multiplier, L: int, who: str, dev) -> torch.Tensor:
    """(2l+1) h_l spread over the entries of degree l: [C_L] float64 on ``dev`` (the caller multiplies in fp64 and rounds once).  With ``multiplier``
    None or a tensor on ``dev`` nothing crosses from the host once the degree index of (L, dev) is cached."""
    key = (L, str(dev))
    if key not in _ENTRY_DEGREE:
        _ENTRY_DEGREE[key] = torch.cat([torch.full(((2 * l + 1) ** 2,), l, dtype=torch.int64) for l in range(L + 1)]).to(dev)
    degree = _ENTRY_DEGREE[key]
    odd = 2.0 * degree.to(torch.float64) + 1.0
    if multiplier is None:
        return odd
    if isinstance(multiplier, torch.Tensor):
        h = multiplier.detach().reshape(-1)
    else:
        h = torch.tensor([float(v) for v in multiplier], dtype=torch.float64)
    if h.shape[0] != L + 1:
        raise ValueError(f"{who}: multiplier holds {h.shape[0]} numbers, expected lmax + 1 = {L + 1}")
    return odd * h.to(device=dev, dtype=torch.float64)[degree]


def fisher_multipliers(kappa: float, lmax: int) -> torch.Tensor:
    """The multipliers of the isotropic matrix-Fisher kernel exp(kappa tr(M^T R)) / c(kappa), the kernel of ``so3_kde`` and
    ``grid_diffuse``: a_l = [I_l(2 kappa) - I_{l+1}(2 kappa)] / ((2l+1) [I_0(2 kappa) - I_1(2 kappa)]), l = 0..lmax, float64 on the CPU.
    The Bessel ratios r_k = I_{k+1} / I_k come from the backward recurrence r_{k-1} = 1 / (2k / x + r_k) in fp64."""
    L = _lmax(lmax, "fisher_multipliers")
    kappa = float(kappa)
    if not (math.isfinite(kappa) and 0.0 <= kappa <= 1.0e6):
        raise ValueError(f"fisher_multipliers: kappa={kappa} outside 0..1e6")
    x = 2.0 * kappa
    if x == 0.0:
        return torch.tensor([1.0] + [0.0] * L, dtype=torch.float64)
    K = L + 40 + int(8.0 * math.sqrt(x))              # the start's error decays like exp(-(K^2 - L^2) / x)
    r = [0.0] * (K + 1)
    for k in range(K, 0, -1):
        r[k - 1] = 1.0 / (2.0 * k / x + r[k])
    out, ratio = [], 1.0                              # ratio = I_l / I_0
    for l in range(L + 1):
        out.append(ratio * (1.0 - r[l]) / ((2 * l + 1) * (1.0 - r[0])))
        ratio *= r[l]
    return torch.tensor(out, dtype=torch.float64)


def heat_multipliers(t: float, lmax: int) -> torch.Tensor:
    """The multipliers exp(-l (l+1) t) of the heat kernel on SO(3) at time t >= 0, l = 0..lmax, float64 on the CPU"""
    L = _lmax(lmax, "heat_multipliers")
    t = float(t)
    if not (math.isfinite(t) and t >= 0.0):
        raise ValueError(f"heat_multipliers: t={t}, expected a finite number >= 0")
    return torch.tensor([math.exp(-l * (l + 1) * t) for l in range(L + 1)], dtype=torch.float64)


def power_spectrum(coeffs, lmax: int) -> torch.Tensor:
    """P_l = (2l+1) |F^l|_F^2, l = 0..lmax: [..,lmax+1] in the dtype of ``coeffs``.  sum_l P_l tends to the integral of p^2 over SO(3)
    (Haar probability measure) as lmax grows; for a discrete measure P_l = sum_ij w_i w_j (2l+1) chi_l(theta_ij)."""
    return torch.stack([(2 * l + 1) * b.flatten(-2).square().sum(-1) for l, b in enumerate(blocks(coeffs, lmax))], dim=-1)


def compose(coeffs_a, coeffs_b, lmax: int, invert_a: bool = False, invert_b: bool = False) -> torch.Tensor:
    """The coefficients of R_a R_b for independent R_a ~ a, R_b ~ b: the block products F_a^l F_b^l.  ``invert_a`` / ``invert_b``: of
    R_a^T R_b (the relative rotation) / R_a R_b^T -- the measure of R^T has the transposed blocks.  [C_L] or [G,C_L] each (one may be
    shared by the groups of the other).  Small ``torch.matmul`` products: plumbing, any device."""
    A, B = blocks(coeffs_a, lmax), blocks(coeffs_b, lmax)
    return from_blocks([torch.matmul(a.transpose(-1, -2) if invert_a else a, b.transpose(-1, -2) if invert_b else b) for a, b in zip(A, B)])


def rotate(coeffs, S, lmax: int, side: str = "left") -> torch.Tensor:
    """The coefficients of S R (``side="left"``: D^l(S) F^l) or R S (``"right"``: F^l D^l(S)) for R ~ coeffs and a fixed rotation
    ``S`` [3,3] on the device of ``coeffs``: a posterior carried into another frame."""
    if side not in ("left", "right"):
        raise ValueError(f"rotate: side={side!r}, expected 'left' or 'right'")
    L = _coeffs(coeffs, lmax, "rotate")
    if not isinstance(S, torch.Tensor) or tuple(S.shape) != (3, 3):
        raise ValueError(f"rotate: S {tuple(getattr(S, 'shape', ()))}, expected [3,3]")
    D = wigner_matrices(S[None].to(coeffs.device), L)[0].to(coeffs.dtype)
    return compose(D, coeffs, L) if side == "left" else compose(coeffs, D, L)
