"""Mirror of the reference's utils/fisher.py: ``MatrixFisherN`` (log-density on the GPU through rnf_fisher_log_prob).

log p(R) = tr(A^T R) - (s0+s1+s2) - log norm, norm = 1/sqrt(8 pi (s0+s1)(s1+s2)(s0+s2))   (utils/fisher.py:93-97,217-232; norm_type 1)
with s the *proper* singular values of A (last one sign-flipped by det(U) det(V), utils/fisher.py:67-76); norm_type 0 is the
small-s approximation of utils/fisher.py:88-91.  norm_type "exact" is the exact normaliser (the integral the reference's type 3 means),
per row on the device through rnf_fisher_exact: finite and smooth for every A.  Differentiable w.r.t. the rotations and w.r.t. A.
``MatrixFisherN.fit`` / ``fit_matrix_fisher`` estimate A from rotations (the inverse of ``mean_rotation``), ``rotation_moments`` is their
sufficient statistic.  ``MatrixFisherMixture`` / ``fit_matrix_fisher_mixture`` fit and evaluate K-component mixtures of exact matrix-Fishers
by EM on the device (csrc/fisher_mixture.h).
"""
import math

import torch

from .. import _lib


def device_proper_svd(A):
    """A [B,3,3] on the GPU -> (U, V, s, lam) fp32 device tensors through rnf_fisher_proper_svd (fp64 Jacobi, one thread per matrix):
    stream-ordered, no host synchronisation (utils/fisher.py:53-76,151-158)."""
    A32 = A.detach().reshape(-1, 3, 3).to(torch.float32).contiguous()
    B, dev = A32.shape[0], A32.device
    U = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
    V = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
    s = torch.empty(B, 3, dtype=torch.float32, device=dev)
    lam = torch.empty(B, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rnf_fisher_proper_svd(A32.data_ptr(), B, U.data_ptr(), V.data_ptr(), s.data_ptr(), lam.data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream))
    return U, V, s, lam


def proper_singular_values(A):
    """[B,3,3] -> [B,3] in fp64 (utils/fisher.py:67-76), by host LAPACK on an fp64 copy of A -- also for a GPU-resident A (one tiny
    device -> host copy).  This serves the lazily computed ``MatrixFisherN.norm`` attribute only (a diagnostic: the density path uses the
    device kernels and never calls it), where round 3's fp32 device values cost ``sum(S) * 6e-8`` of relative accuracy and dropped the
    precision of a float64 A."""
    A64 = A.detach().to("cpu", torch.float64)
    U, S, Vh = torch.linalg.svd(A64)
    S = S.clone()
    S[:, 2] = S[:, 2] * torch.det(U) * torch.det(Vh)
    return S


def device_fisher_exact(A, want="c"):
    """A [B,3,3] on the GPU -> the exact log-normaliser c [B] (want="c"), the mean rotation E[R] = dc/dA [B,3,3] ("mean") or the entropy
    c - tr(A^T E[R]) [B] ("entropy") of MF(A[b]), fp32 device tensors from the wave-per-matrix quadrature kernel (csrc/fisher_exact.h).
    Stream-ordered, no host synchronisation, not differentiable."""
    if not A.is_cuda:
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback): the exact normaliser needs A on the GPU")
    A32 = A.detach().reshape(-1, 3, 3).to(torch.float32).contiguous()
    B, dev = A32.shape[0], A32.device
    out = torch.empty((B, 3, 3) if want == "mean" else (B,), dtype=torch.float32, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if want == "c":
            _lib.check(L.rnf_fisher_exact(A32.data_ptr(), B, out.data_ptr(), None, stream))
        elif want == "mean":
            _lib.check(L.rnf_fisher_exact(A32.data_ptr(), B, None, out.data_ptr(), stream))
        else:
            _lib.check(L.rnf_fisher_entropy(A32.data_ptr(), B, out.data_ptr(), stream))
    return out


def _rotation_groups(rotations, log_weights, who: str):
    """The group arguments of ``rotation_moments`` (its docstring) -> (R fp32 [n,3,3] | [G,n,3,3], lw fp32 [G,n] or None, n, G, shared)."""
    if not rotations.is_cuda:
        raise RuntimeError(f"rotationnormflow_amd runs on the GPU only (no CPU fallback): {who} needs the rotations on the GPU")
    if rotations.dim() not in (3, 4) or tuple(rotations.shape[-2:]) != (3, 3):
        raise ValueError(f"{who}: rotations {tuple(rotations.shape)}, expected [n,3,3] or [G,n,3,3]")
    R = rotations.detach().to(torch.float32).contiguous()
    n = R.shape[-3]
    lw = None
    if log_weights is not None:
        lw = log_weights.detach().to(device=R.device, dtype=torch.float32)
        lw = lw.reshape(1, -1) if lw.dim() == 1 else lw
        if lw.dim() != 2 or lw.shape[1] != n or (R.dim() == 4 and lw.shape[0] != R.shape[0]):
            raise ValueError(f"{who}: log_weights {tuple(log_weights.shape)} for rotations {tuple(rotations.shape)}")
        lw = lw.contiguous()
    shared = R.dim() == 3 and lw is not None
    G = lw.shape[0] if shared else (R.shape[0] if R.dim() == 4 else 1)
    return R, lw, n, G, shared


def rotation_moments(rotations, log_weights=None):
    """Weighted moments M_g = sum_i w_gi R_gi of groups of rotations, fp64 [G,3,3] on the device (rnf_rotation_moments): the sufficient
    statistic of ``fit_matrix_fisher``.  ``rotations`` [n,3,3] (one group), [G,n,3,3], or [n,3,3] with ``log_weights`` [G,n] (one set
    of rotations shared by G weightings -- a grid and one row of log-densities per image).  w_g = softmax(log_weights[g]) (fp64; a -inf
    row contributes 0), or 1/n without log-weights.  Fixed summation order: a group's moment is bit-identical however it is batched.
    A group whose weights are all -inf, or that holds a NaN, yields NaN.  Stream-ordered, no host synchronisation."""
    R, lw, n, G, shared = _rotation_groups(rotations, log_weights, "rotation_moments")
    dev = R.device
    if n < 1 or G < 1:
        raise ValueError(f"rotation_moments: {G} groups of {n} rotations")
    out = torch.empty(G, 3, 3, dtype=torch.float64, device=dev)
    args = _lib.RotationMoments(rotations=R.data_ptr(), log_weights=lw.data_ptr() if lw is not None else None, n=n, G=G,
                                shared_rotations=int(shared), moments_out=out.data_ptr())
    _lib.call("rotation_moments", args, dev)
    return out


def fit_matrix_fisher(moments, max_concentration=1e4, max_iterations=0):
    """The maximum-likelihood matrix-Fisher parameters of moment matrices ``moments`` [B,3,3] (fp64 on the device, e.g. from
    ``rotation_moments``): A with E_A[R] = moments under the exact normaliser (rnf_fisher_fit, csrc/fisher_fit.h).
    -> dict(A [B,3,3] fp32, s [B,3] fp64 proper singular values of A, hessian [B,6] fp64 = d2c/ds2 as (00, 01, 02, 11, 12, 22),
    iterations [B] int32, status [B] int32), all on the device.  status bits: 1 CAPPED (no finite maximiser, or s0 > max_concentration:
    the likelihood's maximiser over |s_i| <= max_concentration, with s0 == max_concentration), 2 NOT_CONVERGED (the last iterate),
    4 INPUT (a moment outside the convex hull of SO(3), or non-finite: NaN).  ``max_iterations`` 0 is the library's cap.
    Stream-ordered, no host synchronisation: reading ``status`` on the host is what waits."""
    if not moments.is_cuda:
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback): fit_matrix_fisher needs the moments on the GPU")
    dev = moments.device
    M = moments.detach().reshape(-1, 3, 3).to(torch.float64).contiguous()
    B = M.shape[0]
    A = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
    s = torch.empty(B, 3, dtype=torch.float64, device=dev)
    H = torch.empty(B, 6, dtype=torch.float64, device=dev)
    it = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    args = _lib.FisherFit(moments=M.data_ptr(), B=B, max_concentration=float(max_concentration), max_iterations=int(max_iterations),
                          A_out=A.data_ptr(), s_out=s.data_ptr(), hessian_out=H.data_ptr(), iterations_out=it.data_ptr(),
                          status_out=st.data_ptr())
    _lib.call("fisher_fit", args, dev)
    return dict(A=A, s=s, hessian=H, iterations=it, status=st)


MIX_EMPTY = 8        # RNF_MIX_EMPTY, beside the RNF_FIT_* bits of fit_matrix_fisher


def fit_matrix_fisher_mixture(rotations, log_weights, A_init, log_pi_init=None, iterations=64, tol=1e-9, max_concentration=1e4,
                              log_resp=False):
    """EM for K-component mixtures of exact matrix-Fishers on the device (rnf_fisher_mixture_fit, csrc/fisher_mixture.h):
    log p(R) = logsumexp_k(log_pi_k + tr(A_k^T R) - c(A_k)) w.r.t. the Haar probability measure.  ``rotations`` / ``log_weights`` as
    ``rotation_moments`` ([n,3,3], [G,n,3,3], or [n,3,3] shared by ``log_weights`` [G,n]; None: w = 1/n); ``A_init`` [G,K,3,3] (or
    [K,3,3] for one group), ``log_pi_init`` [G,K] fp64 or None (uniform; -inf marks an empty component).  At most ``iterations`` EM
    iterations (1..256); a group stops once 0 <= L_t - L_(t-1) <= tol (tol = 0: every iteration runs).
    -> dict(A [G,K,3,3] fp32, log_pi [G,K] fp64, s [G,K,3] fp64, loglik [G,iterations+1] fp64 (entry t: L before iteration t; NaN after
    the last used one), weight_entropy [G] fp64, status [G,K] int32 (RNF_FIT_* bits of the component's last solve, 8: empty),
    iterations [G] int32, log_resp [G,K,n] fp32 with ``log_resp=True``), all on the device.  The state between iterations is exactly
    (A, log_pi): T iterations equal T chained calls of one.  A group's outputs are bit-identical however it is batched; K = 1 gives the
    A, s and status of ``rotation_moments`` + ``fit_matrix_fisher``.  A group with all weights -inf, a NaN, or no live component is NaN
    with status 4.  Stream-ordered, no host synchronisation, capturable."""
    R, lw, n, G, shared = _rotation_groups(rotations, log_weights, "fit_matrix_fisher_mixture")
    dev = R.device
    A0 = A_init.detach().to(device=dev, dtype=torch.float32)
    if A0.dim() not in (3, 4) or tuple(A0.shape[-2:]) != (3, 3) or A0.numel() % (9 * G) or (A0.dim() == 4 and A0.shape[0] != G):
        raise ValueError(f"fit_matrix_fisher_mixture: A_init {tuple(A_init.shape)} for {G} groups, expected [G,K,3,3]")
    A0 = A0.reshape(G, -1, 3, 3).contiguous()
    K = A0.shape[1]
    if not 1 <= K <= 8:
        raise ValueError(f"fit_matrix_fisher_mixture: {K} components outside 1..8")
    if not 1 <= int(iterations) <= 256:
        raise ValueError(f"fit_matrix_fisher_mixture: iterations={iterations} outside 1..256")
    lp0 = None
    if log_pi_init is not None:
        lp0 = log_pi_init.detach().to(device=dev, dtype=torch.float64)
        if lp0.numel() != G * K:
            raise ValueError(f"fit_matrix_fisher_mixture: log_pi_init {tuple(log_pi_init.shape)}, expected [{G},{K}]")
        lp0 = lp0.reshape(G, K).contiguous()
    T = int(iterations)
    out = dict(A=torch.empty(G, K, 3, 3, dtype=torch.float32, device=dev), log_pi=torch.empty(G, K, dtype=torch.float64, device=dev),
               s=torch.empty(G, K, 3, dtype=torch.float64, device=dev), loglik=torch.empty(G, T + 1, dtype=torch.float64, device=dev),
               weight_entropy=torch.empty(G, dtype=torch.float64, device=dev), status=torch.empty(G, K, dtype=torch.int32, device=dev),
               iterations=torch.empty(G, dtype=torch.int32, device=dev))
    if log_resp:
        out["log_resp"] = torch.empty(G, K, n, dtype=torch.float32, device=dev)
    args = _lib.FisherMixtureFit(rotations=R.data_ptr(), log_weights=lw.data_ptr() if lw is not None else None, n=n, G=G,
                                 shared_rotations=int(shared), K=K, A_init=A0.data_ptr(), log_pi_init=lp0.data_ptr() if lp0 is not None else None,
                                 iterations=T, tol=float(tol), max_concentration=float(max_concentration), A_out=out["A"].data_ptr(),
                                 log_pi_out=out["log_pi"].data_ptr(), s_out=out["s"].data_ptr(), loglik_out=out["loglik"].data_ptr(),
                                 weight_entropy_out=out["weight_entropy"].data_ptr(),
                                 log_resp_out=out["log_resp"].data_ptr() if log_resp else None, status_out=out["status"].data_ptr(),
                                 iterations_out=out["iterations"].data_ptr())
    _lib.call("fisher_mixture_fit", args, dev)
    return out


def mixture_init_from_modes(grid, index, mass, separation_rad):
    """The start of a mixture fit from ``grid_pose.grid_modes``: component k sits on mode k with A_k = kappa0 R_k, kappa0 = 2 /
    separation_rad^2 (MF(kappa R) has an angular standard deviation of 1 / sqrt(2 kappa) per axis: half the separation), log_pi_k the log
    of the mode's share of the modes' mass; a missing mode (index -1) or one without mass is an empty component (log_pi = -inf, A = 0).
    grid [Q,3,3], index [g,K] int64, mass [g,K] -> (A_init [g,K,3,3] fp32, log_pi_init [g,K] fp64)."""
    kappa0 = 2.0 / float(separation_rad) ** 2
    have = index >= 0
    A = grid.reshape(-1, 3, 3).to(torch.float32)[index.clamp(min=0)] * kappa0
    A = torch.where(have[..., None, None], A, torch.zeros_like(A))
    m = torch.where(have, mass.to(torch.float64), torch.zeros_like(mass, dtype=torch.float64))
    return A.contiguous(), torch.log(m / m.sum(-1, keepdim=True))


class MatrixFisherMixture(torch.nn.Module):
    """A K-component mixture of exact matrix-Fishers: log p(R) = logsumexp_k(log_weight_k + tr(A_k^T R) - c(A_k)) w.r.t. the Haar
    probability measure.  ``A`` [K,3,3] (fp32) and ``log_weight`` [K] (fp64; -inf drops a component) are registered buffers: they move
    with ``.to()`` and are what ``state_dict()`` stores.  No autograd."""

    def __init__(self, A, log_weight):
        super().__init__()
        if not A.is_cuda:
            raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback): construct MatrixFisherMixture with A on the GPU")
        self.register_buffer("A", A.detach().reshape(-1, 3, 3).to(torch.float32).contiguous().clone())
        self.register_buffer("log_weight", log_weight.detach().reshape(-1).to(device=self.A.device, dtype=torch.float64).contiguous().clone())
        if not 1 <= self.A.shape[0] <= 8 or self.log_weight.shape[0] != self.A.shape[0]:
            raise ValueError(f"MatrixFisherMixture: A {tuple(A.shape)} and log_weight {tuple(log_weight.shape)}, expected [K,3,3] and [K], K in 1..8")

    def _evaluate(self, rotations, want_resp):
        if not rotations.is_cuda:
            raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        if rotations.dim() != 3 or tuple(rotations.shape[-2:]) != (3, 3):
            raise ValueError(f"MatrixFisherMixture: rotations {tuple(rotations.shape)}, expected [n,3,3]")
        if not self.A.is_cuda:
            raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback): move the MatrixFisherMixture to the GPU")
        dev = self.A.device
        A = self.A.to(torch.float32).contiguous()                       # a module-wide .double() / .half() must not change what the kernel reads
        log_weight = self.log_weight.to(torch.float64).contiguous()
        R = rotations.detach().to(device=dev, dtype=torch.float32).contiguous()
        n, K = R.shape[0], A.shape[0]
        logp = torch.empty(n, dtype=torch.float32, device=dev)
        resp = torch.empty(K, n, dtype=torch.float32, device=dev) if want_resp else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rnf_fisher_mixture_log_prob(A.data_ptr(), log_weight.data_ptr(), K, R.data_ptr(), n, logp.data_ptr(),
                                                              resp.data_ptr() if want_resp else None, torch.cuda.current_stream(dev).cuda_stream))
        return logp, resp

    def log_prob(self, rotations):
        """[n,3,3] -> log p [n] fp32 (rnf_fisher_mixture_log_prob: the row function of the E-step)."""
        return self._evaluate(rotations, False)[0]

    def log_responsibilities(self, rotations):
        """[n,3,3] -> log r [n,K] fp32: each row's log posterior membership in each component (-inf for a dropped one)."""
        return self._evaluate(rotations, True)[1].t()

    def responsibilities(self, rotations):
        """[n,3,3] -> r [n,K] fp32, rows summing to 1."""
        return self.log_responsibilities(rotations).exp()

    def components(self):
        """The K components as one ``MatrixFisherN(A [K,3,3], "exact")``."""
        return MatrixFisherN(self.A, "exact")

    @classmethod
    def fit(cls, rotations, log_weights=None, components=4, init=None, separation_deg=15.0, iterations=64, tol=1e-9, max_concentration=1e4):
        """EM fit of one mixture to ``rotations`` [n,3,3] with weights softmax(``log_weights`` [n]) (None: 1/n), by
        ``fit_matrix_fisher_mixture``.  ``init``: A_init [K,3,3], or (A_init, log_pi_init [K]); None with log-weights given starts from
        ``grid_pose.grid_modes`` of the log-weights on the rotations (``components`` modes at least ``separation_deg`` apart, see
        ``mixture_init_from_modes``); None without log-weights is refused.  The result carries ``fit_status`` [K], ``fit_s`` [K,3],
        ``fit_iterations``, ``log_likelihood`` (fp64 scalars on the device) and ``fit`` (the whole output dict)."""
        if rotations.dim() != 3:
            raise ValueError(f"MatrixFisherMixture.fit: rotations {tuple(rotations.shape)}, expected one group [n,3,3]")
        lw = None
        if log_weights is not None:
            lw = log_weights.reshape(1, -1)
            if lw.shape[1] != rotations.shape[0]:
                raise ValueError(f"MatrixFisherMixture.fit: log_weights {tuple(log_weights.shape)} for rotations {tuple(rotations.shape)}")
        if init is None:
            if lw is None:
                raise ValueError("MatrixFisherMixture.fit: without log_weights there are no modes to start from; pass init")
            if not 1 <= int(components) <= 8:
                raise ValueError(f"MatrixFisherMixture.fit: components={components} outside 1..8")
            from .. import grid_pose
            sep = math.radians(float(separation_deg))
            index, _, mass, _, _ = grid_pose.grid_modes(lw.to(device=rotations.device, dtype=torch.float32), rotations, int(components), sep)
            A0, lp0 = mixture_init_from_modes(rotations, index, mass, sep)
        else:
            A0, lp0 = init if isinstance(init, (tuple, list)) else (init, None)
            A0 = A0.reshape(1, -1, 3, 3)
        fit = fit_matrix_fisher_mixture(rotations, lw, A0, lp0, iterations, tol, max_concentration)
        out = cls(fit["A"][0], fit["log_pi"][0])
        out.fit_status, out.fit_s, out.fit_iterations, out.fit = fit["status"][0], fit["s"][0], fit["iterations"][0], fit
        out.log_likelihood = fit["loglik"][0].gather(0, fit["iterations"][0].reshape(1).long())[0]
        return out


def quaternion_to_matrix(q):
    """Real-part-first quaternions -> rotation matrices (semantics of pytorch3d.transforms.quaternion_to_matrix)."""
    w, x, y, z = q.unbind(-1)
    s2 = 2.0 / (q * q).sum(-1)
    m = torch.stack([1 - s2 * (y * y + z * z), s2 * (x * y - z * w), s2 * (x * z + y * w),
                     s2 * (x * y + z * w), 1 - s2 * (x * x + z * z), s2 * (y * z - x * w),
                     s2 * (x * z - y * w), s2 * (y * z + x * w), 1 - s2 * (x * x + y * y)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def _norm_from_singular_values(S, norm_type):
    """matrix_fisher_norm_N (utils/fisher.py:79-97) for the two closed-form approximations; type 0 keeps the reference's batch-global
    ``(S**2).sum()``."""
    if norm_type == 0:
        return (1.0 + (S ** 2).sum() / 6.0 + S[:, 0] * S[:, 1] * S[:, 2] / 6.0) / S.sum(-1).exp()
    return 1.0 / torch.sqrt(8 * math.pi * (S[:, 0] + S[:, 1]) * (S[:, 2] + S[:, 1]) * (S[:, 0] + S[:, 2]))


class _FisherLogProb(torch.autograd.Function):
    """log p(R) = tr(A^T R) - c through rnf_fisher_log_prob; d/dR = g A through rnf_fisher_log_prob_backward (training with a
    matrix-Fisher base differentiates it w.r.t. the flow's output rotation, agent.py:58-64); d/dA -- needed when A is predicted by a
    network and kept in the graph, agent.py:57-65 -- through rnf_fisher_log_prob_backward_param (derivative of the normaliser included)."""

    @staticmethod
    def forward(ctx, inputs, A_param, A, c, norm_type):
        R = inputs.reshape(-1, 3, 3).to(torch.float32).contiguous()
        n, B = R.shape[0], A.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=R.device)
        with torch.cuda.device(R.device):
            _lib.check(_lib.lib().rnf_fisher_log_prob(R.data_ptr(), n, A.data_ptr(), c.data_ptr(), B, out.data_ptr(),
                                                      torch.cuda.current_stream(R.device).cuda_stream))
        ctx.save_for_backward(A, R)
        ctx.in_shape, ctx.in_dtype, ctx.norm_type = inputs.shape, inputs.dtype, norm_type
        ctx.A_shape, ctx.A_dtype, ctx.A_device = A_param.shape, A_param.dtype, A_param.device
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        A, R = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        n, B = g.shape[0], A.shape[0]
        L = _lib.lib()
        g_rot = g_A = None
        with torch.cuda.device(g.device):
            stream = torch.cuda.current_stream(g.device).cuda_stream
            if ctx.needs_input_grad[0]:
                g_rot = torch.empty((n, 3, 3), dtype=torch.float32, device=g.device)
                _lib.check(L.rnf_fisher_log_prob_backward(g.data_ptr(), n, A.data_ptr(), B, g_rot.data_ptr(), stream))
                g_rot = g_rot.reshape(ctx.in_shape).to(ctx.in_dtype)
            if ctx.needs_input_grad[1]:
                g_A = torch.empty((B, 3, 3), dtype=torch.float32, device=g.device)
                scratch = torch.empty(int(L.rnf_fisher_scratch_bytes(B)) // 8, dtype=torch.float64, device=g.device)
                _lib.check(L.rnf_fisher_log_prob_backward_param(g.data_ptr(), R.data_ptr(), n, A.data_ptr(), B, ctx.norm_type, scratch.data_ptr(),
                                                            scratch.numel() * 8, g_A.data_ptr(), stream))
                g_A = g_A.reshape(ctx.A_shape).to(device=ctx.A_device, dtype=ctx.A_dtype)
        return g_rot, g_A, None, None, None


# fail flags of earlier _sample calls (a proposal loop that exhausted its 4096 attempts leaves the identity rotation in that slot): read
# back through pinned memory and checked when their copy has landed -- at the next _sample call or by sampler_failures() -- so that
# sampling never waits for the device
_pending_flags = []


def _check_sampler_flag(wait: bool = False):
    keep = []
    bad = False
    for ev, host, flag in _pending_flags:
        if wait:
            ev.synchronize()
        if ev.query():
            bad = bad or bool(int(host[0]))
        else:
            keep.append((ev, host, flag))
    _pending_flags[:] = keep
    if bad:
        raise RuntimeError("MatrixFisherN._sample: a rejection loop exhausted its 4096 proposals in an earlier call (utils/fisher.py:117-207 "
                           "oversamples 8x and retries; here the slot was left at the identity rotation) -- the parameter matrix is far outside "
                           "the range the ACG envelope covers")


def sampler_failures(wait: bool = True):
    """Raise if any earlier ``MatrixFisherN._sample`` call reported an exhausted rejection loop (waits for outstanding calls by default)."""
    _check_sampler_flag(wait)


class MatrixFisherN(torch.nn.Module):
    """MatrixFisherN(A [B,3,3], norm_type=1).  ``_log_prob(R [N,3,3])`` broadcasts row b over N/B consecutive samples."""

    def __init__(self, A, norm_type=1, approx_num=None):
        super().__init__()
        if isinstance(norm_type, str) and norm_type == "exact":
            # the exact normaliser, per row from the quadrature kernel; the C ABI knows it as RNF_FISHER_NORM_EXACT
            self.norm_type, self._nt = "exact", _lib.FISHER_NORM_EXACT
            self.A = A.reshape(-1, 3, 3)
            self._c = device_fisher_exact(self.A, "c")
            self._norm = None
            return
        if isinstance(norm_type, str) or norm_type not in (0, 1, 2):
            raise NotImplementedError("normaliser approximations 0, 1 (closed forms) and 2 (Monte-Carlo) are built; type 3 indexes ROWS of the "
                                      "[N,3] singular values and cannot serve MatrixFisherN's batched A (utils/fisher.py:102-113) -- "
                                      'norm_type="exact" evaluates the same integral per row')
        self.norm_type = self._nt = int(norm_type)
        self.A = A.reshape(-1, 3, 3)
        if self.norm_type == 2:
            # utils/fisher.py:98-101: mean over approx_num uniform rotations, ONE matrix (the reference's broadcast); on the device with
            # a Philox stream keyed from torch's generator (statistical parity with pytorch3d.random_rotations)
            if approx_num is None or int(approx_num) <= 0:
                raise TypeError("norm_type=2 needs approx_num (the reference passes it to random_rotations, utils/fisher.py:99)")
            if self.A.shape[0] != 1:
                raise RuntimeError("norm_type=2 serves one matrix: the reference broadcasts [approx_num,3,3] against [N,3,3] (utils/fisher.py:100)")
            if not self.A.is_cuda:
                raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback): construct MatrixFisherN with A on the GPU")
            A32 = self.A.detach().to(torch.float32).contiguous()
            self._c = torch.empty(1, dtype=torch.float32, device=A32.device)
            scratch = torch.empty(1, dtype=torch.float64, device=A32.device)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            with torch.cuda.device(A32.device):
                _lib.check(_lib.lib().rnf_fisher_log_const_mc(A32.data_ptr(), 1, int(approx_num), seed, scratch.data_ptr(), 8, self._c.data_ptr(),
                                                              torch.cuda.current_stream(A32.device).cuda_stream))
            self._norm = None
            return
        if self.A.is_cuda:
            # per-sample A from a network (agent.py:57-60): constants on the device, no host SVD and no device->host sync
            A32 = self.A.detach().to(torch.float32).contiguous()
            L = _lib.lib()
            self._c = torch.empty(A32.shape[0], dtype=torch.float32, device=A32.device)
            scratch = torch.empty(2, dtype=torch.float64, device=A32.device)
            with torch.cuda.device(A32.device):
                _lib.check(L.rnf_fisher_log_const_nt(A32.data_ptr(), A32.shape[0], self.norm_type, scratch.data_ptr(), 16, self._c.data_ptr(),
                                                     torch.cuda.current_stream(A32.device).cuda_stream))
            self._norm = None
        else:
            S = proper_singular_values(self.A)
            norm = _norm_from_singular_values(S, self.norm_type)
            self._norm = norm.to(dtype=self.A.dtype)
            self._c = (S.sum(-1) + norm.log()).to(torch.float32)      # log p = tr(A^T R) - c

    @property
    def norm(self):
        """The reference's ``self.norm`` (utils/fisher.py:215); computed lazily when A lives on the GPU (needs the singular values)."""
        if self._norm is None:
            S = proper_singular_values(self.A)
            if self.norm_type in (2, "exact"):               # c = sum S + log norm
                self._norm = (self._c.detach().to(S.device, torch.float64) - S.sum(-1)).exp().to(device=self.A.device, dtype=self.A.dtype)
            else:
                self._norm = _norm_from_singular_values(S, self.norm_type).to(device=self.A.device, dtype=self.A.dtype)
        return self._norm

    def log_const(self):
        return self._c

    def _log_prob(self, inputs, context=9):
        if not inputs.is_cuda:
            raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
        if self.norm_type == 2 and torch.is_grad_enabled() and self.A.requires_grad:
            raise NotImplementedError("rotationnormflow_amd: no gradient w.r.t. A through the Monte-Carlo normaliser (norm_type=2); use 0 or 1")
        if inputs.shape[-1] == 4:
            if torch.is_grad_enabled() and inputs.requires_grad:
                raise NotImplementedError("rotationnormflow_amd: quaternion inputs are not differentiable here; pass rotation matrices")
            inputs = quaternion_to_matrix(inputs)
        dev = inputs.device
        A = self.A.detach().to(device=dev, dtype=torch.float32).contiguous()
        c = self._c.to(dev).contiguous()
        return _FisherLogProb.apply(inputs, self.A, A, c, self._nt)

    @classmethod
    def fit(cls, rotations, log_weights=None, norm_type="exact", max_concentration=1e4):
        """The maximum-likelihood MatrixFisherN of rotations on the device: ``rotations`` [n,3,3] (one distribution), [G,n,3,3] (G of
        them), or [n,3,3] with ``log_weights`` [G,n] (G weightings of one set, e.g. a grid and each image's log-density on it; the
        weights are softmax(log_weights) per row).  Moments in fp64 (``rotation_moments``), then ``fit_matrix_fisher``: the A whose mean
        rotation under the exact normaliser is the sample moment.  The fitted model is always the exact one (``norm_type`` other than
        "exact" is refused).  ``fit_status`` [G] int32 on the device (bits as ``fit_matrix_fisher``), ``fit_s`` and ``fit_iterations``
        are attached; nothing here waits for the device, reading ``fit_status`` on the host does.  Not differentiable."""
        if norm_type != "exact":
            raise NotImplementedError('MatrixFisherN.fit: the fitted model is the exact one (norm_type="exact"); the closed-form normalisers '
                                      "0 / 1 and the Monte-Carlo 2 have other maximisers")
        fit = fit_matrix_fisher(rotation_moments(rotations, log_weights), max_concentration)
        out = cls(fit["A"], "exact")
        out.fit_status, out.fit_s, out.fit_iterations = fit["status"], fit["s"], fit["iterations"]
        return out

    def mean_rotation(self):
        """E[R] = dc/dA of MF(A[b]), [B,3,3] fp32: always from the exact kernel, whatever this instance's norm_type.  Not differentiable."""
        return device_fisher_exact(self.A, "mean")

    def entropy(self):
        """The differential entropy c - tr(A^T E[R]) of MF(A[b]) w.r.t. the Haar probability measure, [B] fp32 (<= 0, 0 at A = 0): always
        with the exact normaliser, summed in fp64 on the device.  Not differentiable."""
        return device_fisher_exact(self.A, "entropy")

    def log_prob(self, inputs, context=None):
        return self._log_prob(inputs)

    def _sample(self, num_samples, context=9):
        """[B, num_samples, 3, 3] rotations (context=9) or quaternions (context=4) ~ MF(A) on A's device.  Exact rejection
        sampler (Bingham through an ACG envelope, utils/fisher.py:117-207) on the GPU with a counter-based Philox stream whose
        key is drawn from torch's default generator, so ``torch.manual_seed`` makes it reproducible."""
        A = self.A
        if not A.is_cuda:
            raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback): construct MatrixFisherN with A on the GPU")
        dev = A.device
        U32, V32, _, lam32 = device_proper_svd(A)            # proper SVD + Bingham parameters on the device: no host LAPACK, no sync
        B = A.shape[0]
        out = torch.empty(B, num_samples, 3, 3, dtype=torch.float32, device=dev)
        _check_sampler_flag()                                # a failure of an EARLIER call surfaces here, without a device wait now
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rnf_fisher_sample(U32.data_ptr(), V32.data_ptr(), lam32.data_ptr(), B, num_samples, seed,
                                                    out.data_ptr(), flag.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            if not torch.cuda.is_current_stream_capturing():
                host = torch.zeros(1, dtype=torch.int32).pin_memory()
                host.copy_(flag, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                _pending_flags.append((ev, host, flag))
        if context == 9:
            return out
        if context == 4:                                     # utils/fisher.py:242-243: matrix_to_quaternion(result)
            quat = torch.empty(B, num_samples, 4, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().rnf_matrix_to_quaternion(out.data_ptr(), B * num_samples, quat.data_ptr(),
                                                               torch.cuda.current_stream(dev).cuda_stream))
            return quat
        return None

    def sample(self, num_samples, context=None):
        return self._sample(num_samples)


# ---- the reference's module-level helpers under their own names (utils/fisher.py:14-207) -----------------------------------------------
# MatrixFisherN above never calls these (it goes to the kernels directly); they exist so that code written against the reference's module
# finds the same names with the same argument meaning.  GPU tensors go through the device kernels; the SVD helpers also accept host tensors
# (torch's LAPACK, as the reference itself does) because they are plain linear algebra, not part of the density path.

def quat_to_rotmat(quat):
    """[B,4] (w, x, y, z), normalised first -> [B,3,3] (utils/fisher.py:14-46)."""
    return quaternion_to_matrix(quat)


def proper_svd_N(A):
    """[N,3,3] -> (U, S, V) with det(U) = det(V) = +1 and the last singular value carrying the sign (utils/fisher.py:67-76)."""
    A = A.reshape(-1, 3, 3)
    if A.is_cuda:
        U, V, s, _ = device_proper_svd(A)
        return U.to(A.dtype), s.to(A.dtype), V.to(A.dtype)
    U, S, Vh = torch.linalg.svd(A.detach())
    V = Vh.transpose(-1, -2).clone()
    U, S = U.clone(), S.clone()
    du, dv = torch.det(U), torch.det(V)
    U[:, :, 2] *= du[:, None]
    V[:, :, 2] *= dv[:, None]
    S[:, 2] *= du * dv
    return U, S, V


def proper_svd(A, clone=False):
    """One [3,3] matrix -> (U [3,3], S [3], V [3,3]) (utils/fisher.py:48-64; `clone` is accepted and has no effect: nothing aliases A here)."""
    U, S, V = proper_svd_N(A.reshape(1, 3, 3))
    return U[0], S[0], V[0]


def matrix_fisher_norm_N(A, type_approx=0, approx_num=17890714):
    """The approximated normalising constant of MF(A), A [N,3,3] -> [N] (utils/fisher.py:79-115): type 0 / 1 closed forms (type 0 keeps
    the reference's batch-global ``(S**2).sum()``), type 2 Monte-Carlo over `approx_num` uniform rotations (ONE matrix, on the GPU).
    Type 3 is refused, see MatrixFisherN; "exact" is the exact normaliser per row (on the GPU)."""
    A = A.reshape(-1, 3, 3)
    if isinstance(type_approx, str) and type_approx == "exact":
        return MatrixFisherN(A, "exact").norm
    if type_approx in (0, 1):
        S = proper_svd_N(A)[1] if A.is_cuda else proper_singular_values(A).to(A.dtype)
        return _norm_from_singular_values(S, type_approx)
    if type_approx == 2:
        return MatrixFisherN(A, 2, approx_num).norm
    raise NotImplementedError('matrix_fisher_norm_N: type_approx 0, 1, 2 and "exact" are built (type 3 serves no batch: use "exact")')


def sample_matrix_fisher(A, num_samples, b=1.5, oversampling_ratio=8):
    """[num_samples,3,3] rotations ~ MF(A) for ONE [3,3] matrix on the GPU (utils/fisher.py:175-207).  The device sampler is an exact
    per-sample rejection loop with the reference's envelope (b = 1.5): `oversampling_ratio` has nothing to size here, other `b` are refused."""
    if float(b) != 1.5:
        raise NotImplementedError("sample_matrix_fisher: the device sampler is built for the reference's envelope parameter b = 1.5")
    return MatrixFisherN(A.reshape(1, 3, 3))._sample(num_samples)[0]
