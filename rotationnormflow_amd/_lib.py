"""ctypes binding of librnf_hip.so (include/rnf_hip.h).  There is no fallback: if the HIP library has not been built
the import of any op fails loudly (build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``python -m rotationnormflow_amd.build``)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librnf_hip.so")

_lib = None
ABI_VERSION = 8
PREC_FP32, PREC_F16X2, PREC_BF16X3 = 0, 1, 2
FISHER_NORM_EXACT = 3   # RNF_FISHER_NORM_EXACT

c_f32p = C.c_void_p      # device or host float*, passed as integer addresses
c_i32p = C.c_void_p


class _Pass(C.Structure):
    """A struct whose first field is its own size (struct_bytes), filled in on construction; unnamed fields are zero / NULL."""

    def __init__(self, **fields):
        super().__init__(struct_bytes=C.sizeof(self), **fields)


class FlowPass(_Pass):
    """RnfFlowPass (include/rnf_hip.h): one pass through a packed flow."""
    _fields_ = [("struct_bytes", C.c_size_t), ("dir", C.c_int32), ("feature_dim", C.c_int32), ("rotation", C.c_void_p),
                ("feature", C.c_void_p), ("n", C.c_int64), ("feature_div", C.c_int64), ("side", C.c_void_p), ("blob", C.c_void_p),
                ("desc", C.c_void_p), ("n_layers", C.c_int32), ("segments", C.c_int32), ("fisher_A", C.c_void_p), ("fisher_c", C.c_void_p),
                ("fisher_B", C.c_int64), ("rotation_out", C.c_void_p), ("ldj_out", C.c_void_p), ("logp_out", C.c_void_p),
                ("sum_out", C.c_void_p), ("states", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class FlowBackward(_Pass):
    """RnfFlowBackward (include/rnf_hip.h): the reverse sweep of a training pass."""
    _fields_ = [("struct_bytes", C.c_size_t), ("dir", C.c_int32), ("feature_dim", C.c_int32), ("states", C.c_void_p),
                ("rotation_out", C.c_void_p), ("feature", C.c_void_p), ("n", C.c_int64), ("plain", C.c_void_p), ("train_desc", C.c_void_p),
                ("n_layers", C.c_int32), ("segments", C.c_int32), ("acts", C.c_void_p), ("side", C.c_void_p), ("side_grad", C.c_void_p),
                ("g_rotation_out", C.c_void_p), ("g_ldj", C.c_void_p), ("grads", C.c_void_p), ("g_rotation_in", C.c_void_p),
                ("g_feature", C.c_void_p), ("layer_scratch", C.c_void_p), ("stream", C.c_void_p)]


class GridModes(_Pass):
    """RnfGridModes (include/rnf_hip.h): top-k pose modes and their mass on an SO(3) grid."""
    _fields_ = [("struct_bytes", C.c_size_t), ("logp", C.c_void_p), ("grid", C.c_void_p), ("Q", C.c_int64), ("g", C.c_int32),
                ("top_k", C.c_int32), ("separation_rad", C.c_double), ("gt", C.c_void_p), ("n_gt", C.c_int32), ("index_out", C.c_void_p),
                ("logp_out", C.c_void_p), ("mass_out", C.c_void_p), ("log_norm_out", C.c_void_p), ("spread_out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class GridCredible(_Pass):
    """RnfGridCredible (include/rnf_hip.h): highest-density credible sets and HPD levels on an SO(3) grid."""
    _fields_ = [("struct_bytes", C.c_size_t), ("logp", C.c_void_p), ("Q", C.c_int64), ("g", C.c_int32), ("levels", C.c_void_p),
                ("n_levels", C.c_int32), ("queries", C.c_void_p), ("n_queries", C.c_int32), ("threshold_out", C.c_void_p),
                ("count_out", C.c_void_p), ("mass_out", C.c_void_p), ("log_norm_out", C.c_void_p), ("query_mass_out", C.c_void_p),
                ("query_count_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class GridLocate(_Pass):
    """RnfGridLocate (include/rnf_hip.h): the grid cell of rotations, and their histogram over the cells."""
    _fields_ = [("struct_bytes", C.c_size_t), ("level", C.c_int32), ("rotations", C.c_void_p), ("n", C.c_int64), ("g", C.c_int32),
                ("offset", C.c_void_p), ("rows_out", C.c_void_p), ("counts", C.c_void_p), ("stream", C.c_void_p)]


class GridFit(_Pass):
    """RnfGridFit (include/rnf_hip.h): how well histograms over the grid's cells fit densities on the grid."""
    _fields_ = [("struct_bytes", C.c_size_t), ("logp", C.c_void_p), ("counts", C.c_void_p), ("Q", C.c_int64), ("g", C.c_int32),
                ("stats_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class GridCellPoints(_Pass):
    """RnfGridCellPoints (include/rnf_hip.h): the chart of SO(3) grid cells, from (row, u in [0,1]^3) to a rotation inside the cell."""
    _fields_ = [("struct_bytes", C.c_size_t), ("level", C.c_int32), ("offset", C.c_void_p), ("rows", C.c_void_p), ("u", C.c_void_p),
                ("n", C.c_int64), ("rot_out", C.c_void_p), ("stream", C.c_void_p)]


class GridSample(_Pass):
    """RnfGridSample (include/rnf_hip.h): draws of grid rows, and of rotations inside their cells, from posteriors on the grid."""
    _fields_ = [("struct_bytes", C.c_size_t), ("logp", C.c_void_p), ("Q", C.c_int64), ("g", C.c_int32), ("level", C.c_int32),
                ("draws", C.c_int64), ("draw_base", C.c_int64), ("draws_total", C.c_int64), ("image_base", C.c_int64), ("method", C.c_int32),
                ("jitter", C.c_int32), ("seed", C.c_uint64), ("offset", C.c_void_p), ("index_out", C.c_void_p), ("target_out", C.c_void_p),
                ("total_out", C.c_void_p), ("rot_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


GRID_SAMPLE_METHODS = {"multinomial": 0, "systematic": 1}   # RNF_GRID_SAMPLE_*


class So3KernelSum(_Pass):
    """RnfSo3KernelSum (include/rnf_hip.h): pairwise sums of matrix-Fisher kernels between two sets of rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("centres", C.c_void_p), ("queries", C.c_void_p), ("log_weights", C.c_void_p), ("n", C.c_int64),
                ("m", C.c_int64), ("G", C.c_int32), ("kappas", C.c_void_p), ("J", C.c_int32), ("leave_one_out", C.c_int32), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class So3KernelMoments(_Pass):
    """RnfSo3KernelMoments (include/rnf_hip.h): responsibility-weighted first moments of the same kernel sum."""
    _fields_ = [("struct_bytes", C.c_size_t), ("centres", C.c_void_p), ("queries", C.c_void_p), ("log_weights", C.c_void_p), ("n", C.c_int64),
                ("m", C.c_int64), ("G", C.c_int32), ("group_queries", C.c_int32), ("kappa", C.c_double), ("log_density", C.c_void_p),
                ("mean", C.c_void_p), ("msd", C.c_void_p), ("rotation", C.c_void_p), ("step", C.c_void_p), ("dlog_normaliser", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class So3AngleCdf(_Pass):
    """RnfSo3AngleCdf (include/rnf_hip.h): the distribution function of the geodesic angle from queries to weighted rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("centres", C.c_void_p), ("queries", C.c_void_p), ("log_weights", C.c_void_p), ("n", C.c_int64),
                ("m", C.c_int64), ("G", C.c_int32), ("group_queries", C.c_int32), ("T", C.c_int32), ("thresholds", C.c_void_p),
                ("query_tau", C.c_void_p), ("mass", C.c_void_p), ("mean_angle", C.c_void_p), ("mean_sq_angle", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class So3SetAngleCdf(_Pass):
    """RnfSo3SetAngleCdf (include/rnf_hip.h): the distribution function of the angle to the nearest member of sets of rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("centres", C.c_void_p), ("queries", C.c_void_p), ("log_weights", C.c_void_p), ("n", C.c_int64),
                ("m", C.c_int64), ("K", C.c_int32), ("G", C.c_int32), ("group_queries", C.c_int32), ("T", C.c_int32),
                ("thresholds", C.c_void_p), ("query_tau", C.c_void_p), ("mass", C.c_void_p), ("mean_angle", C.c_void_p),
                ("mean_sq_angle", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class So3GridLocalSum(_Pass):
    """RnfSo3GridLocalSum (include/rnf_hip.h): neighbour-limited sums of matrix-Fisher kernels over the rows of the SO(3) grid."""
    _fields_ = [("struct_bytes", C.c_size_t), ("level", C.c_int32), ("offset", C.c_void_p), ("grid", C.c_void_p), ("queries", C.c_void_p),
                ("log_weights", C.c_void_p), ("m", C.c_int64), ("G", C.c_int32), ("kappa", C.c_double), ("d2_cut", C.c_double),
                ("out", C.c_void_p), ("count", C.c_void_p), ("stream", C.c_void_p)]


class So3GridLocalMax(_Pass):
    """RnfSo3GridLocalMax (include/rnf_hip.h): the max-plus pass with its arg-max over the same neighbourhoods."""
    _fields_ = [("struct_bytes", C.c_size_t), ("level", C.c_int32), ("offset", C.c_void_p), ("grid", C.c_void_p), ("queries", C.c_void_p),
                ("log_weights", C.c_void_p), ("m", C.c_int64), ("G", C.c_int32), ("kappa", C.c_double), ("d2_cut", C.c_double),
                ("out", C.c_void_p), ("arg", C.c_void_p), ("count", C.c_void_p), ("stream", C.c_void_p)]


class So3GridLocalFisher(_Pass):
    """RnfSo3GridLocalFisher (include/rnf_hip.h): the two neighbour-limited passes on an anisotropic matrix-Fisher kernel."""
    _fields_ = [("struct_bytes", C.c_size_t), ("level", C.c_int32), ("offset", C.c_void_p), ("grid", C.c_void_p), ("queries", C.c_void_p),
                ("log_weights", C.c_void_p), ("m", C.c_int64), ("G", C.c_int32), ("concentration", C.c_double * 9), ("d2_cut", C.c_double),
                ("out", C.c_void_p), ("arg", C.c_void_p), ("count", C.c_void_p), ("stream", C.c_void_p)]


class So3Wigner(_Pass):
    """RnfSo3Wigner (include/rnf_hip.h): the real Wigner matrices of rotations, degrees 0..lmax."""
    _fields_ = [("struct_bytes", C.c_size_t), ("rotations", C.c_void_p), ("n", C.c_int64), ("lmax", C.c_int32), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class So3Fourier(_Pass):
    """RnfSo3Fourier (include/rnf_hip.h): the SO(3) Fourier coefficients of weighted rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("centres", C.c_void_p), ("log_weights", C.c_void_p), ("n", C.c_int64), ("G", C.c_int32),
                ("lmax", C.c_int32), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class So3FourierEval(_Pass):
    """RnfSo3FourierEval (include/rnf_hip.h): a band-limited function on SO(3) at query rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("coeffs", C.c_void_p), ("queries", C.c_void_p), ("m", C.c_int64), ("G", C.c_int32),
                ("group_queries", C.c_int32), ("lmax", C.c_int32), ("out", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


SO3_MAX_DEGREE = 16   # RNF_SO3_MAX_DEGREE

GRID_FIT_STATS =("log_norm", "log_likelihood", "grid_log_likelihood", "g_stat", "chi2", "n", "occupied")   # RNF_GRID_FIT_*


class GridChildren(_Pass):
    """RnfGridChildren (include/rnf_hip.h): the 12 children of SO(3) grid rows one level down, and their rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("level", C.c_int32), ("parents", C.c_void_p), ("n", C.c_int64), ("offset", C.c_void_p),
                ("rows_out", C.c_void_p), ("rot_out", C.c_void_p), ("stream", C.c_void_p)]


class GridBeamSelect(_Pass):
    """RnfGridBeamSelect (include/rnf_hip.h): the best distinct rows per image of the beam search."""
    _fields_ = [("struct_bytes", C.c_size_t), ("logp", C.c_void_p), ("rows", C.c_void_p), ("M", C.c_int64), ("g", C.c_int32),
                ("beam", C.c_int32), ("rows_out", C.c_void_p), ("logp_out", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class RotationMoments(_Pass):
    """RnfRotationMoments (include/rnf_hip.h): fp64 weighted moments of groups of rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("rotations", C.c_void_p), ("log_weights", C.c_void_p), ("n", C.c_int64), ("G", C.c_int64),
                ("shared_rotations", C.c_int32), ("moments_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class FisherFit(_Pass):
    """RnfFisherFit (include/rnf_hip.h): the maximum-likelihood matrix-Fisher parameter of moment matrices."""
    _fields_ = [("struct_bytes", C.c_size_t), ("moments", C.c_void_p), ("B", C.c_int64), ("max_concentration", C.c_double),
                ("max_iterations", C.c_int32), ("A_out", C.c_void_p), ("s_out", C.c_void_p), ("hessian_out", C.c_void_p),
                ("iterations_out", C.c_void_p), ("status_out", C.c_void_p), ("stream", C.c_void_p)]


class FisherMixtureFit(_Pass):
    """RnfFisherMixtureFit (include/rnf_hip.h): EM for mixtures of matrix-Fishers, per group of rotations."""
    _fields_ = [("struct_bytes", C.c_size_t), ("rotations", C.c_void_p), ("log_weights", C.c_void_p), ("n", C.c_int64), ("G", C.c_int64),
                ("shared_rotations", C.c_int32), ("K", C.c_int32), ("A_init", C.c_void_p), ("log_pi_init", C.c_void_p),
                ("iterations", C.c_int32), ("tol", C.c_double), ("max_concentration", C.c_double), ("A_out", C.c_void_p),
                ("log_pi_out", C.c_void_p), ("s_out", C.c_void_p), ("loglik_out", C.c_void_p), ("weight_entropy_out", C.c_void_p),
                ("log_resp_out", C.c_void_p), ("status_out", C.c_void_p), ("iterations_out", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


FIT_CAPPED, FIT_NOT_CONVERGED, FIT_INPUT = 1, 2, 4   # RNF_FIT_*

_SIGNATURES = {
    "rnf_abi_version": (C.c_int, []),
    "rnf_last_error": (C.c_char_p, []),
    "rnf_last_pack_audit": (C.c_double, []),
    "rnf_set_equalize": (C.c_int, [C.c_int]),
    "rnf_set_feature_ms": (C.c_double, [C.c_double]),
    "rnf_set_pack_audit": (C.c_int, [C.c_int]),
    "rnf_set_fused": (C.c_int, [C.c_int]),
    "rnf_set_train_block": (C.c_int, [C.c_int]),
    "rnf_mobius_packed_floats": (C.c_int64, [C.c_int32]),
    "rnf_mobius_packed_floats_prec": (C.c_int64, [C.c_int32, C.c_int32]),
    "rnf_cond_packed_floats_prec": (C.c_int64, [C.c_int32, C.c_int32]),
    "rnf_affine16_packed_floats": (C.c_int64, []),
    "rnf_cond16_packed_floats": (C.c_int64, []),
    "rnf_featproj_packed_floats": (C.c_int64, [C.c_int32]),
    "rnf_pack_mobius": (C.c_int, [c_f32p] * 10 + [C.c_int32, C.c_int32, C.c_int32, c_f32p, c_f32p]),
    "rnf_pack_affine16": (C.c_int, [c_f32p, c_f32p]),
    "rnf_pack_rot16": (C.c_int, [c_f32p, c_f32p]),
    "rnf_gs_packed_floats": (C.c_int64, [C.c_int32]),
    "rnf_pack_gs": (C.c_int, [c_f32p, C.c_int32, c_f32p]),
    "rnf_pack_cond16": (C.c_int, [c_f32p] * 10 + [C.c_int32, C.c_int32, c_f32p, c_f32p]),
    "rnf_pack_cond9": (C.c_int, [c_f32p] * 10 + [C.c_int32, C.c_int32, c_f32p, c_f32p]),
    "rnf_cond36_packed_floats": (C.c_int64, []),
    "rnf_pack_cond36": (C.c_int, [c_f32p] * 10 + [C.c_int32, C.c_int32, c_f32p, c_f32p]),
    "rnf_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "rnf_flow_pass": (C.c_int, [C.POINTER(FlowPass)]),
    "rnf_flow_pass_workspace_bytes": (C.c_size_t, [C.POINTER(FlowPass)]),
    "rnf_flow_backward_pass": (C.c_int, [C.POINTER(FlowBackward)]),
    "rnf_cond_mlp_forward": (C.c_int, [c_f32p, C.c_int64, C.c_int32, c_f32p, C.c_int32, C.c_int32, C.c_int32, c_f32p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "rnf_condrot_matrices": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_void_p, C.c_void_p]),
    "rnf_condrot_svd": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p]),
    "rnf_condlu_matrices": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, c_f32p, C.c_int32, c_f32p,
                                      C.c_void_p]),
    "rnf_condlu_backward": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, c_f32p, c_f32p, c_f32p, c_f32p,
                                      c_f32p, c_f32p, C.c_void_p]),
    "rnf_pack_flow_device": (C.c_int, [c_f32p, c_i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_f32p, c_i32p, C.c_void_p]),
    "rnf_plain_layer_floats": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rnf_flow_forward_train_plain": (C.c_int, [c_f32p, c_f32p, C.c_int64, C.c_int32, c_f32p, c_i32p, C.c_int32, C.c_int32,
                                               c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "rnf_train_acts_floats": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "rnf_fisher_log_prob": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    "rnf_min_geodesic": (C.c_int, [c_f32p, c_f32p, C.c_int64, C.c_int32, c_f32p, C.c_void_p]),
    "rnf_so3_healpix_grid": (C.c_int, [C.c_int32, c_f32p, c_f32p, C.c_void_p]),
    "rnf_grid_modes": (C.c_int, [C.POINTER(GridModes)]),
    "rnf_grid_modes_workspace_bytes": (C.c_size_t, [C.POINTER(GridModes)]),
    "rnf_grid_credible": (C.c_int, [C.POINTER(GridCredible)]),
    "rnf_grid_credible_workspace_bytes": (C.c_size_t, [C.POINTER(GridCredible)]),
    "rnf_so3_grid_children": (C.c_int, [C.POINTER(GridChildren)]),
    "rnf_so3_grid_locate": (C.c_int, [C.POINTER(GridLocate)]),
    "rnf_grid_fit": (C.c_int, [C.POINTER(GridFit)]),
    "rnf_grid_fit_workspace_bytes": (C.c_size_t, [C.POINTER(GridFit)]),
    "rnf_so3_grid_cell_points": (C.c_int, [C.POINTER(GridCellPoints)]),
    "rnf_grid_sample": (C.c_int, [C.POINTER(GridSample)]),
    "rnf_grid_sample_workspace_bytes": (C.c_size_t, [C.POINTER(GridSample)]),
    "rnf_so3_kernel_sum": (C.c_int, [C.POINTER(So3KernelSum)]),
    "rnf_so3_kernel_sum_workspace_bytes": (C.c_size_t, [C.POINTER(So3KernelSum)]),
    "rnf_so3_kernel_moments": (C.c_int, [C.POINTER(So3KernelMoments)]),
    "rnf_so3_kernel_moments_workspace_bytes": (C.c_size_t, [C.POINTER(So3KernelMoments)]),
    "rnf_so3_angle_cdf": (C.c_int, [C.POINTER(So3AngleCdf)]),
    "rnf_so3_angle_cdf_workspace_bytes": (C.c_size_t, [C.POINTER(So3AngleCdf)]),
    "rnf_so3_set_angle_cdf": (C.c_int, [C.POINTER(So3SetAngleCdf)]),
    "rnf_so3_set_angle_cdf_workspace_bytes": (C.c_size_t, [C.POINTER(So3SetAngleCdf)]),
    "rnf_so3_grid_local_sum": (C.c_int, [C.POINTER(So3GridLocalSum)]),
    "rnf_so3_grid_local_max": (C.c_int, [C.POINTER(So3GridLocalMax)]),
    "rnf_so3_grid_local_fisher": (C.c_int, [C.POINTER(So3GridLocalFisher)]),
    "rnf_so3_wigner": (C.c_int, [C.POINTER(So3Wigner)]),
    "rnf_so3_wigner_workspace_bytes": (C.c_size_t, [C.POINTER(So3Wigner)]),
    "rnf_so3_fourier": (C.c_int, [C.POINTER(So3Fourier)]),
    "rnf_so3_fourier_workspace_bytes": (C.c_size_t, [C.POINTER(So3Fourier)]),
    "rnf_so3_fourier_eval": (C.c_int, [C.POINTER(So3FourierEval)]),
    "rnf_so3_fourier_eval_workspace_bytes": (C.c_size_t, [C.POINTER(So3FourierEval)]),
    "rnf_grid_beam_select": (C.c_int, [C.POINTER(GridBeamSelect)]),
    "rnf_grid_beam_select_workspace_bytes": (C.c_size_t, [C.POINTER(GridBeamSelect)]),
    "rnf_fisher_log_const": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    "rnf_fisher_proper_svd": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "rnf_fisher_log_prob_backward": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    "rnf_cond_mlp_backward": (C.c_int, [c_f32p, C.c_int64, C.c_int32, c_f32p, C.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "rnf_matrix_to_quaternion": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    "rnf_fisher_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "rnf_fisher_log_const_mc": (C.c_int, [c_f32p, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p, C.c_size_t, c_f32p, C.c_void_p]),
    "rnf_fisher_log_const_nt": (C.c_int, [c_f32p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, c_f32p, C.c_void_p]),
    "rnf_fisher_exact": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_void_p]),
    "rnf_fisher_entropy": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    "rnf_rotation_moments": (C.c_int, [C.POINTER(RotationMoments)]),
    "rnf_rotation_moments_workspace_bytes": (C.c_size_t, [C.POINTER(RotationMoments)]),
    "rnf_fisher_fit": (C.c_int, [C.POINTER(FisherFit)]),
    "rnf_fisher_mixture_fit": (C.c_int, [C.POINTER(FisherMixtureFit)]),
    "rnf_fisher_mixture_fit_workspace_bytes": (C.c_size_t, [C.POINTER(FisherMixtureFit)]),
    "rnf_fisher_mixture_log_prob": (C.c_int, [c_f32p, C.c_void_p, C.c_int32, c_f32p, C.c_int64, c_f32p, c_f32p, C.c_void_p]),
    "rnf_fisher_log_prob_backward_param": (C.c_int, [c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, c_f32p,
                                                  C.c_void_p]),
    "rnf_fisher_sample": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int64, C.c_uint64, c_f32p, C.c_void_p, C.c_void_p]),
    "rnf_conditioner_forward": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int32, C.c_int32, c_f32p, C.c_void_p]),
}

EXPORTS = tuple(_SIGNATURES)


def load(path):
    """Load one build of the library and bind every export (tools/ab_variants.py loads several builds side by side)."""
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the MI355X HIP library has not been built and there is no CPU fallback. "
            "Run `python -m rotationnormflow_amd.build` (needs hipcc).")
    # torch first: it maps its own HIP runtime (libamdhip64.so.7 under torch/lib), which the dynamic loader then also binds this library to.
    # Loaded the other way round (e.g. build() and smoke() in ONE process) the library would pull the system's runtime from /opt/rocm and the
    # process would hold two HIP runtimes, of which only torch's has the device open ("no ROCm-capable device is detected" in ours).
    import torch  # noqa: F401
    handle = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.rnf_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version mismatch; rebuild")
    return handle


def lib():
    """The loaded library (loads on first use)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def check(rc: int):
    if rc != 0:
        raise RuntimeError("librnf_hip: " + lib().rnf_last_error().decode())


def call(name: str, args, device):
    """Run the struct entry point ``rnf_<name>`` on ``args`` (a ``_Pass``) on ``device``'s current stream.  Where the library exports
    ``rnf_<name>_workspace_bytes`` the workspace is asked for (0: the arguments were refused, ``rnf_last_error`` says why), allocated for the
    duration of the call -- the caching allocator's blocks are 512-byte aligned -- and entered into ``args``."""
    import torch
    L = lib()
    if f"rnf_{name}_workspace_bytes" in _SIGNATURES:
        need = getattr(L, f"rnf_{name}_workspace_bytes")(C.byref(args))
        if need == 0:
            check(1)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        args.workspace, args.workspace_bytes = ws.data_ptr(), need
    with torch.cuda.device(device):
        args.stream = torch.cuda.current_stream(device).cuda_stream
        check(getattr(L, "rnf_" + name)(C.byref(args)))
