"""ctypes binding of libdragposer_hip.so (the C ABI declared in include/dragposer.h).

There is no fallback: if the shared library is missing or cannot be loaded this module raises,
and every product entry point built on it fails loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libdragposer_hip.so")  # (the product reads no environment variable; diagnostic tools pass their build's
                                                              #  path explicitly: bench.py --lib, tools/_diaglib.py)

DP_OK = 0
DP_ERR_INVALID = -1
DP_ERR_DEVICE = -2
DP_ERR_UNSUPPORTED = -3
DP_ERR_LAUNCH = -4
DP_ERR_TIMEOUT = -5
DP_WEIGHTS_FP32 = 0
DP_WEIGHTS_BF16 = 1
DP_MAX_ITERS = 1000000
DP_KERNEL_AUTO, DP_KERNEL_W4, DP_KERNEL_W16 = 0, 1, 2

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int)
_u8 = C.POINTER(C.c_ubyte)


class DpModel(C.Structure):
    _fields_ = [
        ("f_latent_w", _f), ("f_latent_b", _f),
        ("unpool_w", _f * 3), ("conv_w", _f * 3), ("conv_mask", _f * 3), ("conv_b", _f * 3),
        ("mean_q", _f), ("std_q", _f), ("mean_disp", _f), ("std_disp", _f),
        ("parents", _i), ("offsets", _f), ("weight_dtype", C.c_int),
    ]


class DpFolded(C.Structure):
    _fields_ = [
        ("A0", C.c_float * (40 * 24)), ("c0", C.c_float * 40),
        ("A1", C.c_float * (60 * 40)), ("b1", C.c_float * 60),
        ("A2", C.c_float * (92 * 60)), ("b2", C.c_float * 92),
    ]


class DpBatch(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int),
        ("z0", C.c_void_p), ("z_tgt", C.c_void_p), ("cur_rot", C.c_void_p), ("tgt_pos", C.c_void_p),
        ("tgt_rot", C.c_void_p), ("w", C.c_void_p), ("tracked", C.c_void_p),
    ]


class _Sized(C.Structure):
    """dp_params / dp_result start with struct_size = sizeof the struct as THIS binding declares it (include/dragposer.h, 0.5.0)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(type(self))


class DpParams(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint), ("n_iter", C.c_int), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("lambda_rot", C.c_float), ("lambda_tmp", C.c_float), ("early_stop", C.c_int),
        ("stop_eps_pos", C.c_float), ("stop_eps_rot", C.c_float), ("min_loss_incr", C.c_float), ("max_trackers", C.c_int),
        ("kernel", C.c_int),
    ]


class DpSeqState(C.Structure):
    _fields_ = [
        ("global_pos", C.c_void_p), ("global_rot", C.c_void_p), ("latent_buf", C.c_void_p), ("disp_buf", C.c_void_p),
        ("heights_buf", C.c_void_p), ("history", C.c_int), ("n_heights", C.c_int), ("height_joints", C.c_int * 8),
    ]


class DpSeqStep(C.Structure):
    _fields_ = [
        ("adjust_joint", C.c_int), ("adjust_target_joint", C.c_int), ("adjust_weight", C.c_float),
        ("tgt_pos", C.c_void_p), ("pose_ret", C.c_void_p), ("pos_ret", C.c_void_p),
    ]


class DpSeqFrames(C.Structure):
    _fields_ = [
        ("n_steps", C.c_int), ("tgt_pos", C.c_void_p), ("tgt_rot", C.c_void_p), ("tgt_root", C.c_void_p), ("w", C.c_void_p),
        ("tracked", C.c_void_p), ("z_tgt", C.c_void_p), ("z_tgt_step", C.c_int), ("z_tgt_seq", C.c_int),
    ]


class DpSeqResults(_Sized):
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint),
                ("pose_ret", C.c_void_p), ("pos_ret", C.c_void_p), ("world_rot", C.c_void_p), ("iters", C.c_void_p), ("loss", C.c_void_p),
                ("hist_scratch", C.c_void_p), ("status", C.c_void_p)]


class DpTemporalLayer(C.Structure):
    _fields_ = [(n, _f) for n in (
        "sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "ca_in_w", "ca_in_b", "ca_out_w", "ca_out_b",
        "lin1_w", "lin1_b", "lin2_w", "lin2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b", "norm3_w", "norm3_b")]


class DpTemporalModel(C.Structure):
    _fields_ = [
        ("n_heights", C.c_int), ("dim_feedforward", C.c_int), ("n_encoder_layers", C.c_int), ("n_decoder_layers", C.c_int),
        ("max_len", C.c_int), ("sample_step", C.c_int),
        ("in_proj_encoder_w", _f), ("in_proj_encoder_b", _f), ("in_proj_decoder_w", _f), ("in_proj_decoder_b", _f),
        ("out_proj_w", _f), ("out_proj_b", _f), ("pos_encoding", _f),
        ("enc_norm_w", _f), ("enc_norm_b", _f), ("dec_norm_w", _f), ("dec_norm_b", _f),
        ("means_latent", _f), ("stds_latent", _f),
        ("enc", C.POINTER(DpTemporalLayer)), ("dec", C.POINTER(DpTemporalLayer)),
    ]


class DpResult(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint), ("reserved0", C.c_uint), ("z", C.c_void_p), ("z_pre", C.c_void_p), ("pose", C.c_void_p), ("disp", C.c_void_p),
        ("world_disp", C.c_void_p), ("world_rot", C.c_void_p), ("pos", C.c_void_p), ("rot", C.c_void_p),
        ("loss", C.c_void_p), ("iters", C.c_void_p), ("status", C.c_void_p), ("clock", C.c_void_p),
    ]


DP_STATUS_NONFINITE_RESULT, DP_STATUS_BAD_STATE, DP_STATUS_BAD_TARGETS, DP_STATUS_TARGET_NOT_ROTATION = 1, 2, 4, 8
DP_TEMPORAL_TEAM_TIMEOUT = 1
DP_INPUT_LIMIT = 1.0e4


# every symbol include/dragposer.h declares (checked by tests/test_abi.py)
PUBLIC_SYMBOLS = (
    "dp_version", "dp_last_error", "dp_fold_decoder", "dp_create", "dp_destroy", "dp_optimize",
    "dp_forward", "dp_sequence_advance", "dp_optimize_sequence", "dp_kernel_geometry", "dp_auto_kernel", "dp_io_alloc", "dp_io_free", "dp_io_upload", "dp_io_download", "dp_stream_sync", "dp_io_alloc_host", "dp_io_free_host",
    "dp_temporal_create", "dp_temporal_destroy", "dp_temporal_last_error", "dp_temporal_predict", "dp_temporal_status",
)

# every symbol include/dragposer_grad.h declares (tests/test_grad_abi.py)
GRAD_SYMBOLS = ("dp_forward_vjp", "dp_forward_vjp_skeleton")


class DpGradIn(_Sized):
    """include/dragposer_grad.h: dp_grad_in (upstream gradients, device pointers; NULL = zero)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("pose", C.c_void_p), ("disp", C.c_void_p), ("world_disp", C.c_void_p),
                ("world_rot", C.c_void_p), ("pos", C.c_void_p), ("rot", C.c_void_p)]


# every symbol include/dragposer_constraints.h declares (tests/test_constraints_abi.py)
CONSTRAINT_SYMBOLS = ("dp_optimize_constrained", "dp_optimize_constrained_skeleton")


class DpConstraints(_Sized):
    """include/dragposer_constraints.h: dp_constraints, with DP_CONSTRAINTS_INIT's defaults (every weight 0)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint),
                ("w_feet_floor", C.c_float), ("w_head_hips_forward", C.c_float), ("w_head_hips_colinear", C.c_float), ("w_hips_feet_colinear", C.c_float),
                ("floor_joints", C.c_int * 2), ("foot_joints", C.c_int * 2), ("head_joint", C.c_int), ("hips_joint", C.c_int), ("up_axis", C.c_int),
                ("floor_one_sided", C.c_int), ("floor_level", C.c_float), ("fwd_axis", C.c_float * 3), ("fwd_threshold", C.c_float),
                ("fwd_margin", C.c_float), ("feet_radius", C.c_float), ("global_pos", C.c_void_p), ("loss_extra", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.floor_joints[:] = (4, 8)
        self.foot_joints[:] = (3, 7)
        self.head_joint, self.hips_joint, self.up_axis = 13, 0, 1
        self.fwd_axis[:] = (0.0, 0.0, 1.0)
        self.fwd_threshold, self.fwd_margin, self.feet_radius = 0.5, 0.2, 0.2


# every symbol include/dragposer_terms.h declares (tests/test_terms_abi.py)
TERM_SYMBOLS = ("dp_optimize_terms", "dp_optimize_terms_skeleton")
DP_MAX_TERMS = 16
DP_TERM_PLANE, DP_TERM_DISTANCE, DP_TERM_ALIGN = 1, 2, 3
DP_TERM_ONE_SIDED, DP_TERM_DROP_UP = 1, 2


class DpTerm(C.Structure):
    """include/dragposer_terms.h: dp_term, with DP_TERM_INIT's defaults"""
    _fields_ = [("type", C.c_int), ("joint_a", C.c_int), ("joint_b", C.c_int), ("flags", C.c_int), ("weight", C.c_float),
                ("point", C.c_float * 3), ("dir", C.c_float * 3), ("axis_a", C.c_float * 3), ("axis_b", C.c_float * 3),
                ("p0", C.c_float), ("p1", C.c_float), ("per_frame", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        if "joint_b" not in k:
            self.joint_b = -1
        self.dir[:] = (0.0, 1.0, 0.0)
        self.axis_a[:] = (0.0, 0.0, 1.0)
        self.axis_b[:] = (0.0, 0.0, 1.0)


class DpTerms(_Sized):
    """include/dragposer_terms.h: dp_terms, with DP_TERMS_INIT's defaults"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("n_terms", C.c_int), ("up_axis", C.c_int), ("terms", C.c_void_p),
                ("global_pos", C.c_void_p), ("loss_terms", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        if "up_axis" not in k:
            self.up_axis = 1


# every symbol include/dragposer_skeleton.h declares (tests/test_skeleton_abi.py)
SKELETON_SYMBOLS = ("dp_optimize_skeleton", "dp_forward_skeleton", "dp_optimize_sequence_skeleton")
DP_SKELETON_STRIDE = 66


class DpSkeletonIn(_Sized):
    """include/dragposer_skeleton.h: dp_skeleton_in (per-frame bone offsets, a device pointer; stride 66 or 0)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("offsets", C.c_void_p), ("stride", C.c_int)]


# every symbol include/dragposer_sequence_constraints.h declares (tests/test_sequence_constraints_abi.py)
SEQUENCE_CONSTRAINT_SYMBOLS = ("dp_optimize_sequence_constrained", "dp_optimize_sequence_terms")


class DpSeqExtra(_Sized):
    """include/dragposer_sequence_constraints.h: dp_seq_extra (per-step outputs of the terms and the per-term row steps; all optional)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("loss_extra", C.c_void_p), ("loss_terms", C.c_void_p),
                ("joint_pos", C.c_void_p), ("row_step", C.c_int * DP_MAX_TERMS)]


# every symbol include/dragposer_holds.h declares (tests/test_holds_abi.py)
HOLD_SYMBOLS = ("dp_optimize_sequence_holds",)
DP_MAX_HOLDS = 4


class DpHold(C.Structure):
    """include/dragposer_holds.h: dp_hold"""
    _fields_ = [("term", C.c_int), ("level", C.c_float), ("contact_lo", C.c_float), ("contact_hi", C.c_float)]


class DpHolds(_Sized):
    """include/dragposer_holds.h: dp_holds (holds: a HOST array of DpHold; state / trace: device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("n_holds", C.c_int), ("holds", C.c_void_p), ("state", C.c_void_p),
                ("trace", C.c_void_p)]


# every symbol include/dragposer_latent_ar.h declares (tests/test_latent_ar_abi.py)
LATENT_AR_SYMBOLS = ("dp_optimize_sequence_ar",)
DP_MAX_AR_ORDER = 4


class DpLatentAR(_Sized):
    """include/dragposer_latent_ar.h: dp_latent_ar (coeffs / bias / trace: device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("order", C.c_int), ("coeffs", C.c_void_p), ("bias", C.c_void_p),
                ("trace", C.c_void_p)]


# every symbol include/dragposer_gaps.h declares (tests/test_gaps_abi.py)
GAP_SYMBOLS = ("dp_optimize_sequence_gaps",)
DP_GAP_STATE_FLOATS = 16
DP_GAP_MAX_HOLD = 65535
DP_STATUS_TRACKER_HELD, DP_STATUS_TRACKER_LOST, DP_STATUS_NO_TRACKER = 16, 32, 64


class DpGaps(_Sized):
    """include/dragposer_gaps.h: dp_gaps (state / present / trace: device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("max_hold", C.c_int), ("decay", C.c_float), ("state", C.c_void_p),
                ("present", C.c_void_p), ("trace", C.c_void_p)]


# every symbol include/dragposer_live.h declares (tests/test_live_abi.py)
LIVE_SYMBOLS = ("dp_live_step",)


# every symbol include/dragposer_tethers.h declares (tests/test_tethers_abi.py)
TETHER_SYMBOLS = ("dp_optimize_sequence_tethers",)
DP_MAX_TETHERS = 4
DP_TETHER_STATE_FLOATS = 8


class DpTether(C.Structure):
    """include/dragposer_tethers.h: dp_tether"""
    _fields_ = [("term", C.c_int), ("alpha", C.c_float)]


class DpTethers(_Sized):
    """include/dragposer_tethers.h: dp_tethers (tethers: a HOST array of DpTether; state / trace: device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("n_tethers", C.c_int), ("tethers", C.c_void_p), ("state", C.c_void_p),
                ("trace", C.c_void_p)]


# every symbol include/dragposer_points.h declares (tests/test_points_abi.py)
POINT_SYMBOLS = ("dp_optimize_terms_points", "dp_optimize_terms_points_skeleton", "dp_optimize_sequence_terms_points")
DP_MAX_POINTS = 4


class DpPoints(_Sized):
    """include/dragposer_points.h: dp_points (coeff: a HOST array [n_points][22] of floats)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("n_points", C.c_int), ("reserved1", C.c_int), ("coeff", C.c_void_p)]


# every symbol include/dragposer_lm.h declares (tests/test_lm_abi.py)
LM_SYMBOLS = ("dp_optimize_lm",)
DP_LM_MAX_STEPS = 64


class DpLmParams(_Sized):
    """include/dragposer_lm.h: dp_lm_params, with DP_LM_PARAMS_INIT's defaults"""
    _fields_ = [("struct_size", C.c_uint), ("n_steps", C.c_int), ("lambda_rot", C.c_float), ("lambda_tmp", C.c_float), ("mu0", C.c_float),
                ("mu_up", C.c_float), ("mu_down", C.c_float), ("mu_min", C.c_float), ("mu_max", C.c_float), ("early_stop", C.c_int),
                ("stop_eps_pos", C.c_float), ("stop_eps_rot", C.c_float)]

    def __init__(self, *a, **k):
        super().__init__(*a, **dict(dict(n_steps=3, lambda_rot=1.0, lambda_tmp=0.0, mu0=1e-2, mu_up=4.0, mu_down=1.0 / 3.0, mu_min=1e-6, mu_max=1e6), **k))


class DpLmExtra(_Sized):
    """include/dragposer_lm.h: dp_lm_extra (device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("mu", C.c_void_p), ("n_accepted", C.c_void_p), ("loss0", C.c_void_p)]


# every symbol include/dragposer_sequence_lm.h declares (tests/test_lm_sequence_abi.py)
LM_SEQUENCE_SYMBOLS = ("dp_optimize_sequence_lm",)


class DpSeqLmExtra(_Sized):
    """include/dragposer_sequence_lm.h: dp_seq_lm_extra (device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("mu", C.c_void_p), ("mu_trace", C.c_void_p), ("n_accepted", C.c_void_p),
                ("loss0", C.c_void_p), ("joint_pos", C.c_void_p)]


# every symbol include/dragposer_lm_terms.h declares (tests/test_lm_terms_abi.py)
LM_TERMS_SYMBOLS = ("dp_optimize_lm_terms",)

# every symbol include/dragposer_sequence_lm_terms.h declares (tests/test_lm_sequence_terms_abi.py)
LM_SEQUENCE_TERMS_SYMBOLS = ("dp_optimize_sequence_lm_terms",)


# every symbol include/dragposer_calibration.h declares (tests/test_fit_bones_abi.py)
CALIBRATION_SYMBOLS = ("dp_fit_bones_workspace_bytes", "dp_fit_bones")
DP_FIT_MAX_GROUPS = 24
DP_FIT_NO_FRAMES, DP_FIT_SINGULAR = 1, 2


class DpBoneFit(_Sized):
    """include/dragposer_calibration.h: dp_bone_fit, with DP_BONE_FIT_INIT's defaults (groups / base / prior: HOST arrays; workspace: a device pointer)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("n_groups", C.c_int), ("ridge", C.c_float), ("groups", C.c_void_p),
                ("base", C.c_void_p), ("prior", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]

    def __init__(self, *a, **k):
        super().__init__(*a, **dict(dict(n_groups=1, ridge=1e-3), **k))


class DpBoneFitResult(_Sized):
    """include/dragposer_calibration.h: dp_bone_fit_result (device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("scales", C.c_void_p), ("offsets", C.c_void_p), ("normal", C.c_void_p),
                ("rms", C.c_void_p), ("info", C.c_void_p), ("status", C.c_void_p)]


# every symbol include/dragposer_clip_lm.h declares (tests/test_clip_lm_abi.py)
CLIP_LM_SYMBOLS = ("dp_clip_lm_workspace_bytes", "dp_optimize_clip_lm")
DP_CLIP_REFUSED_FRAME = 1


class DpClipLmParams(_Sized):
    """include/dragposer_clip_lm.h: dp_clip_lm_params, with DP_CLIP_LM_PARAMS_INIT's defaults"""
    _fields_ = [("struct_size", C.c_uint), ("n_steps", C.c_int), ("lambda_rot", C.c_float), ("lambda_tmp", C.c_float), ("lambda_smooth", C.c_float),
                ("mu0", C.c_float), ("mu_up", C.c_float), ("mu_down", C.c_float), ("mu_min", C.c_float), ("mu_max", C.c_float)]

    def __init__(self, *a, **k):
        super().__init__(*a, **dict(dict(n_steps=4, lambda_rot=1.0, lambda_tmp=0.0, lambda_smooth=1.0, mu0=1e-2, mu_up=4.0, mu_down=1.0 / 3.0,
                                         mu_min=1e-6, mu_max=1e6), **k))


# every symbol include/dragposer_clip_accel.h declares (tests/test_clip_accel_abi.py)
CLIP_ACCEL_SYMBOLS = ("dp_clip_lm_accel_workspace_bytes", "dp_optimize_clip_lm_accel")
# every symbol include/dragposer_clip_skeleton.h declares (tests/test_clip_skeleton_abi.py)
CLIP_SKELETON_SYMBOLS = ("dp_optimize_clip_lm_skeleton", "dp_optimize_lm_skeleton")


class DpClipAccelParams(_Sized):
    """include/dragposer_clip_accel.h: dp_clip_accel_params, with DP_CLIP_ACCEL_PARAMS_INIT's defaults (accel_loss: a device pointer)"""
    _fields_ = [("struct_size", C.c_uint), ("lambda_accel", C.c_float), ("accel_loss", C.c_void_p)]


class DpClipLmExtra(_Sized):
    """include/dragposer_clip_lm.h: dp_clip_lm_extra (device pointers)"""
    _fields_ = [("struct_size", C.c_uint), ("reserved0", C.c_uint), ("mu", C.c_void_p), ("n_accepted", C.c_void_p), ("clip_loss", C.c_void_p),
                ("loss_hist", C.c_void_p), ("info", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


# every symbol include/dragposer_encoder.h declares (tests/test_encoder_abi.py)
ENCODER_SYMBOLS = ("dp_fold_encoder", "dp_encoder_create", "dp_encoder_destroy", "dp_encoder_last_error", "dp_encoder_geometry", "dp_encode",
                   "dp_sequence_begin", "dp_debug_encoder_image")
DP_ENCODER_IN = 176


class DpEncoderModel(_Sized):
    """include/dragposer_encoder.h: dp_encoder_model (host pointers to the checkpoint's encoder tensors)"""
    _fields_ = [("struct_size", C.c_uint), ("conv_w", _f * 3), ("conv_mask", _f * 3), ("conv_b", _f * 3), ("pool_w", _f * 3),
                ("f_mu_w", _f), ("f_mu_b", _f), ("f_logvar_w", _f), ("f_logvar_b", _f)]


class DpEncoderFolded(C.Structure):
    _fields_ = [("A0", C.c_float * (112 * 176)), ("c0", C.c_float * 112), ("A1", C.c_float * (72 * 112)), ("c1", C.c_float * 72),
                ("A2", C.c_float * (48 * 72)), ("c2", C.c_float * 48), ("Ah", C.c_float * (48 * 48)), ("ch", C.c_float * 48)]


def encoder_model(arrays):
    """the checkpoint's encoder tensors (the keys of data/model_dancedb.npz) -> (DpEncoderModel, the arrays its pointers refer to:
    keep them alive as long as the struct is used)"""
    import numpy as np

    keep = []

    def arr(key, squeeze=False):
        a = np.asarray(arrays[key], dtype=np.float32)
        a = np.ascontiguousarray(a[..., 0] if squeeze else a)
        keep.append(a)
        return a.ctypes.data_as(_f)

    m = DpEncoderModel()
    for l in range(3):
        m.conv_w[l], m.conv_mask[l] = arr(f"encoder.layers.{l}.0.weight", True), arr(f"encoder.layers.{l}.0.mask", True)
        m.conv_b[l], m.pool_w[l] = arr(f"encoder.layers.{l}.0.bias"), arr(f"encoder.layers.{l}.1.weight")
    m.f_mu_w, m.f_mu_b = arr("encoder.f_mu.weight"), arr("encoder.f_mu.bias")
    m.f_logvar_w, m.f_logvar_b = arr("encoder.f_logvar.weight"), arr("encoder.f_logvar.bias")
    return m, keep


_libs = {}


def load(path=None):
    """Load the shared library (once per path; the product never passes one -- tests do, for the test-only second
    implementation libdragposer_hip_ref8.so).  Raises RuntimeError with the build hint when absent."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  dragposer_amd has no CPU fallback."
        )
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 and the device pointers / streams
    # it hands us are only meaningful to THAT runtime.  Import torch (and pin its copy) before our library is
    # resolved, so that the shared SONAME binds libdragposer_hip.so to torch's runtime, never to /opt/rocm's.
    import torch

    bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        C.CDLL(bundled, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(path)
    lib.dp_version.restype = C.c_int
    lib.dp_last_error.restype = C.c_char_p
    lib.dp_last_error.argtypes = [C.c_void_p]
    lib.dp_fold_decoder.argtypes = [C.POINTER(DpModel), C.POINTER(DpFolded)]
    lib.dp_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(DpModel), C.c_int]
    lib.dp_destroy.argtypes = [C.c_void_p]
    lib.dp_optimize.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpResult), C.c_void_p]
    lib.dp_forward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DpResult), C.c_void_p]
    lib.dp_forward_vjp.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DpGradIn), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]
    lib.dp_forward_vjp_skeleton.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DpSkeletonIn), C.POINTER(DpGradIn), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dp_optimize_constrained.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpConstraints), C.POINTER(DpResult),
                                            C.c_void_p]
    lib.dp_optimize_terms.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpTerms), C.POINTER(DpResult), C.c_void_p]
    lib.dp_optimize_constrained_skeleton.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpConstraints),
                                                     C.POINTER(DpSkeletonIn), C.POINTER(DpResult), C.c_void_p]
    lib.dp_optimize_terms_skeleton.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpTerms), C.POINTER(DpSkeletonIn),
                                               C.POINTER(DpResult), C.c_void_p]
    lib.dp_optimize_skeleton.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpSkeletonIn), C.POINTER(DpResult), C.c_void_p]
    lib.dp_forward_skeleton.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DpSkeletonIn), C.POINTER(DpResult), C.c_void_p]
    lib.dp_optimize_sequence_skeleton.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpSkeletonIn),
                                                  C.POINTER(DpSeqState), C.POINTER(DpSeqStep), C.POINTER(DpSeqResults), C.c_void_p]
    _seq_tail = [C.POINTER(DpSkeletonIn), C.POINTER(DpSeqState), C.POINTER(DpSeqStep), C.POINTER(DpSeqResults), C.POINTER(DpSeqExtra), C.c_void_p]
    lib.dp_optimize_sequence_constrained.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams),
                                                     C.POINTER(DpConstraints)] + _seq_tail
    lib.dp_optimize_sequence_terms.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpTerms)] + _seq_tail
    lib.dp_optimize_sequence_holds.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpTerms),
                                               C.POINTER(DpHolds)] + _seq_tail
    lib.dp_optimize_sequence_ar.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpTerms),
                                            C.POINTER(DpHolds), C.POINTER(DpLatentAR)] + _seq_tail
    lib.dp_optimize_sequence_gaps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpTerms),
                                              C.POINTER(DpHolds), C.POINTER(DpLatentAR), C.POINTER(DpGaps)] + _seq_tail
    lib.dp_live_step.argtypes = lib.dp_optimize_sequence_gaps.argtypes
    lib.dp_optimize_sequence_tethers.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpTerms),
                                                 C.POINTER(DpHolds), C.POINTER(DpLatentAR), C.POINTER(DpGaps), C.POINTER(DpTethers)] + _seq_tail
    lib.dp_optimize_terms_points.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpTerms), C.POINTER(DpPoints),
                                             C.POINTER(DpResult), C.c_void_p]
    lib.dp_optimize_terms_points_skeleton.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpTerms), C.POINTER(DpPoints),
                                                      C.POINTER(DpSkeletonIn), C.POINTER(DpResult), C.c_void_p]
    lib.dp_optimize_sequence_terms_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpTerms),
                                                      C.POINTER(DpPoints)] + _seq_tail
    lib.dp_optimize_lm.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpLmParams), C.POINTER(DpResult), C.POINTER(DpLmExtra), C.c_void_p]
    lib.dp_optimize_lm_terms.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpLmParams), C.POINTER(DpTerms), C.POINTER(DpResult),
                                         C.POINTER(DpLmExtra), C.c_void_p]
    lib.dp_optimize_sequence_lm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpLmParams), C.POINTER(DpLatentAR),
                                            C.POINTER(DpSeqState), C.POINTER(DpSeqStep), C.POINTER(DpSeqResults), C.POINTER(DpSeqLmExtra), C.c_void_p]
    lib.dp_optimize_sequence_lm_terms.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpLmParams), C.POINTER(DpTerms),
                                                  C.POINTER(DpLatentAR), C.POINTER(DpSeqState), C.POINTER(DpSeqStep), C.POINTER(DpSeqResults),
                                                  C.POINTER(DpSeqLmExtra), C.POINTER(DpSeqExtra), C.c_void_p]
    lib.dp_fit_bones_workspace_bytes.argtypes = [C.c_int]
    lib.dp_fit_bones_workspace_bytes.restype = C.c_size_t
    lib.dp_fit_bones.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpBoneFit), C.POINTER(DpBoneFitResult), C.c_void_p]
    lib.dp_clip_lm_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.dp_clip_lm_workspace_bytes.restype = C.c_size_t
    lib.dp_optimize_clip_lm.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.c_int, C.POINTER(DpClipLmParams), C.POINTER(DpResult),
                                        C.POINTER(DpClipLmExtra), C.c_void_p]
    lib.dp_clip_lm_accel_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.dp_clip_lm_accel_workspace_bytes.restype = C.c_size_t
    lib.dp_optimize_clip_lm_accel.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.c_int, C.POINTER(DpClipLmParams), C.POINTER(DpClipAccelParams),
                                              C.POINTER(DpResult), C.POINTER(DpClipLmExtra), C.c_void_p]
    lib.dp_optimize_clip_lm_skeleton.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.c_int, C.POINTER(DpClipLmParams), C.POINTER(DpClipAccelParams),
                                                 C.POINTER(DpSkeletonIn), C.POINTER(DpResult), C.POINTER(DpClipLmExtra), C.c_void_p]
    lib.dp_optimize_lm_skeleton.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpLmParams), C.POINTER(DpSkeletonIn), C.POINTER(DpResult),
                                            C.POINTER(DpLmExtra), C.c_void_p]
    lib.dp_sequence_advance.argtypes = [C.c_void_p, C.c_int, C.POINTER(DpResult), C.POINTER(DpSeqState), C.POINTER(DpSeqStep), C.c_void_p]
    lib.dp_optimize_sequence.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DpSeqFrames), C.POINTER(DpParams), C.POINTER(DpSeqState),
                                         C.POINTER(DpSeqStep), C.POINTER(DpSeqResults), C.c_void_p]
    lib.dp_kernel_geometry.argtypes = [C.c_void_p, _i, _i, _i]
    lib.dp_auto_kernel.argtypes = [C.c_void_p, C.c_int]
    lib.dp_auto_kernel.restype = C.c_int
    lib.dp_io_alloc_host.argtypes = [C.c_void_p, C.c_ulonglong, C.POINTER(C.c_void_p)]
    lib.dp_io_free_host.argtypes = [C.c_void_p, C.c_void_p]
    lib.dp_temporal_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(DpTemporalModel), C.c_int]
    lib.dp_temporal_destroy.argtypes = [C.c_void_p]
    lib.dp_temporal_last_error.restype = C.c_char_p
    lib.dp_temporal_last_error.argtypes = [C.c_void_p]
    lib.dp_temporal_predict.argtypes = [C.c_void_p, C.c_int, C.POINTER(DpSeqState), C.c_int, C.c_void_p, C.c_void_p]
    lib.dp_fold_encoder.argtypes = [C.POINTER(DpEncoderModel), C.POINTER(DpEncoderFolded)]
    lib.dp_encoder_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(DpEncoderModel), C.c_int]
    lib.dp_encoder_destroy.argtypes = [C.c_void_p]
    lib.dp_encoder_last_error.restype = C.c_char_p
    lib.dp_encoder_last_error.argtypes = [C.c_void_p]
    lib.dp_encoder_geometry.argtypes = [C.c_void_p, _i, _i, _i]
    lib.dp_encode.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    lib.dp_sequence_begin.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(DpSeqState), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dp_debug_encoder_image.argtypes = [C.POINTER(DpEncoderFolded), _f, _i, C.c_int]
    # private test hooks (not part of include/dragposer.h)
    lib.dp_optimize_debug.argtypes = [C.c_void_p, C.POINTER(DpBatch), C.POINTER(DpParams), C.POINTER(DpResult),
                                      C.c_void_p, C.c_void_p]
    lib.dp_temporal_debug_force_variant.argtypes = [C.c_void_p, C.c_int]
    lib.dp_temporal_debug_team_status.argtypes = [C.c_void_p]
    lib.dp_temporal_status.argtypes = [C.c_void_p]
    lib.dp_temporal_debug_team_fault.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.dp_temporal_debug_team_size.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.dp_temporal_debug_split3.argtypes = [C.c_float, C.POINTER(C.c_ushort)]
    lib.dp_temporal_debug_split3.restype = None
    lib.dp_debug_pack.argtypes = [C.POINTER(DpFolded), _i, _f, _f, C.POINTER(C.c_uint)]
    lib.dp_debug_items.argtypes = [C.POINTER(DpModel), C.c_void_p]
    lib.dp_debug_pack_w16.argtypes = [C.POINTER(DpFolded), C.POINTER(DpModel), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dp_debug_last_launch.argtypes = [C.c_void_p, _i]
    lib.dp_debug_set_w4_layout.argtypes = [C.c_void_p, C.c_int]
    lib.dp_debug_host_ctx.argtypes = [C.POINTER(C.c_void_p)]
    _libs[path] = lib
    return lib


def last_error(ctx=None):
    msg = load().dp_last_error(ctx)
    return msg.decode() if msg else ""


class DragPoserError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dragposer error {code}: {msg}")
        self.code = code
