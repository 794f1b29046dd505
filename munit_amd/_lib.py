"""ctypes binding of libmunit_hip.so (the C ABI declared in include/munit_hip.h).

The product path has NO fallback: if the library is missing or a symbol is absent the import
of the compute ops fails loudly (RuntimeError).  Loading the library needs no GPU, so the
CPU test-suite can check that every declared symbol is exported.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# MUNIT_HIP_LIB: developer override used by tools/ab_bench.sh to A/B two builds of the library in one GPU session
LIB_PATH = os.environ.get("MUNIT_HIP_LIB") or os.path.join(_HERE, "libmunit_hip.so")

ACT = {"none": 0, "relu": 1, "lrelu": 2, "tanh": 3}
PAD = {"zero": 0, "reflect": 1}
COMPUTE = {"f32": 0, "bf16": 1, "f32x3": 2}
DTYPE = {"f32": 0, "bf16": 1}     # MUNIT_DTYPE_*: element type of an activation tensor in HBM


class ConvDesc(Structure):
    """munit_conv_desc."""
    _fields_ = [("B", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int),
                ("Cout", c_int), ("KH", c_int), ("KW", c_int),
                ("stride", c_int), ("pad", c_int), ("pad_mode", c_int),
                ("upsample", c_int), ("act", c_int), ("slope", c_float), ("compute", c_int),
                ("in_dtype", c_int), ("out_dtype", c_int)]


class PrepItem(Structure):
    """munit_prep_item."""
    _fields_ = [("w", c_void_p), ("wp", c_void_p), ("Cout", c_int), ("KH", c_int), ("KW", c_int), ("Cin", c_int),
                ("kind", c_int), ("ps", c_int), ("bf16", c_int)]


class SnItem(Structure):
    """munit_sn_item."""
    _fields_ = [("w", c_void_p), ("u", c_void_p), ("v", c_void_p), ("O", c_int), ("KH", c_int), ("KW", c_int), ("I", c_int),
                ("slot", c_int)]


class ImageDesc(Structure):
    """munit_image_desc."""
    _fields_ = [("src_off", ctypes.c_longlong), ("src_h", c_int), ("src_w", c_int), ("rs_h", c_int), ("rs_w", c_int),
                ("crop_i", c_int), ("crop_j", c_int), ("flip", c_int), ("kind", c_int)]


class GemmProblem(Structure):
    """munit_gemm_problem."""
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p)]


class GridSrc(Structure):
    """munit_grid_src."""
    _fields_ = [("data", c_void_p), ("n", c_int), ("channels", c_int), ("layout", c_int)]


class RectDesc(Structure):
    """munit_rect_desc."""
    _fields_ = [("B", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int), ("x_ld", c_int), ("Cout", c_int), ("y_ld", c_int),
                ("KH", c_int), ("KW", c_int), ("stride", c_int), ("pad_h", c_int), ("pad_w", c_int), ("relu", c_int)]


WINDOW = {"max": 0, "avg": 1}     # MUNIT_WINDOW_*
RECT_TILES = ("128x128", "64x64", "128x64")  # tile argument / answer of munit_conv2d_rect_tile

_P = c_void_p  # device pointers travel as integers
_DESC = POINTER(ConvDesc)

# name -> (restype, argtypes); the keys are exactly the functions include/munit_hip.h declares
SIGNATURES = {
    "munit_version": (c_int, []),
    "munit_last_error": (c_char_p, []),
    "munit_stream_wait_stream": (c_int, [_P, _P]),
    "munit_comm_unique_id": (c_int, [_P, c_size_t]),
    "munit_comm_init": (c_int, [_P, c_int, c_int, _P]),
    "munit_comm_allreduce": (c_int, [_P, _P, c_size_t, _P]),
    "munit_comm_destroy": (c_int, [_P]),
    "munit_shutdown": (c_int, []),
    "munit_conv2d_out_hw": (c_int, [_DESC, POINTER(c_int), POINTER(c_int)]),
    "munit_conv2d_fwd_workspace_bytes": (c_size_t, [_DESC]),
    "munit_conv2d_fwd": (c_int, [_DESC, _P, _P, _P, _P, _P, c_size_t, _P]),
    "munit_conv2d_dgrad_workspace_bytes": (c_size_t, [_DESC]),
    "munit_conv2d_dgrad": (c_int, [_DESC, _P, _P, _P, _P, _P, c_size_t, _P]),
    "munit_conv2d_wgrad_workspace_bytes": (c_size_t, [_DESC]),
    "munit_conv2d_wgrad": (c_int, [_DESC, _P, _P, _P, _P, c_float, _P, c_size_t, _P]),
    "munit_conv2d_prepared_weight_bytes": (c_size_t, [_DESC, c_int]),
    "munit_conv2d_prep_item": (c_int, [_DESC, c_int, _P, _P, POINTER(PrepItem)]),
    "munit_conv2d_prepare_weights": (c_int, [POINTER(PrepItem), _P]),
    "munit_conv2d_prepare_weights_batch": (c_int, [_P, c_int, _P]),
    "munit_conv2d_fwd_prepared": (c_int, [_DESC, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "munit_conv2d_dgrad_prepared": (c_int, [_DESC, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "munit_conv2d_executed_flops": (c_double, [_DESC, c_int]),
    "munit_conv2d_kernel_name": (c_char_p, [_DESC, c_int]),
    "munit_linear_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "munit_linear_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, c_size_t, _P]),
    "munit_linear_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_float, _P, c_size_t, _P]),
    "munit_act_bwd": (c_int, [c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "munit_instnorm_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "munit_instnorm_route": (c_int, [c_int, c_int, c_int, c_int]),
    "munit_instnorm_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int,
                                   c_float, _P, c_size_t, _P]),
    "munit_instnorm_bwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, c_int,
                                   _P, c_size_t, _P]),
    "munit_instnorm_fwd_bf16": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int,
                                        c_float, _P, c_size_t, _P]),
    "munit_instnorm_bwd_bf16": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, c_int,
                                        _P, c_size_t, _P]),
    "munit_layernorm_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "munit_layernorm_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, c_int, c_float, _P, c_size_t, _P]),
    "munit_layernorm_bwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_float, c_int,
                                    c_float, _P, c_size_t, _P]),
    "munit_layernorm_fwd_bf16": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, c_int, c_float, _P, c_size_t, _P]),
    "munit_layernorm_bwd_bf16": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_float, c_int,
                                         c_float, _P, c_size_t, _P]),
    "munit_avgpool3s2_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_avgpool3s2_bwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_gap_fwd": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "munit_gap_bwd": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "munit_loss_workspace_bytes": (c_size_t, [c_size_t]),
    "munit_l1_mean_fwd": (c_int, [_P, _P, _P, c_size_t, c_int, _P, _P, c_size_t, _P]),
    "munit_l1_mean_bwd": (c_int, [_P, _P, _P, c_size_t, c_int, _P, _P, _P, _P]),
    "munit_l1_mean_fwd_bf16": (c_int, [_P, _P, _P, c_size_t, c_int, _P, _P, c_size_t, _P]),
    "munit_l1_mean_bwd_bf16": (c_int, [_P, _P, _P, c_size_t, c_int, _P, _P, _P, _P]),
    "munit_pair_l1_fwd": (c_int, [_P, _P, _P, _P, c_size_t, c_int, _P, _P, c_size_t, _P]),
    "munit_pair_l1_bwd": (c_int, [_P, _P, _P, _P, c_size_t, c_int, _P, _P, _P, _P]),
    "munit_mse_const_fwd": (c_int, [_P, c_float, c_size_t, _P, _P, c_size_t, _P]),
    "munit_mse_const_bwd": (c_int, [_P, c_float, c_size_t, _P, _P, _P]),
    "munit_lsgan_workspace_bytes": (c_size_t, [c_int]),
    "munit_lsgan_fwd": (c_int, [POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float), c_int, _P, _P, _P, c_size_t, _P]),
    "munit_lsgan_bwd": (c_int, [POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float), c_int, _P, POINTER(c_void_p), _P]),
    "munit_nsgan_workspace_bytes": (c_size_t, [c_int]),
    "munit_nsgan_fwd": (c_int, [POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float), c_int, _P, _P, _P, c_size_t, _P]),
    "munit_nsgan_bwd": (c_int, [POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float), c_int, _P, POINTER(c_void_p), _P]),
    "munit_sn_power_iter_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "munit_sn_power_iter": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "munit_sn_act_fwd": (c_int, [_P, _P, _P, _P, c_size_t, c_int, c_int, c_float, _P]),
    "munit_sn_act_bwd_workspace_bytes": (c_size_t, [c_size_t, c_int]),
    "munit_sn_act_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_float, _P, c_size_t, c_int, c_int, c_float, _P, c_size_t, _P]),
    "munit_sn_grad_fix": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "munit_weighted_sum":(c_int, [POINTER(c_void_p), POINTER(c_float), c_int, _P, _P]),
    "munit_adam_step": (c_int, [_P, _P, _P, _P, c_size_t, c_double, c_double, c_double, c_double, c_double, c_int,
                                _P]),
    "munit_extraadam_step": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_double, c_double, c_double, c_double,
                                     c_double, c_int, c_int, _P]),
    "munit_scale": (c_int, [_P, _P, c_size_t, c_float, c_int, _P]),
    "munit_image_ksize": (c_int, [c_int, c_int]),
    "munit_image_preprocess_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "munit_image_preprocess": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "munit_mask_preprocess_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "munit_mask_preprocess": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "munit_label_preprocess_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "munit_label_preprocess": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "munit_image_grid_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "munit_image_grid_u8": (c_int, [POINTER(GridSrc), c_int, c_int, c_int, c_int, c_float, c_float, _P, _P, c_size_t, _P]),
    "munit_seg_input_fwd": (c_int, [_P, _P, c_size_t, _P]),
    "munit_seg_input_bwd": (c_int, [_P, _P, c_size_t, _P]),
    "munit_space_to_batch": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "munit_maxpool3s2_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_maxpool3s2_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_add_relu_fwd": (c_int, [_P, _P, _P, c_size_t, _P]),
    "munit_seg_ce_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "munit_seg_ce_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, c_size_t, _P]),
    "munit_seg_ce_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "munit_seg_ce_gt_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, c_size_t, _P]),
    "munit_seg_ce_gt_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "munit_seg_labels": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "munit_seg_ce_direct_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "munit_seg_ce_direct_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P, c_size_t, _P]),
    "munit_seg_ce_direct_bwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "munit_avgpool7_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_avgpool7_bwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_batchnorm_workspace_bytes": (c_size_t, [c_int]),
    "munit_batchnorm_fwd": (c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_longlong, c_int, _P, _P, c_int, c_int, c_float, c_float,
                                    _P, c_size_t, _P]),
    "munit_batchnorm_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_float, ctypes.c_longlong, c_int, c_int, _P,
                                    c_size_t, _P]),
    "munit_batchnorm_dp_workspace_bytes": (c_size_t, [c_int]),
    "munit_batchnorm_dp_stats_local": (c_int, [_P, ctypes.c_longlong, c_int, c_int, c_int, _P, c_size_t, _P, c_size_t, _P]),
    "munit_batchnorm_dp_fwd_apply": (c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_longlong, c_int, c_int, _P, c_size_t, _P, _P,
                                             c_int, c_float, c_float, _P]),
    "munit_batchnorm_dp_bwd_local": (c_int, [_P, _P, _P, _P, _P, ctypes.c_longlong, c_int, c_int, c_int, c_int, _P, c_size_t,
                                             _P, c_size_t, _P]),
    "munit_batchnorm_dp_bwd_finish": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_float, ctypes.c_longlong, c_int, c_int,
                                              c_int, c_int, _P, c_size_t, _P, c_size_t, _P]),
    "munit_maxpool2_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_maxpool2_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_avgpool16_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_avgpool16_bwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "munit_gemm_f32": (c_int, [POINTER(GemmProblem), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                               c_float, _P]),
    "munit_fid_moments_workspace_bytes": (c_size_t, [c_int, c_int]),
    "munit_fid_moments": (c_int, [_P, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "munit_sqrt_newton_schulz_workspace_bytes": (c_size_t, [c_int, c_int]),
    "munit_sqrt_newton_schulz": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "munit_frechet_distance_workspace_bytes": (c_size_t, [c_int]),
    "munit_frechet_distance": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P, c_size_t, _P]),
    "munit_conv2d_rect_out_hw": (c_int, [POINTER(RectDesc), POINTER(c_int), POINTER(c_int)]),
    "munit_conv2d_rect_tile": (c_int, [POINTER(RectDesc)]),
    "munit_conv2d_rect_fwd": (c_int, [POINTER(RectDesc), _P, _P, _P, _P, c_int, _P]),
    "munit_window3_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "munit_inception_input": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "munit_vgg_input_fwd": (c_int, [_P, _P, c_size_t, _P]),
    "munit_vgg_input_bwd": (c_int, [_P, _P, c_size_t, _P]),
    "munit_in_mse_workspace_bytes": (c_size_t, [c_int, c_int]),
    "munit_in_mse_fwd": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "munit_in_mse_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
}

_lib = None


def load():
    """Load the shared library once; raise RuntimeError (never fall back) when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "munit_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C munit_amd/csrc`). There is no CPU / PyTorch fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError("munit_amd: %s does not export %s" % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().munit_last_error()
        raise RuntimeError("munit_hip %s failed (rc=%d): %s" % (what, rc, (msg or b"").decode()))
