"""ctypes binding of libcgen_hip.so (include/cgen_hip.h).  Loading never needs a GPU; calling does."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CGEN_LIB") or os.path.join(_HERE, "libcgen_hip.so")  # (CGEN_LIB: another build of the same ABI, for A/B runs)

OK, EINVAL, ELAUNCH, EUNSUPPORTED = 0, -1, -2, -3
F32, F16, F32S = 0, 1, 2
DMOL_LOW_BIT = 0x100  # OR-ed into the dtype of cgen_dmol_nll_fwd/bwd: the reference's low_bit=True branch (dmol.py:52-60)
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
UNARY_LEAKY_RELU, UNARY_CLAMP_MIN, UNARY_ADD = 3, 4, 5
MAX_SEG = 4
BLOCK3_PLAN_INTS, BLOCK4_PLAN_INTS, WGRAD_PLAN_INTS = 24, 16, 24  # int32 entries of the cgen_*_plan / _plan_record outputs
PRED_PLAN_LAUNCHES, PRED_PLAN_FIELDS = 13, 8  # cgen_predictor_tiled_plan: records of a full plan, int32 fields per record


class View(C.Structure):
    _fields_ = [("p", C.c_void_p), ("sn", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64), ("c", C.c_int32),
                ("cpad", C.c_int32)]


NULL_VIEW = View(None, 0, 0, 0, 0, 0)


class ConvArgs(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("ks", C.c_int32),
                ("nseg", C.c_int32), ("act", C.c_int32), ("dact", C.c_int32), ("seg", View * MAX_SEG),
                ("weight", C.c_void_p), ("bias", C.c_void_p), ("out", View), ("aux", View), ("res1", View), ("res2", View),
                ("out_rem", C.c_int64), ("res1_rem", C.c_int64)]


class Block3Out(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p), ("out", View), ("aux", View), ("res1", View),
                ("out_rem", C.c_int64), ("res1_rem", C.c_int64)]


class Block3Args(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("nseg", C.c_int32),
                ("nout", C.c_int32), ("pre_act", C.c_int32), ("reserved", C.c_int32), ("seg", View * MAX_SEG),
                ("w_a", C.c_void_p), ("bias_a", C.c_void_p), ("mid", View), ("mid_aux", View), ("o", Block3Out * 2), ("w_a16", C.c_void_p),
                ("w_proj", C.c_void_p), ("bias_proj", C.c_void_p), ("proj_krow", C.c_int32), ("pool", C.c_int32)]  # (the down Block: zero = absent)


class Block4Args(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("nseg", C.c_int32),
                ("nout", C.c_int32), ("fwd", C.c_int32), ("b", C.c_int32), ("seg", View * MAX_SEG),
                ("wimg", C.c_void_p * 3), ("bias", C.c_void_p * 3), ("mid", View * 3), ("mid_aux", View * 3), ("o", Block3Out * 3)]


class WgradArgs(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("ks", C.c_int32),
                ("nseg", C.c_int32), ("act", C.c_int32), ("nsplit", C.c_int32), ("seg", View * MAX_SEG), ("gout", View),
                ("partial_w", C.c_void_p), ("partial_b", C.c_void_p)]


class WprepDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("co", C.c_int32), ("ci_total", C.c_int32), ("ks", C.c_int32),
                ("mode", C.c_int32), ("nseg", C.c_int32), ("seg_off", C.c_int32), ("seg_c", C.c_int32 * MAX_SEG),
                ("dtype", C.c_int32), ("rows_pad", C.c_int32), ("k_pad", C.c_int32), ("reserved", C.c_int32),
                ("numel", C.c_int64)]


class WredDesc(C.Structure):
    _fields_ = [("partial_w", C.c_void_p), ("partial_b", C.c_void_p), ("grad_w", C.c_void_p), ("grad_b", C.c_void_p),
                ("co", C.c_int32), ("ci_total", C.c_int32), ("ks", C.c_int32), ("nsplit", C.c_int32),
                ("accumulate", C.c_int32), ("unscale", C.c_float), ("layout", C.c_int32), ("reserved", C.c_int32),
                ("numel", C.c_int64)]


class WredItem(C.Structure):
    """cgen_wred_item: one workgroup of cgen_wgrad_reduce_tiles (a tile of a site's partials, or a run of its bias gradient)."""
    _fields_ = [("partial", C.c_void_p), ("grad", C.c_void_p), ("kind", C.c_int32), ("nsplit", C.c_int32),
                ("split_stride", C.c_int32), ("vec", C.c_int32), ("v4", C.c_int32), ("accumulate", C.c_int32),
                ("unscale", C.c_float), ("taps", C.c_int32), ("inner", C.c_int32), ("ci_total", C.c_int32), ("layout", C.c_int32),
                ("a0", C.c_int32), ("na", C.c_int32), ("b0", C.c_int32), ("nb", C.c_int32), ("reserved", C.c_int32)]


class AdamwArgs(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p),
                ("count", C.c_int64), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("wd", C.c_float), ("ema_beta", C.c_float), ("warmup_steps", C.c_int32), ("ema_update_after", C.c_int32),
                ("state_dev", C.c_void_p)]


class CfLagrangeArgs(C.Structure):
    """cgen_cf_lagrange_args: the Lagrangian of counterfactual fine-tuning -- inputs, constants and the five output blocks."""
    _fields_ = [("out3", C.c_void_p), ("aux_sum", C.c_void_p), ("aux_add", C.c_void_p), ("lmbda", C.c_void_p), ("beta_dev", C.c_void_p),
                ("nonfinite", C.c_void_p), ("n_nonfinite", C.c_int32), ("inv_b", C.c_float), ("eps", C.c_float), ("damping", C.c_float),
                ("seed_scale", C.c_float), ("beta", C.c_float), ("res", C.c_void_p), ("coef", C.c_void_p), ("gsq_slot", C.c_void_p),
                ("gate", C.c_void_p), ("sums", C.c_void_p)]


class LagrangeStepArgs(C.Structure):
    """cgen_lagrange_step_args: the multiplier, its moments and EMA, its gradient and the tail's state vector."""
    _fields_ = [("lmbda", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p), ("g", C.c_void_p), ("state_dev", C.c_void_p),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("ema_beta", C.c_float),
                ("ema_update_after", C.c_int32)]


class PredHead(C.Structure):
    _fields_ = [("c", C.c_int32), ("res", C.c_int32), ("width", C.c_int32), ("nout", C.c_int32), ("ctx", C.c_int32),
                ("kind", C.c_int32), ("tanh_loc", C.c_int32), ("obs_stride", C.c_int32), ("std_fixed", C.c_float),
                ("reserved", C.c_int32), ("w", C.c_void_p * 8), ("b", C.c_void_p * 8), ("y", C.c_void_p), ("obs", C.c_void_p)]


class PredTrainHead(C.Structure):
    """cgen_pred_train_head: ``hd`` with the RAW weights in hd.w (hd.b[7] = fc.3's bias), the seven BatchNorms and every gradient."""
    _fields_ = [("hd", PredHead), ("gamma", C.c_void_p * 7), ("beta", C.c_void_p * 7), ("running_mean", C.c_void_p * 7),
                ("running_var", C.c_void_p * 7), ("num_batches_tracked", C.c_void_p * 7), ("gw", C.c_void_p * 8), ("gb", C.c_void_p),
                ("ggamma", C.c_void_p * 7), ("gbeta", C.c_void_p * 7)]


class MlpTrainHead(C.Structure):
    """cgen_mlp_train_head: one scalar head (layers.py MLP) in training mode -- input columns with their row strides, the raw
    weights, the two BatchNorms and every gradient."""
    _fields_ = [("nin", C.c_int32), ("width", C.c_int32), ("tanh_loc", C.c_int32), ("obs_stride", C.c_int32), ("std_fixed", C.c_float),
                ("reserved", C.c_int32), ("in_", C.c_void_p * 8), ("in_stride", C.c_int64 * 8), ("obs", C.c_void_p), ("w", C.c_void_p * 3),
                ("bias", C.c_void_p), ("gamma", C.c_void_p * 2), ("beta", C.c_void_p * 2), ("running_mean", C.c_void_p * 2),
                ("running_var", C.c_void_p * 2), ("num_batches_tracked", C.c_void_p * 2), ("gw", C.c_void_p * 3), ("gb", C.c_void_p),
                ("ggamma", C.c_void_p * 2), ("gbeta", C.c_void_p * 2)]


class ResnetArgs(C.Structure):
    """cgen_resnet_args: the weight images, GroupNorm parameters, heads and observations of ChestPredictor's one trunk."""
    _fields_ = [("res", C.c_int32), ("ctx_stride", C.c_int32), ("std_fixed", C.c_float), ("obs_stride", C.c_int32 * 4),
                ("reserved", C.c_int32), ("img_fwd", C.c_void_p * 20), ("img_dg", C.c_void_p * 20), ("gamma", C.c_void_p * 20),
                ("beta", C.c_void_p * 20), ("fc_w", C.c_void_p * 4), ("fc_b", C.c_void_p * 4), ("obs", C.c_void_p * 4), ("ctx", C.c_void_p)]


class ResnetTrainArgs(C.Structure):
    """cgen_resnet_train_args: the eval record, every gradient destination, Dropout's probability and Philox state."""
    _fields_ = [("net", ResnetArgs), ("gw", C.c_void_p * 20), ("ggamma", C.c_void_p * 20), ("gbeta", C.c_void_p * 20),
                ("gfc_w", C.c_void_p * 4), ("gfc_b", C.c_void_p * 4), ("rng", C.c_void_p), ("p_dropout", C.c_float), ("reserved", C.c_int32)]


class AugmentArgs(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("c", C.c_int32), ("h0", C.c_int32), ("w0", C.c_int32), ("r_h", C.c_int32),
                ("r_w", C.c_int32), ("pad_x", C.c_int32), ("pad_y", C.c_int32), ("ctx", C.c_int32), ("stream_id", C.c_uint32),
                ("hflip_p", C.c_float), ("sub", C.c_float), ("mul", C.c_float), ("n_data", C.c_int64), ("data", C.c_void_p),
                ("index", C.c_void_p), ("out", View), ("rng", C.c_void_p), ("draws_in", C.c_void_p), ("draws_out", C.c_void_p),
                ("pa_data", C.c_void_p), ("pa_out", C.c_void_p)]


class LatentTailArgs(C.Structure):
    """cgen_latent_tail_bwd_args: a decoder layer's backward latent tail (1x1 data gradients + reparam backward) as one launch."""
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("z_dim", C.c_int32), ("c", C.c_int32),
                ("coef_stride", C.c_int32), ("acc_q", C.c_int32), ("acc_p", C.c_int32), ("logt", C.c_float), ("parity", C.c_int32), ("reserved", C.c_int32),
                ("g_h", View), ("g_f", View), ("gz_in", View), ("q_loc", View), ("q_ls", View), ("p_loc", View), ("p_ls", View),
                ("z", View), ("out_p", View), ("out_q", View), ("img_fz", C.c_void_p), ("img_fp", C.c_void_p), ("img_pz", C.c_void_p),
                ("coef", C.c_void_p), ("chan_scale", C.c_void_p)]


class DgaussHeadArgs(C.Structure):
    """cgen_dgauss_head_args: the two 1x1 likelihood heads fused with the discretised-Gaussian NLL, one launch each way."""
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("hin", View),
                ("img_loc", C.c_void_p), ("img_ls", C.c_void_p), ("bias_loc", C.c_void_p), ("bias_ls", C.c_void_p),
                ("params", View), ("x", View), ("nll_part", C.c_void_p),
                ("coef_dev", C.c_void_p), ("coef_stride", C.c_int32), ("nsplit", C.c_int32), ("g_h", View), ("g_params", View),
                ("partial_w_loc", C.c_void_p), ("partial_b_loc", C.c_void_p), ("partial_w_ls", C.c_void_p), ("partial_b_ls", C.c_void_p)]


class LatentTailFwdArgs(C.Structure):
    """cgen_latent_tail_fwd_args: a decoder layer's forward latent tail (reparam + KL, z_proj, z_feat_proj) as one launch."""
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("z_dim", C.c_int32), ("c", C.c_int32),
                ("ctx", C.c_int32), ("kl_stride", C.c_int32), ("stream_id", C.c_uint32), ("logt", C.c_float),
                ("h_in_rem", C.c_int64), ("h_out_rem", C.c_int64),
                ("q_loc", View), ("q_ls", View), ("p_loc", View), ("p_ls", View), ("p_feat", View), ("h_in", View), ("pa", View),
                ("eps", View), ("z", View), ("h_out", View), ("zf", View), ("img_p", C.c_void_p), ("img_f", C.c_void_p),
                ("bias_p", C.c_void_p), ("bias_f", C.c_void_p), ("rng", C.c_void_p), ("kl_part", C.c_void_p)]


class MetricVar(C.Structure):
    """cgen_metric_var: one variable of cgen_metric_accum (kind, transform, in-place prediction / target rows, the accumulator block)."""
    _fields_ = [("kind", C.c_int32), ("transform", C.c_int32), ("ncls", C.c_int32), ("reserved", C.c_int32), ("pred", C.c_void_p),
                ("pred_stride", C.c_int64), ("target", C.c_void_p), ("target_stride", C.c_int64), ("pred_scale", C.c_float),
                ("pred_shift", C.c_float), ("tgt_scale", C.c_float), ("tgt_shift", C.c_float), ("norm", C.c_float),
                ("reserved2", C.c_int32), ("acc", C.c_void_p), ("scores", C.c_void_p), ("labels", C.c_void_p),
                ("capacity", C.c_int64), ("row_count", C.c_void_p)]


class PgmMech(C.Structure):
    """cgen_pgm_mech: one mechanism of the parent SCM (kind, the columns it scores and conditions on, its MLP / spline geometry,
    its parameters and their gradient slots)."""
    _fields_ = [("kind", C.c_int32), ("normalize", C.c_int32), ("col", C.c_int32), ("ncls", C.c_int32), ("nctx", C.c_int32),
                ("ctx_col", C.c_int32 * 2), ("nhidden", C.c_int32), ("width", C.c_int32 * 3), ("act", C.c_int32), ("bins", C.c_int32),
                ("bound", C.c_float), ("p", C.c_void_p * 8), ("g", C.c_void_p * 8)]


class PgmPre(C.Structure):
    """cgen_pgm_pre: one entry of the parents vector the HVAE takes (columns copied, or log-standardised as ukbb_preprocess does)."""
    _fields_ = [("col", C.c_int32), ("width", C.c_int32), ("kind", C.c_int32), ("hi", C.c_float), ("lo", C.c_float), ("mu", C.c_float),
                ("sd", C.c_float)]


class PgmCfArgs(C.Structure):
    """cgen_pgm_cf_args: observations, intervention values, mask, Gumbel-max uniforms and the outputs of cgen_pgm_counterfactual."""
    _fields_ = [("obs", C.c_void_p), ("table_rows", C.c_int64), ("index", C.c_void_p), ("do_table", C.c_void_p), ("do_rows", C.c_int64),
                ("do_index", C.c_void_p), ("do_mask_dev", C.c_void_p), ("uniforms", C.c_void_p * 8), ("cf", C.c_void_p), ("eps", C.c_void_p),
                ("pa", C.c_void_p), ("cf_pa", C.c_void_p), ("ncol", C.c_int32), ("rows", C.c_int32), ("do_mask", C.c_uint32),
                ("exact_gumbel", C.c_int32), ("npre", C.c_int32), ("reserved", C.c_int32), ("pre", PgmPre * 8)]


PGM_BERNOULLI, PGM_CATEGORICAL, PGM_SPLINE, PGM_AFFINE, PGM_GUMBEL_MAX = 0, 1, 2, 3, 4
PGM_LEAKY_RELU, PGM_GELU, PGM_SIGMOID = 0, 1, 2
PGM_MAX_MECH, PGM_MAX_WIDTH, PGM_MAX_HIDDEN, PGM_MAX_BINS, PGM_MAX_CLS, PGM_ROWS = 8, 64, 3, 8, 16, 64
PGM_MAX_PRE, PGM_PRE_COPY, PGM_PRE_LOGSTD = 8, 0, 1
METRIC_BINARY, METRIC_CATEGORICAL, METRIC_CONTINUOUS = 0, 1, 2
METRIC_NONE, METRIC_SIGMOID, METRIC_SOFTMAX, METRIC_TANH = 0, 1, 2, 3
METRIC_N, METRIC_CORRECT, METRIC_ABS_ERR, METRIC_SKIPPED, METRIC_OVERFLOW = 0, 1, 2, 3, 4
METRIC_MAX_VARS, METRIC_ACC = 8, 8
STREAM_AUGMENT = 980  # Philox stream id of cgen_batch_augment (the list of taken ids is in csrc/common.h)
STREAM_GUMBEL, STREAM_GUMBEL_COUNT = 989, 8  # 989 + k: the k-th Gumbel-max mechanism's uniforms (PgmCounterfactual.run(rng=)); 989 .. 996
PRED_NORMAL, PRED_CATEGORICAL, PRED_BERNOULLI = 0, 1, 2
PRED_MAX_HEADS, PRED_MAX_OUT = 4, 16
MLP_MAX_IN, MLP_MAX_WIDTH = 8, 64
RESNET_CONVS, RESNET_SITES = 20, 18

i32, i64, u32, u64, f32, vp = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p

# name -> argtypes (all return int unless listed in _RESTYPES).  Kept in lock-step with include/cgen_hip.h:
# tests/test_abi_mirror.py holds every prototype, every struct of STRUCTS (below) and every constant of this module to the
# header as gcc reads it; tests/test_abi.py checks that every declared symbol is exported and bound here.
PROTOTYPES = {
    "cgen_version": [],
    "cgen_h16_format": [],
    "cgen_last_error": [],
    "cgen_conv2d": [C.POINTER(ConvArgs), vp],
    "cgen_conv2d_last_kernel": [],
    "cgen_conv2d_pair_supported": [C.POINTER(ConvArgs), C.POINTER(ConvArgs)],
    "cgen_conv2d_pair": [C.POINTER(ConvArgs), C.POINTER(ConvArgs), vp],
    "cgen_block3_supported": [C.POINTER(Block3Args)],
    "cgen_block3": [C.POINTER(Block3Args), vp],
    "cgen_block3_plan": [C.POINTER(Block3Args), C.POINTER(i32)],
    "cgen_block3_pair_supported": [C.POINTER(Block3Args), C.POINTER(Block3Args)],
    "cgen_block3_pair": [C.POINTER(Block3Args), C.POINTER(Block3Args), vp],
    "cgen_block3_pair_plan": [C.POINTER(Block3Args), C.POINTER(Block3Args), C.POINTER(i32)],
    "cgen_block4_supported": [C.POINTER(Block4Args)],
    "cgen_block4": [C.POINTER(Block4Args), vp],
    "cgen_block4_plan": [C.POINTER(Block4Args), C.POINTER(i32)],
    "cgen_block4_pair_plan": [C.POINTER(Block4Args), C.POINTER(Block4Args), C.POINTER(i32)],
    "cgen_block4_pair_supported": [C.POINTER(Block4Args), C.POINTER(Block4Args)],
    "cgen_block4_pair": [C.POINTER(Block4Args), C.POINTER(Block4Args), vp],
    "cgen_conv2d_wgrad_plan": [C.POINTER(WgradArgs), C.POINTER(i32)],
    "cgen_conv2d_wgrad_plan_record": [C.POINTER(WgradArgs), C.POINTER(i32)],
    "cgen_conv2d_wgrad_batch_plan": [vp, i32, vp, i64, vp, vp, i32, vp, vp],
    "cgen_conv2d_wgrad_batch_run": [vp, vp, i32, i32, vp],
    "cgen_conv2d_wgrad": [C.POINTER(WgradArgs), vp],
    "cgen_weight_prep": [vp, vp, vp, i32, vp],
    "cgen_wgrad_reduce": [vp, vp, vp, i32, vp],
    "cgen_weight_prep_ref": [vp, vp, vp, i32, vp],
    "cgen_wgrad_reduce_tiles": [vp, i32, vp],
    "cgen_wgrad_reduce_ref": [vp, vp, vp, i32, vp],
    "cgen_avgpool_fwd": [i32, i32, i32, i32, i32, View, View, vp],
    "cgen_avgpool_bwd": [i32, i32, i32, i32, i32, View, View, i32, vp],
    "cgen_adaptive_avgpool_fwd": [i32, i32, i32, i32, i32, i32, View, View, vp],
    "cgen_adaptive_avgpool_bwd": [i32, i32, i32, i32, i32, i32, View, View, i32, vp],
    "cgen_upsample_fwd": [i32, i32, i32, i32, i32, i32, View, vp, View, vp],
    "cgen_upsample_bwd": [i32, i32, i32, i32, i32, i32, View, View, i32, vp],
    "cgen_batch_reduce": [i32, i32, i32, i32, View, vp, i32, f32, vp],
    "cgen_batch_broadcast": [i32, i32, i32, i32, vp, View, vp],
    "cgen_axpby": [i32, i32, i32, i32, View, View, f32, f32, i32, i32, vp],
    "cgen_nchw_to_nhwc": [i32, i32, i32, i32, i32, i32, vp, View, f32, f32, vp],
    "cgen_nhwc_to_nchw": [i32, i32, i32, i32, i32, View, vp, vp],
    "cgen_batch_augment": [C.POINTER(AugmentArgs), vp],
    "cgen_batch_augment_arm": [C.POINTER(AugmentArgs)],
    "cgen_batch_augment_planar": [C.POINTER(AugmentArgs), vp],
    "cgen_stem_conv_supported": [i32, i32, i32, i32],
    "cgen_stem_conv_fwd": [i32, i32, i32, i32, i32, i32, i32, View, vp, vp, View, vp],
    "cgen_im2col": [i32, i32, i32, i32, i32, View, View, vp],
    "cgen_reparam_kl_chunks": [i32, i32, i32],
    "cgen_reparam_kl_fwd": [i32, i32, i32, i32, i32, View, View, View, View, View, vp, u32, f32, View, View, vp, i32, vp],
    "cgen_reparam_kl_bwd": [i32, i32, i32, i32, i32, View, View, View, View, View, f32, View, vp, i32, vp, View, View, View,
                            View, i32, i32, vp],
    "cgen_reparam_kl_bwd_rider": [i32, i32, i32, i32, i32, View, View, View, View, View, f32, View, vp, i32, vp, View, View, View,
                                  View, i32, i32, View, View, i32, vp],
    "cgen_latent_tail_bwd_supported": [C.POINTER(LatentTailArgs)],
    "cgen_latent_tail_bwd": [C.POINTER(LatentTailArgs), vp],
    "cgen_latent_tail_fwd_supported": [C.POINTER(LatentTailFwdArgs)],
    "cgen_latent_tail_fwd": [C.POINTER(LatentTailFwdArgs), vp],
    "cgen_kl_channel_sums": [i32, i32, i32, i32, i32, View, View, View, View, f32, vp, i32, vp],
    "cgen_elbo_finalize_fb": [i32, vp, i32, f32, vp, i32, f32, f32, f32, vp, vp, vp, vp],
    "cgen_im2col_strided": [i32, i32, i32, i32, i32, i32, i32, i32, i32, View, View, vp],
    "cgen_col2im_strided": [i32, i32, i32, i32, i32, i32, i32, i32, i32, View, View, i32, vp],
    "cgen_unary_fwd": [i32, i32, f32, i32, i32, i32, i32, View, View, vp],
    "cgen_unary_bwd": [i32, i32, f32, i32, i32, i32, i32, View, View, View, i32, vp],
    "cgen_sample_gaussian": [i32, i32, i32, i32, i32, View, View, View, vp, u32, f32, View, vp],
    "cgen_gaussian_kl_map": [i64, vp, vp, vp, vp, vp, vp],
    "cgen_mediator_mix": [i32, i32, i32, i32, i32, View, View, View, View, View, f32, f32, f32, i32, View, vp],
    "cgen_like_chunks": [i32, i32],
    "cgen_dgauss_nll_fwd": [i32, i32, i32, i32, i32, View, View, vp, vp],
    "cgen_dgauss_nll_bwd": [i32, i32, i32, i32, i32, View, View, vp, i32, View, vp],
    "cgen_dgauss_head_supported": [C.POINTER(DgaussHeadArgs)],
    "cgen_dgauss_head_fwd": [C.POINTER(DgaussHeadArgs), vp],
    "cgen_dgauss_head_bwd": [C.POINTER(DgaussHeadArgs), vp],
    "cgen_dgauss_params": [i32, i32, i32, i32, i32, View, View, f32, vp, vp, vp],
    "cgen_dgauss_sample": [i32, i32, i32, i32, i32, View, f32, vp, u32, vp, vp, vp],
    "cgen_gauss_nll_fwd": [i32, i32, i32, i32, i32, View, View, View, vp, u32, vp, vp],
    "cgen_gauss_nll_bwd": [i32, i32, i32, i32, i32, View, View, View, vp, u32, vp, i32, View, vp],
    "cgen_gauss_sample": [i32, i32, i32, i32, i32, View, f32, vp, u32, vp, vp, vp],
    "cgen_dmol_nll_fwd": [i32, i32, i32, i32, View, View, vp, vp],
    "cgen_dmol_nll_bwd": [i32, i32, i32, i32, View, View, vp, i32, View, vp],
    "cgen_dmol_decode": [i32, i32, i32, i32, View, i32, vp, u32, f32, vp, vp, vp],
    "cgen_dmol_decode_bwd": [i32, i32, i32, i32, View, i32, vp, u32, f32, vp, vp, f32, View, vp],
    "cgen_elbo_finalize": [i32, vp, i32, f32, vp, i32, f32, f32, vp, vp, vp],
    "cgen_cf_dgauss_bwd": [i32, i32, i32, i32, i32, View, View, View, vp, f32, View, View, vp],
    "cgen_cf_dmol_bwd": [i32, i32, i32, i32, i32, View, View, View, vp, f32, View, View, vp],
    "cgen_cf_pixels": [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "cgen_sumsq_partial": [vp, i64, vp, i32, vp],
    "cgen_clip_decide": [vp, i32, vp, f32, f32, vp, vp],
    "cgen_adamw_ema": [C.POINTER(AdamwArgs), vp],
    "cgen_step_commit": [vp, vp],
    "cgen_adamw_ema_const_lr": [C.POINTER(AdamwArgs), vp],
    "cgen_nonfinite_partial": [i32, i32, i32, i32, View, vp, i32, vp],
    "cgen_cf_lagrange": [C.POINTER(CfLagrangeArgs), vp],
    "cgen_lagrange_step": [C.POINTER(LagrangeStepArgs), vp],
    "cgen_predictor_supported": [C.POINTER(PredHead), i32],
    "cgen_predictor_workspace": [C.POINTER(PredHead), i32, C.POINTER(i64)],
    "cgen_predictor_fwd": [C.POINTER(PredHead), i32, i32, vp, vp, vp, vp, vp, vp],
    "cgen_predictor_bwd": [C.POINTER(PredHead), i32, i32, vp, vp, vp, vp, vp],
    "cgen_predictor_tiled_supported": [C.POINTER(PredHead), i32],
    "cgen_predictor_tiled_workspace": [C.POINTER(PredHead), i32, i32, C.POINTER(i64)],
    "cgen_predictor_tiled_fwd": [C.POINTER(PredHead), i32, i32, vp, vp, i64, vp, vp, vp, vp],
    "cgen_predictor_tiled_bwd": [C.POINTER(PredHead), i32, i32, vp, vp, i64, vp, vp, vp],
    "cgen_predictor_tiled_plan": [C.POINTER(PredHead), i32, i32, C.POINTER(i32), i32, C.POINTER(i32)],
    "cgen_predictor_train_workspace": [C.POINTER(PredTrainHead), i32, i32, C.POINTER(i64)],
    "cgen_predictor_train_fwd": [C.POINTER(PredTrainHead), i32, i32, vp, vp, i64, f32, vp, vp, vp, vp],
    "cgen_predictor_train_bwd": [C.POINTER(PredTrainHead), i32, i32, vp, vp, i64, vp, vp, vp],
    "cgen_mlp_train_workspace": [C.POINTER(MlpTrainHead), i32, C.POINTER(i64)],
    "cgen_mlp_train_fwd": [C.POINTER(MlpTrainHead), i32, vp, i64, f32, vp, vp, vp],
    "cgen_mlp_train_bwd": [C.POINTER(MlpTrainHead), i32, vp, i64, vp, vp],
    "cgen_resnet_workspace": [i32, i32, C.POINTER(i64)],
    "cgen_resnet_site": [i32, i32, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)],
    "cgen_resnet_fwd": [C.POINTER(ResnetArgs), i32, vp, vp, i64, vp, vp, vp, vp],
    "cgen_resnet_bwd": [C.POINTER(ResnetArgs), i32, vp, i64, vp, vp, vp],
    "cgen_resnet_train_workspace": [i32, i32, C.POINTER(i64)],
    "cgen_resnet_train_fwd": [C.POINTER(ResnetTrainArgs), i32, vp, vp, i64, vp, vp, vp, vp],
    "cgen_resnet_train_bwd": [C.POINTER(ResnetTrainArgs), i32, vp, vp, i64, vp, vp, vp],
    "cgen_resnet_dropout_keep": [vp, f32, i32, i32, i32, vp, vp],
    "cgen_pgm_workspace": [C.POINTER(PgmMech), i32, i32, C.POINTER(i64)],
    "cgen_pgm_nll_fwd": [C.POINTER(PgmMech), i32, vp, i32, i64, vp, i32, vp, vp, vp],
    "cgen_pgm_nll_fwd_bwd": [C.POINTER(PgmMech), i32, vp, i32, i64, vp, i32, vp, vp, vp, vp, i64, vp],
    "cgen_pgm_counterfactual": [C.POINTER(PgmMech), i32, C.POINTER(PgmCfArgs), vp],
    "cgen_metric_accum": [C.POINTER(MetricVar), i32, i32, vp],
    "cgen_rocauc": [vp, vp, vp, i64, i32, i64, vp, vp, vp],
    "cgen_image_dist": [i32, i64, vp, vp, vp, vp, vp, vp],
    "cgen_philox_normal": [vp, i64, vp, u32, vp],
    "cgen_philox_uniform": [vp, i64, vp, u32, vp],
    "cgen_rng_advance": [vp, u64, vp],
}
_RESTYPES = {"cgen_last_error": C.c_char_p, "cgen_conv2d_last_kernel": C.c_char_p}
ABI_VERSION = 411  # CGEN_ABI_VERSION of include/cgen_hip.h this binding was written against
_NOCHECK = {"cgen_version", "cgen_h16_format", "cgen_last_error", "cgen_conv2d_wgrad_plan", "cgen_conv2d_wgrad_plan_record", "cgen_reparam_kl_chunks", "cgen_like_chunks",
            "cgen_block3_supported", "cgen_block4_supported", "cgen_block4_pair_supported", "cgen_block4_plan", "cgen_block4_pair_plan", "cgen_block3_pair_supported", "cgen_block3_pair_plan", "cgen_block3_plan", "cgen_conv2d_pair_supported", "cgen_stem_conv_supported",
            "cgen_predictor_supported", "cgen_predictor_tiled_supported", "cgen_batch_augment_arm", "cgen_latent_tail_bwd_supported", "cgen_latent_tail_fwd_supported",
            "cgen_dgauss_head_supported", "cgen_conv2d_last_kernel"}


class WgradBatchLaunch(C.Structure):
    _fields_ = [("ncf", C.c_int32), ("ks", C.c_int32), ("lds_bytes", C.c_int32), ("nblocks", C.c_int32), ("blocks_offset", C.c_int64)]


# C struct name -> its mirror, every struct of the header: a new struct is one more line here
STRUCTS = {
    "cgen_view": View,
    "cgen_conv_args": ConvArgs,
    "cgen_block3_out": Block3Out,
    "cgen_block3_args": Block3Args,
    "cgen_block4_args": Block4Args,
    "cgen_wgrad_args": WgradArgs,
    "cgen_wgrad_batch_launch": WgradBatchLaunch,
    "cgen_wprep_desc": WprepDesc,
    "cgen_wred_desc": WredDesc,
    "cgen_wred_item": WredItem,
    "cgen_augment_args": AugmentArgs,
    "cgen_latent_tail_bwd_args": LatentTailArgs,
    "cgen_latent_tail_fwd_args": LatentTailFwdArgs,
    "cgen_dgauss_head_args": DgaussHeadArgs,
    "cgen_pred_head": PredHead,
    "cgen_pred_train_head": PredTrainHead,
    "cgen_resnet_args": ResnetArgs,
    "cgen_resnet_train_args": ResnetTrainArgs,
    "cgen_mlp_train_head": MlpTrainHead,
    "cgen_metric_var": MetricVar,
    "cgen_pgm_mech": PgmMech,
    "cgen_pgm_pre": PgmPre,
    "cgen_pgm_cf_args": PgmCfArgs,
    "cgen_adamw_args": AdamwArgs,
    "cgen_cf_lagrange_args": CfLagrangeArgs,
    "cgen_lagrange_step_args": LagrangeStepArgs,
}


class CgenError(RuntimeError):
    pass


class _Lib:
    def __init__(self, path):
        self.path = path
        self.cdll = C.CDLL(path)
        for name, argtypes in PROTOTYPES.items():
            fn = getattr(self.cdll, name)  # AttributeError if the .so lacks a declared symbol
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int)
            setattr(self, "_raw_" + name, fn)
            setattr(self, name[len("cgen_"):], fn if name in _NOCHECK else self._checked(name, fn))
        if self.cdll.cgen_version() != ABI_VERSION:
            raise CgenError(f"{path}: ABI version {self.cdll.cgen_version()}, this binding needs {ABI_VERSION} -- a stale or foreign build "
                            "(rebuild with causal-gen_amd/build.sh)")
        # 16-bit storage format of THIS build: torch tensors handed over as CGEN_F16 must be in it
        self.h16_is_bf16 = bool(self.cdll.cgen_h16_format())

    def _checked(self, name, fn):
        def call(*a):
            rc = fn(*a)
            if rc != 0:
                raise CgenError(f"{name} failed ({rc}): {self.cdll.cgen_last_error().decode()}")
        call.__name__ = name
        return call


_LIB = None


def load():
    """Load libcgen_hip.so (no GPU needed).  Raises with build instructions when it is absent."""
    global _LIB
    if _LIB is None:
        # torch must be in the process first: it bundles its own libamdhip64, and the kernels here must launch
        # through the SAME HIP runtime instance that owns torch's streams and allocations.
        import torch  # noqa: F401

        if not os.path.exists(LIB_PATH):
            raise CgenError(f"{LIB_PATH} not found: build it with causal-gen_amd/build.sh "
                            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        _LIB = _Lib(LIB_PATH)
    return _LIB


def require_gpu():
    """The product path runs on an MI355X only; fail loudly otherwise."""
    import torch

    lib = load()
    if not torch.cuda.is_available():
        raise CgenError("causal-gen_amd needs a ROCm GPU (gfx950); torch.cuda.is_available() is False and there is "
                        "no CPU fallback by design")
    return lib
