"""ctypes binding of liblanpaint_hip.so (include/lanpaint_hip.h).

This is the whole host<->native boundary: plain pointers (`tensor.data_ptr()`),
sizes and two POD descriptors.  No pybind, no ATen linkage.  The library MUST be
present: there is no CPU or PyTorch fallback for the hot path -- a missing or
stale .so raises at import of the engine.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "liblanpaint_hip.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)
ABI_VERSION = 25

# --- constants mirrored from include/lanpaint_hip.h -------------------------------
LP_OK, LP_E_INVALID, LP_E_UNSUPPORTED, LP_E_LAUNCH, LP_E_ALIGN = 0, -1, -2, -3, -4
LP_COEF_STRIDE = 36
(LP_C_SCALE, LP_C_SQRT_ABT, LP_C_OMA, LP_C_ABT, LP_C_RSIGMA, LP_C_DTX, LP_C_DTY, LP_C_AX, LP_C_AY, LP_C_DX, LP_C_DY,
 LP_C_VALID) = range(12)
LP_C_REGION0, LP_C_REGION1, LP_C_TMODEL, LP_C_RSCALE = 12, 22, 32, 33
(LP_R_E_FULL, LP_R_K_FULL, LP_R_STD_FULL, LP_R_E_HALF, LP_R_K_HALF, LP_R_STD_HALF, LP_R_DT, LP_R_A, LP_R_CX0,
 LP_R_CXT) = range(10)

LP_PH_REPLACE, LP_PH_POST_FIRST, LP_PH_POST_STEADY, LP_PH_PRE_HALF, LP_PH_EMIT, LP_PH_COEFFS, LP_PH_SIGMA = 1, 2, 4, 8, 16, 32, 64
LP_FL_FLOW, LP_FL_MASK_DENOISE, LP_FL_MASK_U8, LP_FL_WRITE_X0S = 1, 2, 4, 8
LP_FL_X0_BF16, LP_FL_X0_F16, LP_FL_XIN_BF16, LP_FL_XIN_F16 = 16, 32, 64, 128
LP_FL_PER_ELEMENT, LP_FL_X0S_GIVEN, LP_FL_CFG_FUSED, LP_FL_MASK_BITS, LP_FL_NO_REGION_SKIP = 256, 512, 1024, 2048, 4096
LP_FL_ES, LP_FL_ES_GATED, LP_FL_ES_CLOSE, LP_FL_ES_RING_BITS, LP_FL_AV = 1 << 13, 1 << 14, 1 << 15, 1 << 16, 1 << 17
LP_TUNE_VEC1, LP_TUNE_VEC4, LP_TUNE_ES_NO_DECIDE, LP_TUNE_ES_NO_FOLD, LP_TUNE_ES_NO_ATOMICS = 1, 2, 4, 8, 16


def mask_bits_bytes(n_el: int) -> int:
    """LP_MASK_BITS_BYTES of the header."""
    return ((int(n_el) + 63) // 64) * 8
LP_REPLACE_KNOWN, LP_REPLACE_VE, LP_REPLACE_FLOW = 0, 1, 2
LP_RNG_PHILOX, LP_RNG_TORCH = 0, 1
LP_NN_ATEN_SCALAR, LP_NN_ATEN_CPU_GENERIC_FMA, LP_NN_ATEN_CPU_GENERIC = 0, 1, 2     # nearest-exact source-index rules
LP_RESHAPE_BINARIZE, LP_RESHAPE_RULE_SHIFT = 1, 8


class LpHyper(C.Structure):
    _fields_ = [("lambda_", C.c_float), ("beta", C.c_float), ("step_size", C.c_float), ("min_step_frac", C.c_float),
                ("is_flow", C.c_int32), ("one_plus_lambda", C.c_float)]


class LpStepDesc(C.Structure):
    _fields_ = [
        ("n_el", C.c_int64), ("el_per_row", C.c_int64), ("rows", C.c_int32), ("phases", C.c_uint32),
        ("flags", C.c_uint32), ("replace_kind", C.c_int32),
        ("lambda_", C.c_float), ("one_plus_lambda", C.c_float), ("beta", C.c_float), ("step_size", C.c_float),
        ("min_step_frac", C.c_float), ("noise_scale", C.c_float), ("cfg_scale", C.c_float), ("cfg_scale_big", C.c_float),
        ("coef", C.c_void_p), ("x", C.c_void_p), ("known", C.c_void_p), ("noise", C.c_void_p), ("y", C.c_void_p),
        ("mask", C.c_void_p), ("x_t", C.c_void_p), ("C", C.c_void_p), ("x0s", C.c_void_p), ("x0", C.c_void_p),
        ("x0_big", C.c_void_p), ("x_in", C.c_void_p), ("xi_post", C.c_void_p), ("xi_pre", C.c_void_p),
        ("rng_seed", C.c_uint64), ("rng_offset", C.c_uint64), ("rng_offset_ptr", C.c_void_p),
        ("abt_el", C.c_void_p), ("ve_el", C.c_void_p), ("rsig_el", C.c_void_p), ("corr_el", C.c_void_p),
        ("t_ve", C.c_void_p), ("t_abt", C.c_void_p), ("t_rsig", C.c_void_p), ("t_model", C.c_void_p),
        ("coef_out", C.c_void_p), ("t_ve_stride", C.c_int32), ("t_abt_stride", C.c_int32),
        ("t_rsig_stride", C.c_int32), ("t_model_stride", C.c_int32),
        ("rng_kind", C.c_int32), ("rng_bg", C.c_uint32), ("rng_inc", C.c_uint32),
        ("rng_state_out", C.c_void_p), ("rng_state_val", C.c_uint64 * 2),
        ("io_table_out", C.c_void_p), ("io_table_val", C.c_uint64 * 2),
        ("es", C.c_void_p), ("es_x0s", C.c_void_p * 3), ("es_ring", C.c_void_p), ("es_partials", C.c_void_p), ("es_host", C.c_void_p),
        ("es_threshold", C.c_double), ("es_seq_base", C.c_int64), ("es_patience_eff", C.c_int32), ("es_index", C.c_int32),
        ("es_n_steps", C.c_int32), ("es_reset", C.c_int32),
        ("sg_sigma", C.c_void_p), ("sg_schedule", C.c_void_p), ("sg_times_out", C.c_void_p), ("sg_scalars_out", C.c_void_p),
        ("sg_seq_out", C.c_void_p), ("sg_valid_out", C.c_void_p), ("sg_min_step_frac", C.c_double),
        ("sg_schedule_len", C.c_int32), ("sg_seq", C.c_int32), ("sg_n_steps", C.c_int32), ("sg_early_stop", C.c_int32),
        ("sg_total_steps", C.c_int32), ("sg_guess", C.c_int32), ("clk_out", C.c_void_p), ("av_bits", C.c_void_p), ("av_frac", C.c_float), ("reserved2", C.c_uint32),
        ("es_xte", C.c_void_p),
        ("tune", C.c_uint32), ("io_valid", C.c_uint32),
    ]


class LpEsState(C.Structure):
    _fields_ = [("stopped", C.c_int32), ("counter", C.c_int32), ("n_ran", C.c_int32), ("cur_slot", C.c_int32),
                ("anchor_slot", C.c_int32), ("write_slot", C.c_int32), ("reserved0", C.c_uint32), ("enabled", C.c_int32),
                ("seq_base", C.c_int64), ("total_ran", C.c_int64), ("threshold_eff", C.c_double), ("abt_val", C.c_double), ("x0s_buf", C.c_void_p * 3)]


LP_ES_SEQ_DONE, LP_ES_TRACE0 = 0x10000, 8
LP_ES_ACC_SLOTS, LP_ES_ACC_SETS = 64, 3
LP_ES_ACC_DOUBLES = LP_ES_ACC_SETS * LP_ES_ACC_SLOTS * 8


class LpFinalDesc(C.Structure):
    _fields_ = [
        ("n_el", C.c_int64), ("flags", C.c_uint32), ("cfg_scale", C.c_float),
        ("model_out", C.c_void_p), ("uncond", C.c_void_p), ("y", C.c_void_p), ("mask", C.c_void_p), ("x_src", C.c_void_p),
        ("x_dst", C.c_void_p), ("out", C.c_void_p), ("rng_bump_ptr", C.c_void_p), ("rng_bump", C.c_uint64),
        ("io_table", C.c_void_p),
    ]


class LpGraphBinding(C.Structure):
    _fields_ = [("node", C.c_void_p), ("func", C.c_void_p), ("grid", C.c_uint32 * 3), ("block", C.c_uint32 * 3),
                ("shared_bytes", C.c_uint32), ("reserved0", C.c_uint32)]


class LpCallDesc(C.Structure):
    _fields_ = [
        ("hyper", C.POINTER(LpHyper)),
        ("ve_sigma", C.c_void_p), ("ve_stride", C.c_int32),
        ("abt", C.c_void_p), ("abt_stride", C.c_int32),
        ("replace_sigma", C.c_void_p), ("rs_stride", C.c_int32),
        ("t_model", C.c_void_p), ("t_stride", C.c_int32),
        ("rows", C.c_int32),
        ("coef_table", C.c_void_p),
        ("replace", C.POINTER(LpStepDesc)),
        ("graph_exec", C.c_void_p),
        ("final", C.POINTER(LpFinalDesc)),
        ("replace_binding", C.POINTER(LpGraphBinding)),
    ]


class LpNodeCallDesc(C.Structure):
    _fields_ = [("sigma", C.c_void_p), ("rows", C.c_int32), ("schedule_len", C.c_int32), ("schedule", C.c_void_p),
                ("is_flow", C.c_int32), ("seq", C.c_int32), ("times_out", C.c_void_p), ("scalars_out", C.c_void_p),
                ("seq_out", C.c_void_p), ("replace", C.POINTER(LpStepDesc)), ("n_steps", C.c_int32),
                ("early_stop", C.c_int32), ("total_steps", C.c_int32), ("n_counts", C.c_int32),
                ("min_step_frac", C.c_double), ("exec_by_count", C.POINTER(C.c_void_p)), ("spin_limit", C.c_int32),
                ("guess", C.c_int32), ("valid_word", C.c_void_p), ("fold_sigma", C.c_int32), ("n_eff", C.c_int32), ("launched", C.c_int32),
                ("speculated", C.c_int32), ("hit", C.c_int32), ("step_f", C.c_float), ("frac", C.c_float),
                ("full_exec_by_count", C.POINTER(C.c_void_p)), ("full_binding_by_count", C.POINTER(C.POINTER(LpGraphBinding))),
                ("one_launch", C.c_int32), ("reserved0", C.c_int32)]


class LpBlendDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("k", C.c_int32), ("mask_batch", C.c_int32), ("mask_h", C.c_int32), ("mask_w", C.c_int32),
                ("mask", C.c_void_p), ("image1", C.c_void_p), ("image2", C.c_void_p), ("out", C.c_void_p),
                ("smooth_out", C.c_void_p), ("nn_rule", C.c_int32), ("reserved0", C.c_int32)]


LP_VMASK_MAX_SIDE, LP_VMASK_D2_NONE = 16384, -1
LP_VMASK_ZERO, LP_VMASK_KEY, LP_VMASK_INNER, LP_VMASK_OUT_U8 = 0, 1, 2, 1


class LpVmaskEdtDesc(C.Structure):
    _fields_ = [("n_keys", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("reserved0", C.c_int32),
                ("keys", C.c_void_p), ("d2", C.c_void_p), ("sdf", C.c_void_p), ("csum", C.c_void_p)]


class LpVmaskFrame(C.Structure):
    _fields_ = [("kind", C.c_int32), ("key_lo", C.c_int32), ("key_hi", C.c_int32), ("sx1", C.c_int32), ("sy1", C.c_int32),
                ("sx2", C.c_int32), ("sy2", C.c_int32), ("reserved0", C.c_int32), ("wf", C.c_double), ("omw", C.c_double)]


class LpVmaskMorphDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_keys", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("flags", C.c_uint32), ("reserved0", C.c_int32), ("frames", C.c_void_p), ("keys", C.c_void_p),
                ("sdf", C.c_void_p), ("out", C.c_void_p)]


class LpVmaskResizeDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("ksize_x", C.c_int32), ("ksize_y", C.c_int32), ("reserved0", C.c_int32),
                ("src", C.c_void_p), ("bounds_x", C.c_void_p), ("weights_x", C.c_void_p), ("bounds_y", C.c_void_p),
                ("weights_y", C.c_void_p), ("dst", C.c_void_p)]


class LpAudioDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("mask_len", C.c_int32), ("batch", C.c_int32), ("channels", C.c_int32), ("cf", C.c_int32),
                ("nn_rule", C.c_int32), ("orig_sb", C.c_int64), ("orig_sc", C.c_int64), ("inp_sb", C.c_int64),
                ("inp_sc", C.c_int64), ("mask", C.c_void_p), ("orig", C.c_void_p), ("inpainted", C.c_void_p),
                ("out", C.c_void_p), ("workspace", C.c_void_p)]


LP_DETAIL_MAX_SIDE, LP_DETAIL_MAX_CHANNELS = 32768, 64


class LpDetailResampleDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32), ("channels", C.c_int32),
                ("y0", C.c_int32), ("x0", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("ksize_x", C.c_int32), ("ksize_y", C.c_int32),
                ("src", C.c_void_p), ("bounds_x", C.c_void_p), ("weights_x", C.c_void_p), ("bounds_y", C.c_void_p),
                ("weights_y", C.c_void_p), ("dst", C.c_void_p)]


class LpDetailStitchDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("y0", C.c_int32), ("x0", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32),
                ("k", C.c_int32), ("mask_batch", C.c_int32),
                ("mask", C.c_void_p), ("original", C.c_void_p), ("detail", C.c_void_p), ("out", C.c_void_p)]


LP_DETAIL_MAX_COMPONENTS, LP_DETAIL_MAX_REGIONS = 4096, 64


class LpDetailResampleRegionsDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32), ("channels", C.c_int32),
                ("regions", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32), ("owner_len", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("ksize_x", C.c_int32), ("ksize_y", C.c_int32),
                ("origins", C.c_void_p), ("src", C.c_void_p), ("bounds_x", C.c_void_p), ("weights_x", C.c_void_p),
                ("bounds_y", C.c_void_p), ("weights_y", C.c_void_p), ("dst", C.c_void_p), ("labels", C.c_void_p),
                ("owner", C.c_void_p), ("scratch", C.c_void_p)]


class LpDetailStitchRegionsDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("regions", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32), ("k", C.c_int32),
                ("mask_batch", C.c_int32), ("owner_len", C.c_int32),
                ("origins", C.c_void_p), ("mask", C.c_void_p), ("original", C.c_void_p), ("detail", C.c_void_p),
                ("out", C.c_void_p), ("labels", C.c_void_p), ("owner", C.c_void_p)]


class LpDetailResampleTrackDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32), ("channels", C.c_int32),
                ("win_h", C.c_int32), ("win_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("ksize_x", C.c_int32), ("ksize_y", C.c_int32),
                ("origins", C.c_void_p), ("src", C.c_void_p), ("bounds_x", C.c_void_p), ("weights_x", C.c_void_p),
                ("bounds_y", C.c_void_p), ("weights_y", C.c_void_p), ("dst", C.c_void_p)]


class LpDetailStitchTrackDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("win_h", C.c_int32), ("win_w", C.c_int32), ("k", C.c_int32), ("mask_batch", C.c_int32),
                ("origins", C.c_void_p), ("mask", C.c_void_p), ("original", C.c_void_p), ("detail", C.c_void_p),
                ("out", C.c_void_p)]


class LpDetailResampleSubjectsDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32), ("channels", C.c_int32),
                ("subjects", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32), ("owner_len", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("ksize_x", C.c_int32), ("ksize_y", C.c_int32),
                ("origins", C.c_void_p), ("src", C.c_void_p), ("bounds_x", C.c_void_p), ("weights_x", C.c_void_p),
                ("bounds_y", C.c_void_p), ("weights_y", C.c_void_p), ("dst", C.c_void_p), ("labels", C.c_void_p),
                ("owner", C.c_void_p), ("scratch", C.c_void_p)]


class LpDetailStitchSubjectsDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("subjects", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32), ("k", C.c_int32),
                ("owner_len", C.c_int32), ("reserved0", C.c_int32),
                ("origins", C.c_void_p), ("mask", C.c_void_p), ("original", C.c_void_p), ("detail", C.c_void_p),
                ("out", C.c_void_p), ("labels", C.c_void_p), ("owner", C.c_void_p)]


LP_COLOR_MIN_COUNT, LP_COLOR_MAX_MARGIN, LP_COLOR_TILE_H, LP_COLOR_TILE_W = 64, 25, 32, 128
LP_COLOR_METHOD_MEAN, LP_COLOR_METHOD_MEAN_STD = 0, 1


class LpColorStatsDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("mask_batch", C.c_int32), ("margin", C.c_int32),
                ("detail", C.c_void_p), ("reference", C.c_void_p), ("mask", C.c_void_p), ("stats", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class LpColorFitDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("clip_frames", C.c_int32), ("smooth", C.c_int32),
                ("method", C.c_int32), ("reserved0", C.c_int32), ("strength", C.c_double),
                ("stats", C.c_void_p), ("coef", C.c_void_p)]


class LpColorApplyDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("detail", C.c_void_p), ("coef", C.c_void_p), ("out", C.c_void_p)]


def lp_color_ws_bytes(batch, height, width, channels):
    """LP_COLOR_WS_BYTES of include/lanpaint_hip.h."""
    tiles = ((int(height) + LP_COLOR_TILE_H - 1) // LP_COLOR_TILE_H) * ((int(width) + LP_COLOR_TILE_W - 1) // LP_COLOR_TILE_W)
    return int(batch) * tiles * (1 + 4 * int(channels)) * 8


LP_FILL_TILE, LP_FILL_SPAN = 32, 5


class LpFillDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("mask_batch", C.c_int32), ("reserved0", C.c_int32),
                ("image", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


class LpOutpaintDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("mask_batch", C.c_int32), ("left", C.c_int32), ("top", C.c_int32), ("right", C.c_int32),
                ("bottom", C.c_int32), ("overlap", C.c_int32), ("reserved0", C.c_int32),
                ("image", C.c_void_p), ("mask", C.c_void_p), ("image_out", C.c_void_p), ("mask_out", C.c_void_p)]


def fill_levels(height, width):
    """The sides of lp_mask_fill's pyramid levels 0 .. L - 1: halved, rounded up, down to (1, 1)."""
    levels = [(int(height), int(width))]
    while levels[-1] != (1, 1):
        h, w = levels[-1]
        levels.append(((h + 1) // 2, (w + 1) // 2))
    return levels


def fill_ws_bytes(batch, height, width, channels):
    """What the C entry lp_fill_ws_bytes returns for arguments inside the limits."""
    pix = sum(h * w for h, w in fill_levels(height, width)[1:])
    return max(16, (int(batch) * pix * (4 * int(channels) + 1) + 15) // 16 * 16)


LP_FILL_PATCH_MAX_RADIUS, LP_FILL_PATCH_MAX_LEVELS, LP_FILL_PATCH_MAX_ITERS, LP_FILL_PATCH_MAX_CHANNELS = 4, 6, 8, 4
LP_FILL_PATCH_TILE = 16
FILL_PATCH_PLANES = (("codes", 4), ("work", 4), ("nnf", 4), ("nnf2", 4), ("hole", 1), ("sets", 1))     # a level's planes, bytes an element


def LP_FILL_PATCH(r, levels, iters, seed):
    """The header's macro: lp_mask_fill's patch form as the int32 mode word of reserved0."""
    word = 1 | (r << 4) | (levels << 8) | (iters << 12) | (seed << 16)
    return word - (1 << 32) if word >= 1 << 31 else word


def fill_patch_levels(height, width, levels):
    """The sides of the patch form's levels 0 .. levels - 1: halved and rounded up."""
    return [(((int(height) - 1) >> l) + 1, ((int(width) - 1) >> l) + 1) for l in range(int(levels))]


def fill_patch_ws_layout(batch, height, width, channels, levels):
    """The patch form's workspace as the header lays it out: [{"h", "w", plane: byte offset of image 0's first element, ...}] for
    level 0 .. levels - 1; image b of a plane starts b * h * w elements further.  "nnf" is the field a level ends with."""
    at, out = fill_ws_bytes(batch, height, width, channels), []
    for h, w in fill_patch_levels(height, width, levels):
        level = {"h": h, "w": w}
        for name, size in FILL_PATCH_PLANES:
            level[name] = at
            at += (int(batch) * h * w * size + 15) // 16 * 16
        out.append(level)
    return out


def fill_patch_ws_bytes(batch, height, width, channels, levels):
    """LP_FILL_PATCH_WS_BYTES of include/lanpaint_hip.h over lp_fill_ws_bytes: what lp_mask_fill's patch form needs."""
    last = fill_patch_ws_layout(batch, height, width, channels, levels)[-1]
    return last["sets"] + (int(batch) * last["h"] * last["w"] + 15) // 16 * 16


class LpMultibandDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("mask_batch", C.c_int32), ("levels", C.c_int32),
                ("image1", C.c_void_p), ("image2", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p), ("ws", C.c_void_p),
                ("ws_bytes", C.c_int64)]


def multiband_levels(height, width, levels):
    """The sides of lp_multiband_blend's pyramid levels 0 .. n: halved, rounded up, `levels` times or until (1, 1)."""
    sizes = [(int(height), int(width))]
    while len(sizes) <= int(levels) and sizes[-1] != (1, 1):
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def multiband_ws_bytes(batch, height, width, channels, levels):
    """What the C entry lp_multiband_ws_bytes returns for arguments inside the limits."""
    pix = sum(h * w for h, w in multiband_levels(height, width, levels)[1:])
    return max(16, (int(batch) * pix * (2 * int(channels) + 1) * 4 + 15) // 16 * 16)


LP_FOCUS_MAX_RING, LP_FOCUS_MIN_COUNT, LP_FOCUS_MAX_VAR, LP_FOCUS_NO_FIT, LP_FOCUS_TILE, LP_FOCUS_TAPS = 8, 64, 16, -1.0, 32, 67


def LP_MULTIBAND_FOCUS(edge, ring, strength16, per_frame):
    """The header's macro: lp_multiband_blend's focus form as the (negative) int32 mode word of `levels`."""
    return ((0x80000000 | edge | (ring << 8) | (strength16 << 12) | (per_frame << 17)) & 0xFFFFFFFF) - (1 << 32)


def focus_ws_layout(batch, height, width, channels):
    """The focus form's workspace as the header's LP_FOCUS_WS_* macros lay it out: byte offsets of "flags" (uint8 [batch, th, tw]),
    "stats" (int64 [batch, 2, 3]), "var" (fp64 [batch, 2]), "K" (int32 [batch]), "taps" (fp32 [batch, 67]), "plane" (fp32
    [batch, height, width, channels]) and the total as "bytes"."""
    r16 = lambda n: (n + 15) // 16 * 16                              # noqa: E731
    b, h, w, c = int(batch), int(height), int(width), int(channels)
    tile = LP_FOCUS_TILE
    out = {"flags": 0}
    out["stats"] = r16(b * ((h + tile - 1) // tile) * ((w + tile - 1) // tile))
    out["var"] = out["stats"] + b * 48
    out["K"] = out["var"] + b * 16
    out["taps"] = out["K"] + r16(b * 4)
    out["plane"] = out["taps"] + r16(b * LP_FOCUS_TAPS * 4)
    out["bytes"] = out["plane"] + r16(b * h * w * c * 4)
    return out


def focus_ws_bytes(batch, height, width, channels):
    """LP_FOCUS_WS_BYTES of include/lanpaint_hip.h: what lp_multiband_ws_bytes returns for a focus word inside the limits."""
    return focus_ws_layout(batch, height, width, channels)["bytes"]


LP_REFINE_MAX_RADIUS = 64


class LpRefineDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("mask_batch", C.c_int32), ("radius", C.c_int32), ("eps", C.c_double),
                ("guide", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


def refine_ws_bytes(batch, height, width, channels, radius):
    """What the C entry lp_refine_ws_bytes returns for arguments inside the limits: (a_0, a_1, a_2, b) as fp32 per pixel."""
    return int(batch) * int(height) * int(width) * 16


LP_STAB_Q_FAR, LP_STAB_MAX_MEDIAN, LP_STAB_MAX_SMOOTH, LP_STAB_MAX_GROW, LP_STAB_MAX_FEATHER = 1 << 30, 3, 8, 256, 64
LP_STAB_SEG_FRAMES, LP_STAB_SD_CAP = 16, 64.0


class LpStabilizeDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("median_radius", C.c_int32), ("smooth_radius", C.c_int32), ("reserved0", C.c_int32),
                ("grow", C.c_double), ("feather", C.c_double), ("q", C.c_void_p), ("out", C.c_void_p)]


LP_GRAIN_BANDS, LP_GRAIN_MIN_COUNT, LP_GRAIN_WHITE_VAR, LP_GRAIN_MAX_STD, LP_GRAIN_MAX_MARGIN = 8, 64, 21845, 64, 25
LP_GRAIN_TILE_H, LP_GRAIN_TILE_W = 16, 64
LP_GRAIN_REGION_ALL, LP_GRAIN_REGION_OUTSIDE, LP_GRAIN_REGION_INSIDE = 0, 1, 2
LP_GRAIN_SIZE_AUTO, LP_GRAIN_MAX_FRAME0 = -1, 1 << 30


class LpGrainStatsDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("mask_batch", C.c_int32), ("margin", C.c_int32), ("flat", C.c_int32), ("region", C.c_int32),
                ("image", C.c_void_p), ("mask", C.c_void_p), ("stats", C.c_void_p)]


class LpGrainFitDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("ref_batch", C.c_int32), ("channels", C.c_int32), ("clip_frames", C.c_int32),
                ("size", C.c_int32), ("reserved0", C.c_int32), ("strength", C.c_double),
                ("gen", C.c_void_p), ("ref", C.c_void_p), ("amp", C.c_void_p), ("size_out", C.c_void_p)]


class LpGrainFieldDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("size", C.c_int32), ("monochrome", C.c_int32), ("frame0", C.c_int64), ("seed", C.c_uint64),
                ("out", C.c_void_p)]


class LpGrainApplyDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("mask_batch", C.c_int32), ("monochrome", C.c_int32), ("frame0", C.c_int64), ("seed", C.c_uint64),
                ("image", C.c_void_p), ("mask", C.c_void_p), ("amp", C.c_void_p), ("size", C.c_void_p), ("out", C.c_void_p)]


LP_PROP_BLOCK, LP_PROP_HALO, LP_PROP_MIN_PIXELS, LP_PROP_FILL_ITERS, LP_PROP_SUBPEL = 8, 4, 16, 3, 16
LP_PROP_MAX_LEVELS, LP_PROP_MAX_SEARCH, LP_PROP_MAX_SMOOTH, LP_PROP_ALIGN, LP_PROP_MAX_GRID = 6, 7, 64, 16, 2048


class LpPropLumaDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("levels", C.c_int32), ("reserved0", C.c_int32), ("image", C.c_void_p), ("pyramid", C.c_void_p)]


class LpPropMatchDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("levels", C.c_int32), ("level", C.c_int32),
                ("search", C.c_int32), ("smooth", C.c_int32), ("src", C.c_void_p), ("tgt", C.c_void_p), ("mask", C.c_void_p),
                ("parent", C.c_void_p), ("vec", C.c_void_p), ("valid", C.c_void_p)]


class LpPropAdvanceDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("levels", C.c_int32), ("reserved0", C.c_int32),
                ("vec", C.c_void_p), ("pos_src", C.c_void_p), ("key", C.c_void_p), ("pos_dst", C.c_void_p), ("out", C.c_void_p),
                ("mask_pyramid", C.c_void_p)]


LP_PROP_MAX_JOBS = 32
LP_PROP_MATCH_WARPED_KEY = 1                                         # LpPropMatchBatchDesc.reserved0: the source form


def LP_PROP_MATCH_GATED(occlusion):
    """The header's macro: the warped-key form with the occlusion gate, `occlusion` 1..255 in bits 8..15 of reserved0."""
    return LP_PROP_MATCH_WARPED_KEY | (occlusion << 8)


class LpPropMatchJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("tgt", C.c_void_p), ("mask", C.c_void_p), ("parent", C.c_void_p), ("vec", C.c_void_p),
                ("valid", C.c_void_p)]


class LpPropMatchBatchDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("levels", C.c_int32), ("level", C.c_int32),
                ("search", C.c_int32), ("smooth", C.c_int32), ("jobs", C.c_int32), ("reserved0", C.c_int32), ("job", C.c_void_p)]


class LpPropFillJob(C.Structure):
    _fields_ = [("vec", C.c_void_p), ("valid", C.c_void_p), ("out", C.c_void_p)]


class LpPropAdvanceJob(C.Structure):
    _fields_ = [("vec", C.c_void_p), ("pos_src", C.c_void_p), ("key", C.c_void_p), ("pos_dst", C.c_void_p), ("out", C.c_void_p),
                ("mask_pyramid", C.c_void_p)]


class LpPropAdvanceBatchDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("levels", C.c_int32), ("jobs", C.c_int32), ("job", C.c_void_p)]


class LpPropMergeDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("span", C.c_int32),
                ("first", C.c_int32), ("reserved0", C.c_int32), ("qa", C.c_void_p), ("qb", C.c_void_p), ("out", C.c_void_p)]


LP_PROP_VIS_MAX_BIAS = 32


class LpPropVisibleDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("occlusion", C.c_int32), ("reserved0", C.c_int32),
                ("pos", C.c_void_p), ("tgt", C.c_void_p), ("key", C.c_void_p), ("mask", C.c_void_p), ("flags", C.c_void_p)]


class LpPropOccludeDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("levels", C.c_int32), ("reserved0", C.c_int32),
                ("code", C.c_void_p), ("flags", C.c_void_p), ("out", C.c_void_p), ("hidden", C.c_void_p),
                ("mask_pyramid", C.c_void_p)]


class LpPropAnchorDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("anchor", C.c_int32), ("smooth", C.c_int32),
                ("pos", C.c_void_p), ("tgt", C.c_void_p), ("key", C.c_void_p), ("mask", C.c_void_p), ("vec", C.c_void_p),
                ("valid", C.c_void_p)]


class LpPropAnchorGatedDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("anchor", C.c_int32), ("smooth", C.c_int32),
                ("occlusion", C.c_int32), ("reserved0", C.c_int32),
                ("pos", C.c_void_p), ("tgt", C.c_void_p), ("key", C.c_void_p), ("mask", C.c_void_p), ("vec", C.c_void_p),
                ("valid", C.c_void_p), ("gated", C.c_void_p)]


class LpPropVisibleJob(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("tgt", C.c_void_p), ("key", C.c_void_p), ("mask", C.c_void_p), ("flags", C.c_void_p)]


class LpPropVisibleBatchDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("occlusion", C.c_int32), ("jobs", C.c_int32), ("job", C.c_void_p)]


class LpPropOccludeJob(C.Structure):
    _fields_ = [("code", C.c_void_p), ("flags", C.c_void_p), ("out", C.c_void_p), ("hidden", C.c_void_p),
                ("mask_pyramid", C.c_void_p), ("count", C.c_void_p)]


class LpPropOccludeBatchDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("levels", C.c_int32), ("jobs", C.c_int32), ("job", C.c_void_p)]


class LpPropMergeVisibleDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("span", C.c_int32),
                ("first", C.c_int32), ("reserved0", C.c_int32), ("qa", C.c_void_p), ("qb", C.c_void_p),
                ("code_a", C.c_void_p), ("mask_a", C.c_void_p), ("code_b", C.c_void_p), ("mask_b", C.c_void_p),
                ("flags_a", C.c_void_p), ("flags_b", C.c_void_p), ("count_a", C.c_void_p), ("count_b", C.c_void_p),
                ("out", C.c_void_p), ("hidden", C.c_void_p)]


LP_TFILL_MAX_REACH = 65535


class LpTfillKnownDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("levels", C.c_int32),
                ("mask_frames", C.c_int32), ("frame0", C.c_int32), ("mask", C.c_void_p), ("pyramid", C.c_void_p),
                ("source", C.c_void_p), ("remaining", C.c_void_p)]


class LpTfillCarryDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("frame", C.c_int32), ("donor", C.c_int32), ("reach", C.c_int32), ("nearer", C.c_int32),
                ("vec", C.c_void_p), ("known", C.c_void_p), ("donor_known", C.c_void_p), ("org_src", C.c_void_p),
                ("pos_src", C.c_void_p), ("org_dst", C.c_void_p), ("pos_dst", C.c_void_p), ("images", C.c_void_p),
                ("filled", C.c_void_p), ("source", C.c_void_p), ("remaining", C.c_void_p)]


LP_TFILL_DISPUTED = -2


class LpTfillCarryPairDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("frame", C.c_int32), ("donor", C.c_int32), ("reach", C.c_int32), ("agree", C.c_int32),
                ("vec", C.c_void_p), ("known", C.c_void_p), ("donor_known", C.c_void_p), ("org_src", C.c_void_p),
                ("pos_src", C.c_void_p), ("org_dst", C.c_void_p), ("pos_dst", C.c_void_p), ("images", C.c_void_p),
                ("filled", C.c_void_p), ("source", C.c_void_p), ("remaining", C.c_void_p), ("witnesses", C.c_void_p)]


LP_TSMOOTH_MAX_RADIUS = 8


class LpTsmoothDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("first", C.c_int32), ("count", C.c_int32), ("radius", C.c_int32), ("tolerance", C.c_int32),
                ("fwd_first", C.c_int32), ("fwd_count", C.c_int32), ("bwd_first", C.c_int32), ("bwd_count", C.c_int32),
                ("fwd", C.c_void_p), ("bwd", C.c_void_p), ("known", C.c_void_p), ("known_stride", C.c_int64),
                ("images", C.c_void_p), ("out", C.c_void_p), ("support", C.c_void_p)]


LP_TSMOOTH_ROBUST_QUORUM = 2


class LpTsmoothRobustDesc(C.Structure):
    _fields_ = LpTsmoothDesc._fields_ + [("replaced", C.c_void_p)]


LP_SHOT_MAX_SEARCH = 3
LP_SHOT_MAX_WINDOW = 16
LP_SHOT_BINS = 64


class LpShotMeasureDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("search", C.c_int32),
                ("plane", C.c_void_p), ("stride", C.c_int64), ("hist", C.c_void_p), ("score", C.c_void_p)]


class LpShotDecideDesc(C.Structure):
    _fields_ = [("frames", C.c_int32), ("threshold", C.c_int32), ("hist", C.c_int32), ("ratio", C.c_int32),
                ("window", C.c_int32), ("reserved0", C.c_int32), ("n_pixels", C.c_int64), ("score", C.c_void_p),
                ("shot", C.c_void_p)]


def prop_level_shape(height, width, level):
    """Level `level` of a height x width plane: ceil(height / 2^level) x ceil(width / 2^level)."""
    return (int(height) + (1 << level) - 1) >> level, (int(width) + (1 << level) - 1) >> level


def prop_level_offset(height, width, level):
    """Where level `level` starts in a frame's pyramid: every level LP_PROP_ALIGN-aligned behind the one below."""
    off = 0
    for k in range(level):
        h, w = prop_level_shape(height, width, k)
        off += (h * w + LP_PROP_ALIGN - 1) // LP_PROP_ALIGN * LP_PROP_ALIGN
    return off


def prop_pyramid_ws_bytes(frames, height, width, levels):
    """What the C entry lp_prop_pyramid_ws_bytes returns for arguments inside the limits."""
    return int(frames) * prop_level_offset(height, width, levels)


def prop_grid(height, width, level=0):
    """The block grid of a level: ceil(h_l / 8) x ceil(w_l / 8)."""
    h, w = prop_level_shape(height, width, level)
    return (h + LP_PROP_BLOCK - 1) // LP_PROP_BLOCK, (w + LP_PROP_BLOCK - 1) // LP_PROP_BLOCK


def lp_components_ws_bytes(height, width):
    """LP_COMPONENTS_WS_BYTES of include/lanpaint_hip.h."""
    return ((int(height) * int(width) + 1023) // 1024) * 4100


def lp_components_frames_ws_bytes(frames, height, width):
    """LP_COMPONENTS_FRAMES_WS_BYTES of include/lanpaint_hip.h."""
    return ((int(frames) * int(height) * int(width) + 1023) // 1024) * 4100


def lp_audio_ws_bytes(mask_len):
    """LP_AUDIO_WS_BYTES of include/lanpaint_hip.h."""
    return 12 * (int(mask_len) + 1)


EXPORTS = {
    # name: (restype, argtypes)
    "lp_abi_version": (C.c_int, []),
    "lp_strerror": (C.c_char_p, [C.c_int]),
    "lp_coeffs": (C.c_int, [C.POINTER(LpHyper), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                            C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lp_sigma_times": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lp_sigma_times_mailbox": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_void_p]),
    "lp_step": (C.c_int, [C.POINTER(LpStepDesc), C.c_void_p]),
    "lp_finalize": (C.c_int, [C.POINTER(LpFinalDesc), C.c_void_p]),
    "lp_mask_blend": (C.c_int, [C.POINTER(LpBlendDesc), C.c_void_p]),
    "lp_timer_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "lp_timer_destroy": (C.c_int, [C.c_void_p]),
    "lp_step_timed": (C.c_int, [C.POINTER(LpStepDesc), C.c_void_p, C.c_void_p]),
    "lp_step_timed_burst": (C.c_int, [C.POINTER(LpStepDesc), C.c_void_p, C.POINTER(C.c_void_p), C.c_int32]),
    "lp_timer_elapsed_ns": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "lp_replay_burst": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(LpStepDesc), C.POINTER(LpStepDesc), C.c_int32, C.c_void_p]),
    "lp_torch_normal": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "lp_philox_normal": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "lp_boundary_ring": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "lp_wmse_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                               C.c_int32, C.c_void_p]),
    "lp_replay_call": (C.c_int, [C.POINTER(LpCallDesc), C.c_void_p]),
    "lp_graph_bind_replace": (C.c_int, [C.c_void_p, C.POINTER(LpStepDesc), C.POINTER(LpGraphBinding)]),
    "lp_graph_clone_tail": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "lp_graph_release": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lp_graph_clone_sigma_root": (C.c_int, [C.c_void_p, C.POINTER(LpStepDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(LpGraphBinding)]),
    "lp_node_call": (C.c_int, [C.POINTER(LpNodeCallDesc), C.c_void_p]),
    "lp_effective_inner_steps": (C.c_int32, [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double]),
    "lp_pack_mask": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lp_pack_mask_latent": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lp_reshape_mask": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p]),
    "lp_vmask_edt": (C.c_int, [C.POINTER(LpVmaskEdtDesc), C.c_void_p]),
    "lp_vmask_morph": (C.c_int, [C.POINTER(LpVmaskMorphDesc), C.c_void_p]),
    "lp_vmask_resize": (C.c_int, [C.POINTER(LpVmaskResizeDesc), C.c_void_p]),
    "lp_audio_merge": (C.c_int, [C.POINTER(LpAudioDesc), C.c_void_p]),
    "lp_mask_bbox": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lp_detail_resample": (C.c_int, [C.POINTER(LpDetailResampleDesc), C.c_void_p]),
    "lp_detail_stitch": (C.c_int, [C.POINTER(LpDetailStitchDesc), C.c_void_p]),
    "lp_mask_components": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p]),
    "lp_detail_resample_regions": (C.c_int, [C.POINTER(LpDetailResampleRegionsDesc), C.c_void_p]),
    "lp_detail_stitch_regions": (C.c_int, [C.POINTER(LpDetailStitchRegionsDesc), C.c_void_p]),
    "lp_mask_bbox_frames": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lp_detail_resample_track": (C.c_int, [C.POINTER(LpDetailResampleTrackDesc), C.c_void_p]),
    "lp_detail_stitch_track": (C.c_int, [C.POINTER(LpDetailStitchTrackDesc), C.c_void_p]),
    "lp_mask_components_frames": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_void_p]),
    "lp_subject_boxes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "lp_detail_resample_subjects": (C.c_int, [C.POINTER(LpDetailResampleSubjectsDesc), C.c_void_p]),
    "lp_detail_stitch_subjects": (C.c_int, [C.POINTER(LpDetailStitchSubjectsDesc), C.c_void_p]),
    "lp_color_stats": (C.c_int, [C.POINTER(LpColorStatsDesc), C.c_void_p]),
    "lp_color_fit": (C.c_int, [C.POINTER(LpColorFitDesc), C.c_void_p]),
    "lp_color_apply": (C.c_int, [C.POINTER(LpColorApplyDesc), C.c_void_p]),
    "lp_mask_fill": (C.c_int, [C.POINTER(LpFillDesc), C.c_void_p]),
    "lp_fill_ws_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lp_outpaint_pad": (C.c_int, [C.POINTER(LpOutpaintDesc), C.c_void_p]),
    "lp_multiband_blend": (C.c_int, [C.POINTER(LpMultibandDesc), C.c_void_p]),
    "lp_multiband_ws_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lp_mask_refine": (C.c_int, [C.POINTER(LpRefineDesc), C.c_void_p]),
    "lp_refine_ws_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lp_mask_signed_d2": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lp_mask_stabilize": (C.c_int, [C.POINTER(LpStabilizeDesc), C.c_void_p]),
    "lp_grain_stats": (C.c_int, [C.POINTER(LpGrainStatsDesc), C.c_void_p]),
    "lp_grain_fit": (C.c_int, [C.POINTER(LpGrainFitDesc), C.c_void_p]),
    "lp_grain_field": (C.c_int, [C.POINTER(LpGrainFieldDesc), C.c_void_p]),
    "lp_grain_apply": (C.c_int, [C.POINTER(LpGrainApplyDesc), C.c_void_p]),
    "lp_prop_pyramid_ws_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lp_prop_luma": (C.c_int, [C.POINTER(LpPropLumaDesc), C.c_void_p]),
    "lp_prop_key_mask": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lp_prop_match": (C.c_int, [C.POINTER(LpPropMatchDesc), C.c_void_p]),
    "lp_prop_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lp_prop_advance": (C.c_int, [C.POINTER(LpPropAdvanceDesc), C.c_void_p]),
    "lp_prop_match_batch": (C.c_int, [C.POINTER(LpPropMatchBatchDesc), C.c_void_p]),
    "lp_prop_fill_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lp_prop_advance_batch": (C.c_int, [C.POINTER(LpPropAdvanceBatchDesc), C.c_void_p]),
    "lp_prop_merge": (C.c_int, [C.POINTER(LpPropMergeDesc), C.c_void_p]),
    "lp_prop_visible": (C.c_int, [C.POINTER(LpPropVisibleDesc), C.c_void_p]),
    "lp_prop_occlude": (C.c_int, [C.POINTER(LpPropOccludeDesc), C.c_void_p]),
    "lp_prop_visible_batch": (C.c_int, [C.POINTER(LpPropVisibleBatchDesc), C.c_void_p]),
    "lp_prop_occlude_batch": (C.c_int, [C.POINTER(LpPropOccludeBatchDesc), C.c_void_p]),
    "lp_prop_merge_visible": (C.c_int, [C.POINTER(LpPropMergeVisibleDesc), C.c_void_p]),
    "lp_prop_anchor_match": (C.c_int, [C.POINTER(LpPropAnchorDesc), C.c_void_p]),
    "lp_prop_anchor_match_gated": (C.c_int, [C.POINTER(LpPropAnchorGatedDesc), C.c_void_p]),
    "lp_tfill_known": (C.c_int, [C.POINTER(LpTfillKnownDesc), C.c_void_p]),
    "lp_tfill_carry": (C.c_int, [C.POINTER(LpTfillCarryDesc), C.c_void_p]),
    "lp_tfill_carry_pair": (C.c_int, [C.POINTER(LpTfillCarryPairDesc), C.c_void_p]),
    "lp_tsmooth": (C.c_int, [C.POINTER(LpTsmoothDesc), C.c_void_p]),
    "lp_tsmooth_robust": (C.c_int, [C.POINTER(LpTsmoothRobustDesc), C.c_void_p]),
    "lp_shot_measure": (C.c_int, [C.POINTER(LpShotMeasureDesc), C.c_void_p]),
    "lp_shot_decide": (C.c_int, [C.POINTER(LpShotDecideDesc), C.c_void_p]),
}


class LanPaintHipError(RuntimeError):
    """A C-ABI call returned a negative status (the reference raises Python
    exceptions only; C codes are mapped to RuntimeError here)."""


_lib = None


def load(path: str | None = None):
    """dlopen the HIP library once; raise loudly when it is missing or stale."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("LANPAINT_AMD_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `python -m lanpaint_amd.build`). lanpaint_amd has no CPU / PyTorch fallback for the Langevin path.")
    lib = C.CDLL(p)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype, fn.argtypes = res, args
    v = lib.lp_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"{p}: ABI version {v}, expected {ABI_VERSION}; rebuild the extension")
    if path is None:
        _lib = lib
    return lib


def check(code: int, what: str = "lanpaint_hip"):
    if code != LP_OK:
        msg = load().lp_strerror(code)
        raise LanPaintHipError(f"{what}: {msg.decode() if msg else code} (code {code})")
