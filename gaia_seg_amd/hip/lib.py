"""ctypes binding of ``libgaiaseg_hip.so`` (C-ABI declared in ``include/gaiaseg_hip.h``).

The library is the product: there is no CPU or eager-PyTorch fallback anywhere in this package.
``load()`` raises ``HipLibraryError`` when the shared object is missing or does not export every
symbol of the header, and every wrapper in :mod:`gaia_seg_amd.hip.functional` raises on a non-zero
return code.
"""
import ctypes
import os
import subprocess
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t,
                    c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.path.join(PKG_ROOT, "lib", "libgaiaseg_hip.so")
CSRC_DIR = os.path.join(PKG_ROOT, "csrc")
ABI_VERSION = 27


class HipLibraryError(RuntimeError):
    pass


class ConvDesc(Structure):
    """Mirror of ``gs_conv_desc``."""
    _fields_ = [("N", c_int32), ("H", c_int32), ("W", c_int32), ("Ci", c_int32), ("Co", c_int32),
                ("Ci_max", c_int32), ("Co_ld", c_int32), ("KH", c_int32), ("KW", c_int32),
                ("stride", c_int32), ("pad", c_int32), ("dil", c_int32), ("Ho", c_int32),
                ("Wo", c_int32), ("x_sn", c_int64), ("x_sh", c_int64), ("x_sw", c_int64),
                ("x_sc", c_int64), ("ldy", c_int32), ("ld_add", c_int32),
                ("role", c_int32), ("reserved", c_int32), ("in_affine", c_void_p)]


def conv_out_size(h, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


def conv_desc(n, h, w, ci, co, k, stride=1, dil=1, pad=None, ci_max=None, co_ld=None, ldx=None,
              ldy=None, ld_add=0, role=0):
    """The one place that fills a ``ConvDesc``: a packed-NHWC input [n, h, w, ci] with row pitch
    ``ldx`` (default ci), a weight of ``ci_max`` (default ci) input channels and row pitch ``co_ld``
    (default co), ``k`` x ``k`` taps (or a (kh, kw) pair), 'same' padding ``dil * (k // 2)`` unless
    ``pad`` is given, output row pitch ``ldy`` (default co).  ``in_affine`` stays null."""
    kh, kw = k if isinstance(k, tuple) else (k, k)
    ldx = ci if ldx is None else ldx
    d = ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co = n, h, w, ci, co
    d.Ci_max = ci if ci_max is None else ci_max
    d.Co_ld = co if co_ld is None else co_ld
    d.KH, d.KW = kh, kw
    d.stride, d.pad, d.dil = stride, dil * (kh // 2) if pad is None else pad, dil
    d.Ho = conv_out_size(h, kh, stride, d.pad, dil)
    d.Wo = conv_out_size(w, kw, stride, d.pad, dil)
    d.x_sn, d.x_sh, d.x_sw, d.x_sc = h * w * ldx, w * ldx, ldx, 1
    d.ldy, d.ld_add = co if ldy is None else ldy, ld_add
    d.role = role
    return d


class DwConvDesc(Structure):
    """Mirror of ``gs_dwconv_desc``."""
    _fields_ = [(k, c_int32) for k in ("N", "H", "W", "C", "C_ld", "KH", "KW", "stride", "pad", "dil",
                                       "ldx", "ldy")]


def dwconv_desc(n, h, w, c, pad, dil=1, c_ld=None, ldx=None, ldy=None, k=3, stride=1):
    """A ``DwConvDesc`` for a packed-NHWC input [n, h, w, c] (row pitch ``ldx``, default c), a weight of
    tap pitch ``c_ld`` (default c) and output row pitch ``ldy`` (default c)."""
    d = DwConvDesc()
    d.N, d.H, d.W, d.C = n, h, w, c
    d.C_ld = c if c_ld is None else c_ld
    d.KH = d.KW = k
    d.stride, d.pad, d.dil = stride, pad, dil
    d.ldx, d.ldy = c if ldx is None else ldx, c if ldy is None else ldy
    return d


class MscaDesc(Structure):
    """Mirror of ``gs_msca_desc``."""
    _fields_ = ([(k, c_int32) for k in ("N", "H", "W", "C", "C_ld", "K0")] + [("K", c_int32 * 3)]
                + [("ldx", c_int32), ("lds", c_int32)])


class MscaFilters(Structure):
    """Mirror of ``gs_msca_filters`` and of ``gs_msca_filter_grads`` (the same 14 addresses)."""
    _fields_ = [("w0", c_void_p), ("b0", c_void_p), ("w_row", c_void_p * 3), ("b_row", c_void_p * 3),
                ("w_col", c_void_p * 3), ("b_col", c_void_p * 3)]


def msca_desc(n, h, w, c, c_ld=None, ldx=None, lds=None, k0=5, k=(7, 11, 21)):
    """A ``MscaDesc`` for a packed-NHWC map [n, h, w, c] (pixel pitch ``ldx`` of x / dx and ``lds`` of
    s / ds, default c) and filters of tap pitch ``c_ld`` (default c)."""
    d = MscaDesc()
    d.N, d.H, d.W, d.C = n, h, w, c
    d.C_ld = c if c_ld is None else c_ld
    d.K0 = k0
    d.K[0], d.K[1], d.K[2] = k
    d.ldx, d.lds = c if ldx is None else ldx, c if lds is None else lds
    return d


def msca_filters(w0, b0, w_row, b_row, w_col, b_col):
    """A ``MscaFilters`` of 14 addresses (ints or None): the filters, or their gradients."""
    f = MscaFilters()
    f.w0, f.b0 = w0, b0
    for i in range(3):
        f.w_row[i], f.b_row[i], f.w_col[i], f.b_col[i] = w_row[i], b_row[i], w_col[i], b_col[i]
    return f


class LayerNormDesc(Structure):
    """Mirror of ``gs_layernorm_desc``."""
    _fields_ = [("rows", c_int64), ("C", c_int32), ("ldx", c_int32), ("ldy", c_int32), ("eps", c_float)]


def layernorm_desc(rows, c, eps=1e-6, ldx=None, ldy=None):
    """A ``LayerNormDesc`` for ``rows`` pixels of ``c`` active channels; pitches default to c."""
    d = LayerNormDesc()
    d.rows, d.C, d.eps = rows, c, eps
    d.ldx, d.ldy = c if ldx is None else ldx, c if ldy is None else ldy
    return d


class GeluGrnDesc(Structure):
    """Mirror of ``gs_gelu_grn_desc``."""
    _fields_ = [(k, c_int32) for k in ("N", "P", "C", "ldx", "ldy", "lddy", "lddx")] + [("eps", c_float)]


def gelu_grn_desc(n, p, c, eps=1e-6, ldx=None, ldy=None, lddy=None, lddx=None):
    """A ``GeluGrnDesc`` for ``n`` samples of ``p`` pixels with ``c`` active channels; pitches default to c."""
    d = GeluGrnDesc()
    d.N, d.P, d.C, d.eps = n, p, c, eps
    d.ldx, d.ldy = c if ldx is None else ldx, c if ldy is None else ldy
    d.lddy, d.lddx = c if lddy is None else lddy, c if lddx is None else lddx
    return d


class AttentionDesc(Structure):
    """Mirror of ``gs_attention_desc``."""
    _fields_ = ([(k, c_int32) for k in ("B", "N", "heads", "ldq", "ldk", "ldv", "ldo", "lddq", "lddk", "lddv",
                                        "lddo")] + [("scale", c_float)])


ATTENTION_HEAD_DIM = 64
ATTENTION_RELPOS_MAX_ROWS = 8192   # GS_ATTENTION_RELPOS_MAX_ROWS


def _fill_pitches(d, c, **pitches):
    """Set the pitch fields of descriptor ``d`` from keywords named like them, forward pitches first:
    a forward pitch (``ldX``) given as None becomes ``c``, a gradient's pitch (``lddX``) the pitch of
    its forward operand ``ldX``."""
    for name, v in pitches.items():
        if v is None:
            v = getattr(d, "ld" + name[3:]) if name.startswith("ldd") else c
        setattr(d, name, v)


def attention_desc(b, n, heads, scale=ATTENTION_HEAD_DIM ** -0.5, ldq=None, ldk=None, ldv=None, ldo=None,
                   lddq=None, lddk=None, lddv=None, lddo=None):
    """An ``AttentionDesc`` for ``b`` images of ``n`` tokens and ``heads`` active heads; a forward pitch
    defaults to 64 * heads, a gradient's pitch to the pitch of its forward operand."""
    d = AttentionDesc()
    d.B, d.N, d.heads, d.scale = b, n, heads, scale
    _fill_pitches(d, ATTENTION_HEAD_DIM * heads, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo,
                  lddq=lddq, lddk=lddk, lddv=lddv, lddo=lddo)
    return d


class AttentionKvDesc(Structure):
    """Mirror of ``gs_attention_kv_desc``."""
    _fields_ = ([(k, c_int32) for k in ("B", "Nq", "Nk", "heads", "ldq", "ldk", "ldv", "ldo", "lddq", "lddk",
                                        "lddv", "lddo")] + [("scale", c_float)])


def attention_kv_desc(b, nq, nk, heads, scale=ATTENTION_HEAD_DIM ** -0.5, ldq=None, ldk=None, ldv=None, ldo=None,
                      lddq=None, lddk=None, lddv=None, lddo=None):
    """An ``AttentionKvDesc`` for ``b`` images of ``nq`` queries and ``nk`` keys and ``heads`` active heads;
    pitches default as in ``attention_desc``."""
    d = AttentionKvDesc()
    d.B, d.Nq, d.Nk, d.heads, d.scale = b, nq, nk, heads, scale
    _fill_pitches(d, ATTENTION_HEAD_DIM * heads, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo,
                  lddq=lddq, lddk=lddk, lddv=lddv, lddo=lddo)
    return d


class WindowAttentionDesc(Structure):
    """Mirror of ``gs_window_attention_desc``."""
    _fields_ = ([(k, c_int32) for k in ("B", "H", "W", "ws", "shift", "heads", "ldq", "ldk", "ldv", "ldo", "lddq",
                                        "lddk", "lddv", "lddo", "ld_table")] + [("scale", c_float)])


WINDOW_ATTENTION_HEAD_DIM = 32


def window_attention_desc(b, h, w, ws, shift, heads, ld_table=None, scale=WINDOW_ATTENTION_HEAD_DIM ** -0.5,
                          ldq=None, ldk=None, ldv=None, ldo=None, lddq=None, lddk=None, lddv=None, lddo=None):
    """A ``WindowAttentionDesc`` for ``b`` padded maps of ``h`` x ``w`` tokens, ``ws`` x ``ws`` windows shifted by
    ``shift`` and ``heads`` active heads; pitches default as in ``attention_desc`` (32 * heads), the table's
    pitch to ``heads``."""
    d = WindowAttentionDesc()
    d.B, d.H, d.W, d.ws, d.shift, d.heads, d.scale = b, h, w, ws, shift, heads, scale
    d.ld_table = heads if ld_table is None else ld_table
    _fill_pitches(d, WINDOW_ATTENTION_HEAD_DIM * heads, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo,
                  lddq=lddq, lddk=lddk, lddv=lddv, lddo=lddo)
    return d


class CellLayerNormDesc(Structure):
    """Mirror of ``gs_cell_layernorm_desc``."""
    _fields_ = ([(k, c_int32) for k in ("B", "H", "W", "C", "Cmax", "ldx", "ldy")] + [("eps", c_float)])


def cell_layernorm_desc(b, h, w, c, cmax=None, eps=1e-5, ldx=None, ldy=None):
    """A ``CellLayerNormDesc`` for ``b`` maps of ``h`` x ``w`` pixels of ``c`` active channels under parameter
    groups of ``cmax`` (default c) channels; pitches default to c."""
    d = CellLayerNormDesc()
    d.B, d.H, d.W, d.C, d.eps = b, h, w, c, eps
    d.Cmax = c if cmax is None else cmax
    d.ldx, d.ldy = c if ldx is None else ldx, c if ldy is None else ldy
    return d


class FcuDownDesc(Structure):
    """Mirror of ``gs_fcu_down_desc``."""
    _fields_ = ([(k, c_int32) for k in ("B", "T", "D", "ldz", "ldxt", "ldo", "lddz", "lddxt")]
                + [("eps", c_float)])


def fcu_down_desc(b, t, d, eps=1e-6, ldz=None, ldxt=None, ldo=None, lddz=None, lddxt=None):
    """A ``FcuDownDesc`` for ``b`` images of ``t`` tokens (+ the cls row) of width ``d``; a forward pitch
    defaults to d, a gradient's pitch to the pitch of its forward operand."""
    desc = FcuDownDesc()
    desc.B, desc.T, desc.D, desc.eps = b, t, d, eps
    _fill_pitches(desc, d, ldz=ldz, ldxt=ldxt, ldo=ldo, lddz=lddz, lddxt=lddxt)
    return desc


OCR_MAX_CLASSES = 256             # GS_OCR_MAX_CLASSES
OCR_GATHER_MAX_CHANNELS = 2048    # GS_OCR_GATHER_MAX_CHANNELS
OCR_ATTEND_MAX_CHANNELS = 512     # GS_OCR_ATTEND_MAX_CHANNELS


class OcrGatherDesc(Structure):
    """Mirror of ``gs_ocr_gather_desc``."""
    _fields_ = ([(k, c_int32) for k in ("B", "P", "K", "C", "ldl", "ldf", "ldc", "lddl", "lddf", "lddc")]
                + [("scale", c_float)])


def ocr_gather_desc(b, p, k, c, scale=1.0, ldl=None, ldf=None, ldc=None, lddl=None, lddf=None, lddc=None):
    """An ``OcrGatherDesc`` for ``b`` images of ``p`` pixels, ``k`` classes and ``c`` active feature
    channels; the logits' pitch defaults to round_up(k, 4), the others to c, a gradient's pitch to the pitch
    of its forward operand."""
    d = OcrGatherDesc()
    d.B, d.P, d.K, d.C, d.scale = b, p, k, c, scale
    d.ldl = (k + 3) // 4 * 4 if ldl is None else ldl
    _fill_pitches(d, c, ldf=ldf, ldc=ldc, lddl=lddl, lddf=lddf, lddc=lddc)
    return d


class OcrAttendDesc(Structure):
    """Mirror of ``gs_ocr_attend_desc``."""
    _fields_ = [(k, c_int32) for k in ("B", "P", "K", "ch", "ldq", "ldk", "ldv", "ldo", "lddq", "lddk", "lddv",
                                       "lddo")]


def ocr_attend_desc(b, p, k, ch, ldq=None, ldk=None, ldv=None, ldo=None, lddq=None, lddk=None, lddv=None,
                    lddo=None):
    """An ``OcrAttendDesc`` for ``b`` images of ``p`` pixels and ``k`` regions of width ``ch``; a forward pitch
    defaults to ch, a gradient's pitch to the pitch of its forward operand."""
    d = OcrAttendDesc()
    d.B, d.P, d.K, d.ch = b, p, k, ch
    _fill_pitches(d, ch, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, lddq=lddq, lddk=lddk, lddv=lddv, lddo=lddo)
    return d


class BnArgs(Structure):
    """Mirror of ``gs_bn_args``."""
    _fields_ = [("gamma", c_void_p), ("beta", c_void_p), ("running_mean", c_void_p),
                ("running_var", c_void_p), ("eps", c_float), ("momentum", c_float),
                ("use_batch_stats", c_int32), ("update_running", c_int32), ("relu", c_int32),
                ("reserved", c_int32), ("relu_mask", c_void_p), ("residual_coeffs", c_void_p)]


class BnBwdFuse(Structure):
    """Mirror of ``gs_bn_bwd_fuse``."""
    _fields_ = [("y", c_void_p), ("act", c_void_p), ("coeffs", c_void_p), ("sums", c_void_p),
                ("fused", POINTER(c_int32)), ("ldy", c_int32), ("ldact", c_int32), ("mode", c_int32),
                ("reserved", c_int32), ("mask", c_void_p), ("ldmask", c_int32), ("reserved2", c_int32)]


class DebugLaunch(Structure):
    """Mirror of ``gs_debug_launch``."""
    _fields_ = [(k, c_int32) for k in ("op", "kloop", "bm", "bn", "splits", "ksteps_per_split",
                                       "in_affine", "bn_bwd_mode")]


OP_FORWARD, OP_DGRAD, OP_WGRAD = 0, 1, 2
KLOOP_GENERIC, KLOOP_FP32, KLOOP_FP32_PAIRS, KLOOP_BF16X3, KLOOP_STREAM = 0, 1, 2, 3, 4
KLOOP_COUNT = 5
# fp16 modes only (set_forward_precision(1), set_train_precision(1)): not a slot of the count / FLOP
# tables, which keep KLOOP_COUNT entries per op; gs_debug_f16_launches(_by_op) counts it
KLOOP_F16 = 5
# gs_set_forward_precision / gs_set_train_precision modes.  FP16: the fast forward launches (and, in
# training mode, the fast data-gradient launches) round both operands once to fp16 (round to nearest
# even, the input after its fp32 in_affine BN + ReLU) and accumulate in fp32 on
# v_mfma_f32_16x16x32_f16; outputs, BN, residual and split-K stay fp32 (include/gaiaseg_hip.h).
PRECISION_FP32, PRECISION_FP16 = 0, 1


class CeDesc(Structure):
    """Mirror of ``gs_ce_desc``."""
    _fields_ = [("N", c_int32), ("h", c_int32), ("w", c_int32), ("Cls", c_int32), ("H", c_int32),
                ("W", c_int32), ("l_sn", c_int64), ("l_sh", c_int64), ("l_sw", c_int64),
                ("l_sc", c_int64), ("ignore_index", c_int32), ("align_corners", c_int32)]


class KdDesc(Structure):
    """Mirror of ``gs_kd_desc``."""
    _fields_ = [("N", c_int32), ("h", c_int32), ("w", c_int32), ("Cls", c_int32), ("H", c_int32),
                ("W", c_int32), ("s_sn", c_int64), ("s_sh", c_int64), ("s_sw", c_int64),
                ("s_sc", c_int64), ("t_sn", c_int64), ("t_sh", c_int64), ("t_sw", c_int64),
                ("t_sc", c_int64), ("T", c_float), ("align_corners", c_int32),
                ("interpolation", c_int32), ("reserved", c_int32)]


class DistillDesc(Structure):
    """Mirror of ``gs_distill_desc``."""
    _fields_ = [("N", c_int32), ("Cls", c_int32), ("hs", c_int32), ("ws", c_int32), ("ht", c_int32),
                ("wt", c_int32), ("H", c_int32), ("W", c_int32), ("s_sn", c_int64), ("s_sh", c_int64),
                ("s_sw", c_int64), ("s_sc", c_int64), ("t_sn", c_int64), ("t_sh", c_int64),
                ("t_sw", c_int64), ("t_sc", c_int64), ("T", c_float), ("align_corners", c_int32)]


PAIRWISE_MAX_P = 128   # GS_PAIRWISE_MAX_P


class PairwiseDesc(Structure):
    """Mirror of ``gs_pairwise_desc``."""
    _fields_ = ([(k, c_int32) for k in ("N", "Cs", "Ct", "H", "W", "Ht", "Wt", "y0", "y1", "x0", "x1",
                                        "reserved")] +
                [(k, c_int64) for k in ("s_sn", "s_sc", "s_sh", "s_sw", "t_sn", "t_sc", "t_sh", "t_sw")] +
                [("T", c_float), ("reserved2", c_int32)])


class CwdDesc(Structure):
    """Mirror of ``gs_cwd_desc``."""
    _fields_ = ([(k, c_int32) for k in ("N", "C", "H", "W")] +
                [(k, c_int64) for k in ("s_sn", "s_sc", "s_sh", "s_sw", "t_sn", "t_sc", "t_sh", "t_sw")] +
                [("T", c_float), ("reserved", c_int32)])


class SlideDesc(Structure):
    """Mirror of ``gs_slide_desc``."""
    _fields_ = [(k, c_int32) for k in ("N", "C", "ld", "hl", "wl", "hc", "wc", "H", "W", "Ho", "Wo",
                                       "ny", "nx", "align_corners", "flip", "reserved")]


class AugmentDesc(Structure):
    """Mirror of ``gs_augment_desc``."""
    _fields_ = ([(k, c_int32) for k in ("src_h", "src_w", "src_is_rgb", "res_h", "res_w", "crop_y",
                                        "crop_x", "crop_h", "crop_w", "out_h", "out_w", "flip",
                                        "pm_enable", "pm_brightness", "pm_contrast",
                                        "pm_contrast_first", "pm_saturation", "pm_hue")] +
                [("pm_delta", c_float), ("pm_alpha", c_float), ("pm_sat_alpha", c_float),
                 ("pm_hue_delta", c_int32), ("to_rgb", c_int32), ("mean", c_float * 3),
                 ("std", c_float * 3), ("pad_val", c_float), ("seg_pad_val", c_int32)])


TTA_MAX_VIEWS = 16   # GS_TTA_MAX_VIEWS
FLIP_CODES = {None: 0, "horizontal": 1, "vertical": 2}   # gs_tta_view.flip, gs_slide_desc.flip


class TtaView(Structure):
    """Mirror of ``gs_tta_view``."""
    _fields_ = [("res_h", c_int32), ("res_w", c_int32), ("flip", c_int32), ("reserved", c_int32),
                ("out", c_void_p)]


class TtaDesc(Structure):
    """Mirror of ``gs_tta_desc`` (passed by value)."""
    _fields_ = [("src_h", c_int32), ("src_w", c_int32), ("src_is_rgb", c_int32), ("n_views", c_int32),
                ("to_rgb", c_int32), ("mean", c_float * 3), ("std", c_float * 3), ("reserved", c_int32),
                ("views", TtaView * TTA_MAX_VIEWS)]


SGD_MAX_GROUPS = 16   # GS_SGD_MAX_GROUPS


class SgdGroups(Structure):
    """Mirror of ``GsSgdGroups`` (passed by value)."""
    _fields_ = [("lr_wd", c_float * (2 * SGD_MAX_GROUPS))]


class AdamwGroups(Structure):
    """Mirror of ``GsAdamwGroups`` (passed by value): per-group {lr, wd} in fp64."""
    _fields_ = [("lr_wd", c_double * (2 * SGD_MAX_GROUPS))]


ADAMW_HYPER_DOUBLES = 8 + 2 * SGD_MAX_GROUPS   # GS_ADAMW_HYPER_DOUBLES


class SgdChunk(Structure):
    """Mirror of ``GsSgdChunk``: {begin, length, group, reserved} in units of 4 floats."""
    _fields_ = [(k, c_int32) for k in ("begin", "length", "group", "reserved")]


class BnCalibLayer(Structure):
    """Mirror of ``GsBnCalibLayer``: one BatchNorm's buffers, its active width and its bank offset."""
    _fields_ = [("running_mean", c_void_p), ("running_var", c_void_p), ("channels", c_int32),
                ("offset", c_int32)]


BN_CALIB_SAVE, BN_CALIB_ADD, BN_CALIB_WRITE = 0, 1, 2   # GS_BN_CALIB_*


_P = c_void_p  # device pointers and the stream travel as plain addresses
_i32, _i64, _f32, _f64, _sz = c_int32, c_int64, c_float, c_double, c_size_t
_CD, _CE, _BN, _KD = POINTER(ConvDesc), POINTER(CeDesc), POINTER(BnArgs), POINTER(KdDesc)
_DD, _PW, _CW = POINTER(DistillDesc), POINTER(PairwiseDesc), POINTER(CwdDesc)
_DW = POINTER(DwConvDesc)
_LN = POINTER(LayerNormDesc)
_MS, _MF = POINTER(MscaDesc), POINTER(MscaFilters)
_GG = POINTER(GeluGrnDesc)
_AT = POINTER(AttentionDesc)
_AK = POINTER(AttentionKvDesc)
_FD = POINTER(FcuDownDesc)
_WA, _CL = POINTER(WindowAttentionDesc), POINTER(CellLayerNormDesc)
_OG, _OA = POINTER(OcrGatherDesc), POINTER(OcrAttendDesc)

# name -> (restype, argtypes): one entry per declaration in include/gaiaseg_hip.h
PROTOTYPES = {
    "gs_abi_version": (_i32, []),
    "gs_error_string": (c_char_p, [_i32]),
    "gs_target_arch": (c_char_p, []),
    "gs_conv2d_workspace_bytes": (_sz, [_CD]),
    "gs_conv2d_in_affine_supported": (_i32, [_CD]),
    "gs_conv2d_forward": (_i32, [_CD, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "gs_conv2d_dgrad": (_i32, [_CD, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_conv2d_wgrad": (_i32, [_CD, _P, _P, _P, _P, _sz, _P]),
    "gs_dwconv2d_workspace_bytes": (_sz, [_DW]),
    "gs_dwconv2d_forward": (_i32, [_DW, _P, _P, _P, _P, _P]),
    "gs_dwconv2d_dgrad": (_i32, [_DW, _P, _P, _P, _i32, _P]),
    "gs_dwconv2d_wgrad": (_i32, [_DW, _P, _P, _P, _P, _sz, _P]),
    "gs_msca_saved_bytes": (_sz, [_MS]),
    "gs_msca_workspace_bytes": (_sz, [_MS]),
    "gs_msca_forward": (_i32, [_MS, _P, _MF, _P, _P, _P]),
    "gs_msca_backward": (_i32, [_MS, _P, _P, _MF, _P, _P, _i32, _MF, _P, _sz, _P]),
    "gs_gate_mul_forward": (_i32, [_P, _P, _P, _i64, _i32, _i32, _i32, _i32, _P]),
    "gs_gate_mul_backward": (_i32, [_P, _P, _P, _P, _P, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P]),
    "gs_deconv2x2_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "gs_deconv2x2_forward": (_i32, [_P, _i32, _i32, _i32, _i32, _i32, _P, _i32, _P, _P, _i32, _P, _sz, _P]),
    "gs_layernorm_forward": (_i32, [_LN, _P, _P, _P, _P, _P, _P, _P]),
    "gs_layernorm_workspace_bytes": (_sz, [_LN]),
    "gs_layernorm_backward": (_i32, [_LN, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_gelu_forward": (_i32, [_P, _P, _i64, _i32, _i32, _i32, _P]),
    "gs_gelu_backward": (_i32, [_P, _P, _P, _i64, _i32, _i32, _i32, _i32, _P]),
    "gs_layer_scale_add_forward": (_i32, [_P, _P, _P, _P, _i64, _i32, _i32, _i32, _i32, _P]),
    "gs_layer_scale_workspace_bytes": (_sz, [_i64, _i32]),
    "gs_layer_scale_backward": (_i32, [_P, _P, _P, _P, _P, _i64, _i32, _i32, _i32, _i32, _P, _sz, _P]),
    "gs_gelu_grn_workspace_bytes": (_sz, [_GG]),
    "gs_gelu_grn_forward": (_i32, [_GG, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "gs_gelu_grn_backward": (_i32, [_GG, _P, _P, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "gs_attention_forward": (_i32, [_AT, _P, _P, _P, _P, _P, _P]),
    "gs_attention_relpos_forward": (_i32, [_AT, _P, _P, _P, _P, _i32, _i32, _i32, _P, _P, _P]),
    "gs_attention_workspace_bytes": (_sz, [_AT]),
    "gs_attention_backward": (_i32, [_AT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_attention_forward_f16": (_i32, [_AT, _P, _P, _P, _P, _P, _P]),
    "gs_attention_relpos_forward_f16": (_i32, [_AT, _P, _P, _P, _P, _i32, _i32, _i32, _P, _P, _P]),
    "gs_attention_workspace_bytes_f16": (_sz, [_AT]),
    "gs_attention_backward_f16": (_i32, [_AT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_attention_kv_forward": (_i32, [_AK, _P, _P, _P, _P, _P, _P]),
    "gs_attention_kv_workspace_bytes": (_sz, [_AK]),
    "gs_attention_kv_backward": (_i32, [_AK, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_debug_set_attention_kv_split": (_i32, [_i32]),
    "gs_window_attention_forward": (_i32, [_WA, _P, _P, _P, _P, _P, _P, _P]),
    "gs_window_attention_workspace_bytes": (_sz, [_WA]),
    "gs_window_attention_backward": (_i32, [_WA, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_debug_set_window_attention_split": (_i32, [_i32]),
    "gs_map_pad": (_i32, [_P, _i32, _P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P]),
    "gs_map_crop": (_i32, [_P, _i32, _P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P]),
    "gs_cell_layernorm_forward": (_i32, [_CL, _P, _P, _P, _P, _P, _P, _P]),
    "gs_cell_layernorm_workspace_bytes": (_sz, [_CL]),
    "gs_cell_layernorm_backward": (_i32, [_CL, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_vit_tokens_forward": (_i32, [_P, _i32, _P, _P, _i32, _P, _i32, _i32, _i32, _i32, _P]),
    "gs_vit_tokens_backward": (_i32, [_P, _i32, _P, _i32, _P, _P, _i32, _i32, _i32, _i32, _P]),
    "gs_fcu_down_workspace_bytes": (_sz, [_FD]),
    "gs_fcu_down_forward": (_i32, [_FD, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gs_fcu_down_backward": (_i32, [_FD, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_fcu_up_add_forward": (_i32, [_P, _P, _P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P]),
    "gs_fcu_up_add_backward": (_i32, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P]),
    "gs_fcu_tokens_forward": (_i32, [_P, _i32, _P, _P, _i32, _i32, _i32, _i32, _P]),
    "gs_fcu_tokens_backward": (_i32, [_P, _i32, _P, _i32, _P, _i32, _i32, _i32, _P]),
    "gs_ocr_gather_workspace_bytes": (_sz, [_OG]),
    "gs_ocr_gather_forward": (_i32, [_OG, _P, _P, _P, _P, _P, _sz, _P]),
    "gs_ocr_gather_backward": (_i32, [_OG, _P, _P, _P, _P, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_ocr_attend_forward": (_i32, [_OA, _P, _P, _P, _P, _P, _P]),
    "gs_ocr_attend_workspace_bytes": (_sz, [_OA]),
    "gs_ocr_attend_backward": (_i32, [_OA, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "gs_colsum_workspace_bytes": (_sz, [_i64, _i32]),
    "gs_colsum": (_i32, [_P, _i64, _i32, _i32, _P, _P, _sz, _P]),
    "gs_bn_stats_workspace_bytes": (_sz, [_i64, _i32]),
    "gs_bn_stats": (_i32, [_P, _i64, _i32, _i32, _P, _P, _sz, _P]),
    "gs_bn_finalize": (_i32, [_P, _f64, _i32, _P, _P, _f32, _f32, _P, _P, _P, _P]),
    "gs_bn_sync_local": (_i32, [_P, _f64, _i32, _P, _P]),
    "gs_bn_sync_merge": (_i32, [_P, _i32, _i32, _P, _P]),
    "gs_bn_stats_finalize": (_i32, [_P, _i64, _i32, _i32, _P, _P, _f32, _f32, _P, _P, _P, _P, _sz,
                                    _P]),
    "gs_bn_calib_fold": (_i32, [_P, _i32, _P, _i64, _i32, _f32, _P]),
    "gs_bn_eval_coeffs": (_i32, [_P, _P, _i32, _P, _P, _f32, _P, _P]),
    "gs_bn_apply": (_i32, [_P, _i64, _i32, _i32, _P, _P, _i32, _i32, _P, _i32, _P]),
    "gs_bn_apply_mask": (_i32, [_P, _i64, _i32, _i32, _P, _P, _i32, _P, _i32, _P, _P]),
    "gs_bn_bwd_workspace_bytes": (_sz, [_i64, _i32]),
    "gs_bn_bwd_reduce": (_i32, [_P, _i32, _P, _i32, _P, _i32, _i64, _i32, _P, _i32, _P, _i32, _P,
                                _P, _sz, _P]),
    "gs_bn_bwd_apply": (_i32, [_P, _i32, _P, _i32, _P, _i32, _i64, _i32, _P, _P, _f64, _i32, _i32,
                               _P, _i32, _P, _P, _P]),
    "gs_avgpool_ceil_forward": (_i32, [_P, _i32, _i32, _i32, _i32, _i32, _i32, _P, _i32, _P]),
    "gs_avgpool_ceil_backward": (_i32, [_P, _i32, _i32, _i32, _i32, _i32, _i32, _P, _i32, _i32, _P]),
    "gs_maxpool_forward": (_i32, [_P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                  _P, _i32, _P, _P]),
    "gs_maxpool_backward": (_i32, [_P, _i32, _P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                   _i32, _P, _i32, _i32, _P]),
    "gs_adaptive_avgpool_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, POINTER(_i32), _i32]),
    "gs_adaptive_avgpool_forward": (_i32, [_P, _i32, _i32, _i32, _i32, _i32, POINTER(_i32), _i32,
                                           _P, _P, _sz, _P]),
    "gs_adaptive_avgpool_backward": (_i32, [_P, _i32, _i32, _i32, _i32, POINTER(_i32), _i32, _P,
                                            _i32, _i32, _P]),
    "gs_bilinear_forward": (_i32, [_P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P, _i32,
                                   _i32, _P]),
    "gs_bilinear_backward_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "gs_bilinear_backward": (_i32, [_P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P, _i32,
                                    _i32, _P, _sz, _P]),
    "gs_copy2d": (_i32, [_P, _i32, _P, _i32, _i64, _i32, _f32, _i32, _P]),
    "gs_scale_nc": (_i32, [_P, _i32, _P, _i32, _i64, _i32, _P, _i32, _P]),
    "gs_ce_workspace_bytes": (_sz, [_CE]),
    "gs_ce_forward": (_i32, [_CE, _P, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "gs_ce_forward_scaled": (_i32, [_CE, _P, _P, _P, _P, _P, _f32, _f32, _P, _P, _sz, _P]),
    "gs_ce_backward": (_i32, [_CE, _P, _P, _P, _P, _P, _f32, _P, _i32, _P]),
    "gs_ce_backward_workspace_bytes": (_sz, [_CE, _i32]),
    "gs_ce_backward_ws": (_i32, [_CE, _P, _P, _P, _P, _P, _f32, _P, _i32, _P, _sz, _P]),
    "gs_ce_label_prob": (_i32, [_CE, _P, _P, _P, _P]),
    "gs_resize_argmax": (_i32, [_CE, _P, _P, _P, _P]),
    "gs_kd_workspace_bytes": (_sz, [_KD]),
    "gs_kd_forward": (_i32, [_KD, _P, _P, _P, _P, _f32, _P, _P, _sz, _P]),
    "gs_kd_backward_workspace_bytes": (_sz, [_KD, _i32]),
    "gs_kd_backward": (_i32, [_KD, _P, _P, _P, _P, _f32, _P, _i32, _P, _sz, _P]),
    "gs_distill_workspace_bytes": (_sz, [_DD]),
    "gs_distill_forward": (_i32, [_DD, _P, _P, _P, _P, _f32, _P, _P, _sz, _P]),
    "gs_distill_backward_workspace_bytes": (_sz, [_DD, _i32]),
    "gs_distill_backward": (_i32, [_DD, _P, _P, _P, _P, _f32, _P, _i32, _P, _sz, _P]),
    "gs_pairwise_save_bytes": (_sz, [_PW]),
    "gs_pairwise_forward": (_i32, [_PW, _P, _P, _f32, _P, _P, _sz, _P]),
    "gs_pairwise_backward": (_i32, [_PW, _P, _P, _sz, _f32, _P, _i32, _P]),
    "gs_cwd_workspace_bytes": (_sz, [_CW]),
    "gs_cwd_forward": (_i32, [_CW, _P, _P, _P, _P, _f32, _P, _P, _sz, _P]),
    "gs_cwd_backward": (_i32, [_CW, _P, _P, _P, _P, _f32, _P, _i32, _P]),
    "gs_cwd_debug_partials": (_i32, [_CW]),
    "gs_slide_fuse": (_i32, [POINTER(SlideDesc), POINTER(_i32), POINTER(_i32), _P, _P, _P, _P, _P]),
    "gs_debug_set_slide_strip": (_i32, [_i32]),
    "gs_seg_augment": (_i32, [POINTER(AugmentDesc), _P, _P, _P, _P, _P]),
    "gs_tta_views": (_i32, [TtaDesc, _P, _P]),
    "gs_seg_overlay": (_i32, [_P, _P, _P, _i32, _i32, _i32, _f64, _P, _P]),
    "gs_batch_rescale": (_i32, [_P, _P, _i32, _i32, _i32, _P, _P, _i32, _i32, _P]),
    "gs_ohem_workspace_bytes": (_sz, []),
    "gs_ohem_weights": (_i32, [_P, _i64, _i64, _f32, _i32, _P, _P, _sz, _P]),
    "gs_confusion_matrix": (_i32, [_P, _P, _i64, _i32, _i32, _P, _P]),
    "gs_sgd_step": (_i32, [_P, _P, _P, _i64, _f32, _f32, _f32, _f32, _i32, _P]),
    "gs_sgd_step_hyper": (_i32, [_P, _P, _P, _i64, _P, _i32, _P]),
    "gs_sgd_set_hyper": (_i32, [_P, _f32, _f32, _f32, _f32, _P]),
    "gs_sgd_set_group_hyper": (_i32, [_P, _f32, _f32, _i32, SgdGroups, _P]),
    "gs_sgd_step_groups": (_i32, [_P, _P, _P, _P, _i32, _P, _i32, _P]),
    "gs_adamw_set_group_hyper": (_i32, [_P, _f64, _f64, _f64, _f64, _i32, AdamwGroups, _P]),
    "gs_adamw_step_groups": (_i32, [_P, _P, _P, _P, _P, _i32, _P, _i32, _P, _i32, _P]),
    "gs_grad_accumulate": (_i32, [_P, _P, _i64, _P]),
    "gs_debug_force_plan": (_i32, [_i32, _i32, _i32]),
    "gs_debug_query_plan": (_i32, [_i32, _i32, _i32, _i32, POINTER(_i32), POINTER(_i32), POINTER(_i32),
                                   POINTER(_i32)]),
    "gs_debug_last_conv_launch": (_i32, [POINTER(DebugLaunch)]),
    "gs_debug_conv_launch_counts": (_i32, [POINTER(_i64), _i32]),
    "gs_debug_k3_flops": (_i32, [POINTER(_f64), _i32]),
    "gs_debug_set_x3_fwd": (_i32, [_i32]),
    "gs_debug_set_splitk_inkernel": (_i32, [_i32]),
    "gs_debug_splitk_combined": (_i64, [_i32]),
    "gs_debug_set_col_finalize": (_i32, [_i32]),
    "gs_debug_col_finalized": (_i64, [_i32]),
    "gs_debug_num_cu": (_i32, []),
    "gs_debug_set_stream_mode": (_i32, [_i32]),
    "gs_debug_conv_launch_flops": (_i32, [POINTER(_f64), _i32]),
    "gs_debug_query_conv_launch": (_i32, [_CD, _i32, POINTER(DebugLaunch)]),
    "gs_debug_f16_launches": (_i32, [POINTER(_i64), POINTER(_f64), _i32]),
    "gs_set_forward_precision": (_i32, [_i32]),
    "gs_get_forward_precision": (_i32, []),
    "gs_set_train_precision": (_i32, [_i32]),
    "gs_get_train_precision": (_i32, []),
    "gs_debug_f16_launches_by_op": (_i32, [POINTER(_i64), POINTER(_f64), _i32]),
    "gs_stream_fork": (_i32, [_P, _P]),
    "gs_conv_bn_workspace_bytes": (_sz, [_CD]),
    "gs_conv_bn_forward": (_i32, [_CD, _P, _P, _BN, _P, _i32, _P, _P, _P, _i32, _P, _sz, _P]),
    "gs_conv_bn_backward": (_i32, [_CD, _P, _P, _P, _P, _i32, _P, _BN, _P, _i32, _i32, _i32, _P, _P,
                                   _P, _P, _P, _P, _i32, _P, _sz, _P, _sz, _P, _P, POINTER(BnBwdFuse),
                                   _i32]),
    "gs_k3_timer_enable": (_i32, [_i32]),
    "gs_k3_timer_read": (_i32, [POINTER(_i64), POINTER(_f64), POINTER(_f64)]),
}

_lib = None


def build(verbose=False, jobs=None):
    """Compile every HIP source for gfx950 into ``gaia_seg_amd/lib/libgaiaseg_hip.so``.

    hipcc cross-compiles without a GPU, so this runs in the build container as well.
    """
    jobs = jobs or min(8, os.cpu_count() or 1)
    cmd = ["make", "-C", CSRC_DIR, "-j%d" % jobs]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise HipLibraryError("building libgaiaseg_hip.so failed (exit %d)" % res.returncode)
    global _lib
    _lib = None
    return LIB_PATH


def load():
    """Load the shared object, bind every prototype, check the ABI version. Raises on any gap."""
    global _lib, LIB_PATH
    if _lib is not None:
        return _lib
    if os.environ.get("GS_HIP_LIB"):   # A/B of two builds of the same library (tuning only)
        LIB_PATH = os.environ["GS_HIP_LIB"]
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            "%s not found: the HIP extension is required (no CPU fallback). Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C gaia_seg_amd/csrc`."
            % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime etc.
        raise HipLibraryError("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError("%s does not export %s" % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.gs_abi_version() != ABI_VERSION:
        raise HipLibraryError("ABI mismatch: library %d, binding %d"
                              % (lib.gs_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


CALL_PROFILE = None


def enable_call_profile():
    """Diagnostics (GS_HOST_PROF): time every call into the library on the host.  Returns the dict
    {name: [calls, seconds]} that the wrappers fill; the seconds are host time inside the C-ABI call
    (argument conversion + the HIP launches it makes), not device time."""
    global CALL_PROFILE
    import time
    lib = load()
    if CALL_PROFILE is not None:
        return CALL_PROFILE
    CALL_PROFILE = {}
    for name in PROTOTYPES:
        fn = getattr(lib, name)
        rec = CALL_PROFILE.setdefault(name, [0, 0.0])

        def wrapped(*a, _fn=fn, _rec=rec, _t=time.perf_counter):
            t0 = _t()
            r = _fn(*a)
            _rec[1] += _t() - t0
            _rec[0] += 1
            return r
        setattr(lib, name, wrapped)
    return CALL_PROFILE


def error_string(code):
    return load().gs_error_string(code).decode()


def check(code, what):
    if code != 0:
        raise HipLibraryError("%s failed: %s (code %d)" % (what, error_string(code), code))
