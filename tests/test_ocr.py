"""OCRNet without a GPU: registry names, DynamicOCRHead's constructor, state-dict keys and refusals, the
cascade segmentor's wiring, the new config, the FLOP count against the CPU restatement (tests/util_ocr.py),
the host-side argument checks of gs_ocr_gather_* / gs_ocr_attend_*, and the refusals of in-place
distillation and of a fixed teacher with a cascade model."""
import copy
import ctypes

import pytest
import torch

from gaia_seg_amd.hip import lib
import util_ocr as U
from util_models import arch_meta

GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
P = 0x10000          # a 16-byte aligned, non-null address.  It is never dereferenced because every call that gets it is
                     # asserted to return a refusal code, and the library refuses before it launches
CONFIG = lib.REPO_ROOT + "/configs/supernet/ocrnet_ar50to101_v1c_os8.py"

OCR_HEAD_KEYS = [
    "conv_seg.weight", "conv_seg.bias",
    "object_context_block.query_project.0.conv.weight", "object_context_block.query_project.0.bn.weight",
    "object_context_block.query_project.0.bn.bias", "object_context_block.query_project.0.bn.running_mean",
    "object_context_block.query_project.0.bn.running_var",
    "object_context_block.query_project.0.bn.num_batches_tracked",
    "object_context_block.query_project.1.conv.weight", "object_context_block.query_project.1.bn.weight",
    "object_context_block.query_project.1.bn.bias", "object_context_block.query_project.1.bn.running_mean",
    "object_context_block.query_project.1.bn.running_var",
    "object_context_block.query_project.1.bn.num_batches_tracked",
    "object_context_block.key_project.0.conv.weight", "object_context_block.key_project.0.bn.weight",
    "object_context_block.key_project.0.bn.bias", "object_context_block.key_project.0.bn.running_mean",
    "object_context_block.key_project.0.bn.running_var",
    "object_context_block.key_project.0.bn.num_batches_tracked",
    "object_context_block.key_project.1.conv.weight", "object_context_block.key_project.1.bn.weight",
    "object_context_block.key_project.1.bn.bias", "object_context_block.key_project.1.bn.running_mean",
    "object_context_block.key_project.1.bn.running_var",
    "object_context_block.key_project.1.bn.num_batches_tracked",
    "object_context_block.value_project.conv.weight", "object_context_block.value_project.bn.weight",
    "object_context_block.value_project.bn.bias", "object_context_block.value_project.bn.running_mean",
    "object_context_block.value_project.bn.running_var",
    "object_context_block.value_project.bn.num_batches_tracked",
    "object_context_block.out_project.conv.weight", "object_context_block.out_project.bn.weight",
    "object_context_block.out_project.bn.bias", "object_context_block.out_project.bn.running_mean",
    "object_context_block.out_project.bn.running_var",
    "object_context_block.out_project.bn.num_batches_tracked",
    "object_context_block.bottleneck.conv.weight", "object_context_block.bottleneck.bn.weight",
    "object_context_block.bottleneck.bn.bias", "object_context_block.bottleneck.bn.running_mean",
    "object_context_block.bottleneck.bn.running_var",
    "object_context_block.bottleneck.bn.num_batches_tracked",
    "bottleneck.conv.weight", "bottleneck.bn.weight", "bottleneck.bn.bias", "bottleneck.bn.running_mean",
    "bottleneck.bn.running_var", "bottleneck.bn.num_batches_tracked",
]


def tiny_model():
    from gaia_seg_amd.models import build_segmentor
    return build_segmentor(copy.deepcopy(U.cascade_cfg()))


# ---- the head and the segmentor ----------------------------------------------------------------------
def test_registry_names():
    from gaia_seg_amd.models.builder import HEADS, SEGMENTORS
    assert HEADS.get("DynamicOCRHead") is not None
    assert SEGMENTORS.get("DynamicCascadeEncoderDecoder") is not None
    assert SEGMENTORS.get("CascadeEncoderDecoder") is not None
    from gaia_seg_amd.hip import ops
    assert callable(ops.ocr_gather) and callable(ops.ocr_attend)


def test_constructor_and_state_dict_keys():
    from gaia_seg_amd.core.bricks import DynamicConvModule
    from gaia_seg_amd.models import build_head
    head = build_head(U.ocr_cfg())
    assert (head.in_channels, head.channels, head.ocr_channels, head.scale) == (512, 16, 8, 1)
    assert sorted(head.state_dict().keys()) == sorted(OCR_HEAD_KEYS)
    ocb = head.object_context_block
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items() if k.endswith("conv.weight")}
    assert shapes == {
        "bottleneck.conv.weight": (16, 512, 3, 3),
        "object_context_block.query_project.0.conv.weight": (8, 16, 1, 1),
        "object_context_block.query_project.1.conv.weight": (8, 8, 1, 1),
        "object_context_block.key_project.0.conv.weight": (8, 16, 1, 1),
        "object_context_block.key_project.1.conv.weight": (8, 8, 1, 1),
        "object_context_block.value_project.conv.weight": (8, 16, 1, 1),
        "object_context_block.out_project.conv.weight": (16, 8, 1, 1),
        "object_context_block.bottleneck.conv.weight": (16, 32, 1, 1)}
    for m in (head.bottleneck, ocb.value_project, ocb.out_project, ocb.bottleneck, *ocb.query_project,
              *ocb.key_project):
        assert isinstance(m, DynamicConvModule)
    # the CPU restatement takes the same state
    U.load_into_ref(U.RefOCRHead(**U.TINY_OCR), head)


def test_refusals():
    from gaia_seg_amd.models import build_head
    with pytest.raises(NotImplementedError, match="scale=1 only"):
        build_head(U.ocr_cfg(scale=2))
    with pytest.raises(NotImplementedError, match="input_transform=None"):
        build_head(U.ocr_cfg(in_channels=[512], in_index=[3], input_transform="multiple_select"))
    head = build_head(U.ocr_cfg())
    feats = [torch.zeros(2, 8, 4, 6)] * 3 + [torch.zeros(2, 384, 4, 6)]
    with pytest.raises(NotImplementedError, match="has no in-place distillation branch"):
        head.forward_train(feats, torch.zeros(2, 19, 4, 6), None, None, None, teacher_logits=torch.zeros(1))
    with pytest.raises(ValueError, match="must read stages of one stride"):
        head.forward(feats, torch.zeros(2, 19, 8, 12))
    with pytest.raises(ValueError, match="must read stages of one stride"):
        head.forward_test(feats, torch.zeros(2, 19, 4, 5), None, None)


def test_cascade_segmentor_structure():
    from torch import nn
    from gaia_seg_amd.models import build_segmentor
    m = tiny_model()
    assert isinstance(m.decode_head, nn.ModuleList) and len(m.decode_head) == m.num_stages == 2
    assert [type(h).__name__ for h in m.decode_head] == ["DynamicFCNHead", "DynamicOCRHead"]
    keys = list(m.state_dict().keys())
    assert "decode_head.0.convs.0.conv.weight" in keys and "decode_head.0.conv_seg.bias" in keys
    assert "decode_head.1.object_context_block.out_project.bn.running_var" in keys
    assert not m.with_auxiliary_head
    assert m.num_classes == 19 and m.align_corners is False
    m.manipulate_arch(arch_meta("sub"))
    active = {id(p) for p in m.active_parameters()}
    for p in m.decode_head.parameters():
        assert id(p) in active
    assert len(active) < sum(1 for _ in m.parameters())          # the depth state skips backbone blocks
    cfg = U.cascade_cfg()
    with pytest.raises(ValueError, match="list of num_stages=2 head configs"):
        build_segmentor(dict(cfg, decode_head=cfg["decode_head"][0]))
    fixed = build_segmentor(dict(copy.deepcopy(cfg), type="CascadeEncoderDecoder"))
    assert sorted(fixed.state_dict().keys()) == sorted(keys)


def test_cascade_loss_dict_and_the_logits_handed_on():
    """the wiring of _decode_head_forward_train / _decode_head_forward_test with the heads' kernels stubbed
    out: stage 1 receives the very tensor stage 0 returned (its gradient path), each stage runs once"""
    m = tiny_model()
    calls = []
    logits0, logits1 = torch.zeros(1, requires_grad=True) + 1, torch.zeros(1) + 2

    def fwd0(x):
        calls.append(("fcn", None))
        return logits0

    def fwd1(x, prev):
        calls.append(("ocr", prev))
        return logits1
    for head, fwd in zip(m.decode_head, (fwd0, fwd1)):
        head.__dict__["forward"] = fwd
        head.__dict__["losses"] = lambda logit, gt, _h=head: dict(loss_seg=logit.sum(), acc_seg=logit.sum())
    losses = m._decode_head_forward_train([None], None, None)
    assert sorted(losses) == ["decode_0.acc_seg", "decode_0.loss_seg", "decode_1.acc_seg", "decode_1.loss_seg"]
    assert [c[0] for c in calls] == ["fcn", "ocr"] and calls[1][1] is logits0 and logits0.requires_grad
    assert float(losses["decode_0.loss_seg"]) == 1 and float(losses["decode_1.loss_seg"]) == 2
    del calls[:]
    assert m._decode_head_forward_test([None], None) is logits1
    assert [c[0] for c in calls] == ["fcn", "ocr"] and calls[1][1] is logits0
    with pytest.raises(NotImplementedError, match="cascade of decode heads"):
        m._decode_head_forward_train([None], None, None, teacher_logits=logits1)


def test_sandwich_and_distiller_refuse_a_cascade_model():
    from gaia_seg_amd.core.runner import check_sandwich_model
    from gaia_seg_amd.models import build_segmentor
    with pytest.raises(ValueError, match="cascade of decode heads"):
        check_sandwich_model(tiny_model())
    cfg = dict(copy.deepcopy(U.cascade_cfg()), type="DynamicDistiller", has_distill_loss=False,
               has_pairwise_loss=False)
    cfg.pop("num_stages")
    with pytest.raises(ValueError, match="cascade of decode heads"):
        build_segmentor(cfg)


def test_config_builds_with_the_restatement_parameter_counts():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    heads = cfg.model["decode_head"]
    assert [h["type"] for h in heads] == ["DynamicFCNHead", "DynamicOCRHead"]
    assert all(h["dropout_ratio"] == 0.1 and h["num_classes"] == 19 for h in heads)
    assert [h["loss_decode"]["loss_weight"] for h in heads] == [0.4, 1.0]
    assert "auxiliary_head" not in cfg.model
    model = build_segmentor(cfg.model)
    assert type(model).__name__ == "DynamicCascadeEncoderDecoder"
    ref = U.RefCascade([U.RefFCNHead(1280, 256, 19, num_convs=1, in_index=2),
                        U.RefOCRHead(2560, 512, 256, 19, in_index=3)])
    for got, want in zip(model.decode_head, ref.decode_head):
        assert sum(p.numel() for p in got.parameters()) == sum(p.numel() for p in want.parameters())
    assert {k for k, _ in model.decode_head.named_parameters()} == {k for k, _ in ref.decode_head.named_parameters()}


def test_model_flops_equals_a_count_on_the_restatement():
    from gaia_seg_amd.core.flops import backbone_flops, model_flops, ocr_head_flops
    m = tiny_model()
    m.manipulate_arch(arch_meta("sub"))
    flops = model_flops(m, 32, 48)
    feats = backbone_flops(m.backbone, 32, 48)[3]
    assert feats[2][1:] == feats[3][1:] == (4, 6)
    inputs = [torch.randn(1, c, h, w).double() for c, h, w in feats]
    ref = U.ref_cascade().double()
    assert flops["decode"] == flops["decode_0"] + flops["decode_1"] == 2.0 * U.count_ocr_macs(ref, inputs)
    assert flops["decode_1"] == ocr_head_flops(m.decode_head[1], feats)
    assert flops["total"] == flops["backbone"] + flops["decode"]
    # the two region products: 2 K P C + 4 K P ch FLOPs
    k, p, c, ch = 19, 24, 16, 8
    convs_only = 2.0 * U.count_macs(ref, inputs)
    assert flops["decode"] - convs_only == 2.0 * k * p * c + 4.0 * k * p * ch


# ---- host-side checks of the C-ABI -------------------------------------------------------------------
def test_binding_and_header(hip_lib):
    assert lib.ABI_VERSION >= 23 and hip_lib.gs_abi_version() == lib.ABI_VERSION
    assert ctypes.sizeof(lib.OcrGatherDesc) == 11 * 4 and ctypes.sizeof(lib.OcrAttendDesc) == 12 * 4
    header = open(lib.REPO_ROOT + "/include/gaiaseg_hip.h").read()
    for name in ("gs_ocr_gather_workspace_bytes", "gs_ocr_gather_forward", "gs_ocr_gather_backward",
                 "gs_ocr_attend_workspace_bytes", "gs_ocr_attend_forward", "gs_ocr_attend_backward"):
        assert name in lib.PROTOTYPES and name + "(" in header
    assert "#define GS_OCR_MAX_CLASSES %d" % lib.OCR_MAX_CLASSES in header
    assert "#define GS_OCR_GATHER_MAX_CHANNELS %d" % lib.OCR_GATHER_MAX_CHANNELS in header
    assert "#define GS_OCR_ATTEND_MAX_CHANNELS %d" % lib.OCR_ATTEND_MAX_CHANNELS in header


def gather_calls(L, d, ws_bytes=1 << 30, ptr=P):
    r = ctypes.byref(d)
    return (L.gs_ocr_gather_forward(r, ptr, ptr, ptr, ptr, ptr, ws_bytes, None),
            L.gs_ocr_gather_backward(r, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 0, ptr, ws_bytes, None))


def attend_calls(L, d, ws_bytes=1 << 30, ptr=P):
    r = ctypes.byref(d)
    return (L.gs_ocr_attend_forward(r, ptr, ptr, ptr, ptr, ptr, None),
            L.gs_ocr_attend_backward(r, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ws_bytes, None))


@pytest.mark.parametrize("change,code", [
    (dict(K=0), GS_E_BADARG), (dict(K=257), GS_E_BADARG), (dict(B=0), GS_E_BADARG), (dict(P=0), GS_E_BADARG),
    (dict(C=6), GS_E_ALIGN), (dict(C=2052, ldf=2052, ldc=2052, lddf=2052, lddc=2052), GS_E_BADARG),
    (dict(ldl=16), GS_E_BADARG), (dict(ldl=22), GS_E_ALIGN), (dict(ldf=4), GS_E_BADARG), (dict(lddc=10), GS_E_ALIGN),
    (dict(scale=float("nan")), GS_E_BADARG), (dict(scale=float("inf")), GS_E_BADARG),
])
def test_gather_bad_descriptors_are_refused_before_any_launch(hip_lib, change, code):
    d = lib.ocr_gather_desc(2, 221, 19, 8)
    for k, v in change.items():
        setattr(d, k, v)
    assert gather_calls(hip_lib, d) == (code, code)
    assert hip_lib.gs_ocr_gather_workspace_bytes(ctypes.byref(d)) == 0


@pytest.mark.parametrize("change,code", [
    (dict(K=0), GS_E_BADARG), (dict(K=257), GS_E_BADARG), (dict(B=0), GS_E_BADARG), (dict(P=0), GS_E_BADARG),
    (dict(ch=6), GS_E_ALIGN), (dict(ch=516, ldq=516), GS_E_BADARG), (dict(ldq=4), GS_E_BADARG),
    (dict(lddv=10), GS_E_ALIGN),
])
def test_attend_bad_descriptors_are_refused_before_any_launch(hip_lib, change, code):
    d = lib.ocr_attend_desc(2, 221, 19, 8)
    for k, v in change.items():
        setattr(d, k, v)
    assert attend_calls(hip_lib, d) == (code, code)
    assert hip_lib.gs_ocr_attend_workspace_bytes(ctypes.byref(d)) == 0


def test_null_pointers_alignment_and_short_workspaces(hip_lib):
    L = hip_lib
    g, a = lib.ocr_gather_desc(2, 221, 19, 8), lib.ocr_attend_desc(2, 221, 19, 8)
    assert gather_calls(L, g, ptr=None) == (GS_E_NULL, GS_E_NULL)
    assert attend_calls(L, a, ptr=None) == (GS_E_NULL, GS_E_NULL)
    assert L.gs_ocr_gather_forward(None, P, P, P, P, P, 1 << 30, None) == GS_E_NULL
    assert L.gs_ocr_attend_forward(None, P, P, P, P, P, None) == GS_E_NULL
    assert L.gs_ocr_gather_workspace_bytes(None) == 0 and L.gs_ocr_attend_workspace_bytes(None) == 0
    assert gather_calls(L, g, ptr=P + 4) == (GS_E_ALIGN, GS_E_ALIGN)
    assert attend_calls(L, a, ptr=P + 4) == (GS_E_ALIGN, GS_E_ALIGN)
    # 221 pixels: four runs of 64 rows for the statistics, two of 128 for the product
    need_g = L.gs_ocr_gather_workspace_bytes(ctypes.byref(g))
    assert need_g == 4 * (2 * 4 * 19 * 2 + 40 + 40 + 2 * 2 * 19 * 8)
    assert gather_calls(L, g, ws_bytes=need_g - 1) == (GS_E_WORKSPACE, GS_E_WORKSPACE)
    need_a = L.gs_ocr_attend_workspace_bytes(ctypes.byref(a))
    assert need_a == 4 * (2 * 2 * 221 * 20 + 2 * 2 * 19 * 8)
    # (the backward alone: the forward takes no workspace and, with nothing wrong, would launch on P)
    assert L.gs_ocr_attend_backward(ctypes.byref(a), P, P, P, P, P, P, P, P, P, P, need_a - 1, None) == GS_E_WORKSPACE
    # the queries need no device and grow with the pixels
    big = lib.ocr_gather_desc(2, 64 * 128, 19, 512)
    assert L.gs_ocr_gather_workspace_bytes(ctypes.byref(big)) > need_g
