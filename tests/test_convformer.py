"""ElasticConvformer without a GPU: the C-ABI surface of the coupling kernels and their host-side refusals,
the reference constructor's names, the search space, the refusals, the configs of record and their FLOP
count, and the condition on the inputs of tests/test_convformer_gpu.py."""
import copy
import ctypes
import json
import os

import pytest

import util_convformer as U
from util_models import make_batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "ref_convformer_ctors.json")
CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_elastic_convformer_adamw.py")
OK, BADARG, ALIGN, WORKSPACE, NULL = 0, -1, -2, -3, -4
P = 4096    # a non-null, 16-byte aligned address; every call below that gets it is asserted to be refused, and the
            # library refuses before it launches


def build(**kw):
    from gaia_seg_amd.models import build_backbone
    return build_backbone(U.tiny_backbone_cfg(**kw))


# ---- the library -----------------------------------------------------------------------------------------
def test_library_exports_the_fcu_abi(hip_lib):
    from gaia_seg_amd.hip import lib
    for name in ("gs_fcu_down_forward", "gs_fcu_down_backward", "gs_fcu_down_workspace_bytes",
                 "gs_fcu_up_add_forward", "gs_fcu_up_add_backward", "gs_fcu_tokens_forward",
                 "gs_fcu_tokens_backward"):
        assert name in lib.PROTOTYPES and hasattr(hip_lib, name)
    assert lib.ABI_VERSION >= 22 and hip_lib.gs_abi_version() == lib.ABI_VERSION
    assert ctypes.sizeof(lib.FcuDownDesc) == 36
    d = lib.fcu_down_desc(2, 6, 72, ldz=80, ldxt=76)
    assert (d.ldz, d.ldxt, d.ldo, d.lddz, d.lddxt) == (80, 76, 72, 80, 76)


def test_fcu_down_refuses_bad_arguments_before_any_launch(hip_lib):
    from gaia_seg_amd.hip import lib
    L = hip_lib
    d = lib.fcu_down_desc(2, 135, 64, 1e-5)
    db = ctypes.byref(d)
    need = L.gs_fcu_down_workspace_bytes(db)
    assert need == 4 * 2 * 64 * 2          # 270 rows of z: two runs of 256, two planes
    assert L.gs_fcu_down_forward(None, P, P, P, P, P, P, P, None) == NULL
    assert L.gs_fcu_down_forward(db, P, None, P, P, P, P, P, None) == NULL
    assert L.gs_fcu_down_forward(db, P + 4, P, P, P, P, P, P, None) == ALIGN
    assert L.gs_fcu_down_backward(db, P, P, P, P, P, P, P, P, P, P, 0, None, need, None) == NULL
    assert L.gs_fcu_down_backward(db, P, P, P, P, P, P, None, P, P, P, 0, P, need, None) == NULL
    assert L.gs_fcu_down_backward(db, P, P, P, P, P, P, P, P, P, P, 0, P, need - 1, None) == WORKSPACE
    for field, value, code in (("D", 66, ALIGN), ("ldo", 66, ALIGN), ("ldz", 60, BADARG), ("lddxt", 32, BADARG),
                               ("T", 0, BADARG), ("B", 0, BADARG), ("eps", 0.0, BADARG)):
        bad = lib.fcu_down_desc(2, 135, 64, 1e-5)
        setattr(bad, field, value)
        bb = ctypes.byref(bad)
        assert L.gs_fcu_down_workspace_bytes(bb) == 0, field
        assert L.gs_fcu_down_forward(bb, P, P, P, P, P, P, P, None) == code, field
        assert L.gs_fcu_down_backward(bb, P, P, P, P, P, P, P, P, P, P, 0, P, 1 << 20, None) == code, field


def test_fcu_up_add_and_tokens_refuse_bad_arguments_before_any_launch(hip_lib):
    L = hip_lib
    fwd = lambda x=P, r=P, out=P, b=2, h=6, w=10, c=68, s=2, ldx=68, ldr=68, ldo=68: \
        L.gs_fcu_up_add_forward(x, r, out, b, h, w, c, s, ldx, ldr, ldo, None)   # noqa: E731
    bwd = lambda dout=P, dr=P, b=2, h=6, w=10, c=68, s=2, lddo=68, lddr=68: \
        L.gs_fcu_up_add_backward(dout, dr, b, h, w, c, s, lddo, lddr, 0, None)   # noqa: E731
    assert fwd(x=None) == NULL and fwd(r=None) == NULL and fwd(out=None) == NULL
    assert bwd(dout=None) == NULL and bwd(dr=None) == NULL
    assert fwd(c=66) == ALIGN and bwd(c=66) == ALIGN and fwd(ldr=70) == ALIGN and fwd(x=P + 8) == ALIGN
    assert fwd(ldo=64) == BADARG and bwd(lddr=64) == BADARG
    assert fwd(s=4) == BADARG and bwd(s=4) == BADARG          # 4 divides neither 6 nor 10
    assert fwd(s=3) == BADARG and bwd(s=3) == BADARG          # 3 divides 6 but not 10
    assert fwd(s=0) == BADARG and bwd(s=0) == BADARG and fwd(h=0) == BADARG
    assert L.gs_fcu_tokens_forward(None, 72, P, P, 72, 2, 6, 72, None) == NULL
    assert L.gs_fcu_tokens_forward(P, 72, P, P, 72, 2, 6, 70, None) == ALIGN
    assert L.gs_fcu_tokens_forward(P, 64, P, P, 72, 2, 6, 72, None) == BADARG
    assert L.gs_fcu_tokens_backward(P, 72, P, 72, None, 2, 6, 72, None) == NULL
    assert L.gs_fcu_tokens_backward(P, 72, P, 72, P, 2, 0, 72, None) == BADARG


# ---- names -----------------------------------------------------------------------------------------------
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("idx", [0, 1])
def test_backbone_names_equal_the_reference_constructor(idx):
    from gaia_seg_amd.models import build_backbone
    case = _fixture()["backbone"][idx]
    assert case["kwargs"]["patch_size"] == (16, 32)[idx]
    if idx == 0:
        assert case["kwargs"] == dict(U.TINY, drop_path=0.0)
    net = build_backbone(dict(type="ElasticConvformer", **case["kwargs"]))
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == case["state_dict"]
    theirs = dict(map(tuple, case["modules"]))
    for path, m in net.named_modules():
        if path and any(True for _ in m.parameters(recurse=False)):
            assert path in theirs, path
    names = [k for k, _ in got]
    assert names[0] == "cls_token" and names[1] == "conv1.weight" and "bn1.running_var" in names
    for part in ("conv_1", "trans_patch_conv", "trans_1"):
        assert any(k.startswith("conv_trans_1.0.%s." % part) for k in names)
    for part in ("cnn_block", "fusion_block", "squeeze_block", "expand_block", "trans_block"):
        assert any(k.startswith("conv_trans_4.0.%s." % part) for k in names)


# ---- the search space ------------------------------------------------------------------------------------
def _widths(net):
    out = []
    for name in net.layers:
        stage = getattr(net, name)
        per = []
        for blk in stage:
            t = blk.transformer
            convs = [blk.conv_1] if blk.stage else [blk.cnn_block, blk.fusion_block]
            proj = (blk.trans_patch_conv.width_state if blk.stage else
                    (blk.squeeze_block.conv_project.width_state, blk.expand_block.conv_project.width_state))
            per.append(([(c.conv1.width_state, c.conv2.width_state, c.conv3.width_state) for c in convs], proj,
                        t.embed_dim_state, t.attn.num_heads, t.attn.w_qs.width_state, t.mlp.layer1.width_state))
        out.append((stage.depth_state, per))
    return net.conv1.width_state, out


def test_manipulate_arch_sets_the_widths_and_stage_4_follows_stage_3():
    net = build()
    assert net.search_space == {"stem", "body"}
    meta = U.arch_of("sub")
    frozen = copy.deepcopy(meta)
    net.manipulate_arch(meta)
    first = _widths(net)
    net.manipulate_arch(meta)
    assert _widths(net) == first and meta == frozen, "manipulate_arch changed the meta or the subnet"
    a = U.SUBNETS["sub"]
    d = a["embed_dim"]
    assert first[0] == a["stem"]
    for i, (depth, per) in enumerate(first[1]):
        j = min(i, 2)
        assert depth == (a["depths"][i] if i < 3 else 1)
        for convs, proj, dim, heads, wq, hidden in per:      # every block of the stage, skipped ones included
            w = a["widths"][j]
            assert all(c == (w // 4, w // 4, w) for c in convs)
            assert proj in (d, (d, w // 4))
            assert (dim, heads, wq, hidden) == (d, a["heads"][j], 64 * a["heads"][j], int(a["ratios"][j] / 10 * d))
    assert [per[0][5] for _, per in first[1]] == [192, 256, 224, 224]
    # the hidden width follows the embedding width whichever key comes first
    block = meta["body"]["block"]
    net.manipulate_arch(net.full_arch_meta())
    net.manipulate_arch({"body": {"block": {"transblock": block["transblock"], "embed_dim": block["embed_dim"],
                                            "convblock": block["convblock"]},
                                  "depth": meta["body"]["depth"]}, "stem": meta["stem"]})
    assert _widths(net) == first
    net.manipulate_arch(net.full_arch_meta())
    assert net.full_arch_meta() == U.arch_of("max")
    assert _widths(net)[1][3] == (1, [([(32, 32, 128)] * 2, (128, 32), 128, 2, 128, 512)])
    with pytest.raises(KeyError):
        net.manipulate_arch({"encoder": {}})
    with pytest.raises(ValueError, match="width"):
        net.manipulate_arch({"body": dict(meta["body"], block=dict(block, convblock={"width": [24, 32, 64]}))})
    with pytest.raises(ValueError, match="depth"):
        net.manipulate_arch({"body": dict(meta["body"], depth=[3, 2, 1])})


def test_active_modules_leave_out_what_the_subnet_does_not_use():
    net = build()
    net.manipulate_arch(U.arch_of("sub"))
    active = {id(p) for m in net.active_modules() for p in m.parameters()}
    names = {n for n, p in net.named_parameters() if id(p) in active}
    assert {"cls_token", "conv1.weight", "bn1.weight", "conv_trans_1.0.trans_patch_conv.bias"} <= names
    assert not any(n.startswith(("conv_trans_1.1.", "conv_trans_3.1.")) for n in names), "a skipped block is active"
    assert any(n.startswith("conv_trans_2.1.squeeze_block.ln1.") for n in names)
    assert any(n.startswith("conv_trans_4.0.expand_block.bn1.") for n in names)
    assert not any("rel_pos_embed" in n for n in names)
    for n in names:
        assert U.active_slice(n, U.SUBNETS["sub"]) is not None, n
    for n, _ in net.named_parameters():
        assert (n in names) == (U.active_slice(n, U.SUBNETS["sub"]) is not None), n
    late = {id(p) for p in net.late_gradient_parameters()}
    late_names = {n for n, p in net.named_parameters() if id(p) in late}
    assert late <= active and "cls_token" in late_names and "conv_trans_1.0.trans_1.attn.proj.weight" in late_names
    assert not any(n.startswith("conv_trans_2") for n in late_names)


def test_train_freezes_the_stem_and_norm_eval_is_a_keyword():
    from torch.nn.modules.batchnorm import _BatchNorm
    net = build().train()
    assert net.norm_eval is True
    assert not net.conv1.weight.requires_grad and not net.bn1.weight.requires_grad and not net.bn1.training
    assert all(not m.training for m in net.modules() if isinstance(m, _BatchNorm))
    assert net.conv_trans_1[0].conv_1.conv1.weight.requires_grad
    net = build(norm_eval=False).train()
    assert not net.bn1.training and not net.bn1.bias.requires_grad
    assert all(m.training for n, m in net.named_modules() if isinstance(m, _BatchNorm) and n != "bn1")
    # mlp_ratio is a multiplier, the sampled ratio is tenths of the embedding width
    assert build(mlp_ratio=[2, 3, 4]).conv_trans_2[0].trans_block.mlp.layer1.out_channels == 3 * 128


# ---- refusals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,kw,exc", [
    ("drop_path", dict(drop_path=0.1), NotImplementedError),
    ("attn_drop", dict(attn_drop=0.1), NotImplementedError),
    ("proj_drop", dict(proj_drop=0.2), NotImplementedError),
    ("relative_position", dict(relative_position=True), NotImplementedError),
    ("patch_size", dict(patch_size=8), NotImplementedError),
    ("patch_size", dict(patch_size=24), NotImplementedError),
    ("depth", dict(depth=10), ValueError),
    ("depth", dict(depth=6), ValueError),                       # 6 <= 2 + 2 + 2
    ("width", dict(body_width=[32, 72, 128]), ValueError),      # 72 / 4 = 18
])
def test_refusals_name_the_key(key, kw, exc):
    with pytest.raises(exc, match=key):
        build(**kw)


def test_the_default_drop_path_is_refused():
    from gaia_seg_amd.models import build_backbone
    cfg = U.tiny_backbone_cfg()
    del cfg["drop_path"]   # the reference's default is 0.1
    with pytest.raises(NotImplementedError, match="drop_path"):
        build_backbone(cfg)


def test_wrap_fp16_model_finds_the_backbone():
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    from gaia_seg_amd.models.backbones.elastic_transformer import ElasticMHA
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(U.tiny_model_cfg())
    net = model.backbone
    assert net.fp16_attention is False
    wrap_fp16_model(model, attention=True)
    mhas = [m for m in net.modules() if isinstance(m, ElasticMHA)]
    assert net.fp16_attention is True and len(mhas) == 7 and all(m.fp16_attention for m in mhas)
    net.fp16_attention = False
    assert not any(m.fp16_attention for m in mhas)


# ---- configs and FLOPs -----------------------------------------------------------------------------------
def _brute_force(stem, widths, d, heads, depths, ratios, h=512, w=1024, patch=16):
    """backbone FLOPs per image, module by module, from the architecture's numbers alone"""
    def conv(ho, wo, cin, cout, k=1):
        return 2.0 * ho * wo * cin * cout * k * k

    def bottleneck(hh, ww, cin, width, stride=1, res_conv=False):
        med, ho, wo = width // 4, hh // stride, ww // stride
        f = conv(hh, ww, cin, med) + conv(ho, wo, med, med, 3) + conv(ho, wo, med, width)
        return f + (conv(ho, wo, cin, width) if res_conv else 0.0)

    def transformer(n, nh, ratio):
        hidden = int(ratio / 10 * d)
        return 3 * 2.0 * n * d * 64 * nh + 4.0 * n * n * 64 * nh + 2.0 * n * 64 * nh * d + 2 * 2.0 * n * d * hidden

    total = conv(h // 2, w // 2, 3, stem, 7)
    h, w, c = h // 4, w // 4, stem
    n = (h * 4 // patch) * (w * 4 // patch) + 1
    strides = [patch // 4, patch // 8, patch // 16, patch // 16]
    for i in range(4):
        j = min(i, 2)
        for k in range(depths[i] if i < 3 else 1):
            if i == 0 and k == 0:
                s = strides[0]
                total += conv(h // s, w // s, c, d, s) + transformer(n, heads[0], ratios[0])
                total += bottleneck(h, w, c, widths[0], res_conv=True)
                c = widths[0]
                continue
            stride = 2 if (i in (1, 2) and k == 0) else 1
            total += bottleneck(h, w, c, widths[j], stride, res_conv=k == 0 and i != 3)
            h, w, c, s = h // stride, w // stride, widths[j], strides[i]
            total += conv(h // s, w // s, c // 4, d)               # the projection, on the pooled map
            total += transformer(n, heads[j], ratios[j])
            total += conv(h // s, w // s, d, c // 4)
            fs = 2 if i == 3 else 1
            total += bottleneck(h, w, c, c, fs, res_conv=i == 3)
            h, w = h // fs, w // fs
    return total


def test_configs_build_and_count_the_brute_force_flops():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.flops import backbone_flops, convformer_backbone_flops, model_flops
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import full_arch_meta
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    assert type(model.backbone).__name__ == "ElasticConvformer" and getattr(model, "neck", None) is None
    assert cfg.optimizer["type"] == "AdamW" and cfg.model["backbone"]["drop_path"] == 0.0
    assert cfg.optimizer["paramwise_cfg"]["custom_keys"]["cls_token"]["decay_mult"] == 0.
    assert cfg.optimizer["paramwise_cfg"]["norm_decay_mult"] == 0.
    assert type(model.auxiliary_head).__name__ == "DynamicFCNHead" and model.auxiliary_head.in_index == 2
    anchors = {m["name"]: m for m in build_model_sampler(cfg.val_sampler).traverse()}
    assert fold_dict(anchors["MAX"])["arch"] == full_arch_meta(model)
    first = build_model_sampler(cfg.train_sampler).candidates()[0]
    assert fold_dict(first)["arch"] == full_arch_meta(model)
    specs = {"MIN": (64, [256, 512, 1024], 384, [6] * 3, [2, 2, 2], [30] * 3),
             "MAX": (64, [384, 768, 1536], 576, [9] * 3, [3, 4, 4], [40] * 3)}
    for name, spec in specs.items():
        model.manipulate_arch(fold_dict(anchors[name])["arch"])
        f = model_flops(model, 512, 1024)
        assert f["backbone"] == _brute_force(*spec), name
        assert backbone_flops(model.backbone, 512, 1024) == convformer_backbone_flops(model.backbone, 512, 1024)
        assert f["total"] == f["backbone"] + f["decode"] + f["aux"] and "neck" not in f
        assert f["decode"] > 0 and f["aux"] > 0 and 0 < f["backbone_3x3"] < f["backbone"]
        feats = backbone_flops(model.backbone, 512, 1024)[3]
        assert feats == [(spec[1][0], 128, 256), (spec[1][1], 64, 128), (spec[1][2], 32, 64), (spec[1][2], 16, 32)]
    assert sorted(anchors) == ["MAX", "MID", "MIN"]
    model.manipulate_arch(fold_dict(anchors["MID"])["arch"])
    assert _brute_force(*specs["MIN"]) < model_flops(model, 512, 1024)["backbone"] < _brute_force(*specs["MAX"])
    sampler = build_model_sampler(cfg.train_sampler)
    for _ in range(20):   # a sampled subnet has widths the kernels can run
        model.manipulate_arch(fold_dict(sampler.sample())["arch"])


# ---- the inputs of the gradient-parity test ------------------------------------------------------------------
@pytest.mark.parametrize("norm_eval", [True, False], ids=["norm_eval", "batch_stats"])
@pytest.mark.parametrize("name", ["max", "sub"])
def test_no_relu_input_of_the_float64_model_lies_near_zero(name, norm_eval):
    """The condition tests/test_convformer_gpu.py asserts on its own float64 pass, here without a GPU: for
    the parameters and the image of record every ReLU input is at least 1e-4 rms away from zero
    (tests/golden/make_convformer_relu_margin.py says how the parameters were made to satisfy it)."""
    net = build()
    U.randomize_convformer(net)
    sd = {k: v.detach().clone().double() for k, v in net.state_dict().items()}
    pre = []
    outs = U.convformer_ref(sd, make_batch(2, U.H, U.W, seed=U.IMG_SEED)[0].double(), U.SUBNETS[name], norm_eval,
                            relu_inputs=pre)
    a = U.SUBNETS[name]
    assert [tuple(o.shape) for o in outs] == [(2, a["widths"][0], 16, 24), (2, a["widths"][1], 8, 12),
                                              (2, a["widths"][2], 4, 6), (2, a["widths"][2], 2, 3)]
    U.assert_relu_margin(pre)
    masked = sum(int((v < 0).sum()) for _, v in pre) / sum(v.numel() for _, v in pre)
    assert 0.01 < masked < 0.5, "the ReLUs must mask a real share of their inputs, got %.3f" % masked
