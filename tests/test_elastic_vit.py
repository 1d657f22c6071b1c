"""ElasticTransformer + DynamicMultiLevelNeck without a GPU: the C-ABI surface of the attention operator,
the reference constructor's names, the search space, the refusals, the config of record and its FLOP
count, and the conditioning of the operator tests' inputs."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import rel_err
import util_vit as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "ref_vit_ctors.json")
CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_elastic_vit.py")


def build(**kw):
    from gaia_seg_amd.models import build_backbone
    return build_backbone(U.tiny_backbone_cfg(**kw))


def test_library_exports_attention_abi(hip_lib):
    from gaia_seg_amd.hip import lib
    for name in ("gs_attention_forward", "gs_attention_workspace_bytes", "gs_attention_backward",
                 "gs_vit_tokens_forward", "gs_vit_tokens_backward"):
        assert name in lib.PROTOTYPES and hasattr(hip_lib, name)
    assert lib.ABI_VERSION >= 19 and hip_lib.gs_abi_version() == lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "gaiaseg_hip.h")) as f:
        body = re.search(r"typedef struct gs_attention_desc \{(.*?)\} gs_attention_desc;", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [n for n, _ in fields] == [n for n, _ in lib.AttentionDesc._fields_]
    assert all(t in ("int32_t", "float") for _, t in fields)
    assert ctypes.sizeof(lib.AttentionDesc) == 4 * len(fields) == 48
    d = lib.attention_desc(2, 7, 3, ldq=576, ldo=200)
    assert (d.ldq, d.ldk, d.lddq, d.lddk, d.ldo, d.lddo) == (576, 192, 576, 192, 200, 200)
    assert abs(d.scale - 0.125) < 1e-9
    # the host-side checks need no device
    assert hip_lib.gs_attention_workspace_bytes(ctypes.byref(d)) == 4 * 2 * 3 * 7 + 8
    d.ldk = 100
    assert hip_lib.gs_attention_workspace_bytes(ctypes.byref(d)) == 0
    assert hip_lib.gs_attention_forward(ctypes.byref(d), None, None, None, None, None, None) == -1
    assert hip_lib.gs_attention_forward(None, None, None, None, None, None, None) == -4


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("idx", [0, 1])
def test_backbone_names_equal_the_reference_constructor(idx):
    from gaia_seg_amd.models import build_backbone
    case = _fixture()["backbone"][idx]
    net = build_backbone(dict(type="ElasticTransformer", **case["kwargs"]))
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == case["state_dict"]
    theirs = dict(map(tuple, case["modules"]))
    for path, m in net.named_modules():
        if path and any(True for _ in m.parameters(recurse=False)):
            assert path in theirs, path
    if idx == 0:
        assert got == [[k, list(s)] for k, s in U.vit_param_names(128, 2, 512, [1, 2, 1], 7)]


@pytest.mark.parametrize("idx", [0, 1])
def test_neck_names_equal_the_reference_constructor(idx):
    from gaia_seg_amd.models import build_neck
    case = _fixture()["neck"][idx]
    neck = build_neck(dict(type="DynamicMultiLevelNeck", **case["kwargs"]))
    assert [[k, list(v.shape)] for k, v in neck.state_dict().items()] == case["state_dict"]
    if idx == 1:
        assert neck.scales == [0.5, 1, 2, 4]
    w = neck.convs[0].conv.weight
    bound = (6.0 / (w.shape[1] * 9 + w.shape[0] * 9)) ** 0.5   # xavier uniform
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.8 * bound
    assert not bool(neck.convs[0].conv.bias.any())


def _widths(net):
    out = []
    for name in net.layers:
        enc = getattr(net, name)
        out.append((enc.num_layers_state, [(l.attn.w_qs.width_state, l.attn.w_ks.width_state,
                                            l.attn.w_vs.width_state, l.attn.num_heads, l.mlp.layer1.width_state)
                                           for l in enc]))
    return net.elastic_patch_embed.projection.width_state, out


def test_manipulate_arch_is_idempotent_and_sets_the_widths():
    import copy
    net = build()
    assert net.search_space == {"embedding", "encoder"}
    meta = U.arch_of("sub")
    frozen = copy.deepcopy(meta)
    net.manipulate_arch(meta)
    first = _widths(net)
    net.manipulate_arch(meta)
    assert _widths(net) == first and meta == frozen, "manipulate_arch changed the meta or the subnet"
    a = U.SUBNETS["sub"]
    d = a["embed_dim"]
    assert first[0] == d
    for i, (layers, per_layer) in enumerate(first[1]):
        assert layers == a["layers"][i]
        for wq, wk, wv, heads, hidden in per_layer:   # every layer of the group, skipped ones included
            assert wq == wk == wv == 64 * a["heads"][i] and heads == a["heads"][i]
            assert hidden == int(a["ratios"][i] / 10 * d)
    assert [per[0][4] for _, per in first[1]] == [192, 256, 224]
    # the hidden width follows the embedding width whichever key comes first
    net.manipulate_arch({"encoder": meta["encoder"], "embedding": meta["embedding"]})
    assert _widths(net) == first
    net.manipulate_arch(net.full_arch_meta())
    assert _widths(net)[1][1][1][0] == (128, 128, 128, 2, 512)
    assert net.full_arch_meta() == U.arch_of("max")
    with pytest.raises(KeyError):
        net.manipulate_arch({"body": {}})
    with pytest.raises(ValueError, match="feedforward_channels"):
        net.manipulate_arch({"encoder": dict(meta["encoder"], feedforward_channels=U.nest(
            "feedforward_channels", [33, 40, 35]))})   # int(3.3 * 128) = 422


def test_active_modules_leave_out_what_the_subnet_does_not_use():
    net = build()
    net.manipulate_arch(U.arch_of("sub"))
    active = {id(p) for m in net.active_modules() for p in m.parameters()}
    names = {n for n, p in net.named_parameters() if id(p) in active}
    assert "cls_token" in names and "pos_embed" in names
    assert "elastic_patch_embed.projection.weight" in names
    assert {n for n in names if n.startswith("elastic_encoder2.0.")} == {
        "elastic_encoder2.0." + s + e for s in ("ln1", "ln2", "attn.w_qs", "attn.w_ks", "attn.w_vs", "attn.proj",
                                                "mlp.layer1", "mlp.layer2") for e in (".weight", ".bias")}
    assert not any(n.startswith("elastic_encoder2.1.") for n in names), "a skipped layer is active"
    assert not any("rel_pos_embed" in n for n in names) and "ln1.weight" not in names
    late = {id(p) for p in net.late_gradient_parameters()}
    late_names = {n for n, p in net.named_parameters() if id(p) in late}
    assert late <= active and "cls_token" in late_names and "elastic_encoder1.0.attn.proj.weight" in late_names
    assert not any(n.startswith("elastic_encoder2") for n in late_names)


@pytest.mark.parametrize("key,kw", [("drop_path", dict(drop_path=0.1)), ("attn_drop", dict(attn_drop=0.1)),
                                    ("proj_drop", dict(proj_drop=0.2)), ("drop_rate", dict(drop_rate=0.1))])
def test_refusals_name_the_key(key, kw):
    with pytest.raises(NotImplementedError, match=key):
        build(**kw)


def test_relative_position_and_default_drop_path_are_refused():
    from gaia_seg_amd.models.backbones.elastic_transformer import ElasticMHA
    with pytest.raises(NotImplementedError, match="relative_position"):
        ElasticMHA(128, 2, drop_path=0.0, relative_position=True)
    cfg = U.tiny_backbone_cfg()
    del cfg["drop_path"]   # the reference's default is 0.1
    from gaia_seg_amd.models import build_backbone
    with pytest.raises(NotImplementedError, match="drop_path"):
        build_backbone(cfg)


def test_neck_refuses_a_fractional_output_size():
    from gaia_seg_amd.models.necks.dynamic_multilevel_neck import scaled_size
    assert scaled_size(32, 0.5) == 16 and scaled_size(3, 4) == 12 and scaled_size(5, 1) == 5
    with pytest.raises(ValueError, match="scales"):
        scaled_size(3, 0.5)


def _closed_form(d, heads, layers, ratios, h=512, w=1024, patch=16, neck_out=768, scales=(4, 2, 1, 0.5)):
    """backbone and neck FLOPs per image, written out"""
    hp, wp = h // patch, w // patch
    n = hp * wp + 1
    backbone = 2.0 * hp * wp * d * 3 * patch * patch                     # patch embedding
    for i in range(3):
        hw, hidden = 64 * heads[i], int(ratios[i] / 10 * d)
        layer = 3 * 2.0 * n * d * hw                                      # w_qs, w_ks, w_vs
        layer += 4.0 * n * n * 64 * heads[i]                              # Q K^T and P V
        layer += 2.0 * n * hw * d                                         # proj
        layer += 2 * 2.0 * n * d * hidden                                 # layer1, layer2
        backbone += layers[i] * layer
    neck = 4 * 2.0 * hp * wp * d * neck_out                               # four 1x1 laterals
    for s in scales:
        neck += 2.0 * (hp * s) * (wp * s) * neck_out * neck_out * 9       # 3x3 at the resized size
    return backbone, neck


def test_config_builds_and_counts_the_closed_form_flops():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.flops import model_flops
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import full_arch_meta
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    assert type(model.backbone).__name__ == "ElasticTransformer"
    assert type(model.neck).__name__ == "DynamicMultiLevelNeck"
    assert model.test_cfg.mode == "slide" and tuple(model.test_cfg.crop_size) == tuple(model.backbone.img_size)
    assert cfg.optimizer["type"] == "SGD" and cfg.model["backbone"]["drop_path"] == 0.0
    anchors = {m["name"]: m for m in build_model_sampler(cfg.val_sampler).traverse()}
    assert fold_dict(anchors["MAX"])["arch"] == full_arch_meta(model)
    first = build_model_sampler(cfg.train_sampler).candidates()[0]
    assert fold_dict(first)["arch"] == full_arch_meta(model)
    for name, spec in (("MIN", (384, [6] * 3, [2] * 3, [30] * 3)), ("MAX", (768, [12] * 3, [4] * 3, [40] * 3))):
        model.manipulate_arch(fold_dict(anchors[name])["arch"])
        f = model_flops(model, 512, 1024)
        backbone, neck = _closed_form(*spec)
        assert f["backbone"] == backbone and f["neck"] == neck, name
        assert f["total"] == f["backbone"] + f["neck"] + f["decode"] + f["aux"]
        assert f["decode"] > 0 and f["aux"] > 0 and f["decode"] == f["decode"]
    # a sampled subnet has ffn widths the kernels can run
    sampler = build_model_sampler(cfg.train_sampler)
    for _ in range(20):
        model.manipulate_arch(fold_dict(sampler.sample())["arch"])


@pytest.mark.parametrize("case", U.ATTENTION_CASES, ids=[c[0] for c in U.ATTENTION_CASES])
def test_operator_inputs_are_well_conditioned(case):
    """float32 torch on the GPU tests' own inputs stays below 1e-5 against float64, so the 3e-5 bound of
    tests/test_attention_gpu.py is a statement about the kernel and not about the data"""
    name, b, n, heads, _, dominant = case
    q, k, v, do = U.attention_inputs(b, n, heads, dominant, 5)[:4]
    ref, f32 = U.attention_ref(q, k, v, do, heads), U.attention_fp32(q, k, v, do, heads)
    for what, a, r in zip(("O", "lse", "dQ", "dK", "dV"), f32, ref):
        if n == 1 and what in ("dQ", "dK"):
            assert not bool(r.any()) and not bool(a.any())
            continue
        assert rel_err(a, r) < 1e-5, "%s %s: %.3g" % (name, what, rel_err(a, r))
    if dominant:   # the dominated queries' scores: the last key about 30 above the rest
        s = (q[:, ::2, :64] @ k[:, :, :64].transpose(1, 2)) * U.SCALE
        assert float((s[..., -1] - s[..., :-1].max(-1).values).min()) > 20
        assert n - 1 >= 2 * U.T, "the dominant key must lie in the last, ragged tile"


def test_vit_ref_matches_its_own_subnet_semantics():
    """vit_ref on the 'sub' slices of a max-size state dict equals vit_ref on physically sliced tensors"""
    net = build()
    U.randomize_vit(net, 1)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    x = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(2)).double()
    outs = U.vit_ref(sd, x, U.SUBNETS["sub"])
    assert len(outs) == 4 and all(tuple(o.shape) == (2, 64, 2, 3) for o in outs)
    assert len(U.vit_ref(sd, x, U.SUBNETS["max"])) == 4
