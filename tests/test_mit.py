"""SegFormer without a GPU: the C-ABI surface and the refusals of gs_attention_kv_*, the constructor's names
against transformers' SegformerModel, tests/util_mit.py's float64 reference against that independent
implementation, the search space, the refusals, the recipe and its FLOP count, and the conditioning of the
operator tests' inputs."""
import copy
import ctypes
import os
import re

import pytest
import torch

from conftest import rel_err
import util_mit as M
import util_vit as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CONFIG = os.path.join(ROOT, "configs", "supernet", "segformer_mit_b1to3_adamw.py")
GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4


def build(**kw):
    from gaia_seg_amd.models import build_backbone
    return build_backbone(M.tiny_backbone_cfg(**kw))


# ---- the C-ABI ---------------------------------------------------------------------------------------------
def test_library_exports_attention_kv_abi(hip_lib):
    from gaia_seg_amd.hip import lib
    for name in ("gs_attention_kv_forward", "gs_attention_kv_workspace_bytes", "gs_attention_kv_backward",
                 "gs_debug_set_attention_kv_split"):
        assert name in lib.PROTOTYPES and hasattr(hip_lib, name)
    assert lib.ABI_VERSION >= 24 and hip_lib.gs_abi_version() == lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "gaiaseg_hip.h")) as f:
        header = f.read()
    for name in ("gs_attention_kv_forward", "gs_attention_kv_workspace_bytes", "gs_attention_kv_backward",
                 "gs_debug_set_attention_kv_split"):
        assert re.search(r"\b%s\(" % name, header), name
    body = re.search(r"typedef struct gs_attention_kv_desc \{(.*?)\} gs_attention_kv_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [n for n, _ in fields] == [n for n, _ in lib.AttentionKvDesc._fields_]
    assert all(t in ("int32_t", "float") for _, t in fields)
    assert ctypes.sizeof(lib.AttentionKvDesc) == 4 * len(fields) == 52
    d = lib.attention_kv_desc(2, 7, 3, 3, ldq=576, ldo=200)
    assert (d.Nq, d.Nk, d.ldq, d.ldk, d.lddq, d.lddk, d.ldo, d.lddo) == (7, 3, 576, 192, 576, 192, 200, 200)
    assert abs(d.scale - 0.125) < 1e-9


def test_attention_kv_refusals_need_no_device(hip_lib):
    """every documented code, returned before any launch (the pointers are never dereferenced)"""
    from gaia_seg_amd.hip import lib
    L = hip_lib
    b, nq, nk, heads, c = 1, 5, 3, 2, 128
    p = 4096   # an aligned, non-null "pointer"

    def fwd(d, q=p, o=p, lse=p):
        return L.gs_attention_kv_forward(ctypes.byref(d) if d is not None else None, q, p, p, o, lse, None)

    def bwd(d, dq=p, wsp=p, wsb=1 << 20):
        return L.gs_attention_kv_backward(ctypes.byref(d) if d is not None else None, p, p, p, p, p, p, dq, p, p, 0,
                                          wsp, wsb, None)

    def desc(**kw):
        d = lib.attention_kv_desc(b, nq, nk, heads, U.SCALE)
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    good = desc()
    need = L.gs_attention_kv_workspace_bytes(ctypes.byref(good))
    assert need == 4 * b * heads * nq + 8    # delta[B][heads][Nq], rounded up to 16 bytes: one slab at this size
    assert fwd(None) == GS_E_NULL and bwd(None) == GS_E_NULL and L.gs_attention_kv_workspace_bytes(None) == 0
    assert fwd(good, q=None) == GS_E_NULL and fwd(good, o=None) == GS_E_NULL and fwd(good, lse=None) == GS_E_NULL
    assert bwd(good, dq=None) == GS_E_NULL and bwd(good, wsp=None) == GS_E_NULL
    for bad in (desc(B=0), desc(Nq=0), desc(Nk=0), desc(Nq=-3), desc(Nk=-1), desc(heads=0), desc(scale=0.0),
                desc(scale=-1.0), desc(ldq=c - 4), desc(ldo=64), desc(lddk=c - 4)):
        assert fwd(bad) == GS_E_BADARG and bwd(bad) == GS_E_BADARG
        assert L.gs_attention_kv_workspace_bytes(ctypes.byref(bad)) == 0
    for bad in (desc(ldk=c + 2), desc(lddv=c + 1)):
        assert fwd(bad) == GS_E_ALIGN and bwd(bad) == GS_E_ALIGN
        assert L.gs_attention_kv_workspace_bytes(ctypes.byref(bad)) == 0
    assert fwd(good, q=p + 4) == GS_E_ALIGN and fwd(good, o=p + 8) == GS_E_ALIGN
    assert bwd(good, dq=p + 4) == GS_E_ALIGN and bwd(good, wsp=p + 4) == GS_E_ALIGN
    assert bwd(good, wsb=need - 1) == GS_E_WORKSPACE and bwd(good, wsb=0) == GS_E_WORKSPACE
    # the forced split: the workspace follows it; a short one is refused; the setter refuses 0 and below -1
    try:
        assert L.gs_debug_set_attention_kv_split(2) == 0
        need2 = L.gs_attention_kv_workspace_bytes(ctypes.byref(desc(Nq=70)))
        assert need2 == 4 * heads * 70 + 2 * 2 * nk * c * 4
        assert bwd(desc(Nq=70), wsb=need2 - 1) == GS_E_WORKSPACE
        assert L.gs_debug_set_attention_kv_split(0) == GS_E_BADARG and L.gs_debug_set_attention_kv_split(-2) == GS_E_BADARG
        # more slabs than query tiles: clipped to one tile per slab
        assert L.gs_debug_set_attention_kv_split(50) == 0
        assert L.gs_attention_kv_workspace_bytes(ctypes.byref(desc(Nq=70))) == 4 * heads * 70 + 3 * 2 * nk * c * 4
    finally:
        assert L.gs_debug_set_attention_kv_split(-1) == 0
    assert L.gs_attention_kv_workspace_bytes(ctypes.byref(good)) == need


def test_split_plan_is_a_function_of_the_descriptor(hip_lib):
    """the planned workspace at the recipe's four stage shapes: S slabs of whole tiles, never below 4 query
    tiles per slab, never more workgroups than CUs (the dK / dV kernel runs one workgroup per CU; 256 CUs are
    assumed without a device), and at least half of them in use"""
    from gaia_seg_amd.hip import lib
    cus = hip_lib.gs_debug_num_cu()
    for b, nq, nk, heads in ((2, 32768, 512, 1), (2, 8192, 512, 2), (2, 2048, 512, 5), (2, 512, 512, 8)):
        d = lib.attention_kv_desc(b, nq, nk, heads)
        need = hip_lib.gs_attention_kv_workspace_bytes(ctypes.byref(d))
        assert need == hip_lib.gs_attention_kv_workspace_bytes(ctypes.byref(d))
        part = 2 * b * nk * 64 * heads * 4
        s, rest = divmod(need - 4 * b * heads * nq, part)
        assert rest == 0 and s > 1, "every stage shape leaves CUs idle at one slab"
        wgs = -(-nk // 128) * heads * b
        assert cus // 2 < s * wgs <= cus and nq // 32 // s >= 4, (nq, s)


# ---- the constructor ---------------------------------------------------------------------------------------
def _hf(name):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(3)
    return transformers.SegformerModel(M.hf_config(M.SUBNETS[name])).eval()


def test_state_dict_names_and_shapes():
    net = build()
    sd = net.state_dict()
    w = M.widths(M.SUBNETS["max"])
    assert tuple(sd["stages.0.patch_embeddings.proj.weight"].shape) == (64, 3, 7, 7)
    assert tuple(sd["stages.2.patch_embeddings.proj.weight"].shape) == (192, 128, 3, 3)
    assert tuple(sd["stages.1.blocks.1.attention.k_proj.weight"].shape) == (128, 128)
    assert tuple(sd["stages.1.blocks.0.attention.sequence_reduction.sequence_reduction.weight"].shape) == (128, 128, 4, 4)
    assert tuple(sd["stages.2.blocks.0.mlp.fc1.weight"].shape) == (768, 192)
    assert tuple(sd["stages.2.blocks.0.mlp.dwconv.dwconv.weight"].shape) == (768, 1, 3, 3)
    assert tuple(sd["stages.3.layer_norm.bias"].shape) == (128,)
    assert not any("sequence_reduction" in k for k in sd if k.startswith("stages.3."))   # sr_ratio 1
    per_block = 18
    assert len(sd) == sum(6 + d * per_block + (4 * d if sr > 1 else 0)
                          for d, sr in zip(M.TINY["num_layers"], M.TINY["sr_ratios"]))
    assert [net.stages[i].layer_norm.weight.shape[0] for i in range(4)] == w
    assert net.stages[0].layer_norm.eps == 1e-6


def test_a_transformers_state_dict_loads_strictly():
    hf = _hf("max")
    net = build()
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want
    assert list(net.state_dict()) == list(want)
    net.load_state_dict(hf.state_dict(), strict=True)
    for k, v in hf.state_dict().items():
        assert torch.equal(net.state_dict()[k], v), k


@pytest.mark.parametrize("name", ["max", "sub"])
def test_reference_equals_transformers_in_float64(name):
    """util_mit.mit_ref against SegformerModel(...).double() on 2 x 3 x 64 x 96: the max arch on the model's own
    weights, the subnet on a model of the subnet's sizes loaded with the leading slices of the max-size
    weights.  (transformers builds every LayerNorm with torch's default eps, whatever its config says: the
    reference is called with that eps.)"""
    hf_max = _hf("max").double()
    sd = hf_max.state_dict()
    hf = hf_max
    if name == "sub":
        hf = _hf("sub").double()
        sliced = {}
        for k, v in hf.state_dict().items():
            idx = M.active_slice(k, M.SUBNETS["sub"])
            assert idx is not None, k
            sliced[k] = sd[k][idx].clone()
            assert sliced[k].shape == v.shape, k
        hf.load_state_dict(sliced, strict=True)
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        want = hf(x, output_hidden_states=True).hidden_states
        got = M.mit_ref(sd, x, M.SUBNETS[name], eps=hf.stages[0].layer_norm.eps)
    assert len(got) == len(want) == 4
    for i, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape and rel_err(g, r) < 1e-9, (i, rel_err(g, r))


# ---- conditioning of the operator tests' inputs ------------------------------------------------------------
@pytest.mark.parametrize("case", M.KV_CASES + [("split",) + M.SPLIT_CASE + (False, False)],
                         ids=[c[0] for c in M.KV_CASES] + ["split"])
def test_operator_inputs_are_well_conditioned(case):
    """float32 torch on the GPU tests' own inputs stays below 1e-5 against float64, so the 3e-5 bound of
    tests/test_attention_kv_gpu.py is a statement about the kernels and not about the data"""
    name, b, nq, nk, heads, _, dominant = case
    q, k, v, do = M.kv_inputs(b, nq, nk, heads, dominant, 9 if name == "split" else 5)[:4]
    ref, f32 = M.kv_ref(q, k, v, do, heads), M.kv_ref(q, k, v, do, heads, dtype=torch.float32)
    for what, a, r in zip(("O", "lse", "dQ", "dK", "dV"), f32, ref):
        if nk == 1 and what in ("dQ", "dK"):
            assert not bool(r.any()) and not bool(a.any())
            continue
        assert rel_err(a, r) < 1e-5, "%s %s: %.3g" % (name, what, rel_err(a, r))
    if dominant:   # the dominated queries' scores: the last key about 30 above the rest, in the ragged key tile
        s = (q[:, ::2, :64] @ k[:, :, :64].transpose(1, 2)) * U.SCALE
        assert float((s[..., -1] - s[..., :-1].max(-1).values).min()) > 20
        assert (nk - 1) % 32 < 31 and nk - 1 >= 32


# ---- arch manipulation -------------------------------------------------------------------------------------
def _state(net):
    return [(st.depth_state, st.patch_embeddings.proj.width_state,
             [(b.attention.num_heads, b.attention.q_proj.width_state, b.attention.k_proj.width_state,
               b.attention.o_proj.width_state, b.mlp.fc1.width_state, b.mlp.fc2.width_state) for b in st.blocks])
            for st in net.stages]


def test_manipulate_arch_sets_the_widths_and_leaves_the_meta_alone():
    net = build()
    assert net.search_space == {"body"}
    meta = M.arch_of("sub")
    frozen = copy.deepcopy(meta)
    net.manipulate_arch(meta)
    first = _state(net)
    net.manipulate_arch(meta)
    assert _state(net) == first and meta == frozen, "manipulate_arch changed the meta or the subnet"
    a = M.SUBNETS["sub"]
    for i, (depth, width, blocks) in enumerate(first):
        d = 64 * a["num_heads"][i]
        assert depth == a["depth"][i] and width == d
        for heads, wq, wk, wo, hidden, out in blocks:   # every block of the stage, skipped ones included
            assert heads == a["num_heads"][i] and wq == wk == wo == out == d
            assert hidden == int(a["mlp_ratio"][i] * d)
    net.manipulate_arch(net.full_arch_meta())
    assert net.full_arch_meta() == M.arch_of("max")
    assert _state(net)[2][2][0] == (3, 192, 192, 192, 768, 192)
    with pytest.raises(KeyError):
        net.manipulate_arch({"encoder": {}})
    with pytest.raises(ValueError, match="mlp_ratio"):
        net.manipulate_arch({"body": dict(meta["body"], mlp_ratio=[2, 4, 3, 2.05])})   # int(2.05 * 64) = 131
    with pytest.raises(ValueError, match="num_heads"):
        net.manipulate_arch({"body": dict(meta["body"], num_heads=[1, 3, 2, 1])})
    with pytest.raises(ValueError, match="depth"):
        net.manipulate_arch({"body": dict(meta["body"], depth=[1, 3, 1, 1])})


def test_active_modules_leave_out_the_skipped_blocks():
    net = build()
    net.manipulate_arch(M.arch_of("sub"))
    active = {id(p) for m in net.active_modules() for p in m.parameters()}
    names = {n for n, p in net.named_parameters() if id(p) in active}
    assert "stages.0.patch_embeddings.proj.weight" in names and "stages.3.layer_norm.bias" in names
    assert "stages.1.blocks.0.attention.sequence_reduction.layer_norm.weight" in names
    assert len([n for n in names if n.startswith("stages.1.blocks.0.")]) == 22
    assert not any(n.startswith("stages.1.blocks.1.") for n in names), "a skipped block is active"
    assert len(names) == len(list(net.named_parameters())) - 22
    late = {id(p) for p in net.late_gradient_parameters()}
    late_names = {n for n, p in net.named_parameters() if id(p) in late}
    assert late <= active and late_names == {n for n in names if n.startswith("stages.0.")}


@pytest.mark.parametrize("key", ["drop_path_rate", "drop_rate", "attn_drop_rate"])
def test_refusals_name_the_key(key):
    with pytest.raises(NotImplementedError, match=key):
        build(**{key: 0.1})


def test_fp16_attention_is_refused_with_its_key():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    small = copy.deepcopy(cfg.model)
    small["backbone"].update(num_layers=[1, 1, 1, 1], num_heads=[1, 1, 1, 1])
    small["decode_head"].update(in_channels=[64] * 4, channels=16)
    small["auxiliary_head"].update(in_channels=64, channels=16)
    model = build_segmentor(small)
    with pytest.raises(NotImplementedError, match=r"fp16\.attention"):
        wrap_fp16_model(model, attention=True)
    assert wrap_fp16_model(model, attention=False) is model and model.backbone.fp16_attention is False


# ---- the recipe and its FLOPs ------------------------------------------------------------------------------
def _closed_form(depth, heads, ratio, h, w, sr=(8, 4, 2, 1), patch=(7, 3, 3, 3), stride=(4, 2, 2, 2), cin=3):
    """backbone FLOPs per image, written out"""
    total = 0.0
    for i in range(4):
        h, w, d = h // stride[i], w // stride[i], 64 * heads[i]
        nq, nk, hidden = h * w, (h // sr[i]) * (w // sr[i]), int(ratio[i] * d)
        total += 2.0 * nq * d * cin * patch[i] ** 2                       # overlapping patch embedding
        block = 2 * 2.0 * nq * d * d + 2 * 2.0 * nk * d * d               # q_proj, o_proj; k_proj, v_proj
        if sr[i] > 1:
            block += 2.0 * nk * d * d * sr[i] ** 2                        # the reduction conv
        block += 2 * 2.0 * nq * nk * 64 * heads[i]                        # Q K^T and P V
        block += 2 * 2.0 * nq * d * hidden + 2.0 * nq * hidden * 9        # fc1, fc2; the depthwise 3x3
        total += depth[i] * block
        cin = d
    return total


def test_flops_of_the_tiny_model_equal_the_closed_form():
    from gaia_seg_amd.core.flops import model_flops
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(copy.deepcopy(M.tiny_model_cfg()))
    got = {}
    for name in ("max", "sub"):
        a = M.SUBNETS[name]
        model.manipulate_arch({"backbone": M.arch_of(name)})
        f = got[name] = model_flops(model, 64, 96)
        assert f["backbone"] == _closed_form(a["depth"], a["num_heads"], a["mlp_ratio"], 64, 96), name
        w = M.widths(a)
        p0 = 16 * 24
        decode = sum(2.0 * (p0 >> (2 * i)) * w[i] * 16 for i in range(4)) + 2.0 * p0 * 64 * 16 + 2.0 * p0 * 16 * 19
        aux = 2.0 * 4 * 6 * w[2] * 16 * 9 + 2.0 * 4 * 6 * 16 * 19
        assert f["decode"] == decode and f["aux"] == aux, name
        assert f["total"] == f["backbone"] + f["decode"] + f["aux"]
    assert got["max"]["total"] > got["sub"]["total"] and got["max"]["backbone_params"] > got["sub"]["backbone_params"]
    n_max = sum(p.numel() for p in model.backbone.parameters())
    assert got["max"]["backbone_params"] == n_max


def test_config_builds_and_its_anchors_fold_to_legal_archs():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.flops import model_flops
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.optimizer import build_param_groups
    from gaia_seg_amd.core.runner import full_arch_meta
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    assert type(model.backbone).__name__ == "DynamicMixVisionTransformer"
    assert type(model.decode_head).__name__ == "DynamicSegformerHead" and model.test_cfg.mode == "whole"
    assert cfg.optimizer["type"] == "AdamW" and cfg.lr_config["warmup"] == "linear" and cfg.lr_config["power"] == 1.0
    pg = build_param_groups(model, cfg.optimizer)
    groups = {name: pg.groups[i] for name, i in pg.index.items()}
    assert groups["decode_head.fusion_conv.conv.weight"] == (10.0, 1.0)
    assert groups["auxiliary_head.conv_seg.weight"] == (10.0, 1.0)
    assert groups["backbone.stages.0.blocks.0.layernorm_before.weight"] == (1.0, 0.0)
    assert groups["backbone.stages.0.blocks.0.attention.q_proj.weight"] == (1.0, 1.0)
    anchors = {m["name"]: m for m in build_model_sampler(cfg.val_sampler).traverse()}
    assert sorted(anchors) == ["MAX", "MID", "MIN"]
    assert fold_dict(anchors["MAX"])["arch"] == full_arch_meta(model)
    flops = {}
    for name, meta in anchors.items():
        arch = fold_dict(meta)["arch"]
        model.manipulate_arch(arch)                      # a hidden width that is no multiple of 4 raises here
        body = arch["backbone"]["body"]
        flops[name] = model_flops(model, 512, 1024)
        assert flops[name]["backbone"] == _closed_form(body["depth"], body["num_heads"], body["mlp_ratio"], 512, 1024)
    assert flops["MAX"]["total"] > flops["MID"]["total"] > flops["MIN"]["total"] > 0
    assert anchors["MIN"]["arch.backbone.body.depth"] == [2, 2, 2, 2]
    sampler = build_model_sampler(cfg.train_sampler)
    for _ in range(20):
        model.manipulate_arch(fold_dict(sampler.sample())["arch"])
