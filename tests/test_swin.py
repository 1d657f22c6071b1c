"""Swin's operators without a GPU: the float64 restatement of tests/util_swin.py against transformers' own
SwinLayer pieces, the float32 error of that restatement on the operator cases (the precondition of the GPU
tolerance), and what the C-ABI entries of csrc/window_attention.hip refuse before any launch (the addresses are
never read)."""
import ctypes

import pytest
import torch

from conftest import rel_err
import util_swin as S

OK_PTR, ODD_PTR, WORD_PTR = 1 << 20, (1 << 20) + 4, (1 << 20) + 2
BADARG, ALIGN, WORKSPACE, NULL = -1, -2, -3, -4


def test_abi_version_and_descriptor_sizes(hip_lib):
    from gaia_seg_amd.hip import lib
    assert lib.ABI_VERSION >= 25 and hip_lib.gs_abi_version() == lib.ABI_VERSION
    assert ctypes.sizeof(lib.WindowAttentionDesc) == 16 * 4 and ctypes.sizeof(lib.CellLayerNormDesc) == 8 * 4
    assert lib.WINDOW_ATTENTION_HEAD_DIM == S.HEAD_DIM == 32


@pytest.mark.parametrize("case", S.WA_CASES + [("split",) + S.SPLIT_CASE + (False, False)], ids=lambda c: c[0])
def test_float32_reference_error_is_far_below_the_gpu_tolerance(case):
    """wa_ref in float32 against float64 on the GPU tests' own inputs: < 1e-5 for every output, dTable included"""
    name, b, h, w, ws, shift, heads, _, dominant = case
    q, k, v, do, _, table = S.wa_inputs(b, h, w, ws, heads, dominant, 9 if name == "split" else 5)
    r64 = S.wa_ref(q, k, v, table, do, b, h, w, ws, shift, heads)
    r32 = S.wa_ref(q, k, v, table, do, b, h, w, ws, shift, heads, dtype=torch.float32)
    errs = [rel_err(a, r) for a, r in zip(r32, r64)]
    print(name, ["%.2e" % e for e in errs])
    assert max(errs) < 1e-5


@pytest.mark.parametrize("geom", [(7, 3, 14, 21, 3), (7, 0, 7, 14, 2), (4, 2, 8, 12, 5), (8, 4, 16, 8, 2)],
                         ids=lambda g: "ws%d-shift%d-%dx%d-h%d" % g)
def test_restatement_equals_transformers_swin_attention(geom):
    """wa_formula against transformers' roll + window_partition + SwinSelfAttention (sdpa) + get_attn_mask +
    window_reverse + roll back of a SwinLayer with always_partition, in float64"""
    transformers = pytest.importorskip("transformers")
    from transformers.models.swin import modeling_swin as MS
    ws, shift, h, w, heads = geom
    b, c = 2, S.HEAD_DIM * heads
    cfg = transformers.SwinConfig(embed_dim=c, depths=[1], num_heads=[heads], window_size=ws)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    layer = MS.SwinLayer(cfg, c, (h, w), heads, shift_size=shift).double().eval()
    att = layer.attention
    table = att.relative_position_bias.relative_position_bias_table.data.normal_(0, 0.5)
    x = torch.randn(b, h * w, c, dtype=torch.float64)
    with torch.no_grad():
        att.o_proj.weight.copy_(torch.eye(c))
        att.o_proj.bias.zero_()
        win = MS.window_partition(layer.cyclic_shift(x.view(b, h, w, c)), ws).view(-1, ws * ws, c)
        mask = layer.get_attn_mask(h, w, dtype=x.dtype, device=x.device)
        assert (mask is None) == (shift == 0)
        out = att(win, mask)[0].view(-1, ws, ws, c)
        want = layer.cyclic_shift(MS.window_reverse(out, ws, h, w), reverse=True).reshape(b, h * w, c)
        got, _ = S.wa_formula(att.q_proj(x), att.k_proj(x), att.v_proj(x), table, b, h, w, ws, shift, heads)
    assert rel_err(got, want) < 1e-12


def _wa_call(L, d, fwd=True, **kw):
    p = dict(q=OK_PTR, k=OK_PTR, v=OK_PTR, table=OK_PTR, o=OK_PTR, lse=OK_PTR, d_o=OK_PTR, dq=OK_PTR, dk=OK_PTR,
             dv=OK_PTR, dtable=OK_PTR, ws=OK_PTR, ws_bytes=None)
    p.update(kw)
    db = ctypes.byref(d) if d is not None else None
    if fwd:
        return L.gs_window_attention_forward(db, p["q"], p["k"], p["v"], p["table"], p["o"], p["lse"], None)
    need = L.gs_window_attention_workspace_bytes(db) if p["ws_bytes"] is None else p["ws_bytes"]
    return L.gs_window_attention_backward(db, p["q"], p["k"], p["v"], p["table"], p["o"], p["lse"], p["d_o"], p["dq"],
                                          p["dk"], p["dv"], p["dtable"], 0, p["ws"], need, None)


def test_window_attention_argument_checks_need_no_gpu(hip_lib):
    from gaia_seg_amd.hip import lib
    L = hip_lib

    def desc(**kw):
        d = lib.window_attention_desc(2, 14, 21, 7, 3, 3)
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    for fwd in (True, False):
        assert _wa_call(L, None, fwd) == NULL
        ptrs = ("q", "k", "v", "table", "o", "lse") + (() if fwd else ("d_o", "dq", "dk", "dv", "dtable", "ws"))
        for name in ptrs:
            assert _wa_call(L, desc(), fwd, **{name: None}) == NULL, name
            if name not in ("table", "dtable"):
                assert _wa_call(L, desc(), fwd, **{name: ODD_PTR}) == ALIGN, name
        for name in ("table",) + (() if fwd else ("dtable",)):
            assert _wa_call(L, desc(), fwd, **{name: WORD_PTR}) == ALIGN, name
        bad = [dict(B=0), dict(H=0), dict(W=0), dict(heads=0), dict(B=65536), dict(heads=65536, ldq=1 << 22),
               dict(ws=1), dict(ws=9), dict(H=15), dict(W=20), dict(shift=-1), dict(shift=7), dict(ldq=92),
               dict(lddo=92), dict(ld_table=2), dict(scale=0.0), dict(scale=-1.0)]
        for kw in bad:
            assert _wa_call(L, desc(**kw), fwd) == BADARG, kw
        for key in ("ldq", "ldk", "ldv", "ldo", "lddq", "lddk", "lddv", "lddo"):
            assert _wa_call(L, desc(**{key: 98}), fwd) == ALIGN, key
    assert L.gs_window_attention_workspace_bytes(ctypes.byref(desc(ws=9))) == 0
    need = L.gs_window_attention_workspace_bytes(ctypes.byref(desc()))
    assert need > 0 and _wa_call(L, desc(), False, ws_bytes=need - 1) == WORKSPACE


def test_window_attention_workspace_follows_the_split(hip_lib):
    """the query is S * heads * (2 ws - 1)^2 floats (rounded up to 16 bytes): it grows with a forced S, a forced
    S is clipped so that no slab is empty, and the plan is a pure function of the descriptor"""
    from gaia_seg_amd.hip import lib
    L = hip_lib
    b, h, w, ws, shift, heads = S.SPLIT_CASE
    d = lib.window_attention_desc(b, h, w, ws, shift, heads)
    part = heads * S.table_rows(ws) * 4

    def r16(x):
        return -(-x // 16) * 16
    plan = L.gs_window_attention_workspace_bytes(ctypes.byref(d))
    assert plan == L.gs_window_attention_workspace_bytes(ctypes.byref(d)) and plan % 16 == 0 and plan >= part
    try:
        sizes = []
        for s in S.SPLITS:
            assert L.gs_debug_set_window_attention_split(s) == 0
            sizes.append(L.gs_window_attention_workspace_bytes(ctypes.byref(d)))
        assert sizes == [r16(s * part) for s in S.SPLITS] and sizes == sorted(set(sizes))
        assert L.gs_debug_set_window_attention_split(1000) == 0          # more slabs than windows: 40
        assert L.gs_window_attention_workspace_bytes(ctypes.byref(d)) == r16(40 * part)
        assert L.gs_debug_set_window_attention_split(27) == 0            # ceil(40 / 27) = 2 per slab: 20 slabs
        assert L.gs_window_attention_workspace_bytes(ctypes.byref(d)) == r16(20 * part)
        assert L.gs_debug_set_window_attention_split(0) == BADARG and L.gs_debug_set_window_attention_split(-2) == BADARG
    finally:
        assert L.gs_debug_set_window_attention_split(-1) == 0
    assert L.gs_window_attention_workspace_bytes(ctypes.byref(d)) == plan


def test_map_and_cell_layernorm_argument_checks_need_no_gpu(hip_lib):
    from gaia_seg_amd.hip import lib
    L = hip_lib

    def pad(src=OK_PTR, dst=OK_PTR, lds=40, ldd=40, b=2, h=5, w=6, hp=7, wp=7, c=36):
        return (L.gs_map_pad(src, lds, dst, ldd, b, h, w, hp, wp, c, 0, None),
                L.gs_map_crop(dst, ldd, src, lds, b, h, w, hp, wp, c, 0, None))
    assert pad(src=None) == (NULL, NULL) and pad(dst=None) == (NULL, NULL)
    assert pad(src=ODD_PTR) == (ALIGN, ALIGN) and pad(c=34) == (ALIGN, ALIGN) and pad(lds=38) == (ALIGN, ALIGN)
    for kw in (dict(b=0), dict(h=0), dict(c=0), dict(hp=4), dict(wp=5), dict(lds=32), dict(ldd=32)):
        assert pad(**kw) == (BADARG, BADARG), kw

    def cell(fwd, x=OK_PTR, y=OK_PTR, wgt=OK_PTR, stat=OK_PTR, ws=OK_PTR, ws_bytes=None, **kw):
        d = lib.cell_layernorm_desc(2, 4, 6, 12, 20, ldx=16, ldy=16)
        for key, val in kw.items():
            setattr(d, key, val)
        db = ctypes.byref(d)
        if fwd:
            return L.gs_cell_layernorm_forward(db, x, wgt, wgt, y, stat, stat, None)
        need = L.gs_cell_layernorm_workspace_bytes(db) if ws_bytes is None else ws_bytes
        return L.gs_cell_layernorm_backward(db, x, y, wgt, stat, stat, x, wgt, wgt, 0, ws, need, None)
    for fwd in (True, False):
        assert cell(fwd, x=None) == NULL and cell(fwd, stat=None) == NULL and cell(fwd, wgt=None) == NULL
        assert cell(fwd, y=ODD_PTR) == ALIGN and cell(fwd, C=10) == ALIGN and cell(fwd, ldx=18) == ALIGN
        for kw in (dict(B=0), dict(H=3), dict(W=5), dict(C=24), dict(ldy=8), dict(eps=0.0)):
            assert cell(fwd, **kw) == BADARG, kw
    assert L.gs_cell_layernorm_forward(None, OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR, None) == NULL
    need = L.gs_cell_layernorm_workspace_bytes(ctypes.byref(lib.cell_layernorm_desc(2, 4, 6, 12, 20, ldx=16, ldy=16)))
    assert need == 1 * 2 * 48 * 4 and cell(False, ws_bytes=need - 1) == WORKSPACE and cell(False, ws=None) == NULL


# ---- the backbone --------------------------------------------------------------------------------------
WIDE = dict(depths=[2, 2, 2, 1], num_heads=[2, 4, 8, 16], window_size=7, mlp_ratio=4)
WIDE_SUB = dict(depth=[1, 2, 1, 1], num_heads=[1, 2, 4, 8], mlp_ratio=[4, 4, 4, 4])


def _backbone(base=S.TINY, **kw):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(S.tiny_backbone_cfg(base, **kw))
    S.randomize_swin(m, 3)
    return m


def _hf(arch, base):
    transformers = pytest.importorskip("transformers")
    return transformers.SwinBackbone(S.hf_config(base, arch)).double().eval()


@pytest.mark.parametrize("hw", [(64, 96), (224, 224)], ids=["64x96", "224x224"])
def test_reference_equals_transformers_swin_backbone_in_float64(hw):
    """swin_ref on a transformers state dict against SwinBackbone(...).double() (sdpa) at 1e-9: MAX"""
    hf = _hf(None, S.DOUBLING)
    sd = hf.state_dict()
    x = torch.randn(1 if hw[0] > 100 else 2, 3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = hf(x).feature_maps
        got = S.swin_ref(sd, x, S.DOUBLING_SUBNETS["max"])
    assert len(got) == 4
    for a, b in zip(got, want):
        assert a.shape == b.shape and rel_err(a, b) < 1e-9


def _slice_for(name, sd_super, sub_shape, cmax_of):
    """the subnet's tensor: leading slices, except the merge, whose [4 Cmax] axis is sliced group-wise"""
    t = sd_super[name]
    if ".downsample." in name:
        c = sub_shape[-1] // 4
        cmax = t.shape[-1] // 4
        cols = torch.cat([torch.arange(g * cmax, g * cmax + c) for g in range(4)])
        t = t[..., cols]
        return t[:sub_shape[0]] if t.dim() == 2 else t
    return t[tuple(slice(0, n) for n in sub_shape)]


@pytest.mark.parametrize("hw", [(64, 96), (224, 224)], ids=["64x96", "224x224"])
def test_a_doubling_subnet_equals_transformers_of_exactly_its_sizes(hw):
    """a supernet of heads 2/4/8/16 on subnet 1/2/4/8 with depths 1/2/1/1: swin_ref slices the supernet's state
    dict (the merge group-wise: columns g * Cmax + c by index); a SwinBackbone of exactly the subnet's sizes gets
    the same slices by name and must agree at 1e-9"""
    m = _backbone(WIDE).double()
    sd = m.state_dict()
    hf = _hf(WIDE_SUB, WIDE)
    sub_sd = {k: _slice_for(k, sd, tuple(v.shape), None) for k, v in hf.state_dict().items()}
    k = "swin.encoder.layers.1.downsample.norm.weight"           # by name and index: Cmax = 128, C = 64
    assert torch.equal(sub_sd[k], torch.cat([sd[k][g * 128:g * 128 + 64] for g in range(4)]))
    k = "swin.encoder.layers.1.downsample.reduction.weight"
    assert torch.equal(sub_sd[k][5, 64 + 3], sd[k][5, 128 + 3]) and sub_sd[k].shape == (128, 256)
    hf.load_state_dict(sub_sd, strict=True)
    x = torch.randn(1, 3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = hf(x).feature_maps
        got = S.swin_ref(sd, x, WIDE_SUB)
    for a, b in zip(got, want):
        assert a.shape == b.shape and rel_err(a, b) < 1e-9


def test_a_transformers_state_dict_loads_strictly_and_round_trips():
    hf = _hf(None, S.DOUBLING)
    m = _backbone(S.DOUBLING)
    sd = {k: v.float() for k, v in hf.state_dict().items()}
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd, strict=True)
    out = m.state_dict()
    for k, v in sd.items():
        assert out[k].shape == v.shape and torch.equal(out[k], v), k
    assert out["swin.encoder.layers.0.downsample.norm.weight"].shape == (4 * 32,)
    assert out["swin.encoder.layers.0.downsample.reduction.weight"].shape == (64, 4 * 32)
    # the reduction is held as a 2x2 conv: tap (row, col) of input c is column (2 col + row) * Cmax + c
    red = m.stages[0].downsample.reduction
    assert torch.equal(red.weight[7, 5, 1, 0], sd["swin.encoder.layers.0.downsample.reduction.weight"][7, 1 * 32 + 5])
    assert torch.equal(red.weight[7, 5, 0, 1], sd["swin.encoder.layers.0.downsample.reduction.weight"][7, 2 * 32 + 5])


def test_arch_manipulation_and_active_modules():
    m = _backbone()
    assert m.full_arch_meta() == {"body": S.SUBNETS["max"]}
    meta = {"body": {k: list(v) for k, v in S.SUBNETS["sub"].items()}}
    keep = {"body": {k: list(v) for k, v in S.SUBNETS["sub"].items()}}
    m.manipulate_arch(meta)
    assert meta == keep                                            # metas are only read
    st = m.stages
    assert [s.depth_state for s in st] == [1, 2, 1, 1] and [s.num_heads_state for s in st] == [1, 2, 2, 1]
    assert m.swin.embeddings.patch_embeddings.projection.width_state == 32
    assert [st[i].downsample.reduction.width_state for i in range(3)] == [64, 64, 32]
    b = st[1].blocks[1]
    assert b.attention.q_proj.width_state == 64 and b.mlp.fc1.width_state == 128 and b.mlp.fc2.width_state == 64
    assert st[2].blocks[0].mlp.fc1.width_state == int(3 * 64) and [blk.shift for blk in st[0].blocks] == [0, 3]
    active = m.active_modules()
    assert st[0].blocks[0] in active and st[0].blocks[1] not in active and st[2].blocks[1] not in active
    assert m.swin.layernorm not in active and st[0].downsample in active and st[3].downsample is None
    assert all(m.hidden_states_norms["stage%d" % i] in active for i in (1, 2, 3, 4))
    late = {id(p) for p in m.late_gradient_parameters()}
    assert id(st[0].blocks[0].attention.q_proj.weight) in late and id(st[1].blocks[0].attention.q_proj.weight) not in late
    with pytest.raises(ValueError):
        m.manipulate_arch({"body": dict(depth=[3, 2, 2, 1], num_heads=[2, 2, 3, 2], mlp_ratio=[4] * 4)})
    with pytest.raises(ValueError):
        m.manipulate_arch({"body": dict(depth=[2, 2, 2, 1], num_heads=[3, 2, 3, 2], mlp_ratio=[4] * 4)})
    with pytest.raises(ValueError, match="multiple of 4"):
        m.manipulate_arch({"body": dict(depth=[2, 2, 2, 1], num_heads=[1, 2, 3, 2], mlp_ratio=[0.33, 4, 4, 4])})


@pytest.mark.parametrize("kw,key", [(dict(drop_path_rate=0.1), "drop_path_rate"), (dict(drop_rate=0.1), "drop_rate"),
                                    (dict(attn_drop_rate=0.1), "attn_drop_rate"),
                                    (dict(use_abs_pos_embed=True), "use_abs_pos_embed"),
                                    (dict(window_size=12), "window_size"), (dict(window_size=1), "window_size")])
def test_refusals_name_their_key(kw, key):
    from gaia_seg_amd.models import build_backbone
    with pytest.raises(NotImplementedError, match=key):
        build_backbone(S.tiny_backbone_cfg(**kw))


def test_fp16_attention_and_a_table_of_another_window_are_refused():
    m = _backbone()
    assert m.fp16_attention is False
    m.fp16_attention = False
    with pytest.raises(NotImplementedError, match="fp16.attention"):
        m.fp16_attention = True
    other = _backbone(window_size=4).state_dict()
    with pytest.raises(NotImplementedError, match="relative_position_bias_table"):
        m.load_state_dict(other, strict=True)


# ---- the recipe and its FLOPs ------------------------------------------------------------------------------
def _closed_form(depth, heads, ratio, h, w, ws=7, cin=3):
    """backbone FLOPs per image, written out: what runs"""
    h, w = h // 4, w // 4
    total = 2.0 * h * w * 32 * heads[0] * cin * 16                        # the 4x4 stride-4 patch embedding
    for i in range(4):
        d, hidden = 32 * heads[i], int(ratio[i] * 32 * heads[i])
        hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
        block = 3 * 2.0 * hp * wp * d * d + 2.0 * h * w * d * d           # q, k, v on the padded map; o on the cropped
        block += 2 * 2.0 * hp * wp * ws * ws * 32 * heads[i]              # Q K^T and P V inside the windows
        block += 2 * 2.0 * h * w * d * hidden                             # fc1, fc2
        total += depth[i] * block
        if i < 3:
            h, w = h // 2, w // 2
            total += 2.0 * h * w * 32 * heads[i + 1] * d * 4              # the merge: a 2x2 stride-2 conv
    return total


def test_flops_of_the_tiny_backbone_equal_the_closed_form():
    from gaia_seg_amd.core.flops import backbone_flops
    m = _backbone()
    got = {}
    for name in ("max", "sub"):
        a = S.SUBNETS[name]
        m.manipulate_arch({"body": a})
        total, params, _, feats = got[name] = backbone_flops(m, 64, 96)
        assert total == _closed_form(a["depth"], a["num_heads"], a["mlp_ratio"], 64, 96), name
        assert feats == [(32 * hd, 64 // s, 96 // s) for hd, s in zip(a["num_heads"], (4, 8, 16, 32))]
    assert got["max"][0] > got["sub"][0] and got["max"][1] > got["sub"][1]
    unread = sum(p.numel() for p in m.swin.layernorm.parameters())
    m.manipulate_arch(m.full_arch_meta())
    assert got["max"][1] == sum(p.numel() for p in m.parameters()) - unread


def test_config_builds_and_its_anchors_fold_to_legal_archs():
    import os
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.flops import model_flops
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.optimizer import build_param_groups
    from gaia_seg_amd.core.runner import full_arch_meta
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(os.path.join(lib.REPO_ROOT, "configs", "supernet", "upernet_swin_t2b_adamw.py"))
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    assert type(model.backbone).__name__ == "DynamicSwinTransformer"
    assert type(model.decode_head).__name__ == "DynamicUPerHead" and model.auxiliary_head.in_index == 2
    assert cfg.optimizer["type"] == "AdamW" and cfg.lr_config["warmup"] == "linear" and cfg.lr_config["power"] == 1.0
    pg = build_param_groups(model, cfg.optimizer)
    groups = {name: pg.groups[i] for name, i in pg.index.items()}
    blk = "backbone.swin.encoder.layers.0.blocks.0."
    assert groups["auxiliary_head.conv_seg.weight"] == (10.0, 1.0)
    assert groups[blk + "layernorm_before.weight"] == (1.0, 0.0)
    assert groups["backbone.swin.encoder.layers.0.downsample.norm.weight"] == (1.0, 0.0)
    assert groups[blk + "attention.relative_position_bias.relative_position_bias_table"] == (1.0, 0.0)
    assert groups[blk + "attention.q_proj.weight"] == (1.0, 1.0)
    anchors = {m["name"]: m for m in build_model_sampler(cfg.val_sampler).traverse()}
    assert sorted(anchors) == ["MAX", "MID", "MIN"]
    assert fold_dict(anchors["MAX"])["arch"] == full_arch_meta(model)
    assert anchors["MIN"]["arch.backbone.body.depth"] == [2, 2, 6, 2]
    assert anchors["MIN"]["arch.backbone.body.num_heads"] == [3, 6, 12, 24]
    assert min(anchors["MID"]["arch.backbone.body.mlp_ratio"]) < 4
    flops = {}
    for name, meta in anchors.items():
        arch = fold_dict(meta)["arch"]
        model.manipulate_arch(arch)                      # a hidden width that is no multiple of 4 raises here
        body = arch["backbone"]["body"]
        flops[name] = model_flops(model, 512, 1024)
        assert flops[name]["backbone"] == _closed_form(body["depth"], body["num_heads"], body["mlp_ratio"], 512, 1024)
    assert flops["MAX"]["total"] > flops["MID"]["total"] > flops["MIN"]["total"] > 0
    sampler = build_model_sampler(cfg.train_sampler)
    for _ in range(20):
        model.manipulate_arch(fold_dict(sampler.sample())["arch"])
