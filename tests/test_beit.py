"""The BEiT backbone and its two operators without a GPU: the C-ABI's host argument checks, the
relative-position index against the values the reference's constructor produces
(tests/golden/ref_beit_ctors.json, written by tests/golden/make_ref_beit_ctor_fixture.py), state-dict names
and shapes in every variant, checkpoint loading, the initialisation and the refusals."""
import ctypes
import json
import os

import pytest
import torch

import util_beit as U

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ref_beit_ctors.json")
GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
OK_PTR, ODD_PTR = 1 << 20, (1 << 20) + 4      # never read: every call below is refused before a launch
# the kernel-backed class that stands where the reference has a torch one
KERNEL_TYPE = {"Linear": "DynamicLinear", "LayerNorm": "DynamicLayerNorm", "Conv2d": "DynamicConv2d",
               "ConvTranspose2d": "ConvTranspose2x2", "SyncBatchNorm": "DynamicBatchNorm2d",
               "MaxPool2d": "MaxPool"}


def _cases():
    with open(FIXTURE) as f:
        return json.load(f)


CASES = _cases()


def _build(kwargs):
    from gaia_seg_amd.models import build_backbone
    return build_backbone(dict(type="BEiT", **kwargs))


def test_header_binding_and_exports_agree_with_the_new_symbols(hip_lib):
    import test_c_abi
    from gaia_seg_amd.hip import lib
    test_c_abi.test_header_and_binding_agree()
    test_c_abi.test_library_exports_every_symbol()
    for name in ("gs_attention_relpos_forward", "gs_deconv2x2_forward", "gs_deconv2x2_workspace_bytes"):
        assert name in lib.PROTOTYPES and hasattr(hip_lib, name)


def test_relpos_attention_argument_checks_need_no_gpu(hip_lib):
    from gaia_seg_amd.hip import lib
    L = hip_lib

    def call(d, q=OK_PTR, table=OK_PTR, ld_table=2, wh=2, ww=3, o=OK_PTR, lse=OK_PTR):
        return L.gs_attention_relpos_forward(ctypes.byref(d) if d is not None else None, q, OK_PTR, OK_PTR, table,
                                             ld_table, wh, ww, o, lse, None)

    def desc(n=7, heads=2, **kw):
        d = lib.attention_desc(1, n, heads)
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    assert call(None) == GS_E_NULL
    assert call(desc(), table=None) == GS_E_NULL                   # null table
    assert call(desc(), q=None) == GS_E_NULL and call(desc(), lse=None) == GS_E_NULL
    assert call(desc(n=8)) == GS_E_BADARG                          # N != Wh * Ww + 1
    assert call(desc(n=6)) == GS_E_BADARG
    assert call(desc(), wh=0, ww=3) == GS_E_BADARG and call(desc(), wh=2, ww=-3) == GS_E_BADARG
    assert call(desc(), ld_table=1) == GS_E_BADARG                 # ld_table < heads
    assert call(desc(), q=ODD_PTR) == GS_E_ALIGN                   # misaligned pointer
    assert call(desc(), o=ODD_PTR) == GS_E_ALIGN and call(desc(), table=OK_PTR + 2) == GS_E_ALIGN
    assert call(desc(ldq=130)) == GS_E_ALIGN                       # odd pitch
    assert call(desc(ldo=64)) == GS_E_BADARG and call(desc(heads=0)) == GS_E_BADARG
    # the window cap: 32 x 64 and 40 x 40 are admitted by the size check (refused here only for the null
    # table that follows it), 64 x 64 is not
    for wh, ww, want in ((32, 64, GS_E_NULL), (40, 40, GS_E_NULL), (64, 64, GS_E_BADARG), (33, 64, GS_E_BADARG)):
        assert call(desc(n=wh * ww + 1), table=None, wh=wh, ww=ww) == want, (wh, ww)
    assert (2 * 32 - 1) * (2 * 64 - 1) + 3 <= lib.ATTENTION_RELPOS_MAX_ROWS < (2 * 33 - 1) * (2 * 64 - 1) + 3



def test_deconv_argument_checks_need_no_gpu(hip_lib):
    L = hip_lib
    need = L.gs_deconv2x2_workspace_bytes(2, 3, 5, 8, 12)
    assert need >= 2 * 3 * 5 * 4 * 12 * 4
    assert L.gs_deconv2x2_workspace_bytes(2, 3, 5, 6, 12) == 0 and L.gs_deconv2x2_workspace_bytes(0, 3, 5, 8, 12) == 0

    def call(x=OK_PTR, n=2, h=3, w=5, cin=8, ldx=8, w4=OK_PTR, cout=12, bias=OK_PTR, y=OK_PTR, ldy=12, ws=OK_PTR,
             ws_bytes=need):
        return L.gs_deconv2x2_forward(x, n, h, w, cin, ldx, w4, cout, bias, y, ldy, ws, ws_bytes, None)

    assert call(x=None) == GS_E_NULL and call(w4=None) == GS_E_NULL and call(y=None) == GS_E_NULL
    assert call(n=0) == GS_E_BADARG and call(h=-1) == GS_E_BADARG and call(cout=0) == GS_E_BADARG
    assert call(ldx=4) == GS_E_BADARG and call(ldy=8) == GS_E_BADARG
    assert call(cin=6) == GS_E_ALIGN and call(cout=10) == GS_E_ALIGN
    assert call(ldx=10) == GS_E_ALIGN and call(ldy=14) == GS_E_ALIGN                       # odd pitch
    assert call(x=ODD_PTR) == GS_E_ALIGN and call(y=ODD_PTR) == GS_E_ALIGN                 # misaligned pointer
    assert call(bias=ODD_PTR) == GS_E_ALIGN and call(w4=ODD_PTR) == GS_E_ALIGN
    assert call(ws=None) == GS_E_WORKSPACE and call(ws_bytes=need - 1) == GS_E_WORKSPACE
    assert call(n=1 << 20, h=1 << 10, w=1 << 10) == GS_E_BADARG                            # > 2^31 - 1 output pixels


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_names_shapes_and_index_equal_the_reference_constructor(case):
    from gaia_seg_amd.models.backbones.beit import relative_position_index
    net = _build(case["kwargs"])
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == case["state_dict"]
    theirs = dict(map(tuple, case["modules"]))
    mine = {p: type(m).__name__ for p, m in net.named_modules() if p}
    assert set(mine) == set(theirs)
    for path, name in theirs.items():
        assert mine[path] == KERNEL_TYPE.get(name, name), path
    patch = case["kwargs"]["patch_size"]
    wh, ww = (s // patch for s in case["kwargs"]["img_size"])
    want = case["relative_position_index"]
    assert len(want) == {"block_tables": 4, "shared_bias": 1, "abs_pos_only": 0}[case["tag"].split("_", 2)[2]]
    for key, values in want.items():
        ref = torch.tensor(values)
        assert torch.equal(relative_position_index((wh, ww)), ref), key      # the port's host function
        assert torch.equal(sd[key], ref), key                                 # what state_dict() writes
        assert torch.equal(U.relpos_index(wh, ww), ref), key                  # the tests' own restatement
    assert not any("relative_position_index" in k for k, _ in net.named_buffers())   # nothing N x N is held


def test_index_of_both_window_orientations_differ():
    a, b = U.relpos_index(2, 3), U.relpos_index(3, 2)
    assert a.shape == b.shape and not torch.equal(a, b)
    assert int(a.max()) == 3 * 5 + 2 and int(a[1:, 1:].max()) == 3 * 5 - 1 and int(a[1:, 1:].min()) == 0


def test_a_state_dict_with_index_keys_loads_and_another_table_size_is_refused(tmp_path):
    from gaia_seg_amd.core.checkpoint import load_checkpoint
    kw = CASES[0]["kwargs"]                  # patch 16, window 2 x 3, a table per block
    src, dst = _build(kw), _build(kw)
    U.randomize_beit(src, seed=3)
    sd = src.state_dict()
    assert "blocks.0.attn.relative_position_index" in sd
    dst.load_state_dict(sd, strict=True)
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), k
    path = str(tmp_path / "beit.pth")
    torch.save(dict(state_dict=sd), path)
    dst = _build(kw)
    load_checkpoint(dst, path, strict=True)
    assert torch.equal(dst.blocks[2].attn.relative_position_bias_table, src.blocks[2].attn.relative_position_bias_table)
    # a 3 x 3 window's table (28 rows) into the 2 x 3 model (18 rows); pos_embed likewise
    other = _build(dict(kw, img_size=(48, 48)))
    assert tuple(other.blocks[0].attn.relative_position_bias_table.shape) == (28, 1)
    for load in (lambda m, s: m.load_state_dict(s), lambda m, s: (torch.save(dict(state_dict=s), path),
                                                                  load_checkpoint(m, path))):
        with pytest.raises(RuntimeError) as e:
            load(_build(kw), other.state_dict())
        assert "relative_position_bias_table" in str(e.value) and "28" in str(e.value) and "18" in str(e.value)
    kw_abs = CASES[2]["kwargs"]
    with pytest.raises(RuntimeError) as e:
        torch.save(dict(state_dict=_build(dict(kw_abs, img_size=(48, 48))).state_dict()), path)
        load_checkpoint(_build(kw_abs), path)
    assert "pos_embed" in str(e.value) and "10" in str(e.value) and "7" in str(e.value)


def test_init_rescales_the_residual_projections_by_depth():
    torch.manual_seed(0)
    net = _build(dict(img_size=(32, 48), embed_dim=128, depth=4, num_heads=2, out_indices=[0, 1, 2, 3],
                      use_rel_pos_bias=True, init_values=0.1, qkv_bias=True))
    w0, w3 = net.blocks[0].attn.proj.weight.detach(), net.blocks[3].attn.proj.weight.detach()
    assert w0.numel() == w3.numel() == 16384
    assert abs(float(w3.std() / w0.std()) - 0.5) <= 0.05          # sqrt(2 * 1) / sqrt(2 * 4), within 10 %
    f0, f3 = net.blocks[0].mlp.fc2.weight.detach(), net.blocks[3].mlp.fc2.weight.detach()
    assert abs(float(f3.std() / f0.std()) - 0.5) <= 0.05
    assert abs(float(net.blocks[0].attn.qkv.weight.std()) - 0.02) < 0.002    # truncated normal, std 0.02
    assert float(net.blocks[0].attn.qkv.weight.abs().max()) <= 2.0
    for m in net.modules():
        if isinstance(m, torch.nn.LayerNorm):
            assert bool((m.weight == 1).all()) and not bool(m.bias.any())
    assert not bool(net.blocks[1].mlp.fc1.bias.any()) and not bool(net.blocks[1].attn.proj.bias.any())
    assert not bool(net.blocks[1].attn.relative_position_bias_table.any()) and not bool(net.blocks[1].attn.q_bias.any())
    assert bool((net.blocks[1].gamma_1 == 0.1).all()) and bool(net.cls_token.any())
    assert not net.train().training                                # eval mode whatever is asked for


@pytest.mark.parametrize("key,kw", [
    ("hybrid_backbone", dict(hybrid_backbone=torch.nn.Identity())),
    ("num_heads", dict(embed_dim=128, num_heads=4)),               # head dimension 32
    ("patch_size", dict(patch_size=4)),
    ("out_indices", dict(out_indices=[0, 1, 2])),
    ("out_indices", dict(out_indices=[0, 1, 2, 2])),
    ("img_size", dict(img_size=(33 * 16, 64 * 16), use_rel_pos_bias=True)),   # a window past the kernel's cap
])
def test_refusals_name_the_key(key, kw):
    base = dict(img_size=(32, 48), embed_dim=128, depth=4, num_heads=2, out_indices=[0, 1, 2, 3])
    base.update(kw)
    with pytest.raises((NotImplementedError, ValueError), match=key):
        _build(base)


def test_the_in_tree_and_beit_large_windows_are_admitted():
    from gaia_seg_amd.models.backbones.beit import RelativePositionBias
    assert RelativePositionBias((32, 64), 12).relative_position_bias_table.shape == (8004, 12)
    assert RelativePositionBias((40, 40), 16).relative_position_bias_table.shape == (6244, 16)


def test_distiller_config_names_the_beit_b16_teacher():
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(os.path.join(os.path.dirname(HERE), "configs", "supernet",
                                       "upernet_elastic_vit_distiller_beit.py"))
    t = cfg.model.teacher_segmentor
    assert cfg.model.type == "DynamicDistiller" and t.backbone.type == "BEiT"
    bb = t.backbone
    assert (bb.embed_dim, bb.depth, bb.num_heads, bb.init_values, bb.qkv_bias) == (768, 12, 12, 0.1, True)
    assert bb.use_rel_pos_bias and not bb.use_abs_pos_emb and list(bb.out_indices) == [3, 5, 7, 11]
    assert tuple(bb.img_size) == tuple(cfg.crop_size)
    assert list(t.decode_head.in_channels) == [768] * 4
