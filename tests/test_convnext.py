"""DynamicConvNeXt without a GPU: constructor, state-dict names and shapes, arch manipulation, the 7x7
depthwise layout, the refusals, the host-side argument checks of every new C-ABI entry (they return
before any launch), FLOP known answers and the supernet config with its three anchors."""
import ctypes

import pytest
import torch

from gaia_seg_amd.hip import lib
import util_convnext as U

GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
P = 0x10000          # a 16-byte aligned, non-null address.  It is never dereferenced because every call that gets it is
                     # asserted to return a refusal code, and the library refuses before it launches
CONFIG = lib.REPO_ROOT + "/configs/supernet/upernet_convnext_t2b.py"


def tiny():
    from gaia_seg_amd.models import build_backbone
    return build_backbone(U.tiny_backbone_cfg())


# ---- the backbone ------------------------------------------------------------------------------------
def test_constructor_and_state_dict_names():
    from gaia_seg_amd.core.bricks import DynamicLayerNorm, DynamicLinear, GELU, is_hwio
    from gaia_seg_amd.models.builder import BACKBONES
    assert BACKBONES.get("DynamicConvNeXt") is not None
    m = tiny()
    sd = m.state_dict()
    dims, depths = U.TINY["dims"], U.TINY["depths"]
    want = {"stem.weight": (8, 3, 4, 4), "stem.bias": (8,), "ln1.weight": (8,), "ln1.bias": (8,)}
    for i in range(4):
        want["norm%d.weight" % i] = want["norm%d.bias" % i] = (dims[i],)
    for i in (1, 2, 3):
        want["ln%d.weight" % (i + 1)] = want["ln%d.bias" % (i + 1)] = (dims[i - 1],)
        want["ds%d_conv.weight" % i] = (dims[i], dims[i - 1], 2, 2)
        want["ds%d_conv.bias" % i] = (dims[i],)
    for i, (d, n) in enumerate(zip(dims, depths)):
        for j in range(n):
            p = "dynamic_convnext_block_%d.%d." % (i + 1, j)
            want.update({p + "dwconv.weight": (d, 1, 7, 7), p + "dwconv.bias": (d,), p + "ln1.weight": (d,),
                         p + "ln1.bias": (d,), p + "pwconv1.weight": (4 * d, d), p + "pwconv1.bias": (4 * d,),
                         p + "pwconv2.weight": (d, 4 * d), p + "pwconv2.bias": (d,), p + "gamma": (d,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    blk = m.dynamic_convnext_block_3[2]
    assert isinstance(blk.pwconv1, DynamicLinear) and isinstance(blk.norm, DynamicLayerNorm)
    assert isinstance(blk.act, GELU) and blk.norm.data_format == "channels_last" and blk.norm.eps == 1e-6
    assert m.stem_ln is m.ln1 and m.ds3_ln is m.ln4 and m.ln2.data_format == "channels_first"
    # physically the linear weight is HWIO [1][1][in][out_ld]
    assert tuple(blk.pwconv1.weight.shape) == (96, 24, 1, 1) and is_hwio(blk.pwconv1.weight)
    assert blk.pwconv1.weight._gs_phys_shape == (1, 1, 24, 96)
    # init: zero biases, unit norms, the layer scale at its init value, truncated normal weights
    assert float(blk.pwconv1.bias.abs().max()) == 0 and float(m.stem.bias.abs().max()) == 0
    assert bool((m.norm2.weight == 1).all()) and bool((m.ln3.bias == 0).all())
    assert torch.allclose(blk.gamma, torch.full((24,), 1e-6))
    w = m.dynamic_convnext_block_4[0].pwconv1.weight
    assert 0.015 < float(w.std()) < 0.025 and abs(float(w.mean())) < 0.002
    # a reference checkpoint's nn.Linear weight loads, and comes back 2-D
    ref = torch.nn.Linear(24, 96)
    blk.pwconv1.load_state_dict(ref.state_dict())
    assert torch.equal(blk.pwconv1.state_dict()["weight"], ref.weight) and is_hwio(blk.pwconv1.weight)
    assert float(blk.pwconv1.weight[5, 7, 0, 0]) == float(ref.weight[5, 7])


def test_no_layer_scale_and_norm_layer_names():
    from gaia_seg_amd.core.bricks import build_norm_layer
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(U.tiny_backbone_cfg(layer_scale_init_value=0))
    assert m.dynamic_convnext_block_1[0].gamma is None and not any(k.endswith("gamma") for k in m.state_dict())
    assert build_norm_layer(dict(type="DynLN", eps=1e-6, data_format="channels_first"), 8, postfix=3)[0] == "ln3"
    assert build_norm_layer(dict(type="LN"), 8)[0] == "ln"
    assert build_norm_layer(dict(type="BN"), 8, postfix=2)[0] == "bn2"
    assert build_norm_layer(dict(type="DynSyncBN", group_size=1), 8, postfix=1)[0] == "bn1"


def test_manipulate_body_reaches_every_child():
    m = tiny()
    meta = {"width": [4, 8, 12, 16], "depth": [1, 2, 2, 1]}      # a dict of lists (DL)
    m.manipulate_arch({"body": meta})
    assert m.body_state == meta
    convs = [m.stem, m.ds1_conv, m.ds2_conv, m.ds3_conv]
    for i, name in enumerate(m.blocks):
        stage = getattr(m, name)
        assert (stage.depth_state, stage.width_state) == (meta["depth"][i], meta["width"][i])
        assert convs[i].width_state == meta["width"][i]
        for blk in stage:                                         # inactive blocks included
            assert blk.width_state == meta["width"][i] and blk.dwconv.width_state == meta["width"][i]
            assert blk.pwconv1.width_state == 4 * meta["width"][i] and blk.pwconv2.width_state == meta["width"][i]
    active = {id(x) for x in m.active_modules()}
    assert id(m.dynamic_convnext_block_1[0]) in active and id(m.dynamic_convnext_block_1[1]) not in active
    assert id(m.dynamic_convnext_block_3[1]) in active and id(m.dynamic_convnext_block_3[2]) not in active
    assert {id(m.stem), id(m.ln1), id(m.ds3_conv), id(m.norm0), id(m.norm3)} <= active
    with pytest.raises(ValueError):
        m.manipulate_arch({"body": {"width": [4, 8, 12, 16], "depth": [1, 2, 4, 1]}})
    with pytest.raises(KeyError):
        m.manipulate_arch({"stem": {"width": 4}})


def test_depthwise_7x7_layout_and_the_groupings_still_refused():
    from gaia_seg_amd.core.bricks import DynamicConv2d, is_hwio
    c = DynamicConv2d(20, 20, 7, padding=3, groups=20)
    assert c.depthwise and tuple(c.weight.shape) == (20, 1, 7, 7)
    assert c.weight.stride() == (1, 20, 140, 20) and is_hwio(c.weight)      # [7][7][1][C_ld]
    assert c.weight._gs_phys_shape == (7, 7, 1, 20) and tuple(c.bias.shape) == (20,)
    c.load_state_dict({"weight": torch.arange(980.0).view(20, 1, 7, 7), "bias": torch.zeros(20)})
    assert is_hwio(c.weight) and float(c.weight[7, 0, 5, 2]) == 7 * 49 + 5 * 7 + 2
    for kw in (dict(kernel_size=5, groups=8), dict(kernel_size=7, groups=8, stride=2), dict(kernel_size=7, groups=4),
               dict(kernel_size=(7, 3), groups=8)):
        with pytest.raises(NotImplementedError) as e:
            DynamicConv2d(8, 8, **kw)
        assert str(e.value) == "DynConv2d: groups != 1 is not used on the supernet hot path"


def test_drop_path_is_refused():
    from gaia_seg_amd.models import build_backbone
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        build_backbone(U.tiny_backbone_cfg(drop_path_rate=0.1))


# ---- host-side checks of the C-ABI ---------------------------------------------------------------------
def test_binding_and_header(hip_lib):
    assert lib.ABI_VERSION >= 18 and ctypes.sizeof(lib.LayerNormDesc) == 24
    header = open(lib.REPO_ROOT + "/include/gaiaseg_hip.h").read()
    for name in ("gs_layernorm_forward", "gs_layernorm_backward", "gs_layernorm_workspace_bytes", "gs_gelu_forward",
                 "gs_gelu_backward", "gs_layer_scale_add_forward", "gs_layer_scale_backward",
                 "gs_layer_scale_workspace_bytes"):
        assert name + "(" in header and name in lib.PROTOTYPES and hasattr(hip_lib, name)


def dw_calls(L, d, ws_bytes=1 << 30):
    db = ctypes.byref(d)
    return (L.gs_dwconv2d_forward(db, P, P, None, P, None), L.gs_dwconv2d_dgrad(db, P, P, P, 0, None),
            L.gs_dwconv2d_wgrad(db, P, P, P, P, ws_bytes, None))


@pytest.mark.parametrize("change,code", [
    (dict(C=6), GS_E_ALIGN), (dict(ldx=10), GS_E_ALIGN), (dict(C_ld=10), GS_E_ALIGN),
    (dict(KW=3), GS_E_BADARG), (dict(KH=3), GS_E_BADARG), (dict(KH=5, KW=5), GS_E_BADARG), (dict(KH=9, KW=9), GS_E_BADARG),
    (dict(stride=2), GS_E_BADARG), (dict(dil=0), GS_E_BADARG), (dict(pad=-1), GS_E_BADARG),
    (dict(ldy=4), GS_E_BADARG), (dict(pad=0, dil=2), GS_E_BADARG),          # Ho = 9 - 12 < 1
])
def test_dwconv7_bad_descriptors_are_refused_before_any_launch(hip_lib, change, code):
    d = lib.dwconv_desc(2, 9, 11, 8, pad=3, k=7)
    for k, v in change.items():
        setattr(d, k, v)
    assert dw_calls(hip_lib, d) == (code, code, code)
    assert hip_lib.gs_dwconv2d_workspace_bytes(ctypes.byref(d)) == 0


def test_dwconv7_workspace_query(hip_lib):
    q = hip_lib.gs_dwconv2d_workspace_bytes
    prev, seen = 0, set()
    for n, h, w in [(1, 1, 1), (1, 3, 5), (2, 9, 11), (1, 16, 16), (1, 16, 17), (2, 13, 17), (2, 16, 64), (2, 64, 128),
                    (2, 128, 256), (8, 128, 256)]:
        need = q(ctypes.byref(lib.dwconv_desc(n, h, w, 8, pad=3, k=7)))
        assert need >= prev and need >= 49 * 8 * 4 and need % 16 == 0, (n, h, w, need)
        prev = need
        seen.add(need)
    assert len(seen) > 4
    d = lib.dwconv_desc(2, 13, 17, 8, pad=3, k=7)            # 442 output pixels: two runs of 256
    assert q(ctypes.byref(d)) == 2 * 49 * 8 * 4
    assert hip_lib.gs_dwconv2d_wgrad(ctypes.byref(d), P, P, P, P, 2 * 49 * 8 * 4 - 1, None) == GS_E_WORKSPACE
    assert hip_lib.gs_dwconv2d_wgrad(ctypes.byref(d), P, P, P, P + 4, 1 << 20, None) == GS_E_ALIGN
    assert hip_lib.gs_dwconv2d_forward(ctypes.byref(d), P, None, None, P, None) == GS_E_NULL
    # the 3x3 query is what it was: one [9][C] partial per run
    assert q(ctypes.byref(lib.dwconv_desc(2, 13, 17, 8, pad=1))) == 2 * 9 * 8 * 4


def ln_fwd(L, d, x=P, w=P, b=P, y=P, mean=P, rstd=P):
    return L.gs_layernorm_forward(ctypes.byref(d) if d is not None else None, x, w, b, y, mean, rstd, None)


def ln_bwd(L, d, x=P, y=P, w=P, mean=P, rstd=P, dx=P, dw=P, db=P, ws=P, ws_bytes=1 << 30):
    return L.gs_layernorm_backward(ctypes.byref(d) if d is not None else None, x, y, w, mean, rstd, dx, dw, db,
                                   0, ws, ws_bytes, None)


def test_layernorm_argument_checks(hip_lib):
    # (one entry per call, each with exactly one thing wrong and its refusal asserted: a call with nothing
    # wrong would launch on P)
    q = hip_lib.gs_layernorm_workspace_bytes
    for change, code in [(dict(C=6), GS_E_ALIGN), (dict(ldx=10), GS_E_ALIGN), (dict(ldy=14), GS_E_ALIGN),
                         (dict(rows=0), GS_E_BADARG), (dict(C=0), GS_E_BADARG), (dict(ldx=4), GS_E_BADARG),
                         (dict(ldy=4), GS_E_BADARG), (dict(eps=0.0), GS_E_BADARG), (dict(eps=-1.0), GS_E_BADARG)]:
        d = lib.layernorm_desc(105, 8, 1e-6, ldx=16, ldy=12)
        for k, v in change.items():
            setattr(d, k, v)
        assert (ln_fwd(hip_lib, d), ln_bwd(hip_lib, d)) == (code, code), change
        assert q(ctypes.byref(d)) == 0
    d = lib.layernorm_desc(105, 8, 1e-6, ldx=16, ldy=12)
    assert (ln_fwd(hip_lib, None), ln_bwd(hip_lib, None)) == (GS_E_NULL, GS_E_NULL) and q(None) == 0
    for name in ("x", "w", "y", "mean", "rstd"):
        assert (ln_fwd(hip_lib, d, **{name: None}), ln_bwd(hip_lib, d, **{name: None})) == (GS_E_NULL, GS_E_NULL), name
    assert ln_fwd(hip_lib, d, b=None) == GS_E_NULL
    for name in ("dx", "dw", "db", "ws"):
        assert ln_bwd(hip_lib, d, **{name: None}) == GS_E_NULL, name
    for name in ("x", "w", "y"):
        assert (ln_fwd(hip_lib, d, **{name: P + 4}), ln_bwd(hip_lib, d, **{name: P + 4})) == (GS_E_ALIGN, GS_E_ALIGN), name
    assert ln_fwd(hip_lib, d, b=P + 8) == GS_E_ALIGN
    for name in ("dx", "dw", "db", "ws"):
        assert ln_bwd(hip_lib, d, **{name: P + 4}) == GS_E_ALIGN, name
    need = q(ctypes.byref(d))
    assert need == 2 * 8 * 4                                  # one run of up to 256 rows, [2][C]
    assert ln_bwd(hip_lib, d, ws_bytes=need - 1) == GS_E_WORKSPACE
    big = lib.layernorm_desc(257, 1024, 1e-6)
    assert q(ctypes.byref(big)) == 2 * 2 * 1024 * 4


def test_gelu_and_layer_scale_argument_checks(hip_lib):
    L = hip_lib
    fwd = lambda x=P, y=P, rows=105, c=8, ldx=8, ldy=12: L.gs_gelu_forward(x, y, rows, c, ldx, ldy, None)   # noqa: E731
    bwd = lambda x=P, dy=P, dx=P, rows=105, c=8, ldx=8, lddy=12, lddx=16: L.gs_gelu_backward(          # noqa: E731
        x, dy, dx, rows, c, ldx, lddy, lddx, None)
    assert fwd(x=None) == fwd(y=None) == GS_E_NULL and fwd(x=P + 4) == fwd(y=P + 8) == GS_E_ALIGN
    assert fwd(rows=0) == fwd(c=0) == fwd(ldx=4) == fwd(c=16, ldy=12) == GS_E_BADARG
    assert fwd(c=6) == fwd(ldx=10) == fwd(ldy=14) == GS_E_ALIGN
    assert bwd(x=None) == bwd(dy=None) == bwd(dx=None) == GS_E_NULL
    assert bwd(x=P + 4) == bwd(dy=P + 4) == bwd(dx=P + 4) == bwd(c=6) == bwd(lddx=18) == GS_E_ALIGN
    assert bwd(rows=-1) == bwd(lddy=4) == bwd(lddx=4) == GS_E_BADARG

    def ls_fwd(i=P, z=P, g=P, o=P, rows=105, c=8, ldi=8, ldz=12, ldo=16):
        return L.gs_layer_scale_add_forward(i, z, g, o, rows, c, ldi, ldz, ldo, None)

    def ls_bwd(do=P, z=P, g=P, dz=P, dg=P, rows=105, c=8, lddo=8, ldz=12, lddz=16, ws=P, ws_bytes=1 << 20):
        return L.gs_layer_scale_backward(do, z, g, dz, dg, rows, c, lddo, ldz, lddz, ws, ws_bytes, None)

    for name in ("i", "z", "g", "o"):
        assert ls_fwd(**{name: None}) == GS_E_NULL and ls_fwd(**{name: P + 4}) == GS_E_ALIGN, name
    assert ls_fwd(rows=0) == ls_fwd(c=0) == ls_fwd(ldi=4) == ls_fwd(ldo=4) == GS_E_BADARG
    assert ls_fwd(c=6) == ls_fwd(ldz=14) == GS_E_ALIGN
    for name in ("do", "z", "g", "dz", "dg", "ws"):
        assert ls_bwd(**{name: None}) == GS_E_NULL and ls_bwd(**{name: P + 4}) == GS_E_ALIGN, name
    assert ls_bwd(rows=0) == ls_bwd(lddo=4) == ls_bwd(lddz=4) == GS_E_BADARG and ls_bwd(c=6) == GS_E_ALIGN
    q = L.gs_layer_scale_workspace_bytes
    assert q(105, 8) == 8 * 4 and q(257, 8) == 2 * 8 * 4 and q(0, 8) == q(105, 6) == 0
    assert ls_bwd(ws_bytes=q(105, 8) - 1) == GS_E_WORKSPACE


# ---- FLOPs, config, anchors ---------------------------------------------------------------------------
def test_flops_of_one_tiny_block_by_hand():
    from gaia_seg_amd.core.flops import backbone_flops
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(U.tiny_backbone_cfg())
    m.manipulate_arch({"body": {"width": [4, 8, 12, 16], "depth": [1, 1, 1, 1]}})
    total, params, k3, feats = backbone_flops(m, 32, 64)
    assert feats == [(4, 8, 16), (8, 4, 8), (12, 2, 4), (16, 1, 2)] and k3 == 0
    want = 2 * 8 * 16 * 4 * 3 * 16                                # stem: 4x4 conv, 3 -> 4 channels, 8x16 out
    want_p = 3 * 4 * 16 + 4 + 2 * 4
    for (c, h, w), cn in zip(feats, (8, 12, 16, None)):
        # one block: depthwise 7x7 (2*49*C per pixel), linear C -> 4C and 4C -> C (2*4C*C per pixel each)
        want += h * w * (2 * 49 * c + 2 * 4 * c * c + 2 * 4 * c * c)
        want_p += (49 * c + c) + 2 * c + (4 * c * c + 4 * c) + (4 * c * c + c) + c + 2 * c      # ... gamma, norm{i}
        if cn is not None:                                        # downsample: LN, 2x2 stride-2 conv C -> Cn
            want += 2 * (h // 2) * (w // 2) * cn * c * 4
            want_p += 2 * c + cn * c * 4 + cn
    assert total == want and params == want_p
    assert params == U.convnext_param_count([4, 8, 12, 16], [1, 1, 1, 1])


def closed_form_params(dims, depths):
    """torchvision-style ConvNeXt without its classifier and final norm, plus the four output norms of
    the segmentation backbone"""
    stem = 3 * dims[0] * 4 * 4 + dims[0] + 2 * dims[0]
    down = sum(2 * a + a * b * 2 * 2 + b for a, b in zip(dims, dims[1:]))
    block = lambda d: 7 * 7 * d + d + 2 * d + d * 4 * d + 4 * d + 4 * d * d + d + d      # noqa: E731
    return stem + down + sum(n * block(d) for d, n in zip(dims, depths)) + sum(2 * d for d in dims)


def test_config_loads_and_its_anchors_are_convnext_t_s_b():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.flops import model_flops
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.models import build_backbone, build_segmentor
    cfg = Config.fromfile(CONFIG)
    assert cfg.model.backbone.dims == [128, 256, 512, 1024] and cfg.model.backbone.depths == [3, 3, 27, 3]
    assert cfg.model.decode_head.type == "DynamicUPerHead" and cfg.model.decode_head.in_channels == [128, 256, 512, 1024]
    assert cfg.model.auxiliary_head.in_index == 2 and cfg.optimizer.type == "SGD"
    anchors = {m["name"]: m for m in build_model_sampler(cfg.val_sampler).traverse()}
    assert anchors["ConvNeXt-T"]["arch.backbone.body.width"] == [96, 192, 384, 768]
    assert anchors["ConvNeXt-T"]["arch.backbone.body.depth"] == [3, 3, 9, 3]
    assert anchors["ConvNeXt-S"]["arch.backbone.body.depth"] == [3, 3, 27, 3]
    assert anchors["ConvNeXt-B"]["arch.backbone.body.width"] == [128, 256, 512, 1024]
    sampler = build_model_sampler(cfg.train_sampler)
    for _ in range(40):
        meta = sampler.sample()
        w, d = meta["arch.backbone.body.width"], meta["arch.backbone.body.depth"]
        assert w[0] in (96, 112, 128) and w == [w[0], 2 * w[0], 4 * w[0], 8 * w[0]]
        assert d[2] in (9, 18, 27) and d[:2] + d[3:] == [3, 3, 3]
    model = build_segmentor(cfg.model)
    for name, meta in anchors.items():
        model.manipulate_arch(fold_dict(meta)["arch"])
        got = model_flops(model, 512, 1024)["backbone_params"]
        assert got == closed_form_params(meta["arch.backbone.body.width"], meta["arch.backbone.body.depth"]), name
    # a fixed-size ConvNeXt-T built directly has exactly the closed form's parameters
    t = closed_form_params([96, 192, 384, 768], [3, 3, 9, 3])
    fixed = build_backbone(dict(type="DynamicConvNeXt", depths=[3, 3, 9, 3], dims=[96, 192, 384, 768]))
    assert sum(p.numel() for p in fixed.parameters()) == t


def test_checkpoint_round_trip_keeps_names_shapes_and_layout(tmp_path):
    from gaia_seg_amd.core.bricks import is_hwio
    from gaia_seg_amd.core.checkpoint import load_checkpoint, save_checkpoint
    a, b = tiny(), tiny()
    U.randomize_convnext(a, 3)
    path = str(tmp_path / "convnext.pth")
    save_checkpoint(a, path, meta=dict(note="tiny"))
    ck = torch.load(path, map_location="cpu")
    assert tuple(ck["state_dict"]["dynamic_convnext_block_2.1.pwconv1.weight"].shape) == (64, 16)
    assert ck["state_dict"]["dynamic_convnext_block_2.1.dwconv.weight"].is_contiguous()
    load_checkpoint(b, path, strict=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert is_hwio(b.dynamic_convnext_block_2[1].pwconv1.weight) and is_hwio(b.dynamic_convnext_block_2[1].dwconv.weight)
