"""DynamicConvNeXtV2 without a GPU: the float64 restatement of tests/util_convnextv2.py against transformers'
ConvNextV2Backbone / ConvNextV2GRN (third-party code, installed on the CPU machine), strict loading of a
transformers state dict, names, shapes, init, arch manipulation, refusals, the config with its anchors, FLOP and
parameter counts against counts taken from the transformers model, and the host-side argument checks of the
gs_gelu_grn_* entries (they return before any launch)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gaia_seg_amd.hip import lib
import util_convnextv2 as U

GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
P = 0x10000          # a 16-byte aligned, non-null address.  It is never dereferenced because every call that gets it is
                     # asserted to return a refusal code, and the library refuses before it launches
CONFIG = lib.REPO_ROOT + "/configs/supernet/upernet_convnextv2_n2b_adamw.py"


def tiny(**kw):
    from gaia_seg_amd.models import build_backbone
    return build_backbone(U.tiny_backbone_cfg(**kw))


def hf_model(arch):
    transformers = pytest.importorskip("transformers")
    return transformers.ConvNextV2Backbone(U.hf_config(arch)).double().eval()


def image(h=64, w=96, seed=1):
    return torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def randomized_state_dict(seed=0):
    m = tiny()
    U.randomize_convnextv2(m, seed)
    return {k: v.double() for k, v in m.state_dict().items()}


# ---- against transformers --------------------------------------------------------------------------------
def test_the_grn_formula_equals_transformers_grn_of_gelu_in_float64():
    pytest.importorskip("transformers")
    from transformers.models.convnextv2.modeling_convnextv2 import ConvNextV2GRN
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 7, 24, generator=g, dtype=torch.float64)
    x[1] = 0                                                     # a zero sample: Nx = 0 / eps
    x[..., 3] = 0                                                # a zero channel
    grn = ConvNextV2GRN(24).double()
    with torch.no_grad():
        grn.weight.copy_(torch.randn(1, 1, 1, 24, generator=g))
        grn.bias.copy_(torch.randn(1, 1, 1, 24, generator=g))
    want = grn(F.gelu(x))
    got = U.grn_formula(F.gelu(x), grn.weight[0, 0, 0], grn.bias[0, 0, 0])
    assert float((got - want).abs().max()) <= 1e-12
    # and the operator reference of the GPU tests, on its [N, P, C] rows
    dy = torch.randn(3, 35, 24, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    grn(F.gelu(xr)).backward(dy.view(3, 5, 7, 24))
    y, G, dx, dw, db = U.gelu_grn_ref(x.view(3, 35, 24), grn.weight[0, 0, 0].detach(), grn.bias[0, 0, 0].detach(), dy)
    assert float((y - want.view(3, 35, 24)).abs().max()) <= 1e-12
    assert float((dx - xr.grad.view(3, 35, 24)).abs().max()) <= 1e-12 and bool(torch.isfinite(dx).all())
    assert float((dw - grn.weight.grad[0, 0, 0]).abs().max()) <= 1e-10
    assert float((db - grn.bias.grad[0, 0, 0]).abs().max()) <= 1e-10
    assert float(G[1].abs().max()) == 0 and float(G[:, 3].abs().max()) == 0


def test_restatement_equals_transformers_backbone_in_float64():
    a = U.SUBNETS["max"]
    hf = hf_model(a)
    sd = randomized_state_dict()
    hf.load_state_dict(sd, strict=True)
    img = image()
    with torch.no_grad():
        want = hf(img).feature_maps
        got = U.convnextv2_ref(sd, img, a["width"], a["depth"])
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.shape == w.shape and float((g - w).abs().max()) <= 1e-9 * max(1.0, float(w.abs().max()))


def test_a_subnet_equals_transformers_of_exactly_its_sizes():
    a = U.SUBNETS["sub"]
    hf = hf_model(a)
    sd = randomized_state_dict()
    hf.load_state_dict(U.slice_state_dict(sd, {k: v.shape for k, v in hf.state_dict().items()}), strict=True)
    img = image()
    with torch.no_grad():
        want = hf(img).feature_maps
        got = U.convnextv2_ref(sd, img, a["width"], a["depth"])
    for g, w in zip(got, want):
        assert g.shape == w.shape and float((g - w).abs().max()) <= 1e-9 * max(1.0, float(w.abs().max()))


def test_a_transformers_state_dict_loads_strictly_and_round_trips(tmp_path):
    from gaia_seg_amd.core.bricks import is_hwio
    from gaia_seg_amd.core.checkpoint import load_checkpoint, save_checkpoint
    hf = hf_model(U.SUBNETS["max"]).float()
    with torch.no_grad():
        for p in hf.parameters():
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    want = hf.state_dict()
    m = tiny()
    assert list(m.state_dict()) == list(want)                    # the same names in the same order
    m.load_state_dict(want, strict=True)
    got = m.state_dict()
    assert all(got[k].shape == want[k].shape and torch.equal(got[k], want[k]) for k in want)
    blk = m.encoder.stages[2].layers[1]
    assert is_hwio(blk.pwconv1.weight) and is_hwio(blk.dwconv.weight)
    assert float(blk.pwconv1.weight[5, 7, 0, 0]) == float(want["encoder.stages.2.layers.1.pwconv1.weight"][5, 7])
    hf.load_state_dict(got, strict=True)                         # and back
    path = str(tmp_path / "convnextv2.pth")
    save_checkpoint(m, path, meta=dict(note="tiny"))
    b = tiny()
    load_checkpoint(b, path, strict=True)
    assert all(torch.equal(v, want[k]) for k, v in b.state_dict().items())


# ---- the backbone ------------------------------------------------------------------------------------
def test_registry_names_shapes_and_init():
    from gaia_seg_amd.core.bricks import DynamicGRN, DynamicLayerNorm, DynamicLinear
    from gaia_seg_amd.models.backbones import DynamicConvNeXt
    from gaia_seg_amd.models.builder import BACKBONES
    assert BACKBONES.get("DynamicConvNeXtV2") is not None
    m = tiny()
    dims, depths = U.TINY["dims"], U.TINY["depths"]
    want = {"embeddings.patch_embeddings.weight": (8, 3, 4, 4), "embeddings.patch_embeddings.bias": (8,),
            "embeddings.layernorm.weight": (8,), "embeddings.layernorm.bias": (8,)}
    for i, (d, n) in enumerate(zip(dims, depths)):
        s = "encoder.stages.%d." % i
        want["hidden_states_norms.stage%d.weight" % (i + 1)] = want["hidden_states_norms.stage%d.bias" % (i + 1)] = (d,)
        if i:
            want[s + "downsampling_layer.0.weight"] = want[s + "downsampling_layer.0.bias"] = (dims[i - 1],)
            want[s + "downsampling_layer.1.weight"] = (d, dims[i - 1], 2, 2)
            want[s + "downsampling_layer.1.bias"] = (d,)
        for j in range(n):
            p = s + "layers.%d." % j
            want.update({p + "dwconv.weight": (d, 1, 7, 7), p + "dwconv.bias": (d,), p + "layernorm.weight": (d,),
                         p + "layernorm.bias": (d,), p + "pwconv1.weight": (4 * d, d), p + "pwconv1.bias": (4 * d,),
                         p + "grn.weight": (1, 1, 1, 4 * d), p + "grn.bias": (1, 1, 1, 4 * d),
                         p + "pwconv2.weight": (d, 4 * d), p + "pwconv2.bias": (d,)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert not any("gamma" in k for k in want) and not list(m.encoder.stages[0].downsampling_layer)
    assert sum(p.numel() for p in m.parameters()) == U.convnextv2_param_count(dims, depths)
    blk = m.encoder.stages[2].layers[2]
    assert isinstance(blk.grn, DynamicGRN) and isinstance(blk.pwconv1, DynamicLinear)
    assert isinstance(blk.layernorm, DynamicLayerNorm) and blk.layernorm.eps == 1e-6 and blk.grn.eps == 1e-6
    assert m.stem is m.embeddings.patch_embeddings and m.ds3_ln is m.encoder.stages[3].downsampling_layer[0]
    assert m.out_norm(2) is m.hidden_states_norms["stage3"] and m.out_norm(2).data_format == "channels_first"
    # init: zero GRN, zero biases, unit norms, truncated normal weights
    assert all(float(b.grn.weight.abs().max()) == 0 and float(b.grn.bias.abs().max()) == 0
               for s in m.encoder.stages for b in s.layers)
    assert float(blk.pwconv1.bias.abs().max()) == 0 and float(m.stem.bias.abs().max()) == 0
    assert bool((m.out_norm(1).weight == 1).all()) and bool((m.ds2_ln.bias == 0).all())
    w = m.encoder.stages[3].layers[0].pwconv1.weight
    assert 0.015 < float(w.std()) < 0.025 and abs(float(w.mean())) < 0.002
    # the V1 class keeps its own names
    v1 = DynamicConvNeXt(depths=[1, 1, 1, 1], dims=[4, 8, 12, 16])
    assert "stem.weight" in v1.state_dict() and "dynamic_convnext_block_1.0.gamma" in v1.state_dict()
    assert not any("grn" in k for k in v1.state_dict())


def test_manipulate_body_reaches_every_child_and_active_modules():
    m = tiny()
    assert m.full_arch_meta() == {"body": {"width": [8, 16, 24, 32], "depth": [2, 2, 3, 2]}}
    meta = {"width": [4, 8, 12, 16], "depth": [1, 2, 2, 1]}
    m.manipulate_arch({"body": meta})
    assert m.body_state == meta
    convs = [m.stem, m.ds1_conv, m.ds2_conv, m.ds3_conv]
    for i in range(4):
        stage = m.stage(i)
        assert (stage.depth_state, stage.width_state) == (meta["depth"][i], meta["width"][i])
        assert convs[i].width_state == meta["width"][i]
        for blk in stage:                                         # inactive blocks included
            assert blk.width_state == meta["width"][i] and blk.dwconv.width_state == meta["width"][i]
            assert blk.pwconv1.width_state == 4 * meta["width"][i] and blk.pwconv2.width_state == meta["width"][i]
    active = {id(x) for x in m.active_modules()}
    assert id(m.stage(0)[0]) in active and id(m.stage(0)[1]) not in active
    assert id(m.stage(2)[1]) in active and id(m.stage(2)[2]) not in active
    assert {id(m.stem), id(m.stem_ln), id(m.ds3_conv), id(m.out_norm(0)), id(m.out_norm(3))} <= active
    late = {id(p) for p in m.late_gradient_parameters()}
    assert id(m.stem.weight) in late and id(m.stage(0)[1].grn.weight) in late and id(m.ds1_conv.weight) not in late
    only = tiny(out_indices=[1, 3])
    assert id(only.out_norm(0)) not in {id(x) for x in only.active_modules()}
    with pytest.raises(ValueError):
        m.manipulate_arch({"body": {"width": [4, 8, 12, 16], "depth": [1, 2, 4, 1]}})
    with pytest.raises(KeyError):
        m.manipulate_arch({"stem": {"width": 4}})


def test_refusals():
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        tiny(drop_path_rate=0.1)
    with pytest.raises(AssertionError):
        tiny(depths=[2, 2, 2])
    with pytest.raises(TypeError):
        tiny(layer_scale_init_value=1e-6)                        # V2 has no layer scale


# ---- host-side checks of the C-ABI ---------------------------------------------------------------------
def test_binding_and_header(hip_lib):
    assert lib.ABI_VERSION >= 26 and hip_lib.gs_abi_version() == lib.ABI_VERSION
    assert ctypes.sizeof(lib.GeluGrnDesc) == 32
    header = open(lib.REPO_ROOT + "/include/gaiaseg_hip.h").read()
    for name in ("gs_gelu_grn_workspace_bytes", "gs_gelu_grn_forward", "gs_gelu_grn_backward"):
        assert name + "(" in header and name in lib.PROTOTYPES and hasattr(hip_lib, name)
    assert "gs_gelu_grn_desc" in header


def grn_fwd(L, d, x=P, w=P, b=P, y=P, G=P, ws=P, ws_bytes=1 << 30):
    return L.gs_gelu_grn_forward(ctypes.byref(d) if d is not None else None, x, w, b, y, G, ws, ws_bytes, None)


def grn_bwd(L, d, x=P, y=P, w=P, G=P, dx=P, dw=P, db=P, ws=P, ws_bytes=1 << 30):
    return L.gs_gelu_grn_backward(ctypes.byref(d) if d is not None else None, x, y, w, G, dx, dw, db, ws, ws_bytes,
                                  None)


def grn_calls(L, d, **kw):
    """Both entries under a fault that both see (an argument of one entry alone goes to grn_fwd / grn_bwd: the
    other entry, with nothing wrong, would launch on P)."""
    return grn_fwd(L, d, **kw), grn_bwd(L, d, **kw)


def test_gelu_grn_argument_checks(hip_lib):
    q = hip_lib.gs_gelu_grn_workspace_bytes
    mk = lambda: lib.gelu_grn_desc(3, 35, 8, 1e-6, ldx=16, ldy=12, lddy=12, lddx=16)    # noqa: E731
    for change, code in [(dict(C=6), GS_E_ALIGN), (dict(ldx=10), GS_E_ALIGN), (dict(ldy=14), GS_E_ALIGN),
                         (dict(lddy=14), GS_E_ALIGN), (dict(lddx=18), GS_E_ALIGN),
                         (dict(N=0), GS_E_BADARG), (dict(P=0), GS_E_BADARG), (dict(C=0), GS_E_BADARG),
                         (dict(N=-1), GS_E_BADARG), (dict(N=65536), GS_E_BADARG),
                         (dict(ldx=4), GS_E_BADARG), (dict(ldy=4), GS_E_BADARG), (dict(lddy=4), GS_E_BADARG),
                         (dict(lddx=4), GS_E_BADARG), (dict(eps=0.0), GS_E_BADARG), (dict(eps=-1.0), GS_E_BADARG)]:
        d = mk()
        for k, v in change.items():
            setattr(d, k, v)
        assert grn_calls(hip_lib, d) == (code, code), change
        assert q(ctypes.byref(d)) == 0
    d = mk()
    assert grn_calls(hip_lib, None) == (GS_E_NULL, GS_E_NULL) and q(None) == 0
    for name in ("x", "w", "y", "G", "ws"):
        assert grn_calls(hip_lib, d, **{name: None}) == (GS_E_NULL, GS_E_NULL), name
        assert grn_calls(hip_lib, d, **{name: P + 4}) == (GS_E_ALIGN, GS_E_ALIGN), name
    assert grn_fwd(hip_lib, d, b=None) == GS_E_NULL and grn_fwd(hip_lib, d, b=P + 8) == GS_E_ALIGN
    for name in ("dx", "dw", "db"):
        assert grn_bwd(hip_lib, d, **{name: None}) == GS_E_NULL, name
        assert grn_bwd(hip_lib, d, **{name: P + 4}) == GS_E_ALIGN, name
    need = q(ctypes.byref(d))
    assert need == 3 * 8 * (2 * 1 + 4) * 4                       # one run per sample: [2][C], and [4][C] per sample
    assert grn_calls(hip_lib, d, ws_bytes=need - 1) == (GS_E_WORKSPACE, GS_E_WORKSPACE)
    # the runs are cut per sample: 576 pixels are 3 runs of each of the 3 samples, not ceil(1728 / 256) = 7
    assert q(ctypes.byref(lib.gelu_grn_desc(3, 576, 96))) == 3 * 96 * (2 * 3 + 4) * 4


def test_the_tape_op_checks_its_operands():
    from gaia_seg_amd.hip import ops

    class X:                                                     # what _active_width reads of an activation
        C = 12

    with pytest.raises(ValueError, match="at most 8"):
        ops._active_width(X, torch.zeros(1, 1, 1, 8), "gelu_grn")
    X.C = 6
    with pytest.raises(ValueError, match="multiple of 4"):
        ops._active_width(X, torch.zeros(1, 1, 1, 8), "gelu_grn")
    X.C = 8
    assert ops._active_width(X, torch.zeros(1, 1, 1, 8), "gelu_grn") == 8
    assert ops._active_width(X, torch.zeros(8), "layernorm") == 8


# ---- FLOPs, config, anchors ---------------------------------------------------------------------------
def hf_counts(arch, h, w):
    """(multiply-add FLOPs of the convs and linears, parameters) counted on the transformers model itself"""
    transformers = pytest.importorskip("transformers")
    hf = transformers.ConvNextV2Backbone(U.hf_config(arch)).eval()
    flops = [0.0]

    def hook(mod, inp, out):
        per_out = mod.in_features if isinstance(mod, torch.nn.Linear) else \
            mod.in_channels // mod.groups * mod.kernel_size[0] * mod.kernel_size[1]
        flops[0] += 2.0 * out.numel() * per_out

    for mod in hf.modules():
        if isinstance(mod, (torch.nn.Linear, torch.nn.Conv2d)):
            mod.register_forward_hook(hook)
    with torch.no_grad():
        hf(torch.zeros(1, 3, h, w))
    return flops[0], sum(p.numel() for p in hf.parameters())


def test_flops_and_parameters_of_the_tiny_subnets_against_transformers():
    from gaia_seg_amd.core.flops import backbone_flops
    m = tiny()
    for name, a in U.SUBNETS.items():
        m.manipulate_arch({"body": {"width": a["width"], "depth": a["depth"]}})
        total, params, k3, feats = backbone_flops(m, 64, 96)
        assert (total, params) == hf_counts(a, 64, 96), name
        assert params == U.convnextv2_param_count(a["width"], a["depth"]) and k3 == 0
        assert feats == [(c, 16 >> i, 24 >> i) for i, c in enumerate(a["width"])]


def test_config_builds_and_its_anchors():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.flops import model_flops
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    assert cfg.model.backbone.type == "DynamicConvNeXtV2"
    assert cfg.model.backbone.dims == [128, 256, 512, 1024] and cfg.model.backbone.depths == [3, 3, 27, 3]
    assert cfg.model.decode_head.type == "DynamicUPerHead" and cfg.model.decode_head.in_channels == [128, 256, 512, 1024]
    assert cfg.optimizer.type == "AdamW" and cfg.optimizer.weight_decay == 0.05
    assert cfg.optimizer.paramwise_cfg.norm_decay_mult == 0
    assert dict(cfg.optimizer.paramwise_cfg.custom_keys["grn"]) == dict(decay_mult=0.)
    anchors = [m for m in build_model_sampler(cfg.val_sampler).traverse()]
    assert [m["name"] for m in anchors] == ["V2-Nano", "V2-Tiny", "V2-Base"]
    assert anchors[0]["arch.backbone.body.width"] == [80, 160, 320, 640]
    assert anchors[0]["arch.backbone.body.depth"] == [2, 2, 8, 2]
    assert anchors[1]["arch.backbone.body.width"] == [96, 192, 384, 768]
    assert anchors[1]["arch.backbone.body.depth"] == [3, 3, 9, 3]
    sampler = build_model_sampler(cfg.train_sampler)
    for _ in range(40):
        meta = sampler.sample()
        w, d = meta["arch.backbone.body.width"], meta["arch.backbone.body.depth"]
        assert w[0] in (80, 96, 112, 128) and w == [w[0], 2 * w[0], 4 * w[0], 8 * w[0]]
        assert d in ([2, 2, 8, 2], [3, 3, 9, 3], [3, 3, 18, 3], [3, 3, 27, 3])
    model = build_segmentor(cfg.model)
    # the MAX anchor is the whole supernet
    assert fold_dict(anchors[2])["arch"]["backbone"] == model.backbone.full_arch_meta()
    for meta in anchors:
        model.manipulate_arch(fold_dict(meta)["arch"])
        got = model_flops(model, 64, 128)
        a = dict(width=meta["arch.backbone.body.width"], depth=meta["arch.backbone.body.depth"])
        flops, params = hf_counts(a, 64, 128)
        assert got["backbone_params"] == params == U.convnextv2_param_count(a["width"], a["depth"]), meta["name"]
        assert got["backbone"] == flops, meta["name"]
