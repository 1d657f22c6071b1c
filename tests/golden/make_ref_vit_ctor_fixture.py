"""Generates tests/golden/ref_vit_ctors.json by RUNNING the reference's own CONSTRUCTORS of the elastic
vision transformer and its neck on stand-in bricks.  Run in the build container only:

    python tests/golden/make_ref_vit_ctor_fixture.py

As tests/golden/make_ref_ctor_fixtures.py does for the other models: the class nodes are cut out of the
reference files by AST and compiled in memory (the file text is never copied); the names they import from
the absent gaiavision / mmcv / mmseg / mmcls packages are bound to small real torch modules defined here
(ElasticLinear -> nn.Linear, build_norm_layer(ElaLN) -> ('ln<postfix>', nn.LayerNorm), build_conv_layer ->
nn.Conv2d, DynamicConvModule -> conv (+ bias when there is no norm)).  What is pinned is what the
reference's own code decides: module and parameter names, their order and their shapes.

  ElasticFFN / ElasticRelativePosition2D / ElasticMHA / ElasticTransformerEncoderLayer / ElasticEncoder /
  ElasticPatchEmbed / ElasticTransformer.__init__     gaiaseg/models/backbones/elastic_transformer.py
  DynamicMultiLevelNeck.__init__                      gaiaseg/models/necks/dynamic_multilevel_neck.py

tests/test_elastic_vit.py builds the same configurations through this repo's registries and requires the
same names and shapes."""
import ast
import json
import os
import warnings

import torch
import torch.nn as nn

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

BACKBONE_CASES = [
    dict(tag="tiny", kwargs=dict(embed_dim=128, num_heads=2, feedforward_channels=512, num_layers=[1, 2, 1],
                                 patch_size=16, img_size=(32, 48), drop_path=0.0,
                                 out_indices=[None, [0], None], out_stages=[0, 1, 2])),
    dict(tag="square_patch8", kwargs=dict(embed_dim=64, num_heads=1, feedforward_channels=192, num_layers=[2, 1, 1],
                                          patch_size=8, img_size=32, drop_path=0.0,
                                          out_indices=[None, None, None], out_stages=[2])),
]
NECK_CASES = [
    dict(tag="four_levels", kwargs=dict(in_channels=[128, 128, 128, 128], out_channels=16, scales=[4, 2, 1, 0.5])),
    dict(tag="one_level_default_scales", kwargs=dict(in_channels=[24], out_channels=8)),
]


def _class(rel, cls, namespace):
    with open(os.path.join(REF, rel)) as f:
        tree = ast.parse(f.read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    node.decorator_list = []
    ns = dict(namespace)
    exec(compile(ast.Module(body=[node], type_ignores=[]), rel, "exec"), ns)
    return ns[cls]


class DynamicMixin:
    pass


class BaseBackbone(nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg


class DropPath(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p


def build_norm_layer(cfg, num_features, postfix=""):
    return "ln%s" % postfix, nn.LayerNorm(num_features)


def build_conv_layer(cfg, *args, **kwargs):
    return nn.Conv2d(*args, **kwargs)


def build_activation_layer(cfg):
    return nn.GELU()


class DynamicConvModule(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=kwargs.get("padding", 0),
                              bias=kwargs.get("norm_cfg") is None)


def to_2tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _noop(*a, **k):
    return None


def dump(mod):
    return dict(modules=[[p, type(m).__name__] for p, m in mod.named_modules() if p],
                state_dict=[[k, list(v.shape)] for k, v in mod.state_dict().items()])


def main():
    torch.manual_seed(0)
    base = dict(nn=nn, torch=torch, warnings=warnings, DynamicMixin=DynamicMixin, BaseBackbone=BaseBackbone,
                ElasticLinear=nn.Linear, DropPath=DropPath, build_norm_layer=build_norm_layer,
                build_conv_layer=build_conv_layer, build_activation_layer=build_activation_layer,
                to_2tuple=to_2tuple, kaiming_init=_noop, constant_init=_noop, trunc_normal_=_noop,
                _BatchNorm=nn.modules.batchnorm._BatchNorm, DynamicConvModule=DynamicConvModule,
                xavier_init=_noop)
    rel = "gaiaseg/models/backbones/elastic_transformer.py"
    ns = dict(base)
    for name in ("ElasticFFN", "ElasticRelativePosition2D", "ElasticMHA", "ElasticTransformerEncoderLayer",
                 "ElasticEncoder", "ElasticPatchEmbed", "ElasticTransformer"):
        ns[name] = _class(rel, name, ns)
    neck = _class("gaiaseg/models/necks/dynamic_multilevel_neck.py", "DynamicMultiLevelNeck", base)
    out = dict(backbone=[], neck=[])
    for c in BACKBONE_CASES:
        net = ns["ElasticTransformer"](**c["kwargs"])
        out["backbone"].append(dict(tag=c["tag"], kwargs=c["kwargs"], **dump(net)))
    for c in NECK_CASES:
        out["neck"].append(dict(tag=c["tag"], kwargs=c["kwargs"], **dump(neck(**c["kwargs"]))))
    path = os.path.join(HERE, "ref_vit_ctors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote %s: %s" % (path, {k: len(v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
