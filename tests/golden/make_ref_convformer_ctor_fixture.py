"""Generates tests/golden/ref_convformer_ctors.json by RUNNING the reference's own CONSTRUCTORS of the
ElasticConvformer backbone on stand-in bricks.  Run in the build container only:

    python tests/golden/make_ref_convformer_ctor_fixture.py

As tests/golden/make_ref_vit_ctor_fixture.py does for the elastic transformer: the class nodes are cut out of
the reference file by AST and compiled in memory (the file text is never copied); the names they import from
the absent gaiavision / mmcv / mmseg / mmcls packages are bound to small real torch modules defined here
(ElasticLinear -> nn.Linear, build_norm_layer(ElaLN) -> ('ln<postfix>', nn.LayerNorm), build_norm_layer(DynBN)
-> ('bn<postfix>', nn.BatchNorm2d), build_conv_layer -> nn.Conv2d, build_activation_layer -> nn.ReLU /
nn.GELU).  What is pinned is what the reference's own code decides: module and parameter names, their order
and their shapes.

  ElasticFFN / ElasticRelativePosition2D / ElasticMHA / Elastic_trans_Block / Elastic_conv_Block /
  Elastic_conv2trans / Elastic_trans2conv / Elastic_ConvTrans_Block / Elastic_Block /
  ElasticConvformer.__init__                          gaiaseg/models/backbones/elastic_convformer.py

tests/test_convformer.py builds the same configurations through this repo's registry and requires the same
names and shapes."""
import ast
import json
import os
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REL = "gaiaseg/models/backbones/elastic_convformer.py"

CASES = [
    dict(tag="tiny", kwargs=dict(embed_dim=128, num_heads=[2, 2, 2], mlp_ratio=[4, 4, 4], depth=9, stem_width=16,
                                 body_width=[32, 64, 128], body_depth=[2, 2, 2], patch_size=16, drop_path=0.0)),
    dict(tag="patch32", kwargs=dict(embed_dim=64, num_heads=[1, 2, 1], mlp_ratio=[2, 3, 4], depth=6, stem_width=16,
                                    body_width=[16, 32, 48], body_depth=[1, 2, 1], patch_size=32, drop_path=0.0)),
]
CLASSES = ("ElasticFFN", "ElasticRelativePosition2D", "ElasticMHA", "Elastic_trans_Block", "Elastic_conv_Block",
           "Elastic_conv2trans", "Elastic_trans2conv", "Elastic_ConvTrans_Block", "Elastic_Block",
           "ElasticConvformer")


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
    if cfg["type"] == "ElaLN":
        return "ln%s" % postfix, nn.LayerNorm(num_features)
    assert cfg["type"] == "DynBN", cfg
    return "bn%s" % postfix, nn.BatchNorm2d(num_features)


def build_conv_layer(cfg, *args, **kwargs):
    return nn.Conv2d(*args, **kwargs)


def build_activation_layer(cfg):
    return {"ReLU": nn.ReLU, "GELU": nn.GELU}[cfg["type"]]()


def _noop(*a, **k):
    return None


def dump(mod):
    return dict(modules=[[p, type(m).__name__] for p, m in mod.named_modules() if p],
                state_dict=[[k, list(v.shape)] for k, v in mod.state_dict().items()])


def main():
    torch.manual_seed(0)
    ns = dict(nn=nn, torch=torch, F=F, warnings=warnings, DynamicMixin=DynamicMixin, BaseBackbone=BaseBackbone,
              ElasticLinear=nn.Linear, DropPath=DropPath, build_norm_layer=build_norm_layer,
              build_conv_layer=build_conv_layer, build_activation_layer=build_activation_layer,
              kaiming_init=_noop, load_checkpoint=_noop, get_root_logger=_noop,
              to_2tuple=lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v))
    for name in CLASSES:
        ns[name] = _class(REL, name, ns)
    out = dict(backbone=[])
    for c in CASES:
        net = ns["ElasticConvformer"](**c["kwargs"])
        out["backbone"].append(dict(tag=c["tag"], kwargs=c["kwargs"], **dump(net)))
    path = os.path.join(HERE, "ref_convformer_ctors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote %s: %s" % (path, [(b["tag"], len(b["state_dict"])) for b in out["backbone"]]))


if __name__ == "__main__":
    main()
