"""Generates tests/golden/ref_beit_ctors.json by RUNNING the reference's own CONSTRUCTORS of the BEiT
backbone on stand-in helpers.  Run in the build container only:

    python tests/golden/make_ref_beit_ctor_fixture.py

As tests/golden/make_ref_vit_ctor_fixture.py does for the elastic transformer: the class nodes are cut out
of gaiaseg/models/backbones/beit.py by AST and compiled in memory (the file text is never copied); the
names they import from the absent timm / mmseg packages are bound to small stand-ins defined here
(to_2tuple, a no-op trunc_normal_).  What is recorded is data the reference's code produces: module names
and types, parameter and buffer names and shapes, and the VALUES of every ``relative_position_index``
buffer -- the index formula tests/test_beit.py holds the port's host function (and through it the kernel's
documented index) against.

  DropPath / Mlp / Attention / Block / PatchEmbed / RelativePositionBias / BEiT.__init__

Windows 2 x 3 and 3 x 2, ``patch_size`` 16 and 8 (the two ``fpn1..4`` branches), and the three position
variants: a table per block, one shared bias (with the absolute embedding), the absolute embedding only."""
import ast
import json
import math
import os
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REL = "gaiaseg/models/backbones/beit.py"

_TINY = dict(embed_dim=64, depth=4, num_heads=1, out_indices=[0, 1, 2, 3])
_VARIANTS = {
    "block_tables": dict(use_rel_pos_bias=True, use_abs_pos_emb=False, init_values=0.1, qkv_bias=True),
    "shared_bias": dict(use_shared_rel_pos_bias=True, use_abs_pos_emb=True),
    "abs_pos_only": dict(),
}
CASES = [dict(tag="p%d_%dx%d_%s" % (patch, wh, ww, name),
              kwargs=dict(img_size=(wh * patch, ww * patch), patch_size=patch, **_TINY, **variant))
         for patch in (16, 8) for (wh, ww) in ((2, 3), (3, 2)) for name, variant in _VARIANTS.items()]


def to_2tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _noop(*a, **k):
    return None


def _classes(names, namespace):
    with open(os.path.join(REF, REL)) as f:
        tree = ast.parse(f.read())
    ns = dict(namespace)
    for name in names:
        node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)
        node.decorator_list = []
        exec(compile(ast.Module(body=[node], type_ignores=[]), REL, "exec"), ns)
    return ns


def dump(mod):
    sd = mod.state_dict()
    return dict(modules=[[p, type(m).__name__] for p, m in mod.named_modules() if p],
                state_dict=[[k, list(v.shape)] for k, v in sd.items()],
                relative_position_index={k: v.tolist() for k, v in sd.items()
                                         if k.endswith("relative_position_index")})


def main():
    torch.manual_seed(0)
    ns = _classes(("DropPath", "Mlp", "Attention", "Block", "PatchEmbed", "RelativePositionBias", "BEiT"),
                  dict(nn=nn, torch=torch, math=math, partial=partial, F=F, to_2tuple=to_2tuple,
                       trunc_normal_=_noop, drop_path=_noop))
    out = [dict(tag=c["tag"], kwargs=c["kwargs"], **dump(ns["BEiT"](**c["kwargs"]))) for c in CASES]
    path = os.path.join(HERE, "ref_beit_ctors.json")
    with open(path, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
