"""Model-space files and sampling rules (core/model_space.py), the forward-precision dispatch of
the C-ABI (host arithmetic) and the option checks of tools/test_supernet.py: no GPU needed."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from gaia_seg_amd.core.model_space import (ModelSpace, build_sample_rule, dump_model_space,
                                           load_model_space)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = "arch.backbone.body.depth"
WIDTH = "arch.backbone.body.width"


def _space():
    """Eight distinct subnets: stage-3 depth 6 or 23, four widths each, made-up FLOPs / metrics."""
    rows = []
    for i in range(8):
        d3 = 6 if i < 4 else 23
        rows.append({"name": "s%d" % i, DEPTH: [3, 4, d3, 3], WIDTH: [64, 128, 256, 512 + 128 * (i % 4)],
                     "arch.backbone.stem.width": 64, "overhead.flops": 1e11 * (i + 1),
                     "metric.direct.mIoU": [0.3, 0.7, 0.5, 0.1, 0.9, 0.2, 0.6, 0.4][i]})
    return ModelSpace(rows)


def _names(ms):
    return [r["name"] for r in ms]


def test_filter_on_tuple_valued_key():
    ms = _space()
    assert isinstance(ms.rows[0][DEPTH], tuple)
    out = ms.apply_rule(dict(func_str="lambda x: x['arch.backbone.body.depth'] == (3, 4, 23, 3)"))
    assert _names(out) == ["s4", "s5", "s6", "s7"]
    same = ms.apply_rule(dict(type="eval", func_str="lambda x: x['overhead.flops'] <= 3e11"))
    assert _names(same) == ["s0", "s1", "s2"]


def test_parallel_gives_one_group_per_sub_rule():
    ms = _space()
    rule = build_sample_rule(dict(type="parallel", rules=[
        dict(func_str="lambda x: x['arch.backbone.body.depth'][2] == 6"),
        dict(func_str="lambda x: x['arch.backbone.body.depth'][2] == 23"),
        dict(func_str="lambda x: x['overhead.flops'] > 6.5e11")]))
    groups = rule([list(ms.rows)])
    assert [[r["name"] for r in g] for g in groups] == [["s0", "s1", "s2", "s3"],
                                                         ["s4", "s5", "s6", "s7"], ["s6", "s7"]]
    # two input groups x two sub-rules -> four groups, input-group-major
    groups = build_sample_rule(dict(type="parallel", rules=[
        dict(func_str="lambda x: True"), dict(func_str="lambda x: False")]))(groups[:2])
    assert [len(g) for g in groups] == [4, 0, 4, 0]


def test_seeded_random_sample_is_reproducible_in_both_modes():
    ms = _space()
    split = dict(type="parallel", rules=[dict(func_str="lambda x: x['arch.backbone.body.depth'][2] == 6"),
                                         dict(func_str="lambda x: x['arch.backbone.body.depth'][2] == 23")])
    for mode, value, per_group in (("number", 2, 2), ("ratio", 0.75, 3)):
        rule = dict(type="sequential", rules=[split, dict(type="sample", operation="random",
                                                          value=value, mode=mode, seed=7)])
        a, b = _names(ms.apply_rule(rule)), _names(ms.apply_rule(rule))
        assert a == b and len(a) == 2 * per_group, (mode, a)
        assert set(a[:per_group]) <= {"s0", "s1", "s2", "s3"}
        assert set(a[per_group:]) <= {"s4", "s5", "s6", "s7"}
    other = dict(type="sequential", rules=[split, dict(type="sample", operation="random", value=2, seed=8)])
    draws = {tuple(_names(ms.apply_rule(dict(other, rules=[split, dict(type="sample", operation="random",
                                                                       value=2, seed=s)]))))
             for s in range(6)}
    assert len(draws) > 1       # the seed matters


def test_top_by_metric_key():
    ms = _space()
    best = ms.apply_rule(dict(type="sample", operation="top", key="metric.direct.mIoU", value=1))
    assert _names(best) == ["s4"]
    top3 = ms.apply_rule(dict(type="sample", operation="top", key="metric.direct.mIoU", value=3))
    assert _names(top3) == ["s4", "s1", "s6"]
    half = ms.apply_rule(dict(type="sample", operation="top", key="overhead.flops", value=0.5, mode="ratio"))
    assert _names(half) == ["s7", "s6", "s5", "s4"]


def test_merge_keeps_order_and_drops_duplicates():
    ms = _space()
    rows = list(ms.rows)
    dup = dict(rows[1], name="s1-again")     # same architecture as s1
    groups = [[rows[2], rows[1]], [dup, rows[5]], [rows[2]]]
    merged = build_sample_rule(dict(type="merge"))(groups)
    assert len(merged) == 1 and [r["name"] for r in merged[0]] == ["s2", "s1", "s5"]


def test_example_rules_config():
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_test_supernet.py"))
    ms = _space().apply_rule(cfg.model_sampling_rules)
    names = _names(ms)
    # band 2e11..4e11 = s1, s2, s3; all shallow: one group of three -> two drawn; deep group empty
    assert len(names) == 2 and set(names) <= {"s1", "s2", "s3"}


def test_unknown_rule_type_rejected():
    with pytest.raises(ValueError, match="unknown"):
        build_sample_rule(dict(type="shuffle"))
    with pytest.raises(ValueError):
        build_sample_rule(dict(type="sample", operation="best", value=1))
    with pytest.raises(ValueError):
        build_sample_rule(dict(type="sequential", rules=[dict(type="nope")]))


def test_count_flops_file_round_trip(tmp_path):
    rows = [{"name": "R50", DEPTH: [3, 4, 6, 3], WIDTH: [64, 128, 256, 512], "arch.backbone.stem.width": 64,
             "overhead.flops": 238.5e9, "overhead.backbone_flops": 170.8e9, "overhead.params": 23.51e6},
            {"name": "R101", DEPTH: [3, 4, 23, 3], WIDTH: [64, 128, 256, 512], "arch.backbone.stem.width": 64,
             "overhead.flops": 393.7e9, "overhead.backbone_flops": 326.0e9, "overhead.params": 42.5e6}]
    src = tmp_path / "flops.json"
    with open(src, "w") as fh:
        json.dump(rows, fh, indent=1)          # tools/count_flops.py's writer
    first = load_model_space(str(src))
    assert first[0][DEPTH] == (3, 4, 6, 3)
    dump_model_space(first, str(tmp_path / "again.json"))
    again = load_model_space(str(tmp_path / "again.json"))
    assert again == first
    assert json.load(open(tmp_path / "again.json")) == rows
    # JSON lines are accepted as well
    with open(tmp_path / "rows.jsonl", "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    assert load_model_space(str(tmp_path / "rows.jsonl")) == first
    packed = ModelSpace(first).pack()
    assert packed[1] == {"backbone": {"stem": {"width": 64},
                                      "body": {"depth": [3, 4, 23, 3], "width": [64, 128, 256, 512]}}}


# ---- forward precision: what the planner would launch (host arithmetic) ----------------------
def _r50_eval_descs(lib):
    """The convs of the R50 bottlenecks (conv1 1x1, conv2 3x3 (strided at a stage's first block),
    conv3 1x1 with the deferred BN + ReLU, downsample) for one 1024x2048 image."""
    out = []
    h, w, cin = 256, 512, 64
    for stage, (planes, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2))):
        cout = 4 * planes
        for first in (True, False):
            s = stride if first else 1
            ci = cin if first else cout
            ho, wo = h // s, w // s
            convs = [(h, w, ci, planes, 1, 1, False), (h, w, planes, planes, 3, s, True),
                     (ho, wo, planes, cout, 1, 1, True)]
            if first:
                convs.append((h, w, ci, cout, 1, s, False))
            for (hh, ww, c_in, c_out, k, st, aff) in convs:
                d = lib.conv_desc(1, hh, ww, c_in, c_out, k, st, role=1 if k == 3 else 0)
                out.append(("s%d %dx%d %d->%d" % (stage + 1, k, k, c_in, c_out), d, aff))
            if first:
                h, w = ho, wo
        cin = cout
    return out


def _query(L, lib, d, op, aff):
    coeffs = (ctypes.c_float * 4)()
    d.in_affine = ctypes.addressof(coeffs) if aff and L.gs_conv2d_in_affine_supported(ctypes.byref(d)) else None
    q = lib.DebugLaunch()
    assert L.gs_debug_query_conv_launch(ctypes.byref(d), op, ctypes.byref(q)) == 0
    return (q.kloop, q.bm, q.bn, q.splits, q.ksteps_per_split, q.in_affine)


def test_forward_precision_dispatch_without_gpu():
    from gaia_seg_amd.hip import lib
    L = lib.load()
    assert lib.KLOOP_F16 == 5 and lib.KLOOP_COUNT == 5
    assert L.gs_get_forward_precision() == 0
    assert L.gs_set_forward_precision(2) == -1 and L.gs_set_forward_precision(-1) == -1
    descs = _r50_eval_descs(lib)
    ops = (lib.OP_FORWARD, lib.OP_DGRAD, lib.OP_WGRAD)
    before = {(name, op): _query(L, lib, d, op, aff) for name, d, aff in descs for op in ops}
    assert L.gs_set_forward_precision(1) == 0
    try:
        assert L.gs_get_forward_precision() == 1
        f16 = {(name, op): _query(L, lib, d, op, aff) for name, d, aff in descs for op in ops}
    finally:
        assert L.gs_set_forward_precision(0) == 0
    after = {(name, op): _query(L, lib, d, op, aff) for name, d, aff in descs for op in ops}
    assert after == before                         # switch at 0 == never set
    n_f16 = n_aff = 0
    for (name, op), q in f16.items():
        if op != lib.OP_FORWARD:
            assert q == before[(name, op)], (name, op)     # gradients ignore the switch
            continue
        b = before[(name, op)]
        assert b[0] != lib.KLOOP_F16
        if b[0] in (lib.KLOOP_STREAM, lib.KLOOP_GENERIC) or b[1] != 64:
            assert q == b, name                    # the streaming / generic kernels stay fp32
        else:
            assert q[0] == lib.KLOOP_F16 and q[1] == 64 and q[2] in (64, 48), (name, q)
            assert q[3] == b[3] and q[5] == b[5], name    # split-K and in_affine unchanged
            n_f16 += 1
            n_aff += q[5]
    # every 3x3 of the bottlenecks and the deferred-input conv3s that the tile kernel takes
    assert all(f16[(name, lib.OP_FORWARD)][0] == lib.KLOOP_F16 for name, _, _ in descs if "3x3" in name)
    assert n_f16 >= 10 and n_aff >= 4, (n_f16, n_aff)


# ---- tools/test_supernet.py option checks ------------------------------------------------------
@pytest.mark.parametrize("extra", [["--show"], ["--show-dir", "x"], ["--format-only"], ["--save-results"],
                                   ["--launcher", "slurm"], ["--launcher", "mpi"], ["--aug-test"],
                                   ["--eval", "mDice"], ["--eval-options", "efficient_test=True"]])
def test_test_supernet_refuses_unsupported_options(extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "test_supernet.py"), "cfg.py", "ck.pth"] + extra
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 2, res.stderr[-2000:]
    assert "not supported" in res.stderr or "supported" in res.stderr.split("error:")[-1], res.stderr[-2000:]
