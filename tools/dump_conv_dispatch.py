#!/usr/bin/env python
"""Dump what the conv entry points WOULD launch (host arithmetic, no GPU) for a fixed grid of
descriptors and library modes, or check a library against such a dump.

    python tools/dump_conv_dispatch.py --out tests/golden/conv_dispatch_table.json
    python tools/dump_conv_dispatch.py --check tests/golden/conv_dispatch_table.json

The table is the record of the dispatch: tests/test_conv_dispatch_table.py asserts that the library
reproduces it row for row, so a change of a gate, a plan or a K loop has to edit the table in the
open.  Regenerate it only from a build whose dispatch is the intended one (GS_HIP_LIB selects the
library; the environment must not carry GS_* tuning switches).

Grid: the convolutions of the MIN, R50 and MAX subnets of
configs/_dynamic_/model_samplers/ar50to101v2.py (output stride 32, and output stride 8 with dilations
2 / 4) and of the FCN / PSP / UPer heads, at 1024x512 batch 2 and 769x769 batch 4; dense and sliced
leading dimensions, role 0 and 1, in_affine null and set.  Per descriptor and mode: the three
gs_debug_query_conv_launch answers, gs_conv2d_workspace_bytes and gs_conv2d_in_affine_supported;
per GEMM view of a descriptor: gs_debug_query_plan.
"""
import argparse
import ctypes
import json
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from gaia_seg_amd.hip import lib  # noqa: E402

MAX_W, MAX_STEM = (80, 160, 320, 640), 64
SUBNETS = {"MIN": (32, (48, 96, 192, 384)), "R50": (64, (64, 128, 256, 512)),
           "MAX": (64, (80, 160, 320, 640))}
INPUTS = ((2, 512, 1024), (4, 769, 769))
STRIDES = {32: ((1, 2, 2, 2), (1, 1, 1, 1)), 8: ((1, 2, 1, 1), (1, 1, 2, 4))}
HEAD_CH, AUX_CH, NCLS = 512, 256, 20          # 19 classes, Co padded to a multiple of 4
# (name, calls that enter the mode, calls that leave it)
MODES = [
    ("default", [], []),
    ("fwd_fp16", [("gs_set_forward_precision", 1)], [("gs_set_forward_precision", 0)]),
    ("train_fp16", [("gs_set_train_precision", 1)], [("gs_set_train_precision", 0)]),
    ("x3_fwd_0", [("gs_debug_set_x3_fwd", 0)], [("gs_debug_set_x3_fwd", -1)]),
    ("x3_fwd_1", [("gs_debug_set_x3_fwd", 1)], [("gs_debug_set_x3_fwd", -1)]),
    ("x3_fwd_2", [("gs_debug_set_x3_fwd", 2)], [("gs_debug_set_x3_fwd", -1)]),
    ("stream_0", [("gs_debug_set_stream_mode", 0)], [("gs_debug_set_stream_mode", -1)]),
    ("stream_2", [("gs_debug_set_stream_mode", 2)], [("gs_debug_set_stream_mode", -1)]),
    ("plan_128x128x4", [("gs_debug_force_plan", 128, 128, 4)], [("gs_debug_force_plan", 0, 0, 0)]),
    ("plan_64x96x2", [("gs_debug_force_plan", 64, 96, 2)], [("gs_debug_force_plan", 0, 0, 0)]),
    ("plan_64x80x8", [("gs_debug_force_plan", 64, 80, 8)], [("gs_debug_force_plan", 0, 0, 0)]),
]
PLAN_MODES = ("default", "plan_128x128x4", "plan_64x96x2", "plan_64x80x8")
# descriptor row: N H W Ci Co Ci_max Co_ld K stride pad dil x_sw ldy role in_affine nchw
FIELDS = ("N", "H", "W", "Ci", "Co", "Ci_max", "Co_ld", "K", "stride", "pad", "dil", "x_sw", "ldy",
          "role", "in_affine", "nchw")


_out = lib.conv_out_size


def grid():
    """The descriptor rows, deduplicated, in a fixed order."""
    rows, seen = [], set()

    def add(n, h, w, ci, co, ci_max, co_ld, k, s=1, d=1, ldx=None, ldy=None, role=0, aff=0, nchw=0):
        p = d * (k // 2)
        for lx, ly in {(ci, co), (ldx or ci, ldy or co)}:
            r = (n, h, w, ci, co, ci_max, co_ld, k, s, p, d, lx, ly, role, aff, nchw)
            if r not in seen:
                seen.add(r)
                rows.append(r)

    for name, (stem, widths) in SUBNETS.items():
        for n, ih, iw in INPUTS:
            add(n, ih, iw, 3, stem, 3, MAX_STEM, 7, s=2, nchw=1)
            h0, w0 = _out(_out(ih, 7, 2, 3, 1), 3, 2, 1, 1), _out(_out(iw, 7, 2, 3, 1), 3, 2, 1, 1)
            for os_, (strides, dils) in STRIDES.items():
                if os_ == 8 and name != "R50":      # the dilated backbone: one subnet is enough
                    continue
                h, w, cin, cin_max, feats = h0, w0, stem, MAX_STEM, []
                for pl, pl_max, s, d in zip(widths, MAX_W, strides, dils):
                    for first in (True, False):
                        st = s if first else 1
                        ho, wo = _out(h, 3, st, d, d), _out(w, 3, st, d, d)
                        add(n, h, w, cin, pl, cin_max, pl_max, 1, ldx=cin_max, ldy=pl_max)
                        for role in (0, 1):
                            for aff in (0, 1):
                                add(n, h, w, pl, pl, pl_max, pl_max, 3, s=st, d=d, ldx=pl_max,
                                    ldy=pl_max, role=role, aff=aff)
                        for aff in (0, 1):
                            add(n, ho, wo, pl, 4 * pl, pl_max, 4 * pl_max, 1, ldx=pl_max,
                                ldy=4 * pl_max, aff=aff)
                        if first:
                            add(n, h, w, cin, 4 * pl, cin_max, 4 * pl_max, 1, s=st, ldx=cin_max,
                                ldy=4 * pl_max)
                        h, w, cin, cin_max = ho, wo, 4 * pl, 4 * pl_max
                    feats.append((h, w, cin, cin_max))
                # heads on this backbone
                (h2, w2, c2, c2m), (h3, w3, c3, c3m) = feats[2], feats[3]
                add(n, h2, w2, c2, AUX_CH, c2m, AUX_CH, 3, ldx=c2m)                      # aux FCN
                add(n, h2, w2, AUX_CH, NCLS, AUX_CH, NCLS, 1)
                add(n, h3, w3, c3, HEAD_CH, c3m, HEAD_CH, 3, ldx=c3m)                    # FCN
                add(n, h3, w3, HEAD_CH, HEAD_CH, HEAD_CH, HEAD_CH, 3, ldy=c3 + HEAD_CH)
                add(n, h3, w3, c3 + HEAD_CH, HEAD_CH, c3m + HEAD_CH, HEAD_CH, 3)
                add(n, h3, w3, HEAD_CH, NCLS, HEAD_CH, NCLS, 1)
                for ps in (1, 2, 3, 6):                                                  # PSP / UPer PPM
                    add(n, ps, ps, c3, HEAD_CH, c3m, HEAD_CH, 1, ldx=c3m)
                add(n, h3, w3, c3 + 4 * HEAD_CH, HEAD_CH, c3m + 4 * HEAD_CH, HEAD_CH, 3)
                for hh, ww, cc, ccm in feats[:3]:                                        # UPer FPN
                    add(n, hh, ww, cc, HEAD_CH, ccm, HEAD_CH, 1, ldx=ccm)
                    add(n, hh, ww, HEAD_CH, HEAD_CH, HEAD_CH, HEAD_CH, 3, ldy=4 * HEAD_CH)
                add(n, feats[0][0], feats[0][1], 4 * HEAD_CH, HEAD_CH, 4 * HEAD_CH, HEAD_CH, 3)
    return rows


def make_desc(row):
    f = dict(zip(FIELDS, row))
    d = lib.conv_desc(f["N"], f["H"], f["W"], f["Ci"], f["Co"], f["K"], f["stride"], f["dil"], f["pad"],
                      f["Ci_max"], f["Co_ld"], f["x_sw"], f["ldy"], role=f["role"])
    if f["nchw"]:
        d.x_sw, d.x_sh, d.x_sc, d.x_sn = 1, f["W"], f["H"] * f["W"], f["Ci"] * f["H"] * f["W"]
    d.in_affine = 0x1000 if f["in_affine"] else None      # never dereferenced by the queries
    return d


def gemm_views(rows):
    """(M, N, K, max_splits) of the forward / dgrad / wgrad GEMMs of every descriptor, deduplicated."""
    out, seen = [], set()
    for row in rows:
        d = make_desc(row)
        kk = d.KH * d.KW
        for v in ((d.N * d.Ho * d.Wo, d.Co, kk * d.Ci, 64), (d.N * d.H * d.W, d.Ci, kk * d.Co, 64),
                  (kk * d.Ci, d.Co, d.N * d.Ho * d.Wo, 512)):
            if v not in seen:
                seen.add(v)
                out.append(v)
    return out


def _call(L, calls):
    for name, *args in calls:
        rc = getattr(L, name)(*args)
        assert rc == 0, (name, args, rc)


def answers(L, row):
    d = make_desc(row)
    out = []
    q = lib.DebugLaunch()
    for op in (lib.OP_FORWARD, lib.OP_DGRAD, lib.OP_WGRAD):
        rc = L.gs_debug_query_conv_launch(ctypes.byref(d), op, ctypes.byref(q))
        out.append((rc,) if rc != 0 else
                   (q.kloop, q.bm, q.bn, q.splits, q.ksteps_per_split, q.in_affine))
    out.append(int(L.gs_conv2d_workspace_bytes(ctypes.byref(d))))
    out.append(int(L.gs_conv2d_in_affine_supported(ctypes.byref(d))))
    return out


def plan_answer(L, view):
    v = [ctypes.c_int32() for _ in range(4)]
    rc = L.gs_debug_query_plan(*view, *[ctypes.byref(x) for x in v])
    return [rc] if rc != 0 else [x.value for x in v]


def dump(L):
    """{'descs': rows, 'modes': names, 'launches': distinct [kloop, bm, bn, splits, ksteps, in_affine]
    (or [error code]), 'answers': distinct [forward, dgrad, wgrad launch, workspace bytes, in_affine
    supported], 'index': [desc][mode] -> answer, 'views': GEMMs, 'plan_modes': names,
    'plans': [view][plan mode] -> [bm, bn, splits, ksteps]}"""
    rows = grid()
    views = gemm_views(rows)
    launches, uniq, index = {}, {}, [[0] * len(MODES) for _ in rows]
    plans = [[None] * len(PLAN_MODES) for _ in views]
    for mi, (name, enter, leave) in enumerate(MODES):
        _call(L, enter)
        try:
            for di, row in enumerate(rows):
                a = answers(L, row)
                a[:3] = [launches.setdefault(x, len(launches)) for x in a[:3]]
                index[di][mi] = uniq.setdefault(tuple(a), len(uniq))
            if name in PLAN_MODES:
                for vi, view in enumerate(views):
                    plans[vi][PLAN_MODES.index(name)] = plan_answer(L, view)
        finally:
            _call(L, leave)
    return {"fields": list(FIELDS), "descs": [list(r) for r in rows], "modes": [m[0] for m in MODES],
            "launches": [list(x) for x in launches], "answers": [list(a) for a in uniq], "index": index, "views": [list(v) for v in views],
            "plan_modes": list(PLAN_MODES), "plans": plans}


def write(table, path):
    """One key per block, rows packed up to ~600 characters per line (the file is data, not prose)."""
    with open(path, "w") as f:
        f.write("{\n")
        keys = list(table)
        for k in keys:
            v = table[k]
            f.write(' "%s": ' % k)
            if v and isinstance(v[0], list):
                lines, cur = [], ""
                for r in v:
                    t = json.dumps(r, separators=(",", ":"))
                    if cur and len(cur) + len(t) > 600:
                        lines.append(cur)
                        cur = ""
                    cur += ("," if cur else "") + t
                lines.append(cur)
                f.write("[\n" + ",\n".join(lines) + "\n ]")
            else:
                f.write(json.dumps(v))
            f.write(",\n" if k != keys[-1] else "\n")
        f.write("}\n")


def differences(L, table):
    """Rows of `table` the library does not reproduce, as readable strings (empty = it matches)."""
    got = dump(L)
    bad = []
    for k in ("fields", "descs", "modes", "views", "plan_modes"):
        if got[k] != table[k]:
            return ["the grid itself differs at '%s': regenerate the table" % k]
    def expand(t, di, mi):
        a = t["answers"][t["index"][di][mi]]
        return [t["launches"][i] for i in a[:3]] + a[3:]

    for di, row in enumerate(table["descs"]):
        for mi, mode in enumerate(table["modes"]):
            want, have = expand(table, di, mi), expand(got, di, mi)
            if want != have:
                bad.append("desc %s mode %s: table %s, library %s" % (dict(zip(FIELDS, row)), mode, want, have))
    for vi, view in enumerate(table["views"]):
        for pi, mode in enumerate(table["plan_modes"]):
            if table["plans"][vi][pi] != got["plans"][vi][pi]:
                bad.append("plan M,N,K,max_splits %s mode %s: table %s, library %s"
                           % (view, mode, table["plans"][vi][pi], got["plans"][vi][pi]))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--check")
    args = ap.parse_args()
    L = lib.load()
    if args.check:
        bad = differences(L, json.load(open(args.check)))
        for b in bad[:40]:
            print(b)
        print("%d rows differ" % len(bad))
        return 1 if bad else 0
    table = dump(L)
    write(table, args.out)
    print("%d descriptors x %d modes, %d distinct answers, %d GEMM views -> %s"
          % (len(table["descs"]), len(MODES), len(table["answers"]), len(table["views"]), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
