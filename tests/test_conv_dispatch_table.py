"""The conv dispatch is a recorded table (no GPU needed: the queries are host arithmetic).

tests/golden/conv_dispatch_table.json holds, for a fixed grid of descriptors (the convolutions of the
MIN / R50 / MAX subnets and of the FCN / PSP / UPer heads at 1024x512 batch 2 and 769x769 batch 4) and
eleven library modes (default, fp16 forward, fp16 training, three bf16x3 forward modes, two streaming
modes, three forced plans), what gs_debug_query_conv_launch answers for the three ops, what
gs_conv2d_workspace_bytes and gs_conv2d_in_affine_supported return, and gs_debug_query_plan for every
GEMM view.  It was dumped with tools/dump_conv_dispatch.py from the commit BEFORE the routing of the
conv entry points moved into csrc/igemm_route.h; the library must reproduce it row for row.  A change
of a gate, a plan or a K loop therefore has to regenerate the table, in the open.

The table assumes the default environment (no GS_* tuning switch set) and 256 compute units, which is
what the planner sees on an MI355X and what it falls back to without a device.
"""
import importlib.util
import json
import os

from gaia_seg_amd.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_dispatch_table.json")


def _tool():
    spec = importlib.util.spec_from_file_location(
        "dump_conv_dispatch", os.path.join(ROOT, "tools", "dump_conv_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_covers_the_grid():
    table = json.load(open(TABLE))
    tool = _tool()
    assert os.path.getsize(TABLE) < 200 * 1024
    assert table["descs"] == [list(r) for r in tool.grid()]
    assert table["modes"] == [m[0] for m in tool.MODES] and len(table["modes"]) == 11
    f = table["fields"]
    col = {k: {r[f.index(k)] for r in table["descs"]} for k in f}
    assert col["K"] == {1, 3, 7} and col["stride"] == {1, 2} and col["dil"] == {1, 2, 4}
    assert col["role"] == {0, 1} and col["in_affine"] == {0, 1} and col["N"] == {2, 4}
    assert any(r[f.index("x_sw")] > r[f.index("Ci")] for r in table["descs"])     # sliced inputs
    assert any(r[f.index("ldy")] > r[f.index("Co")] for r in table["descs"])      # sliced outputs
    # every K loop and both answers of the in_affine query occur
    kloops = {(op, table["launches"][a[op]][0]) for a in table["answers"] for op in range(3)
              if len(table["launches"][a[op]]) == 6}
    assert {k for op, k in kloops if op == lib.OP_FORWARD} == {0, 1, 2, 3, 4, 5}
    assert {k for op, k in kloops if op == lib.OP_DGRAD} == {0, 1, 2, 3, 4, 5}
    assert {k for op, k in kloops if op == lib.OP_WGRAD} == {0, 1, 2}
    assert {a[4] for a in table["answers"]} == {0, 1}


def test_library_reproduces_the_dispatch_table():
    assert lib.load().gs_debug_num_cu() == 256, "the table is for 256 compute units"
    switches = sorted(k for k in os.environ if k.startswith("GS_") and k != "GS_HIP_LIB")
    bad = _tool().differences(lib.load(), json.load(open(TABLE)))
    assert not bad, "%d rows differ (GS_* switches in the environment: %s); first: %s" % (
        len(bad), switches or "none", bad[:5])
