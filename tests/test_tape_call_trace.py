"""The tape ops ask the same of the C-ABI as the recorded trace (no GPU needed).

tests/golden/tape_call_trace.json holds, for every case of tools/dump_tape_call_trace.py (a config, an
input size), what tests/host_dry_run.py --trace reports for two consecutive train steps with every
library entry stubbed: the number of calls, the calls per entry and the SHA-256 of the canonical call
lines (entry, every scalar argument, null-ness of every pointer, every descriptor field by field).
It was dumped from the tree that gave the tape ops one accumulate rule (ops._input_grad); the Python
layer must reproduce it call for call.  (The dump before it came from the commit BEFORE the stream state
moved from hip/ops.py to hip/streams.py; the rule changed no call count, and of the arguments only the
accumulate flag of the attention backwards of three cases, 1 -> 0.)  A change of what an op passes to a
kernel has to regenerate the file, in the open.

What the stubbed run cannot see:
  * stream order (every stream handle is 0 under the stub);
  * the side-stream weight-gradient queue (the dry run sets ops.SIDE_WGRAD = False);
  * the branch streams (CUDA devices only).
Those are covered on the GPU by test_branch_streams_gpu.py, test_stream_1x1_gpu.py, test_stem_gpu.py,
test_runner_gpu.py and test_ddp_gpu.py.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tape_call_trace.json")


def _tool():
    spec = importlib.util.spec_from_file_location(
        "dump_tape_call_trace", os.path.join(ROOT, "tools", "dump_tape_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


def test_golden_covers_the_cases():
    golden = json.load(open(GOLDEN))["cases"]
    assert [(c["config"], c["size"]) for c in golden] == TOOL.CASES
    assert os.path.getsize(GOLDEN) < 64 * 1024
    entries = set().union(*(c["counts"] for c in golden))
    for op in ("conv_bn", "layernorm", "gelu_grn", "cell_layernorm", "attention", "attention_kv",
               "window_attention", "vit_tokens", "fcu_tokens", "fcu_down", "ocr_gather", "ocr_attend",
               "layer_scale", "dwconv2d"):
        assert "gs_%s_backward" % op in entries or "gs_%s_dgrad" % op in entries, op


@pytest.mark.parametrize("config,size", TOOL.CASES, ids=[c[0] for c in TOOL.CASES])
def test_tape_ops_reproduce_the_call_trace(config, size):
    want = next(c for c in json.load(open(GOLDEN))["cases"] if c["config"] == config)
    got = TOOL.trace(config, size)
    if got["counts"] != want["counts"]:
        diff = {k: (want["counts"].get(k, 0), got["counts"].get(k, 0))
                for k in sorted(set(want["counts"]) | set(got["counts"]))
                if want["counts"].get(k, 0) != got["counts"].get(k, 0)}
        print("calls per entry (recorded, now):", diff)
    assert got["counts"] == want["counts"]
    assert got["calls"] == want["calls"]
    assert got["sha256"] == want["sha256"], (
        "same calls per entry, other arguments: diff the --trace-out of tests/host_dry_run.py")
