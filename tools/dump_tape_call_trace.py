"""Record what the tape ops ask of the C-ABI: tests/golden/tape_call_trace.json.

For every case below, tests/host_dry_run.py --trace steps the config's model twice on CPU tensors
with every library entry stubbed, and reports the number of calls, the calls per entry and the
SHA-256 of the canonical call lines (arguments, null-ness of every pointer, every descriptor field).
tests/test_tape_call_trace.py runs the same cases and compares.  The golden file was dumped from the
tree that gave the tape ops one accumulate rule (ops._input_grad).  Against the dump before it, taken
from the commit BEFORE the stream state moved out of hip/ops.py, the calls and the calls per entry are the
same for every case; the digests of the ViT, Convformer and SegFormer cases differ, in the accumulate flag
of gs_attention_backward / gs_attention_kv_backward alone (1 -> 0, profiles/r27_accumulate_rule.md).
--root dumps from another checkout (with tests/host_dry_run.py of this tree copied into it):

    python tools/dump_tape_call_trace.py [--root CHECKOUT] > tests/golden/tape_call_trace.json

A change of what a tape op passes to a kernel has to regenerate the file, in the open.

Cases are the configs under configs/supernet/ at 64x128 (the elastic ViT's img_size is fixed:
512x1024).  The three plain ResNet configs are stepped at the R50 arch, the others at their max
arch.  (pspnet_ar50to101v2_inplace_distill is therefore the PSP supernet's max arch: the sandwich
members and their distillation loss are the runner's, a bare train_step has none.)  Left out:
  * the three DynamicDistiller configs (pspnet_ar50to101v2_distiller, .._distiller_cwd,
    upernet_elastic_vit_distiller_beit): the segmentor refuses to be built without a teacher
    checkpoint file.  With them attention_relpos, deconv2x2 and the frozen path of vit_tokens stay
    outside the trace; the GPU tests (test_beit_gpu.py, test_beit_ops_gpu.py, test_attention_gpu.py)
    cover them.
  * the _fp16, _paramwise, _elastic_scale, _finetune and _test_supernet* variants of
    fcn_ar50to101v2, upernet_elastic_vit(_adamw_fp16) and upernet_convnext_t2b_adamw: they differ
    from a listed config in optimizer, precision, data or evaluation settings, none of which a
    stubbed train_step sees.
  * deeplabv3_ar50to101_v1c_os8 and pspnet_ar50to101_v1c_os8: their ops (ASPP, PPM, the dilated
    v1c backbone) are those of deeplabv3plus and pspnet / ocrnet above."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [   # (config under configs/supernet/, input size)
    ("fcn_ar50to101v2", "64x128"),
    ("pspnet_ar50to101v2", "64x128"),
    ("upernet_ar50to101v2", "64x128"),
    ("deeplabv3plus_ar50to101_v1c_os8", "64x128"),
    ("ocrnet_ar50to101_v1c_os8", "64x128"),
    ("pspnet_ar50to101v2_inplace_distill", "64x128"),
    ("upernet_convnext_t2b", "64x128"),
    ("upernet_convnextv2_n2b_adamw", "64x128"),
    ("upernet_elastic_convformer_adamw", "64x128"),
    ("segformer_mit_b1to3_adamw", "64x128"),
    ("upernet_swin_t2b_adamw", "64x128"),
    ("upernet_elastic_vit_adamw", "512x1024"),
]


def trace(config, size, root=ROOT, out=None):
    """The dry run's report for one case (a subprocess: the stubs patch the library module)."""
    cmd = [sys.executable, os.path.join(root, "tests", "host_dry_run.py"),
           "configs/supernet/%s.py" % config, "--size", size, "--trace"]
    if out:
        cmd += ["--trace-out", out]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if res.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), res.stderr[-3000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    root = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
    cases = []
    for config, size in CASES:
        cases.append(dict(config=config, size=size, **trace(config, size, root)))
        print("%s: %d calls" % (config, cases[-1]["calls"]), file=sys.stderr)
    json.dump({"cases": cases}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
