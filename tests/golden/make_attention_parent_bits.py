"""Generates tests/golden/attention_parent_bits.json: the SHA-256 of the little-endian fp32 bytes of every
output of the attention entries, as given by the library built from the commit BEFORE the attention kernels
were rewritten as one template per kernel over the MFMA operand format.  Run on the GPU, against that build:

    make -C gaia_seg_amd/csrc          # in a checkout of the parent commit
    python tests/golden/make_attention_parent_bits.py /path/to/parent/libgaiaseg_hip.so [out.json]

What it records (tests/util_attention_gpu.output_digests): for every case of util_vit.ATTENTION_CASES, on the
fp32 and on the fp16-operand entries, O, lse, dQ, dK, dV with accumulate 0 and 1; for every case of
util_attention_gpu.RELPOS_CASES, in both precisions, O and lse of the relative-position forward.
tests/test_attention_gpu.py::test_attention_matches_parent_bits recomputes them with the working tree's
library and asserts equality."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    os.environ["GS_HIP_LIB"] = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "attention_parent_bits.json")
    from gaia_seg_amd.hip import lib
    import util_attention_gpu as A
    L = lib.load()
    bits = {}
    for kind, case in A.BITS_CASES:
        for precision in A.PRECISIONS:
            bits["%s/%s/%s" % (kind, case[0], precision)] = A.output_digests(L, lib, kind, case, precision)
            print(kind, case[0], precision, flush=True)
    with open(out, "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases from %s" % (out, len(bits), os.environ["GS_HIP_LIB"]))


if __name__ == "__main__":
    main()
