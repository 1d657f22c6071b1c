#!/usr/bin/env python
"""Compare the gfx950 device code of two builds of the library, kernel by kernel.

    python tools/compare_isa.py PARENT_OBJ_DIR BRANCH_OBJ_DIR [--objects igemm_fwd ...]
                                [--rows-fast-from-12] [--out report.md]

For every object file present in both directories (gaia_seg_amd/lib/obj/*.o of each build) the
gfx950 code object is extracted (llvm-objdump --offloading), the kernels and their register / LDS /
scratch metadata are read from the AMDGPU notes (llvm-readelf --notes) and every kernel is
disassembled (llvm-objdump -d --no-show-raw-insn).  Required for "identical": a bijection between the
two sets of kernel symbols, equal metadata per pair, and equal disassembly per pair once addresses and
symbol names are stripped.  Bytes are not compared: two builds of one source give code objects that
differ outside the code.

--rows-fast-from-12 maps the parent's igemm_rows_fast_kernel symbols from the twelve-parameter
signature <BM, BN, BTRANS, KS, ABL, ROLE, PIPE, PAIR, AFF, X3, SK, F16> (last seen in 56ee07d) to
<BM, BN, BTRANS, KS, ROLE, KLOOP, AFF, SK, TIMELINE>; without it symbols must match by name.
Exit status 0 only if every pair is identical.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size")
KLOOP_FP32, KLOOP_FP32_PAIRS, KLOOP_BF16X3, KLOOP_F16 = 1, 2, 3, 5     # include/gaiaseg_hip.h


def run(cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, text=True).stdout


def code_object(obj, tmp):
    """Path of the gfx950 code object extracted from the fat object `obj` (None if it has none)."""
    base = os.path.join(tmp, os.path.basename(obj))
    if os.path.exists(base):
        os.remove(base)
    os.symlink(os.path.abspath(obj), base)
    run([os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(obj)], cwd=tmp)
    hits = [f for f in os.listdir(tmp)
            if f.startswith(os.path.basename(obj) + ".") and f.endswith("gfx950")]
    if len(hits) > 1:
        raise SystemExit("%s: expected one gfx950 code object, found %s" % (obj, hits))
    return os.path.join(tmp, hits[0]) if hits else None     # (None: host-only object)


def metadata(co):
    """{kernel symbol: {field: value}} from the AMDGPU metadata note."""
    out, cur = {}, {}
    for line in run([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).splitlines():
        m = re.match(r"\s+(?:- )?(\.[a-z_]+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if line.lstrip().startswith("- .") and re.match(r"  - \.", line):   # next kernel record
            cur = {}
        key, val = m.groups()
        if key in META:
            cur[key] = val
        elif key == ".name":
            out[val] = cur
    return out


def disassembly(co):
    """{symbol: [instruction lines, addresses and symbol references stripped]}"""
    out, cur = {}, None
    text = run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co])
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s*//.*$", "", line.strip())        # address (and branch target) comment
        cur.append(re.sub(r"\s+", " ", ins))
    return out


def targs(sym):
    """Template arguments of a mangled kernel name as ints (Li<n>E / Lb<0|1>E), in order."""
    return [int(v.replace("n", "-")) for v in re.findall(r"L[ib](n?\d+)E", sym.split("EEv")[0])]


def rows_fast_new_name(sym):
    """The nine-parameter symbol of a twelve-parameter igemm_rows_fast_kernel symbol."""
    a = targs(sym)
    assert len(a) == 12, sym
    bm, bn, btrans, ks, abl, role, pipe, pair, aff, x3, sk, f16 = a
    assert abl == 0 and pipe == 1, sym
    kloop = KLOOP_F16 if f16 else (KLOOP_BF16X3 if x3 else (KLOOP_FP32_PAIRS if pair else KLOOP_FP32))
    new = "Li%dELi%dELb%dELi%dELi%dELi%dELb%dELb%dELb0E" % (bm, bn, btrans, ks, role, kloop, aff, sk)
    head, tail = sym.split("igemm_rows_fast_kernelI", 1)
    return head + "igemm_rows_fast_kernelI" + new + tail[tail.index("EEv"):]


def compare_object(name, parent_obj, branch_obj, tmp, remap):
    ptmp, btmp = os.path.join(tmp, "p"), os.path.join(tmp, "b")
    os.makedirs(ptmp, exist_ok=True)
    os.makedirs(btmp, exist_ok=True)
    pco, bco = code_object(parent_obj, ptmp), code_object(branch_obj, btmp)
    pm, bm = (metadata(pco), metadata(bco)) if pco and bco else ({}, {})
    pd, bd = (disassembly(pco), disassembly(bco)) if pco and bco else ({}, {})
    if bool(pco) != bool(bco):
        raise SystemExit("%s: device code in only one of the builds" % name)
    rename = {}
    for s in pm:
        rename[s] = rows_fast_new_name(s) if remap and "igemm_rows_fast_kernelI" in s else s
    only_parent = sorted(s for s in pm if rename[s] not in bm)
    only_branch = sorted(set(bm) - set(rename.values()))
    diff = []
    lines = 0
    for s in sorted(pm):
        t = rename[s]
        if t not in bm:
            continue
        lines += len(pd.get(s, []))
        same_isa = pd.get(s) is not None and pd.get(s) == bd.get(t)
        if pm[s] != bm[t] or not same_isa:
            diff.append((s, t, pm[s], bm[t], same_isa))
    return dict(name=name, parent=len(pm), branch=len(bm), only_parent=only_parent,
                only_branch=only_branch, diff=diff, lines=lines, families=families(pm))


def families(meta):
    """Kernel count per template name (the <length><name> component of the mangled symbol)."""
    fam = {}
    for s in meta:
        name = s
        for m in re.finditer(r"\d+", s):
            cand = s[m.end():m.end() + int(m.group(0))]
            if cand.endswith("_kernel"):
                name = cand
                break
        fam[name] = fam.get(name, 0) + 1
    return fam


def report(results):
    out = ["| object | kernels parent | kernels branch | pairs | identical | instruction lines |",
           "|---|---|---|---|---|---|"]
    ok = True
    for r in results:
        pairs = r["parent"] - len(r["only_parent"])
        out.append("| %s | %d | %d | %d | %d | %d |" % (r["name"], r["parent"], r["branch"], pairs,
                                                       pairs - len(r["diff"]), r["lines"]))
        ok = ok and not (r["only_parent"] or r["only_branch"] or r["diff"])
    out.append("")
    fam = {}
    for r in results:
        for k, v in r["families"].items():
            fam[k] = fam.get(k, 0) + v
    out.append("Kernels by template (parent): " + ", ".join("%d `%s`" % (v, k) for k, v in sorted(fam.items())))
    out.append("")
    for r in results:
        for s in r["only_parent"]:
            out.append("* %s: only in the parent: `%s`" % (r["name"], s))
        for s in r["only_branch"]:
            out.append("* %s: only in the branch: `%s`" % (r["name"], s))
        for s, t, a, b, same_isa in r["diff"]:
            out.append("* %s: `%s` -> `%s`: disassembly %s; parent %s; branch %s"
                       % (r["name"], s, t, "identical" if same_isa else "DIFFERS", a, b))
    out.append("every pair identical" if ok else "NOT identical")
    return ok, "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--objects", nargs="*")
    ap.add_argument("--rows-fast-from-12", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    names = args.objects or sorted(f[:-2] for f in os.listdir(args.parent)
                                   if f.endswith(".o") and os.path.exists(os.path.join(args.branch, f)))
    results = []
    for n in names:
        with tempfile.TemporaryDirectory() as tmp:
            results.append(compare_object(n, os.path.join(args.parent, n + ".o"),
                                          os.path.join(args.branch, n + ".o"), tmp,
                                          args.rows_fast_from_12))
        print("%s: %d kernels, %d differ" % (n, results[-1]["parent"], len(results[-1]["diff"])),
              file=sys.stderr)
    ok, text = report(results)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
