"""Host-only dry run of a training step (no GPU): every C-ABI entry point is replaced by a no-op stub,
so only the Python orchestration runs, on CPU tensors.  Used as a subprocess by
tests/test_host_logic.py and tests/test_tape_call_trace.py (the stubs patch the library module
globally) and by hand to profile the host cost of a step:

    python tests/host_dry_run.py [steps] [CONFIG.py] [--size HxW] [--profile N]
    python tests/host_dry_run.py CONFIG.py [--size HxW] --trace [--trace-out FILE]

The three ResNet configs of test_host_logic.py (fcn / pspnet / upernet _ar50to101v2) are stepped at
the R50 arch; every other config is stepped as built, at its max arch.

Without --trace it prints one JSON line: {"ms_per_step": ..., "unreachable_per_step": ...} — the
second number is what gc.collect() finds after one step: anything above zero is a reference cycle
that keeps device memory of a finished step alive until the cyclic collector runs.

With --trace the stub records every call of the first two steps of a fresh model (the first
allocates the gradients, the second accumulates) as one canonical line: the entry name, every
non-pointer argument by repr, every pointer as null / ptr (lib.PROTOTYPES tells them apart), every
descriptor as its field list.  It prints {"calls": ..., "counts": {entry: n}, "sha256": ...} of
those lines; --trace-out writes the lines themselves so that two checkouts can be diffed."""
import ctypes
import gc
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaia_seg_amd.hip import lib, ops  # noqa: E402

R50_CONFIGS = ("fcn_ar50to101v2", "pspnet_ar50to101v2", "upernet_ar50to101v2")


def _is(ctype, base):
    return isinstance(ctype, type) and issubclass(ctype, base)


def _fmt_struct(s):
    return "{%s}" % ",".join("%s=%s" % (f[0], _fmt(f[1], getattr(s, f[0]), True)) for f in s._fields_)


def _fmt(ctype, v, field=False):
    """Canonical text of the value ``v`` given for an argument (or held by a field) of C type ``ctype``."""
    if ctype in (ctypes.c_void_p, ctypes.c_char_p):
        return "ptr" if v else "null"
    if _is(ctype, ctypes.Structure):
        return _fmt_struct(v)
    if _is(ctype, ctypes.Array):
        return "[%s]" % ",".join(_fmt(ctype._type_, e, True) for e in v)
    if _is(ctype, ctypes._Pointer):
        if field or v is None:
            return "ptr" if v else "null"
        obj = getattr(v, "_obj", None)          # ctypes.byref(x)
        if obj is None:
            obj = v.contents if isinstance(v, ctypes._Pointer) else v   # pointer(x) / an array itself
        if isinstance(obj, ctypes.Structure):
            return "&" + _fmt_struct(obj)
        if isinstance(obj, ctypes.Array):
            return "&" + _fmt(type(obj), obj)
        return "ptr"                            # an output scalar
    return repr(v)


class _Stub:
    def __init__(self, trace=None):
        self._trace = trace

    def __getattr__(self, name):
        value = (1 << 20) if name.endswith("_bytes") else 1 if name.endswith("_supported") else 0
        trace = self._trace
        if trace is None:
            f = lambda *a: value      # noqa: E731
        else:
            argtypes = lib.PROTOTYPES[name][1]

            def f(*a):
                assert len(a) == len(argtypes), (name, len(a), len(argtypes))
                trace.append("%s(%s)" % (name, ", ".join(_fmt(t, v) for t, v in zip(argtypes, a))))
                return value
        setattr(self, name, f)
        return f


def _patch(stub):
    """Every module of the package that holds or binds ``_L``, ``current_stream_ptr`` or
    ``require_gpu_tensor`` gets the stubbed one (they are bound with from-imports)."""
    lib._lib = stub
    lib.load = lambda: stub
    for name, mod in list(sys.modules.items()):
        if mod is None or not name.startswith("gaia_seg_amd"):
            continue
        for attr, repl in (("_L", lambda: stub), ("current_stream_ptr", lambda: 0),
                           ("require_gpu_tensor", lambda t, what: None)):
            if attr in vars(mod):
                setattr(mod, attr, repl)
    ops.SIDE_WGRAD = False


def main():
    argv = sys.argv[1:]
    tracing = "--trace" in argv
    trace = [] if tracing else None
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    _patch(_Stub(trace))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = next((a for a in argv if a.endswith(".py")), "configs/supernet/fcn_ar50to101v2.py")
    h, w = (int(v) for v in argv[argv.index("--size") + 1].split("x")) if "--size" in argv else (64, 128)
    cfg = Config.fromfile(os.path.join(root, name))
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"),
                            test_cfg=cfg.get("test_cfg")).train()
    if os.path.splitext(os.path.basename(name))[0] in R50_CONFIGS:
        r50 = {"arch.backbone.stem.width": 64, "arch.backbone.body.width": [64, 128, 256, 512],
               "arch.backbone.body.depth": [3, 4, 6, 3]}
        model.manipulate_arch(fold_dict(r50)["arch"])
    batch = make_batch(2, h, w, 19, 0, torch.device("cpu"))

    def step():
        out = model.train_step(batch, None)
        out["loss"].backward()

    if tracing:
        del trace[:]    # (what building the model called)
        for i in (1, 2):
            trace.append("# step %d" % i)
            step()
        counts = {}
        for line in trace:
            if not line.startswith("#"):
                entry = line[:line.index("(")]
                counts[entry] = counts.get(entry, 0) + 1
        text = "\n".join(trace) + "\n"
        if "--trace-out" in argv:
            with open(argv[argv.index("--trace-out") + 1], "w") as f:
                f.write(text)
        print(json.dumps({"calls": sum(counts.values()), "counts": dict(sorted(counts.items())),
                          "sha256": hashlib.sha256(text.encode()).hexdigest()}))
        return

    for _ in range(3):
        step()
    gc.collect()
    step()
    unreachable = gc.collect()
    n = int(argv[0]) if argv and argv[0].isdigit() else 10
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        best = min(best, (time.perf_counter() - t0) / n)
    if "--profile" in argv:
        import cProfile
        import pstats
        pr = cProfile.Profile()
        pr.enable()
        for _ in range(n):
            step()
        pr.disable()
        pstats.Stats(pr).sort_stats("tottime").print_stats(int(argv[argv.index("--profile") + 1]))
    print(json.dumps({"ms_per_step": round(best * 1e3, 2), "unreachable_per_step": unreachable}))


if __name__ == "__main__":
    main()
