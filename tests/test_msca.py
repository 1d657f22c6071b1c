"""gs_msca_* and gs_gate_mul_* without a GPU: the header and the binding agree, every argument error comes
back with its code before any launch, and the byte queries behave."""
import ctypes
import os
import re

from gaia_seg_amd.hip import lib

GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
P = 0x10000          # a 16-byte aligned, non-null address.  It is never dereferenced because every call that
#                      gets it has exactly one thing wrong and is refused before any launch.
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "gaiaseg_hip.h")
ENTRIES = {"gs_msca_saved_bytes": 1, "gs_msca_workspace_bytes": 1, "gs_msca_forward": 6, "gs_msca_backward": 11,
           "gs_gate_mul_forward": 9, "gs_gate_mul_backward": 14}


def desc(**change):
    d = lib.msca_desc(2, 9, 11, 8, c_ld=16, ldx=12, lds=24)
    for k, v in change.items():
        if k.startswith("K") and k != "K0":
            d.K[int(k[1])] = v
        else:
            setattr(d, k, v)
    return d


def table(**change):
    p = dict(w0=P, b0=P, w_row=[P] * 3, b_row=[P] * 3, w_col=[P] * 3, b_col=[P] * 3)
    for k, v in change.items():
        if "." in k:
            name, i = k.split(".")
            p[name] = list(p[name])
            p[name][int(i)] = v
        else:
            p[k] = v
    return lib.msca_filters(p["w0"], p["b0"], p["w_row"], p["b_row"], p["w_col"], p["b_col"])


def fwd(L, d, x=P, f="default", s=P, saved=P):
    f = table() if f == "default" else f
    return L.gs_msca_forward(ctypes.byref(d) if d is not None else None, x, ctypes.byref(f) if f is not None else None,
                             s, saved, None)


def bwd(L, d, x=P, ds=P, f="default", saved=P, dx=P, g="default", ws=P, ws_bytes=1 << 40):
    f = table() if f == "default" else f
    g = table() if g == "default" else g
    return L.gs_msca_backward(ctypes.byref(d) if d is not None else None, x, ds,
                              ctypes.byref(f) if f is not None else None, saved, dx, 0,
                              ctypes.byref(g) if g is not None else None, ws, ws_bytes, None)


def test_header_declares_the_entries_and_the_binding_matches(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert len(lib.PROTOTYPES[name][1]) == nargs and hasattr(hip_lib, name), name
    assert lib.ABI_VERSION >= 27 and hip_lib.gs_abi_version() == lib.ABI_VERSION
    assert ctypes.sizeof(lib.MscaDesc) == 11 * 4 and ctypes.sizeof(lib.MscaFilters) == 14 * 8


def test_msca_bad_descriptors_are_refused_before_any_launch(hip_lib):
    L = hip_lib
    for change, code in [(dict(N=0), GS_E_BADARG), (dict(H=0), GS_E_BADARG), (dict(W=-1), GS_E_BADARG),
                         (dict(C=0), GS_E_BADARG), (dict(K0=4), GS_E_BADARG), (dict(K0=9), GS_E_BADARG),
                         (dict(K0=0), GS_E_BADARG), (dict(K0=6), GS_E_BADARG), (dict(K1=23), GS_E_BADARG),
                         (dict(K2=-1), GS_E_BADARG), (dict(ldx=4), GS_E_BADARG), (dict(lds=4), GS_E_BADARG),
                         (dict(C_ld=4), GS_E_BADARG), (dict(C=6), GS_E_ALIGN), (dict(C_ld=18), GS_E_ALIGN),
                         (dict(ldx=14), GS_E_ALIGN), (dict(lds=26), GS_E_ALIGN)]:
        d = desc(**change)
        assert (fwd(L, d), bwd(L, d)) == (code, code), change
        assert L.gs_msca_saved_bytes(ctypes.byref(d)) == 0 and L.gs_msca_workspace_bytes(ctypes.byref(d)) == 0, change
    for i in range(3):
        for k in (0, 8, 22):
            d = desc(**{"K%d" % i: k})
            assert (fwd(L, d), bwd(L, d)) == (GS_E_BADARG, GS_E_BADARG), (i, k)
    assert (fwd(L, None), bwd(L, None)) == (GS_E_NULL, GS_E_NULL)
    assert L.gs_msca_saved_bytes(None) == 0 and L.gs_msca_workspace_bytes(None) == 0


def test_msca_bad_pointers_are_refused_before_any_launch(hip_lib):
    L = hip_lib
    d = desc()
    for name in ("x", "s", "saved"):
        assert fwd(L, d, **{name: None}) == GS_E_NULL and fwd(L, d, **{name: P + 4}) == GS_E_ALIGN, name
    for name in ("x", "ds", "saved", "dx", "ws"):
        assert bwd(L, d, **{name: None}) == GS_E_NULL and bwd(L, d, **{name: P + 4}) == GS_E_ALIGN, name
    assert fwd(L, d, f=None) == bwd(L, d, f=None) == bwd(L, d, g=None) == GS_E_NULL
    members = ["w0", "b0"] + ["%s.%d" % (n, i) for n in ("w_row", "b_row", "w_col", "b_col") for i in range(3)]
    assert len(members) == 14
    for m in members:
        assert fwd(L, d, f=table(**{m: None})) == GS_E_NULL and fwd(L, d, f=table(**{m: P + 8})) == GS_E_ALIGN, m
        assert bwd(L, d, f=table(**{m: None})) == GS_E_NULL and bwd(L, d, f=table(**{m: P + 8})) == GS_E_ALIGN, m
        assert bwd(L, d, g=table(**{m: None})) == GS_E_NULL and bwd(L, d, g=table(**{m: P + 8})) == GS_E_ALIGN, m
    need = L.gs_msca_workspace_bytes(ctypes.byref(d))
    assert bwd(L, d, ws_bytes=need - 1) == GS_E_WORKSPACE


def test_msca_byte_queries(hip_lib):
    L = hip_lib
    q = lambda f, n, h, w, c=8: f(ctypes.byref(lib.msca_desc(n, h, w, c, c_ld=16, ldx=16, lds=24)))    # noqa: E731
    assert q(L.gs_msca_saved_bytes, 2, 9, 11) == 4 * 2 * 9 * 11 * 8 * 4        # a and the three row results
    # the scratch holds at least the gradients of those four tensors, and depends on the pixel count alone
    assert q(L.gs_msca_workspace_bytes, 2, 9, 11) > 4 * 2 * 9 * 11 * 8 * 4
    assert q(L.gs_msca_workspace_bytes, 1, 64, 3) == q(L.gs_msca_workspace_bytes, 3, 1, 64) == q(
        L.gs_msca_workspace_bytes, 2, 8, 12)
    shapes = sorted([(1, 1, 1), (1, 1, 64), (1, 9, 8), (2, 5, 7), (1, 3, 40), (1, 40, 3), (1, 33, 17), (2, 9, 11),
                     (2, 24, 40), (2, 64, 128), (2, 128, 256), (4, 128, 256)], key=lambda s: s[0] * s[1] * s[2])
    for f in (L.gs_msca_saved_bytes, L.gs_msca_workspace_bytes):
        sizes = [q(f, *s) for s in shapes]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes), sizes
    assert q(L.gs_msca_workspace_bytes, 2, 9, 11, 16) > q(L.gs_msca_workspace_bytes, 2, 9, 11, 8)


def test_gate_mul_argument_checks(hip_lib):
    L = hip_lib
    fwd_ = lambda g=P, u=P, y=P, rows=105, c=8, ldg=8, ldu=12, ldy=16: L.gs_gate_mul_forward(   # noqa: E731
        g, u, y, rows, c, ldg, ldu, ldy, None)
    bwd_ = lambda dy=P, g=P, u=P, dg=P, du=P, rows=105, c=8, lddy=8, ldg=12, ldu=16, lddg=8, lddu=12: (   # noqa: E731
        L.gs_gate_mul_backward(dy, g, u, dg, du, rows, c, lddy, ldg, ldu, lddg, lddu, 0, None))
    for name in ("g", "u", "y"):
        assert fwd_(**{name: None}) == GS_E_NULL and fwd_(**{name: P + 4}) == GS_E_ALIGN, name
    assert fwd_(rows=0) == fwd_(c=0) == fwd_(ldg=4) == fwd_(ldu=4) == fwd_(c=16, ldy=12) == GS_E_BADARG
    assert fwd_(c=6) == fwd_(ldg=10) == fwd_(ldy=18) == GS_E_ALIGN
    for name in ("dy", "g", "u", "dg", "du"):
        assert bwd_(**{name: None}) == GS_E_NULL and bwd_(**{name: P + 4}) == GS_E_ALIGN, name
    assert bwd_(rows=-1) == bwd_(c=0) == bwd_(lddy=4) == bwd_(lddg=4) == bwd_(lddu=4) == GS_E_BADARG
    assert bwd_(c=6) == bwd_(ldu=18) == bwd_(lddg=10) == GS_E_ALIGN
