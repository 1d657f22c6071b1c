"""The depthwise convolution without a GPU: gs_dwconv2d_* check their descriptor and pointers on the
host before any launch, the workspace query is host arithmetic, and DynamicConv2d(groups=C) has the
depthwise logical shape on the HWIO physical layout."""
import ctypes

import pytest
import torch

from gaia_seg_amd.hip import lib

GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
P = 0x10000          # a 16-byte aligned, non-null address.  It is never dereferenced because every call that gets it is
                     # asserted to return a refusal code, and the library refuses before it launches


def _ref(d):
    return ctypes.byref(d) if d is not None else None


def fwd(L, d, x=P, w=P, y=P):
    return L.gs_dwconv2d_forward(_ref(d), x, w, None, y, None)


def dgrad(L, d, y=P, w=P, dx=P):
    return L.gs_dwconv2d_dgrad(_ref(d), y, w, dx, 0, None)


def wgrad(L, d, x=P, y=P, dw=P, ws=P, ws_bytes=1 << 30):
    return L.gs_dwconv2d_wgrad(_ref(d), x, y, dw, ws, ws_bytes, None)


def calls(L, d, **kw):
    """the return codes of forward, dgrad and wgrad under a fault all three see (the descriptor, or y)"""
    return fwd(L, d, **kw), dgrad(L, d, **kw), wgrad(L, d, **kw)


def test_binding_and_header(hip_lib):
    assert lib.ABI_VERSION >= 17 and ctypes.sizeof(lib.DwConvDesc) == 12 * 4
    header = open(lib.REPO_ROOT + "/include/gaiaseg_hip.h").read()
    for name in ("gs_dwconv2d_workspace_bytes", "gs_dwconv2d_forward", "gs_dwconv2d_dgrad",
                 "gs_dwconv2d_wgrad"):
        assert name + "(" in header and name in lib.PROTOTYPES and hasattr(hip_lib, name)


@pytest.mark.parametrize("change,code", [
    (dict(C=6), GS_E_ALIGN), (dict(C=8, ldx=10), GS_E_ALIGN), (dict(C=8, ldy=9), GS_E_ALIGN),
    (dict(C=8, C_ld=10), GS_E_ALIGN),
    (dict(KH=5, KW=5), GS_E_BADARG), (dict(KH=1, KW=1), GS_E_BADARG), (dict(KW=1), GS_E_BADARG),
    (dict(stride=2), GS_E_BADARG), (dict(stride=0), GS_E_BADARG),
    (dict(dil=0), GS_E_BADARG), (dict(pad=-1), GS_E_BADARG),
    (dict(N=0), GS_E_BADARG), (dict(H=0), GS_E_BADARG), (dict(C=0), GS_E_BADARG),
    (dict(ldx=4), GS_E_BADARG), (dict(ldy=4), GS_E_BADARG), (dict(C_ld=4), GS_E_BADARG),
    (dict(pad=0, dil=5), GS_E_BADARG),            # Ho = 9 - 10 < 1
])
def test_bad_descriptors_are_refused_before_any_launch(hip_lib, change, code):
    d = lib.dwconv_desc(2, 9, 11, 8, pad=1)
    for k, v in change.items():
        setattr(d, k, v)
    assert calls(hip_lib, d) == (code, code, code)
    assert hip_lib.gs_dwconv2d_workspace_bytes(ctypes.byref(d)) == 0


def test_null_and_misaligned_pointers(hip_lib):
    # (an argument goes only to the entries that take it: an entry with nothing wrong would launch on P)
    L, d = hip_lib, lib.dwconv_desc(2, 9, 11, 8, pad=1)
    assert calls(L, None) == (GS_E_NULL,) * 3
    assert (fwd(L, d, x=None), wgrad(L, d, x=None)) == (GS_E_NULL, GS_E_NULL)
    assert (fwd(L, d, w=None), dgrad(L, d, w=None)) == (GS_E_NULL, GS_E_NULL)
    assert calls(L, d, y=None) == (GS_E_NULL,) * 3
    assert dgrad(L, d, dx=None) == GS_E_NULL
    assert wgrad(L, d, dw=None) == GS_E_NULL
    assert wgrad(L, d, ws=None) == GS_E_NULL
    assert (fwd(L, d, x=P + 4), wgrad(L, d, x=P + 4)) == (GS_E_ALIGN, GS_E_ALIGN)
    assert (fwd(L, d, w=P + 8), dgrad(L, d, w=P + 8)) == (GS_E_ALIGN, GS_E_ALIGN)
    assert calls(L, d, y=P + 4) == (GS_E_ALIGN,) * 3
    assert dgrad(L, d, dx=P + 12) == GS_E_ALIGN
    assert wgrad(L, d, dw=P + 4) == GS_E_ALIGN
    assert wgrad(L, d, ws=P + 4) == GS_E_ALIGN
    assert L.gs_dwconv2d_forward(ctypes.byref(d), P, P, P + 4, P, None) == GS_E_ALIGN   # bias
    need = L.gs_dwconv2d_workspace_bytes(ctypes.byref(d))
    assert need > 0 and wgrad(L, d, ws_bytes=need - 1) == GS_E_WORKSPACE


def test_workspace_query_is_monotone_in_the_pixel_count(hip_lib):
    prev, seen = 0, set()
    for n, h, w in [(1, 1, 1), (1, 3, 5), (2, 9, 11), (1, 16, 16), (1, 16, 17), (1, 33, 17), (2, 16, 64),
                    (2, 64, 128), (2, 128, 256), (8, 128, 256)]:
        need = hip_lib.gs_dwconv2d_workspace_bytes(ctypes.byref(lib.dwconv_desc(n, h, w, 8, pad=1)))
        assert need >= prev and need >= 9 * 8 * 4 and need % 16 == 0, (n, h, w, need)
        prev = need
        seen.add(need)
    assert len(seen) > 4
    # proportional to C; the output size, not the input size, counts
    d8, d64 = lib.dwconv_desc(2, 16, 64, 8, pad=1), lib.dwconv_desc(2, 16, 64, 64, pad=1)
    q = hip_lib.gs_dwconv2d_workspace_bytes
    assert q(ctypes.byref(d64)) == 8 * q(ctypes.byref(d8))
    assert q(ctypes.byref(lib.dwconv_desc(2, 16, 64, 8, pad=0))) < q(ctypes.byref(d8))


def test_depthwise_dynconv_shape_and_layout():
    from gaia_seg_amd.core.bricks import DynamicConv2d, is_hwio
    c = DynamicConv2d(20, 20, 3, padding=6, dilation=6, groups=20, bias=False)
    assert c.depthwise and c.groups == 20
    assert tuple(c.weight.shape) == (20, 1, 3, 3)
    # physical [3][3][1][C_ld]: channel-contiguous taps
    assert c.weight.stride() == (1, 20, 60, 20) and is_hwio(c.weight)
    assert c.weight._gs_phys_shape == (3, 3, 1, 20)
    assert tuple(c.state_dict()["weight"].shape) == (20, 1, 3, 3)
    c.load_state_dict({"weight": torch.arange(180.0).view(20, 1, 3, 3)})
    assert is_hwio(c.weight) and float(c.weight[7, 0, 2, 1]) == 7 * 9 + 2 * 3 + 1
    odd = DynamicConv2d(6, 6, 3, padding=1, groups=6)            # C_ld rounds up to a float4 multiple
    assert odd.weight.stride() == (1, 8, 24, 8) and tuple(odd.bias.shape) == (6,)
    dense = DynamicConv2d(8, 8, 3, padding=1)
    assert not dense.depthwise and dense.groups == 1 and tuple(dense.weight.shape) == (8, 8, 3, 3)


@pytest.mark.parametrize("kwargs", [dict(groups=2), dict(groups=8, kernel_size=1), dict(groups=8, stride=2),
                                    dict(groups=8, kernel_size=5), dict(groups=4)])
def test_other_groupings_keep_the_old_refusal(kwargs):
    from gaia_seg_amd.core.bricks import DynamicConv2d
    kw = dict(kernel_size=3)
    kw.update(kwargs)
    with pytest.raises(NotImplementedError) as e:
        DynamicConv2d(8, 8, **kw)
    assert str(e.value) == "DynConv2d: groups != 1 is not used on the supernet hot path"
    with pytest.raises(NotImplementedError):
        DynamicConv2d(8, 16, 3, groups=8)


def test_separable_module_children_and_keys():
    from gaia_seg_amd.core.bricks import DynamicDepthwiseSeparableConvModule
    m = DynamicDepthwiseSeparableConvModule(24, 16, 3, padding=2, dilation=2, norm_cfg=dict(type="BN"))
    keys = set(m.state_dict())
    for pre in ("depthwise_conv", "pointwise_conv"):
        assert {pre + ".conv.weight", pre + ".bn.weight", pre + ".bn.bias", pre + ".bn.running_mean",
                pre + ".bn.running_var", pre + ".bn.num_batches_tracked"} <= keys
    assert len(keys) == 12
    dw, pw = m.depthwise_conv.conv, m.pointwise_conv.conv
    assert dw.depthwise and (dw.padding, dw.dilation) == (2, 2) and tuple(dw.weight.shape) == (24, 1, 3, 3)
    assert not pw.depthwise and tuple(pw.weight.shape) == (16, 24, 1, 1)
    assert m.depthwise_conv.bn.num_features == 24 and m.pointwise_conv.bn.num_features == 16
