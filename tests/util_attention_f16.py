"""The CPU witness of the fp16-operand attention kernels (csrc/attention_f16.hip):
float64 attention on the same fp32 inputs with the kernels' rounding points and nothing else,

  * Q, K, V and dO * 2^e (the kernels' power-of-two gradient scale) rounded to fp16,
  * exp(S - rowmax) rounded to fp16 for the O product (the row sum adds the unrounded values),
  * exp(S - lse) rounded to fp16 for dV, dS = P (dP - delta) rounded to fp16 (saturating),
  * delta = <dO, O> from the unrounded dO.

Its error against tests/util_vit.attention_ref is the budget of the kernels: each quantity of a kernel must
be within FACTOR times the witness's own error for that quantity.  FACTOR = 3 is the project's "bounded
factor of the arithmetic's own error" (tests/parity.py); the witness cannot reproduce the running-maximum
rounding of P or the summation order."""
import math

import torch

import util_vit as U

FACTOR = 3.0
F16_MAX = 65504.0


def r16(x):
    """round to fp16 (through fp32, as the kernels do), saturating; back to float64"""
    return x.float().clamp(-F16_MAX, F16_MAX).half().double()


def grad_scale_exponent(do):
    """e with 2^e * max|dO| in [4, 8); 0 for a zero (or non-finite) maximum; |e| <= 126"""
    m = float(do.abs().max())
    if m == 0.0 or not math.isfinite(m):
        return 0
    return max(-126, min(126, 3 - math.frexp(m)[1]))


def heads_view(t, heads):
    b, n, _ = t.shape
    return t.double().view(b, n, heads, U.HEAD_DIM).transpose(1, 2)


def tokens_view(t):
    b, h, n, d = t.shape
    return t.transpose(1, 2).reshape(b, n, h * d)


def witness(q, k, v, do, heads, scale=U.SCALE, bias=None):
    """-> (O, lse [b, heads, n], dQ, dK, dV) in float64; do=None gives the forward pair only; ``bias``: an
    additive [heads, N, N] term of the scaled scores (never rounded)"""
    qh, kh, vh = (r16(heads_view(t, heads)) for t in (q, k, v))
    s = qh @ kh.transpose(-2, -1) * scale
    if bias is not None:
        s = s + bias
    m = s.max(dim=-1, keepdim=True).values
    p = (s - m).exp()
    l = p.sum(dim=-1, keepdim=True)
    o = r16(p) @ vh / l
    lse = (m + l.log()).squeeze(-1)
    if do is None:
        return tokens_view(o), lse
    e = grad_scale_exponent(do)
    gs = 2.0 ** e
    doh = heads_view(do, heads)
    g = r16(doh * gs)
    delta = (doh * o).sum(dim=-1, keepdim=True) * gs
    pl = (s - lse.unsqueeze(-1)).exp()
    dv = r16(pl).transpose(-2, -1) @ g
    ds = r16(pl * (g @ vh.transpose(-2, -1) - delta))
    dq = ds @ kh * scale
    dk = ds.transpose(-2, -1) @ qh * scale
    return (tokens_view(o), lse) + tuple(tokens_view(t) / gs for t in (dq, dk, dv))
