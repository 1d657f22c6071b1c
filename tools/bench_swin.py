#!/usr/bin/env python
"""Times gs_window_attention_* (forward, and forward + backward) at the four stage maps of a 1024 x 512 crop of
the Swin-B supernet (B = 2, window 7, shift 3, maps padded to the window: 259x133, 133x70, 70x35, 35x21 with 4 /
8 / 16 / 32 heads) beside two yardsticks that do not depend on the code under test:

  (a) fp32 torch on the same device doing the same job through autograd: roll, window partition,
      scaled_dot_product_attention with the gathered bias + mask, reverse, roll back;
  (b) gs_copy2d of the operator's own bytes (Q, K, V read, O written): the memory floor.

Every figure is the median of per-iteration event pairs after warm-up, random operands.  One JSON line per
shape.  Usage: python tools/bench_swin.py [--iters 30] [--warmup 5]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(259, 133, 4), (133, 70, 8), (70, 35, 16), (35, 21, 32)]
B, WS, SHIFT, HEAD_DIM = 2, 7, 3, 32


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def torch_geometry(h, w, dev):
    yp, xp = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")

    def r(t, n):
        return (t >= n - WS).long() + (t >= n - SHIFT).long()
    region = (3 * r(yp, h) + r(xp, w)).view(h // WS, WS, w // WS, WS).permute(0, 2, 1, 3).reshape(-1, WS * WS)
    mask = torch.where(region[:, :, None] == region[:, None, :], 0.0, -100.0)
    iy, ix = torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")
    iy, ix = iy.reshape(-1), ix.reshape(-1)
    idx = (iy[:, None] - iy[None, :] + WS - 1) * (2 * WS - 1) + (ix[:, None] - ix[None, :] + WS - 1)
    return mask.to(dev), idx.reshape(-1).to(dev)


def torch_window_attention(q, k, v, table, mask, idx, h, w, heads):
    n = WS * WS

    def part(t):
        t = torch.roll(t.view(B, h, w, heads * HEAD_DIM), (-SHIFT, -SHIFT), (1, 2))
        t = t.view(B, h // WS, WS, w // WS, WS, heads, HEAD_DIM).permute(0, 1, 3, 5, 2, 4, 6)
        return t.reshape(-1, heads, n, HEAD_DIM)
    bias = table[idx].view(n, n, heads).permute(2, 0, 1)[None] + mask[:, None]            # [nw, heads, n, n]
    bias = bias[None].expand(B, -1, -1, -1, -1).reshape(-1, heads, n, n)
    o = torch.nn.functional.scaled_dot_product_attention(part(q), part(k), part(v), attn_mask=bias)
    o = o.view(B, h // WS, w // WS, heads, WS, WS, HEAD_DIM).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, h, w, -1)
    return torch.roll(o, (SHIFT, SHIFT), (1, 2)).reshape(B, h * w, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", action="store_true",
                    help="only the training step (images/s) of configs/supernet/upernet_swin_t2b_adamw.py on its MIN / "
                         "MID / MAX anchors and a sampled mix")
    ap.add_argument("--mix", type=int, default=8)
    args = ap.parse_args()
    if args.steps:
        from bench_segformer import bench_steps   # the same runner set-up, on this recipe
        from gaia_seg_amd.core.config import Config
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        cfg = Config.fromfile(os.path.join(root, "configs", "supernet", "upernet_swin_t2b_adamw.py"))
        args.iters, args.warmup = min(args.iters, 6), min(args.warmup, 2)
        print(json.dumps({"images_per_s": bench_steps(cfg, args)}), flush=True)
        return
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    L, dev = lib.load(), "cuda"
    for h, w, heads in SHAPES:
        c, rows = HEAD_DIM * heads, B * h * w
        g = torch.Generator(device=dev).manual_seed(1)
        q, k, v, do = (torch.randn(B, h * w, c, device=dev, generator=g) for _ in range(4))
        table = 0.5 * torch.randn((2 * WS - 1) ** 2, heads, device=dev, generator=g)
        o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
        dt, lse = torch.empty_like(table), torch.empty(B * heads * h * w, device=dev)
        d = lib.window_attention_desc(B, h, w, WS, SHIFT, heads)
        db = ctypes.byref(d)
        need = L.gs_window_attention_workspace_bytes(db)
        wsb = torch.empty(need, dtype=torch.uint8, device=dev)
        st = current_stream_ptr()

        def fwd():
            lib.check(L.gs_window_attention_forward(db, q.data_ptr(), k.data_ptr(), v.data_ptr(), table.data_ptr(),
                                                    o.data_ptr(), lse.data_ptr(), st), "fwd")

        def fwd_bwd():
            fwd()
            lib.check(L.gs_window_attention_backward(db, q.data_ptr(), k.data_ptr(), v.data_ptr(), table.data_ptr(),
                                                     o.data_ptr(), lse.data_ptr(), do.data_ptr(), dq.data_ptr(),
                                                     dk.data_ptr(), dv.data_ptr(), dt.data_ptr(), 0, wsb.data_ptr(),
                                                     need, st), "bwd")

        def bwd():
            lib.check(L.gs_window_attention_backward(db, q.data_ptr(), k.data_ptr(), v.data_ptr(), table.data_ptr(),
                                                     o.data_ptr(), lse.data_ptr(), do.data_ptr(), dq.data_ptr(),
                                                     dk.data_ptr(), dv.data_ptr(), dt.data_ptr(), 0, big_ws.data_ptr(),
                                                     big_ws.numel(), st), "bwd")

        def copy_floor():   # two copies = two reads + two writes of [rows][C]: the operator's 3 reads + 1 write
            for src, dst in ((q, o), (k, dq)):
                lib.check(L.gs_copy2d(src.data_ptr(), c, dst.data_ptr(), c, rows, c, 1.0, 0, st), "copy")

        mask, idx = torch_geometry(h, w, dev)
        tq, tk, tv, tt = (t.clone().requires_grad_(True) for t in (q, k, v, table))

        def torch_fwd():
            with torch.no_grad():
                torch_window_attention(tq, tk, tv, tt, mask, idx, h, w, heads)

        def torch_fwd_bwd():
            for t in (tq, tk, tv, tt):
                t.grad = None
            torch_window_attention(tq, tk, tv, tt, mask, idx, h, w, heads).backward(do)

        # the two implementations agree before they are timed
        fwd_bwd()
        torch_fwd_bwd()
        ref = torch_window_attention(tq, tk, tv, tt, mask, idx, h, w, heads).detach()
        err = {"O": float((o - ref).abs().max() / ref.abs().max()),
               "dQ": float((dq - tq.grad).abs().max() / tq.grad.abs().max()),
               "dTable": float((dt - tt.grad).abs().max() / tt.grad.abs().max())}
        res = {"shape": [B, h, w, heads], "slabs": need // (heads * (2 * WS - 1) ** 2 * 4),
               "fwd_ms": median_ms(fwd, args.iters, args.warmup),
               "fwd_bwd_ms": median_ms(fwd_bwd, args.iters, args.warmup),
               "torch_fwd_ms": median_ms(torch_fwd, args.iters, args.warmup),
               "torch_fwd_bwd_ms": median_ms(torch_fwd_bwd, args.iters, args.warmup),
               "copy_floor_ms": median_ms(copy_floor, args.iters, args.warmup), "vs_torch_err": err}
        # the backward alone at the plan and at forced splits, interleaved rounds in this one process
        items, plan = B * (h // WS) * (w // WS), res["slabs"]
        forced = sorted({1, max(1, plan // 4), max(1, plan // 2), plan, min(items, 2 * plan), min(items, 4 * plan),
                         items})
        big_ws = torch.empty(items * heads * (2 * WS - 1) ** 2 * 4 + 16, dtype=torch.uint8, device=dev)
        rounds = {s: [] for s in forced}
        try:
            for _ in range(5):
                for s in forced:
                    assert L.gs_debug_set_window_attention_split(s) == 0
                    rounds[s].append(median_ms(bwd, max(5, args.iters // 3), 2))
        finally:
            assert L.gs_debug_set_window_attention_split(-1) == 0
        res["bwd_ms_by_forced_split"] = {str(s): [round(min(t), 4), round(sorted(t)[len(t) // 2], 4)]
                                         for s, t in rounds.items()}   # [min, median] of five rounds
        res["fwd_over_floor"] = res["fwd_ms"] / res["copy_floor_ms"]
        res["fwd_not_slower_than_torch"] = res["fwd_ms"] <= res["torch_fwd_ms"]
        res["fwd_bwd_not_slower_than_torch"] = res["fwd_bwd_ms"] <= res["torch_fwd_bwd_ms"]
        print(json.dumps(res), flush=True)
    bench_map_ops(L, lib, current_stream_ptr(), args)


def bench_map_ops(L, lib, st, args):
    """the window pad / crop and the patch merging's cell LayerNorm at the stage-1 map of the same crop
    (B = 2, 256 x 128 -> 259 x 133, C = 128), beside a gs_copy2d of the same map"""
    dev, h, w, hp, wp, c = "cuda", 256, 128, 259, 133, 128
    g = torch.Generator(device=dev).manual_seed(2)
    x, dy = (torch.randn(B, h, w, c, device=dev, generator=g) for _ in range(2))
    big, y, dx = torch.empty(B, hp, wp, c, device=dev), torch.empty_like(x), torch.empty_like(x)
    wt, bs = torch.randn(4 * c, device=dev, generator=g), torch.randn(4 * c, device=dev, generator=g)
    dw, dbs = torch.empty_like(wt), torch.empty_like(bs)
    cells = B * h * w // 4
    stats = torch.empty(2 * cells, device=dev)
    d = lib.cell_layernorm_desc(B, h, w, c, c, 1e-5)
    db = ctypes.byref(d)
    need = L.gs_cell_layernorm_workspace_bytes(db)
    wsb = torch.empty(need, dtype=torch.uint8, device=dev)

    def pad():
        lib.check(L.gs_map_pad(x.data_ptr(), c, big.data_ptr(), c, B, h, w, hp, wp, c, 0, st), "pad")

    def crop():
        lib.check(L.gs_map_crop(big.data_ptr(), c, y.data_ptr(), c, B, h, w, hp, wp, c, 0, st), "crop")

    def cell_fwd():
        lib.check(L.gs_cell_layernorm_forward(db, x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(),
                                              stats.data_ptr(), stats.data_ptr() + 4 * cells, st), "cell fwd")

    def cell_bwd():
        lib.check(L.gs_cell_layernorm_backward(db, x.data_ptr(), dy.data_ptr(), wt.data_ptr(), stats.data_ptr(),
                                               stats.data_ptr() + 4 * cells, dx.data_ptr(), dw.data_ptr(),
                                               dbs.data_ptr(), 0, wsb.data_ptr(), need, st), "cell bwd")

    def copy():
        lib.check(L.gs_copy2d(x.data_ptr(), c, y.data_ptr(), c, B * h * w, c, 1.0, 0, st), "copy")

    cell_fwd()
    res = {"map_ops_shape": [B, h, w, c], "padded": [hp, wp]}
    for name, fn in (("pad_ms", pad), ("crop_ms", crop), ("cell_ln_fwd_ms", cell_fwd), ("cell_ln_bwd_ms", cell_bwd),
                     ("copy_ms", copy)):
        res[name] = median_ms(fn, args.iters, args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
