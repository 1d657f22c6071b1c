"""``optimizer.paramwise_cfg`` -> parameter groups for the flat-arena SGD.

``build_param_groups`` restates the grouping rule of mmcv 1.3.0's
``DefaultOptimizerConstructor.add_params`` (mmcv/runner/optimizer/default_constructor.py).  mmcv is
not part of this tree, so the rule is a reconstruction from its documented behaviour:

  * ``custom_keys``: keys sorted alphabetically, then by length, longest first; the first key that is
    a SUBSTRING of the parameter's full name wins: lr = base_lr * lr_mult, weight_decay = base_wd *
    decay_mult (both default 1).  A custom match overrides every rule below.
  * otherwise a parameter named ``bias`` outside a norm module gets ``bias_lr_mult``; for the decay,
    in this order, parameters of a norm module (weight and bias) get ``norm_decay_mult``, else a
    parameter named ``bias`` gets ``bias_decay_mult``.
  * ``dwconv_decay_mult`` / ``bypass_duplicate`` are accepted without effect (no depthwise
    convolutions, no shared parameters here); ``dcn_offset_lr_mult`` is refused (so is DCN).
  * parameters with ``requires_grad=False`` are in no group (torch.optim.SGD never steps them).

One group per distinct (lr_mult, decay_mult) pair, group 0 being (1, 1).  The rest of the module is
the host arithmetic that turns groups into the chunk table of ``gs_sgd_step_groups``: the arena is
in forward order, so BatchNorm parameters in a group of their own cut a subnet's few merged ranges
into many fragments (84-294 for the anchors of the in-tree supernets), which one table-driven launch
covers.  Nothing here needs a GPU.
"""
import bisect
from collections import OrderedDict

import numpy as np
from torch import nn
from torch.nn.modules.batchnorm import _BatchNorm
from torch.nn.modules.instancenorm import _InstanceNorm

MAX_GROUPS = 16           # GS_SGD_MAX_GROUPS (include/gaiaseg_hip.h)
# floats per chunk of the table: the fastest of 4 K / 16 K / 64 K on the MI355X
# (tools/bench_paramwise.py, profiles/r06_paramwise_sgd.md)
CHUNK_FLOATS = 4096

OPTIMIZER_KEYS = ("type", "lr", "momentum", "weight_decay", "paramwise_cfg")
# keys of torch.optim.SGD that are accepted only with torch's default (nothing else is implemented)
OPTIMIZER_DEFAULTS = {"nesterov": False, "dampening": 0}
PARAMWISE_KEYS = ("custom_keys", "bias_lr_mult", "bias_decay_mult", "norm_decay_mult",
                  "dwconv_decay_mult", "bypass_duplicate", "dcn_offset_lr_mult")
_NORMS = (_BatchNorm, _InstanceNorm, nn.GroupNorm, nn.LayerNorm)


def check_optimizer_cfg(optimizer_cfg):
    """Refuse what the arena SGD would otherwise drop in silence.  Returns the plain dict."""
    opt = dict(optimizer_cfg)
    if opt.get("type", "SGD") != "SGD":
        raise NotImplementedError("only SGD (the in-tree config) has a fused arena kernel")
    for k, v in opt.items():
        if k in OPTIMIZER_KEYS:
            continue
        if k in OPTIMIZER_DEFAULTS:
            if v != OPTIMIZER_DEFAULTS[k]:
                raise NotImplementedError("optimizer.%s=%r: only torch's default %r is implemented"
                                          % (k, v, OPTIMIZER_DEFAULTS[k]))
            continue
        raise KeyError("optimizer: unknown key %r (have %s)"
                       % (k, sorted(OPTIMIZER_KEYS + tuple(OPTIMIZER_DEFAULTS))))
    return opt


class ParamGroups:
    """``groups``: [(lr_mult, decay_mult)], group 0 = (1, 1); ``index``: {parameter name: group}
    over the trainable parameters."""

    def __init__(self, groups, index):
        self.groups, self.index = list(groups), dict(index)

    def __len__(self):
        return len(self.groups)

    def lrs(self, base_lr):
        return [base_lr * lm for lm, _ in self.groups]

    def weight_decays(self, base_wd):
        return [base_wd * dm for _, dm in self.groups]

    def members(self, g):
        return [n for n, i in self.index.items() if i == g]


def param_multipliers(model, paramwise_cfg):
    """{parameter name: (lr_mult, decay_mult)} over the trainable parameters, in named_parameters
    order: the rule of the module docstring."""
    pw = dict(paramwise_cfg or {})
    unknown = set(pw) - set(PARAMWISE_KEYS)
    if unknown:
        raise KeyError("paramwise_cfg: unknown keys %s (have %s)" % (sorted(unknown), sorted(PARAMWISE_KEYS)))
    if "dcn_offset_lr_mult" in pw:
        raise NotImplementedError("paramwise_cfg.dcn_offset_lr_mult: deformable convolutions are not "
                                  "implemented")
    custom = pw.get("custom_keys") or {}
    if not isinstance(custom, dict):
        raise TypeError("paramwise_cfg.custom_keys must be a dict, got %s" % type(custom).__name__)
    for key, val in custom.items():
        bad = set(val) - {"lr_mult", "decay_mult"}
        if bad:
            raise KeyError("paramwise_cfg.custom_keys[%r]: unknown keys %s" % (key, sorted(bad)))
    sorted_keys = sorted(sorted(custom), key=len, reverse=True)
    bias_lr = float(pw.get("bias_lr_mult", 1.))
    bias_decay = float(pw.get("bias_decay_mult", 1.))
    norm_decay = float(pw.get("norm_decay_mult", 1.))
    out = {}
    for prefix, module in model.named_modules():
        is_norm = isinstance(module, _NORMS)
        for name, p in module.named_parameters(recurse=False):
            full = "%s.%s" % (prefix, name) if prefix else name
            if not p.requires_grad or full in out:
                continue
            for key in sorted_keys:
                if key in full:
                    out[full] = (float(custom[key].get("lr_mult", 1.)),
                                 float(custom[key].get("decay_mult", 1.)))
                    break
            else:
                lr_mult = bias_lr if name == "bias" and not is_norm else 1.
                decay_mult = norm_decay if is_norm else bias_decay if name == "bias" else 1.
                out[full] = (lr_mult, decay_mult)
    order = {n: i for i, (n, _) in enumerate(model.named_parameters())}
    return dict(sorted(out.items(), key=lambda kv: order[kv[0]]))


def build_param_groups(model, optimizer_cfg):
    """``cfg.optimizer`` -> ParamGroups, or None when there is no ``paramwise_cfg`` or it yields the
    single group (1, 1): the runner then takes the ungrouped path, launch for launch what it is
    without this module."""
    opt = check_optimizer_cfg(optimizer_cfg)
    if opt.get("paramwise_cfg") is None:
        return None
    mults = param_multipliers(model, opt["paramwise_cfg"])
    groups, index = [(1., 1.)], {}
    for name, pair in mults.items():
        if pair not in groups:
            groups.append(pair)
        index[name] = groups.index(pair)
    if len(groups) > MAX_GROUPS:
        raise ValueError("paramwise_cfg yields %d parameter groups; at most %d (GS_SGD_MAX_GROUPS)"
                         % (len(groups), MAX_GROUPS))
    if len(groups) == 1:
        return None
    return ParamGroups(groups, index)


# ---- arena arithmetic: segments -> fragments -> chunk table ----
def segment_groups(layout, index, align=64):
    """[(begin, end, group)] per arena segment in arena order from ``arena_layout``'s list and
    {name: group}; a parameter without a group (frozen) gets -1."""
    segs = []
    for name, _p, _phys, off, n in layout:
        padded = -(-max(n, 1) // align) * align
        segs.append((off, off + padded, index.get(name, -1)))
    return segs


def group_fragments(ranges, segs, starts=None):
    """Cut sorted disjoint [begin, end) ``ranges`` (whole segments) at every change of group:
    [(begin, end, group)] with neighbours of one group merged.  A range that covers a segment without
    a group is an error (a frozen parameter must not be stepped)."""
    if starts is None:
        starts = [s[0] for s in segs]
    out, cur = [], None
    for lo, hi in ranges:
        i = bisect.bisect_left(starts, lo)
        if i == len(segs) or segs[i][0] != lo:
            raise ValueError("range [%d, %d) does not begin at a segment" % (lo, hi))
        while i < len(segs) and segs[i][0] < hi:
            b, e, g = segs[i]
            if e > hi:
                raise ValueError("range [%d, %d) ends inside a segment" % (lo, hi))
            if g < 0:
                raise ValueError("the segment at %d has no parameter group (frozen?) but is stepped" % b)
            if cur is not None and cur[2] == g and cur[1] == b:
                cur[1] = e
            else:
                cur = [b, e, g]
                out.append(cur)
            i += 1
    return [tuple(f) for f in out]


def chunk_table(fragments, chunk_floats=CHUNK_FLOATS):
    """int32 array [n_chunks, 4] of {begin, length, group, 0} in units of 4 floats: every fragment cut
    into chunks of at most ``chunk_floats`` floats (GsSgdChunk, include/gaiaseg_hip.h)."""
    if chunk_floats <= 0 or chunk_floats % 4:
        raise ValueError("chunk_floats must be a positive multiple of 4, got %r" % (chunk_floats,))
    if not fragments:
        return np.zeros((0, 4), dtype=np.int32)
    fr = np.asarray(fragments, dtype=np.int64)
    if (fr[:, :2] % 4).any():
        raise ValueError("fragments must begin and end at multiples of 4 floats")
    begin, length, group = fr[:, 0], fr[:, 1] - fr[:, 0], fr[:, 2]
    per = -(-length // chunk_floats)
    which = np.repeat(np.arange(len(fr)), per)
    first = np.cumsum(per) - per
    k = np.arange(per.sum()) - first[which]                  # chunk number inside its fragment
    cb = begin[which] + k * chunk_floats
    cl = np.minimum(chunk_floats, begin[which] + length[which] - cb)
    if cb.size and (cb + cl).max() // 4 >= 2 ** 31:
        raise ValueError("arena too large for 32-bit chunk offsets")
    tab = np.zeros((len(cb), 4), dtype=np.int32)
    tab[:, 0], tab[:, 1], tab[:, 2] = cb // 4, cl // 4, group[which]
    return tab


class ChunkTableCache:
    """{set of ranges: (table, chunks, fragments)} under one grouping, least recently used entries
    evicted ONE AT A TIME beyond ``max_entries``.  ``upload`` turns the int32 array into what the
    caller launches with (ParamArena: a device tensor; identity here, so this runs without a GPU).
    The cache is only a cache: whoever keeps a launch that names a table alive beyond the call -- a
    captured step graph -- must hold the table it was handed (IterBasedRunner keeps them in the graph
    entry), so an eviction never frees memory a live graph reads.  An entry just inserted or just
    fetched is the newest, so preparing a subnet's few tables never evicts one of them."""

    def __init__(self, segs, chunk_floats=CHUNK_FLOATS, upload=None, max_entries=512, numel=None):
        if max_entries < 8:
            raise ValueError("max_entries must be at least 8 (a subnet prepares three tables)")
        self.segs, self.starts = list(segs), [s[0] for s in segs]
        self.chunk_floats, self.upload, self.max_entries = chunk_floats, upload, max_entries
        self.numel = numel if numel is not None else (self.segs[-1][1] if self.segs else 0)
        self.entries = OrderedDict()

    def __len__(self):
        return len(self.entries)

    def __contains__(self, ranges):
        return tuple(ranges) in self.entries

    def get(self, ranges, build=True):
        key = tuple(ranges)
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            return hit
        if not build:
            raise KeyError("no chunk table was prepared for these ranges")
        frags = group_fragments(key, self.segs, self.starts)
        tab = chunk_table(frags, self.chunk_floats)
        # bounds, on the host, before anything can be launched with the table
        if len(tab) and int((tab[:, 0].astype(np.int64) + tab[:, 1]).max()) * 4 > self.numel:
            raise ValueError("chunk table leaves the arena")
        dev = None if not len(tab) else tab if self.upload is None else self.upload(tab)
        hit = self.entries[key] = (dev, len(tab), len(frags))
        while len(self.entries) > self.max_entries:
            self.entries.popitem(last=False)
        return hit
