"""``cfg.optimizer`` (SGD or AdamW) and its ``paramwise_cfg`` -> parameter groups and chunk tables for the
flat-arena optimizer kernels (DESIGN.md sections 18 and 29).

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
covers.  AdamW (``gs_adamw_step_groups``) takes the same tables cut PER PARAMETER, each chunk with the
slot of its parameter's step counter in column 3.  Nothing here needs a GPU.
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
# torch.optim.AdamW: its own keys, its defaults, SGD's keys (refused by name) and the switches that
# are accepted only at a value that changes nothing (``foreach`` / ``fused`` / ``capturable`` choose
# between torch implementations of the same update; the arena kernel is the only one here)
ADAMW_KEYS = ("type", "lr", "betas", "eps", "weight_decay", "paramwise_cfg", "constructor")
ADAMW_DEFAULTS = {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01}
ADAMW_SGD_ONLY = ("momentum", "nesterov", "dampening")
ADAMW_NEUTRAL = {"amsgrad": (False,), "maximize": (False,), "foreach": (None, False, True),
                 "capturable": (False, True), "fused": (None, False, True)}
PARAMWISE_KEYS = ("custom_keys", "bias_lr_mult", "bias_decay_mult", "norm_decay_mult",
                  "dwconv_decay_mult", "bypass_duplicate", "dcn_offset_lr_mult")
_NORMS = (_BatchNorm, _InstanceNorm, nn.GroupNorm, nn.LayerNorm)


def check_optimizer_cfg(optimizer_cfg):
    """Refuse what the arena optimizers would otherwise drop in silence.  Returns the plain dict; for
    ``type='AdamW'`` with torch.optim.AdamW's defaults filled in (betas, eps, weight_decay 0.01)."""
    opt = dict(optimizer_cfg)
    kind = opt.get("type", "SGD")
    if kind == "AdamW":
        return _check_adamw_cfg(opt)
    if kind != "SGD":
        raise NotImplementedError("optimizer.type=%r: only SGD and AdamW have a fused arena kernel"
                                  % (kind,))
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


def _check_adamw_cfg(opt):
    if opt.get("constructor", "DefaultOptimizerConstructor") != "DefaultOptimizerConstructor":
        raise NotImplementedError("optimizer.constructor=%r: only mmcv's DefaultOptimizerConstructor; "
                                  "layer-wise lr decay constructors are not implemented"
                                  % (opt["constructor"],))
    for k, v in opt.items():
        if k in ADAMW_KEYS:
            continue
        if k in ADAMW_SGD_ONLY:
            raise NotImplementedError("optimizer.%s is a key of SGD: AdamW does not take it" % k)
        if k in ADAMW_NEUTRAL:
            if v not in ADAMW_NEUTRAL[k]:
                raise NotImplementedError("optimizer.%s=%r is not implemented for AdamW (only %s)"
                                          % (k, v, " / ".join(repr(x) for x in ADAMW_NEUTRAL[k])))
            continue
        raise KeyError("optimizer: unknown key %r for AdamW (have %s)"
                       % (k, sorted(ADAMW_KEYS + tuple(ADAMW_NEUTRAL))))
    if "lr" not in opt:
        raise KeyError("optimizer: AdamW needs lr")
    betas = opt.get("betas", ADAMW_DEFAULTS["betas"])
    if not isinstance(betas, (tuple, list)) or len(betas) != 2:
        raise ValueError("optimizer.betas must be a pair, got %r" % (betas,))
    for i, b in enumerate(betas):
        if not 0.0 <= b < 1.0:
            raise ValueError("optimizer.betas[%d]=%r is outside [0, 1)" % (i, b))
    eps = opt.get("eps", ADAMW_DEFAULTS["eps"])
    if not eps > 0.0:
        raise ValueError("optimizer.eps=%r must be > 0" % (eps,))
    wd = opt.get("weight_decay", ADAMW_DEFAULTS["weight_decay"])
    if not wd >= 0.0:
        raise ValueError("optimizer.weight_decay=%r must be >= 0" % (wd,))
    opt.pop("constructor", None)
    opt.update(betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=wd)
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
    """``cfg.optimizer`` -> ParamGroups.  SGD: None when there is no ``paramwise_cfg`` or it yields the
    single group (1, 1): the runner then takes the ungrouped path, launch for launch what it is
    without this module.  AdamW: always groups, the single group (1, 1) over every trainable parameter
    included -- its kernel has the table-driven path only (every chunk needs its parameter's counter)."""
    opt = check_optimizer_cfg(optimizer_cfg)
    adamw = opt.get("type", "SGD") == "AdamW"
    if opt.get("paramwise_cfg") is None and not adamw:
        return None
    mults = param_multipliers(model, opt.get("paramwise_cfg"))
    groups, index = [(1., 1.)], {}
    for name, pair in mults.items():
        if pair not in groups:
            groups.append(pair)
        index[name] = groups.index(pair)
    if len(groups) > MAX_GROUPS:
        raise ValueError("paramwise_cfg yields %d parameter groups; at most %d (GS_SGD_MAX_GROUPS)"
                         % (len(groups), MAX_GROUPS))
    if len(groups) == 1 and not adamw:
        return None
    return ParamGroups(groups, index)


# ---- arena arithmetic: segments -> fragments -> chunk table ----
def segment_groups(layout, index, align=64, per_param=False):
    """[(begin, end, group)] per arena segment in arena order from ``arena_layout``'s list and
    {name: group}; a parameter without a group (frozen) gets -1.  ``per_param`` (AdamW): a fourth
    column, the parameter's SLOT -- its position in ``layout``, which indexes the step counters."""
    segs = []
    for slot, (name, _p, _phys, off, n) in enumerate(layout):
        padded = -(-max(n, 1) // align) * align
        seg = (off, off + padded, index.get(name, -1))
        segs.append(seg + (slot,) if per_param else seg)
    return segs


def group_fragments(ranges, segs, starts=None):
    """Cut sorted disjoint [begin, end) ``ranges`` (whole segments) at every change of group:
    [(begin, end, group)] with neighbours of one group merged.  A range that covers a segment without
    a group is an error (a frozen parameter must not be stepped).  With per-parameter segments
    (``segment_groups(per_param=True)``) the cut is at EVERY parameter boundary, nothing is merged and
    the fragments are (begin, end, group, slot)."""
    if starts is None:
        starts = [s[0] for s in segs]
    out, cur = [], None
    for lo, hi in ranges:
        i = bisect.bisect_left(starts, lo)
        if i == len(segs) or segs[i][0] != lo:
            raise ValueError("range [%d, %d) does not begin at a segment" % (lo, hi))
        while i < len(segs) and segs[i][0] < hi:
            b, e, g = segs[i][:3]
            if e > hi:
                raise ValueError("range [%d, %d) ends inside a segment" % (lo, hi))
            if g < 0:
                raise ValueError("the segment at %d has no parameter group (frozen?) but is stepped" % b)
            if len(segs[i]) == 4:
                out.append(list(segs[i]))
            elif cur is not None and cur[2] == g and cur[1] == b:
                cur[1] = e
            else:
                cur = [b, e, g]
                out.append(cur)
            i += 1
    return [tuple(f) for f in out]


def chunk_table(fragments, chunk_floats=CHUNK_FLOATS):
    """int32 array [n_chunks, 4] of {begin, length, group, slot} in units of 4 floats: every fragment
    cut into chunks of at most ``chunk_floats`` floats (GsSgdChunk, include/gaiaseg_hip.h).  Column 3
    is 0 for (begin, end, group) fragments (SGD) and the parameter's slot for per-parameter
    (begin, end, group, slot) fragments (AdamW: a chunk never spans two parameters, and one
    parameter's chunks are contiguous)."""
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
    if fr.shape[1] == 4:
        tab[:, 3] = fr[:, 3][which]
    return tab


class ChunkTableCache:
    """{set of ranges: (table, chunks, fragments)} under one grouping, least recently used entries
    evicted ONE AT A TIME beyond ``max_entries``.  ``upload`` turns the int32 array into what the
    caller launches with (ParamArena: a device tensor; identity here, so this runs without a GPU).
    The cache is only a cache: whoever keeps a launch that names a table alive beyond the call -- a
    captured step graph -- must hold the table it was handed (IterBasedRunner keeps them in the graph
    entry), so an eviction never frees memory a live graph reads.  An entry just inserted or just
    fetched is the newest, so preparing a subnet's few tables never evicts one of them."""

    def __init__(self, segs, chunk_floats=CHUNK_FLOATS, upload=None, max_entries=512, numel=None,
                 n_slots=None):
        if max_entries < 8:
            raise ValueError("max_entries must be at least 8 (a subnet prepares three tables)")
        self.segs, self.starts = list(segs), [s[0] for s in segs]
        self.chunk_floats, self.upload, self.max_entries = chunk_floats, upload, max_entries
        self.numel = numel if numel is not None else (self.segs[-1][1] if self.segs else 0)
        # per-parameter tables (AdamW): the number of step counters column 3 may index
        self.n_slots = n_slots if n_slots is not None else len(self.segs)
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
        if len(tab) and not (0 <= int(tab[:, 3].min()) and int(tab[:, 3].max()) < max(self.n_slots, 1)):
            raise ValueError("chunk table names a step counter outside [0, %d)" % self.n_slots)
        dev = None if not len(tab) else tab if self.upload is None else self.upload(tab)
        hit = self.entries[key] = (dev, len(tab), len(frags))
        while len(self.entries) > self.max_entries:
            self.entries.popitem(last=False)
        return hit
