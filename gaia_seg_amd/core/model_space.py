"""Model samplers: the host-side mirror of ``gaiavision.model_space`` used by the supernet trainer.

The sampler classes are an absent dependency; their behaviour is reconstructed from the configs
that instantiate them (configs/_dynamic_/model_samplers/ar50to101v2.py:2-116) and the call sites
(tools/train_supernet.py:189-190 build; tools/extract_subnet.py:104-106 and
gaiaseg/core/evaluation/cross_arch_eval_hooks.py:53-59 ``traverse`` / ``anchor_name``) —
SURVEY.md Appendix A15.  A *meta* is a flat dict with dotted keys
(``'arch.backbone.body.width': [64,128,256,512]``); ``fold_dict`` turns it into the nested form
``manipulate_arch`` consumes.
"""
import copy
import json
import random

from .registry import Registry, build_from_cfg

MODEL_SAMPLERS = Registry("model sampler")


def build_model_sampler(cfg):
    return build_from_cfg(cfg, MODEL_SAMPLERS)


class BaseModelSampler:
    def __init__(self, mode="sample"):
        self.mode = mode
        self._rng = random

    def set_mode(self, mode):
        assert mode in ("sample", "traverse")
        self.mode = mode

    def seed(self, seed):
        """Private RNG stream (default: the global ``random`` module, seeded by --seed)."""
        self._rng = random.Random(seed)
        for child in self.children():
            child.seed(self._rng.randrange(1 << 30))

    def children(self):
        return []

    def sample(self):
        raise NotImplementedError

    def traverse(self):
        raise NotImplementedError

    def __call__(self):
        return self.sample() if self.mode == "sample" else self.traverse()


@MODEL_SAMPLERS.register_module("anchor")
class AnchorSampler(BaseModelSampler):
    """anchors: list of metas. sample() = one uniformly; traverse() = all, in order."""

    def __init__(self, anchors, **kw):
        super().__init__(**kw)
        self.anchors = [dict(a) for a in anchors]

    def sample(self):
        return copy.deepcopy(self._rng.choice(self.anchors))

    def traverse(self):
        return copy.deepcopy(self.anchors)

    def anchor_name(self, idx):
        return self.anchors[idx].get("name", str(idx))

    def __len__(self):
        return len(self.anchors)


def _grid(start, end, step):
    vals, v = [], start
    while v <= end:
        vals.append(v)
        v += step
    return vals


@MODEL_SAMPLERS.register_module("range")
class RangeSampler(BaseModelSampler):
    """Uniform draw on {start, start+step, .., end}; per-element for list-valued ranges;
    ascending=True keeps the elements non-decreasing (redraw until satisfied)."""

    def __init__(self, key, start, end, step, ascending=False, **kw):
        super().__init__(**kw)
        self.key, self.start, self.end, self.step = key, start, end, step
        self.ascending = ascending
        self.is_list = isinstance(start, (list, tuple))
        if self.is_list:
            assert len(start) == len(end) == len(step)

    def _draw(self):
        if not self.is_list:
            return self._rng.choice(_grid(self.start, self.end, self.step))
        return [self._rng.choice(_grid(s, e, st)) for s, e, st in zip(self.start, self.end, self.step)]

    def sample(self):
        v = self._draw()
        if self.ascending and self.is_list:
            for _ in range(1000):
                if all(a <= b for a, b in zip(v, v[1:])):
                    break
                v = self._draw()
            else:
                v = sorted(v)
        return {self.key: v}

    def traverse(self):
        if not self.is_list:
            return [{self.key: v} for v in _grid(self.start, self.end, self.step)]
        out = [[]]
        for s, e, st in zip(self.start, self.end, self.step):
            out = [o + [v] for o in out for v in _grid(s, e, st)]
        if self.ascending:
            out = [o for o in out if all(a <= b for a, b in zip(o, o[1:]))]
        return [{self.key: o} for o in out]


@MODEL_SAMPLERS.register_module("candidate")
class CandidateSampler(BaseModelSampler):
    def __init__(self, key, candidates, **kw):
        super().__init__(**kw)
        self.key, self.candidates = key, list(candidates)

    def sample(self):
        return {self.key: copy.deepcopy(self._rng.choice(self.candidates))}

    def traverse(self):
        return [{self.key: copy.deepcopy(c)} for c in self.candidates]


class _Container(BaseModelSampler):
    def __init__(self, model_samplers, **kw):
        super().__init__(**kw)
        self.model_samplers = [build_model_sampler(c) if isinstance(c, dict) else c
                               for c in model_samplers]

    def children(self):
        return self.model_samplers

    def set_mode(self, mode):
        super().set_mode(mode)
        for c in self.model_samplers:
            c.set_mode(mode)


@MODEL_SAMPLERS.register_module("composite")
class CompositeSampler(_Container):
    """One draw of every child merged into one meta."""

    def sample(self):
        meta = {}
        for c in self.model_samplers:
            meta.update(c.sample())
        return meta

    def traverse(self):
        out = [{}]
        for c in self.model_samplers:
            out = [dict(o, **m) for o in out for m in c.traverse()]
        return out


@MODEL_SAMPLERS.register_module("concat")
class ConcatSampler(_Container):
    """Union of the children's candidates.  sample() returns the LIST of candidate metas of this
    step (every anchor + one draw of each random child), from which the hook picks one."""

    def candidates(self):
        out = []
        for c in self.model_samplers:
            if isinstance(c, AnchorSampler):
                out.extend(c.traverse())
            else:
                m = c.sample()
                out.extend(m if isinstance(m, list) else [m])
        return out

    def sample(self):
        return self._rng.choice(self.candidates())

    def traverse(self):
        out = []
        for c in self.model_samplers:
            out.extend(c.traverse())
        return out


@MODEL_SAMPLERS.register_module("repeat")
class RepeatSampler(BaseModelSampler):
    """``times`` independent draws of the wrapped sampler."""

    def __init__(self, times, model_sampler, **kw):
        super().__init__(**kw)
        self.times = times
        self.model_sampler = (build_model_sampler(model_sampler)
                              if isinstance(model_sampler, dict) else model_sampler)

    def children(self):
        return [self.model_sampler]

    def sample(self):
        return [self.model_sampler.sample() for _ in range(self.times)]

    def traverse(self):
        return self.model_sampler.traverse()


def arch_key(meta):
    """Hashable identity of the architecture part of a meta (cache key for plans / graphs)."""
    def freeze(v):
        if isinstance(v, (list, tuple)):
            return tuple(freeze(x) for x in v)
        if isinstance(v, dict):
            return tuple(sorted((k, freeze(x)) for k, x in v.items()))
        return v
    return tuple(sorted((k, freeze(v)) for k, v in meta.items() if k.startswith("arch")))


# ------------------------------------------------------------------------------------------------
# Model-space files and sampling rules (tools/test_supernet.py)
#
# A reconstruction: gaiavision's ``ModelSpaceManager`` / ``build_sample_rule`` are absent
# dependencies.  Their behaviour is restated from what the reference's configs and tools ask of them
# (``model_space_path`` + ``model_sampling_rules`` of the test configs, tools/test_supernet.py's
# ``ModelSpaceManager.load(path).ms_manager.apply_rule(rule).pack()``), with the semantics below
# (DESIGN.md section 16):
#   * a model-space file is a JSON list of flat metas with dotted keys (what tools/count_flops.py
#     writes) or the same metas as JSON lines; lists become tuples before any rule sees them;
#   * the rules work on a list of GROUPS (lists of rows), starting from one group of every row;
#   * filter (``func_str``; no type or type='eval'): keep the rows of each group the lambda accepts;
#   * 'sequential': its ``rules`` in order;  'parallel': every sub-rule on every input group, one
#     output group per (input group, sub-rule), input-group-major;
#   * 'sample': per group, ``operation`` 'random' (a draw from random.Random(seed, group index):
#     identical on every rank and every call) or 'top' (sorted by ``key``, largest first), of
#     ``value`` rows (mode 'number') or int(value * len(group)) rows (mode 'ratio'); the
#     rows keep the drawn / sorted order;
#   * 'merge': the groups concatenated in order, later duplicates (same arch_key) dropped: one group.
# ------------------------------------------------------------------------------------------------


def _tuplify(v):
    if isinstance(v, (list, tuple)):
        return tuple(_tuplify(x) for x in v)
    if isinstance(v, dict):
        return {k: _tuplify(x) for k, x in v.items()}
    return v


def _listify(v):
    if isinstance(v, (list, tuple)):
        return [_listify(x) for x in v]
    if isinstance(v, dict):
        return {k: _listify(x) for k, x in v.items()}
    return v


def load_model_space(path):
    """Rows of a model-space file (JSON list or JSON lines) with list values as tuples."""
    with open(path) as fh:
        text = fh.read()
    if text.lstrip().startswith("["):
        rows = json.loads(text)
    else:
        rows = [json.loads(line) for line in text.splitlines() if line.strip()]
    for i, r in enumerate(rows):
        if not isinstance(r, dict):
            raise ValueError("%s: row %d is a %s, not a flat meta" % (path, i, type(r).__name__))
    return [_tuplify(r) for r in rows]


def dump_model_space(rows, path):
    """Write rows as a JSON list (tools/count_flops.py's format); tuples are written as lists."""
    with open(path, "w") as fh:
        json.dump([_listify(r) for r in rows], fh, indent=1)


class ModelSpace:
    """The rows of a model space; ``apply_rule`` narrows them, ``pack`` hands them to the model."""

    def __init__(self, rows):
        self.rows = [_tuplify(dict(r)) for r in rows]

    @classmethod
    def load(cls, path):
        return cls(load_model_space(path))

    def dump(self, path):
        dump_model_space(self.rows, path)

    def apply_rule(self, rule):
        if isinstance(rule, dict):
            rule = build_sample_rule(rule)
        groups = rule([list(self.rows)])
        return ModelSpace([r for g in groups for r in g])

    def pack(self):
        """The nested arch of every row, the form ``manipulate_arch`` takes (fold_dict(meta)['arch'])."""
        from .dynamic import fold_dict
        return [_listify(fold_dict(r).get("arch", {})) for r in self.rows]

    def __len__(self):
        return len(self.rows)

    def __iter__(self):
        return iter(self.rows)


class _FilterRule:
    def __init__(self, func_str):
        self.func_str = func_str
        self.fn = eval(func_str, {"__builtins__": __builtins__}, {})  # config text, like the config
        if not callable(self.fn):
            raise ValueError("func_str must evaluate to a callable, got %r" % (func_str,))

    def __call__(self, groups):
        return [[r for r in g if self.fn(r)] for g in groups]


class _SequentialRule:
    def __init__(self, rules):
        self.rules = [build_sample_rule(r) for r in rules]

    def __call__(self, groups):
        for r in self.rules:
            groups = r(groups)
        return groups


class _ParallelRule:
    def __init__(self, rules):
        self.rules = [build_sample_rule(r) for r in rules]

    def __call__(self, groups):
        out = []
        for g in groups:
            for r in self.rules:
                out.extend(r([list(g)]))
        return out


class _SampleRule:
    def __init__(self, operation, value, mode="number", key=None, seed=0, func_str=None):
        if operation not in ("random", "top"):
            raise ValueError("sample: operation must be 'random' or 'top', got %r" % (operation,))
        if mode not in ("number", "ratio"):
            raise ValueError("sample: mode must be 'number' or 'ratio', got %r" % (mode,))
        if operation == "top" and key is None:
            raise ValueError("sample: operation='top' needs a key")
        self.operation, self.value, self.mode, self.key, self.seed = operation, value, mode, key, seed
        self.filter = _FilterRule(func_str) if func_str else None

    def _count(self, n):
        k = int(self.value) if self.mode == "number" else int(self.value * n)
        return max(0, min(n, k))

    def __call__(self, groups):
        if self.filter is not None:
            groups = self.filter(groups)
        out = []
        for gi, g in enumerate(groups):
            k = self._count(len(g))
            if self.operation == "random":
                out.append(random.Random(self.seed * 1000003 + gi).sample(list(g), k))
            else:
                out.append(sorted(g, key=lambda r: r[self.key], reverse=True)[:k])
        return out


class _MergeRule:
    def __call__(self, groups):
        seen, out = set(), []
        for g in groups:
            for r in g:
                k = arch_key(r)
                if k not in seen:
                    seen.add(k)
                    out.append(r)
        return [out]


def build_sample_rule(cfg):
    """A callable list-of-groups -> list-of-groups from a rule config (see the section comment)."""
    if callable(cfg) and not isinstance(cfg, dict):
        return cfg
    cfg = dict(cfg)
    t = cfg.pop("type", None)
    if t is None or t == "eval":
        if set(cfg) != {"func_str"}:
            raise ValueError("a filter rule takes exactly func_str, got %s" % sorted(cfg))
        return _FilterRule(cfg["func_str"])
    if t == "sequential":
        return _SequentialRule(cfg.pop("rules"))
    if t == "parallel":
        return _ParallelRule(cfg.pop("rules"))
    if t == "sample":
        return _SampleRule(**cfg)
    if t == "merge":
        if cfg:
            raise ValueError("merge takes no options, got %s" % sorted(cfg))
        return _MergeRule()
    raise ValueError("unknown model-sampling rule type %r (have eval, sequential, parallel, sample, "
                     "merge)" % (t,))


# ------------------------------------------------------------------------------------------------
# data.input_shape: the third elastic dimension
#
# A reconstruction: gaiavision's ``ScaleManipulator`` is an absent dependency and the reference has
# its calls commented out.  The value forms are the ones the reference writes down: the scale
# sampler's ints (a short side, configs/_dynamic_/model_samplers/ar50to101v2_scale.py), the
# ``x['data.input_shape'][-1] == 800`` of its rules (a sequence ending in H, W) and the string
# "3,800,800" that its tools/count_flops.py accepts.
# ------------------------------------------------------------------------------------------------


def _positive_int(x, v):
    if isinstance(x, bool) or not isinstance(x, int) or x <= 0:
        raise ValueError("data.input_shape=%r: sizes must be positive integers" % (v,))
    return x


def parse_input_shape(v):
    """A meta's ``data.input_shape`` value -> ('short', S) or ('exact', H, W); ValueError otherwise.

    An int S is a short side; a sequence (H, W) or (C, H, W) with C == 3, or the same as a
    comma-separated string, is an exact target."""
    if isinstance(v, str):
        try:
            v = tuple(int(p) for p in v.split(","))
        except ValueError:
            raise ValueError("data.input_shape=%r: a string must be comma-separated integers" % (v,))
        if len(v) == 1:
            raise ValueError("data.input_shape=%r: a string names (H, W) or (C, H, W)" % (v,))
    if isinstance(v, (list, tuple)):
        if len(v) not in (2, 3):
            raise ValueError("data.input_shape=%r: a sequence must be (H, W) or (C, H, W)" % (v,))
        if len(v) == 3 and (isinstance(v[0], bool) or v[0] != 3):
            raise ValueError("data.input_shape=%r: C must be 3" % (v,))
        return ("exact", _positive_int(v[-2], v), _positive_int(v[-1], v))
    return ("short", _positive_int(v, v))


def resolve_input_shape(v, h, w):
    """The size (H, W) a batch of size (h, w) takes under ``data.input_shape = v``.

    int S: the short side becomes S and the long side floor(S * long / short + 0.5) (integer
    arithmetic, so the result does not depend on floating-point rounding); a sequence or string:
    exactly its last two entries, the aspect ratio is not kept.  The caller passes the batch through
    when the result equals (h, w).  Anything else raises ValueError."""
    parsed = parse_input_shape(v)
    if parsed[0] == "exact":
        return parsed[1], parsed[2]
    s = parsed[1]
    if h <= 0 or w <= 0:
        raise ValueError("resolve_input_shape: batch size (%r, %r) must be positive" % (h, w))
    short, long_ = min(h, w), max(h, w)
    scaled = (2 * s * long_ + short) // (2 * short)     # floor(S * long / short + 0.5)
    return (s, scaled) if h <= w else (scaled, s)
