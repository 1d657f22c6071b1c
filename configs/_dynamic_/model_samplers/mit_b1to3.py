# Search space of the SegFormer (Mix Transformer) supernet and its train / val samplers.
# Per stage: depth, heads of width 64 (stage width = 64 x heads) and the Mix-FFN ratio (hidden width =
# ratio x width; integer ratios keep every hidden width a multiple of 4).
# Anchors: MIN (MiT-B1 depths 2/2/2/2 with fewer heads in stages 3 and 4 and smaller ratios), MID, MAX
# (MiT-B3: depths 3/4/18/3, heads 1/2/5/8, ratio 4).
_D = 'arch.backbone.body.depth'
_H = 'arch.backbone.body.num_heads'
_R = 'arch.backbone.body.mlp_ratio'
_product = lambda a, b, c, d: [[w, x, y, z] for w in a for x in b for y in c for z in d]  # noqa: E731


def _anchor(name, depth, heads, ratio):
    return {'name': name, _D: depth, _H: heads, _R: ratio}


_MIN = _anchor('MIN', [2, 2, 2, 2], [1, 2, 4, 6], [2, 2, 3, 3])
_MID = _anchor('MID', [2, 3, 10, 2], [1, 2, 5, 7], [3, 3, 4, 4])
_MAX = _anchor('MAX', [3, 4, 18, 3], [1, 2, 5, 8], [4, 4, 4, 4])

train_sampler = dict(
    type='concat',
    model_samplers=[
        dict(type='anchor', anchors=[_MAX, _MIN, _MID]),
        dict(type='repeat', times=2, model_sampler=dict(
            type='composite',
            model_samplers=[
                dict(type='candidate', key=_D,
                     candidates=_product([2, 3], [2, 3, 4], list(range(2, 19, 2)), [2, 3])),
                dict(type='candidate', key=_H, candidates=_product([1], [2], [4, 5], [6, 7, 8])),
                dict(type='candidate', key=_R, candidates=_product([2, 3, 4], [2, 3, 4], [3, 4], [3, 4]))])),
    ])
val_sampler = dict(type='anchor', anchors=[_MIN, _MID, _MAX])
