# Search space of the Swin supernet and its train / val samplers.
# Per stage: depth, heads of width 32 (stage width = 32 x heads) and the MLP ratio (hidden width = ratio x width;
# the ratios below keep every hidden width a multiple of 4).
# Anchors: MIN (Swin-T: depths 2/2/6/2, heads 3/6/12/24), MID, MAX (Swin-B: depths 2/2/18/2, heads 4/8/16/32).
_D = 'arch.backbone.body.depth'
_H = 'arch.backbone.body.num_heads'
_R = 'arch.backbone.body.mlp_ratio'
_product = lambda a, b, c, d: [[w, x, y, z] for w in a for x in b for y in c for z in d]  # noqa: E731


def _anchor(name, depth, heads, ratio):
    return {'name': name, _D: depth, _H: heads, _R: ratio}


_MIN = _anchor('MIN', [2, 2, 6, 2], [3, 6, 12, 24], [4, 4, 4, 4])
_MID = _anchor('MID', [2, 2, 12, 2], [3, 7, 14, 28], [4, 4, 3, 3])
_MAX = _anchor('MAX', [2, 2, 18, 2], [4, 8, 16, 32], [4, 4, 4, 4])

train_sampler = dict(
    type='concat',
    model_samplers=[
        dict(type='anchor', anchors=[_MAX, _MIN, _MID]),
        dict(type='repeat', times=2, model_sampler=dict(
            type='composite',
            model_samplers=[
                dict(type='candidate', key=_D, candidates=_product([2], [2], list(range(6, 19, 2)), [2])),
                dict(type='candidate', key=_H,
                     candidates=_product([3, 4], [6, 7, 8], [12, 14, 16], [24, 28, 32])),
                dict(type='candidate', key=_R, candidates=_product([4], [4], [3, 4], [3, 4]))])),
    ])
val_sampler = dict(type='anchor', anchors=[_MIN, _MID, _MAX])
