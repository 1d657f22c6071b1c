# Search space of the SegNeXt (MSCAN) supernet and its train / val samplers.
# Per stage: depth, width and the feed-forward ratio (hidden width = int(ratio x width)).  Every width is a
# multiple of 8 (the stem runs at half of the stage-1 width, and the kernels move float4 channel quads), so
# every hidden width is a multiple of 4.
# Anchors: MIN (MSCAN-T: depths 3/3/5/2 cut to 2/2/4/2, widths 32/64/160/256, ratio 4), MID (MSCAN-S with
# depths 2/2/4/2), MAX (MSCAN-B: depths 3/3/12/3, widths 64/128/320/512, ratios 8/8/4/4).
_D = 'arch.backbone.body.depth'
_W = 'arch.backbone.body.width'
_R = 'arch.backbone.body.mlp_ratio'
_product = lambda a, b, c, d: [[w, x, y, z] for w in a for x in b for y in c for z in d]  # noqa: E731


def _anchor(name, depth, width, ratio):
    return {'name': name, _D: depth, _W: width, _R: ratio}


_MIN = _anchor('MIN', [2, 2, 4, 2], [32, 64, 160, 256], [4, 4, 4, 4])
_MID = _anchor('MID', [2, 2, 4, 2], [64, 128, 320, 512], [8, 8, 4, 4])
_MAX = _anchor('MAX', [3, 3, 12, 3], [64, 128, 320, 512], [8, 8, 4, 4])

train_sampler = dict(
    type='concat',
    model_samplers=[
        dict(type='anchor', anchors=[_MAX, _MIN, _MID]),
        dict(type='repeat', times=2, model_sampler=dict(
            type='composite',
            model_samplers=[
                dict(type='candidate', key=_D,
                     candidates=_product([2, 3], [2, 3], list(range(4, 13, 2)), [2, 3])),
                dict(type='candidate', key=_W,
                     candidates=_product([32, 48, 64], [64, 96, 128], [160, 240, 320], [256, 384, 512])),
                dict(type='candidate', key=_R, candidates=_product([4, 6, 8], [4, 6, 8], [4], [4]))])),
    ])
val_sampler = dict(type='anchor', anchors=[_MIN, _MID, _MAX])
