# Search space of the ConvNeXt V2 Nano .. Base seg supernet and its train / val samplers.
# Stage-1 width 80 / 96 / 112 / 128 with the later stages at 2x, 4x and 8x of it (one draw moves all
# four, as in the ConvNeXt V2 family); depths [2, 2, 8, 2] (Nano), [3, 3, 9, 3] (Tiny), [3, 3, 18, 3] and
# [3, 3, 27, 3] (Base).
# Anchors: V2-Nano (MIN), V2-Tiny, V2-Base (MAX).
_widths = [[w, 2 * w, 4 * w, 8 * w] for w in (80, 96, 112, 128)]
_depths = [[2, 2, 8, 2], [3, 3, 9, 3], [3, 3, 18, 3], [3, 3, 27, 3]]


def _anchor(name, width, depth):
    return {'name': name, 'arch.backbone.body.width': width, 'arch.backbone.body.depth': depth}


_N = _anchor('V2-Nano', _widths[0], _depths[0])
_T = _anchor('V2-Tiny', _widths[1], _depths[1])
_B = _anchor('V2-Base', _widths[3], _depths[3])

train_sampler = dict(
    type='concat',
    model_samplers=[
        dict(type='anchor', anchors=[_B, _N, _T]),
        dict(type='repeat', times=2, model_sampler=dict(
            type='composite',
            model_samplers=[dict(type='candidate', key='arch.backbone.body.width', candidates=_widths),
                            dict(type='candidate', key='arch.backbone.body.depth', candidates=_depths)])),
    ])
val_sampler = dict(type='anchor', anchors=[_N, _T, _B])
