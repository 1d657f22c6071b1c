# Search space of the ConvNeXt-T .. ConvNeXt-B seg supernet and its train / val samplers.
# Stage-1 width 96 / 112 / 128 with the later stages at 2x, 4x and 8x of it (one draw moves all four, as
# in the ConvNeXt family); stage-3 depth 9 / 18 / 27, the other stages stay at 3 blocks.
# Anchors: ConvNeXt-T (MIN), ConvNeXt-S (the middle: T's widths at B's depths), ConvNeXt-B (MAX).
_widths = [[w, 2 * w, 4 * w, 8 * w] for w in (96, 112, 128)]
_depths = [[3, 3, d, 3] for d in (9, 18, 27)]


def _anchor(name, width, depth):
    return {'name': name, 'arch.backbone.body.width': width, 'arch.backbone.body.depth': depth}


_T = _anchor('ConvNeXt-T', _widths[0], _depths[0])
_S = _anchor('ConvNeXt-S', _widths[0], _depths[2])
_B = _anchor('ConvNeXt-B', _widths[2], _depths[2])

train_sampler = dict(
    type='concat',
    model_samplers=[
        dict(type='anchor', anchors=[_B, _T, _S]),
        dict(type='repeat', times=2, model_sampler=dict(
            type='composite',
            model_samplers=[dict(type='candidate', key='arch.backbone.body.width', candidates=_widths),
                            dict(type='candidate', key='arch.backbone.body.depth', candidates=_depths)])),
    ])
val_sampler = dict(type='anchor', anchors=[_T, _S, _B])
