# Search space of the elastic ViT seg supernet and its train / val samplers.
# Embedding width 384 .. 768 in steps of 64 (ViT-S .. ViT-B); per encoder group 6 .. 12 heads of width 64,
# a feed-forward ratio of 30 / 35 / 40 tenths of the embedding width (the ratios at which
# int(ratio / 10 * embed_dim) is a multiple of 4 for every width above) and 2 .. 4 layers (the backbone
# hands out the second layer of its first group, so a group keeps at least two).
# Anchors: MIN (ViT-S width, 6 layers), MID, MAX (ViT-B: 768 wide, 12 heads, 12 layers, ratio 40).
_E = 'arch.backbone.embedding.embed_dim'
_L = 'arch.backbone.encoder.num_layers'
_H = 'arch.backbone.encoder.num_heads.num_heads.num_heads'
_F = 'arch.backbone.encoder.feedforward_channels.feedforward_channels.feedforward_channels'
_dims = list(range(384, 769, 64))
_triples = lambda values: [[a, b, c] for a in values for b in values for c in values]  # noqa: E731


def _anchor(name, dim, layers, heads, ratio):
    return {'name': name, _E: dim, _L: [layers] * 3, _H: [heads] * 3, _F: [ratio] * 3}


_MIN = _anchor('MIN', 384, 2, 6, 30)
_MID = _anchor('MID', 576, 3, 9, 35)
_MAX = _anchor('MAX', 768, 4, 12, 40)

train_sampler = dict(
    type='concat',
    model_samplers=[
        dict(type='anchor', anchors=[_MAX, _MIN, _MID]),
        dict(type='repeat', times=2, model_sampler=dict(
            type='composite',
            model_samplers=[dict(type='candidate', key=_E, candidates=_dims),
                            dict(type='candidate', key=_L, candidates=_triples([2, 3, 4])),
                            dict(type='candidate', key=_H, candidates=_triples(list(range(6, 13)))),
                            dict(type='candidate', key=_F, candidates=_triples([30, 35, 40]))])),
    ])
val_sampler = dict(type='anchor', anchors=[_MIN, _MID, _MAX])
