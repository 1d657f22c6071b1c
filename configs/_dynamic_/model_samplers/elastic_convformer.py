# Search space of the elastic Conformer seg supernet and its train / val samplers.
# Conv widths 256 .. 384 / 512 .. 768 / 1024 .. 1536 in steps of 64 (stage 4 follows stage 3), embedding
# width 384 .. 576 in steps of 64, per stage 6 .. 9 heads of width 64 and a feed-forward ratio of
# 30 / 35 / 40 tenths of the embedding width (int(ratio / 10 * embed_dim) is a multiple of 4 for every
# width above).
# Depth ranges, chosen here: stage 1 runs 2 .. 3 blocks, stages 2 and 3 run 2 .. 4 (stage 4 always runs its
# one block).  A stage keeps at least two blocks so that every stage has a coupled block: the first block
# of stage 1 has no coupling units, and one block per stage would leave stage 1 without any.  The maxima
# [3, 4, 4] (+ 1) are the 12 blocks of Conformer-S and Conformer-B.  The stem is not searched (the backbone
# freezes it).
# Anchors: MIN (Conformer-S-like: embed 384, 6 heads, widths 256 / 512 / 1024, at the smallest depths and
# ratio), MID, MAX (Conformer-B-like: embed 576, 9 heads, widths 384 / 768 / 1536, depths [3, 4, 4], ratio 40).
_B = 'arch.backbone.body.'
_S = 'arch.backbone.stem.width'
_D = _B + 'depth'
_W = _B + 'block.convblock.width'
_E = _B + 'block.embed_dim.width'
_H = _B + 'block.transblock.MHA.num_heads.num_heads'
_F = _B + 'block.transblock.FFN.feedforward_channels.feedforward_channels'
_triples = lambda values: [[a, b, c] for a in values for b in values for c in values]  # noqa: E731


def _anchor(name, dim, depths, heads, widths, ratio):
    return {'name': name, _S: 64, _D: depths, _W: widths, _E: dim, _H: [heads] * 3, _F: [ratio] * 3}


_MIN = _anchor('MIN', 384, [2, 2, 2], 6, [256, 512, 1024], 30)
_MID = _anchor('MID', 448, [2, 3, 3], 7, [320, 640, 1280], 35)
_MAX = _anchor('MAX', 576, [3, 4, 4], 9, [384, 768, 1536], 40)

train_sampler = dict(
    type='concat',
    model_samplers=[
        dict(type='anchor', anchors=[_MAX, _MIN, _MID]),
        dict(type='repeat', times=2, model_sampler=dict(
            type='composite',
            model_samplers=[dict(type='candidate', key=_S, candidates=[64]),
                            dict(type='candidate', key=_D,
                                 candidates=[[a, b, c] for a in (2, 3) for b in (2, 3, 4) for c in (2, 3, 4)]),
                            dict(type='candidate', key=_W,
                                 candidates=[[a, b, c] for a in range(256, 385, 64) for b in range(512, 769, 64)
                                             for c in range(1024, 1537, 64)]),
                            dict(type='candidate', key=_E, candidates=list(range(384, 577, 64))),
                            dict(type='candidate', key=_H, candidates=_triples(list(range(6, 10)))),
                            dict(type='candidate', key=_F, candidates=_triples([30, 35, 40]))])),
    ])
val_sampler = dict(type='anchor', anchors=[_MIN, _MID, _MAX])
