# The R50..R101(+) search space of ar50to101v2.py with the third elastic dimension: the input scale.
# The scale candidates are the reference's (configs/_dynamic_/model_samplers/ar50to101v2_flops.py:1-4,
# key 'data.input_shape', a 'candidate' sampler inside a 'composite').  A value S is the short side of
# the batch; it is APPLIED only by a config that sets apply_input_shape = True.
# train: one scale draw merged with one draw of the arch sampler of ar50to101v2.py (each step one of
# its 5 anchors and 3 random subnets); val: R50 and R101 at two scales of the range.
_scale = dict(key='data.input_shape', candidates=(480, 560, 640, 720, 800, 880, 960))
_stem = dict(key='arch.backbone.stem.width', start=32, end=64, step=16)
_width = dict(key='arch.backbone.body.width', start=[48, 96, 192, 384], end=[80, 160, 320, 640],
              step=[16, 32, 64, 128], ascending=True)
_depth = dict(key='arch.backbone.body.depth', start=[2, 2, 5, 2], end=[4, 6, 29, 4],
              step=[1, 2, 2, 1])


def _anchor(name, stem, width, depth, scale=None):
    a = {'name': name, 'arch.backbone.stem.width': stem, 'arch.backbone.body.width': width,
         'arch.backbone.body.depth': depth}
    if scale is not None:
        a['name'] = '%s@%d' % (name, scale)
        a['data.input_shape'] = scale
    return a


_R50 = (64, [64, 128, 256, 512], [3, 4, 6, 3])
_R77 = (64, [64, 128, 256, 512], [3, 4, 15, 3])
_R101 = (64, [64, 128, 256, 512], [3, 4, 23, 3])

train_sampler = dict(
    type='composite',
    model_samplers=[
        dict(type='candidate', **_scale),
        dict(type='concat', model_samplers=[
            dict(type='anchor', anchors=[
                _anchor('MAX', _stem['end'], _width['end'], _depth['end']),
                _anchor('MIN', _stem['start'], _width['start'], _depth['start']),
                _anchor('R101', *_R101), _anchor('R77', *_R77), _anchor('R50', *_R50)]),
            dict(type='repeat', times=3, model_sampler=dict(
                type='composite',
                model_samplers=[dict(type='range', **_stem), dict(type='range', **_width),
                                dict(type='range', **_depth)])),
        ]),
    ])
val_sampler = dict(type='anchor', anchors=[
    _anchor('R50', *_R50, scale=480), _anchor('R50', *_R50, scale=800),
    _anchor('R101', *_R101, scale=480), _anchor('R101', *_R101, scale=800)])
