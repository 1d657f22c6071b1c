"""DynamicConvNeXtV2 backbone: ConvNeXt V2 (arXiv 2301.00808) with dynamic stage widths and depths.

The V1 block with the layer scale removed and a Global Response Normalization after the GELU of the
4C-wide hidden layer: ``x + pwconv2(GRN(GELU(pwconv1(LN(dwconv7x7(x))))))``.  GELU and GRN are one operator
(ops.gelu_grn on csrc/grn.hip), so the GELU output never exists in memory; everything else runs on the
kernels of DynamicConvNeXt, whose search space, arch manipulation, execution order, side-stream checkpoint
and deploy-mode truncation this class inherits.

Module and parameter names are those of transformers' ``ConvNextV2Backbone`` with all four ``out_features``
(``embeddings.patch_embeddings``, ``embeddings.layernorm``, ``encoder.stages.{i}.downsampling_layer.{0,1}`` for
i = 1..3, ``encoder.stages.{i}.layers.{j}.{dwconv, layernorm, pwconv1, grn, pwconv2}``,
``hidden_states_norms.stage{1..4}``), with 2-D linear weights, [C, 1, 7, 7] depthwise weights and
[1, 1, 1, 4C] GRN parameters in the state dict, so such a state dict loads with ``strict=True``.

Not implemented: stochastic depth (``drop_path_rate > 0`` is refused).
"""
import torch.nn as nn

from ...core.bricks import DynamicConv2d, DynamicGRN, DynamicLayerNorm, DynamicLinear
from ...hip import ops
from ..builder import BACKBONES
from .dynamic_convnext import DynamicBlock, DynamicConvNeXt, DynamicConvNeXtBlock


class DynamicConvNeXtV2Block(DynamicConvNeXtBlock):
    """x + pwconv2(GRN(GELU(pwconv1(LN(dwconv7x7(x)))))), every layer on its leading active slice."""

    def __init__(self, dim):
        nn.Module.__init__(self)
        self.dwconv = DynamicConv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.layernorm = DynamicLayerNorm(dim, eps=1e-6, data_format="channels_last")
        self.pwconv1 = DynamicLinear(dim, 4 * dim)
        self.grn = DynamicGRN(4 * dim)
        self.pwconv2 = DynamicLinear(4 * dim, dim)
        self.init_state(width=dim)

    norm = property(lambda self: self.layernorm)

    def forward_act(self, tape, x):
        y = self.dwconv.forward_act(tape, x)
        y = self.layernorm.forward_act(tape, y)
        y = self.pwconv1.forward_act(tape, y)
        y = self.grn.forward_act(tape, y)
        y = self.pwconv2.forward_act(tape, y)
        return ops.layer_scale_add(tape, x, y, None)


class DynamicV2Layers(DynamicBlock):
    """The ``layers`` of one stage: ``depth`` V2 blocks at their maximum width, the first ``depth_state`` run."""

    def __init__(self, dim, depth):
        nn.ModuleList.__init__(self, [DynamicConvNeXtV2Block(dim) for _ in range(depth)])
        self.init_state(depth=depth, width=dim)


class _Embeddings(nn.Module):
    def __init__(self, in_chans, dim):
        super().__init__()
        self.patch_embeddings = DynamicConv2d(in_chans, dim, kernel_size=4, stride=4, padding=0)
        self.layernorm = DynamicLayerNorm(dim, eps=1e-6, data_format="channels_first")


class _Stage(nn.Module):
    """``downsampling_layer`` (LayerNorm, 2x2 stride-2 conv; empty in front of the first stage) and ``layers``"""

    def __init__(self, in_dim, dim, depth):
        super().__init__()
        self.downsampling_layer = nn.ModuleList() if in_dim is None else nn.ModuleList([
            DynamicLayerNorm(in_dim, eps=1e-6, data_format="channels_first"),
            DynamicConv2d(in_dim, dim, kernel_size=2, stride=2, padding=0)])
        self.layers = DynamicV2Layers(dim, depth)


class _Encoder(nn.Module):
    def __init__(self, dims, depths):
        super().__init__()
        self.stages = nn.ModuleList([_Stage(dims[i - 1] if i else None, dims[i], depths[i]) for i in range(4)])


@BACKBONES.register_module()
class DynamicConvNeXtV2(DynamicConvNeXt):
    """ConvNeXt V2 with the ``body = {width, depth}`` search space of DynamicConvNeXt: Atto to Huge are one
    architecture that differs in stage width and stage-3 depth only."""

    def __init__(self, depths, dims, in_chans=3, drop_path_rate=0., out_indices=(0, 1, 2, 3), pretrained=None):
        nn.Module.__init__(self)
        if drop_path_rate > 0:
            raise NotImplementedError("drop_path_rate > 0: stochastic depth is not implemented "
                                      "(set drop_path_rate=0)")
        if len(depths) != 4 or len(dims) != 4:
            raise AssertionError("DynamicConvNeXtV2 has four stages: depths and dims need four entries")
        self.depths, self.dims, self.out_indices = list(depths), list(dims), list(out_indices)
        self.init_state(body={"depth": list(depths), "width": list(dims)})
        self.embeddings = _Embeddings(in_chans, dims[0])
        self.encoder = _Encoder(self.dims, self.depths)
        self.hidden_states_norms = nn.ModuleDict({
            "stage%d" % (i + 1): DynamicLayerNorm(dims[i], eps=1e-6, data_format="channels_first")
            for i in range(4)})
        self.init_weights(pretrained)

    # ---- DynamicConvNeXt's view of the modules ----
    stem = property(lambda self: self.embeddings.patch_embeddings)
    stem_ln = property(lambda self: self.embeddings.layernorm)
    ds1_ln = property(lambda self: self.encoder.stages[1].downsampling_layer[0])
    ds2_ln = property(lambda self: self.encoder.stages[2].downsampling_layer[0])
    ds3_ln = property(lambda self: self.encoder.stages[3].downsampling_layer[0])
    ds1_conv = property(lambda self: self.encoder.stages[1].downsampling_layer[1])
    ds2_conv = property(lambda self: self.encoder.stages[2].downsampling_layer[1])
    ds3_conv = property(lambda self: self.encoder.stages[3].downsampling_layer[1])

    def stage(self, i):
        return self.encoder.stages[i].layers

    def out_norm(self, i):
        return self.hidden_states_norms["stage%d" % (i + 1)]

    def init_weights(self, pretrained=None):
        """DynamicConvNeXt's init (truncated normal 0.02, zero biases, unit LayerNorms) and zero GRN
        parameters, transformers' init; then the checkpoint, if a path is given."""
        for m in self.modules():
            if isinstance(m, DynamicGRN):
                nn.init.constant_(m.weight, 0)
                nn.init.constant_(m.bias, 0)
        super().init_weights(pretrained)
