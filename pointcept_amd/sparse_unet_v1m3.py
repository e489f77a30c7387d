"""SpUNet-v1m3 on the engine: drop-in for pointcept/models/sparse_unet/spconv_unet_v1m3_pdnorm.py (registry name "SpUNet-v1m3", the
prompt-driven-BatchNorm U-Net that Point Prompt Training trains), with the reference's constructor arguments (:232-246), its
_init_weights including zero_init (:373-389) and its state-dict keys: conv_input.{conv,bn}, down.{s}.{conv,bn},
enc.{s}.block{i}.{conv1,bn1,conv2,bn2,proj_conv,proj_norm}, up.{s}.{conv,bn}, dec.{s}.block{i}..., final; every norm holds
bns.{j}.* (norm_decouple) or bn.*, and modulation.1.* (norm_adaptive).  Registered only when named:
compat.register_models(MODELS, names=["SpUNet-v1m3"]).

* PDBatchNorm needs no kernel of its own.  PPT's context is ONE row (embedding_table(tensor([idx])): [1, context_channels]), so the
  (shift, scale) of :63-74 are one [C] vector each and BN(x) * (1 + scale) + shift is BatchNorm with gamma' = gamma (1 + scale),
  beta' = beta (1 + scale) + shift (gamma = 1, beta = 0 with norm_affine=False).  functional.batch_norm_act takes weight and bias as
  differentiable inputs: the whole prompt-driven norm, its following ReLU and the relu(bn2(.) + residual) tail run in the existing
  BatchNorm kernels, and the modulation's gradients come back through autograd on [C] vectors.  The per-condition running statistics,
  the step counters (nn.batched_bn_counters) and the fused act / residual arguments are nn.BatchNorm1d's.  Wherever
  nn.BatchNorm1d.forward would fall back (CPU tensors, one row, an unsupported width, a hooked or replaced norm, a context of more
  than one row) the norm runs the reference's three-step form.
* Everything around the stages -- the Hilbert pre-sort, the hash table, duplicate marking, the rulebook prefetch, the enc_mode
  mean -- is SpUNetBase._forward itself (sparse_unet.py); this file only tells it how to call a stage with (condition, context).
* `condition` may be a list, a tuple or a string (:395-399).
"""
from __future__ import annotations

from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn

from . import config as _config
from . import nn as PNN
from . import spconv_api as spconv
from .sparse_unet import SpUNetBase, trunc_normal_


class PDBatchNorm(nn.Module):
    """spconv_unet_v1m3_pdnorm.py:25-74"""

    def __init__(self, num_features, context_channels=256, eps=1e-3, momentum=0.01, conditions=("ScanNet", "S3DIS", "Structured3D"),
                 decouple=True, adaptive=False, affine=True):
        super().__init__()
        self.conditions = conditions
        self.decouple = decouple
        self.adaptive = adaptive
        self.affine = affine
        if self.decouple:
            self.bns = nn.ModuleList([PNN.BatchNorm1d(num_features=num_features, eps=eps, momentum=momentum, affine=affine) for _ in conditions])
        else:
            self.bn = PNN.BatchNorm1d(num_features=num_features, eps=eps, momentum=momentum, affine=affine)
        if self.adaptive:
            self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(context_channels, 2 * num_features, bias=True))

    def norm_of(self, condition):
        if self.decouple:
            assert condition in self.conditions
            return self.bns[self.conditions.index(condition)]
        return self.bn

    def forward(self, feat, condition=None, context=None, relu=None, residual=None):
        """relu(PDNorm(feat) [+ residual]) with `relu` the ReLU module that follows the norm in the reference (None: no activation)"""
        bn = self.norm_of(condition)
        shift = scale = None
        if self.adaptive:
            assert context is not None
            with torch.autocast(device_type=feat.device.type, enabled=False):     # [1, 2C] from a [1, context_channels] row: fp32
                shift, scale = self.modulation(context.float()).chunk(2, dim=1)
        kind = None
        if PNN.foldable(bn) and (not self.adaptive or context.shape[0] == 1) and (residual is None or _config.FUSE_BN_TAIL):
            kind = "none" if relu is None else PNN.fused_act(bn, relu)
        if kind is not None and bn.kernel_path(feat, residual, need_affine=False):
            weight, bias = bn.weight, bn.bias
            if self.adaptive:          # gamma' = gamma (1 + scale), beta' = beta (1 + scale) + shift
                one = 1.0 + scale.reshape(-1)
                weight = one if weight is None else weight * one
                bias = shift.reshape(-1) if bias is None else bias * one + shift.reshape(-1)
            elif weight is None:
                weight, bias = feat.new_ones(feat.shape[1], dtype=torch.float32), feat.new_zeros(feat.shape[1], dtype=torch.float32)
            return bn(feat, residual=residual, act=kind, weight=weight, bias=bias)
        # the reference's three-step form
        feat = bn(feat)
        if self.adaptive:
            feat = feat * (1.0 + scale) + shift
        if residual is not None:
            feat = feat + residual
        return feat if relu is None else relu(feat)


class BasicBlock(spconv.SparseModule):
    """:77-146"""
    expansion = 1

    def __init__(self, in_channels, embed_channels, stride=1, norm_fn=None, indice_key=None, bias=False):
        super().__init__()
        assert norm_fn is not None
        self.in_channels = in_channels
        self.embed_channels = embed_channels
        if in_channels == embed_channels:
            self.proj = spconv.SparseSequential(nn.Identity())
        else:
            self.proj_conv = spconv.SubMConv3d(in_channels, embed_channels, kernel_size=1, bias=False)
            self.proj_norm = norm_fn(embed_channels)
        self.conv1 = spconv.SubMConv3d(in_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn1 = norm_fn(embed_channels)
        self.relu = PNN.ReLU()
        self.conv2 = spconv.SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn2 = norm_fn(embed_channels)
        self.stride = stride

    def forward(self, x, condition, context):
        residual = x
        out = self.conv1(x)
        out = out.replace_feature(self.bn1(out.features, condition, context, relu=self.relu))
        out = self.conv2(out)
        if self.in_channels == self.embed_channels:
            residual = self.proj(residual)
        else:
            residual = residual.replace_feature(self.proj_norm(self.proj_conv(residual).features, condition, context))
        return out.replace_feature(self.bn2(out.features, condition, context, relu=self.relu, residual=residual.features))


class _ConvNormAct(nn.Module):
    """conv -> PDNorm -> ReLU: SPConvDown (:149-176), SPConvUp (:179-205), SPConvPatchEmbedding (:208-227)"""

    def __init__(self, conv, out_channels, norm_fn):
        super().__init__()
        self.conv = conv
        self.bn = norm_fn(out_channels)
        self.relu = PNN.ReLU()

    def forward(self, x, condition, context):
        out = self.conv(x)
        return out.replace_feature(self.bn(out.features, condition, context, relu=self.relu))


class _Blocks(nn.Sequential):
    def forward(self, x, condition, context):
        for block in self:
            x = block(x, condition, context)
        return x


class SpUNetV1m3(SpUNetBase):
    """SpUNet-v1m3 (:230-432)"""

    def __init__(self, in_channels, num_classes=0, base_channels=32, context_channels=256, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                 layers=(2, 3, 4, 6, 2, 2, 2, 2), enc_mode=False, conditions=("ScanNet", "S3DIS", "Structured3D"), zero_init=True,
                 norm_decouple=True, norm_adaptive=True, norm_affine=False):
        nn.Module.__init__(self)          # the stages below replace SpUNetBase's; its forward pass is kept (it reads the attributes listed there)
        assert len(layers) % 2 == 0 and len(layers) == len(channels)
        self.skip = True
        self.in_channels, self.num_classes, self.base_channels = in_channels, num_classes, base_channels
        self.channels, self.layers = channels, layers
        self.num_stages = len(layers) // 2
        self.enc_mode = enc_mode
        self.conditions = conditions
        self.zero_init = zero_init
        norm_fn = partial(PDBatchNorm, eps=1e-3, momentum=0.01, conditions=conditions, context_channels=context_channels,
                          decouple=norm_decouple, adaptive=norm_adaptive, affine=norm_affine)
        self.conv_input = _ConvNormAct(spconv.SubMConv3d(in_channels, base_channels, kernel_size=5, padding=1, bias=False, indice_key="stem"),
                                       base_channels, norm_fn)
        enc_channels, dec_channels = base_channels, channels[-1]
        self.down, self.up, self.enc = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.dec = nn.ModuleList() if not self.enc_mode else None
        for s in range(self.num_stages):
            self.down.append(_ConvNormAct(spconv.SparseConv3d(enc_channels, channels[s], kernel_size=2, stride=2, bias=False,
                                                              indice_key=f"spconv{s + 1}"), channels[s], norm_fn))
            self.enc.append(_Blocks(OrderedDict((f"block{i}", BasicBlock(channels[s], channels[s], norm_fn=norm_fn, indice_key=f"subm{s + 1}"))
                                                for i in range(layers[s]))))
            if not self.enc_mode:
                self.up.append(_ConvNormAct(spconv.SparseInverseConv3d(channels[len(channels) - s - 2], dec_channels, kernel_size=2, bias=False,
                                                                       indice_key=f"spconv{s + 1}"), dec_channels, norm_fn))
                self.dec.append(_Blocks(OrderedDict(
                    (f"block{i}", BasicBlock(dec_channels + enc_channels if i == 0 else dec_channels, dec_channels, norm_fn=norm_fn,
                                             indice_key=f"subm{s}"))
                    for i in range(layers[len(channels) - s - 1]))))
            enc_channels = channels[s]
            dec_channels = channels[len(channels) - s - 2]
        final_in = channels[-1] if not self.enc_mode else channels[self.num_stages - 1]
        self.final = (spconv.SubMConv3d(final_in, num_classes, kernel_size=1, padding=1, bias=True)
                      if num_classes > 0 else spconv.Identity())
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, (nn.Linear, spconv.SubMConv3d)):
            trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm1d):
            if m.affine:
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, PDBatchNorm):
            if self.zero_init and m.adaptive:
                nn.init.constant_(m.modulation[-1].weight, 0)
                nn.init.constant_(m.modulation[-1].bias, 0)

    def _forward(self, input_dict):
        condition = input_dict["condition"]
        if isinstance(condition, (list, tuple)):
            condition = condition[0]
        context = input_dict["context"] if "context" in input_dict.keys() else None
        return super()._forward(input_dict, call=lambda m, x: m(x, condition, context))
