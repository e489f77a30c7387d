"""OA-CNNs on the engine: drop-in for pointcept/models/oacnns/oacnns_v1m1_base.py (registry name "OACNNs", ctor :193-206,
forward(input_dict{grid_coord, feat, offset}) -> [N, num_classes] :283-307, same state-dict keys: stem.{0,3,6}.weight,
enc.{s}.down.0.weight, enc.{s}.blocks.{b}.{proj,weight,l_w,adaptive,fuse,voxel_block}.*, dec.{s}.up.0.weight,
dec.{s}.fuse.{0,3}.{weight,bias}, final.{weight,bias}; UpBlock.blocks stays an empty ModuleList as in the reference).

The convolutions run on the sparse-convolution kernels (spconv_api), the Linears on the GEMM kernels (nn.Linear), every
BatchNorm -> ReLU pair in one BatchNorm pass.  The adaptive aggregation of a BasicBlock (:87-102) runs on csrc/cluster_agg.hip:
the grid clusters of all levels are built once per DonwBlock (:160-164, one host read for the block) and shared by its blocks, the
L centerings in one launch per pass, the L exp-weighted cluster sums and the softmax mix in one launch per pass, without float
atomics.  PTC_OACNN_AGG=0 sends centering and aggregation to the reference's ATen expression (A/B baseline).
"""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from . import config as _config
from . import functional as PF
from . import nn as PNN
from . import ops
from . import spconv_api as spconv
from .structure import offset2batch


def trunc_normal_(tensor, mean=0.0, std=1.0, a=-2.0, b=2.0):  # timm.layers.trunc_normal_
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


def _seq(mods: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """nn.Sequential(Linear, BatchNorm1d, ReLU, ...) with each BatchNorm -> ReLU pair in one pass (PNN.fused_act on the live modules)"""
    for m, act in PNN.plain_feature_runs(mods):
        x = m(x) if act is None else m(x, act=act)
    return x


class BasicBlock(nn.Module):
    """oacnns_v1m1_base.py:12-111"""

    def __init__(self, in_channels, embed_channels, norm_fn=None, indice_key=None, depth=4, groups=None, grid_size=None, bias=False):
        super().__init__()
        assert embed_channels % groups == 0
        self.groups = groups
        self.embed_channels = embed_channels
        self.proj = nn.ModuleList()
        self.grid_size = grid_size
        self.weight = nn.ModuleList()
        self.l_w = nn.ModuleList()

        def lin_bn_relu():
            return nn.Sequential(PNN.Linear(embed_channels, embed_channels, bias=False), norm_fn(embed_channels), PNN.ReLU())

        self.proj.append(lin_bn_relu())
        for _ in range(depth - 1):
            self.proj.append(lin_bn_relu())
            self.l_w.append(lin_bn_relu())
            self.weight.append(PNN.Linear(embed_channels, embed_channels, bias=False))
        self.adaptive = PNN.Linear(embed_channels, depth - 1, bias=False)
        self.fuse = nn.Sequential(PNN.Linear(embed_channels * 2, embed_channels, bias=False), norm_fn(embed_channels), PNN.ReLU())
        self.voxel_block = spconv.SparseSequential(
            spconv.SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=1, padding=1, indice_key=indice_key, bias=bias),
            norm_fn(embed_channels), PNN.ReLU(),
            spconv.SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=1, padding=1, indice_key=indice_key, bias=bias),
            norm_fn(embed_channels))
        self.act = PNN.ReLU()

    def forward(self, x, clusters: ops.GridClusters):
        feat = x.features
        L = len(self.l_w)
        pws = [_seq(self.l_w[i], feat) for i in range(L)]
        center, agg = ((PF.cluster_center, PF.cluster_agg) if _config.OACNN_AGG
                       else (PF.cluster_center_torch, PF.cluster_agg_torch))
        pws = center(pws, clusters)
        us = [self.weight[i](pws[i]) for i in range(L)]
        vs = [_seq(self.proj[i], feat) for i in range(L)]
        feats = agg(us, vs, self.adaptive(feat), clusters)
        f = _seq(self.proj[-1], feat)
        f = torch.cat([f, feats], dim=1)
        f = _seq(self.fuse, f) + x.features
        res = f
        x = self.voxel_block(x.replace_feature(f))
        return x.replace_feature(self.act(x.features + res))


class DonwBlock(nn.Module):
    """oacnns_v1m1_base.py:114-168 (the reference's spelling)"""

    def __init__(self, in_channels, embed_channels, depth, sp_indice_key, point_grid_size, num_ref=16, groups=None, norm_fn=None,
                 sub_indice_key=None):
        super().__init__()
        self.num_ref = num_ref
        self.depth = depth
        self.point_grid_size = point_grid_size
        self.down = spconv.SparseSequential(
            spconv.SparseConv3d(in_channels, embed_channels, kernel_size=2, stride=2, indice_key=sp_indice_key, bias=False),
            norm_fn(embed_channels), PNN.ReLU())
        self.blocks = nn.ModuleList()
        for _ in range(depth):
            self.blocks.append(BasicBlock(in_channels=embed_channels, embed_channels=embed_channels, depth=len(point_grid_size) + 1,
                                          groups=groups, grid_size=point_grid_size, norm_fn=norm_fn, indice_key=sub_indice_key))

    def forward(self, x):
        x = self.down(x)
        # all levels of the block at once (one host read: the cluster counts), shared by every block of the stage
        clusters = ops.grid_clusters(x.indices, self.point_grid_size, x.spatial_shape, x.batch_size)
        for block in self.blocks:
            x = block(x, clusters)
        return x


class UpBlock(nn.Module):
    """oacnns_v1m1_base.py:171-209"""

    def __init__(self, in_channels, skip_channels, embed_channels, depth, sp_indice_key, norm_fn=None, down_ratio=2, sub_indice_key=None):
        super().__init__()
        assert depth > 0
        self.up = spconv.SparseSequential(
            spconv.SparseInverseConv3d(in_channels, embed_channels, kernel_size=down_ratio, indice_key=sp_indice_key, bias=False),
            norm_fn(embed_channels), PNN.ReLU())
        self.blocks = nn.ModuleList()
        self.fuse = nn.Sequential(
            PNN.Linear(skip_channels + embed_channels, embed_channels), norm_fn(embed_channels), PNN.ReLU(),
            PNN.Linear(embed_channels, embed_channels), norm_fn(embed_channels), PNN.ReLU())

    def forward(self, x, skip_x):
        x = self.up(x)
        f = torch.cat([x.features, skip_x.features], dim=1)
        return x.replace_feature(_seq(self.fuse, f) + x.features)


class OACNNs(nn.Module):
    def __init__(self, in_channels, num_classes, embed_channels=64, enc_num_ref=(16, 16, 16, 16), enc_channels=(64, 64, 128, 256),
                 groups=(2, 4, 8, 16), enc_depth=(2, 3, 6, 4), down_ratio=(2, 2, 2, 2), dec_channels=(96, 96, 128, 256),
                 point_grid_size=((16, 32, 64), (8, 16, 24), (4, 8, 12), (2, 4, 6)), dec_depth=(2, 2, 2, 2)):
        super().__init__()
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.num_stages = len(enc_channels)
        self.embed_channels = embed_channels
        norm_fn = partial(PNN.BatchNorm1d, eps=1e-3, momentum=0.01)

        def subm(cin):
            return spconv.SubMConv3d(cin, embed_channels, kernel_size=3, padding=1, indice_key="stem", bias=False)

        self.stem = spconv.SparseSequential(
            subm(in_channels), norm_fn(embed_channels), PNN.ReLU(),
            subm(embed_channels), norm_fn(embed_channels), PNN.ReLU(),
            subm(embed_channels), norm_fn(embed_channels), PNN.ReLU())
        self.enc = nn.ModuleList()
        self.dec = nn.ModuleList()
        for i in range(self.num_stages):
            self.enc.append(DonwBlock(
                in_channels=embed_channels if i == 0 else enc_channels[i - 1], embed_channels=enc_channels[i], depth=enc_depth[i],
                norm_fn=norm_fn, groups=groups[i], point_grid_size=list(point_grid_size[i]), num_ref=enc_num_ref[i],
                sp_indice_key=f"spconv{i}", sub_indice_key=f"subm{i + 1}"))
            self.dec.append(UpBlock(
                in_channels=enc_channels[-1] if i == self.num_stages - 1 else dec_channels[i + 1],
                skip_channels=embed_channels if i == 0 else enc_channels[i - 1], embed_channels=dec_channels[i], depth=dec_depth[i],
                norm_fn=norm_fn, sp_indice_key=f"spconv{i}", sub_indice_key=f"subm{i}"))
        self.final = spconv.SubMConv3d(dec_channels[0], num_classes, kernel_size=1)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, (nn.Linear, spconv.SubMConv3d)):
            trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward(self, input_dict):
        with PNN.batched_bn_counters():
            return self._forward(input_dict)

    def _forward(self, input_dict):
        grid_coord, feat, offset = input_dict["grid_coord"], input_dict["feat"], input_dict["offset"]
        batch = offset2batch(offset, int(feat.shape[0]))
        indices = torch.cat([batch.unsqueeze(-1).int(), grid_coord.int()], dim=1).contiguous()
        n = indices.shape[0]
        table = ops.HashTable(indices)
        rep = ops.rulebook_subm(indices, 1, table)[0]
        n_dup = (rep != torch.arange(n, device=rep.device, dtype=rep.dtype)).sum().reshape(1).to(torch.int64)
        host = torch.cat([ops.coord_max(grid_coord), n_dup]).tolist()      # the one host sync of the stem
        ops.check_coord_range(host[:3], offset.numel())
        # The reference declares max + 1 (:289-291); the engine's strided maps keep every coarse site (as the oracle's do), so the
        # declared shape gets the SpUNet margin: every coarse coordinate then lies inside the shape its level reports, which the grid
        # clusters size their keys from.
        sparse_shape = [int(m) + 96 for m in host[:3]]
        x = spconv.SparseConvTensor(features=feat, indices=indices, spatial_shape=sparse_shape, batch_size=int(offset.numel()))
        x.indice_dict["__hash__"] = table
        spconv.mark_duplicates(x, host[3] > 0)
        spconv.prefetch_down_rulebooks(x, [f"spconv{i}" for i in range(self.num_stages)])
        x = self.stem(x)
        skips = [x]
        for i in range(self.num_stages):
            x = self.enc[i](x)
            skips.append(x)
        x = skips.pop(-1)
        for i in reversed(range(self.num_stages)):
            x = self.dec[i](x, skips.pop(-1))
        x = self.final(x)
        return x.features
