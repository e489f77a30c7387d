"""Masked Scene Contrast on the engine: drop-in for pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py
("MSC-v1m1"), with the reference's constructor arguments, state-dict keys (mask_token, color_head.*, normal_head.*, backbone.*),
forward(data_dict) keys and result-dict keys.  Registered only when named: compat.register_models(MODELS, names=["MSC-v1m1"]).

* generate_cross_masks: ops.msc_cross_masks -- the voxel_grid ids of floor(origin / mask_grid_size) over the union of both views,
  ranked by a key sort; point_mask[i] = patch_mask[rank[i]].  One host read (patch_num, for randperm); no dense patch map.
* match_contrastive_pair: ops.msc_match (27 grid cells per query instead of the whole scene) + ops.msc_select.  One host read (the
  number of matched queries and the largest count, for randint); the randperm cut to matching_max_pair stays in torch.
* compute_contrastive_loss: functional.msc_nce -- gather, normalise, tile-wise S = A B^T with an online log-sum-exp; the P x P
  matrix is never stored.  dist.all_reduce when the world size is above 1, as there.
* The mask-token blend and the reconstruction heads (masked-row gather, Linear(C, 3), squared error, cosine) stay in torch.
* The four random draws go through `draw(kind, ...)`: randperm(patch_num), randint(count.max(), count.shape), randperm(P) and
  random.random(), each made as the reference makes it, in its order, on its device; tests replay recorded draws through it.
* PTC_MSC=0: the reference's own expression written on ops.knn_query and torch (A/B baseline; the CPU path of the port).

MSC-v1m2 (masked_scene_contrast_v1m2_csc.py, configs/scannet/pretrain-msc-v1m2-0-spunet-csc.py: the ScanNet-Pair / PointContrast
recipe with mask_rate = 0 and no reconstruction heads) is MaskedSceneContrastCSC: the same masks, matching, backbone and forward;
only compute_contrastive_loss differs.  It takes the two origin coordinates and computes, per scene, one InfoNCE per partition class
of rel = x1[j] - x2[i] (distance bands r1 / r2, above / below): functional.msc_csc_nce -- pairs grouped by scene on the device, the
class of a logit computed in the tile from staged coordinates, five online log-sum-exps per row, no P_b x P_b tensor and no host
read (the reference reads 1 + scenes times).  PTC_MSC=0: functional.msc_csc_nce_torch, the reference's loop.  The ScanNet-Pair
dataset class and the PointContrast data pipeline stay the reference's.
"""
from __future__ import annotations

import random
from itertools import chain

import torch
import torch.distributed as dist
import torch.nn as nn

from . import config as _config
from . import functional as PF
from . import ops
from .compat import build_backbone
from .structure import offset2batch


def _world_size() -> int:
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class MaskedSceneContrast(nn.Module):
    """MSC-v1m1 (masked_scene_contrast_v1m1_base.py:24-310)"""

    def __init__(self, backbone, backbone_in_channels, backbone_out_channels, mask_grid_size=0.1, mask_rate=0.4, view1_mix_prob=0,
                 view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=8192, nce_t=0.4, contrast_weight=1,
                 reconstruct_weight=1, reconstruct_color=True, reconstruct_normal=True):
        super().__init__()
        self.backbone = build_backbone(backbone)
        self.mask_grid_size = mask_grid_size
        self.mask_rate = mask_rate
        self.view1_mix_prob = view1_mix_prob
        self.view2_mix_prob = view2_mix_prob
        self.matching_max_k = matching_max_k
        self.matching_max_radius = matching_max_radius
        self.matching_max_pair = matching_max_pair
        self.nce_t = nce_t
        self.contrast_weight = contrast_weight
        self.reconstruct_weight = reconstruct_weight
        self.reconstruct_color = reconstruct_color
        self.reconstruct_normal = reconstruct_normal
        self.mask_token = nn.Parameter(torch.zeros(1, backbone_in_channels))
        nn.init.trunc_normal_(self.mask_token, mean=0.0, std=0.02)
        self.color_head = nn.Linear(backbone_out_channels, 3) if reconstruct_color else None
        self.normal_head = nn.Linear(backbone_out_channels, 3) if reconstruct_normal else None
        self.last = {}               # the integers of the last forward (masks, match_index), for tests and tools

    # ---- the random draws, as the reference makes them (:114, :166, :171, :249, :253) ----
    def draw(self, kind, *args, device=None):
        if kind == "patch_perm":
            return torch.randperm(args[0])
        if kind == "select":         # args = (count.max(), count.shape)
            return torch.randint(args[0], args[1], device=device)
        if kind == "pair_perm":
            return torch.randperm(args[0])
        if kind == "mix":
            return random.random()
        raise ValueError(kind)

    @staticmethod
    def _kernels(t: torch.Tensor) -> bool:
        return _config.MSC_KERNELS and t.is_cuda

    # ---- :69-141 ----
    @torch.no_grad()
    def generate_cross_masks(self, view1_origin_coord, view1_offset, view2_origin_coord, view2_offset):
        assert self.mask_rate <= 0.5
        if self._kernels(view1_origin_coord):
            return ops.msc_cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, self.mask_grid_size,
                                       self.mask_rate, rand_perm=lambda n: self.draw("patch_perm", n))
        from .torch_geometric_api import voxel_grid

        view1_batch, view2_batch = offset2batch(view1_offset), offset2batch(view2_offset)
        view1_batch_count = view1_batch.bincount(minlength=view1_offset.numel())
        view2_batch_count = view2_batch.bincount(minlength=view2_offset.numel())
        union_origin_coord = torch.cat(list(chain.from_iterable(zip(view1_origin_coord.split(view1_batch_count.tolist()),
                                                                    view2_origin_coord.split(view2_batch_count.tolist())))))
        union_batch = offset2batch(view1_offset + view2_offset)
        mask_patch_grid_coord = torch.floor(union_origin_coord.div(self.mask_grid_size))
        mask_patch_cluster = voxel_grid(pos=mask_patch_grid_coord, size=1, batch=union_batch, start=0)
        unique, cluster, counts = torch.unique(mask_patch_cluster, sorted=True, return_inverse=True, return_counts=True)
        patch_num = unique.shape[0]
        patch_max_point = counts.max().item()
        patch2point_map = cluster.new_zeros(patch_num, patch_max_point)
        patch2point_mask = torch.lt(torch.arange(patch_max_point, device=cluster.device).unsqueeze(0), counts.unsqueeze(-1))
        _, sorted_cluster_indices = torch.sort(cluster)
        patch2point_map[patch2point_mask] = sorted_cluster_indices
        patch_mask = torch.zeros(patch_num, device=union_origin_coord.device).int()
        rand_perm = self.draw("patch_perm", patch_num)
        mask_patch_num = int(patch_num * self.mask_rate)
        patch_mask[rand_perm[0:mask_patch_num]] = 1
        patch_mask[rand_perm[mask_patch_num:mask_patch_num * 2]] = 2
        point_mask = torch.zeros(union_origin_coord.shape[0], device=union_origin_coord.device).int()
        point_mask[patch2point_map[patch_mask == 1][patch2point_mask[patch_mask == 1]]] = 1
        point_mask[patch2point_map[patch_mask == 2][patch2point_mask[patch_mask == 2]]] = 2
        point_mask_split = point_mask.split(torch.stack([view1_batch_count, view2_batch_count], dim=-1).flatten().tolist())
        return torch.cat(point_mask_split[0::2]) == 1, torch.cat(point_mask_split[1::2]) == 2

    # ---- :143-172 ----
    @torch.no_grad()
    def match_contrastive_pair(self, view1_coord, view1_offset, view2_coord, view2_offset, max_k, max_radius):
        if self._kernels(view1_coord):
            count, cand, stats = ops.msc_match(max_k, max_radius, view2_coord.float(), view2_offset.int(), view1_coord.float(),
                                               view1_offset.int())
            n_matched, max_count = stats.tolist()
            r = self.draw("select", max_count, (n_matched,), device=count.device)
            index = ops.msc_select(count, cand, r)
        else:
            index, distance = ops.knn_query(max_k, view2_coord.float(), view2_offset.int(), view1_coord.float(), view1_offset.int())
            index = torch.cat([torch.arange(index.shape[0], device=index.device, dtype=torch.long).view(-1, 1, 1).expand(-1, max_k, 1),
                               index.long().view(-1, max_k, 1)], dim=-1)[distance.squeeze(-1) < max_radius]
            unique, count = index[:, 0].unique(return_counts=True)
            select = torch.cumsum(count, dim=0) - self.draw("select", count.max(), count.shape, device=count.device) % count - 1
            index = index[select]
        if index.shape[0] > self.matching_max_pair:
            index = index[self.draw("pair_perm", index.shape[0])[: self.matching_max_pair].to(index.device)]
        return index

    # ---- :174-203 ----
    def compute_contrastive_loss(self, view1_feat, view1_offset, view2_feat, view2_offset, match_index):
        assert view1_offset.shape == view2_offset.shape
        if self._kernels(view1_feat):
            loss, pos_sim, neg_sim = PF.msc_nce(view1_feat, view2_feat, match_index, self.nce_t)
        else:
            loss, pos_sim, neg_sim = PF.msc_nce_torch(view1_feat, view2_feat, match_index, self.nce_t)
        world = _world_size()
        if world > 1:
            dist.all_reduce(loss)
            dist.all_reduce(pos_sim)
            dist.all_reduce(neg_sim)
        return loss / world, pos_sim / world, neg_sim / world

    def _contrast(self, view1_feat, view1_origin_coord, view1_offset, view2_feat, view2_origin_coord, view2_offset, match_index):
        """forward's call of compute_contrastive_loss; v1m2 passes the origin coordinates as well"""
        return self.compute_contrastive_loss(view1_feat, view1_offset, view2_feat, view2_offset, match_index)

    # ---- :205-310 ----
    def forward(self, data_dict):
        view1_origin_coord = data_dict["view1_origin_coord"]
        view1_coord = data_dict["view1_coord"]
        view1_feat = data_dict["view1_feat"]
        view1_offset = data_dict["view1_offset"].int()
        view2_origin_coord = data_dict["view2_origin_coord"]
        view2_coord = data_dict["view2_coord"]
        view2_feat = data_dict["view2_feat"]
        view2_offset = data_dict["view2_offset"].int()

        view1_point_mask, view2_point_mask = self.generate_cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset)
        view1_mask_tokens = self.mask_token.expand(view1_coord.shape[0], -1)
        view1_weight = view1_point_mask.unsqueeze(-1).type_as(view1_mask_tokens)
        view1_feat = view1_feat * (1 - view1_weight) + view1_mask_tokens * view1_weight
        view2_mask_tokens = self.mask_token.expand(view2_coord.shape[0], -1)
        view2_weight = view2_point_mask.unsqueeze(-1).type_as(view2_mask_tokens)
        view2_feat = view2_feat * (1 - view2_weight) + view2_mask_tokens * view2_weight

        view1_data_dict = dict(origin_coord=view1_origin_coord, coord=view1_coord, feat=view1_feat, offset=view1_offset)
        view2_data_dict = dict(origin_coord=view2_origin_coord, coord=view2_coord, feat=view2_feat, offset=view2_offset)
        if "view1_grid_coord" in data_dict.keys():
            view1_data_dict["grid_coord"] = data_dict["view1_grid_coord"]
        if "view2_grid_coord" in data_dict.keys():
            view2_data_dict["grid_coord"] = data_dict["view2_grid_coord"]

        # view mixing strategy
        if self.draw("mix") < self.view1_mix_prob:
            view1_data_dict["offset"] = torch.cat([view1_offset[1:-1:2], view1_offset[-1].unsqueeze(0)], dim=0)
        if self.draw("mix") < self.view2_mix_prob:
            view2_data_dict["offset"] = torch.cat([view2_offset[1:-1:2], view2_offset[-1].unsqueeze(0)], dim=0)

        view1_feat = self.backbone(view1_data_dict)
        view2_feat = self.backbone(view2_data_dict)
        match_index = self.match_contrastive_pair(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset,
                                                  max_k=self.matching_max_k, max_radius=self.matching_max_radius)
        self.last = dict(view1_point_mask=view1_point_mask, view2_point_mask=view2_point_mask, match_index=match_index)
        nce_loss, pos_sim, neg_sim = self._contrast(view1_feat, view1_origin_coord, view1_offset, view2_feat, view2_origin_coord,
                                                    view2_offset, match_index)
        loss = nce_loss * self.contrast_weight
        result_dict = dict(nce_loss=nce_loss, pos_sim=pos_sim, neg_sim=neg_sim)

        if self.color_head is not None:
            assert "view1_color" in data_dict.keys()
            assert "view2_color" in data_dict.keys()
            view1_color_pred = self.color_head(view1_feat[view1_point_mask])
            view2_color_pred = self.color_head(view2_feat[view2_point_mask])
            color_loss = (torch.sum((view1_color_pred - data_dict["view1_color"][view1_point_mask]) ** 2)
                          + torch.sum((view2_color_pred - data_dict["view2_color"][view2_point_mask]) ** 2)
                          ) / (view1_color_pred.shape[0] + view2_color_pred.shape[0])
            loss = loss + color_loss * self.reconstruct_weight
            result_dict["color_loss"] = color_loss

        if self.normal_head is not None:
            assert "view1_normal" in data_dict.keys()
            assert "view2_normal" in data_dict.keys()
            view1_normal_pred = self.normal_head(view1_feat[view1_point_mask])
            view2_normal_pred = self.normal_head(view2_feat[view2_point_mask])
            view1_normal_pred = view1_normal_pred / (torch.norm(view1_normal_pred, p=2, dim=1, keepdim=True) + 1e-10)
            view2_normal_pred = view2_normal_pred / (torch.norm(view2_normal_pred, p=2, dim=1, keepdim=True) + 1e-10)
            normal_loss = (torch.sum(view1_normal_pred * data_dict["view1_normal"][view1_point_mask])
                           + torch.sum(view2_normal_pred * data_dict["view2_normal"][view2_point_mask])
                           ) / (view1_normal_pred.shape[0] + view2_normal_pred.shape[0])
            loss = loss + normal_loss * self.reconstruct_weight
            result_dict["normal_loss"] = normal_loss

        result_dict["loss"] = loss
        return result_dict


class MaskedSceneContrastCSC(MaskedSceneContrast):
    """MSC-v1m2 (masked_scene_contrast_v1m2_csc.py:24-377): MSC-v1m1 with the contrastive loss split into CSC partitions"""

    def __init__(self, backbone, backbone_in_channels, backbone_out_channels, mask_grid_size=0.1, mask_rate=0.4, view1_mix_prob=0,
                 view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=8192, nce_t=0.4, contrast_weight=1,
                 reconstruct_weight=1, reconstruct_color=True, reconstruct_normal=True, partitions=4, r1=0.125, r2=2):
        super().__init__(backbone, backbone_in_channels, backbone_out_channels, mask_grid_size, mask_rate, view1_mix_prob, view2_mix_prob,
                         matching_max_k, matching_max_radius, matching_max_pair, nce_t, contrast_weight, reconstruct_weight,
                         reconstruct_color, reconstruct_normal)
        self.partitions = partitions
        self.r1 = r1
        self.r2 = r2

    # ---- :202-264 ----
    def compute_contrastive_loss(self, view1_feat, view1_coord, view1_offset, view2_feat, view2_coord, view2_offset, match_index):
        assert view1_offset.shape == view2_offset.shape
        fn = PF.msc_csc_nce if self._kernels(view1_feat) else PF.msc_csc_nce_torch
        loss, pos_sim, neg_sim = fn(view1_feat, view1_coord, view1_offset, view2_feat, view2_coord, match_index, self.nce_t, self.r1,
                                    self.r2, self.partitions)
        world = _world_size()
        if world > 1:
            dist.all_reduce(loss)
            dist.all_reduce(pos_sim)
            dist.all_reduce(neg_sim)
        return loss / world, pos_sim / world, neg_sim / world

    def _contrast(self, view1_feat, view1_origin_coord, view1_offset, view2_feat, view2_origin_coord, view2_offset, match_index):
        return self.compute_contrastive_loss(view1_feat, view1_origin_coord, view1_offset, view2_feat, view2_origin_coord, view2_offset,
                                             match_index)
