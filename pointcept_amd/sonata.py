"""Sonata self-distillation on the engine: drop-in for pointcept/models/sonata/sonata_v1m1_base.py ("Sonata-v1m1"), with the
reference's constructor arguments, state-dict keys (student.*, teacher.*, the weight-norm parametrisation of the prototype layer with
original0 frozen at 1), forward(data_dict) keys, result-dict keys, forward(..., return_point=True) and the trainer hooks
before_train / before_step / after_step.  Registered only when named: compat.register_models(MODELS, names=["Sonata-v1m1"]).
The backbone is the engine's PT-v3m2 (enc_mode, mask_token, traceable pooling).

* The three losses (mask, roll-mask, unmask): functional.sonata_distill -- csrc/sonata.hip keeps the Sinkhorn-Knopp matrix as two
  scaling vectors, reads teacher and student logits through match_index as they are (bf16 under autocast) and stores nothing of
  size pairs x prototypes.  The rolled and the principal-view teacher rows are reached by composing match_index with a row index:
  the rolled / masked copies of the [points, prototypes] logits that the reference makes are not made.  dist.all_reduce on the
  column sums and the row count when the world size is above 1, as there.
* match_neighbour: ops.msc_match(1, match_max_r, ...) -- the nearest point of the other view among the 27 grid cells around the
  query -- and the rows with a match; equal to knn_query(1) + `distance < match_max_r` row for row.  One host read (the row count).
* generate_mask: ops.sonata_patch_rank -- one key sort over (batch, cell) and a run numbering; point_mask = patch_mask[cluster].
  One host read (patch_num, for randperm).
* STAYS IN TORCH: the head (Linear, GELU, Linear, normalise, the weight-normed prototype Linear: library GEMMs, autograd), the
  up-cast concatenation, the EMA (torch._foreach_*) and the schedulers.
* The random draws go through `draw(kind, ...)`: randperm(patch_num) and the mask jitter's randn_like, each made as the reference
  makes it; tests replay recorded draws through it.
* PTC_SONATA=0 (config.SONATA_KERNELS), and CPU tensors: the reference's own expression -- torch.unique over (batch, cell) rows,
  ops.knn_query + radius filter, functional.sonata_distill_torch.
"""
from __future__ import annotations

import math
from itertools import chain

import torch
import torch.distributed as dist
import torch.nn as nn

from . import config as _config
from . import functional as PF
from . import ops
from .compat import build_backbone
from .structure import Point, batch2offset, offset2batch, offset2bincount


def _world_size() -> int:
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class CosineScheduler:
    """pointcept/utils/scheduler.py CosineScheduler as the model uses it: a linear warm-up from start_value to base_value over
    warmup_iters steps (both ends included), then half a cosine from base_value to final_value; final_value from total_iters on."""

    def __init__(self, base_value, final_value, total_iters, start_value=0, warmup_iters=0):
        self.base_value, self.final_value, self.start_value = base_value, final_value, start_value
        self.total_iters, self.warmup_iters = int(total_iters), int(warmup_iters)
        self.iter = 0

    def get(self, it):
        if it >= self.total_iters:
            return self.final_value
        if it < self.warmup_iters:
            if self.warmup_iters == 1:
                return float(self.start_value)
            return self.start_value + (self.base_value - self.start_value) * it / (self.warmup_iters - 1)
        span = self.total_iters - self.warmup_iters
        return self.final_value + 0.5 * (self.base_value - self.final_value) * (1 + math.cos(math.pi * (it - self.warmup_iters) / span))

    def step(self):
        value = self.get(self.iter)
        self.iter += 1
        return value

    def reset(self):
        self.iter = 0

    def __getitem__(self, it):
        return self.get(it)


class OnlineCluster(nn.Module):
    """:27-68: Linear, GELU, Linear, L2 normalisation, a weight-normed prototype layer whose magnitudes are frozen at 1 -- the
    output is the cosine similarity to each prototype.  enable_mlp=False (Concerto's concerto_v1m1_base.py:41-49) leaves the MLP out:
    the input is normalised and meets the prototypes directly."""

    def __init__(self, in_channels, hidden_channels=4096, embed_channels=512, num_prototypes=4096, enable_mlp=True):
        super().__init__()
        if enable_mlp:
            self.mlp = nn.Sequential(nn.Linear(in_channels, hidden_channels), nn.GELU(), nn.Linear(hidden_channels, embed_channels))
        self.apply(self._init_weights)
        self.prototype = torch.nn.utils.parametrizations.weight_norm(nn.Linear(embed_channels, num_prototypes, bias=False))
        self.prototype.parametrizations.weight.original0.data.fill_(1)
        self.prototype.parametrizations.weight.original0.requires_grad = False

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def forward(self, feat):
        if hasattr(self, "mlp"):
            feat = self.mlp(feat)
        eps = 1e-6 if feat.dtype == torch.float16 else 1e-12
        feat = nn.functional.normalize(feat, dim=-1, p=2, eps=eps)
        return self.prototype(feat)


class Sonata(nn.Module):
    """Sonata-v1m1 (sonata_v1m1_base.py:71-532)"""

    def __init__(self, backbone, head_in_channels, head_hidden_channels=4096, head_embed_channels=512, head_num_prototypes=4096,
                 teacher_custom=None, num_global_view=2, num_local_view=4, mask_size_start=0.1, mask_size_base=0.4,
                 mask_size_warmup_ratio=0.05, mask_ratio_start=0.3, mask_ratio_base=0.7, mask_ratio_warmup_ratio=0.05, mask_jitter=None,
                 teacher_temp_start=0.04, teacher_temp_base=0.07, teacher_temp_warmup_ratio=0.05, student_temp=0.1, mask_loss_weight=2 / 8,
                 roll_mask_loss_weight=2 / 8, unmask_loss_weight=4 / 8, momentum_base=0.996, momentum_final=1, match_max_k=8,
                 match_max_r=0.08, up_cast_level=2):
        super().__init__()
        self.mask_loss_weight = mask_loss_weight
        self.roll_mask_loss_weight = roll_mask_loss_weight
        self.unmask_loss_weight = unmask_loss_weight
        self.num_global_view = num_global_view
        self.num_local_view = num_local_view
        self.mask_size = self.mask_size_start = mask_size_start
        self.mask_size_base = mask_size_base
        self.mask_size_warmup_ratio = mask_size_warmup_ratio
        self.mask_size_scheduler = None
        self.mask_ratio = self.mask_ratio_start = mask_ratio_start
        self.mask_ratio_base = mask_ratio_base
        self.mask_ratio_warmup_ratio = mask_ratio_warmup_ratio
        self.mask_ratio_scheduler = None
        self.mask_jitter = mask_jitter
        self.teacher_temp = self.teacher_temp_start = teacher_temp_start
        self.teacher_temp_base = teacher_temp_base
        self.teacher_temp_warmup_ratio = teacher_temp_warmup_ratio
        self.teacher_temp_scheduler = None
        self.student_temp = student_temp
        self.momentum = self.momentum_base = momentum_base
        self.momentum_final = momentum_final
        self.momentum_scheduler = None
        self.match_max_k = match_max_k
        self.match_max_r = match_max_r
        self.up_cast_level = up_cast_level
        assert unmask_loss_weight + mask_loss_weight + roll_mask_loss_weight > 0
        assert num_global_view > 1 or roll_mask_loss_weight == 0
        assert num_global_view == 1 or num_global_view == 2

        student, teacher = dict(), dict()
        student["backbone"] = build_backbone(dict(backbone))
        teacher["backbone"] = build_backbone(dict(backbone, **(teacher_custom or {})))       # e.g. no drop path for the teacher
        head = lambda: OnlineCluster(head_in_channels, head_hidden_channels, head_embed_channels, head_num_prototypes)
        if self.mask_loss_weight > 0 or self.roll_mask_loss_weight > 0:
            student["mask_head"], teacher["mask_head"] = head(), head()
        if self.unmask_loss_weight > 0:
            student["unmask_head"], teacher["unmask_head"] = head(), head()
        self.student = nn.ModuleDict(student)
        self.teacher = nn.ModuleDict(teacher)
        for k, v in self.student.items():
            self.teacher[k].load_state_dict(v.state_dict())
        for p in self.teacher.parameters():
            p.requires_grad = False
        self.last = {}               # the integers of the last forward (masks, clusters, match indices), for tests and tools

    # ---- trainer hooks (:187-265) ----
    def before_train(self):
        total_steps = self.trainer.cfg.scheduler.total_steps
        curr_step = self.trainer.start_epoch * len(self.trainer.train_loader)
        self.mask_size_scheduler = CosineScheduler(start_value=self.mask_size_start, base_value=self.mask_size_base,
                                                   final_value=self.mask_size_base,
                                                   warmup_iters=int(total_steps * self.mask_size_warmup_ratio), total_iters=total_steps)
        self.mask_ratio_scheduler = CosineScheduler(start_value=self.mask_ratio_start, base_value=self.mask_ratio_base,
                                                    final_value=self.mask_ratio_base,
                                                    warmup_iters=int(total_steps * self.mask_ratio_warmup_ratio), total_iters=total_steps)
        self.teacher_temp_scheduler = CosineScheduler(start_value=self.teacher_temp_start, base_value=self.teacher_temp_base,
                                                      final_value=self.teacher_temp_base,
                                                      warmup_iters=int(total_steps * self.teacher_temp_warmup_ratio),
                                                      total_iters=total_steps)
        self.momentum_scheduler = CosineScheduler(base_value=self.momentum_base, final_value=self.momentum_final, total_iters=total_steps)
        for s in (self.mask_size_scheduler, self.mask_ratio_scheduler, self.teacher_temp_scheduler, self.momentum_scheduler):
            s.iter = curr_step

    def before_step(self):
        self.mask_size = self.mask_size_scheduler.step()
        self.mask_ratio = self.mask_ratio_scheduler.step()
        self.teacher_temp = self.teacher_temp_scheduler.step()
        self.momentum = self.momentum_scheduler.step()
        writer = getattr(getattr(self, "trainer", None), "writer", None)
        if writer is not None:
            writer.add_scalar("params/mask_size", self.mask_size, self.mask_size_scheduler.iter)
            writer.add_scalar("params/mask_ratio", self.mask_ratio, self.mask_ratio_scheduler.iter)
            writer.add_scalar("params/teacher_temp", self.teacher_temp, self.teacher_temp_scheduler.iter)
            writer.add_scalar("params/momentum", self.momentum, self.momentum_scheduler.iter)

    def after_step(self):
        with torch.no_grad():
            m = self.momentum
            student_param_list = list(self.student.parameters())
            teacher_param_list = list(self.teacher.parameters())
            torch._foreach_mul_(teacher_param_list, m)
            torch._foreach_add_(teacher_param_list, student_param_list, alpha=1 - m)

    # ---- the random draws, as the reference makes them (:307, :388) ----
    def draw(self, kind, *args, device=None):
        if kind == "patch_perm":
            return torch.randperm(args[0], device=device)
        if kind == "jitter":         # args = (the masked coordinates,)
            return torch.randn_like(args[0])
        raise ValueError(kind)

    @staticmethod
    def _kernels(t: torch.Tensor) -> bool:
        return _config.SONATA_KERNELS and t.is_cuda

    @staticmethod
    def sinkhorn_knopp(feat, temp, num_iter=3):
        return PF.sonata_sinkhorn_torch(feat, temp, num_iter, dist.all_reduce if _world_size() > 1 else None)

    # ---- :293-310 ----
    @torch.no_grad()
    def generate_mask(self, coord, offset):
        batch = offset2batch(offset)
        index = batch.unsqueeze(-1).expand(-1, coord.shape[1])
        min_coord = torch.zeros((offset.numel(), coord.shape[1]), dtype=coord.dtype, device=coord.device).scatter_reduce(
            0, index, coord, "amin", include_self=False)
        grid_coord = ((coord - min_coord[batch]) // self.mask_size).int()
        if self._kernels(coord):
            point_cluster, facts = ops.sonata_patch_rank(grid_coord, batch, offset.numel())
            patch_num, bad = facts.tolist()
            if bad:
                raise ops.PtcoreError("Sonata.generate_mask: a scene spans more than 2^20 mask cells on one axis")
        else:
            unique, point_cluster = torch.unique(torch.cat([batch.unsqueeze(-1), grid_coord], dim=-1), dim=0, sorted=True,
                                                 return_inverse=True)
            patch_num = unique.shape[0]
        mask_patch_num = int(patch_num * self.mask_ratio)
        patch_index = self.draw("patch_perm", patch_num, device=coord.device).to(coord.device)
        patch_mask = torch.zeros(patch_num, dtype=torch.bool, device=coord.device)
        patch_mask[patch_index[:mask_patch_num]] = True
        return patch_mask[point_cluster], point_cluster

    # ---- :312-333 ----
    @torch.no_grad()
    def match_neighbour(self, view1_coord, view1_offset, view2_coord, view2_offset):
        if self._kernels(view1_coord):
            count, cand, _ = ops.msc_match(1, self.match_max_r, view2_coord.float(), view2_offset.int(), view1_coord.float(),
                                           view1_offset.int())
            index1 = torch.nonzero(count > 0)[:, 0]
            return torch.stack([index1, cand[index1, 0].long()], dim=-1)
        index2, distance = ops.knn_query(1, view2_coord.float(), view2_offset.int(), view1_coord.float(), view1_offset.int())
        index1 = torch.arange(index2.shape[0], device=index2.device, dtype=torch.long).unsqueeze(-1)
        return torch.cat([index1, index2.long()], dim=-1)[distance.squeeze(-1) < self.match_max_r]

    # ---- :335-348 ----
    def _roll_rows(self, offset):
        """the row order of roll_point: [pc1, pc1', pc2, pc2'] -> [pc1', pc1, pc2', pc2]"""
        n = self.num_global_view
        bs = len(offset) // n
        rows = torch.arange(int(offset[-1]) if len(offset) else 0, device=offset.device).split(offset2bincount(offset).tolist())
        return list(chain(*[rows[n * b: n * (b + 1)][::-1] for b in range(bs)]))

    @torch.no_grad()
    def roll_point(self, point):
        rows = self._roll_rows(point.offset)
        index = torch.cat(rows, dim=0)
        data_dict = {}
        for key in point.keys():
            if key in ["feat", "coord", "origin_coord"]:
                data_dict[key] = point[key][index]
            elif key == "batch":
                data_dict[key] = torch.cat([torch.ones_like(point.batch[r]) * i for i, r in enumerate(rows)], dim=0)
        return Point(data_dict)

    # ---- :350-358 ----
    def up_cast(self, point):
        for _ in range(self.up_cast_level):
            assert "pooling_parent" in point.keys()
            assert "pooling_inverse" in point.keys()
            parent = point.pop("pooling_parent")
            inverse = point.pop("pooling_inverse")
            parent.feat = torch.cat([parent.feat, point.feat[inverse]], dim=-1)
            point = parent
        return point

    def distill_loss(self, teacher_sim, student_sim, match_index, student_batch, num_scenes):
        """:437-454: the Sinkhorn-Knopp targets of the matched teacher rows against the matched student rows, averaged per scene
        and over the scenes"""
        return PF.sonata_distill(teacher_sim, student_sim, match_index, student_batch, self.teacher_temp, self.student_temp,
                                 all_reduce=dist.all_reduce if _world_size() > 1 else None, num_scenes=num_scenes)

    # ---- :360-532 ----
    def forward(self, data_dict, return_point=False):
        if return_point:
            point = self.teacher.backbone(data_dict)
            return dict(point=self.up_cast(point))

        with torch.no_grad():
            global_point = Point(feat=data_dict["global_feat"], coord=data_dict["global_coord"],
                                 origin_coord=data_dict["global_origin_coord"], offset=data_dict["global_offset"],
                                 grid_size=data_dict["grid_size"][0])
            global_mask, global_cluster = self.generate_mask(global_point.coord, global_point.offset)
            mask_global_coord = global_point.coord.clone().detach()
            if self.mask_jitter is not None:
                mask_global_coord[global_mask] += torch.clip(self.draw("jitter", mask_global_coord[global_mask]).mul(self.mask_jitter),
                                                             max=self.mask_jitter * 2)
            mask_global_point = Point(feat=data_dict["global_feat"], coord=mask_global_coord,
                                      origin_coord=data_dict["global_origin_coord"], mask=global_mask,
                                      offset=data_dict["global_offset"], grid_size=data_dict["grid_size"][0])
            local_point = Point(feat=data_dict["local_feat"], coord=data_dict["local_coord"], origin_coord=data_dict["local_origin_coord"],
                                offset=data_dict["local_offset"], grid_size=data_dict["grid_size"][0])
            result_dict = dict(loss=[])
            global_point_ = self.up_cast(self.teacher.backbone(global_point))
            global_feat = global_point_.feat
        self.last = dict(global_mask=global_mask, global_cluster=global_cluster)

        if self.mask_loss_weight > 0 or self.roll_mask_loss_weight > 0:
            with torch.no_grad():
                teacher_sim = self.teacher.mask_head(global_feat)
            mask_global_point_ = self.up_cast(self.student.backbone(mask_global_point))
            mask_pred_sim = self.student.mask_head(mask_global_point_.feat)
            scenes = mask_global_point_.offset.numel()

            if self.mask_loss_weight > 0:
                match_index = self.match_neighbour(mask_global_point_.origin_coord, mask_global_point_.offset,
                                                   global_point_.origin_coord, global_point_.offset)
                self.last["mask_match_index"] = match_index
                mask_loss = self.distill_loss(teacher_sim, mask_pred_sim, match_index, mask_global_point_.batch, scenes)
                result_dict["mask_loss"] = mask_loss
                result_dict["loss"].append(mask_loss * self.mask_loss_weight)

            if self.roll_mask_loss_weight > 0:
                with torch.no_grad():
                    rows = self._roll_rows(global_point_.offset)
                    roll_index = torch.cat(rows, dim=0)
                    match_index = self.match_neighbour(mask_global_point_.origin_coord, mask_global_point_.offset,
                                                       global_point_.origin_coord[roll_index],
                                                       torch.cumsum(torch.tensor([r.numel() for r in rows], device=roll_index.device), 0))
                    self.last["roll_mask_match_index"] = match_index
                    # row j of the rolled teacher is row roll_index[j] of the teacher: its logits are not copied
                    match_index = torch.stack([match_index[:, 0], roll_index[match_index[:, 1]]], dim=-1)
                roll_mask_loss = self.distill_loss(teacher_sim, mask_pred_sim, match_index, mask_global_point_.batch, scenes)
                result_dict["roll_mask_loss"] = roll_mask_loss
                result_dict["loss"].append(roll_mask_loss * self.roll_mask_loss_weight)

        if self.unmask_loss_weight > 0:
            with torch.no_grad():
                teacher_sim = self.teacher.unmask_head(global_feat)
            local_point_ = self.up_cast(self.student.backbone(local_point))
            unmask_pred_sim = self.student.unmask_head(local_point_.feat)
            with torch.no_grad():
                principal_view_mask = global_point_.batch % self.num_global_view == 0
                principal_rows = torch.nonzero(principal_view_mask)[:, 0]
                principal_view_batch = global_point_.batch[principal_rows] // self.num_global_view
                match_index = self.match_neighbour(local_point_.origin_coord,
                                                   local_point_.offset[self.num_local_view - 1:: self.num_local_view],
                                                   global_point_.origin_coord[principal_rows], batch2offset(principal_view_batch))
                self.last["unmask_match_index"] = match_index
                match_index = torch.stack([match_index[:, 0], principal_rows[match_index[:, 1]]], dim=-1)
            unmask_loss = self.distill_loss(teacher_sim, unmask_pred_sim, match_index, local_point_.batch, local_point_.offset.numel())
            result_dict["unmask_loss"] = unmask_loss
            result_dict["loss"].append(unmask_loss * self.unmask_loss_weight)
        result_dict["loss"] = sum(result_dict["loss"])

        if _world_size() > 1:
            for loss in result_dict.values():
                dist.all_reduce(loss, op=dist.ReduceOp.AVG)
        return result_dict
