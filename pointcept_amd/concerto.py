"""Concerto joint 2D-3D self-supervised pretraining on the engine: drop-in for pointcept/models/concerto/concerto_v1m1_base.py
("Concerto-v1m1"), with the reference's constructor arguments and defaults, state-dict keys (enc2d_model.*, patch_proj.*,
enc2d_head_student.*, enc2d_head_teacher.* -- built and never called, as there --, student.*, teacher.*), forward(data_dict) result
keys (mask_loss, roll_mask_loss, unmask_loss, enc2d_loss, loss), forward(..., return_point=True) and the trainer hooks.  Registered
only when named: compat.register_models(MODELS, names=["Concerto-v1m1"]).  Built on sonata.py: the schedulers, generate_mask,
match_neighbour, the rolled rows, the recorded draws and the distillation loss (functional.sonata_distill) are Sonata's.

What differs from Sonata (:575-872):
* the teacher applies ONE head to the global view for all three distillation losses: mask_head when either mask weight is positive,
  else unmask_head;
* the EMA moves the heads always and the backbone only when sonata_model_type == "online" (the offline teacher is a loaded Sonata
  checkpoint); the prototypes of enc2d_head_teacher are copied from enc2d_head_student;
* the 2D-3D term (:745-866), here on csrc/concerto.hip:
    - the student's masked global view is up-cast enc2d_upcast_level - up_cast_level levels further;
    - pool_corr: functional.concerto_pool_corr per pooling level -- one launch for all images -- on the cluster CSR the m2 pooling
      recorded (`_ptc_pool_csr`; nothing is sorted again);
    - functional.concerto_patch_pairs: the (point, image) pairs of the first global view of every scene binned by image patch -- a key
      sort, the sorted unique patch ids and a CSR; the dense [all patches, C] tensor of the reference's scatter_mean is never made;
    - functional.concerto_patch_mean: the mean 3D feature of the U patches that hold a pair, gather-form backward;
    - patch_proj on those U rows only (functional.linear);
    - functional.concerto_align_loss: the mean-centred cosine against the frozen image encoder's patch features, read through the
      patch ids, forward and gradient in one kernel.
  ONE DIFFERENCE from the reference: a pair whose pooled pixel coordinate truncates outside [0, patch_h) x [0, patch_w), or whose image
  index is at or beyond its scene's img_num, aliases into another image's patches there; here it is left out (on both paths).
* `enc2d_model=`: a module passed here IS the frozen image encoder and load_enc2d (transformers' AutoModel.from_pretrained) is not
  called -- what class_embedding= is to the PPT classes.
* self.last additionally records the integers of the branch: the pooled correspondence of every level, the patch ids, the pair count.
* PTC_CONCERTO=0 (config.CONCERTO_KERNELS), and CPU tensors: the reference's own expression -- the dense scatter_mean, patch_proj over
  every patch, torch.unique, two gathers, CosineSimilarity.
* STAYS IN TORCH: the image encoder and the three ENC2D_forward conventions, the up-cast concatenations, the EMA.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn as nn

from . import config as _config
from . import functional as PF
from .compat import build_backbone
from .sonata import OnlineCluster, Sonata, _world_size
from .structure import Point, batch2offset


class Concerto(Sonata):
    """Concerto-v1m1 (concerto_v1m1_base.py:81-872)"""

    def __init__(self, image_weight_name, image_weight_path, backbone, head_in_channels, backbone_out_channels, embedding_channels, patch_w,
                 patch_h, student_pretrained_path=None, teacher_pretrained_path=None, student_pretrained=False, head_hidden_channels=4096,
                 head_embed_channels=512, head_num_prototypes=4096, enc2d_head_in_channels=384, enc2d_head_hidden_channels=4096,
                 enc2d_head_embed_channels=256, enc2d_head_num_prototypes=384, teacher_custom=None, num_global_view=2, num_local_view=4,
                 mask_size_start=0.1, mask_size_base=0.4, mask_size_warmup_ratio=0.05, mask_ratio_start=0.3, mask_ratio_base=0.7,
                 mask_ratio_warmup_ratio=0.05, mask_jitter=None, teacher_temp_start=0.04, teacher_temp_base=0.07,
                 teacher_temp_warmup_ratio=0.05, student_temp=0.1, mask_loss_weight=2 / 10, roll_mask_loss_weight=2 / 10,
                 unmask_loss_weight=4 / 10, enc2d_loss_weight=2 / 10, momentum_base=0.996, momentum_final=1, match_max_k=8,
                 match_max_r=0.08, up_cast_level=2, enc2d_upcast_level=4, enc2d_cos_shift=True, sonata_model_type="offline",
                 enc2d_model=None):
        nn.Module.__init__(self)
        assert sonata_model_type in ["online", "offline"]
        self.mask_loss_weight = mask_loss_weight
        self.roll_mask_loss_weight = roll_mask_loss_weight
        self.unmask_loss_weight = unmask_loss_weight
        self.enc2d_loss_weight = enc2d_loss_weight
        self.num_global_view = num_global_view
        self.num_local_view = num_local_view
        self.mask_size = self.mask_size_start = mask_size_start
        self.mask_size_base = mask_size_base
        self.mask_size_warmup_ratio = mask_size_warmup_ratio
        self.mask_ratio = self.mask_ratio_start = mask_ratio_start
        self.mask_ratio_base = mask_ratio_base
        self.mask_ratio_warmup_ratio = mask_ratio_warmup_ratio
        self.teacher_temp = self.teacher_temp_start = teacher_temp_start
        self.teacher_temp_base = teacher_temp_base
        self.teacher_temp_warmup_ratio = teacher_temp_warmup_ratio
        self.mask_size_scheduler = self.mask_ratio_scheduler = self.teacher_temp_scheduler = self.momentum_scheduler = None
        self.mask_jitter = mask_jitter
        self.student_temp = student_temp
        self.momentum = self.momentum_base = momentum_base
        self.momentum_final = momentum_final
        self.match_max_k = match_max_k
        self.match_max_r = match_max_r
        self.up_cast_level = up_cast_level
        self.enc2d_upcast_level = enc2d_upcast_level
        assert unmask_loss_weight + mask_loss_weight + roll_mask_loss_weight + enc2d_loss_weight > 0
        assert num_global_view > 1 or roll_mask_loss_weight == 0
        assert num_global_view == 1 or num_global_view == 2

        student, teacher = dict(), dict()
        student_backbone = build_backbone(dict(backbone))
        if student_pretrained_path is not None:
            student_backbone = self.load_sonata(student_backbone, path=student_pretrained_path)
        teacher_backbone = build_backbone(dict(backbone, **(teacher_custom or {})))       # e.g. no drop path for the teacher
        if sonata_model_type == "offline":
            if teacher_pretrained_path is None:
                raise ValueError('Concerto: sonata_model_type="offline" loads the teacher from teacher_pretrained_path')
            teacher_backbone = self.load_sonata(teacher_backbone, path=teacher_pretrained_path)
        student["backbone"], teacher["backbone"] = student_backbone, teacher_backbone

        if self.enc2d_loss_weight > 0:
            self.patch_h, self.patch_w = patch_h, patch_w
            self.image_weight_name = image_weight_name
            self.enc2d_model = enc2d_model if enc2d_model is not None else self.load_enc2d(image_weight_name, image_weight_path)
            self.enc2d_model.requires_grad_(False)
            self._num_channels = enc2d_head_in_channels
            self.patch_proj = nn.Linear(backbone_out_channels, self._num_channels)
            enc2d_head = lambda **kw: OnlineCluster(enc2d_head_in_channels, enc2d_head_hidden_channels, enc2d_head_in_channels,
                                                    enc2d_head_num_prototypes, **kw)
            self.enc2d_head_student = enc2d_head()                       # built, kept in step by after_step, never called (:239-245)
            self.enc2d_head_teacher = enc2d_head(enable_mlp=False)
            self.enc2d_head_student.prototype.load_state_dict(self.enc2d_head_teacher.prototype.state_dict())
            for p in self.enc2d_head_teacher.parameters():
                p.requires_grad = False

        head = lambda: OnlineCluster(head_in_channels, head_hidden_channels, head_embed_channels, head_num_prototypes)
        if self.mask_loss_weight > 0 or self.roll_mask_loss_weight > 0:
            student["mask_head"], teacher["mask_head"] = head(), head()
        if self.unmask_loss_weight > 0:
            student["unmask_head"], teacher["unmask_head"] = head(), head()
        if self.enc2d_loss_weight > 0 and self.unmask_loss_weight + self.mask_loss_weight + self.roll_mask_loss_weight == 0:
            student["unmask_head"], teacher["unmask_head"] = head(), head()
        self.student = nn.ModuleDict(student)
        self.teacher = nn.ModuleDict(teacher)
        for k, v in self.student.items():
            if "head" in k:
                self.teacher[k].load_state_dict(v.state_dict())
        if sonata_model_type == "online":
            self.teacher.backbone.load_state_dict(self.student.backbone.state_dict())
        for p in self.teacher.parameters():
            p.requires_grad = False
        self.enc2d_cos_shift = enc2d_cos_shift
        self.sonata_model_type = sonata_model_type
        self.last = {}

    # ---- :284-306 ----
    def load_enc2d(self, model_name, model_weight):
        from transformers import AutoModel

        return AutoModel.from_pretrained(model_weight, trust_remote_code=True).eval()

    def load_sonata(self, model, path):
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        checkpoint = torch.load(path, map_location=device)
        weight, found = {}, False
        if "state_dict" in checkpoint.keys():
            checkpoint = checkpoint["state_dict"]
            for key, value in checkpoint.items():
                if "module.student.backbone." in key:
                    found = True
                    weight[key.replace("module.student.backbone.", "module.")[7:]] = value      # module.xxx.xxx -> xxx.xxx
        info = model.load_state_dict(weight if found else checkpoint)
        print(f"Missing keys: {info[0]}")
        print(f"Unexpected keys: {info[1]}")
        return model

    # ---- :308-325 ----
    @torch.no_grad()
    def ENC2D_forward(self, x):
        if "radio" in self.image_weight_name:                     # RADIO: (summary, features)
            _, features = self.enc2d_model(x)
            return features.reshape(-1, self.patch_h * self.patch_w, self._num_channels)
        if hasattr(self.enc2d_model, "vision_model"):             # SigLIPv2
            return self.enc2d_model.vision_model(x).last_hidden_state
        return self.enc2d_model(x).last_hidden_state[:, -self.patch_h * self.patch_w:, :]     # DINOv2.5: register tokens in front

    # ---- :398-429 ----
    def after_step(self):
        with torch.no_grad():
            m = self.momentum
            if self.sonata_model_type == "online":
                student_param_list = list(self.student.backbone.parameters())
                teacher_param_list = list(self.teacher.backbone.parameters())
                torch._foreach_mul_(teacher_param_list, m)
                torch._foreach_add_(teacher_param_list, student_param_list, alpha=1 - m)
            student_param_list = [p for n, p in self.student.named_parameters() if "head" in n]
            teacher_param_list = [p for n, p in self.teacher.named_parameters() if "head" in n]
            torch._foreach_mul_(teacher_param_list, m)
            torch._foreach_add_(teacher_param_list, student_param_list, alpha=1 - m)
            if self.enc2d_loss_weight > 0:
                src = [p for n, p in self.enc2d_head_student.named_parameters() if "prototype" in n]
                dst = [p for n, p in self.enc2d_head_teacher.named_parameters() if "prototype" in n]
                torch._foreach_copy_(dst, src)

    force_kernels = None             # tests: True runs the branch on the kernels whatever the device (the host emulation)

    def _kernels_2d(self, t: torch.Tensor) -> bool:
        return bool(_config.CONCERTO_KERNELS and t.is_cuda) if self.force_kernels is None else bool(self.force_kernels)

    # ---- :514-526 ----
    def up_cast(self, point, upcast_level=None):
        for _ in range(self.up_cast_level if upcast_level is None else upcast_level):
            assert "pooling_parent" in point.keys()
            assert "pooling_inverse" in point.keys()
            parent = point.pop("pooling_parent")
            inverse = point.pop("pooling_inverse")
            parent.feat = torch.cat([parent.feat, point.feat[inverse]], dim=-1)
            point = parent
        return point

    # ---- :528-573 ----
    @staticmethod
    @torch.no_grad()
    def pool_corr(point, correspondence, levels=None, use_kernels=None):
        """the correspondences of the input points pooled down the chain to `point`; `levels` (a list) receives every level's result"""
        point_feat = dict(offset=point.offset, feat=point.feat)
        chain = []
        while "pooling_parent" in point.keys():
            assert "pooling_inverse" in point.keys()
            assert "idx_ptr" in point.keys()
            csr = point["_ptc_pool_csr"] if "_ptc_pool_csr" in point.keys() else None
            parent = point.pop("pooling_parent")
            inverse = point.pop("pooling_inverse")
            idx_ptr = point.pop("idx_ptr")
            chain.append((torch.sort(inverse)[1], idx_ptr) if csr is None else csr)
            point = parent
        for perm, idx_ptr in reversed(chain):
            correspondence = PF.concerto_pool_corr(correspondence, perm, idx_ptr, use_kernels=use_kernels)
            if levels is not None:
                levels.append(correspondence)
        point_feat["correspondence"] = correspondence
        return Point(point_feat)

    def _enc2d_loss_reference(self, feature3d, correspondence, scene, img_offset, img_num, feature2d):
        """:786-842 as the reference writes it (PTC_CONCERTO=0, CPU tensors): scatter_mean into a dense [all patches, C] tensor,
        patch_proj over all of it, torch.unique and two gathers"""
        pairs = PF.concerto_patch_pairs_torch(correspondence, scene, img_offset, img_num, 0, self.patch_h, self.patch_w)
        point = pairs.perm
        feature_index = torch.repeat_interleave(pairs.patch_ids, pairs.indptr[1:] - pairs.indptr[:-1])
        total = torch.zeros((feature2d.shape[0], feature3d.shape[1]), dtype=feature3d.dtype, device=feature3d.device)
        total = total.index_add(0, feature_index, feature3d[point])
        count = torch.bincount(feature_index, minlength=feature2d.shape[0]).clamp(min=1).to(feature3d.dtype)
        feature3d_mask = self.patch_proj(total / count.unsqueeze(-1))
        feature_index = torch.unique(feature_index)
        return pairs, PF.concerto_align_loss_torch(feature2d, feature_index, feature3d_mask[feature_index], self.enc2d_cos_shift, 1e-6)

    # ---- :753-853 ----
    def alignment_loss(self, point, global_correspondence, img_num, images=None, feature2d=None):
        """The 2D-3D term from the up-cast student point on: pool_corr, the patch binning, the patch means, patch_proj and the centred
        cosine.  None when the batch holds no image.  feature2d [all patches, C]: the image encoder's output where the caller
        already has it (tools/concerto_step.py times the point side alone); otherwise ENC2D_forward(images)."""
        levels = []
        point_batch = point.batch
        use_kernels = self._kernels_2d(point.feat)
        to_feature = self.pool_corr(point, global_correspondence, levels, use_kernels)
        with torch.no_grad():
            # the first global view of every scene (enc2d_mask, :756-777) and the scene of each of its points
            rows = torch.nonzero(point_batch % self.num_global_view == 0)[:, 0]
            scene = point_batch[rows] // self.num_global_view
            img_num = img_num.to(rows.device).long()
            img_offset = torch.cumsum(img_num, 0) - img_num
            total_img_num = int(img_num.sum())
        correspondence = to_feature["correspondence"]
        self.last.update(pooled_correspondence=levels, total_img_num=total_img_num)
        if total_img_num == 0:
            return None
        if feature2d is None:
            with torch.no_grad():
                feature2d = self.ENC2D_forward(images)
                feature2d = feature2d.contiguous().view(-1, feature2d.shape[-1])
        if use_kernels:
            pairs = PF.concerto_patch_pairs(correspondence, scene, img_offset, img_num, total_img_num, self.patch_h, self.patch_w,
                                            rows=rows, use_kernels=True)
            feature3d_mask = PF.concerto_patch_mean(to_feature["feat"], pairs, use_kernels=True)
            if pairs.num_patches and feature3d_mask.is_cuda:
                feature3d_mask = PF.linear(feature3d_mask, self.patch_proj.weight, self.patch_proj.bias)
            else:
                feature3d_mask = self.patch_proj(feature3d_mask)
            loss = PF.concerto_align_loss(feature2d, pairs.patch_ids, feature3d_mask, self.enc2d_cos_shift, 1e-6, use_kernels=True)
        else:
            pairs, loss = self._enc2d_loss_reference(to_feature["feat"][rows], correspondence[rows], scene, img_offset, img_num, feature2d)
        self.last.update(patch_ids=pairs.patch_ids, num_pairs=pairs.num_pairs)
        return loss

    # ---- :575-872 ----
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
            mask_global = dict(feat=data_dict["global_feat"], coord=mask_global_coord, origin_coord=data_dict["global_origin_coord"],
                               mask=global_mask, offset=data_dict["global_offset"], grid_size=data_dict["grid_size"][0])
            local_point = Point(feat=data_dict["local_feat"], coord=data_dict["local_coord"], origin_coord=data_dict["local_origin_coord"],
                                offset=data_dict["local_offset"], grid_size=data_dict["grid_size"][0])
            result_dict = dict(loss=[])
            global_point_ = self.up_cast(self.teacher.backbone(global_point))
            # one shared teacher head for the masked and the unmasked views; mask (global) before unmask (local)
            if self.mask_loss_weight > 0 or self.roll_mask_loss_weight > 0:
                teacher_sim = self.teacher.mask_head(global_point_.feat)
            else:
                teacher_sim = self.teacher.unmask_head(global_point_.feat)
        self.last = dict(global_mask=global_mask, global_cluster=global_cluster)
        mask_global_point_ = None

        if self.mask_loss_weight > 0 or self.roll_mask_loss_weight > 0:
            mask_global_point_ = self.up_cast(self.student.backbone(Point(mask_global)))
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
                    match_index = torch.stack([match_index[:, 0], roll_index[match_index[:, 1]]], dim=-1)
                roll_mask_loss = self.distill_loss(teacher_sim, mask_pred_sim, match_index, mask_global_point_.batch, scenes)
                result_dict["roll_mask_loss"] = roll_mask_loss
                result_dict["loss"].append(roll_mask_loss * self.roll_mask_loss_weight)

        if self.unmask_loss_weight > 0:
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

        if self.enc2d_loss_weight > 0:
            if self.mask_loss_weight == 0 or self.roll_mask_loss_weight == 0:
                mask_global_point_ = self.up_cast(self.student.backbone(Point(mask_global)))
            mask_global_point_enc2d = self.up_cast(mask_global_point_, upcast_level=self.enc2d_upcast_level - self.up_cast_level)
            loss = self.alignment_loss(mask_global_point_enc2d, data_dict["global_correspondence"], data_dict["img_num"],
                                       images=data_dict["images"])
            if loss is not None:
                result_dict["enc2d_loss"] = loss
                result_dict["loss"].append(loss * self.enc2d_loss_weight)
            elif self.mask_loss_weight + self.unmask_loss_weight + self.roll_mask_loss_weight > 0:
                result_ssl_loss = sum(result_dict["loss"]) / (self.mask_loss_weight + self.unmask_loss_weight + self.roll_mask_loss_weight)
                result_dict["enc2d_loss"] = result_ssl_loss
                result_dict["loss"].append(result_ssl_loss * self.enc2d_loss_weight)
        result_dict["loss"] = sum(result_dict["loss"])

        if _world_size() > 1:
            for loss in result_dict.values():
                dist.all_reduce(loss, op=dist.ReduceOp.AVG)
        return result_dict
