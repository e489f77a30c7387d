"""Context-aware classifier on the engine: drop-in for pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py
("CAC-v1m1"), with the reference's constructor arguments and defaults, state-dict keys (backbone.*, seg_head.*, proj.0/2.*,
apd_proj.0/2.*, feat_proj_layer.0/1/3.*), its three forward modes and result-dict keys.  Registered only when named:
compat.register_models(MODELS, names=["CAC-v1m1"]).

* post_refine_proto_batch: functional.cac_pool_soft (softmax, confidence gate and the [K, n] x [n, C] pooling of every scene in one
  launch, nothing of size [N, K] stored) -> proj on the [S, K, 2C] prototypes -> functional.cac_cos_logits (row norms in the kernel).
* get_adaptive_perspective: functional.cac_pool_hard (one pass instead of one pass per class present; no unique(), no host read) ->
  apd_proj -> functional.cac_cos_logits.
* get_distill_loss: functional.cac_distill (row losses, entropies and the per-class sums; no [N, K] temporaries, no unique()).
* BatchNorm order: in train mode feat_proj_layer runs once per scene inside the refinement and then once on the whole batch in the
  adaptive branch, as in the reference -- running_mean / running_var / num_batches_tracked (B + 1 after one forward) follow it; the
  scene boundaries are the forward's one host read.  In eval mode the projection runs on the whole batch at once.
* Linear and BatchNorm1d are the engine's; the criteria (CrossEntropyLoss, LovaszLoss with loss_weight / ignore_index) map onto
  functional.cross_entropy / lovasz_softmax (both up to 1024 classes; above 64 the Lovasz kernels sort the classes present only: ~56 B x
  present classes x points of workspace, one host read of their number per call); an already built callable is taken as is; any other
  criterion type is refused by name.
* Autocast: the kernels take fp32.  Under autocast their inputs are cast with .float() (functional.cac_*), the Linear layers follow
  autocast as everywhere in the engine.
* PTC_CAC=0 (config.CAC_KERNELS), CPU tensors, and shapes the kernels refuse (K outside 2..256, C not a multiple of 16 up to 128)
  take functional.cac_*_torch: the reference's own expression, loops included.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import config as _config
from . import functional as PF
from . import nn as PNN
from . import ops
from .compat import build_backbone
from .criteria import Criteria
from .structure import Point


class CACSegmentor(nn.Module):
    """CAC-v1m1 (context_aware_classifier_v1m1_base.py:17-275)"""

    def __init__(self, num_classes, backbone_out_channels, backbone=None, criteria=None, cos_temp=15, main_weight=1, pre_weight=1,
                 pre_self_weight=1, kl_weight=1, conf_thresh=0, detach_pre_logits=False):
        super().__init__()
        self.num_classes = num_classes
        self.cos_temp = cos_temp
        self.main_weight = main_weight
        self.pre_weight = pre_weight
        self.pre_self_weight = pre_self_weight
        self.kl_weight = kl_weight
        self.conf_thresh = conf_thresh
        self.detach_pre_logits = detach_pre_logits
        c = backbone_out_channels
        self.backbone = build_backbone(backbone)
        self.seg_head = PNN.Linear(c, num_classes)
        self.proj = nn.Sequential(PNN.Linear(c * 2, c * 2, bias=False), PNN.ReLU(), PNN.Linear(c * 2, c))
        self.apd_proj = nn.Sequential(PNN.Linear(c * 2, c * 2, bias=False), PNN.ReLU(), PNN.Linear(c * 2, c))
        self.feat_proj_layer = nn.Sequential(PNN.Linear(c, c, bias=False), PNN.BatchNorm1d(c), PNN.ReLU(), PNN.Linear(c, c))
        self.criteria = criteria if callable(criteria) else Criteria(criteria, "CAC-v1m1", row_terms=False)
        self.last = {}               # integers of the last forward (rows past the gate per scene, class counts), for tests and tools

    def _kernels(self, feat: torch.Tensor) -> bool:
        return bool(_config.CAC_KERNELS and feat.is_cuda and ops.cac_supported(self.num_classes, feat.shape[1]))

    def _project(self, x):
        for m, act in PNN.plain_feature_runs(self.feat_proj_layer):
            x = m(x) if act is None else m(x, act=act)
        return x

    def _project_scenes(self, x, offset):
        """feat_proj_layer as the refinement applies it: per scene in train mode (the BatchNorm statistics are the scene's)"""
        if not self.training:
            return self._project(x)
        ends = offset.tolist()
        return torch.cat([self._project(x[start:end]) for start, end in zip([0] + ends[:-1], ends)], 0)

    # ---- :66-71 ----
    @staticmethod
    def get_pred(x, proto):
        return PF.cac_cos_logits_torch(x, proto)

    # ---- :73-96 (times cos_temp) ----
    def get_adaptive_perspective(self, feat, target, new_proto, proto):
        if self._kernels(feat):
            new_proto, count = PF.cac_pool_hard(feat, target, new_proto, 1e-4)
        else:
            new_proto, count = PF.cac_pool_hard_torch(feat, target, new_proto, 1e-4)
        self.last["class_count"] = count
        new_proto = self.apd_proj(torch.cat([new_proto, proto], -1))
        raw_feat = self._project(feat)
        if self._kernels(feat):
            return PF.cac_cos_logits(raw_feat, new_proto, None, self.cos_temp)
        return PF.cac_cos_logits_torch(raw_feat, new_proto, None, self.cos_temp)

    # ---- :98-150 (times cos_temp) ----
    def post_refine_proto_batch(self, feat, pred, proto, offset=None):
        if self.detach_pre_logits:
            pred = pred.detach()
        pool = PF.cac_pool_soft if self._kernels(feat) else PF.cac_pool_soft_torch
        pred_proto, _, passed = pool(feat, pred, offset, self.conf_thresh, 1e-7)
        self.last["passed"] = passed
        pred_proto = torch.cat([pred_proto, proto.unsqueeze(0).expand(pred_proto.shape[0], -1, -1).to(pred_proto.dtype)], -1)
        pred_proto = self.proj(pred_proto)
        x = self._project(feat) if offset is None else self._project_scenes(feat, offset)
        cos = PF.cac_cos_logits if self._kernels(feat) else PF.cac_cos_logits_torch
        return cos(x, pred_proto, offset, self.cos_temp)

    # ---- :152-199 ----
    def get_distill_loss(self, pred, soft, target, smoothness=0.5, eps=0):
        if _config.CAC_KERNELS and pred.is_cuda and 2 <= pred.shape[1] <= 256:
            return PF.cac_distill(pred, soft, target, smoothness, eps)
        return PF.cac_distill_torch(pred, soft, target, smoothness, eps)

    # ---- :201-275 ----
    def forward(self, data_dict):
        offset = data_dict["offset"]
        point = self.backbone(data_dict)
        feat = point.feat if isinstance(point, Point) else point
        seg_logits = self.seg_head(feat)
        self.last = {}
        if self.training:
            target = data_dict["segment"]
            pre_logits = seg_logits.clone()
            refine_logits = self.post_refine_proto_batch(feat=feat, pred=seg_logits, proto=self.seg_head.weight.squeeze(), offset=offset)
            cac_pred = self.get_adaptive_perspective(feat=feat, target=target, new_proto=self.seg_head.weight.detach().data.squeeze(),
                                                     proto=self.seg_head.weight.squeeze())
            seg_loss = self.criteria(refine_logits, target) * self.main_weight
            pre_loss = self.criteria(cac_pred, target) * self.pre_weight
            pre_self_loss = self.criteria(pre_logits, target) * self.pre_self_weight
            kl_loss = self.get_distill_loss(pred=refine_logits, soft=cac_pred.detach(), target=target) * self.kl_weight
            loss = seg_loss + pre_loss + pre_self_loss + kl_loss
            return dict(loss=loss, seg_loss=seg_loss, pre_loss=pre_loss, pre_self_loss=pre_self_loss, kl_loss=kl_loss)
        refine_logits = self.post_refine_proto_batch(feat=feat, pred=seg_logits, proto=self.seg_head.weight.squeeze(), offset=offset)
        if "segment" in data_dict.keys():
            loss = self.criteria(seg_logits, data_dict["segment"])
            return dict(loss=loss, seg_logits=refine_logits)
        return dict(seg_logits=refine_logits)
