"""PointGroup on the engine: drop-in for pointcept/models/point_group/point_group_v1m1_base.py ("PG-v1m1") and
point_group_v1m2_custom_criteria.py ("PG-v1m2"), with the reference's constructor arguments, state-dict keys (backbone.*,
bias_head.{0,1,3}.*, seg_head.*) and return dicts.  Registered only when named: compat.register_models(MODELS, names=["PG-v1m1"]).

* Heads: the engine's Linear and BatchNorm1d(eps=1e-3, momentum=0.01) with the ReLU fused into the norm pass.  Semantic loss on the
  cross-entropy / Lovasz kernels; the masked L1 + negative-cosine offset losses in one fused pass each way (csrc/pg_cluster.hip).
* Eval: centres, softmax and the ignore mask stay on the device.  Ignored points are not compacted: they get batch index -1, so they
  have no neighbours and seed no cluster, which leaves every other point's list, cluster and seed as the reference computes them on
  the compacted points.  Ball query -> clustering -> per-cluster scores read the host twice (nActive, the cluster counts); then the
  per-cluster (count, class, score) and the dense masks are copied out.
* When every point is ignored the outputs are empty; the reference raises IndexError there (proposals_idx[:, 1] on a 1-D tensor).
* PTC_PG_CLUSTER=0: the reference's own eval expression with the torch ball query and the host BFS, and the reference's loss
  expression (A/B baseline).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import config as _config
from . import functional as PF
from . import nn as PNN
from . import ops
from .compat import build_backbone  # noqa: F401  (its first home; kept importable from here)
from .structure import Point, batch2offset, offset2batch


class _Criteria:
    """build_criteria(criteria) of point_group_v1m2 (losses/builder.py:22-31) on the engine's loss kernels: CrossEntropyLoss and
    multiclass LovaszLoss with the reference's default settings (losses/misc.py, losses/lovasz.py); other settings raise.  Both serve up
    to 1024 classes; above 64 LovaszLoss sorts the classes present only (functional.lovasz_softmax: ~56 B x present classes x points of
    workspace and one host read of their number per call)"""

    SUPPORTED = {
        "CrossEntropyLoss": ("cross_entropy", dict(weight=None, size_average=None, reduce=None, reduction="mean", label_smoothing=0.0)),
        "LovaszLoss": ("lovasz_softmax", dict(mode="multiclass", class_seen=None, per_image=False)),
    }

    def __init__(self, cfg):
        self.terms = []
        for c in cfg or []:
            c = dict(c)
            kind = c.pop("type")
            w = float(c.pop("loss_weight", 1.0))
            ignore = int(c.pop("ignore_index", -1))
            if kind not in self.SUPPORTED:
                raise ValueError(f"PG-v1m2 criteria: {kind} is not on the engine's loss kernels")
            fn, defaults = self.SUPPORTED[kind]
            other = {k: v for k, v in c.items() if k not in defaults or defaults[k] != v}
            if other:       # any other setting would silently train a different loss
                raise ValueError(f"PG-v1m2 criteria: {kind} with {other} is not on the engine's loss kernels")
            self.terms.append((getattr(PF, fn), w, ignore))

    def __call__(self, pred, target):
        loss = 0
        for fn, w, ignore in self.terms:
            loss = loss + fn(pred, target, ignore) * w
        return loss


class PointGroup(nn.Module):
    """PG-v1m1 (point_group_v1m1_base.py:22-179)"""

    def __init__(self, backbone, backbone_out_channels=64, semantic_num_classes=20, semantic_ignore_index=-1,
                 segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300,
                 cluster_propose_points=100, cluster_min_points=50, voxel_size=0.02):
        super().__init__()
        self.semantic_num_classes = semantic_num_classes
        self.segment_ignore_index = segment_ignore_index
        self.semantic_ignore_index = semantic_ignore_index
        self.instance_ignore_index = instance_ignore_index
        self.cluster_thresh = cluster_thresh
        self.cluster_closed_points = cluster_closed_points
        self.cluster_propose_points = cluster_propose_points
        self.cluster_min_points = cluster_min_points
        self.voxel_size = voxel_size
        self.backbone = build_backbone(backbone)
        c = backbone_out_channels
        self.bias_head = nn.Sequential(PNN.Linear(c, c), PNN.BatchNorm1d(c, eps=1e-3, momentum=0.01), PNN.ReLU(), PNN.Linear(c, 3))
        self.seg_head = PNN.Linear(c, semantic_num_classes)

    # ---- pieces shared with v1m2 ----
    def seg_loss(self, logit_pred, segment):
        return PF.cross_entropy(logit_pred, segment, self.semantic_ignore_index)

    def features(self, data_dict):
        return self.backbone(data_dict)

    def heads(self, feat):
        x = feat
        for m, act in PNN.plain_feature_runs(self.bias_head):
            x = m(x) if act is None else m(x, act=act)
        return x, self.seg_head(feat)

    def forward(self, data_dict):
        return self._forward_heads(data_dict, self.features(data_dict))

    def _forward_heads(self, data_dict, feat):
        coord = data_dict["coord"]
        instance_centroid = data_dict["instance_centroid"]
        offset = data_dict["offset"]
        bias_pred, logit_pred = self.heads(feat)
        if "segment" in data_dict.keys() and "instance" in data_dict.keys():
            segment = data_dict["segment"]
            instance = data_dict["instance"]
            seg_loss = self.seg_loss(logit_pred, segment)
            if _config.PG_CLUSTER:
                bias_l1_loss, bias_cosine_loss = PF.pg_bias_loss(bias_pred, coord, instance_centroid, instance, self.instance_ignore_index)
            else:
                bias_l1_loss, bias_cosine_loss = PF.pg_bias_loss_torch(bias_pred, coord, instance_centroid, instance,
                                                                       self.instance_ignore_index)
            loss = seg_loss + bias_l1_loss + bias_cosine_loss
            return_dict = dict(loss=loss, seg_loss=seg_loss, bias_l1_loss=bias_l1_loss, bias_cosine_loss=bias_cosine_loss)
        else:
            return_dict = dict()
        if not self.training:
            proposals = self._proposals if _config.PG_CLUSTER else self._proposals_torch
            scores, masks, classes = proposals(coord, bias_pred, logit_pred, offset)
            return_dict["pred_scores"] = scores
            return_dict["pred_masks"] = masks
            return_dict["pred_classes"] = classes
        return return_dict

    def _centres_and_segments(self, coord, bias_pred, logit_pred):
        center_pred = coord + bias_pred
        center_pred /= self.voxel_size
        prob = F.softmax(logit_pred, dim=-1)
        segment_pred = torch.max(prob, 1)[1]
        ignored = torch.zeros_like(segment_pred, dtype=torch.bool)
        for index in self.segment_ignore_index:
            ignored |= segment_pred == index
        return center_pred, prob, segment_pred, ignored

    @torch.no_grad()
    def _proposals(self, coord, bias_pred, logit_pred, offset):
        center_pred, prob, segment_pred, ignored = self._centres_and_segments(coord, bias_pred, logit_pred)
        n = center_pred.shape[0]
        batch = torch.where(ignored, torch.full_like(segment_pred, -1), offset2batch(offset, n))
        label = torch.where(ignored, torch.full_like(segment_pred, -1), segment_pred).to(torch.int32)
        idx, start_len, _ = ops.pg_ball_query(center_pred, batch, offset.numel(), float(self.cluster_thresh))   # host read 1
        cidx, coff = ops.pg_cluster(label, idx, start_len, self.cluster_min_points, skip_negative=True)      # host read 2
        count, cls, score = ops.pg_proposal_scores(logit_pred, label, cidx, coff)    # softmax(logits)[member, class], fp32
        stats = torch.stack([count.float(), cls.float(), score]).cpu()                                        # output copies
        keep = stats[0] > self.cluster_propose_points
        p = int(keep.sum())
        if p == 0:
            return torch.tensor([]), torch.zeros((0, n), dtype=torch.int32), torch.tensor([])
        row = torch.full((keep.numel(),), -1, dtype=torch.int64)
        row[keep] = torch.arange(p)
        masks = ops.pg_proposal_masks(cidx, row.to(cidx.device), p, n).cpu()
        return stats[2][keep].contiguous(), masks, stats[1][keep].to(torch.int64)

    @torch.no_grad()
    def _proposals_torch(self, coord, bias_pred, logit_pred, offset):
        """point_group_v1m1_base.py:101-179 with the torch ball query and the host BFS"""
        center_pred, logit_pred, segment_pred, ignored = self._centres_and_segments(coord, bias_pred, logit_pred)
        mask = ~ignored
        if mask.sum() == 0:
            proposals_idx = torch.zeros((0, 2)).int()
            proposals_offset = torch.zeros(1).int()
        else:
            center_pred_ = center_pred[mask]
            segment_pred_ = segment_pred[mask]
            batch_ = offset2batch(offset, center_pred.shape[0])[mask]
            offset_ = nn.ConstantPad1d((1, 0), 0)(batch2offset(batch_))
            idx, start_len = PF.pg_ball_query_torch(center_pred_, batch_.int(), offset_.cpu(), float(self.cluster_thresh))
            proposals_idx, proposals_offset = PF.pg_bfs_cluster_host(segment_pred_.int().cpu(), idx.cpu(), start_len.cpu(),
                                                                     self.cluster_min_points)
            proposals_idx[:, 1] = mask.nonzero().view(-1).cpu()[proposals_idx[:, 1].long()].int()
        proposals_pred = torch.zeros((proposals_offset.shape[0] - 1, center_pred.shape[0]), dtype=torch.int)
        proposals_pred[proposals_idx[:, 0].long(), proposals_idx[:, 1].long()] = 1
        instance_pred = segment_pred.cpu()[proposals_idx[:, 1][proposals_offset[:-1].long()].long()]
        proposals_mask = proposals_pred.sum(1) > self.cluster_propose_points
        proposals_pred = proposals_pred[proposals_mask]
        instance_pred = instance_pred[proposals_mask]
        if len(proposals_pred) == 0:
            return torch.tensor([]), proposals_pred, torch.tensor([])
        lp = logit_pred.float().cpu()
        scores = torch.stack([lp[proposals_pred[k].bool(), instance_pred[k]].mean() for k in range(len(proposals_pred))])
        return scores, proposals_pred, instance_pred


class PointGroupV1m2(PointGroup):
    """PG-v1m2 (point_group_v1m2_custom_criteria.py:25-203): configurable semantic criteria, freeze_backbone, return_point and the
    pooling_parent unwinding of a Point-returning backbone"""

    def __init__(self, backbone, backbone_out_channels=64, semantic_num_classes=20, semantic_ignore_index=-1,
                 segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300,
                 cluster_propose_points=100, cluster_min_points=50, voxel_size=0.02, criteria=None, freeze_backbone=False):
        super().__init__(backbone, backbone_out_channels, semantic_num_classes, semantic_ignore_index, segment_ignore_index,
                         instance_ignore_index, cluster_thresh, cluster_closed_points, cluster_propose_points, cluster_min_points,
                         voxel_size)
        self.seg_criteria = _Criteria(criteria)
        self.freeze_backbone = freeze_backbone
        if self.freeze_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False

    def seg_loss(self, logit_pred, segment):
        return self.seg_criteria(logit_pred, segment)

    def forward(self, data_dict, return_point=False):
        if return_point:
            return dict(point=self.backbone(data_dict))
        point = self.backbone(data_dict)
        if isinstance(point, Point) or (isinstance(point, dict) and "feat" in point):
            while "pooling_parent" in point.keys():
                assert "pooling_inverse" in point.keys()
                parent = point.pop("pooling_parent")
                inverse = point.pop("pooling_inverse")
                parent.feat = torch.cat([parent.feat, point.feat[inverse]], dim=-1)
                point = parent
            feat = point.feat
        else:
            feat = point
        return self._forward_heads(data_dict, feat)
