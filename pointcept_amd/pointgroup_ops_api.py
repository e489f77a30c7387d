"""Mirror of libs/pointgroup_ops (`import pointgroup_ops`; functions/functions.py:1-176): ballquery_batch_p, bfs_cluster,
BallQueryBatchP, BFSCluster and Clustering with the reference's signatures and return dtypes, on csrc/pg_cluster.hip.
Installed only on request: pointcept_amd.compat.install(pointgroup=True).

* ballquery_batch_p(coords, batch_idxs, batch_offsets, radius, meanActive) -> (idx [nActive] int32, start_len [n, 2] int32) on the
  device.  The output is sized exactly, so meanActive is accepted and ignored (no retry).  Each list holds the first 1000 neighbours
  in ascending index order, as the reference's kernel finds them; the starts are a deterministic exclusive scan (the reference's
  atomicAdd cursor orders them arbitrarily).  d2 is the reference's unfused fp32 expression; nvcc may contract it into FMAs, so the
  CUDA build can differ from this one by an ulp exactly at d2 == radius^2.
* bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold) -> (cluster_idxs [sumNPoint, 2] int32, cluster_offsets
  [nCluster + 1] int32).  CPU tensors in, CPU tensors out, as the reference's; the clustering itself runs on the GPU.  Cluster order,
  membership and each cluster's first row (its seed) are the reference's; inside a cluster the members are listed in ascending point
  order instead of BFS order.  The lists are taken to be ball-query lists: symmetric (j in list(i) iff i in list(j)) unless one of
  them holds 1000 entries (possibly truncated); components with such a list follow the sequential BFS rule exactly, every other
  component is resolved as an undirected one.  Arbitrary asymmetric lists shorter than 1000 entries are outside that contract.
  List bounds are checked (on the host copies, or with a few small reads of device inputs) before any kernel reads them.
* Both accept tensors of the device they are given; without a GPU the engine's operators refuse to run (no CPU fallback).
PTC_PG_CLUSTER=0: the chunked brute-force torch ball query and the host BFS (functional.pg_ball_query_torch / pg_bfs_cluster_host).
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import config as _config
from . import functional as PF
from . import ops
from ._lib import PtcoreError


class BallQueryBatchP(Function):
    @staticmethod
    def forward(ctx, coords, batch_idxs, batch_offsets, radius, meanActive):
        assert coords.is_contiguous() and batch_idxs.is_contiguous() and batch_offsets.is_contiguous()
        if not _config.PG_CLUSTER:
            return PF.pg_ball_query_torch(coords, batch_idxs, batch_offsets.cpu(), float(radius))
        idx, start_len, _ = ops.pg_ball_query(coords, batch_idxs, batch_offsets.numel() - 1, float(radius))
        return idx, start_len

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None


ballquery_batch_p = BallQueryBatchP.apply


def _check_lists(idx: torch.Tensor, start_len: torch.Tensor, n: int) -> None:
    """bounds of the lists before any kernel reads them (a few small host reads when the lists live on the device)"""
    if start_len.dim() != 2 or start_len.shape[1] != 2:
        raise PtcoreError(f"bfs_cluster: start_len must be [N, 2], got {tuple(start_len.shape)}")
    if n == 0:
        return
    s, ln = start_len[:, 0].long(), start_len[:, 1].long()
    s_min, ln_min, end_max = [int(v) for v in torch.stack([s.min(), ln.min(), (s + ln).max()]).tolist()]
    if s_min < 0 or ln_min < 0 or end_max > idx.numel():
        raise PtcoreError("bfs_cluster: start_len addresses entries outside ball_query_idxs")
    if idx.numel():
        i_min, i_max = [int(v) for v in torch.stack([idx.min(), idx.max()]).tolist()]
        if i_min < 0 or i_max >= n:
            raise PtcoreError("bfs_cluster: ball_query_idxs holds a point index outside [0, N)")


class BFSCluster(Function):
    @staticmethod
    def forward(ctx, semantic_label, ball_query_idxs, start_len, threshold):
        N = start_len.size(0)
        assert semantic_label.is_contiguous()
        assert ball_query_idxs.is_contiguous()
        assert start_len.is_contiguous()
        if not _config.PG_CLUSTER:
            return PF.pg_bfs_cluster_host(semantic_label, ball_query_idxs, start_len, int(threshold))
        on_host = not start_len.is_cuda
        _check_lists(ball_query_idxs, start_len, N)
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else start_len.device
        ci, co = ops.pg_cluster(semantic_label.to(dev, torch.int32), ball_query_idxs.to(dev, torch.int32),
                                start_len.to(dev, torch.int32), int(threshold))
        return (ci.cpu(), co.cpu()) if on_host else (ci, co)

    @staticmethod
    def backward(ctx, a=None):
        return None


bfs_cluster = BFSCluster.apply


class Clustering:
    """functions.py:47-150, unchanged in behaviour: its scatter / gather run on the tensors' own devices"""

    def __init__(self, ignored_labels, class_mapping, thresh=0.03, closed_points=300, min_points=50, propose_points=100,
                 score_func=torch.max) -> None:
        self.ignored_labels = ignored_labels
        self.thresh = thresh
        self.closed_points = closed_points
        self.min_points = min_points
        self.class_mapping = class_mapping
        self.propose_points = propose_points
        self.score_func = score_func

    def cluster(self, vertices, scores):
        labels = torch.max(scores, 1)[1]
        proposals_idx, proposals_offset = self.cluster_(vertices, labels)
        proposals_pred = torch.zeros((proposals_offset.shape[0] - 1, vertices.shape[0]), dtype=torch.int)
        proposals_pred[proposals_idx[:, 0].long(), proposals_idx[:, 1].long()] = 1
        labels = labels[proposals_idx[:, 1][proposals_offset[:-1].long()].long()]
        proposals_pointnum = proposals_pred.sum(1)
        npoint_mask = proposals_pointnum > self.propose_points
        proposals_pred = proposals_pred[npoint_mask]
        labels = labels[npoint_mask]
        return proposals_pred, labels

    def cluster_(self, vertices, labels):
        batch_idxs = torch.zeros_like(labels)
        mask_non_ignored = torch.ones_like(labels).bool()
        for ignored_label in self.ignored_labels:
            mask_non_ignored = mask_non_ignored & (self.class_mapping[labels] != ignored_label)
        object_idxs = mask_non_ignored.nonzero().view(-1)
        vertices_ = vertices[object_idxs].float()
        labels_ = labels[object_idxs].int()
        if vertices_.numel() == 0:
            return torch.zeros((0, 2)).int(), torch.zeros(1).int()
        batch_idxs_ = batch_idxs[object_idxs].int()
        batch_offsets_ = torch.FloatTensor([0, object_idxs.shape[0]]).int().cuda()
        idx, start_len = ballquery_batch_p(vertices_, batch_idxs_, batch_offsets_, self.thresh, self.closed_points)
        proposals_idx, proposals_offset = bfs_cluster(labels_.cpu(), idx.cpu(), start_len.cpu(), self.min_points)
        proposals_idx[:, 1] = object_idxs.cpu()[proposals_idx[:, 1].long()].int()
        return proposals_idx, proposals_offset

    def get_instances(self, vertices, scores):
        proposals_pred, labels = self.cluster(vertices, scores)
        instances = {}
        for proposal_id in range(len(proposals_pred)):
            clusters_i = proposals_pred[proposal_id]
            score = scores[clusters_i.bool().to(scores.device), labels[proposal_id]]
            score = self.score_func(score)
            instances[proposal_id] = {}
            instances[proposal_id]["conf"] = score.cpu().numpy()
            instances[proposal_id]["label_id"] = self.class_mapping.cpu()[labels[proposal_id]]
            instances[proposal_id]["pred_mask"] = clusters_i.cpu().numpy()
        return instances
