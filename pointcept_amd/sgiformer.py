"""SGIFormer on the engine: drop-in for pointcept/models/sgiformer/sgiformer_v1m1_base.py ("SGIFormer-v1m1") with loss.py and nms.py,
with the reference's constructor arguments and defaults, result-dict keys and state-dict keys (backbone.*, decoder.seg_head.*,
decoder.bias_head.*, decoder.feat_proj.*, decoder.rep_layer.*, decoder.query_learn.weight, decoder.sp_feat_proj.*, decoder.x_mask.*,
decoder.sp_pos.gauss_B, decoder.{cross,self,feat_query,feat_self}_attn_layers.N.attn.{in_proj_weight,in_proj_bias,out_proj.weight,
out_proj.bias}, ...norm.*, decoder.ffn_layers.N.net.{0,3}.*, decoder.out_norm.*, decoder.out_cls.*, decoder.out_score.*).  Registered
only when named: compat.register_models(MODELS, names=["SGIFormer-v1m1"]); the shipped config
(configs/scannetpp/insseg-sgiformer-v1m1-0-ptv3-base.py) puts it on PT-v3m1.

* The four attentions of a decoder layer (query <- superpoint with the predicted mask, query self, superpoint <- query, superpoint
  self) run on functional.sgi_attention: all scenes of the batch in one launch, ragged, nothing of size [heads, Lq, Lk] in memory.  The
  reference loops over scenes and lets nn.MultiheadAttention return its head-averaged probabilities.  The projections of
  nn.MultiheadAttention are the engine's Linear under torch's parameter names.
* forward_head's attention mask is bit-packed for all scenes in one launch (functional.sgi_pack_mask); the rule (sigmoid < 0.5, a row
  that would be fully masked is cleared) guarantees the attention kernel its open key per row.
* The matcher's cost matrices of all scenes of a level come from one launch (functional.sgi_match_cost) and reach the host in ONE
  copy per level; the assignment itself is scipy.optimize.linear_sum_assignment, as in the reference.
* prepare_target: functional.sgi_targets (integer counts, no [N, instances] one-hot).  Points with instance == -1 count towards the
  size of their superpoint and towards nothing else: the reference's torch_scatter.scatter(segment_, instance_, reduce="max") (:566)
  indexes with -1 there, which the CUDA library leaves undefined; the engine and the golden generator define it as "such rows are
  skipped".  The ground-truth mask bit is 2 count > superpoint size, the reference's `mean > 0.5` for a true (not floored) mean.
* Superpoint pooling: torch.unique on batch << 48 | superpoint as in the reference, then the engine's segment kernels.
* Left on torch in this port: the query sampler (top-k, rep_layer's softmax over rows, act.T @ feat), norm_query @ sp_mask_feat.T, the
  class-weighted cross entropies, the per-scene losses on the matched rows, mask_matrix_nms (at most topk_insts rows).
* Attention-probability dropout is not implemented by the kernels: dropout must be 0 (the shipped value); drop-path lives in the
  backbone and is untouched.
* PTC_SGI=0 (config.SGI_KERNELS), CPU tensors and head dims other than 32 take functional.sgi_*_torch: the reference's own expression,
  loops included.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as PF
from . import nn as PNN
from .compat import build_backbone
from .structure import Point


def _bounds(counts):
    out, at = [], 0
    for n in counts:
        out.append((at, at + int(n)))
        at += int(n)
    return out


class PositionEmbeddingCoordsSine(nn.Module):
    """the decoder's Fourier position code (:26-187; only pos_type="fourier" is used by SGIFormerDecoder and ported): coordinates scaled
    to [0, 1] per scene, times 2 pi, projected by the fixed Gaussian matrix `gauss_B` [d_in, d_pos / 2] -> (sin, cos).  No gradient."""

    def __init__(self, temperature=10000, normalize=False, scale=None, pos_type="fourier", d_pos=None, d_in=3, gauss_scale=1.0):
        super().__init__()
        if pos_type != "fourier":
            raise NotImplementedError("PositionEmbeddingCoordsSine: only pos_type='fourier' is ported (the decoder's)")
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        assert d_pos is not None and d_pos % 2 == 0
        self.temperature, self.normalize, self.pos_type, self.d_pos = temperature, normalize, pos_type, d_pos
        self.scale = 2 * torch.pi if scale is None else scale
        self.register_buffer("gauss_B", torch.empty((d_in, d_pos // 2)).normal_() * gauss_scale)

    @torch.no_grad()
    def forward(self, xyz, num_channels=None, input_range=None):
        """xyz [n, d_in] of ONE scene, input_range = (min [d_in], max [d_in]) -> [n, num_channels]"""
        d_out = (self.gauss_B.shape[1] * 2 if num_channels is None else num_channels) // 2
        assert 0 < d_out <= self.gauss_B.shape[1]
        xyz = xyz.float()
        if self.normalize:
            xyz = (xyz - input_range[0][None]) / (input_range[1][None] - input_range[0][None])
        proj = torch.mm(xyz * (2 * torch.pi), self.gauss_B[:, :d_out].float())
        return torch.cat([proj.sin(), proj.cos()], dim=1)


class _MultiheadAttention(nn.Module):
    """nn.MultiheadAttention(d_model, nhead, batch_first=True)'s parameters under its names and initialisation; the projections on the
    engine's GEMM, the attention of all scenes in one functional.sgi_attention"""

    def __init__(self, d_model, nhead):
        super().__init__()
        assert d_model % nhead == 0
        self.embed_dim, self.num_heads = d_model, nhead
        self.in_proj_weight = nn.Parameter(torch.empty((3 * d_model, d_model)))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = PNN.Linear(d_model, d_model)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, query, key, value, lq, lk, mask=None):
        e, h = self.embed_dim, self.num_heads
        w, b = self.in_proj_weight, self.in_proj_bias
        q = PF.linear(query, w[:e], b[:e]).view(-1, h, e // h)
        k = PF.linear(key, w[e:2 * e], b[e:2 * e]).view(-1, h, e // h)
        v = PF.linear(value, w[2 * e:], b[2 * e:]).view(-1, h, e // h)
        out = PF.sgi_attention(q, k, v, lq, lk, mask)
        return self.out_proj(out.reshape(-1, e))


def _no_attention_dropout(dropout):
    if dropout != 0.0:
        raise NotImplementedError("SGIFormer on the engine: attention-probability dropout is not in the kernels; dropout must be 0")


class CrossAttentionLayer(nn.Module):
    """:190-224 on the rows of all scenes at once"""

    def __init__(self, d_model=256, nhead=8, dropout=0.0):
        super().__init__()
        _no_attention_dropout(dropout)
        self.attn = _MultiheadAttention(d_model, nhead)
        self.norm = PNN.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, source, query, lk, lq, attn_masks=None, pe=None, query_pe=None):
        q = query if query_pe is None else query + query_pe
        k = source if pe is None else source + pe
        output = self.attn(q, k, source, lq, lk, attn_masks)
        return self.norm(self.dropout(output) + query)


class SelfAttentionLayer(nn.Module):
    """:227-248 on the rows of all scenes at once"""

    def __init__(self, d_model=256, nhead=8, dropout=0.0):
        super().__init__()
        _no_attention_dropout(dropout)
        self.attn = _MultiheadAttention(d_model, nhead)
        self.norm = PNN.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, lx, pe=None):
        q = x if pe is None else x + pe
        output = self.attn(q, q, x, lx, lx)
        return self.norm(self.dropout(output) + x)


class FFN(nn.Module):
    """:251-270"""

    def __init__(self, d_model, hidden_dim, dropout=0.0, activation_fn="relu"):
        super().__init__()
        self.net = nn.Sequential(PNN.Linear(d_model, hidden_dim), PNN.ReLU() if activation_fn == "relu" else PNN.GELU(), nn.Dropout(dropout),
                                 PNN.Linear(hidden_dim, d_model), nn.Dropout(dropout))
        self.norm = PNN.LayerNorm(d_model)

    def forward(self, x):
        return self.norm(self.net(x) + x)


class SGIFormerDecoder(nn.Module):
    """:273-478.  Queries and superpoints of all scenes are kept as ragged row blocks ([S * Lq, d] and [sum M_i, d]); the lists of the
    reference's result dict are views of them."""

    def __init__(self, dec_num_layer=3, num_sample_query=200, num_learn_query=200, num_classes=18, in_channel=32, d_model=256, nhead=8,
                 hidden_dim=1024, dropout=0.0, activation_fn="relu", attn_mask=True, use_score=False, alpha=0.4):
        super().__init__()
        norm_fn = lambda c: PNN.BatchNorm1d(c, eps=1e-3, momentum=0.01)  # noqa: E731
        self.use_score = use_score
        self.dec_num_layer = dec_num_layer
        self.num_classes = num_classes
        self.d_model = d_model
        self.attn_mask = attn_mask
        self.alpha = alpha
        self.seg_head = nn.Sequential(PNN.Linear(in_channel, in_channel), norm_fn(in_channel), PNN.ReLU(), PNN.Linear(in_channel, num_classes + 1))
        self.bias_head = nn.Sequential(PNN.Linear(in_channel, in_channel), norm_fn(in_channel), PNN.ReLU(), PNN.Linear(in_channel, 3))
        self.feat_proj = nn.Sequential(PNN.Linear(in_channel, d_model), PNN.LayerNorm(d_model), PNN.ReLU())
        self.rep_layer = nn.Sequential(PNN.Linear(d_model, num_sample_query), PNN.LayerNorm(num_sample_query), PNN.ReLU())
        self.query_learn = nn.Embedding(num_learn_query, d_model)
        self.sp_feat_proj = nn.Sequential(PNN.Linear(in_channel, d_model), PNN.LayerNorm(d_model), PNN.ReLU())
        self.x_mask = nn.Sequential(PNN.Linear(d_model, d_model), PNN.ReLU())
        self.sp_pos = PositionEmbeddingCoordsSine(pos_type="fourier", d_pos=d_model, normalize=True)
        self.feat_query_attn_layers = nn.ModuleList([])
        self.feat_self_attn_layers = nn.ModuleList([])
        self.cross_attn_layers = nn.ModuleList([])
        self.self_attn_layers = nn.ModuleList([])
        self.ffn_layers = nn.ModuleList([])
        for i in range(self.dec_num_layer):
            self.cross_attn_layers.append(CrossAttentionLayer(d_model, nhead, dropout))
            self.self_attn_layers.append(SelfAttentionLayer(d_model, nhead, dropout))
            self.ffn_layers.append(FFN(d_model, hidden_dim, dropout, activation_fn))
            if i < self.dec_num_layer - 1:
                self.feat_query_attn_layers.append(CrossAttentionLayer(d_model, nhead, dropout))
                self.feat_self_attn_layers.append(SelfAttentionLayer(d_model, nhead, dropout))
        self.out_norm = PNN.LayerNorm(d_model)
        self.out_cls = nn.Sequential(PNN.Linear(d_model, d_model), PNN.ReLU(), PNN.Linear(d_model, num_classes + 1))
        if self.use_score:
            self.out_score = nn.Sequential(PNN.Linear(d_model, d_model), PNN.ReLU(), PNN.Linear(d_model, 1))

    def forward_head(self, query, sp_mask_feat, lq, lk):
        """:359-381 -> (cls list, score list | None, mask list, packed attention masks | None)"""
        norm_query = self.out_norm(query)
        qb, kb = _bounds(lq), _bounds(lk)
        pred_cls = self.out_cls(norm_query)
        pred_cls_list = [pred_cls[a:b] for a, b in qb]
        pred_score_list = None
        if self.use_score:
            pred_score = self.out_score(norm_query)
            pred_score_list = [pred_score[a:b] for a, b in qb]
        pred_mask_list = [torch.einsum("nd, md->nm", norm_query[a:b], sp_mask_feat[c:d]) for (a, b), (c, d) in zip(qb, kb)]
        attn_masks = PF.sgi_pack_mask(pred_mask_list) if self.attn_mask else None
        return pred_cls_list, pred_score_list, pred_mask_list, attn_masks

    def forward(self, point):
        seg_logits = self.seg_head(point.feat)
        bias = self.bias_head(point.feat)
        n_list, lk = point.bincount_host, point.sp_bincount_host
        pb, kb = _bounds(n_list), _bounds(lk)

        # get query (:390-415; torch)
        score = seg_logits.softmax(dim=-1)[:, :-1]
        feat_proj = self.feat_proj(point.feat)
        query_list = []
        for a, b in pb:
            score_ = score[a:b]
            max_score_, _ = score_.max(dim=-1)
            _, topk_idx = max_score_.topk(int(self.alpha * score_.shape[0]), sorted=False)
            top_proj_feat_ = feat_proj[a:b][topk_idx, :]
            rep_ = self.rep_layer(top_proj_feat_)
            act_ = torch.softmax(rep_, dim=0)
            query_ = act_.T @ top_proj_feat_.to(act_.dtype)
            query_list.append(torch.cat((query_, self.query_learn.weight.to(query_.dtype)), dim=0))
        lq = [q.shape[0] for q in query_list]
        query = torch.cat(query_list, 0)

        # get pos (:417-431)
        with torch.no_grad():
            sp_coord = PF.segment_csr((point.coord + bias.detach().to(point.coord.dtype)).float(), point.sp_indptr, "mean", point.sp_perm, True)
            sp_pos = torch.cat([self.sp_pos(sp_coord[a:b], num_channels=self.d_model, input_range=(sp_coord[a:b].min(0)[0], sp_coord[a:b].max(0)[0]))
                                for a, b in kb], 0)
        sp_feat = self.sp_feat_proj(point.sp_feat)
        sp_mask_feat = self.x_mask(sp_feat)

        # decoding (:433-462)
        aux_pred_list = [self.forward_head(query, sp_mask_feat, lq, lk)]
        attn_masks = aux_pred_list[-1][-1]
        for i in range(self.dec_num_layer):
            source = sp_feat + sp_pos.to(sp_feat.dtype)
            query = self.cross_attn_layers[i](source, query, lk, lq, attn_masks)
            query = self.self_attn_layers[i](query, lq)
            query = self.ffn_layers[i](query)
            if i < self.dec_num_layer - 1:
                sp_feat = self.feat_query_attn_layers[i](query, sp_feat, lq, lk, query_pe=sp_pos.to(sp_feat.dtype))
                sp_feat = self.feat_self_attn_layers[i](sp_feat, lk, sp_pos.to(sp_feat.dtype))
            aux_pred_list.append(self.forward_head(query, sp_mask_feat, lq, lk))
            attn_masks = aux_pred_list[-1][-1]
        pred_cls_list, pred_score_list, pred_mask_list, _ = aux_pred_list.pop(-1)
        return {
            "cls_list": pred_cls_list,
            "score_list": pred_score_list,
            "mask_list": pred_mask_list,
            "aux_pred_list": [{"cls_list": c, "score_list": s, "mask_list": m} for c, s, m, _ in aux_pred_list],
            "seg_logits": seg_logits,
            "bias": bias,
        }


# ---- loss.py ----
def get_iou(inputs, targets):
    binarized_inputs = (inputs.sigmoid() >= 0.5).float()
    targets = (targets > 0.5).float()
    intersection = (binarized_inputs * targets).sum(-1)
    union = targets.sum(-1) + binarized_inputs.sum(-1) - intersection
    return intersection / (union + 1e-6)


def dice_loss(inputs, targets):
    inputs = inputs.sigmoid()
    numerator = 2 * (inputs * targets).sum(-1)
    denominator = inputs.sum(-1) + targets.sum(-1)
    return (1 - (numerator + 1) / (denominator + 1)).mean()


class HungarianMatcher:
    """loss.py:387-434 for the three costs of the shipped configs (QueryClassificationCost, MaskBCECost, MaskDiceCost), every scene of
    a level at once: the cost matrices from functional.sgi_match_cost, one device -> host copy, scipy's assignment per scene."""

    COSTS = ("QueryClassificationCost", "MaskBCECost", "MaskDiceCost")

    def __init__(self, costs):
        w = {}
        for c in costs:
            c = dict(c)
            kind = c.pop("type")
            if kind not in self.COSTS or kind in w or set(c) != {"weight"}:
                raise ValueError(f"SGIFormer matcher: cost {kind} {c} is not one of {self.COSTS} with a weight")
            w[kind] = float(c["weight"])
        self.weights = tuple(w.get(k, 0.0) for k in self.COSTS)

    @torch.no_grad()
    def __call__(self, pred_cls_list, pred_mask_list, targets):
        """-> per scene (query ids, object ids) int64 on the device; empty for a scene without instances"""
        from scipy.optimize import linear_sum_assignment

        dev = pred_mask_list[0].device
        costs = PF.sgi_match_cost(pred_mask_list, pred_cls_list, targets.masks, targets.cls, self.weights)
        shapes = [c.shape for c in costs]
        flat = torch.cat([c.reshape(-1) for c in costs]).cpu().numpy()       # the level's one copy
        out, at = [], 0
        for lq, g in shapes:
            if g == 0:
                out.append((torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)))
                continue
            q_ids, o_ids = linear_sum_assignment(flat[at:at + lq * g].reshape(lq, g))
            at += lq * g
            out.append((torch.as_tensor(q_ids, dtype=torch.int64, device=dev), torch.as_tensor(o_ids, dtype=torch.int64, device=dev)))
        return out


class SGIFormerLoss(nn.Module):
    """loss.py:124-328"""

    def __init__(self, matcher, loss_weight, non_object_weight, num_classes, fix_dice_loss_weight, iter_matcher, fix_mean_loss=False,
                 semantic_ignore_index=-1, loss_cls_type="ce_loss"):
        super().__init__()
        if isinstance(matcher, dict):
            m = dict(matcher)
            if m.pop("type") != "HungarianMatcher":
                raise ValueError(f"SGIFormer criteria: matcher {matcher['type']} is not ported")
            matcher = HungarianMatcher(**m)
        self.matcher = matcher
        self.class_weight = [1] * num_classes + [non_object_weight]
        self.loss_weight = loss_weight
        self.num_classes = num_classes
        self.fix_dice_loss_weight = fix_dice_loss_weight
        self.iter_matcher = iter_matcher
        self.fix_mean_loss = fix_mean_loss
        self.loss_cls_type = loss_cls_type
        self.semantic_ignore_index = semantic_ignore_index
        self.last_matched = []          # per level (final level first, then the auxiliary ones): per scene (query ids, object ids)

    def get_loss(self, pred_inst_info, targets, gt_masks, matched_idx_list=None):
        pred_cls_list = pred_inst_info["cls_list"]
        pred_mask_list = pred_inst_info["mask_list"]
        pred_score_list = pred_inst_info["score_list"]
        device = pred_mask_list[0].device
        zero = lambda: torch.tensor(0.0, requires_grad=True, device=device)  # noqa: E731
        if self.iter_matcher or matched_idx_list is None:
            matched_idx_list = self.matcher([c.detach() for c in pred_cls_list], [m.detach() for m in pred_mask_list], targets)
        self.last_matched.append(matched_idx_list)
        cls_loss_list, score_loss_list, mask_bce_loss_list, mask_dice_loss_list = [], [], [], []
        for i in range(len(targets.cls)):
            if len(targets.cls[i]) == 0:
                cls_loss_list.append(zero())
                score_loss_list.append(zero())
                mask_bce_loss_list.append(zero())
                mask_dice_loss_list.append(zero())
                continue
            pred_idx, gt_idx = matched_idx_list[i]
            pred_cls = pred_cls_list[i].float()
            pred_mask = pred_mask_list[i].float()
            pred_score = pred_score_list[i].float() if pred_score_list is not None else None
            num_classes = pred_cls.shape[1] - 1
            gt_cls = pred_cls.new_full((len(pred_cls),), num_classes, dtype=torch.long)
            gt_cls[pred_idx] = targets.cls[i][gt_idx]
            assert self.loss_cls_type == "ce_loss"
            cls_loss_list.append(F.cross_entropy(pred_cls, gt_cls, pred_cls.new_tensor(self.class_weight)))
            pred_mask = pred_mask[pred_idx]
            gt_mask = gt_masks[i][gt_idx]
            mask_bce_loss_list.append(F.binary_cross_entropy_with_logits(pred_mask, gt_mask.float()))
            mask_dice_loss_list.append(dice_loss(pred_mask, gt_mask.float()))
            if pred_score is None:
                continue
            with torch.no_grad():
                gt_score = get_iou(pred_mask, gt_mask).unsqueeze(1)
            filter_id, _ = torch.where(gt_score > 0.5)
            if filter_id.numel():
                score_loss_list.append(F.mse_loss(pred_score[filter_id], gt_score[filter_id]))
        n_scene = len(pred_mask_list)
        cls_loss = torch.mean(torch.stack(cls_loss_list))
        score_loss = torch.stack(score_loss_list).sum() / n_scene if len(score_loss_list) else zero()
        if len(mask_bce_loss_list):
            mask_bce_loss = torch.stack(mask_bce_loss_list).sum() / n_scene
            mask_dice_loss = torch.stack(mask_dice_loss_list).sum()
            if self.fix_dice_loss_weight:
                mask_dice_loss = mask_dice_loss / n_scene * 4
            if self.fix_mean_loss:
                mask_bce_loss = mask_bce_loss * n_scene / len(mask_bce_loss_list)
                mask_dice_loss = mask_dice_loss * n_scene / len(mask_dice_loss_list)
        else:
            mask_bce_loss, mask_dice_loss = zero(), zero()
        loss = (self.loss_weight[0] * cls_loss + self.loss_weight[1] * mask_bce_loss + self.loss_weight[2] * mask_dice_loss
                + self.loss_weight[3] * score_loss)
        return loss, dict(loss_cls=cls_loss, loss_mask=mask_bce_loss, loss_dice=mask_dice_loss, loss_score=score_loss), matched_idx_list

    @staticmethod
    def loss_bias(pred_bias, gt_bias, gt_mask):
        bias_dist = torch.sum(torch.abs(pred_bias - gt_bias), dim=-1)
        return torch.sum(bias_dist * gt_mask) / (torch.sum(gt_mask) + 1e-8)

    def forward(self, pred, target):
        targets = target["inst_info"]
        gt_point_info = target["point_info"]
        gt_masks = targets.masks.to_bool()
        self.last_matched = []
        pred_inst_info = dict(cls_list=pred["cls_list"], mask_list=pred["mask_list"], score_list=pred["score_list"])
        loss, loss_dict, matched_idx_list = self.get_loss(pred_inst_info, targets, gt_masks)
        if "aux_pred_list" in pred:
            for pred_inst_info_ in pred["aux_pred_list"]:
                aux_loss, _, _ = self.get_loss(pred_inst_info_, targets, gt_masks, None if self.iter_matcher else matched_idx_list)
                loss = loss + aux_loss
        if "seg_logits" in pred:
            if pred["seg_logits"] is not None:
                if gt_point_info["segment"].max() >= 0:
                    seg_logits = pred["seg_logits"].float()
                    loss_seg = F.cross_entropy(seg_logits, gt_point_info["segment"], seg_logits.new_tensor(self.class_weight),
                                               ignore_index=self.semantic_ignore_index)
                else:
                    loss_seg = torch.tensor(0.0, requires_grad=True, device=loss.device)
                loss = loss + self.loss_weight[4] * loss_seg
            else:
                loss_seg = torch.tensor(0.0, requires_grad=True, device=loss.device)
            loss_dict["loss_seg"] = loss_seg
        if "bias" in pred:
            if pred["bias"] is not None:
                loss_bias = self.loss_bias(pred["bias"].float(), gt_point_info["bias"], gt_point_info["mask"])
                loss = loss + self.loss_weight[5] * loss_bias
            else:
                loss_bias = torch.tensor(0.0, device=loss.device)
            loss_dict["loss_bias"] = loss_bias
        loss_dict["loss"] = loss
        return loss_dict


# ---- nms.py ----
def mask_matrix_nms(masks, labels, scores, kernel="linear"):
    """Matrix NMS (SOLOv2) with the linear kernel over at most topk_insts masks, as the model calls nms.py:5-129: scores sorted, each
    decayed by min_i (1 - iou_ij) / (1 - max_k iou_ki) over the better-scored masks i of its class -> (scores, labels, masks, keep)."""
    if kernel != "linear":
        raise NotImplementedError("mask_matrix_nms: only the linear kernel (the model's) is ported")
    if len(labels) == 0:
        return scores.new_zeros(0), labels.new_zeros(0), masks.new_zeros(0, *masks.shape[-1:]), labels.new_zeros(0)
    area = masks.sum(1).float()
    scores, keep = torch.sort(scores, descending=True)
    masks, area, labels = masks[keep], area[keep], labels[keep]
    n = len(labels)
    flat = masks.reshape(n, -1).float()
    inter = torch.mm(flat, flat.transpose(1, 0))
    area_m = area.expand(n, n)
    iou = (inter / (area_m + area_m.transpose(1, 0) - inter)).triu(diagonal=1)
    same = (labels.expand(n, n) == labels.expand(n, n).transpose(1, 0)).triu(diagonal=1)
    decay_iou = iou * same
    compensate, _ = decay_iou.max(0)
    compensate = compensate.expand(n, n).transpose(1, 0)
    coefficient, _ = ((1 - decay_iou) / (1 - compensate)).min(0)
    scores, order = torch.sort(scores * coefficient, descending=True)
    return scores, labels[order], masks[order], keep[order]


class SGIFormer(nn.Module):
    """SGIFormer-v1m1 (:482-686)"""

    def __init__(self, backbone, decoder=None, criteria=None, topk_insts=200, score_thr=0.0, npoint_thr=100, sp_score_thr=0.55, nms=True,
                 semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1):
        super().__init__()
        self.backbone = build_backbone(backbone)
        self.decoder = decoder if isinstance(decoder, nn.Module) else SGIFormerDecoder(**decoder)
        self.criteria = criteria if isinstance(criteria, nn.Module) else SGIFormerLoss(**criteria)
        self.topk_insts = topk_insts
        self.score_thr = score_thr
        self.npoint_thr = npoint_thr
        self.sp_score_thr = sp_score_thr
        self.nms = nms
        self.semantic_num_classes = semantic_num_classes
        self.semantic_ignore_index = semantic_ignore_index
        self.segment_ignore_index = segment_ignore_index
        self.instance_ignore_index = instance_ignore_index

    @torch.no_grad()
    def prepare_target(self, point):
        """:516-585; inst_info is a functional.SGITargets of the whole batch"""
        if self.instance_ignore_index != -1:
            raise NotImplementedError("SGIFormer on the engine: instance_ignore_index must be -1")
        segment = point.segment.clone()
        segment_ignore_index = torch.tensor(self.segment_ignore_index, device=point.segment.device)
        segment[torch.isin(point.segment, segment_ignore_index)] = self.semantic_ignore_index
        for cls in sorted(self.segment_ignore_index, reverse=True):
            if cls == self.semantic_ignore_index:
                continue
            segment[segment >= cls] -= 1
        point_info = dict(segment=segment, coord=point.coord, bias=point.instance_centroid - point.coord,
                          mask=point.instance != self.instance_ignore_index)
        inst_info = PF.sgi_targets(point.instance, segment, point.sp_inverse, point.offset)
        return dict(point_info=point_info, inst_info=inst_info)

    def pool_superpoints(self, point):
        """:599-612: batched superpoints by unique(batch << 48 | superpoint), features by the engine's segment mean"""
        _, cluster = torch.unique(point.batch.long() << 48 | point.superpoint.long(), return_inverse=True)
        perm = torch.sort(cluster, stable=True).indices
        counts = torch.bincount(cluster)
        indptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
        point["sp_perm"], point["sp_indptr"] = perm, indptr
        point["sp_feat"] = PF.segment_csr(point.feat, indptr, "mean", perm, True)
        point["sp_batch"] = point.batch[perm[indptr[:-1]]]
        n_scene = point.offset.numel()
        sp_count = torch.bincount(point.sp_batch, minlength=n_scene)
        point["sp_offset"] = torch.cumsum(sp_count, 0)
        point["sp_inverse"] = cluster
        ends, sp = torch.stack([point.offset.to(sp_count.dtype), sp_count]).tolist()        # the forward's host read of the sizes
        point["bincount_host"] = [b - a for a, b in zip([0] + ends[:-1], ends)]
        point["sp_bincount_host"] = sp
        return point

    def forward(self, data_dict, return_point=False):
        if return_point:
            return dict(point=self.backbone(data_dict))
        point = self.backbone(data_dict)
        assert isinstance(point, Point)
        while "pooling_parent" in point.keys():
            assert "pooling_inverse" in point.keys()
            parent = point.pop("pooling_parent")
            inverse = point.pop("pooling_inverse")
            parent.feat = torch.cat([parent.feat, point.feat[inverse]], dim=-1)
            point = parent
        point = self.pool_superpoints(point)
        pred = self.decoder(point)
        if "segment" in data_dict.keys() and "instance" in data_dict.keys():
            return_dict = self.criteria(pred, self.prepare_target(point))
        else:
            return_dict = dict()
        if not self.training:
            return_dict.update(self.predict(pred, point))
        return return_dict

    @torch.no_grad()
    def predict(self, pred, point):
        """:620-684"""
        assert len(pred["cls_list"]) == 1          # assume bs=1 for inference
        pred_cls = pred["cls_list"][0].float()
        pred_mask = pred["mask_list"][0].float()
        pred_score = F.softmax(pred_cls, dim=-1)[:, :-1]
        if pred["score_list"] is not None:
            pred_score = pred_score * pred["score_list"][0].float()
        pred_classes = torch.arange(self.semantic_num_classes, device=pred_score.device).unsqueeze(0).repeat(len(pred_cls), 1).flatten(0, 1)
        pred_score, topk_idx = pred_score.flatten(0, 1).topk(self.topk_insts, sorted=False)
        pred_classes = pred_classes[topk_idx]
        topk_idx = torch.div(topk_idx, self.semantic_num_classes, rounding_mode="floor")
        pred_mask = pred_mask[topk_idx]
        pred_mask_sigmoid = pred_mask.sigmoid()
        mask_scores = (pred_mask_sigmoid * (pred_mask > 0)).sum(1) / ((pred_mask > 0).sum(1) + 1e-6)
        pred_score = pred_score * mask_scores
        if self.nms:
            pred_score, pred_classes, pred_mask_sigmoid, _ = mask_matrix_nms(pred_mask_sigmoid, pred_classes, pred_score, kernel="linear")
        pred_mask = pred_mask_sigmoid[:, point.sp_inverse] > self.sp_score_thr
        score_mask = pred_score > self.score_thr
        pred_score, pred_classes, pred_mask = pred_score[score_mask], pred_classes[score_mask], pred_mask[score_mask]
        npoint_mask = pred_mask.sum(1) > self.npoint_thr
        pred_score, pred_classes, pred_mask = pred_score[npoint_mask], pred_classes[npoint_mask], pred_mask[npoint_mask]
        sort_score, sort_index = pred_score.sort(descending=True)
        return dict(pred_scores=sort_score.cpu().numpy(), pred_masks=pred_mask[sort_index].cpu().numpy(),
                    pred_classes=pred_classes[sort_index].cpu().numpy())
