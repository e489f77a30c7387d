"""Generate tests/golden/sgiformer_tiny.npz by running the REFERENCE'S OWN SGIFormer files (pointcept/models/sgiformer/
sgiformer_v1m1_base.py, loss.py, nms.py, imported unmodified through oracle/ref_import.py on the CPU stand-ins of oracle/shims.py; the
backbone the reference's PT-v3m1 from its own registry) in fp32 on the CPU.  Only runnable where the reference tree exists; the .npz
output is committed.

    python tests/golden/make_golden_sgiformer.py

torch_scatter.scatter, which the SGIFormer file calls and the shims do not carry, is the stand-in `scatter` below: sum / mean / max
over dim 0, integer sources (an integer mean is floor-divided, as the library does), rows whose index is negative skipped (the
library's CUDA kernel leaves them undefined; sgiformer_v1m1_base.py:566 scatters with instance == -1).

sgiformer_tiny.npz: CFG below -- a three-stage PT-v3m1 (2 orders, patch 64, channels 16/32/64, decoder 32/32), decoder d_model 64 with
2 heads (head dim 32), 24 + 24 queries, 3 layers, gelu, attn_mask -- on three scenes of pointcept_amd.synthetic.indoor_superpoint_batch
(regenerated from their seeds and checked against stored checksums), deterministic weights (oracle.ptv3_model.deterministic_state_dict)
with decoder.x_mask.0.weight multiplied by MASK_SCALE and decoder.out_norm.bias lowered by NORM_SHIFT: the superpoint mask features are
ReLU outputs, so with the unshifted normalised queries no row is fully masked after the first layer, and no mask logit may sit at the
attention-mask threshold; and with decoder.bias_head.3.bias moved by BIAS_NUDGE (at most 0.01): the offset loss is an L1 norm, and with
the unmoved bias one residual of a labelled point is 3.5e-7 -- the sign of such a residual, and with it the gradient of the whole
bias head, is decided by rounding.  For use_score False and True.  The generator asserts:
  * every scene but one has >= 5 instances and >= 40 superpoints, one has no instance, and some points of the others carry instance -1;
  * the floored integer mean of the reference's target masks equals the rule 2 count > superpoint size on these scenes;
  * at every level no mask logit lies within 1e-3 of 0, at least one query row hits the all-masked rule and at least one does not;
  * no component of the offset residual (prediction - target) of a labelled point lies within 5e-4 of 0, the kink of the L1 loss;
  * the sampler's top-k set is separated from the next value by more than 1e-6;
  * every Hungarian assignment survives a +-1e-4 relative perturbation of its cost matrix.
Stored: seeds, sizes, cell, checksums, the key list; the seven train losses; the matched indices per level and scene; every parameter's
gradient norm and, for use_score False, the decoder's full gradients; the eval scores, classes and masks of the first scene alone.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle import ptv3_model as om  # noqa: E402
from oracle import ref_import  # noqa: E402
from pointcept_amd import synthetic  # noqa: E402

BACKBONE = dict(type="PT-v3m1", in_channels=6, order=("z", "z-trans"), stride=(2, 2), enc_depths=(1, 1, 1), enc_channels=(16, 32, 64),
                enc_num_head=(1, 2, 4), enc_patch_size=(64, 64, 64), dec_depths=(1, 1), dec_channels=(32, 32), dec_num_head=(2, 2),
                dec_patch_size=(64, 64), drop_path=0.0, shuffle_orders=False, enable_flash=False, enable_rpe=True,
                upcast_attention=True, upcast_softmax=True)
NUM_CLASSES = 18
DECODER = dict(num_classes=NUM_CLASSES, in_channel=32, dec_num_layer=3, num_sample_query=24, num_learn_query=24, d_model=64, nhead=2,
               hidden_dim=128, dropout=0.0, activation_fn="gelu", attn_mask=True, use_score=False, alpha=0.4)
CRITERIA = dict(matcher=dict(type="HungarianMatcher", costs=[dict(type="QueryClassificationCost", weight=0.5), dict(type="MaskBCECost", weight=1.0),
                                                             dict(type="MaskDiceCost", weight=1.0)]),
                loss_weight=[0.8, 1.0, 1.0, 0.5, 0.4, 0.4], num_classes=NUM_CLASSES, non_object_weight=0.1, fix_dice_loss_weight=False,
                iter_matcher=True, fix_mean_loss=True)
MODEL = dict(topk_insts=60, score_thr=0.0, npoint_thr=20, nms=True, semantic_num_classes=NUM_CLASSES, semantic_ignore_index=-1,
             segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1)
SCENES = [(236, 3000), (201, 1200), (378, 3000)]
CELL = 0.2
SD_SEED = 95
MASK_SCALE = 8.0
NORM_SHIFT = 0.2
BIAS_NUDGE = (-0.00205, 0.009675, -0.0051)
FWD_SEED = 11          # torch.manual_seed before every forward: PT-v3m1's SerializedPooling shuffles its orders with the CPU generator
TRAIN_LOSSES = ("loss_cls", "loss_mask", "loss_dice", "loss_score", "loss_seg", "loss_bias", "loss")
DATA_KEYS = ("coord", "grid_coord", "feat", "segment", "instance", "instance_centroid", "superpoint", "offset")


def scatter(src, index, dim=0, out=None, dim_size=None, reduce="sum"):
    """torch_scatter.scatter over dim 0 for the calls of sgiformer_v1m1_base.py: rows with a negative index are skipped"""
    assert dim == 0 and out is None and index.dim() == 1
    keep = index >= 0
    src, index = src[keep], index[keep].long()
    n = int(dim_size) if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
    shape = (n,) + tuple(src.shape[1:])
    idx = index.view((-1,) + (1,) * (src.dim() - 1)).expand_as(src)
    if reduce in ("sum", "add", "mean"):
        res = torch.zeros(shape, dtype=src.dtype).scatter_add_(0, idx, src)
        if reduce == "mean":
            count = torch.bincount(index, minlength=n).clamp_(min=1).view((-1,) + (1,) * (src.dim() - 1))
            res = res / count if res.is_floating_point() else torch.div(res, count, rounding_mode="floor")
        return res
    if reduce == "max":
        low = torch.finfo(src.dtype).min if src.is_floating_point() else torch.iinfo(src.dtype).min
        res = torch.full(shape, low, dtype=src.dtype).scatter_reduce_(0, idx, src, "amax", include_self=True)
        return torch.where(res == low, torch.zeros_like(res), res)          # untouched rows are 0, as in the library
    raise NotImplementedError(reduce)


def load_reference_sgiformer():
    ref_import.load()
    sys.modules["torch_scatter"].scatter = scatter
    name = "pointcept.models.sgiformer.sgiformer_v1m1_base"
    if name not in sys.modules:
        pk = types.ModuleType("pointcept.models.sgiformer")
        pk.__path__ = [ref_import.REF + "/pointcept/models/sgiformer"]
        sys.modules["pointcept.models.sgiformer"] = pk
    return importlib.import_module(name)


def config(use_score):
    return dict(MODEL, backbone=dict(BACKBONE), decoder=dict(DECODER, use_score=use_score), criteria=dict(CRITERIA))


def batch(scenes=SCENES):
    return synthetic.indoor_superpoint_batch([s for s, _ in scenes], [n for _, n in scenes], CELL)


def checksum(b):
    return np.asarray([float(np.asarray(b[k]).astype(np.float64).sum()) for k in sorted(b)])


def state_dict_for(model):
    sd = om.deterministic_state_dict(model, SD_SEED)
    sd["decoder.x_mask.0.weight"] = sd["decoder.x_mask.0.weight"] * MASK_SCALE
    sd["decoder.out_norm.bias"] = sd["decoder.out_norm.bias"] - NORM_SHIFT
    sd["decoder.bias_head.3.bias"] = sd["decoder.bias_head.3.bias"] + torch.tensor(BIAS_NUDGE)
    return sd


def to_inputs(b):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}


class Recorder:
    """wraps the reference's matcher and forward_head: cost matrices and assignments per call, mask logits per level"""

    def __init__(self, model):
        self.costs, self.matched, self.levels = [], [], []
        matcher = model.criteria.matcher
        call = matcher.__class__.__call__

        def matched(pred_inst, gt_inst, **kw):
            from scipy.optimize import linear_sum_assignment

            q, o = call(matcher, pred_inst, gt_inst, **kw)
            with torch.no_grad():
                cost = torch.stack([c(pred_inst, gt_inst) for c in matcher.costs]).sum(dim=0).numpy().astype(np.float64)
            for sign in (1.0, -1.0):            # +-1e-4 relative, entry by entry in a checkerboard, and uniformly
                for pert in (cost * (1 + sign * 1e-4 * (((np.indices(cost.shape).sum(0)) % 2) * 2 - 1)), cost * (1 + sign * 1e-4)):
                    q2, o2 = linear_sum_assignment(pert)
                    assert np.array_equal(q2, q.numpy()) and np.array_equal(o2, o.numpy()), "assignment is not stable"
            self.matched.append((q.numpy().copy(), o.numpy().copy()))
            return q, o

        model.criteria.matcher = matched
        head = model.decoder.forward_head

        def forward_head(query_list, sp_mask_feat_list):
            res = head(query_list, sp_mask_feat_list)
            self.levels.append(([m.detach().clone() for m in res[2]], [a.clone() for a in res[3]]))
            return res

        model.decoder.forward_head = forward_head


def check_sampler_margin(model, inp):
    """the top-k set of the sampler (:404-409) against the next value, per scene"""
    torch.manual_seed(FWD_SEED)
    with torch.no_grad():
        point = model.backbone(dict(inp))
        score = model.decoder.seg_head(point.feat).softmax(dim=-1)[:, :-1].max(dim=-1)[0]
    ends = inp["offset"].tolist()
    gaps = []
    for a, b in zip([0] + ends[:-1], ends):
        s = score[a:b].sort(descending=True)[0]
        k = int(model.decoder.alpha * (b - a))
        gaps.append(float(s[k - 1] - s[k]))
    return gaps


def run_train(R, sd, inp, use_score):
    ref = R.SGIFormer(**config(use_score))
    ref.load_state_dict(sd)
    ref.train()
    gaps = check_sampler_margin(ref, inp)
    ref.train()
    rec = Recorder(ref)
    loss_bias = ref.criteria.loss_bias

    def recorded_loss_bias(pred_bias, gt_bias, gt_mask):
        rec.bias_residual = float((pred_bias - gt_bias).detach()[gt_mask.bool()].abs().min())
        return loss_bias(pred_bias, gt_bias, gt_mask)

    ref.criteria.loss_bias = recorded_loss_bias
    torch.manual_seed(FWD_SEED)
    out = ref(dict(inp))
    out["loss"].backward()
    return ref, out, rec, gaps


def run_eval(R, sd, inp, use_score):
    ref = R.SGIFormer(**config(use_score))
    ref.load_state_dict(sd)
    ref.eval()
    torch.manual_seed(FWD_SEED)
    with torch.no_grad():
        return ref(dict(inp))


def main():
    R = load_reference_sgiformer()
    b = batch()
    assert sorted(b) == sorted(DATA_KEYS), sorted(b)
    inp = to_inputs(b)
    ends = b["offset"].tolist()
    bounds = list(zip([0] + ends[:-1], ends))
    n_inst = [len(np.unique(b["instance"][a:e][b["instance"][a:e] >= 0])) for a, e in bounds]
    n_sp = [len(np.unique(b["superpoint"][a:e])) for a, e in bounds]
    assert sorted(n_inst)[0] == 0 and all(g >= 5 for g in sorted(n_inst)[1:]), n_inst
    assert all(m >= 40 for g, m in zip(n_inst, n_sp) if g), n_sp
    assert all((b["instance"][a:e] == -1).any() for (a, e), g in zip(bounds, n_inst) if g)
    one = batch(SCENES[:1])
    res = dict(scene_seeds=np.asarray([s for s, _ in SCENES]), n_points=np.asarray([n for _, n in SCENES]), cell=np.asarray(CELL),
               input_keys=np.asarray(sorted(b)), input_checksum=checksum(b), eval_checksum=checksum(one), sd_seed=np.asarray(SD_SEED),
               mask_scale=np.asarray(MASK_SCALE), norm_shift=np.asarray(NORM_SHIFT), bias_nudge=np.asarray(BIAS_NUDGE), fwd_seed=np.asarray(FWD_SEED), n_inst=np.asarray(n_inst), n_sp=np.asarray(n_sp))
    for use_score in (False, True):
        tag = f"score{int(use_score)}"
        sd = state_dict_for(R.SGIFormer(**config(use_score)))
        res[f"{tag}/keys"] = np.asarray(list(sd.keys()))
        res[f"{tag}/sd_checksum"] = np.asarray([float(v.double().sum()) for v in sd.values()])
        ref, out, rec, gaps = run_train(R, sd, inp, use_score)
        assert min(gaps) > 1e-6, gaps
        assert rec.bias_residual > 5e-4, rec.bias_residual
        print(tag, "smallest offset residual", rec.bias_residual)
        assert set(out) == set(TRAIN_LOSSES), sorted(out)
        n_level = DECODER["dec_num_layer"] + 1
        assert len(rec.levels) == n_level and len(rec.matched) == n_level * sum(1 for g in n_inst if g)
        for lv, (logits, masks) in enumerate(rec.levels):
            near = min(float(x.abs().min()) for x in logits)
            assert near > 1e-3, (lv, near)
            cleared = sum(int(((x.sigmoid() < 0.5).sum(-1) == x.shape[-1]).sum()) for x in logits)
            rows = sum(x.shape[0] for x in logits)
            assert 0 < cleared < rows, (lv, cleared, rows)
            print(tag, "level", lv, "nearest logit", near, "rows cleared", cleared, "of", rows)
        # the reference's integer-mean masks against 2 count > size
        target = ref.prepare_target(types.SimpleNamespace(**{k: v for k, v in inp.items()}, sp_inverse=torch.unique(
            (torch.repeat_interleave(torch.arange(len(ends)), torch.tensor([e - a for a, e in bounds])) << 48) | inp["superpoint"],
            return_inverse=True)[1]))
        from pointcept_amd import functional as PF

        mine = PF.sgi_targets_torch(inp["instance"], target["point_info"]["segment"], torch.unique(
            (torch.repeat_interleave(torch.arange(len(ends)), torch.tensor([e - a for a, e in bounds])) << 48) | inp["superpoint"],
            return_inverse=True)[1], inp["offset"])
        for i, info in enumerate(target["inst_info"]):
            assert torch.equal(info["mask"].bool(), mine.masks.to_bool()[i]) or info["mask"].shape[0] == 0, i
            assert torch.equal(info["cls"].long(), mine.cls[i]), i
        # matched indices: the reference calls the matcher for the final level first, then for the auxiliary levels in order
        for j, (q, o) in enumerate(rec.matched):
            res[f"{tag}/matched/{j}/query"] = q
            res[f"{tag}/matched/{j}/object"] = o
        for k in TRAIN_LOSSES:
            res[f"{tag}/out/{k}"] = np.asarray(float(out[k].detach()))
        res[f"{tag}/param_names"] = np.asarray([k for k, _ in ref.named_parameters()])
        res[f"{tag}/grad_norms"] = np.asarray([float(p.grad.double().norm()) if p.grad is not None else -1.0 for _, p in ref.named_parameters()])
        for k, p in ref.named_parameters():
            if k.startswith("decoder.") and p.grad is not None and not use_score:      # (the file-size limit: one setting's full gradients)
                res[f"{tag}/grad/{k}"] = p.grad.numpy().astype(np.float32)
        ev = run_eval(R, sd, to_inputs(one), use_score)
        assert set(ev) == set(TRAIN_LOSSES) | {"pred_scores", "pred_masks", "pred_classes"}
        assert len(ev["pred_scores"]) >= 3, len(ev["pred_scores"])
        res[f"{tag}/eval/pred_scores"] = ev["pred_scores"].astype(np.float32)
        res[f"{tag}/eval/pred_classes"] = ev["pred_classes"].astype(np.int64)
        res[f"{tag}/eval/pred_masks"] = np.packbits(ev["pred_masks"], axis=1)
        res[f"{tag}/eval/loss"] = np.asarray(float(ev["loss"]))
        print(tag, {k: float(out[k].detach()) for k in TRAIN_LOSSES}, "sampler gaps", gaps, "eval instances", len(ev["pred_scores"]))
    np.savez_compressed(os.path.join(OUT, "sgiformer_tiny.npz"), **res)
    print("sgiformer_tiny.npz:", os.path.getsize(os.path.join(OUT, "sgiformer_tiny.npz")), "bytes; instances", n_inst, "superpoints", n_sp)


if __name__ == "__main__":
    main()
