"""build_criteria(criteria) (pointcept/models/losses/builder.py:22-31) on the engine's loss kernels, shared by the module-level ports
that take a `criteria=` config list (context_aware_classifier.py, point_prompt_training.py) and by segmentor.DefaultSegmentorV2.

Mapped, each with loss_weight / ignore_index:
  CrossEntropyLoss(weight, label_smoothing, reduction = mean | sum)   all defaults: functional.cross_entropy (csrc/loss.hip), as before;
                                                                       anything else: a term of functional.seg_criteria
  FocalLoss(gamma, alpha float | list, reduction = mean)              a term of functional.seg_criteria (csrc/criteria.hip)
  DiceLoss(smooth, exponent)                                          a term of functional.seg_criteria
  LovaszLoss(mode = multiclass)                                       functional.lovasz_softmax (csrc/lovasz.hip), its own kernels
The row-local terms of a list that share an ignore_index go into ONE seg_criteria call: one pass over the logits per direction for all of
them (a default CrossEntropyLoss joins the call when it has company; alone it keeps today's kernels).  See functional.seg_criteria for
the shapes the kernels serve, the torch twins behind them and PTC_CRITERIA=0.
Refused by name: SmoothCELoss and FocalLoss(reduction="sum") (both raise AttributeError in the reference: nothing to be faithful to),
BinaryFocalLoss ([N] predictions, not seg logits), reduction="none", any other type or setting."""
from __future__ import annotations

import torch

from . import functional as PF


class Criteria:
    """the name-mapped criteria list (see the module docstring); any other type, or a setting the kernels do not implement, is refused
    by name (`owner` names the model in the message).  row_terms=False keeps the list to default CrossEntropyLoss and LovaszLoss: the
    contract of the ports whose losses were validated with those two alone (CAC-v1m1, PPT)."""

    SUPPORTED = {
        "CrossEntropyLoss": ("cross_entropy", dict(weight=None, size_average=None, reduce=None, reduction="mean", label_smoothing=0.0)),
        "LovaszLoss": ("lovasz_softmax", dict(mode="multiclass", class_seen=None, per_image=False)),
    }

    def __init__(self, cfg, owner: str = "criteria", row_terms: bool = True):
        self.terms = []          # in list order: (fn, loss_weight, ignore_index) | ("fused", [config dicts], ignore_index)
        groups = {}              # ignore_index -> the fused entry that collects its row-local terms
        for c in cfg or []:
            c = dict(c)
            kind = c.pop("type")
            w = float(c.pop("loss_weight", 1.0))
            ignore = int(c.pop("ignore_index", -1))
            if kind in self.SUPPORTED:
                fn, defaults = self.SUPPORTED[kind]
                other = {k: v for k, v in c.items() if k not in defaults or defaults[k] != v}
                if not other and kind == "LovaszLoss":
                    self.terms.append((getattr(PF, fn), w, ignore))
                    continue
                if other and (kind == "LovaszLoss" or not row_terms):      # any other setting would silently train a different loss
                    raise ValueError(f"{owner} criteria: {kind} with {other} is not on the engine's loss kernels")
                c = other        # settings spelled out at their defaults say nothing
            elif not row_terms or (kind not in PF.CRITERIA_ROW_TERMS and kind not in PF.CRITERIA_REFUSED):
                raise ValueError(f"{owner} criteria: {kind} is not on the engine's loss kernels")
            term = dict(c, type=kind, loss_weight=w)
            try:
                PF.criteria_terms([term])
            except ValueError as e:
                raise ValueError(f"{owner} {e}") from None
            if ignore not in groups:
                groups[ignore] = ("fused", [], ignore)
                self.terms.append(groups[ignore])
            groups[ignore][1].append(term)
        for i, entry in enumerate(self.terms):       # a default CrossEntropyLoss on its own: exactly the call it always took
            if entry[0] == "fused" and len(entry[1]) == 1 and entry[1][0]["type"] == "CrossEntropyLoss" and \
                    set(entry[1][0]) == {"type", "loss_weight"}:
                self.terms[i] = (PF.cross_entropy, entry[1][0]["loss_weight"], entry[2])
        self._on_device = {}

    def _fused_terms(self, i, terms, like):
        """the group's config dicts with their class vectors (weight, list alpha) as fp32 tensors on the logits' device, made once"""
        key = (i, like.device)
        if key not in self._on_device:
            out = []
            for t in terms:
                t = dict(t)
                for name in ("weight", "alpha"):
                    if isinstance(t.get(name), (list, tuple)):
                        t[name] = torch.tensor(t[name], dtype=torch.float32, device=like.device)
                out.append(t)
            self._on_device[key] = out
        return self._on_device[key]

    def __call__(self, pred, target):
        loss = 0
        for i, (fn, w, ignore) in enumerate(self.terms):
            if fn == "fused":
                loss = loss + PF.seg_criteria(pred, target, self._fused_terms(i, w, pred), ignore)
            else:
                loss = loss + fn(pred, target, ignore) * w
        return loss
