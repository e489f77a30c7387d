"""build_criteria(criteria) (pointcept/models/losses/builder.py:22-31) on the engine's loss kernels, shared by the module-level ports
that take a `criteria=` config list (context_aware_classifier.py, point_prompt_training.py)."""
from __future__ import annotations

from . import functional as PF


class Criteria:
    """the name-mapped criteria list: CrossEntropyLoss -> functional.cross_entropy, LovaszLoss -> functional.lovasz_softmax, each with
    loss_weight / ignore_index; any other type, or a setting the kernels do not implement, is refused by name (`owner` names the
    model in the message)"""

    SUPPORTED = {
        "CrossEntropyLoss": ("cross_entropy", dict(weight=None, size_average=None, reduce=None, reduction="mean", label_smoothing=0.0)),
        "LovaszLoss": ("lovasz_softmax", dict(mode="multiclass", class_seen=None, per_image=False)),
    }

    def __init__(self, cfg, owner: str = "criteria"):
        self.terms = []
        for c in cfg or []:
            c = dict(c)
            kind = c.pop("type")
            w = float(c.pop("loss_weight", 1.0))
            ignore = int(c.pop("ignore_index", -1))
            if kind not in self.SUPPORTED:
                raise ValueError(f"{owner} criteria: {kind} is not on the engine's loss kernels")
            fn, defaults = self.SUPPORTED[kind]
            other = {k: v for k, v in c.items() if k not in defaults or defaults[k] != v}
            if other:       # any other setting would silently train a different loss
                raise ValueError(f"{owner} criteria: {kind} with {other} is not on the engine's loss kernels")
            self.terms.append((getattr(PF, fn), w, ignore))

    def __call__(self, pred, target):
        loss = 0
        for fn, w, ignore in self.terms:
            loss = loss + fn(pred, target, ignore) * w
        return loss
