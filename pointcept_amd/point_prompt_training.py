"""Point Prompt Training on the engine: drop-ins for pointcept/models/point_prompt_training/
point_prompt_training_v1m1_language_guided.py ("PPT-v1m1"), point_prompt_training_v1m2_decoupled.py ("PPT-v1m2") and
point_prompt_training_v1m3_neo.py ("PPT-v1m3"), with the reference's constructor arguments and defaults, state-dict keys
(backbone.*, embedding_table.weight, proj_head.*, logit_scale, the persistent class_embedding of v1m1, the non-persistent
class_embeddings of v1m3, seg_heads.{i}.* of v1m2), its three forward modes (train: loss; eval with labels: loss + seg_logits; test:
seg_logits), backbone_mode, freeze_backbone and v1m3's pooling_parent / pooling_inverse up-cast loop.  Registered only when named:
compat.register_models(MODELS, names=["PPT-v1m1", "SpUNet-v1m3"]).

* The language-guided head -- proj_head, the row normalisation, the product with the selected class rows and exp(logit_scale) -- is
  functional.ppt_head: one kernel per direction (csrc/ppt.hip), the [N, 512] projection never stored.  v1m1 selects the class rows by
  valid_index and divides by the plain norm (eps = 0); v1m3 selects by split(num_classes) and uses F.normalize's eps (1e-12, 1e-6 for
  fp16).  The logits are fp32, also under autocast.  PTC_PPT=0 (config.PPT_KERNELS), CPU tensors and shapes the kernel refuses take
  functional.ppt_head_torch, the reference's expression.
* CLIP is not needed at run time: the two language-guided classes take `class_embedding=` (a [K_all, D] tensor, or a path to a .pt /
  .npy file holding one; unit rows as the reference stores them) and `logit_scale=` (the LOG scale, CLIP's ln 100 by default).  Only
  when class_embedding is absent do they `import clip` and do what the reference does; without that package they raise an error that
  names the argument.  logit_scale is a frozen Parameter as in the reference (clip_model.requires_grad_(False)); its value reaches the
  kernel as a host float, read once per parameter version.
* v1m2's heads are the engine's Linear; the backbone comes from compat.build_backbone (SpUNet-v1m3, PT-v3m1 with PDNorm, ...); the
  criteria are criteria.Criteria (CrossEntropyLoss / LovaszLoss on the engine's loss kernels) or an already built callable.
* backbone_mode=True returns the backbone's features: PPT as the multi-dataset backbone of another model (PG-v1m1 in
  configs/s3dis/insseg-ppt-v1m1-0-pointgroup-spunet-ft.py).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

from . import functional as PF
from . import nn as PNN
from .compat import build_backbone
from .criteria import Criteria
from .structure import Point

_BACKBONES = ("SpUNet-v1m3", "PT-v2m3", "PT-v3m1")
_NO_CLIP = ("{name}: no class_embedding= was given and the `clip` package is not installed -- pass class_embedding= (a [classes, D] "
            "tensor of unit rows, or a path to a .pt / .npy file holding one) and logit_scale= (the log scale, ln 100 for CLIP)")


def _backbone_type(backbone):
    if isinstance(backbone, nn.Module) or backbone is None:
        return None
    return backbone["type"] if isinstance(backbone, dict) else backbone.type


def _load_embedding(src) -> torch.Tensor:
    if isinstance(src, (str, os.PathLike)):
        path = os.fspath(src)
        if path.endswith(".npy"):
            import numpy as np

            src = torch.from_numpy(np.load(path))
        else:
            src = torch.load(path, map_location="cpu")
    if isinstance(src, (list, tuple)):
        src = torch.cat([torch.as_tensor(s) for s in src], 0)
    src = torch.as_tensor(src).detach().float()
    if src.dim() != 2:
        raise ValueError(f"class_embedding: expected [classes, D], got {tuple(src.shape)}")
    return src.clone()


def _clip_text(name, clip_model, prompts):
    """what the reference does (v1m1 :61-77): -> (unit text embeddings of `prompts`, projection width, logit_scale)"""
    try:
        import clip
    except ImportError as e:
        raise ImportError(_NO_CLIP.format(name=name)) from e
    model, _ = clip.load(clip_model, device="cpu", download_root="./.cache/clip")
    model.requires_grad_(False)
    emb = model.encode_text(clip.tokenize(prompts))
    emb = emb / emb.norm(dim=-1, keepdim=True)
    return emb.detach().float(), int(model.text_projection.shape[1]), model.logit_scale


class _LanguageHead(nn.Module):
    """proj_head + logit_scale + the class rows of the two language-guided classes"""

    def _init_head(self, backbone_out_channels, width, logit_scale):
        self.proj_head = PNN.Linear(backbone_out_channels, width)
        ls = logit_scale.detach().clone().float() if isinstance(logit_scale, torch.Tensor) else torch.tensor(float(logit_scale))
        self.logit_scale = nn.Parameter(ls.reshape(()), requires_grad=False)
        self._scale_cache = None

    def _log_scale(self):
        """the frozen log scale as a host float (one device read per parameter version); the Parameter itself if it requires grad"""
        p = self.logit_scale
        if p.requires_grad:
            return p
        key = (p._version, p.data_ptr())
        if self._scale_cache is None or self._scale_cache[0] != key:
            self._scale_cache = (key, float(p.detach()))
        return self._scale_cache[1]

    def _logits(self, feat, rows, eps):
        return PF.ppt_head(feat, self.proj_head.weight, self.proj_head.bias, rows, self._log_scale(), eps)


def _outputs(module, seg_logits, data_dict):
    """train: loss; eval with labels: loss and seg_logits; test: seg_logits (v1m1 :108-118)"""
    if module.training:
        return dict(loss=module.criteria(seg_logits, data_dict["segment"]))
    if "segment" in data_dict.keys():
        return dict(loss=module.criteria(seg_logits, data_dict["segment"]), seg_logits=seg_logits)
    return dict(seg_logits=seg_logits)


def _context(module, data_dict):
    condition = data_dict["condition"][0] if isinstance(data_dict["condition"], (list, tuple)) else data_dict["condition"]
    assert condition in module.conditions
    index = module.conditions.index(condition)
    data_dict["context"] = module.embedding_table(torch.tensor([index], device=data_dict["coord"].device))
    return condition, index


class PointPromptTraining(_LanguageHead):
    """PPT-v1m1 (point_prompt_training_v1m1_language_guided.py:18-118)"""

    def __init__(self, backbone=None, criteria=None, backbone_out_channels=96, context_channels=256,
                 conditions=("Structured3D", "ScanNet", "S3DIS"), template="[x]", clip_model="ViT-B/16",
                 class_name=("wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "bookcase", "picture",
                             "counter", "desk", "shelves", "curtain", "dresser", "pillow", "mirror", "ceiling", "refrigerator", "television",
                             "shower curtain", "nightstand", "toilet", "sink", "lamp", "bathtub", "garbagebin", "board", "beam", "column",
                             "clutter", "otherstructure", "otherfurniture", "otherprop"),
                 valid_index=((0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 23, 25, 26, 33, 34, 35),
                              (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 20, 22, 24, 25, 27, 34),
                              (0, 1, 4, 5, 6, 7, 8, 10, 19, 29, 30, 31, 32)),
                 backbone_mode=False, class_embedding=None, logit_scale=math.log(100.0)):
        super().__init__()
        assert len(conditions) == len(valid_index)
        assert _backbone_type(backbone) in _BACKBONES + (None,)
        self.backbone = build_backbone(backbone)
        self.criteria = criteria if callable(criteria) else Criteria(criteria, "PPT-v1m1", row_terms=False)
        self.conditions = conditions
        self.valid_index = valid_index
        self.embedding_table = nn.Embedding(len(conditions), context_channels)
        self.backbone_mode = backbone_mode
        if not self.backbone_mode:
            if class_embedding is None:
                emb, width, logit_scale = _clip_text("PPT-v1m1", clip_model, [template.replace("[x]", name) for name in class_name])
            else:
                emb = _load_embedding(class_embedding)
                width = emb.shape[1]
                if emb.shape[0] != len(class_name):
                    raise ValueError(f"PPT-v1m1: class_embedding has {emb.shape[0]} rows for {len(class_name)} class names")
            self.register_buffer("class_embedding", emb)
            self._init_head(backbone_out_channels, width, logit_scale)

    def forward(self, data_dict):
        _, index = _context(self, data_dict)
        point = self.backbone(data_dict)
        feat = point.feat if isinstance(point, Point) else point
        if self.backbone_mode:
            return feat
        rows = self.class_embedding[list(self.valid_index[index]), :]
        return _outputs(self, self._logits(feat, rows, 0.0), data_dict)          # :99 divides by the plain norm


class PointPromptTrainingDecoupled(nn.Module):
    """PPT-v1m2 (point_prompt_training_v1m2_decoupled.py:18-79): one segmentation head per dataset"""

    def __init__(self, backbone=None, criteria=None, backbone_out_channels=96, context_channels=256,
                 conditions=("Structured3D", "ScanNet", "S3DIS"), num_classes=(25, 20, 13), backbone_mode=False):
        super().__init__()
        assert len(conditions) == len(num_classes)
        assert _backbone_type(backbone) in _BACKBONES + (None,)
        self.backbone = build_backbone(backbone)
        self.criteria = criteria if callable(criteria) else Criteria(criteria, "PPT-v1m2", row_terms=False)
        self.conditions = conditions
        self.embedding_table = nn.Embedding(len(conditions), context_channels)
        self.backbone_mode = backbone_mode
        self.seg_heads = nn.ModuleList([PNN.Linear(backbone_out_channels, num_cls) for num_cls in num_classes])

    def forward(self, data_dict):
        _, index = _context(self, data_dict)
        point = self.backbone(data_dict)
        feat = point.feat if isinstance(point, Point) else point
        if self.backbone_mode:
            return feat
        return _outputs(self, self.seg_heads[index](feat), data_dict)


_NEO_CLASS_NAMES = (
    ("wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "picture", "desk", "shelves", "curtain", "dresser",
     "pillow", "mirror", "ceiling", "refrigerator", "television", "nightstand", "sink", "lamp", "otherstructure", "otherfurniture",
     "otherprop"),
    ("wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain",
     "refridgerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture"),
    ("ceiling", "floor", "wall", "beam", "column", "window", "door", "table", "chair", "sofa", "bookcase", "board", "clutter"),
)


class PointPromptTrainingNeo(_LanguageHead):
    """PPT-v1m3 (point_prompt_training_v1m3_neo.py:23-140): no prompt, class names per dataset, a Point-returning backbone"""

    def __init__(self, backbone=None, criteria=None, backbone_out_channels=96, conditions=("Structured3D", "ScanNet", "S3DIS"),
                 template="[x]", clip_model="ViT-B/16", class_names=None, freeze_backbone=False, backbone_mode=False, class_embedding=None,
                 logit_scale=math.log(100.0)):
        super().__init__()
        if class_names is None:
            class_names = [list(names) for names in _NEO_CLASS_NAMES]
        assert len(conditions) == len(class_names)
        self.backbone = build_backbone(backbone)
        self.criteria = criteria if callable(criteria) else Criteria(criteria, "PPT-v1m3", row_terms=False)
        self.conditions = conditions
        self.freeze_backbone = freeze_backbone
        if self.freeze_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False
        self.backbone_mode = backbone_mode
        if not self.backbone_mode:
            num_classes = [len(names) for names in class_names]
            if class_embedding is None:
                prompts = [template.replace("[x]", name) for names in class_names for name in names]
                emb, width, logit_scale = _clip_text("PPT-v1m3", clip_model, prompts)          # row-wise: the reference's per-dataset calls, concatenated
            else:
                emb = _load_embedding(class_embedding)
                width = emb.shape[1]
                if emb.shape[0] != sum(num_classes):
                    raise ValueError(f"PPT-v1m3: class_embedding has {emb.shape[0]} rows for {sum(num_classes)} class names")
            self.register_buffer("class_embeddings", emb, persistent=False)
            self.num_classes = num_classes
            self._init_head(backbone_out_channels, width, logit_scale)

    def forward(self, data_dict):
        condition = data_dict["condition"][0] if isinstance(data_dict["condition"], (list, tuple)) else data_dict["condition"]
        if self.freeze_backbone:
            with torch.no_grad():
                point = self.backbone(data_dict)
        else:
            point = self.backbone(data_dict)
        while "pooling_parent" in point.keys():
            assert "pooling_inverse" in point.keys()
            parent = point.pop("pooling_parent")
            inverse = point.pop("pooling_inverse")
            parent.feat = torch.cat([parent.feat, point.feat[inverse]], dim=-1)
            point = parent
        if self.backbone_mode:
            return point.feat
        feat = point.feat
        dt = torch.get_autocast_dtype("cuda") if (feat.is_cuda and torch.is_autocast_enabled("cuda")) else feat.dtype
        eps = 1e-6 if dt == torch.float16 else 1e-12          # :119, on the dtype proj_head's output has in the reference
        rows = self.class_embeddings.split(self.num_classes)[self.conditions.index(condition)]
        return _outputs(self, self._logits(feat, rows, eps), data_dict)
