"""Generate tests/golden/ppt_tiny.npz by running the REFERENCE'S OWN Point Prompt Training files (pointcept/models/
point_prompt_training/point_prompt_training_v1m1_language_guided.py and point_prompt_training_v1m2_decoupled.py, their backbone the
reference's spconv_unet_v1m3_pdnorm.py and their criteria the reference's CrossEntropyLoss + LovaszLoss from its own registries; all
imported unmodified through oracle/ref_import.py on the CPU stand-ins of oracle/shims.py) in fp32.  CLIP is not installed here: a
stand-in `clip` module is registered whose load / tokenize / encode_text return seeded unit rows of width CLIP_WIDTH and
logit_scale = ln 100 -- the reference files use nothing else of it.  Only runnable where the reference tree exists; the .npz output is
committed.

    python tests/golden/make_golden_ppt.py

ppt_tiny.npz: two scenes from pointcept_amd.synthetic.indoor_scene, collated (regenerated from their seeds and checked against stored
checksums); a tiny SpUNet-v1m3 (BACKBONE below: norm_adaptive and norm_affine on, zero_init off) with deterministic weights
(oracle.ptv3_model.deterministic_state_dict, seed SD_SEED; class_embedding and logit_scale keep the stand-in's values), so every
modulation Linear is nonzero and the prompt-driven norm is not a no-op.  For PPT-v1m1 and PPT-v1m2, each under the conditions ScanNet
(20 classes) and S3DIS (13 classes; the labels are taken modulo 13): the train loss, every parameter's gradient norm, the full
gradients of proj_head / seg_heads, embedding_table and one modulation Linear, the BatchNorm buffers of that norm site for the used
condition and for an unused one, and the eval-mode loss and seg_logits (every 8th row; with labels and without are equal, asserted).
PPT-v1m3 needs a Point-returning backbone (PT-v3 with pooling parents), which the tiny sparse U-Net is not: it gets head-only goldens --
the reference file's own expression (:117-129: Linear, F.normalize with eps 1e-12, the split class rows, exp(logit_scale)) evaluated in
float64 on seeded features, with its gradients.
"""
import importlib
import math
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

BACKBONE = dict(type="SpUNet-v1m3", in_channels=6, num_classes=0, base_channels=16, context_channels=256,
                channels=(16, 32, 48, 64, 64, 48, 32, 32), layers=(1, 2, 1, 1, 1, 1, 2, 1), norm_adaptive=True, norm_affine=True,
                zero_init=False)
CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
CFG = dict(backbone=BACKBONE, criteria=CRITERIA, backbone_out_channels=32, context_channels=256)
SCENES = [(83, 1400), (84, 1000)]
SD_SEED = 93
CLIP_WIDTH = 64
CLIP_SEED = 17
CONDITIONS = {"ScanNet": 20, "S3DIS": 13}          # condition -> its number of classes (v1m1's valid_index, v1m2's num_classes)
UNUSED = "Structured3D"
NORM_SITE = "backbone.enc.0.block0.bn2"           # the norm whose modulation gradient and buffers are stored
HEADS = ("proj_head.", "seg_heads.", "embedding_table.", NORM_SITE + ".modulation.1.")
V1M3_CLASSES = (25, 20, 13)
EVAL_STRIDE = 8                                    # the eval logits are stored for every 8th row


class AttrDict(dict):
    """a config dict with attribute access (the reference asserts on `backbone.type`)"""
    __getattr__ = dict.__getitem__


def clip_standin():
    """a module with the three calls the reference makes: load -> (model, None), tokenize, model.encode_text"""
    clip = types.ModuleType("clip")

    class _Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.text_projection = torch.nn.Parameter(torch.zeros(CLIP_WIDTH, CLIP_WIDTH))
            self.logit_scale = torch.nn.Parameter(torch.tensor(math.log(100.0)))

        def encode_text(self, tokens):
            rows = [torch.randn(CLIP_WIDTH, generator=torch.Generator().manual_seed(CLIP_SEED + int(t))) for t in tokens]
            return torch.stack(rows) * 3.0          # not unit length: the caller normalises

    clip.load = lambda name, device="cpu", download_root=None: (_Model(), None)
    clip.tokenize = lambda prompts: torch.tensor([sum(ord(ch) * (i + 1) for i, ch in enumerate(p)) % 100003 for p in prompts])
    return clip


def class_embedding(prompts):
    """the unit rows the stand-in gives for `prompts` (what a caller passes to the engine's class_embedding=)"""
    c = clip_standin()
    e = c.load("ViT-B/16")[0].encode_text(c.tokenize(list(prompts)))
    return e / e.norm(dim=-1, keepdim=True)


def load_reference_ppt():
    ref_import.load()
    losses = sys.modules.get("pointcept.models.losses")
    if losses is not None and not hasattr(losses, "build_criteria"):      # a bare stub package left by another loader: complete it
        losses.build_criteria = importlib.import_module("pointcept.models.losses.builder").build_criteria
        for name in ("misc", "lovasz"):
            importlib.import_module("pointcept.models.losses." + name)
    sys.modules["clip"] = clip_standin()
    importlib.import_module("pointcept.models.sparse_unet.spconv_unet_v1m3_pdnorm")
    pre = "pointcept.models.point_prompt_training."
    return {"v1m1": importlib.import_module(pre + "point_prompt_training_v1m1_language_guided").PointPromptTraining,
            "v1m2": importlib.import_module(pre + "point_prompt_training_v1m2_decoupled").PointPromptTraining}


def batch():
    return synthetic.collate([synthetic.indoor_scene(s, n) for s, n in SCENES])


def checksum(b):
    return np.asarray([float(np.asarray(b[k]).astype(np.float64).sum()) for k in sorted(b)])


def inputs_for(inp, condition):
    d = dict(inp)
    k = CONDITIONS[condition]
    d["segment"] = torch.where(inp["segment"] >= 0, inp["segment"] % k, inp["segment"])
    d["condition"] = [condition]
    return d


def build(cls):
    return cls(**dict(CFG, backbone=AttrDict(BACKBONE)))


def state_dict_for(model):
    sd = om.deterministic_state_dict(model, SD_SEED)
    own = model.state_dict()
    for k in ("class_embedding", "logit_scale"):          # CLIP's: frozen, kept as the stand-in gives them
        if k in own:
            sd[k] = own[k].detach().clone()
    return sd


def run_train(cls, sd, inp):
    ref = build(cls)
    ref.load_state_dict(sd)
    ref.train()
    out = ref(dict(inp))
    out["loss"].backward()
    return ref, out


def run_eval(cls, sd, inp):
    ref = build(cls)
    ref.load_state_dict(sd)
    ref.eval()
    with torch.no_grad():
        with_labels = ref(dict(inp))
        without = ref({k: v for k, v in inp.items() if k != "segment"})
    return with_labels, without


def v1m3_head(feat, weight, bias, class_embeddings, num_classes, index, logit_scale):
    """point_prompt_training_v1m3_neo.py:117-129 on given features"""
    h = torch.nn.functional.linear(feat, weight, bias)
    h = torch.nn.functional.normalize(h, dim=-1, p=2, eps=1e-12)
    sim = h @ class_embeddings.split(list(num_classes))[index].t()
    return logit_scale.exp() * sim


def v1m3_inputs():
    g = torch.Generator().manual_seed(CLIP_SEED + 1)
    feat = torch.randn(200, 32, generator=g)
    weight = torch.randn(CLIP_WIDTH, 32, generator=g) / math.sqrt(32)
    bias = 0.1 * torch.randn(CLIP_WIDTH, generator=g)
    emb = torch.nn.functional.normalize(torch.randn(sum(V1M3_CLASSES), CLIP_WIDTH, generator=g), dim=1)
    cot = torch.randn(200, V1M3_CLASSES[1], generator=g)
    return feat, weight, bias, emb, cot


def main():
    R = load_reference_ppt()
    b = batch()
    inp = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    res = dict(scene_seeds=np.asarray([s for s, _ in SCENES]), n_points=np.asarray([n for _, n in SCENES]), input_keys=np.asarray(sorted(b)),
               input_checksum=checksum(b), sd_seed=np.asarray(SD_SEED), eval_stride=np.asarray(EVAL_STRIDE))
    for tag, cls in R.items():
        sd = state_dict_for(build(cls))
        res[f"{tag}/keys"] = np.asarray(list(sd.keys()))
        res[f"{tag}/sd_checksum"] = np.asarray([float(v.double().sum()) for v in sd.values()])
        if tag == "v1m1":
            res["class_embedding"] = sd["class_embedding"].numpy().astype(np.float32)
            res["logit_scale"] = np.asarray(float(sd["logit_scale"]))
        for cond in CONDITIONS:
            d = inputs_for(inp, cond)
            ref, out = run_train(cls, sd, d)
            assert set(out) == {"loss"}
            key = f"{tag}/{cond}"
            res[f"{key}/loss"] = np.asarray(float(out["loss"].detach()))
            named = [(k, p) for k, p in ref.named_parameters()]
            res[f"{tag}/param_names"] = np.asarray([k for k, _ in named])
            res[f"{key}/has_grad"] = np.asarray([p.grad is not None for _, p in named])
            res[f"{key}/grad_norms"] = np.asarray([float(p.grad.double().norm()) if p.grad is not None else 0.0 for _, p in named])
            for k, p in named:
                if k.startswith(HEADS) and p.grad is not None:
                    res[f"{key}/grad/{k}"] = p.grad.numpy().astype(np.float32)
            state = ref.state_dict()
            conds = list(ref.backbone.conditions)
            for which, name in (("used", cond), ("unused", UNUSED)):
                pre = f"{NORM_SITE}.bns.{conds.index(name)}."
                for buf in ("running_mean", "running_var", "num_batches_tracked"):
                    res[f"{key}/bn_{which}/{buf}"] = state[pre + buf].numpy()
                    if which == "unused":
                        assert torch.equal(state[pre + buf], sd[pre + buf])
            with_labels, without = run_eval(cls, sd, d)
            assert set(with_labels) == {"loss", "seg_logits"} and set(without) == {"seg_logits"}
            assert torch.equal(with_labels["seg_logits"], without["seg_logits"])
            res[f"{key}/eval/loss"] = np.asarray(float(with_labels["loss"]))
            res[f"{key}/eval/seg_logits"] = with_labels["seg_logits"][::EVAL_STRIDE].numpy().astype(np.float32)
            print(key, "train loss", float(out["loss"].detach()), "eval loss", float(with_labels["loss"]),
                  "modulation grad norm", float(dict(named)[NORM_SITE + ".modulation.1.weight"].grad.norm()))
            assert float(dict(named)[NORM_SITE + ".modulation.1.weight"].grad.norm()) > 0
    # PPT-v1m3: head-only, float64
    feat, weight, bias, emb, cot = (t.double() for t in v1m3_inputs())
    feat.requires_grad_(True), weight.requires_grad_(True), bias.requires_grad_(True)
    logits = v1m3_head(feat, weight, bias, emb, V1M3_CLASSES, 1, torch.tensor(math.log(100.0), dtype=torch.float64))
    (logits * cot).sum().backward()
    res["v1m3/logits"] = logits.detach().numpy().astype(np.float32)
    res["v1m3/dfeat"] = feat.grad.numpy().astype(np.float32)
    res["v1m3/dweight"] = weight.grad.numpy().astype(np.float32)
    res["v1m3/dbias"] = bias.grad.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "ppt_tiny.npz"), **res)
    print("ppt_tiny.npz:", os.path.getsize(os.path.join(OUT, "ppt_tiny.npz")), "bytes")


if __name__ == "__main__":
    main()
