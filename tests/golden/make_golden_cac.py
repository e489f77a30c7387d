"""Generate tests/golden/cac_tiny.npz by running the REFERENCE'S OWN context-aware classifier file (pointcept/models/
context_aware_classifier/context_aware_classifier_v1m1_base.py, imported unmodified through oracle/ref_import.py on the CPU stand-ins
of oracle/shims.py; its backbone the reference's SpUNet-v1m1 and its criteria the reference's CrossEntropyLoss + LovaszLoss, from its
own registries) in fp32.  A no-op Tensor.cuda is installed while the reference runs, for the file's `.cuda()` calls on a CPU run.
Only runnable where the reference tree exists; the .npz output is committed.

    python tests/golden/make_golden_cac.py

cac_tiny.npz: CFG below -- 24 classes over labels 0..19 and -1, so four classes never occur (the absent-class branch of the adaptive
perspective), cos_temp 15, conf_thresh 0.75 -- two scenes from pointcept_amd.synthetic.indoor_scene, collated (regenerated from their
seeds and checked against stored checksums), deterministic weights (oracle.ptv3_model.deterministic_state_dict, seed SD_SEED) with
seg_head.weight multiplied by HEAD_SCALE: with the unscaled weights every row's largest probability is below 0.09, the gate would
drop every row and the refinement would be tested on zeros.  The generator asserts that in the train-mode forward between 10 % and
90 % of the rows of every scene pass the gate and no row's largest probability lies within 5e-4 of the threshold (in the eval-mode
forward, whose features differ by the BatchNorm mode: some rows pass, none within 1e-4).
Stored: seeds, sizes, checksums; the key list and a float64 sum per tensor; per-scene pass counts (train, eval) and per-class label counts; for
detach_pre_logits True and False the five train losses, every parameter's gradient norm, the full gradients of seg_head, proj,
apd_proj and feat_proj_layer, and the three BatchNorm buffers after the train forward; the eval-mode loss and seg_logits with labels
and seg_logits without.
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

BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, base_channels=16, channels=(16, 32, 48, 64, 64, 48, 32, 32),
                layers=(1, 2, 1, 1, 1, 1, 2, 1))
CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
CFG = dict(num_classes=24, backbone_out_channels=32, backbone=BACKBONE, criteria=CRITERIA, cos_temp=15, conf_thresh=0.75)
SCENES = [(81, 1400), (82, 1000)]
SD_SEED = 91
HEAD_SCALE = 16.125
HEADS = ("seg_head.", "proj.", "apd_proj.", "feat_proj_layer.")
BN_BUFFERS = ("feat_proj_layer.1.running_mean", "feat_proj_layer.1.running_var", "feat_proj_layer.1.num_batches_tracked")
TRAIN_LOSSES = ("loss", "seg_loss", "pre_loss", "pre_self_loss", "kl_loss")


def load_reference_cac():
    ref_import.load()
    name = "pointcept.models.context_aware_classifier.context_aware_classifier_v1m1_base"
    if name not in sys.modules:
        pk = types.ModuleType("pointcept.models.context_aware_classifier")
        pk.__path__ = [ref_import.REF + "/pointcept/models/context_aware_classifier"]
        sys.modules["pointcept.models.context_aware_classifier"] = pk
    return importlib.import_module(name)


def batch():
    return synthetic.collate([synthetic.indoor_scene(s, n) for s, n in SCENES])


def checksum(b):
    return np.asarray([float(np.asarray(b[k]).astype(np.float64).sum()) for k in sorted(b)])


class host_cuda:
    """Tensor.cuda returns the tensor itself while the reference's file runs on the CPU"""

    def __enter__(self):
        self.saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda t, *a, **k: t
        return self

    def __exit__(self, *exc):
        torch.Tensor.cuda = self.saved


def state_dict_for(model):
    sd = om.deterministic_state_dict(model, SD_SEED)
    sd["seg_head.weight"] = sd["seg_head.weight"] * HEAD_SCALE
    return sd


def run_train(R, sd, inp, detach):
    """one train-mode forward + backward of the reference model"""
    ref = R.CACSegmentor(**dict(CFG, detach_pre_logits=detach))
    ref.load_state_dict(sd)
    ref.train()
    with host_cuda():
        out = ref(dict(inp))
        out["loss"].backward()
    return ref, out


def run_eval(R, sd, inp):
    ref = R.CACSegmentor(**CFG)
    ref.load_state_dict(sd)
    ref.eval()
    with host_cuda(), torch.no_grad():
        with_labels = ref(dict(inp))
        without = ref({k: v for k, v in inp.items() if k != "segment"})
    return ref, with_labels, without


def gate_figures(R, sd, inp, train):
    """per scene: rows whose largest probability passes conf_thresh; the smallest distance of a largest probability to the threshold
    (the backbone's BatchNorm in train or eval mode: the features, and with them the gate, differ)"""
    ref = R.CACSegmentor(**CFG)
    ref.load_state_dict(sd)
    ref.train(train)
    with torch.no_grad():
        feat = ref.backbone(dict(inp))
        p = torch.softmax(ref.seg_head(feat), 1).max(1)[0]
    ends = inp["offset"].tolist()
    passed = [int((p[a:b] >= CFG["conf_thresh"]).sum()) for a, b in zip([0] + ends[:-1], ends)]
    return passed, float((p - CFG["conf_thresh"]).abs().min())


def main():
    R = load_reference_cac()
    b = batch()
    inp = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    sd = state_dict_for(R.CACSegmentor(**CFG))
    res = dict(scene_seeds=np.asarray([s for s, _ in SCENES]), n_points=np.asarray([n for _, n in SCENES]), input_keys=np.asarray(sorted(b)),
               input_checksum=checksum(b), sd_seed=np.asarray(SD_SEED), head_scale=np.asarray(HEAD_SCALE), keys=np.asarray(list(sd.keys())),
               sd_checksum=np.asarray([float(v.double().sum()) for v in sd.values()]))
    ref_e, with_labels, without = run_eval(R, sd, inp)
    passed, nearest = gate_figures(R, sd, inp, True)
    sizes = [n for _, n in SCENES]
    assert all(0.1 * n <= p <= 0.9 * n for p, n in zip(passed, sizes)), (passed, sizes)
    assert nearest > 5e-4, nearest
    passed_eval, nearest_eval = gate_figures(R, sd, inp, False)
    assert nearest_eval > 1e-4 and all(0 < p < n for p, n in zip(passed_eval, sizes)), (passed_eval, nearest_eval)
    res["pass_count_eval"] = np.asarray(passed_eval)
    seg = inp["segment"]
    res["pass_count"] = np.asarray(passed)
    res["class_count"] = torch.bincount(seg[seg >= 0], minlength=CFG["num_classes"]).numpy()
    assert int((res["class_count"] == 0).sum()) >= 4 and bool((seg == -1).any())
    res["eval/loss"] = np.asarray(float(with_labels["loss"]))
    res["eval/seg_logits"] = with_labels["seg_logits"].numpy().astype(np.float32)
    res["eval/seg_logits_nolabel"] = without["seg_logits"].numpy().astype(np.float32)
    for detach in (True, False):
        tag = f"detach{int(detach)}"
        ref, out = run_train(R, sd, inp, detach)
        assert set(out) == set(TRAIN_LOSSES)
        for k in TRAIN_LOSSES:
            res[f"{tag}/out/{k}"] = np.asarray(float(out[k].detach()))
        res["param_names"] = np.asarray([k for k, _ in ref.named_parameters()])
        res[f"{tag}/grad_norms"] = np.asarray([float(p.grad.double().norm()) for _, p in ref.named_parameters()])
        for k, p in ref.named_parameters():
            if k.startswith(HEADS):
                res[f"{tag}/grad/{k}"] = p.grad.numpy().astype(np.float32)
        state = ref.state_dict()
        for k in BN_BUFFERS:
            res[f"{tag}/bn/{k}"] = state[k].numpy()
        print(tag, {k: float(out[k].detach()) for k in TRAIN_LOSSES}, "num_batches_tracked", int(state[BN_BUFFERS[2]]))
    np.savez_compressed(os.path.join(OUT, "cac_tiny.npz"), **res)
    print("cac_tiny.npz:", len(sd), "state entries; rows past the gate", passed, "of", sizes, "nearest to the threshold", nearest, "eval", passed_eval, nearest_eval,
          "eval loss", float(with_labels["loss"]))


if __name__ == "__main__":
    main()
