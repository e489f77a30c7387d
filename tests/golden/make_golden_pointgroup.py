"""Generate tests/golden/pointgroup_tiny.npz by running the REFERENCE'S OWN PointGroup file (pointcept/models/point_group/
point_group_v1m1_base.py, imported unmodified through oracle/ref_import.py on the CPU stand-ins of oracle/shims.py; its backbone the
reference's SpUNet-v1m1 from its own registry) in fp32.  `pointgroup_ops` is the Python restatement of the CUDA extension
(tests/pg_oracle.py).  Only runnable where the reference tree exists; the .npz output is committed.

    python tests/golden/make_golden_pointgroup.py

pointgroup_tiny.npz: CFG below, two synthetic instance scenes (pointcept_amd.synthetic.indoor_instance_scene, regenerated from their
seeds and checked against stored checksums), deterministic weights (oracle.ptv3_model.deterministic_state_dict, seed SD_SEED: a
function of the key names; the fixture keeps the reference's key list and a float64 sum per tensor).  Stored: one train-mode forward +
backward (loss, seg_loss, bias_l1_loss, bias_cosine_loss; the full gradient of every bias_head / seg_head parameter; the gradient norm
of every parameter); then the eval-mode forward: its head outputs (bias_pred, logit_pred, captured by forward hooks), pred_scores,
pred_classes and pred_masks as member lists (mask_members, concatenated; mask_offsets).  Ops-level fixtures on designed inputs:
the restatement's lists and clusters of a collapsed clump with mixed labels (ops_*).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle import ptv3_model as om  # noqa: E402
from oracle import ref_import  # noqa: E402
from pointcept_amd import synthetic  # noqa: E402
import pg_oracle  # noqa: E402

BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, base_channels=16, channels=(16, 32, 48, 64, 64, 48, 32, 32),
                layers=(1, 2, 1, 1, 1, 1, 2, 1))
CFG = dict(backbone=BACKBONE, backbone_out_channels=32, semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1),
           instance_ignore_index=-1, cluster_thresh=6.0, cluster_closed_points=300, cluster_propose_points=8, cluster_min_points=4,
           voxel_size=0.02)
SCENES = [(71, 2200), (72, 1500)]
SD_SEED = 81


def load_reference_pointgroup():
    ref_import.load()
    sys.modules["pointgroup_ops"] = pg_oracle.stand_in_module()
    name = "pointcept.models.point_group.point_group_v1m1_base"
    if name not in sys.modules:
        pk = types.ModuleType("pointcept.models.point_group")
        pk.__path__ = [ref_import.REF + "/pointcept/models/point_group"]
        sys.modules["pointcept.models.point_group"] = pk
    return importlib.import_module(name)


def batch():
    scenes = [synthetic.indoor_instance_scene(s, n) for s, n in SCENES]
    for s in scenes:
        s.pop("bbox")
    return synthetic.collate(scenes)


def checksum(b):
    return np.asarray([float(b["coord"].astype(np.float64).sum()), float(b["feat"].astype(np.float64).sum()), float(b["segment"].sum()),
                       float(b["instance"].sum()), float(b["instance_centroid"].astype(np.float64).sum())])


def ops_fixture():
    rng = np.random.default_rng(5)
    xyz = np.concatenate([rng.normal(0, 0.05, (1300, 3)), rng.normal(0, 1.5, (500, 3))]).astype(np.float32)
    lab = (rng.random(1800) < 0.2).astype(np.int32)
    b = np.zeros(1800, np.int32)
    idx, sl = pg_oracle.ballquery_batch_p(xyz, b, [0, 1800], 1.0)
    ci, co = pg_oracle.bfs_cluster(lab, idx, sl, 3)
    return dict(ops_xyz=xyz, ops_label=lab, ops_radius=np.asarray(1.0, np.float32), ops_threshold=np.asarray(3), ops_idx=idx,
                ops_start_len=sl, ops_cluster_idxs=ci, ops_cluster_offsets=co)


def main():
    R = load_reference_pointgroup()
    torch.manual_seed(0)
    ref = R.PointGroup(**CFG)
    sd = om.deterministic_state_dict(ref, SD_SEED)
    ref.load_state_dict(sd)
    b = batch()
    inp = {k: torch.from_numpy(v) for k, v in b.items()}
    ref.train()
    out = ref(dict(inp))
    out["loss"].backward()
    heads = {}
    ref.bias_head.register_forward_hook(lambda m, i, o: heads.__setitem__("bias", o.detach().clone()))
    ref.seg_head.register_forward_hook(lambda m, i, o: heads.__setitem__("logit", o.detach().clone()))
    ref.eval()
    with torch.no_grad():
        ev = ref(dict(inp))
    masks = ev["pred_masks"].numpy()
    members = [np.nonzero(m)[0] for m in masks]
    res = dict(scene_seeds=np.asarray([s for s, _ in SCENES]), n_points=np.asarray([n for _, n in SCENES]), input_checksum=checksum(b),
               sd_seed=np.asarray(SD_SEED), keys=np.asarray(list(sd.keys())), sd_checksum=np.asarray([float(v.double().sum()) for v in sd.values()]),
               param_names=np.asarray([k for k, _ in ref.named_parameters()]),
               grad_norms=np.asarray([float(p.grad.double().norm()) for _, p in ref.named_parameters()]),
               eval_bias_pred=heads["bias"].numpy(), eval_logit_pred=heads["logit"].numpy(),
               pred_scores=ev["pred_scores"].numpy().astype(np.float32), pred_classes=ev["pred_classes"].numpy().astype(np.int64),
               mask_members=np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32),
               mask_offsets=np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64), **ops_fixture())
    for k in ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss"):
        res[k] = np.asarray(float(out[k].detach()))
        res["eval_" + k] = np.asarray(float(ev[k]))
    for k, p in ref.named_parameters():
        if k.startswith(("bias_head.", "seg_head.")):
            res["grad/" + k] = p.grad.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "pointgroup_tiny.npz"), **res)
    print("pointgroup_tiny.npz:", len(sd), "state entries, loss", float(out["loss"]), "proposals", len(members),
          "sizes", [len(m) for m in members], "classes", ev["pred_classes"].tolist())


if __name__ == "__main__":
    main()
