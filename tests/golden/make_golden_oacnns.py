"""Generate tests/golden/oacnns_tiny.npz by running the REFERENCE'S OWN OA-CNNs file (pointcept/models/oacnns/oacnns_v1m1_base.py,
imported unmodified through oracle/ref_import.py on the CPU stand-ins of oracle/shims.py: spconv, torch_geometric's voxel_grid and
scatter) in fp32.  Only runnable where the reference tree exists; the .npz output is committed.

    python tests/golden/make_golden_oacnns.py

oacnns_tiny.npz: CFG below (3 stages, grid sizes with non-powers of two: 3, 6, 9, 5; L = 4 / 3 / 3 levels), two synthetic scenes
(2600 + 1100 voxels), deterministic weights (oracle.ptv3_model.deterministic_state_dict, seed 61: a function of the key names, so a
consumer regenerates it from its own state dict; the fixture keeps the key list and a float64 sum per tensor to check that).  The
batch is regenerated from the scene seeds (pointcept_amd.synthetic) and checked against stored checksums.  Stored: the eval-mode logits
(every 4th row), then one train-mode step (cross entropy, ignore_index -1): its logits (every 8th row), loss, every BatchNorm's running
statistics after the step, the gradient norm of every parameter and the full gradient (grad/<name>) of every parameter of at most
FULL_GRAD_MAX elements (all BatchNorm affines, the adaptive / weight / l_w / proj Linears of the 16-channel blocks) and of final.*.
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

CFG = dict(in_channels=6, num_classes=13, embed_channels=16, enc_num_ref=[16, 16, 16], enc_channels=[16, 16, 24], groups=[4, 4, 4],
           enc_depth=[1, 2, 1], down_ratio=[2, 2, 2], dec_channels=[16, 16, 24],
           point_grid_size=[[3, 6, 9, 16], [2, 6, 9], [2, 3, 5]], dec_depth=[1, 1, 1])
SCENES = [(41, 2600), (42, 1100)]
SD_SEED = 61
FULL_GRAD_MAX = 512


def load_reference_oacnns():
    ref_import.load()
    name = "pointcept.models.oacnns.oacnns_v1m1_base"
    if name not in sys.modules:
        pk = types.ModuleType("pointcept.models.oacnns")
        pk.__path__ = [ref_import.REF + "/pointcept/models/oacnns"]
        sys.modules["pointcept.models.oacnns"] = pk
    return importlib.import_module(name)


def batch():
    return synthetic.collate([synthetic.indoor_scene(s, n) for s, n in SCENES])


def main():
    R = load_reference_oacnns()
    torch.manual_seed(0)
    ref = R.OACNNs(**CFG)
    sd = om.deterministic_state_dict(ref, SD_SEED)
    ref.load_state_dict(sd)
    b = batch()
    inp = {k: torch.from_numpy(v) for k, v in b.items()}
    ref.eval()
    with torch.no_grad():
        logits_eval = ref(dict(inp)).numpy()
    ref.train()
    logits = ref(dict(inp))
    loss = torch.nn.functional.cross_entropy(logits, inp["segment"].long() % CFG["num_classes"], ignore_index=-1)
    loss.backward()
    names = [k for k, _ in ref.named_parameters()]
    out = dict(scene_seeds=np.asarray([s for s, _ in SCENES]), n_points=np.asarray([n for _, n in SCENES]),
               input_checksum=np.asarray([float(b["grid_coord"].sum()), float(b["feat"].astype(np.float64).sum()),
                                          float(b["segment"].sum())]),
               sd_seed=np.asarray(SD_SEED), keys=np.asarray(list(sd.keys())),
               sd_checksum=np.asarray([float(v.double().sum()) for v in sd.values()]), param_names=np.asarray(names),
               logits_eval=logits_eval[::4].astype(np.float32), logits_train=logits.detach().numpy()[::8].astype(np.float32),
               logits_absmax=np.asarray(float(np.abs(logits_eval).max())), loss=np.asarray(float(loss.detach())),
               grad_norms=np.asarray([float(p.grad.double().norm()) for _, p in ref.named_parameters()]))
    for k, v in ref.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["after/" + k] = v.numpy()
    for k, p in ref.named_parameters():
        if p.numel() <= FULL_GRAD_MAX or k.startswith("final."):
            out["grad/" + k] = p.grad.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "oacnns_tiny.npz"), **out)
    print("oacnns_tiny.npz:", len(sd), "state entries, loss", float(loss.detach()))


if __name__ == "__main__":
    main()
