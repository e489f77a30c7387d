"""Generate tests/golden/msc_tiny.npz by running the REFERENCE'S OWN Masked Scene Contrast file (pointcept/models/
masked_scene_contrast/masked_scene_contrast_v1m1_base.py, imported unmodified through oracle/ref_import.py on the CPU stand-ins of
oracle/shims.py: spconv, torch_geometric's voxel_grid, timm; its backbone the reference's SpUNet-v1m1 from its own registry) in fp32.
Stand-ins that live here: `pointops.knn_query` = oracle/pointops.py; a no-op Tensor.cuda for the file's `.cuda()` call on a CPU run;
recording wrappers around torch.randperm / torch.randint / random.random.  Only runnable where the reference tree exists; the .npz
output is committed.

    python tests/golden/make_golden_msc.py

msc_tiny.npz: CFG below (matching_max_pair deliberately small, view 1 mixed), two scenes per view from
pointcept_amd.synthetic.contrastive_views (regenerated from their seeds and checked against stored checksums), deterministic weights
(oracle.ptv3_model.deterministic_state_dict, seed SD_SEED; key list and a float64 sum per tensor).  Stored: the recorded draws in
call order (patch_perm, mix [2], select_r, pair_perm), both point masks, match_index, every entry of the result dict, the gradient
norm of every parameter, the full gradients of mask_token and the two heads, and the histogram of match counts.  The generator
asserts that some view-1 points have 0, 1 and k matches, that P exceeds matching_max_pair, and that floor(x / g) equals
floor(x * (1 / g)) in fp32 for every origin coordinate (the two forms ATen uses for a division by a scalar on the host and on a GPU),
so that the masks are the same on either.
"""
import importlib
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle import pointops as opo  # noqa: E402
from oracle import ptv3_model as om  # noqa: E402
from oracle import ref_import  # noqa: E402
from pointcept_amd import synthetic  # noqa: E402

BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, base_channels=16, channels=(16, 32, 48, 64, 64, 48, 32, 32),
                layers=(1, 2, 1, 1, 1, 1, 2, 1))
CFG = dict(backbone=BACKBONE, backbone_in_channels=6, backbone_out_channels=32, mask_grid_size=0.1, mask_rate=0.4, view1_mix_prob=0.8,
           view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=256, nce_t=0.4, contrast_weight=1,
           reconstruct_weight=1, reconstruct_color=True, reconstruct_normal=True)
SCENES = [(81, 1400), (82, 1000)]
SD_SEED = 91
DRAW_SEED = 1
HEADS = ("mask_token", "color_head.", "normal_head.")


def knn_query(nsample, xyz, offset, new_xyz, new_offset):
    i, d = opo.knn_query(int(nsample), xyz.numpy(), offset.numpy(), new_xyz.numpy(), new_offset.numpy())
    return torch.from_numpy(i), torch.from_numpy(d)


def load_reference_msc(pointops=None):
    ref_import.load()
    ref_import.load_dataset_utils()          # gives pointcept.models.utils its offset2batch
    sys.modules["pointops"] = pointops or types.SimpleNamespace(knn_query=knn_query)
    name = "pointcept.models.masked_scene_contrast.masked_scene_contrast_v1m1_base"
    if name not in sys.modules:
        pk = types.ModuleType("pointcept.models.masked_scene_contrast")
        pk.__path__ = [ref_import.REF + "/pointcept/models/masked_scene_contrast"]
        sys.modules["pointcept.models.masked_scene_contrast"] = pk
    return importlib.import_module(name)


def batch():
    return synthetic.contrastive_views_batch([s for s, _ in SCENES], [n for _, n in SCENES])


def checksum(b):
    return np.asarray([float(b[k].astype(np.float64).sum()) for k in sorted(b)])


class recorded_draws:
    """torch.randperm / torch.randint / random.random record what they return while the reference's forward runs"""

    def __init__(self):
        self.log = []

    def __enter__(self):
        self.saved = (torch.randperm, torch.randint, random.random, torch.Tensor.cuda)
        rp, ri, rr = self.saved[:3]

        def wrap(kind, fn):
            def f(*a, **k):
                v = fn(*a, **k)
                self.log.append((kind, v.clone() if torch.is_tensor(v) else v))
                return v
            return f

        torch.randperm, torch.randint, random.random = wrap("randperm", rp), wrap("randint", ri), wrap("random", rr)
        torch.Tensor.cuda = lambda t, *a, **k: t
        return self

    def __exit__(self, *exc):
        torch.randperm, torch.randint, random.random, torch.Tensor.cuda = self.saved


def run_reference(R, sd, inp, capture):
    """one train-mode forward + backward of the reference model; capture(masks, match_index) sees the integers"""
    ref = R.MaskedSceneContrast(**CFG)
    ref.load_state_dict(sd(ref))
    ref.train()
    gm, mp = ref.generate_cross_masks, ref.match_contrastive_pair
    got = {}
    ref.generate_cross_masks = lambda *a, **k: got.setdefault("masks", gm(*a, **k))
    ref.match_contrastive_pair = lambda *a, **k: got.setdefault("match", mp(*a, **k))
    torch.manual_seed(DRAW_SEED)
    random.seed(DRAW_SEED)
    with recorded_draws() as rec:
        out = ref(dict(inp))
    out["loss"].backward()
    capture(got["masks"], got["match"], rec.log)
    return ref, out


def main():
    R = load_reference_msc()
    b = batch()
    inp = {k: torch.from_numpy(v) for k, v in b.items()}
    for v in ("view1", "view2"):
        x = b[f"{v}_origin_coord"]
        g = np.float32(CFG["mask_grid_size"])
        assert np.array_equal(np.floor(x / g), np.floor(x * (np.float32(1.0) / g))), "a coordinate sits on a patch boundary"
    kept = {}
    holder = {}
    ref0 = R.MaskedSceneContrast(**CFG)
    sd = om.deterministic_state_dict(ref0, SD_SEED)
    ref, out = run_reference(R, lambda m: sd, inp, lambda masks, match, log: kept.update(masks=masks, match=match, log=log))
    kinds = [k for k, _ in kept["log"]]
    assert kinds == ["randperm", "random", "random", "randint", "randperm"], kinds
    # match-count histogram of all view-1 points
    idx, dist = knn_query(8, inp["view2_origin_coord"], inp["view2_offset"].int(), inp["view1_origin_coord"], inp["view1_offset"].int())
    cnt = (dist < CFG["matching_max_radius"]).sum(1)
    hist = torch.bincount(cnt, minlength=9).numpy()
    assert hist[0] > 0 and hist[1] > 0 and hist[8] > 0, hist
    assert int((cnt > 0).sum()) > CFG["matching_max_pair"] and kept["match"].shape[0] == CFG["matching_max_pair"]
    assert kept["log"][1][1] < CFG["view1_mix_prob"], "view 1 is not mixed with this seed"
    res = dict(scene_seeds=np.asarray([s for s, _ in SCENES]), n_points=np.asarray([n for _, n in SCENES]), input_keys=np.asarray(sorted(b)),
               input_checksum=checksum(b), sd_seed=np.asarray(SD_SEED), keys=np.asarray(list(sd.keys())),
               sd_checksum=np.asarray([float(v.double().sum()) for v in sd.values()]),
               draw_patch_perm=kept["log"][0][1].numpy(), draw_mix=np.asarray([kept["log"][1][1], kept["log"][2][1]]),
               draw_select_r=kept["log"][3][1].numpy(), draw_pair_perm=kept["log"][4][1].numpy(),
               view1_point_mask=kept["masks"][0].numpy(), view2_point_mask=kept["masks"][1].numpy(), match_index=kept["match"].numpy(),
               match_count_hist=hist, param_names=np.asarray([k for k, _ in ref.named_parameters()]),
               grad_norms=np.asarray([float(p.grad.double().norm()) for _, p in ref.named_parameters()]))
    for k, v in out.items():
        res["out/" + k] = np.asarray(float(v.detach()))
    for k, p in ref.named_parameters():
        if k.startswith(HEADS):
            res["grad/" + k] = p.grad.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "msc_tiny.npz"), **res)
    print("msc_tiny.npz:", len(sd), "state entries;", {k: float(v.detach()) for k, v in out.items()}, "count histogram", hist.tolist(),
          "masked", int(kept["masks"][0].sum()), int(kept["masks"][1].sum()), "mix draws", res["draw_mix"].tolist())


if __name__ == "__main__":
    main()
