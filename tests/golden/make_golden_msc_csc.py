"""Generate tests/golden/msc_csc_tiny.npz by running the REFERENCE'S OWN MSC-v1m2 file (pointcept/models/masked_scene_contrast/
masked_scene_contrast_v1m2_csc.py, imported unmodified through oracle/ref_import.py on the CPU stand-ins that make_golden_msc.py
uses for the v1m1 file: oracle/shims.py, `pointops.knn_query` = oracle/pointops.py, a no-op Tensor.cuda, the recording wrappers
around the random draws) in fp32, with the tiny SpUNet of msc_tiny.npz.  Only runnable where the reference tree exists; the .npz
output is committed.

    python tests/golden/make_golden_msc_csc.py

msc_csc_tiny.npz: CFG below -- mask_rate 0.4 and both heads on (every result key), two scenes, matching_max_pair small enough that
the randperm cut happens, so that the scenes interleave in match_index; r1 / r2 chosen for the extent of these crops so that all
five partition classes are present.  Stored: what msc_tiny.npz stores (seeds and checksums of the inputs and weights, the recorded
draws, both masks, match_index, every result entry, gradient norms, the head gradients, the match-count histogram) plus the
settings r1, r2, partitions, matching_max_pair, view1_mix_prob and class_hist [scene, 5]: the members of each class (4 = the rest)
in each scene's P_b x P_b partition matrix.  The generator asserts that (a) some scene holds all five classes, (b) no pair distance
lies within 1e-4 relative of r1 or r2, (c) rel.z == 0 occurs off the diagonal.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_msc as G  # noqa: E402

from oracle import ptv3_model as om  # noqa: E402
from oracle import ref_import  # noqa: E402

CFG = dict(G.CFG, view1_mix_prob=0, matching_max_pair=192, partitions=4, r1=0.11, r2=0.21)
SD_SEED = 92
DRAW_SEED = 2
NAME = "pointcept.models.masked_scene_contrast.masked_scene_contrast_v1m2_csc"


def load_reference_msc_csc():
    G.load_reference_msc()                   # the package stand-in, pointops and the shims, as for the v1m1 file
    return importlib.import_module(NAME)


def class_hist(x1, x2, batch, n_scenes, r1, r2):
    """[scene, 5] from the reference's rule written on numpy (fp32): element (i, j) of a scene from rel = x1[j] - x2[i]"""
    hist = np.zeros((n_scenes, 5), np.int64)
    z0 = False
    for b in np.unique(batch):
        a, c = x1[batch == b], x2[batch == b]
        rel = a[None, :, :] - c[:, None, :]
        d = np.sqrt((rel.astype(np.float32) ** 2).sum(2, dtype=np.float32) + np.float32(1e-7))
        for r in (r1, r2):
            assert (np.abs(d - r) / r).min() > 1e-4, ("a pair distance within 1e-4 of a radius", r)
        up, down = rel[:, :, 2] > 0, rel[:, :, 2] < 0
        cls = np.full(d.shape, 4)
        mid, far = (d > r1) & (d <= r2), d > r2
        cls[mid & up], cls[mid & down], cls[far & up], cls[far & down] = 0, 1, 2, 3
        hist[b] = np.bincount(cls.ravel(), minlength=5)
        z0 = z0 or bool(((rel[:, :, 2] == 0) & ~np.eye(len(a), dtype=bool)).any())
    return hist, z0


def run_reference(R, sd, inp):
    import random

    ref = R.MaskedSceneContrast(**CFG)
    ref.load_state_dict(sd(ref))
    ref.train()
    gm, mp = ref.generate_cross_masks, ref.match_contrastive_pair
    got = {}
    ref.generate_cross_masks = lambda *a, **k: got.setdefault("masks", gm(*a, **k))
    ref.match_contrastive_pair = lambda *a, **k: got.setdefault("match", mp(*a, **k))
    torch.manual_seed(DRAW_SEED)
    random.seed(DRAW_SEED)
    with G.recorded_draws() as rec:
        out = ref(dict(inp))
    out["loss"].backward()
    return ref, out, got["masks"], got["match"], rec.log


def generate():
    R = load_reference_msc_csc()
    b = G.batch()
    inp = {k: torch.from_numpy(v) for k, v in b.items()}
    for v in ("view1", "view2"):
        x = b[f"{v}_origin_coord"]
        g = np.float32(CFG["mask_grid_size"])
        assert np.array_equal(np.floor(x / g), np.floor(x * (np.float32(1.0) / g))), "a coordinate sits on a patch boundary"
    sd = om.deterministic_state_dict(R.MaskedSceneContrast(**CFG), SD_SEED)
    ref, out, masks, match, log = run_reference(R, lambda m: sd, inp)
    assert [k for k, _ in log] == ["randperm", "random", "random", "randint", "randperm"]
    idx, dist = G.knn_query(8, inp["view2_origin_coord"], inp["view2_offset"].int(), inp["view1_origin_coord"], inp["view1_offset"].int())
    cnt = (dist < CFG["matching_max_radius"]).sum(1)
    hist = torch.bincount(cnt, minlength=9).numpy()
    assert hist[0] > 0 and hist[1] > 0 and hist[8] > 0, hist
    assert int((cnt > 0).sum()) > CFG["matching_max_pair"] and match.shape[0] == CFG["matching_max_pair"]
    mi = match.numpy()
    scene = np.searchsorted(b["view1_offset"], mi[:, 0], side="right")
    assert (scene[1:] != scene[:-1]).sum() > 8, "the scenes do not interleave"
    ch, z0 = class_hist(b["view1_origin_coord"][mi[:, 0]], b["view2_origin_coord"][mi[:, 1]], scene, len(b["view1_offset"]),
                        np.float32(CFG["r1"]), np.float32(CFG["r2"]))
    assert (ch > 0).all(1).any(), ("no scene holds all five classes", ch)
    assert z0, "no rel.z == 0 off the diagonal"
    res = dict(scene_seeds=np.asarray([s for s, _ in G.SCENES]), n_points=np.asarray([n for _, n in G.SCENES]), input_keys=np.asarray(sorted(b)),
               input_checksum=G.checksum(b), sd_seed=np.asarray(SD_SEED), keys=np.asarray(list(sd.keys())),
               sd_checksum=np.asarray([float(v.double().sum()) for v in sd.values()]),
               draw_patch_perm=log[0][1].numpy(), draw_mix=np.asarray([log[1][1], log[2][1]]), draw_select_r=log[3][1].numpy(),
               draw_pair_perm=log[4][1].numpy(), view1_point_mask=masks[0].numpy(), view2_point_mask=masks[1].numpy(), match_index=mi,
               match_count_hist=hist, param_names=np.asarray([k for k, _ in ref.named_parameters()]),
               grad_norms=np.asarray([float(p.grad.double().norm()) for _, p in ref.named_parameters()]),
               r1=np.asarray(CFG["r1"]), r2=np.asarray(CFG["r2"]), partitions=np.asarray(CFG["partitions"]),
               matching_max_pair=np.asarray(CFG["matching_max_pair"]), view1_mix_prob=np.asarray(float(CFG["view1_mix_prob"])), class_hist=ch)
    for k, v in out.items():
        res["out/" + k] = np.asarray(float(v.detach()))
    for k, p in ref.named_parameters():
        if k.startswith(G.HEADS):
            res["grad/" + k] = p.grad.numpy().astype(np.float32)
    return res


def main():
    res = generate()
    np.savez_compressed(os.path.join(G.OUT, "msc_csc_tiny.npz"), **res)
    print("msc_csc_tiny.npz:", {k[4:]: float(v) for k, v in res.items() if k.startswith("out/")}, "class histogram", res["class_hist"].tolist(),
          "count histogram", res["match_count_hist"].tolist())


if __name__ == "__main__":
    main()
