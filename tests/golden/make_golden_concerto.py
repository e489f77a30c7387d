"""Generate tests/golden/concerto_tiny.npz by running the REFERENCE'S OWN Concerto file (pointcept/models/concerto/
concerto_v1m1_base.py, imported unmodified through oracle/ref_import.py on the CPU stand-ins of oracle/shims.py; its backbone the
reference's PT-v3m2 from its own registry) in fp32.  Process-local patches that live here: `torch.Tensor.cuda` as identity,
`load_enc2d` replaced on the imported class by pointcept_amd.synthetic.stand_in_image_encoder, `transformers` as an empty stub (its
AutoModel is never reached), `torch_scatter.segment_coo` / `pointops.knn_query` / the recorded draws of make_golden_sonata.py, and
stand-ins for `torch_scatter.segment_csr` (reduce = "sum") and `torch_scatter.scatter_mean`.  Only runnable where the reference tree
exists; the .npz output is committed.

    python tests/golden/make_golden_concerto.py

concerto_tiny.npz: CFG below -- the tiny PT-v3m2 of the Sonata golden on its fp32 attention branch, all four loss weights on,
sonata_model_type "online", up_cast_level 1 and enc2d_upcast_level 2, so that the 2D-3D term works one level above the distillation
heads with TWO pooling levels under it (the shipped config has one), a 6 x 5 patch grid, 24 image channels -- on two scenes from
pointcept_amd.synthetic.multi_view_image_batch with 3 and 2 images (the second scene's third view is padding, -1).  Stored: the
recorded draws, the pooled correspondence of both levels (each from the reference's own pool_corr), the argument and the result of
the reference's torch.unique over the patch keys, every entry of the result dict, the gradient norm of every student parameter, the
full gradient of patch_proj, and the state-dict key list with a float64 sum per tensor.  The generator asserts that every match list
and the patch list are non-empty, that a patch holds several pairs, that a cluster has no valid member for some image, that no pooled
pixel coordinate lies outside its image (where the reference would alias into another image's patches and the port leaves the pair
out), and that no pooled coordinate of the second level lies within 1e-4 of an integer unless all members of its cluster are equal:
there the order of summation, which the reference leaves to torch.sort, could change the patch a point falls into.
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
sys.path.insert(0, OUT)

import make_golden_sonata as MS  # noqa: E402
from oracle import ref_import  # noqa: E402
from pointcept_amd import synthetic  # noqa: E402

BACKBONE = dict(MS.BACKBONE)
PATCH_H, PATCH_W, ENC2D_CHANNELS = 6, 5, 24
CFG = dict(image_weight_name="stand-in", image_weight_path=None, backbone=BACKBONE, head_in_channels=256 + 512,
           backbone_out_channels=128 + 256 + 512, embedding_channels=ENC2D_CHANNELS, patch_w=PATCH_W, patch_h=PATCH_H,
           head_hidden_channels=32, head_embed_channels=16, head_num_prototypes=64, enc2d_head_in_channels=ENC2D_CHANNELS,
           enc2d_head_hidden_channels=32, enc2d_head_embed_channels=16, enc2d_head_num_prototypes=16, teacher_custom=dict(drop_path=0.0),
           num_global_view=2, num_local_view=4, mask_size_start=0.1, mask_ratio_start=0.3, mask_jitter=0.0008, teacher_temp_start=0.04,
           student_temp=0.1, mask_loss_weight=2 / 10, roll_mask_loss_weight=2 / 10, unmask_loss_weight=4 / 10, enc2d_loss_weight=2 / 10,
           match_max_r=0.12, up_cast_level=1, enc2d_upcast_level=2, enc2d_cos_shift=True, sonata_model_type="online")
SCENE_SEEDS = (71, 72)
IMG_NUMS = (3, 2)
GLOBAL_SIZE, LOCAL_SIZE = 600, 250
SD_SEED = 19
DRAW_SEED = 3
ORDER_SEED = 5
LOSSES = ("mask_loss", "roll_mask_loss", "unmask_loss", "enc2d_loss", "loss")


def segment_csr(src, indptr, out=None, reduce="sum"):
    """torch_scatter.segment_csr over dim 0 for the calls of pool_corr"""
    assert out is None and reduce == "sum"
    m = indptr.numel() - 1
    seg = torch.repeat_interleave(torch.arange(m), indptr[1:] - indptr[:-1])
    return torch.zeros((m,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, seg, src[: seg.numel()])


def scatter_mean(src, index, dim=0, out=None, dim_size=None):
    assert dim == 0 and out is None and dim_size is not None
    total = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype).index_add(0, index, src)
    count = torch.bincount(index, minlength=dim_size).clamp(min=1).to(src.dtype)
    return total / count.view((-1,) + (1,) * (src.dim() - 1))


def stand_in_encoder():
    return synthetic.stand_in_image_encoder(PATCH_H, PATCH_W, ENC2D_CHANNELS)


def load_reference_concerto():
    MS.load_reference_sonata()                    # the stand-ins of the Sonata generator, PT-v3m2 registered
    ts = sys.modules["torch_scatter"]
    shim_csr = ts.segment_csr if not hasattr(ts.segment_csr, "_concerto") else ts.segment_csr._concerto

    def csr(src, indptr, out=None, reduce="sum"):
        return segment_csr(src, indptr, out, reduce) if reduce == "sum" else shim_csr(src, indptr, out, reduce)

    csr._concerto = shim_csr
    ts.segment_csr, ts.scatter_mean = csr, scatter_mean
    if "transformers" not in sys.modules:
        sys.modules["transformers"] = types.SimpleNamespace(AutoModel=None)
    if "timm" not in sys.modules:
        timm, layers = types.ModuleType("timm"), types.ModuleType("timm.layers")
        layers.trunc_normal_ = torch.nn.init.trunc_normal_
        timm.layers = layers
        sys.modules["timm"], sys.modules["timm.layers"] = timm, layers
    mu = sys.modules["pointcept.models.utils"]
    if not hasattr(mu, "bincount2offset"):
        mu.bincount2offset = lambda bincount: torch.cumsum(bincount, dim=0)
    torch.Tensor.cuda = lambda self, *a, **k: self
    name = "pointcept.models.concerto.concerto_v1m1_base"
    if name not in sys.modules:
        pk = types.ModuleType("pointcept.models.concerto")
        pk.__path__ = [ref_import.REF + "/pointcept/models/concerto"]
        sys.modules["pointcept.models.concerto"] = pk
    R = importlib.import_module(name)
    R.Concerto.load_enc2d = lambda self, model_name, model_weight: stand_in_encoder()
    return R


def batch():
    return synthetic.multi_view_image_batch(list(SCENE_SEEDS), GLOBAL_SIZE, LOCAL_SIZE, list(IMG_NUMS), PATCH_H, PATCH_W)


def state_dict_for(model):
    MS.SD_SEED, keep = SD_SEED, MS.SD_SEED
    try:
        return MS.state_dict_for(model)
    finally:
        MS.SD_SEED = keep


class recorded_unique:
    """records (argument, result) of the plain torch.unique(x) calls -- the one over the patch keys (:830)"""

    def __init__(self):
        self.log = []

    def __enter__(self):
        self.saved = torch.unique

        def f(*a, **k):
            v = self.saved(*a, **k)
            if len(a) == 1 and not k:
                self.log.append((a[0].clone(), v.clone()))
            return v

        torch.unique = f
        return self

    def __exit__(self, *exc):
        torch.unique = self.saved


def generate():
    R = load_reference_concerto()
    b = batch()
    inp = {k: torch.from_numpy(v) for k, v in b.items()}
    torch.manual_seed(0)
    ref = R.Concerto(**{**CFG, "backbone": dict(BACKBONE)})
    sd = state_dict_for(ref)
    ref.load_state_dict(sd)
    ref.train()
    kept = {"match": [], "chain": []}
    gm, mn, pc = ref.generate_mask, ref.match_neighbour, R.Concerto.pool_corr
    ref.generate_mask = lambda *a, **k: kept.setdefault("mask", gm(*a, **k))
    ref.match_neighbour = lambda *a, **k: (kept["match"].append(mn(*a, **k)), kept["match"][-1])[1]

    def pool_corr(point, correspondence):
        p = point
        while "pooling_parent" in p.keys():
            kept["chain"].append((p["pooling_inverse"].clone(), p["idx_ptr"].clone()))
            p = p["pooling_parent"]
        kept["corr_in"] = correspondence.clone()
        kept["to_feature"] = pc(point, correspondence)
        return kept["to_feature"]

    ref.pool_corr = pool_corr
    del MS.KNN_LOG[:]
    torch.manual_seed(DRAW_SEED)
    with MS.recorded_draws() as rec, recorded_unique() as uni:
        out = ref(dict(inp))
    out["loss"].backward()
    assert [k for k, _ in rec.log] == ["randperm", "randn_like"], [k for k, _ in rec.log]
    assert sorted(out) == sorted(LOSSES) and len(kept["match"]) == 3 == len(MS.KNN_LOG) and len(uni.log) == 1
    assert all(mi.shape[0] > 0 for mi in kept["match"]), "an empty match list"

    # ---- the pooled correspondence of every level, each from the reference's own pool_corr on a one-level chain
    chain = kept["chain"][::-1]                                   # from the input points down
    assert len(chain) == 2, "two pooling levels lie under the enc2d point"
    Point = sys.modules["pointcept.models.utils.structure"].Point
    levels, corr = [], kept["corr_in"]
    for inverse, idx_ptr in chain:
        m = idx_ptr.numel() - 1
        one = Point(dict(offset=torch.tensor([m]), feat=torch.zeros(m, 1), pooling_inverse=inverse, idx_ptr=idx_ptr,
                         pooling_parent=Point(dict(offset=torch.tensor([inverse.numel()]), feat=torch.zeros(inverse.numel(), 1)))))
        corr = pc(one, corr)["correspondence"]
        levels.append(corr)
    assert torch.equal(levels[-1], kept["to_feature"]["correspondence"])
    assert bool((levels[0][..., 0] == -1).any()) and bool((levels[1][..., 0] == -1).any()), "no cluster without a valid member"
    # second level: a coordinate within 1e-4 of an integer only where every member of the cluster holds that value
    inverse, idx_ptr = chain[1]
    valid = (levels[0] != -1).all(-1)                                     # [M1, V]
    lo = torch.full(levels[1].shape, float("inf")).index_reduce_(0, inverse, torch.where(valid[..., None], levels[0], torch.tensor(float("inf"))), "amin")
    hi = torch.full(levels[1].shape, -float("inf")).index_reduce_(0, inverse, torch.where(valid[..., None], levels[0], torch.tensor(-float("inf"))), "amax")
    near = ((levels[1] - levels[1].round()).abs() < 1e-4) & (levels[1] != -1)
    assert bool((lo[near] == hi[near]).all()), "a pooled coordinate of the second level sits on a patch boundary"
    final = levels[-1]
    live = (final != -1).any(-1)
    r, c = final[..., 0].long(), final[..., 1].long()
    assert bool(((r >= 0) & (r < PATCH_H) & (c >= 0) & (c < PATCH_W))[live].all()), "a pooled coordinate outside its image"
    assert not bool(live[:, IMG_NUMS[1]:][kept["to_feature"]["offset"][1]:].any()), "a padded view holds a pair"

    keys_all, patch_ids = uni.log[0]
    assert patch_ids.numel() > 0 and int(torch.bincount(keys_all).max()) >= 2, "no patch holds several pairs"

    mask, cluster = kept["mask"]
    params = [(k, p) for k, p in ref.named_parameters() if k.startswith("student.")]
    assert all(p.grad is None for k, p in ref.named_parameters() if k.startswith(("teacher.", "enc2d_model.", "enc2d_head_")))
    res = dict(scene_seeds=np.asarray(SCENE_SEEDS), img_nums=np.asarray(IMG_NUMS), view_sizes=np.asarray([GLOBAL_SIZE, LOCAL_SIZE]),
               input_keys=np.asarray(sorted(b)), input_checksum=MS.checksum(b), sd_seed=np.asarray(SD_SEED),
               order_seed=np.asarray(ORDER_SEED), keys=np.asarray(list(sd.keys())),
               sd_checksum=np.asarray([float(v.double().sum()) for v in sd.values()]),
               draw_patch_perm=rec.log[0][1].numpy(), draw_jitter=rec.log[1][1].numpy(),
               global_mask=mask.numpy(), global_cluster=cluster.numpy().astype(np.int64),
               mask_match_index=kept["match"][0].numpy(), roll_mask_match_index=kept["match"][1].numpy(),
               unmask_match_index=kept["match"][2].numpy(),
               pooled_correspondence_0=levels[0].numpy().astype(np.float32), pooled_correspondence_1=levels[1].numpy().astype(np.float32),
               patch_ids=patch_ids.numpy().astype(np.int64), num_pairs=np.asarray(int(keys_all.numel())),
               param_names=np.asarray([k for k, _ in params]),
               grad_norms=np.asarray([0.0 if p.grad is None else float(p.grad.double().norm()) for _, p in params]),
               has_grad=np.asarray([p.grad is not None for _, p in params]))
    for k in LOSSES:
        res["out/" + k] = np.asarray(float(out[k].detach()))
    for k, p in ref.named_parameters():
        if k.startswith("patch_proj."):
            res["grad/" + k] = p.grad.numpy().astype(np.float32)
    return res


def main():
    res = generate()
    np.savez_compressed(os.path.join(OUT, "concerto_tiny.npz"), **res)
    print("concerto_tiny.npz:", len(res["keys"]), "state entries;", {k: float(res["out/" + k]) for k in LOSSES}, "pairs",
          int(res["num_pairs"]), "patches", int(res["patch_ids"].shape[0]), "levels",
          [tuple(res[f"pooled_correspondence_{i}"].shape) for i in range(2)])


if __name__ == "__main__":
    main()
