"""-m gpu: MSC-v1m2, the CSC-partitioned InfoNCE (csrc/msc.hip section 5, functional.msc_csc_nce, MaskedSceneContrastCSC).  The
check_* bodies take a device; tests/test_msc_csc_cpu.py runs them on the host emulation at small shapes.

Kernel against float64: loss, pos_sim, neg_sim, dfeat1, dfeat2 of functional.msc_csc_nce against functional.msc_csc_nce_torch (the
reference's expression: scene loop, dense partition matrices, one masked CrossEntropy per class) run in float64, with the
tolerance rule of tests/test_gpu_msc.py (fixed before any kernel figure was seen): the error of the same torch expression in fp32
against the float64 result is measured in the test; the kernel may have 4 x that error and never less than 4 fp32 ulps of the
scale of the quantity (1 for pos_sim / neg_sim, max(|loss|, 1 / nce_t) for the loss, the largest float64 gradient element for dfeat1
/ dfeat2).  Both sides take the classes from the same fp32 coordinates, so float64 is a value oracle over identical classes.

Inputs (csc_inputs): several scenes of given pair counts (0 allowed: the scene counts in the divisor), match_index rows shuffled so
that scenes interleave, view-2 rows repeated, one zero feature row on each side.  Coordinates lie on a lattice of 1/32, so squared
distances are multiples of 1/1024 and the radii, placed half-way between two of them, are at least 3.8e-4 relative away from every
distance (the helper asserts 1e-4 on the torch side); the lattice also gives rel.z == 0 off the diagonal in every scene of a few
pairs.  Three radii settings: "all" (all five classes in the largest scene), "rest" (r1 beyond the scene: only the rest class, one
plain InfoNCE per scene over `partitions`), "diag" (r1 = 0.01: diagonal elements fall into classes 0-3).  The helper asserts, on
the torch side, which classes are present, and that the kernel's per-scene member counts equal the torch histogram exactly.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_msc as T  # noqa: E402
from pointcept_amd import functional as PF  # noqa: E402
from pointcept_amd import ops  # noqa: E402

NCE_FLOOR_ULPS, ULP = T.NCE_FLOOR_ULPS, T.ULP
LATTICE = 32
R_MID, R_FAR = (92.5 / 1024) ** 0.5, (655.5 / 1024) ** 0.5          # 0.3006, 0.8001: half-way between two lattice distances
RADII = {"all": (R_MID, R_FAR), "rest": (10.0, 20.0), "diag": (0.01, R_FAR)}
SHAPES = {"one_pair": (1,), "four_scenes": (1, 17, 64, 65), "middle_empty": (40, 0, 30), "one_scene_1000": (1000,)}


def dev():
    return torch.device("cuda")


def csc_inputs(device, sizes, c, seed=0, n_rows=None, repeats=True, zero_row=True):
    """-> feat1, coord1, offset1, feat2, coord2, match_index (rows shuffled across scenes)"""
    g = torch.Generator().manual_seed(seed)
    f1s, f2s, x1s, x2s, mis, off1 = [], [], [], [], [], []
    o1 = o2 = 0
    for pb in sizes:
        n1, n2 = n_rows or max(2 * pb, 4), n_rows or max(pb // 2 + 3, 4)
        f1 = torch.randn(n1, c, generator=g)
        f2 = torch.randn(n2, c, generator=g) + 0.5 * torch.randn(1, c, generator=g)
        x1 = torch.randint(0, LATTICE + 1, (n1, 3), generator=g).float() / LATTICE
        x2 = torch.randint(0, LATTICE + 1, (n2, 3), generator=g).float() / LATTICE
        i1 = torch.randperm(n1, generator=g)[:pb]
        i2 = torch.randint(n2, (pb,), generator=g) if repeats else torch.randperm(n2, generator=g)[:pb]
        jit = torch.randint(-1, 2, (pb, 3), generator=g).float() / LATTICE
        if pb:
            jit[0] = torch.tensor([0.0, 0.0, 1.0 / LATTICE])
            _, first = np.unique(i2.numpy(), return_index=True)          # the first pair of a repeated view-2 row places it
            x2[i2[first]] = (x1[i1] + jit)[first]                        # a matched pair is at most one lattice step apart
        if zero_row and pb > 2:
            f1[i1[1]] = 0
            f2[i2[2]] = 0
        f1s.append(f1), f2s.append(f2), x1s.append(x1), x2s.append(x2)
        mis.append(torch.stack([i1 + o1, i2 + o2], 1))
        o1, o2 = o1 + n1, o2 + n2
        off1.append(o1)
    mi = torch.cat(mis)
    mi = mi[torch.randperm(mi.shape[0], generator=g)]
    to = lambda t: t.to(device)
    return to(torch.cat(f1s)), to(torch.cat(x1s)), to(torch.tensor(off1, dtype=torch.int32)), to(torch.cat(f2s)), to(torch.cat(x2s)), to(mi)


def class_histogram(coord1, offset1, coord2, match_index, r1, r2):
    """torch side: [scenes, 5] members of each class (4 = the rest) over each scene's P_b x P_b partition matrix, the diagonal's
    classes, whether rel.z == 0 occurs off the diagonal; asserts that no distance is within 1e-4 relative of a radius"""
    from pointcept_amd.structure import offset2batch

    batch = offset2batch(offset1)[match_index[:, 0]]
    x1, x2 = coord1[match_index[:, 0]].float(), coord2[match_index[:, 1]].float()
    hist = torch.zeros((offset1.numel(), 5), dtype=torch.int64)
    diag, z0 = [], False
    for b in batch.unique().tolist():
        sel = batch == b
        part = PF.msc_csc_partitions(x1[sel], x2[sel], r1, r2)
        rel = x1[sel].unsqueeze(0) - x2[sel].unsqueeze(1)
        d = torch.sqrt(torch.sum(rel.pow(2), 2).add(1e-7))
        for r in (r1, r2):
            assert float(((d - r).abs() / r).min()) > 1e-4, ("a distance within 1e-4 of a radius", r)
        cls = torch.where(part < 0, torch.full_like(part, 4), part).long()
        hist[b] = torch.bincount(cls.flatten(), minlength=5).cpu()
        diag += torch.diagonal(cls).tolist()
        off = ~torch.eye(cls.shape[0], dtype=torch.bool, device=cls.device)
        z0 = z0 or bool(((rel[:, :, 2] == 0) & off).any())
    return hist, diag, z0


def _run_csc(fn, f1, x1, off1, f2, x2, mi, t, r1, r2, partitions=4):
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    loss, pos, neg = fn(a, x1, off1, b, x2, mi, t, r1, r2, partitions)
    loss.backward()
    return [loss.detach(), pos.detach(), neg.detach(), a.grad, b.grad]


def check_degeneracy(sizes, mode, hist, diag, z0):
    big = int(np.argmax(sizes))
    if mode == "all" and max(sizes) >= 17:
        assert bool((hist[big] > 0).all()), hist
    if mode == "rest":
        assert int(hist[:, :4].sum()) == 0 and int(hist[:, 4].sum()) == sum(s * s for s in sizes)
    if mode == "diag":
        assert any(k < 4 for k in diag), diag
    if max(sizes) >= 17:
        assert z0, "no rel.z == 0 off the diagonal"


def check_csc(device, sizes, c, t, mode, seed=0, partitions=4):
    r1, r2 = RADII[mode]
    f1, x1, off1, f2, x2, mi = csc_inputs(device, sizes, c, seed=seed)
    hist, diag, z0 = class_histogram(x1, off1, x2, mi, r1, r2)
    check_degeneracy(sizes, mode, hist, diag, z0)
    _, counts, _ = ops.msc_csc_nce_fwd(f1, x1, off1, f2, x2, mi, t, r1, r2, partitions)
    assert torch.equal(counts.cpu(), hist), (counts.cpu(), hist)
    ref = _run_csc(PF.msc_csc_nce_torch, f1.double(), x1, off1, f2.double(), x2, mi, t, r1, r2, partitions)
    tor = _run_csc(PF.msc_csc_nce_torch, f1, x1, off1, f2, x2, mi, t, r1, r2, partitions)
    got = _run_csc(PF.msc_csc_nce, f1, x1, off1, f2, x2, mi, t, r1, r2, partitions)
    figures = {}
    for name, r, a, k in zip(("loss", "pos_sim", "neg_sim", "dfeat1", "dfeat2"), ref, tor, got):
        big = 1.0 if name.endswith("_sim") else max(float(r.abs()), 1.0 / t) if name == "loss" else float(r.abs().max())
        e_torch = float((a.double() - r).abs().max())
        e_kernel = float((k.double() - r).abs().max())
        bound = max(4 * e_torch, NCE_FLOOR_ULPS * ULP * big)
        figures[name] = (e_kernel, e_torch, bound)
        print(f"msc_csc_nce sizes={sizes} C={c} t={t} {mode} {name}: kernel err {e_kernel:.3e}  torch fp32 err {e_torch:.3e}  bound {bound:.3e}  scale {big:.3e}")
    for name, (e_kernel, e_torch, bound) in figures.items():
        assert e_kernel <= bound, (name, sizes, c, t, mode, e_kernel, e_torch, bound)
    return figures


def _bound(ref, t):
    """2 x 4 ulps of the scale, per quantity (one floor for each of the two kernel results compared)"""
    return [2 * NCE_FLOOR_ULPS * ULP * s for s in (max(abs(float(ref[0])), 1.0 / t), 1.0, 1.0, float(ref[3].abs().max()), float(ref[4].abs().max()))]


def check_single_scene_reduction(device, p, c, t, partitions=4):
    """one scene, only the rest class: loss * partitions is the plain InfoNCE of msc_nce on the same pairs, within 2 x 4 ulps of
    max(|loss|, 1 / t); pos_sim and neg_sim within 2 x 4 ulps of 1.  The gradients of the two kernels are sums of P terms taken in
    different orders (this kernel keeps the diagonal's -1 out of its accumulators), so a few ulps of the largest element do not
    bound their difference: each is held to the float64 rule of check_nce against msc_nce_torch in float64 (the v1m1 oracle), and
    their difference to the sum of the two allowances."""
    f1, x1, off1, f2, x2, mi = csc_inputs(device, (p,), c, seed=3)
    r1, r2 = RADII["rest"]
    got = _run_csc(PF.msc_csc_nce, f1, x1, off1, f2, x2, mi, t, r1, r2, partitions)
    ref = T._run_nce(PF.msc_nce, f1, f2, mi, t)
    r64 = T._run_nce(PF.msc_nce_torch, f1.double(), f2.double(), mi, t)
    tor = T._run_nce(PF.msc_nce_torch, f1, f2, mi, t)
    scale = (partitions, 1, 1, partitions, partitions)
    failed = []
    for name, g, r, d, a, s, b in zip(("loss", "pos_sim", "neg_sim", "dfeat1", "dfeat2"), got, ref, r64, tor, scale, _bound(ref, t)):
        err = float((g * s - r).abs().max())
        if name.startswith("dfeat"):
            allow = max(4 * float((a.double() - d).abs().max()), NCE_FLOOR_ULPS * ULP * float(d.abs().max()))
            e64 = float((g.double() * s - d).abs().max())
            print(f"single scene P={p} C={c} t={t} {name}: |csc * {s} - float64 nce| {e64:.3e}  allowance {allow:.3e}")
            failed += [(name, e64, allow)] if e64 > allow else []
            b = 2 * allow
        print(f"single scene P={p} C={c} t={t} {name}: |csc * {s} - nce| {err:.3e}  bound {b:.3e}")
        failed += [(name, err, b)] if err > b else []
    assert not failed, failed


def check_permutation(device, sizes, c, t):
    f1, x1, off1, f2, x2, mi = csc_inputs(device, sizes, c, seed=4)
    r1, r2 = RADII["all"]
    a = _run_csc(PF.msc_csc_nce, f1, x1, off1, f2, x2, mi, t, r1, r2)
    perm = torch.randperm(mi.shape[0], generator=torch.Generator().manual_seed(9)).to(device)
    b = _run_csc(PF.msc_csc_nce, f1, x1, off1, f2, x2, mi[perm], t, r1, r2)
    for name, x, y, bound in zip(("loss", "pos_sim", "neg_sim", "dfeat1", "dfeat2"), a, b, _bound(a, t)):
        err = float((x - y).abs().max())
        print(f"permutation sizes={sizes} {name}: {err:.3e}  bound {bound:.3e}")
        assert err <= bound, (name, err, bound)


def check_reproducible(device, sizes, c, t):
    f1, x1, off1, f2, x2, mi = csc_inputs(device, sizes, c, seed=5)
    r1, r2 = RADII["all"]
    a = _run_csc(PF.msc_csc_nce, f1, x1, off1, f2, x2, mi, t, r1, r2)
    b = _run_csc(PF.msc_csc_nce, f1, x1, off1, f2, x2, mi, t, r1, r2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.parametrize("mode", sorted(RADII))
@pytest.mark.parametrize("t", [0.4, 0.07])
@pytest.mark.parametrize("c", [32, 96])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_csc_nce_against_float64(shape, c, t, mode):
    check_csc(dev(), SHAPES[shape], c, t, mode)


@pytest.mark.parametrize("p,c,t", [(1, 32, 0.4), (200, 96, 0.07), (1000, 96, 0.4)])
def test_single_scene_reduces_to_msc_nce(p, c, t):
    check_single_scene_reduction(dev(), p, c, t)


def test_permutation_of_match_index():
    check_permutation(dev(), (1, 17, 64, 65), 96, 0.4)
    check_permutation(dev(), (300, 0, 500), 32, 0.07)


def test_csc_nce_reproducible():
    check_reproducible(dev(), (700, 1300, 0, 1000), 96, 0.4)


def test_csc_nce_peak_memory_at_8192():
    """one scene of 8192 pairs (each dense fp32 matrix of the torch expression is 256 MB): forward + backward stay under the 32 MB
    above the inputs that test_gpu_msc.py::test_nce_peak_memory_at_8192 allows MSC-v1m1, with the same 12 000-row feature matrices"""
    f1, x1, off1, f2, x2, mi = csc_inputs(dev(), (8192,), 96, n_rows=12000, repeats=False, zero_row=False)
    r1, r2 = RADII["all"]
    a, b = f1.requires_grad_(True), f2.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, _, _ = PF.msc_csc_nce(a, x1, off1, b, x2, mi, 0.4, r1, r2)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"msc_csc_nce P=8192 C=96: peak allocation above the inputs {peak / 2**20:.1f} MB")
    assert bool(torch.isfinite(loss)) and peak < 32 * 2**20


# ---------------------------------------------------------------------------------------------------------------- model
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msc_csc_tiny.npz"))


def gold_cfg(g):
    return dict(T.GOLD_CFG, view1_mix_prob=float(g["view1_mix_prob"]), matching_max_pair=int(g["matching_max_pair"]),
                partitions=int(g["partitions"]), r1=float(g["r1"]), r2=float(g["r2"]))


def check_port_against_golden(device):
    """as test_gpu_msc.check_port_against_golden, for MaskedSceneContrastCSC and the v1m2 reference file's run: the recorded draws
    replayed give its masks and match_index exactly (the randperm cut interleaves the two scenes), its losses within 1e-4 (of
    max(|value|, 1) for the cosine means), gradient norms within 2e-2 where they are not rounding noise, head gradients within 2e-3"""
    from pointcept_amd import synthetic
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrastCSC

    g = golden()
    torch.manual_seed(0)
    model = MaskedSceneContrastCSC(**gold_cfg(g))
    model.load_state_dict(T.golden_state(g, model))
    model = model.to(device).train()
    batch = synthetic.to_torch(T.golden_batch(g), device)
    out, grads = T._model_run(model, batch, T.Recorder(T.golden_draws(g)))
    assert model.draw.i == 5
    for k in ("view1_point_mask", "view2_point_mask", "match_index"):
        assert np.array_equal(model.last[k].cpu().numpy(), g[k]), k
    mi = torch.from_numpy(g["match_index"])
    off1 = batch["view1_offset"].cpu()
    scene = torch.bucketize(mi[:, 0].contiguous(), off1, right=True)
    assert int((scene[1:] != scene[:-1]).sum()) > 8, "the scenes do not interleave"
    hist, _, z0 = class_histogram(batch["view1_origin_coord"].cpu(), off1, batch["view2_origin_coord"].cpu(), mi, float(g["r1"]), float(g["r2"]))
    assert np.array_equal(hist.numpy(), g["class_hist"]) and bool((hist > 0).all(1).any()) and z0
    assert set(out) == set(T.GOLD_LOSSES)
    for k in T.GOLD_LOSSES:
        ref = float(g["out/" + k])
        print(f"golden {k}: port {float(out[k]):.8g} reference {ref:.8g}")
        assert abs(float(out[k]) - ref) <= 1e-4 * max(abs(ref), 1.0 if k in T.COSINE_MEANS else 0.0), k
    names = [str(k) for k in g["param_names"]]
    assert names == [k for k, _ in model.named_parameters()] and set(grads) == set(names)
    norms = np.asarray([float(grads[k].double().norm()) for k in names])
    big = g["grad_norms"] > 1e-4 * g["grad_norms"].max()
    assert np.allclose(norms[big], g["grad_norms"][big], rtol=2e-2), np.abs(norms[big] / g["grad_norms"][big] - 1).max()
    heads = [k for k in g.files if k.startswith("grad/")]
    assert len(heads) == 5
    for k in heads:
        assert T._rel(grads[k[5:]], g[k]) < 2e-3, (k, T._rel(grads[k[5:]], g[k]))


def test_port_matches_reference_golden():
    check_port_against_golden(dev())


def test_state_dict_keys_are_the_references():
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrastCSC

    g = golden()
    assert list(MaskedSceneContrastCSC(**gold_cfg(g)).state_dict().keys()) == [str(k) for k in g["keys"]]


def test_registered_only_when_named():
    from pointcept_amd import compat

    assert "MSC-v1m2" not in compat.MODEL_CLASSES
    assert compat.OPT_IN_MODEL_CLASSES["MSC-v1m2"] == ("masked_scene_contrast", "MaskedSceneContrastCSC")

    class Registry:
        def __init__(self):
            self.got = {}

        def register_module(self, name, force=False, module=None):
            self.got[name] = module

    r = Registry()
    compat.register_models(r)
    assert "MSC-v1m2" not in r.got
    assert compat.register_models(r, names=["MSC-v1m2"]) == ["MSC-v1m2"] and r.got["MSC-v1m2"].__name__ == "MaskedSceneContrastCSC"


CSC_TINY_CFG = dict(T.TINY_CFG, partitions=4, r1=0.06, r2=0.2)


def test_kernel_path_against_torch_path(monkeypatch):
    """as test_gpu_msc.py::test_kernel_path_against_torch_path: one model, the same draws, PTC_MSC=0 against the kernels.  Equal
    integers; equal reconstruction losses; nce_loss within 2 x 4 ulps of max(|loss|, 1 / nce_t), pos_sim / neg_sim within 2 x 4 ulps
    of 1; every gradient within 1e-3 of its largest element"""
    from pointcept_amd import config
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrastCSC

    torch.manual_seed(0)
    model = MaskedSceneContrastCSC(**CSC_TINY_CFG).to(dev())
    batch = T.two_views([3000, 2500], 60, dev())
    monkeypatch.setattr(config, "MSC_KERNELS", False)
    rec = T.Recorder()
    out_t, grad_t = T._model_run(model, batch, rec)
    ints_t = dict(model.last)
    monkeypatch.setattr(config, "MSC_KERNELS", True)
    out_k, grad_k = T._model_run(model, batch, T.Recorder(rec.log))
    for k in ("view1_point_mask", "view2_point_mask", "match_index"):
        assert torch.equal(ints_t[k], model.last[k]), k
    assert ints_t["match_index"].shape[0] == CSC_TINY_CFG["matching_max_pair"]
    assert set(out_k) == set(T.GOLD_LOSSES) == set(out_t)
    for k in out_k:
        print(k, float(out_k[k]), float(out_t[k]))
    t = CSC_TINY_CFG["nce_t"]
    nce_bound = 2 * NCE_FLOOR_ULPS * ULP * max(abs(float(out_t["nce_loss"])), 1.0 / t)
    assert abs(float(out_k["nce_loss"]) - float(out_t["nce_loss"])) <= nce_bound
    for k in ("pos_sim", "neg_sim"):
        assert abs(float(out_k[k]) - float(out_t[k])) <= 2 * NCE_FLOOR_ULPS * ULP
    for k in ("color_loss", "normal_loss"):
        assert float(out_k[k]) == float(out_t[k]), k
    assert set(grad_k) == set(n for n, _ in model.named_parameters()) == set(grad_t)
    for k in grad_k:
        assert T._rel(grad_k[k], grad_t[k]) < 1e-3, (k, T._rel(grad_k[k], grad_t[k]))


def check_config_recipe(device, sizes):
    """the settings of configs/scannet/pretrain-msc-v1m2-0-spunet-csc.py at a reduced size: mask_rate = 0, no reconstruction heads,
    partitions = 4, r1 = 2, r2 = 20"""
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrastCSC

    torch.manual_seed(0)
    model = MaskedSceneContrastCSC(backbone=T.TINY_BACKBONE, backbone_in_channels=6, backbone_out_channels=32, mask_grid_size=0.1, mask_rate=0,
                                   view1_mix_prob=0, view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=4096,
                                   nce_t=0.4, contrast_weight=1, reconstruct_weight=1, reconstruct_color=False, reconstruct_normal=False,
                                   partitions=4, r1=2, r2=20).to(device)
    batch = T.two_views(sizes, 80, device)
    out = model(dict(batch))
    out["loss"].backward()
    assert set(out) == {"nce_loss", "pos_sim", "neg_sim", "loss"}
    for k, v in out.items():
        assert bool(torch.isfinite(v)), k
    assert not bool(model.last["view1_point_mask"].any()) and not bool(model.last["view2_point_mask"].any())
    assert model.last["match_index"].shape[0] > 64
    for k, p in model.backbone.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    return out


def test_config_recipe_step():
    check_config_recipe(dev(), [20000, 15000])
