"""-m gpu: Masked Scene Contrast (csrc/msc.hip, pointcept_amd/masked_scene_contrast.py).  The check_* bodies take a device;
tests/test_msc_cpu.py runs them on the host emulation at small shapes.

Matching: counts and lists exactly equal ops.knn_query(8, ...) + `dist < max_radius` (the brute-force kernel) on designed cases and
at 2 x 100 000 points; pair selection exactly the torch expression of masked_scene_contrast_v1m1_base.py:154-169.
Cross masks: exactly the reference expression (:69-141 written on torch_geometric_api.voxel_grid) for a given rand_perm.
InfoNCE: loss, pos_sim, neg_sim, dfeat1, dfeat2 against a float64 restatement.  Tolerance (set before any kernel figure was seen):
the error of the reference's own fp32 torch expression against the same float64 result on the same inputs and device is measured in
the test; the kernel may have 4 x that error (headroom for another summation order at equal precision), and never less than
NCE_FLOOR_ULPS = 4 fp32 ulps (4 * 2^-23) of the largest value that enters the quantity compared -- an fp32 result cannot be asked
to be closer than a few roundings of its largest term.  That value is: for pos_sim / neg_sim 1.0 (they are means of dot products of
unit vectors; the rounding error of a dot product scales with sum |a_i b_i| <= 1, not with the possibly cancelling result); for the
loss max(|loss|, 1 / nce_t) (it is a mean of lse_i - S_ii / nce_t, terms of that size); for dfeat1 / dfeat2 the largest gradient
element of the float64 result.  Every figure is printed before it is asserted.
Measured on the MI355X (profiles/msc_ops.txt), kernel | torch fp32 expression, largest absolute error: P = 8192, C = 96, t = 0.4: dfeat1
5.1e-3 | 5.1e-3 of 6.4e2, dfeat2 2.8e-3 | 2.7e-3 of 1.7e3; t = 0.07: dfeat1 2.4e-2 | 2.4e-2 of 3.6e3, dfeat2 1.8e-2 | 1.9e-2 of 9.8e3
(the zero feature row sets the scale, 1 / 1e-7); the three scalars within 4 ulps of their scale on both sides.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pointcept_amd import functional as PF  # noqa: E402
from pointcept_amd import ops  # noqa: E402

K = 8
NCE_FLOOR_ULPS = 4
ULP = 2.0 ** -23


def dev():
    return torch.device("cuda")


# ---------------------------------------------------------------------------------------------------------------- matching
def designed_cases():
    """name -> (view-2 xyz, view-2 offset, view-1 xyz, view-1 offset, max_radius)"""
    rng = np.random.default_rng(3)
    f = np.float32
    cases = {}
    r = f(0.03)
    # scene 0: fewer than k points; scene 1: empty in view 2; scene 2: dense
    v2 = np.concatenate([rng.normal(0, 0.01, (5, 3)), rng.normal(1, 0.02, (400, 3))]).astype(f)
    v1 = np.concatenate([rng.normal(0, 0.01, (30, 3)), rng.normal(0, 0.01, (20, 3)), rng.normal(1, 0.02, (300, 3))]).astype(f)
    cases["few_empty_dense"] = (v2, [5, 5, 405], v1, [30, 50, 350], r)
    # exactly k and k + 1 neighbours in range, duplicates (ties by index), a point at distance exactly max_radius
    q = np.zeros((3, 3), f)
    q[1, 0], q[2, 0] = 10, 20
    ring = lambda c, n, d: np.stack([c + d * np.cos(np.arange(n)), d * np.sin(np.arange(n)), np.zeros(n)], 1)
    v2 = np.concatenate([ring(0, K, 0.01), ring(10, K + 1, 0.01), np.tile([[20.0, 0, 0]], (3, 1)), [[20.0 + 0.25, 0, 0]], [[20.0, 0.125, 0]]]).astype(f)
    cases["k_kplus1_dup_boundary"] = (v2, [len(v2)], q, [3], f(0.25))
    # non-finite rows on both sides
    v2 = rng.normal(0, 0.02, (200, 3)).astype(f)
    v1 = rng.normal(0, 0.02, (100, 3)).astype(f)
    v2[7, 1], v2[9, 0], v1[3, 2], v1[4, 0] = np.nan, np.inf, np.nan, -np.inf
    cases["nan_rows"] = (v2, [200], v1, [100], r)
    # extent / radius far beyond the 16-bit cell fields: the cell edge grows
    v2 = np.concatenate([rng.normal(0, 0.02, (300, 3)), rng.normal(0, 0.02, (300, 3)) + 9000.0]).astype(f)
    v1 = np.concatenate([rng.normal(0, 0.02, (150, 3)), rng.normal(0, 0.02, (150, 3)) + 9000.0, rng.normal(0, 0.02, (20, 3)) - 5000.0]).astype(f)
    cases["wild_extent_grows_cells"] = (v2, [600], v1, [320], r)
    cases["m_zero"] = (rng.normal(0, 0.02, (50, 3)).astype(f), [50], np.zeros((0, 3), f), [0], r)
    cases["n_zero"] = (np.zeros((0, 3), f), [0], rng.normal(0, 0.02, (50, 3)).astype(f), [50], r)
    return cases


def _t(a, device, dtype=None):
    if torch.is_tensor(a):
        return a.to(device=device, dtype=dtype or a.dtype)
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(device)


def check_match(device, v2, off2, v1, off1, radius, oracle=None):
    x2, x1 = _t(v2, device), _t(v1, device)
    o2, o1 = _t(off2, device, torch.int32), _t(off1, device, torch.int32)
    count, cand, stats = ops.msc_match(K, float(radius), x2, o2, x1, o1)
    if x1.shape[0]:
        cnt_ref, cand_ref = PF.msc_candidates_torch(K, float(radius), x2, o2, x1, o1)
    else:
        cnt_ref, cand_ref = torch.zeros(0, dtype=torch.int32), torch.zeros((0, K), dtype=torch.int32)
    assert torch.equal(count.cpu(), cnt_ref.cpu())
    assert torch.equal(cand.cpu(), cand_ref.cpu())
    n_matched, max_count = stats.tolist()
    assert n_matched == int((cnt_ref > 0).sum()) and max_count == (int(cnt_ref.max()) if cnt_ref.numel() else 0)
    if oracle is not None:
        idx, dist = oracle(K, x2.cpu().numpy(), o2.cpu().numpy(), x1.cpu().numpy(), o1.cpu().numpy())
        keep = dist < np.float32(radius)
        assert np.array_equal(count.cpu().numpy(), keep.sum(1)) and np.array_equal(cand.cpu().numpy(), np.where(keep, idx, -1))
    return count, cand, stats


def check_select(device, count, cand, seed=0):
    n_matched = int((count > 0).sum())
    if n_matched == 0:
        assert ops.msc_select(count, cand, torch.zeros(0, dtype=torch.int64, device=device)).shape == (0, 2)
        return None
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(int(count.max()), (n_matched,), generator=g).to(device)
    got = ops.msc_select(count, cand, r)
    ref = PF.msc_select_torch(count, cand, r)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref.cpu())
    return got


def two_views(sizes, seed, device, jitter=0.004, shift=(-1.3, 0.4, -0.2)):
    """origin coordinates of two overlapping crops per scene (some negative), as collated view1_* / view2_* tensors"""
    from pointcept_amd import synthetic

    b = synthetic.contrastive_views_batch([seed + i for i in range(len(sizes))], sizes, shift=shift, jitter=jitter)
    return synthetic.to_torch(b, device)


# ---------------------------------------------------------------------------------------------------------------- cross masks
def cross_masks_reference(o1, off1, o2, off2, grid, rate, rand_perm):
    """generate_cross_masks (:69-141) as the reference writes it, on torch_geometric_api.voxel_grid"""
    from itertools import chain

    from pointcept_amd.structure import offset2batch
    from pointcept_amd.torch_geometric_api import voxel_grid

    b1, b2 = offset2batch(off1.long()), offset2batch(off2.long())
    c1, c2 = b1.bincount(minlength=off1.numel()), b2.bincount(minlength=off2.numel())
    union = torch.cat(list(chain.from_iterable(zip(o1.split(c1.tolist()), o2.split(c2.tolist())))))
    union_batch = offset2batch((off1.long() + off2.long()))
    cluster_id = voxel_grid(pos=torch.floor(union.div(grid)), size=1, batch=union_batch, start=0)
    unique, cluster, counts = torch.unique(cluster_id, sorted=True, return_inverse=True, return_counts=True)
    patch_num = unique.shape[0]
    perm = rand_perm(patch_num)
    k = int(patch_num * rate)
    patch_mask = torch.zeros(patch_num, dtype=torch.int32)
    patch_mask[perm[0:k]] = 1
    patch_mask[perm[k:2 * k]] = 2
    point_mask = patch_mask.to(o1.device)[cluster]
    parts = point_mask.split(torch.stack([c1, c2], -1).flatten().tolist())
    return torch.cat(parts[0::2]) == 1, torch.cat(parts[1::2]) == 2, patch_num, counts


def check_cross_masks(device, o1, off1, o2, off2, grid, rate, seed=0):
    perm_of = lambda n: torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    m1, m2 = ops.msc_cross_masks(o1, off1, o2, off2, grid, rate, rand_perm=perm_of)
    r1, r2, patch_num, counts = cross_masks_reference(o1, off1, o2, off2, grid, rate, perm_of)
    assert m1.dtype == torch.bool and torch.equal(m1.cpu(), r1.cpu()) and torch.equal(m2.cpu(), r2.cpu())
    # view 1 holds only tag 1, view 2 only tag 2: a patch is masked in at most one view
    c1 = torch.floor(o1.float().div(grid))
    c2 = torch.floor(o2.float().div(grid))
    cluster, pn = ops.msc_patch_rank(c1, off1, c2, off2)
    assert int(pn) == patch_num
    t1 = torch.zeros(patch_num, dtype=torch.bool, device=device).index_put_((cluster[: len(o1)][m1].long(),), torch.tensor(True, device=device))
    t2 = torch.zeros(patch_num, dtype=torch.bool, device=device).index_put_((cluster[len(o1):][m2].long(),), torch.tensor(True, device=device))
    assert not bool((t1 & t2).any())
    return m1, m2, patch_num, counts


# ---------------------------------------------------------------------------------------------------------------- InfoNCE
def nce_inputs(device, p, c, n1=None, n2=None, seed=0, repeats=True, zero_row=True):
    g = torch.Generator().manual_seed(seed)
    n1, n2 = n1 or max(2 * p, 8), n2 or max(p // 2 + 3, 8)
    f1 = torch.randn(n1, c, generator=g)
    f2 = torch.randn(n2, c, generator=g) + 0.5 * torch.randn(1, c, generator=g)
    i1 = torch.randperm(n1, generator=g)[:p]
    i2 = torch.randint(n2, (p,), generator=g) if repeats else torch.randperm(n2, generator=g)[:p]      # view-2 rows repeat
    if zero_row and p > 2:
        f1[i1[1]] = 0
        f2[i2[2]] = 0
    return f1.to(device), f2.to(device), torch.stack([i1, i2], 1).to(device)


def _run_nce(fn, f1, f2, mi, t):
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    loss, pos, neg = fn(a, b, mi, t)
    loss.backward()
    return [loss.detach(), pos.detach(), neg.detach(), a.grad, b.grad]


def check_nce(device, p, c, t, seed=0):
    f1, f2, mi = nce_inputs(device, p, c, seed=seed)
    ref = _run_nce(PF.msc_nce_torch, f1.double(), f2.double(), mi, t)
    tor = _run_nce(PF.msc_nce_torch, f1, f2, mi, t)
    got = _run_nce(PF.msc_nce, f1, f2, mi, t)
    figures = {}
    for name, r, a, k in zip(("loss", "pos_sim", "neg_sim", "dfeat1", "dfeat2"), ref, tor, got):
        big = 1.0 if name.endswith("_sim") else max(float(r.abs()), 1.0 / t) if name == "loss" else float(r.abs().max())
        e_torch = float((a.double() - r).abs().max())
        e_kernel = float((k.double() - r).abs().max())
        bound = max(4 * e_torch, NCE_FLOOR_ULPS * ULP * big)
        figures[name] = (e_kernel, e_torch, bound)
        print(f"msc_nce P={p} C={c} t={t} {name}: kernel err {e_kernel:.3e}  torch fp32 err {e_torch:.3e}  bound {bound:.3e}  scale {big:.3e}")
    for name, (e_kernel, e_torch, bound) in figures.items():
        assert e_kernel <= bound, (name, p, c, t, e_kernel, e_torch, bound)
    return figures


def check_nce_reproducible(device, p, c, t):
    f1, f2, mi = nce_inputs(device, p, c, seed=5)
    a = _run_nce(PF.msc_nce, f1, f2, mi, t)
    b = _run_nce(PF.msc_nce, f1, f2, mi, t)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.parametrize("name", sorted(designed_cases()))
def test_match_designed(name):
    count, cand, _ = check_match(dev(), *designed_cases()[name])
    check_select(dev(), count, cand)


def test_match_designed_counts():
    """the designed rings hold what their names say"""
    count, _, _ = check_match(dev(), *designed_cases()["k_kplus1_dup_boundary"])
    assert count.tolist() == [K, K, 4]          # k of k; k of k + 1; three duplicates + (0, .125, 0); the point at exactly 0.25 is out


def test_match_2x100k_against_brute_force():
    b = two_views([100000, 100000], 40, dev())
    count, cand, stats = check_match(dev(), b["view2_origin_coord"], b["view2_offset"], b["view1_origin_coord"], b["view1_offset"], 0.03)
    hist = torch.bincount(count.long(), minlength=K + 1)
    assert int(hist[0]) > 0 and int(hist[1]) > 0 and int(hist[K]) > 0
    check_select(dev(), count, cand, seed=3)


def test_cross_masks():
    b = two_views([60000, 40000], 50, dev())
    for rate in (0.4, 0.5):
        m1, m2, patch_num, _ = check_cross_masks(dev(), b["view1_origin_coord"], b["view1_offset"], b["view2_origin_coord"], b["view2_offset"], 0.1, rate)
        assert bool((b["view1_origin_coord"] < 0).any()) and patch_num > 100 and bool(m1.any()) and bool(m2.any())


def test_cross_masks_one_large_patch():
    """a patch holding more than half of a scene, and negative cells whose ids collide"""
    g = torch.Generator().manual_seed(1)
    o1 = torch.cat([torch.rand(700, 3, generator=g) * 0.09 + 0.2, torch.rand(300, 3, generator=g) * 4 - 2]).to(dev())
    o2 = (torch.rand(800, 3, generator=g) * 4 - 2).to(dev())
    off1, off2 = torch.tensor([1000], device=dev()), torch.tensor([800], device=dev())
    for seed in range(3):
        _, _, _, counts = check_cross_masks(dev(), o1, off1, o2, off2, 0.1, 0.5, seed=seed)
    assert int(counts.max()) > 500


@pytest.mark.parametrize("t", [0.4, 0.07])
@pytest.mark.parametrize("c", [32, 96])
@pytest.mark.parametrize("p", [1, 17, 1000, 8192])
def test_nce_against_float64(p, c, t):
    check_nce(dev(), p, c, t)


def test_nce_reproducible():
    check_nce_reproducible(dev(), 3000, 96, 0.4)


def test_nce_peak_memory_at_8192():
    """the P x P matrix (256 MB) never exists: forward + backward stay under 32 MB above the inputs.  The feature matrices have
    12 000 rows so that the two dense gradient tensors the backward returns (2 x 12 000 x 96 fp32 = 9.2 MB; 2 x 127 MB at the
    ScanNet config's 330 000 rows, as for the torch expression) fit under the limit: what is bounded is the working set of the loss."""
    f1, f2, mi = nce_inputs(dev(), 8192, 96, n1=12000, n2=12000, repeats=False, zero_row=False)
    a, b = f1.requires_grad_(True), f2.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, _, _ = PF.msc_nce(a, b, mi, 0.4)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"msc_nce P=8192 C=96: peak allocation above the inputs {peak / 2**20:.1f} MB")
    assert peak < 32 * 2**20


# ---------------------------------------------------------------------------------------------------------------- model
TINY_BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, base_channels=16, channels=(16, 32, 48, 64, 64, 48, 32, 32),
                     layers=(1, 2, 1, 1, 1, 1, 2, 1))
TINY_CFG = dict(backbone=TINY_BACKBONE, backbone_in_channels=6, backbone_out_channels=32, mask_grid_size=0.1, mask_rate=0.4,
                view1_mix_prob=0.8, view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=512, nce_t=0.4,
                contrast_weight=1, reconstruct_weight=1, reconstruct_color=True, reconstruct_normal=True)


GOLD_CFG = dict(TINY_CFG, matching_max_pair=256)
GOLD_LOSSES = ("nce_loss", "pos_sim", "neg_sim", "color_loss", "normal_loss", "loss")
COSINE_MEANS = ("pos_sim", "neg_sim", "normal_loss")


def golden():
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msc_tiny.npz"))


def golden_batch(g):
    """the fixture's two-view batch, regenerated from its seeds and checked against its checksums"""
    from pointcept_amd import synthetic

    b = synthetic.contrastive_views_batch([int(s) for s in g["scene_seeds"]], [int(n) for n in g["n_points"]])
    assert sorted(b) == [str(k) for k in g["input_keys"]]
    assert np.array_equal(np.asarray([float(b[k].astype(np.float64).sum()) for k in sorted(b)]), g["input_checksum"])
    return b


def golden_state(g, model):
    """the fixture's deterministic weights for `model` (same key list, same float64 sums)"""
    from oracle.ptv3_model import deterministic_state_dict

    sd = deterministic_state_dict(model, int(g["sd_seed"]))
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert np.allclose([float(v.double().sum()) for v in sd.values()], g["sd_checksum"], rtol=0, atol=1e-9)
    return sd


def golden_draws(g):
    return [("patch_perm", torch.from_numpy(g["draw_patch_perm"])), ("mix", float(g["draw_mix"][0])), ("mix", float(g["draw_mix"][1])),
            ("select", torch.from_numpy(g["draw_select_r"])), ("pair_perm", torch.from_numpy(g["draw_pair_perm"]))]


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def check_port_against_golden(device):
    """the port, with the reference run's draws replayed, gives the reference file's integers exactly and its losses and gradients
    at the fp32 tolerances of the SpUNet golden test (tests/test_gpu_spunet.py: loss 1e-4 relative, head gradients 2e-3 of their
    largest element, gradient norms 2e-2 where they are not rounding noise).  pos_sim, neg_sim and normal_loss are means of cosines:
    their 1e-4 is taken of max(|value|, 1), the size of their terms."""
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrast

    g = golden()
    torch.manual_seed(0)
    model = MaskedSceneContrast(**GOLD_CFG)
    model.load_state_dict(golden_state(g, model))
    model = model.to(device).train()
    from pointcept_amd import synthetic

    batch = synthetic.to_torch(golden_batch(g), device)
    out, grads = _model_run(model, batch, Recorder(golden_draws(g)))
    assert model.draw.i == 5
    for k in ("view1_point_mask", "view2_point_mask", "match_index"):
        assert np.array_equal(model.last[k].cpu().numpy(), g[k]), k
    hist = g["match_count_hist"]
    assert hist[0] > 0 and hist[1] > 0 and hist[K] > 0 and g["match_index"].shape[0] == GOLD_CFG["matching_max_pair"] < int(hist[1:].sum())
    assert set(out) == set(GOLD_LOSSES)
    for k in GOLD_LOSSES:
        ref = float(g["out/" + k])
        print(f"golden {k}: port {float(out[k]):.8g} reference {ref:.8g}")
        assert abs(float(out[k]) - ref) <= 1e-4 * max(abs(ref), 1.0 if k in COSINE_MEANS else 0.0), k
    names = [str(k) for k in g["param_names"]]
    assert names == [k for k, _ in model.named_parameters()] and set(grads) == set(names)
    norms = np.asarray([float(grads[k].double().norm()) for k in names])
    big = g["grad_norms"] > 1e-4 * g["grad_norms"].max()
    assert np.allclose(norms[big], g["grad_norms"][big], rtol=2e-2), np.abs(norms[big] / g["grad_norms"][big] - 1).max()
    heads = [k for k in g.files if k.startswith("grad/")]
    assert len(heads) == 5
    for k in heads:
        assert _rel(grads[k[5:]], g[k]) < 2e-3, (k, _rel(grads[k[5:]], g[k]))


class Recorder:
    """records the draws of a run / replays them into another one"""

    def __init__(self, replay=None):
        self.replay, self.log, self.i = replay, [], 0

    def __call__(self, kind, *args, device=None):
        from pointcept_amd.masked_scene_contrast import MaskedSceneContrast

        if self.replay is None:
            v = MaskedSceneContrast.draw(None, kind, *args, device=device)
            self.log.append((kind, v.cpu() if torch.is_tensor(v) else v))
            return v
        kind_was, v = self.replay[self.i]
        self.i += 1
        assert kind_was == kind
        return v.to(device) if torch.is_tensor(v) and device is not None else v


def _model_run(model, batch, rec):
    model.draw = rec
    model.zero_grad(set_to_none=True)
    out = model(dict(batch))
    out["loss"].backward()
    return {k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_kernel_path_against_torch_path(monkeypatch):
    """one process, the same draws: identical masks and match_index.  Both legs run the same backbone kernels on the same inputs,
    so the features are equal and the reconstruction losses with them; nce_loss may differ by the InfoNCE tolerance on each side
    -- 4 fp32 ulps of max(|loss|, 1 / nce_t) for the kernel (the floor of test_nce_against_float64) plus as much for the torch
    expression -- and pos_sim / neg_sim by the same 8 ulps of 1.  Gradients (mask_token, heads, every parameter): 1e-3 of the
    largest element, the fp32 bound of the SpUNet golden test's full-gradient comparison."""
    from pointcept_amd import config
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrast

    torch.manual_seed(0)
    model = MaskedSceneContrast(**TINY_CFG).to(dev())
    batch = two_views([3000, 2500], 60, dev())
    monkeypatch.setattr(config, "MSC_KERNELS", False)
    rec = Recorder()
    out_t, grad_t = _model_run(model, batch, rec)
    ints_t = dict(model.last)
    monkeypatch.setattr(config, "MSC_KERNELS", True)
    out_k, grad_k = _model_run(model, batch, Recorder(rec.log))
    for k in ("view1_point_mask", "view2_point_mask", "match_index"):
        assert torch.equal(ints_t[k], model.last[k]), k
    assert ints_t["match_index"].shape[0] == TINY_CFG["matching_max_pair"]
    assert set(out_k) == set(GOLD_LOSSES) == set(out_t)
    for k in out_k:
        print(k, float(out_k[k]), float(out_t[k]))
    t = TINY_CFG["nce_t"]
    nce_bound = 2 * NCE_FLOOR_ULPS * ULP * max(abs(float(out_t["nce_loss"])), 1.0 / t)
    assert abs(float(out_k["nce_loss"]) - float(out_t["nce_loss"])) <= nce_bound
    for k in ("pos_sim", "neg_sim"):
        assert abs(float(out_k[k]) - float(out_t[k])) <= 2 * NCE_FLOOR_ULPS * ULP
    for k in ("color_loss", "normal_loss"):
        assert float(out_k[k]) == float(out_t[k]), k
    assert abs(float(out_k["loss"]) - float(out_t["loss"])) <= nce_bound + ULP * abs(float(out_t["loss"]))
    assert set(grad_k) == set(n for n, _ in model.named_parameters()) == set(grad_t)
    for k in grad_k:
        assert _rel(grad_k[k], grad_t[k]) < 1e-3, (k, _rel(grad_k[k], grad_t[k]))


def test_port_matches_reference_golden():
    check_port_against_golden(dev())


def test_state_dict_keys_are_the_references():
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrast

    assert list(MaskedSceneContrast(**GOLD_CFG).state_dict().keys()) == [str(k) for k in golden()["keys"]]


def test_registered_only_when_named():
    from pointcept_amd import compat

    assert "MSC-v1m1" not in compat.MODEL_CLASSES and compat.OPT_IN_MODEL_CLASSES["MSC-v1m1"] == ("masked_scene_contrast", "MaskedSceneContrast")


def test_scannet_config_step():
    """fp32, 2 scenes per view x 100 000 points, SpUNet base channels: finite losses, a gradient for every parameter, no ATen mm /
    unique and no library GEMM inside the three stages, at most three host reads (device-to-host copies in the profiler trace)
    across masks and matching"""
    from torch.profiler import ProfilerActivity, profile

    from pointcept_amd.masked_scene_contrast import MaskedSceneContrast

    torch.manual_seed(0)
    model = MaskedSceneContrast(backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                                              layers=(2, 3, 4, 6, 2, 2, 2, 2)), backbone_in_channels=6, backbone_out_channels=96).to(dev())
    batch = two_views([100000, 100000], 70, dev())
    out = model(dict(batch))
    out["loss"].backward()
    for k, v in out.items():
        assert bool(torch.isfinite(v)), k
    assert all(p.grad is not None for p in model.parameters())
    f1 = torch.randn(200000, 96, device=dev(), requires_grad=True)
    f2 = torch.randn(200000, 96, device=dev(), requires_grad=True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as reads:
        model.generate_cross_masks(batch["view1_origin_coord"], batch["view1_offset"].int(), batch["view2_origin_coord"], batch["view2_offset"].int())
        model.match_contrastive_pair(batch["view1_origin_coord"], batch["view1_offset"].int(), batch["view2_origin_coord"],
                                     batch["view2_offset"].int(), 8, 0.03)
        torch.cuda.synchronize()
    d2h = [e.name for e in reads.events() if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name]
    kernels = [e.name for e in reads.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert any("msc_match_kernel" in k for k in kernels), "the profiler captured no kernel of the matching"
    assert 1 <= len(d2h) <= 3, d2h            # >= 1: the check does see copies
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        m1, m2 = model.generate_cross_masks(batch["view1_origin_coord"], batch["view1_offset"].int(), batch["view2_origin_coord"], batch["view2_offset"].int())
        mi = model.match_contrastive_pair(batch["view1_origin_coord"], batch["view1_offset"].int(), batch["view2_origin_coord"],
                                          batch["view2_offset"].int(), 8, 0.03)
        loss, _, _ = model.compute_contrastive_loss(f1, batch["view1_offset"], f2, batch["view2_offset"], mi)
        loss.backward()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [n for n in names if n in ("aten::mm", "aten::unique", "aten::_unique2", "aten::unique_dim", "aten::matmul", "aten::addmm")
           or "Cijk" in n or "gemm" in n.lower()]
    assert not bad, bad
    assert mi.shape[0] == 8192
