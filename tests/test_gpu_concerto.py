"""-m gpu: Concerto-v1m1 (csrc/concerto.hip, pointcept_amd/concerto.py).  The check_* bodies take a device; tests/test_concerto_cpu.py
runs them on the host emulation at their small shapes.

Every kernel against a float64 evaluation of its torch twin (functional.concerto_*_torch) on the values the kernel reads -- the upcast
values for 16-bit inputs.  Tolerance: the rule of tests/test_gpu_sonata.py::bounds, set before any kernel figure was seen: the error
of the fp32 twin against the float64 twin is measured in the test; the kernel may have 4 x that error, never less than FLOOR_ULPS = 4
fp32 ulps of the scale of the quantity compared, plus half an ulp of the output dtype where the output is 16-bit.  Scales: the loss
10 * mean(1 - cos) -> max(|loss|, 10) (terms up to 20); a row of dy or of a patch mean -> its largest float64 element, ROW BY ROW (the
clamp-branch rows of dy are 10^6 times larger than the others: one scale for the tensor would check nothing on the ordinary rows).
The pooled correspondence: bit-equal to the twin at the first level (integer inputs: exact sums, one correctly rounded division),
1e-5 against float64 at the second (the fp32 spacing at coordinates below 64 is 3.8e-6).  Every figure is printed before it is asserted.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pointcept_amd import functional as PF  # noqa: E402
from pointcept_amd import ops  # noqa: E402

FLOOR_ULPS = 4
ULP = 2.0 ** -23
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def dev():
    return torch.device("cuda")


def row_bound(ref, tor, out_dtype):
    """per row: (torch fp32 error, bound, scale) of a [rows, width] quantity"""
    ref = ref.reshape(ref.shape[0], -1)
    scale = ref.abs().amax(1)
    e_torch = (tor.double().reshape(ref.shape) - ref).abs().amax(1)
    return e_torch, torch.maximum(4 * e_torch, FLOOR_ULPS * ULP * scale) + HALF_ULP[out_dtype] * scale, scale


def assert_rows(tag, got, ref, tor, out_dtype):
    e_torch, bound, scale = row_bound(ref, tor, out_dtype)
    e_kernel = (got.double().reshape(ref.shape[0], -1) - ref.reshape(ref.shape[0], -1)).abs().amax(1)
    worst = int(torch.argmax(e_kernel / bound.clamp(min=1e-300))) if ref.shape[0] else 0
    if ref.shape[0]:
        print(f"{tag}: worst row {worst}: kernel err {float(e_kernel[worst]):.3e}  torch fp32 err {float(e_torch[worst]):.3e}  "
              f"bound {float(bound[worst]):.3e}  scale {float(scale[worst]):.3e};  max kernel err {float(e_kernel.max()):.3e}")
    assert bool((e_kernel <= bound).all()), (tag, worst, float(e_kernel[worst]), float(bound[worst]))


# ---------------------------------------------------------------------------------------------------------------- pooled correspondence
SIZES = (1, 2, 8, 33)


def clusters(m, seed):
    """(perm = the points sorted by cluster, idx_ptr [m + 1], n): clusters of 1, 2, 8 and 33 members, the points shuffled"""
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor([SIZES[i % 4] for i in range(m)])
    inverse = torch.repeat_interleave(torch.arange(m), counts)
    inverse = inverse[torch.randperm(inverse.numel(), generator=g)]
    perm = torch.argsort(inverse, stable=True)
    return perm, torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)]), int(counts.sum())


def corr_case(m, v, dtype, seed=0):
    perm, idx_ptr, n = clusters(m, seed + m)
    g = torch.Generator().manual_seed(seed * 31 + m * 7 + v)
    corr = torch.randint(0, 40, (n, v, 2), generator=g)
    corr[torch.rand(n, v, generator=g) < 0.3] = -1
    if v:
        corr[perm[idx_ptr[m - 1]:idx_ptr[m]], 0] = -1                 # a cluster without a valid member for image 0
        corr[perm[0], v - 1] = torch.tensor([-1, 5])                  # a half-valid pair: adds 5, is not counted
    return corr.to(dtype), perm, idx_ptr


def check_pool_corr(device, m, v, dtype):
    corr, perm, idx_ptr = (t.to(device) for t in corr_case(m, v, dtype))
    got = PF.concerto_pool_corr(corr, perm, idx_ptr, use_kernels=True)
    twin = PF.concerto_pool_corr_torch(corr, perm, idx_ptr)
    assert got.shape == (m, v, 2) and got.dtype == torch.float32
    assert torch.equal(got, twin.float()), float((got - twin).abs().max())
    if v == 0:
        return
    assert bool((got[m - 1, 0] == -1).all())
    members = corr[perm[idx_ptr[0]:idx_ptr[1]], v - 1].double()
    full = (members != -1).all(1)
    want = members.clamp(min=0).sum(0) / full.sum() if bool(full.any()) else torch.full((2,), -1.0, dtype=torch.float64, device=device)
    assert torch.allclose(got[0, v - 1].double(), want, rtol=1e-7, atol=0)      # the half-valid pair's 5 is in the sum, not in the count
    # second level, fed the first's output
    m2 = -(-m // 3)
    perm2, idx_ptr2 = torch.arange(m, device=device), torch.tensor([min(3 * i, m) for i in range(m2 + 1)], device=device)
    got2 = PF.concerto_pool_corr(got, perm2, idx_ptr2, use_kernels=True)
    ref2 = PF.concerto_pool_corr_torch(got.double(), perm2, idx_ptr2)
    err = float((got2.double() - ref2).abs().max())
    print(f"pool_corr M={m} V={v} {str(dtype)[6:]}: second level err {err:.3e} (bound 1e-5)")
    assert err <= 1e-5 and torch.equal(got2 == -1, ref2 == -1)


POOL_CASES = [(m, v, d) for m in (1, 255, 257) for v in (0, 1, 3, 5) for d in (torch.int64,)] + \
             [(257, 3, torch.int32), (257, 3, torch.float32), (255, 5, torch.float32), (1, 1, torch.int32)]


@pytest.mark.parametrize("m,v,dtype", POOL_CASES)
def test_pool_corr(m, v, dtype):
    check_pool_corr(dev(), m, v, dtype)


# ---------------------------------------------------------------------------------------------------------------- patch binning
PH, PW = 6, 5


def pairs_case(ns, v, img_nums, seed=0, valid=0.6, one_patch=False):
    """pooled correspondence [n, v, 2] fp32 of n = ns + 7 points of which rows = 3 .. ns + 2 are selected, scene per selected row
    (ascending), img_offset, img_num; the views at or beyond a scene's img_num hold -1, as the collate pads them"""
    g = torch.Generator().manual_seed(seed * 101 + ns + v)
    n = ns + 7
    corr = torch.rand(n, v, 2, generator=g) * torch.tensor([PH, PW]) * 0.999
    if one_patch:
        corr = torch.rand(n, v, 2, generator=g) * 0.9 + torch.tensor([2.0, 3.0])
    corr[torch.rand(n, v, generator=g) >= valid] = -1
    rows = torch.arange(3, 3 + ns)
    img_num = torch.tensor(img_nums)
    scene = torch.sort(torch.randint(0, len(img_nums), (ns,), generator=g)).values
    if one_patch:
        scene = torch.zeros(ns, dtype=torch.int64)
        corr[:, 1:] = -1
    pad =torch.arange(v)[None] >= img_num[scene][:, None]
    sel = corr[rows]
    sel[pad] = -1
    corr[rows] = sel
    return corr.float(), rows, scene, torch.cumsum(img_num, 0) - img_num, img_num


def reference_keys(corr, rows, scene, img_offset):
    """valid_index and feature_index as concerto_v1m1_base.py:786-823 forms them"""
    sel = corr[rows]
    mask = torch.any(sel != -1, dim=2)
    pi, vi = torch.where(mask)
    fi = torch.cat([img_offset[scene[pi]].unsqueeze(-1), vi.unsqueeze(-1), sel[pi, vi]], dim=-1).long()
    return pi, vi, fi[:, 0] * PH * PW + fi[:, 1] * PH * PW + fi[:, 2] * PW + fi[:, 3]


def same_pairs(a, b):
    return (torch.equal(a.patch_ids, b.patch_ids) and torch.equal(a.indptr, b.indptr) and torch.equal(a.perm, b.perm)
            and torch.equal(a.pair_patch, b.pair_patch))


def check_patch_pairs(device, ns, v, img_nums, valid=0.6, one_patch=False):
    corr, rows, scene, img_offset, img_num = (t.to(device) for t in pairs_case(ns, v, img_nums, valid=valid, one_patch=one_patch))
    total = int(img_num.sum())
    got = PF.concerto_patch_pairs(corr, scene, img_offset, img_num, total, PH, PW, rows=rows, use_kernels=True)
    twin = PF.concerto_patch_pairs_torch(corr, scene, img_offset, img_num, total, PH, PW, rows=rows)
    pi, vi, keys = reference_keys(corr, rows, scene, img_offset)
    ids, counts = torch.unique(keys, return_counts=True)
    assert torch.equal(got.patch_ids, ids) and torch.equal(got.indptr[1:] - got.indptr[:-1], counts) and int(got.indptr[0]) == 0
    assert got.num_patches == ids.numel() and got.num_pairs == keys.numel()
    assert same_pairs(got, twin)
    # inside a patch: ascending point row, then view
    order = torch.argsort(keys * (ns * max(v, 1)) + pi * max(v, 1) + vi)
    assert torch.equal(got.perm, rows[pi[order]])
    assert torch.equal(got.pair_patch >= 0, torch.zeros_like(got.pair_patch, dtype=torch.bool).index_put((pi, vi), torch.tensor(True, device=device)))
    return got


@pytest.mark.parametrize("ns,v,img_nums", [(1, 1, (1,)), (40, 3, (3, 2)), (300, 3, (3, 1, 2)), (257, 5, (5, 4)), (10, 0, (0, 0))])
def test_patch_pairs(ns, v, img_nums):
    check_patch_pairs(dev(), ns, v, img_nums)


def check_patch_pairs_edge_cases(device):
    none = check_patch_pairs(device, 30, 3, (3, 3), valid=-1.0)
    assert none.num_patches == 0 and none.num_pairs == 0 and none.indptr.tolist() == [0]
    one = check_patch_pairs(device, 50, 3, (3,), valid=2.0, one_patch=True)
    assert one.num_patches == 1 and one.num_pairs == 50 and int(one.patch_ids[0]) == 2 * PW + 3
    # pairs outside their image or beyond their scene's images are left out and leave every other output unchanged
    corr, rows, scene, img_offset, img_num = (t.to(device) for t in pairs_case(60, 3, (3, 2)))
    total = int(img_num.sum())
    clean = corr.clone()
    bad = corr.clone()
    spots = [(rows[0], 0, (PH + 0.5, 1.0)), (rows[5], 1, (2.0, PW + 0.0)), (rows[9], 0, (-3.2, 1.0)), (rows[11], 1, (1.0, float("nan"))),
             (rows[20], 0, (-1.0, 2.0)), (rows[-1], 2, (1.0, 1.0))]          # the last: view 2 of a scene with two images
    assert int(scene[-1]) == 1 and int(img_num[1]) == 2
    for p, view, rc in spots:
        bad[p, view] = torch.tensor(rc, device=device)
        clean[p, view] = -1
    bad[rows[30], 0] = torch.tensor([-0.5, 1.5], device=device)              # trunc(-0.5) = 0: INSIDE, as .long() has it
    clean[rows[30], 0] = torch.tensor([0.0, 1.5], device=device)
    for path in (True, False):
        a = PF.concerto_patch_pairs(bad, scene, img_offset, img_num, total, PH, PW, rows=rows, use_kernels=path)
        b = PF.concerto_patch_pairs(clean, scene, img_offset, img_num, total, PH, PW, rows=rows, use_kernels=path)
        assert same_pairs(a, b) and int(a.patch_ids.max()) < total * PH * PW and int(a.patch_ids.min()) >= 0
    assert same_pairs(a, PF.concerto_patch_pairs(bad, scene, img_offset, img_num, total, PH, PW, rows=rows, use_kernels=True))


def test_patch_pairs_edge_cases():
    check_patch_pairs_edge_cases(dev())


# ---------------------------------------------------------------------------------------------------------------- patch means
def mean_case(device, c, dtype, seed=0):
    """60 selected points of 67, three views; point rows[4] falls into three different patches"""
    corr, rows, scene, img_offset, img_num = pairs_case(60, 3, (3, 3), seed=seed, valid=0.7)
    corr[rows[4]] = torch.tensor([[0.5, 0.5], [1.5, 2.5], [3.5, 4.5]])
    args = [t.to(device) for t in (corr, scene, img_offset, img_num)]
    pairs = PF.concerto_patch_pairs_torch(args[0], args[1], args[2], args[3], 6, PH, PW, rows=rows.to(device))
    g = torch.Generator().manual_seed(seed + c)
    feat = torch.randn(corr.shape[0], c, generator=g).to(dtype).to(device)
    grad = torch.randn(pairs.num_patches, c, generator=g).to(dtype).to(device)
    return pairs, feat, grad


def _mean_run(fn, feat, pairs, grad, **kw):
    f = feat.clone().requires_grad_(True)
    out = fn(f, pairs, **kw)
    out.backward(grad.to(out.dtype))
    return out.detach(), f.grad


def check_patch_mean(device, c, dtype):
    pairs, feat, grad = mean_case(device, c, dtype)
    pp = pairs.pair_patch
    assert bool(((pp >= 0).sum(1) == 3).any())                                   # a point in V different patches
    assert pairs.num_patches > 3 and pairs.num_pairs > pairs.num_patches
    up = lambda t, d: t.float().to(d)
    ref = _mean_run(PF.concerto_patch_mean_torch, up(feat, torch.float64), pairs, up(grad, torch.float64))
    tor = _mean_run(PF.concerto_patch_mean_torch, up(feat, torch.float32), pairs, up(grad, torch.float32))
    got = _mean_run(PF.concerto_patch_mean, feat, pairs, grad, use_kernels=True)
    assert got[0].dtype == dtype and got[1].dtype == dtype and got[1].shape == feat.shape
    assert_rows(f"patch_mean C={c} {str(dtype)[6:]} fwd", got[0], ref[0], tor[0], dtype)
    assert_rows(f"patch_mean C={c} {str(dtype)[6:]} bwd", got[1], ref[1], tor[1], dtype)
    named = torch.zeros(feat.shape[0], dtype=torch.bool, device=device)
    named[pairs.perm] = True
    assert not bool(got[1][~named].any())                                        # rows without a pair: exactly zero
    again = _mean_run(PF.concerto_patch_mean, feat, pairs, grad, use_kernels=True)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def check_same_patch_twice(device):
    """A point that reaches one patch through two views counts twice in the mean and receives the patch's gradient twice.  The
    binning itself cannot produce this -- the key holds the view, so two views of a point are two images -- hence the pair lists
    are written by hand: patch 0 holds point 0 twice and point 1 once."""
    corr = torch.tensor([[[1.2, 1.2], [1.7, 1.4]], [[1.1, 1.9], [-1.0, -1.0]]], device=device)
    z = torch.zeros(2, dtype=torch.int64, device=device)
    args = (corr, z, torch.tensor([0], device=device), torch.tensor([2], device=device), 2, PH, PW)
    for path in (True, False):
        pairs = PF.concerto_patch_pairs(*args, use_kernels=path)
        assert pairs.patch_ids.tolist() == [1 * PW + 1, PH * PW + 1 * PW + 1] and pairs.indptr.tolist() == [0, 2, 3]
    feat =torch.tensor([[1.0, 2.0, 3.0], [5.0, 6.0, 7.0]], device=device)
    pairs = ops.ConcertoPairs(torch.tensor([7], device=device), torch.tensor([0, 3], device=device), torch.tensor([0, 0, 1], device=device),
                              torch.tensor([[0, 0], [0, -1]], device=device), None)
    got = _mean_run(PF.concerto_patch_mean, feat, pairs, torch.ones(1, 3, device=device), use_kernels=True)
    assert torch.allclose(got[0], (2 * feat[0] + feat[1])[None] / 3) and torch.allclose(got[1], torch.tensor([[2 / 3] * 3, [1 / 3] * 3], device=device))


@pytest.mark.parametrize("c,dtype", [(3, torch.float32), (96, torch.float32), (1184, torch.float32), (96, torch.bfloat16), (1184, torch.float16)])
def test_patch_mean(c, dtype):
    check_patch_mean(dev(), c, dtype)


def test_same_patch_through_two_views():
    check_same_patch_twice(dev())


# ---------------------------------------------------------------------------------------------------------------- centred cosine
DTYPE_PAIRS = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32)]
_ALIGN = {}


def align_case(device, u, d, shift, xd, yd, seed=0):
    """(feature2d [2u + 3, d] with NaN in every row no id names, ids [u], y [u, d]); row 0 of x and the last row of y are constant
    (zero without the shift): their centred norm is below eps -- the clamp branch"""
    g = torch.Generator().manual_seed(seed * 13 + u * 7 + d)
    nx = 2 * u + 3
    ids = torch.sort(torch.randperm(nx, generator=g)[:u]).values
    x = torch.full((nx, d), float("nan"))
    x[ids] = torch.randn(u, d, generator=g) * 1.5 + 0.3
    y = torch.randn(u, d, generator=g) * 0.7 - 0.2
    x[ids[0]] = 0.75 if shift else 0.0
    y[u - 1] = -1.25 if shift else 0.0
    return x.to(xd).to(device), ids.to(device), y.to(yd).to(device)


def _align_run(fn, x, ids, y, shift, **kw):
    yy = y.clone().requires_grad_(True)
    loss = fn(x, ids, yy, shift, 1e-6, **kw)
    loss.backward()
    return loss.detach(), yy.grad


def align_references(device, u, d, shift, xd, yd):
    key = (str(device), u, d, shift, xd, yd)
    if key not in _ALIGN:
        x, ids, y = align_case(device, u, d, shift, xd, yd)
        ref = _align_run(PF.concerto_align_loss_torch, x.float().double(), ids, y.float().double(), shift)
        tor = _align_run(PF.concerto_align_loss_torch, x.float(), ids, y.float(), shift)
        _ALIGN[key] = ((x, ids, y), ref, tor)
    return _ALIGN[key]


def check_align(device, u, d, shift, xd, yd):
    (x, ids, y), ref, tor = align_references(device, u, d, shift, xd, yd)
    got = _align_run(PF.concerto_align_loss, x, ids, y, shift, use_kernels=True)
    tag = f"align U={u} D={d} shift={int(shift)} {str(xd)[6:]}/{str(yd)[6:]}"
    assert got[0].dtype == torch.float32 and got[0].dim() == 0 and got[1].dtype == yd and got[1].shape == y.shape
    assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[1]).all())        # the NaN rows of feature2d are never read
    scale = max(abs(float(ref[0])), 10.0)
    e_torch, e_kernel = abs(float(tor[0]) - float(ref[0])), abs(float(got[0]) - float(ref[0]))
    bound = max(4 * e_torch, FLOOR_ULPS * ULP * scale)
    print(f"{tag} loss: kernel err {e_kernel:.3e}  torch fp32 err {e_torch:.3e}  bound {bound:.3e}  loss {float(ref[0]):.6f}")
    assert e_kernel <= bound, (tag, e_kernel, e_torch, bound)
    assert_rows(tag + " dy", got[1], ref[1], tor[1], yd)
    # the clamp branch: a constant x row gives cos = 0 and no gradient; a constant y row gives the clamped gradient a / eps
    assert not bool(got[1][0].any()) or u == 1
    if u > 1:
        assert float(got[1][u - 1].float().abs().max()) > 1e3 * float(got[1][1 if u > 2 else 0].float().abs().max())
    again = _align_run(PF.concerto_align_loss, x, ids, y, shift, use_kernels=True)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


ALIGN_CASES = [(u, d, s, xd, yd) for u in (1, 63, 65, 300) for d in (6, 100, 384, 1024, 1536) for s in (True, False) for xd, yd in DTYPE_PAIRS]


@pytest.mark.parametrize("u,d,shift,xd,yd", ALIGN_CASES)
def test_align_loss(u, d, shift, xd, yd):
    check_align(dev(), u, d, shift, xd, yd)


def check_align_special(device):
    """no gradient asked: no dy; no patches: the twin's value (NaN) without a launch; more channels than a wave holds: the twin"""
    x, ids, y = align_case(device, 5, 100, True, torch.float32, torch.float32)
    with torch.no_grad():
        a = PF.concerto_align_loss(x, ids, y, True, use_kernels=True)
    assert abs(float(a) - float(PF.concerto_align_loss_torch(x, ids, y, True))) < 1e-5
    e = PF.concerto_align_loss(x, ids[:0], y[:0].clone().requires_grad_(True), True, use_kernels=True)
    assert bool(torch.isnan(e)) and e.requires_grad
    assert ops.concerto_align_supported(2048) and not ops.concerto_align_supported(2049)
    wide = torch.randn(3, 2056, device=device)
    b = PF.concerto_align_loss(wide, torch.arange(3, device=device), wide.flip(0).clone(), True, use_kernels=True)
    assert torch.equal(b, PF.concerto_align_loss_torch(wide, torch.arange(3, device=device), wide.flip(0).clone(), True))
    # a scaled upstream gradient scales dy
    yy = y.clone().requires_grad_(True)
    (PF.concerto_align_loss(x, ids, yy, True, use_kernels=True) * 0.25).backward()
    one = _align_run(PF.concerto_align_loss, x, ids, y, True, use_kernels=True)[1]
    assert torch.allclose(yy.grad, one * 0.25, rtol=1e-6, atol=0)


def test_align_special_cases():
    check_align_special(dev())


# ---------------------------------------------------------------------------------------------------------------- model
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "concerto_tiny.npz"))


import test_gpu_sonata as S  # noqa: E402

GOLD_BACKBONE = dict(S.GOLD_BACKBONE)
GOLD_PATCH_H, GOLD_PATCH_W, GOLD_CHANNELS = 6, 5, 24
GOLD_CFG = dict(image_weight_name="stand-in", image_weight_path=None, backbone=GOLD_BACKBONE, head_in_channels=256 + 512,
                backbone_out_channels=128 + 256 + 512, embedding_channels=GOLD_CHANNELS, patch_w=GOLD_PATCH_W, patch_h=GOLD_PATCH_H,
                head_hidden_channels=32, head_embed_channels=16, head_num_prototypes=64, enc2d_head_in_channels=GOLD_CHANNELS,
                enc2d_head_hidden_channels=32, enc2d_head_embed_channels=16, enc2d_head_num_prototypes=16,
                teacher_custom=dict(drop_path=0.0), num_global_view=2, num_local_view=4, mask_size_start=0.1, mask_ratio_start=0.3,
                mask_jitter=0.0008, teacher_temp_start=0.04, student_temp=0.1, mask_loss_weight=2 / 10, roll_mask_loss_weight=2 / 10,
                unmask_loss_weight=4 / 10, enc2d_loss_weight=2 / 10, match_max_r=0.12, up_cast_level=1, enc2d_upcast_level=2,
                enc2d_cos_shift=True, sonata_model_type="online")          # = make_golden_concerto.py CFG
GOLD_LOSSES = ("mask_loss", "roll_mask_loss", "unmask_loss", "enc2d_loss", "loss")
GOLD_INTS = ("global_mask", "global_cluster", "mask_match_index", "roll_mask_match_index", "unmask_match_index")


class Registry:
    """what compat.register_models needs of the reference's MODELS"""

    def __init__(self):
        self.modules = {}

    def register_module(self, name, force=False, module=None):
        self.modules[name] = module


def concerto_class():
    from pointcept_amd import compat

    reg = Registry()
    assert compat.register_models(reg, names=["Concerto-v1m1"]) == ["Concerto-v1m1"] and list(reg.modules) == ["Concerto-v1m1"]
    return reg.modules["Concerto-v1m1"]


def golden_batch(g, img_nums=None):
    from pointcept_amd import synthetic

    nums = [int(v) for v in g["img_nums"]] if img_nums is None else img_nums
    b = synthetic.multi_view_image_batch([int(s) for s in g["scene_seeds"]], int(g["view_sizes"][0]), int(g["view_sizes"][1]), nums,
                                         GOLD_PATCH_H, GOLD_PATCH_W)
    if img_nums is None:
        assert sorted(b) == [str(k) for k in g["input_keys"]]
        assert np.array_equal(np.asarray([float(b[k].astype(np.float64).sum()) for k in sorted(b)]), g["input_checksum"])
    return b


def golden_model(g, device, **over):
    from pointcept_amd import synthetic

    torch.manual_seed(0)
    model = concerto_class()(**{**GOLD_CFG, "backbone": dict(GOLD_BACKBONE), **over},
                             enc2d_model=synthetic.stand_in_image_encoder(GOLD_PATCH_H, GOLD_PATCH_W, GOLD_CHANNELS))
    if not over:
        model.load_state_dict(S.golden_state(g, model))
    return model.to(device).train()


def check_state_dict_keys():
    g = golden()
    model = golden_model(g, torch.device("cpu"))
    keys = list(model.state_dict().keys())
    assert keys == [str(k) for k in g["keys"]]
    for prefix in ("enc2d_model.", "patch_proj.", "enc2d_head_student.mlp.", "enc2d_head_student.prototype.", "enc2d_head_teacher.prototype.",
                   "student.backbone.", "student.mask_head.", "student.unmask_head.", "teacher.unmask_head."):
        assert any(k.startswith(prefix) for k in keys), prefix
    assert not any(k.startswith("enc2d_head_teacher.mlp.") for k in keys)
    frozen = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert all(k.startswith(("teacher.", "enc2d_model.", "enc2d_head_teacher.")) or k.endswith("original0") for k in frozen)
    assert all(not p.requires_grad for k, p in model.named_parameters() if k.startswith(("teacher.", "enc2d_model.")))
    # only the 2D-3D weight positive: the extra unmask_head pair (:260-268)
    only = golden_model(g, torch.device("cpu"), mask_loss_weight=0, roll_mask_loss_weight=0, unmask_loss_weight=0)
    assert sorted(only.student.keys()) == ["backbone", "unmask_head"] == sorted(only.teacher.keys())
    # the reference's defaults
    import inspect

    sig = inspect.signature(concerto_class().__init__).parameters
    assert [sig[k].default for k in ("mask_loss_weight", "roll_mask_loss_weight", "unmask_loss_weight", "enc2d_loss_weight")] == [0.2, 0.2, 0.4, 0.2]
    assert sig["enc2d_upcast_level"].default == 4 and sig["sonata_model_type"].default == "offline" and sig["enc2d_model"].default is None


def check_port_against_golden(device, force_kernels=None):
    """the port, with the reference run's draws replayed, against the reference file's run: integers exactly, the first pooled level
    exactly and the second at 1e-5, the patch ids exactly, every loss at 1e-4 relative, gradient norms at rtol 2e-2 where they are not
    rounding noise (the tolerances of the Sonata golden test), the gradient of patch_proj at 2e-3 of its largest element"""
    from pointcept_amd import synthetic

    g = golden()
    model = golden_model(g, device)
    model.force_kernels = force_kernels
    batch = synthetic.to_torch(golden_batch(g), device)
    draws = [("patch_perm", torch.from_numpy(g["draw_patch_perm"])), ("jitter", torch.from_numpy(g["draw_jitter"]))]
    out, grads = S._model_run(model, batch, S.Recorder(draws), int(g["order_seed"]))
    assert model.draw.i == 2
    for k in GOLD_INTS:
        assert np.array_equal(model.last[k].cpu().numpy(), g[k]), k
    levels = [t.cpu().numpy() for t in model.last["pooled_correspondence"]]
    assert len(levels) == 2
    assert np.array_equal(levels[0], g["pooled_correspondence_0"])
    err = float(np.abs(levels[1].astype(np.float64) - g["pooled_correspondence_1"]).max())
    print(f"golden pooled correspondence, second level: err {err:.3e}")
    assert err <= 1e-5 and np.array_equal(levels[1] == -1, g["pooled_correspondence_1"] == -1)
    assert np.array_equal(model.last["patch_ids"].cpu().numpy(), g["patch_ids"]) and model.last["num_pairs"] == int(g["num_pairs"])
    assert g["patch_ids"].shape[0] > 0 and int(g["num_pairs"]) > g["patch_ids"].shape[0]
    assert set(out) == set(GOLD_LOSSES)
    for k in GOLD_LOSSES:
        ref = float(g["out/" + k])
        print(f"golden {k}: port {float(out[k]):.8g} reference {ref:.8g}")
    for k in GOLD_LOSSES:
        assert abs(float(out[k]) - float(g["out/" + k])) <= 1e-4 * abs(float(g["out/" + k])), k
    names = [str(k) for k in g["param_names"]]
    assert names == [k for k, _ in model.named_parameters() if k.startswith("student.")]
    student = {k: v for k, v in grads.items() if k.startswith("student.")}
    assert set(student) == set(n for n, h in zip(names, g["has_grad"]) if h)
    assert not any(k.startswith(("teacher.", "enc2d_model.", "enc2d_head_")) for k in grads)
    norms = np.asarray([float(grads[k].double().norm()) if h else 0.0 for k, h in zip(names, g["has_grad"])])
    big = g["grad_norms"] > 1e-4 * g["grad_norms"].max()
    assert np.allclose(norms[big], g["grad_norms"][big], rtol=2e-2), np.abs(norms[big] / g["grad_norms"][big] - 1).max()
    for k in ("patch_proj.weight", "patch_proj.bias"):
        rel = S._rel(grads[k], g["grad/" + k])
        print(f"golden grad {k}: rel {rel:.3e}")
        assert rel < 2e-3, (k, rel)
    return model


def check_zero_image_batch(device):
    """no image in the batch: enc2d_loss is the weighted mean of the other losses (:854-866)"""
    from pointcept_amd import synthetic

    g = golden()
    model = golden_model(g, device)
    batch = synthetic.to_torch(golden_batch(g, [0, 0]), device)
    assert batch["global_correspondence"].shape[1:] == (0, 2) and batch["images"].shape[0] == 0
    out, grads = S._model_run(model, batch, S.Recorder(), 0)
    w = (0.2, 0.2, 0.4)
    want = sum(float(out[k]) * wk for k, wk in zip(GOLD_LOSSES[:3], w)) / sum(w)
    assert abs(float(out["enc2d_loss"]) - want) <= 1e-6 * abs(want)
    assert abs(float(out["loss"]) - (want * sum(w) + 0.2 * want)) <= 1e-6 * abs(want)
    assert model.last["total_img_num"] == 0 and [tuple(t.shape[1:]) for t in model.last["pooled_correspondence"]] == [(0, 2)] * 2
    assert "patch_proj.weight" not in grads and any(k.startswith("student.backbone.") for k in grads)


def check_return_point(device):
    from pointcept_amd import synthetic

    g = golden()
    model = golden_model(g, device).eval()
    b = synthetic.to_torch(golden_batch(g), device)
    with torch.no_grad():
        point = model(dict(feat=b["global_feat"], coord=b["global_coord"], origin_coord=b["global_origin_coord"], offset=b["global_offset"],
                           grid_size=b["grid_size"][0]), return_point=True)["point"]
    assert point.feat.shape == (point.coord.shape[0], GOLD_CFG["head_in_channels"]) and "pooling_parent" in point.keys()
    assert bool(torch.isfinite(point.feat).all())


def check_after_step(device):
    """online: every teacher parameter moves to m t + (1 - m) s; the prototypes of enc2d_head_teacher are copied from the student's"""
    g = golden()
    model = golden_model(g, device)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    with torch.no_grad():
        model.enc2d_head_student.prototype.parametrizations.weight.original1.add_(0.5)
    model.momentum = 0.9
    model.after_step()
    for k, p in model.teacher.named_parameters():
        want = 0.9 * before["teacher." + k] + 0.1 * before["student." + k]
        assert torch.allclose(p, want, rtol=1e-6, atol=1e-7), k
    assert torch.equal(model.enc2d_head_teacher.prototype.parametrizations.weight.original1,
                       model.enc2d_head_student.prototype.parametrizations.weight.original1)
    assert not any(p.requires_grad for p in model.teacher.parameters())
    model.sonata_model_type = "offline"                                   # the loaded teacher backbone stays; the heads still move
    frozen = {k: p.detach().clone() for k, p in model.teacher.backbone.named_parameters()}
    model.after_step()
    assert all(torch.equal(p, frozen[k]) for k, p in model.teacher.backbone.named_parameters())


def test_registered_only_when_named():
    from pointcept_amd import compat

    assert "Concerto-v1m1" not in compat.MODEL_CLASSES and compat.OPT_IN_MODEL_CLASSES["Concerto-v1m1"] == ("concerto", "Concerto")
    assert concerto_class().__name__ == "Concerto"


def test_state_dict_keys_are_the_references():
    check_state_dict_keys()


def test_port_matches_reference_golden():
    from pointcept_amd import config

    assert config.CONCERTO_KERNELS is True
    check_port_against_golden(dev())


def test_port_matches_reference_golden_on_the_torch_path(monkeypatch):
    from pointcept_amd import config

    monkeypatch.setattr(config, "CONCERTO_KERNELS", False)
    check_port_against_golden(dev())


def test_zero_image_batch_takes_the_fallback():
    check_zero_image_batch(dev())


def test_return_point():
    check_return_point(dev())


def test_after_step():
    check_after_step(dev())
