"""-m gpu: PointGroup on the engine (csrc/pg_cluster.hip, pointcept_amd.pointgroup_ops_api, pointcept_amd.point_group).

* ball query equals the Python restatement of bfs_cluster_kernel.cu:16-61 (tests/pg_oracle.py) exactly: lengths and lists, incl.
  exactly 1000 / 1001 neighbours, NaN rows, extents that grow the cell edge, an empty batch segment, n = 0, a collapsed 5000-point
  scene; at 2 x 100 000 noisy centres against the chunked brute-force torch formulation (itself checked against the restatement);
* bfs_cluster equals the restatement of bfs_cluster.cpp:53-123: offsets, seeds and sorted member sets (the collapsed scene gives one
  1000-point cluster and 4000 singletons), a cluster of exactly `threshold` points, mixed labels inside one ball;
* bit-reproducibility of the clustering and of the offset-loss gradients; the offset losses against float64 torch autograd;
* the models: the kernel path against PTC_PG_CLUSTER=0's reference expression, the reference's state-dict keys, a PG-v1m2 PT-v3m1
  eval forward, and the ScanNet v1m1 step at 2 x 100 000 points in bf16 (finite, close to fp32, no library GEMM / ATen scatter, at
  most two host reads in the eval clustering before its output copies).
The check_* bodies also run on the host emulation (tests/test_pointgroup_cpu.py)."""
import os

import numpy as np
import pytest
import torch

import pg_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def noisy_centres(sizes, seed=0, n_inst=40, spread=0.6, extent=100.0):
    """instance centres in voxel units with Gaussian noise (a trained model's centre predictions), per scene"""
    rng = np.random.default_rng(seed)
    xs, bs = [], []
    for b, n in enumerate(sizes):
        c = rng.uniform(0, extent, (n_inst, 3))
        lab = rng.integers(0, n_inst, n)
        xs.append((c[lab] + rng.normal(0, spread, (n, 3))).astype(np.float32))
        bs.append(np.full(n, b, np.int32))
    return np.concatenate(xs), np.concatenate(bs)


def offsets_of(b, n_batch):
    return np.concatenate([[0], np.cumsum(np.bincount(b, minlength=n_batch))]).astype(np.int64)


def designed_cases():
    """name -> (xyz [n,3] f32, batch [n] i32, n_batch, radius)"""
    rng = np.random.default_rng(7)
    cases = {}
    # exactly 1000 neighbours for the points of a 1000-point clump, 1001 for those of a 1001-point clump
    a = rng.uniform(0, 0.1, (1000, 3)).astype(np.float32)
    b = rng.uniform(0, 0.1, (1001, 3)).astype(np.float32) + np.float32(10)
    cases["exactly_1000_and_1001"] = (np.concatenate([a, b]), np.zeros(2001, np.int32), 1, 1.0)
    x, bb = noisy_centres([600, 500], seed=3, n_inst=8, spread=0.8, extent=10)
    x[[3, 50, 700]] = np.nan
    x[11, 1] = np.inf
    x[12, 2] = -np.inf
    cases["nan_and_inf_rows"] = (x, bb, 2, 1.5)
    x, bb = noisy_centres([700], seed=4, n_inst=10, spread=0.5, extent=10)
    x[:5] = np.float32([[1e6, 0, 0], [-1e6, 3, 3], [0, 2e7, 0], [5, 5, -3e6], [1e6 + 0.5, 0, 0]])
    cases["wild_extent_grows_cells"] = (x, bb, 1, 1.5)
    x, bb = noisy_centres([400, 300], seed=5, n_inst=6, spread=0.7, extent=8)
    bb = np.where(bb == 1, 2, bb).astype(np.int32)          # segment 1 empty
    order = np.argsort(bb, kind="stable")
    cases["empty_batch_segment"] = (x[order], bb[order], 3, 1.5)
    cases["n_zero"] = (np.zeros((0, 3), np.float32), np.zeros(0, np.int32), 1, 1.5)
    x = rng.normal(0, 0.05, (5000, 3)).astype(np.float32)
    cases["collapsed_5000"] = (x, np.zeros(5000, np.int32), 1, 1.5)
    x, bb = noisy_centres([900, 800], seed=6, n_inst=12, spread=0.9, extent=12)
    cases["boundary_radius"] = (np.round(x * 2) / 2, bb, 2, 1.0)      # many pairs exactly at d2 == r2
    return cases


# ------------------------------------------------------------------------------------------------------------------------------
# checks (device-agnostic)
# ------------------------------------------------------------------------------------------------------------------------------
def check_ball_query(device, xyz, b, n_batch, radius):
    from pointcept_amd import ops

    idx_o, sl_o = O.ballquery_batch_p(xyz, b, offsets_of(b, n_batch), radius)
    idx, sl, n_trunc = ops.pg_ball_query(torch.from_numpy(xyz).to(device), torch.from_numpy(b).to(device), n_batch, radius)
    sl = sl.cpu().numpy()
    assert np.array_equal(sl[:, 1], sl_o[:, 1]), "list lengths differ"
    assert np.array_equal(sl[:, 0], sl_o[:, 0]), "starts differ from the exclusive scan"
    assert np.array_equal(idx.cpu().numpy(), idx_o), "lists differ"
    return idx_o, sl_o, n_trunc


def check_cluster(device, label, idx, sl, threshold):
    from pointcept_amd import ops

    ref = O.bfs_cluster(label, idx, sl, threshold)
    ci, co = ops.pg_cluster(torch.from_numpy(label).to(device), torch.from_numpy(idx).to(device), torch.from_numpy(sl).to(device),
                            threshold)
    assert ci.dtype == torch.int32 and co.dtype == torch.int32 and ci.shape[1] == 2
    got = (ci.cpu().numpy(), co.cpu().numpy())
    O.assert_same_clusters(ref, got)
    return got


def check_collapsed(device):
    xyz = np.random.default_rng(1).normal(0, 0.05, (5000, 3)).astype(np.float32)
    b = np.zeros(5000, np.int32)
    idx, sl, n_trunc = check_ball_query(device, xyz, b, 1, 1.5)
    assert n_trunc == 5000 and (sl[:, 1] == 1000).all()
    ci, co = check_cluster(device, np.zeros(5000, np.int32), idx, sl, 1)
    sizes = np.diff(co)
    assert sizes[0] == 1000 and (sizes[1:] == 1).all() and len(sizes) == 4001
    ci, co = check_cluster(device, np.zeros(5000, np.int32), idx, sl, 50)
    assert np.array_equal(np.diff(co), [1000])


def check_threshold_and_mixed_labels(device):
    rng = np.random.default_rng(2)
    # three well separated clumps of 30, 29 and 31 points; threshold 30 keeps the first and the third
    xyz = np.concatenate([rng.uniform(0, 0.5, (n, 3)) + 10 * k for k, n in enumerate([30, 29, 31])]).astype(np.float32)
    perm = rng.permutation(xyz.shape[0])
    xyz = xyz[perm]
    b = np.zeros(xyz.shape[0], np.int32)
    idx, sl, _ = check_ball_query(device, xyz, b, 1, 1.0)
    _, co = check_cluster(device, np.zeros(xyz.shape[0], np.int32), idx, sl, 30)
    assert sorted(np.diff(co).tolist()) == [30, 31]
    # one ball, three labels interleaved
    xyz = rng.uniform(0, 0.5, (300, 3)).astype(np.float32)
    lab = rng.integers(0, 3, 300).astype(np.int32)
    idx, sl, _ = check_ball_query(device, xyz, np.zeros(300, np.int32), 1, 1.0)
    _, co = check_cluster(device, lab, idx, sl, 1)
    assert len(co) == 4


def check_truncated_mixed(device, n=2600, seed=3):
    """dense clumps (truncated lists) with several labels and sparse tails: the exact path with multi-point BFS levels"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.normal(0, 0.3, (n // 2, 3)), rng.normal(0, 2.0, (n - n // 2, 3))]).astype(np.float32)
    xyz = xyz[rng.permutation(n)]
    lab = (rng.random(n) < 0.15).astype(np.int32)
    idx, sl, n_trunc = check_ball_query(device, xyz, np.zeros(n, np.int32), 1, 1.2)
    assert n_trunc > 0
    for t in (1, 5):
        check_cluster(device, lab, idx, sl, t)


def check_reproducible(device, xyz, b, n_batch, radius, label, threshold):
    from pointcept_amd import ops

    x, bb = torch.from_numpy(xyz).to(device), torch.from_numpy(b).to(device)
    outs = []
    for _ in range(2):
        idx, sl, _ = ops.pg_ball_query(x, bb, n_batch, radius)
        ci, co = ops.pg_cluster(torch.from_numpy(label).to(device), idx, sl, threshold)
        outs.append([t.cpu() for t in (idx, sl, ci, co)])
    for a, c in zip(*outs):
        assert torch.equal(a, c)


def bias_inputs(device, n, dtype, seed=0, ignore_frac=0.3, zero_rows=True):
    g = torch.Generator().manual_seed(seed)
    bp = torch.randn(n, 3, generator=g)
    coord = torch.randn(n, 3, generator=g) * 2
    cen = coord + torch.randn(n, 3, generator=g)
    inst = torch.randint(0, 9, (n,), generator=g)
    inst[torch.rand(n, generator=g) < ignore_frac] = -1
    if zero_rows:
        bp[:7] = 0.0                    # |bp| = 0: the norm's subgradient
        bp[7:12] = (cen - coord)[7:12]  # bp == gt: abs' subgradient
        cen[12:17] = coord[12:17]       # gt == 0
        inst[:20] = 3
    return bp.to(device, dtype), coord.to(device), cen.to(device), inst.to(device)


def check_bias_loss(device, n, dtype, all_ignored=False):
    from pointcept_amd import functional as PF

    bp, coord, cen, inst = bias_inputs(device, n, dtype)
    if all_ignored:
        inst = torch.full_like(inst, -1)
    x = bp.detach().clone().requires_grad_(True)
    l1, cs = PF.pg_bias_loss(x, coord, cen, inst, -1)
    (l1 * 0.7 + cs * 1.3).backward()
    l1, cs = l1.detach(), cs.detach()
    r = bp.detach().double().cpu().requires_grad_(True)
    rl1, rcs = PF.pg_bias_loss_torch(r, coord.double().cpu(), cen.double().cpu(), inst.cpu(), -1)
    (rl1 * 0.7 + rcs * 1.3).backward()
    assert l1.dtype == torch.float32 and cs.dtype == torch.float32
    assert abs(float(l1) - float(rl1)) <= 1e-5 * max(1.0, abs(float(rl1)))
    assert abs(float(cs) - float(rcs)) <= 1e-5 * max(1.0, abs(float(rcs)))
    g, rg = x.grad.double().cpu(), r.grad
    assert torch.isfinite(g).all()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    scale = float(rg.abs().max()) + 1e-30
    assert float((g - rg).abs().max()) <= tol * scale, (float((g - rg).abs().max()), scale)
    if all_ignored:
        assert float(l1) == 0.0 and float(cs) == 0.0 and float(g.abs().max()) == 0.0


def check_bias_reproducible(device, n):
    from pointcept_amd import functional as PF

    bp, coord, cen, inst = bias_inputs(device, n, torch.bfloat16, seed=4)
    grads, losses = [], []
    for _ in range(2):
        x = bp.detach().clone().requires_grad_(True)
        l1, cs = PF.pg_bias_loss(x, coord, cen, inst, -1)
        (l1 + cs).backward()
        grads.append(x.grad.cpu())
        losses.append(torch.stack([l1, cs]).detach().cpu())
    assert torch.equal(grads[0], grads[1]) and torch.equal(losses[0], losses[1])


# ------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(designed_cases()))
def test_ball_query_equals_the_oracle(cuda, name):
    check_ball_query(cuda, *designed_cases()[name])


def test_torch_formulation_equals_the_oracle(cuda):
    from pointcept_amd import functional as PF

    for name in ("exactly_1000_and_1001", "nan_and_inf_rows", "empty_batch_segment", "boundary_radius"):
        xyz, b, nb, r = designed_cases()[name]
        off = offsets_of(b, nb)
        idx_o, sl_o = O.ballquery_batch_p(xyz, b, off, r)
        idx, sl = PF.pg_ball_query_torch(torch.from_numpy(xyz).to(cuda), torch.from_numpy(b).to(cuda), torch.from_numpy(off), r)
        assert np.array_equal(sl.cpu().numpy(), sl_o) and np.array_equal(idx.cpu().numpy(), idx_o), name


def test_ball_query_2x100k_equals_the_torch_formulation(cuda):
    from pointcept_amd import functional as PF
    from pointcept_amd import ops

    xyz, b = noisy_centres([100000, 100000], seed=11, n_inst=60, spread=3.0, extent=150)
    x, bb = torch.from_numpy(xyz).to(cuda), torch.from_numpy(b).to(cuda)
    idx, sl, _ = ops.pg_ball_query(x, bb, 2, 1.5)
    idx_t, sl_t = PF.pg_ball_query_torch(x, bb, torch.from_numpy(offsets_of(b, 2)), 1.5)
    assert torch.equal(sl, sl_t) and torch.equal(idx, idx_t)
    lab = (np.arange(xyz.shape[0]) % 3).astype(np.int32)
    ci, co = ops.pg_cluster(torch.from_numpy(lab).to(cuda), idx, sl, 50)
    ref = PF.pg_bfs_cluster_host(torch.from_numpy(lab), idx.cpu(), sl.cpu(), 50)
    O.assert_same_clusters((ref[0].numpy(), ref[1].numpy()), (ci.cpu().numpy(), co.cpu().numpy()))


def test_collapsed_scene_gives_one_1000_point_cluster(cuda):
    check_collapsed(cuda)


def test_cluster_threshold_and_mixed_labels(cuda):
    check_threshold_and_mixed_labels(cuda)


def test_cluster_truncated_components_follow_the_sequential_rule(cuda):
    check_truncated_mixed(cuda)
    check_truncated_mixed(cuda, n=6000, seed=4)


def test_cluster_on_designed_cases(cuda):
    for name, (xyz, b, nb, r) in designed_cases().items():
        idx, sl, _ = check_ball_query(cuda, xyz, b, nb, r)
        lab = (np.arange(xyz.shape[0]) % 2).astype(np.int32)
        for t in (1, 3):
            check_cluster(cuda, lab, idx, sl, t)


def test_clustering_bit_reproducible(cuda):
    xyz, b = noisy_centres([20000, 15000], seed=12, n_inst=30, spread=0.4, extent=30)
    check_reproducible(cuda, xyz, b, 2, 1.5, (np.arange(xyz.shape[0]) % 2).astype(np.int32), 10)
    x = np.random.default_rng(3).normal(0, 0.05, (5000, 3)).astype(np.float32)
    check_reproducible(cuda, x, np.zeros(5000, np.int32), 1, 1.5, np.zeros(5000, np.int32), 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_bias_loss_against_float64_autograd(cuda, dtype):
    check_bias_loss(cuda, 70000, dtype)
    check_bias_loss(cuda, 300, dtype, all_ignored=True)


def test_bias_loss_gradients_bit_reproducible(cuda):
    check_bias_reproducible(cuda, 200000)


def test_mirror_signatures_and_dtypes(cuda):
    from pointcept_amd import compat

    import sys

    saved = sys.modules.pop("pointgroup_ops", None)
    try:
        compat.install(pointgroup=True)
        import pointgroup_ops as P

        xyz, b = noisy_centres([3000], seed=8, n_inst=5, spread=0.5, extent=10)
        idx, sl = P.ballquery_batch_p(torch.from_numpy(xyz).to(cuda), torch.from_numpy(b).to(cuda),
                                      torch.tensor([0, 3000], dtype=torch.int32, device=cuda), 1.5, 300)
        assert idx.dtype == torch.int32 and sl.dtype == torch.int32 and idx.is_cuda and sl.shape == (3000, 2)
        lab = torch.zeros(3000, dtype=torch.int32)
        ci, co = P.bfs_cluster(lab, idx.cpu(), sl.cpu(), 50)
        assert not ci.is_cuda and ci.dtype == torch.int32 and co.dtype == torch.int32
        O.assert_same_clusters(O.bfs_cluster(lab.numpy(), idx.cpu().numpy(), sl.cpu().numpy(), 50), (ci.numpy(), co.numpy()))
        with pytest.raises(Exception):
            P.bfs_cluster(lab, idx.cpu()[:10], sl.cpu(), 50)
    finally:
        sys.modules.pop("pointgroup_ops", None)
        if saved is not None:
            sys.modules["pointgroup_ops"] = saved


# ------------------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------------------
SPUNET = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2))
PG_CFG = dict(backbone=SPUNET, backbone_out_channels=96, semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1),
              instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# tests/golden/make_golden_pointgroup.py: the reference file's configuration of pointgroup_tiny.npz
GOLD_BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, base_channels=16, channels=(16, 32, 48, 64, 64, 48, 32, 32),
                     layers=(1, 2, 1, 1, 1, 1, 2, 1))
GOLD_CFG = dict(backbone=GOLD_BACKBONE, backbone_out_channels=32, semantic_num_classes=20, semantic_ignore_index=-1,
                segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1, cluster_thresh=6.0, cluster_closed_points=300,
                cluster_propose_points=8, cluster_min_points=4, voxel_size=0.02)
LOSSES = ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss")


def golden():
    return np.load(os.path.join(GOLD, "pointgroup_tiny.npz"))


def golden_batch(g):
    """the two synthetic scenes of the golden, regenerated from their seeds and checked against the stored checksums"""
    from pointcept_amd import synthetic

    scenes = [synthetic.indoor_instance_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])]
    for sc in scenes:
        sc.pop("bbox")
    b = synthetic.collate(scenes)
    ck = [float(b["coord"].astype(np.float64).sum()), float(b["feat"].astype(np.float64).sum()), float(b["segment"].sum()),
          float(b["instance"].sum()), float(b["instance_centroid"].astype(np.float64).sum())]
    assert np.allclose(ck, g["input_checksum"], rtol=1e-9), "synthetic.indoor_instance_scene no longer gives the golden's scenes"
    return b


def golden_state(g, net):
    from oracle import ptv3_model as om

    sd = om.deterministic_state_dict(net, int(g["sd_seed"]))
    assert list(sd.keys()) == [str(k) for k in g["keys"]], "state-dict keys differ from the reference file's"
    assert np.allclose([float(v.double().sum()) for v in sd.values()], g["sd_checksum"], rtol=1e-9)
    return sd


def members_of(masks):
    m = [np.nonzero(r)[0] for r in np.asarray(masks)]
    return (np.concatenate(m).astype(np.int32) if m else np.zeros(0, np.int32)), np.concatenate([[0], np.cumsum([len(x) for x in m])])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def check_eval_outputs_equal_golden(ev, g, score_tol=1e-5):
    """pred_masks (as member lists) and pred_classes identical, pred_scores within score_tol, the reference's dtypes"""
    assert ev["pred_masks"].dtype == torch.int32 and not ev["pred_masks"].is_cuda
    mem, off = members_of(ev["pred_masks"].numpy())
    assert np.array_equal(off, g["mask_offsets"]) and np.array_equal(mem, g["mask_members"]), "proposal masks differ from the reference"
    assert ev["pred_classes"].dtype == torch.int64 and np.array_equal(ev["pred_classes"].numpy(), g["pred_classes"])
    assert ev["pred_scores"].dtype == torch.float32
    assert np.allclose(ev["pred_scores"].numpy(), g["pred_scores"], rtol=score_tol, atol=score_tol)


def check_port_against_golden(device, cls=None, loss_tol=2e-3, grad_tol=2e-2, head_tol=2e-2):
    """the port on the golden's weights and scenes: train-mode losses and head gradients, eval-mode head outputs and losses against
    the reference file's; then the eval clustering with the heads pinned to the reference's head outputs gives the reference's
    proposals exactly"""
    from pointcept_amd import synthetic
    from pointcept_amd.point_group import PointGroup

    g = golden()
    net = (cls or PointGroup)(**GOLD_CFG)
    net.load_state_dict(golden_state(g, net))
    net = net.to(device).train()
    inp = synthetic.to_torch(golden_batch(g), device)
    out = net(dict(inp))
    out["loss"].backward()
    for k in LOSSES:
        assert abs(float(out[k]) - float(g[k])) <= loss_tol * max(1.0, abs(float(g[k]))), (k, float(out[k]), float(g[k]))
    heads = {k: p for k, p in net.named_parameters() if k.startswith(("bias_head.", "seg_head."))}
    scale = max(float(np.abs(g["grad/" + k]).max()) for k in heads)
    for k, p in heads.items():
        ours, ref = p.grad.cpu().numpy(), g["grad/" + k]
        if np.abs(ref).max() <= 1e-5 * scale:
            # bias_head.0.bias: a Linear bias followed by a training-mode BatchNorm has a zero gradient; both sides hold rounding noise
            assert np.abs(ours).max() <= 1e-5 * scale, k
        else:
            assert _rel(ours, ref) <= grad_tol, (k, _rel(ours, ref))
    net.eval()
    seen = {}
    own_heads = net.heads

    def recording(f):
        seen["bias"], seen["logit"] = own_heads(f)
        return seen["bias"], seen["logit"]

    net.heads = recording
    with torch.no_grad():
        ev = net(dict(inp))
    assert _rel(seen["bias"].cpu().numpy(), g["eval_bias_pred"]) <= head_tol
    assert _rel(seen["logit"].cpu().numpy(), g["eval_logit_pred"]) <= head_tol
    for k in LOSSES:
        assert abs(float(ev[k]) - float(g["eval_" + k])) <= loss_tol * max(1.0, abs(float(g["eval_" + k]))), k
    bias = torch.from_numpy(g["eval_bias_pred"]).to(device)
    logit = torch.from_numpy(g["eval_logit_pred"]).to(device)
    net.heads = lambda f: (bias, logit)
    with torch.no_grad():
        ev = net(dict(inp))
    check_eval_outputs_equal_golden(ev, g)
    del net.heads


def check_golden_ops_fixture(device):
    """the reference restatement's lists and clusters stored in the golden, reproduced by the kernels"""
    from pointcept_amd import ops

    g = golden()
    xyz, lab = g["ops_xyz"], g["ops_label"]
    idx, sl, _ = ops.pg_ball_query(torch.from_numpy(xyz).to(device), torch.zeros(xyz.shape[0], dtype=torch.int32, device=device), 1,
                                   float(g["ops_radius"]))
    assert np.array_equal(sl.cpu().numpy(), g["ops_start_len"]) and np.array_equal(idx.cpu().numpy(), g["ops_idx"])
    ci, co = ops.pg_cluster(torch.from_numpy(lab).to(device), idx, sl, int(g["ops_threshold"]))
    O.assert_same_clusters((g["ops_cluster_idxs"], g["ops_cluster_offsets"]), (ci.cpu().numpy(), co.cpu().numpy()))


def instance_batch(device, sizes=(100000, 100000), seeds=(61, 62)):
    from pointcept_amd import synthetic

    return synthetic.to_torch(synthetic.indoor_instance_batch(seeds, sizes), device)


def test_state_dict_keys_are_the_references(cuda):
    """PG-v1m1 and PG-v1m2 have the reference file's keys (stored in the golden), in its order"""
    from pointcept_amd.point_group import PointGroup, PointGroupV1m2

    g = golden()
    crit = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]
    for net in (PointGroup(**GOLD_CFG), PointGroupV1m2(**GOLD_CFG, criteria=crit)):
        assert list(net.state_dict().keys()) == [str(k) for k in g["keys"]]


def test_port_matches_reference_golden(cuda):
    check_port_against_golden(cuda)


def test_v1m2_port_matches_reference_golden(cuda):
    """PG-v1m2 with the reference criteria list [CrossEntropyLoss] computes what PG-v1m1 does"""
    from functools import partial

    from pointcept_amd.point_group import PointGroupV1m2

    check_port_against_golden(cuda, partial(PointGroupV1m2, criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]))


def test_golden_ops_fixture(cuda):
    check_golden_ops_fixture(cuda)


def test_v1m2_refuses_criteria_it_does_not_implement():
    from pointcept_amd.point_group import PointGroupV1m2

    for bad in (dict(type="CrossEntropyLoss", label_smoothing=0.1), dict(type="CrossEntropyLoss", weight=[1.0] * 20),
                dict(type="LovaszLoss", mode="binary"), dict(type="FocalLoss")):
        with pytest.raises(ValueError):
            PointGroupV1m2(**GOLD_CFG, criteria=[bad])


def test_registered_only_when_named():
    from pointcept_amd import compat

    class Reg:
        def __init__(self):
            self.names = []

        def register_module(self, name, force, module):
            self.names.append(name)

    r = Reg()
    compat.register_models(r)
    assert "PG-v1m1" not in r.names and "PG-v1m2" not in r.names
    assert compat.register_models(Reg(), names=["PG-v1m1", "PG-v1m2"]) == ["PG-v1m1", "PG-v1m2"]


def _eval_both(net, batch, monkeypatch):
    from pointcept_amd import config

    net.eval()
    with torch.no_grad():
        out_k = net(dict(batch))
        monkeypatch.setattr(config, "PG_CLUSTER", False)
        out_t = net(dict(batch))
        monkeypatch.setattr(config, "PG_CLUSTER", True)
    return out_k, out_t


def check_eval_equal(out_k, out_t):
    for k in ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss"):
        assert abs(float(out_k[k]) - float(out_t[k])) <= 1e-4 * max(1.0, abs(float(out_t[k]))), k
    assert out_k["pred_masks"].dtype == torch.int32 and not out_k["pred_masks"].is_cuda
    assert torch.equal(out_k["pred_masks"], out_t["pred_masks"])
    assert torch.equal(out_k["pred_classes"], out_t["pred_classes"])
    assert out_k["pred_scores"].dtype == out_t["pred_scores"].dtype
    assert torch.allclose(out_k["pred_scores"], out_t["pred_scores"].float(), rtol=1e-5, atol=1e-6)


def test_v1m1_eval_kernels_equal_the_reference_expression(cuda, monkeypatch):
    from pointcept_amd.point_group import PointGroup

    torch.manual_seed(0)
    net = PointGroup(**{**PG_CFG, "cluster_propose_points": 20, "cluster_min_points": 10}).to(cuda)
    batch = instance_batch(cuda, (30000, 20000))
    # a bias head that predicts the offsets (plus noise): realistic centres; the seg head's logits from the labels
    with torch.no_grad():
        net.bias_head[3].weight.zero_()
        net.bias_head[3].bias.zero_()
        net.seg_head.weight.zero_()
        net.seg_head.bias.zero_()
    net.eval()
    with torch.no_grad():
        feat = net.backbone(dict(batch))
        gt = batch["instance_centroid"] - batch["coord"]
        gt = torch.where(batch["instance"][:, None] >= 0, gt, torch.zeros_like(gt))
        noise = torch.randn_like(gt) * 0.05
        seg = batch["segment"].clamp(min=0)
        logits = torch.nn.functional.one_hot(seg, 20).float() * 4 + torch.randn(seg.shape[0], 20, device=cuda) * 0.5
    heads = lambda f: (gt + noise, logits)          # noqa: E731
    net.heads = heads
    out_k, out_t = _eval_both(net, batch, monkeypatch)
    assert out_k["pred_masks"].shape[0] >= 3
    check_eval_equal(out_k, out_t)


def test_eval_all_points_ignored_returns_empty(cuda):
    from pointcept_amd.point_group import PointGroup

    net = PointGroup(**PG_CFG).to(cuda).eval()
    batch = instance_batch(cuda, (3000, 2000))
    n = batch["coord"].shape[0]
    logits = torch.zeros(n, 20, device=cuda)
    logits[:, 0] = 5.0                               # every point predicted as class 0 (ignored)
    net.heads = lambda f: (torch.zeros(n, 3, device=cuda), logits)
    with torch.no_grad():
        out = net(dict(batch))
    assert out["pred_masks"].shape == (0, n) and out["pred_scores"].numel() == 0 and out["pred_classes"].numel() == 0


def test_v1m2_ptv3_eval_forward(cuda):
    from pointcept_amd.point_group import PointGroupV1m2

    bb = dict(type="PT-v3m1", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
              enc_depths=(1, 1, 1, 1, 1), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
              enc_patch_size=(128,) * 5, dec_depths=(1, 1, 1, 1), dec_channels=(64, 64, 128, 256), dec_num_head=(4, 4, 8, 16),
              dec_patch_size=(128,) * 4, drop_path=0.0, shuffle_orders=False)
    crit = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1), dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0,
                                                                                 ignore_index=-1)]
    net = PointGroupV1m2(backbone=bb, backbone_out_channels=64, criteria=crit).to(cuda)
    batch = instance_batch(cuda, (8000, 6000))
    net.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(dict(batch))
    out["loss"].backward()
    assert torch.isfinite(out["loss"])
    net.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(dict(batch))
    assert out["pred_masks"].dtype == torch.int32 and out["pred_masks"].shape[1] == batch["coord"].shape[0]
    assert set(out) >= {"loss", "pred_scores", "pred_masks", "pred_classes"}


def test_scannet_v1m1_step_2x100k_bf16(cuda):
    from pointcept_amd.point_group import PointGroup

    torch.manual_seed(0)
    net = PointGroup(**PG_CFG).to(cuda).train()
    batch = instance_batch(cuda)
    sd = {k: v.clone() for k, v in net.state_dict().items()}

    def step(amp):
        net.load_state_dict(sd)
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = net(dict(batch))
        out["loss"].backward()
        return out, net.bias_head[0].weight.grad.float().clone()

    out32, g32 = step(False)
    step(True)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out16, g16 = step(True)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert any("pg_bias_fwd_kernel" in k for k in names), "the profiler captured no kernel of the step"
    assert not [k for k in names if k.startswith("Cijk_")], "library GEMM in the PointGroup step"
    aten = [k for k in names if "at::native" in k and any(s in k for s in ("scatter", "index_add", "indexFunc", "index_put"))]
    assert not aten, aten
    for k in ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss"):
        assert torch.isfinite(out16[k]) and abs(float(out16[k]) - float(out32[k])) <= 0.05 * max(1.0, abs(float(out32[k]))), k
    rel = float((g16 - g32).norm() / g32.norm())
    assert rel < 0.1, rel


def test_eval_clustering_reads_the_host_at_most_twice(cuda):
    """realistic centres: the clustering of one eval forward issues at most 2 device-to-host copies before its 2 output copies"""
    from pointcept_amd.point_group import PointGroup

    net = PointGroup(**PG_CFG).to(cuda).eval()
    batch = instance_batch(cuda, (100000, 100000))
    n = batch["coord"].shape[0]
    gt = batch["instance_centroid"] - batch["coord"]
    gt = torch.where(batch["instance"][:, None] >= 0, gt, torch.zeros_like(gt))
    logits = torch.nn.functional.one_hot(batch["segment"].clamp(min=0), 20).float()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        scores, masks, classes = net._proposals(batch["coord"], gt, logits, batch["offset"])
        torch.cuda.synchronize()
    d2h = [e for e in prof.events() if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name]
    assert 2 <= len(d2h) <= 4, [e.name for e in d2h]        # >= the 2 output copies: the check does see copies
    assert masks.shape[0] > 0 and masks.shape[1] == n
