"""-m gpu: OA-CNNs (pointcept/models/oacnns/oacnns_v1m1_base.py) on the engine.

  * grid-cluster maps (csrc/cluster_agg.hip + ptc_sort_keys / ptc_pool_maps_*) against oracle/shims.voxel_grid + torch.unique:
    bit-exact partition and numbering;
  * segmented centering and the fused adaptive aggregation, forward and backward, against a float64 torch restatement of :87-102,
    including 1-row clusters, a cluster of >= 50 000 rows, >= 400 000 rows, and a scene whose weight logits sit 100 below the rest
    (its clusters are governed by the 1e-6: the maximum must be the global one); bit-reproducibility of outputs and gradients;
  * the port against tests/golden/oacnns_tiny.npz (the reference file on the CPU stand-ins, fp32) and against the reference file itself
    running on the engine's B3 mirrors (compat.install(geometric=True));
  * one bf16 and one fp16 + GradScaler step of the ScanNet configuration at 2 x 100 000 voxels: finite, close to fp32, no library GEMM
    and no ATen scatter / index_add kernel.

The check_* bodies take a device: tests/test_oacnns_cpu.py runs them at small shapes on the host emulation of the kernel sources.
"""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def make_indices(scenes, seed=0, big_cluster=0):
    """int32 [N, 4] (batch, x, y, z) of len(scenes) scenes: scenes[b] = (rows, extent, shift); rows drawn without duplicates inside a
    box of `extent` voxels moved by `shift` (so a scene's own minimum differs from the global one).  big_cluster > 0: the first scene
    also gets that many rows packed in one 64^3 corner box (one cluster at every cell size >= 64)."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for b, (rows, extent, shift) in enumerate(scenes):
        lin = torch.randperm(extent ** 3, generator=g)[:rows]
        xyz = torch.stack([lin % extent, (lin // extent) % extent, lin // (extent * extent)], 1) + shift
        if b == 0 and big_cluster:
            lin2 = torch.randperm(64 ** 3, generator=g)[:big_cluster]
            xyz = torch.cat([xyz + 64, torch.stack([lin2 % 64, (lin2 // 64) % 64, lin2 // 4096], 1)])
        parts.append(torch.cat([torch.full((xyz.shape[0], 1), b, dtype=torch.int64), xyz], 1))
    return torch.cat(parts).to(torch.int32)


def reference_clusters(ind, size):
    from oracle import shims

    ids = shims.voxel_grid(pos=ind[:, 1:].float(), size=size, batch=ind[:, 0].long())
    return torch.unique(ids, return_inverse=True)[1]


def _shape(ind):
    return [int(m) + 1 for m in ind[:, 1:].long().max(0).values]


# ------------------------------------------------------------------------------------------------------------------------------------
# checks (device-agnostic bodies)
# ------------------------------------------------------------------------------------------------------------------------------------
def check_cluster_maps(device, scenes, sizes, seed=0):
    from pointcept_amd import ops

    ind = make_indices(scenes, seed)
    gc = ops.grid_clusters(ind.to(device), sizes, _shape(ind), len(scenes))
    for l, s in enumerate(sizes):
        ref = reference_clusters(ind, s)
        assert torch.equal(gc.cluster[l].cpu(), ref), f"size {s}"
        assert gc.n_cluster[l] == int(ref.max()) + 1
        order, ip = gc.order[l].cpu(), gc.indptr[l].cpu()
        assert torch.equal(torch.sort(order).values, torch.arange(ind.shape[0]))
        assert torch.equal(ref[order], torch.repeat_interleave(torch.arange(gc.n_cluster[l]), ip[1:] - ip[:-1]))
    return gc


def agg_reference(us, vs, a, gc):
    """float64 restatement of oacnns_v1m1_base.py:92-102 (the reference's own expression, index_add scatters)"""
    from pointcept_amd import functional as PF

    return PF.cluster_agg_torch(us, vs, a, gc)


def make_agg_inputs(gc, n, c, dtype, seed=1, shift_rows=None):
    g = torch.Generator().manual_seed(seed)
    L = gc.levels
    us = [torch.randn(n, c, generator=g, dtype=torch.float64) * 2 for _ in range(L)]
    if shift_rows is not None:
        for u in us:
            u[shift_rows] -= 100.0        # one scene far below the global max: its clusters are governed by the 1e-6
    vs = [torch.randn(n, c, generator=g, dtype=torch.float64) for _ in range(L)]
    a = torch.randn(n, L, generator=g, dtype=torch.float64)
    dout = torch.randn(n, c, generator=g, dtype=torch.float64)
    rnd = lambda t: t.to(dtype).to(torch.float64)   # noqa: E731  the reference sees the operands the kernel sees
    return [rnd(u) for u in us], [rnd(v) for v in vs], rnd(a), rnd(dout)


def run_agg(us, vs, a, dout, gc, device, dtype):
    from pointcept_amd import functional as PF

    ut = [u.to(device, dtype).requires_grad_() for u in us]
    vt = [v.to(device, dtype).requires_grad_() for v in vs]
    at = a.to(device, dtype).requires_grad_()
    out = PF.cluster_agg(ut, vt, at, gc)
    out.backward(dout.to(device, dtype))
    return out.detach(), [t.grad for t in ut], [t.grad for t in vt], at.grad


def check_agg_against_float64(device, dtype, gc, n, c, shift_rows=None, seed=1):
    us, vs, a, dout = make_agg_inputs(gc, n, c, dtype, seed, shift_rows)
    out, du, dv, da = run_agg(us, vs, a, dout, gc, device, dtype)
    assert out.dtype == dtype and all(t.dtype == dtype for t in du + dv + [da])
    gcc = _cpu_clusters(gc)
    u64 = [u.clone().requires_grad_() for u in us]
    v64 = [v.clone().requires_grad_() for v in vs]
    a64 = a.clone().requires_grad_()
    ref = agg_reference(u64, v64, a64, gcc)
    ref.backward(dout)
    tol = {torch.float32: 2e-5, torch.float16: 4e-3, torch.bfloat16: 2e-2}[dtype]
    assert torch.isfinite(out).all()
    assert _rel(out, ref) < tol, ("out", _rel(out, ref))
    assert _rel(da, a64.grad) < 4 * tol, ("da", _rel(da, a64.grad))
    for l in range(gc.levels):
        assert _rel(dv[l], v64[l].grad) < 4 * tol, ("dv", l, _rel(dv[l], v64[l].grad))
        assert _rel(du[l], u64[l].grad) < 4 * tol, ("du", l, _rel(du[l], u64[l].grad))
    if shift_rows is not None:     # the shifted scene's clusters are epsilon-dominated: S ~ 0 there, as in the reference
        assert float(ref.detach()[shift_rows].abs().max()) < 1e-6 * float(ref.detach().abs().max())
        assert float(out[shift_rows.to(out.device)].abs().max()) < 1e-6 * float(ref.detach().abs().max()) + 1e-30
    return out, du, dv, da


def check_agg_reproducible(device, dtype, gc, n, c):
    us, vs, a, dout = make_agg_inputs(gc, n, c, dtype, seed=3)
    r1 = run_agg(us, vs, a, dout, gc, device, dtype)
    r2 = run_agg(us, vs, a, dout, gc, device, dtype)
    flat = lambda r: [r[0]] + list(r[1]) + list(r[2]) + [r[3]]   # noqa: E731
    for x, y in zip(flat(r1), flat(r2)):
        assert torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                           y.view(torch.int16 if y.element_size() == 2 else torch.int32))


def check_agg_max_ties(device, gc, n, c):
    """several elements equal to the global max (1-row clusters of a centered input give exact zeros): the max's gradient is spread
    evenly over all of them, as torch's backward of a full max() does"""
    us, vs, a, dout = make_agg_inputs(gc, n, c, torch.float32, seed=5)
    us = [-u.abs() for u in us]
    for u in us:
        u[: 7, : 3] = 0.0
    out, du, dv, da = run_agg(us, vs, a, dout, gc, device, torch.float32)
    u64 = [u.clone().requires_grad_() for u in us]
    ref = agg_reference(u64, vs, a, _cpu_clusters(gc))
    ref.backward(dout)
    for l in range(gc.levels):    # (the max's gradient is a sum over every element with cancellation: fp32 rounding of that sum)
        assert _rel(du[l], u64[l].grad) < 1e-3, _rel(du[l], u64[l].grad)


def check_center(device, dtype, gc, n, c):
    from pointcept_amd import functional as PF

    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(n, c, generator=g, dtype=torch.float64).to(dtype).double() + 3 for _ in range(gc.levels)]
    dys = [torch.randn(n, c, generator=g, dtype=torch.float64).to(dtype).double() for _ in range(gc.levels)]
    xt = [x.to(device, dtype).requires_grad_() for x in xs]
    ys = PF.cluster_center(xt, gc)
    sum((y.float() * d.to(device, torch.float32)).sum() for y, d in zip(ys, dys)).backward()
    x64 = [x.clone().requires_grad_() for x in xs]
    yr = PF.cluster_center_torch(x64, _cpu_clusters(gc))
    sum((y * d).sum() for y, d in zip(yr, dys)).backward()
    tol = {torch.float32: 1e-5, torch.float16: 4e-3, torch.bfloat16: 2e-2}[dtype]
    for l in range(gc.levels):
        assert ys[l].dtype == dtype
        assert _rel(ys[l], yr[l]) < tol and _rel(xt[l].grad, x64[l].grad) < tol


def _cpu_clusters(gc):
    from pointcept_amd import ops

    return ops.GridClusters([t.cpu() for t in gc.order], [t.cpu() for t in gc.cluster], [t.cpu() for t in gc.indptr], list(gc.n_cluster))


def check_refuses_bad_shapes(device, gc, n):
    from pointcept_amd import functional as PF
    from pointcept_amd._lib import PtcoreError

    for c in (6, 260):
        us = [torch.zeros(n, c, device=device) for _ in range(gc.levels)]
        with pytest.raises(PtcoreError):
            PF.cluster_agg(us, us, torch.zeros(n, gc.levels, device=device), gc)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ------------------------------------------------------------------------------------------------------------------------------------
SCENES = [(3000, 40, 0), (2000, 30, 17), (900, 24, 5)]


@pytest.mark.gpu
def test_cluster_maps_match_voxel_grid_and_unique(cuda):
    check_cluster_maps(cuda, SCENES, [2, 6, 9, 24])
    check_cluster_maps(cuda, [(50000, 60, 3), (30000, 50, 40)], [1, 3, 7, 64], seed=4)


@pytest.fixture(scope="module")
def mixed(cuda):
    """three scenes with clusters of 1 row upwards, the middle scene shifted by -100 in the weight logits"""
    from pointcept_amd import ops

    ind = make_indices(SCENES, seed=2)
    gc = ops.grid_clusters(ind.to(cuda), [1, 3, 6, 9], _shape(ind), len(SCENES))
    rows = torch.nonzero(ind[:, 0] == 1)[:, 0]
    return gc, ind.shape[0], rows


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("c", [64, 96, 256])
def test_aggregation_against_float64(cuda, mixed, dtype, c):
    gc, n, rows = mixed
    assert min(gc.indptr[0][1:] - gc.indptr[0][:-1]).item() == 1
    check_agg_against_float64(cuda, dtype, gc, n, c, shift_rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_aggregation_three_levels_large(cuda, dtype):
    """>= 400 000 rows (every workgroup walks many row tiles) with one cluster of >= 50 000 rows, L = 3"""
    from pointcept_amd import ops

    ind = make_indices([(350000, 120, 0), (60000, 60, 9)], seed=6, big_cluster=60000)
    gc = ops.grid_clusters(ind.to(cuda), [4, 16, 64], _shape(ind), 2)
    n = ind.shape[0]
    assert n >= 400000
    assert int((gc.indptr[2][1:] - gc.indptr[2][:-1]).max()) >= 50000
    check_agg_against_float64(cuda, dtype, gc, n, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_aggregation_bit_reproducible(cuda, mixed, dtype):
    gc, n, _ = mixed
    check_agg_reproducible(cuda, dtype, gc, n, 96)


@pytest.mark.gpu
def test_aggregation_max_ties(cuda, mixed):
    gc, n, _ = mixed
    check_agg_max_ties(cuda, gc, n, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_centering_against_float64(cuda, mixed, dtype):
    gc, n, _ = mixed
    check_center(cuda, dtype, gc, n, 128)


@pytest.mark.gpu
def test_aggregation_refuses_unsupported_widths(cuda, mixed):
    gc, n, _ = mixed
    check_refuses_bad_shapes(cuda, gc, n)


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(GOLD, "oacnns_tiny.npz"))


def golden_cfg():
    return dict(in_channels=6, num_classes=13, embed_channels=16, enc_num_ref=[16, 16, 16], enc_channels=[16, 16, 24], groups=[4, 4, 4],
                enc_depth=[1, 2, 1], down_ratio=[2, 2, 2], dec_channels=[16, 16, 24],
                point_grid_size=[[3, 6, 9, 16], [2, 6, 9], [2, 3, 5]], dec_depth=[1, 1, 1])


def golden_state(g, net):
    """the fixture's weights: deterministic_state_dict is a function of the key names and the seed, regenerated here from `net` and
    checked against the fixture's key list and per-tensor sums"""
    from oracle import ptv3_model as om

    sd = om.deterministic_state_dict(net, int(g["sd_seed"]))
    assert list(sd.keys()) == list(g["keys"])
    assert np.allclose([float(v.double().sum()) for v in sd.values()], g["sd_checksum"], rtol=1e-9, atol=1e-9)
    return sd


def golden_batch(g, device):
    from pointcept_amd import synthetic

    b = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    assert np.allclose([float(b["grid_coord"].sum()), float(b["feat"].astype(np.float64).sum()), float(b["segment"].sum())],
                       g["input_checksum"], rtol=1e-12)
    t = {k: torch.from_numpy(b[k]).to(device) for k in ("grid_coord", "feat", "offset", "segment")}
    t["feat"] = t["feat"].float()
    return t


def check_model_against_golden(net, g, device):
    from pointcept_amd import functional as PF

    assert list(net.state_dict().keys()) == list(g["keys"])
    net.load_state_dict(golden_state(g, net))
    net = net.to(device)
    b = golden_batch(g, device)
    amax = float(g["logits_absmax"])
    net.eval()
    with torch.no_grad():
        out = net(dict(b)).float().cpu().numpy()
    assert np.isfinite(out).all()
    assert np.abs(out[::4] - g["logits_eval"]).max() <= 1e-3 * amax
    net.train()
    logits = net(dict(b))
    loss = PF.cross_entropy(logits, b["segment"].long() % 13, -1)
    loss.backward()
    assert np.abs(logits.detach().float().cpu().numpy()[::8] - g["logits_train"]).max() <= 1e-3 * amax
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    names = [k for k, _ in net.named_parameters()]
    assert names == list(g["param_names"])
    norms = np.asarray([float(p.grad.double().norm()) for _, p in net.named_parameters()])
    big = g["grad_norms"] > 1e-4 * g["grad_norms"].max()
    assert np.allclose(norms[big], g["grad_norms"][big], rtol=2e-2), np.abs(norms[big] / g["grad_norms"][big] - 1).max()
    gmax = float(g["grad_norms"].max())
    for k, p in net.named_parameters():
        if "grad/" + k in g.files:
            ref = torch.from_numpy(g["grad/" + k])
            # biases in front of a BatchNorm have a zero gradient up to rounding on both sides
            assert float((p.grad.cpu() - ref).norm()) <= 2e-2 * float(ref.norm()) + 1e-4 * gmax, k
    sd = net.state_dict()
    for k in g.files:
        if k.startswith("after/"):
            assert _rel(sd[k[6:]], torch.from_numpy(g[k])) < 1e-3, k


@pytest.mark.gpu
def test_oacnns_port_matches_reference_golden(cuda):
    from pointcept_amd.oacnns import OACNNs

    torch.manual_seed(0)
    check_model_against_golden(OACNNs(**golden_cfg()), golden(), cuda)


@pytest.mark.gpu
def test_oacnns_registered_only_when_named():
    from pointcept_amd import compat
    from pointcept_amd.oacnns import OACNNs

    class Reg:
        def __init__(self):
            self.d = {}

        def register_module(self, name, force, module):
            self.d[name] = module

    r = Reg()
    assert "OACNNs" not in compat.register_models(r)
    assert compat.register_models(r, names=["OACNNs"]) == ["OACNNs"] and r.d["OACNNs"] is OACNNs


@pytest.mark.gpu
@pytest.mark.needs_reference
def test_reference_oacnns_file_on_the_b3_mirrors_matches_the_port(cuda):
    import importlib
    import sys
    import types

    from oracle import ref_import
    from pointcept_amd import compat
    from pointcept_amd.oacnns import OACNNs

    if not ref_import.available():
        pytest.skip("reference tree absent")
    ref_import.load()
    mod = "pointcept.models.oacnns.oacnns_v1m1_base"
    names = ["spconv", "spconv.pytorch", "spconv.pytorch.modules", "flash_attn", "torch_scatter", "pointops", "pointops2",
             "pointops2.pointops", "pointops2.functions", "pointops2.functions.pointops", "pointrope", "torch_geometric",
             "torch_geometric.nn", "torch_geometric.nn.pool", "torch_geometric.utils", "pointcept.models.oacnns", mod]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        compat.install(force=True, geometric=True)
        sys.modules.pop(mod, None)
        pk = types.ModuleType("pointcept.models.oacnns")
        pk.__path__ = [ref_import.REF + "/pointcept/models/oacnns"]
        sys.modules["pointcept.models.oacnns"] = pk
        sys.modules["pointcept.models.builder"].MODELS._module_dict.pop("OACNNs", None)
        R = importlib.import_module(mod)
        assert R.voxel_grid.__module__ == "pointcept_amd.torch_geometric_api"
        g = golden()
        torch.manual_seed(0)
        a, b = R.OACNNs(**golden_cfg()), OACNNs(**golden_cfg())
        sd = golden_state(g, b)
        a.load_state_dict(sd)
        b.load_state_dict(sd)
        a, b = a.to(cuda).train(), b.to(cuda).train()
        batch = golden_batch(g, cuda)
        outs = []
        for net in (a, b):
            o = net(dict(batch))
            torch.nn.functional.cross_entropy(o, batch["segment"].long() % 13, ignore_index=-1).backward()
            outs.append(o.detach())
        assert _rel(outs[1], outs[0]) < 1e-3
        ga = dict(a.named_parameters())
        for k, p in b.named_parameters():
            assert float((p.grad - ga[k].grad).norm()) <= 2e-2 * float(ga[k].grad.norm()) + 1e-6, k
    finally:
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


SCANNET = dict(in_channels=9, num_classes=20, embed_channels=64, enc_channels=[64, 64, 128, 256], groups=[4, 4, 8, 16],
               enc_depth=[3, 3, 9, 8], dec_channels=[256, 256, 256, 256],
               point_grid_size=[[8, 12, 16, 16], [6, 9, 12, 12], [4, 6, 8, 8], [3, 4, 6, 6]], dec_depth=[2, 2, 2, 2],
               enc_num_ref=[16, 16, 16, 16])


def scannet_batch(device, n_per_scene=100000, seeds=(51, 52)):
    from pointcept_amd import synthetic

    b = synthetic.collate([synthetic.indoor_scene(s, n_per_scene) for s in seeds])
    t = synthetic.to_torch(b, device)
    t["feat"] = torch.cat([t["feat"], t["feat"][:, :3]], 1).contiguous()      # 9 input channels (coord, color, normal)
    return t


@pytest.mark.gpu
def test_scannet_config_amp_steps(cuda):
    from pointcept_amd import functional as PF
    from pointcept_amd.oacnns import OACNNs

    torch.manual_seed(0)
    net = OACNNs(**SCANNET).to(cuda).train()
    b = scannet_batch(cuda)
    assert b["feat"].shape[0] >= 150000

    def step(dtype, scaler=None):
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
            loss = PF.cross_entropy(net(dict(b)).float(), b["segment"], -1)
        (scaler.scale(loss) if scaler else loss).backward()
        torch.cuda.synchronize()
        grads = [p.grad for p in net.parameters() if p.grad is not None]
        if scaler:
            inv = 1.0 / scaler.get_scale()
            grads = [g * inv for g in grads]
        assert all(torch.isfinite(g).all() for g in grads)
        return float(loss)

    state = {k: v.clone() for k, v in net.state_dict().items()}
    l32 = step(None)
    net.load_state_dict(state)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        lbf = step(torch.bfloat16)
    net.load_state_dict(state)
    l16 = step(torch.float16, torch.amp.GradScaler("cuda", init_scale=1024.0))
    assert np.isfinite([l32, lbf, l16]).all()
    assert abs(lbf - l32) < 2e-2 * l32 and abs(l16 - l32) < 1e-2 * l32, (l32, lbf, l16)
    names = {e.name for e in prof.events()}
    assert not [k for k in names if k.startswith("Cijk_")], "library GEMM in the OA-CNNs step"
    aten = [k for k in names if "at::native" in k and any(s in k for s in ("scatter", "index_add", "indexFunc"))]
    assert not aten, aten
