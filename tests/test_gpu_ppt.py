"""-m gpu: Point Prompt Training (csrc/ppt.hip, pointcept_amd/point_prompt_training.py, pointcept_amd/sparse_unet_v1m3.py).  The
check_* bodies take a device; tests/test_ppt_cpu.py runs them on the host emulation / the CPU backend at the same small shapes.

Kernel against float64: every output (logits, inv_norm) and gradient (dx, dW, db) of functional.ppt_head is compared with
functional.ppt_head_torch (the reference's expression) run in float64.  Tolerance, the rule of test_gpu_cac.py, set before any kernel
figure was seen:
  fp32 inputs    the error of ppt_head_torch in fp32 on the same inputs and device is measured in the test; the kernel may have 4 x that
                 and never less than FLOOR_ULPS = 4 fp32 ulps (4 * 2^-23) of the quantity's scale
  16-bit inputs  the yardstick is the reference's autocast expression (ppt_head_torch under torch.autocast) against float64 on the same
                 rounded inputs, margin 2 x, same floor: the kernel makes the same class of roundings (16-bit x and W into the MFMA, a
                 16-bit dx) and keeps h, the norm and the class product in fp32
Scales: exp(logit_scale) for the logits (exp(logit_scale) times a cosine), the largest inv for inv_norm, the largest element of the
float64 gradient for each gradient.  Every figure is printed before it is asserted.
Rows per workgroup and pass: 128 in the forward (4 waves x 32), 32 in the backward, whose workgroups own 256-row ranges: N = 1000
runs the forward's pass loop (4 workgroups x 2 passes), both tail tiles and 4 reduction partials.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pointcept_amd import functional as PF  # noqa: E402
from pointcept_amd import ops  # noqa: E402

FLOOR_ULPS = 4
ULP = 2.0 ** -23
LOGIT_SCALE = math.log(100.0)          # CLIP's trained logit_scale is ln 100 (clamped there)
SHAPES = [(1, 32, 64, 1), (333, 64, 512, 20), (700, 96, 512, 25), (300, 96, 768, 200), (130, 128, 1024, 13), (1000, 64, 128, 20)]
NAMES = ("logits", "inv_norm", "dx", "dW", "db")


def dev():
    return torch.device("cuda")


def _compare(tag, ref, yard, got, scales, margin, assert_names=NAMES):
    figures = {}
    for name, r, a, k in zip(NAMES, ref, yard, got):
        big = scales[name] if name in scales else float(r.abs().max())
        e_yard = float((a.double() - r).abs().max()) if r.numel() else 0.0
        e_kernel = float((k.double() - r).abs().max()) if r.numel() else 0.0
        bound = max(margin * e_yard, FLOOR_ULPS * ULP * big)
        figures[name] = (e_kernel, e_yard, bound)
        print(f"{tag} {name}: kernel err {e_kernel:.3e}  yardstick err {e_yard:.3e}  bound {bound:.3e}  scale {big:.3e}")
        if name in assert_names:
            assert bool(torch.isfinite(k).all()), (tag, name)
    for name, (e_kernel, e_yard, bound) in figures.items():
        if name in assert_names:
            assert e_kernel <= bound, (tag, name, e_kernel, e_yard, bound)
    return figures


def head_inputs(device, n, c, d, k, seed=0, dtype=torch.float32):
    """x [N, C], W [D, C], b [D], unit class rows e [K, D], a cotangent [N, K]; for a 16-bit dtype x and W hold values of that dtype"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g)
    w = torch.randn(d, c, generator=g) / math.sqrt(c)
    b = 0.1 * torch.randn(d, generator=g)
    e = torch.nn.functional.normalize(torch.randn(k, d, generator=g), dim=1)
    cot = torch.randn(n, k, generator=g)
    if dtype != torch.float32:
        x, w = x.to(dtype).float(), w.to(dtype).float()
    return [t.to(device) for t in (x, w, b, e, cot)]


def _run(fn, x, w, b, e, cot, eps, scale_t=None, **kw):
    a, ww, bb = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ls = torch.tensor(LOGIT_SCALE, dtype=torch.float64 if w.dtype == torch.float64 else torch.float32, device=x.device) if scale_t is None else scale_t
    logits, inv = fn(a, ww, bb, e, ls, eps, return_inv_norm=True, **kw)
    (logits * cot.to(logits.dtype)).sum().backward()
    return [logits.detach(), inv.detach(), a.grad, ww.grad, bb.grad]


def run_all(device, x, w, b, e, cot, eps, dtype):
    """(float64 reference, yardstick, kernel) on the same inputs"""
    ref = _run(PF.ppt_head_torch, x.double(), w.double(), b.double(), e.double(), cot.double(), eps)
    if dtype == torch.float32:
        yard = _run(PF.ppt_head_torch, x, w, b, e, cot, eps)
        got = _run(PF.ppt_head, x, w, b, e, cot, eps, use_kernels=True)
    else:
        with torch.autocast(device_type=device.type, dtype=dtype):
            yard = _run(PF.ppt_head_torch, x, w, b, e, cot, eps)
        got = _run(PF.ppt_head, x.to(dtype), w, b, e, cot, eps, use_kernels=True)
        assert got[2].dtype == dtype
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32
    return ref, yard, got


def check_head(device, n, c, d, k, dtype=torch.float32, eps=0.0, seed=0):
    assert ops.ppt_head_supported(c, d, k, dtype)
    x, w, b, e, cot = head_inputs(device, n, c, d, k, seed, dtype)
    ref, yard, got = run_all(device, x, w, b, e, cot, eps, dtype)
    scales = dict(logits=math.exp(LOGIT_SCALE), inv_norm=float(ref[1].max()))
    return _compare(f"ppt_head N={n} C={c} D={d} K={k} {dtype} eps={eps}", ref, yard, got, scales, 4 if dtype == torch.float32 else 2)


# ---------------------------------------------------------------------------------------------------------------- designed cases
def ill_conditioned(device, n=64, c=64, d=128, k=8, seed=3):
    """W with singular values from 1 down to 1e-3 and rows x near its weakest right singular vector (float64 construction)"""
    g = torch.Generator().manual_seed(seed)
    u, _ = torch.linalg.qr(torch.randn(d, c, generator=g, dtype=torch.float64))
    v, _ = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=torch.float64))
    s = torch.logspace(0, -3, c, dtype=torch.float64)
    w = (u * s) @ v.t()
    x = v[:, -1][None, :] * (1 + 0.1 * torch.randn(n, 1, generator=g, dtype=torch.float64)) + 1e-4 * torch.randn(n, c, generator=g, dtype=torch.float64)
    e = torch.nn.functional.normalize(torch.randn(k, d, generator=g), dim=1)
    cot = torch.randn(n, k, generator=g)
    return [t.float().to(device) for t in (x, w, torch.zeros(d), e, cot)]


def check_ill_conditioned(device):
    """the norm comes from h itself: logits and inv_norm meet the rule where the collapsed quadratic form x^T (W^T W) x, evaluated in
    fp32 on the same inputs, misses it by orders of magnitude (asserted: the case discriminates).  dx, dW and db are held to the same
    4 x rule: the backward's M x_i + u (= W^T h_i, which cancels here) is formed from a float64 M and u and accumulated in double."""
    x, w, b, e, cot = ill_conditioned(device)
    ref, yard, got = run_all(device, x, w, b, e, cot, 1e-12, torch.float32)
    scales = dict(logits=math.exp(LOGIT_SCALE), inv_norm=float(ref[1].max()))
    fig = _compare("ppt_head ill-conditioned W", ref, yard, got, scales, 4)
    m, xd = (w.t() @ w), x
    quad = 1.0 / ((xd @ m) * xd).sum(1).clamp_min(0).sqrt()
    e_quad = float((quad.double() - ref[1]).abs().max())
    print(f"ppt_head ill-conditioned W: collapsed quadratic form inv_norm err {e_quad:.3e} (bound {fig['inv_norm'][2]:.3e})")
    assert e_quad > 10 * fig["inv_norm"][2]
    return fig


def check_zero_row(device):
    """a row with x = 0 and b = 0 under eps = 1e-12: h = 0, logits exactly 0, the gradient that of h / eps (dh = dn / eps), all finite.
    The clamped row's dx (1e12 times the others) is compared at its own scale, the other rows at theirs."""
    n, c, d, k = 70, 32, 64, 5
    x, w, b, e, cot = head_inputs(device, n, c, d, k, 5)
    b = torch.zeros_like(b)
    x[37] = 0
    ref, yard, got = run_all(device, x, w, b, e, cot, 1e-12, torch.float32)
    assert float(got[0][37].abs().max()) == 0.0 and float(got[1][37]) == float(np.float32(1.0) / np.float32(1e-12))
    want = (math.exp(LOGIT_SCALE) * cot[37].double() @ e.double() @ w.double()) / 1e-12
    assert float((got[2][37].double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    live = torch.ones(n, dtype=torch.bool, device=device)
    live[37] = False
    for r in (ref, yard, got):
        assert bool(torch.isfinite(r[2]).all())
    cut = lambda r: [r[0], r[1][live], r[2][live], r[3], r[4]]
    scales = dict(logits=math.exp(LOGIT_SCALE), inv_norm=float(ref[1][live].max()))
    _compare("ppt_head zero row (live rows)", cut(ref), cut(yard), cut(got), scales, 4)
    e_k, e_t = float((got[2][37].double() - ref[2][37]).abs().max()), float((yard[2][37].double() - ref[2][37]).abs().max())
    big = float(ref[2][37].abs().max())
    print(f"ppt_head zero row dx_clamped_row: kernel err {e_k:.3e}  torch fp32 err {e_t:.3e}  scale {big:.3e}")
    assert e_k <= max(4 * e_t, FLOOR_ULPS * ULP * big)


def check_selection(device):
    """v1m1 selects class rows by valid_index, v1m3 by split(num_classes): the same rows give the same bits"""
    n, c, d = 150, 32, 64
    x, w, b, e_all, _ = head_inputs(device, n, c, d, 36, 6)
    cot = torch.randn(n, 13, generator=torch.Generator().manual_seed(7)).to(device)
    by_index = e_all[list(range(5, 18)), :]
    by_split = e_all.split([5, 13, 18])[1]
    a = _run(PF.ppt_head, x, w, b, by_index, cot, 1e-12, use_kernels=True)
    s = _run(PF.ppt_head, x, w, b, by_split, cot, 1e-12, use_kernels=True)
    for u, v in zip(a, s):
        assert torch.equal(u, v)
    scattered = e_all[[0, 1, 4, 5, 6, 7, 8, 10, 19, 29, 30, 31, 32], :]          # S3DIS' valid_index
    got = _run(PF.ppt_head, x, w, b, scattered, cot, 0.0, use_kernels=True)
    ref = _run(PF.ppt_head_torch, x.double(), w.double(), b.double(), scattered.double(), cot.double(), 0.0)
    yard = _run(PF.ppt_head_torch, x, w, b, scattered, cot, 0.0)
    _compare("ppt_head valid_index rows", ref, yard, got, dict(logits=math.exp(LOGIT_SCALE), inv_norm=float(ref[1].max())), 4)


def check_ignored_rows(device):
    """dlogits = 0 on some rows (ignored labels): their dx is exactly 0 and they add exactly 0 to every reduction -- dW and db keep
    their bits when the ignored rows' features are replaced by others"""
    n, c, d, k = 300, 64, 128, 20
    x, w, b, e, cot = head_inputs(device, n, c, d, k, 8)
    dead = torch.rand(n, generator=torch.Generator().manual_seed(9)).to(device) < 0.4
    cot[dead] = 0
    x2 = x.clone()
    x2[dead] = torch.randn(int(dead.sum()), c, generator=torch.Generator().manual_seed(10)).to(device) * 3
    a = _run(PF.ppt_head, x, w, b, e, cot, 1e-12, use_kernels=True)
    s = _run(PF.ppt_head, x2, w, b, e, cot, 1e-12, use_kernels=True)
    assert float(a[2][dead].abs().max()) == 0.0 and float(s[2][dead].abs().max()) == 0.0
    assert torch.equal(a[2], s[2]) and torch.equal(a[3], s[3]) and torch.equal(a[4], s[4])
    assert float(a[3].abs().max()) > 0
    dl = cot.contiguous()
    w32 = w
    G, M, u = e @ w32, w32.double().t() @ w32.double(), w32.double().t() @ b.double()
    r1 = ops.ppt_head_bwd(x, dl, a[0], a[1], G, M, u, d, math.exp(LOGIT_SCALE), 1e-12)
    r2 = ops.ppt_head_bwd(x2, dl, s[0], s[1], G, M, u, d, math.exp(LOGIT_SCALE), 1e-12)
    for p, q in zip(r1, r2):          # dx, A, Bm, v, asum, rsum
        assert torch.equal(p, q)


def check_reproducible(device, n, c, d, k, dtype=torch.float32):
    x, w, b, e, cot = head_inputs(device, n, c, d, k, 11, dtype)
    xin = x.to(dtype)
    a = _run(PF.ppt_head, xin, w, b, e, cot, 1e-12, use_kernels=True)
    s = _run(PF.ppt_head, xin, w, b, e, cot, 1e-12, use_kernels=True)
    for u, v in zip(a, s):
        assert torch.equal(u, v)


def check_refusal(device):
    """C = 40, D = 96, K = 300: supported is 0 and the torch path is taken -- no error, the torch function's bits"""
    for n, c, d, k in ((50, 40, 64, 8), (50, 32, 96, 8), (50, 32, 64, 300)):
        assert not ops.ppt_head_supported(c, d, k, torch.float32)
        x, w, b, e, cot = head_inputs(device, n, c, d, k, 12)
        assert not PF.ppt_head_kernels(x, w, e, True)
        got = _run(PF.ppt_head, x, w, b, e, cot, 1e-12, use_kernels=True)
        tor = _run(PF.ppt_head_torch, x, w, b, e, cot, 1e-12)
        for u, v in zip(got, tor):
            assert torch.equal(u, v)
    assert ops.ppt_head_supported(96, 512, 200, torch.bfloat16) and not ops.ppt_head_supported(96, 512, 20, torch.float64)
    assert not ops.ppt_head_supported(160, 512, 20, torch.float32) and not ops.ppt_head_supported(96, 1088, 20, torch.float32)


def check_logit_scale_grad(device):
    """logit_scale is frozen in the reference; if it requires grad its gradient is (dlogits * logits).sum()"""
    x, w, b, e, cot = head_inputs(device, 90, 32, 64, 7, 13)
    out = []
    for fn, kw in ((PF.ppt_head, dict(use_kernels=True)), (PF.ppt_head_torch, {})):
        ls = torch.tensor(LOGIT_SCALE, device=device, requires_grad=True)
        (fn(x, w, b, e, ls, 1e-12, **kw) * cot).sum().backward()
        out.append(float(ls.grad))
    print("ppt_head d logit_scale: kernel path", out[0], "torch", out[1])
    assert abs(out[0] - out[1]) <= 1e-4 * abs(out[1])


# ---------------------------------------------------------------------------------------------------------------- kernel tests
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,c,d,k", SHAPES)
def test_head_against_float64(n, c, d, k, dtype):
    check_head(dev(), n, c, d, k, dtype, eps=0.0 if k == 25 else 1e-12)


def test_head_f16_against_float64():
    check_head(dev(), 333, 64, 512, 20, torch.float16, eps=1e-6)


def test_ill_conditioned_projection():
    check_ill_conditioned(dev())


def test_zero_row_under_eps():
    check_zero_row(dev())


def test_one_class_only():
    check_head(dev(), 100, 32, 64, 1, torch.float32, eps=1e-12, seed=4)


def test_valid_index_and_split_selection_agree():
    check_selection(dev())


def test_ignored_rows_add_exactly_zero():
    check_ignored_rows(dev())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_reproducible(dtype):
    check_reproducible(dev(), 5000, 96, 512, 20, dtype)


def test_refused_shapes_take_the_torch_path():
    check_refusal(dev())


def test_logit_scale_gradient():
    check_logit_scale_grad(dev())


# ---------------------------------------------------------------------------------------------------------------- models
# tests/golden/make_golden_ppt.py: the reference files' configuration of ppt_tiny.npz
TINY_BACKBONE = dict(type="SpUNet-v1m3", in_channels=6, num_classes=0, base_channels=16, context_channels=256,
                     channels=(16, 32, 48, 64, 64, 48, 32, 32), layers=(1, 2, 1, 1, 1, 1, 2, 1), norm_adaptive=True, norm_affine=True,
                     zero_init=False)
CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
GOLD_CFG = dict(backbone=TINY_BACKBONE, criteria=CRITERIA, backbone_out_channels=32, context_channels=256)
CONDITIONS = {"ScanNet": 20, "S3DIS": 13}
UNUSED = "Structured3D"
NORM_SITE = "backbone.enc.0.block0.bn2"
V1M3_CLASSES = (25, 20, 13)


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppt_tiny.npz"))


def golden_batch(g, device, condition):
    """the fixture's batch, regenerated from its seeds and checked against its checksums; labels modulo the condition's class count"""
    from pointcept_amd import synthetic

    b = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    assert sorted(b) == [str(k) for k in g["input_keys"]]
    assert np.array_equal(np.asarray([float(np.asarray(b[k]).astype(np.float64).sum()) for k in sorted(b)]), g["input_checksum"])
    batch = synthetic.to_torch(b, device)
    seg = batch["segment"]
    batch["segment"] = torch.where(seg >= 0, seg % CONDITIONS[condition], seg)
    batch["condition"] = [condition]
    return batch


def build_model(tag, g, **kw):
    from pointcept_amd import point_prompt_training as P

    if tag == "v1m1":
        return P.PointPromptTraining(**dict(GOLD_CFG, class_embedding=torch.from_numpy(g["class_embedding"]), logit_scale=float(g["logit_scale"]), **kw))
    return P.PointPromptTrainingDecoupled(**dict(GOLD_CFG, **kw))


def golden_state(tag, g, model):
    from oracle.ptv3_model import deterministic_state_dict

    sd = deterministic_state_dict(model, int(g["sd_seed"]))
    own = model.state_dict()
    for k in ("class_embedding", "logit_scale"):
        if k in own:
            sd[k] = own[k].detach().clone()
    assert list(sd.keys()) == [str(k) for k in g[f"{tag}/keys"]]
    assert np.allclose([float(v.double().sum()) for v in sd.values()], g[f"{tag}/sd_checksum"], rtol=0, atol=1e-6)
    return sd


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _model(tag, g, device, **kw):
    torch.manual_seed(0)
    model = build_model(tag, g, **kw)
    model.load_state_dict(golden_state(tag, g, model))
    return model.to(device)


def _train_step(model, batch):
    model.train()
    model.zero_grad(set_to_none=True)
    out = model(dict(batch))
    out["loss"].backward()
    return {k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def check_port_against_golden(device, tags=("v1m1", "v1m2")):
    """PPT-v1m1 / -v1m2 on SpUNet-v1m3 against the reference files' golden, at the fp32 tolerances of the SpUNet golden test that
    test_gpu_cac.py cites (loss 1e-4 relative, stored gradients 2e-3 of their largest element, gradient norms 2e-2 where they are not
    rounding noise, BatchNorm buffers 1e-4 relative, eval logits 1e-4 of their largest element): the train loss, which parameters get
    a gradient, the norms, the stored gradients of the head, the embedding table and one modulation Linear; the BatchNorm buffers of
    the active condition updated and those of an inactive one untouched (bit for bit); the eval loss and logits, with and without labels."""
    g = golden()
    stride = int(g["eval_stride"])
    for tag in tags:
        for cond in CONDITIONS:
            key = f"{tag}/{cond}"
            batch = golden_batch(g, device, cond)
            model = _model(tag, g, device)
            before = {k: v.detach().clone() for k, v in model.state_dict().items()}
            out, grads = _train_step(model, batch)
            assert set(out) == {"loss"}
            ref = float(g[f"{key}/loss"])
            print(f"golden {key} loss: port {float(out['loss']):.8g} reference {ref:.8g}")
            assert abs(float(out["loss"]) - ref) <= 1e-4 * abs(ref), key
            names = [str(k) for k in g[f"{tag}/param_names"]]
            assert names == [k for k, p in model.named_parameters()]
            assert [n for n, h in zip(names, g[f"{key}/has_grad"]) if h] == [n for n in names if n in grads]
            gn = g[f"{key}/grad_norms"]
            norms = np.asarray([float(grads[k].double().norm()) if k in grads else 0.0 for k in names])
            big = gn > 1e-4 * gn.max()
            assert np.allclose(norms[big], gn[big], rtol=2e-2), np.abs(norms[big] / gn[big] - 1).max()
            stored = [k for k in g.files if k.startswith(f"{key}/grad/")]
            assert len(stored) == 5          # the used head's weight + bias, embedding_table, modulation.1 weight + bias of the stored norm site
            for k in stored:
                name = k[len(key) + 6:]
                assert _rel(grads[name], g[k]) < 2e-3, (k, _rel(grads[name], g[k]))
            state = model.state_dict()
            conds = list(model.backbone.conditions)
            used, unused = (f"{NORM_SITE}.bns.{conds.index(c)}." for c in (cond, UNUSED))
            assert int(state[used + "num_batches_tracked"]) == int(g[f"{key}/bn_used/num_batches_tracked"]) == 1
            for buf in ("running_mean", "running_var"):
                assert _rel(state[used + buf], g[f"{key}/bn_used/{buf}"]) <= 1e-4, (key, buf)
                assert not torch.equal(state[used + buf], before[used + buf])
            for k in state:
                if ".bns." in k and f".bns.{conds.index(cond)}." not in k:
                    assert torch.equal(state[k], before[k]), k
            for buf in ("running_mean", "running_var", "num_batches_tracked"):
                assert np.array_equal(state[unused + buf].cpu().numpy(), g[f"{key}/bn_unused/{buf}"])
            model = _model(tag, g, device).eval()
            with torch.no_grad():
                with_labels = model(dict(batch))
                without = model({k: v for k, v in batch.items() if k != "segment"})
            assert set(with_labels) == {"loss", "seg_logits"} and set(without) == {"seg_logits"}
            assert abs(float(with_labels["loss"]) - float(g[f"{key}/eval/loss"])) <= 1e-4 * abs(float(g[f"{key}/eval/loss"]))
            for got in (with_labels["seg_logits"], without["seg_logits"]):
                assert got.shape[1] == CONDITIONS[cond]
                print(f"golden {key} eval logits: relative error {_rel(got[::stride], g[f'{key}/eval/seg_logits']):.3e}")
                assert _rel(got[::stride], g[f"{key}/eval/seg_logits"]) <= 1e-4


def check_v1m3_head_against_golden(device, use_kernels=None):
    """PPT-v1m3's head (split class rows, F.normalize's eps) against the reference expression's float64 golden, fp32 tolerances as above"""
    sys_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    import sys
    sys.path.insert(0, sys_path)
    try:
        import make_golden_ppt as M
    finally:
        sys.path.remove(sys_path)
    g = golden()
    feat, weight, bias, emb, cot = (t.to(device) for t in M.v1m3_inputs())
    feat.requires_grad_(True), weight.requires_grad_(True), bias.requires_grad_(True)
    rows = emb.split(list(V1M3_CLASSES))[1]
    logits = PF.ppt_head(feat, weight, bias, rows, LOGIT_SCALE, 1e-12, use_kernels=use_kernels)
    (logits * cot).sum().backward()
    assert _rel(logits, g["v1m3/logits"]) <= 1e-4
    for got, k in ((feat.grad, "v1m3/dfeat"), (weight.grad, "v1m3/dweight"), (bias.grad, "v1m3/dbias")):
        assert _rel(got, g[k]) < 2e-3, (k, _rel(got, g[k]))


class _PointBackbone(torch.nn.Module):
    """a Point-returning backbone with one pooling level (PT-v3's enc_mode output): the child level's features and its parent"""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(6, 16)

    def forward(self, data_dict):
        from pointcept_amd.structure import Point

        feat = data_dict["feat"]
        n = feat.shape[0]
        inverse = torch.arange(n, device=feat.device) // 2
        child = Point(feat=torch.tanh(self.lin(feat))[: (n + 1) // 2] * 2.0)
        child["pooling_parent"] = Point(feat=torch.tanh(self.lin(feat)))
        child["pooling_inverse"] = inverse
        return child


def check_v1m3_module(device, use_kernels=None):
    """PPT-v1m3: the pooling_parent / pooling_inverse up-cast loop, the split selection, the three return dicts, freeze_backbone,
    backbone_mode; state-dict keys (class_embeddings is not persistent)"""
    from pointcept_amd.point_prompt_training import PointPromptTrainingNeo

    g = torch.Generator().manual_seed(21)
    emb = torch.nn.functional.normalize(torch.randn(sum(V1M3_CLASSES), 64, generator=g), dim=1)
    names = [[f"c{i}_{j}" for j in range(k)] for i, k in enumerate(V1M3_CLASSES)]
    torch.manual_seed(1)
    model = PointPromptTrainingNeo(backbone=_PointBackbone(), criteria=lambda p, t: torch.nn.functional.cross_entropy(p, t, ignore_index=-1),
                                   backbone_out_channels=32, class_names=names, class_embedding=emb, freeze_backbone=True).to(device)
    assert list(model.state_dict().keys()) == ["logit_scale", "backbone.lin.weight", "backbone.lin.bias", "proj_head.weight", "proj_head.bias"]
    assert not any(p.requires_grad for p in model.backbone.parameters()) and not model.logit_scale.requires_grad
    n = 301
    data = dict(feat=torch.randn(n, 6, generator=g).to(device), segment=torch.randint(-1, 20, (n,), generator=g).to(device), condition=["ScanNet"])
    model.train()
    out = model(dict(data))
    assert set(out) == {"loss"}
    out["loss"].backward()
    assert model.proj_head.weight.grad is not None and model.backbone.lin.weight.grad is None
    model.eval()
    with torch.no_grad():
        ev = model(dict(data))
        te = model({k: v for k, v in data.items() if k != "segment"})
        full = torch.tanh(model.backbone.lin(data["feat"]))
        up = torch.cat([full, (full[: (n + 1) // 2] * 2.0)[torch.arange(n, device=device) // 2]], -1)
        want = PF.ppt_head_torch(up, model.proj_head.weight, model.proj_head.bias, model.class_embeddings.split(list(V1M3_CLASSES))[1],
                                 model.logit_scale, 1e-12)
    assert set(ev) == {"loss", "seg_logits"} and set(te) == {"seg_logits"} and ev["seg_logits"].shape == (n, 20)
    assert _rel(ev["seg_logits"], want) <= 1e-5 and torch.equal(ev["seg_logits"], te["seg_logits"])
    model.backbone_mode = True
    with torch.no_grad():
        assert model(dict(data)).shape == (n, 32)


def test_port_matches_reference_golden():
    check_port_against_golden(dev())


def test_v1m3_head_matches_reference_golden():
    check_v1m3_head_against_golden(dev())


def test_v1m3_module():
    check_v1m3_module(dev())


def test_state_dict_keys_are_the_references():
    g = golden()
    for tag in ("v1m1", "v1m2"):
        keys = list(build_model(tag, g).state_dict().keys())
        assert keys == [str(k) for k in g[f"{tag}/keys"]]
        own = [k for k in keys if not k.startswith("backbone.")]
        if tag == "v1m1":
            assert own == ["logit_scale", "class_embedding", "embedding_table.weight", "proj_head.weight", "proj_head.bias"]
        else:
            assert own == ["embedding_table.weight"] + [f"seg_heads.{i}.{p}" for i in range(3) for p in ("weight", "bias")]
        site = [k[len(NORM_SITE) + 1:] for k in keys if k.startswith(NORM_SITE + ".")]
        assert site == [f"bns.{j}.{p}" for j in range(3) for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")] + \
            ["modulation.1.weight", "modulation.1.bias"]


def test_registered_only_when_named():
    from pointcept_amd import compat

    want = {"SpUNet-v1m3": ("sparse_unet_v1m3", "SpUNetV1m3"), "PPT-v1m1": ("point_prompt_training", "PointPromptTraining"),
            "PPT-v1m2": ("point_prompt_training", "PointPromptTrainingDecoupled"), "PPT-v1m3": ("point_prompt_training", "PointPromptTrainingNeo")}
    for name, target in want.items():
        assert name not in compat.MODEL_CLASSES and compat.OPT_IN_MODEL_CLASSES[name] == target

    class _Registry:
        def __init__(self):
            self.got = {}

        def register_module(self, name, force, module):
            self.got[name] = module

    r = _Registry()
    assert sorted(compat.register_models(r)) == sorted(compat.MODEL_CLASSES) and not set(want) & set(r.got)
    assert compat.register_models(r, names=list(want)) == list(want) and r.got["PPT-v1m3"].__name__ == "PointPromptTrainingNeo"


def check_condition_forms(device):
    """`condition` as a list (the collated batch), a tuple or a plain string (spconv_unet_v1m3_pdnorm.py:395-399): the same bits"""
    g = golden()
    batch = golden_batch(g, device, "S3DIS")
    model = _model("v1m1", g, device).eval()
    outs = []
    with torch.no_grad():
        for cond in (["S3DIS"], ("S3DIS",), "S3DIS"):
            outs.append(model(dict(batch, condition=cond))["seg_logits"])
        feats = [model.backbone(dict(batch, condition=cond, context=model.embedding_table.weight[2:3])) for cond in (["S3DIS"], "S3DIS")]
    assert outs[0].shape[1] == 13 and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.equal(feats[0], feats[1])


def test_condition_forms():
    check_condition_forms(dev())


def test_zero_init():
    """the reference's _init_weights: zero_init zeroes every modulation Linear"""
    from pointcept_amd.sparse_unet_v1m3 import PDBatchNorm, SpUNetV1m3

    cfg = {k: v for k, v in TINY_BACKBONE.items() if k != "type"}
    net = SpUNetV1m3(**dict(cfg, zero_init=True, norm_affine=False))
    sites = [m for m in net.modules() if isinstance(m, PDBatchNorm)]
    assert len(sites) == 33 and all(float(m.modulation[1].weight.detach().abs().max()) == 0.0 and float(m.modulation[1].bias.detach().abs().max()) == 0.0 for m in sites)
    assert all(m.bns[0].weight is None for m in sites)
    net = SpUNetV1m3(**cfg)
    assert all(float(m.modulation[1].weight.detach().abs().max()) > 0 for m in net.modules() if isinstance(m, PDBatchNorm))


def test_clip_fallback_and_its_error(monkeypatch):
    """without class_embedding= the classes import `clip` and do what the reference does (a stand-in module here); without the
    package they raise an error that names the argument"""
    import sys

    from pointcept_amd.point_prompt_training import PointPromptTraining, PointPromptTrainingNeo

    sys_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    monkeypatch.syspath_prepend(sys_path)
    import make_golden_ppt as M

    monkeypatch.setitem(sys.modules, "clip", M.clip_standin())
    model = PointPromptTraining(backbone=torch.nn.Identity(), criteria=CRITERIA, backbone_out_channels=32)
    g = golden()
    assert np.array_equal(model.class_embedding.numpy(), g["class_embedding"]) and float(model.logit_scale) == float(np.float32(g["logit_scale"]))
    assert model.proj_head.weight.shape == (M.CLIP_WIDTH, 32) and not model.logit_scale.requires_grad
    neo = PointPromptTrainingNeo(backbone=torch.nn.Identity(), criteria=CRITERIA, backbone_out_channels=32)
    assert neo.class_embeddings.shape == (58, M.CLIP_WIDTH) and neo.num_classes == [25, 20, 13]
    assert "class_embeddings" not in neo.state_dict()
    monkeypatch.setitem(sys.modules, "clip", None)          # `import clip` raises ImportError
    for cls in (PointPromptTraining, PointPromptTrainingNeo):
        with pytest.raises(ImportError, match="class_embedding="):
            cls(backbone=torch.nn.Identity(), criteria=CRITERIA, backbone_out_channels=32)
    assert not hasattr(PointPromptTraining(backbone=torch.nn.Identity(), backbone_mode=True), "proj_head")      # backbone mode needs neither


def test_criteria_are_mapped_or_refused_by_name():
    g = golden()
    with pytest.raises(ValueError, match="FocalLoss"):
        build_model("v1m2", g, criteria=[dict(type="FocalLoss")])
    fn = lambda pred, target: pred.sum() * 0          # noqa: E731
    assert build_model("v1m2", g, criteria=fn).criteria is fn


def test_kernel_path_against_torch_path(monkeypatch):
    """PTC_PPT=0 and the kernel path, one process, the same model and batch: the loss agrees to 1e-5 relative (both legs run the same
    backbone kernels; the head's two forms differ by fp32 rounding); gradients 1e-3 of their largest element"""
    from pointcept_amd import config

    g = golden()
    batch = golden_batch(g, dev(), "ScanNet")
    model = _model("v1m1", g, dev())
    monkeypatch.setattr(config, "PPT_KERNELS", False)
    out_t, grad_t = _train_step(model, batch)
    monkeypatch.setattr(config, "PPT_KERNELS", True)
    assert PF.ppt_head_kernels(torch.zeros(4, 32, device=dev()), model.proj_head.weight, model.class_embedding[:20])
    out_k, grad_k = _train_step(model, batch)
    print("loss: kernel", float(out_k["loss"]), "torch", float(out_t["loss"]))
    assert abs(float(out_k["loss"]) - float(out_t["loss"])) <= 1e-5 * abs(float(out_t["loss"]))
    assert set(grad_k) == set(grad_t)
    for k in grad_k:
        assert _rel(grad_k[k], grad_t[k]) < 1e-3, (k, _rel(grad_k[k], grad_t[k]))


def _close(name, got, ref, rtol, atol):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    bad = (got - ref).abs() > atol + rtol * ref.abs()
    assert not bool(bad.any()), (name, float((got - ref).abs().max()))


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("tail", [False, True])
def test_folded_pdbatchnorm_equals_the_three_step_form(affine, tail):
    """[257, 48]: the fold (gamma' = gamma (1 + scale), beta' = beta (1 + scale) + shift into functional.batch_norm_act, ReLU and the
    residual tail fused) against BatchNorm1d -> * (1 + scale) + shift -> (+ residual) -> ReLU in torch: output, running statistics, and
    the gradients of x, the residual, the context, the modulation Linear and the affine pair, at the fp32 BatchNorm tolerances of
    test_gpu_kernels.py::test_batch_norm_act_train (y 2e-5, running statistics 1e-5, dx 1e-4, parameter gradients 1e-3)"""
    from pointcept_amd import nn as PNN
    from pointcept_amd.sparse_unet_v1m3 import PDBatchNorm

    g = torch.Generator().manual_seed(31 + affine)
    n, c = 257, 48
    torch.manual_seed(2)
    norm = PDBatchNorm(c, context_channels=64, conditions=("A", "B"), decouple=True, adaptive=True, affine=affine).to(dev()).train()
    with torch.no_grad():
        if affine:
            norm.bns[1].weight.copy_(torch.rand(c, generator=g) + 0.5)
            norm.bns[1].bias.copy_(torch.randn(c, generator=g) * 0.3)
    x = (torch.randn(n, c, generator=g) * 2 + 0.7).to(dev())
    res = (torch.randn(n, c, generator=g) * 1.5).to(dev()) if tail else None
    ctx = torch.randn(1, 64, generator=g).to(dev())
    dy = torch.randn(n, c, generator=g).to(dev())
    relu = PNN.ReLU()
    params = list(norm.bns[1].parameters()) + list(norm.modulation.parameters())
    state0 = {k: v.clone() for k, v in norm.state_dict().items()}

    def run(fold):
        norm.load_state_dict(state0)
        norm.zero_grad(set_to_none=True)
        xs = [t.clone().requires_grad_(True) if t is not None else None for t in (x, res, ctx)]
        if fold:
            y = norm(xs[0], "B", xs[2], relu=relu, residual=xs[1])
        else:
            bn = norm.bns[1]
            shift, scale = norm.modulation(xs[2]).chunk(2, dim=1)
            y = torch.nn.functional.batch_norm(xs[0], bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)
            y = y * (1.0 + scale) + shift
            y = torch.relu(y + xs[1] if tail else y)
        y.backward(dy)
        return y.detach(), [t.grad for t in xs if t is not None], [p.grad.clone() for p in params], {k: v.clone() for k, v in norm.state_dict().items()}

    assert norm.bns[1].kernel_path(x, res, need_affine=False)
    y_f, gin_f, gp_f, st_f = run(True)
    y_r, gin_r, gp_r, st_r = run(False)
    _close("y", y_f, y_r, 2e-5, 2e-5)
    for k in ("bns.1.running_mean", "bns.1.running_var"):
        _close(k, st_f[k], st_r[k], 1e-5, 1e-5)
        assert not torch.equal(st_f[k], state0[k])
    assert int(st_f["bns.1.num_batches_tracked"]) == 1 and all(torch.equal(st_f[k], state0[k]) for k in st_f if k.startswith("bns.0."))
    _close("dx", gin_f[0], gin_r[0], 1e-4, 1e-4 * max(float(gin_r[0].abs().max()), 1e-3))
    if tail:
        _close("dres", gin_f[1], gin_r[1], 1e-6, 1e-6)
    for name, a, b in [("dcontext", gin_f[-1], gin_r[-1])] + [(f"dparam{i}", a, b) for i, (a, b) in enumerate(zip(gp_f, gp_r))]:
        _close(name, a, b, 1e-3, 1e-3 * float(b.abs().max()) + 1e-4)


def test_ppt_backbone_mode_under_pointgroup():
    """configs/s3dis/insseg-ppt-v1m1-0-pointgroup-spunet-ft.py: PPT-v1m1 with backbone_mode=True as PG-v1m1's backbone, one forward"""
    from test_gpu_pointgroup import instance_batch

    from pointcept_amd.point_group import PointGroup

    ppt = dict(type="PPT-v1m1", backbone=dict(TINY_BACKBONE), backbone_out_channels=32, context_channels=256,
               conditions=("Structured3D", "ScanNet", "S3DIS"), backbone_mode=True)
    net = PointGroup(backbone=ppt, backbone_out_channels=32, semantic_num_classes=13, semantic_ignore_index=-1, segment_ignore_index=(-1,),
                     instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100,
                     cluster_min_points=50).to(dev()).train()
    batch = instance_batch(dev(), (3000, 2000))
    batch["segment"] = torch.where(batch["segment"] >= 0, batch["segment"] % 13, batch["segment"])
    batch["condition"] = ["S3DIS"]
    out = net(dict(batch))
    assert bool(torch.isfinite(out["loss"]))
    out["loss"].backward()
    assert net.backbone.embedding_table.weight.grad is not None and float(net.backbone.embedding_table.weight.grad[2].abs().max()) > 0
    assert float(net.backbone.embedding_table.weight.grad[:2].abs().max()) == 0.0
