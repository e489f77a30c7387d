"""-m gpu: the context-aware classifier (csrc/cac.hip, pointcept_amd/context_aware_classifier.py).  The check_* bodies take a device;
tests/test_cac_cpu.py runs them on the host emulation at small shapes.

Kernels against float64: every output and gradient of functional.cac_pool_soft / cac_pool_hard / cac_cos_logits / cac_distill is
compared with its *_torch twin (the reference's expression) run in float64.  Tolerance, the rule of check_nce in test_gpu_msc.py, set
before any kernel figure was seen: the error of the same *_torch expression in fp32 on the same inputs and device is measured in the
test; the kernel may have 4 x that error and never less than FLOOR_ULPS = 4 fp32 ulps (4 * 2^-23) of the quantity's scale.  Scales:
  proto (soft, hard)   max |x|: a prototype is a weighted mean of rows of x, the rounding of sum_i w_i x_i / sum_i w_i scales with it
  wsum                 its largest entry (a sum of non-negative weights)
  cosine logits        cos_temp (cos_temp times a dot product of unit vectors)
  distillation loss    max(|loss|, 1)
  every gradient       the largest element of the float64 gradient
Integers (rows past the gate, class counts) are exact.  Every figure is printed before it is asserted.
Measured on the MI355X over the parametrised cases: every quantity meets its bound; the closest is dlogits of the soft pooling with a
one-row scene (K = 24, C = 96: kernel 2.4e-6, torch fp32 6.5e-7, bound 2.6e-6 of a largest element 3.4), where x_i . dproto_k and
proto_k . dproto_k cancel -- the kernel forms the second in double.
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
ONE_SCENE = (600,)
RAGGED = (300, 1, 700, 45)            # a one-row scene; sizes that are no multiple of the 32-row tile; more than one row range


def dev():
    return torch.device("cuda")


def _compare(tag, names, ref, tor, got, scales):
    figures = {}
    for name, r, a, k in zip(names, ref, tor, got):
        big = scales[name] if name in scales else float(r.abs().max())
        e_torch = float((a.double() - r).abs().max()) if r.numel() else 0.0
        e_kernel = float((k.double() - r).abs().max()) if r.numel() else 0.0
        bound = max(4 * e_torch, FLOOR_ULPS * ULP * big)
        figures[name] = (e_kernel, e_torch, bound)
        print(f"{tag} {name}: kernel err {e_kernel:.3e}  torch fp32 err {e_torch:.3e}  bound {bound:.3e}  scale {big:.3e}")
        assert bool(torch.isfinite(k).all()), (tag, name)
    for name, (e_kernel, e_torch, bound) in figures.items():
        assert e_kernel <= bound, (tag, name, e_kernel, e_torch, bound)
    return figures


def _offset(sizes, device):
    return torch.tensor(np.cumsum(sizes), dtype=torch.int64, device=device)


# ---------------------------------------------------------------------------------------------------------------- soft pooling
def soft_inputs(device, sizes, k, c, thresh, seed=0, dead_scene=None, absent=None):
    """x [N, C], logits [N, K] with no row's largest probability within 1e-4 of the threshold (asserted); dead_scene: a scene whose
    rows are all near-uniform (none passes the gate); absent = (scene, class): that class has probability exactly 0 there"""
    g = torch.Generator().manual_seed(seed)
    n = int(sum(sizes))
    x = torch.randn(n, c, generator=g)
    logits = torch.randn(n, k, generator=g) * 3
    ends = np.cumsum(sizes)
    if dead_scene is not None:
        a, b = (0 if dead_scene == 0 else int(ends[dead_scene - 1])), int(ends[dead_scene])
        logits[a:b] *= 0.01
    if absent is not None:
        sc, cls = absent
        a, b = (0 if sc == 0 else int(ends[sc - 1])), int(ends[sc])
        logits[a:b, cls] = -200.0
    if thresh > 0:
        for _ in range(20):
            near = (torch.softmax(logits.double(), 1).max(1)[0] - thresh).abs() < 1e-3
            if not bool(near.any()):
                break
            logits[near] *= 1.37
    pmax = torch.softmax(logits.double(), 1).max(1)[0]
    if thresh > 0:
        assert float((pmax - thresh).abs().min()) > 1e-4
    return x.to(device), logits.to(device), _offset(sizes, device), pmax


def _run_pool_soft(fn, x, logits, offset, thresh, detach, cot):
    a = x.clone().requires_grad_(True)
    l = logits.clone().requires_grad_(not detach)
    proto, wsum, passed = fn(a, l.detach() if detach else l, offset, thresh, 1e-7)
    (proto * cot.to(proto.dtype)).sum().backward()
    out = [proto.detach(), wsum.detach(), a.grad]
    if not detach:
        out.append(l.grad)
    return out, passed


def check_pool_soft(device, sizes, k, c, thresh, detach, seed=0, **kw):
    x, logits, offset, pmax = soft_inputs(device, sizes, k, c, thresh, seed, **kw)
    cot = torch.randn(len(sizes), k, c, generator=torch.Generator().manual_seed(seed + 1)).to(device)
    ref, p_ref = _run_pool_soft(PF.cac_pool_soft_torch, x.double(), logits.double(), offset, thresh, detach, cot)
    tor, _ = _run_pool_soft(PF.cac_pool_soft_torch, x, logits, offset, thresh, detach, cot)
    got, p_got = _run_pool_soft(PF.cac_pool_soft, x, logits, offset, thresh, detach, cot)
    ends = offset.tolist()
    want = [int((pmax[a:b] >= thresh).sum()) if thresh > 0 else b - a for a, b in zip([0] + ends[:-1], ends)]
    assert p_got.tolist() == want == p_ref.tolist(), (p_got.tolist(), want)
    names = ("proto", "wsum", "dx") + (() if detach else ("dlogits",))
    _compare(f"cac_pool_soft sizes={sizes} K={k} C={c} thresh={thresh} detach={detach}", names, ref, tor, got,
             dict(proto=float(x.abs().max()), wsum=float(ref[1].abs().max())))
    return got, p_got


# ---------------------------------------------------------------------------------------------------------------- hard pooling
def hard_inputs(device, n, k, c, seed=0, labels=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g)
    base = torch.randn(k, c, generator=g)
    if labels is None:
        labels = torch.randint(-1, max(k - 2, 1), (n,), generator=g)         # -1 rows; the last classes never occur
    return x.to(device), labels.to(device), base.to(device)


def _run_pool_hard(fn, x, target, base, cot):
    a = x.clone().requires_grad_(True)
    proto, count = fn(a, target, base, 1e-4)
    if proto.requires_grad:
        (proto * cot.to(proto.dtype)).sum().backward()
    return [proto.detach(), a.grad if a.grad is not None else torch.zeros_like(a)], count


def check_pool_hard(device, n, k, c, seed=0, labels=None):
    x, target, base = hard_inputs(device, n, k, c, seed, labels)
    cot = torch.randn(k, c, generator=torch.Generator().manual_seed(seed + 1)).to(device)
    ref, c_ref = _run_pool_hard(PF.cac_pool_hard_torch, x.double(), target, base.double(), cot)
    tor, _ = _run_pool_hard(PF.cac_pool_hard_torch, x, target, base, cot)
    got, c_got = _run_pool_hard(PF.cac_pool_hard, x, target, base, cot)
    assert c_got.dtype == torch.int64 and torch.equal(c_got.cpu(), c_ref.cpu())
    absent = (c_got == 0).cpu()
    assert torch.equal(got[0].cpu()[absent], base.cpu()[absent])             # an absent class keeps its incoming row, bit for bit
    _compare(f"cac_pool_hard N={n} K={k} C={c}", ("proto", "dx"), ref, tor, got, dict(proto=float(max(x.abs().max(), base.abs().max()))))
    return got, c_got


# ---------------------------------------------------------------------------------------------------------------- cosine classifier
def cos_inputs(device, sizes, k, c, seed=0, zero_proto_scene=None):
    g = torch.Generator().manual_seed(seed)
    n = int(sum(sizes))
    x = torch.randn(n, c, generator=g) + 0.3 * torch.randn(1, c, generator=g)
    x[min(5, n - 1)] = 0                                                       # the normalise clamp
    proto = torch.randn(len(sizes), k, c, generator=g)
    if zero_proto_scene is not None:
        proto[zero_proto_scene] = 0
    return x.to(device), proto.to(device), _offset(sizes, device)


def _run_cos(fn, x, proto, offset, cos_temp, cot):
    a, p = x.clone().requires_grad_(True), proto.clone().requires_grad_(True)
    out = fn(a, p, offset, cos_temp)
    (out * cot.to(out.dtype)).sum().backward()
    return [out.detach(), a.grad, p.grad]


def check_cos(device, sizes, k, c, cos_temp=15.0, seed=0, shared=False, **kw):
    x, proto, offset = cos_inputs(device, sizes, k, c, seed, **kw)
    if shared:
        proto, offset = proto[0], None
    cot = torch.randn(x.shape[0], k, generator=torch.Generator().manual_seed(seed + 1)).to(device)
    # the zero row's gradient is cot @ phat / 1e-12: compare the rows that are not clamped at the gradient's own scale, the clamped row at its own
    ref = _run_cos(PF.cac_cos_logits_torch, x.double(), proto.double(), offset, cos_temp, cot)
    tor = _run_cos(PF.cac_cos_logits_torch, x, proto, offset, cos_temp, cot)
    got = _run_cos(PF.cac_cos_logits, x, proto, offset, cos_temp, cot)
    zero = (x == 0).all(1)
    split = lambda r: [r[0], r[1][~zero], r[1][zero], r[2]]
    _compare(f"cac_cos sizes={sizes} K={k} C={c} shared={shared}", ("out", "dx", "dx_clamped_rows", "dproto"), split(ref), split(tor), split(got),
             dict(out=float(cos_temp)))
    return got


# ---------------------------------------------------------------------------------------------------------------- distillation
def distill_inputs(device, n, k, seed=0, labels=None, peaked_class=None):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, k, generator=g) * 4
    soft = torch.randn(n, k, generator=g) * 4
    if labels is None:
        labels = torch.randint(-1, max(k - 2, 1), (n,), generator=g)
    if peaked_class is not None:                # every row of that class: softmax(soft) is one-hot to rounding
        rows = labels == peaked_class
        soft[rows] = 0
        soft[rows, 0] = 200.0
    return pred.to(device), soft.to(device), labels.to(device)


def _run_distill(fn, pred, soft, target, eps):
    p = pred.clone().requires_grad_(True)
    loss = fn(p, soft, target, 0.5, eps)
    if loss.requires_grad:
        loss.backward()
    return [loss.detach().reshape(1), p.grad if p.grad is not None else torch.zeros_like(p)]


def check_distill(device, n, k, eps, seed=0, **kw):
    pred, soft, target = distill_inputs(device, n, k, seed, **kw)
    ref = _run_distill(PF.cac_distill_torch, pred.double(), soft.double(), target, eps)
    tor = _run_distill(PF.cac_distill_torch, pred, soft, target, eps)
    got = _run_distill(PF.cac_distill, pred, soft, target, eps)
    _compare(f"cac_distill N={n} K={k} eps={eps}", ("loss", "dpred"), ref, tor, got, dict(loss=max(float(ref[0].abs()), 1.0)))
    return got


# ---------------------------------------------------------------------------------------------------------------- reproducibility, refusal
def check_reproducible(device, n, k, c):
    sizes = (n // 2, n - n // 2)
    x, logits, offset, _ = soft_inputs(device, sizes, k, c, 0.0, 3)
    cot = torch.randn(2, k, c, generator=torch.Generator().manual_seed(4)).to(device)
    target = torch.randint(-1, k, (n,), generator=torch.Generator().manual_seed(5)).to(device)
    base = torch.randn(k, c, generator=torch.Generator().manual_seed(6)).to(device)
    cotn = torch.randn(n, k, generator=torch.Generator().manual_seed(7)).to(device)

    def once():
        out = _run_pool_soft(PF.cac_pool_soft, x, logits, offset, 0.3, False, cot)[0]
        out += _run_pool_hard(PF.cac_pool_hard, x, target, base, cot[0])[0]
        out += _run_cos(PF.cac_cos_logits, x, cot, offset, 15.0, cotn)
        out += _run_distill(PF.cac_distill, logits, cotn, target, 0.1)
        return out

    a, b = once(), once()
    assert len(a) == 11
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def check_refusal(device):
    from pointcept_amd._lib import PtcoreError

    x20, x32 = torch.randn(50, 20, device=device), torch.randn(50, 32, device=device)
    with pytest.raises(PtcoreError):
        PF.cac_pool_soft(x20, torch.randn(50, 8, device=device), None, 0.0)
    with pytest.raises(PtcoreError):
        PF.cac_pool_soft(x32, torch.randn(50, 300, device=device), None, 0.0)
    with pytest.raises(PtcoreError):
        PF.cac_cos_logits(x20, torch.randn(8, 20, device=device))
    with pytest.raises(PtcoreError):
        PF.cac_pool_hard(x32, torch.zeros(50, dtype=torch.int64, device=device), torch.randn(300, 32, device=device))
    with pytest.raises(PtcoreError):
        PF.cac_distill(torch.randn(50, 300, device=device), torch.randn(50, 300, device=device), torch.zeros(50, dtype=torch.int64, device=device))
    assert not ops.cac_supported(300, 32) and not ops.cac_supported(20, 20) and ops.cac_supported(200, 96)


# ---------------------------------------------------------------------------------------------------------------- kernel tests
@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("thresh", [0.0, 0.75])
@pytest.mark.parametrize("sizes", [ONE_SCENE, RAGGED])
@pytest.mark.parametrize("c", [32, 48, 96])
@pytest.mark.parametrize("k", [2, 20, 24, 200])
def test_pool_soft_against_float64(k, c, sizes, thresh, detach):
    check_pool_soft(dev(), sizes, k, c, thresh, detach)


@pytest.mark.parametrize("c", [32, 48, 96])
@pytest.mark.parametrize("k", [2, 20, 24, 200])
def test_pool_hard_against_float64(k, c):
    check_pool_hard(dev(), 1046, k, c)


@pytest.mark.parametrize("sizes", [ONE_SCENE, RAGGED])
@pytest.mark.parametrize("c", [32, 48, 96])
@pytest.mark.parametrize("k", [2, 20, 24, 200])
def test_cos_against_float64(k, c, sizes):
    check_cos(dev(), sizes, k, c)


@pytest.mark.parametrize("k,c", [(20, 96), (200, 32)])
def test_cos_shared_prototypes(k, c):
    """proto [K, C]: the adaptive branch's one set for every row"""
    check_cos(dev(), ONE_SCENE, k, c, shared=True)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("k", [2, 20, 24, 200])
def test_distill_against_float64(k, eps):
    check_distill(dev(), 1046, k, eps)


def designed(device):
    """the designed cases; each compares with float64 under the same rule and adds what its name says"""
    n, k, c = 200, 24, 32
    # every row ignored
    ignored = torch.full((n,), -1, dtype=torch.int64)
    got, count = check_pool_hard(device, n, k, c, labels=ignored)
    assert int(count.sum()) == 0 and float(got[1].abs().max()) == 0.0
    got = check_distill(device, n, k, 0.0, labels=ignored)
    assert float(got[0]) == 0.0 and float(got[1].abs().max()) == 0.0
    # one class only
    one = torch.full((n,), 3, dtype=torch.int64)
    _, count = check_pool_hard(device, n, k, c, labels=one)
    assert count.tolist() == [0, 0, 0, n] + [0] * (k - 4)
    check_distill(device, n, k, 0.1, labels=one)
    # a class present in one scene and absent (probability exactly 0) in another
    got, _ = check_pool_soft(device, (90, 70), k, c, 0.0, False, absent=(1, 5))
    assert float(got[1][1, 5]) == 0.0 and float(got[0][1, 5].abs().max()) == 0.0 and float(got[1][0, 5]) > 0.0
    # a class all of whose rows carry the smallest entropy weight the expression can give (a one-hot soft row: -log(1 + 1e-4))
    labels = torch.randint(0, 6, (n,), generator=torch.Generator().manual_seed(9))
    labels[:3], labels[3:][labels[3:] == 4] = 4, 2
    check_distill(device, n, k, 0.0, labels=labels, peaked_class=4)
    # a scene in which no row passes the gate: zero prototypes, zero cosines, no NaN in the value or the gradient
    got, passed = check_pool_soft(device, (90, 70), k, c, 0.75, False, dead_scene=1)
    assert passed.tolist()[1] == 0 and passed.tolist()[0] > 0 and float(got[0][1].abs().max()) == 0.0 and float(got[1][1].abs().max()) == 0.0
    got = check_cos(device, (90, 70), k, c, zero_proto_scene=1)
    assert float(got[0][90:].abs().max()) == 0.0


def test_designed_cases():
    designed(dev())


def test_reproducible_at_300k():
    """N = 300 000 rows: every workgroup walks several tiles; every output and gradient of the four Functions twice, equal bits"""
    check_reproducible(dev(), 300000, 20, 96)


def test_refuses_what_it_does_not_implement():
    check_refusal(dev())


# ---------------------------------------------------------------------------------------------------------------- model
TINY_BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, base_channels=16, channels=(16, 32, 48, 64, 64, 48, 32, 32),
                     layers=(1, 2, 1, 1, 1, 1, 2, 1))
CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
GOLD_CFG = dict(num_classes=24, backbone_out_channels=32, backbone=TINY_BACKBONE, criteria=CRITERIA, cos_temp=15, conf_thresh=0.75)
TRAIN_LOSSES = ("loss", "seg_loss", "pre_loss", "pre_self_loss", "kl_loss")
BN = "feat_proj_layer.1."


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cac_tiny.npz"))


def golden_batch(g):
    """the fixture's batch, regenerated from its seeds and checked against its checksums"""
    from pointcept_amd import synthetic

    b = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    assert sorted(b) == [str(k) for k in g["input_keys"]]
    assert np.array_equal(np.asarray([float(np.asarray(b[k]).astype(np.float64).sum()) for k in sorted(b)]), g["input_checksum"])
    return b


def golden_state(g, model):
    from oracle.ptv3_model import deterministic_state_dict

    sd = deterministic_state_dict(model, int(g["sd_seed"]))
    sd["seg_head.weight"] = sd["seg_head.weight"] * float(g["head_scale"])
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert np.allclose([float(v.double().sum()) for v in sd.values()], g["sd_checksum"], rtol=0, atol=1e-9)
    return sd


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _model(g, device, **kw):
    from pointcept_amd.context_aware_classifier import CACSegmentor

    torch.manual_seed(0)
    model = CACSegmentor(**dict(GOLD_CFG, **kw))
    model.load_state_dict(golden_state(g, model))
    return model.to(device)


def _train_step(model, batch):
    model.train()
    model.zero_grad(set_to_none=True)
    out = model(dict(batch))
    out["loss"].backward()
    return {k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def check_port_against_golden(device):
    """the port gives the reference file's integers exactly (rows past the gate per scene, class counts, num_batches_tracked) and its
    losses, gradients and BatchNorm buffers at the fp32 tolerances of the SpUNet golden test (tests/test_gpu_spunet.py, as cited by
    test_gpu_msc.py: loss 1e-4 relative, head gradients 2e-3 of their largest element, gradient norms 2e-2 where they are not rounding
    noise); BatchNorm buffers 1e-4 relative; the eval logits 1e-4 of their largest element, as a loss.  Both detach settings, both eval modes."""
    from pointcept_amd import synthetic

    g = golden()
    batch = synthetic.to_torch(golden_batch(g), device)
    names = [str(k) for k in g["param_names"]]
    for detach in (True, False):
        tag = f"detach{int(detach)}"
        model = _model(g, device, detach_pre_logits=detach)
        out, grads = _train_step(model, batch)
        assert model.last["passed"].tolist() == g["pass_count"].tolist()
        assert model.last["class_count"].tolist() == g["class_count"].tolist() and int((g["class_count"] == 0).sum()) >= 4
        state = model.state_dict()
        assert int(state[BN + "num_batches_tracked"]) == int(g[f"{tag}/bn/{BN}num_batches_tracked"]) == len(g["n_points"]) + 1
        for k in ("running_mean", "running_var"):
            assert _rel(state[BN + k], g[f"{tag}/bn/{BN}{k}"]) <= 1e-4, (k, _rel(state[BN + k], g[f"{tag}/bn/{BN}{k}"]))
        assert set(out) == set(TRAIN_LOSSES)
        for k in TRAIN_LOSSES:
            ref = float(g[f"{tag}/out/{k}"])
            print(f"golden {tag} {k}: port {float(out[k]):.8g} reference {ref:.8g}")
            assert abs(float(out[k]) - ref) <= 1e-4 * abs(ref), (tag, k)
        assert names == [k for k, _ in model.named_parameters()] and set(grads) == set(names)
        norms = np.asarray([float(grads[k].double().norm()) for k in names])
        gn = g[f"{tag}/grad_norms"]
        big = gn > 1e-4 * gn.max()
        assert np.allclose(norms[big], gn[big], rtol=2e-2), np.abs(norms[big] / gn[big] - 1).max()
        heads = [k for k in g.files if k.startswith(f"{tag}/grad/")]
        assert len(heads) == 13
        for k in heads:
            name = k[len(tag) + 6:]
            assert _rel(grads[name], g[k]) < 2e-3, (k, _rel(grads[name], g[k]))
    model = _model(g, device).eval()
    with torch.no_grad():
        with_labels = model(dict(batch))
        without = model({k: v for k, v in batch.items() if k != "segment"})
    assert set(with_labels) == {"loss", "seg_logits"} and set(without) == {"seg_logits"}
    assert abs(float(with_labels["loss"]) - float(g["eval/loss"])) <= 1e-4 * abs(float(g["eval/loss"]))
    assert model.last["passed"].tolist() == g["pass_count_eval"].tolist()
    for got, key in ((with_labels["seg_logits"], "eval/seg_logits"), (without["seg_logits"], "eval/seg_logits_nolabel")):
        print(f"golden {key}: relative error {_rel(got, g[key]):.3e}")
        assert _rel(got, g[key]) <= 1e-4, (key, _rel(got, g[key]))


def test_port_matches_reference_golden():
    check_port_against_golden(dev())


def test_state_dict_keys_are_the_references():
    from pointcept_amd.context_aware_classifier import CACSegmentor

    keys = list(CACSegmentor(**GOLD_CFG).state_dict().keys())
    assert keys == [str(k) for k in golden()["keys"]]
    own = [k for k in keys if not k.startswith("backbone.")]
    assert own == ["seg_head.weight", "seg_head.bias", "proj.0.weight", "proj.2.weight", "proj.2.bias", "apd_proj.0.weight", "apd_proj.2.weight",
                   "apd_proj.2.bias", "feat_proj_layer.0.weight", "feat_proj_layer.1.weight", "feat_proj_layer.1.bias",
                   "feat_proj_layer.1.running_mean", "feat_proj_layer.1.running_var", "feat_proj_layer.1.num_batches_tracked",
                   "feat_proj_layer.3.weight", "feat_proj_layer.3.bias"]


def test_registered_only_when_named():
    from pointcept_amd import compat

    assert "CAC-v1m1" not in compat.MODEL_CLASSES and compat.OPT_IN_MODEL_CLASSES["CAC-v1m1"] == ("context_aware_classifier", "CACSegmentor")


def test_criteria_are_mapped_or_refused_by_name():
    from pointcept_amd.context_aware_classifier import CACSegmentor

    with pytest.raises(ValueError, match="FocalLoss"):
        CACSegmentor(**dict(GOLD_CFG, criteria=[dict(type="FocalLoss")]))
    fn = lambda pred, target: pred.sum() * 0
    assert CACSegmentor(**dict(GOLD_CFG, criteria=fn)).criteria is fn


def test_kernel_path_against_torch_path(monkeypatch):
    """one process, the same model and batch: equal integers; both legs run the same backbone and Linear kernels, so the five losses
    differ by the rounding of the three stages only -- 1e-5 relative, a tenth of the golden's loss tolerance, covers fp32 sums over
    2 400 rows on both sides; gradients 1e-3 of their largest element, the bound of test_gpu_msc.py's kernel-against-torch test"""
    from pointcept_amd import config, synthetic

    g = golden()
    batch = synthetic.to_torch(golden_batch(g), dev())
    model = _model(g, dev())
    monkeypatch.setattr(config, "CAC_KERNELS", False)
    out_t, grad_t = _train_step(model, batch)
    ints_t = {k: v.tolist() for k, v in model.last.items()}
    monkeypatch.setattr(config, "CAC_KERNELS", True)
    out_k, grad_k = _train_step(model, batch)
    assert ints_t == {k: v.tolist() for k, v in model.last.items()}
    for k in TRAIN_LOSSES:
        print(k, float(out_k[k]), float(out_t[k]))
        assert abs(float(out_k[k]) - float(out_t[k])) <= 1e-5 * abs(float(out_t[k])), k
    assert set(grad_k) == set(n for n, _ in model.named_parameters()) == set(grad_t)
    for k in grad_k:
        assert _rel(grad_k[k], grad_t[k]) < 1e-3, (k, _rel(grad_k[k], grad_t[k]))


def test_refused_shape_takes_the_torch_functions():
    """C = 20: the ops raise, the wrapper's three stages run the torch functions"""
    from pointcept_amd.context_aware_classifier import CACSegmentor

    model = CACSegmentor(num_classes=8, backbone_out_channels=20, backbone=torch.nn.Identity(), criteria=CRITERIA, conf_thresh=0.2).to(dev())
    assert not model._kernels(torch.zeros(4, 20, device=dev()))
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(300, 20, generator=g).to(dev())
    target = torch.randint(-1, 8, (300,), generator=g).to(dev())
    offset = torch.tensor([120, 300], device=dev())
    model.train()
    logits = model.seg_head(feat)
    refine = model.post_refine_proto_batch(feat, logits, model.seg_head.weight, offset)
    cac = model.get_adaptive_perspective(feat, target, model.seg_head.weight.detach(), model.seg_head.weight)
    loss = model.criteria(refine, target) + model.get_distill_loss(refine, cac.detach(), target)
    loss.backward()
    assert bool(torch.isfinite(loss)) and refine.shape == (300, 8) and model.seg_head.weight.grad is not None


def test_scannet_shape_step():
    """fp32, 3 scenes x 100 000 points, the ScanNet config's SpUNet, K = 20, C = 96: finite losses, a gradient for every parameter;
    inside the wrapper's three stages no ATen mm / unique and no library GEMM, and at most one device-to-host copy per forward (the
    offsets, for the per-scene BatchNorm)"""
    from torch.profiler import ProfilerActivity, profile

    from pointcept_amd import synthetic
    from pointcept_amd.context_aware_classifier import CACSegmentor

    torch.manual_seed(0)
    model = CACSegmentor(num_classes=20, backbone_out_channels=96, criteria=CRITERIA, conf_thresh=0.75,
                         backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                                       layers=(2, 3, 4, 6, 2, 2, 2, 2))).to(dev()).train()
    batch = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(90 + i, 100000) for i in range(3)]), dev())
    out = model(dict(batch))
    out["loss"].backward()
    for k, v in out.items():
        assert bool(torch.isfinite(v)), k
    assert all(p.grad is not None for p in model.parameters())
    n = int(batch["offset"][-1])
    feat = torch.randn(n, 96, device=dev(), requires_grad=True)
    target, offset = batch["segment"], batch["offset"]
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        logits = model.seg_head(feat)
        refine = model.post_refine_proto_batch(feat, logits, model.seg_head.weight, offset)
        cac = model.get_adaptive_perspective(feat, target, model.seg_head.weight.detach(), model.seg_head.weight)
        kl = model.get_distill_loss(refine, cac.detach(), target)
        (kl + cac.sum() * 0.5).backward()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    for kern in ("cac_pool_fwd_kernel", "cac_cos_fwd_kernel", "cac_distill_fwd_kernel", "cac_pool_bwd_soft_kernel", "cac_cos_bwd_kernel"):
        assert any(kern in k for k in kernels), f"the profiler captured no {kern}"
    bad = [x for x in names if x in ("aten::mm", "aten::unique", "aten::_unique2", "aten::unique_dim", "aten::matmul", "aten::addmm", "aten::bmm")
           or "Cijk" in x or ("gemm" in x.lower() and "gemm3_kernel" not in x)]        # gemm3_kernel: the engine's own wide-contraction Linear
    assert not bad, bad
    d2h = [e.name for e in prof.events() if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name]
    assert len(d2h) <= 1, d2h
