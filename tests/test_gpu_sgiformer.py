"""-m gpu: the SGIFormer decoder kernels (csrc/sgiformer.hip) and the SGIFormer-v1m1 port (pointcept_amd/sgiformer.py).

Kernels: the ragged masked attention against an fp32 torch formulation written here, at the bar tests/test_gpu_kernels.py::
test_attention_fwd_bwd applies to bf16-operand attention against the fp32 oracle (forward rtol 2^-6 + atol 2^-9 max|v|, backward rtol
2^-5 + atol 1e-2 max|grad|, relative Frobenius error 2^-8 / 2^-7; inputs representable in bf16, as there); tail bits of the packed
mask; bit-reproducible backward; peak memory; the integer kernels exactly; the matcher cost against float64 beside the reference's own
fp32 expression.  Model: tests/golden/sgiformer_tiny.npz (the reference's files run unmodified by tests/golden/
make_golden_sgiformer.py) at the tolerances of tests/test_gpu_cac.py's model test.  No test here reads the reference tree.
The check_* functions take the device: tests/test_sgiformer_cpu.py runs them on the host emulation of the kernel sources."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pointcept_amd import functional as PF  # noqa: E402

H, D = 2, 32
ATTN_SHAPES = [((1,), (1,)), ((17,), (31,)), ((48,), (32,)), ((48,), (33,)), ((5,), (65,)), ((400,), (200,)), ((48, 48, 3), (1, 130, 64))]


def dev():
    return torch.device("cuda")


def _close(name, got, ref, rtol, atol):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} out of tolerance, max abs err {float(err.max()):.3g}, ref absmax {float(ref.abs().max()):.3g}"


def _fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


# ------------------------------------------------------------------------------------------------ attention
def attention_oracle(q, k, v, lq, lk, masks):
    """softmax(q k^T / sqrt(D) + mask) v per scene and head in the dtype of q (fp32 / fp64), written out plainly"""
    outs, aq, ak = [], 0, 0
    for i, (nq, nk) in enumerate(zip(lq, lk)):
        s = torch.einsum("qhd,khd->hqk", q[aq:aq + nq], k[ak:ak + nk]) * (q.shape[-1] ** -0.5)
        if masks is not None:
            s = s.masked_fill(masks[i][None], float("-inf"))
        outs.append(torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v[ak:ak + nk]))
        aq, ak = aq + nq, ak + nk
    return torch.cat(outs, 0)


def attention_masks(lq, lk, seed):
    """random masks with every row open somewhere; row 1 of each scene (when it exists) has its single open key in the last,
    partial word -- the last key of the scene"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for a, b in zip(lq, lk):
        m = torch.rand(a, b, generator=g) < 0.6
        m[torch.arange(a), torch.randint(0, b, (a,), generator=g)] = False
        if a > 1:
            m[1] = True
            m[1, b - 1] = False
        out.append(m)
    return out


def attention_inputs(lq, lk, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: (torch.randn(n, H, D, generator=g) * 1.5).to(torch.bfloat16).to(dtype)  # noqa: E731
    return mk(sum(lq)), mk(sum(lk)), mk(sum(lk)), torch.randn(sum(lq), H, D, generator=g).to(torch.bfloat16).to(dtype)


def _run_attention(device, q, k, v, go, lq, lk, mask):
    q, k, v = [t.detach().clone().to(device).requires_grad_() for t in (q, k, v)]
    out = PF.sgi_attention(q, k, v, lq, lk, mask, use_kernels=True)
    out.backward(go.to(device))
    return out.detach(), q.grad, k.grad, v.grad


def check_attention(device, lq, lk, use_mask, dtype=torch.float32):
    q, k, v, go = attention_inputs(lq, lk, sum(lq) + 7 * sum(lk), dtype)
    masks = attention_masks(lq, lk, 3) if use_mask else None
    dmask = None if masks is None else [m.to(device) for m in masks]
    out, dq, dk, dv = _run_attention(device, q, k, v, go, lq, lk, dmask)
    assert out.dtype == dtype and dq.dtype == dtype
    q32, k32, v32 = [t.detach().clone().float().requires_grad_() for t in (q, k, v)]
    ref = attention_oracle(q32, k32, v32, lq, lk, masks)
    ref.backward(go.float())
    vmax = float(v.float().abs().max())
    _close("out", out, ref, 1.0 / 64, 2.0 ** -9 * vmax)
    for name, got, want in (("dq", dq, q32.grad), ("dk", dk, k32.grad), ("dv", dv, v32.grad)):
        _close(name, got, want, 1.0 / 32, 1e-2 * float(want.abs().max()))
    if sum(lq) * sum(lk) >= 256:      # whole-tensor figures need more than a handful of elements
        assert _fro(out, ref) < 2.0 ** -8, _fro(out, ref)
        for got, want in ((dq, q32.grad), (dk, k32.grad), (dv, v32.grad)):
            assert _fro(got, want) < 2.0 ** -7, _fro(got, want)
    # bit-reproducible, forward and backward
    again = _run_attention(device, q, k, v, go, lq, lk, dmask)
    for a, b in zip((out, dq, dk, dv), again):
        assert torch.equal(a, b)
    if use_mask:                      # garbage in the bits past Lk must not matter
        packed = PF.SGIPacked.from_bool(dmask)
        words, at = packed.words.clone(), 0
        for a, b in zip(lq, lk):
            w = (b + 31) // 32
            if b % 32:
                rows = words[at:at + a * w].view(a, w)
                rows[:, -1] |= torch.tensor(-(1 << (b % 32)), dtype=torch.int64).to(torch.int32).to(words.device)
            at += a * w
        assert not torch.equal(words, packed.words) or all(b % 32 == 0 for b in lk)
        dirty = _run_attention(device, q, k, v, go, lq, lk, PF.SGIPacked(words, packed.off, packed.rows, packed.cols))
        for a, b in zip((out, dq, dk, dv), dirty):
            assert torch.equal(a, b)


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("lq,lk", ATTN_SHAPES)
def test_attention_against_fp32(lq, lk, use_mask):
    check_attention(dev(), lq, lk, use_mask)


@pytest.mark.parametrize("lq,lk", [((48,), (33,)), ((48, 48, 3), (1, 130, 64))])
def test_attention_bf16_rows(lq, lk):
    check_attention(dev(), lq, lk, True, torch.bfloat16)


def check_refusal(device):
    """head dims the kernels do not implement are refused by the op and take the torch function in the wrapper"""
    from pointcept_amd import ops
    from pointcept_amd._lib import PtcoreError

    q = torch.randn(6, 2, 16, device=device)
    assert not ops.sgi_attn_supported(16) and not ops.sgi_attn_supported(64) and ops.sgi_attn_supported(32)
    with pytest.raises(PtcoreError):
        ops.sgi_attn_fwd(q, q, q, ops.sgi_cu([6], device), ops.sgi_cu([6], device))
    out = PF.sgi_attention(q, q, q, [6], [6], use_kernels=True)
    assert torch.allclose(out, attention_oracle(q, q, q, [6], [6], None), atol=1e-5)


def test_refuses_other_head_dims():
    check_refusal(dev())


def test_attention_peak_memory():
    """one scene, Lq = Lk = 2048, H = 8, D = 32: forward + backward allocate less beyond their inputs and outputs than the 134 MB of one
    [8, 2048, 2048] fp32 tensor"""
    d = dev()
    L, heads = 2048, 8
    q, k, v = [torch.randn(L, heads, D, device=d, requires_grad=True) for _ in range(3)]
    go = torch.randn(L, heads, D, device=d)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = PF.sgi_attention(q, k, v, [L], [L])
    out.backward(go)
    torch.cuda.synchronize()
    results = sum(t.numel() * t.element_size() for t in (out, q.grad, k.grad, v.grad))
    extra = torch.cuda.max_memory_allocated() - base - results
    print(f"peak beyond inputs and outputs: {extra / 1e6:.2f} MB")
    assert extra < 8 * L * L * 4


# ------------------------------------------------------------------------------------------------ integer kernels
def check_pack_mask(device):
    g = torch.Generator().manual_seed(5)
    for m in (1, 31, 32, 33, 200):
        logits = [torch.randn(6, m, generator=g), torch.randn(3, m + 1, generator=g), torch.randn(1, 70, generator=g)]
        logits[0][2] = -logits[0][2].abs() - 0.01            # a row the rule clears
        logits[0][3] = logits[0][3].abs() + 0.01             # a row with nothing masked
        logits = [x.to(device) for x in logits]
        got = PF.sgi_pack_mask(logits, use_kernels=True)
        want = PF.SGIPacked.from_bool(PF.sgi_pack_mask_torch(logits))
        assert torch.equal(got.words, want.words) and torch.equal(got.off, want.off), m
        assert not got.to_bool()[0][2].any() and not got.to_bool()[0][3].any()


def test_pack_mask_is_the_torch_rule():
    check_pack_mask(dev())


def target_case(device):
    """three scenes: instances 0..3 with -1 points; no instance at all; a superpoint split 50 / 50 between two instances, one wholly
    inside an instance, one shared with -1 points, and an instance id (1) that no point carries"""
    g = torch.Generator().manual_seed(9)
    inst0 = torch.randint(-1, 4, (300,), generator=g)
    sp0 = torch.randint(0, 37, (300,), generator=g)
    sp0[:37] = torch.arange(37)
    inst1 = torch.full((120,), -1)
    sp1 = 37 + torch.arange(120) % 33
    #            sp 0 : 2 + 2          sp 1 : 4 of inst 2     sp 2 : 3 of inst 0 + 2 of -1     sp 3 : -1 only
    inst2 = torch.tensor([0, 0, 2, 2, 2, 2, 2, 2, 0, 0, 0, -1, -1, -1])
    sp2 = 70 + torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3])
    instance = torch.cat([inst0, inst1, inst2])
    sp = torch.cat([sp0, sp1, sp2])
    segment = torch.randint(-1, 12, (instance.numel(),), generator=g)
    offset = torch.tensor([300, 420, 434])
    return [t.to(device) for t in (instance, segment, sp, offset)]


def check_targets(device):
    instance, segment, sp, offset = target_case(device)
    got = PF.sgi_targets(instance, segment, sp, offset, use_kernels=True)
    want = PF.sgi_targets_torch(instance, segment, sp, offset)
    assert [tuple(c.shape) for c in got.counts] == [(4, 37), (0, 33), (3, 4)]
    for a, b in zip(got.counts, want.counts):
        assert a.dtype == torch.int32 and torch.equal(a, b)
    assert torch.equal(got.masks.words, want.masks.words) and torch.equal(got.masks.off, want.masks.off)
    for a, b in zip(got.cls, want.cls):
        assert a.dtype == torch.int64 and torch.equal(a, b)
    m = got.masks.to_bool()[2]
    assert m.tolist() == [[False, False, True, False], [False, False, False, False], [False, True, False, False]]   # 0.5 is not > 0.5
    assert int(got.cls[2][1]) == 0


def test_targets_are_exact():
    check_targets(dev())


# ------------------------------------------------------------------------------------------------ matcher cost
def cost_float64(mask_logits, cls_logits, gt_masks, gt_cls, weights):
    """the reference's expression (loss.py:15-52, :331-384) evaluated in float64"""
    x, t = mask_logits.double(), gt_masks.double()
    softplus = torch.nn.functional.softplus
    pos, neg = softplus(-x), softplus(x)
    bce = (pos @ t.T + neg @ (1 - t).T) / x.shape[1]
    sig = x.sigmoid()
    dice = 1 - (2 * sig @ t.T + 1) / (sig.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)
    return -cls_logits.double().softmax(-1)[:, gt_cls] * weights[0] + bce * weights[1] + dice * weights[2]


def check_match_cost(device, g_n, m, lq=48, c=19, seed=0):
    g = torch.Generator().manual_seed(seed + 13 * g_n + m)
    weights = (0.5, 1.0, 1.0)
    logits = [torch.randn(lq, m, generator=g) * 3, torch.randn(lq, m + 5, generator=g) * 3]
    cls = [torch.randn(lq, c, generator=g), torch.randn(lq, c, generator=g)]
    gts = [torch.rand(g_n, m, generator=g) < 0.3, torch.rand(0, m + 5, generator=g) < 0.3]
    gcl = [torch.randint(0, c - 1, (g_n,), generator=g), torch.zeros(0, dtype=torch.int64)]
    to = lambda xs: [x.to(device) for x in xs]  # noqa: E731
    got = PF.sgi_match_cost(to(logits), to(cls), to(gts), to(gcl), weights, use_kernels=True)
    tor = PF.sgi_match_cost_torch(to(logits), to(cls), to(gts), to(gcl), weights)
    assert got[0].shape == (lq, g_n) and got[1].shape == (lq, 0) and got[0].dtype == torch.float32
    ref = cost_float64(logits[0], cls[0], gts[0], gcl[0], weights)
    e_kernel = float((got[0].double().cpu() - ref).abs().max())
    e_torch = float((tor[0].double().cpu() - ref).abs().max())
    print(f"match cost G={g_n} M={m}: kernel error {e_kernel:.3e}, the fp32 torch expression's {e_torch:.3e}")
    assert e_kernel <= 2 * e_torch + 1e-7, (e_kernel, e_torch)


@pytest.mark.parametrize("m", [1, 33, 200])
@pytest.mark.parametrize("g_n", [1, 7])
def test_match_cost_against_float64(g_n, m):
    check_match_cost(dev(), g_n, m)


def check_match_cost_nonfinite(device):
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(48, 33, generator=g)
    logits[3, 5], logits[7, 0], logits[9, 32] = float("inf"), float("-inf"), float("nan")
    args = ([logits.to(device)], [torch.randn(48, 19, generator=g).to(device)], [(torch.rand(7, 33, generator=g) < 0.3).to(device)],
            [torch.randint(0, 18, (7,), generator=g).to(device)])
    got = PF.sgi_match_cost(*args, use_kernels=True)[0]
    tor = PF.sgi_match_cost_torch(*args)[0]
    for r in (3, 7, 9):
        assert (got[r] == 1e6).all() and (tor[r] == 1e6).all(), r
    keep = torch.ones(48, dtype=torch.bool)
    keep[[3, 7, 9]] = False
    assert torch.isfinite(got[keep]).all() and float((got[keep] - tor[keep]).abs().max()) < 1e-5


def test_match_cost_nonfinite_rows_are_1e6():
    check_match_cost_nonfinite(dev())


# ------------------------------------------------------------------------------------------------ model against the golden
TRAIN_LOSSES = ("loss_cls", "loss_mask", "loss_dice", "loss_score", "loss_seg", "loss_bias", "loss")
BACKBONE = dict(type="PT-v3m1", in_channels=6, order=("z", "z-trans"), stride=(2, 2), enc_depths=(1, 1, 1), enc_channels=(16, 32, 64),
                enc_num_head=(1, 2, 4), enc_patch_size=(64, 64, 64), dec_depths=(1, 1), dec_channels=(32, 32), dec_num_head=(2, 2),
                dec_patch_size=(64, 64), drop_path=0.0, shuffle_orders=False, enable_flash=False, enable_rpe=True,
                upcast_attention=True, upcast_softmax=True)
NUM_CLASSES = 18
DECODER = dict(num_classes=NUM_CLASSES, in_channel=32, dec_num_layer=3, num_sample_query=24, num_learn_query=24, d_model=64, nhead=2,
               hidden_dim=128, dropout=0.0, activation_fn="gelu", attn_mask=True, use_score=False, alpha=0.4)
CRITERIA = dict(matcher=dict(type="HungarianMatcher", costs=[dict(type="QueryClassificationCost", weight=0.5), dict(type="MaskBCECost", weight=1.0),
                                                             dict(type="MaskDiceCost", weight=1.0)]),
                loss_weight=[0.8, 1.0, 1.0, 0.5, 0.4, 0.4], num_classes=NUM_CLASSES, non_object_weight=0.1, fix_dice_loss_weight=False,
                iter_matcher=True, fix_mean_loss=True)
MODEL = dict(topk_insts=60, score_thr=0.0, npoint_thr=20, nms=True, semantic_num_classes=NUM_CLASSES, semantic_ignore_index=-1,
             segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1)


def gold_config(use_score, **kw):
    return dict(MODEL, backbone=dict(BACKBONE), decoder=dict(DECODER, use_score=use_score), criteria=dict(CRITERIA), **kw)


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgiformer_tiny.npz"))


def golden_batch(g, first_only=False):
    """the fixture's batch, regenerated from its seeds and checked against its checksums"""
    from pointcept_amd import synthetic

    n = 1 if first_only else len(g["scene_seeds"])
    b = synthetic.indoor_superpoint_batch([int(s) for s in g["scene_seeds"][:n]], [int(s) for s in g["n_points"][:n]], float(g["cell"]))
    assert sorted(b) == [str(k) for k in g["input_keys"]]
    want = g["eval_checksum"] if first_only else g["input_checksum"]
    assert np.array_equal(np.asarray([float(np.asarray(b[k]).astype(np.float64).sum()) for k in sorted(b)]), want)
    return b


def golden_state(g, model, use_score):
    from oracle.ptv3_model import deterministic_state_dict

    tag = f"score{int(use_score)}"
    sd = deterministic_state_dict(model, int(g["sd_seed"]))
    sd["decoder.x_mask.0.weight"] = sd["decoder.x_mask.0.weight"] * float(g["mask_scale"])
    sd["decoder.out_norm.bias"] = sd["decoder.out_norm.bias"] - float(g["norm_shift"])
    sd["decoder.bias_head.3.bias"] = sd["decoder.bias_head.3.bias"] + torch.from_numpy(g["bias_nudge"]).float()
    assert list(sd.keys()) == [str(k) for k in g[f"{tag}/keys"]]
    assert np.allclose([float(v.double().sum()) for v in sd.values()], g[f"{tag}/sd_checksum"], rtol=0, atol=1e-9)
    return sd


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _model(g, device, use_score):
    from pointcept_amd.sgiformer import SGIFormer

    torch.manual_seed(0)
    model = SGIFormer(**gold_config(use_score))
    model.load_state_dict(golden_state(g, model, use_score), strict=True)
    return model.to(device)


def _train_step(g, model, batch):
    model.train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(int(g["fwd_seed"]))
    out = model(dict(batch))
    out["loss"].backward()
    return {k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _matched(model):
    """the matcher's assignments in the order the reference's matcher is called: level by level (the final level first), the scenes
    with instances in order"""
    out = []
    for level in model.criteria.last_matched:
        for q, o in level:
            if q.numel():
                out.append((q.cpu().numpy(), o.cpu().numpy()))
    return out


def check_port_against_golden(device, use_score):
    """the port gives the reference files' matched indices exactly and their losses, gradients and eval output at the fp32 tolerances of
    tests/test_gpu_cac.py's model test: loss 1e-4 relative, gradients 2e-3 of their largest element and gradient norms 2e-2, both where
    they are not rounding noise (norm above 1e-4 of the largest); eval masks and classes exactly, scores 1e-4 of the largest."""
    from pointcept_amd import synthetic

    g = golden()
    tag = f"score{int(use_score)}"
    batch = synthetic.to_torch(golden_batch(g), device)
    model = _model(g, device, use_score)
    out, grads = _train_step(g, model, batch)
    assert set(out) == set(TRAIN_LOSSES)
    matched = _matched(model)
    n_ref = sum(1 for k in g.files if k.startswith(f"{tag}/matched/") and k.endswith("/query"))
    assert len(matched) == n_ref == 4 * 2
    for j, (q, o) in enumerate(matched):
        assert np.array_equal(q, g[f"{tag}/matched/{j}/query"]) and np.array_equal(o, g[f"{tag}/matched/{j}/object"]), j
    for k in TRAIN_LOSSES:
        ref = float(g[f"{tag}/out/{k}"])
        print(f"golden {tag} {k}: port {float(out[k]):.8g} reference {ref:.8g}")
        assert abs(float(out[k]) - ref) <= 1e-4 * abs(ref), (tag, k, float(out[k]), ref)
    names = [str(k) for k in g[f"{tag}/param_names"]]
    assert names == [k for k, _ in model.named_parameters()]
    gn = g[f"{tag}/grad_norms"]
    assert set(grads) == {n for n, v in zip(names, gn) if v >= 0}
    norms = np.asarray([float(grads[k].double().norm()) if k in grads else -1.0 for k in names])
    big = gn > 1e-4 * gn.max()
    assert np.allclose(norms[big], gn[big], rtol=2e-2), np.abs(norms[big] / gn[big] - 1).max()
    heads = [k for k in g.files if k.startswith(f"{tag}/grad/")]
    assert bool(heads) == (not use_score)
    worst = 0.0
    noise = {n for n, v in zip(names, gn) if v <= 1e-4 * gn.max()}      # e.g. a bias in front of a BatchNorm: zero but for rounding
    for k in heads:
        name = k[len(tag) + 6:]
        if name in noise:
            continue
        worst = max(worst, _rel(grads[name], g[k]))
        assert _rel(grads[name], g[k]) < 2e-3, (k, _rel(grads[name], g[k]))
    print(f"golden {tag}: worst decoder gradient error {worst:.3e} of the largest element")
    # eval: the first scene alone (the reference asserts batch size 1)
    one = synthetic.to_torch(golden_batch(g, first_only=True), device)
    model = _model(g, device, use_score).eval()        # fresh: the train step above has moved the BatchNorm running statistics
    torch.manual_seed(int(g["fwd_seed"]))
    with torch.no_grad():
        ev = model(dict(one))
    assert set(ev) == set(TRAIN_LOSSES) | {"pred_scores", "pred_masks", "pred_classes"}
    assert abs(float(ev["loss"]) - float(g[f"{tag}/eval/loss"])) <= 1e-4 * abs(float(g[f"{tag}/eval/loss"]))
    scores, classes = g[f"{tag}/eval/pred_scores"], g[f"{tag}/eval/pred_classes"]
    masks = np.unpackbits(g[f"{tag}/eval/pred_masks"], axis=1)[:, :ev["pred_masks"].shape[1]].astype(bool)
    assert ev["pred_masks"].shape == masks.shape and ev["pred_scores"].shape == scores.shape
    # instances are identified by (class, mask): equal scores may come out in either order
    key = lambda c, m: (int(c), np.packbits(m).tobytes())  # noqa: E731
    ref_scores = {}
    for c, m, s in zip(classes, masks, scores):
        ref_scores.setdefault(key(c, m), []).append(float(s))
    got_scores = {}
    for c, m, s in zip(ev["pred_classes"], ev["pred_masks"], ev["pred_scores"]):
        got_scores.setdefault(key(c, m), []).append(float(s))
    assert set(ref_scores) == set(got_scores)
    for k in ref_scores:
        assert np.allclose(sorted(got_scores[k]), sorted(ref_scores[k]), rtol=0, atol=1e-4 * float(scores.max())), (got_scores[k], ref_scores[k])
    assert np.all(np.diff(ev["pred_scores"]) <= 0)
    with pytest.raises(AssertionError):
        with torch.no_grad():
            model(dict(batch))            # eval keeps the reference's batch-size-1 assertion


@pytest.mark.parametrize("use_score", [False, True])
def test_port_matches_reference_golden(use_score):
    check_port_against_golden(dev(), use_score)


def test_torch_path_matches_reference_golden(monkeypatch):
    """PTC_SGI=0: the reference's own expression on the same backbone, the same bars"""
    from pointcept_amd import config

    monkeypatch.setattr(config, "SGI_KERNELS", False)
    check_port_against_golden(dev(), False)


def test_golden_assignments_from_kernel_and_torch_costs():
    """linear_sum_assignment on the kernel's and on the torch expression's cost matrices gives the same pairs on the golden scenes"""
    from scipy.optimize import linear_sum_assignment

    from pointcept_amd import synthetic

    g = golden()
    model = _model(g, dev(), False).train()
    batch = synthetic.to_torch(golden_batch(g), dev())
    torch.manual_seed(int(g["fwd_seed"]))
    with torch.no_grad():
        point = model.pool_superpoints(model.backbone(dict(batch)))
        pred = model.decoder(point)
        targets = model.prepare_target(point)["inst_info"]
    for level in [pred] + pred["aux_pred_list"]:
        a = PF.sgi_match_cost(level["mask_list"], level["cls_list"], targets.masks, targets.cls, model.criteria.matcher.weights)
        b = PF.sgi_match_cost_torch(level["mask_list"], level["cls_list"], targets.masks, targets.cls, model.criteria.matcher.weights)
        for x, y in zip(a, b):
            if x.shape[1]:
                p, q = linear_sum_assignment(x.cpu().numpy()), linear_sum_assignment(y.cpu().numpy())
                assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])


def test_bf16_autocast_train_step():
    from pointcept_amd import synthetic

    g = golden()
    model = _model(g, dev(), True).train()
    batch = synthetic.to_torch(golden_batch(g), dev())
    torch.manual_seed(int(g["fwd_seed"]))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(dict(batch))
    out["loss"].backward()
    assert set(out) == set(TRAIN_LOSSES) and all(torch.isfinite(v).all() for v in out.values())
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)


def test_state_dict_round_trip_and_keys():
    from pointcept_amd.sgiformer import SGIFormer

    g = golden()
    for use_score in (False, True):
        model = SGIFormer(**gold_config(use_score))
        keys = list(model.state_dict().keys())
        assert keys == [str(k) for k in g[f"score{int(use_score)}/keys"]]
        other = SGIFormer(**gold_config(use_score))
        other.load_state_dict(model.state_dict(), strict=True)
    for k in ("decoder.cross_attn_layers.0.attn.in_proj_weight", "decoder.cross_attn_layers.0.attn.in_proj_bias",
              "decoder.feat_self_attn_layers.1.attn.out_proj.weight", "decoder.self_attn_layers.2.attn.out_proj.bias", "decoder.sp_pos.gauss_B",
              "decoder.query_learn.weight"):
        assert k in keys, k


def test_registered_only_when_named_and_built_from_a_config():
    from pointcept_amd import compat
    from pointcept_amd.sgiformer import SGIFormer

    assert "SGIFormer-v1m1" not in compat.MODEL_CLASSES and compat.OPT_IN_MODEL_CLASSES["SGIFormer-v1m1"] == ("sgiformer", "SGIFormer")

    class Registry:
        def __init__(self):
            self.table = {}

        def register_module(self, name=None, module=None, force=False):
            self.table[name] = module

    reg = Registry()
    assert compat.register_models(reg, names=["SGIFormer-v1m1"]) == ["SGIFormer-v1m1"] and reg.table["SGIFormer-v1m1"] is SGIFormer
    model = compat.build_backbone(dict(type="SGIFormer-v1m1", **gold_config(False)))
    assert isinstance(model, SGIFormer)


def test_constructor_defaults_are_the_references():
    import inspect

    from pointcept_amd.sgiformer import SGIFormer, SGIFormerDecoder, SGIFormerLoss

    d = {k: v.default for k, v in inspect.signature(SGIFormerDecoder.__init__).parameters.items() if k != "self"}
    assert d == dict(dec_num_layer=3, num_sample_query=200, num_learn_query=200, num_classes=18, in_channel=32, d_model=256, nhead=8,
                     hidden_dim=1024, dropout=0.0, activation_fn="relu", attn_mask=True, use_score=False, alpha=0.4)
    m = {k: v.default for k, v in inspect.signature(SGIFormer.__init__).parameters.items() if k not in ("self", "backbone")}
    assert m == dict(decoder=None, criteria=None, topk_insts=200, score_thr=0.0, npoint_thr=100, sp_score_thr=0.55, nms=True,
                     semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1)
    c = {k: v.default for k, v in inspect.signature(SGIFormerLoss.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert c == dict(fix_mean_loss=False, semantic_ignore_index=-1, loss_cls_type="ce_loss")
