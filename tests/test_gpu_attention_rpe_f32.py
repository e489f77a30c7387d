"""-m gpu: the fp32 RPE window-attention kernels (csrc/attention_rpe_f32.h) -- the reference's dense branch with relative position bias
(ptv3m1:29-48,190-206) in a run without autocast: fp32 q / k / v, logits, bias, softmax, accumulation and outputs.

Kernel level against the reference formulation in float64 on the CPU, window by window; the gradients also at the scale of a mean loss
(dout x 1e-6), where a too coarse fixed point for the table gradient would round every addend away.  Model level: the PT-v3m1 RPE
configuration without autocast runs every SerializedAttention on the kernels and agrees with the torch formulation and the golden."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = [([256, 256], 2, 20), ([1024, 1024, 1024], 4, 32), ([200, 200, 200], 3, 18), ([33], 1, 4), ([1024, 330], 2, 32),
         ([1, 2, 31, 65], 3, 8)]


def rpe_reference(qkv, cu, scale, gc, table, bnd):
    """ptv3m1:29-48,190-206 on the CPU in float64, window by window (the lines of test_gpu_kernels._rpe_reference)."""
    T, _, H, D = qkv.shape
    R = 2 * bnd + 1
    out = torch.zeros(T, H, D, dtype=torch.float64)
    lse = torch.zeros(H, T, dtype=torch.float64)
    for a, b in zip(cu[:-1].tolist(), cu[1:].tolist()):
        if b <= a:
            continue
        q, k, v = (qkv[a:b, j].permute(1, 0, 2) for j in range(3))                  # [H, L, D]
        rel = gc[a:b, None, :].long() - gc[None, a:b, :].long()                     # [L(query), L(key), 3]
        idx = rel.clamp(-bnd, bnd) + bnd + torch.arange(3) * R
        bias = table[idx.reshape(-1)].view(b - a, b - a, 3, H).sum(2).permute(2, 0, 1)
        logits = (q * scale) @ k.transpose(1, 2) + bias
        lse[:, a:b] = torch.logsumexp(logits, dim=-1)
        out[a:b] = (torch.softmax(logits, dim=-1) @ v).permute(1, 0, 2)
    return out, lse


def _inputs(lens, H, bnd):
    g = torch.Generator().manual_seed(sum(lens) + H + bnd)
    T = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    qkv = torch.randn(T, 3, H, 16, generator=g) * 1.2
    gc = torch.randint(0, 3 * bnd, (T, 3), generator=g).to(torch.int32)          # offsets beyond +-bnd get clamped
    gc[::7] += 40000                                                               # large coordinates: 16-bit packing
    table = torch.randn(3 * (2 * bnd + 1), H, generator=g) * 0.5
    dout = torch.randn(T, H, 16, generator=g)
    return cu, qkv, gc, table, dout


def _within(name, got, ref, tol):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} out of tolerance, worst err {float(err.max()):.3g} (tol at worst " \
                          f"{float(torch.as_tensor(tol).expand_as(err).flatten()[int(torch.argmax(err - tol))]):.3g})"


def check_kernels_against_the_float64_reference(dev, lens, H, bnd):
    """Body shared with the CPU tier (tests/test_rpe_f32_emulation_cpu.py runs it with dev = cpu on the host emulation)."""
    from pointcept_amd import functional as PF
    from pointcept_amd import ops

    cu, qkv, gc, table, dout = _inputs(lens, H, bnd)
    scale, L = 0.25, max(lens)
    assert ops.attn_rpe_supported(16, L, bnd, torch.float32)
    args = (cu.to(dev), L, scale)
    out, lse = ops.attn_rpe_fwd(qkv.to(dev), *args, gc.to(dev), table.to(dev), bnd)
    assert out.dtype == torch.float32 and lse.dtype == torch.float32
    q64, t64 = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    ref, ref_lse = rpe_reference(q64, cu, scale, gc, t64, bnd)
    vmax = float(qkv[:, 2].abs().max())
    _within("out", out, ref.detach(), 1e-5 * vmax)
    _within("lse", lse, ref_lse.detach(), 1e-5 * ref_lse.detach().abs().clamp(min=1.0))
    for dscale in (1.0, 1e-6):                   # 1e-6: the per-pair gradients of a mean loss over ~1e5 rows
        do = dout * dscale
        q64.grad, t64.grad = None, None
        ref.backward(do.double(), retain_graph=True)
        dqkv, dtab = ops.attn_rpe_bwd(qkv.to(dev), out, do.to(dev), lse, *args, gc.to(dev), table.to(dev), bnd)
        assert dqkv.dtype == torch.float32 and dtab.dtype == torch.float32
        _within(f"dqkv x{dscale}", dqkv, q64.grad, 1e-4 * float(q64.grad.abs().max()))
        _within(f"d_rpe_table x{dscale}", dtab, t64.grad, 1e-4 * float(t64.grad.abs().max()))
        d2, t2 = ops.attn_rpe_bwd(qkv.to(dev), out, do.to(dev), lse, *args, gc.to(dev), table.to(dev), bnd)
        assert torch.equal(dqkv, d2), "dqkv is not bit-reproducible"
        assert torch.equal(dtab, t2), "the fixed-point table gradient is not bit-reproducible"
    # autograd wrapper: the same kernels
    xq, tq = qkv.to(dev).requires_grad_(True), table.to(dev).requires_grad_(True)
    o = PF.attn_rpe_qkvpacked(xq, cu.to(dev), L, scale, gc.to(dev), tq, bnd)
    assert o.dtype == torch.float32 and torch.equal(o.detach(), out)
    (o * dout.to(dev)).sum().backward()
    dqkv, dtab = ops.attn_rpe_bwd(qkv.to(dev), out, dout.to(dev), lse, *args, gc.to(dev), table.to(dev), bnd)
    assert torch.equal(xq.grad, dqkv)
    assert torch.equal(tq.grad, dtab)


def check_overlong_window_is_poisoned(dev):
    """A window longer than max_seqlen (the LDS images are sized from max_seqlen) comes back as NaN rows, forward and backward; the
    other windows are what they are without it."""
    from pointcept_amd import ops

    g = torch.Generator().manual_seed(5)
    lens, H, bnd = [40, 100, 64], 2, 6                                # max_seqlen = 64: the middle window is too long
    T = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32).to(dev)
    qkv = torch.randn(T, 3, H, 16, generator=g).to(dev)
    gc = torch.randint(0, 20, (T, 3), generator=g).to(torch.int32).to(dev)
    table = (torch.randn(3 * (2 * bnd + 1), H, generator=g) * 0.5).to(dev)
    dout = torch.randn(T, H, 16, generator=g).to(dev)
    out, lse = ops.attn_rpe_fwd(qkv, cu, 64, 0.25, gc, table, bnd)
    assert torch.isnan(out[40:140]).all() and torch.isnan(lse[:, 40:140]).all()
    d, _ = ops.attn_rpe_bwd(qkv, out, dout, lse, cu, 64, 0.25, gc, table, bnd)
    assert torch.isnan(d[40:140]).all()
    keep = torch.cat([torch.arange(0, 40), torch.arange(140, T)]).to(dev)
    cu_ok = torch.tensor([0, 40, 104], dtype=torch.int32).to(dev)
    o2, l2 = ops.attn_rpe_fwd(qkv[keep].contiguous(), cu_ok, 64, 0.25, gc[keep].contiguous(), table, bnd)
    assert torch.equal(out[keep], o2) and torch.equal(lse[:, keep], l2)
    d2, _ = ops.attn_rpe_bwd(qkv[keep].contiguous(), o2, dout[keep].contiguous(), l2, cu_ok, 64, 0.25, gc[keep].contiguous(), table, bnd)
    assert torch.equal(d[keep], d2)


def check_empty_batch(dev):
    from pointcept_amd import ops

    H, bnd = 2, 4
    cu = torch.zeros(1, dtype=torch.int32, device=dev)
    qkv = torch.zeros(0, 3, H, 16, device=dev)
    table = torch.randn(3 * (2 * bnd + 1), H).to(dev)
    gc = torch.zeros(0, 3, dtype=torch.int32, device=dev)
    out, lse = ops.attn_rpe_fwd(qkv, cu, 16, 0.25, gc, table, bnd)
    assert out.shape == (0, H, 16) and lse.shape == (H, 0)
    d, dt = ops.attn_rpe_bwd(qkv, out, out, lse, cu, 16, 0.25, gc, table, bnd)
    assert d.shape == qkv.shape and torch.equal(dt, torch.zeros_like(table))


@pytest.mark.parametrize("lens,H,bnd", CASES, ids=[f"{'-'.join(map(str, c[0]))}_H{c[1]}_b{c[2]}" for c in CASES])
def test_attention_rpe_f32_against_the_float64_reference(cuda, lens, H, bnd):
    check_kernels_against_the_float64_reference(cuda, lens, H, bnd)


def test_attention_rpe_f32_poisons_a_window_longer_than_max_seqlen(cuda):
    check_overlong_window_is_poisoned(cuda)


def test_attention_rpe_f32_empty_batch(cuda):
    check_empty_batch(cuda)


def test_attention_rpe_f32_domain(cuda):
    """fp32 is accepted by the RPE entries only: the other attention entries keep refusing it, fp64 is refused everywhere."""
    from pointcept_amd import functional as PF
    from pointcept_amd import ops
    from pointcept_amd._lib import PtcoreError

    assert ops.attn_rpe_supported(16, 1024, 32, torch.float32)
    assert ops.attn_rpe_supported(16, 1024, 32)
    assert not ops.attn_rpe_supported(16, 1025, 32, torch.float32)
    assert not ops.attn_rpe_supported(18, 256, 8, torch.float32)
    assert not ops.attn_rpe_supported(16, 256, 8, torch.float64)
    cu = torch.tensor([0, 64], dtype=torch.int32, device=cuda)
    qkv = torch.randn(64, 3, 2, 16, device=cuda)
    with pytest.raises(PtcoreError):
        ops.attn_varlen_fwd(qkv, cu, 64, 0.25)
    table = torch.zeros(3 * 9, 2, device=cuda)
    gc = torch.zeros(64, 3, dtype=torch.int32, device=cuda)
    with pytest.raises(PtcoreError):
        PF.attn_rpe_qkvpacked(qkv.double(), cu, 64, 0.25, gc, table, 4)


def test_ptv3_rpe_branch_on_the_fp32_kernels_without_autocast(cuda, monkeypatch):
    """The PT-v3m1 RPE configuration without autocast (Pointcept's tester; `enable_amp = False`), train and eval: every
    SerializedAttention goes through the fp32 kernels; features, loss and every gradient (the RPE tables included) agree with the
    torch formulation (config.RPE_KERNEL = False) and both meet the golden at the bars of the existing fp32 test."""
    from pointcept_amd import config, synthetic
    from pointcept_amd import point_transformer_v3 as m

    from test_gpu_model import RPE_CFG, _models

    g = np.load(os.path.join(GOLD, "ptv3_rpe.npz"))
    _, eng = _models(RPE_CFG, seed=2)
    eng = eng.to(cuda)
    sd = {k: v.clone() for k, v in eng.state_dict().items()}        # each pass starts from it (train mode moves BatchNorm statistics)
    batch = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    tol = 2e-3 * float(g["feat_absmax"])
    calls = []
    real = m.PF.attn_rpe_qkvpacked

    def spy(qkv, *a, **k):
        calls.append(qkv.dtype)
        return real(qkv, *a, **k)

    monkeypatch.setattr(m.PF, "attn_rpe_qkvpacked", spy)
    n_attn = sum(1 for mod in eng.modules() if isinstance(mod, m.SerializedAttention))
    res = {}
    for tag, on in (("kernel", True), ("torch", False)):
        monkeypatch.setattr(config, "RPE_KERNEL", on)
        eng.load_state_dict(sd)
        calls.clear()
        eng.eval()
        torch.manual_seed(5)
        with torch.no_grad():
            fe = eng(synthetic.to_torch(batch, cuda)).feat
        assert fe.dtype == torch.float32
        assert calls == ([torch.float32] * n_attn if on else []), (tag, calls, n_attn)
        fe = fe.cpu()
        assert np.abs(fe.numpy()[::4] - g["feat_eval_rows"]).max() <= tol, tag
        eng.train()
        eng.zero_grad(set_to_none=True)
        calls.clear()
        torch.manual_seed(6)
        feat = eng(synthetic.to_torch(batch, cuda)).feat
        loss = feat.pow(2).mean()
        loss.backward()
        loss = loss.detach()
        assert calls == ([torch.float32] * n_attn if on else []), (tag, calls, n_attn)
        assert np.abs(feat.detach().cpu().numpy()[::4] - g["feat_train_rows"]).max() <= tol, tag
        assert abs(loss.item() - float(g["loss"])) <= 2e-3 * float(g["loss"]), tag
        res[tag] = (fe, feat.detach().cpu(), float(loss), {k: p.grad.detach().cpu().clone() for k, p in eng.named_parameters()})
    for i in (0, 1):
        fk, ft = res["kernel"][i], res["torch"][i]
        assert float((fk - ft).abs().max()) <= 1e-4 * float(ft.max() - ft.min())
    assert abs(res["kernel"][2] - res["torch"][2]) <= 1e-4 * abs(res["torch"][2])
    bad = []
    for name, gt in res["torch"][3].items():
        gk = res["kernel"][3][name]
        if float(gt.norm()) > 1e-6:          # (as test_gpu_model: below that a gradient is rounding noise, e.g. biases in front of a norm)
            err = float((gk - gt).norm() / gt.norm())
            if not err < 1e-3:
                bad.append((name, err))
    assert not bad, bad
    assert float(res["kernel"][3]["dec.dec0.block0.attn.rpe.rpe_table"].abs().max()) > 0


def test_attention_rpe_f32_memory_is_not_quadratic(cuda):
    """64 windows x 1024 x 4 heads under no_grad: the kernel path's peak allocation above its inputs and outputs stays below 64 MB
    (the torch formulation's [P, H, K, K] fp32 logits alone are 1 GB)."""
    from pointcept_amd import functional as PF

    P, K, H, bnd = 64, 1024, 4, 32
    g = torch.Generator().manual_seed(1)
    cu = (torch.arange(P + 1, dtype=torch.int32) * K).to(cuda)
    qkv = torch.randn(P * K, 3, H, 16, generator=g).to(cuda)
    gc = torch.randint(0, 100, (P * K, 3), generator=g).to(torch.int32).to(cuda)
    table = torch.randn(3 * (2 * bnd + 1), H, generator=g).to(cuda)
    out_bytes = P * K * H * 16 * 4
    with torch.no_grad():
        PF.attn_rpe_qkvpacked(qkv, cu, K, 0.25, gc, table, bnd)          # warm: library load, workspace caches
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = PF.attn_rpe_qkvpacked(qkv, cu, K, 0.25, gc, table, bnd)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
    assert torch.isfinite(out).all()
    extra = peak - base - out_bytes
    assert extra < 64 * 2 ** 20, extra
