"""-m gpu: the engine's PT-v3m1 (drop-in module level) against
  (a) the golden output of the REFERENCE model (tests/golden/ptv3_tiny.npz, BASELINE config 1),
  (b) the standalone CPU oracle run live on the same seeded inputs, forward AND backward.

Tolerances: index maps bit-exact.  Features: the only lossy step is bf16 attention (the reference
itself rounds qkv and the attention output to bf16, ptv3m1:209,215); engine and oracle agree on
those roundings up to fp32 accumulation order, so logits agree to ~1e-2 of their range.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
TINY = dict(in_channels=6, order=ORDERS, enc_depths=(1, 1, 1, 1, 1), dec_depths=(1, 1, 1, 1),
            enc_patch_size=(1024,) * 5, dec_patch_size=(1024,) * 4, drop_path=0.0, shuffle_orders=False)


def _models(cfg, seed=0):
    from oracle import ptv3_model as om
    from pointcept_amd.point_transformer_v3 import PointTransformerV3

    torch.manual_seed(0)
    orc = om.PointTransformerV3(**cfg)
    eng = PointTransformerV3(**cfg)
    assert list(orc.state_dict().keys()) == list(eng.state_dict().keys())
    for (k, a), (_, b) in zip(orc.state_dict().items(), eng.state_dict().items()):
        assert a.shape == b.shape, k
    sd = om.deterministic_state_dict(orc, seed)
    orc.load_state_dict(sd)
    eng.load_state_dict(sd)
    return orc, eng


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def test_ptv3_tiny_forward_matches_reference_golden_and_oracle(cuda):
    from pointcept_amd import synthetic

    g = np.load(os.path.join(GOLD, "ptv3_tiny.npz"))
    orc, eng = _models(TINY)
    eng = eng.to(cuda).eval()
    orc.eval()
    scene = synthetic.collate([synthetic.indoor_scene(int(g["scene_seed"]), int(g["n_points"]))])
    assert scene["grid_coord"].sum() == g["input_checksum"][0]
    torch.manual_seed(5)
    with torch.no_grad():
        pe = eng(synthetic.to_torch(scene, cuda))
    out = pe.feat.float().cpu().numpy()
    assert np.isfinite(out).all()
    # (a) golden rows produced by the reference model itself
    err = np.abs(out[::16] - g["feat_rows"]).max() / float(g["feat_absmax"])
    assert err < 2e-2, f"engine vs reference golden: rel err {err:.3e}"
    # (b) live oracle: also the integer maps, bit-exact
    torch.manual_seed(5)
    with torch.no_grad():
        po = orc({k: torch.from_numpy(v) for k, v in scene.items()})
    assert _rel(pe.feat, po.feat) < 2e-2
    for key in ("serialized_code", "serialized_order", "serialized_inverse"):
        assert torch.equal(pe[key].cpu(), po[key]), key
    assert pe.serialized_depth == po.serialized_depth
    assert torch.equal(pe.pad.cpu(), po.pad) and torch.equal(pe.unpad.cpu(), po.unpad)
    assert torch.equal(pe.cu_seqlens_key.cpu(), po.cu_seqlens_key)


@pytest.mark.parametrize("amp", [torch.bfloat16, torch.float16])
def test_block_executor_step_is_bit_identical_to_the_composed_step(cuda, monkeypatch, amp):
    """config.EXEC_BLOCK (default on): every PT-v3m1 Block as one C call per direction (csrc/block_exec.hip) against the same
    model with the Blocks composed from ~16 autograd Functions each -- bf16 autocast, drop_path > 0 (the seeded device RNG draws the
    same DropPath masks), ragged two-scene batch: loss and EVERY parameter gradient must be identical (same kernels, same operands,
    same order); and the number of Blocks the executor actually served is checked, so that a silent fall-back cannot pass."""
    from pointcept_amd import config, synthetic
    from pointcept_amd import functional as PF
    from pointcept_amd.segmentor import DefaultSegmentorV2

    cfg = dict(TINY, enc_patch_size=(128,) * 5, dec_patch_size=(128,) * 4, enc_depths=(2, 1, 1, 1, 1), drop_path=0.3)
    _, eng_b = _models(cfg, seed=5)
    torch.manual_seed(1)
    eng = DefaultSegmentorV2(20, 64, eng_b).to(cuda).train()
    batch = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(41, 5000), synthetic.indoor_scene(42, 900)]), cuda)
    calls = {"n": 0}
    real = PF.ptv3_block

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(PF, "ptv3_block", counted)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(config, "EXEC_BLOCK", on)
        calls["n"] = 0
        eng.zero_grad(set_to_none=True)
        for m_ in eng.modules():                                   # same BatchNorm running-statistics start
            if isinstance(m_, torch.nn.BatchNorm1d):
                m_.reset_running_stats()
        torch.manual_seed(9)
        with torch.autocast("cuda", dtype=amp):       # f16 (round 4): the reference's recipe; the attention kernels do the call site's casts
            loss = eng(dict(batch))["loss"]
        (loss * (1024.0 if amp == torch.float16 else 1.0)).backward()       # a fixed loss scale stands in for GradScaler
        res[on] = (float(loss.detach()), {k: p.grad.clone() for k, p in eng.named_parameters()}, calls["n"])
    n_blocks = sum(1 for m_ in eng.modules() if type(m_).__name__ == "Block")
    n_wide = sum(1 for m_ in eng.modules() if type(m_).__name__ == "Block" and m_.channels > 512)   # (round 6: the 512-channel stage too, on gemm3.h)
    assert res[True][2] == n_blocks - n_wide and res[False][2] == 0, (res[True][2], res[False][2], n_blocks, n_wide)
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    for k in res[True][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k


def test_ptv3_attention_dropout_on_the_flash_path(cuda):
    """enable_flash=True with attn_drop > 0 (ptv3m1:212: dropout_p = attn_drop while training): the model constructs, a seeded training
    step is reproducible and differs from the step without dropout, eval mode ignores the dropout, and every gradient is finite."""
    from pointcept_amd import synthetic
    from pointcept_amd.segmentor import DefaultSegmentorV2

    cfg = dict(TINY, enc_patch_size=(128,) * 5, dec_patch_size=(128,) * 4)
    batch = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(51, 3000), synthetic.indoor_scene(52, 700)]), cuda)
    res = {}
    for drop in (0.0, 0.2):
        from pointcept_amd.point_transformer_v3 import PointTransformerV3

        _, eng0 = _models(cfg, seed=3)                                  # (the oracle model has no attention dropout: same weights, engine only)
        eng_b = PointTransformerV3(**dict(cfg, attn_drop=drop))
        eng_b.load_state_dict(eng0.state_dict())
        torch.manual_seed(2)
        eng = DefaultSegmentorV2(20, 64, eng_b).to(cuda)
        eng.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            ev = eng(dict(batch))["loss"]
        eng.train()
        losses = []
        for rep in range(2):
            eng.zero_grad(set_to_none=True)
            for m_ in eng.modules():
                if isinstance(m_, torch.nn.BatchNorm1d):
                    m_.reset_running_stats()
            torch.manual_seed(21)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = eng(dict(batch))["loss"]
            loss.backward()
            losses.append(float(loss.detach()))
            assert all(torch.isfinite(p.grad).all() for p in eng.parameters() if p.grad is not None)
        assert losses[0] == losses[1], losses
        res[drop] = (float(ev), losses[0])
    assert res[0.0][0] == res[0.2][0]            # eval: dropout inactive, identical weights -> identical loss
    assert res[0.0][1] != res[0.2][1] and abs(res[0.0][1] - res[0.2][1]) < 0.5 * abs(res[0.0][1])


def test_ptv3_two_scenes_forward_backward_vs_oracle(cuda):
    """ragged batch (one scene shorter than a patch at deep stages), train mode (BatchNorm batch
    statistics, pooling-order shuffles from the seeded CPU RNG), loss + every parameter gradient."""
    from oracle import ptv3_model as om
    from pointcept_amd import synthetic
    from pointcept_amd.segmentor import DefaultSegmentorV2

    cfg = dict(TINY, enc_patch_size=(128,) * 5, dec_patch_size=(128,) * 4)
    orc_b, eng_b = _models(cfg, seed=3)
    torch.manual_seed(1)
    orc = om.SegmentorV2(20, 64, orc_b)
    eng = DefaultSegmentorV2(20, 64, eng_b)
    eng.seg_head.load_state_dict(orc.seg_head.state_dict())
    eng = eng.to(cuda)
    orc.train()
    eng.train()
    batch = synthetic.collate([synthetic.indoor_scene(21, 2500), synthetic.indoor_scene(22, 700)])
    torch.manual_seed(9)
    lo = orc({k: torch.from_numpy(v) for k, v in batch.items()})["loss"]
    lo.backward()
    torch.manual_seed(9)
    le = eng(synthetic.to_torch(batch, cuda))["loss"]
    le.backward()
    assert abs(le.item() - lo.item()) < 2e-2 * abs(lo.item()), (le.item(), lo.item())
    go = dict(orc.named_parameters())
    rows = []
    for name, p in eng.named_parameters():
        assert p.grad is not None, f"no gradient for {name}"
        assert torch.isfinite(p.grad).all(), name
        r = go[name].grad
        rows.append((name, float((p.grad.cpu() - r).norm()), float(r.norm()), float(r.abs().max())))
    gmax = max(r[3] for r in rows)
    # Parameters whose true gradient is zero (biases feeding a batch-statistics BatchNorm) only carry
    # rounding noise on both sides: compare those absolutely, the rest relatively (Frobenius norm).
    report, bad = [], []
    for name, dn, rn, rmax in rows:
        rel = dn / max(rn, 1e-30)
        report.append(f"{rel:10.3e} {rn:10.3e} {name}")
        if rmax < 1e-5 * gmax:
            if dn > 1e-4 * gmax * max(1.0, float(go[name].numel()) ** 0.5):
                bad.append((name, rel, rn))
        elif rel > 0.1:
            bad.append((name, rel, rn))
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/grad_report.txt", "w") as f:
        f.write("rel_fro_err   ref_norm   parameter\n" + "\n".join(report) + "\n")
    assert not bad, f"gradient mismatch: {bad[:8]}"
    # running statistics of the BatchNorm layers follow the same batch statistics
    for (k, a), (_, b) in zip(eng.backbone.state_dict().items(), orc.backbone.state_dict().items()):
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert _rel(a, b) < 2e-2, k


def test_ptv3_autocast_bf16_close_to_fp32(cuda):
    from pointcept_amd import synthetic

    _, eng = _models(TINY)
    eng = eng.to(cuda).eval()
    scene = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(3, 4096)]), cuda)
    with torch.no_grad():
        torch.manual_seed(5)
        ref = eng(dict(scene)).feat.float()
        torch.manual_seed(5)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp = eng(dict(scene)).feat.float()
    assert torch.isfinite(amp).all()
    assert _rel(amp, ref) < 0.15  # bf16 activations end to end


def test_ptv3_deterministic(cuda):
    """no atomics anywhere: two runs give bit-identical logits and gradients."""
    from pointcept_amd import synthetic
    from pointcept_amd.segmentor import DefaultSegmentorV2

    _, eng_b = _models(dict(TINY, enc_patch_size=(256,) * 5, dec_patch_size=(256,) * 4))
    eng = DefaultSegmentorV2(20, 64, eng_b).to(cuda).train()
    batch = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(5, 3000)]), cuda)
    outs = []
    for _ in range(2):
        eng.zero_grad(set_to_none=True)
        torch.manual_seed(2)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = eng(dict(batch))["loss"]
        loss.backward()
        outs.append((loss.detach().clone(), [p.grad.clone() for p in eng.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)


def test_ptv3_outdoor_depth12_four_channels(cuda):
    """BASELINE configs[4] in small: LiDAR-like sweeps, in_channels = 4 (coord | strength,
    nuscenes/semseg-pt-v3m1-0-base.py:16), grid extent ~2500 voxels => serialization depth 12 (39-bit keys, 5 radix
    passes), very sparse neighbourhoods far from the sensor.  Integer maps bit-exact, features vs the live oracle."""
    from pointcept_amd import synthetic

    cfg = dict(TINY, in_channels=4, enc_patch_size=(256,) * 5, dec_patch_size=(256,) * 4)
    orc, eng = _models(cfg, seed=7)
    eng = eng.to(cuda).eval()
    orc.eval()
    batch = synthetic.collate([synthetic.outdoor_scene(81, 5000), synthetic.outdoor_scene(82, 3000)])
    assert int(batch["grid_coord"].max() + 1).bit_length() == 12
    torch.manual_seed(5)
    with torch.no_grad():
        pe = eng(synthetic.to_torch(batch, cuda))
    torch.manual_seed(5)
    with torch.no_grad():
        po = orc({k: torch.from_numpy(v) for k, v in batch.items()})
    assert pe.serialized_depth == po.serialized_depth == 12
    for key in ("serialized_code", "serialized_order", "serialized_inverse"):
        assert torch.equal(pe[key].cpu(), po[key]), key
    assert torch.isfinite(pe.feat).all()
    assert _rel(pe.feat, po.feat) < 2e-2


def test_ptv3_mix3d_duplicate_voxels(cuda):
    """Mix3D (scannet/semseg-pt-v3m1-0-base.py:6 mix_prob) merges two scenes into one batch item WITHOUT re-voxelising:
    duplicate grid coordinates inside one item are legal input.  Equal keys keep their input order in
    the sorts (stable, App. A.3), the rulebook lets the lowest row win: engine == oracle, maps bit-exact."""
    from oracle import ptv3_model as om
    from pointcept_amd import synthetic
    from pointcept_amd.segmentor import DefaultSegmentorV2

    cfg = dict(TINY, enc_patch_size=(128,) * 5, dec_patch_size=(128,) * 4)
    orc_b, eng_b = _models(cfg, seed=8)
    torch.manual_seed(1)
    orc = om.SegmentorV2(20, 64, orc_b)
    eng = DefaultSegmentorV2(20, 64, eng_b)
    eng.seg_head.load_state_dict(orc.seg_head.state_dict())
    eng = eng.to(cuda).train()
    orc.train()
    a, b = synthetic.indoor_scene(91, 1800), synthetic.indoor_scene(92, 1200)
    mixed = {k: np.concatenate([a[k], b[k]]) for k in a}
    assert len(mixed["grid_coord"]) > len(np.unique(mixed["grid_coord"], axis=0))
    batch = synthetic.collate([mixed, synthetic.indoor_scene(93, 500)])
    torch.manual_seed(9)
    oo = orc({k: torch.from_numpy(v) for k, v in batch.items()})
    oo["loss"].backward()
    torch.manual_seed(9)
    oe = eng(synthetic.to_torch(batch, cuda), return_point=True)
    oe["loss"].backward()
    assert abs(oe["loss"].item() - oo["loss"].item()) < 2e-2 * abs(oo["loss"].item())
    worst = 0.0
    for name, p in eng.named_parameters():
        r = dict(orc.named_parameters())[name].grad
        if float(r.norm()) > 1e-3:
            worst = max(worst, float((p.grad.cpu() - r).norm() / r.norm()))
    assert worst < 0.1, worst


def test_ptv3_fp16_autocast(cuda):
    """the reference trains under fp16 AMP (train.py:202-208; attention itself still runs in bf16, ptv3m1:209)."""
    from pointcept_amd import synthetic
    from pointcept_amd.segmentor import DefaultSegmentorV2

    _, eng_b = _models(dict(TINY, enc_patch_size=(256,) * 5, dec_patch_size=(256,) * 4))
    eng = DefaultSegmentorV2(20, 64, eng_b).to(cuda).train()
    batch = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(5, 3000)]), cuda)
    torch.manual_seed(2)
    ref = eng(dict(batch))["loss"]
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    eng.zero_grad(set_to_none=True)
    torch.manual_seed(2)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = eng(dict(batch))["loss"]
    scaler.scale(loss).backward()
    assert torch.isfinite(loss) and abs(loss.item() - ref.item()) < 5e-2 * abs(ref.item())
    for name, p in eng.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


RPE_CFG = dict(TINY, enc_patch_size=(256,) * 5, dec_patch_size=(256,) * 4, enable_flash=False, enable_rpe=True,
               upcast_attention=True, upcast_softmax=True)


def test_ptv3_dense_rpe_branch_matches_reference_golden_and_oracle(cuda):
    """enable_flash=False + enable_rpe=True (ptv3m1:29-48,173-206).  Patch size = min(smallest scene, 256) at
    every stage (200, 50, ... here), RPE tables receive gradients.  fp32 end to end: 1e-3 of the output range."""
    from pointcept_amd import synthetic

    g = np.load(os.path.join(GOLD, "ptv3_rpe.npz"))
    orc, eng = _models(RPE_CFG, seed=2)
    assert [k for k, _ in eng.named_parameters()] == list(g["param_names"])
    eng = eng.to(cuda)
    batch = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    assert batch["grid_coord"].sum() == g["input_checksum"][0]
    tol = 2e-3 * float(g["feat_absmax"])
    eng.eval()
    torch.manual_seed(5)   # pooling shuffles the order rows with the CPU generator (ptv3m1:408-412); seeds of make_golden.py
    with torch.no_grad():
        out = eng(synthetic.to_torch(batch, cuda)).feat.float().cpu().numpy()
    assert np.abs(out[::4] - g["feat_eval_rows"]).max() <= tol
    eng.train()
    torch.manual_seed(6)
    feat = eng(synthetic.to_torch(batch, cuda)).feat
    loss = feat.float().pow(2).mean()
    loss.backward()
    assert np.abs(feat.detach().float().cpu().numpy()[::4] - g["feat_train_rows"]).max() <= tol
    assert abs(loss.item() - float(g["loss"])) <= 2e-3 * float(g["loss"])
    orc.train()
    torch.manual_seed(6)
    fo = orc({k: torch.from_numpy(v) for k, v in batch.items()}).feat
    fo.pow(2).mean().backward()
    go = dict(orc.named_parameters())
    for name, p in eng.named_parameters():
        r = go[name].grad
        assert p.grad is not None, name
        if float(r.norm()) > 1e-6:
            assert float((p.grad.cpu() - r).norm() / r.norm()) < 2e-2, name
    assert float(eng.dec.dec0.block0.attn.rpe.rpe_table.grad.abs().max()) > 0


PDNORM_CFG = dict(TINY, pdnorm_bn=True, pdnorm_ln=True, pdnorm_decouple=True, pdnorm_adaptive=True,
                  pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D"))


def test_ptv3_pdnorm_ppt_configuration_matches_reference_golden(cuda):
    """The PPT configuration of PT-v3m1 (prompt-driven normalisation, configs/*/semseg-pt-v3m1-*-ppt-*.py) on the GPU against
    the REFERENCE model file's own output (tests/golden/ptv3_pdnorm_tiny.npz, make_golden_pdnorm.py): state-dict keys, eval and
    train features, loss, the gradient norm of every parameter; the norm layers of the conditions that were not selected get
    no gradient on either side."""
    from oracle import ptv3_model as om
    from pointcept_amd import synthetic
    from pointcept_amd.point_transformer_v3 import PointTransformerV3

    g = np.load(os.path.join(GOLD, "ptv3_pdnorm_tiny.npz"))
    torch.manual_seed(0)
    eng = PointTransformerV3(**PDNORM_CFG)
    assert list(eng.state_dict().keys()) == list(g["state_keys"])
    assert [k for k, _ in eng.named_parameters()] == list(g["param_names"])
    eng.load_state_dict(om.deterministic_state_dict(eng, 23))
    eng = eng.to(cuda)
    batch = synthetic.collate([synthetic.indoor_scene(61, 2000), synthetic.indoor_scene(62, 600)])
    assert batch["grid_coord"].sum() == g["input_checksum"][0]

    def inputs():
        d = synthetic.to_torch(batch, cuda)
        d["condition"] = "S3DIS"
        d["context"] = torch.randn(1, 256, generator=torch.Generator().manual_seed(5)).to(cuda)
        return d

    tol = 2e-3 * float(g["feat_absmax"])
    eng.eval()
    torch.manual_seed(5)
    with torch.no_grad():
        out = eng(inputs()).feat.float().cpu().numpy()
    assert np.abs(out[::4] - g["feat_eval_rows"]).max() <= tol
    eng.train()
    torch.manual_seed(6)
    feat = eng(inputs()).feat
    loss = (feat.float() * torch.linspace(-1, 1, feat.shape[1], device=feat.device)).pow(2).mean()
    loss.backward()
    assert np.abs(feat.detach().float().cpu().numpy()[::4] - g["feat_train_rows"]).max() <= tol
    assert abs(loss.item() - float(g["loss"])) <= 2e-3 * float(g["loss"])
    for (name, p), ref in zip(eng.named_parameters(), g["grad_norms"]):
        if ref < 0:
            assert p.grad is None, f"{name}: the reference gives this parameter no gradient"
        else:
            assert p.grad is not None, name
            if ref > 1e-6:
                assert abs(float(p.grad.double().norm()) - ref) <= 3e-2 * ref, (name, float(p.grad.norm()), ref)


@pytest.mark.parametrize("amp", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ptv3_rpe_branch_on_the_kernels_under_autocast(cuda, monkeypatch, amp):
    """A13 under bf16 AND fp16 autocast (the latter is what configs/s3dis/semseg-pt-v3m1-1-rpe.py runs: `_base_/default_runtime.py`
    amp_dtype float16): the RPE branch runs on the window-attention kernels (attention_rpe.h).  Same model, same
    batch, same seeds with the kernels and with the dense torch formulation (PTC_RPE_KERNEL=0 semantics via config): features,
    loss and every gradient (the RPE tables included) agree to bf16 accuracy; both against the fp32 oracle."""
    from pointcept_amd import config, synthetic
    from pointcept_amd import point_transformer_v3 as m

    g = np.load(os.path.join(GOLD, "ptv3_rpe.npz"))
    orc, eng = _models(RPE_CFG, seed=2)
    eng = eng.to(cuda).train()
    batch = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    res = {}
    calls = {"n": 0}
    real = m.PF.attn_rpe_qkvpacked

    def spy(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(m.PF, "attn_rpe_qkvpacked", spy)
    for tag, on in (("kernel", True), ("dense", False)):
        monkeypatch.setattr(config, "RPE_KERNEL", on)
        eng.zero_grad(set_to_none=True)
        torch.manual_seed(6)
        with torch.autocast("cuda", dtype=amp):
            feat = eng(synthetic.to_torch(batch, cuda)).feat
        loss = feat.float().pow(2).mean()
        (loss * 256.0).backward()              # a GradScaler-like factor: fp16 gradients of this tiny model underflow without one
        res[tag] = (feat.detach().float().cpu(), float(loss), {k: p.grad.detach().float().cpu().clone() / 256.0 for k, p in eng.named_parameters()})
    n_rpe_blocks = sum(1 for mod in eng.modules() if isinstance(mod, m.SerializedAttention))
    assert calls["n"] == n_rpe_blocks, (calls, n_rpe_blocks)           # every attention of the kernel run went through the kernels
    fk, fd = res["kernel"][0], res["dense"][0]
    scale = float(fd.abs().max())
    assert float((fk - fd).abs().max()) <= 3e-2 * scale
    assert abs(res["kernel"][1] - res["dense"][1]) <= 2e-2 * abs(res["dense"][1])
    orc.train()
    torch.manual_seed(6)
    fo = orc({k: torch.from_numpy(v) for k, v in batch.items()}).feat
    fo.pow(2).mean().backward()
    go = {k: p.grad for k, p in orc.named_parameters()}
    for name in res["kernel"][2]:
        r = go[name]
        if float(r.norm()) > 1e-6:
            ek = float((res["kernel"][2][name] - r).norm() / r.norm())
            ed = float((res["dense"][2][name] - r).norm() / r.norm())
            # bf16: no worse than the bf16 torch formulation (+3 %).  fp16: the kernels keep bf16 OPERANDS between their f16 load / store
            # paths (8 mantissa bits against the 11 of torch's fp16 matmuls: rounding noise up to 8 x), as the flash branch does
            assert ek <= (2.0 if amp == torch.bfloat16 else 8.0) * ed + 3e-2, (name, ek, ed)
    assert float(res["kernel"][2]["dec.dec0.block0.attn.rpe.rpe_table"].abs().max()) > 0


def test_bench_step_under_ddp_over_rccl_single_rank(cuda, tmp_path):
    """The N > 1 path of bench.py on the one GPU a gpurun box has: PTC_FORCE_DDP=1 initialises the "nccl" (= RCCL) process
    group at world size 1 and wraps the model in DistributedDataParallel (bucket hooks, gradient_as_bucket_view, the
    all-reduce launched on RCCL's stream) around the engine's autograd Functions.  Same seeds with and without the wrapper:
    the loss after the timed steps must be identical (a one-rank all-reduce averages over one rank).  Both runs also write
    --dump-outputs: the seg head's logits, gradients and updated parameters of the last step agree as well."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
           "--points", "20000", "--no-secondary", "--no-cpu-baseline"]
    lines, dumps = {}, {}
    for tag, force in (("ddp", "1"), ("plain", "0")):
        env = dict(os.environ, PTC_FORCE_DDP=force, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT="29531")
        r = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / tag)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[tag] = json.loads(r.stdout.strip().splitlines()[-1])
        dumps[tag] = {f.stem: np.load(f) for f in sorted((tmp_path / tag).glob("*.npy"))}
    assert lines["ddp"]["ddp"] is True and lines["plain"]["ddp"] is False
    assert lines["ddp"]["n_gpus"] == 1 and lines["ddp"]["rccl_ranks"] == 1
    assert lines["ddp"]["config"]["final_loss"] == lines["plain"]["config"]["final_loss"], (lines["ddp"]["config"], lines["plain"]["config"])
    d, p = dumps["ddp"], dumps["plain"]
    assert set(p) == {"loss", "logits", "grad_norm", "grad_sample", "param_sample"}
    assert {k: list(a.shape) for k, a in p.items()} == lines["plain"]["dumped_outputs"]["arrays"]
    assert p["logits"].shape == (min(lines["plain"]["config"]["points_per_gpu"], 1 << 16), 20)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in p.values())
    assert round(float(p["loss"]), 4) == lines["plain"]["config"]["final_loss"]
    for k in p:
        scale = max(float(np.abs(p[k]).max()), 1e-6)
        assert float(np.abs(d[k] - p[k]).max()) <= 1e-2 * scale, (k, float(np.abs(d[k] - p[k]).max()), scale)


def test_ptv3_enable_flash_false_uses_the_shrunk_patch(cuda):
    """enable_flash=False without RPE: same data-dependent patch size (ptv3m1:173-176), served by the window-attention
    kernel (bf16 operands) -- compared with the oracle's dense fp32 branch."""
    from pointcept_amd import synthetic

    cfg = dict(TINY, enc_patch_size=(256,) * 5, dec_patch_size=(256,) * 4, enable_flash=False, upcast_attention=True,
               upcast_softmax=True)
    orc, eng = _models(cfg, seed=3)
    eng = eng.to(cuda).eval()
    orc.eval()
    batch = synthetic.collate([synthetic.indoor_scene(25, 1000), synthetic.indoor_scene(26, 150)])
    with torch.no_grad():
        torch.manual_seed(5)
        pe = eng(synthetic.to_torch(batch, cuda))
        torch.manual_seed(5)
        po = orc({k: torch.from_numpy(v) for k, v in batch.items()})
    assert eng.enc.enc0.block0.attn.patch_size == 150 and eng.dec.dec0.block0.attn.patch_size == 150
    assert torch.equal(pe.pad.cpu(), po.pad) and torch.equal(pe.unpad.cpu(), po.unpad)
    assert _rel(pe.feat, po.feat) < 2e-2


ENC_CFG = dict(in_channels=6, order=ORDERS, enc_depths=(1, 1, 1, 1, 1), enc_channels=(32, 64, 128, 256, 512),
               enc_num_head=(2, 4, 8, 16, 32), enc_patch_size=(128,) * 5, drop_path=0.0, shuffle_orders=False, enc_mode=True)


def test_ptv3_enc_mode_chain_matches_reference_golden_and_oracle(cuda):
    """enc_mode=True: the returned Point carries the pooling_parent / pooling_inverse chain in the CALLER's
    row order; DefaultSegmentorV2 unrolls it (default.py:69-74) into [N, 992] features.  Golden rows of the reference,
    then loss and gradients against the live oracle."""
    from oracle import ptv3_model as om
    from pointcept_amd import synthetic
    from pointcept_amd.segmentor import DefaultSegmentorV2

    g = np.load(os.path.join(GOLD, "ptv3_enc_mode.npz"))
    orc_b, eng_b = _models(ENC_CFG, seed=3)
    torch.manual_seed(1)
    orc = om.SegmentorV2(20, 992, orc_b)
    eng = DefaultSegmentorV2(20, 992, eng_b)
    eng.seg_head.load_state_dict(orc.seg_head.state_dict())
    eng = eng.to(cuda)
    batch = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    assert batch["grid_coord"].sum() == g["input_checksum"][0]
    captured = {}
    eng.seg_head.register_forward_pre_hook(lambda m, inp: captured.__setitem__("feat", inp[0].detach()))
    eng.eval()
    torch.manual_seed(5)
    with torch.no_grad():
        out = eng({k: v for k, v in synthetic.to_torch(batch, cuda).items() if k != "segment"}, return_point=True)
    feat = captured["feat"].float().cpu().numpy()
    assert feat.shape == (int(g["stage_sizes"][0]), 992) and out["seg_logits"].shape == (feat.shape[0], 20)
    assert "pooling_parent" not in out["point"].keys()
    assert np.abs(feat[::32] - g["feat_rows"]).max() <= 2e-2 * float(g["feat_absmax"])
    assert np.allclose(np.linalg.norm(feat.astype(np.float64), axis=0), g["feat_col_norm"], rtol=2e-2, atol=1e-3)
    eng.train()
    orc.train()
    torch.manual_seed(9)
    lo = orc({k: torch.from_numpy(v) for k, v in batch.items()})["loss"]
    lo.backward()
    torch.manual_seed(9)
    le = eng(synthetic.to_torch(batch, cuda))["loss"]
    le.backward()
    assert abs(le.item() - lo.item()) < 2e-2 * abs(lo.item())
    go = dict(orc.named_parameters())
    num = den = 0.0
    rows = []
    for name, p in eng.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        r = go[name].grad
        dn, rn = float((p.grad.cpu() - r).norm()), float(r.norm())
        num, den = num + dn * dn, den + rn * rn
        rows.append((dn / max(rn, 1e-30), rn, name))
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/grad_report_enc_mode.txt", "w") as f:
        f.write("\n".join(f"{a:10.3e} {b:10.3e} {c}" for a, b, c in rows) + "\n")
    # Measured (r01_bc, deterministic kernels): 0.060 for the whole gradient vector, per tensor 0.007 at stage 4 rising to
    # 0.05-0.09 from stage 3 outwards -- the error enters in the backward of the last pooling, whose train-mode BatchNorm
    # normalises over 13 rows (a 1e-3 bf16-attention difference in the activations is divided by a tiny batch variance);
    # seg_head and stage 4 agree to < 1 %.  In decoder mode the skip connections dominate those gradients (1-3 % there).
    # Reproduced WITHOUT the engine: rounding only the attention probabilities to bf16 inside the fp32 CPU oracle (what the
    # MFMA operand is) moves its own gradients by 4-7 % at stages 0-2 and 0.5 % at stage 4 / seg_head -- same profile.
    assert (num / den) ** 0.5 < 0.1, (num / den) ** 0.5
    big = max(r[1] for r in rows)
    assert all(a < 0.2 for a, b, _ in rows if b > 1e-2 * big), [r for r in rows if r[1] > 1e-2 * big and r[0] >= 0.2][:5]


M2_CFG = dict(in_channels=6, order=ORDERS, enc_depths=(1, 1, 1, 2, 1), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
              dec_depths=(1, 1, 1, 1), dec_channels=(64, 64, 128, 256), dec_num_head=(4, 4, 8, 16), enc_patch_size=(128,) * 5,
              dec_patch_size=(128,) * 4, drop_path=0.0, shuffle_orders=False, layer_scale=0.5)   # = tests/golden/make_golden.py M2_CFG


def test_ptv3m2_matches_reference_golden(cuda):
    """the engine's module-level PT-v3m2 (GridPooling / GridUnpooling / LayerScale / Linear stem,
    pointcept_amd/point_transformer_v3m2.py) against tests/golden/ptv3m2_tiny.npz = the REFERENCE's own
    point_transformer_v3m2_sonata.py: state-dict keys, eval features, train-mode loss and every gradient norm."""
    from oracle import ptv3_model as om
    from pointcept_amd import synthetic
    from pointcept_amd.point_transformer_v3m2 import PointTransformerV3 as M2

    g = np.load(os.path.join(GOLD, "ptv3m2_tiny.npz"))
    torch.manual_seed(0)
    eng = M2(**M2_CFG)
    assert list(eng.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    sd = om.deterministic_state_dict(eng, 33)
    assert abs(float(sum(float(v.double().abs().sum()) for v in sd.values())) - float(g["weight_checksum"])) < 1e-6 * float(g["weight_checksum"])
    eng.load_state_dict(sd)
    eng = eng.to(cuda)
    batch = synthetic.collate([synthetic.indoor_scene(int(s), int(n)) for s, n in zip(g["scene_seeds"], g["n_points"])])
    assert batch["grid_coord"].sum() == g["input_checksum"][0]
    inp = synthetic.to_torch(batch, cuda)
    inp["grid_size"] = 0.02
    eng.eval()
    torch.manual_seed(5)
    with torch.no_grad():
        out = eng(dict(inp)).feat.float().cpu().numpy()
    assert np.isfinite(out).all()
    err = np.abs(out[::8] - g["feat_rows"]).max() / float(g["feat_absmax"])
    assert err < 2e-2, f"engine PT-v3m2 vs reference golden: rel err {err:.3e}"
    eng.train()
    torch.manual_seed(5)
    f = eng(dict(inp)).feat
    loss = (f * torch.linspace(-1, 1, f.shape[1], device=f.device)).pow(2).mean()
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) < 2e-2 * abs(float(g["loss"])), (float(loss), float(g["loss"]))
    ref = dict(zip([str(k) for k in g["grad_names"]], g["grad_norms"]))
    gmax = max(ref.values())
    for name, p in eng.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        gn, rn = float(p.grad.norm()), ref[name]
        assert abs(gn - rn) <= 0.1 * rn + 1e-4 * gmax, (name, gn, rn)
