"""-m gpu: Sonata-v1m1 (csrc/sonata.hip, pointcept_amd/sonata.py).  The check_* bodies take a device; tests/test_sonata_cpu.py runs
them on the host emulation at small shapes.

Distillation loss: loss and d loss / d student_sim of functional.sonata_distill, and the Sinkhorn scaling vectors a / b of the pass-level
ops, against float64.  Tolerance (the rule of tests/test_gpu_msc.py, set before any kernel figure was seen): the error of the
reference's own fp32 torch expression (functional.sonata_distill_torch; for a / b the scaling iteration written in torch) against the
same expression in float64 on the same inputs -- the upcast values for 16-bit inputs -- is measured in the test; the kernel may have
4 x that error, and never less than FLOOR_ULPS = 4 fp32 ulps (4 * 2^-23) of the scale of the quantity compared: max(|loss|,
1 / student_temp) for the loss (a mean of lse_i - sum_k target_ik s_ik / student_temp, terms of that size), the largest float64 element
for dpred and for a / b.  A 16-bit student receives its gradient in its own dtype: that output rounding, half a 16-bit ulp (2^-8 for
bf16, 2^-11 for fp16) of the largest element, is added to the bound of dpred and of nothing else.  Every figure is printed before it is
asserted.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pointcept_amd import functional as PF  # noqa: E402
from pointcept_amd import ops  # noqa: E402
from pointcept_amd._lib import PtcoreError  # noqa: E402

FLOOR_ULPS = 4
ULP = 2.0 ** -23
STUDENT_TEMP = 0.1
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # 7 / 10 stored significand bits
# scenes of the designed batch: 0, 1 and 3 hold pairs, 2 (in the middle) and 4 (at the end) hold none -> the divisor is 4
SCENES, MATCHED_SCENES, DIVISOR = 5, (0, 1, 3), 4


def dev():
    return torch.device("cuda")


def distill_inputs(device, m, k, dtype=torch.float32, seed=0, scenes=SCENES, matched=MATCHED_SCENES):
    """(teacher_sim [nt, K], student_sim [ns, K], match_index [m, 2], student_batch [ns]): cosine-like logits in [-1, 1]; teacher
    rows drawn with repetition from half as many rows; student rows a sorted subset of the rows of the `matched` scenes, so that
    unmatched student rows and scenes without pairs exist.  With m < len(matched) the first scenes stay empty."""
    g = torch.Generator().manual_seed(seed * 7919 + m * 31 + k)
    nt = max(m // 2 + 3, 4)
    per = max(-(-2 * m // len(matched)), 3)                      # student rows per scene
    ns = per * scenes
    batch = torch.arange(scenes).repeat_interleave(per)
    teacher = (torch.rand(nt, k, generator=g) * 2 - 1).to(dtype)
    student = (torch.rand(ns, k, generator=g) * 2 - 1).to(dtype)
    pool = torch.cat([torch.arange(s * per, (s + 1) * per) for s in matched])
    rows = pool[torch.randperm(pool.numel(), generator=g)[:m]].sort().values
    trow = torch.randint(nt, (m,), generator=g)
    if m >= 3:
        trow[2] = trow[0]                                            # a teacher row matched several times
    mi = torch.stack([rows, trow], 1)
    return teacher.to(device), student.to(device), mi.to(device), batch.to(device)


def _up(x, dtype):
    """the values the kernel reads, in the reference's dtype"""
    return x.float().to(dtype)


def _run(fn, teacher, student, mi, batch, tt, **kw):
    s = student.clone().requires_grad_(True)
    loss = fn(teacher, s, mi, batch, tt, STUDENT_TEMP, **kw)
    loss.backward()
    return loss.detach(), s.grad


_REFS = {}


def references(device, m, k, tt, dtype, seed=0):
    """inputs, and the torch expression in float64 and in fp32 on them: computed once per shape and left unchanged"""
    key = (str(device), m, k, tt, dtype, seed)
    if key not in _REFS:
        inp = distill_inputs(device, m, k, dtype, seed)
        t, s, mi, sb = inp
        ref = _run(PF.sonata_distill_torch, _up(t, torch.float64), _up(s, torch.float64), mi, sb, tt)
        tor = _run(PF.sonata_distill_torch, _up(t, torch.float32), _up(s, torch.float32), mi, sb, tt)
        _REFS[key] = (inp, ref, tor)
    return _REFS[key]


def bounds(ref, tor, dtype):
    """{name: (torch fp32 error, bound, scale)} for the loss and dpred"""
    out = {}
    for name, r, a in zip(("loss", "dpred"), ref, tor):
        scale = max(float(r.abs()), 1.0 / STUDENT_TEMP) if name == "loss" else float(r.abs().max())
        e_torch = float((a.double() - r).abs().max())
        extra = HALF_ULP[dtype] * scale if name == "dpred" else 0.0
        out[name] = (e_torch, max(4 * e_torch, FLOOR_ULPS * ULP * scale) + extra, scale)
    return out


def assert_close(tag, got, ref, bnd):
    figures = {}
    for name, k_, r in zip(("loss", "dpred"), got, ref):
        e_torch, bound, scale = bnd[name]
        e_kernel = float((k_.double() - r).abs().max())
        figures[name] = (e_kernel, e_torch, bound)
        print(f"sonata_distill {tag} {name}: kernel err {e_kernel:.3e}  torch fp32 err {e_torch:.3e}  bound {bound:.3e}  scale {scale:.3e}")
    for name, (e_kernel, e_torch, bound) in figures.items():
        assert e_kernel <= bound, (tag, name, e_kernel, e_torch, bound)
    return figures


def check_distill(device, m, k, tt, dtype, caps=(1, 3, 0)):
    (t, s, mi, sb), ref, tor = references(device, m, k, tt, dtype)
    if m >= 3:
        assert mi[:, 1].unique().numel() < m                         # teacher rows matched several times
    bnd = bounds(ref, tor, dtype)
    matched = torch.zeros(s.shape[0], dtype=torch.bool, device=device)
    matched[mi[:, 0]] = True
    for cap in caps:
        got = _run(PF.sonata_distill, t, s, mi, sb, tt, num_scenes=SCENES, max_groups=cap, use_kernels=True)
        assert got[0].dtype == torch.float32 and got[1].dtype == dtype
        assert_close(f"M={m} K={k} temp={tt} {str(dtype)[6:]} cap={cap}", got, ref, bnd)
        assert not bool(got[1][~matched].any())                      # unmatched student rows: exactly zero
        assert bool(torch.isfinite(got[1]).all())


def scaling_iteration(t, mi, tt, num_iter, dtype):
    """the Sinkhorn iteration on scaling vectors written in torch: (a after num_iter column normalisations, b after num_iter - 1 row
    normalisations, c of the last of them)"""
    e = torch.exp(t.float().to(dtype)[mi[:, 1]] / tt)
    n, k = e.shape
    b = torch.ones(n, dtype=dtype, device=t.device)
    c = None
    for it in range(num_iter):
        a = 1.0 / (k * (e * b[:, None]).sum(0))
        if it + 1 < num_iter:
            c = (e * a[None, :]).sum(1)
            b = 1.0 / (n * c)
    return a, b, c


def check_scaling_vectors(device, m, k, tt, dtype, cap):
    """the pass-level ops: a after three iterations and b after two, against the float64 iteration"""
    t, s, mi, sb = distill_inputs(device, m, k, dtype, seed=1)
    a64, b64, _ = scaling_iteration(t, mi, tt, 3, torch.float64)
    a32, b32, _ = scaling_iteration(t, mi, tt, 3, torch.float32)
    r = ops.sonata_colsum(t, mi, tt, None, cap)
    a = torch.reciprocal(r * k)
    c, b, r = ops.sonata_rowpass(t, mi, tt, a, m, True, cap)
    assert torch.equal(r, ops.sonata_colsum(t, mi, tt, b, cap))      # the fused column sums are the stand-alone pass's, bit for bit
    a = torch.reciprocal(r * k)
    c, b, r = ops.sonata_rowpass(t, mi, tt, a, m, True, cap)
    c2, b2, none = ops.sonata_rowpass(t, mi, tt, a, m, False, cap)
    assert none is None and torch.equal(c, c2) and torch.equal(b, b2)
    a = torch.reciprocal(r * k)
    assert torch.equal(a, PF.sonata_sinkhorn_scales(t, mi, tt, 3, None, cap))
    figures = {}
    for name, got, r64, r32 in (("a", a, a64, a32), ("b", b, b64, b32)):
        scale = float(r64.abs().max())
        e_torch = float((r32.double() - r64).abs().max())
        e_kernel = float((got.double() - r64).abs().max())
        bound = max(4 * e_torch, FLOOR_ULPS * ULP * scale)
        figures[name] = (e_kernel, bound)
        print(f"sonata scaling M={m} K={k} temp={tt} {str(dtype)[6:]} cap={cap} {name}: kernel err {e_kernel:.3e}  torch fp32 err {e_torch:.3e}  "
              f"bound {bound:.3e}  scale {scale:.3e}")
    for name, (e_kernel, bound) in figures.items():
        assert e_kernel <= bound, (name, e_kernel, bound)


def check_divisor(device):
    """the torch side against a hand-written expectation: scenes 2 and 4 hold no pairs; scene 2 counts as a zero, scene 4 does not
    count -- and the kernels agree with it"""
    m, k, tt = 40, 64, 0.07
    (t, s, mi, sb), ref, tor = references(device, m, k, tt, torch.float32)
    scene = sb[mi[:, 0]]
    assert sorted(scene.unique().tolist()) == list(MATCHED_SCENES) and int(sb.max()) == SCENES - 1
    target = PF.sonata_sinkhorn_torch(t.double()[mi[:, 1]], tt)
    assert torch.allclose(target.sum(1), torch.ones(m, dtype=torch.float64, device=device), rtol=0, atol=1e-12)
    rows = -(target * torch.log_softmax(s.double()[mi[:, 0]] / STUDENT_TEMP, -1)).sum(-1)
    want = sum(float(rows[scene == i].mean()) for i in MATCHED_SCENES) / DIVISOR
    assert abs(float(ref[0]) - want) <= 1e-12 * abs(want)
    got = _run(PF.sonata_distill, t, s, mi, sb, tt, num_scenes=SCENES, use_kernels=True)
    assert_close("divisor", got, ref, bounds(ref, tor, torch.float32))
    # num_scenes read from student_batch gives the same bits
    again = _run(PF.sonata_distill, t, s, mi, sb, tt, use_kernels=True)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


def check_empty(device, monkeypatch):
    """M = 0: nothing is launched, the result is the torch path's (NaN), the gradient all zeros"""
    t, s, mi, sb = distill_inputs(device, 5, 64)

    def refuse(*a, **k):
        raise AssertionError("a kernel was launched for an empty match_index")

    for name in ("sonata_colsum", "sonata_rowpass", "sonata_distill_fwd", "sonata_distill_bwd"):
        monkeypatch.setattr(ops, name, refuse)
    got = _run(PF.sonata_distill, t, s, mi[:0], sb, 0.07, use_kernels=True)
    ref = _run(PF.sonata_distill_torch, t, s, mi[:0], sb, 0.07)
    assert torch.allclose(got[0], ref[0], equal_nan=True) and bool(torch.isnan(got[0]))
    assert got[1].shape == s.shape and not bool(got[1].any()) and not bool(ref[1].any())


def check_unsupported_k(device):
    t, s, mi, sb = distill_inputs(device, 30, 100)
    assert not ops.sonata_supported(100) and ops.sonata_supported(64) and ops.sonata_supported(8192) and not ops.sonata_supported(8256)
    got = _run(PF.sonata_distill, t, s, mi, sb, 0.07, use_kernels=True)
    ref = _run(PF.sonata_distill_torch, t, s, mi, sb, 0.07)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    with pytest.raises(PtcoreError):
        ops.sonata_colsum(t, mi, 0.07)
    with pytest.raises(PtcoreError):
        ops.sonata_colsum(t[:, :64].double(), mi, 0.07)


def check_reproducible(device, m, k, dtype=torch.float32):
    t, s, mi, sb = distill_inputs(device, m, k, dtype, seed=2)
    a = _run(PF.sonata_distill, t, s, mi, sb, 0.04, num_scenes=SCENES, use_kernels=True)
    b = _run(PF.sonata_distill, t, s, mi, sb, 0.04, num_scenes=SCENES, use_kernels=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def check_permutation(device, m, k, tt):
    """pairs permuted inside their scenes: another summation order, the same result within the tolerance"""
    (t, s, mi, sb), ref, tor = references(device, m, k, tt, torch.float32)
    g = torch.Generator().manual_seed(4)
    scene = sb[mi[:, 0]].cpu()
    order = torch.cat([idx[torch.randperm(idx.numel(), generator=g)] for idx in (torch.nonzero(scene == i)[:, 0] for i in range(SCENES))])
    assert not torch.equal(order, torch.arange(m)) and torch.equal(scene[order], scene)
    got = _run(PF.sonata_distill, t, s, mi[order.to(device)], sb, tt, num_scenes=SCENES, max_groups=3, use_kernels=True)
    assert_close(f"permuted M={m} K={k}", got, ref, bounds(ref, tor, torch.float32))


def check_sharded(device, m, k, tt, cap=0):
    """the pairs of scenes (0, 1) on one rank and of scenes (2, 3) on another: the pass-level ops driven in lockstep with the column
    sums and the row count summed by hand give the loss and gradients of the unsharded run"""
    shards = [distill_inputs(device, m, k, seed=10 + i, scenes=2, matched=(0, 1)) for i in range(2)]
    nt0, ns0 = shards[0][0].shape[0], shards[0][1].shape[0]
    t = torch.cat([shards[0][0], shards[1][0]])
    s = torch.cat([shards[0][1], shards[1][1]])
    mi = torch.cat([shards[0][2], shards[1][2] + torch.tensor([ns0, nt0], device=device)])
    sb = torch.cat([shards[0][3], shards[1][3] + 2])
    ref = _run(PF.sonata_distill_torch, t.double(), s.double(), mi, sb, tt)
    tor = _run(PF.sonata_distill_torch, t, s, mi, sb, tt)
    n = 2 * m
    r = sum(ops.sonata_colsum(x[0], x[2], tt, None, cap) for x in shards)
    for it in range(3):
        a = torch.reciprocal(r * k)
        if it < 2:
            r = sum(ops.sonata_rowpass(x[0], x[2], tt, a, n, True, cap)[2] for x in shards)
    loss, grads = 0, []
    half = torch.full((1,), 0.5, device=device)
    for x in shards:
        l, means, state = ops.sonata_distill_fwd(x[0], x[1], x[2], x[3], 2, tt, STUDENT_TEMP, a, cap)
        assert means.shape == (2,) and abs(float(means.mean()) - float(l)) <= 1e-6 * abs(float(l))
        loss = loss + 0.5 * l[0]
        grads.append(ops.sonata_distill_bwd(state, tt, STUDENT_TEMP, half, cap))
    assert_close(f"sharded M=2x{m} K={k}", (loss, torch.cat(grads)), ref, bounds(ref, tor, torch.float32))
    # and the all_reduce hook of the functional sees exactly those tensors: the row count first, then three K-vectors
    seen = []
    PF.sonata_distill(shards[0][0], shards[0][1], shards[0][2], shards[0][3], tt, STUDENT_TEMP, all_reduce=lambda x: seen.append(tuple(x.shape)),
                      num_scenes=2, use_kernels=True)
    assert seen == [(1,), (k,), (k,), (k,)]


# ---------------------------------------------------------------------------------------------------------------- GPU tests
SHAPES = [(m, k) for k in (64, 192, 4096) for m in (1, 63, 65, 1000)] + [(20000, 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tt", [0.04, 0.07])
@pytest.mark.parametrize("m,k", SHAPES)
def test_distill_against_float64(m, k, tt, dtype):
    check_distill(dev(), m, k, tt, dtype)


@pytest.mark.parametrize("cap", [1, 3, 0])
@pytest.mark.parametrize("m,k,tt,dtype", [(1, 64, 0.04, torch.float32), (65, 192, 0.04, torch.bfloat16), (1000, 4096, 0.07, torch.float32),
                                          (1000, 4096, 0.04, torch.bfloat16), (20000, 64, 0.04, torch.float32)])
def test_scaling_vectors_against_float64(m, k, tt, dtype, cap):
    check_scaling_vectors(dev(), m, k, tt, dtype, cap)


def test_fp16_logits():
    check_distill(dev(), 65, 192, 0.07, torch.float16)


def test_divisor_counts_a_middle_scene_without_pairs_and_not_a_trailing_one():
    check_divisor(dev())


def test_no_pairs(monkeypatch):
    check_empty(dev(), monkeypatch)


def test_unsupported_k_takes_the_torch_path():
    check_unsupported_k(dev())


def test_two_runs_are_equal():
    check_reproducible(dev(), 1000, 4096)
    check_reproducible(dev(), 20000, 64, torch.bfloat16)


def test_permuting_pairs_within_a_scene():
    check_permutation(dev(), 1000, 192, 0.04)


@pytest.mark.parametrize("cap", [3, 0])
def test_sharded_passes_equal_the_unsharded_run(cap):
    check_sharded(dev(), 500, 192, 0.04, cap)


def test_no_m_by_k_temporary():
    """M = K = 4096 in fp32: one M x K fp32 matrix is 64 MiB; the forward may allocate a quarter of that above its inputs (the
    partial rows of a pass at 256 workgroups are 4 MiB)"""
    t, s, mi, sb = distill_inputs(dev(), 4096, 4096)
    s.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = PF.sonata_distill(t, s, mi, sb, 0.07, STUDENT_TEMP, num_scenes=SCENES)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"sonata_distill M=K=4096: peak allocation of the forward above the inputs {peak / 2**20:.2f} MiB")
    assert bool(torch.isfinite(loss)) and peak < 16 * 2**20


# ---------------------------------------------------------------------------------------------------------------- model
GOLD_BACKBONE = dict(type="PT-v3m2", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
                     enc_depths=(1, 1, 1, 2, 1), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32), enc_patch_size=(128,) * 5,
                     drop_path=0.0, shuffle_orders=False, enable_rpe=True, enable_flash=False, upcast_attention=True, upcast_softmax=True,
                     traceable=True, enc_mode=True, mask_token=True)
GOLD_CFG = dict(backbone=GOLD_BACKBONE, head_in_channels=128 + 256 + 512, head_hidden_channels=32, head_embed_channels=16,
                head_num_prototypes=64, teacher_custom=dict(drop_path=0.0), num_global_view=2, num_local_view=4, mask_size_start=0.1,
                mask_ratio_start=0.3, mask_jitter=0.0008, teacher_temp_start=0.04, student_temp=0.1, mask_loss_weight=2 / 8,
                roll_mask_loss_weight=2 / 8, unmask_loss_weight=4 / 8, match_max_r=0.12, up_cast_level=2)    # = make_golden_sonata.py CFG
GOLD_LOSSES = ("mask_loss", "roll_mask_loss", "unmask_loss", "loss")
GOLD_INTS = ("global_mask", "global_cluster", "mask_match_index", "roll_mask_match_index", "unmask_match_index")


def golden():
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sonata_tiny.npz"))


def golden_batch(g):
    """the fixture's multi-view batch, regenerated from its seeds and checked against its checksums"""
    from pointcept_amd import synthetic

    b = synthetic.multi_view_batch([int(s) for s in g["scene_seeds"]], int(g["view_sizes"][0]), int(g["view_sizes"][1]))
    assert sorted(b) == [str(k) for k in g["input_keys"]]
    assert np.array_equal(np.asarray([float(b[k].astype(np.float64).sum()) for k in sorted(b)]), g["input_checksum"])
    return b


def golden_state(g, model):
    """the fixture's deterministic weights for `model` (same key list, same float64 sums); the frozen weight-norm magnitudes are 1"""
    from oracle.ptv3_model import deterministic_state_dict

    sd = deterministic_state_dict(model, int(g["sd_seed"]))
    for k in sd:
        if k.endswith("parametrizations.weight.original0"):
            sd[k] = torch.ones_like(sd[k])
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert np.allclose([float(v.double().sum()) for v in sd.values()], g["sd_checksum"], rtol=0, atol=1e-9)
    return sd


class Recorder:
    """records the draws of a run / replays them into another one"""

    def __init__(self, replay=None):
        self.replay, self.log, self.i = replay, [], 0

    def __call__(self, kind, *args, device=None):
        from pointcept_amd.sonata import Sonata

        if self.replay is None:
            v = Sonata.draw(None, kind, *args, device=device)
            self.log.append((kind, v.cpu()))
            return v
        kind_was, v = self.replay[self.i]
        self.i += 1
        assert kind_was == kind
        return v.to(args[0].device if kind == "jitter" else device)


def golden_model(g, device):
    from pointcept_amd.sonata import Sonata

    torch.manual_seed(0)
    model = Sonata(**{**GOLD_CFG, "backbone": dict(GOLD_BACKBONE)})
    model.load_state_dict(golden_state(g, model))
    return model.to(device).train()


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _model_run(model, batch, rec, order_seed=0):
    model.draw = rec
    model.zero_grad(set_to_none=True)
    torch.manual_seed(order_seed)            # the backbone's shuffles of the serialization orders (CPU generator)
    out = model(dict(batch))
    out["loss"].backward()
    return {k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def check_port_against_golden(device):
    """the port, with the reference run's draws replayed, gives the reference file's integers exactly and its losses and gradients
    at the fp32 tolerances of the MSC golden test (tests/test_gpu_msc.py: losses 1e-4 relative, head gradients 2e-3 of their largest
    element, gradient norms 2e-2 where they are not rounding noise); no gradient reaches the teacher.
    The fixture's backbone takes the fp32 attention branch (enable_flash=False, enable_rpe=True): with enable_flash=True the
    engine's PT-v3 attention takes bf16 operands whatever the dtype of the run (the reference's flash-attention cast), and
    1 / teacher_temp = 25 multiplies what that leaves in the logits -- measured on the MI355X with such a fixture, mask_loss 6.5115652
    against 6.5126033 (1.6e-4) with kernels and with PTC_SONATA=0 alike while the host met it to 2e-6, i.e. the difference was the
    backbone's, and a reference run in fp32 is no yardstick for it at 1e-4.  With the fp32 branch, measured on the MI355X:
    mask_loss 6.5780973, roll_mask_loss 6.5895882, unmask_loss 6.3491011, loss 6.4664717 against 6.5780983, 6.5895882, 6.3491006,
    6.4664717 (1.5e-7), and on the host 6.5780978 / 6.5780983 with the losses on the emulated kernels."""
    from pointcept_amd import synthetic

    g = golden()
    model = golden_model(g, device)
    batch = synthetic.to_torch(golden_batch(g), device)
    draws = [("patch_perm", torch.from_numpy(g["draw_patch_perm"])), ("jitter", torch.from_numpy(g["draw_jitter"]))]
    out, grads = _model_run(model, batch, Recorder(draws), int(g["order_seed"]))
    assert model.draw.i == 2
    for k in GOLD_INTS:
        assert np.array_equal(model.last[k].cpu().numpy(), g[k]), k
        assert g[k].shape[0] > 0
    assert max(np.bincount(g[k][:, 1]).max() for k in GOLD_INTS[2:]) >= 2      # a teacher row matched twice
    assert set(out) == set(GOLD_LOSSES)
    for k in GOLD_LOSSES:
        ref = float(g["out/" + k])
        print(f"golden {k}: port {float(out[k]):.8g} reference {ref:.8g}")
        assert abs(float(out[k]) - ref) <= 1e-4 * abs(ref), k
    names = [str(k) for k in g["param_names"]]
    assert names == [k for k, _ in model.named_parameters() if k.startswith("student.")]
    assert set(grads) == set(n for n, h in zip(names, g["has_grad"]) if h) and not any(k.startswith("teacher.") for k in grads)
    have = np.asarray(g["has_grad"], bool)
    norms = np.asarray([float(grads[k].double().norm()) if h else 0.0 for k, h in zip(names, have)])
    big = g["grad_norms"] > 1e-4 * g["grad_norms"].max()
    assert np.allclose(norms[big], g["grad_norms"][big], rtol=2e-2), np.abs(norms[big] / g["grad_norms"][big] - 1).max()
    heads = [k for k in g.files if k.startswith("grad/")]
    assert len(heads) == 10
    for k in heads:
        assert _rel(grads[k[5:]], g[k]) < 2e-3, (k, _rel(grads[k[5:]], g[k]))


def check_state_dict_keys():
    from pointcept_amd.sonata import Sonata

    g = golden()
    keys = list(Sonata(**{**GOLD_CFG, "backbone": dict(GOLD_BACKBONE)}).state_dict().keys())
    assert keys == [str(k) for k in g["keys"]]
    assert any(k.endswith("prototype.parametrizations.weight.original0") for k in keys) and keys[0].startswith("student.")


def check_ema(device):
    """after_step at the fixture's momentum: every teacher parameter against the stored float64 sums"""
    g = golden()
    model = golden_model(g, device)
    model.momentum = float(g["ema_momentum"])
    model.after_step()
    teacher = [(k, p) for k, p in model.named_parameters() if k.startswith("teacher.")]
    assert [k for k, _ in teacher] == [str(k) for k in g["ema_names"]]
    got = np.asarray([float(p.detach().double().sum()) for _, p in teacher])
    got_abs = np.asarray([float(p.detach().double().abs().sum()) for _, p in teacher])
    assert np.allclose(got_abs, g["ema_abs_sum"], rtol=1e-6, atol=0)
    assert np.all(np.abs(got - g["ema_sum"]) <= 1e-6 * g["ema_abs_sum"])
    frozen = [p for k, p in teacher if k.endswith("original0")]
    assert len(frozen) == 2 and all(bool((p == 1).all()) for p in frozen)        # 0.9 * 1 + 0.1 * 1
    assert not any(p.requires_grad for _, p in teacher)


def check_match_neighbour(device, name):
    """the cell-grid search with k = 1 against knn_query(1) + `distance < match_max_r`, row for row"""
    import types

    import test_gpu_msc as T
    from pointcept_amd.sonata import Sonata

    v2, off2, v1, off1, radius = T.designed_cases()[name]
    x2, x1 = T._t(v2, device), T._t(v1, device)
    o2, o1 = T._t(off2, device, torch.int32), T._t(off1, device, torch.int32)
    this = types.SimpleNamespace(match_max_r=float(radius), _kernels=lambda t: True)
    got = Sonata.match_neighbour(this, x1, o1, x2, o2)
    assert got.dtype == torch.int64 and got.dim() == 2 and got.shape[1] == 2
    if x1.shape[0] == 0:
        assert got.shape[0] == 0
        return got
    this._kernels = lambda t: False
    ref = Sonata.match_neighbour(this, x1, o1, x2, o2)
    assert torch.equal(got.cpu(), ref.cpu())
    return got


def check_generate_mask(device, mask_size, mask_ratio):
    """point_mask and point_cluster of the key-sort path against the torch.unique expression for the same permutation"""
    import types

    from pointcept_amd import synthetic
    from pointcept_amd.sonata import Sonata

    b = synthetic.to_torch(synthetic.multi_view_batch([11, 12, 13], 900, 300), device)
    coord, offset = b["global_coord"] * 3.0 - 1.0, b["global_offset"]
    this = types.SimpleNamespace(mask_size=mask_size, mask_ratio=mask_ratio, _kernels=lambda t: False, draw=Recorder())
    mask_t, cluster_t = Sonata.generate_mask(this, coord, offset)
    this._kernels, this.draw = (lambda t: True), Recorder(this.draw.log)
    mask_k, cluster_k = Sonata.generate_mask(this, coord, offset)
    assert torch.equal(cluster_k, cluster_t) and torch.equal(mask_k, mask_t) and mask_k.dtype == torch.bool
    patch_num = int(cluster_t.max()) + 1
    assert patch_num > 20 and int(torch.unique(cluster_t[mask_t]).numel()) == int(patch_num * mask_ratio)
    return patch_num


def check_autocast_step(device, dtype=torch.bfloat16):
    """a mixed-precision train step: finite gradients on every trainable student parameter, none on the teacher"""
    from pointcept_amd import synthetic
    from pointcept_amd.sonata import Sonata

    torch.manual_seed(0)
    model = Sonata(**{**GOLD_CFG, "backbone": dict(GOLD_BACKBONE)}).to(device).train()
    batch = synthetic.to_torch(synthetic.multi_view_batch([21, 22], 700, 300), device)
    with torch.autocast(device_type=device.type, dtype=dtype):
        out = model(dict(batch))
    assert out["loss"].dtype == torch.float32 and bool(torch.isfinite(out["loss"]))
    out["loss"].backward()
    for k, p in model.named_parameters():
        if k.startswith("teacher."):
            assert p.grad is None and not p.requires_grad, k
        elif p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        else:
            assert k.endswith("original0") and p.grad is None, k


def check_return_point(device):
    from pointcept_amd import synthetic

    g = golden()
    model = golden_model(g, device).eval()
    b = synthetic.to_torch(golden_batch(g), device)
    with torch.no_grad():
        point = model(dict(feat=b["global_feat"], coord=b["global_coord"], origin_coord=b["global_origin_coord"], offset=b["global_offset"],
                           grid_size=b["grid_size"][0]), return_point=True)["point"]
    assert point.feat.shape == (point.coord.shape[0], GOLD_CFG["head_in_channels"]) and point.coord.shape[0] < b["global_coord"].shape[0]
    assert "pooling_parent" in point.keys() and bool(torch.isfinite(point.feat).all())


def test_registered_only_when_named():
    from pointcept_amd import compat

    assert "Sonata-v1m1" not in compat.MODEL_CLASSES and compat.OPT_IN_MODEL_CLASSES["Sonata-v1m1"] == ("sonata", "Sonata")


def test_state_dict_keys_are_the_references():
    check_state_dict_keys()


def test_port_matches_reference_golden():
    check_port_against_golden(dev())


def test_port_matches_reference_golden_on_the_torch_path(monkeypatch):
    from pointcept_amd import config

    monkeypatch.setattr(config, "SONATA_KERNELS", False)
    check_port_against_golden(dev())


def test_ema_step_equals_the_stored_teacher():
    check_ema(dev())


@pytest.mark.parametrize("name", ["few_empty_dense", "k_kplus1_dup_boundary", "m_zero", "n_zero", "nan_rows", "wild_extent_grows_cells"])
def test_match_neighbour_designed(name):
    check_match_neighbour(dev(), name)


def test_generate_mask_equals_the_unique_expression():
    check_generate_mask(dev(), 0.1, 0.3)
    check_generate_mask(dev(), 0.4, 0.7)


def test_bf16_autocast_train_step():
    check_autocast_step(dev())


def test_return_point():
    check_return_point(dev())
