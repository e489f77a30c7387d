"""-m gpu: the criteria kernels (csrc/criteria.hip; functional.seg_criteria / cross_entropy / focal_loss / dice_loss, criteria.Criteria,
segmentor.DefaultSegmentorV2 with config dicts).  The check_* bodies take a device; tests/test_criteria_cpu.py runs them on the host
emulation at the small shapes.

Every loss and gradient is compared against the float64 evaluation of its torch twin (functional.*_torch, the reference's expressions)
on the values the kernel reads -- the upcast values for 16-bit logits.  Tolerance (the rule of tests/test_gpu_sonata.py::bounds, set
before any kernel figure was seen): the error of the same twin in fp32 against float64 is measured in the test; the kernel may have
4 x that error and never less than FLOOR_ULPS = 4 fp32 ulps (4 * 2^-23) of the scale of the quantity compared.  Scale of a loss:
max(|loss|, 1) -- the summed terms (lse - x[t], softplus(|x|), 1 - num / den) are of order one or more whatever their mean is.
Gradients are scaled ROW BY ROW (class weights and the Dice coefficients spread the rows' magnitudes over orders): each row's error is
divided by the row's largest float64 element, the figure is the maximum over the rows, for the twin and for the kernel alike; a row whose
float64 gradient is all zero must be exactly zero.  A 16-bit logits tensor receives its gradient in its own dtype: half a 16-bit ulp
(2^-8 bf16, 2^-11 fp16) of the row's scale is added to the gradient bound and to nothing else -- and, for fp16, half the spacing of
its subnormals (2^-25, absolute): Dice's gradients at a few hundred rows are of the order 1e-7 and leave fp16's normal range.  Every
figure is printed before it is asserted.  Fused against separate calls is compared in fp32 only (three 16-bit roundings against one would need another bound)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pointcept_amd import config  # noqa: E402
from pointcept_amd import functional as PF  # noqa: E402
from pointcept_amd import ops  # noqa: E402
from pointcept_amd.criteria import Criteria  # noqa: E402

FLOOR_ULPS = 4
ULP = 2.0 ** -23
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_SUBNORMAL = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}      # absolute; bf16 has fp32's exponent range
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criteria_tiny.npz")
# SemanticKITTI's class weights (configs/semantic_kitti/semseg-spunet-v1m1-0-base.py)
KITTI_WEIGHT = [3.1557, 8.7029, 7.8281, 6.1354, 6.3161, 7.9937, 8.9704, 10.1922, 1.6155, 4.2187, 1.9385, 5.5455, 2.0198, 2.6261, 1.3212,
                5.1102, 2.5492, 5.8585, 7.3929]
KITTI_CRITERIA = [dict(type="CrossEntropyLoss", weight=KITTI_WEIGHT, loss_weight=1.0, ignore_index=-1),
                  dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]


def dev():
    return torch.device("cuda")


def case(device, n, c, dtype=torch.float32, seed=0, strided=False, amp=3.0, wild=True):
    """(logits [n, c], labels [n]): a fifth of the rows ignored (-1), class 1 absent (c > 2); `wild`: two labels outside [0, c) that are
    not the ignore_index (not counted by CrossEntropy / Focal, clamped by Dice).  strided: a [:, :c] view of a [n, c + 3] tensor."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + c)
    x = (torch.randn(n, c + 3, generator=g) * amp).to(dtype)
    t = torch.randint(0, c, (n,), generator=g)
    t[torch.rand(n, generator=g) < 0.2] = -1
    if c > 2:
        t[t == 1] = 0
    t[0] = 1 if c == 2 else 2                   # a counted row of a class with a positive weight, whatever n
    if wild and n >= 4:
        t[n // 2], t[n // 3] = c + 3, -7
    x = x.to(device)
    return (x[:, :c] if strided else x[:, :c].contiguous()), t.to(device)


def class_weight(c):
    """[c] positive weights with a zero entry at class 0 (and every 7th)"""
    return [0.0 if j % 7 == 0 else 0.5 + (j * 5 % 11) / 4 for j in range(c)]


def alpha_list(c):
    return [0.05 + 0.9 * j / max(c - 1, 1) for j in range(c)]


def _up(x, dtype):
    """the values the kernel reads, in the reference's dtype"""
    return x.float().to(dtype)


def _run(fn, x, t, *a, **kw):
    x = x.detach().clone().requires_grad_(True)
    loss = fn(x, t, *a, **kw)
    loss.backward()
    return loss.detach(), (x.grad if x.grad is not None else torch.zeros_like(x))


def twin_pair(x, t, terms, ignore_index):
    """(float64 result, fp32 result) of the torch twins on the values the kernel reads"""
    return (_run(PF.seg_criteria_torch, _up(x, torch.float64), t, terms, ignore_index),
            _run(PF.seg_criteria_torch, _up(x, torch.float32), t, terms, ignore_index))


def bounds(ref, tor, dtype):
    """{"loss": (twin error, bound, scale), "grad": (twin row-scaled error, bound, live rows)}"""
    scale = max(abs(float(ref[0])), 1.0)
    e_loss = abs(float(tor[0].double() - ref[0]))
    rs = ref[1].abs().amax(1)
    live = rs > 0
    e_grad = float(((tor[1].double() - ref[1]).abs().amax(1)[live] / rs[live]).max()) if bool(live.any()) else 0.0
    return {"loss": (e_loss, max(4 * e_loss, FLOOR_ULPS * ULP * scale), scale),
            "grad": (e_grad, max(4 * e_grad, FLOOR_ULPS * ULP) + HALF_ULP[dtype], live, HALF_SUBNORMAL[dtype])}


def assert_close(tag, got, ref, bnd):
    e_t, b_l, scale = bnd["loss"]
    e_k = abs(float(got[0].double() - ref[0]))
    print(f"criteria {tag} loss: kernel err {e_k:.3e}  torch fp32 err {e_t:.3e}  bound {b_l:.3e}  scale {scale:.3e}")
    g_t, b_g, live, sub = bnd["grad"]
    rs = ref[1].abs().amax(1)
    g_k, over = 0.0, 0.0
    if bool(live.any()):
        rows = (got[1].double() - ref[1]).abs().amax(1)[live] / rs[live]
        excess = rows - (b_g + sub / rs[live])              # per row: the relative bound plus the absolute subnormal term over the row's scale
        g_k, over = float(rows.max()), float(excess.max())
    print(f"criteria {tag} grad (row-scaled): kernel err {g_k:.3e}  torch fp32 err {g_t:.3e}  bound {b_g:.3e} (+ {sub:.1e} / row scale)  "
          f"worst excess {over:.3e}  live rows {int(live.sum())}")
    assert e_k <= b_l, (tag, "loss", e_k, e_t, b_l)
    assert over <= 0.0, (tag, "grad", g_k, g_t, b_g, over)
    assert not bool(got[1][~live].any()), (tag, "rows without a gradient must be exactly zero")
    return e_k, g_k


def check_terms(device, tag, x, t, terms, ignore_index=-1):
    """seg_criteria on the kernels against the float64 twin under the rule above"""
    ref, tor = twin_pair(x, t, terms, ignore_index)
    got = _run(PF.seg_criteria, x, t, terms, ignore_index, use_kernels=True)
    assert got[0].dtype == torch.float32 and got[1].dtype == x.dtype and got[1].shape == x.shape
    assert_close(tag, got, ref, bounds(ref, tor, x.dtype))
    return got, ref, tor


def check_ce(device, n, c, dtype, eps, reduction, strided=False):
    x, t = case(device, n, c, dtype, strided=strided)
    term = dict(type="CrossEntropyLoss", weight=class_weight(c), label_smoothing=eps, reduction=reduction, loss_weight=0.75)
    got, _, _ = check_terms(device, f"CE N={n} C={c} {str(dtype)[6:]} eps={eps} {reduction} strided={strided}", x, t, [term])
    if x.is_cuda:       # the public entry point is this very call, loss_weight apart
        pub = _run(PF.cross_entropy, x, t, -1, class_weight(c), eps, reduction)
        one = _run(PF.seg_criteria, x, t, [dict(term, loss_weight=1.0)], -1)
        assert torch.equal(pub[0], one[0]) and torch.equal(pub[1], one[1])


def check_ce_nan(device):
    """mean over a zero denominator is nan, as ATen: every row ignored (gradient all zero), and only zero-weight classes present (nan
    on the counted rows, zero on the ignored ones), with and without smoothing"""
    x, t = case(device, 257, 19, wild=False)
    w = class_weight(19)
    for name, labels in (("all rows ignored", torch.full_like(t, -1)), ("zero-weight classes only", torch.where(t >= 0, t * 0 + 7, t))):
        for eps in (0.0, 0.1):
            term = [dict(type="CrossEntropyLoss", weight=w, label_smoothing=eps)]
            ref = _run(PF.seg_criteria_torch, x.double(), labels, term, -1)
            got = _run(PF.seg_criteria, x, labels, term, -1, use_kernels=True)
            print(f"criteria CE {name} eps={eps}: kernel {float(got[0])} torch {float(ref[0])}; nan gradients {int(got[1].isnan().sum())} / "
                  f"{int(ref[1].isnan().sum())}")
            assert bool(ref[0].isnan()) and bool(got[0].isnan())
            assert torch.equal(got[1].isnan(), ref[1].isnan())
            assert not bool(got[1][~got[1].isnan()].any())
    labels = torch.where(t >= 0, t * 0 + 7, t)        # reduction="sum" has no denominator: finite, and zero at eps = 0
    check_terms(device, "CE zero-weight classes only, sum", x, labels, [dict(type="CrossEntropyLoss", weight=w, reduction="sum")])


def check_focal(device, n, c, dtype, gamma, listed, strided=False):
    x, t = case(device, n, c, dtype, strided=strided)
    term = dict(type="FocalLoss", gamma=gamma, alpha=alpha_list(c) if listed else 0.25, loss_weight=1.5)
    check_terms(device, f"Focal N={n} C={c} {str(dtype)[6:]} gamma={gamma} alpha={'list' if listed else 0.25} strided={strided}", x, t, [term])


def check_focal_saturated(device):
    """logits of +-30: sigma and 1 - sigma leave fp32's range of 1 - x; the closed form has no such subtraction"""
    x, t = case(device, 257, 19)
    x = torch.where(x > 0, torch.full_like(x, 30.0), torch.full_like(x, -30.0))
    got, _, _ = check_terms(device, "Focal +-30", x, t, [dict(type="FocalLoss", gamma=2.0, alpha=0.5)])
    assert bool(torch.isfinite(got[1]).all())


def check_focal_none_counted(device):
    """no counted row: a zero TENSOR and a zero gradient (the reference returns the float 0.0)"""
    x, t = case(device, 257, 19)
    t = torch.where((t >= 0) & (t < 19), torch.full_like(t, -1), t)        # the two wild labels stay: they are not counted either
    got = _run(PF.seg_criteria, x, t, [dict(type="FocalLoss")], -1, use_kernels=True)
    twin = _run(PF.focal_loss_torch, x, t)
    print(f"criteria Focal no counted row: kernel {float(got[0])} twin {float(twin[0])}")
    assert float(got[0]) == 0.0 and float(twin[0]) == 0.0 and not bool(got[1].any()) and not bool(twin[1].any())


def check_dice(device, n, c, dtype, exponent, ignore_index=-1, strided=False):
    x, t = case(device, n, c, dtype, strided=strided)
    if c > 2 and n >= 4:
        assert not bool((t == 1).any()) and bool((t >= c).any()) and bool(((t < 0) & (t != ignore_index)).any())   # absent class, clamps
    term = dict(type="DiceLoss", smooth=1, exponent=exponent, loss_weight=2.0)
    check_terms(device, f"Dice N={n} C={c} {str(dtype)[6:]} e={exponent} ignore={ignore_index} strided={strided}", x, t, [term], ignore_index)


def check_dice_no_valid_row(device):
    x, t = case(device, 257, 19)
    t = torch.full_like(t, -1)
    got, ref, _ = check_terms(device, "Dice no valid row", x, t, [dict(type="DiceLoss")])
    assert float(got[0]) == 0.0 and float(ref[0]) == 0.0 and not bool(got[1].any())


FUSED = lambda c: [dict(type="CrossEntropyLoss", weight=class_weight(c), label_smoothing=0.1, loss_weight=0.7),      # noqa: E731
                   dict(type="FocalLoss", gamma=2.0, alpha=alpha_list(c), loss_weight=1.3),
                   dict(type="DiceLoss", smooth=1, exponent=2, loss_weight=0.5)]


def check_fused(device, n, c, dtype, strided=False):
    """all three terms in one call: against the float64 twin, and (fp32) against the sum of the three one-term calls"""
    x, t = case(device, n, c, dtype, strided=strided)
    terms = FUSED(c)
    got, ref, tor = check_terms(device, f"fused N={n} C={c} {str(dtype)[6:]} strided={strided}", x, t, terms)
    if dtype == torch.float32:
        parts = [_run(PF.seg_criteria, x, t, [term], -1, use_kernels=True) for term in terms]
        apart = (sum(p[0].double() for p in parts), sum(p[1].double() for p in parts))
        assert_close(f"fused against separate N={n} C={c}", got, apart, bounds(ref, tor, dtype))
    return got


def check_duplicate_terms(device):
    """a list that names one class twice: a second call behind the first, the same sum"""
    x, t = case(device, 257, 19)
    terms = FUSED(19) + [dict(type="CrossEntropyLoss", reduction="sum", loss_weight=0.01)]
    check_terms(device, "two CrossEntropyLoss terms", x, t, terms)


def check_determinism(device):
    a, b = check_fused(device, 513, 19, torch.bfloat16), check_fused(device, 513, 19, torch.bfloat16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def check_default_cross_entropy_bits(device):
    """the three new arguments at their defaults: exactly the call cross_entropy always was"""
    for dtype, strided in ((torch.bfloat16, True), (torch.float32, False)):
        x, t = case(device, 513, 20, dtype, strided=strided, wild=False)
        old = _run(PF.cross_entropy, x, t, -1)
        new = _run(PF.cross_entropy, x, t, -1, None, 0.0, "mean")
        kw = _run(PF.cross_entropy, x, t, ignore_index=-1, weight=None, label_smoothing=0.0, reduction="mean")
        assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]) and torch.equal(old[0], kw[0]) and torch.equal(old[1], kw[1])


def check_wide_fallbacks(device, c):
    """33 classes and more: CrossEntropy on the element-wise kernels (check_ce), Focal and Dice on their twins -- the same numbers as the
    twin called directly, and the kernel entry points refuse the shape"""
    x, t = case(device, 257, c)
    for term, twin in ((dict(type="FocalLoss", gamma=2.0, alpha=0.25), lambda a, b: PF.focal_loss_torch(a, b, 2.0, 0.25, -1)),
                       (dict(type="DiceLoss", exponent=2), lambda a, b: PF.dice_loss_torch(a, b, 1, 2, -1))):
        got, ref = _run(PF.seg_criteria, x, t, [term], -1, use_kernels=True), _run(twin, x, t)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    spec = ops.CriteriaSpec(-1)
    spec.flags = ops.CRITERIA_FOCAL
    with pytest.raises(PF.PtcoreError, match="classes"):
        ops.criteria_rows_fwd(x, t, spec)
    x19, t19 = case(device, 257, 19)         # another exponent: the twin as well
    got, ref = _run(PF.dice_loss, x19, t19, 1, 4, -1, use_kernels=True), _run(PF.dice_loss_torch, x19, t19, 1, 4, -1)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def check_criteria_kitti(device):
    """Criteria with the SemanticKITTI list: the weighted CrossEntropy term on the criteria kernels + Lovasz on its own"""
    x, t = case(device, 513, 19, torch.bfloat16, strided=True, wild=False)
    crit = Criteria(KITTI_CRITERIA)
    assert crit.terms[0][0] == "fused" and crit.terms[1][0] is PF.lovasz_softmax
    use = dict(use_kernels=True) if not x.is_cuda else {}

    def by_hand(a, b):
        return PF.seg_criteria(a, b, [KITTI_CRITERIA[0]], -1, **use) + PF.lovasz_softmax(a, b, -1)

    got = _run(lambda a, b: crit(a, b), x, t) if x.is_cuda else None
    hand = _run(by_hand, x, t)
    if got is not None:
        assert torch.equal(got[0], hand[0]) and torch.equal(got[1], hand[1])
    ce = [KITTI_CRITERIA[0]]
    check_terms(device, "KITTI weighted CE", x, t, ce)
    ref = _run(PF.seg_criteria_torch, _up(x, torch.float64), t, ce, -1)
    lov = _run(PF.lovasz_softmax, x, t, -1)
    assert abs(float(hand[0]) - float(ref[0]) - float(lov[0])) <= 1e-5 * max(1.0, abs(float(hand[0])))
    plain = Criteria([dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1), KITTI_CRITERIA[1]])
    assert [e[0] for e in plain.terms] == [PF.cross_entropy, PF.lovasz_softmax]          # the default list: the calls it always took


class _Head(torch.nn.Module):
    """backbone stand-in: the point's features as they come"""

    def forward(self, point):
        return point.feat


def check_segmentor_with_config_dicts(device):
    """DefaultSegmentorV2(criteria=[dict(...)]) end to end: the loss is Criteria's on the head's logits, and it trains the head"""
    from pointcept_amd.segmentor import DefaultSegmentorV2

    torch.manual_seed(0)
    cfg = [dict(KITTI_CRITERIA[0]), dict(type="FocalLoss", gamma=2.0, alpha=0.25, loss_weight=0.5, ignore_index=-1),
           dict(type="DiceLoss", loss_weight=0.5, ignore_index=-1), dict(KITTI_CRITERIA[1])]
    model = DefaultSegmentorV2(19, 16, _Head(), criteria=cfg).to(device).train()
    assert [e[0] if isinstance(e[0], str) else e[0].__name__ for e in model.criteria_list.terms] == ["fused", "lovasz_softmax"]
    feat, seg = case(device, 300, 16, wild=False)
    seg = seg.clamp(max=18)
    batch = dict(feat=feat, segment=seg, offset=torch.tensor([300], device=device))
    out = model(batch)
    out["loss"].backward()
    logits = model.seg_head(feat).detach()
    want = PF.seg_criteria_torch(logits.double(), seg, cfg[:3], -1) + PF.lovasz_softmax(logits, seg, -1).double()
    print(f"criteria segmentor: loss {float(out['loss']):.7f}  twins + lovasz {float(want):.7f}")
    assert abs(float(out["loss"]) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    assert model.seg_head.weight.grad is not None and bool(torch.isfinite(model.seg_head.weight.grad).all()) and \
        float(model.seg_head.weight.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="unknown criterion"):
        DefaultSegmentorV2(19, 16, _Head(), criteria=("ce", "dice"))
    assert DefaultSegmentorV2(19, 16, _Head(), criteria=("ce", "lovasz")).criteria_list is None


# ---- the golden: the reference's own modules in fp32 on seeded cases (tests/golden/make_golden_criteria.py) -------------------------------
GOLDEN_CASES = [      # (n, c, seed, ignore_index, term)
    (120, 19, 1, -1, dict(type="CrossEntropyLoss", weight=class_weight(19), label_smoothing=0.1, reduction="mean", loss_weight=0.5)),
    (120, 19, 2, -1, dict(type="CrossEntropyLoss", weight=KITTI_WEIGHT, reduction="sum", loss_weight=1.0)),
    (120, 19, 3, -1, dict(type="FocalLoss", gamma=2.0, alpha=0.5, loss_weight=1.0)),
    (70, 13, 4, -1, dict(type="FocalLoss", gamma=0.0, alpha=alpha_list(13), loss_weight=2.0)),
    (120, 19, 5, -1, dict(type="DiceLoss", smooth=1, exponent=2, loss_weight=1.0)),
    (70, 13, 6, 2, dict(type="DiceLoss", smooth=1, exponent=3, loss_weight=0.5)),
]


def golden_case(ci):
    n, c, seed, ignore, term = GOLDEN_CASES[ci]
    x, t = case(torch.device("cpu"), n, c, seed=seed, wild=False)
    if ignore != -1:
        t = torch.where(t == -1, torch.full_like(t, ignore), t)
    return x, t, ignore, term


def check_golden(device, use_kernels):
    """both paths against the reference's fp32 numbers: two fp32 evaluations in different operation orders, 1e-5 of the loss's scale and
    of the gradient's largest element"""
    g = np.load(GOLDEN)
    assert int(g["n_cases"]) == len(GOLDEN_CASES)
    for ci in range(len(GOLDEN_CASES)):
        x, t, ignore, term = golden_case(ci)
        assert np.array_equal(g[f"labels_{ci}"], t.numpy().astype(np.int16)) and float(g[f"logits_sum_{ci}"]) == float(x.double().sum())
        got = _run(PF.seg_criteria, x.to(device), t.to(device), [term], ignore, use_kernels=use_kernels)
        e_l = abs(float(got[0]) - float(g[f"loss_{ci}"]))
        e_g = float(np.abs(got[1].cpu().numpy() - g[f"grad_{ci}"]).max())
        s_g = float(np.abs(g[f"grad_{ci}"]).max())
        print(f"criteria golden {ci} {term['type']} kernels={use_kernels}: loss {float(got[0]):.7f} / {float(g[f'loss_{ci}']):.7f}  grad err {e_g:.3e} "
              f"of {s_g:.3e}")
        assert e_l <= 1e-5 * max(1.0, abs(float(g[f"loss_{ci}"]))) and e_g <= 1e-5 * s_g


# ---- -m gpu --------------------------------------------------------------------------------------------------------------------------
NS, CS = (1, 255, 257, 513), (2, 19, 20, 32)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


@pytest.mark.parametrize("n,c,dtype,eps,reduction,strided",
                         [(n, c, torch.float32, eps, red, False) for n in NS for c in CS for eps, red in ((0.0, "mean"), (0.1, "sum"))] +
                         [(257, 19, dt, 0.1, "mean", st) for dt in DTYPES for st in (False, True)] +
                         [(513, 32, torch.bfloat16, 0.0, "sum", True), (255, 20, torch.float16, 0.0, "mean", True)] +
                         [(n, c, dt, eps, red, st) for c in (33, 200) for n, dt, eps, red, st in
                          ((257, torch.float32, 0.1, "mean", False), (513, torch.bfloat16, 0.0, "sum", True), (1, torch.float16, 0.1, "sum", False))])
def test_cross_entropy_weighted_smoothed(n, c, dtype, eps, reduction, strided):
    check_ce(dev(), n, c, dtype, eps, reduction, strided)


def test_cross_entropy_zero_denominators():
    check_ce_nan(dev())


@pytest.mark.parametrize("n,c,dtype,gamma,listed,strided",
                         [(n, c, torch.float32, g, ls, False) for n in NS for c in CS for g, ls in ((2.0, True), (0.0, False))] +
                         [(257, 19, dt, 2.0, False, st) for dt in DTYPES for st in (False, True)] + [(513, 32, torch.bfloat16, 0.0, True, True)])
def test_focal(n, c, dtype, gamma, listed, strided):
    check_focal(dev(), n, c, dtype, gamma, listed, strided)


def test_focal_saturated_logits():
    check_focal_saturated(dev())


def test_focal_no_counted_row():
    check_focal_none_counted(dev())


@pytest.mark.parametrize("n,c,dtype,exponent,ignore_index,strided",
                         [(n, c, torch.float32, e, -1, False) for n in NS for c in CS for e in (1, 2, 3)] +
                         [(257, 19, dt, 2, -1, st) for dt in DTYPES for st in (False, True)] +
                         [(257, 19, torch.float32, e, 2, False) for e in (1, 2, 3)] + [(513, 32, torch.bfloat16, 3, 5, True)])
def test_dice(n, c, dtype, exponent, ignore_index, strided):
    check_dice(dev(), n, c, dtype, exponent, ignore_index, strided)


def test_dice_no_valid_row():
    check_dice_no_valid_row(dev())


@pytest.mark.parametrize("n,c,dtype,strided", [(n, c, torch.float32, False) for n in NS for c in CS] +
                         [(513, 19, dt, st) for dt in DTYPES for st in (False, True)])
def test_fused_three_terms_and_against_separate_calls(n, c, dtype, strided):
    check_fused(dev(), n, c, dtype, strided)


def test_a_class_named_twice_takes_a_second_call():
    check_duplicate_terms(dev())


def test_two_runs_are_bit_equal():
    check_determinism(dev())


def test_default_arguments_keep_the_bits_of_the_old_call():
    check_default_cross_entropy_bits(dev())


@pytest.mark.parametrize("c", [33, 200])
def test_focal_and_dice_fall_back_above_32_classes(c):
    check_wide_fallbacks(dev(), c)


def test_criteria_with_the_semantic_kitti_list():
    check_criteria_kitti(dev())


def test_segmentor_takes_the_reference_config_dicts():
    check_segmentor_with_config_dicts(dev())


def test_golden_on_the_kernels():
    check_golden(dev(), True)


def test_golden_on_the_torch_path(monkeypatch):
    monkeypatch.setattr(config, "CRITERIA_KERNELS", False)
    x, t, ignore, term = golden_case(0)
    a = _run(PF.seg_criteria, x.to(dev()), t.to(dev()), [term], ignore)             # the switch, read at call time
    b = _run(PF.seg_criteria_torch, x.to(dev()), t.to(dev()), [term], ignore)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check_golden(dev(), None)
