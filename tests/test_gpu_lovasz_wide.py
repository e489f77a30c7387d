"""-m gpu: Lovasz-Softmax over the classes present only (csrc/lovasz.hip, the row-compacted path: ptc_lovasz_present +
ptc_lovasz_softmax_rows behind ops.lovasz_present / ops.lovasz_softmax(..., present=)), 65..1024 classes and, with an explicit handle,
any width.  The check_* bodies take a device; tests/test_lovasz_wide_cpu.py runs them on the host emulation at small shapes.

Bars, those of the existing Lovasz tests (tests/test_gpu_kernels.py) -- the per-slot arithmetic is the same:
  loss vs the reference module's value (tests/golden/lovasz_wide.npz)       1e-4 relative
  loss vs the fp64 oracle (oracle.losses.lovasz_softmax)                    2e-6 relative for fp32 logits, 1e-5 for 16-bit
  gradient vs the fp64 oracle                                               1e-4 of its largest element (fp32), 2e-2 (16-bit: the
                                                                            gradient is rounded to the logits' dtype)
  gradient vs the reference module's fp32 gradient (golden)                 1e-3 of the oracle's largest element (the reference's
                                                                            own gradient carries the cancellation of lovasz.py:31-32)
  rows path vs the dense path (c = 20, 64; explicit handle)                 loss 2e-6 relative, gradient 1e-4 of the largest element
Every figure is printed before it is asserted.  The oracle drops the labels equal to ignore_index; labels that are negative or >= c
are mapped to ignore_index before it sees them (the kernels' rule, lovasz_keys_kernel's).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import losses  # noqa: E402
from pointcept_amd import functional as PF  # noqa: E402
from pointcept_amd import ops  # noqa: E402
from pointcept_amd._lib import PtcoreError  # noqa: E402

# (index, n, c, p_ignore, n_used, spread, mode) of oracle.ptv3_model.lovasz_case; mode "all": the first c labels are 0..c-1 (every class
# present), "mirror": counted labels y -> c-1-y (the present classes sit at the top)
GOLDEN_CASES = [(10, 257, 200, 0.10, 37, 2.0, "plain"), (11, 300, 100, 0.0, 100, 1.0, "all"), (12, 65, 65, 0.0, 1, 1.0, "plain"),
                (10, 257, 200, 0.10, 37, 2.0, "mirror")]
GOLDEN_PRESENT = [37, 100, 1, 37]


def dev():
    return torch.device("cuda")


def wide_case(index, n, c, p_ignore, n_used, spread, mode):
    from oracle import ptv3_model as om

    x, y = om.lovasz_case(index, n, c, p_ignore, n_used, spread)
    if mode == "all":
        y[:c] = torch.arange(c)
    elif mode == "mirror":
        y = torch.where(y >= 0, c - 1 - y, y)
    return x, y


def golden_cases():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lovasz_wide.npz"))
    assert int(g["n_cases"]) == len(GOLDEN_CASES)
    for ci, spec in enumerate(GOLDEN_CASES):
        assert [float(v) for v in g[f"spec_{ci}"]] == [float(v) for v in spec[:6]] and str(g[f"mode_{ci}"]) == spec[6]
        x, y = wide_case(*spec)
        assert abs(float(x.double().sum()) - float(g[f"logits_sum_{ci}"])) < 1e-6 and np.array_equal(y.numpy(), g[f"labels_{ci}"])
        assert len(np.unique(y.numpy()[y.numpy() >= 0])) == GOLDEN_PRESENT[ci]
        yield ci, x, y, float(g[f"loss_{ci}"]), g[f"grad_{ci}"]


_oracle_cache = {}


def oracle(key, x, y, ignore_index=-1):
    """fp64 loss and gradient, computed once per case and shared (read-only) by the tests that need it"""
    if key not in _oracle_cache:
        c = x.shape[1]
        yo = y.clone()
        yo[(yo < 0) | (yo >= c)] = ignore_index
        lo, do = losses.lovasz_softmax(x.float().numpy(), yo.numpy(), ignore_index)
        do.setflags(write=False)
        _oracle_cache[key] = (lo, do)
    return _oracle_cache[key]


def run(device, x, y, ignore_index=-1, handle=False, scale=1.0):
    """-> (loss, gradient of loss w.r.t. x as numpy fp32 [n, c] of the leaf's own shape)"""
    xe = x.clone().to(device).requires_grad_(True)
    yd = y.to(device)
    present = PF.lovasz_present(yd, x.shape[1], ignore_index) if handle else None
    loss = PF.lovasz_softmax(xe, yd, ignore_index, present=present)
    (loss * scale).backward()
    return float(loss.detach()), xe.grad.float().cpu().numpy() / scale


def check_against_oracle(device, tag, x, y, ignore_index=-1, handle=False, scale=1.0):
    sixteen = x.dtype != torch.float32
    lo, do = oracle(tag, x, y, ignore_index)
    loss, g = run(device, x, y, ignore_index, handle, scale)
    gmax = max(float(np.abs(do).max()), 1e-12)
    lerr, gerr = abs(loss - lo), float(np.abs(g - do).max()) if do.size else 0.0
    lbar, gbar = (1e-5 if sixteen else 2e-6) * max(abs(lo), 1e-3), (2e-2 if sixteen else 1e-4) * gmax
    print(f"{tag}: loss {loss:.8g} oracle {lo:.8g} err {lerr:.3e} (bar {lbar:.3e}) | grad err {gerr:.3e} (bar {gbar:.3e}, max {gmax:.3e})")
    assert np.isfinite(loss) and np.isfinite(g).all(), tag
    assert lerr <= lbar, (tag, loss, lo)
    assert gerr <= gbar, (tag, gerr, gmax)
    return loss, g


def labelled(n, c, seed, classes=None, p_ignore=0.1, spread=2.0, dtype=torch.float32):
    """logits [n, c] and labels drawn from `classes` (default: all c), a share of them -1"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, generator=g) * spread).to(dtype)
    classes = torch.arange(c) if classes is None else torch.as_tensor(classes)
    y = classes[torch.randint(0, len(classes), (n,), generator=g)]
    y[torch.rand(n, generator=g) < p_ignore] = -1
    return x, y


# ------------------------------------------------------------------------------------------------------------------------ bodies
def check_golden(device):
    for ci, x, y, loss_ref, grad_ref in golden_cases():
        loss, g = check_against_oracle(device, f"golden{ci}", x, y, scale=2.5)
        _, do = oracle(f"golden{ci}", x, y)
        gmax = max(float(np.abs(do).max()), 1e-12)
        print(f"golden{ci}: reference loss {loss_ref:.8g}, err {abs(loss - loss_ref):.3e}; grad vs reference {np.abs(g - grad_ref).max():.3e}")
        assert abs(loss - loss_ref) <= 1e-4 * max(abs(loss_ref), 1e-3), (ci, loss, loss_ref)
        assert np.abs(g - grad_ref).max() <= 1e-3 * gmax, ci


def check_shape(device, n, c, n_classes=None, seed=0):
    """n_classes: labels drawn from that many classes spread over [0, c)"""
    classes = None if n_classes is None else torch.linspace(0, c - 1, n_classes).long().unique()
    x, y = labelled(n, c, 1000 * c + n + seed, classes)
    if n == 1:
        y[0] = c // 2                      # one point, counted
    return check_against_oracle(device, f"shape n={n} c={c} classes={n_classes}", x, y)


def check_label_patterns(device):
    n, c = 257, 200
    x, y = labelled(n, c, 31, classes=[123], p_ignore=0.2)
    check_against_oracle(device, "one present class", x, y)
    x, y = labelled(600, c, 32, p_ignore=0.0)
    y[:c] = torch.arange(c)
    check_against_oracle(device, "every class present", x, y)
    x, y = labelled(n, c, 33, classes=list(range(190, 200)))
    check_against_oracle(device, "present classes 190..199", x, y)
    x, y = labelled(n, c, 34, classes=list(range(5, 40)), p_ignore=0.0)
    y[y == 17] = 18
    y[100] = 17
    check_against_oracle(device, "a class with a single point", x, y)
    for ign in (0, 199):
        x, y = labelled(n, c, 35 + ign, p_ignore=0.0)
        y[::7] = ign
        loss, g = check_against_oracle(device, f"ignore_index {ign} inside the class range", x, y, ignore_index=ign)
        assert float(np.abs(g[::7]).max()) == 0.0
    x, y = labelled(n, c, 36, classes=list(range(0, 50)))
    y[::5] = 200
    y[1::5] = 4000
    y[2::5] = -7
    loss, g = check_against_oracle(device, "labels >= c and negative labels are not counted", x, y)
    assert float(np.abs(g[::5]).max()) == 0.0 and float(np.abs(g[1::5]).max()) == 0.0 and float(np.abs(g[2::5]).max()) == 0.0
    x, _ = labelled(n, c, 37)
    loss, g = run(device, x, torch.full((n,), -1, dtype=torch.int64))
    assert loss == 0.0 and float(np.abs(g).max()) == 0.0 and g.shape == (n, c)
    loss, g = run(device, torch.zeros(0, c), torch.zeros(0, dtype=torch.int64))
    assert loss == 0.0 and g.shape == (0, c)


def check_dtypes_and_layouts(device, n=257):
    c = 200
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        x, y = labelled(n, c, 41, classes=list(range(0, 200, 3)), dtype=dtype)
        check_against_oracle(device, f"dense {dtype}", x, y)
        # a [:, :200] view of a 208-column head output: the gradient of the columns past c is exactly 0
        g = torch.Generator().manual_seed(42)
        wide = (torch.randn(n, 208, generator=g) * 2).to(dtype)
        lo, do = oracle(f"strided {dtype}", wide[:, :c], y)
        we = wide.clone().to(device).requires_grad_(True)
        loss = PF.lovasz_softmax(we[:, :c], y.to(device), -1)
        loss.backward()
        got = we.grad.float().cpu().numpy()
        sixteen = dtype != torch.float32
        print(f"strided {dtype}: loss err {abs(float(loss) - lo):.3e} grad err {np.abs(got[:, :c] - do).max():.3e} of {np.abs(do).max():.3e}")
        assert abs(float(loss) - lo) <= (1e-5 if sixteen else 2e-6) * abs(lo)
        assert np.abs(got[:, :c] - do).max() <= (2e-2 if sixteen else 1e-4) * np.abs(do).max()
        assert float(np.abs(got[:, c:]).max()) == 0.0
        # odd c, base address one element past an aligned one: element-wise loads
        c2 = 101
        x2, y2 = labelled(n, c2, 43, classes=list(range(0, 101, 2)), dtype=dtype)
        lo, do = oracle(f"unaligned {dtype}", x2, y2)
        flat = torch.zeros(n * c2 + 1, dtype=dtype)
        flat[1:] = x2.reshape(-1)
        xd = flat.to(device)[1:].view(n, c2)
        assert xd.data_ptr() % 16 != 0 and xd.is_contiguous()
        loss, dl = ops.lovasz_softmax(xd, y2.to(device), -1)
        dl = dl.cpu().numpy()                          # the op's own fp32 gradient: the fp32 bar
        print(f"unaligned {dtype}: loss err {abs(float(loss) - lo):.3e} grad err {np.abs(dl - do).max():.3e} of {np.abs(do).max():.3e}")
        assert abs(float(loss) - lo) <= (1e-5 if sixteen else 2e-6) * abs(lo)
        assert np.abs(dl - do).max() <= 1e-4 * np.abs(do).max()


def check_nan_workspace(device, n=257, c=200):
    """the C entry points on buffers the caller filled with NaN / 0xff: whatever they do not write shows up"""
    from pointcept_amd._lib import check, dtype_code, lib, ptr

    x, y = labelled(n, c, 51, classes=list(range(3, 90, 2)))
    lo, do = oracle("nan workspace", x, y)
    xd, yd = x.to(device), y.to(device)
    ints = torch.full((3 * c + 1,), -0x01010102, dtype=torch.int32, device=device)
    count, row_of, class_of, n_present = ints[:c], ints[c:2 * c], ints[2 * c:3 * c], ints[3 * c:]
    check(lib().ptc_lovasz_present(ptr(yd), n, c, -1, ptr(count), ptr(row_of), ptr(class_of), ptr(n_present), ops.stream_ptr()), "present")
    rows = int(n_present[0])
    yc = y[y >= 0].numpy()
    assert rows == len(np.unique(yc)) and count.tolist() == np.bincount(yc, minlength=c).tolist()
    assert class_of[:rows].tolist() == sorted(np.unique(yc).tolist()) and class_of[rows:].tolist() == [-1] * (c - rows)
    assert row_of.tolist() == [sorted(np.unique(yc).tolist()).index(j) if j in set(yc.tolist()) else -1 for j in range(c)]
    nbytes = lib().ptc_lovasz_softmax_rows_workspace_bytes(n, c, rows)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
    loss = torch.full((), float("nan"), device=device)
    dl = torch.full((n, c), float("nan"), device=device)
    check(lib().ptc_lovasz_softmax_rows(ptr(xd), c, ptr(yd), n, c, dtype_code(xd), -1, ptr(count), ptr(row_of), ptr(class_of), ptr(n_present),
                                        rows, ptr(loss), ptr(dl), ptr(ws), nbytes, ops.stream_ptr()), "rows")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dl).all())
    assert abs(float(loss) - lo) <= 2e-6 * abs(lo) and np.abs(dl.cpu().numpy() - do).max() <= 1e-4 * np.abs(do).max()
    # nothing counted / no rows: loss 0 and a zero gradient over NaN-filled outputs
    loss.fill_(float("nan"))
    dl.fill_(float("nan"))
    none = torch.full((n,), -1, dtype=torch.int64, device=device)
    check(lib().ptc_lovasz_present(ptr(none), n, c, -1, ptr(count), ptr(row_of), ptr(class_of), ptr(n_present), ops.stream_ptr()), "present")
    assert int(n_present[0]) == 0 and row_of.tolist() == [-1] * c and lib().ptc_lovasz_softmax_rows_workspace_bytes(n, c, 0) == 0
    check(lib().ptc_lovasz_softmax_rows(ptr(xd), c, ptr(none), n, c, dtype_code(xd), -1, ptr(count), ptr(row_of), ptr(class_of), ptr(n_present),
                                        0, ptr(loss), ptr(dl), None, 0, ops.stream_ptr()), "rows")
    assert float(loss) == 0.0 and float(dl.abs().max()) == 0.0


def check_rows_against_dense(device, n, c, n_absent, dtype=torch.float32):
    """the same logits through the dense path (no handle, c <= 64) and the rows path (explicit handle) -> (loss, gradient) differences"""
    x, y = labelled(n, c, 61 + c, classes=list(range(0, c - n_absent)), dtype=dtype)
    xd, yd = x.to(device), y.to(device)
    l0, d0 = ops.lovasz_softmax(xd, yd, -1)
    l1, d1 = ops.lovasz_softmax(xd, yd, -1, present=ops.lovasz_present(yd, c, -1))
    lerr = abs(float(l1) - float(l0)) / abs(float(l0))
    gmax = float(d0.abs().max())
    gerr = float((d1 - d0).abs().max()) / gmax
    print(f"rows vs dense n={n} c={c} absent={n_absent}: loss {float(l1):.8g} vs {float(l0):.8g}, relative {lerr:.3e}; gradient {gerr:.3e} of the largest element")
    assert lerr <= 2e-6 and gerr <= 1e-4
    return lerr, gerr


def check_reproducible(device, n, c, n_classes):
    classes = torch.linspace(0, c - 1, n_classes).long().unique()
    x, y = labelled(n, c, 71, classes)
    xd, yd = x.to(device), y.to(device)
    l0, d0 = ops.lovasz_softmax(xd, yd, -1)
    l1, d1 = ops.lovasz_softmax(xd, yd, -1)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)


def check_refusals(device):
    """all on the host: nothing is launched with a handle that does not describe the call's labels"""
    n = 50
    y = torch.randint(0, 20, (n,), generator=torch.Generator().manual_seed(81)).to(device)
    with pytest.raises(PtcoreError):
        PF.lovasz_softmax(torch.zeros(n, 1025, device=device), y, -1)
    with pytest.raises(PtcoreError):
        PF.lovasz_present(y, 1025, -1)
    x = torch.randn(n, 100, generator=torch.Generator().manual_seed(82)).to(device)
    other = y.clone()
    h = PF.lovasz_present(other, 100, -1)
    with pytest.raises(PtcoreError, match="another target"):
        PF.lovasz_softmax(x, y, -1, present=h)
    assert np.isfinite(float(PF.lovasz_softmax(x, other, -1, present=h)))
    other[3] = 7                                                   # an in-place edit: the version counter moves
    with pytest.raises(PtcoreError, match="edited in place"):
        PF.lovasz_softmax(x, other, -1, present=h)
    h = PF.lovasz_present(y, 100, -1)
    with pytest.raises(PtcoreError):
        PF.lovasz_softmax(x[:, :99], y, -1, present=h)             # another num_classes
    with pytest.raises(PtcoreError):
        PF.lovasz_softmax(x, y, 5, present=h)                      # another ignore_index
    with pytest.raises(PtcoreError):
        PF.lovasz_softmax(x, y, -1, present=object())


def check_segmentor(device, n=3000):
    """DefaultSegmentorV2 at 200 classes: the handle is asked for before the backbone runs; loss and head gradient against the oracle's
    CE + Lovasz.  Bars: the loss 2e-3 relative as test_segmentor_ce_plus_lovasz (the engine's Linear in between); the weight gradient
    2e-3 of its largest element -- a sum over the rows of dlogits x feat through the same Linear arithmetic, relative rounding no worse."""
    from pointcept_amd.segmentor import DefaultSegmentorV2

    calls = []

    class Feat(torch.nn.Module):
        def forward(self, point):
            calls.append("backbone")
            return point["feat"]

    real = ops.lovasz_present

    def recording(*a, **k):
        calls.append("present")
        return real(*a, **k)

    torch.manual_seed(0)
    seg = DefaultSegmentorV2(200, 64, Feat(), criteria=("ce", "lovasz")).to(device).train()
    g = torch.Generator().manual_seed(13)
    feat = torch.randn(n, 64, generator=g)
    y = torch.randint(-1, 60, (n,), generator=g) * 3
    y[y < 0] = -1
    ops.lovasz_present = recording
    try:
        out = seg(dict(feat=feat.to(device), segment=y.to(device), offset=torch.tensor([n], device=device)))
    finally:
        ops.lovasz_present = real
    assert calls == ["present", "backbone"], calls
    out["loss"].backward()
    w, b = seg.seg_head.weight.detach().cpu().double(), seg.seg_head.bias.detach().cpu().double()
    logits = (feat.double() @ w.t() + b).requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(logits, y, ignore_index=-1)
    ce.backward()
    lv, dlv = losses.lovasz_softmax(logits.detach().numpy(), y.numpy(), -1)
    want = float(ce) + lv
    dw = (logits.grad + torch.from_numpy(dlv)).t() @ feat.double()
    got = seg.seg_head.weight.grad.detach().cpu().double()
    print(f"segmentor: loss {float(out['loss']):.8g} oracle {want:.8g}; head gradient err {float((got - dw).abs().max()):.3e} of {float(dw.abs().max()):.3e}")
    assert abs(float(out["loss"]) - want) <= 2e-3 * want
    assert float((got - dw).abs().max()) <= 2e-3 * float(dw.abs().max())


# ------------------------------------------------------------------------------------------------------------------------ GPU entries
def test_golden_cases():
    check_golden(dev())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("c", [65, 100, 101, 200, 1024])
def test_shapes_against_the_oracle(c, n):
    check_shape(dev(), n, c)


def test_more_rows_than_step_workgroups():
    """n = 9000, c = 200, 150 classes present: P * ceil(n / 256) = 5400 > LV_STEP_BLOCKS, lovasz_step's grid-stride loop and the capped partials"""
    x, y = labelled(9000, 200, 72, torch.linspace(0, 199, 150).long().unique())
    assert len(y[y >= 0].unique()) == 150
    check_against_oracle(dev(), "n=9000 c=200 P=150", x, y)


def test_label_patterns():
    check_label_patterns(dev())


def test_dtypes_and_layouts():
    check_dtypes_and_layouts(dev())


def test_nan_filled_workspace_and_outputs():
    check_nan_workspace(dev())


@pytest.mark.parametrize("n,c,n_absent", [(5000, 20, 0), (5000, 20, 7), (5000, 64, 30), (333, 64, 1)])
def test_rows_path_against_the_dense_path(n, c, n_absent):
    check_rows_against_dense(dev(), n, c, n_absent)


def test_reproducible():
    check_reproducible(dev(), 9000, 200, 150)


def test_refusals_happen_on_the_host():
    check_refusals(dev())


def test_segmentor_asks_before_the_backbone_and_matches_the_oracle():
    check_segmentor(dev())


def test_scannet200_shape():
    """n = 819200, c = 200, bf16, 60 classes present: finite, in (0, 1], the same bits twice"""
    n, c = 819200, 200
    g = torch.Generator().manual_seed(91)
    x = torch.randn(n, c, generator=g).to(torch.bfloat16).to(dev())
    y = torch.randint(0, 60, (n,), generator=g) * 3
    y[torch.rand(n, generator=g) < 0.05] = -1
    y = y.to(dev())
    h = ops.lovasz_present(y, c, -1)
    assert h.rows() == 60
    l0, d0 = ops.lovasz_softmax(x, y, -1, present=h)
    l1, d1 = ops.lovasz_softmax(x, y, -1, present=h)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    assert 0.0 < float(l0) <= 1.0 and bool(torch.isfinite(d0).all())
