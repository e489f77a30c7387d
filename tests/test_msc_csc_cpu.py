"""-m "not gpu": MSC-v1m2's partitioned InfoNCE (csrc/msc.hip section 5) on the host emulation of the kernel sources -- the bodies
of tests/test_gpu_msc_csc.py with device = cpu at small shapes -- plus the port's torch path (PTC_MSC=0) on the CPU backend against
the golden, and, where the reference tree exists, the golden's regeneration and functional.msc_csc_nce_torch against the
reference's own compute_contrastive_loss."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_msc as T
import test_gpu_msc_csc as C

CPU = torch.device("cpu")
HAS_REFERENCE = os.path.isdir("/root/reference/pointcept")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("mode", sorted(C.RADII))
@pytest.mark.parametrize("sizes,c,t", [((1,), 32, 0.4), ((1, 17, 64, 65), 96, 0.07), ((40, 0, 30), 32, 0.07), ((150,), 96, 0.4), ((70, 3), 132, 0.4)])
def test_csc_nce_on_the_emulation(emu, sizes, c, t, mode):
    C.check_csc(CPU, sizes, c, t, mode)


def test_single_scene_reduces_to_msc_nce_on_the_emulation(emu):
    C.check_single_scene_reduction(CPU, 1, 32, 0.4)
    C.check_single_scene_reduction(CPU, 130, 96, 0.07)


def test_permutation_on_the_emulation(emu):
    C.check_permutation(CPU, (1, 17, 64, 65), 96, 0.4)


def test_reproducible_on_the_emulation(emu):
    C.check_reproducible(CPU, (70, 0, 90), 96, 0.4)


def test_dropped_pairs_on_the_emulation(emu):
    """a pair whose view-1 row lies beyond the last offset belongs to no scene: it is left out, as if it were not listed"""
    from pointcept_amd import functional as PF

    f1, x1, off1, f2, x2, mi = C.csc_inputs(CPU, (20, 30), 32, seed=6)
    r1, r2 = C.RADII["all"]
    full = C._run_csc(PF.msc_csc_nce, f1, x1, off1, f2, x2, mi, 0.4, r1, r2)
    first = mi[:, 0] < int(off1[0])
    cut = C._run_csc(PF.msc_csc_nce, f1, x1, off1[:1], f2, x2, mi, 0.4, r1, r2)
    only = C._run_csc(PF.msc_csc_nce, f1, x1, off1[:1], f2, x2, mi[first], 0.4, r1, r2)
    for a, b in zip(cut, only):
        assert torch.equal(a, b)
    assert not torch.equal(full[0], cut[0])


def test_refuses_what_it_does_not_implement(emu):
    from pointcept_amd import functional as PF
    from pointcept_amd._lib import PtcoreError

    f1, x1, off1, f2, x2, mi = C.csc_inputs(CPU, (5, 6), 32)
    ok = lambda **k: PF.msc_csc_nce(k.get("f1", f1), k.get("x1", x1), off1, k.get("f2", f2), x2, k.get("mi", mi), 0.4, k.get("r1", 0.1), k.get("r2", 0.5))
    assert bool(torch.isfinite(ok()[0]))
    with pytest.raises(PtcoreError):
        ok(r1=0.6)                                                   # r1 > r2
    with pytest.raises(PtcoreError):
        ok(f1=f1[:, :30], f2=f2[:, :30])                             # C not a multiple of 4
    with pytest.raises(PtcoreError):
        ok(f1=torch.randn(f1.shape[0], 260), f2=torch.randn(f2.shape[0], 260))
    with pytest.raises(PtcoreError):
        ok(mi=mi[:0])                                                # P < 1
    with pytest.raises(PtcoreError):
        ok(x1=x1[:-1])
    from pointcept_amd import ops

    with pytest.raises(PtcoreError):
        ops.msc_csc_nce_fwd(f1.half(), x1, off1, f2.half(), x2, mi, 0.4, 0.1, 0.5)      # the functional casts up; the op takes fp32 only
    with pytest.raises(PtcoreError):
        ops.msc_csc_nce_fwd(f1.double(), x1, off1, f2.double(), x2, mi, 0.4, 0.1, 0.5)


def test_registration_and_state_dict_keys():
    C.test_registered_only_when_named()
    import mock_backend

    with mock_backend.cpu_ops():
        C.test_state_dict_keys_are_the_references()


def test_port_matches_reference_golden_on_the_host(monkeypatch):
    """PTC_MSC=0 on the CPU backend against the v1m2 reference run"""
    import mock_backend
    from pointcept_amd import config

    monkeypatch.setattr(config, "MSC_KERNELS", False)
    with mock_backend.cpu_ops():
        C.check_port_against_golden(CPU)


def test_golden_loss_from_the_kernels_on_the_emulation(emu):
    """the fixture's match_index and coordinates through csrc/msc.hip itself: its class histogram exactly, and, on random features,
    the torch path's loss"""
    from pointcept_amd import functional as PF
    from pointcept_amd import ops, synthetic

    g = C.golden()
    b = synthetic.to_torch(T.golden_batch(g), CPU)
    mi = torch.from_numpy(g["match_index"])
    gen = torch.Generator().manual_seed(0)
    f1 = torch.randn(b["view1_origin_coord"].shape[0], 32, generator=gen)
    f2 = torch.randn(b["view2_origin_coord"].shape[0], 32, generator=gen)
    args = (b["view1_origin_coord"], b["view1_offset"], f2, b["view2_origin_coord"], mi, 0.4, float(g["r1"]), float(g["r2"]))
    out, counts, _ = ops.msc_csc_nce_fwd(f1, *args)
    assert np.array_equal(counts.numpy(), g["class_hist"])
    ref = PF.msc_csc_nce_torch(f1.double(), args[0], args[1], f2.double(), *args[3:])
    assert abs(float(out[0]) - float(ref[0])) <= 1e-5 * abs(float(ref[0]))


def test_config_recipe_on_the_host(monkeypatch):
    import mock_backend
    from pointcept_amd import config

    monkeypatch.setattr(config, "MSC_KERNELS", False)
    with mock_backend.cpu_ops():
        C.check_config_recipe(CPU, [1500, 1200])


def _generator():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_msc_csc as M

    return M


@pytest.mark.skipif(not HAS_REFERENCE, reason="needs the reference tree")
def test_needs_reference_golden_regenerates():
    """needs_reference: the committed fixture is what the reference's v1m2 file computes now"""
    M = _generator()
    g = C.golden()
    res = M.generate()
    assert sorted(res) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(res[k]), g[k]
        if a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=1e-6, atol=1e-7), k
        else:
            assert np.array_equal(a, b), k


@pytest.mark.skipif(not HAS_REFERENCE, reason="needs the reference tree")
@pytest.mark.parametrize("mode", sorted(C.RADII))
def test_needs_reference_torch_expression_is_the_references(mode):
    """needs_reference: functional.msc_csc_nce_torch against compute_contrastive_loss of the reference's file called directly, on
    shuffled multi-scene input with an empty scene and a scene of one pair: values and gradients"""
    from pointcept_amd import functional as PF

    M = _generator()
    R = M.load_reference_msc_csc()
    r1, r2 = C.RADII[mode]
    f1, x1, off1, f2, x2, mi = C.csc_inputs(CPU, (40, 0, 1, 25), 32, seed=7)
    this = SimpleSelf(R, nce_t=0.07, r1=r1, r2=r2, partitions=4)
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    with M.G.recorded_draws():                                       # its no-op Tensor.cuda
        ref = R.MaskedSceneContrast.compute_contrastive_loss(this, a, x1, off1, b, x2, off1, mi)
    ref[0].backward()
    got = C._run_csc(PF.msc_csc_nce_torch, f1, x1, off1, f2, x2, mi, 0.07, r1, r2)
    for name, x, y in zip(("loss", "pos_sim", "neg_sim", "dfeat1", "dfeat2"), got, [ref[0].detach(), ref[1], ref[2], a.grad, b.grad]):
        assert torch.allclose(x, y, rtol=1e-6, atol=1e-7 * max(1.0, float(y.abs().max()))), name


class SimpleSelf:
    """the attributes compute_contrastive_loss and compute_partitions read from the model"""

    def __init__(self, R, **kw):
        self.__dict__.update(kw)
        self.nce_criteria = torch.nn.CrossEntropyLoss(reduction="mean")
        self.compute_partitions = lambda c1, c2: R.MaskedSceneContrast.compute_partitions(self, c1, c2)
