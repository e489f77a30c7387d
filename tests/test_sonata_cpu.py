"""-m "not gpu": Sonata-v1m1's distillation loss (csrc/sonata.hip) on the host emulation of the kernel sources -- the bodies of
tests/test_gpu_sonata.py with device = cpu at small shapes -- plus the port's torch path on the CPU backend against the golden and,
where the reference tree exists, against the reference's own sinkhorn_knopp."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_sonata as S

CPU = torch.device("cpu")
HAS_REFERENCE = os.path.isdir("/root/reference/pointcept")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("m,k,tt,dtype", [(1, 64, 0.04, torch.float32), (63, 64, 0.07, torch.bfloat16), (65, 192, 0.04, torch.float32),
                                          (40, 192, 0.07, torch.float16), (9, 4096, 0.04, torch.float32), (5, 8192, 0.07, torch.bfloat16)])
def test_distill_on_the_emulation(emu, m, k, tt, dtype):
    S.check_distill(CPU, m, k, tt, dtype)


@pytest.mark.parametrize("m,k,tt,dtype,cap", [(1, 64, 0.04, torch.float32, 0), (65, 192, 0.04, torch.bfloat16, 3), (70, 1088, 0.07, torch.float32, 1),
                                              (9, 4096, 0.04, torch.float32, 2)])
def test_scaling_vectors_on_the_emulation(emu, m, k, tt, dtype, cap):
    S.check_scaling_vectors(CPU, m, k, tt, dtype, cap)


def test_divisor_on_the_emulation(emu):
    S.check_divisor(CPU)


def test_no_pairs_on_the_emulation(emu, monkeypatch):
    S.check_empty(CPU, monkeypatch)


def test_unsupported_k_on_the_emulation(emu):
    S.check_unsupported_k(CPU)


def test_reproducible_on_the_emulation(emu):
    S.check_reproducible(CPU, 100, 192)


def test_permutation_on_the_emulation(emu):
    S.check_permutation(CPU, 120, 192, 0.04)


def test_sharded_on_the_emulation(emu):
    S.check_sharded(CPU, 60, 192, 0.04, 3)


def test_rows_outside_their_tensor_are_left_out(emu):
    """a pair that names a row past the end of either tensor reads and writes nothing and contributes nothing"""
    from pointcept_amd import ops

    t, s, mi, sb = S.distill_inputs(CPU, 20, 64)
    bad = mi.clone()
    bad[3, 1] = t.shape[0]
    bad[7, 1] = -1
    keep = torch.ones(20, dtype=torch.bool)
    keep[[3, 7]] = False
    r = ops.sonata_colsum(t, bad, 0.07)
    assert torch.allclose(r, ops.sonata_colsum(t, mi[keep], 0.07), rtol=1e-6, atol=0)      # other tiles: another summation order
    c, b, _ = ops.sonata_rowpass(t, bad, 0.07, torch.reciprocal(r * 64), 18)
    assert c[3] == 0 and b[7] == 0 and bool((c[keep] > 0).all())
    bad[5, 0] = s.shape[0]
    loss, _, state = ops.sonata_distill_fwd(t, s, bad, sb, S.SCENES, 0.07, 0.1, torch.reciprocal(r * 64))
    d = ops.sonata_distill_bwd(state, 0.07, 0.1, torch.ones(1))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d).all())
    assert not bool(d[mi[[3, 5, 7], 0]].any()) and bool(d[mi[0, 0]].any())


def test_config_flag_and_cpu_tensors_take_the_torch_path(monkeypatch):
    from pointcept_amd import config
    from pointcept_amd import functional as PF

    assert config.SONATA_KERNELS is True and "PTC_SONATA=0" in config.__doc__
    t, s, mi, sb = S.distill_inputs(CPU, 30, 64)
    a = S._run(PF.sonata_distill, t, s, mi, sb, 0.07)                 # CPU tensors outside the emulation: no kernel exists for them
    b = S._run(PF.sonata_distill_torch, t, s, mi, sb, 0.07)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    d = S._run(PF.sonata_distill_torch, t.double(), s.double(), mi, sb, 0.07)
    assert d[0].dtype == torch.float64 and abs(float(d[0]) - float(b[0])) < 1e-5


def _generator():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_sonata as M

    return M


@pytest.mark.skipif(not HAS_REFERENCE, reason="needs the reference tree")
@pytest.mark.parametrize("m,k,tt", [(1, 64, 0.07), (50, 64, 0.04), (200, 192, 0.07)])
def test_needs_reference_sinkhorn_is_the_references(m, k, tt):
    """needs_reference: functional.sonata_sinkhorn_torch against Sonata.sinkhorn_knopp of the reference's file called directly"""
    from pointcept_amd import functional as PF

    R = _generator().load_reference_sonata()
    t, _, mi, _ = S.distill_inputs(CPU, m, k)
    ref = R.Sonata.sinkhorn_knopp(t[mi[:, 1]], tt)
    got = PF.sonata_sinkhorn_torch(t[mi[:, 1]], tt)
    assert torch.allclose(got, ref, rtol=1e-6, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- model
def test_scheduler_matches_the_numpy_schedule():
    """warm-up by linspace (both ends), half a cosine, the final value from total_iters on"""
    from pointcept_amd.sonata import CosineScheduler

    for start, base, final, warm, total in ((0.1, 0.4, 0.4, 5, 100), (0.04, 0.07, 0.07, 1, 20), (0, 0.996, 1.0, 0, 50)):
        s = CosineScheduler(start_value=start, base_value=base, final_value=final, warmup_iters=warm, total_iters=total)
        it = np.arange(total - warm)
        want = np.concatenate([np.linspace(start, base, warm), final + 0.5 * (base - final) * (1 + np.cos(np.pi * it / len(it)))])
        got = np.asarray([s.step() for _ in range(total + 3)])
        assert np.allclose(got[:total], want, rtol=1e-12, atol=1e-15) and np.all(got[total:] == final) and s.iter == total + 3
        assert s[0] == got[0] and s.get(total) == final


def test_registration_and_state_dict_keys():
    S.test_registered_only_when_named()
    import mock_backend

    with mock_backend.cpu_ops():
        S.check_state_dict_keys()


def test_port_matches_reference_golden_on_the_host(monkeypatch):
    """PTC_SONATA=0 on the CPU backend against the reference run"""
    import mock_backend
    from pointcept_amd import config

    monkeypatch.setattr(config, "SONATA_KERNELS", False)
    with mock_backend.cpu_ops():
        S.check_port_against_golden(CPU)


def test_golden_losses_from_the_kernels_on_the_emulation(monkeypatch):
    """the same run with the three losses on csrc/sonata.hip (host emulation), the backbone on its CPU stand-ins"""
    import emu_backend
    from pointcept_amd import functional as PF
    from pointcept_amd import sonata

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    calls = []

    def distill(*a, **k):
        calls.append(a[2].shape[0])
        return PF.sonata_distill(*a, **dict(k, use_kernels=True))

    monkeypatch.setattr(sonata, "PF", type("PFk", (), {"sonata_distill": staticmethod(distill), "sonata_sinkhorn_torch": PF.sonata_sinkhorn_torch}))
    with emu_backend.hybrid(["sonata_supported", "sonata_colsum", "sonata_rowpass", "sonata_distill_fwd", "sonata_distill_bwd"]):
        S.check_port_against_golden(CPU)
    assert len(calls) == 3 and min(calls) > 0


def test_ema_on_the_host():
    import mock_backend

    with mock_backend.cpu_ops():
        S.check_ema(CPU)


def test_return_point_on_the_host():
    import mock_backend

    with mock_backend.cpu_ops():
        S.check_return_point(CPU)


@pytest.mark.parametrize("name", ["few_empty_dense", "k_kplus1_dup_boundary", "m_zero", "n_zero", "nan_rows", "wild_extent_grows_cells"])
def test_match_neighbour_on_the_emulation(emu, name):
    S.check_match_neighbour(CPU, name)


def test_generate_mask_on_the_emulation(emu):
    assert S.check_generate_mask(CPU, 0.4, 0.7) > 20


def test_bf16_autocast_step_on_the_host(monkeypatch):
    import mock_backend
    from pointcept_amd import config

    monkeypatch.setattr(config, "SONATA_KERNELS", False)
    with mock_backend.cpu_ops():
        S.check_autocast_step(CPU)


@pytest.mark.skipif(not HAS_REFERENCE, reason="needs the reference tree")
def test_needs_reference_golden_regenerates():
    """needs_reference: the committed fixture is what the reference's file computes now.  Its forward is reproducible to the bit; the
    backward of the CPU stand-ins accumulates in thread order, and two runs of the generator differ by up to 1.5e-4 of a gradient norm
    (measured: mask_token), so the gradients are compared at 1e-3 of their largest entry"""
    M = _generator()
    g = S.golden()
    res = M.generate()
    assert sorted(res) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(res[k]), g[k]
        if k == "grad_norms" or k.startswith("grad/"):
            assert np.abs(a - b).max() <= 1e-3 * np.abs(b).max(), k
        elif a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=1e-6, atol=1e-7), k
        else:
            assert np.array_equal(a, b), k
    assert M.CFG == S.GOLD_CFG
