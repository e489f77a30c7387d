"""-m "not gpu": the context-aware classifier's kernels (csrc/cac.hip) on the host emulation of the kernel sources
(tests/host_emulation, tests/emu_backend.py) -- the bodies of tests/test_gpu_cac.py with device = cpu at small shapes: the four
Functions and their gradients against float64 under the same tolerance rule, the gate and class counts exactly, the designed cases,
bit-reproducibility, refusal -- plus the port's torch path (PTC_CAC=0) on the CPU backend against the golden, and the reference file
itself run live on the stand-ins."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_cac as T

CPU = torch.device("cpu")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("sizes,k,c,thresh,detach", [((100,), 2, 32, 0.0, False), ((70, 1, 133, 45), 20, 48, 0.75, False),
                                                     ((150,), 24, 32, 0.75, True), ((40, 300), 200, 96, 0.75, False)])
def test_pool_soft_on_the_emulation(emu, sizes, k, c, thresh, detach):
    T.check_pool_soft(CPU, sizes, k, c, thresh, detach)


@pytest.mark.parametrize("n,k,c", [(150, 2, 32), (333, 24, 48), (300, 200, 96)])
def test_pool_hard_on_the_emulation(emu, n, k, c):
    T.check_pool_hard(CPU, n, k, c)


@pytest.mark.parametrize("sizes,k,c", [((100,), 2, 32), ((70, 1, 133, 45), 20, 48), ((40, 300), 200, 96)])
def test_cos_on_the_emulation(emu, sizes, k, c):
    T.check_cos(CPU, sizes, k, c)


def test_cos_shared_prototypes_on_the_emulation(emu):
    T.check_cos(CPU, (150,), 24, 32, shared=True)


@pytest.mark.parametrize("n,k,eps", [(150, 2, 0.0), (333, 24, 0.1), (300, 200, 0.0)])
def test_distill_on_the_emulation(emu, n, k, eps):
    T.check_distill(CPU, n, k, eps)


def test_designed_cases_on_the_emulation(emu):
    T.designed(CPU)


def test_reproducible_on_the_emulation(emu):
    T.check_reproducible(CPU, 700, 20, 32)


def test_refusal_on_the_emulation(emu):
    T.check_refusal(CPU)


def test_registration_and_state_dict_keys():
    T.test_registered_only_when_named()
    T.test_criteria_are_mapped_or_refused_by_name()
    T.test_state_dict_keys_are_the_references()


def test_port_matches_reference_golden_on_the_host():
    """CPU tensors always take the torch functions: the port on the CPU backend against the reference file's golden"""
    import mock_backend

    with mock_backend.cpu_ops():
        T.check_port_against_golden(CPU)


def test_port_kernels_match_reference_golden_on_the_emulation():
    """the three stages on csrc/cac.hip itself (host emulation) inside the port on the CPU backend, against the golden"""
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    from pointcept_amd.context_aware_classifier import CACSegmentor

    real = ["cac_supported", "cac_pool_fwd", "cac_pool_bwd", "cac_cos_fwd", "cac_cos_bwd", "cac_distill_fwd", "cac_distill_bwd"]
    saved = CACSegmentor._kernels
    CACSegmentor._kernels = lambda self, feat: True
    try:
        with emu_backend.hybrid(real):
            T.check_port_against_golden(CPU)
    finally:
        CACSegmentor._kernels = saved


@pytest.mark.skipif(not os.path.isdir("/root/reference/pointcept"), reason="needs the reference tree")
def test_needs_reference_file_gives_the_golden_losses():
    """needs_reference: the reference file, unmodified, run live on the stand-ins with the fixture's inputs and weights gives the
    fixture's losses"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_cac as M

    g = T.golden()
    R = M.load_reference_cac()
    inp = {k: torch.from_numpy(np.asarray(v)) for k, v in T.golden_batch(g).items()}
    for detach in (True, False):
        ref0 = R.CACSegmentor(**M.CFG)
        _, out = M.run_train(R, T.golden_state(g, ref0), inp, detach)
        for k in T.TRAIN_LOSSES:
            assert float(out[k].detach()) == pytest.approx(float(g[f"detach{int(detach)}/out/{k}"]), rel=1e-6), k
    _, with_labels, _ = M.run_eval(R, T.golden_state(g, R.CACSegmentor(**M.CFG)), inp)
    assert float(with_labels["loss"]) == pytest.approx(float(g["eval/loss"]), rel=1e-6)
