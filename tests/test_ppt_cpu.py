"""-m "not gpu": Point Prompt Training on the host -- the language-guided head's kernels (csrc/ppt.hip) on the host emulation of the
kernel sources (tests/host_emulation, tests/emu_backend.py): the bodies of tests/test_gpu_ppt.py with device = cpu at the same small
shapes; the model-level bodies (SpUNet-v1m3, PPT-v1m1 / -v1m2 / -v1m3) on the CPU backend (tests/mock_backend.py) against the golden
recorded from the reference's own files."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_ppt as T

CPU = torch.device("cpu")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,c,d,k", T.SHAPES)
def test_head_on_the_emulation(emu, n, c, d, k, dtype):
    T.check_head(CPU, n, c, d, k, dtype, eps=0.0 if k == 25 else 1e-12)


def test_head_f16_on_the_emulation(emu):
    T.check_head(CPU, 333, 64, 512, 20, torch.float16, eps=1e-6)


def test_designed_cases_on_the_emulation(emu):
    T.check_ill_conditioned(CPU)
    T.check_zero_row(CPU)
    T.check_head(CPU, 100, 32, 64, 1, torch.float32, eps=1e-12, seed=4)
    T.check_selection(CPU)
    T.check_ignored_rows(CPU)


def test_reproducible_on_the_emulation(emu):
    T.check_reproducible(CPU, 700, 64, 128, 20)
    T.check_reproducible(CPU, 700, 64, 128, 20, torch.bfloat16)


def test_refusal_and_logit_scale_on_the_emulation(emu):
    T.check_refusal(CPU)
    T.check_logit_scale_grad(CPU)


def test_registration_state_dict_keys_and_construction(monkeypatch):
    T.test_registered_only_when_named()
    T.test_state_dict_keys_are_the_references()
    T.test_zero_init()
    T.test_criteria_are_mapped_or_refused_by_name()
    T.test_clip_fallback_and_its_error(monkeypatch)


def test_port_matches_reference_golden_on_the_host():
    """CPU tensors take functional.ppt_head_torch and the three-step norm: the port on the CPU backend against the reference files' golden"""
    import mock_backend

    with mock_backend.cpu_ops():
        T.check_port_against_golden(CPU)
        T.check_condition_forms(CPU)
        T.check_v1m3_module(CPU)
        T.check_v1m3_head_against_golden(CPU)


def test_port_head_kernels_match_reference_golden_on_the_emulation(monkeypatch):
    """the language-guided head on csrc/ppt.hip itself (host emulation) inside PPT-v1m1 on the CPU backend, against the golden"""
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    from pointcept_amd import functional as PF

    calls = []
    real = PF.ppt_head
    monkeypatch.setattr(PF, "ppt_head", lambda *a, **k: (calls.append(1), real(*a, **dict(k, use_kernels=True)))[1])
    with emu_backend.hybrid(["ppt_head_supported", "ppt_head_fwd", "ppt_head_bwd"]):
        T.check_port_against_golden(CPU, tags=("v1m1",))
        T.check_v1m3_head_against_golden(CPU, use_kernels=True)
    assert len(calls) == 7          # 2 conditions x (train, eval with labels, eval without) + the v1m3 head


@pytest.mark.skipif(not os.path.isdir("/root/reference/pointcept"), reason="needs the reference tree")
def test_needs_reference_files_give_the_golden_losses():
    """needs_reference: the reference files, unmodified, run live on the stand-ins with the fixture's inputs and weights give the
    fixture's losses"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_ppt as M

    g = T.golden()
    R = M.load_reference_ppt()
    inp = {k: v for k, v in T.golden_batch(g, CPU, "ScanNet").items()}
    for tag, cls in R.items():
        sd = M.state_dict_for(M.build(cls))
        assert list(sd.keys()) == [str(k) for k in g[f"{tag}/keys"]]
        _, out = M.run_train(cls, sd, inp)
        assert float(out["loss"].detach()) == pytest.approx(float(g[f"{tag}/ScanNet/loss"]), rel=1e-6), tag
