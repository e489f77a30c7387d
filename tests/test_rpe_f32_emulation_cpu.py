"""-m "not gpu": the fp32 RPE window-attention kernels (csrc/attention_rpe_f32.h) on the host emulation of the kernel sources
(tests/host_emulation, tests/emu_backend.py): the bodies of tests/test_gpu_attention_rpe_f32.py with device = cpu at small shapes --
fragment layouts of the 16x16x4 fp32 MFMA, LDS images, masking, poisoning and the fixed-point table gradient against the float64
reference, before any GPU time is spent."""
import pytest
import torch

import test_gpu_attention_rpe_f32 as T


@pytest.fixture(autouse=True)
def _emulator():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")


@pytest.mark.parametrize("lens,H,bnd", [([33], 1, 4), ([200, 200, 200], 3, 18)], ids=["33_H1_b4", "200x3_H3_b18"])
def test_fp32_rpe_kernels_against_the_float64_reference_on_the_emulation(lens, H, bnd):
    import emu_backend

    with emu_backend.emulated_ops():
        T.check_kernels_against_the_float64_reference(torch.device("cpu"), lens, H, bnd)


def test_fp32_rpe_poisons_an_overlong_window_on_the_emulation():
    import emu_backend

    with emu_backend.emulated_ops():
        T.check_overlong_window_is_poisoned(torch.device("cpu"))


def test_fp32_rpe_empty_batch_on_the_emulation():
    import emu_backend

    with emu_backend.emulated_ops():
        T.check_empty_batch(torch.device("cpu"))


def test_other_attention_entries_still_refuse_fp32_on_the_emulation():
    import emu_backend
    from pointcept_amd import ops
    from pointcept_amd._lib import PtcoreError

    cu = torch.tensor([0, 64], dtype=torch.int32)
    qkv = torch.randn(64, 3, 2, 16)
    with emu_backend.emulated_ops():
        with pytest.raises(PtcoreError):
            ops.attn_varlen_fwd(qkv, cu, 64, 0.25)
