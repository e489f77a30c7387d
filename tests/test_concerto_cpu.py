"""-m "not gpu": Concerto-v1m1's alignment kernels (csrc/concerto.hip) on the host emulation of the kernel sources -- the bodies of
tests/test_gpu_concerto.py with device = cpu at their small shapes -- plus the port's torch path on the CPU backend against the golden
and, where the reference tree exists, the twin of pool_corr against the reference's own static method."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_concerto as C

CPU = torch.device("cpu")
HAS_REFERENCE = os.path.isdir("/root/reference/pointcept")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("m,v,dtype", [(1, 1, torch.int64), (1, 0, torch.int64), (255, 3, torch.int64), (257, 5, torch.int32),
                                       (257, 3, torch.float32), (255, 0, torch.float32)])
def test_pool_corr_on_the_emulation(emu, m, v, dtype):
    C.check_pool_corr(CPU, m, v, dtype)


@pytest.mark.parametrize("ns,v,img_nums", [(1, 1, (1,)), (40, 3, (3, 2)), (257, 5, (5, 4)), (10, 0, (0, 0))])
def test_patch_pairs_on_the_emulation(emu, ns, v, img_nums):
    C.check_patch_pairs(CPU, ns, v, img_nums)


def test_patch_pairs_edge_cases_on_the_emulation(emu):
    C.check_patch_pairs_edge_cases(CPU)


@pytest.mark.parametrize("c,dtype", [(3, torch.float32), (96, torch.bfloat16), (1184, torch.float32)])
def test_patch_mean_on_the_emulation(emu, c, dtype):
    C.check_patch_mean(CPU, c, dtype)


def test_same_patch_through_two_views_on_the_emulation(emu):
    C.check_same_patch_twice(CPU)


@pytest.mark.parametrize("u,d,shift,xd,yd", [(1, 6, True, torch.float32, torch.float32), (63, 100, True, torch.bfloat16, torch.bfloat16),
                                             (65, 384, False, torch.float16, torch.float32), (5, 1024, True, torch.float32, torch.float32),
                                             (9, 1536, True, torch.bfloat16, torch.bfloat16), (6, 1536, False, torch.float32, torch.float32),
                                             (65, 6, False, torch.bfloat16, torch.bfloat16)])
def test_align_loss_on_the_emulation(emu, u, d, shift, xd, yd):
    C.check_align(CPU, u, d, shift, xd, yd)


def test_align_special_cases_on_the_emulation(emu):
    C.check_align_special(CPU)


def test_config_flag_and_cpu_tensors_take_the_torch_path():
    from pointcept_amd import config
    from pointcept_amd import functional as PF

    assert config.CONCERTO_KERNELS is True and "PTC_CONCERTO=0" in config.__doc__
    x, ids, y = C.align_case(CPU, 20, 100, True, torch.float32, torch.float32)
    a = C._align_run(PF.concerto_align_loss, x, ids, y, True)           # CPU tensors outside the emulation: no kernel exists for them
    b = C._align_run(PF.concerto_align_loss_torch, x, ids, y, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    corr, perm, idx_ptr = C.corr_case(9, 3, torch.int64)
    assert torch.equal(PF.concerto_pool_corr(corr, perm, idx_ptr), PF.concerto_pool_corr_torch(corr, perm, idx_ptr))


def test_cosine_clamp_is_the_installed_torchs():
    """the facts about torch.nn.CosineSimilarity the kernel relies on, read from the installed torch: each norm is clamped at eps on
    its own, and the clamp passes the gradient at |y| == eps"""
    cos = torch.nn.CosineSimilarity(dim=1, eps=1e-6)
    assert abs(float(cos(torch.tensor([[1e-8, 0.0]]), torch.tensor([[1e3, 0.0]]))) - 0.01) < 1e-6      # one clamp per operand
    y = torch.tensor([[0.0, 0.0]], requires_grad=True)
    cos(torch.tensor([[1.0, 0.0]]), y).sum().backward()
    assert y.grad.tolist() == [[1e6, 0.0]]                                # below eps: x / |x| / eps
    y = torch.tensor([[1e-6, 0.0]], requires_grad=True)
    cos(torch.tensor([[1.0, 0.0]]), y).sum().backward()
    assert y.grad.abs().max() < 1e-3                                       # at eps: the unclamped gradient (0 along y)


def _generator():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_concerto as M

    return M


@pytest.mark.skipif(not HAS_REFERENCE, reason="needs the reference tree")
@pytest.mark.parametrize("m,v,dtype", [(9, 3, torch.int64), (257, 5, torch.float32), (40, 0, torch.int64)])
def test_needs_reference_pool_corr_twin_is_the_references(m, v, dtype):
    """needs_reference: functional.concerto_pool_corr_torch against Concerto.pool_corr of the reference's file, two levels"""
    from pointcept_amd import functional as PF

    saved = torch.Tensor.cuda
    try:
        M = _generator()
        R = M.load_reference_concerto()
        Point = sys.modules["pointcept.models.utils.structure"].Point
        corr, perm, idx_ptr = C.corr_case(m, v, dtype)
        inverse = torch.empty_like(perm)
        inverse[perm] = torch.repeat_interleave(torch.arange(m), idx_ptr[1:] - idx_ptr[:-1])
        m2 = -(-m // 3)
        inverse2 = torch.arange(m) // 3
        idx_ptr2 = torch.tensor([min(3 * i, m) for i in range(m2 + 1)])
        top = Point(dict(offset=torch.tensor([inverse.numel()]), feat=torch.zeros(inverse.numel(), 1)))
        mid = Point(dict(offset=torch.tensor([m]), feat=torch.zeros(m, 1), pooling_inverse=inverse, idx_ptr=idx_ptr, pooling_parent=top))
        low = Point(dict(offset=torch.tensor([m2]), feat=torch.zeros(m2, 1), pooling_inverse=inverse2, idx_ptr=idx_ptr2, pooling_parent=mid))
        ref = R.Concerto.pool_corr(low, corr)["correspondence"]
        one = PF.concerto_pool_corr_torch(corr, perm, idx_ptr)
        two = PF.concerto_pool_corr_torch(one, torch.arange(m), idx_ptr2)
        assert two.shape == ref.shape and torch.allclose(two, ref.to(two.dtype), rtol=1e-6, atol=0)
    finally:
        torch.Tensor.cuda = saved


# ---------------------------------------------------------------------------------------------------------------- model
def test_registration_and_state_dict_keys():
    C.test_registered_only_when_named()
    import mock_backend

    with mock_backend.cpu_ops():
        C.check_state_dict_keys()


def test_port_matches_reference_golden_on_the_host(monkeypatch):
    """PTC_CONCERTO=0 / PTC_SONATA=0 on the CPU backend against the reference run"""
    import mock_backend
    from pointcept_amd import config

    monkeypatch.setattr(config, "SONATA_KERNELS", False)
    monkeypatch.setattr(config, "CONCERTO_KERNELS", False)
    with mock_backend.cpu_ops():
        C.check_port_against_golden(CPU)


def test_golden_alignment_from_the_kernels_on_the_emulation(monkeypatch):
    """the same run with the 2D-3D branch on csrc/concerto.hip (host emulation), everything else on its CPU stand-ins"""
    import emu_backend
    from pointcept_amd import config

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    monkeypatch.setattr(config, "SONATA_KERNELS", False)
    with emu_backend.hybrid(["concerto_pool_corr", "concerto_patch_pairs", "concerto_patch_mean_bwd", "concerto_align_supported",
                             "concerto_align", "sort_keys", "segment_csr_fwd"]):
        C.check_port_against_golden(CPU, force_kernels=True)


def test_zero_image_batch_on_the_host(monkeypatch):
    import mock_backend
    from pointcept_amd import config

    monkeypatch.setattr(config, "SONATA_KERNELS", False)
    with mock_backend.cpu_ops():
        C.check_zero_image_batch(CPU)


def test_return_point_and_after_step_on_the_host():
    import mock_backend

    with mock_backend.cpu_ops():
        C.check_return_point(CPU)
        C.check_after_step(CPU)


def test_enc2d_forward_conventions():
    """RADIO's (summary, features) tuple, SigLIP's vision_model, and the last patch_h * patch_w tokens of last_hidden_state"""
    import types

    from pointcept_amd.concerto import Concerto

    tokens = torch.arange(2 * 9 * 4, dtype=torch.float32).view(2, 9, 4)
    this = types.SimpleNamespace(patch_h=2, patch_w=3, _num_channels=4, image_weight_name="dinov2",
                                 enc2d_model=lambda x: types.SimpleNamespace(last_hidden_state=tokens))
    assert torch.equal(Concerto.ENC2D_forward(this, None), tokens[:, 3:])
    this.image_weight_name, this.enc2d_model = "c-radio", (lambda x: (None, tokens[:, :6].reshape(12, 4)))
    assert torch.equal(Concerto.ENC2D_forward(this, None), tokens[:, :6])
    this.image_weight_name = "siglip2"
    this.enc2d_model = types.SimpleNamespace(vision_model=lambda x: types.SimpleNamespace(last_hidden_state=tokens[:, :6]))
    assert torch.equal(Concerto.ENC2D_forward(this, None), tokens[:, :6])


@pytest.mark.skipif(not HAS_REFERENCE, reason="needs the reference tree")
def test_needs_reference_golden_regenerates():
    """needs_reference: the committed fixture is what the reference's file computes now (gradients at 1e-3 of their largest entry: the
    backward of the CPU stand-ins accumulates in thread order, see tests/test_sonata_cpu.py)"""
    saved = torch.Tensor.cuda
    try:
        M = _generator()
        g = C.golden()
        res = M.generate()
    finally:
        torch.Tensor.cuda = saved
    assert sorted(res) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(res[k]), g[k]
        if k == "grad_norms" or k.startswith("grad/"):
            assert np.abs(a - b).max() <= 1e-3 * np.abs(b).max(), k
        elif a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=1e-6, atol=1e-7), k
        else:
            assert np.array_equal(a, b), k
    assert M.CFG == C.GOLD_CFG
