"""-m "not gpu": the SGIFormer decoder kernels (csrc/sgiformer.hip) on the host emulation of the kernel sources (tests/host_emulation,
tests/emu_backend.py) -- the bodies of tests/test_gpu_sgiformer.py with device = cpu at its edge shapes -- plus the port's torch path
(the reference's expression, what CPU tensors take) on the CPU backend against the golden, the port with the kernels on the emulation
against the golden, and the reference's files run live on the stand-ins."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_sgiformer as T

CPU = torch.device("cpu")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("lq,lk", [s for s in T.ATTN_SHAPES if sum(s[0]) < 400])
def test_attention_on_the_emulation(emu, lq, lk, use_mask):
    T.check_attention(CPU, lq, lk, use_mask)


def test_attention_bf16_rows_on_the_emulation(emu):
    T.check_attention(CPU, (48, 3), (33, 64), True, torch.bfloat16)


def test_refusal_on_the_emulation(emu):
    T.check_refusal(CPU)


def test_pack_mask_on_the_emulation(emu):
    T.check_pack_mask(CPU)


def test_targets_on_the_emulation(emu):
    T.check_targets(CPU)


@pytest.mark.parametrize("g_n,m", [(1, 1), (7, 33), (7, 200)])
def test_match_cost_on_the_emulation(emu, g_n, m):
    T.check_match_cost(CPU, g_n, m)


def test_match_cost_nonfinite_on_the_emulation(emu):
    T.check_match_cost_nonfinite(CPU)


def test_keys_defaults_and_registration():
    T.test_state_dict_round_trip_and_keys()
    T.test_constructor_defaults_are_the_references()
    T.test_registered_only_when_named_and_built_from_a_config()


@pytest.mark.parametrize("use_score", [False, True])
def test_port_matches_reference_golden_on_the_host(use_score):
    """CPU tensors always take the torch functions: the port on the CPU backend against the reference files' golden"""
    import mock_backend

    with mock_backend.cpu_ops():
        T.check_port_against_golden(CPU, use_score)


def test_port_kernels_on_the_emulation_match_the_torch_path():
    """the decoder on csrc/sgiformer.hip itself (host emulation) inside the port on the CPU backend: the integers (attention masks,
    targets, matched indices) equal the torch path's; the losses agree to the bf16 operands of the attention"""
    import emu_backend
    import mock_backend
    from pointcept_amd import functional as PF
    from pointcept_amd import synthetic

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    g = T.golden()
    batch = synthetic.to_torch(T.golden_batch(g), CPU)
    with mock_backend.cpu_ops():
        model = T._model(g, CPU, True)
        out_t, _ = T._train_step(g, model, batch)
        matched_t = T._matched(model)
    real = ["sgi_attn_supported", "sgi_attn_fwd", "sgi_attn_bwd", "sgi_pack_mask", "sgi_match_cost", "sgi_targets"]
    saved = PF._sgi_use_kernels
    PF._sgi_use_kernels = lambda t, use_kernels: True
    try:
        with emu_backend.hybrid(real):
            out_k, _ = T._train_step(g, model, batch)
            matched_k = T._matched(model)
    finally:
        PF._sgi_use_kernels = saved
    assert len(matched_k) == len(matched_t)
    for (a, b), (c, d) in zip(matched_k, matched_t):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    for k in T.TRAIN_LOSSES:
        print(k, float(out_k[k]), float(out_t[k]))
        assert abs(float(out_k[k]) - float(out_t[k])) <= 2.0 ** -8 * abs(float(out_t[k])) + 1e-6, k


@pytest.mark.skipif(not os.path.isdir("/root/reference/pointcept"), reason="needs the reference tree")
def test_needs_reference_files_give_the_golden_losses():
    """needs_reference: the reference's files, unmodified, run live on the stand-ins with the fixture's inputs and weights give the
    fixture's losses and matched indices"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_sgiformer as M

    g = T.golden()
    R = M.load_reference_sgiformer()
    inp = M.to_inputs(T.golden_batch(g))
    sd = T.golden_state(g, R.SGIFormer(**M.config(False)), False)
    _, out, rec, _ = M.run_train(R, sd, inp, False)
    for k in T.TRAIN_LOSSES:
        assert float(out[k].detach()) == pytest.approx(float(g[f"score0/out/{k}"]), rel=1e-5), k
    for j, (q, o) in enumerate(rec.matched):
        assert np.array_equal(q, g[f"score0/matched/{j}/query"]) and np.array_equal(o, g[f"score0/matched/{j}/object"])
