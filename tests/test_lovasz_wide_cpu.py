"""-m "not gpu": the row-compacted Lovasz-Softmax kernels (csrc/lovasz.hip: lovasz_count / _rank / _keys_wide / _step_rows /
_finish_rows / _dlogits_wide around the segmented sort) on the host emulation of the kernel sources (tests/host_emulation,
tests/emu_backend.py) -- the bodies of tests/test_gpu_lovasz_wide.py with device = cpu at small shapes, under the same bars; the
refusals and the segmentor on the CPU backend with the two Lovasz ops on the emulation; and the reference module itself run live
against the fixture."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_lovasz_wide as T

CPU = torch.device("cpu")
REAL = ["lovasz_softmax", "lovasz_present"]


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.fixture()
def hybrid():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.hybrid(REAL):
        yield


def test_wide_shapes_fail_without_the_rows_path_entry_points():
    """the C ABI carries the three entry points of the path (a library from before it raises AttributeError in _lib.lib())"""
    from pointcept_amd import _lib

    for name in ("ptc_lovasz_present", "ptc_lovasz_softmax_rows_workspace_bytes", "ptc_lovasz_softmax_rows"):
        assert name in _lib.exported_symbols()


def test_golden_cases_on_the_emulation(emu):
    T.check_golden(CPU)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("c", [65, 100, 101, 200])
def test_shapes_on_the_emulation(emu, c, n):
    T.check_shape(CPU, n, c)


def test_1024_classes_on_the_emulation(emu):
    T.check_shape(CPU, 65, 1024)


def test_more_rows_than_step_workgroups_on_the_emulation(emu):
    """n = 5400, 200 classes, all present: 200 * ceil(5400 / 256) = 4400 > LV_STEP_BLOCKS"""
    x, y = T.labelled(5400, 200, 73, p_ignore=0.05)
    y[:200] = torch.arange(200)
    T.check_against_oracle(CPU, "emulation n=5400 c=200 P=200", x, y)


def test_label_patterns_on_the_emulation(emu):
    T.check_label_patterns(CPU)


def test_dtypes_and_layouts_on_the_emulation(emu):
    T.check_dtypes_and_layouts(CPU, n=131)


def test_nan_filled_workspace_on_the_emulation(emu):
    T.check_nan_workspace(CPU, n=131)


@pytest.mark.parametrize("n,c,n_absent", [(700, 20, 0), (700, 20, 7), (333, 64, 30)])
def test_rows_path_against_the_dense_path_on_the_emulation(emu, n, c, n_absent):
    T.check_rows_against_dense(CPU, n, c, n_absent)


def test_reproducible_on_the_emulation(emu):
    T.check_reproducible(CPU, 700, 200, 150)


def test_refusals_on_the_cpu_backend(hybrid):
    T.check_refusals(CPU)


def test_segmentor_on_the_cpu_backend(hybrid):
    T.check_segmentor(CPU, n=600)


def test_cpu_labels_ask_for_no_handle():
    """on the CPU backend alone (oracle stand-ins, three-argument lovasz_softmax) the segmentor asks for nothing"""
    import mock_backend
    from pointcept_amd import ops
    from pointcept_amd.segmentor import DefaultSegmentorV2

    class Feat(torch.nn.Module):
        def forward(self, point):
            return point["feat"]

    def never(*a, **k):
        raise AssertionError("a handle was asked for on CPU tensors")

    real, ops.lovasz_present = ops.lovasz_present, never
    try:
        with mock_backend.cpu_ops():
            seg = DefaultSegmentorV2(200, 64, Feat(), criteria=("ce", "lovasz")).train()
            g = torch.Generator().manual_seed(3)
            out = seg(dict(feat=torch.randn(100, 64, generator=g), segment=torch.randint(-1, 200, (100,), generator=g), offset=torch.tensor([100])))
            assert bool(torch.isfinite(out["loss"]))
    finally:
        ops.lovasz_present = real


@pytest.mark.needs_reference
@pytest.mark.skipif(not os.path.isdir("/root/reference/pointcept"), reason="needs the reference tree")
def test_needs_reference_module_gives_the_golden():
    """needs_reference: the reference's LovaszLoss, unmodified, run live on the regenerated cases gives the fixture's losses and gradients"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_lovasz_wide as M

    lov = M.load_reference_lovasz()
    for ci, x, y, loss_ref, grad_ref in T.golden_cases():
        loss, grad = M.run_reference(lov, x, y)
        assert loss == pytest.approx(loss_ref, rel=1e-6), ci
        assert np.abs(grad - grad_ref).max() <= 1e-6 * np.abs(grad_ref).max(), ci
