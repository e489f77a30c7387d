"""-m "not gpu": OA-CNNs' kernels (csrc/cluster_agg.hip) on the host emulation of the kernel sources (tests/host_emulation,
tests/emu_backend.py) -- the bodies of tests/test_gpu_oacnns.py with device = cpu at small shapes: grid-cluster maps against
voxel_grid + torch.unique, centering and aggregation forward / backward against float64, the epsilon-dominated scene, ties at the
global max, bit-reproducibility -- plus the integrity of tests/golden/oacnns_tiny.npz against the port's state dict."""
import numpy as np
import pytest
import torch

import test_gpu_oacnns as T

CPU = torch.device("cpu")
SMALL = [(300, 14, 0), (200, 12, 9), (90, 8, 3)]


@pytest.fixture(autouse=True)
def _emulator(request):
    if "golden" in request.node.name:
        yield
        return
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.fixture
def small():
    from pointcept_amd import ops

    ind = T.make_indices(SMALL, seed=2)
    gc = ops.grid_clusters(ind, [1, 3, 6, 9], T._shape(ind), len(SMALL))
    return gc, ind.shape[0], torch.nonzero(ind[:, 0] == 1)[:, 0]


def test_cluster_maps_on_the_emulation():
    T.check_cluster_maps(CPU, SMALL, [2, 6, 9, 24])
    T.check_cluster_maps(CPU, [(400, 16, 40), (100, 6, 0)], [1, 5, 64], seed=3)


@pytest.mark.parametrize("dtype,c", [(torch.float32, 64), (torch.bfloat16, 96), (torch.float16, 32)], ids=["f32_64", "bf16_96", "f16_32"])
def test_aggregation_against_float64_on_the_emulation(small, dtype, c):
    gc, n, rows = small
    T.check_agg_against_float64(CPU, dtype, gc, n, c, shift_rows=rows)


def test_aggregation_three_levels_on_the_emulation():
    from pointcept_amd import ops

    ind = T.make_indices([(500, 16, 0)], seed=4, big_cluster=700)
    gc = ops.grid_clusters(ind, [2, 6, 64], T._shape(ind), 1)
    assert int((gc.indptr[2][1:] - gc.indptr[2][:-1]).max()) >= 700      # more rows than one pass of the workgroup covers
    T.check_agg_against_float64(CPU, torch.float32, gc, ind.shape[0], 16)


def test_aggregation_reproducible_and_max_ties_on_the_emulation(small):
    gc, n, _ = small
    T.check_agg_reproducible(CPU, torch.float16, gc, n, 32)
    T.check_agg_max_ties(CPU, gc, n, 32)
    T.check_refuses_bad_shapes(CPU, gc, n)


def test_centering_against_float64_on_the_emulation(small):
    gc, n, _ = small
    T.check_center(CPU, torch.float32, gc, n, 48)
    T.check_center(CPU, torch.bfloat16, gc, n, 16)


def test_oacnns_golden_file_integrity():
    """the committed fixture against the port: state-dict keys, the regenerated weights (key list and per-tensor sums), the regenerated
    batch (checksums), one gradient norm per parameter, full gradients of the small parameters, finite logits"""
    from pointcept_amd.oacnns import OACNNs

    g = T.golden()
    net = OACNNs(**T.golden_cfg())
    assert list(net.state_dict().keys()) == list(g["keys"])
    net.load_state_dict(T.golden_state(g, net))
    b = T.golden_batch(g, CPU)
    n = int(b["offset"][-1])
    assert [k for k, _ in net.named_parameters()] == list(g["param_names"])
    assert g["grad_norms"].shape == (len(g["param_names"]),) and np.isfinite(g["grad_norms"]).all()
    for k, p in net.named_parameters():
        if p.numel() <= 512 or k.startswith("final."):
            assert g["grad/" + k].shape == tuple(p.shape), k
    assert g["logits_eval"].shape == ((n + 3) // 4, 13) and g["logits_train"].shape == ((n + 7) // 8, 13)
    assert np.isfinite(g["logits_eval"]).all() and np.isfinite(float(g["loss"]))
    assert all(len(net.enc[i].blocks[0].l_w) == len(T.golden_cfg()["point_grid_size"][i]) for i in range(3))
    assert all(len(d.blocks) == 0 for d in net.dec)
