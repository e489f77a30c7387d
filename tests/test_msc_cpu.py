"""-m "not gpu": Masked Scene Contrast's kernels (csrc/msc.hip) on the host emulation of the kernel sources (tests/host_emulation,
tests/emu_backend.py) -- the bodies of tests/test_gpu_msc.py with device = cpu at small shapes: matching against ops.knn_query + the
radius filter AND against oracle/pointops.py, pair selection, cross masks against the reference expression, InfoNCE against float64
(the tolerance rule of test_gpu_msc.py), bit-reproducibility -- plus the port's torch path (PTC_MSC=0) on the CPU backend."""
import os

import numpy as np
import pytest
import torch

import test_gpu_msc as T

CPU = torch.device("cpu")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    import mock_backend
    from pointcept_amd import ops

    with emu_backend.emulated_ops():
        saved = ops.knn_query
        ops.knn_query = mock_backend.knn_query          # pointops.hip's LDS tiles are emulated too, but the oracle is the point here
        try:
            yield
        finally:
            ops.knn_query = saved


def _oracle_knn(k, xyz, off, new_xyz, new_off):
    from oracle import pointops as opo

    return opo.knn_query(k, xyz, off, new_xyz, new_off)


@pytest.mark.parametrize("name", sorted(T.designed_cases()))
def test_match_designed_on_the_emulation(emu, name):
    case = T.designed_cases()[name]
    count, cand, _ = T.check_match(CPU, *case, oracle=_oracle_knn if case[2].shape[0] else None)
    T.check_select(CPU, count, cand)
    if name == "k_kplus1_dup_boundary":
        assert count.tolist() == [T.K, T.K, 4]


def test_match_against_the_emulated_brute_force_kernel():
    """ptc_knn_query itself (not the oracle) on the emulation, two scenes"""
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        b = T.two_views([1500, 1200], 41, CPU)
        count, cand, _ = T.check_match(CPU, b["view2_origin_coord"], b["view2_offset"], b["view1_origin_coord"], b["view1_offset"], 0.03)
        hist = torch.bincount(count.long(), minlength=T.K + 1)
        assert int(hist[0]) > 0 and int(hist[T.K]) > 0
        T.check_select(CPU, count, cand, seed=2)


def test_cross_masks_on_the_emulation(emu):
    b = T.two_views([2500, 2000], 51, CPU)
    for rate in (0.4, 0.5):
        m1, m2, patch_num, _ = T.check_cross_masks(CPU, b["view1_origin_coord"], b["view1_offset"], b["view2_origin_coord"], b["view2_offset"], 0.1, rate)
        assert bool((b["view1_origin_coord"] < 0).any()) and patch_num > 20 and bool(m1.any()) and bool(m2.any())


def test_cross_masks_one_large_patch_on_the_emulation(emu):
    g = torch.Generator().manual_seed(1)
    o1 = torch.cat([torch.rand(700, 3, generator=g) * 0.09 + 0.2, torch.rand(300, 3, generator=g) * 4 - 2])
    o2 = torch.rand(800, 3, generator=g) * 4 - 2
    _, _, _, counts = T.check_cross_masks(CPU, o1, torch.tensor([1000]), o2, torch.tensor([800]), 0.1, 0.5)
    assert int(counts.max()) > 500


@pytest.mark.parametrize("p,c,t", [(1, 32, 0.4), (17, 96, 0.07), (150, 32, 0.07), (200, 96, 0.4), (70, 132, 0.4)])
def test_nce_on_the_emulation(emu, p, c, t):
    T.check_nce(CPU, p, c, t)


def test_nce_reproducible_on_the_emulation(emu):
    T.check_nce_reproducible(CPU, 130, 96, 0.4)


def test_nce_refuses_what_it_does_not_implement(emu):
    from pointcept_amd import functional as PF
    from pointcept_amd._lib import PtcoreError

    f = torch.randn(10, 30)
    with pytest.raises(PtcoreError):
        PF.msc_nce(f, f, torch.zeros((2, 2), dtype=torch.int64), 0.4)
    with pytest.raises(PtcoreError):
        PF.msc_nce(torch.randn(10, 32), torch.randn(10, 32), torch.zeros((0, 2), dtype=torch.int64), 0.4)


def test_two_view_builder():
    from pointcept_amd import synthetic

    b = synthetic.contrastive_views_batch([7, 8], [3000, 2000])
    for v in ("view1", "view2"):
        n = int(b[f"{v}_offset"][-1])
        assert len(b[f"{v}_offset"]) == 2
        for k, w in (("origin_coord", 3), ("coord", 3), ("grid_coord", 3), ("color", 3), ("normal", 3), ("feat", 6)):
            assert b[f"{v}_{k}"].shape == (n, w), k
        assert b[f"{v}_grid_coord"].dtype == np.int64 and (b[f"{v}_grid_coord"] >= 0).all()
        assert (b[f"{v}_origin_coord"] < 0).any()
        lo = 0
        for hi in b[f"{v}_offset"]:          # one point per voxel inside a scene
            assert len(np.unique(b[f"{v}_grid_coord"][lo:hi], axis=0)) == hi - lo
            lo = hi


def test_registration_and_state_dict_keys():
    """the port's state-dict keys are the reference file's (stored in the golden), in its order"""
    T.test_registered_only_when_named()
    import mock_backend

    with mock_backend.cpu_ops():
        T.test_state_dict_keys_are_the_references()


def test_port_matches_reference_golden_on_the_host(monkeypatch):
    """PTC_MSC=0 on the CPU backend: the reference run's draws replayed give its masks and match_index exactly, its losses and
    gradients at the SpUNet golden tolerances"""
    import mock_backend
    from pointcept_amd import config

    monkeypatch.setattr(config, "MSC_KERNELS", False)
    with mock_backend.cpu_ops():
        T.check_port_against_golden(CPU)


def test_golden_kernels_on_the_emulation(emu):
    """the fixture's integers from csrc/msc.hip itself (host emulation): masks from the recorded patch permutation, match_index from
    the recorded randint and randperm"""
    from pointcept_amd import ops, synthetic

    g = T.golden()
    b = synthetic.to_torch(T.golden_batch(g), CPU)
    m1, m2 = ops.msc_cross_masks(b["view1_origin_coord"], b["view1_offset"], b["view2_origin_coord"], b["view2_offset"], 0.1, 0.4,
                                 rand_perm=lambda n: torch.from_numpy(g["draw_patch_perm"]))
    assert np.array_equal(m1.numpy(), g["view1_point_mask"]) and np.array_equal(m2.numpy(), g["view2_point_mask"])
    count, cand, stats = ops.msc_match(8, 0.03, b["view2_origin_coord"], b["view2_offset"], b["view1_origin_coord"], b["view1_offset"])
    assert np.array_equal(torch.bincount(count.long(), minlength=9).numpy(), g["match_count_hist"])
    assert stats.tolist() == [len(g["draw_select_r"]), 8]
    index = ops.msc_select(count, cand, torch.from_numpy(g["draw_select_r"]))
    assert np.array_equal(index[torch.from_numpy(g["draw_pair_perm"])[:256]].numpy(), g["match_index"])


def _reference_msc():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_msc as M

    return M


def _compare_with_fixture(g, ref, out, masks, match, log, tol):
    assert np.array_equal(masks[0].numpy(), g["view1_point_mask"]) and np.array_equal(masks[1].numpy(), g["view2_point_mask"])
    assert np.array_equal(match.numpy(), g["match_index"])
    assert np.array_equal(log[0][1].numpy(), g["draw_patch_perm"]) and np.array_equal(log[3][1].numpy(), g["draw_select_r"])
    for k in T.GOLD_LOSSES:
        assert float(out[k].detach()) == pytest.approx(float(g["out/" + k]), rel=tol, abs=tol if k in T.COSINE_MEANS else 0), k
    for k, p in ref.named_parameters():
        if "grad/" + k in g.files:
            assert T._rel(p.grad, g["grad/" + k]) <= 10 * tol, k


@pytest.mark.skipif(not os.path.isdir("/root/reference/pointcept"), reason="needs the reference tree")
def test_needs_reference_golden_regenerates():
    """needs_reference: the committed fixture is what the reference file computes now, with equal seeds, on the stand-ins"""
    M = _reference_msc()
    g = T.golden()
    R = M.load_reference_msc()
    inp = {k: torch.from_numpy(v) for k, v in T.golden_batch(g).items()}
    kept = {}
    ref, out = M.run_reference(R, lambda m: T.golden_state(g, m), inp, lambda masks, match, log: kept.update(masks=masks, match=match, log=log))
    _compare_with_fixture(g, ref, out, kept["masks"], kept["match"], kept["log"], 1e-6)


@pytest.mark.skipif(not os.path.isdir("/root/reference/pointcept"), reason="needs the reference tree")
def test_needs_reference_file_on_the_mirrors_matches_the_golden(monkeypatch):
    """needs_reference: the reference's MSC file itself, unmodified, with the two library names it imports bound to what
    compat.install(geometric=True) installs -- `voxel_grid` of torch_geometric_api and `pointops` = pointops_api, whose knn_query
    runs ptc_knn_query on the host emulation -- and equal seeds agrees with the fixture: the mirrors serve the unmodified file"""
    import sys

    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    from pointcept_amd import compat

    M = _reference_msc()
    g = T.golden()
    R = M.load_reference_msc()
    mods = {}
    saved = {k: sys.modules.get(k) for k in ("pointops", "torch_geometric", "torch_geometric.nn", "torch_geometric.nn.pool", "torch_geometric.utils")}
    try:
        for k in saved:
            sys.modules.pop(k, None)
        compat.install(geometric=True)
        mods = {k: sys.modules[k] for k in saved}
    finally:
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v
    monkeypatch.setattr(R, "pointops", mods["pointops"])
    monkeypatch.setattr(R, "voxel_grid", mods["torch_geometric.nn.pool"].voxel_grid)
    inp = {k: torch.from_numpy(v) for k, v in T.golden_batch(g).items()}
    kept = {}
    with emu_backend.emulated_ops():
        ref, out = M.run_reference(R, lambda m: T.golden_state(g, m), inp, lambda masks, match, log: kept.update(masks=masks, match=match, log=log))
    _compare_with_fixture(g, ref, out, kept["masks"], kept["match"], kept["log"], 1e-6)


def test_torch_path_of_the_port_on_the_host(monkeypatch):
    """PTC_MSC=0 is the CPU path: a train step on the CPU backend, its draws recorded and replayed to the same integers and losses"""
    import mock_backend
    from pointcept_amd import config
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrast

    monkeypatch.setattr(config, "MSC_KERNELS", False)
    with mock_backend.cpu_ops():
        torch.manual_seed(0)
        model = MaskedSceneContrast(**T.TINY_CFG)
        batch = T.two_views([900, 700], 61, CPU)
        rec = T.Recorder()
        out, grads = T._model_run(model, batch, rec)
        ints = dict(model.last)
        out2, _ = T._model_run(model, batch, T.Recorder(rec.log))
    assert [k for k, _ in rec.log] == ["patch_perm", "mix", "mix", "select", "pair_perm"]
    assert ints["match_index"].shape == (T.TINY_CFG["matching_max_pair"], 2)
    for k in ("view1_point_mask", "view2_point_mask", "match_index"):
        assert torch.equal(ints[k], model.last[k])
    assert set(out) == {"nce_loss", "pos_sim", "neg_sim", "color_loss", "normal_loss", "loss"}
    for k in out:
        assert bool(torch.isfinite(out[k])) and float(out[k]) == float(out2[k]), k
    assert set(grads) == set(n for n, _ in model.named_parameters())
