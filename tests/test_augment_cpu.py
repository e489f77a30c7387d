"""-m "not gpu": the augmentation kernels (csrc/augment.hip) on the host emulation of the kernel sources -- the bodies of
tests/test_gpu_augment.py with device = cpu --, the torch twin against the golden, a dry run of the same bodies on the twin (the CPU
stand-in of the kernels), and, where the reference tree exists, the twin against the live reference classes with patched draws."""
import os

import numpy as np
import pytest
import torch

import test_gpu_augment as A

CPU = torch.device("cpu")
HAS_REFERENCE = os.path.isdir("/root/reference/pointcept")
keep_global_rng = A.keep_global_rng        # autouse here too: the global generators are left as they were found


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("name", list(A.CASES))
def test_case_on_the_emulation(emu, name):
    A.check_case(CPU, name, True)


def test_golden_cases_are_what_they_claim():
    A.check_rotated_box_is_told_apart()
    A.check_elastic_grid_shapes()


def test_closed_gates_leave_the_bits_on_the_emulation(emu):
    A.check_gate_false(CPU, True)


def test_empty_chain_coord_only_and_conversions_on_the_emulation(emu):
    A.check_empty_chain_and_coord_only(CPU, True)
    A.check_conversions(CPU, True)


def test_seeds_and_prefix_independence_on_the_emulation(emu):
    A.check_determinism(CPU, True)


def test_generator_statistics_on_the_emulation(emu):
    A.check_generator(CPU, True)


def test_refusals_on_the_emulation(emu):
    A.check_refusals(CPU, True)


def test_scannet_config_end_to_end_on_the_emulation(emu):
    A.check_scannet_config_end_to_end(CPU, True)


@pytest.mark.parametrize("name", list(A.CASES))
def test_twin_against_the_golden(name):
    """kernels=False: engine and twin are the same code, so the twin's own bound is what is checked"""
    A.check_case(CPU, name, False)


def test_gpu_test_bodies_dry_run_on_the_twin():
    """the remaining bodies of tests/test_gpu_augment.py on CPU tensors, which take the twin: their python, the fixtures and the planner's
    refusals are exercised without a kernel"""
    A.check_gate_false(CPU, False)
    A.check_empty_chain_and_coord_only(CPU, False)
    A.check_conversions(CPU, False)
    A.check_refusals(CPU, False)
    A.check_refusals(CPU, None)


def test_cpu_tensors_and_the_switch_take_the_twin():
    from pointcept_amd import config

    assert config.AUGMENT_KERNELS is True and "PTC_AUGMENT=0" in config.__doc__
    cfg, data, draws, _ = A.load_case("carried_box", CPU)
    a = A.AUG.Compose(cfg)(dict(data), draws)                    # CPU tensors outside the emulation: no kernel exists for them
    b = A.AUG.Compose(cfg, force_kernels=False)(dict(data), draws)
    assert all(torch.equal(a[k], b[k]) for k in A.POINT_KEYS)


def test_the_planner_fuses(emu):
    """launch accounting of the ScanNet chain on the kernels: one compose per run of affine transforms, a reduce before each transform
    that needs the box of a rotated or thinned cloud and none where the box is carried, one write of each output per flush"""
    cfg, data, draws, _ = A.load_case("carried_box", CPU)
    c = A.AUG.Compose(cfg, force_kernels=True)
    c(dict(data), draws)
    # reduce (2) + compose [CenterShift, Scale, Flip, Shift, Rotate(box carried)] (1) + reduce (2) + compose [CenterShift] (1) + apply (1)
    assert c.last_launches == 7, c.last_launches
    cfg, data, draws, _ = A.load_case("chain_scannet_two_tiles_plus_one", CPU)
    c = A.AUG.Compose(cfg, force_kernels=True)
    c(dict(data), draws)
    assert c.last_launches <= 24, c.last_launches


def test_shuffle_and_dropout_bookkeeping():
    sc = {k: torch.from_numpy(v) for k, v in A.scene("box", 50, 3).items()}
    perm = torch.randperm(50)
    out = A.AUG.ShufflePoint()(dict(sc), dict(index=perm))
    assert all(torch.equal(out[k], sc[k][perm]) for k in sc)
    sc["sampled_index"] = torch.tensor([3, 7, 49])
    keep = torch.tensor([1, 7, 20, 30])
    out = A.AUG.RandomDropout(dropout_application_ratio=1.0)(dict(sc), dict(gate=0.0, index=keep))
    assert out["coord"].shape[0] == 6 and torch.equal(out["segment"], sc["segment"][torch.tensor([1, 3, 7, 20, 30, 49])])
    assert out["sampled_index"].tolist() == [1, 2, 5]
    out = A.AUG.RandomDropout(dropout_ratio=0.2, dropout_application_ratio=1.0)(dict(coord=sc["coord"]), dict(gate=0.0))
    assert out["coord"].shape[0] == 40


@pytest.mark.needs_reference
@pytest.mark.skipif(not HAS_REFERENCE, reason="/root/reference not present")
def test_twin_against_the_live_reference_classes():
    """the reference's classes, draws patched to a fresh seed (not the golden's), against the twin fed the recorded draws"""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_augment as G

    ref = G.load_reference_transforms()
    for name in ("carried_box", "color_ops_then_normalize", "elastic_two_stages", "chain_scannet_two_tiles_plus_one"):
        kind, n, seed, cfg, forced, keys = A.CASES[name]
        sc = A.scene(kind, n, seed)
        gold, rows = G.run_reference(ref, cfg, sc, forced, seed + 1000)
        draws = [A.to_draw(c, [(fn, v) for fn, v in r], CPU) for c, r in zip(cfg, rows)]
        out = A.AUG.Compose(cfg, force_kernels=False)({k: torch.from_numpy(v) for k, v in sc.items()}, draws)
        for key in keys:
            scale = max(float(np.abs(gold[key]).max()), float(np.abs(sc[key]).max()))
            err = float(np.abs(out[key].numpy().astype(np.float64) - gold[key]).max())
            assert err <= 16 * 2.0 ** -24 * scale * len(cfg), (name, key, err)
