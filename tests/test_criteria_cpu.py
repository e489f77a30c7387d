"""-m "not gpu": the criteria kernels (csrc/criteria.hip) on the host emulation of the kernel sources -- the bodies of
tests/test_gpu_criteria.py with device = cpu at their small shapes -- plus the torch twins on CPU tensors, the refusals by name, the
golden on the torch path and, where the reference tree exists, the twins against the reference's own modules."""
import os

import pytest
import torch

import test_gpu_criteria as C

CPU = torch.device("cpu")
HAS_REFERENCE = os.path.isdir("/root/reference/pointcept")


@pytest.fixture()
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        yield


@pytest.mark.parametrize("n,c,dtype,eps,reduction,strided", [
    (1, 2, torch.float32, 0.0, "mean", False), (255, 19, torch.float32, 0.1, "sum", False), (257, 20, torch.bfloat16, 0.1, "mean", True),
    (513, 32, torch.float16, 0.0, "sum", True), (257, 33, torch.float32, 0.1, "mean", False), (257, 200, torch.bfloat16, 0.0, "sum", True)])
def test_cross_entropy_on_the_emulation(emu, n, c, dtype, eps, reduction, strided):
    C.check_ce(CPU, n, c, dtype, eps, reduction, strided)


def test_cross_entropy_zero_denominators_on_the_emulation(emu):
    C.check_ce_nan(CPU)


@pytest.mark.parametrize("n,c,dtype,gamma,listed,strided", [
    (1, 2, torch.float32, 2.0, False, False), (255, 19, torch.float32, 2.0, True, False), (257, 20, torch.bfloat16, 0.0, False, True),
    (513, 32, torch.float16, 2.0, True, True)])
def test_focal_on_the_emulation(emu, n, c, dtype, gamma, listed, strided):
    C.check_focal(CPU, n, c, dtype, gamma, listed, strided)


def test_focal_edges_on_the_emulation(emu):
    C.check_focal_saturated(CPU)
    C.check_focal_none_counted(CPU)


@pytest.mark.parametrize("n,c,dtype,exponent,ignore_index,strided", [
    (1, 2, torch.float32, 2, -1, False), (255, 19, torch.float32, 1, -1, False), (257, 19, torch.float32, 3, 2, False),
    (257, 20, torch.bfloat16, 2, -1, True), (513, 32, torch.float16, 3, 5, True)])
def test_dice_on_the_emulation(emu, n, c, dtype, exponent, ignore_index, strided):
    C.check_dice(CPU, n, c, dtype, exponent, ignore_index, strided)


def test_dice_no_valid_row_on_the_emulation(emu):
    C.check_dice_no_valid_row(CPU)


@pytest.mark.parametrize("n,c,dtype,strided", [(1, 2, torch.float32, False), (257, 19, torch.float32, False), (513, 32, torch.float32, True),
                                               (255, 20, torch.bfloat16, True)])
def test_fused_on_the_emulation(emu, n, c, dtype, strided):
    C.check_fused(CPU, n, c, dtype, strided)


def test_duplicates_determinism_and_default_bits_on_the_emulation(emu):
    C.check_duplicate_terms(CPU)
    C.check_determinism(CPU)
    C.check_default_cross_entropy_bits(CPU)


def test_wide_fallbacks_on_the_emulation(emu):
    C.check_wide_fallbacks(CPU, 33)


def test_kitti_criteria_on_the_emulation(emu):
    C.check_criteria_kitti(CPU)


def test_golden_on_the_emulation(emu):
    C.check_golden(CPU, True)


def test_golden_on_the_torch_path():
    C.check_golden(CPU, None)
    C.check_golden(CPU, False)


def test_config_flag_and_cpu_tensors_take_the_twins():
    from pointcept_amd import config
    from pointcept_amd import functional as PF

    assert config.CRITERIA_KERNELS is True and "PTC_CRITERIA=0" in config.__doc__
    x, t = C.case(CPU, 257, 19)
    terms = C.FUSED(19)
    a = C._run(PF.seg_criteria, x, t, terms)                  # CPU tensors outside the emulation: no kernel exists for them
    b = C._run(PF.seg_criteria_torch, x, t, terms)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = C._run(PF.cross_entropy, x, t, -1, C.class_weight(19), 0.1, "sum")
    b = C._run(PF.cross_entropy_torch, x, t, -1, C.class_weight(19), 0.1, "sum")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(PF.focal_loss(x, t, 2.0, 0.25), PF.focal_loss_torch(x, t, 2.0, 0.25))
    assert torch.equal(PF.dice_loss(x, t, 1, 2), PF.dice_loss_torch(x, t, 1, 2))
    crit = C.Criteria(C.KITTI_CRITERIA[:1] + [dict(type="DiceLoss", loss_weight=0.5, ignore_index=-1)])
    assert torch.equal(crit(x, t), PF.seg_criteria_torch(x, t, [C.KITTI_CRITERIA[0], dict(type="DiceLoss", loss_weight=0.5)], -1))


def test_segmentor_takes_the_reference_config_dicts_on_the_stand_ins():
    import mock_backend

    with mock_backend.cpu_ops():
        C.check_segmentor_with_config_dicts(CPU)


@pytest.mark.parametrize("cfg,match", [
    (dict(type="SmoothCELoss"), "SmoothCELoss.*AttributeError"),
    (dict(type="FocalLoss", reduction="sum"), "FocalLoss.*sum.*AttributeError"),
    (dict(type="BinaryFocalLoss"), r"BinaryFocalLoss.*\[N\] predictions"),
    (dict(type="CrossEntropyLoss", reduction="none"), "CrossEntropyLoss.*none"),
    (dict(type="FocalLoss", reduction="none"), "FocalLoss.*none"),
    (dict(type="CrossEntropyLoss", reduce=False), "size_average / reduce"),
    (dict(type="DiceLoss", reduction="mean"), "DiceLoss has no setting"),
    (dict(type="FocalLoss", gamma=2), "float gamma"),
    (dict(type="LovaszLoss", mode="binary"), "LovaszLoss with"),
    (dict(type="MSELoss"), "MSELoss is not on the engine's loss kernels")])
def test_refusals_by_name(cfg, match):
    from pointcept_amd.segmentor import DefaultSegmentorV2

    with pytest.raises(ValueError, match=match):
        C.Criteria([cfg], "owner")
    with pytest.raises(ValueError, match=match):
        DefaultSegmentorV2(19, 16, C._Head(), criteria=[cfg])


def test_seg_criteria_refuses_what_criteria_refuses():
    from pointcept_amd import functional as PF

    x, t = C.case(CPU, 9, 5)
    for term in (dict(type="SmoothCELoss"), dict(type="BinaryFocalLoss"), dict(type="FocalLoss", reduction="sum"),
                 dict(type="CrossEntropyLoss", reduction="none"), dict(type="LovaszLoss")):
        with pytest.raises(ValueError, match=term["type"]):
            PF.seg_criteria(x, t, [term])
    with pytest.raises(ValueError, match="one ignore_index"):
        PF.seg_criteria(x, t, [dict(type="DiceLoss", ignore_index=-1), dict(type="FocalLoss", ignore_index=255)])
    with pytest.raises(TypeError):
        PF.cross_entropy(x, t, -1, None, 0.0, "mean", None)


def test_the_ports_with_a_pinned_criteria_set_keep_it():
    """CAC-v1m1 and PPT construct Criteria(row_terms=False): default CrossEntropyLoss and LovaszLoss, everything else refused as before"""
    with pytest.raises(ValueError, match="FocalLoss is not on the engine's loss kernels"):
        C.Criteria([dict(type="FocalLoss")], "PPT-v1m1", row_terms=False)
    with pytest.raises(ValueError, match="CrossEntropyLoss with .*weight"):
        C.Criteria([dict(type="CrossEntropyLoss", weight=[1.0] * 19)], "CAC-v1m1", row_terms=False)
    crit = C.Criteria([dict(type="CrossEntropyLoss", loss_weight=2.0, ignore_index=-1), dict(type="LovaszLoss", mode="multiclass")], row_terms=False)
    assert [e[0].__name__ for e in crit.terms] == ["cross_entropy", "lovasz_softmax"] and crit.terms[0][1:] == (2.0, -1)


def test_groups_by_ignore_index_and_list_order():
    crit = C.Criteria([dict(type="CrossEntropyLoss", ignore_index=-1), dict(type="LovaszLoss", ignore_index=-1),
                       dict(type="DiceLoss", ignore_index=-1), dict(type="FocalLoss", ignore_index=255), dict(type="CrossEntropyLoss", ignore_index=255)])
    kinds = [(e[0] if isinstance(e[0], str) else e[0].__name__, e[2]) for e in crit.terms]
    assert kinds == [("fused", -1), ("lovasz_softmax", -1), ("fused", 255)]
    assert [t["type"] for t in crit.terms[0][1]] == ["CrossEntropyLoss", "DiceLoss"]
    assert [t["type"] for t in crit.terms[2][1]] == ["FocalLoss", "CrossEntropyLoss"]


@pytest.mark.needs_reference
@pytest.mark.skipif(not HAS_REFERENCE, reason="/root/reference not present")
def test_twins_against_the_references_own_modules():
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_criteria as G
    from pointcept_amd import functional as PF

    misc = G.load_reference_misc()
    for ci in range(len(C.GOLDEN_CASES)):
        x, t, ignore, term = C.golden_case(ci)
        loss, grad = G.run_reference(G.build_reference(misc, term, ignore), x, t)        # the same expressions: the same bits
        got = C._run(PF.seg_criteria_torch, x, t, [term], ignore)
        assert float(got[0]) == loss and torch.equal(got[1], torch.from_numpy(grad)), ci
    assert misc.FocalLoss()(torch.zeros(3, 4), torch.full((3,), -1)) == 0.0                   # the float the engine returns as a tensor
    for bad in (lambda: misc.SmoothCELoss()(torch.zeros(3, 4), torch.zeros(3, dtype=torch.long)),
                lambda: misc.FocalLoss(reduction="sum")(torch.zeros(3, 4), torch.zeros(3, dtype=torch.long))):
        with pytest.raises(AttributeError, match="total"):
            bad()
