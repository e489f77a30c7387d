"""-m "not gpu": limits and shape rules have one definition, on the C side (include/ptcore.h LIMITS, csrc/ptcore_augment.h, the
*_supported / ptc_spconv_blk_min_rows entry points); pointcept_amd.ops reads or asks.  Each test keeps a FROZEN copy of the Python
formula that the lookup replaced -- the record of the behaviour before -- and compares the library's answer with it over a grid; the
entry points are host code, so they run on the host emulation build (tests/emu_backend.py).  The last tests call an op one past a
limit on a tiny input: the refusal must come from the library (a PtcoreError that carries its status code)."""
import itertools
import types

import pytest
import torch

CPU = torch.device("cpu")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


@pytest.fixture()
def emu(monkeypatch):
    import emu_backend
    from pointcept_amd import ops

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    monkeypatch.delenv("PTC_CONV8", raising=False)
    monkeypatch.setattr(ops, "_asked", {})           # answers are cached per argument tuple: start from none
    with emu_backend.emulated_ops():
        yield


# ---- the formulas as pointcept_amd/ops.py held them before the library was asked -----------------------------------------------
def frozen_block_plan(c_in, c_out, kv, dtype, n_rows):
    if dtype == torch.float32 or kv != 27:
        return None
    if c_in == c_out and c_in in (32, 64):
        return (128, 416) if n_rows >= 4096 else None
    if c_in % 32 == 0 and c_out % 32 == 0 and c_in <= 1024 and c_out <= 1024 and (c_in // (64 if c_in % 64 == 0 else 32)) * (c_out // 32) <= 256 \
            and n_rows >= 1024:
        return (128, 416)
    return None


def frozen_provider_get(c_in, c_out, kv, dtype, n_rows, conv, conv8_on=True):
    plan = frozen_block_plan(c_in, c_out, kv, dtype, n_rows)
    conv_kernel = (c_in == c_out and c_in in (32, 64)) or (conv8_on and c_in >= 96)
    return None if plan is None or (conv and not conv_kernel) else plan


def conv8_rule(c_in, c_out, kv, dtype, n_rows):
    """conv8_supported of csrc/conv8.h for tables of the standard geometry"""
    return dtype != torch.float32 and kv == 27 and c_in % 32 == 0 and 96 <= c_in <= 1024 and c_out % 32 == 0 and c_out <= 1024 and n_rows >= 256


def frozen_attn_rpe_supported(head_dim, max_seqlen, pos_bnd, dtype):
    lp = (int(max_seqlen) + 31) & ~31
    r = 2 * int(pos_bnd) + 1
    t4 = (3 * r + 3) & ~3
    if dtype == torch.float32:
        fits = max(lp * 136 + t4 * 12 + 32, lp * 144 + t4 * 4) <= 163840
    elif dtype in (torch.bfloat16, torch.float16):
        fits = lp * 72 + lp * 8 + t4 * 8 <= 163840
    else:
        return False
    return head_dim == 16 and 1 <= max_seqlen <= 1024 and pos_bnd >= 0 and fits


CHANNELS = (8, 16, 32, 36, 48, 64, 96, 112, 128, 192, 256, 512, 1024, 1056)
ROWS = (255, 256, 1023, 1024, 4095, 4096)
PLAN_GRID = list(itertools.product(CHANNELS, CHANNELS, DTYPES, (1, 27), ROWS))


def _provider_get(ops, c_in, c_out, kv, dtype, n_rows, conv):
    """BlockProvider.get over a table of [kv, n_rows] that says it is on the GPU; the tables themselves are not built (ops.BlockTables
    is replaced by the caller): what comes back is their (bm, hcap) or None"""
    provider = ops.BlockProvider(types.SimpleNamespace(is_cuda=True, shape=(kv, n_rows)))
    return provider.get(c_in, c_out, dtype, conv=conv)


def test_block_plan_is_the_frozen_rule(emu):
    from pointcept_amd import ops

    assert (ops.BLOCK_BM, ops.BLOCK_HCAP) == (128, 416)
    for c_in, c_out, dtype, kv, n_rows in PLAN_GRID:
        assert ops.block_plan(c_in, c_out, kv, dtype, n_rows) == frozen_block_plan(c_in, c_out, kv, dtype, n_rows), (c_in, c_out, dtype, kv, n_rows)
    assert ops.block_plan(64, 64, 27, torch.bfloat16) == (128, 416) and ops.block_plan(64, 64, 27, torch.float64) is None      # n_rows defaults to "many"


def test_block_provider_differs_from_the_frozen_rule_only_where_conv8_refuses(emu, monkeypatch):
    """conv=True used to say yes through `c_in >= 96` alone; conv8_supported also wants c_in % 32 == 0, c_in <= 1024, c_out % 32 == 0,
    c_out <= 1024 and n_rows >= 256.  The cases where the two answers differ must be exactly the frozen-yes cases that lean on
    `c_in >= 96` while conv8_supported says no.  (Both rules sit behind block_plan, whose sliced-wgrad7 rule already demands multiples
    of 32 up to 1024 and 1024 rows: see the count printed below.)"""
    from pointcept_amd import ops

    monkeypatch.setattr(ops, "BlockTables", lambda nbr, bm, hcap: (bm, hcap))
    differing, expected, agreeing_conv8 = set(), set(), 0
    for (c_in, c_out, dtype, kv, n_rows), conv in itertools.product(PLAN_GRID, (False, True)):
        case = (c_in, c_out, dtype, kv, n_rows, conv)
        frozen, got = frozen_provider_get(c_in, c_out, kv, dtype, n_rows, conv), _provider_get(ops, c_in, c_out, kv, dtype, n_rows, conv)
        through_96_alone = frozen is not None and conv and not (c_in == c_out and c_in in (32, 64))
        if through_96_alone and not conv8_rule(c_in, c_out, kv, dtype, n_rows):
            expected.add(case)
        if got != frozen:
            differing.add(case)
        elif through_96_alone:
            agreeing_conv8 += 1
    print(f"{len(PLAN_GRID) * 2} cases: {len(differing)} differ, {len(expected)} expected to, {agreeing_conv8} conv8 cases agree")
    assert differing == expected
    assert agreeing_conv8 > 0
    assert _provider_get(ops, 128, 128, 27, torch.bfloat16, 1024, True) == (128, 416)        # a conv8 shape
    assert _provider_get(ops, 64, 64, 27, torch.float16, 4096, True) == (128, 416)           # a conv7 shape
    assert _provider_get(ops, 64, 32, 27, torch.bfloat16, 4096, True) is None                # wgrad7 alone: the backward asks
    assert _provider_get(ops, 64, 32, 27, torch.bfloat16, 4096, False) == (128, 416)
    cpu_table = ops.BlockProvider(torch.zeros((27, 4096), dtype=torch.int32))
    assert cpu_table.get(64, 64, torch.bfloat16) is None                                     # not on the GPU: nothing is asked or built


def test_block_provider_follows_the_librarys_conv8_switch(emu, monkeypatch):
    """PTC_CONV8 is read by the library alone: with it off the wide shapes get no tables for a convolution, as the frozen rule said
    with config.CONV8 off"""
    from pointcept_amd import ops

    monkeypatch.setattr(ops, "BlockTables", lambda nbr, bm, hcap: (bm, hcap))
    monkeypatch.setenv("PTC_CONV8", "0")
    for c_in, c_out, n_rows, conv in itertools.product((64, 96, 128, 256), (64, 96, 128), (1024, 4096), (False, True)):
        assert _provider_get(ops, c_in, c_out, 27, torch.bfloat16, n_rows, conv) == \
            frozen_provider_get(c_in, c_out, 27, torch.bfloat16, n_rows, conv, conv8_on=False), (c_in, c_out, n_rows, conv)


def test_attn_rpe_supported_is_the_frozen_formula(emu):
    from pointcept_amd import ops

    differing = []
    for case in itertools.product((16, 18), (1, 31, 32, 33, 512, 1023, 1024, 1025), (0, 8, 32, 64, 1024, 4096, 4097), DTYPES + (torch.float64,)):
        if ops.attn_rpe_supported(*case) != frozen_attn_rpe_supported(*case):
            differing.append(case)
    assert differing == []
    assert ops.attn_rpe_supported(16, 1024, 32) and not ops.attn_rpe_supported(16, 1024, 4096)      # dtype defaults to bf16


def test_attn_hd_supported_answers_head_dim_16(emu):
    from pointcept_amd import ops

    assert ops.ATTN_HEAD_DIM == 16
    for max_seqlen in (0, 1, 1024, 1025):
        assert ops.attn_hd_supported(16, max_seqlen) == (1 <= max_seqlen <= 1024)
    assert not ops.attn_hd_supported(15, 128) and ops.attn_hd_supported(64, 512) and not ops.attn_hd_supported(65, 128)


def test_gather_rows_add_supported_is_the_frozen_rule(emu):
    from pointcept_amd import ops

    for dtype, c in itertools.product(DTYPES + (torch.float64,), (1, 2, 4, 6, 8, 12, 16, 20, 36, 64)):
        src = torch.zeros((2, c), dtype=dtype)
        frozen = dtype in DTYPES and c % (4 if dtype == torch.float32 else 8) == 0
        assert ops.gather_rows_add_supported(src, src) == frozen, (dtype, c)
    assert not ops.gather_rows_add_supported(torch.zeros(2, 8), torch.zeros(2, 16))


def test_limits_are_read_from_the_headers_without_the_library(monkeypatch):
    """every attribute of the issue's table: the header's value, and no library behind it (check_coord_range and spconv_api run on CPU)"""
    from pointcept_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("a limit was read through the library")

    monkeypatch.setattr(ops, "lib", no_library)
    monkeypatch.setattr(_lib, "lib", no_library)
    K, KA = _lib.HEADER.constants, _lib.AUGMENT_HEADER.constants
    assert (ops.VOX_MAX, ops.BATCH_MAX) == (1 << K["PTC_VOX_BITS"], K["PTC_VOX_BATCH_MAX"]) == (1 << 18, 1023)
    assert (ops.BLOCK_BM, ops.BLOCK_HCAP) == (K["PTC_BLOCK_BM"], K["PTC_BLOCK_HCAP"]) == (128, 416)
    assert (ops.CRITERIA_ROWS_MAX_C, ops.CRITERIA_CE_MAX_C) == (32, 1024) and (ops.CRITERIA_CE, ops.CRITERIA_FOCAL, ops.CRITERIA_DICE) == (1, 2, 4)
    assert (ops.LOVASZ_DENSE_MAX_C, ops.LOVASZ_MAX_C, ops.PG_MAX_NEIGHBOURS, ops.MSC_MAX_K) == (64, 1024, 1000, 8)
    assert (ops.AUG_MAX_OPS, ops.AUG_MAX_COLOR_OPS) == (KA["PTC_AUG_MAX_OPS"], KA["PTC_AUG_MAX_COLOR_OPS"]) == (16, 8)
    assert (ops.AUG_CENTER_SHIFT, ops.AUG_ROTATE, ops.AUG_SCALE, ops.AUG_FLIP, ops.AUG_SHIFT) == (0, 1, 2, 3, 4)
    assert (ops.AUG_C_AUTOCONTRAST, ops.AUG_C_TRANSLATION, ops.AUG_C_JITTER, ops.AUG_C_NORMALIZE) == (0, 1, 2, 3)
    assert ops.ACT_CODES == {"none": 0, "gelu": 1, "relu": 2}
    assert ops._CONCERTO_CORR_TYPES == {torch.float32: 0, torch.int32: 1, torch.int64: 2}
    assert (ops.EDGE_ROWS_GROUP, ops.EDGE_ROWS_SUB, ops.EDGE_ROWS_REL) == (0, 1, 2) == (ops.EDGE_REDUCE_INTERP, ops.EDGE_REDUCE_AGG, ops.EDGE_REDUCE_POS)
    assert (ops.EDGE_SCATTER_GROUP, ops.EDGE_SCATTER_SUB, ops.EDGE_SCATTER_INTERP, ops.EDGE_SCATTER_AGG) == (0, 1, 2, 3)
    ops.check_coord_range([ops.VOX_MAX - 1] * 3, ops.BATCH_MAX)
    with pytest.raises(ops.PtcoreError):
        ops.check_coord_range([ops.VOX_MAX, 0, 0], 1)
    with pytest.raises(ops.PtcoreError):
        ops.check_coord_range([0, 0, 0], ops.BATCH_MAX + 1)


# ---- one past a limit: the library refuses ----------------------------------------------------------------------------------------
def _refused_by_the_library(call):
    from pointcept_amd import ops

    with pytest.raises(ops.PtcoreError) as e:
        call()
    assert e.value.code is not None and e.value.code < 0, e.value        # a status of the entry point, not a check on the Python side


def test_msc_match_refuses_k_past_the_limit(emu):
    from pointcept_amd import ops

    xyz = torch.tensor([[0., 0., 0.], [0.01, 0., 0.], [0., 0.01, 0.], [0.5, 0.5, 0.5]])
    offset = torch.tensor([4], dtype=torch.int32)
    count, cand, stats = ops.msc_match(ops.MSC_MAX_K, 0.05, xyz, offset, xyz, offset)
    assert cand.shape == (4, 8) and count.tolist() == [3, 3, 3, 1]
    _refused_by_the_library(lambda: ops.msc_match(ops.MSC_MAX_K + 1, 0.05, xyz, offset, xyz, offset))


def test_aug_apply_refuses_colour_ops_past_the_limit(emu):
    from pointcept_amd import ops

    color = torch.full((4, 3), 255.0)
    normalize = (ops.AUG_C_NORMALIZE, 0.0, 0.0, 0.0, None, 0, ops.AUG_STREAM_COLOR)
    out = ops.aug_apply(color=color, color_ops=[normalize] * ops.AUG_MAX_COLOR_OPS)[2]
    assert torch.allclose(out, torch.full((4, 3), 255.0 / 255.0 ** 8))
    _refused_by_the_library(lambda: ops.aug_apply(color=color, color_ops=[normalize] * (ops.AUG_MAX_COLOR_OPS + 1)))


def test_criteria_refuse_focal_past_the_row_limit(emu):
    from pointcept_amd import ops

    spec = ops.CriteriaSpec(-1)
    spec.flags = ops.CRITERIA_FOCAL
    target = torch.tensor([0, 5, 31, 2])
    out = ops.criteria_rows_fwd(torch.zeros(4, ops.CRITERIA_ROWS_MAX_C), target, spec)[0]
    assert torch.isfinite(out).all()
    _refused_by_the_library(lambda: ops.criteria_rows_fwd(torch.zeros(4, ops.CRITERIA_ROWS_MAX_C + 1), target, spec))
    spec.flags = ops.CRITERIA_CE            # cross entropy alone goes on, up to its own limit
    assert torch.isfinite(ops.criteria_rows_fwd(torch.zeros(4, ops.CRITERIA_ROWS_MAX_C + 1), target, spec)[0]).all()
    _refused_by_the_library(lambda: ops.criteria_rows_fwd(torch.zeros(4, ops.CRITERIA_CE_MAX_C + 1), target, spec))


def test_attention_refuses_a_window_past_the_limit(emu):
    """no rows: the checks alone run"""
    from pointcept_amd import ops

    L = ops.lib()
    assert L.ptc_attn_varlen_fwd(None, None, 0, 0, 2, ops._K["PTC_ATTN_MAX_SEQLEN"], 0.25, ops._DT[torch.bfloat16], None, None, None) == 0
    _refused_by_the_library(lambda: L.ptc_attn_varlen_fwd(None, None, 0, 0, 2, ops._K["PTC_ATTN_MAX_SEQLEN"] + 1, 0.25, ops._DT[torch.bfloat16],
                                                          None, None, None))
    rpe = lambda pos_bnd, max_seqlen: L.ptc_attn_rpe_fwd(None, None, None, None, pos_bnd, 0, 0, 2, max_seqlen, 0.25, ops._DT[torch.bfloat16], None, None, None)  # noqa: E731
    assert rpe(8, 1024) == 0
    _refused_by_the_library(lambda: rpe(ops._K["PTC_ATTN_RPE_MAX_POS_BND"] + 1, 32))      # out of range
    _refused_by_the_library(lambda: rpe(ops._K["PTC_ATTN_RPE_MAX_POS_BND"], 32))          # in range, but the table does not fit LDS
