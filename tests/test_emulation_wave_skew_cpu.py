"""-m "not gpu": the host emulation's WAVE-SKEWED schedules (tests/host_emulation/hip/hip_runtime.h, PTC_EMU_SCHED = wave_asc | wave_desc).

Under the default schedule every wave of a workgroup advances from collective to collective together, so a workgroup barrier that is
missing between one wave's LDS read and another wave's later write of the same bytes cannot show.  Under the skewed schedules one wave
runs alone until all of it is parked at a workgroup barrier (lowest wave first, or highest first): the largest skew the barriers in
the source permit.  A kernel whose barriers are sufficient computes the same thing under all three; one that lacks a barrier does not
(csrc/mlp.hip's backward did: its weight-gradient loop re-read the dm / y images of a tile behind the tile's last barrier while a
wave that was ahead stored the next tile over them).

  1. the detector tested on itself: two tiny kernels (tests/host_emulation/sched_selftest.hip), with and without the barrier;
  2. existing emulated test bodies, unchanged, under both skewed schedules: for every kernel file with a workgroup barrier the
     cheapest case that reaches it, the persistent tile walkers with few enough workgroups that each walks three tiles or more, one
     case or more of every emulation-backed family file;
  3. for the persistent MLP / Linear / GEMM kernels, every output bit-identical across the three schedules."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

CPU = torch.device("cpu")
SCHEDS = ("wave_asc", "wave_desc")
# emulation-only workgroup caps: persistent kernels walk several tiles per workgroup at a few hundred rows
CAPS = {"PTC_EMU_CONV7_WGS": "3", "PTC_EMU_LINEAR2_WGS": "2", "PTC_EMU_GEMM3_WGS": "8", "PTC_EMU_CAC_TILE_WGS": "1",
        "PTC_MLP_BWD_WGS": "2", "PTC_MLP_FWD_WGS": "2"}
ROWS = 3 * 128 * 2 + 5         # two workgroups of 128-row tiles: four and three tiles (the last one ragged)


@pytest.fixture()
def emu(monkeypatch):
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    for k, v in CAPS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("PTC_EMU_SCHED", raising=False)
    with emu_backend.emulated_ops():
        yield emu_backend.build()


# ---- 1. the detector on itself ------------------------------------------------------------------------------------------------------
def _selftest(lib, with_barrier):
    out = np.full((2, 4, 64), -1, dtype=np.int32)
    lib.emu_sched_selftest.argtypes = [ctypes.c_int, ctypes.c_void_p]
    assert lib.emu_sched_selftest(int(with_barrier), out.ctypes.data) == 0
    return out


def _selftest_race_free():
    it, wave, lane = np.meshgrid(np.arange(2), np.arange(4), np.arange(64), indexing="ij")
    return (1000 * (it + 1) + 64 * ((wave + 1) % 4) + lane).astype(np.int32)      # what the neighbour wrote in the SAME iteration


def test_detector_with_the_barrier_all_schedules_agree(emu, monkeypatch):
    want = _selftest_race_free()
    for sched in (None, "lockstep") + SCHEDS:
        if sched is not None:
            monkeypatch.setenv("PTC_EMU_SCHED", sched)
        assert np.array_equal(_selftest(emu, True), want), sched


def test_detector_without_the_barrier_fires_under_the_skewed_schedules_only(emu, monkeypatch):
    """No barrier at the loop end.  lockstep: every wave has read before any wave writes again -- the race-free result, the race is
    invisible.  wave_asc: wave 0 runs ahead to the next barrier and has written its row of iteration 1 before wave 3 -- its only
    reader -- reads it in iteration 0; waves 0..2 read rows whose writers come later.  wave_desc: wave 3 reads wave 0's row in time, then
    every wave w < 3 finds the row of wave w + 1 already overwritten.  The last iteration's reads sit behind a barrier all waves reached
    with their last rows written: right in every schedule."""
    clean = _selftest_race_free()
    lane = np.arange(64)
    monkeypatch.setenv("PTC_EMU_SCHED", "lockstep")
    assert np.array_equal(_selftest(emu, False), clean)
    asc = clean.copy()
    asc[0, 3] = 2000 + 64 * 0 + lane
    monkeypatch.setenv("PTC_EMU_SCHED", "wave_asc")
    assert np.array_equal(_selftest(emu, False), asc)
    desc = clean.copy()
    for w in range(3):
        desc[0, w] = 2000 + 64 * (w + 1) + lane
    monkeypatch.setenv("PTC_EMU_SCHED", "wave_desc")
    assert np.array_equal(_selftest(emu, False), desc)
    assert not np.array_equal(asc, clean) and not np.array_equal(desc, clean) and not np.array_equal(asc, desc)


# ---- 2. existing bodies under the skewed schedules -------------------------------------------------------------------------------------
bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
# (module, function, positional arguments after the device, keyword arguments) -- beside each: the kernel file with a workgroup barrier it is
# the cheapest case of.  Bodies of tests/test_gpu_kernels.py as in tests/test_host_emulation_cpu.py, the family files' check_* functions as
# in their *_cpu.py files.
K = "test_gpu_kernels"
SKEWED = [
    # persistent tile walkers, three tiles or more per workgroup (CAPS)
    (K, "test_mlp_one_kernel_per_direction", (), dict(dtype=bf16, c=64, n=1100)),      # mlp.hip
    (K, "test_mlp_one_kernel_per_direction", (), dict(dtype=f16, c=32, n=1100)),
    (K, "test_linear_identity_table", (), dict(dtype=bf16, n=ROWS, cin=32, cout=96)),                         # fwd2.h linear2_kernel
    (K, "test_linear_identity_table", (), dict(dtype=bf16, n=ROWS, cin=64, cout=64)),
    (K, "test_linear_with_the_residual_joint_in_its_epilogue", (), dict(dtype=bf16, cin=64, cout=64)),        # fwd2_joint.h
    (K, "test_linear_identity_table", (), dict(dtype=bf16, n=520, cin=128, cout=384)),                        # gemm3.h kv = 1, wgrad3.h
    (K, "test_linear_gather_tables", (), dict(dtype=bf16, cin=128, cout=384)),                                # gemm3.h kv = 2 (gathered input gradient)
    (K, "test_spconv_fwd_block_staged", (), dict(c=32, ordered=False, n_rows=2100)),                          # conv7.h, conv5.h (follow-up launch)
    (K, "test_spconv_wgrad_block_staged", (), dict(c=32, ordered=True, n_rows=1600)),                         # wgrad7.h
    (K, "test_spconv_fwd_block_staged_wide", (), dict(c=(224, 96), ordered=False, n_rows=700)),               # conv8.h
    # one-tile / non-persistent kernels: the cheapest case per file
    (K, "test_spconv_fwd_and_wgrad", (), dict(dtype=bf16, cin=32, cout=32, ksize=3)),                         # spconv.hip, wgrad2_body.inc
    (K, "test_spconv_fwd_chunked_pipeline", (), dict(cin=128, cout=128, ksize=3, n_pts=700)),                 # conv3.h
    (K, "test_linear_identity_table", (), dict(dtype=f32, n=1000, cin=32, cout=64)),                          # spconv.hip fp32 kernels
    (K, "test_patch_pad_maps", (), dict(counts=[10, 3, 7], K=4)),                                             # maps.hip
    (K, "test_pool_maps", (), dict(n_pts=3000)),
    (K, "test_rulebook_blocks", (), dict(ordered=True)),                                                      # blocks.hip
    (K, "test_exclusive_scan", (), dict(n=16385)), (K, "test_sort_keys_stable", (), dict(n=4097)),            # scan_sort.hip
    (K, "test_coord_max", (), dict(n=5000, dtype=torch.int32)),
    (K, "test_layer_norm_fwd_bwd", (), dict(c=36, xdt=f32, ydt=bf16)),                                        # norm.hip
    (K, "test_add_norm_fused_joint", (), dict(c=48, mode="ln_add_ln")),
    (K, "test_batch_norm_act_train", (), dict(dtype=f32, n=900, c=6, act="gelu")),                            # bn.hip
    (K, "test_cross_entropy_fwd_bwd", (), dict(dtype=f32, n=300, c=40, strided=True)),                        # loss.hip
    (K, "test_lovasz_softmax_matches_reference_golden_and_oracle", (), dict()),                               # lovasz.hip
    (K, "test_seg_eval_hist_matches_the_reference_formula", (), dict(dtype=f32)),                             # evalhist.hip
    (K, "test_pointops_knn_query", (), dict(nsample=3)),                                                      # pointops.hip
    (K, "test_attention_fwd_bwd", (), dict(lens=[48, 48, 17], H=2)),                                          # attention.hip
    (K, "test_attention_f16_io_equals_the_reference_cast_passes", (), dict(lens=[1, 2, 31, 32, 33, 65], H=3, one_pass="1")),   # attention_bwd1.h
    (K, "test_attention_dropout_fwd_bwd", (), dict(lens=[200], H=2, p=0.5)),                                  # attention_drop.h
    (K, "test_attention_other_head_dims_fwd_bwd", (), dict(D=18, lens=[1, 2, 31, 32, 33, 65], H=6, dtype=bf16)),   # attention_hd.h
    (K, "test_attention_rpe_f16_io_equals_the_cast_passes", (), dict(lens=[33], H=1, bnd=4)),                 # attention_rpe.h
    # the emulation-backed family files
    ("test_gpu_attention_rpe_f32", "check_kernels_against_the_float64_reference", ([33], 1, 4), {}),          # attention_rpe_f32.h
    ("test_gpu_cac", "check_pool_soft", ((70, 1, 133, 45), 20, 48, 0.75, False), {}),                         # cac.hip
    ("test_gpu_cac", "check_pool_hard", (150, 2, 32), {}), ("test_gpu_cac", "check_cos", ((100,), 2, 32), {}),
    ("test_gpu_cac", "check_distill", (150, 2, 0.0), {}), ("test_gpu_cac", "check_reproducible", (700, 20, 32), {}),
    ("test_gpu_msc", "check_nce", (150, 32, 0.07), {}),                                                       # msc.hip
    ("test_gpu_msc_csc", "check_csc", ((1, 17, 64, 65), 96, 0.07, None), {}),
    ("test_gpu_sonata", "check_distill", (65, 192, 0.04, f32), {}),                                           # sonata.hip
    ("test_gpu_sonata", "check_scaling_vectors", (65, 192, 0.04, bf16, 1), {}),                                # (one workgroup: five tiles)
    ("test_gpu_sgiformer", "check_attention", ((48, 3), (33, 64), True, bf16), {}),                           # sgiformer.hip
    ("test_gpu_sgiformer", "check_match_cost", (7, 33), {}),
    ("test_gpu_oacnns", "_oacnns_small", (), {}),                                                             # cluster_agg.hip
    ("test_gpu_pointgroup", "check_threshold_and_mixed_labels", (), {}),                                      # pg_cluster.hip, cell_grid.hip
    ("test_gpu_pointgroup", "check_bias_loss", (100, f32), dict(all_ignored=True)),
    ("test_gpu_lovasz_wide", "check_shape", (65, 100), {}), ("test_gpu_lovasz_wide", "check_rows_against_dense", (333, 64, 30), {}),
]


def _oacnns_small(T):
    """tests/test_oacnns_cpu.py's `small` scenes: cluster maps, aggregation forward / backward against float64, centering"""
    from pointcept_amd import ops

    scenes = [(300, 14, 0), (200, 12, 9), (90, 8, 3)]
    ind = T.make_indices(scenes, seed=2)
    gc = ops.grid_clusters(ind, [1, 3, 6, 9], T._shape(ind), len(scenes))
    T.check_agg_against_float64(CPU, torch.float16, gc, ind.shape[0], 32, shift_rows=torch.nonzero(ind[:, 0] == 1)[:, 0])
    T.check_center(CPU, torch.float32, gc, ind.shape[0], 48)


def _ids():
    return [f"{m.replace('test_gpu_', '')}.{f.replace('test_', '')}-{i}" for i, (m, f, _, _) in enumerate(SKEWED)]


@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("mod,name,args,kw", SKEWED, ids=_ids())
def test_emulated_test_bodies_under_the_wave_skewed_schedules(emu, monkeypatch, mod, name, args, kw, sched):
    """the body's own assertions -- oracle, bit-identity with the split kernels, reproducibility -- with one wave of every workgroup
    running as far ahead of the others as the barriers in the kernel source allow"""
    T = importlib.import_module(mod)
    monkeypatch.setenv("PTC_EMU_SCHED", sched)
    if name == "_oacnns_small":
        return _oacnns_small(T)
    fn = getattr(T, name)
    if mod == "test_gpu_msc_csc":
        args = args[:3] + (sorted(T.RADII)[0],)
    if "monkeypatch" in inspect.signature(fn).parameters:
        kw = dict(kw, monkeypatch=monkeypatch)
    fn(CPU, *args, **kw)


# ---- 3. the persistent MLP / Linear / GEMM kernels: every output the same bits under the three schedules ----------------------------------
# (None of them has an output that may depend on the order of the waves: no LDS or global floating-point atomics, every output element
#  and every partial sum is owned by one lane; the weight-gradient partials of mlp_bwd are summed over workgroups in index order.)
def _rand(g, *shape, scale=1.0, dtype=bf16):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _run_mlp(c, dtype):
    from pointcept_amd import ops

    g = torch.Generator().manual_seed(c)
    n, hid = ROWS, 4 * c
    x, dm = _rand(g, n, c, dtype=dtype), _rand(g, n, c, scale=0.25, dtype=dtype)
    w1, w2 = _rand(g, hid, c, scale=c ** -0.5, dtype=dtype), _rand(g, c, hid, scale=hid ** -0.5, dtype=dtype)
    b1, b2, a = torch.randn(hid, generator=g) * 0.5, torch.randn(c, generator=g), torch.randn(n, c, generator=g)
    rs = (torch.rand(n, generator=g) > 0.3).float() / 0.7
    out = [ops.mlp_fwd(x, w1, b1, w2, b2)] + list(ops.mlp_fwd(x, w1, b1, w2, b2, a, rs)) + list(ops.mlp_bwd(dm, x, w1, b1, w2.t().contiguous()))
    ref = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(x.double(), w1.double(), b1.double())), w2.double(), b2.double())
    return out, (out[0], ref)


def _run_linear2(cin, cout, dtype=bf16):
    from pointcept_amd import ops

    g = torch.Generator().manual_seed(cin + cout)
    n = ROWS
    x, w, b = _rand(g, n + 40, cin, dtype=dtype), _rand(g, cout, cin, scale=cin ** -0.5, dtype=dtype), torch.randn(cout, generator=g)
    tab = torch.randint(0, n + 40, (1, n), generator=g).int()
    tab[0, ::7] = -1                                                     # absent rows: the bias alone
    out = [ops.spconv_fwd(x[:n].contiguous(), w[:, None, :].contiguous(), b, None), ops.spconv_fwd(x, w[:, None, :].contiguous(), b, tab)]
    return out, (out[0], torch.nn.functional.linear(x[:n].double(), w.double(), b.double()))


def _run_joint(c, dtype=bf16):
    from pointcept_amd import ops

    g = torch.Generator().manual_seed(c)
    n = ROWS
    x, w, b = _rand(g, n + 40, c, dtype=dtype), _rand(g, c, c, scale=c ** -0.5, dtype=dtype), torch.randn(c, generator=g)
    a, rs = torch.randn(n, c, generator=g), (torch.rand(n, generator=g) > 0.3).float() / 0.7
    tab = torch.randint(0, n + 40, (n,), generator=g).int()
    gam, bet = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    z, y, st = ops.linear_joint_fwd(x, w, b, tab, a, rs, (gam, bet, 1e-5), dtype)
    out = [z, y, st] + list(ops.linear_norm_joint_fwd(x[:n].contiguous(), w, b, (gam, bet, 1e-6), a, (gam, bet, 1e-5), dtype))
    ref = a.double() + rs.double()[:, None] * torch.nn.functional.linear(x.double()[tab.long()], w.double(), b.double())
    return out, (z, ref)


def _run_gemm3(kv, dtype=bf16):
    from pointcept_amd import ops

    cin, cout, n, n_in = 128, 384, 520, 560            # 64-row tiles: 9 x 3 of them on 8 workgroups -- three or four each
    g = torch.Generator().manual_seed(kv)
    x, w, b = _rand(g, n_in, cin, dtype=dtype), _rand(g, cout, kv, cin, scale=(kv * cin) ** -0.5, dtype=dtype), torch.randn(cout, generator=g)
    tab = torch.randint(0, n_in, (kv, n), generator=g).int()
    tab[kv - 1, ::5] = -1
    out = [ops.spconv_fwd(x, w, b, tab)]
    xg = torch.where((tab >= 0)[:, :, None], x.double()[tab.clamp(min=0).long()], torch.zeros((), dtype=torch.float64))      # [kv, n, cin]
    ref = torch.einsum("knc,okc->no", xg, w.double()) + b.double()
    return out, (out[0], ref)


@pytest.mark.parametrize("what,args", [("mlp", (64, bf16)), ("mlp", (32, f16)), ("linear2", (32, 96)), ("linear2", (64, 64)), ("joint", (64,)),
                                       ("gemm3", (1,)), ("gemm3", (2,))], ids=lambda v: v if isinstance(v, str) else "-".join(str(a).replace("torch.", "") for a in v))
def test_persistent_kernels_give_the_same_bits_under_every_schedule(emu, monkeypatch, what, args):
    run = {"mlp": _run_mlp, "linear2": _run_linear2, "joint": _run_joint, "gemm3": _run_gemm3}[what]
    monkeypatch.setenv("PTC_EMU_SCHED", "lockstep")
    base, (got, ref) = run(*args)
    # 2^-7: one rounding of a 16-bit output (2^-9 bf16, 2^-11 f16, relative to the entry) plus those of the hidden tensor, as an L2 ratio
    assert float((got.double() - ref).norm() / ref.norm()) < 2.0 ** -7
    for sched in SCHEDS:
        monkeypatch.setenv("PTC_EMU_SCHED", sched)
        other, _ = run(*args)
        for i, (u, v) in enumerate(zip(base, other)):
            assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), (what, args, sched, i)
