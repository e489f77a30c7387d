"""-m "not gpu": the kernel SOURCES of pointcept_amd/csrc compiled for the host and executed on the CPU (tests/host_emulation/hip/
hip_runtime.h: every lane of a workgroup is a fiber; __syncthreads, shuffles, ballots, the MFMA instructions, ds_read_b64_tr_b16 and
raw buffer loads are modelled as collectives over the 64-lane wave; tests/emu_backend.py builds the library and binds
pointcept_amd.ops to it).  The bodies of -m gpu kernel tests then run with device = cpu against the same oracles.

What this tier is: a check of everything that is a function of PROGRAM ORDER in the product's HIP code -- index arithmetic, LDS
staging, cross-lane exchanges, MFMA tilings and fragment layouts, dtype dispatch, argument validation -- without a GPU.  The
emulator's matrix / transpose-read / buffer-load models are themselves validated by the fact that kernels which pass on the MI355X
(GPU tier, round 2) reproduce their oracles here: implicit GEMM convolution forward / input gradient / weight gradient
(16x16x32 MFMA, ds_read_b64_tr_b16, raw buffer loads), window attention forward / backward for head_dim 16 and 18 and with RPE
(32x32x16 MFMA), norms, maps, rulebooks, reductions.
What it is not: timing, memory ordering between waves, the summation order inside an MFMA -- and code that relies on the LOCKSTEP
execution of a wave between two collectives without saying so.  (The radix sort's rank / publish step did: every lane reads a
running LDS counter and the lowest lane of each digit group then publishes the new value.  It now states the lockstep with two
`__builtin_amdgcn_wave_barrier()` -- no instruction, the gfx950 binary is byte-identical (tools/kernel_fingerprint.py) -- which the
emulator honours as a wave-level wait; the sort and everything built on it runs here since.)
ptc_rope3d_xyz (written after round 2's GPU time was spent) has only ever run here."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
F32, F16, BF16 = 0, 1, 2          # ptc_dtype tags of include/ptcore.h


@pytest.fixture(scope="module")
def emu():
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    from pointcept_amd import _lib

    L = _lib.bind(emu_backend.build(), checked=False, partial=True)     # the header's signatures; status integers returned
    L.emu_last_error = L.ptc_last_error
    return L


def _tag(t):
    return {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}[t.dtype]


def test_header_constants_match(emu):
    import re

    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ptcore.h")).read()
    for name, val in (("PTC_F32", F32), ("PTC_F16", F16), ("PTC_BF16", BF16)):
        m = re.search(name + r"\s*=\s*(\d+)", hdr)
        assert m and int(m.group(1)) == val, name


def test_rope3d_on_the_host_emulation_matches_the_reference_cpu_golden(emu):
    """harness check: the GPU-validated ptc_rope3d, run thread by thread on the CPU, reproduces tests/golden/pointrope.npz
    (= libs/pointrope's own pointrope_cpu)"""
    g = np.load(os.path.join(GOLD, "pointrope.npz"))
    for ci in range(int(g["n_cases"])):
        B, N, H, D = (int(v) for v in g[f"shape_{ci}"])
        base, fwd = (float(v) for v in g[f"params_{ci}"])
        tok = torch.from_numpy(g[f"tokens_{ci}"].copy()).contiguous()
        pos = torch.from_numpy(g[f"pos_{ci}"].copy()).contiguous()
        assert emu.ptc_rope3d(tok.data_ptr(), F32, pos.data_ptr(), B * N, H, D, base, fwd, None) == 0
        # 2e-4: the bar of the GPU test of the same kernel (integer positions up to 300: the angle pos * (F0 / base^(i/Q)) of the CUDA
        # kernel and F0 * pos / base^(i/Q) of pointrope_cpu differ by an ulp of a 300-radian angle); the oracle with the kernel's
        # order of operations is matched much closer
        from oracle import pointrope as orope
        assert np.abs(tok.numpy() - g[f"out_{ci}"]).max() <= 2e-4 * np.abs(g[f"out_{ci}"]).max(), ci
        assert np.abs(tok.numpy() - orope.pointrope(g[f"tokens_{ci}"], g[f"pos_{ci}"], base, fwd)).max() <= 2e-5 * np.abs(g[f"out_{ci}"]).max(), ci


def test_rope3d_xyz_on_the_host_emulation(emu):
    """ptc_rope3d_xyz, thread by thread on the CPU: the reference Point3DRoPE golden (fp32), every dtype pair against the fp32 result
    rounded once, the pass-through slab, in place == out of place, sign = -1 inverts, and the argument checks."""
    g = np.load(os.path.join(GOLD, "ptv3m3_tiny.npz"))
    for ci in range(int(g["n_rope_cases"])):
        q, k = torch.from_numpy(g[f"rope_q_{ci}"]), torch.from_numpy(g[f"rope_k_{ci}"])
        xyz, f = torch.from_numpy(g[f"rope_xyz_{ci}"]).contiguous(), torch.from_numpy(g[f"rope_inv_freq_{ci}"]).contiguous()
        v = torch.randn(q.shape, generator=torch.Generator().manual_seed(ci))
        qkv = torch.stack((q, k, v), dim=1).contiguous()
        n, S, H, D = qkv.shape
        want = torch.stack((torch.from_numpy(g[f"rope_q_out_{ci}"]), torch.from_numpy(g[f"rope_k_out_{ci}"]), v), dim=1)

        def run(src, out_dtype, sign=1.0, rot=2):
            dst = torch.full(src.shape, float("nan")).to(out_dtype)
            rc = emu.ptc_rope3d_xyz(src.data_ptr(), _tag(src), dst.data_ptr(), _tag(dst), xyz.data_ptr(), f.data_ptr(), n, S, rot, H, D, sign, None)
            assert rc == 0, emu.emu_last_error()
            return dst

        out = run(qkv, torch.float32)
        assert (out - want).abs().max() <= 3e-6 * max(1.0, float(want.abs().max())), ci
        assert torch.equal(out[:, 2], qkv[:, 2])
        back = run(out, torch.float32, sign=-1.0)
        assert (back - qkv).abs().max() <= 5e-6 * float(qkv.abs().max())
        only_q = run(qkv, torch.float32, rot=1)                         # rot_slabs = 1: k passes through
        assert torch.equal(only_q[:, 1], qkv[:, 1]) and torch.equal(only_q[:, 0], out[:, 0])
        for in_dt in (torch.float32, torch.bfloat16, torch.float16):
            src = qkv.to(in_dt)
            ref32 = run(src.float(), torch.float32)
            for out_dt in (torch.float32, torch.bfloat16, torch.float16):
                got = run(src, out_dt)
                assert torch.equal(got, ref32.to(out_dt)), (ci, in_dt, out_dt)             # fp32 arithmetic, one rounding
        buf = qkv.to(torch.bfloat16).clone()
        keep_v = buf[:, 2].clone()
        assert emu.ptc_rope3d_xyz(buf.data_ptr(), BF16, buf.data_ptr(), BF16, xyz.data_ptr(), f.data_ptr(), n, S, 2, H, D, 1.0, None) == 0
        assert torch.equal(buf, run(qkv.to(torch.bfloat16), torch.bfloat16)) and torch.equal(buf[:, 2], keep_v)
    # argument checks (same code path as the library)
    z = torch.zeros(4, 3, 2, 18)
    x3, fr = torch.zeros(4, 3), torch.zeros(3)
    assert emu.ptc_rope3d_xyz(z.data_ptr(), F32, z.data_ptr(), BF16, x3.data_ptr(), fr.data_ptr(), 4, 3, 2, 2, 18, 1.0, None) == -1     # in place, two dtypes
    assert emu.ptc_rope3d_xyz(z.data_ptr(), F32, z.data_ptr(), F32, x3.data_ptr(), fr.data_ptr(), 4, 3, 2, 2, 20, 1.0, None) == -2
    assert emu.ptc_rope3d_xyz(z.data_ptr(), 7, z.data_ptr(), F32, x3.data_ptr(), fr.data_ptr(), 4, 3, 2, 2, 18, 1.0, None) == -1        # bad dtype tag


def test_rope3d_xyz_host_emulation_agrees_with_the_engine_formulation(emu):
    """the kernel (emulated) against functional.rope_xyz_torch -- the same arithmetic in torch ops -- on a random bf16 batch: bit-identical bf16 outputs."""
    from pointcept_amd import functional as PF

    gen = torch.Generator().manual_seed(12)
    n, H, D = 777, 3, 18
    qkv = torch.randn(n, 3, H, D, generator=gen).to(torch.bfloat16)
    xyz = (torch.rand(n, 3, generator=gen) * 9.0 - 2.0).contiguous()
    f = (1.0 / (10.0 ** (torch.arange(0, D // 3, 2).float() / (D // 3)))).contiguous()
    dst = torch.empty_like(qkv)
    assert emu.ptc_rope3d_xyz(qkv.data_ptr(), BF16, dst.data_ptr(), BF16, xyz.data_ptr(), f.data_ptr(), n, 3, 2, H, D, 1.0, None) == 0
    ref = PF.rope_xyz_torch(qkv, xyz, f)
    diff = (dst.float() - ref.float()).abs()
    # sin / cos come from two math libraries (glibc here, the device library on the GPU, ATen in the torch path): a last-bit
    # difference in sin / cos may flip a bf16 rounding of the product
    assert float((diff > 0).float().mean()) < 2e-3 and float(diff.max()) <= 2 ** -7 * float(ref.float().abs().max())


def test_serialize_encode_on_the_host_emulation_is_bit_exact(emu):
    """ptc_serialize_encode (csrc/serialize.hip, A2-A5) thread by thread on the CPU against tests/golden/serialization.npz = the
    reference's own `encode` for the four orders at depths 3..16, int64 and int32 coordinates, with and without the batch prefix;
    plus the entry point's argument checks."""
    g = np.load(os.path.join(GOLD, "serialization.npz"))
    depths = sorted(int(k.split("_")[1]) for k in g.files if k.startswith("gc_"))
    assert len(depths) >= 4
    orders = np.asarray([0, 1, 2, 3], dtype=np.int32)            # z, z-trans, hilbert, hilbert-trans (PTC_ORDER_*)
    for d in depths:
        gc, b, code = np.ascontiguousarray(g[f"gc_{d}"]), np.ascontiguousarray(g[f"batch_{d}"].astype(np.int64)), g[f"code_{d}"]
        n = gc.shape[0]
        for coords, is64 in ((gc.astype(np.int64), 1), (gc.astype(np.int32), 0)):
            out = np.full((4, n), -1, dtype=np.int64)
            rc = emu.ptc_serialize_encode(coords.ctypes.data, is64, b.ctypes.data, n, d, orders.ctypes.data, 4, out.ctypes.data, None)
            assert rc == 0 and np.array_equal(out, code), (d, is64)
        sub = np.asarray([3, 0], dtype=np.int32)                  # a subset of the orders, no batch prefix
        out = np.full((2, n), -1, dtype=np.int64)
        c64 = gc.astype(np.int64)
        assert emu.ptc_serialize_encode(c64.ctypes.data, 1, None, n, d, sub.ctypes.data, 2, out.ctypes.data, None) == 0
        low = (1 << (3 * d)) - 1
        assert np.array_equal(out[0], code[3] & low) and np.array_equal(out[1], code[0] & low), d
    assert emu.ptc_serialize_encode(None, 1, None, 10, 17, orders.ctypes.data, 4, None, None) == -1 and b"depth" in emu.emu_last_error()
    bad = np.asarray([0, 9], dtype=np.int32)
    assert emu.ptc_serialize_encode(None, 1, None, 10, 8, bad.ctypes.data, 2, None, None) == -1 and b"bad order" in emu.emu_last_error()
    assert emu.ptc_serialize_encode(None, 1, None, 0, 8, orders.ctypes.data, 4, None, None) == 0


def test_checked_and_raw_views_do_not_share_function_objects(emu):
    """a checked view bound FIRST on the same CDLL (attribute access on a CDLL caches one function object: an errcheck set through
    it would act in every view): the raw views -- the fixture's, bound before, and one bound after -- still return the status, the
    checked one raises it with the library's message"""
    import emu_backend
    from pointcept_amd import _lib

    cdll = emu_backend.build()
    checked = _lib.bind(cdll, checked=True, partial=True)
    raw = _lib.bind(cdll, checked=False, partial=True)
    orders = np.asarray([0, 1, 2, 3], dtype=np.int32)
    bad = (None, 1, None, 10, 17, orders.ctypes.data, 4, None, None)
    assert checked.ptc_serialize_encode is not raw.ptc_serialize_encode
    assert raw.ptc_serialize_encode(*bad) == -1 and emu.ptc_serialize_encode(*bad) == -1
    with pytest.raises(_lib.PtcoreError, match=r"^ptc_serialize_encode failed with code -1: .*depth") as e:
        checked.ptc_serialize_encode(*bad)
    assert e.value.code == -1
    assert raw.ptc_serialize_encode(*bad) == -1 and b"depth" in raw.ptc_last_error()
    assert checked.ptc_serialize_encode(None, 1, None, 0, 8, orders.ctypes.data, 4, None, None) == 0
    # emulated_ops(): checked behind ops.lib / _lib.lib, the raw view yielded and behind lib(checked=False)
    from pointcept_amd import ops

    with emu_backend.emulated_ops() as raw2:
        assert _lib.lib(checked=False) is raw2 and ops.lib() is _lib.lib() and ops.lib() is not raw2
        assert raw2.ptc_serialize_encode(*bad) == -1
        with pytest.raises(_lib.PtcoreError, match="depth"):
            ops.lib().ptc_serialize_encode(*bad)
        with pytest.raises(_lib.PtcoreError, match="ptc_no_such_entry: not part of the host emulation"):
            ops.lib().ptc_no_such_entry
    assert emu.ptc_serialize_encode(*bad) == -1


# ---- the bodies of -m gpu kernel tests on the emulated ops (tests/emu_backend.py) ---------------------------------------------
EMULATED_GPU_TESTS = [
    # keys, rows, rulebooks, pair operators (no LDS)
    ("test_serialize_encode_bit_exact", dict(depth=9, i64=True)), ("test_serialize_encode_bit_exact", dict(depth=16, i64=False)),
    ("test_gather_rows", dict(dtype=torch.float32, c=3)), ("test_gather_rows", dict(dtype=torch.bfloat16, c=96)),
    ("test_gather_rows", dict(dtype=torch.float16, c=16)),
    ("test_segment_csr", dict(dtype=torch.float32, reduce="max", c=64)), ("test_segment_csr", dict(dtype=torch.bfloat16, reduce="mean", c=3)),
    ("test_segment_csr", dict(dtype=torch.float32, reduce="sum", c=3)), ("test_segment_csr", dict(dtype=torch.bfloat16, reduce="min", c=64)),
    ("test_rulebook_subm", dict(ksize=3, dup=False)), ("test_rulebook_subm", dict(ksize=3, dup=True)),
    ("test_rulebook_subm", dict(ksize=5, dup=False)), ("test_rulebook_down", dict()),
    ("test_pointops2_pair_operators_match_the_reference_formulations", dict(seed=0)),
    # LDS + shuffles + workgroup barriers
    ("test_exclusive_scan", dict(n=1000)), ("test_exclusive_scan", dict(n=16384)), ("test_exclusive_scan", dict(n=16385)),
    ("test_exclusive_scan", dict(n=70000)),
    ("test_sort_keys_stable", dict(n=65)), ("test_sort_keys_stable", dict(n=4097)), ("test_sort_keys_bit_window", dict()),
    ("test_patch_pad_maps", dict(counts=[10, 3, 7], K=4)), ("test_patch_pad_maps", dict(counts=[1024, 1025, 5000, 1], K=1024)),
    ("test_attn_tables_match_index_algebra", dict(counts=[48, 49, 100, 7], K=48)),
    ("test_pool_level_counts", dict(row=0)), ("test_coord_max", dict(n=5000, dtype=torch.int32)),
    ("test_column_sum", dict(dtype=torch.float32, n=3000, c=64)),
    ("test_layer_norm_fwd_bwd", dict(c=64, xdt=torch.float32, ydt=torch.float32)),
    ("test_layer_norm_fwd_bwd", dict(c=36, xdt=torch.float32, ydt=torch.bfloat16)), ("test_layer_norm_fwd_bwd", dict(c=432, xdt=torch.bfloat16, ydt=torch.float32)),
    ("test_layer_norm_fwd_bwd", dict(c=1024, xdt=torch.bfloat16, ydt=torch.bfloat16)), ("test_layer_norm_empty_and_unsupported", dict()),
    ("test_cross_entropy_fwd_bwd", dict(dtype=torch.bfloat16, n=1000, c=20, strided=True)), ("test_cross_entropy_fwd_bwd", dict(dtype=torch.bfloat16, n=1, c=20, strided=False)),
    ("test_cross_entropy_fwd_bwd", dict(dtype=torch.float32, n=700, c=13, strided=False)), ("test_cross_entropy_fwd_bwd", dict(dtype=torch.float32, n=300, c=40, strided=True)),
    ("test_lovasz_softmax_matches_reference_golden_and_oracle", dict()), ("test_lovasz_softmax_16bit_strided_and_edge_cases", dict(dtype=torch.bfloat16, n=5000)),
    ("test_lovasz_softmax_16bit_strided_and_edge_cases", dict(dtype=torch.float16, n=56000)),
    ("test_layer_norm_affine_variants", dict(c=48, kw=dict(bias=False))), ("test_layer_norm_affine_variants", dict(c=18, kw=dict(elementwise_affine=False))),
    ("test_add_norm_fused_joint", dict(c=32, mode="ln_add_ln")), ("test_add_norm_fused_joint", dict(c=128, mode="add_ln_scaled")),
    ("test_add_norm_fused_joint", dict(c=48, mode="ln_add_ln")), ("test_add_norm_fused_joint", dict(c=432, mode="add_ln_scaled")),
    ("test_add_norm_fused_joint", dict(c=96, mode="f16_add_cast")), ("test_add_norm_fused_joint", dict(c=192, mode="fp32")),
    ("test_batch_norm_act_train", dict(dtype=torch.float32, n=3000, c=64, act="gelu")),
    ("test_batch_norm_act_train", dict(dtype=torch.bfloat16, n=2500, c=54, act="gelu")),      # 4-byte lanes
    ("test_batch_norm_act_train", dict(dtype=torch.bfloat16, n=1200, c=252, act="relu")),     # 8-byte lanes
    ("test_batch_norm_act_train", dict(dtype=torch.float32, n=3001, c=36, act="none")),       # fp32: 16-byte lanes still (36 = 9 x 4)
    ("test_batch_norm_act_train", dict(dtype=torch.float32, n=900, c=6, act="gelu")),         # fp32, 8-byte lanes
    ("test_batch_norm_add_act_is_the_residual_block_tail", dict(dtype=torch.bfloat16, n=5003, c=96)),
    ("test_pointops_knn_query", dict(nsample=3)), ("test_seg_eval_hist_matches_the_reference_formula", dict(dtype=torch.float32)),
    ("test_pointops_edge_operators", dict(c=8, w_c=4)), ("test_pointops_edge_operators", dict(c=3, w_c=1)), ("test_pointops_edge_operators", dict(c=6, w_c=2)),
    ("test_pair_list_attention_steps_and_their_gradients", dict(c=12)), ("test_pair_list_attention_steps_and_their_gradients", dict(c=5)),
    # MFMA kernels: implicit-GEMM convolution / Linear (16x16x32 bf16 / f16, 16x16x4 f32) and window attention (32x32x16 bf16)
    ("test_linear_gather_tables", dict(dtype=torch.bfloat16, cin=32, cout=96)),
    ("test_linear_gather_tables", dict(dtype=torch.bfloat16, cin=128, cout=384)),      # gemm3.h (gathered rows, kv = 2) and wgrad3.h on the emulation
    ("test_linear_identity_table", dict(dtype=torch.bfloat16, n=333, cin=256, cout=128)),
    ("test_linear_with_the_residual_joint_in_its_epilogue", dict(dtype=torch.bfloat16, cin=64, cout=64)),
    ("test_linear_with_the_residual_joint_in_its_epilogue", dict(dtype=torch.float16, cin=128, cout=32)),
    ("test_linear_with_the_residual_joint_in_its_epilogue", dict(dtype=torch.bfloat16, cin=128, cout=128)),
    ("test_mlp_one_kernel_per_direction", dict(dtype=torch.bfloat16, c=64, n=1100)), ("test_mlp_one_kernel_per_direction", dict(dtype=torch.float16, c=32, n=1100)),
    ("test_mlp_one_kernel_per_direction", dict(dtype=torch.bfloat16, c=32, n=129)), ("test_mlp_one_kernel_per_direction", dict(dtype=torch.float16, c=64, n=100)),
    ("test_unpooling_gather_with_addend", dict(dtype=torch.bfloat16, c=64)), ("test_unpooling_gather_with_addend", dict(dtype=torch.float32, c=20)),
    ("test_linear_identity_table", dict(dtype=torch.float32, n=1000, cin=32, cout=64)),
    ("test_linear_identity_table", dict(dtype=torch.bfloat16, n=300, cin=72, cout=288)), ("test_linear_identity_table", dict(dtype=torch.bfloat16, n=300, cin=288, cout=72)),
    ("test_linear_identity_table", dict(dtype=torch.float16, n=200, cin=432, cout=108)), ("test_linear_identity_table", dict(dtype=torch.bfloat16, n=150, cin=1008, cout=252)),
    ("test_spconv_fwd_and_wgrad", dict(dtype=torch.bfloat16, cin=32, cout=32, ksize=3)),
    ("test_spconv_fwd_chunked_pipeline", dict(cin=128, cout=128, ksize=3, n_pts=700)),      # conv3 with the two-chunk gather ring (DEEP)
    # (sizes: the smallest that still give several 128-row blocks per persistent workgroup / slice sequence -- the emulated MFMA loops
    #  of these six cases were 6 of the CPU tier's 13 minutes at 4500 / 2500 rows)
    ("test_sort_keys_at_the_packing_boundary", dict(n=1)), ("test_sort_keys_at_the_packing_boundary", dict(n=5000)),
    ("test_sort_keys_at_the_packing_boundary", dict(n=8193)),
    ("test_rulebook_blocks", dict(ordered=True)), ("test_spconv_fwd_block_staged", dict(c=64, ordered=True, n_rows=2100)),
    ("test_spconv_fwd_block_staged", dict(c=32, ordered=False, n_rows=2100)),
    ("test_spconv_fwd_block_staged_wide", dict(c=(224, 96), ordered=False, n_rows=700)),      # conv8: three 64-channel chunks + the 32-channel tail; staged blocks + blocks served by the conv3 follow-up
    ("test_spconv_wgrad_block_staged", dict(c=64, ordered=True, n_rows=1600)), ("test_spconv_wgrad_block_staged", dict(c=32, ordered=True, n_rows=1600)),
    ("test_spconv_wgrad_block_staged", dict(c=64, ordered=False, n_rows=1600)),
    ("test_spconv_wgrad_block_staged", dict(c=(128, 96), ordered=True, n_rows=1150)),     # channel slices on both sides (c = 96 alone: GPU suite)
    ("test_conv_tiny_inputs", dict(n=17)), ("test_spconv_dgrad_via_mirrored_table", dict()), ("test_spconv_down_up_tables", dict()),
    ("test_pool_maps", dict(n_pts=3000)),
    ("test_attention_fwd_bwd", dict(lens=[48, 48, 17], H=2)), ("test_attention_fwd_bwd", dict(lens=[1, 2, 31, 32, 33, 65], H=3)),
    ("test_attention_forward_launch_plans_agree_bit_for_bit", dict(lens=[256, 1, 300], H=2)),
    ("test_attention_launch_plan_cache_survives_more_shapes_than_it_holds", dict(n_shapes=66)),
    ("test_attention_large_logits", dict()), ("test_attention_dropout_fwd_bwd", dict(lens=[1, 2, 31, 32, 33, 65], H=3, p=0.25)),
    ("test_attention_dropout_fwd_bwd", dict(lens=[200], H=2, p=0.5)), ("test_attention_f16_io_equals_the_reference_cast_passes", dict(lens=[1, 2, 31, 32, 33, 65], H=3, one_pass="0")),
    ("test_attention_f16_io_equals_the_reference_cast_passes", dict(lens=[1, 2, 31, 32, 33, 65], H=3, one_pass="1")),
    ("test_attention_fwd_bwd", dict(lens=[300, 1024], H=1)),
    ("test_attention_backward_poisons_a_sequence_longer_than_max_seqlen", dict(one_pass="0")),
    ("test_attention_backward_poisons_a_sequence_longer_than_max_seqlen", dict(one_pass="1")),
    ("test_attention_other_head_dims_fwd_bwd", dict(D=18, lens=[1, 2, 31, 32, 33, 65], H=6, dtype=torch.bfloat16)),
    ("test_attention_other_head_dims_fwd_bwd", dict(D=18, lens=[1, 2, 31, 32, 33, 65], H=6, dtype=torch.float16)),
    ("test_attention_other_head_dims_fwd_bwd", dict(D=40, lens=[200, 100], H=2, dtype=torch.float16)),
    ("test_attention_with_fused_rope_equals_the_two_pass_form", dict(lens=[1, 2, 31, 32, 33, 65], H=6, dtype=torch.bfloat16)),
    ("test_attention_with_fused_rope_equals_the_two_pass_form", dict(lens=[1, 2, 31, 32, 33, 65], H=6, dtype=torch.float16)),
    ("test_attention_rpe_fwd_bwd", dict(lens=[200, 200, 200], H=3, bnd=18)),
    ("test_attention_rpe_f16_io_equals_the_cast_passes", dict(lens=[33], H=1, bnd=4)),
    ("test_attention_rpe_f16_io_equals_the_cast_passes", dict(lens=[200, 200, 200], H=3, bnd=18)),
]   # (in-place GPU tests -- rope3d, cross entropy -- are not in the list: with device = cpu their `.to(device)` aliases the input the
#    oracle is then fed with; tests that construct `pointcept_amd.nn` modules or open a CUDA autocast region cannot run on CPU tensors)


@pytest.mark.parametrize("name,kw", EMULATED_GPU_TESTS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(EMULATED_GPU_TESTS)])
def test_gpu_kernel_test_bodies_on_the_host_emulation(name, kw, monkeypatch):
    """tests/test_gpu_kernels.py bodies, unchanged, with device = cpu and pointcept_amd.ops bound to the host emulation of the SAME
    kernel sources: the product's serialization keys, row gathers, segmented reductions (forward and backward), submanifold and
    strided rulebooks (incl. duplicate voxels), rotary embedding and pair-list attention operators against their oracles, on the CPU."""
    import emu_backend
    import test_gpu_kernels as T

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    os.environ["PTC_EMU_CONV7_WGS"] = "3"      # conv7 is persistent: few workgroups = several blocks each at test sizes (emulation only)
    import inspect

    fn = getattr(T, name)
    if "monkeypatch" in inspect.signature(fn).parameters:
        kw = dict(kw, monkeypatch=monkeypatch)
    with emu_backend.emulated_ops():
        fn(torch.device("cpu"), **kw)


def _pointops2_edge_tests():
    from test_gpu_tests_dry_run_cpu import POINTOPS2_EDGE_TESTS

    return POINTOPS2_EDGE_TESTS + [("test_wrappers_refuse_bad_arguments_before_any_launch", dict())]


@pytest.mark.parametrize("name,kw", _pointops2_edge_tests(), ids=[f"{n}-{'-'.join(str(v) for v in k.values())}" for n, k in _pointops2_edge_tests()])
def test_gpu_pointops2_edge_test_bodies_on_the_host_emulation(name, kw):
    """tests/test_gpu_pointops2_edges.py, bodies unchanged, on the host emulation of csrc/pointops2.hip (no LDS, no wave
    intrinsics: one fiber per thread, atomics in program order): ragged, degenerate and empty pair lists, every gradient subset
    and the entry points' clears run the real kernel source on the CPU in every CPU run."""
    import emu_backend
    import test_gpu_pointops2_edges as T

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        getattr(T, name)(torch.device("cpu"), **kw)


def test_segmented_duplicate_merge_on_the_emulated_segment_kernel(monkeypatch):
    """functional._merge_duplicate_rows on the REAL ptc_segment_csr_fwd kernel (emulated) equals a per-row loop, fp32 and bf16 gradients."""
    import emu_backend
    from pointcept_amd import functional as PF

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    g = torch.Generator().manual_seed(3)
    n = 900
    rep = torch.arange(n)
    for r in torch.randperm(n, generator=g)[:200].tolist():
        if r > 0:
            rep[r] = int(torch.randint(0, r, (1,), generator=g))
    for _ in range(4):
        rep = torch.where(rep[rep] != rep, rep[rep], rep)
    assert bool((rep[rep] == rep).all())
    for dt, tol in ((torch.float32, 1e-6), (torch.bfloat16, 2.0 ** -7)):
        grad = torch.randn(n, 48, generator=g).to(dt)
        with emu_backend.emulated_ops():
            got = PF._merge_duplicate_rows(grad, rep)
        want = grad.float().clone()
        for r in range(n):
            if int(rep[r]) != r:
                want[int(rep[r])] += grad[r].float()
        want = torch.where((torch.bincount(rep, minlength=n) == 0)[:, None], grad.float(), want).to(dt)
        assert got.dtype == want.dtype and float((got.float() - want.float()).abs().max()) <= tol * float(want.float().abs().max()), dt


def test_ptv3m3_model_with_its_real_attention_and_rope_kernels_on_the_emulation(monkeypatch):
    """tests/test_gpu_m3_litept.py::test_ptv3m3_matches_reference_golden, body unchanged, on a hybrid
    backend: the model's window attention (head_dim 18: csrc/attention_hd.h, forward AND backward) and its Point3DRoPE pass
    (ptc_rope3d_xyz) run their REAL kernels on the host emulation, every other op on its oracle stand-in -- against the golden of the
    reference's own point_transformer_v3m3_utonia.py: eval features, train loss, every gradient norm."""
    import emu_backend
    import test_gpu_m3_litept as P

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.hybrid(["attn_varlen_fwd", "attn_varlen_bwd", "attn_hd_supported", "rope3d_xyz"]):
        P.test_ptv3m3_matches_reference_golden(torch.device("cpu"))


INDEX_AND_ATTENTION_OPS = ["coord_max", "serialize_encode", "sort_keys", "patch_pad_maps", "attn_tables", "pool_level_counts", "pool_maps",
                           "pool_child_codes", "gather_rows", "segment_csr_fwd", "segment_csr_bwd", "HashTable", "rulebook_subm", "rulebook_down",
                           "attn_varlen_fwd", "attn_varlen_bwd", "attn_hd_supported"]


@pytest.mark.parametrize("mod,name", [("test_gpu_model", "test_ptv3_tiny_forward_matches_reference_golden_and_oracle"),
                                      ("test_gpu_model", "test_ptv3_two_scenes_forward_backward_vs_oracle"),
                                      ("test_gpu_m3_litept", "test_litept_matches_reference_golden"),
                                      ("test_gpu_spunet", "test_spunet_tiny_matches_reference_golden_and_oracle"),
                                      ("test_gpu_spunet", "test_spunet_base_channels_single_scene_and_duplicates")])
def test_models_with_their_real_index_pipeline_and_attention_on_the_emulation(mod, name):
    """Model-level GPU tests, bodies unchanged, on the hybrid backend: the whole INDEX pipeline of the engine -- coordinate maxima,
    space-filling-curve keys, radix sort, pad / attention / pooling maps, voxel hash and submanifold rulebooks -- the row gathers,
    the segmented pooling reductions (forward and backward) and the window attention (forward and backward) run their REAL kernels
    on the host emulation inside the model; the GEMM-shaped ops stay on their oracle stand-ins (the emulated MFMA convolutions are
    checked at operator level above; a whole model of them would take minutes).  PT-v3m1 against the reference golden and the
    oracle model with every gradient; LitePT against the golden of the reference's own file."""
    import importlib

    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    T = importlib.import_module(mod)
    with emu_backend.hybrid(INDEX_AND_ATTENTION_OPS):
        getattr(T, name)(torch.device("cpu"))


@pytest.mark.skipif(os.environ.get("PTC_EMU_FULL_MODEL") != "1", reason="3.5 minutes: opt in with PTC_EMU_FULL_MODEL=1")
def test_whole_ptv3_step_with_every_kernel_on_the_emulation():
    """tests/test_gpu_model.py::test_ptv3_two_scenes_forward_backward_vs_oracle, body unchanged, with EVERY op of the engine on its real
    kernel (the MFMA convolutions and Linears -- forward, input gradient, weight gradient -- included; the three torch-side norm
    predicates keep their stand-in answers): PT-v3m1 forward + backward on two scenes against the oracle model, every gradient.
    Last run: passed in 219 s (8 host cores, one in use)."""
    import emu_backend
    import mock_backend
    import test_gpu_model as T

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    names = [n for n in mock_backend._STANDINS if n not in ("layer_norm_supported", "layer_norm_available", "layer_norm_joint_available", "batch_norm_supported", "linear_supported_ex")]
    with emu_backend.hybrid(names):
        T.test_ptv3_two_scenes_forward_backward_vs_oracle(torch.device("cpu"))


@pytest.mark.parametrize("ignore_index", [0, 5, 255])
def test_lovasz_kernels_with_an_ignore_index_inside_and_outside_the_class_range(ignore_index):
    """lovasz.py:149-166 drops the points labelled ignore_index whatever its value: the ScanNet configs use -1, SemanticKITTI-style label maps
    0 or 255.  The kernels' loss and gradient against the fp64 oracle for an ignore_index that IS a class index (its points must not count
    as foreground of that class) and for one above the range."""
    import emu_backend
    from oracle import losses
    from pointcept_amd import functional as PF

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    g = torch.Generator().manual_seed(3)
    n, c = 3000, 13
    x = torch.randn(n, c, generator=g) * 2
    y = torch.randint(0, c, (n,), generator=g)
    with emu_backend.emulated_ops():
        xe = x.clone().requires_grad_(True)
        loss = PF.lovasz_softmax(xe, y, ignore_index)
        loss.backward()
    lo, do = losses.lovasz_softmax(x.numpy(), y.numpy(), ignore_index)
    assert abs(float(loss.detach()) - lo) <= 2e-6 * abs(lo)
    assert np.abs(xe.grad.numpy() - do).max() <= 1e-4 * np.abs(do).max()
    if ignore_index < c:
        assert float(xe.grad[y == ignore_index].abs().max()) == 0.0


def test_cast_many_kernel_on_the_emulation_and_in_the_cast_cache(monkeypatch):
    """ptc_cast_many (one launch for the per-step fp32 -> 16-bit refresh of all weight shadows; the default refresh of functional._CastCache): on the
    emulation, for bf16 and f16, tensors whose sizes are not multiples of the 8-element unit and whose storage is not 16-byte
    aligned -- bit-identical to Tensor.to(); and through functional._CastCache (second step reuses the descriptor table, an
    in-place update of one weight refreshes it)."""
    import emu_backend
    from pointcept_amd import functional as PF
    from pointcept_amd import ops

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    g = torch.Generator().manual_seed(9)
    big = torch.randn(4096 + 3, generator=g)
    srcs = [torch.randn(n, generator=g) * 3 for n in (1, 7, 8, 9, 64, 1000, 27 * 32 * 32)] + [big[3:1003]]       # the last one: unaligned view
    for dt in (torch.bfloat16, torch.float16):
        dsts = [torch.full((s.numel(),), float("nan")).to(dt) for s in srcs]
        rows, prefix = [], [0]
        for s_, d_ in zip(srcs, dsts):
            rows.append([s_.data_ptr(), d_.data_ptr(), s_.numel()])
            prefix.append(prefix[-1] + (s_.numel() + 7) // 8)
        with emu_backend.emulated_ops():
            ops.cast_many(torch.tensor(rows, dtype=torch.int64), torch.tensor(prefix, dtype=torch.int64), len(rows), prefix[-1], dt)
        for s_, d_ in zip(srcs, dsts):
            assert torch.equal(d_, s_.to(dt)), (dt, s_.numel())
    # through the cache
    cache = PF._CastCache(cuda_only=False)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))      # the cache only takes the kernel route for CUDA tensors
    ws = [torch.nn.Parameter(torch.randn(24, 16, generator=g)), torch.nn.Parameter(torch.randn(5, 27, 8, generator=g))]
    with emu_backend.emulated_ops():
        for step in range(3):
            for w in ws:
                assert torch.equal(cache.get(w, torch.bfloat16), w.detach().to(torch.bfloat16)), step
            with torch.no_grad():
                ws[step % 2].mul_(1.5)                                                # the optimizer moves a weight: version counter
    assert cache._cast_desc is not None
    # a process that ran bf16 AND fp16 autocast holds shadows of both kinds: every refresh must serve each kind in its own dtype
    # (round 5: torch._foreach_copy_ over a mixed destination list wrote the first dtype's bit patterns into the second's shadows)
    with emu_backend.emulated_ops():
        for step in range(3):
            for dt in (torch.float16, torch.bfloat16):
                for w in ws:
                    assert torch.equal(cache.get(w, dt), w.detach().to(dt)), (step, dt)
            with torch.no_grad():
                for w in ws:
                    w.add_(0.125)
    assert set(cache._cast_desc) == {torch.bfloat16, torch.float16}


def test_pending_rope_kernel_gpu_test_body_on_the_emulation():
    """tests/test_gpu_m3_litept.py::test_rope3d_xyz_kernel_matches_reference_golden_and_inverts, body unchanged (golden cases,
    dtype pairs, the in-place library call, the 819200-row round trip), on the emulated kernel."""
    import emu_backend
    import test_gpu_m3_litept as P

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    with emu_backend.emulated_ops():
        P.test_rope3d_xyz_kernel_matches_reference_golden_and_inverts(torch.device("cpu"))


def test_block_executor_is_bit_identical_to_the_composed_path_on_the_emulation(monkeypatch):
    """csrc/block_exec.hip (one C call per PT-v3m1 Block and direction) against the same Block composed from the functional layer's
    autograd Functions, every kernel REAL on the host emulation: the two outputs (fp32 stream, bf16 copy), the gradients of both
    inputs and of all 18 parameters must be IDENTICAL -- 32 channels with DropPath row scales and an fp32 stream, 64 channels with a
    bf16 stream (first block of a stage) and the block-staged convolution (conv7)."""
    import numpy as np

    import emu_backend
    from oracle import maps as omaps
    from oracle import sfc as osfc
    from pointcept_amd import functional as PF
    from pointcept_amd import ops, synthetic

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))      # the weight-shadow cache only serves CUDA tensors
    PF.invalidate_weight_casts()

    def run(n_pts, C, H, patch, a_dtype, with_rs, blk_tables):
        b = synthetic.indoor_batch(2, n_pts)
        bt = omaps.offset2batch(b["offset"]); gc = b["grid_coord"]
        depth = int(gc.max()+1).bit_length()
        code = osfc.encode_c(gc, bt, depth, ("hilbert",))[0]
        o = np.argsort(code, kind="stable")
        ind = np.concatenate([bt[o,None], gc[o]],1).astype(np.int32)
        n = ind.shape[0]
        g = torch.Generator().manual_seed(C)
        def P(*s, scale=1.0): return (torch.randn(*s, generator=g)*scale).requires_grad_(True)
        params = [P(C,3,3,3,C,scale=(27*C)**-0.5), P(C,scale=0.1), P(C,C,scale=C**-0.5), P(C,scale=0.1), (1+P(C,scale=0.1)).detach().requires_grad_(True), P(C,scale=0.1),
                  (1+P(C,scale=0.1)).detach().requires_grad_(True), P(C,scale=0.1), P(3*C,C,scale=C**-0.5), P(3*C,scale=0.1), P(C,C,scale=C**-0.5), P(C,scale=0.1),
                  (1+P(C,scale=0.1)).detach().requires_grad_(True), P(C,scale=0.1), P(4*C,C,scale=C**-0.5), P(4*C,scale=0.1), P(C,4*C,scale=(4*C)**-0.5), P(C,scale=0.1)]
        x0 = torch.randn(n, C, generator=g).to(a_dtype)
        xc = torch.randn(n, C, generator=g).to(torch.bfloat16)
        with emu_backend.emulated_ops():
            nbr = ops.rulebook_subm(torch.from_numpy(ind), 3)
            offs = torch.from_numpy(b["offset"].astype(np.int64))
            order = torch.from_numpy(np.argsort(np.random.default_rng(1).permutation(n)))   # some serialization order
            inverse = torch.empty_like(order); inverse[order] = torch.arange(n)
            # per-scene order must keep scenes contiguous: build from a key (batch, random)
            key = torch.from_numpy(bt[o].astype(np.int64))*10**9 + torch.from_numpy(np.random.default_rng(2).integers(0,10**8,n))
            order = torch.argsort(key); inverse = torch.empty_like(order); inverse[order]=torch.arange(n)
            pad, unpad, cu, dup = ops.patch_pad_maps(offs, [int(v) for v in offs], patch)
            tabs = ops.attn_tables(order, inverse, pad, unpad, dup)
            blk = ops.BlockTables(nbr) if blk_tables else None
            rs1 = (torch.rand(n, generator=g) > 0.3).float()/0.7 if with_rs else None
            rs2 = (torch.rand(n, generator=g) > 0.3).float()/0.7 if with_rs else None
            meta = dict(dt=torch.bfloat16, n_pad=int(tabs[0].shape[1]), n_seq=int(cu.numel())-1, heads=H, patch=patch, scale=16**-0.5, eps_cpe=1e-5, eps_n1=1e-5, eps_n2=1e-5,
                        nbr=nbr, blk=blk, tabs=tabs, cu=cu)
            dz = torch.randn(n, C, generator=g); dyb = torch.randn(n, C, generator=g).to(torch.bfloat16)
            res = []
            for mode in ("exec", "composed"):
                for p in params: p.grad = None
                x0r = x0.clone().requires_grad_(True); xcr = xc.clone().requires_grad_(True)
                if mode == "exec":
                    x3, xb = PF.ptv3_block(x0r, xcr, rs1, rs2, meta, params)
                else:
                    (wc,bc,wl,bl,gcp,bcp,g1,b1,wq,bq,wp,bp,g2,b2,w1,bb1,w2,bb2) = params
                    class LN:  # minimal norm holder
                        def __init__(s,w,b): s.weight,s.bias,s.eps=w,b,1e-5
                    class BP:
                        def get(s,*a,**k): return blk
                    conv = PF.sparse_conv(xcr, wc.reshape(C,27,C), bc, nbr, nbr, True, None, None, BP() if blk is not None else None)
                    lin = PF.linear(conv, wl, bl)
                    x1, y1 = PF.add_norm(lin, x0r, None, LN(gcp,bcp), LN(g1,b1), torch.bfloat16)
                    qkv = PF.linear(y1, wq, bq, tabs[0], tabs[1])
                    out = PF.attn_varlen_qkvpacked(qkv.reshape(-1,3,H,16), cu, patch, 16**-0.5)
                    a = PF.linear(out.reshape(-1,C), wp, bp, tabs[2], tabs[3])
                    x2, y2 = PF.add_norm(a, x1, rs1, None, LN(g2,b2), torch.bfloat16)
                    m = PF.mlp_gelu(y2, w1, bb1, w2, bb2)
                    x3, xb = PF.add_norm(m, x2, rs2, None, None, torch.bfloat16)
                torch.autograd.backward([x3, xb], [dz, dyb])
                res.append([x3.detach().clone(), xb.detach().clone(), x0r.grad.clone(), xcr.grad.clone()] + [p.grad.clone() for p in params])
        names = ["x3","xb3","dx0","dxc"]+list(PF._BLK_PARAMS)
        worst = 0.0
        for nm,a_,b_ in zip(names,res[0],res[1]):
            d = float((a_.float()-b_.float()).abs().max()); worst=max(worst,d)
            if d != 0.0: print("   DIFF", nm, d, float(b_.float().abs().max()))
        assert worst == 0.0
        print(f"n={n} C={C} H={H} patch={patch} a={a_dtype} rs={with_rs} blk={blk_tables}: max |exec - composed| over outputs and 22 gradients = {worst}")

    try:
        run(700, 32, 2, 128, torch.float32, True, False)
        run(2300, 64, 4, 128, torch.bfloat16, False, True)
        run(500, 96, 6, 128, torch.float32, True, False)      # round 5: a width that is no power of two (PT-v3m2's 96 / 192): separate joints, run-time-width LayerNorm
    finally:
        PF.invalidate_weight_casts()
