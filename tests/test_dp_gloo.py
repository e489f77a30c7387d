"""N > 1 path on CPU: world_size 2, gloo backend, rendezvous on 127.0.0.1.  Covers the host logic
bench.py uses for data parallelism (pointcept_amd/dp.py): process-group init from the torchrun
environment, disjoint scene sharding, DDP gradient averaging with per-rank BatchNorm statistics,
barrier + max-over-ranks timing.  (The HIP ops themselves cannot run on CPU by design.)
"""
import os
import socket
import sys

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from pointcept_amd import dp

    dev = torch.device("cpu")
    dp.init_distributed(backend="gloo")
    torch.manual_seed(0)  # identical initial weights on every rank
    model = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.BatchNorm1d(16), torch.nn.GELU(), torch.nn.Linear(16, 5))
    ddp = dp.wrap_ddp(model, dev)
    seeds = dp.scene_seeds(rank, 3)
    g = torch.Generator().manual_seed(seeds[0])
    x = torch.randn(64 + 8 * rank, 6, generator=g)  # ragged per-rank batch
    y = torch.randint(0, 5, (x.shape[0],), generator=g)
    loss = torch.nn.functional.cross_entropy(ddp(x), y)
    loss.backward()
    dp.barrier(dev)
    t = dp.max_over_ranks(1.0 + rank, dev)
    total = dp.sum_over_ranks(float(x.shape[0]), dev)
    grads = [p.grad.numpy().copy() for p in model.parameters()]
    # local (un-averaged) gradient of the same loss on a fresh copy
    torch.manual_seed(0)
    ref = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.BatchNorm1d(16), torch.nn.GELU(), torch.nn.Linear(16, 5))
    torch.nn.functional.cross_entropy(ref(x), y).backward()
    q.put((rank, seeds, t, total, grads, [p.grad.numpy().copy() for p in ref.parameters()],
           model[1].running_mean.numpy().copy()))  # numpy: plain pickles, no shared-memory handles
    torch.distributed.destroy_process_group()


def test_ddp_gloo_world2():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, s0, t0, n0, g0, l0, bn0), (r1, s1, t1, n1, g1, l1, bn1) = res
    assert set(s0).isdisjoint(s1)                      # scenes shard, no overlap
    assert t0 == t1 == 2.0                             # max over ranks
    assert n0 == n1 == 64 + 72                         # sum over ranks
    import numpy as np

    for a, b, la, lb in zip(g0, g1, l0, l1):
        assert np.allclose(a, b, atol=1e-7)            # all-reduced gradients are identical on both ranks
        assert np.allclose(a, (la + lb) / 2, atol=1e-6)  # ... and equal the mean of the local gradients
    assert not np.allclose(bn0, bn1)                   # broadcast_buffers=False: BN statistics stay per rank


def _engine_worker(rank, world, port, q):
    """the ENGINE's PT-v3m1 (python layer + autograd wrappers; ops on the CPU stand-ins of tests/mock_backend.py) under
    DistributedDataParallel over gloo: one process per rank, different scenes per rank, CE + Lovasz loss."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import mock_backend
    from pointcept_amd import dp, synthetic
    from pointcept_amd.point_transformer_v3 import PointTransformerV3
    from pointcept_amd.segmentor import DefaultSegmentorV2

    dev = torch.device("cpu")
    dp.init_distributed(backend="gloo")
    cfg = dict(in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), enc_depths=(1, 1, 1, 1, 1), dec_depths=(1, 1, 1, 1),
               enc_patch_size=(64,) * 5, dec_patch_size=(64,) * 4, drop_path=0.0, shuffle_orders=False)
    with mock_backend.cpu_ops():
        torch.manual_seed(0)                                       # identical initial weights on every rank
        model = DefaultSegmentorV2(20, 64, PointTransformerV3(**cfg), criteria=("ce", "lovasz")).train()
        ddp = dp.wrap_ddp(model, dev)
        seeds = dp.scene_seeds(rank, 2, base_seed=700)
        batch = synthetic.collate([synthetic.indoor_scene(s, 300 + 60 * rank) for s in seeds])
        batch = {k: torch.from_numpy(v) for k, v in batch.items()}
        torch.manual_seed(5)
        loss = ddp(dict(batch))["loss"]
        loss.backward()
        dp.barrier(dev)
        names = [n for n, _ in model.named_parameters()]
        grads = [p.grad.numpy().copy() for _, p in model.named_parameters()]
        # the same loss on a fresh, unwrapped copy: the local (un-averaged) gradient
        torch.manual_seed(0)
        ref = DefaultSegmentorV2(20, 64, PointTransformerV3(**cfg), criteria=("ce", "lovasz")).train()
        torch.manual_seed(5)
        ref(dict(batch))["loss"].backward()
        local = [p.grad.numpy().copy() for _, p in ref.named_parameters()]
    q.put((rank, float(loss.detach()), names, grads, local))
    torch.distributed.destroy_process_group()


def test_engine_model_under_ddp_gloo_world2():
    """N > 1 path with the engine's own model and autograd Functions: the all-reduced gradients are identical on both
    ranks and equal the mean of the two local gradients (scenes shard, the only exchange is the gradient all-reduce)."""
    import numpy as np

    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, l0, names, g0, loc0), (_, l1, _, g1, loc1) = res
    assert l0 != l1                                                   # different scenes per rank
    gmax = max(float(np.abs(a).max()) for a in g0)
    for n, a, b, la, lb in zip(names, g0, g1, loc0, loc1):
        assert np.allclose(a, b, atol=1e-7 * max(gmax, 1.0)), n        # identical after the all-reduce
        assert np.allclose(a, (la + lb) / 2, rtol=2e-2, atol=2e-3 * gmax), n   # = mean of the local gradients (bf16 attention roundings)


def _executor_worker(rank, world, port, q, emu_lib):
    """ONE PT-v3m1 Block through the block executor (csrc/block_exec.hip, every kernel real on the host emulation) under
    DistributedDataParallel(gradient_as_bucket_view=True, static_graph off) over gloo: the executor returns its 18 parameter gradients as
    VIEWS of one slab; DDP must take them into its buckets on the first step (grad = None) and on a second step where .grad already IS
    a bucket view (zero_grad(set_to_none=False): autograd accumulates in place)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      PTC_EMU_LIB=emu_lib)
    torch.set_num_threads(2)
    import numpy as np

    import emu_backend
    from oracle import maps as omaps
    from oracle import sfc as osfc
    from pointcept_amd import dp, ops, synthetic
    from pointcept_amd import functional as PF

    C, H, patch = 32, 2, 64

    class OneBlock(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(0)                     # identical initial weights on every rank

            def P(*s, scale=1.0, one=False):
                return torch.nn.Parameter(torch.randn(*s, generator=g) * scale + (1.0 if one else 0.0))
            self.params = torch.nn.ParameterList([
                P(C, 3, 3, 3, C, scale=(27 * C) ** -0.5), P(C, scale=0.1), P(C, C, scale=C ** -0.5), P(C, scale=0.1), P(C, scale=0.1, one=True), P(C, scale=0.1),
                P(C, scale=0.1, one=True), P(C, scale=0.1), P(3 * C, C, scale=C ** -0.5), P(3 * C, scale=0.1), P(C, C, scale=C ** -0.5), P(C, scale=0.1),
                P(C, scale=0.1, one=True), P(C, scale=0.1), P(4 * C, C, scale=C ** -0.5), P(4 * C, scale=0.1), P(C, 4 * C, scale=(4 * C) ** -0.5), P(C, scale=0.1)])

        def forward(self, x0, xc, meta):
            return PF.ptv3_block(x0, xc, None, None, meta, list(self.params))

    dev = torch.device("cpu")
    dp.init_distributed(backend="gloo")
    model = OneBlock()
    ddp = dp.wrap_ddp(model, dev)
    assert type(ddp).__name__ == "DistributedDataParallel" and ddp.gradient_as_bucket_view and not ddp.static_graph
    ref = OneBlock()
    torch.Tensor.is_cuda = property(lambda self: True)               # the weight-shadow cache only serves CUDA tensors (this process only)
    out = []
    with emu_backend.emulated_ops():
        for it in range(2):
            b = synthetic.indoor_batch(2, 150 + 40 * rank + 10 * it)        # different scenes per rank and step
            bt = omaps.offset2batch(b["offset"])
            code = osfc.encode_c(b["grid_coord"], bt, int(b["grid_coord"].max() + 1).bit_length(), ("hilbert",))[0]
            o = np.argsort(code, kind="stable")
            ind = np.concatenate([bt[o, None], b["grid_coord"][o]], 1).astype(np.int32)
            n = ind.shape[0]
            g = torch.Generator().manual_seed(100 * rank + it)
            nbr = ops.rulebook_subm(torch.from_numpy(ind), 3)
            offs = torch.from_numpy(b["offset"].astype(np.int64))
            key = torch.from_numpy(bt[o].astype(np.int64)) * 10 ** 9 + torch.randint(0, 10 ** 8, (n,), generator=g)
            order = torch.argsort(key)
            inverse = torch.empty_like(order)
            inverse[order] = torch.arange(n)
            pad, unpad, cu, dup = ops.patch_pad_maps(offs, [int(v) for v in offs], patch)
            tabs = ops.attn_tables(order, inverse, pad, unpad, dup)
            meta = dict(dt=torch.bfloat16, n_pad=int(tabs[0].shape[1]), n_seq=int(cu.numel()) - 1, heads=H, patch=patch, scale=16 ** -0.5, eps_cpe=1e-5,
                        eps_n1=1e-5, eps_n2=1e-5, nbr=nbr, blk=None, tabs=tabs, cu=cu)
            x0, xc = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g).to(torch.bfloat16)
            dz, dyb = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g)
            if it == 1:
                ddp.zero_grad(set_to_none=False)                     # .grad stays the bucket view; this step accumulates into it
            x3, xb = ddp(x0, xc, meta)
            ((x3 * dz).sum() + (xb.float() * dyb).sum()).backward()
            views = sum(int(p.grad._base is not None or p.grad.storage_offset() != 0) for p in model.parameters())   # grads living in DDP's buckets
            ref.zero_grad(set_to_none=True)
            y3, yb = ref(x0, xc, meta)
            ((y3 * dz).sum() + (yb.float() * dyb).sum()).backward()
            out.append(([p.grad.detach().numpy().copy() for p in model.params], [p.grad.detach().numpy().copy() for p in ref.params], views))
    q.put((rank, out))
    torch.distributed.destroy_process_group()


def test_block_executor_slab_gradients_under_ddp_gloo_world2():
    """the executor's slab-view parameter gradients through DDP's bucket views, two ranks, two steps; after each
    step every rank holds the mean of the two ranks' local gradients (the executor run without DDP on the same inputs)."""
    import numpy as np
    import pytest

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import emu_backend

    if not emu_backend.available():
        pytest.skip("no host clang++ under /opt/rocm")
    lib = emu_backend.library_path()
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_executor_worker, args=(r, world, port, q, lib)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=900) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for it in range(2):
        g0, l0, v0 = res[0][it]
        g1, l1, _ = res[1][it]
        assert v0 == len(g0), (it, v0)                                              # gradient_as_bucket_view: every .grad is a view of a bucket
        for k, (a, b, la, lb) in enumerate(zip(g0, g1, l0, l1)):
            scale = max(float(np.abs(la).max()), float(np.abs(lb).max()), 1e-6)
            assert np.array_equal(a, b), (it, k)                                   # identical after the all-reduce
            assert np.allclose(a, (la + lb) / 2, rtol=1e-5, atol=1e-5 * scale), (it, k, float(np.abs(a - (la + lb) / 2).max()), scale)
            assert float(np.abs(la - lb).max()) > 1e-3 * scale                     # the ranks really saw different data


def _run_bench(*argv, env_extra=None, timeout=300):
    import subprocess

    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, env=env, timeout=timeout)


def test_bench_self_launch_gloo_stub():
    """`python bench.py --gpus 2` WITHOUT a torchrun environment spawns its own two ranks (the role of
    pointcept/engines/launch.py:106-136); rank 0 prints ONE JSON line with n_gpus = 2 = the size of the process group.
    --stub: gloo + CPU tensors + a small torch model through the SAME dp.py / timing / JSON code as the GPU run; once plain and
    once with --full."""
    import json

    outs = {}
    for mode in ("plain", "full"):
        r = _run_bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "2", "--stub", *(["--full"] if mode == "full" else []))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = outs[mode] = json.loads(lines[0])
        assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["steps"] == 3 and out["warmup"] == 1
        assert out["config"]["global_batch"] == 4 and out["config"]["parallelism"] == "dp2" and out["scaling"] == "weak"
        assert out["value"] > 0 and abs(out["value"] - 4 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-2 * out["value"]
    # a plain run measures the headline only; --full adds the multi-rank diagnostics (VERDICT r2 next 6 ii): every rank's own step
    # time and the step time without the gradient exchange
    assert not {"per_rank_ms_per_step", "ms_per_step_without_gradient_exchange", "exposed_allreduce_ms_per_step"} & set(outs["plain"])
    out = outs["full"]
    assert len(out["per_rank_ms_per_step"]) == 2 and all(v > 0 for v in out["per_rank_ms_per_step"])
    assert out["ms_per_step_without_gradient_exchange"] > 0 and out["exposed_allreduce_ms_per_step"] is not None
    # per-rank CPU affinity (VERDICT r3 next 7 i): the ranks of a node get disjoint core sets and a bounded thread pool
    aff = out["cpu_affinity_rank0"]
    assert aff["pinned"] == (len(os.sched_getaffinity(0)) >= 1) and aff["cores"] >= 1 and 1 <= aff["threads"] <= 8


def test_bench_dump_outputs_stub(tmp_path):
    """--dump-outputs DIR: after the timed steps, the last step's loss, logits, gradients and updated parameters as float32 / float64
    .npy files under 64 MB; two runs with the same arguments write the same arrays, a different step count different ones."""
    import json

    import numpy as np

    dumps = {}
    for tag, steps in (("a", "2"), ("b", "2"), ("c", "3")):
        r = _run_bench("--gpus", "1", "--steps", steps, "--warmup", "1", "--batch", "2", "--stub", "--dump-outputs", str(tmp_path / tag))
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert out["steps"] == int(steps) and out["dumped_outputs"]["dir"] == str(tmp_path / tag)
        dumps[tag] = {f.stem: np.load(f) for f in sorted((tmp_path / tag).glob("*.npy"))}
        assert set(dumps[tag]) == {"loss", "logits", "grad_norm", "grad_sample", "param_sample"}
        assert {k: list(a.shape) for k, a in dumps[tag].items()} == out["dumped_outputs"]["arrays"]
        assert all(a.dtype in (np.float32, np.float64) for a in dumps[tag].values())
        assert sum(a.nbytes for a in dumps[tag].values()) <= 64 << 20
        assert round(float(dumps[tag]["loss"]), 4) == out["config"]["final_loss"]
        assert dumps[tag]["logits"].shape == (2 * 256, 20) and dumps[tag]["grad_norm"].shape == (6,)
    for k in dumps["a"]:
        assert np.array_equal(dumps["a"][k], dumps["b"][k]), k
    assert not np.array_equal(dumps["a"]["param_sample"], dumps["c"]["param_sample"])


def test_bench_runs_the_prebuilt_library_of_a_read_only_tree(monkeypatch):
    """bench.py on a built tree this user cannot write (another build compared through --dump-outputs): HIPCC="" sends every
    build() of the run to the library already built; a writable tree keeps its rebuild-on-demand"""
    import bench
    from pointcept_amd import build as B

    monkeypatch.setenv("HIPCC", "unset below; restored after the test")
    monkeypatch.delenv("HIPCC")
    monkeypatch.setattr(bench.os, "access", lambda path, mode: True)
    bench.use_prebuilt_library_if_read_only()
    assert "HIPCC" not in os.environ
    monkeypatch.setattr(bench.os, "access", lambda path, mode: False)
    bench.use_prebuilt_library_if_read_only()
    assert os.environ["HIPCC"] == ""
    monkeypatch.setattr(B, "HIPCC", os.environ["HIPCC"])
    monkeypatch.setattr(B, "_build_locked", None)
    assert B.build() == B.LIB


def test_rank_core_share_is_disjoint_and_numa_local():
    """dp.rank_core_share: even split of the GPU's NUMA-local cores among the ranks on that node, an even slice of the allowed
    cores when the topology is unknown; disjoint across ranks either way"""
    from pointcept_amd import dp

    allowed = list(range(256))
    numa = [list(range(0, 128))] * 4 + [list(range(128, 256))] * 4          # 8 GPUs, 4 per socket
    shares = [dp.rank_core_share(r, 8, allowed, numa) for r in range(8)]
    assert all(len(s) == 32 for s in shares)
    assert all(set(shares[r]) <= set(numa[r]) for r in range(8))
    assert len(set().union(*map(set, shares))) == 256
    # unknown topology: plain slices
    shares = [dp.rank_core_share(r, 8, allowed, None) for r in range(8)]
    assert [s[0] for s in shares] == [32 * r for r in range(8)] and all(len(s) == 32 for s in shares)
    # a cgroup that allows fewer cores than ranks: every rank still gets at least one core
    shares = [dp.rank_core_share(r, 8, [3, 5, 9], None) for r in range(8)]
    assert all(len(s) >= 1 for s in shares)
    # NUMA list known for some GPUs only -> falls back to slices of the allowed set
    assert dp.rank_core_share(1, 2, list(range(8)), [list(range(4)), None]) == [4, 5, 6, 7]


def test_bench_refuses_fewer_gpus_than_asked():
    """no GPU in this container: --gpus 2 must fail loudly, never print an n_gpus = 1 line"""
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        import pytest

        pytest.skip("needs a box with fewer than 2 GPUs")
    r = _run_bench("--gpus", "2", "--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert "refusing" in (r.stderr + r.stdout)
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())
    # a torchrun environment whose world size disagrees with --gpus is refused as well
    r = _run_bench("--gpus", "4", "--steps", "1", "--warmup", "0", "--stub",
                   env_extra=dict(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29512"))
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)
