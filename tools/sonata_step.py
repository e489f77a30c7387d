"""Sonata-v1m1 at the shipped head shape (configs/sonata/pretrain-sonata-v1m1-0-base.py: 1088 -> 4096 -> 256 -> 4096 prototypes, bf16
autocast) on synthetic multi-view crops: the distillation loss alone (forward + backward on random cosine-like logits of M matched
rows) and one train step of the model on a reduced PT-v3m2, kernel path (csrc/sonata.hip) against PTC_SONATA=0 (the reference's
dense Sinkhorn-Knopp expression) in one process, alternating, with the spread of the repeats and the peak allocation.

    python tools/sonata_step.py [--pairs 65536] [--scenes 2] [--points 20000] [--reps 7] [--out profiles/sonata_ops.txt]

Each measurement runs in a child process of its own under a time limit; the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BACKBONE = dict(type="PT-v3m2", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2), enc_depths=(1, 1, 1, 2, 1),
                enc_channels=(48, 96, 192, 384, 512), enc_num_head=(3, 6, 12, 24, 32), enc_patch_size=(1024,) * 5, drop_path=0.0,
                shuffle_orders=True, traceable=True, enc_mode=True, mask_token=True)
K = 4096


def child(what, pairs, scenes, points, reps):
    import torch

    from pointcept_amd import config, synthetic
    from pointcept_amd import functional as PF
    from pointcept_amd.sonata import Sonata

    dev = torch.device("cuda")
    torch.manual_seed(0)
    res = {}
    if what == "loss":
        nt, ns = pairs // 2 + 3, pairs + pairs // 4
        teacher = (torch.rand(nt, K, device=dev) * 2 - 1).bfloat16()
        student = (torch.rand(ns, K, device=dev) * 2 - 1).bfloat16().requires_grad_(True)
        rows = torch.randperm(ns, device=dev)[:pairs].sort().values
        mi = torch.stack([rows, torch.randint(nt, (pairs,), device=dev)], 1)
        batch = (torch.arange(ns, device=dev) * 8) // ns

        def fn():
            student.grad = None
            PF.sonata_distill(teacher, student, mi, batch, 0.07, 0.1, num_scenes=8).backward()
        res["shape"] = f"M {pairs} pairs x K {K}, bf16 logits, 8 scenes"
    else:
        model = Sonata(backbone=BACKBONE, head_in_channels=192 + 384 + 512, head_hidden_channels=4096, head_embed_channels=256,
                       head_num_prototypes=K, teacher_custom=dict(drop_path=0.0), mask_jitter=0.01, match_max_r=0.32).to(dev).train()
        opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4)
        b = synthetic.to_torch(synthetic.multi_view_batch([400 + i for i in range(scenes)], points, points // 3), dev)

        def fn():
            opt.zero_grad(set_to_none=True)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                loss = model(dict(b))["loss"]
            loss.backward()
            opt.step()
            model.after_step()
        fn()
        res["shape"] = (f"{scenes} scenes, global {int(b['global_coord'].shape[0])} / local {int(b['local_coord'].shape[0])} points, pairs "
                        f"{[int(model.last[k].shape[0]) for k in ('mask_match_index', 'roll_mask_match_index', 'unmask_match_index')]}, bf16 autocast")
    times, peak = {True: [], False: []}, {}
    for kernels in (True, False):                  # warm-up of both sides
        config.SONATA_KERNELS = kernels
        fn()
        fn()
    for _ in range(reps):                          # alternating, so that drift hits both sides alike
        for kernels in (True, False):
            config.SONATA_KERNELS = kernels
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[kernels].append(e0.elapsed_time(e1))
    for kernels in (True, False):
        config.SONATA_KERNELS = kernels
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[kernels] = (torch.cuda.max_memory_allocated() - base) / 2**20
    res.update(kernel_ms=times[True], torch_ms=times[False], peak_mb_kernel=peak[True], peak_mb_torch=peak[False])
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--limit", type=int, default=100, help="seconds per child")
    ap.add_argument("--stages", default="loss,step")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.pairs, a.scenes, a.points, a.reps)
    lines = [f"Sonata-v1m1, head 1088 -> 4096 -> 256 -> {K} prototypes; median [min .. max] of {a.reps} alternating repeats, ms, each one "
             f"event-timed call including its host reads; peak = allocation of one call above what was allocated before it; comparison "
             f"side = PTC_SONATA=0 on the same build"]
    for what in a.stages.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--pairs", str(a.pairs),
               "--scenes", str(a.scenes), "--points", str(a.points), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"{what}: child failed with status {r.returncode}: {r.stderr[-400:]}")
            print(lines[-1])
            if r.returncode in (124, 134, 137, 139, -6, -11):
                break                               # a fault or a hang: nothing more is started on the GPU
            continue
        res = json.loads(got[0][7:])
        fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"
        k, t = res["kernel_ms"], res["torch_ms"]
        verdict = "faster beyond the spread" if max(k) < min(t) else "slower beyond the spread" if min(k) > max(t) else "within the spread"
        lines.append(f"{what:5s} kernels {fmt(k)}   PTC_SONATA=0 {fmt(t)}   -> {verdict}   peak {res['peak_mb_kernel']:.1f} MB | {res['peak_mb_torch']:.1f} MB"
                     f"   ({res['shape']})")
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
