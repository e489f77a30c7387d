"""The criteria kernels (csrc/criteria.hip) at the outdoor batch -- 8 LiDAR sweeps of ~180 000 voxels, 19 classes, bf16 logits:

  kitti   the SemanticKITTI criteria (class-weighted CrossEntropyLoss + LovaszLoss, semantic_kitti/semseg-spunet-v1m1-0-base.py)
          through criteria.Criteria on random logits, forward + backward;
  fused3  class-weighted label-smoothed CrossEntropyLoss + FocalLoss + DiceLoss through criteria.Criteria (one seg_criteria call),
          forward + backward;
  step    one train step of SpUNet-v1m1 (4 input channels, 19 classes, SGD, bf16 autocast) on synthetic.outdoor_scene sweeps with the
          SemanticKITTI criteria.

Kernel path against PTC_CRITERIA=0 (the torch twins: the reference's expressions) in one process on the same inputs, alternating, with
the spread of the repeats and the peak allocation of one call.

    python tools/criteria_step.py [--scenes 8] [--rows 180000] [--reps 9] [--out profiles/criteria_step.txt]

Each measurement runs in a child process of its own under a time limit; the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KITTI_WEIGHT = [3.1557, 8.7029, 7.8281, 6.1354, 6.3161, 7.9937, 8.9704, 10.1922, 1.6155, 4.2187, 1.9385, 5.5455, 2.0198, 2.6261, 1.3212,
                5.1102, 2.5492, 5.8585, 7.3929]
KITTI = [dict(type="CrossEntropyLoss", weight=KITTI_WEIGHT, loss_weight=1.0, ignore_index=-1),
         dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
FUSED3 = [dict(type="CrossEntropyLoss", weight=KITTI_WEIGHT, label_smoothing=0.1, loss_weight=1.0, ignore_index=-1),
          dict(type="FocalLoss", gamma=2.0, alpha=0.25, loss_weight=1.0, ignore_index=-1),
          dict(type="DiceLoss", smooth=1, exponent=2, loss_weight=1.0, ignore_index=-1)]
SPUNET_BASE = dict(channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2))  # semseg-spunet-v1m1-0-base.py


def child(what, scenes, rows, reps):
    import torch

    from pointcept_amd import config, synthetic
    from pointcept_amd.criteria import Criteria

    dev = torch.device("cuda")
    torch.manual_seed(0)
    res = {}
    if what in ("kitti", "fused3"):
        crit = Criteria(KITTI if what == "kitti" else FUSED3)
        n = scenes * rows
        logits = (torch.randn(n, 19, device=dev) * 3).bfloat16().requires_grad_(True)
        target = torch.randint(0, 19, (n,), device=dev)
        target[torch.rand(n, device=dev) < 0.05] = -1

        def fn():
            logits.grad = None
            crit(logits, target).backward()
        res["shape"] = f"{n} rows x 19 classes, bf16 logits, 5 % ignored"
    else:
        from pointcept_amd.sparse_unet import SpUNetBase

        crit = Criteria(KITTI)
        model = SpUNetBase(4, 19, **SPUNET_BASE).to(dev).train()
        opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
        batch = synthetic.to_torch(synthetic.collate([synthetic.outdoor_scene(5000 + i, azimuth_steps=3300) for i in range(scenes)]), dev)
        seg = batch["segment"].long()

        def fn():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = crit(model(dict(batch)), seg)
            loss.backward()
            opt.step()
        res["shape"] = f"SpUNet-v1m1, {scenes} sweeps, {int(seg.numel())} voxels, 19 classes, SGD, bf16 autocast"
    times, peak = {True: [], False: []}, {}
    for kernels in (True, False):                  # warm-up of both sides
        config.CRITERIA_KERNELS = kernels
        fn()
        fn()
    for _ in range(reps):                          # alternating, so that drift hits both sides alike
        for kernels in (True, False):
            config.CRITERIA_KERNELS = kernels
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[kernels].append(e0.elapsed_time(e1))
    for kernels in (True, False):
        config.CRITERIA_KERNELS = kernels
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
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--rows", type=int, default=180000, help="rows per scene of the kitti / fused3 stages")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--stages", default="kitti,fused3,step")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.scenes, a.rows, a.reps)
    lines = [f"criteria kernels against PTC_CRITERIA=0 on the same build; median [min .. max] of {a.reps} alternating repeats, ms, each one "
             f"event-timed forward + backward (step: + optimizer); peak = allocation of one call above what was allocated before it"]
    for what in a.stages.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--scenes", str(a.scenes),
               "--rows", str(a.rows), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"{what}: child failed with status {r.returncode}: {r.stderr[-400:]}")
            print(lines[-1])
            if r.returncode in (124, 134, 137, 139, -6, -11):
                break                               # a fault or a hang: nothing more is started on the GPU
            continue
        res = json.loads(got[0][7:])
        fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"      # noqa: E731
        k, t = res["kernel_ms"], res["torch_ms"]
        verdict = "faster beyond the spread" if max(k) < min(t) else "slower beyond the spread" if min(k) > max(t) else "within the spread"
        lines.append(f"{what:6s} kernels {fmt(k)}   PTC_CRITERIA=0 {fmt(t)}   -> {verdict}   peak {res['peak_mb_kernel']:.1f} MB | "
                     f"{res['peak_mb_torch']:.1f} MB   ({res['shape']})")
        print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
