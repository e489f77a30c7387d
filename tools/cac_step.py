"""CAC-v1m1 at the ScanNet config's shape (configs/scannet/semseg-cac-v1m1-0-spunet-base.py: SpUNet base channels, fp32,
3 scenes x 100 000 points, C = 96) for K = 20 (ScanNet) and K = 200 (ScanNet200): the three stages of the wrapper -- soft pooling +
cosine logits (the refinement), hard pooling + cosine logits (the adaptive branch), the distillation loss, each forward + backward --
the eval forward and the whole train step, kernel path (csrc/cac.hip) against PTC_CAC=0 (the reference's expression in torch) in one
process, alternating, with the spread of the repeats; and the peak allocation of the three wrapper stages.

    python tools/cac_step.py [--scenes 3] [--points 100000] [--reps 7] [--out profiles/cac_ops.txt]

Each measurement runs in a child process of its own under a time limit; the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2))
CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1), dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
STAGES = ("refine", "adaptive", "distill", "eval", "step")


def child(what, k, scenes, points, reps):
    import torch

    from pointcept_amd import config, synthetic
    from pointcept_amd.context_aware_classifier import CACSegmentor

    dev = torch.device("cuda")
    torch.manual_seed(0)
    # above 64 classes the criteria are the cross entropy alone (both sides alike), as when profiles/cac_ops.txt was taken: the engine's
    # Lovasz kernels stopped at 64 classes then
    model = CACSegmentor(num_classes=k, backbone_out_channels=96, backbone=BACKBONE, criteria=CRITERIA if k <= 64 else CRITERIA[:1],
                         conf_thresh=0.75).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    b = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(300 + i, points) for i in range(scenes)]), dev)
    n, offset = int(b["offset"][-1]), b["offset"]
    torch.manual_seed(1)
    feat = torch.randn(n, 96, device=dev, requires_grad=True)
    target = (b["segment"] if k == 20 else torch.where(b["segment"] < 0, b["segment"], torch.randint(0, k - 10, (n,), device=dev))).long()
    logits = (torch.randn(n, k, device=dev) * 4).requires_grad_(True)
    soft = torch.randn(n, k, device=dev) * 4
    head = model.seg_head.weight

    def refine():
        feat.grad = logits.grad = None
        model.train()
        model.post_refine_proto_batch(feat, logits, head, offset).sum().backward()

    def adaptive():
        feat.grad = None
        model.train()
        model.get_adaptive_perspective(feat, target, head.detach(), head).sum().backward()

    def distill():
        logits.grad = None
        model.get_distill_loss(logits, soft, target).backward()

    def eval_forward():
        model.eval()
        with torch.no_grad():
            model({key: v for key, v in b.items() if key != "segment"})

    def train_step():
        model.train()
        opt.zero_grad(set_to_none=True)
        model(dict(b))["loss"].backward()
        opt.step()

    fn = dict(refine=refine, adaptive=adaptive, distill=distill, eval=eval_forward, step=train_step)[what]
    res = {"points": n}
    times = {True: [], False: []}
    for kernels in (True, False):                  # warm-up of both sides
        config.CAC_KERNELS = kernels
        fn()
        fn()
    for _ in range(reps):                          # alternating, so that drift hits both sides alike
        for kernels in (True, False):
            config.CAC_KERNELS = kernels
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[kernels].append(e0.elapsed_time(e1))
    res["kernel_ms"], res["torch_ms"] = times[True], times[False]
    if what in ("refine", "adaptive", "distill"):
        for kernels in (True, False):
            config.CAC_KERNELS = kernels
            feat.grad = logits.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            res["peak_mb_kernel" if kernels else "peak_mb_torch"] = (torch.cuda.max_memory_allocated() - base) / 2**20
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=3)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--limit", type=int, default=90, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.k, a.scenes, a.points, a.reps)
    lines = [f"CAC-v1m1, ScanNet config shape: {a.scenes} scenes x {a.points} points before voxelisation (the size after it is on every "
             f"line), C = 96, fp32, SpUNet base channels, conf_thresh 0.75; median [min .. max] of {a.reps} alternating repeats, ms, each one "
             f"event-timed call (the three stages forward + backward) including its host reads; comparison side = PTC_CAC=0 on the same build; "
             f"criteria CrossEntropy + Lovasz, above 64 classes CrossEntropy alone (as in profiles/cac_ops.txt)"]
    stop = False
    for k in a.classes:
        for what in STAGES:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--k", str(k), "--scenes",
                   str(a.scenes), "--points", str(a.points), "--reps", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not got:
                lines.append(f"K={k:3d} {what}: child failed with status {r.returncode}: {r.stderr[-400:]}")
                print(lines[-1])
                if r.returncode in (124, 134, 137, 139, -6, -11):
                    stop = True                         # a fault or a hang: nothing more is started on the GPU
                    break
                continue
            res = json.loads(got[0][7:])
            fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"
            kt, tt = res["kernel_ms"], res["torch_ms"]
            verdict = "faster beyond the spread" if max(kt) < min(tt) else "slower beyond the spread" if min(kt) > max(tt) else "within the spread"
            lines.append(f"K={k:3d} {what:9s} kernels {fmt(kt)}   PTC_CAC=0 {fmt(tt)}   -> {verdict}   ({res['points']} points)")
            print(lines[-1])
            if "peak_mb_kernel" in res:
                lines.append(f"{'':15s} peak allocation above its inputs: kernels {res['peak_mb_kernel']:.1f} MB, PTC_CAC=0 {res['peak_mb_torch']:.1f} MB")
                print(lines[-1])
        if stop:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
