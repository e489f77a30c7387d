"""PPT-v1m1 on SpUNet-v1m3 (configs/scannet/semseg-ppt-v1m1-0-sc-st-spunet.py: SpUNet base channels, bf16 autocast) at 8 scenes x
100 000 voxels, K = 20 (the ScanNet condition), D = 512 (CLIP ViT-B/16): the language-guided head alone (forward + backward, on
features of the backbone's output dtype) and the whole train step, with time and peak allocation, kernel path (csrc/ppt.hip) against
PTC_PPT=0 (the reference's expression in torch) in one process, alternating, with the spread of the repeats.

    python tools/ppt_step.py [--scenes 8] [--points 100000] [--reps 7] [--out profiles/ppt_step.txt]

Each measurement runs in a child process of its own under a time limit; the parent never touches the GPU."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BACKBONE = dict(type="SpUNet-v1m3", in_channels=6, num_classes=0, base_channels=32, context_channels=256,
                channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2), zero_init=False, norm_decouple=True,
                norm_adaptive=True, norm_affine=True, conditions=("Structured3D", "ScanNet", "S3DIS"))
CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1), dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
STAGES = ("head", "step")
WIDTH = 512


def child(what, scenes, points, reps):
    import torch

    from pointcept_amd import config, synthetic
    from pointcept_amd.point_prompt_training import PointPromptTraining

    dev = torch.device("cuda")
    torch.manual_seed(0)
    emb = torch.nn.functional.normalize(torch.randn(36, WIDTH), dim=1)
    model = PointPromptTraining(backbone=BACKBONE, criteria=CRITERIA, backbone_out_channels=96, class_embedding=emb,
                                logit_scale=math.log(100.0)).to(dev)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.1, momentum=0.9, nesterov=True)
    b = synthetic.to_torch(synthetic.collate([synthetic.indoor_scene(300 + i, points) for i in range(scenes)]), dev)
    b["condition"] = ["ScanNet"]
    n = int(b["offset"][-1])
    torch.manual_seed(1)
    feat = torch.randn(n, 96, device=dev).to(torch.bfloat16).requires_grad_(True)
    cot = torch.randn(n, 20, device=dev)
    rows = model.class_embedding[list(model.valid_index[1]), :]

    def head():
        feat.grad = model.proj_head.weight.grad = model.proj_head.bias.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model._logits(feat, rows, 0.0)
        (logits.float() * cot).sum().backward()

    def train_step():
        model.train()
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(dict(b))["loss"]
        loss.backward()
        opt.step()

    fn = dict(head=head, step=train_step)[what]
    res = {"points": n}
    times = {True: [], False: []}
    for kernels in (True, False):                  # warm-up of both sides
        config.PPT_KERNELS = kernels
        fn()
        fn()
    for _ in range(reps):                          # alternating, so that drift hits both sides alike
        for kernels in (True, False):
            config.PPT_KERNELS = kernels
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[kernels].append(e0.elapsed_time(e1))
    res["kernel_ms"], res["torch_ms"] = times[True], times[False]
    for kernels in (True, False):
        config.PPT_KERNELS = kernels
        feat.grad = None
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        res["peak_mb_kernel" if kernels else "peak_mb_torch"] = (torch.cuda.max_memory_allocated() - base) / 2**20
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.scenes, a.points, a.reps)
    lines = [f"PPT-v1m1 on SpUNet-v1m3 (base channels, PDNorm decoupled + adaptive + affine), condition ScanNet: {a.scenes} scenes x {a.points} "
             f"points before voxelisation (the size after it is on every line), C = 96, D = {WIDTH}, K = 20, bf16 autocast; median [min .. max] "
             f"of {a.reps} alternating repeats, ms, each one event-timed call (head: functional.ppt_head forward + backward on bf16 features; "
             f"step: forward, backward, SGD) including its host reads; comparison side = PTC_PPT=0 on the same build"]
    for what in STAGES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--scenes", str(a.scenes),
               "--points", str(a.points), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"{what}: child failed with status {r.returncode}: {r.stderr[-400:]}")
            print(lines[-1])
            if r.returncode in (124, 134, 137, 139, -6, -11):
                break                               # a fault or a hang: nothing more is started on the GPU
            continue
        res = json.loads(got[0][7:])
        fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"       # noqa: E731
        kt, tt = res["kernel_ms"], res["torch_ms"]
        verdict = "faster beyond the spread" if max(kt) < min(tt) else "slower beyond the spread" if min(kt) > max(tt) else "within the spread"
        lines.append(f"{what:5s} kernels {fmt(kt)}   PTC_PPT=0 {fmt(tt)}   -> {verdict}   ({res['points']} points)")
        print(lines[-1])
        lines.append(f"{'':5s} peak allocation above what was held before the call: kernels {res['peak_mb_kernel']:.1f} MB, "
                     f"PTC_PPT=0 {res['peak_mb_torch']:.1f} MB")
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if any("child failed" in ln for ln in lines) else 0


if __name__ == "__main__":
    sys.exit(main())
