"""MSC-v1m1 at the ScanNet config's shape (configs/scannet/pretrain-msc-v1m1-0-spunet-base.py: SpUNet base channels, fp32, SGD,
4 scenes per view, crops of 100 000 points that hold about 83 000 after voxelisation): the three stages of the wrapper (cross masks, matching + pair selection, InfoNCE
forward + backward) and the whole train step, kernel path (csrc/msc.hip) against PTC_MSC=0 (the reference's expression on
ptc_knn_query and torch) in one process, alternating, with the spread of the repeats; and the peak allocation of the loss.

    python tools/msc_step.py [--scenes 4] [--points 100000] [--reps 7] [--out profiles/msc_ops.txt]
    python tools/msc_step.py --model v1m2 [--r1 2 --r2 20] [--stages loss,step] [--out profiles/msc_csc_ops.txt]

--model v1m2: MSC-v1m2 with the settings of configs/scannet/pretrain-msc-v1m2-0-spunet-csc.py (mask_rate 0, no reconstruction heads,
partitions 4, r1 / r2 from the command line); its `loss` and `step` stages run MaskedSceneContrastCSC, whose loss is the partitioned
InfoNCE (functional.msc_csc_nce against functional.msc_csc_nce_torch).

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


def child(what, scenes, points, reps, which="v1m1", r1=2.0, r2=20.0):
    import torch

    from pointcept_amd import config, synthetic
    from pointcept_amd.masked_scene_contrast import MaskedSceneContrast, MaskedSceneContrastCSC

    dev = torch.device("cuda")
    torch.manual_seed(0)
    if which == "v1m2":
        model = MaskedSceneContrastCSC(backbone=BACKBONE, backbone_in_channels=6, backbone_out_channels=96, mask_rate=0, reconstruct_color=False,
                                       reconstruct_normal=False, partitions=4, r1=r1, r2=r2).to(dev)
    else:
        model = MaskedSceneContrast(backbone=BACKBONE, backbone_in_channels=6, backbone_out_channels=96).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.8, nesterov=True)
    b = synthetic.to_torch(synthetic.contrastive_views_batch([300 + i for i in range(scenes)], [points] * scenes), dev)
    o1, o2 = b["view1_origin_coord"], b["view2_origin_coord"]
    f1, f2 = b["view1_offset"].int(), b["view2_offset"].int()
    torch.manual_seed(1)
    x1 = torch.randn(o1.shape[0], 96, device=dev, requires_grad=True)
    x2 = torch.randn(o2.shape[0], 96, device=dev, requires_grad=True)
    mi = model.match_contrastive_pair(o1, f1, o2, f2, 8, 0.03)

    def loss_step():
        x1.grad = x2.grad = None
        if which == "v1m2":
            model.compute_contrastive_loss(x1, o1, f1, x2, o2, f2, mi)[0].backward()
        else:
            model.compute_contrastive_loss(x1, f1, x2, f2, mi)[0].backward()

    def train_step():
        opt.zero_grad(set_to_none=True)
        model(dict(b))["loss"].backward()
        opt.step()

    stages = dict(masks=lambda: model.generate_cross_masks(o1, f1, o2, f2), matching=lambda: model.match_contrastive_pair(o1, f1, o2, f2, 8, 0.03),
                  loss=loss_step, step=train_step)
    fn = stages[what]
    res = {"points_view1": int(o1.shape[0]), "points_view2": int(o2.shape[0]), "pairs": int(mi.shape[0])}
    if which == "v1m2":
        from pointcept_amd import ops

        _, counts, _ = ops.msc_csc_nce_fwd(x1.detach(), o1, f1, x2.detach(), o2, mi, 0.4, r1, r2)
        res["class_members"] = counts.sum(0).tolist()
        res["pairs_per_scene"] = [int(round(v ** 0.5)) for v in counts.sum(1).tolist()]
    times = {True: [], False: []}
    for kernels in (True, False):                  # warm-up of both sides
        config.MSC_KERNELS = kernels
        fn()
        fn()
    for _ in range(reps):                          # alternating, so that drift hits both sides alike
        for kernels in (True, False):
            config.MSC_KERNELS = kernels
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[kernels].append(e0.elapsed_time(e1))
    res["kernel_ms"], res["torch_ms"] = times[True], times[False]
    if what == "loss":
        for kernels in (True, False):
            config.MSC_KERNELS = kernels
            x1.grad = x2.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            loss_step()
            torch.cuda.synchronize()
            res["peak_mb_kernel" if kernels else "peak_mb_torch"] = (torch.cuda.max_memory_allocated() - base) / 2**20
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--limit", type=int, default=70, help="seconds per child")
    ap.add_argument("--model", choices=("v1m1", "v1m2"), default="v1m1")
    ap.add_argument("--r1", type=float, default=2.0, help="v1m2: inner radius of the CSC partitions")
    ap.add_argument("--r2", type=float, default=20.0, help="v1m2: outer radius")
    ap.add_argument("--stages", default="masks,matching,loss,step")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.scenes, a.points, a.reps, a.model, a.r1, a.r2)
    head = "MSC-v1m1" if a.model == "v1m1" else f"MSC-v1m2 (mask_rate 0, no heads, partitions 4, r1 {a.r1:g}, r2 {a.r2:g})"
    lines = [f"{head}, ScanNet config shape: {a.scenes} scenes per view, crops of {a.points} points before voxelisation (the sizes after "
             f"it are on every line), fp32, SpUNet base channels; median [min .. max] of {a.reps} alternating repeats, ms, each one "
             f"event-timed call including its host reads; comparison side = PTC_MSC=0 on the same build"]
    for what in a.stages.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--scenes", str(a.scenes),
               "--points", str(a.points), "--reps", str(a.reps), "--model", a.model, "--r1", str(a.r1), "--r2", str(a.r2)]
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
        lines.append(f"{what:9s} kernels {fmt(k)}   PTC_MSC=0 {fmt(t)}   -> {verdict}   (view1 {res['points_view1']} points = {res['points_view1'] // a.scenes} per scene, view2 {res['points_view2']}, P {res['pairs']})")
        if "peak_mb_kernel" in res:
            lines.append(f"{'':9s} peak allocation of loss forward + backward above its inputs: kernels {res['peak_mb_kernel']:.1f} MB, PTC_MSC=0 {res['peak_mb_torch']:.1f} MB")
        print(lines[-1] if "peak_mb_kernel" not in res else lines[-2] + "\n" + lines[-1])
        if "class_members" in res and what == "loss":
            lines.append(f"{'':9s} pairs per scene {res['pairs_per_scene']}, members of the classes 0-3 and the rest over all scenes {res['class_members']}")
            print(lines[-1])
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
