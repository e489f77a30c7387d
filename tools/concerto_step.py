"""Concerto-v1m1 at the shape of configs/concerto/pretrain-concerto-v1m1-0-base.py (the PT-v3m2 backbone of that config on six input
channels, up_cast_level 2, enc2d_upcast_level 3, backbone_out_channels 1184, enc2d_head_in_channels 1536, 37 x 37 patches, 4 images
per scene, bf16 autocast) with the stand-in image encoder of pointcept_amd.synthetic, so that the timing is the point side's:

  align  the alignment branch alone, Concerto.alignment_loss forward + backward (pool_corr through the loss) on a hand-made pooled
         point: `--points` input points per global view in clusters of four, random pixel correspondences (half of them -1), random
         bf16 features of 1184 channels and precomputed bf16 patch features of 1536 channels;
  step   one train step of the model (forward, backward, AdamW, after_step) on synthetic multi-view crops with images.

Kernel path (csrc/concerto.hip) against PTC_CONCERTO=0 (the reference's per-image pool_corr loop, dense scatter_mean, patch_proj over
every patch, torch.unique, gathers and elementwise cosine) in one process on the same inputs, alternating, with the spread of the
repeats and the peak allocation.

    python tools/concerto_step.py [--scenes 2] [--points 100000] [--step-points 20000] [--reps 7] [--out profiles/concerto_step.txt]

Each measurement runs in a child process of its own under a time limit; the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BACKBONE = dict(type="PT-v3m2", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2), enc_depths=(3, 3, 3, 12, 3),
                enc_channels=(48, 96, 192, 384, 512), enc_num_head=(3, 6, 12, 24, 32), enc_patch_size=(1024,) * 5, drop_path=0.0,
                shuffle_orders=True, traceable=True, enc_mode=True, mask_token=True)
TINY = dict(BACKBONE, enc_depths=(1, 1, 1, 1, 1))
PATCH, IMAGES, C3D, C2D = 37, 4, 96 + 192 + 384 + 512, 1536


def build(backbone, dev):
    from pointcept_amd import synthetic
    from pointcept_amd.concerto import Concerto

    return Concerto(image_weight_name="stand-in", image_weight_path=None, backbone=backbone, head_in_channels=192 + 384 + 512,
                    backbone_out_channels=C3D, embedding_channels=C2D, patch_w=PATCH, patch_h=PATCH, head_hidden_channels=4096,
                    head_embed_channels=256, head_num_prototypes=4096, enc2d_head_in_channels=C2D, enc2d_head_hidden_channels=4096,
                    enc2d_head_embed_channels=256, enc2d_head_num_prototypes=4096, teacher_custom=dict(drop_path=0.0), mask_jitter=0.01,
                    match_max_r=0.32, up_cast_level=2, enc2d_upcast_level=3, sonata_model_type="online",
                    enc2d_model=synthetic.stand_in_image_encoder(PATCH, PATCH, C2D)).to(dev).train()


def child(what, scenes, points, step_points, reps):
    import torch

    from pointcept_amd import config, synthetic
    from pointcept_amd.structure import Point

    dev = torch.device("cuda")
    torch.manual_seed(0)
    res = {}
    if what == "align":
        model = build(TINY, dev)
        views = 2 * scenes
        n0, m = views * points, views * points // 4
        batch0 = torch.arange(views, device=dev).repeat_interleave(points)
        corr = torch.randint(0, PATCH, (n0, IMAGES, 2), device=dev)
        corr[torch.rand(n0, IMAGES, device=dev) < 0.5] = -1
        inverse = torch.arange(n0, device=dev) // 4
        idx_ptr = torch.arange(0, n0 + 1, 4, device=dev)
        feat = torch.randn(m, C3D, device=dev).bfloat16().requires_grad_(True)
        feature2d = torch.randn(scenes * IMAGES * PATCH * PATCH, C2D, device=dev).bfloat16()
        img_num = torch.full((scenes,), IMAGES, device=dev)
        offset = torch.arange(1, views + 1, device=dev) * (points // 4)

        def fn():
            feat.grad = None
            model.patch_proj.zero_grad(set_to_none=True)
            parent = Point(dict(feat=feat.new_zeros(1, 1), offset=offset * 4, batch=batch0))
            point = Point(dict(feat=feat, offset=offset, batch=batch0[::4].contiguous(), pooling_parent=parent, pooling_inverse=inverse,
                               idx_ptr=idx_ptr))
            point["_ptc_pool_csr"] = (torch.arange(n0, device=dev), idx_ptr)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                loss = model.alignment_loss(point, corr, img_num, feature2d=feature2d)
            loss.backward()
        fn()
        res["shape"] = (f"{scenes} scenes x 2 global views x {points} points -> {m} pooled points, {IMAGES} images of {PATCH} x {PATCH} patches "
                        f"per scene, {model.last['num_pairs']} pairs in {int(model.last['patch_ids'].numel())} patches, {C3D} -> {C2D} channels, bf16")
    else:
        model = build(BACKBONE, dev)
        opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4)
        b = synthetic.to_torch(synthetic.multi_view_image_batch([400 + i for i in range(scenes)], step_points, step_points // 3,
                                                                [IMAGES] * scenes, PATCH, PATCH, patch_size=0.03, pixels_per_patch=1), dev)

        def fn():
            opt.zero_grad(set_to_none=True)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                loss = model(dict(b))["loss"]
            loss.backward()
            opt.step()
            model.after_step()
        fn()
        res["shape"] = (f"{scenes} scenes, global {int(b['global_coord'].shape[0])} / local {int(b['local_coord'].shape[0])} points, "
                        f"{model.last['num_pairs']} pairs in {int(model.last['patch_ids'].numel())} patches, bf16 autocast")
    times, peak = {True: [], False: []}, {}
    for kernels in (True, False):                  # warm-up of both sides
        config.CONCERTO_KERNELS = kernels
        fn()
        fn()
    for _ in range(reps):                          # alternating, so that drift hits both sides alike
        for kernels in (True, False):
            config.CONCERTO_KERNELS = kernels
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[kernels].append(e0.elapsed_time(e1))
    for kernels in (True, False):
        config.CONCERTO_KERNELS = kernels
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
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--points", type=int, default=100000, help="input points per global view of the align stage")
    ap.add_argument("--step-points", type=int, default=20000, help="points per global crop of the step stage")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds per child")
    ap.add_argument("--stages", default="align,step")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.scenes, a.points, a.step_points, a.reps)
    lines = [f"Concerto-v1m1, patch_proj {C3D} -> {C2D}, {PATCH} x {PATCH} patches, {IMAGES} images per scene, stand-in image encoder; median "
             f"[min .. max] of {a.reps} alternating repeats, ms, each one event-timed call including its host reads; peak = allocation of "
             f"one call above what was allocated before it; comparison side = PTC_CONCERTO=0 on the same build"]
    for what in a.stages.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what, "--scenes", str(a.scenes),
               "--points", str(a.points), "--step-points", str(a.step_points), "--reps", str(a.reps)]
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
        lines.append(f"{what:5s} kernels {fmt(k)}   PTC_CONCERTO=0 {fmt(t)}   -> {verdict}   peak {res['peak_mb_kernel']:.1f} MB | "
                     f"{res['peak_mb_torch']:.1f} MB   ({res['shape']})")
        print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
