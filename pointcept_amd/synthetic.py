"""Seeded synthetic voxelised scenes (SURVEY section 8(d) / Appendix B generators) for bench.py and
the tests: there is no network for datasets, so every measurement uses these.

indoor_scene : room 7 x 5 x 2.8 m (floor + 4 walls, 12000 pts/m^2) + 14 boxes, voxelised at 0.02 m,
               sphere-cropped to `point_max` voxels (pointcept/datasets/transform.py:1015-1057),
               feat = colour(3) | normal(3), segment in [0,20) with 5 % ignore (-1).
Layout matches point_collate_fn (pointcept/datasets/utils.py:19-73): coord [N,3] f32,
grid_coord [N,3] i64, feat [N,6] f32, segment [N] i64, offset [B] i64.
"""
from __future__ import annotations

import numpy as np


def _rect(rng, o, u, v, n):
    a = rng.random((n, 1))
    b = rng.random((n, 1))
    return np.asarray(o, float) + a * np.asarray(u, float) + b * np.asarray(v, float)


def _box(rng, c, s, n):
    c = np.array(c, float)
    s = np.array(s, float)
    P, Nrm = [], []
    for ax in range(3):
        for sg in (-1, 1):
            o = c.copy()
            o[ax] += sg * s[ax] / 2
            u = np.zeros(3)
            v = np.zeros(3)
            u[(ax + 1) % 3] = s[(ax + 1) % 3]
            v[(ax + 2) % 3] = s[(ax + 2) % 3]
            P.append(_rect(rng, o - u / 2 - v / 2, u, v, n))
            nn = np.zeros(3)
            nn[ax] = sg
            Nrm.append(np.tile(nn, (n, 1)))
    return np.concatenate(P), np.concatenate(Nrm)


def indoor_scene(seed: int, point_max: int = 102400, grid: float = 0.02, density: int = 12000):
    rng = np.random.default_rng(seed)
    L, W, H = 7.0, 5.0, 2.8
    parts = [
        (_rect(rng, [0, 0, 0], [L, 0, 0], [0, W, 0], int(L * W * density)), [0, 0, 1]),
        (_rect(rng, [0, 0, 0], [L, 0, 0], [0, 0, H], int(L * H * density)), [0, 1, 0]),
        (_rect(rng, [0, W, 0], [L, 0, 0], [0, 0, H], int(L * H * density)), [0, -1, 0]),
        (_rect(rng, [0, 0, 0], [0, W, 0], [0, 0, H], int(W * H * density)), [1, 0, 0]),
        (_rect(rng, [L, 0, 0], [0, W, 0], [0, 0, H], int(W * H * density)), [-1, 0, 0]),
    ]
    P = [p for p, _ in parts]
    Nr = [np.tile(np.asarray(nv, float), (p.shape[0], 1)) for p, nv in parts]
    for _ in range(14):
        s = rng.uniform(0.3, 1.6, 3)
        bp, bn = _box(rng, [rng.uniform(0.8, L - 0.8), rng.uniform(0.8, W - 0.8), s[2] / 2], s, int(density * 1.2))
        P.append(bp)
        Nr.append(bn)
    p = np.concatenate(P)
    nrm = np.concatenate(Nr)
    gc = np.floor(p / grid).astype(np.int64)
    gc -= gc.min(0)
    # one point per voxel (GridSample train mode keeps one representative per voxel)
    key = (gc[:, 0] * 4096 + gc[:, 1]) * 4096 + gc[:, 2]
    _, first = np.unique(key, return_index=True)
    gc, nrm = gc[first], nrm[first]
    if gc.shape[0] > point_max:  # SphereCrop: the point_max voxels nearest a random voxel
        centre = gc[rng.integers(gc.shape[0])]
        d2 = ((gc - centre) ** 2).sum(1)
        keep = np.argpartition(d2, point_max)[:point_max]
        keep = keep[rng.permutation(point_max)]  # dataloader order is not spatially sorted
        gc, nrm = gc[keep], nrm[keep]
    gc = gc - gc.min(0)
    n = gc.shape[0]
    coord = ((gc + 0.5) * grid).astype(np.float32)
    colour = rng.random((n, 3)).astype(np.float32)
    feat = np.concatenate([colour, nrm.astype(np.float32)], axis=1)
    segment = rng.integers(0, 20, size=n).astype(np.int64)
    segment[rng.random(n) < 0.05] = -1
    return dict(coord=coord, grid_coord=gc.astype(np.int64), feat=feat, segment=segment)


def outdoor_scene(seed: int, point_max: int = 0, grid: float = 0.05, azimuth_steps: int = 2200):
    """LiDAR-like sweep (SURVEY 8(d) outdoor generator, BASELINE configs[4]): 64-96 beams at elevations -30..+10 deg,
    `azimuth_steps` columns; below-horizon beams hit the ground plane z = -1.8 m (range clipped to 60 m), the others
    return from U(8, 50) m; 2.5 % Gaussian range noise; voxelised at `grid` (0.05 m -> extent ~2400 voxels, depth 12);
    feat = coord | strength (in_channels = 4, nuscenes/semseg-pt-v3m1-0-base.py:16); 16 classes."""
    rng = np.random.default_rng(seed)
    beams = int(rng.integers(64, 97))
    elev = np.deg2rad(np.linspace(-30.0, 10.0, beams))[:, None]
    azim = np.linspace(0.0, 2 * np.pi, azimuth_steps, endpoint=False)[None, :] + rng.uniform(0, 2 * np.pi)
    down = np.broadcast_to(elev < 0, (beams, azimuth_steps))
    r_ground = np.minimum(1.8 / np.maximum(np.sin(-elev), 1e-6), 60.0)
    r = np.where(down, np.broadcast_to(r_ground, (beams, azimuth_steps)), rng.uniform(8.0, 50.0, (beams, azimuth_steps)))
    r = r * (1.0 + 0.025 * rng.standard_normal(r.shape))
    keep = rng.random(r.shape) < np.where(down, 1.0, 0.35)     # most above-horizon beams see the sky
    ce = np.broadcast_to(np.cos(elev), r.shape)
    p = np.stack([r * ce * np.cos(azim), r * ce * np.sin(azim), r * np.broadcast_to(np.sin(elev), r.shape)], axis=-1)[keep]
    gc = np.floor(p / grid).astype(np.int64)
    gc -= gc.min(0)
    key = (gc[:, 0] * 8192 + gc[:, 1]) * 8192 + gc[:, 2]
    _, first = np.unique(key, return_index=True)
    first = first[rng.permutation(first.shape[0])]
    if point_max and first.shape[0] > point_max:   # half the budget nearest the sensor (dense), half anywhere (keeps the extent)
        near = np.argsort((p[first] ** 2).sum(1), kind="stable")
        far = np.ones(first.shape[0], dtype=bool)
        far[near[: point_max // 2]] = False
        first = np.concatenate([first[near[: point_max // 2]], first[np.flatnonzero(far)[: point_max - point_max // 2]]])
        first = first[rng.permutation(first.shape[0])]
    gc, p = gc[first], p[first]
    gc = gc - gc.min(0)
    n = gc.shape[0]
    coord = p.astype(np.float32)
    feat = np.concatenate([coord, rng.random((n, 1)).astype(np.float32)], axis=1)
    segment = rng.integers(0, 16, size=n).astype(np.int64)
    segment[rng.random(n) < 0.05] = -1
    return dict(coord=coord, grid_coord=gc.astype(np.int64), feat=feat, segment=segment)


def collate(scenes):
    """point_collate_fn equivalent: concatenate and build the cumulative `offset`."""
    out = {k: np.concatenate([s[k] for s in scenes]) for k in scenes[0]}
    out["offset"] = np.cumsum([s["coord"].shape[0] for s in scenes]).astype(np.int64)
    return out


def indoor_batch(batch: int, point_max: int, rank: int = 0, base_seed: int = 0):
    """seeds s = 1000*rank + scene_index (+ base_seed)."""
    return collate([indoor_scene(base_seed + 1000 * rank + i, point_max) for i in range(batch)])


def to_torch(batch, device):
    import torch

    return {k: torch.from_numpy(v).to(device) for k, v in batch.items()}


def instance_parse(coord, segment, instance, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1):
    """InstanceParser (pointcept/datasets/transform.py:1312-1355): instance ids renumbered over the non-ignored classes,
    instance_centroid [N, 3] (the instance's mean coordinate, -1 elsewhere) and bbox [K, 8] (centre, size, theta 0, class shifted
    past the vacated ignore classes)."""
    instance = instance.copy()
    mask = ~np.isin(segment, segment_ignore_index)
    instance[~mask] = instance_ignore_index
    unique, inverse = np.unique(instance[mask], return_inverse=True)
    instance[mask] = inverse
    centroid = np.ones((coord.shape[0], 3)) * instance_ignore_index
    bbox = np.ones((len(unique), 8)) * instance_ignore_index
    vacancy = [index for index in segment_ignore_index if index >= 0]
    for k in range(len(unique)):
        m = instance == k
        c = coord[m]
        cls = np.array([segment[m][0]], dtype=c.dtype)
        cls -= np.greater(cls, vacancy).sum()
        centroid[m] = c.mean(0)
        bbox[k] = np.concatenate([(c.max(0) + c.min(0)) / 2, c.max(0) - c.min(0), np.zeros(1, dtype=c.dtype), cls])
    return instance, centroid.astype(np.float32), bbox.astype(np.float32)


def indoor_instance_scene(seed: int, point_max: int = 102400, grid: float = 0.02, density: int = 12000, n_boxes: int = 14):
    """indoor_scene's room for instance segmentation: floor = class 0, walls = class 1, each box one instance of a class in [2, 20);
    adds instance, instance_centroid and bbox as InstanceParser computes them (classes 0 / 1 and -1 ignored)."""
    rng = np.random.default_rng(seed)
    L, W, H = 7.0, 5.0, 2.8
    walls = [([0, 0, 0], [L, 0, 0], [0, W, 0], [0, 0, 1]), ([0, 0, 0], [L, 0, 0], [0, 0, H], [0, 1, 0]),
             ([0, W, 0], [L, 0, 0], [0, 0, H], [0, -1, 0]), ([0, 0, 0], [0, W, 0], [0, 0, H], [1, 0, 0]),
             ([L, 0, 0], [0, W, 0], [0, 0, H], [-1, 0, 0])]
    P, Nr, S, I = [], [], [], []
    for k, (o, u, v, nv) in enumerate(walls):
        a = np.linalg.norm(u) * np.linalg.norm(v)
        p = _rect(rng, o, u, v, int(a * density))
        P.append(p)
        Nr.append(np.tile(np.asarray(nv, float), (p.shape[0], 1)))
        S.append(np.full(p.shape[0], 0 if k == 0 else 1))
        I.append(np.full(p.shape[0], -1))
    for b in range(n_boxes):
        s = rng.uniform(0.3, 1.6, 3)
        bp, bn = _box(rng, [rng.uniform(0.8, L - 0.8), rng.uniform(0.8, W - 0.8), s[2] / 2], s, int(density * 1.2))
        P.append(bp)
        Nr.append(bn)
        S.append(np.full(bp.shape[0], int(rng.integers(2, 20))))
        I.append(np.full(bp.shape[0], b))
    p, nrm, seg, ins = np.concatenate(P), np.concatenate(Nr), np.concatenate(S), np.concatenate(I)
    gc = np.floor(p / grid).astype(np.int64)
    gc -= gc.min(0)
    key = (gc[:, 0] * 4096 + gc[:, 1]) * 4096 + gc[:, 2]
    _, first = np.unique(key, return_index=True)
    if first.shape[0] > point_max:
        centre = gc[first[rng.integers(first.shape[0])]]
        d2 = ((gc[first] - centre) ** 2).sum(1)
        first = first[np.argpartition(d2, point_max)[:point_max]]
    first = first[rng.permutation(first.shape[0])]      # dataloader order
    gc, nrm, seg, ins = gc[first], nrm[first], seg[first], ins[first]
    gc = gc - gc.min(0)
    n = gc.shape[0]
    coord = ((gc + 0.5) * grid).astype(np.float32)
    feat = np.concatenate([rng.random((n, 3)).astype(np.float32), nrm.astype(np.float32)], axis=1)
    segment = seg.astype(np.int64)
    instance, centroid, bbox = instance_parse(coord, segment, ins.astype(np.int64))
    return dict(coord=coord, grid_coord=gc.astype(np.int64), feat=feat, segment=segment, instance=instance.astype(np.int64),
                instance_centroid=centroid, bbox=bbox)


def indoor_instance_batch(seeds, sizes):
    """collated indoor_instance_scene batch (the per-scene bbox tables dropped: they are not per-point)"""
    scenes = [indoor_instance_scene(s, n) for s, n in zip(seeds, sizes)]
    for sc in scenes:
        sc.pop("bbox")
    return collate(scenes)


def indoor_superpoint_batch(seeds, sizes, cell: float = 0.5):
    """indoor_instance_batch plus a `superpoint` id per point: the coarse grid cell of edge `cell` crossed with the instance id,
    numbered 0.. per scene (an over-segmentation whose pieces never straddle two instances or an instance and the background)"""
    scenes = [indoor_instance_scene(s, n) for s, n in zip(seeds, sizes)]
    for sc in scenes:
        sc.pop("bbox")
        c = np.floor(sc["coord"] / cell).astype(np.int64)
        c -= c.min(0)
        key = ((c[:, 0] * 4096 + c[:, 1]) * 4096 + c[:, 2]) * 4096 + (sc["instance"] + 1)
        sc["superpoint"] = np.unique(key, return_inverse=True)[1].reshape(-1).astype(np.int64)
    return collate(scenes)


def contrastive_views(seed: int, point_max: int = 102400, grid: float = 0.02, shift=(-1.3, 0.4, -0.2), jitter: float = 0.004):
    """Two views of one indoor scene as ContrastiveViewsGenerator + the MSC config's pipelines leave them
    (configs/scannet/pretrain-msc-v1m1-0-spunet-base.py): each an independent sphere crop of about `point_max` points (the crops
    overlap in part), rotated about z and jittered, voxelised at `grid` (one point per voxel).  Per view: origin_coord (the scene's
    coordinate before the augmentation, shifted by `shift` so that some are negative: points shared by both crops keep equal origin
    coordinates), coord, grid_coord, color, normal, feat = color | normal, under view1_* / view2_* keys."""
    rng = np.random.default_rng(seed)
    s = indoor_scene(seed, int(point_max * 1.6), grid)
    origin = (s["coord"] + np.asarray(shift, np.float32)).astype(np.float32)
    n = origin.shape[0]
    take = min(point_max, n)
    c1 = origin[rng.integers(n)]
    near = np.argsort(((origin - c1) ** 2).sum(1), kind="stable")
    c2 = origin[near[int(rng.integers(take // 8, max(take // 2, take // 8 + 1)))]]
    out = {}
    for v, c in (("view1", c1), ("view2", c2)):
        d2 = ((origin - c) ** 2).sum(1)
        keep = np.argpartition(d2, take - 1)[:take] if take < n else np.arange(n)
        a = rng.uniform(0, 2 * np.pi)
        rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        p = (origin[keep] - c) @ rot.T + rng.normal(0, jitter, (keep.shape[0], 3))
        gc = np.floor(p / grid).astype(np.int64)
        gc -= gc.min(0)
        _, first = np.unique((gc[:, 0] * 8192 + gc[:, 1]) * 8192 + gc[:, 2], return_index=True)
        first = first[rng.permutation(first.shape[0])]
        keep, p, gc = keep[first], p[first], gc[first]
        colour = s["feat"][keep, :3]
        normal = (s["feat"][keep, 3:] @ rot.T).astype(np.float32)
        out.update({f"{v}_origin_coord": origin[keep], f"{v}_coord": p.astype(np.float32), f"{v}_grid_coord": gc,
                    f"{v}_color": colour, f"{v}_normal": normal, f"{v}_feat": np.concatenate([colour, normal], 1)})
    return out


def contrastive_views_batch(seeds, sizes, **kw):
    """collated contrastive_views scenes with view1_offset / view2_offset (point_collate_fn on the view keys)"""
    scenes = [contrastive_views(s, n, **kw) for s, n in zip(seeds, sizes)]
    out = {k: np.concatenate([sc[k] for sc in scenes]) for k in scenes[0]}
    for v in ("view1", "view2"):
        out[f"{v}_offset"] = np.cumsum([sc[f"{v}_coord"].shape[0] for sc in scenes]).astype(np.int64)
    return out


def multi_view_crops(seed: int, global_size: int, local_size: int, num_global: int = 2, num_local: int = 4, grid: float = 0.02,
                     shift=(-1.3, 0.4, -0.2), jitter: float = 0.004):
    """The views of one indoor scene as MultiViewGenerator + the Sonata config's pipelines leave them
    (configs/sonata/pretrain-sonata-v1m1-0-base.py): num_global sphere crops of about global_size points around nearby centres and
    num_local crops of about local_size points around centres inside the first (principal) global crop, each rotated about z,
    scaled by 0.9 .. 1.1, jittered and voxelised at `grid` (one point per voxel).  Per group: lists of origin_coord (the scene's
    coordinate before the augmentation, shifted by `shift`), cell (the view's voxel, >= 0) and feat = colour | normal."""
    rng = np.random.default_rng(seed)
    s = indoor_scene(seed, int(global_size * 2.5), grid)
    origin = (s["coord"] + np.asarray(shift, np.float32)).astype(np.float32)
    n = origin.shape[0]
    c0 = origin[rng.integers(n)]
    near = np.argsort(((origin - c0) ** 2).sum(1), kind="stable")

    def crop(centre, take):
        take = min(take, n)
        d2 = ((origin - centre) ** 2).sum(1)
        keep = np.argpartition(d2, take - 1)[:take] if take < n else np.arange(n)
        a = rng.uniform(0, 2 * np.pi)
        rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        p = ((origin[keep] - centre) @ rot.T) * rng.uniform(0.9, 1.1) + rng.normal(0, jitter, (keep.shape[0], 3))
        gc = np.floor(p / grid).astype(np.int64)
        gc -= gc.min(0)
        _, first = np.unique((gc[:, 0] * 8192 + gc[:, 1]) * 8192 + gc[:, 2], return_index=True)
        first = first[rng.permutation(first.shape[0])]
        keep, gc = keep[first], gc[first]
        normal = (s["feat"][keep, 3:] @ rot.T).astype(np.float32)
        return origin[keep], gc, np.concatenate([s["feat"][keep, :3], normal], 1)

    out = {}
    for group, num, size, spread in (("global", num_global, global_size, global_size // 4), ("local", num_local, local_size, global_size // 2)):
        views = [crop(c0 if (group == "global" and v == 0) else origin[near[int(rng.integers(0, max(spread, 1)))]], size) for v in range(num)]
        out[f"{group}_origin_coord"], out[f"{group}_cell"], out[f"{group}_feat"] = (list(x) for x in zip(*views))
    return out


def multi_view_batch(seeds, global_size: int, local_size: int, grid: float = 0.02, **kw):
    """collated multi_view_crops scenes under the keys Sonata's forward reads: global_* / local_* coord, origin_coord, feat and
    offset (one entry per view, the views of a scene adjacent), and grid_size (one entry per scene).  The model derives the voxel of a
    point from coord, trunc((coord - the minimum over the whole group) / grid_size), and two points of a view in one voxel leave the
    tie order of the serialization sort to the implementation.  So that a fixture has one answer, coord = (cell + 1.5 + u) grid with
    |u| <= 0.1, and the first view of each group starts with an anchor point at 0.05 grid on every axis (zero features, an origin
    100 m away from the scene: it matches nothing): every other point then lies 0.35 .. 0.55 of a cell inside the voxel cell + 1,
    one point per voxel, and stays there under a coordinate jitter of up to a quarter of a cell on either point."""
    scenes = [multi_view_crops(s, global_size, local_size, grid=grid, **kw) for s in seeds]
    rng = np.random.default_rng(int(seeds[0]) * 7919 + 1)
    out = {}
    for group in ("global", "local"):
        origin = [v for sc in scenes for v in sc[f"{group}_origin_coord"]]
        feat = [v for sc in scenes for v in sc[f"{group}_feat"]]
        coord = [((c + 1.5 + rng.uniform(-0.1, 0.1, c.shape)) * grid).astype(np.float32) for sc in scenes for c in sc[f"{group}_cell"]]
        origin[0] = np.concatenate([origin[0][:1] - np.float32(100.0), origin[0]])
        feat[0] = np.concatenate([np.zeros_like(feat[0][:1]), feat[0]])
        coord[0] = np.concatenate([np.full((1, 3), 0.05 * grid, np.float32), coord[0]])
        out[f"{group}_origin_coord"], out[f"{group}_coord"], out[f"{group}_feat"] = np.concatenate(origin), np.concatenate(coord), np.concatenate(feat)
        out[f"{group}_offset"] = np.cumsum([v.shape[0] for v in coord]).astype(np.int64)
    out["grid_size"] = np.full(len(seeds), grid, np.float32)
    return out


def multi_view_image_batch(seeds, global_size: int, local_size: int, img_nums, patch_h: int, patch_w: int, patch_size: float = 0.16,
                           pixels_per_patch: int = 2, grid: float = 0.02, **kw):
    """multi_view_batch plus what Concerto's forward reads for its 2D-3D term, in collated form:
    global_correspondence [points of the global views, max(img_nums), 2] int64 -- the image patch (row, col) each point projects to in
    every image of its scene, -1 where it falls outside the image and in the padded views of a scene with fewer images --, images
    [sum(img_nums), 3, patch_h * pixels_per_patch, patch_w * pixels_per_patch] float32 and img_num [scenes] int64.  Image v of a
    scene looks straight down at the scene's first global view: a rotation about z, a shift of up to a third of the patch grid and a
    patch edge of patch_size metres of the scene (origin_coord), so that neighbouring points share a patch and part of every view
    lies outside every image."""
    out = multi_view_batch(seeds, global_size, local_size, grid=grid, **kw)
    img_nums = [int(v) for v in img_nums]
    assert len(img_nums) == len(seeds)
    rng = np.random.default_rng(int(seeds[0]) * 104729 + 7)
    offset = np.concatenate([[0], out["global_offset"]])
    views_per_scene = (len(offset) - 1) // len(seeds)
    vmax = max(img_nums) if img_nums else 0
    corr = np.full((int(offset[-1]), vmax, 2), -1, np.int64)
    for b, n_img in enumerate(img_nums):
        lo, hi = int(offset[b * views_per_scene]), int(offset[(b + 1) * views_per_scene])
        first = out["global_origin_coord"][lo:int(offset[b * views_per_scene + 1])]
        centre = np.median(first[:, :2], 0)
        xy = out["global_origin_coord"][lo:hi, :2] - centre
        for v in range(n_img):
            a = rng.uniform(0, 2 * np.pi)
            rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            shift = rng.uniform(-1 / 3, 1 / 3, 2) * np.array([patch_h, patch_w])
            rc = np.floor((xy @ rot.T) / patch_size + np.array([patch_h, patch_w]) / 2 + shift).astype(np.int64)
            inside = (rc[:, 0] >= 0) & (rc[:, 0] < patch_h) & (rc[:, 1] >= 0) & (rc[:, 1] < patch_w)
            corr[lo:hi, v][inside] = rc[inside]
    out["global_correspondence"] = corr
    out["images"] = rng.uniform(-1, 1, (sum(img_nums), 3, patch_h * pixels_per_patch, patch_w * pixels_per_patch)).astype(np.float32)
    out["img_num"] = np.asarray(img_nums, np.int64)
    return out


def stand_in_image_encoder(patch_h: int, patch_w: int, channels: int, num_register_tokens: int = 5):
    """A small deterministic stand-in for the frozen image encoder of Concerto (no download, no random initialisation): every image
    patch is averaged over its pixels, mapped to `channels` by a fixed sinusoidal matrix and given a fixed positional term; the result
    is an object with last_hidden_state [images, num_register_tokens + patch_h * patch_w, channels], the register / class tokens in
    FRONT as in the DINOv2 family (Concerto.ENC2D_forward takes the last patch_h * patch_w tokens)."""
    import types

    import torch

    class StandInImageEncoder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            c = torch.arange(channels, dtype=torch.float64)
            p = torch.arange(patch_h * patch_w, dtype=torch.float64)
            self.proj = torch.nn.Parameter(torch.stack([torch.sin(0.37 * (k + 1) * (c + 1)) for k in range(3)]).float())
            self.pos = torch.nn.Parameter((0.5 * torch.cos(0.11 * (p[:, None] + 1) * (c[None] + 2) % 6.283)).float())
            self.register = torch.nn.Parameter(torch.cos(0.23 * (torch.arange(num_register_tokens, dtype=torch.float64)[:, None] + 1) * (c[None] + 1)).float())

        def forward(self, x):
            pooled = torch.nn.functional.adaptive_avg_pool2d(x.to(self.proj.dtype), (patch_h, patch_w))       # [I, 3, ph, pw]
            tokens = pooled.flatten(2).transpose(1, 2) @ self.proj + self.pos                                # [I, ph * pw, C]
            tokens = torch.cat([self.register[None].expand(x.shape[0], -1, -1), tokens], dim=1)
            return types.SimpleNamespace(last_hidden_state=tokens)

    return StandInImageEncoder().eval()
