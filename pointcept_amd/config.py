"""Engine feature switches (environment variables, read once at import).

Every switch selects between two forms of the same math that are BOTH on libptcore.so -- there is no CPU path and no
library (hipBLASLt / ATen / SDPA) backend to switch to (round 4: PTC_OWN_LINEAR / PTC_OWN_NORM are gone; the library
comparison lives in tools/linear_kernels.py).  They exist so one GPU session can A/B a fusion against
the unfused form of the same math (tests/test_gpu_model.py runs the oracle comparison under both
settings), and so a regression can be bisected without a rebuild.

  PTC_FUSE_GATHER=0  serialized attention gathers / un-gathers rows with ptc_gather_rows instead of
                     folding the permutation into the qkv / proj GEMMs (kv = 1 gather tables)
  PTC_SORT_POINTS=0  PT-v3m1 keeps the caller's (dataloader) row order at stage 0 instead of physically
                     sorting the points along the first serialization curve for L2 locality
  PTC_FUSE_MLP=0     the MLP runs fc1, GELU, fc2 as three kernels (+2 in the backward) instead of fusing GELU into
                     fc1's epilogue and GELU' into the epilogue of fc2's input gradient
  PTC_PREFETCH_LEVELS=0  every SerializedPooling fetches its own sizes (two host syncs per stage) instead of the one
                     up-front copy of all level sizes (ptc_pool_level_counts)
  PTC_RPE_KERNEL=0   the RPE attention branch (enable_flash=False, enable_rpe=True) keeps the dense [P,H,K,K] torch
                     formulation instead of the window-attention kernels of csrc/attention_rpe.h -- under bf16 / fp16 autocast
                     and in fp32 runs without autocast (csrc/attention_rpe_f32.h) alike
  PTC_EXEC_BLOCK=0   a PT-v3m1 Block is enqueued by ~16 Python autograd Functions (the fused joints below) instead of one C call per
                     direction (csrc/block_exec.hip: same kernels, same operands, bit-identical; ~20 ms less host time per step)
  PTC_WGRAD_BLK=0    the weight gradient of the 32 / 64-channel submanifold convolutions runs on the global-gather kernel (wgrad2) instead
                     of the block-staged, accumulator-stationary one (csrc/wgrad7.h)
  PTC_FUSE_BN_TAIL=0 SpUNet's residual block runs bn2, the residual add and the ReLU as three passes (the reference's form) instead of in
                     the BatchNorm's apply pass (ptc_batch_norm_add_act_*), and every BatchNorm site increments its step counter itself
                     instead of one multi-tensor launch per forward
  PTC_CONV8=0        3^3 convolutions of 96 channels and more on the global-gather kernel conv3 instead of the block-staged conv8
                     (round 6; forward and input gradient; profiles/r06_t_conv8_himg.txt)
  PTC_BLK_MLP_FUSED=0  the MLP of a 32- / 64-channel Block runs on the split kernels (fc1 + GELU, fc2 + joint; GELU' input gradient,
                     fc1 input gradient, two weight gradients) instead of csrc/mlp.hip's one kernel per direction (round 6)
  PTC_OACNN_AGG=0    OA-CNNs' segmented centering and adaptive aggregation (oacnns.py) run as the reference's ATen expression
                     (exp / index_add scatters / softmax / einsum) instead of csrc/cluster_agg.hip (A/B baseline; the grid clusters
                     stay on the kernels either way)
  PTC_PG_CLUSTER=0   PointGroup's clustering, proposal scores and offset losses (point_group.py, pointgroup_ops_api) run as the
                     torch formulation: chunked brute-force ball query, host BFS, the reference's loss expression (A/B baseline and
                     cross-check of csrc/pg_cluster.hip)
  PTC_MSC=0          Masked Scene Contrast's cross masks, view matching, pair selection and InfoNCE loss (masked_scene_contrast.py) run
                     as the reference's own expression on ops.knn_query and torch -- voxel_grid + unique, brute-force kNN + radius
                     filter, the dense P x P similarity matrix; for MSC-v1m2 the per-scene loop with its dense partition matrices and
                     one masked CrossEntropy per class -- instead of csrc/msc.hip (A/B baseline, and the CPU path of the port)
  PTC_CAC=0          the context-aware classifier's prototype pooling, cosine classifier and distillation loss
                     (context_aware_classifier.py) run as the reference's own expression -- per-class and per-scene loops, dense
                     softmax / one-hot temporaries, library GEMMs -- instead of csrc/cac.hip (A/B baseline, and the CPU path of the port)
  PTC_SGI=0          SGIFormer's decoder attention, attention-mask packing, matcher cost and target builder (sgiformer.py) run as the
                     reference's own expression -- a Python loop over scenes, dense [heads, Lq, Lk] probabilities, [Lq, M] BCE maps,
                     an [N, instances] one-hot -- instead of csrc/sgiformer.hip (A/B baseline, and the CPU path of the port)
  PTC_SONATA=0       Sonata's distillation loss (sonata.py, functional.sonata_distill) runs as the reference's own expression -- the
                     gathered teacher rows, exp and three Sinkhorn-Knopp iterations over a dense M x K fp32 matrix, log_softmax of the
                     gathered student rows and their product -- instead of the scaling-vector passes of csrc/sonata.hip (A/B baseline,
                     and the CPU path of the port); view matching and the masks run as knn_query + radius filter and torch.unique
  PTC_PPT=0          Point Prompt Training's language-guided head (point_prompt_training.py, functional.ppt_head) runs as the
                     reference's own expression -- proj_head, the row norm, the division and the class matmul, four passes over an
                     [N, 512] tensor that autograd keeps -- instead of csrc/ppt.hip (A/B baseline, and the CPU path of the port)
  PTC_CONCERTO=0     Concerto's 2D-3D alignment branch (concerto.py, functional.concerto_*) runs as the reference's own expression -- the
                     per-(level, image) pool_corr loop, a dense [all patches, C] scatter_mean, patch_proj over all of it, torch.unique,
                     two gathers and the elementwise centred cosine -- instead of csrc/concerto.hip (A/B baseline, and the CPU path)
  PTC_CRITERIA=0     the criteria terms of csrc/criteria.hip (functional.seg_criteria: class-weighted / label-smoothed / summed
                     CrossEntropyLoss, FocalLoss, DiceLoss; criteria.Criteria) run as their torch twins -- the reference's own
                     expressions, several fp32 [N, C] temporaries per term and direction -- instead of one fused pass per direction
                     (A/B baseline, and the CPU path); the default CrossEntropyLoss and LovaszLoss keep their kernels either way
  PTC_AUGMENT=0      the device-side point augmentations (augment.py: CenterShift ... ElasticDistortion, the Chromatic* ops, Compose)
                     run as their torch twins -- the reference's transforms op by op in fp32, one [n, 3] temporary or more per
                     transform -- instead of the pending-affine / flush kernels of csrc/augment.hip (A/B baseline, and the CPU path)
  PTC_FUSE_BLOCK=0   the three residual joints of a PTv3 Block run as separate LayerNorm / add / cast
                     kernels instead of the fused add_norm passes
"""
from __future__ import annotations

import os


def _flag(name: str, default: bool) -> bool:
    v = os.environ.get(name)
    if v is None:
        return default
    return v.strip().lower() not in ("0", "false", "off", "no", "")


FUSE_GATHER = _flag("PTC_FUSE_GATHER", True)
SORT_POINTS = _flag("PTC_SORT_POINTS", True)
FUSE_BLOCK = _flag("PTC_FUSE_BLOCK", True)
EXEC_BLOCK = _flag("PTC_EXEC_BLOCK", True)
FUSE_MLP = _flag("PTC_FUSE_MLP", True)
# PTC_CONV8 and PTC_BLK_MLP_FUSED are read by the library alone (csrc/conv8.h conv8_enabled, ptc_ptv3_block_mlp_fused); Python asks it
# (ops.BlockProvider.get, ops.block_mlp_fused): a value beginning with 0 turns the kernel off
PREFETCH_LEVELS = _flag("PTC_PREFETCH_LEVELS", True)
RPE_KERNEL = _flag("PTC_RPE_KERNEL", True)
OACNN_AGG = _flag("PTC_OACNN_AGG", True)
PG_CLUSTER = _flag("PTC_PG_CLUSTER", True)
MSC_KERNELS = _flag("PTC_MSC", True)
CAC_KERNELS = _flag("PTC_CAC", True)
SGI_KERNELS = _flag("PTC_SGI", True)
SONATA_KERNELS = _flag("PTC_SONATA", True)
PPT_KERNELS = _flag("PTC_PPT", True)
CONCERTO_KERNELS = _flag("PTC_CONCERTO", True)
CRITERIA_KERNELS = _flag("PTC_CRITERIA", True)
AUGMENT_KERNELS = _flag("PTC_AUGMENT", True)
WGRAD_BLK = _flag("PTC_WGRAD_BLK", True)
FUSE_BN_TAIL = _flag("PTC_FUSE_BN_TAIL", True)
BATCH_BN_COUNTERS = _flag("PTC_BATCH_BN_COUNTERS", True)
