"""Operator-level drop-in (SURVEY 8(b) level B3): make `import spconv.pytorch`, `import flash_attn`
`import torch_scatter`, `import pointops`, `import pointops2.pointops` and `import pointrope` resolve to the engine, so the reference's model files
(point_transformer_v3m1_base.py, spconv_unet_v1m1_base.py, structure.py, modules.py) run UNMODIFIED
on libptcore.so.  Call once before importing pointcept.models:

    import pointcept_amd.compat; pointcept_amd.compat.install()

Only names the hot-path files use are provided; real packages already imported are left alone
unless force=True.
"""
from __future__ import annotations

import sys
import types


def install(force: bool = False, geometric: bool = False, pointgroup: bool = False) -> None:
    """geometric=True also provides torch_geometric.{nn.pool.voxel_grid, utils.scatter} (torch_geometric_api), which OA-CNNs' and
    PTv2's files import; opt-in, so that the default install leaves a caller's own torch_geometric (or stand-in) untouched.
    pointgroup=True also provides `pointgroup_ops` (pointgroup_ops_api), which PointGroup's files import; opt-in likewise."""
    from . import flash_attn_api, pointops2_api, pointops_api, pointrope_api, spconv_api, torch_scatter_api

    def put(name, module):
        if force or name not in sys.modules:
            sys.modules[name] = module

    sp = types.ModuleType("spconv")
    sp.pytorch = spconv_api
    put("spconv", sp)
    put("spconv.pytorch", spconv_api)
    put("spconv.pytorch.modules", spconv_api.modules)
    fa = types.ModuleType("flash_attn")
    fa.flash_attn_varlen_qkvpacked_func = flash_attn_api.flash_attn_varlen_qkvpacked_func
    put("flash_attn", fa)
    ts = types.ModuleType("torch_scatter")
    ts.segment_csr = torch_scatter_api.segment_csr
    put("torch_scatter", ts)
    put("pointops", pointops_api)
    # libs/pointops2: `import pointops2.pointops as pointops` (stratified_transformer_v1m1_origin.py:21, v1m2_refine.py:31)
    p2 = types.ModuleType("pointops2")
    p2.pointops = pointops2_api
    p2f = types.ModuleType("pointops2.functions")
    p2f.pointops = pointops2_api
    p2.functions = p2f
    put("pointops2", p2)
    put("pointops2.pointops", pointops2_api)
    put("pointops2.functions", p2f)
    put("pointops2.functions.pointops", pointops2_api)
    put("pointrope", pointrope_api)      # libs/pointrope: `import pointrope as _kernels` (litept_v1.py:26)
    if geometric:
        from . import torch_geometric_api as tg

        top = types.ModuleType("torch_geometric")
        top.nn, top.utils = tg.nn, tg.utils
        put("torch_geometric", top)
        put("torch_geometric.nn", tg.nn)
        put("torch_geometric.nn.pool", tg.nn.pool)
        put("torch_geometric.utils", tg.utils)
    if pointgroup:
        from . import pointgroup_ops_api

        put("pointgroup_ops", pointgroup_ops_api)     # libs/pointgroup_ops: `from pointgroup_ops import ballquery_batch_p, bfs_cluster`


# ------------------------------------------------------------------------------------------------
# module level: the engine's backbones under the reference's registry names
# ------------------------------------------------------------------------------------------------
MODEL_CLASSES = {                                   # registry name (reference file:line) -> (engine module, class)
    "PT-v3m1": ("point_transformer_v3", "PointTransformerV3"),        # point_transformer_v3m1_base.py:518
    "PT-v3m2": ("point_transformer_v3m2", "PointTransformerV3"),      # point_transformer_v3m2_sonata.py:544
    "PT-v3m3": ("point_transformer_v3m3", "PointTransformerV3"),      # point_transformer_v3m3_utonia.py:686
    "LitePT-v1": ("litept", "LitePT"),                                # litept_v1.py:593
    "SpUNet-v1m1": ("sparse_unet", "SpUNetBase"),                     # spconv_unet_v1m1_base.py:88
    "SpUNetNoSkipBase": ("sparse_unet", "SpUNetNoSkipBase"),          # spconv_unet_v1m1_base.py:283 (registered under its class name)
}
# ports registered only when named: register_models(MODELS, names=["OACNNs"])
OPT_IN_MODEL_CLASSES = {
    "OACNNs": ("oacnns", "OACNNs"),                                   # oacnns_v1m1_base.py:212
    "PG-v1m1": ("point_group", "PointGroup"),                         # point_group_v1m1_base.py:22
    "PG-v1m2": ("point_group", "PointGroupV1m2"),                     # point_group_v1m2_custom_criteria.py:25
    "MSC-v1m1": ("masked_scene_contrast", "MaskedSceneContrast"),     # masked_scene_contrast_v1m1_base.py:24
    "MSC-v1m2": ("masked_scene_contrast", "MaskedSceneContrastCSC"),  # masked_scene_contrast_v1m2_csc.py:24
    "CAC-v1m1": ("context_aware_classifier", "CACSegmentor"),         # context_aware_classifier_v1m1_base.py:17
    "SGIFormer-v1m1": ("sgiformer", "SGIFormer"),                      # sgiformer/sgiformer_v1m1_base.py:482
    "Sonata-v1m1": ("sonata", "Sonata"),                              # sonata/sonata_v1m1_base.py:71
    "SpUNet-v1m3": ("sparse_unet_v1m3", "SpUNetV1m3"),                # sparse_unet/spconv_unet_v1m3_pdnorm.py:230
    "PPT-v1m1": ("point_prompt_training", "PointPromptTraining"),     # point_prompt_training_v1m1_language_guided.py:18
    "PPT-v1m2": ("point_prompt_training", "PointPromptTrainingDecoupled"),   # point_prompt_training_v1m2_decoupled.py:18
    "PPT-v1m3": ("point_prompt_training", "PointPromptTrainingNeo"),  # point_prompt_training_v1m3_neo.py:23
    "Concerto-v1m1": ("concerto", "Concerto"),                        # concerto/concerto_v1m1_base.py:82
}


def build_backbone(cfg):
    """an engine backbone from a config dict (its `type` one of compat.MODEL_CLASSES / OPT_IN_MODEL_CLASSES), else the
    reference's registry (inside a Pointcept checkout); a module is taken as is"""
    import importlib

    import torch.nn as nn

    if isinstance(cfg, nn.Module):
        return cfg
    kw = dict(cfg)
    name = kw.pop("type")
    if name in MODEL_CLASSES or name in OPT_IN_MODEL_CLASSES:
        mod, cls = MODEL_CLASSES.get(name) or OPT_IN_MODEL_CLASSES[name]
        return getattr(importlib.import_module(f"{__package__}.{mod}"), cls)(**kw)
    from pointcept.models.builder import build_model

    return build_model(cfg)


def register_models(registry, names=None, force: bool = True) -> list:
    """Registers the engine's module-level ports in the reference's `MODELS` registry (pointcept/models/builder.py) under the
    names the reference's configs use, replacing the CUDA-library implementations (`force=True`), so that
    `MODELS.build(cfg.model.backbone)` constructs them.  Returns the names registered.  Without `names`: every name of
    MODEL_CLASSES; the OPT_IN_MODEL_CLASSES (OA-CNNs, PointGroup, MSC-v1m1 / -v1m2, CAC, SGIFormer, Sonata, SpUNet-v1m3,
    PPT-v1m1 / -v1m2 / -v1m3, Concerto-v1m1) only when named.

        from pointcept.models.builder import MODELS
        import pointcept_amd.compat; pointcept_amd.compat.register_models(MODELS)
    """
    import importlib

    done = []
    for name in (names or MODEL_CLASSES):
        mod, cls = MODEL_CLASSES[name] if name in MODEL_CLASSES else OPT_IN_MODEL_CLASSES[name]
        registry.register_module(name, force=force, module=getattr(importlib.import_module(f"{__package__}.{mod}"), cls))
        done.append(name)
    return done

