"""Generate tests/golden/criteria_tiny.npz by running the REFERENCE'S OWN CrossEntropyLoss, FocalLoss and DiceLoss
(pointcept/models/losses/misc.py, imported unmodified through oracle/ref_import.py) in fp32 on the CPU on the seeded cases of
tests/test_gpu_criteria.py (GOLDEN_CASES / golden_case).  Only runnable where the reference tree exists; the .npz output is committed.

    python tests/golden/make_golden_criteria.py

The reference's CrossEntropyLoss.__init__ moves its class weight to the GPU (.cuda()): it is constructed without a weight and the weight
of its inner nn.CrossEntropyLoss is set on the CPU.  Stored per case, with the discipline of lovasz_wide.npz: the labels and a float64
checksum of the logits (the tests regenerate both from the seed and compare), the reference's loss (loss_weight included) and its
gradient w.r.t. the logits.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle import ref_import  # noqa: E402


def load_reference_misc():
    ref_import.load()
    if "pointcept.models.losses" not in sys.modules:
        pkg = types.ModuleType("pointcept.models.losses")
        pkg.__path__ = [ref_import.REF + "/pointcept/models/losses"]
        sys.modules["pointcept.models.losses"] = pkg
    return importlib.import_module("pointcept.models.losses.misc")


def build_reference(misc, term, ignore_index):
    """the reference module of one config dict, on the CPU"""
    term = dict(term)
    kind = term.pop("type")
    if kind == "CrossEntropyLoss":
        weight = term.pop("weight", None)
        crit = misc.CrossEntropyLoss(ignore_index=ignore_index, **term)
        if weight is not None:
            crit.loss.weight = torch.tensor(weight)
        return crit
    return getattr(misc, kind)(ignore_index=ignore_index, **term)


def run_reference(crit, x, y):
    x = x.clone().requires_grad_(True)
    loss = crit(x, y)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def main():
    from test_gpu_criteria import GOLDEN_CASES, golden_case

    misc = load_reference_misc()
    blobs = {}
    for ci in range(len(GOLDEN_CASES)):
        x, y, ignore, term = golden_case(ci)
        loss, grad = run_reference(build_reference(misc, term, ignore), x, y)
        blobs[f"logits_sum_{ci}"], blobs[f"labels_{ci}"] = np.asarray(float(x.double().sum())), y.numpy().astype(np.int16)
        blobs[f"loss_{ci}"], blobs[f"grad_{ci}"] = np.asarray(loss), grad
    blobs["n_cases"] = np.asarray(len(GOLDEN_CASES))
    path = os.path.join(OUT, "criteria_tiny.npz")
    np.savez_compressed(path, **blobs)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
