#!/usr/bin/env python3
"""The REFERENCE's own ``mixup_cross_entropy_loss`` and ``mixup`` (imported from the reference checkout; build container only) on the
seeded cases of tests/loss_restate.py, float32 on the CPU.  Stores results only: per case the loss and the first 4096 elements of
d loss / d input (torch autograd through the reference's expression); per mixup run (np.random.seed(B), inputs [B, 1, 4, 8]) the mixed
inputs and the soft targets.

    python tests/golden/make_golden_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AUDIOPURE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))    # the reference checkout
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "audio_models/ConvNets_SpeechCommands"))

import mixup as ref_mixup                                              # noqa: E402  (reference module)
import loss_restate as L                                               # noqa: E402

out = {}
for c in L.CASES:
    z, y, soft = L.case(c)
    xs = torch.from_numpy(z).requires_grad_(True)
    loss = ref_mixup.mixup_cross_entropy_loss(xs, torch.from_numpy(soft))
    din, = torch.autograd.grad(loss, xs)
    out[f"mce/{L.case_id(c)}/loss"] = loss.detach().numpy().copy()
    out[f"mce/{L.case_id(c)}/din"] = din.numpy().reshape(-1)[:L.GOLDEN_FULL].copy()
for B, K in L.MIXUP_GOLDEN:
    x, y = L.mixup_inputs(B, K)
    np.random.seed(B)
    xm, ym = ref_mixup.mixup(torch.from_numpy(x), torch.from_numpy(y), K)
    out[f"mixup/{B}/inputs"] = xm.numpy().copy()
    out[f"mixup/{B}/targets"] = ym.numpy().copy()
path = os.path.join(HERE, "golden_loss_v1.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
