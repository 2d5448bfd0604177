#!/usr/bin/env python3
"""One and two train() steps of the REFERENCE's own 2-D ConvNet classes (imported from the reference checkout; build container only)
at the small constructor arguments of tests/convnet_train_restate.py, on that file's seeded weights and inputs: model.train(),
CrossEntropyLoss, backward() (train_speech_commands.py:131-140), float32 on the CPU, B = 4.  Stores results only:
logits, loss, every running statistic after one and two steps; of the first step (the second's are the same: the parameters
do not move) gradients of tensors of at most 4096 elements in full, of larger ones the L2 norm and 64 seeded elements; and which ReLU inputs (a handful, all within rounding of 0) this float32 run decided the
other way than the float64 restatement, so that a comparison can tell rounding from decisions.

    python tests/golden/make_golden_convnet_train.py
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AUDIOPURE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))    # the reference checkout
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "audio_models/ConvNets_SpeechCommands"))
warnings.filterwarnings("ignore")

import models as ref_models                                            # noqa: E402  (reference package)
from models.resnet import ResNet, Bottleneck                           # noqa: E402
from models.dpn import DPN                                             # noqa: E402
import convnet_train_restate as R                                      # noqa: E402

mid, res, blocks, dense = zip(*R._SmallDPN.TABLE)
REFERENCE = {
    "resnext": lambda: ref_models.CifarResNeXt(R.NUM_CLASSES, cardinality=2, depth=11, base_width=16, widen_factor=1, in_channels=1),
    "resnet": lambda: ResNet(Bottleneck, [1, 1, 1, 1], num_classes=R.NUM_CLASSES, in_channels=1),
    "wideresnet": lambda: ref_models.WideResNet(depth=10, widen_factor=1, dropRate=0, num_classes=R.NUM_CLASSES, in_channels=1),
    "dpn": lambda: DPN(R.NUM_CLASSES, 1, dict(in_planes=mid, out_planes=res, num_blocks=blocks, dense_depth=dense)),
    "densenet": lambda: ref_models.DenseNet(depth=10, growthRate=12, compressionRate=2, num_classes=R.NUM_CLASSES, in_channels=1),
}

out = {}
for name, make in REFERENCE.items():
    m = R.init(make(), R.SEED[name])
    mine = R.CASES[name]()
    assert list(m.state_dict()) == list(mine.state_dict()), name          # the same keys, hence the same seeded weights
    x, y = R.inputs(name)
    for i, idx in R.flips_of(name, R.module_masks(m, x)):      # the ReLU inputs this float32 run decides the other way than float64
        out[f"{name}/flips/{i}"] = np.asarray(idx, dtype=np.int64)
    for step in (1, 2):
        got = R.module_step(m, x, y)
        out[f"{name}/{step}/logits"] = got["logits"].numpy().copy()
        out[f"{name}/{step}/loss"] = got["loss"].numpy().copy()
        for k, v in got["running"].items():
            out[f"{name}/{step}/running/{k}"] = v.numpy().copy()
        if step == 2:                                   # (at fixed parameters the gradients do not depend on the running statistics)
            continue
        for k, g in list(got["grads"].items()) + [("dx", got["dx"])]:
            g = g.numpy().reshape(-1)
            if g.size <= R.GOLDEN_FULL:
                out[f"{name}/{step}/grad/{k}"] = g.copy()
            else:
                out[f"{name}/{step}/gradnorm/{k}"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
                out[f"{name}/{step}/gradpick/{k}"] = g[R.golden_pick(name, k, g.size)].copy()
    print(f"{name:11s} params {sum(p.numel() for p in m.parameters()):>8d}  loss {float(got['loss']):.4f}")
path = os.path.join(HERE, "golden_convnet_train_v1.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
