#!/usr/bin/env python3
"""One and two train() steps of the REFERENCE's own VGG and WideResNet(dropRate=0.3) classes (imported from the reference checkout;
build container only) at the small sizes of tests/convnet_dropout_restate.py, on that file's seeded weights and inputs, with
``torch.nn.functional.dropout`` patched to the masks of ``ap_dropout``'s rule (convnet_dropout_restate.patched_dropout): model.train(),
CrossEntropyLoss, backward(), float32 on the CPU, B = 4.  Stores results only, laid out as make_golden_convnet_train.py does: logits,
loss, running statistics after one and two steps; of the first step gradients of tensors of at most 4096 elements in full, of larger
ones the L2 norm and 64 seeded elements; and which ReLU inputs this float32 run decided the other way than the float64 restatement.

The reference's VGG takes its feature stack as an argument and builds a 512 -> 4096 -> 4096 classifier; for the eighth-width case the
stack is ``make_layers`` on configuration E divided by 8 and the three Linear layers of that classifier are replaced by 64 -> 512 ->
512 -> 10 ones -- the class, its forward and its two nn.Dropout() modules are the reference's.

    python tests/golden/make_golden_convnet_dropout.py
"""
import os
import sys
import warnings

import numpy as np
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AUDIOPURE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))    # the reference checkout
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "audio_models/ConvNets_SpeechCommands"))
warnings.filterwarnings("ignore")

import models as ref_models                                            # noqa: E402  (reference package)
from models import vgg as ref_vgg                                      # noqa: E402
import convnet_train_restate as R                                      # noqa: E402
import convnet_dropout_restate as D                                    # noqa: E402


def small_vgg():
    m = ref_vgg.VGG(ref_vgg.make_layers([v if v == "M" else v // 8 for v in ref_vgg.cfg["E"]], batch_norm=True, in_channels=1),
                    num_classes=D.NUM_CLASSES, init_weights=False)
    m.classifier[0], m.classifier[3], m.classifier[6] = nn.Linear(64, 512), nn.Linear(512, 512), nn.Linear(512, D.NUM_CLASSES)
    return m


REFERENCE = {
    "vgg": small_vgg,
    "wideresnetD": lambda: ref_models.WideResNet(depth=10, widen_factor=1, dropRate=0.3, num_classes=D.NUM_CLASSES, in_channels=1),
}

out = {}
for name, make in REFERENCE.items():
    m = R.init(make(), D.SEED[name])
    mine = D.CASES[name]()
    assert list(m.state_dict()) == list(mine.state_dict()), name          # the same keys, hence the same seeded weights
    assert all(a.shape == b.shape for a, b in zip(m.state_dict().values(), mine.state_dict().values())), name
    x, y = D.inputs(name)
    for i, idx in D.flips_of(name, D.module_masks(m, x)):
        out[f"{name}/flips/{i}"] = np.asarray(idx, dtype=np.int64)
    for step in (1, 2):
        got = D.module_step(m, x, y)
        out[f"{name}/{step}/logits"] = got["logits"].numpy().copy()
        out[f"{name}/{step}/loss"] = got["loss"].numpy().copy()
        for k, v in got["running"].items():
            out[f"{name}/{step}/running/{k}"] = v.numpy().copy()
        if step == 2:
            continue
        for k, g in list(got["grads"].items()) + [("dx", got["dx"])]:
            g = g.numpy().reshape(-1)
            if g.size <= D.GOLDEN_FULL:
                out[f"{name}/{step}/grad/{k}"] = g.copy()
            else:
                out[f"{name}/{step}/gradnorm/{k}"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
                out[f"{name}/{step}/gradpick/{k}"] = g[D.golden_pick(name, k, g.size)].copy()
    print(f"{name:11s} params {sum(p.numel() for p in m.parameters()):>8d}  loss {float(got['loss']):.4f}")
path = os.path.join(HERE, "golden_convnet_dropout_v1.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
