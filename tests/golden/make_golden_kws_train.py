"""Golden vectors of the KWS classifier's training step from the REFERENCE's own model class (audio_models/RCNN_KWS/model.py,
loaded by file path as in make_golden_kws.py) in .train(), with the loss of its training script: CrossEntropyLoss on the
log-probabilities (train.py:79,148-149 -- a second log-softmax on top of the model's; reproduced, not fixed), loss.backward().
Weights are those of golden_kws_v1.npz (m32, m40) and are not stored again; inputs are regenerated from audiopure_amd.synth.
Run in the build container only; commits tests/golden/golden_kws_train_v1.npz."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from audiopure_amd import synth  # noqa: E402

spec = importlib.util.spec_from_file_location("kws_model_ref", "/root/reference/audio_models/RCNN_KWS/model.py")
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

G = np.load(os.path.join(ROOT, "tests", "golden", "golden_kws_v1.npz"))
SMALLEST = 4                                                   # tensors kept of the B = 1 case


def step(n_mels, T, B):
    m = mod.KWSModel(in_size=n_mels).train()
    m.load_state_dict({k.split("/sd/")[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"m{n_mels}/sd/")})
    x = torch.from_numpy(synth.uniform(f"kwstrain/{n_mels}/{T}", (B, 1, n_mels, T), 1, -80.0, 20.0)).requires_grad_(True)
    y = torch.arange(B) * 7 % 4
    lp = m(x)
    loss = torch.nn.CrossEntropyLoss()(lp, y)
    loss.backward()
    return loss.detach(), lp.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}


out = {}
loss, lp, gx, gp = step(32, 161, 3)
out["m32/T161_B3/loss"], out["m32/T161_B3/logp"], out["m32/T161_B3/dx"] = loss.numpy(), lp.numpy(), gx.numpy()
for k, v in gp.items():
    out[f"m32/T161_B3/grad/{k}"] = v.numpy()
loss, lp, gx, gp = step(40, 81, 1)                            # the B = 1 squeeze path (model.py:58,111-112)
out["m40/T81_B1/loss"], out["m40/T81_B1/dx"] = loss.numpy(), gx.numpy()
for k in sorted(gp, key=lambda k: gp[k].numel())[:SMALLEST]:
    out[f"m40/T81_B1/grad/{k}"] = gp[k].numpy()
path = os.path.join(ROOT, "tests", "golden", "golden_kws_train_v1.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
